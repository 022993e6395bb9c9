// SparseVFC fields in 4 to 8 dimensions: the kernel-value cache of the EM loop and the fused evaluator.
//
// Reference: `_con_K` spateo/tdr/morphometrics/morphofield/gaussian_process.py:16-36 and dynamo's SparseVFC (SURVEY.md
// Appendix A) take any number of columns; so do the analytical Jacobian (morphofield_dg/GPVectorField.py:143-190) and
// compute_acceleration / compute_curvature / compute_divergence (GPVectorField.py:12-52, 97-121).  The 3-D path of this
// library packs a point into one 16 / 32-byte x4 vector; here the points are plain row-major n x d arrays.
//   * ublk_build_d_kernel writes U = con_K(x, ctrl) in the layout of ublk_build_kernel (Ublk[m/16][n][16], zero padding,
//     the same store pattern: a wave owns 64 cells and every store instruction covers whole 128-byte lines).  Everything
//     after it in an EM iteration (Gram tiles + reduce, mvf_rhs_cached, mvf_apply_cached, the E-step) reads the cache, P, Y
//     and the coefficients only, so it runs unchanged at any d.
//   * eval_d_kernel is eval_mfma_kernel (mvf_eval.hip) for d-dimensional points and dy <= 8 output columns: one
//     v_mfma_f64_16x16x4_f64 product [v | W] = K [C | C (x) c] (W[f][i] = sum_m K_m C[m, f] c_m[i]), then
//     J[f][i] = -2 beta (p_i v_f - W[f][i]) with the kernel values from kernel_value_d on the VALU.
// Both compute K(x, c) with kernel_value_d, bit-identical to mvf_con_k at the same d.
#include "mvf_common.h"

namespace mvf {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int HUB = 16;      // == UB of mvf_gram.hip: control points per cache block
constexpr int HCHUNK = 256;  // == GCHUNK: the cache pads the cells to a multiple of this
constexpr int HGT = 128;     // == GT: ... and the control points to a multiple of this

static inline int64_t highd_npad(int64_t n) { return cdiv(n, HCHUNK) * HCHUNK; }
static inline int64_t highd_mpad(int64_t m) { return cdiv(m, HGT) * HGT; }

template <typename T, int D>
__global__ __launch_bounds__(256) void ublk_build_d_kernel(const T* __restrict__ x, int64_t n, int64_t n_pad,
                                                           const T* __restrict__ ctrl, int64_t m, int64_t m_pad, T s,
                                                           int cb_per_block, T* __restrict__ ublk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ublk_d_smem[];
    T* sctrl = reinterpret_cast<T*>(ublk_d_smem);  // [cb_per_block * 16][D] scaled control points (padded ones: 0)
    const int64_t cb0 = (int64_t)blockIdx.y * cb_per_block;
    const int ncb = (int)min((int64_t)cb_per_block, m_pad / HUB - cb0);
    for (int e = threadIdx.x; e < ncb * HUB * D; e += 256) {
        const int64_t c = cb0 * HUB + e / D;
        sctrl[e] = c < m ? ctrl[c * D + e % D] * s : T(0);
    }
    __syncthreads();
    // the store pattern of ublk_build_kernel: lane l of store instruction q writes the 16 bytes at tile offset (64 q + l) * 16
    constexpr int PER = 16 / sizeof(T);  // elements per 16-byte store
    constexpr int Q = HUB / PER;         // store instructions per block and wave (4 float32 / 8 float64)
    constexpr int LPC = HUB / PER;       // lanes per cell inside one instruction
    typedef T vec_t __attribute__((ext_vector_type(PER)));
    const int lane = threadIdx.x & 63;
    const int64_t wbase = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63);  // first cell of this wave
    if (wbase >= n_pad) return;
    const int j0 = (lane % LPC) * PER;  // this lane's control points inside a block: j0 .. j0 + PER - 1
    // The Q cells of a lane are taken QH at a time: the float64 builder at D >= 7 holding all eight cells' coordinates and two
    // control points' (160 float64 values) ran at 255 VGPRs + 6 AGPRs and one wave per SIMD; in two passes of four cells the
    // control points are read from LDS twice instead.  Same values, same store instructions, in another order.
    constexpr int QH = (sizeof(T) == 8 && D >= 7) ? Q / 2 : Q;
    for (int q0 = 0; q0 < Q; q0 += QH) {
        T p[QH][D];
        bool live[QH];
#pragma unroll
        for (int h = 0; h < QH; ++h) {
            const int64_t i = wbase + (64 / LPC) * (q0 + h) + lane / LPC;
            live[h] = i < n;
#pragma unroll
            for (int k = 0; k < D; ++k) p[h][k] = live[h] ? x[i * D + k] * s : T(0);
        }
        for (int b = 0; b < ncb; ++b) {
            T c[PER][D];
            bool clive[PER];
#pragma unroll
            for (int jj = 0; jj < PER; ++jj) {
                clive[jj] = (cb0 + b) * HUB + j0 + jj < m;
#pragma unroll
                for (int k = 0; k < D; ++k) c[jj][k] = sctrl[(b * HUB + j0 + jj) * D + k];
            }
            vec_t* dst = reinterpret_cast<vec_t*>(ublk + ((cb0 + b) * n_pad + wbase) * HUB) + lane;
#pragma unroll
            for (int h = 0; h < QH; ++h) {
                vec_t o;
#pragma unroll
                for (int jj = 0; jj < PER; ++jj) {
                    const T k = kernel_value_d<D>(p[h], c[jj]);
                    o[jj] = (live[h] && clive[jj]) ? k : T(0);
                }
                __builtin_nontemporal_store(o, dst + 64 * (q0 + h));
            }
        }
    }
}

struct EvalDOut {
    double *v, *jac, *div, *acc, *curv;
};

constexpr int ED_CHUNK = 64;  // control points staged per pass

// Query tiles of 16 per wave: the accumulators are QT x NCT MFMA tiles (8 VGPRs each).  Few column tiles: four query tiles
// share each B operand read; five column tiles (d = dy = 8 with the Jacobian): one query tile, its kernel value feeding
// five MFMAs.  At most 40 accumulator VGPRs either way.
template <int NCT>
struct EvalDShape {
    static constexpr int QT = NCT == 1 ? 4 : (NCT == 2 ? 2 : 1);
    static constexpr int QB = 4 * 16 * QT;      // queries per workgroup (4 waves)
    static constexpr int ROW = 16 * NCT + 1;    // padded LDS row (doubles): conflict-free column reads
};

// [v | W] columns: v_f = column f (f < dy), W[f][i] = column dy + f D + i; ncols = dy (v only) or dy (1 + D).
template <typename T, int D, int NCT>
__global__ __launch_bounds__(256) void eval_d_kernel(const T* __restrict__ x, int64_t n, const T* __restrict__ ctrl,
                                                     int64_t m, T s, double jscale /* -2 beta / s */,
                                                     const double* __restrict__ C, int dy, int ncols, int flags,
                                                     EvalDOut o) {
    using Sh = EvalDShape<NCT>;
    constexpr int QT = Sh::QT, QB = Sh::QB, ROW = Sh::ROW;
    constexpr size_t STAGE = ED_CHUNK * (D * sizeof(T) + ROW * sizeof(double));
    constexpr size_t RES = (size_t)QB * ROW * sizeof(double);
    __shared__ __attribute__((aligned(16))) unsigned char smem_raw[STAGE > RES ? STAGE : RES];
    T* sc = reinterpret_cast<T*>(smem_raw);                                              // [ED_CHUNK][D], scaled
    double* sB = reinterpret_cast<double*>(smem_raw + ED_CHUNK * D * sizeof(T));         // [ED_CHUNK][ROW]
    double* res = reinterpret_cast<double*>(smem_raw);                                   // [QB][ROW], after the product

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * QB;
    const int64_t wq0 = q0 + wave * 16 * QT;  // first query of this wave
    T p[QT][D];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int64_t i = wq0 + 16 * t + li;
#pragma unroll
        for (int k = 0; k < D; ++k) p[t][k] = (i < n) ? x[i * D + k] * s : T(0);
    }
    f64x4 acc[QT][NCT];
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc[t][c] = f64x4{0.0, 0.0, 0.0, 0.0};

    for (int64_t m0 = 0; m0 < m; m0 += ED_CHUNK) {
        const int mc = (int)min((int64_t)ED_CHUNK, m - m0);
        __syncthreads();
        for (int e = threadIdx.x; e < ED_CHUNK * D; e += 256) {
            const int j = e / D;
            sc[e] = j < mc ? ctrl[(m0 + j) * D + e % D] * s : T(0);
        }
        for (int e = threadIdx.x; e < ED_CHUNK * 16 * NCT; e += 256) {
            const int j = e / (16 * NCT), col = e % (16 * NCT);
            double val = 0.0;  // a padded control point / column contributes K x 0
            if (j < mc && col < ncols) {
                const int64_t g = m0 + j;
                if (col < dy) {
                    val = C[g * dy + col];
                } else {
                    const int f = (col - dy) / D, i = (col - dy) % D;
                    val = C[g * dy + f] * (double)(ctrl[g * D + i] * s);  // the scaled coordinate as the loop sees it
                }
            }
            sB[j * ROW + col] = val;
        }
        __syncthreads();
        const int nks = (mc + 3) >> 2;
        for (int ks = 0; ks < nks; ++ks) {
            const int j = 4 * ks + lk;
            T c[D];
#pragma unroll
            for (int k = 0; k < D; ++k) c[k] = sc[j * D + k];
            double b[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) b[ct] = sB[j * ROW + 16 * ct + li];
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                const double kv = (double)kernel_value_d<D>(p[t], c);
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
                    acc[t][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv, b[ct], acc[t][ct], 0, 0, 0);
            }
        }
    }
    __syncthreads();  // the staging area becomes the result area
    // D[row = lk + 4 r][col = li] of query tile t, column tile ct -> res[query of the workgroup][column]
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                res[(wave * 16 * QT + 16 * t + lk + 4 * r) * ROW + 16 * ct + li] = acc[t][ct][r];
    __syncthreads();
    if (threadIdx.x >= QB) return;
    const int64_t q = q0 + threadIdx.x;
    if (q >= n) return;
    const double* row = res + threadIdx.x * ROW;
    // register arrays indexed by compile-time indices only (f < 8 unrolled, guarded by dy): no scratch
    double v[8];
#pragma unroll
    for (int f = 0; f < 8; ++f) v[f] = f < dy ? row[f] : 0.0;
    if (flags & MVF_EVAL_V) {
#pragma unroll
        for (int f = 0; f < 8; ++f)
            if (f < dy) o.v[q * dy + f] = v[f];
    }
    if (!(flags & (MVF_EVAL_JAC | MVF_EVAL_DIV | MVF_EVAL_ACC | MVF_EVAL_CURV))) return;
    double pd[D];  // the scaled point as the loop saw it
#pragma unroll
    for (int i = 0; i < D; ++i) pd[i] = (double)(x[q * D + i] * s);
    double a[8], dv = 0.0;
#pragma unroll
    for (int f = 0; f < 8; ++f) {
        a[f] = 0.0;
        if (f < dy) {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const double J = (pd[i] * v[f] - row[dy + f * D + i]) * jscale;
                if (flags & MVF_EVAL_JAC) o.jac[(int64_t)(f * D + i) * n + q] = J;
                if (i == f) dv += J;
                a[f] = i == 0 ? J * v[0] : a[f] + J * v[i];
            }
        }
    }
    // (dy == D is checked by the host entry whenever DIV / ACC / CURV is asked for)
    if (flags & MVF_EVAL_DIV) o.div[q] = dv;
    if (flags & MVF_EVAL_ACC) {
#pragma unroll
        for (int f = 0; f < D; ++f) o.acc[q * D + f] = a[f];
    }
    if (flags & MVF_EVAL_CURV) {
        double vv = 0.0, va = 0.0;
#pragma unroll
        for (int f = 0; f < D; ++f) vv += v[f] * v[f], va += v[f] * a[f];
        const double nv = sqrt(vv);
        const double den = (nv * nv) * (nv * nv);  // ||v||^4 as norm(v)**4
#pragma unroll
        for (int f = 0; f < D; ++f) o.curv[q * D + f] = (a[f] * vv - v[f] * va) / den;
    }
}

template <typename T, int D, int NCT>
static void launch_eval_d_nct(const T* x, int64_t n, const T* ctrl, int64_t m, T s, double jscale, const double* C, int dy,
                              int ncols, int flags, const EvalDOut& o, hipStream_t st) {
    const dim3 grid((unsigned)cdiv(n, EvalDShape<NCT>::QB));
    hipLaunchKernelGGL((eval_d_kernel<T, D, NCT>), grid, dim3(256), 0, st, x, n, ctrl, m, s, jscale, C, dy, ncols, flags,
                       o);
}

// column tiles: v only = 1; with the Jacobian ceil(dy (1 + D) / 16) <= ceil(8 (1 + D) / 16)
template <typename T, int D>
static int launch_eval_d(int nct, const T* x, int64_t n, const T* ctrl, int64_t m, T s, double jscale, const double* C,
                         int dy, int ncols, int flags, const EvalDOut& o, hipStream_t st) {
    switch (nct) {
        case 1: launch_eval_d_nct<T, D, 1>(x, n, ctrl, m, s, jscale, C, dy, ncols, flags, o, st); return 0;
        case 2: launch_eval_d_nct<T, D, 2>(x, n, ctrl, m, s, jscale, C, dy, ncols, flags, o, st); return 0;
        case 3: launch_eval_d_nct<T, D, 3>(x, n, ctrl, m, s, jscale, C, dy, ncols, flags, o, st); return 0;
        case 4:
            if constexpr (D >= 6) {
                launch_eval_d_nct<T, D, 4>(x, n, ctrl, m, s, jscale, C, dy, ncols, flags, o, st);
                return 0;
            }
            break;
        case 5:
            if constexpr (D == 8) {
                launch_eval_d_nct<T, D, 5>(x, n, ctrl, m, s, jscale, C, dy, ncols, flags, o, st);
                return 0;
            }
            break;
        default: break;
    }
    return set_error("mvf_eval_d: no kernel for d=%d with %d column tiles", D, nct);
}

template <typename T>
static int launch_eval_d_dim(int d, int nct, const T* x, int64_t n, const T* ctrl, int64_t m, T s, double jscale,
                             const double* C, int dy, int ncols, int flags, const EvalDOut& o, hipStream_t st) {
    switch (d) {
        case 4: return launch_eval_d<T, 4>(nct, x, n, ctrl, m, s, jscale, C, dy, ncols, flags, o, st);
        case 5: return launch_eval_d<T, 5>(nct, x, n, ctrl, m, s, jscale, C, dy, ncols, flags, o, st);
        case 6: return launch_eval_d<T, 6>(nct, x, n, ctrl, m, s, jscale, C, dy, ncols, flags, o, st);
        case 7: return launch_eval_d<T, 7>(nct, x, n, ctrl, m, s, jscale, C, dy, ncols, flags, o, st);
        case 8: return launch_eval_d<T, 8>(nct, x, n, ctrl, m, s, jscale, C, dy, ncols, flags, o, st);
        default: return set_error("mvf_eval_d: d must be in 4 .. 8, got %d", d);
    }
}

template <typename T>
static void launch_ublk_d(int d, dim3 grid, size_t lds, hipStream_t st, const T* x, int64_t n, int64_t n_pad, const T* ctrl,
                          int64_t m, int64_t m_pad, T s, int cb_per_block, T* ublk) {
#define MVF_UBLK_D_CASE(DV)                                                                                                \
    case DV:                                                                                                               \
        hipLaunchKernelGGL((ublk_build_d_kernel<T, DV>), grid, dim3(256), lds, st, x, n, n_pad, ctrl, m, m_pad, s,         \
                           cb_per_block, ublk);                                                                            \
        break;
    switch (d) {
        MVF_UBLK_D_CASE(4)
        MVF_UBLK_D_CASE(5)
        MVF_UBLK_D_CASE(6)
        MVF_UBLK_D_CASE(7)
        default:
            MVF_UBLK_D_CASE(8)
    }
#undef MVF_UBLK_D_CASE
}

}  // namespace mvf

using namespace mvf;

extern "C" int mvf_ublk_build_d(const void* x, int64_t n, const void* ctrl, int64_t m, int d, double beta, void* ublk,
                                size_t ublk_bytes, mvf_dtype dtype, void* stream) {
    MVF_REQUIRE(d >= 4 && d <= 8, "mvf_ublk_build_d: d must be in 4 .. 8, got %d (d <= 3: mvf_ublk_build)", d);
    MVF_REQUIRE(n > 0 && m > 0, "mvf_ublk_build_d: need n > 0 and m > 0");
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "mvf_ublk_build_d: bad dtype %d", (int)dtype);
    MVF_REQUIRE(beta >= 0.0 && std::isfinite(beta), "mvf_ublk_build_d: beta must be finite and >= 0");
    MVF_REQUIRE(x && ctrl && ublk, "mvf_ublk_build_d: null pointer");
    const size_t need = mvf_ublk_bytes(n, m, dtype);
    MVF_REQUIRE(ublk_bytes >= need, "mvf_ublk_build_d: buffer too small (%zu < %zu)", ublk_bytes, need);
    const int64_t n_pad = highd_npad(n), m_pad = highd_mpad(m);
    const int cb_per_block = 32;  // 512 control points per workgroup column (16 - 32 KiB of LDS at d = 8)
    const dim3 grid((unsigned)(n_pad / 256), (unsigned)cdiv(m_pad / HUB, cb_per_block));
    MVF_REQUIRE(grid.y <= 65535, "mvf_ublk_build_d: m too large");
    MVF_REQUIRE(n_pad / 256 <= 0x7fffffffLL, "mvf_ublk_build_d: n too large");
    hipStream_t st = (hipStream_t)stream;
    const double s = std::sqrt(beta * LOG2E);
    if (dtype == MVF_F32)
        launch_ublk_d<float>(d, grid, (size_t)cb_per_block * HUB * d * sizeof(float), st, (const float*)x, n, n_pad,
                             (const float*)ctrl, m, m_pad, (float)s, cb_per_block, (float*)ublk);
    else
        launch_ublk_d<double>(d, grid, (size_t)cb_per_block * HUB * d * sizeof(double), st, (const double*)x, n, n_pad,
                              (const double*)ctrl, m, m_pad, s, cb_per_block, (double*)ublk);
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" int mvf_eval_d(const void* x, int64_t n, const void* ctrl, int64_t m, int d, double beta, const double* C,
                          int dy, int flags, double* v, double* jac, double* div, double* acc, double* curv,
                          mvf_dtype dtype, void* stream) {
    MVF_REQUIRE(d >= 4 && d <= 8, "mvf_eval_d: d must be in 4 .. 8, got %d (d <= 3: mvf_eval)", d);
    MVF_REQUIRE(dy >= 1 && dy <= 8, "mvf_eval_d: dy must be in 1 .. 8, got %d", dy);
    MVF_REQUIRE(n >= 0 && m >= 0, "mvf_eval_d: bad shape n=%lld m=%lld", (long long)n, (long long)m);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "mvf_eval_d: bad dtype %d", (int)dtype);
    MVF_REQUIRE(beta > 0.0 && std::isfinite(beta), "mvf_eval_d: beta must be finite and > 0");
    const int known = MVF_EVAL_V | MVF_EVAL_JAC | MVF_EVAL_DIV | MVF_EVAL_ACC | MVF_EVAL_CURV;
    MVF_REQUIRE(flags != 0 && !(flags & ~known),
                "mvf_eval_d: flags 0x%x: only V, JAC, DIV, ACC and CURV are defined in 4 .. 8 dimensions", flags);
    MVF_REQUIRE(!(flags & (MVF_EVAL_DIV | MVF_EVAL_ACC | MVF_EVAL_CURV)) || dy == d,
                "mvf_eval_d: divergence / acceleration / curvature need dy == d (dy=%d, d=%d)", dy, d);
    MVF_REQUIRE(!(flags & MVF_EVAL_V) || v, "mvf_eval_d: v requested but null");
    MVF_REQUIRE(!(flags & MVF_EVAL_JAC) || jac, "mvf_eval_d: jac requested but null");
    MVF_REQUIRE(!(flags & MVF_EVAL_DIV) || div, "mvf_eval_d: div requested but null");
    MVF_REQUIRE(!(flags & MVF_EVAL_ACC) || acc, "mvf_eval_d: acc requested but null");
    MVF_REQUIRE(!(flags & MVF_EVAL_CURV) || curv, "mvf_eval_d: curv requested but null");
    if (n == 0) return 0;
    MVF_REQUIRE(x && (m == 0 || (ctrl && C)), "mvf_eval_d: null input");
    MVF_REQUIRE(cdiv(n, 64) <= 0x7fffffffLL, "mvf_eval_d: n too large");
    const int ncols = (flags & ~MVF_EVAL_V) ? dy * (1 + d) : dy;
    const int nct = (int)cdiv(ncols, 16);
    hipStream_t st = (hipStream_t)stream;
    const double s = std::sqrt(beta * LOG2E);
    // (x - c) = (scaled difference) / s, with s as the kernel rounds it
    const double jscale = -2.0 * beta / ((dtype == MVF_F32) ? (double)(float)s : s);
    const EvalDOut o{v, jac, div, acc, curv};
    const int rc = dtype == MVF_F32
                       ? launch_eval_d_dim<float>(d, nct, (const float*)x, n, (const float*)ctrl, m, (float)s, jscale, C, dy,
                                                  ncols, flags, o, st)
                       : launch_eval_d_dim<double>(d, nct, (const double*)x, n, (const double*)ctrl, m, s, jscale, C, dy,
                                                   ncols, flags, o, st);
    if (rc) return rc;
    MVF_LAUNCH_CHECK();
    return 0;
}
