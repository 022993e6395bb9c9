// Values and spatial gradients of a WIDE field  v(x) = sum_m K(x, c_m) C[m, :]  with dy = #keys output columns at d <= 3
//
// Reference: dynamo `vector_field_function` / `Jacobian_rkhs_gaussian` for Dy = #keys on the result of
// spateo/tdr/interpolations/interpolation_sparseVFC.py:63 (in-tree twin of the Jacobian: morphofield_dg/GPVectorField.py:143-190,
// J[f][i][q] = -2 beta sum_m K(x_q, c_m) C[m, f] (x_q - c_m)_i, layout (dy, d, n)).
//
// The identity of eval_mfma_kernel (mvf_eval.hip), for any number of columns:
//     sum_m K_m C[m, f] (p - c_m)_i = p_i v_f - W_i[f],     v = K @ C,   W_i = (K (.) c_i) @ C
// so values + gradient are 1 + d products of a GENERATED queries x m operand with C, on the matrix cores
// (v_mfma_f64_16x16x4_f64, float64 accumulation).  c_i multiplies the A side: a lane forms K once per k-step and d float64
// products K c_i; the B operand (a 16-column tile of C from LDS) is then shared by the 1 + d MFMAs of a column tile.
//
// Workgroup = 4 waves; a wave owns ONE tile of 16 queries, the workgroup one panel of EW_PANEL = 64 columns: 4 column tiles x
// (1 + d) operands = 16 accumulator tiles (128 VGPRs) per wave and 16 MFMAs per kernel value per lane.  The control points and
// the panel's rows of C are staged in LDS EW_CHUNK = 64 control points at a time.  One workgroup runs over all m for its
// (query tile, panel): no split-K, no atomics, the same bits on every call.  The Jacobian tiles go through LDS on the way out
// so that 16 lanes write 16 consecutive queries of one (f, i) row.
#include "mvf_common.h"

namespace mvf {

constexpr int EW_PANEL = 64;   // columns of C per workgroup (tests/_eval_wide_cases.py: PANEL)
constexpr int EW_CHUNK = 64;   // control points staged per pass (tests/_eval_wide_cases.py: CHUNK)
constexpr int EW_BROW = 72;    // padded row (doubles) of the staged panel of C
constexpr int EW_TROW = 17;    // padded row of a transposed 16 x 16 result tile
typedef double f64x4 __attribute__((ext_vector_type(4)));

// NOPS = 1 (values only) or 1 + d (values and Jacobian sums).  The second launch bound keeps 4 operands within 256 registers
// (160 / 184 VGPRs, no scratch): 3 / 2 workgroups per CU, so that one's staging hides behind the others' MFMAs; without it the
// compiler takes 148 VGPRs + 128 AGPRs and one workgroup per CU (profiles/eval_wide.md).
template <typename T, int NOPS>
__global__ __launch_bounds__(256, 2) void eval_wide_kernel(const T* __restrict__ x4, int64_t n, const T* __restrict__ ctrl4,
                                                        int64_t m, T s, double jscale /* -2 beta / s */,
                                                        const double* __restrict__ C, int64_t ldc, int dy, int flags,
                                                        double* __restrict__ v, int64_t ldv, double* __restrict__ jac) {
    using V4T = typename Vec4<T>::type;
    constexpr int D = NOPS - 1;
    constexpr size_t STAGE = EW_CHUNK * EW_BROW * sizeof(double);
    constexpr size_t RES = 4 * (NOPS > 1 ? NOPS : 1) * 16 * EW_TROW * sizeof(double);
    __shared__ __attribute__((aligned(16))) unsigned char smem_raw[STAGE > RES ? STAGE : RES];
    __shared__ V4T sc[EW_CHUNK];
    double* sB = reinterpret_cast<double*>(smem_raw);   // [EW_CHUNK][EW_BROW]
    double* res = reinterpret_cast<double*>(smem_raw);  // [wave][operand][16][EW_TROW], after the products

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * 64 + wave * 16;  // first query of this wave's tile
    const int f0 = (int)blockIdx.y * EW_PANEL;                // first column of this workgroup's panel
    const int pw = min(EW_PANEL, dy - f0);                    // live columns of the panel
    const int nct = (pw + 15) >> 4;                           // live 16-column tiles (uniform over the workgroup)

    const int64_t qa = q0 + li;  // the query of this lane on the A side, and after the transposition of the results
    const V4T xv = (qa < n) ? reinterpret_cast<const V4T*>(x4)[qa] : V4T{0, 0, 0, 0};
    const T px = xv.x * s, py = xv.y * s, pz = xv.z * s;

    f64x4 acc[4][NOPS];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int o = 0; o < NOPS; ++o) acc[ct][o] = f64x4{0.0, 0.0, 0.0, 0.0};

    for (int64_t m0 = 0; m0 < m; m0 += EW_CHUNK) {
        const int mc = (int)min((int64_t)EW_CHUNK, m - m0);
        __syncthreads();
        if (tid < EW_CHUNK) {
            V4T cs = V4T{0, 0, 0, 0};  // a padded control point meets rows of zeros: K x 0
            if (tid < mc) {
                const V4T cv = reinterpret_cast<const V4T*>(ctrl4)[m0 + tid];
                cs = V4T{cv.x * s, cv.y * s, cv.z * s, 0};
            }
            sc[tid] = cs;
        }
        {
            const int col = tid & 63;
            for (int row = tid >> 6; row < EW_CHUNK; row += 4)
                sB[row * EW_BROW + col] = (row < mc && col < pw) ? C[(m0 + row) * ldc + f0 + col] : 0.0;
        }
        __syncthreads();
        const int nks = (mc + 3) >> 2;
        for (int ks = 0; ks < nks; ++ks) {
            const int j = 4 * ks + lk;
            const V4T cv = sc[j];
            double a[NOPS];
            a[0] = (double)kernel_value(px, py, pz, cv.x, cv.y, cv.z);
            if constexpr (D >= 1) a[1] = a[0] * (double)cv.x;
            if constexpr (D >= 2) a[2] = a[0] * (double)cv.y;
            if constexpr (D >= 3) a[3] = a[0] * (double)cv.z;
            const double* brow = sB + j * EW_BROW + li;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                if (ct < nct) {
                    const double b = brow[16 * ct];
#pragma unroll
                    for (int o = 0; o < NOPS; ++o)
                        acc[ct][o] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[o], b, acc[ct][o], 0, 0, 0);
                }
            }
        }
    }

    // D[i = lk + 4 r][j = li] of a tile: query q0 + lk + 4 r, column f0 + 16 ct + li
    if (flags & MVF_EVAL_V) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const int f = f0 + 16 * ct + li;
            if (ct < nct && f < dy) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t q = q0 + lk + 4 * r;
                    if (q < n) v[q * ldv + f] = acc[ct][0][r];
                }
            }
        }
    }
    if constexpr (NOPS > 1) {
        if (!(flags & MVF_EVAL_JAC)) return;  // (uniform; no barrier follows)
        const double pd[3] = {(double)px, (double)py, (double)pz};  // the scaled point as the loop saw it
        double* mine = res + (size_t)wave * NOPS * 16 * EW_TROW;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            if (ct < nct) {  // (uniform over the workgroup: every wave meets the same barriers)
                __syncthreads();  // the staging area, or the previous tile, has been read
#pragma unroll
                for (int o = 0; o < NOPS; ++o)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mine[(o * 16 + li) * EW_TROW + lk + 4 * r] = acc[ct][o][r];
                __syncthreads();
                // lane (li, lk) now takes query q0 + li of the columns f0 + 16 ct + lk + 4 r
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int jc = lk + 4 * r;
                    const int f = f0 + 16 * ct + jc;
                    if (f < dy && qa < n) {
                        const double vf = mine[jc * EW_TROW + li];
#pragma unroll
                        for (int i = 0; i < D; ++i) {
                            const double w = mine[((1 + i) * 16 + jc) * EW_TROW + li];
                            jac[((int64_t)f * D + i) * n + qa] = (pd[i] * vf - w) * jscale;
                        }
                    }
                }
            }
        }
    }
}

template <typename T, int NOPS>
static void launch_eval_wide(dim3 grid, hipStream_t st, const void* x4, int64_t n, const void* ctrl4, int64_t m, double s,
                             double jscale, const double* C, int64_t ldc, int dy, int flags, double* v, int64_t ldv,
                             double* jac) {
    hipLaunchKernelGGL((eval_wide_kernel<T, NOPS>), grid, dim3(256), 0, st, (const T*)x4, n, (const T*)ctrl4, m, (T)s, jscale,
                       C, ldc, dy, flags, v, ldv, jac);
}

template <typename T>
static void dispatch_eval_wide(int nops, dim3 grid, hipStream_t st, const void* x4, int64_t n, const void* ctrl4, int64_t m,
                               double s, double jscale, const double* C, int64_t ldc, int dy, int flags, double* v,
                               int64_t ldv, double* jac) {
    switch (nops) {
        case 1: launch_eval_wide<T, 1>(grid, st, x4, n, ctrl4, m, s, jscale, C, ldc, dy, flags, v, ldv, jac); break;
        case 2: launch_eval_wide<T, 2>(grid, st, x4, n, ctrl4, m, s, jscale, C, ldc, dy, flags, v, ldv, jac); break;
        case 3: launch_eval_wide<T, 3>(grid, st, x4, n, ctrl4, m, s, jscale, C, ldc, dy, flags, v, ldv, jac); break;
        default: launch_eval_wide<T, 4>(grid, st, x4, n, ctrl4, m, s, jscale, C, ldc, dy, flags, v, ldv, jac); break;
    }
}

}  // namespace mvf

using namespace mvf;

extern "C" int mvf_eval_wide(const void* x4, int64_t n, const void* ctrl4, int64_t m, int d, double beta, const double* C,
                             int64_t ldc, int dy, int flags, double* v, int64_t ldv, double* jac, mvf_dtype dtype,
                             void* stream) {
    MVF_REQUIRE(n >= 0 && m >= 0, "mvf_eval_wide: bad shape");
    MVF_REQUIRE(d >= 1 && d <= 3, "mvf_eval_wide: d must be 1, 2 or 3, got %d", d);
    MVF_REQUIRE(dy >= 0, "mvf_eval_wide: dy must be >= 0, got %d", dy);
    MVF_REQUIRE(beta > 0.0 && std::isfinite(beta), "mvf_eval_wide: beta must be finite and > 0");
    MVF_REQUIRE(flags != 0 && !(flags & ~(MVF_EVAL_V | MVF_EVAL_JAC)),
                "mvf_eval_wide: flags must be a non-empty subset of MVF_EVAL_V | MVF_EVAL_JAC, got %d", flags);
    MVF_REQUIRE(ldc >= dy, "mvf_eval_wide: ldc %lld < dy %d", (long long)ldc, dy);
    MVF_REQUIRE(!(flags & MVF_EVAL_V) || ldv >= dy, "mvf_eval_wide: ldv %lld < dy %d", (long long)ldv, dy);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "mvf_eval_wide: bad dtype %d", (int)dtype);
    if (n == 0 || dy == 0) return 0;
    MVF_REQUIRE(x4 && (m == 0 || (ctrl4 && C)), "mvf_eval_wide: null input");
    MVF_REQUIRE(!(flags & MVF_EVAL_V) || v, "mvf_eval_wide: v requested but null");
    MVF_REQUIRE(!(flags & MVF_EVAL_JAC) || jac, "mvf_eval_wide: jac requested but null");
    const int64_t panels = cdiv(dy, EW_PANEL), qblocks = cdiv(n, 64);
    MVF_REQUIRE(panels <= 65535 && qblocks <= 2147483647LL, "mvf_eval_wide: problem too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    const double s = std::sqrt(beta * LOG2E);
    // (x - c) = (scaled difference) / s, with s as the kernel rounds it
    const double jscale = -2.0 * beta / ((dtype == MVF_F32) ? (double)(float)s : s);
    const int nops = (flags & MVF_EVAL_JAC) ? 1 + d : 1;
    dim3 grid((unsigned)qblocks, (unsigned)panels);
    if (dtype == MVF_F32)
        dispatch_eval_wide<float>(nops, grid, st, x4, n, ctrl4, m, s, jscale, C, ldc, dy, flags, v, ldv, jac);
    else
        dispatch_eval_wide<double>(nops, grid, st, x4, n, ctrl4, m, s, jscale, C, ldc, dy, flags, v, ldv, jac);
    MVF_LAUNCH_CHECK();
    return 0;
}
