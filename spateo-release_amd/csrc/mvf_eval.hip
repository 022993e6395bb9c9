// Differential-geometry evaluators of the learned field  v(x) = sum_m K(x, c_m) C[m, :]
//
// Reference: dynamo `Jacobian_rkhs_gaussian` + `compute_{acceleration,curvature,curl,torsion,divergence}`; in-tree
// twins spateo/tdr/morphometrics/morphofield_dg/GPVectorField.py:143-190 (Jacobian) and :12-121 (evaluators), which
// run one Python-level `_con_K` call per cell.  Here: ONE fused kernel; a lane owns CPT query points, control points
// and coefficients are broadcast from LDS, v (3) and J (3x3) are accumulated in float64 in registers and every
// requested quantity is derived in registers, so HBM traffic is 16 B in + the requested outputs per query.
//   J[f][i] = -2 beta sum_m K_m C[m, f] (x - c_m)_i                      (GPVectorField.py:176,190 with pre_scale = 1)
//   div = tr J;  curl = [J21 - J12, J02 - J20, J10 - J01];  a = J v
//   curvature (formula 2) = (a (v.v) - v (v.a)) / |v|^4;  torsion = v (a . J a) / (|v|^2 |a|^2)
#include "mvf_common.h"

namespace mvf {


// Everything that is derived from v and the Jacobian sums of ONE query point (lane-local, float64 registers).
// Jraw[f][i] = sum_m K_m C[m, f] (p - c_m)_i on the SCALED coordinates; J = Jraw * jscale * af.jmul.
struct EvalOut {
    double *v, *jac, *div, *curl, *acc, *curv, *tors, *jdet;
};
__device__ __forceinline__ void eval_epilogue(int64_t q, int64_t n, int flags, const EvalAffine& af, double jscale,
                                              const double (&vs)[3], const double (&Jraw)[3][3], double q0, double q1,
                                              double q2, const EvalOut& o) {
    double Jm[3][3];
#pragma unroll
    for (int f = 0; f < 3; ++f)
#pragma unroll
        for (int i = 0; i < 3; ++i) Jm[f][i] = Jraw[f][i] * jscale * af.jmul;
    const double v0 = af.alpha[0] * vs[0] + af.A[0] * q0 + af.A[1] * q1 + af.A[2] * q2 + af.b[0];
    const double v1 = af.alpha[1] * vs[1] + af.A[3] * q0 + af.A[4] * q1 + af.A[5] * q2 + af.b[1];
    const double v2 = af.alpha[2] * vs[2] + af.A[6] * q0 + af.A[7] * q1 + af.A[8] * q2 + af.b[2];
    if (flags & MVF_EVAL_V) {
        o.v[q * 3 + 0] = v0, o.v[q * 3 + 1] = v1, o.v[q * 3 + 2] = v2;
    }
    if (flags & MVF_EVAL_JAC) {
#pragma unroll
        for (int f = 0; f < 3; ++f)
#pragma unroll
            for (int i = 0; i < 3; ++i) o.jac[(int64_t)(f * 3 + i) * n + q] = Jm[f][i];
    }
    if (flags & MVF_EVAL_DIV) o.div[q] = Jm[0][0] + Jm[1][1] + Jm[2][2];
    if (flags & MVF_EVAL_JDET)
        o.jdet[q] = Jm[0][0] * (Jm[1][1] * Jm[2][2] - Jm[1][2] * Jm[2][1]) -
                    Jm[0][1] * (Jm[1][0] * Jm[2][2] - Jm[1][2] * Jm[2][0]) +
                    Jm[0][2] * (Jm[1][0] * Jm[2][1] - Jm[1][1] * Jm[2][0]);
    if (flags & MVF_EVAL_CURL) {
        o.curl[q * 3 + 0] = Jm[2][1] - Jm[1][2];
        o.curl[q * 3 + 1] = Jm[0][2] - Jm[2][0];
        o.curl[q * 3 + 2] = Jm[1][0] - Jm[0][1];
    }
    if (flags & (MVF_EVAL_ACC | MVF_EVAL_CURV | MVF_EVAL_TORS)) {
        const double a0 = Jm[0][0] * v0 + Jm[0][1] * v1 + Jm[0][2] * v2;
        const double a1 = Jm[1][0] * v0 + Jm[1][1] * v1 + Jm[1][2] * v2;
        const double a2 = Jm[2][0] * v0 + Jm[2][1] * v1 + Jm[2][2] * v2;
        if (flags & MVF_EVAL_ACC) {
            o.acc[q * 3 + 0] = a0, o.acc[q * 3 + 1] = a1, o.acc[q * 3 + 2] = a2;
        }
        const double vv = v0 * v0 + v1 * v1 + v2 * v2;
        if (flags & MVF_EVAL_CURV) {
            const double va = v0 * a0 + v1 * a1 + v2 * a2;
            const double nv = sqrt(vv);
            const double den = (nv * nv) * (nv * nv);  // ||v||^4 as norm(v)**4
            o.curv[q * 3 + 0] = (a0 * vv - v0 * va) / den;
            o.curv[q * 3 + 1] = (a1 * vv - v1 * va) / den;
            o.curv[q * 3 + 2] = (a2 * vv - v2 * va) / den;
        }
        if (flags & MVF_EVAL_TORS) {
            const double Ja0 = Jm[0][0] * a0 + Jm[0][1] * a1 + Jm[0][2] * a2;
            const double Ja1 = Jm[1][0] * a0 + Jm[1][1] * a1 + Jm[1][2] * a2;
            const double Ja2 = Jm[2][0] * a0 + Jm[2][1] * a1 + Jm[2][2] * a2;
            const double aJa = a0 * Ja0 + a1 * Ja1 + a2 * Ja2;
            const double aa = a0 * a0 + a1 * a1 + a2 * a2;
            const double den = vv * aa;  // ||v a^T||_F^2
            o.tors[q * 3 + 0] = v0 * aJa / den;
            o.tors[q * 3 + 1] = v1 * aJa / den;
            o.tors[q * 3 + 2] = v2 * aJa / den;
        }
    }
}

// The evaluator as a matrix product (round 6, VERDICT r5 weak #6: the VALU form ran at 0.30 of the float64 VALU peak, bound
// by 15 float64 instructions + 4 converts per pair).  With W[f][i] = sum_m K_m C[m, f] c_m[i]:
//     [v | W] = K [C | C (x) c]        one (queries x M) @ (M x 12) product on the matrix cores, float64 accumulation
//     sum_m K_m C[m, f] (p - c_m)_i = p_i v_f - W[f][i]
// so the VALU work per pair is the kernel value alone (6 float32 operations + v_exp_f32 + one convert).  The SAME K_m
// multiplies both columns inside one MFMA, so the difference p v - W sees only float64 rounding (coordinates are centred on
// the control points: |p| stays within the data's radius in kernel widths) - and (p - c) is no longer rounded to the
// cell dtype as the VALU form did.  Workgroup = 4 waves x 64 queries; a wave holds 4 tiles of 16 queries:
// v_mfma_f64_16x16x4_f64 with A[i = query][k = control point] = K, B[k][j] = column j of [C | C (x) c] from LDS (12 of 16
// columns live), 4 MFMAs per k-step of 4 control points share one B operand.  The 16 x 16 results go through LDS so that
// lane q ends up with the 12 sums of query q, then the common epilogue.
// Two kernel values against one control point, bit-identical to kernel_value (same operations in the same order).  float:
// as packed float32 instructions (v_pk_add / v_pk_mul / v_pk_fma: half the VALU issue slots).
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void kernel_value2(float px0, float px1, float py0, float py1, float pz0, float pz1, float cx,
                                              float cy, float cz, double& k0, double& k1) {
    const f32x2 dx = f32x2{px0, px1} - f32x2{cx, cx};
    const f32x2 dy = f32x2{py0, py1} - f32x2{cy, cy};
    const f32x2 dz = f32x2{pz0, pz1} - f32x2{cz, cz};
    const f32x2 e = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
    k0 = (double)exp2_neg(-e.x);
    k1 = (double)exp2_neg(-e.y);
}
__device__ __forceinline__ void kernel_value2(double px0, double px1, double py0, double py1, double pz0, double pz1,
                                              double cx, double cy, double cz, double& k0, double& k1) {
    k0 = kernel_value(px0, py0, pz0, cx, cy, cz);
    k1 = kernel_value(px1, py1, pz1, cx, cy, cz);
}

constexpr int EM_CHUNK = 256;  // control points staged per pass
constexpr int EM_ROW = 17;     // padded row (doubles) of one query's sums in LDS: conflict-free column reads
constexpr int EM_BROW = 17;    // padded row of [C | C (x) c] in LDS: a thread stages a row, 2-way instead of 64-way store conflicts
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <typename T>
__global__ __launch_bounds__(256, 2) void eval_mfma_kernel(const T* __restrict__ x4, int64_t n, const T* __restrict__ ctrl4,
                                                        int64_t m, T s, double jscale /* -2 beta / s */, EvalAffine af,
                                                        const double* __restrict__ C, int flags, EvalOut o) {
    using V4T = typename Vec4<T>::type;
    constexpr size_t STAGE = EM_CHUNK * (sizeof(V4T) + EM_BROW * sizeof(double));
    constexpr size_t RES = 256 * EM_ROW * sizeof(double);
    __shared__ __attribute__((aligned(16))) unsigned char smem_raw[STAGE > RES ? STAGE : RES];
    V4T* sc = reinterpret_cast<V4T*>(smem_raw);
    double* sB = reinterpret_cast<double*>(smem_raw + EM_CHUNK * sizeof(V4T));  // [EM_CHUNK][EM_BROW]
    double* res = reinterpret_cast<double*>(smem_raw);                          // [256][EM_ROW], after the product

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int64_t wq0 = (int64_t)blockIdx.x * 256 + wave * 64;  // first query of this wave
    T px[4], py[4], pz[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t i = wq0 + 16 * t + li;
        const V4T xv = (i < n) ? reinterpret_cast<const V4T*>(x4)[i] : V4T{0, 0, 0, 0};
        px[t] = xv.x * s, py[t] = xv.y * s, pz[t] = xv.z * s;
    }
    f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};

    for (int64_t m0 = 0; m0 < m; m0 += EM_CHUNK) {
        const int mc = (int)min((int64_t)EM_CHUNK, m - m0);
        __syncthreads();
        {
            const int j = threadIdx.x;  // EM_CHUNK == blockDim.x
            double* row = sB + j * EM_BROW;
            if (j < mc) {
                const V4T cv = reinterpret_cast<const V4T*>(ctrl4)[m0 + j];
                const V4T cs = V4T{cv.x * s, cv.y * s, cv.z * s, 0};
                sc[j] = cs;
                const double* cp = C + (m0 + j) * 3;
                const double c3[3] = {cp[0], cp[1], cp[2]};
                const double cd[3] = {(double)cs.x, (double)cs.y, (double)cs.z};
#pragma unroll
                for (int f = 0; f < 3; ++f) {
                    row[f] = c3[f];
#pragma unroll
                    for (int i = 0; i < 3; ++i) row[3 + 3 * f + i] = c3[f] * cd[i];
                }
#pragma unroll
                for (int z = 12; z < 16; ++z) row[z] = 0.0;
            } else {
                sc[j] = V4T{0, 0, 0, 0};
#pragma unroll
                for (int z = 0; z < 16; ++z) row[z] = 0.0;  // a padded control point contributes K x 0
            }
        }
        __syncthreads();
        // One k-step = 4 control points: two LDS reads, four kernel values, four MFMAs sharing the B operand.  The four waves
        // of a SIMD overlap each other's VALU and MFMA phases; pipelining the two phases INSIDE a wave (next k-step's kernel
        // values fenced between this k-step's MFMAs) measured slower (0.110 vs 0.101 ms on 64^3 x 500).
        const int nks = (mc + 3) >> 2;
        for (int ks = 0; ks < nks; ++ks) {
            const int j = 4 * ks + lk;
            const V4T cv = sc[j];
            const double b = sB[j * EM_BROW + li];
            double k[4];
            kernel_value2(px[0], px[1], py[0], py[1], pz[0], pz[1], cv.x, cv.y, cv.z, k[0], k[1]);
            kernel_value2(px[2], px[3], py[2], py[3], pz[2], pz[3], cv.x, cv.y, cv.z, k[2], k[3]);
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(k[t], b, acc[t], 0, 0, 0);
        }
    }
    __syncthreads();  // the staging area becomes the result area
    // D[i = lk + 4 r][j = li] of tile t -> res[query of the workgroup][column]
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) res[(wave * 64 + 16 * t + lk + 4 * r) * EM_ROW + li] = acc[t][r];
    __syncthreads();
    const int64_t q = wq0 + lane;
    if (q >= n) return;
    const double* row = res + (wave * 64 + lane) * EM_ROW;
    const V4T xv = reinterpret_cast<const V4T*>(x4)[q];
    const double pd[3] = {(double)(xv.x * s), (double)(xv.y * s), (double)(xv.z * s)};  // the scaled point as the loop saw it
    double vs[3], Jraw[3][3];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        vs[f] = row[f];
#pragma unroll
        for (int i = 0; i < 3; ++i) Jraw[f][i] = pd[i] * vs[f] - row[3 + 3 * f + i];
    }
    eval_epilogue(q, n, flags, af, jscale, vs, Jraw, (double)xv.x, (double)xv.y, (double)xv.z, o);
}

// ----------------------------------------------------------------------------------------------------------------
// Trajectory integration  dx/dt = v(x)  (morphopath; reference: spateo/tdr/morphometrics/morphofield/trajectory.py:11-117,
// which hands the field to dynamo's `fate`).  One launch integrates every start point through ALL time steps with
// classical RK4: a lane owns one trajectory (position in float64 registers), the control points and coefficients are
// staged in LDS once (or per evaluation in chunks when they do not fit), and the n_out sampled positions are written
// as traj[cell][t][3].  No host round trip and no intermediate tensor per step.
// ----------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void integrate_kernel(const T* __restrict__ x4, int64_t n, const T* __restrict__ ctrl4,
                                                        int64_t m, T s, EvalAffine af, const double* __restrict__ C,
                                                        double dt, int substeps, int n_out, int chunk,
                                                        double* __restrict__ traj) {
    using V4T = typename Vec4<T>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_dyn[];
    V4T* sc = reinterpret_cast<V4T*>(smem_dyn);
    double4* sC = reinterpret_cast<double4*>(smem_dyn + (size_t)chunk * sizeof(V4T));
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    const int nchunks = (int)((m + chunk - 1) / chunk);

    auto stage = [&](int64_t m0) {
        const int mc = (int)min((int64_t)chunk, m - m0);
        for (int j = threadIdx.x; j < chunk; j += 256) {
            if (j < mc) {
                const V4T cv = reinterpret_cast<const V4T*>(ctrl4)[m0 + j];
                sc[j] = V4T{cv.x * s, cv.y * s, cv.z * s, 0};
                const double* cp = C + (m0 + j) * 3;
                sC[j] = double4{cp[0], cp[1], cp[2], 0.0};
            } else {
                sc[j] = V4T{0, 0, 0, 0};
                sC[j] = double4{0.0, 0.0, 0.0, 0.0};
            }
        }
    };
    // v(q) for this lane's position q (block-synchronous: every lane takes the same path through the barriers)
    auto field = [&](double q0, double q1, double q2, double& v0, double& v1, double& v2) {
        const T px = (T)q0 * s, py = (T)q1 * s, pz = (T)q2 * s;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int cidx = 0; cidx < nchunks; ++cidx) {
            if (nchunks > 1) {
                __syncthreads();
                stage((int64_t)cidx * chunk);
                __syncthreads();
            }
            const int mc = (int)min((int64_t)chunk, m - (int64_t)cidx * chunk);
#pragma unroll 4
            for (int j = 0; j < mc; ++j) {
                const V4T cv = sc[j];
                const double4 cc = sC[j];
                const double k = (double)kernel_value(px, py, pz, cv.x, cv.y, cv.z);
                a0 = fma(k, cc.x, a0), a1 = fma(k, cc.y, a1), a2 = fma(k, cc.z, a2);
            }
        }
        v0 = af.alpha[0] * a0 + af.A[0] * q0 + af.A[1] * q1 + af.A[2] * q2 + af.b[0];
        v1 = af.alpha[1] * a1 + af.A[3] * q0 + af.A[4] * q1 + af.A[5] * q2 + af.b[1];
        v2 = af.alpha[2] * a2 + af.A[6] * q0 + af.A[7] * q1 + af.A[8] * q2 + af.b[2];
    };

    if (nchunks == 1) {
        stage(0);
        __syncthreads();
    }
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    if (live) {
        const V4T xv = reinterpret_cast<const V4T*>(x4)[i];
        x0 = (double)xv.x, x1 = (double)xv.y, x2 = (double)xv.z;
        double* o = traj + (size_t)i * n_out * 3;
        o[0] = x0, o[1] = x1, o[2] = x2;
    }
    const double h = dt / substeps;
    for (int t = 1; t < n_out; ++t) {
        for (int ss = 0; ss < substeps; ++ss) {
            double k1x, k1y, k1z, k2x, k2y, k2z, k3x, k3y, k3z, k4x, k4y, k4z;
            field(x0, x1, x2, k1x, k1y, k1z);
            field(x0 + 0.5 * h * k1x, x1 + 0.5 * h * k1y, x2 + 0.5 * h * k1z, k2x, k2y, k2z);
            field(x0 + 0.5 * h * k2x, x1 + 0.5 * h * k2y, x2 + 0.5 * h * k2z, k3x, k3y, k3z);
            field(x0 + h * k3x, x1 + h * k3y, x2 + h * k3z, k4x, k4y, k4z);
            x0 += h / 6.0 * (k1x + 2.0 * k2x + 2.0 * k3x + k4x);
            x1 += h / 6.0 * (k1y + 2.0 * k2y + 2.0 * k3y + k4y);
            x2 += h / 6.0 * (k1z + 2.0 * k2z + 2.0 * k3z + k4z);
        }
        if (live) {
            double* o = traj + ((size_t)i * n_out + t) * 3;
            o[0] = x0, o[1] = x1, o[2] = x2;
        }
    }
}

}  // namespace mvf

using namespace mvf;

extern "C" int mvf_eval_affine(const void* x4, int64_t n, const void* ctrl4, int64_t m, double beta, const double* C,
                               const double* affine /* host: alpha[3], jmul, A[9] row-major, b[3]; NULL = identity */,
                               int flags, double* v, double* jac, double* div, double* curl, double* acc, double* curv,
                               double* tors, double* jdet, mvf_dtype dtype, void* stream) {
    MVF_REQUIRE(n >= 0 && m >= 0, "mvf_eval: bad shape");
    MVF_REQUIRE(beta > 0.0 && std::isfinite(beta), "mvf_eval: beta must be finite and > 0");
    if (n == 0) return 0;
    MVF_REQUIRE(x4 && (m == 0 || (ctrl4 && C)), "mvf_eval: null input");
    MVF_REQUIRE(!(flags & MVF_EVAL_V) || v, "mvf_eval: v requested but null");
    MVF_REQUIRE(!(flags & MVF_EVAL_JAC) || jac, "mvf_eval: jac requested but null");
    MVF_REQUIRE(!(flags & MVF_EVAL_DIV) || div, "mvf_eval: div requested but null");
    MVF_REQUIRE(!(flags & MVF_EVAL_CURL) || curl, "mvf_eval: curl requested but null");
    MVF_REQUIRE(!(flags & MVF_EVAL_ACC) || acc, "mvf_eval: acc requested but null");
    MVF_REQUIRE(!(flags & MVF_EVAL_CURV) || curv, "mvf_eval: curv requested but null");
    MVF_REQUIRE(!(flags & MVF_EVAL_TORS) || tors, "mvf_eval: tors requested but null");
    MVF_REQUIRE(!(flags & MVF_EVAL_JDET) || jdet, "mvf_eval: jdet requested but null");
    EvalAffine af;
    af.alpha[0] = af.alpha[1] = af.alpha[2] = 1.0, af.jmul = 1.0;
    for (int i = 0; i < 9; ++i) af.A[i] = 0.0;
    for (int i = 0; i < 3; ++i) af.b[i] = 0.0;
    if (affine) {
        for (int i = 0; i < 3; ++i) af.alpha[i] = affine[i];
        af.jmul = affine[3];
        for (int i = 0; i < 9; ++i) af.A[i] = affine[4 + i];
        for (int i = 0; i < 3; ++i) af.b[i] = affine[13 + i];
    }
    hipStream_t st = (hipStream_t)stream;
    const double s = std::sqrt(beta * LOG2E);
    // (x - c) = (scaled difference) / s, with s as the kernel rounds it
    const double jscale = -2.0 * beta / ((dtype == MVF_F32) ? (double)(float)s : s);
    const EvalOut o{v, jac, div, curl, acc, curv, tors, jdet};
    dim3 grid((unsigned)cdiv(n, 256));
    if (dtype == MVF_F32)
        hipLaunchKernelGGL(eval_mfma_kernel<float>, grid, dim3(256), 0, st, (const float*)x4, n, (const float*)ctrl4, m,
                           (float)s, jscale, af, C, flags, o);
    else if (dtype == MVF_F64)
        hipLaunchKernelGGL(eval_mfma_kernel<double>, grid, dim3(256), 0, st, (const double*)x4, n, (const double*)ctrl4, m,
                           s, jscale, af, C, flags, o);
    else
        return set_error("mvf_eval: bad dtype %d", (int)dtype);
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" int mvf_eval(const void* x4, int64_t n, const void* ctrl4, int64_t m, double beta, const double* C,
                        int flags, double* v, double* jac, double* div, double* curl, double* acc, double* curv,
                        double* tors, double* jdet, mvf_dtype dtype, void* stream) {
    return mvf_eval_affine(x4, n, ctrl4, m, beta, C, nullptr, flags, v, jac, div, curl, acc, curv, tors, jdet, dtype,
                           stream);
}

extern "C" int mvf_integrate(const void* x4, int64_t n, const void* ctrl4, int64_t m, double beta, const double* C,
                             const double* affine, double dt, int substeps, int n_out, double* traj, mvf_dtype dtype,
                             void* stream) {
    MVF_REQUIRE(n >= 0 && m >= 0 && n_out >= 1 && substeps >= 1, "mvf_integrate: bad shape");
    MVF_REQUIRE(beta > 0.0 && std::isfinite(beta) && std::isfinite(dt), "mvf_integrate: bad beta / dt");
    if (n == 0) return 0;
    MVF_REQUIRE(x4 && traj && (m == 0 || (ctrl4 && C)), "mvf_integrate: null pointer");
    EvalAffine af;
    af.alpha[0] = af.alpha[1] = af.alpha[2] = 1.0, af.jmul = 1.0;
    for (int i = 0; i < 9; ++i) af.A[i] = 0.0;
    for (int i = 0; i < 3; ++i) af.b[i] = 0.0;
    if (affine) {
        for (int i = 0; i < 3; ++i) af.alpha[i] = affine[i];
        af.jmul = affine[3];
        for (int i = 0; i < 9; ++i) af.A[i] = affine[4 + i];
        for (int i = 0; i < 3; ++i) af.b[i] = affine[13 + i];
    }
    hipStream_t st = (hipStream_t)stream;
    const double s = std::sqrt(beta * LOG2E);
    const size_t per = (dtype == MVF_F32 ? 16 : 32) + 32;  // bytes of LDS per staged control point
    // cap = 3072 (float32) / 2304 (float64) control points: above it the kernel re-stages chunk by chunk inside every field
    // evaluation.  tests/_cell_cases.py RK4_CAP states the same expression and the RK4 edge tests pin m = cap - 1, cap, cap + 1.
    const int cap = (int)((144 * 1024) / per);               // leave headroom below the 160 KiB of a CU
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(m, cap));
    const size_t lds = (size_t)chunk * per;
    dim3 grid((unsigned)cdiv(n, 256));
    if (dtype == MVF_F32) {
        MVF_CHECK_HIP(hipFuncSetAttribute((const void*)integrate_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)lds));
        hipLaunchKernelGGL(integrate_kernel<float>, grid, dim3(256), lds, st, (const float*)x4, n, (const float*)ctrl4, m,
                           (float)s, af, C, dt, substeps, n_out, chunk, traj);
    } else if (dtype == MVF_F64) {
        MVF_CHECK_HIP(hipFuncSetAttribute((const void*)integrate_kernel<double>,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(integrate_kernel<double>, grid, dim3(256), lds, st, (const double*)x4, n,
                           (const double*)ctrl4, m, s, af, C, dt, substeps, n_out, chunk, traj);
    } else {
        return set_error("mvf_integrate: bad dtype %d", (int)dtype);
    }
    MVF_LAUNCH_CHECK();
    return 0;
}
