// The O(N) glue of one `Morpho_pairwise` iteration between the fused assignment (mvf_assign) and the non-rigid update
// (mvf_gram / mvf_solve_minnorm / mvf_apply / mvf_pinv_diag), so that nothing of size NA or NB crosses the link inside the
// loop of spateo/alignment/methods/morpho_class.py:280-294:
//
//   mvf_align_alpha      alpha_i = exp(psi(kappa_i + K_NA_spatial_i) - psi(kappa_i NA + Sp_spatial))  (:1250-1252) and the next
//                        assignment's model_mul_i = alpha_i exp(-SigmaDiag_i / sigma2)                 (:1087)
//   mvf_align_moments    every reduction `_update_rigid` (:1300-1408), `_update_sigma2` (:1410-1435) and `_get_optimal_R`
//                        (:1437-1469) take from the cell arrays, without P: 64 float64 in one block
//   mvf_align_transform  RnA = coordsA R^T + t, XAHat = VnA + RnA (:1404, :293), PXB_term = P coordsB - RnA K_NA (:1276) and
//                        Y = PXB_term / K_NA, written in the layouts mvf_assign and mvf_gram read
//
// and for the SVI mode of that loop (:283-284, 894-896: one batch of B per iteration, running averages with step_size):
//
//   mvf_align_gather         the batch's rows of xb4, coordsB and every prepared B layer into contiguous batch buffers
//   mvf_align_alpha_svi      mvf_align_alpha with the blend of :1240-1247
//   mvf_align_transform_svi  the blended PXB_term of :1270-1274 and the Gram stage's operands for unit weights
//
// All arithmetic is float64 whatever the cell dtype (the library is built with -ffp-contract=off: a * b + c is a rounded
// product and a rounded sum, never an fma).  No floating-point atomics: every workgroup writes its partial sums to the
// workspace and ONE workgroup adds them in workgroup order, so two calls give the same bits.
//
// Operation order of mvf_align_transform (what tests/test_gpu_align_kernels.py evaluates in NumPy, to the last place), per
// cell with x = coordsA row, v = VnA row (widened from the cell dtype), k = K_NA, o = origin (0 when NULL), d = 0, 1, 2:
//   RnA_d      = ((x_0 R[d][0] + x_1 R[d][1]) + x_2 R[d][2]) + t_d
//   XAHat_d    = v_d + RnA_d                          xa4_d = (T)(XAHat_d - o_d), xa4_3 = 0
//   PXB_term_d = PXB_d - (RnA_d - o_d) k              (PXB = P (coordsB - o): what mvf_assign returns for xb4 = coordsB - o)
//   Y_d        = k != 0 ? PXB_term_d / k : 0          Y4_d = (T)Y_d, Y4_3 = 0,  Pw = (T)k
//
// The second-order sums of mvf_align_moments are taken on CENTRED rows, as the reference takes them: a first pass forms the
// weighted means on the device, a second pass the products of differences.  Raw moments with the mean taken out afterwards
// cancel when a slice sits far from the origin.
#include "mvf_common.h"

namespace mvf {
namespace {

constexpr int AL_MAX_BLOCKS = 1024;    // workgroups of a reduction pass (each strides over the cells)
constexpr int AL_CELLS_PER_BLOCK = 1024;
constexpr int AL_S1 = 16;              // partial sums per workgroup, first pass (14 used)
constexpr int AL_S2 = 32;              // second pass (27 used)
static_assert(MVF_ALIGN_MOMENT_DOUBLES == 64, "block layout mismatch with mvf.h");

// digamma for x > 0: psi(x) = psi(x + k) - sum_{j < k} 1 / (x + j) up to x + k >= 10, then the asymptotic series
// ln x - 1/(2x) - sum B_2j / (2j x^2j) through x^-14 (the first omitted term is 4.4e-17 at x = 10).  The host evaluates the
// same formula in Python for gamma (spateo_amd.align._digamma).
__device__ __forceinline__ double digamma_pos(double x) {
    double s = 0.0;
    while (x < 10.0) {
        s += 1.0 / x;
        x += 1.0;
    }
    const double r = 1.0 / x, r2 = r * r;
    double p = 1.0 / 12.0;
    p = p * r2 - 691.0 / 32760.0;
    p = p * r2 + 1.0 / 132.0;
    p = p * r2 - 1.0 / 240.0;
    p = p * r2 + 1.0 / 252.0;
    p = p * r2 - 1.0 / 120.0;
    p = p * r2 + 1.0 / 12.0;
    return ((log(x) - 0.5 * r) - p * r2) - s;
}

__global__ __launch_bounds__(256) void align_alpha_kernel(const double* __restrict__ kappa, const double* __restrict__ Ks,
                                                          const double* __restrict__ sd, int64_t n, double Sp_spatial,
                                                          double sigma2, double* __restrict__ alpha,
                                                          double* __restrict__ model_mul) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double kp = kappa[i];
    const double a = exp(digamma_pos(kp + Ks[i]) - digamma_pos(kp * (double)n + Sp_spatial));
    alpha[i] = a;
    model_mul[i] = a * exp(-sd[i] / sigma2);
}

// the SVI blend of :1240-1247: step * (the value above) + (1 - step) * alpha; step == 1 takes the value itself, so that the
// bits are mvf_align_alpha's whatever `alpha` held
__global__ __launch_bounds__(256) void align_alpha_svi_kernel(const double* __restrict__ kappa, const double* __restrict__ Ks,
                                                              const double* __restrict__ sd, int64_t n, double Sp_spatial,
                                                              double sigma2, double step, double* __restrict__ alpha,
                                                              double* __restrict__ model_mul) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double kp = kappa[i];
    double a = exp(digamma_pos(kp + Ks[i]) - digamma_pos(kp * (double)n + Sp_spatial));
    if (step < 1.0) a = step * a + (1.0 - step) * alpha[i];
    alpha[i] = a;
    model_mul[i] = a * exp(-sd[i] / sigma2);
}

struct Rt {
    double R[9], t[3], o[3];
};

struct Org {
    double o[3];
};

template <typename T>
__global__ __launch_bounds__(256) void align_transform_svi_kernel(const double* __restrict__ RnA, const double* __restrict__ PXB,
                                                                  const double* __restrict__ K, int64_t n, Org org, double step,
                                                                  double* __restrict__ PXB_term, T* __restrict__ Y4,
                                                                  T* __restrict__ Pw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double k = K[i], rest = 1.0 - step;
    double pt[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double now = PXB[3 * i + d] - (RnA[3 * i + d] - org.o[d]) * k;
        pt[d] = step * now + rest * PXB_term[3 * i + d];
        PXB_term[3 * i + d] = pt[d];
    }
    typename Vec4<T>::type u;
    u.x = (T)pt[0], u.y = (T)pt[1], u.z = (T)pt[2], u.w = (T)0;
    *reinterpret_cast<typename Vec4<T>::type*>(Y4 + 4 * i) = u;
    Pw[i] = (T)k;
}

// ---- the batch gather --------------------------------------------------------------------------------------------------
// Segment y of the grid: 0 = the per-row small parts (one lane per batch row: its xb4 vector, its three coordsB values and
// every layer's row constant b), 1 + l = the prepared rows of layer l, moved as 16-byte chunks with consecutive lanes on
// consecutive chunks of a row (rows are ld * sizeof(T) bytes, a multiple of 64, and start 16-byte aligned).
struct GatherArgs {
    const uint4* ysrc[MVF_ASSIGN_MAX_LAYERS];
    uint4* ydst[MVF_ASSIGN_MAX_LAYERS];
    int64_t chunks[MVF_ASSIGN_MAX_LAYERS];   // 16-byte chunks per row
    const double* bsrc[MVF_ASSIGN_MAX_LAYERS];
    double* bdst[MVF_ASSIGN_MAX_LAYERS];
    int nlayers;
    int x4_chunks;                           // 16-byte chunks per xb4 row: 1 (float32) or 2 (float64)
};

__device__ __forceinline__ int64_t batch_row(const int32_t* __restrict__ perm, int64_t nb, int64_t start, int64_t j) {
    int64_t p = start + j;                   // start < nb and j < bs <= nb: one wrap at the most
    if (p >= nb) p -= nb;
    return (int64_t)perm[p];
}

__global__ __launch_bounds__(256) void align_gather_kernel(const int32_t* __restrict__ perm, int64_t nb, int64_t start, int64_t bs,
                                                           const uint4* __restrict__ xb4, uint4* __restrict__ xb4_out,
                                                           const double* __restrict__ B, double* __restrict__ B_out,
                                                           GatherArgs ga) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.y == 0) {
        for (int64_t j = first; j < bs; j += stride) {
            const int64_t r = batch_row(perm, nb, start, j);
            for (int c = 0; c < ga.x4_chunks; ++c) xb4_out[j * ga.x4_chunks + c] = xb4[r * ga.x4_chunks + c];
            B_out[3 * j] = B[3 * r], B_out[3 * j + 1] = B[3 * r + 1], B_out[3 * j + 2] = B[3 * r + 2];
            for (int l = 0; l < ga.nlayers; ++l) ga.bdst[l][j] = ga.bsrc[l][r];
        }
        return;
    }
    const int l = (int)blockIdx.y - 1;
    const int64_t cpr = ga.chunks[l], total = bs * cpr;
    const uint4* __restrict__ src = ga.ysrc[l];
    uint4* __restrict__ dst = ga.ydst[l];
    for (int64_t c = first; c < total; c += stride) {
        const int64_t j = c / cpr, off = c - j * cpr;
        dst[c] = src[batch_row(perm, nb, start, j) * cpr + off];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void align_transform_kernel(const double* __restrict__ A, const T* __restrict__ V4,
                                                              const double* __restrict__ PXB, const double* __restrict__ K,
                                                              int64_t n, Rt rt, double* __restrict__ RnA,
                                                              double* __restrict__ XAHat, T* __restrict__ xa4,
                                                              double* __restrict__ PXB_term, T* __restrict__ Y4,
                                                              T* __restrict__ Pw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x0 = A[3 * i], x1 = A[3 * i + 1], x2 = A[3 * i + 2];
    double v[3] = {0.0, 0.0, 0.0};
    if (V4) {
        const typename Vec4<T>::type u = *reinterpret_cast<const typename Vec4<T>::type*>(V4 + 4 * i);
        v[0] = (double)u.x, v[1] = (double)u.y, v[2] = (double)u.z;
    }
    double rn[3], xh[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        rn[d] = ((x0 * rt.R[3 * d] + x1 * rt.R[3 * d + 1]) + x2 * rt.R[3 * d + 2]) + rt.t[d];
        xh[d] = v[d] + rn[d];
    }
    if (RnA) RnA[3 * i] = rn[0], RnA[3 * i + 1] = rn[1], RnA[3 * i + 2] = rn[2];
    if (XAHat) XAHat[3 * i] = xh[0], XAHat[3 * i + 1] = xh[1], XAHat[3 * i + 2] = xh[2];
    if (xa4) {
        typename Vec4<T>::type u;
        u.x = (T)(xh[0] - rt.o[0]), u.y = (T)(xh[1] - rt.o[1]), u.z = (T)(xh[2] - rt.o[2]), u.w = (T)0;
        *reinterpret_cast<typename Vec4<T>::type*>(xa4 + 4 * i) = u;
    }
    if (PXB_term || Y4 || Pw) {
        const double k = K[i];
        double pt[3], y[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            pt[d] = PXB[3 * i + d] - (rn[d] - rt.o[d]) * k;
            y[d] = k != 0.0 ? pt[d] / k : 0.0;
        }
        if (PXB_term) PXB_term[3 * i] = pt[0], PXB_term[3 * i + 1] = pt[1], PXB_term[3 * i + 2] = pt[2];
        if (Y4) {
            typename Vec4<T>::type u;
            u.x = (T)y[0], u.y = (T)y[1], u.z = (T)y[2], u.w = (T)0;
            *reinterpret_cast<typename Vec4<T>::type*>(Y4 + 4 * i) = u;
        }
        if (Pw) Pw[i] = (T)k;
    }
}

template <int NS>
__device__ __forceinline__ void block_store(const double (&s)[NS], int used, double* __restrict__ part, int stride) {
    __shared__ double red[4];
    for (int k = 0; k < used; ++k) {
        const double t = block_sum<256>(s[k], red);
        if (threadIdx.x == 0) part[(int64_t)blockIdx.x * stride + k] = t;
    }
}

// first pass: the weighted first-order sums.  s[0..2] K_NA . coordsA, s[3..5] K_NA . VnA, s[6..8] K_NB . coordsB, s[9] sum K_NB
// (Sp), s[10] sum K_NA, s[11] sum K_NA_spatial, s[12] sum K_NA_sigma2, s[13] sum K_NA_sigma2 SigmaDiag
template <typename T>
__global__ __launch_bounds__(256) void align_moments1_kernel(const double* __restrict__ A, const T* __restrict__ V4,
                                                             const double* __restrict__ K, const double* __restrict__ Ks,
                                                             const double* __restrict__ K2, const double* __restrict__ sd,
                                                             int64_t na, const double* __restrict__ B,
                                                             const double* __restrict__ KB, int64_t nb,
                                                             double* __restrict__ part) {
    double s[AL_S1];
#pragma unroll
    for (int k = 0; k < AL_S1; ++k) s[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < na; i += stride) {
        const double k = K[i], k2 = K2[i];
        const typename Vec4<T>::type u = *reinterpret_cast<const typename Vec4<T>::type*>(V4 + 4 * i);
        s[0] += k * A[3 * i], s[1] += k * A[3 * i + 1], s[2] += k * A[3 * i + 2];
        s[3] += k * (double)u.x, s[4] += k * (double)u.y, s[5] += k * (double)u.z;
        s[10] += k, s[11] += Ks[i], s[12] += k2, s[13] += k2 * sd[i];
    }
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < nb; j += stride) {
        const double k = KB[j];
        s[6] += k * B[3 * j], s[7] += k * B[3 * j + 1], s[8] += k * B[3 * j + 2];
        s[9] += k;
    }
    block_store<AL_S1>(s, 14, part, AL_S1);
}

// out[k] = sum over the workgroups, in order, of part[b * stride + k] (k < used); then the means mu_XA, mu_Vn, mu_XB =
// s[0..8] / Sp into out[14..22] (0 when Sp == 0) and zeros / `extra` behind the second pass's slots
__global__ __launch_bounds__(256) void align_finish1_kernel(const double* __restrict__ part, int nblk, const double* extra,
                                                            double* __restrict__ out) {
    __shared__ double red[4];
    __shared__ double tot[14];
    for (int k = 0; k < 14; ++k) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblk; b += 256) s += part[(int64_t)b * AL_S1 + k];
        const double t = block_sum<256>(s, red);
        if (threadIdx.x == 0) tot[k] = t;
    }
    __syncthreads();
    if (threadIdx.x < 14) out[threadIdx.x] = tot[threadIdx.x];
    if (threadIdx.x < 9) out[14 + threadIdx.x] = tot[9] != 0.0 ? tot[threadIdx.x] / tot[9] : 0.0;
    if (threadIdx.x >= 50 && threadIdx.x < MVF_ALIGN_MOMENT_DOUBLES)
        out[threadIdx.x] = (threadIdx.x == 50 && extra) ? extra[0] : 0.0;
}

// second pass, on rows centred by the device's means mu (out[14..22]); with xc = x - mu_XA, vc = v - mu_Vn and
// pc = PXB - K_NA (mu_XB - o):  s[0..8] sum K_NA xc vc^T, s[9..17] sum xc pc^T, s[18..20] sum K_NA xc, s[21..23] sum K_NA vc,
// s[24..26] sum pc
template <typename T>
__global__ __launch_bounds__(256) void align_moments2_kernel(const double* __restrict__ A, const T* __restrict__ V4,
                                                             const double* __restrict__ K, const double* __restrict__ PXB,
                                                             int64_t na, Rt rt, const double* __restrict__ out,
                                                             double* __restrict__ part) {
    double s[AL_S2];
#pragma unroll
    for (int k = 0; k < AL_S2; ++k) s[k] = 0.0;
    double ma[3], mv[3], mb[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) ma[d] = out[14 + d], mv[d] = out[17 + d], mb[d] = out[20 + d] - rt.o[d];
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < na; i += stride) {
        const double k = K[i];
        const typename Vec4<T>::type u = *reinterpret_cast<const typename Vec4<T>::type*>(V4 + 4 * i);
        const double xc[3] = {A[3 * i] - ma[0], A[3 * i + 1] - ma[1], A[3 * i + 2] - ma[2]};
        const double vc[3] = {(double)u.x - mv[0], (double)u.y - mv[1], (double)u.z - mv[2]};
        double pc[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) pc[d] = PXB[3 * i + d] - k * mb[d];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double kx = k * xc[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) s[3 * a + b] += kx * vc[b], s[9 + 3 * a + b] += xc[a] * pc[b];
            s[18 + a] += kx, s[21 + a] += k * vc[a], s[24 + a] += pc[a];
        }
    }
    block_store<AL_S2>(s, 27, part, AL_S2);
}

__global__ __launch_bounds__(256) void align_finish2_kernel(const double* __restrict__ part, int nblk, double* __restrict__ out) {
    __shared__ double red[4];
    for (int k = 0; k < 27; ++k) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblk; b += 256) s += part[(int64_t)b * AL_S2 + k];
        const double t = block_sum<256>(s, red);
        if (threadIdx.x == 0) out[23 + k] = t;
    }
}

int reduce_blocks(int64_t n) { return (int)std::min<int64_t>(AL_MAX_BLOCKS, std::max<int64_t>(1, cdiv(n, AL_CELLS_PER_BLOCK))); }

Rt make_rt(const double* Rt_host, const double* origin) {
    Rt rt;
    for (int i = 0; i < 9; ++i) rt.R[i] = Rt_host ? Rt_host[i] : (i % 4 == 0 ? 1.0 : 0.0);
    for (int i = 0; i < 3; ++i) rt.t[i] = Rt_host ? Rt_host[9 + i] : 0.0, rt.o[i] = origin ? origin[i] : 0.0;
    return rt;
}

}  // namespace
}  // namespace mvf

using namespace mvf;

extern "C" int mvf_align_alpha(const double* kappa, const double* K_NA_spatial, const double* SigmaDiag, int64_t na,
                               double Sp_spatial, double sigma2, double* alpha, double* model_mul, void* stream) {
    if (na == 0) return 0;
    MVF_REQUIRE(na > 0 && cdiv(na, 256) < ((int64_t)1 << 31), "mvf_align_alpha: bad cell count");
    MVF_REQUIRE(sigma2 > 0.0 && Sp_spatial >= 0.0, "mvf_align_alpha: need sigma2 > 0 and Sp_spatial >= 0");
    MVF_REQUIRE(kappa && K_NA_spatial && SigmaDiag && alpha && model_mul, "mvf_align_alpha: null pointer");
    hipLaunchKernelGGL(align_alpha_kernel, dim3((unsigned)cdiv(na, 256)), dim3(256), 0, (hipStream_t)stream, kappa, K_NA_spatial,
                       SigmaDiag, na, Sp_spatial, sigma2, alpha, model_mul);
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t mvf_align_workspace_bytes(int64_t na, int64_t nb) {
    if (na <= 0 || nb <= 0) return 0;
    return (size_t)reduce_blocks(std::max(na, nb)) * (AL_S1 + AL_S2) * sizeof(double);
}

extern "C" int mvf_align_moments(const double* coordsA, const void* VnA4, const double* K_NA, const double* K_NA_spatial,
                                 const double* K_NA_sigma2, const double* SigmaDiag, const double* PXB, int64_t na,
                                 const double* coordsB, const double* K_NB, int64_t nb, const double* origin, const double* extra,
                                 double* out, void* workspace, size_t workspace_bytes, mvf_dtype dtype, void* stream) {
    if (na == 0 || nb == 0) return 0;
    MVF_REQUIRE(na > 0 && nb > 0, "mvf_align_moments: negative size");
    MVF_REQUIRE(na < ((int64_t)1 << 40) && nb < ((int64_t)1 << 40), "mvf_align_moments: too many cells");
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "mvf_align_moments: bad dtype %d", (int)dtype);
    MVF_REQUIRE(coordsA && VnA4 && K_NA && K_NA_spatial && K_NA_sigma2 && SigmaDiag && PXB && coordsB && K_NB && out && workspace,
                "mvf_align_moments: null pointer");
    const int nblk = reduce_blocks(std::max(na, nb));
    const size_t need = (size_t)nblk * (AL_S1 + AL_S2) * sizeof(double);
    MVF_REQUIRE(workspace_bytes >= need, "mvf_align_moments: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    double* part1 = (double*)workspace;
    double* part2 = part1 + (size_t)nblk * AL_S1;
    const Rt rt = make_rt(nullptr, origin);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MVF_F32)
        hipLaunchKernelGGL(align_moments1_kernel<float>, dim3(nblk), dim3(256), 0, st, coordsA, (const float*)VnA4, K_NA,
                           K_NA_spatial, K_NA_sigma2, SigmaDiag, na, coordsB, K_NB, nb, part1);
    else
        hipLaunchKernelGGL(align_moments1_kernel<double>, dim3(nblk), dim3(256), 0, st, coordsA, (const double*)VnA4, K_NA,
                           K_NA_spatial, K_NA_sigma2, SigmaDiag, na, coordsB, K_NB, nb, part1);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(align_finish1_kernel, dim3(1), dim3(256), 0, st, part1, nblk, extra, out);
    MVF_LAUNCH_CHECK();
    if (dtype == MVF_F32)
        hipLaunchKernelGGL(align_moments2_kernel<float>, dim3(nblk), dim3(256), 0, st, coordsA, (const float*)VnA4, K_NA, PXB, na,
                           rt, out, part2);
    else
        hipLaunchKernelGGL(align_moments2_kernel<double>, dim3(nblk), dim3(256), 0, st, coordsA, (const double*)VnA4, K_NA, PXB, na,
                           rt, out, part2);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(align_finish2_kernel, dim3(1), dim3(256), 0, st, part2, nblk, out);
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" int mvf_align_transform(const double* coordsA, const void* VnA4, const double* PXB, const double* K_NA, int64_t na,
                                   const double* Rt_host, const double* origin, double* RnA, double* XAHat, void* xa4,
                                   double* PXB_term, void* Y4, void* Pw, mvf_dtype dtype, void* stream) {
    if (na == 0) return 0;
    MVF_REQUIRE(na > 0 && cdiv(na, 256) < ((int64_t)1 << 31), "mvf_align_transform: bad cell count");
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "mvf_align_transform: bad dtype %d", (int)dtype);
    MVF_REQUIRE(coordsA && Rt_host, "mvf_align_transform: null pointer");
    MVF_REQUIRE(!(PXB_term || Y4 || Pw) || (PXB && K_NA), "mvf_align_transform: PXB_term / Y4 / Pw need PXB and K_NA");
    MVF_REQUIRE(RnA || XAHat || xa4 || PXB_term || Y4 || Pw, "mvf_align_transform: no output requested");
    const Rt rt = make_rt(Rt_host, origin);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(na, 256));
    if (dtype == MVF_F32)
        hipLaunchKernelGGL(align_transform_kernel<float>, grid, dim3(256), 0, st, coordsA, (const float*)VnA4, PXB, K_NA, na, rt, RnA,
                           XAHat, (float*)xa4, PXB_term, (float*)Y4, (float*)Pw);
    else
        hipLaunchKernelGGL(align_transform_kernel<double>, grid, dim3(256), 0, st, coordsA, (const double*)VnA4, PXB, K_NA, na, rt,
                           RnA, XAHat, (double*)xa4, PXB_term, (double*)Y4, (double*)Pw);
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" int mvf_align_gather(const int32_t* perm, int64_t nb, int64_t start, int64_t bs, const void* xb4, void* xb4_out,
                                const double* coordsB, double* coordsB_out, const mvf_assign_layer* layers, int nlayers,
                                void* const* Yp_out, double* const* b_out, mvf_dtype dtype, void* stream) {
    if (bs == 0) return 0;
    MVF_REQUIRE(nb > 0 && nb < ((int64_t)1 << 31), "mvf_align_gather: bad cell count");
    MVF_REQUIRE(bs > 0 && bs <= nb && start >= 0 && start < nb, "mvf_align_gather: need 0 <= start < nb and 0 <= bs <= nb");
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "mvf_align_gather: bad dtype %d", (int)dtype);
    MVF_REQUIRE(nlayers >= 0 && nlayers <= MVF_ASSIGN_MAX_LAYERS, "mvf_align_gather: 0 .. %d layers, got %d",
                MVF_ASSIGN_MAX_LAYERS, nlayers);
    MVF_REQUIRE(perm && xb4 && xb4_out && coordsB && coordsB_out && (nlayers == 0 || (layers && Yp_out && b_out)),
                "mvf_align_gather: null pointer");
    const int64_t dsize = dtype == MVF_F32 ? 4 : 8;
    GatherArgs ga;
    ga.nlayers = nlayers, ga.x4_chunks = (int)(4 * dsize / 16);
    int64_t most = bs;
    for (int l = 0; l < MVF_ASSIGN_MAX_LAYERS; ++l) {
        ga.ysrc[l] = nullptr, ga.ydst[l] = nullptr, ga.bsrc[l] = nullptr, ga.bdst[l] = nullptr, ga.chunks[l] = 0;
        if (l >= nlayers) continue;
        if (layers[l].metric == MVF_ASSIGN_LABEL) {  // the B labels travel in b; the table has no rows per cell: nothing else to gather
            MVF_REQUIRE(layers[l].b && b_out[l], "mvf_align_gather: layer %d: null pointer", l);
            MVF_REQUIRE(layers[l].ld >= 1, "mvf_align_gather: layer %d: a label layer's ld is the table's row length L >= 1", l);
            ga.bsrc[l] = layers[l].b, ga.bdst[l] = b_out[l];
            continue;
        }
        MVF_REQUIRE(layers[l].Yp && layers[l].b && Yp_out[l] && b_out[l], "mvf_align_gather: layer %d: null pointer", l);
        MVF_REQUIRE(layers[l].ld > 0 && layers[l].ld % 16 == 0, "mvf_align_gather: layer %d: ld = %lld is not a positive multiple of 16",
                    l, (long long)layers[l].ld);
        MVF_REQUIRE((((uintptr_t)layers[l].Yp | (uintptr_t)Yp_out[l]) & 15) == 0, "mvf_align_gather: layer %d: rows not 16-byte aligned", l);
        ga.ysrc[l] = (const uint4*)layers[l].Yp, ga.ydst[l] = (uint4*)Yp_out[l];
        ga.bsrc[l] = layers[l].b, ga.bdst[l] = b_out[l];
        ga.chunks[l] = layers[l].ld * dsize / 16;
        most = std::max(most, bs * ga.chunks[l]);
    }
    MVF_REQUIRE((((uintptr_t)xb4 | (uintptr_t)xb4_out) & 15) == 0, "mvf_align_gather: xb4 not 16-byte aligned");
    const unsigned gx = (unsigned)std::min<int64_t>(4096, cdiv(most, 256));
    hipLaunchKernelGGL(align_gather_kernel, dim3(gx, (unsigned)(1 + nlayers)), dim3(256), 0, (hipStream_t)stream, perm, nb, start, bs,
                       (const uint4*)xb4, (uint4*)xb4_out, coordsB, coordsB_out, ga);
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" int mvf_align_alpha_svi(const double* kappa, const double* K_NA_spatial, const double* SigmaDiag, int64_t na,
                                   double Sp_spatial, double sigma2, double step, double* alpha, double* model_mul, void* stream) {
    if (na == 0) return 0;
    MVF_REQUIRE(na > 0 && cdiv(na, 256) < ((int64_t)1 << 31), "mvf_align_alpha_svi: bad cell count");
    MVF_REQUIRE(sigma2 > 0.0 && Sp_spatial >= 0.0, "mvf_align_alpha_svi: need sigma2 > 0 and Sp_spatial >= 0");
    MVF_REQUIRE(step > 0.0 && step <= 1.0, "mvf_align_alpha_svi: need 0 < step <= 1");
    MVF_REQUIRE(kappa && K_NA_spatial && SigmaDiag && alpha && model_mul, "mvf_align_alpha_svi: null pointer");
    hipLaunchKernelGGL(align_alpha_svi_kernel, dim3((unsigned)cdiv(na, 256)), dim3(256), 0, (hipStream_t)stream, kappa, K_NA_spatial,
                       SigmaDiag, na, Sp_spatial, sigma2, step, alpha, model_mul);
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" int mvf_align_transform_svi(const double* RnA, const double* PXB, const double* K_NA, int64_t na, const double* origin,
                                       double step, double* PXB_term, void* Y4, void* Pw, mvf_dtype dtype, void* stream) {
    if (na == 0) return 0;
    MVF_REQUIRE(na > 0 && cdiv(na, 256) < ((int64_t)1 << 31), "mvf_align_transform_svi: bad cell count");
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "mvf_align_transform_svi: bad dtype %d", (int)dtype);
    MVF_REQUIRE(step > 0.0 && step <= 1.0, "mvf_align_transform_svi: need 0 < step <= 1");
    MVF_REQUIRE(RnA && PXB && K_NA && PXB_term && Y4 && Pw, "mvf_align_transform_svi: null pointer");
    Org org;
    for (int i = 0; i < 3; ++i) org.o[i] = origin ? origin[i] : 0.0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(na, 256));
    if (dtype == MVF_F32)
        hipLaunchKernelGGL(align_transform_svi_kernel<float>, grid, dim3(256), 0, st, RnA, PXB, K_NA, na, org, step, PXB_term,
                           (float*)Y4, (float*)Pw);
    else
        hipLaunchKernelGGL(align_transform_svi_kernel<double>, grid, dim3(256), 0, st, RnA, PXB, K_NA, na, org, step, PXB_term,
                           (double*)Y4, (double*)Pw);
    MVF_LAUNCH_CHECK();
    return 0;
}
