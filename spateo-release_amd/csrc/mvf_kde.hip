// Density of the cloud: mvf_kde, the fused log of a weighted kernel sum per (target, group of sources) - what
// `KernelDensity(kernel, bandwidth).fit(coords).score_samples(coords)` of pc_KDE (spateo/tdr/morphometrics/morphology.py:109)
// computes, without the N x N matrix and without leaving log space where a plain sum underflows.  gfx950 only.
//
// out[i, c] = log sum_{j: group[j] == c} w_j K(|t_i - s_j| / h), unnormalised (the host adds the constants), in two passes over
// tiles of 256 sources, as mvf_assign takes its row maxima first and its sums second:
//   pass 1  shift[i, c] = the largest log term, max_j (log w_j + log K_ij): with unit weights that is log K at the NEAREST source
//           of the group (every kernel falls with the distance), with weights it is what keeps a 1e-300 next to a 1e300;
//   pass 2  sum[i, c] = sum_j exp(log w_j + log K_ij - shift[i, c]): its largest term is exactly 1, so it neither overflows nor
//           vanishes;  out = shift + log(sum), or -inf when the group has no source with w > 0 in reach.
// The two kernels with an exp in them (gaussian, exponential) take that form literally.  The four of compact support have no
// exp to underflow - K lies in (0, 1] inside the support - so their shift is the largest WEIGHT in reach (1, and no pass 1,
// without weights) and pass 2 adds (w_j / shift) K_ij in plain arithmetic.
//
// Geometry: a lane owns one target, a workgroup 256 of them (grid.x), one column (grid.z) and one split of the sources
// (grid.y: about 1024 workgroups per column, at least 4096 sources each).  A tile of 256 sources is compacted, in source
// order, to those of the column with w > 0 (ballot + popcount: the inner loop then has no branch on the group, and a source
// belongs to exactly one column, so the exp count is n x N whatever C is; what C costs is one tile load per column); every
// lane reads the same source from LDS (a broadcast) and adds its term to ONE float64 accumulator in source order.
// Columns on the VALU, not on v_mfma_f64_16x16x4_f64: a one-hot operand would spend 16 multiply-adds per pair where one add
// is needed, and the exp - some 40 float64 instructions - dominates either way.  No atomics: split partials go to the
// workspace and one lane folds them in split order, so two calls give equal bits.  Distances are explicit coordinate
// differences in float64 whatever the storage dtype, never |x|^2 + |y|^2 - 2 x.y.
#include "mvf_common.h"

namespace mvf {

constexpr int KDE_THREADS = 256;            // targets per workgroup == sources per LDS tile
constexpr int64_t KDE_MIN_CHUNK = 4096;     // sources per split at least
constexpr int64_t KDE_TARGET_WGS = 1024;    // the sources are split until the grid has about this many workgroups
constexpr int KDE_MAX_COLUMNS = MVF_KDE_MAX_COLUMNS;

// sources per split: a function of n and N alone - never of the device, and never of C, so the bits of a column do not depend
// on which other columns the call computes
static inline int64_t kde_chunk(int64_t n, int64_t N) {
    const int64_t splits = std::max<int64_t>(1, std::min(cdiv(N, KDE_MIN_CHUNK), cdiv(KDE_TARGET_WGS, cdiv(n, KDE_THREADS))));
    return cdiv(cdiv(N, splits), KDE_THREADS) * KDE_THREADS;
}
// [partials: splits x n x C][shift: n x C] float64
static inline size_t kde_ws_bytes(int64_t n, int64_t N, int C) {
    return (size_t)(cdiv(N, kde_chunk(n, N)) + 1) * (size_t)n * (size_t)C * 8;
}

struct KdeScale {
    double h;            // the compact kernels' support is sqrt(d2) < h, as sklearn tests it
    double h2;           // h * h
    double h2_up;        // h * h (1 + 2^-50): d2 above it is out of reach whatever the rounding of the root
    double inv_h;        // 1 / h
    double half_inv_h2;  // 0.5 / (h * h)
};

// log K for the two kernels of unbounded support, from the squared distance
template <int KERNEL>
__device__ __forceinline__ double kde_log_k(double d2, const KdeScale& sc) {
    if constexpr (KERNEL == MVF_KDE_GAUSSIAN)
        return -(d2 * sc.half_inv_h2);
    else
        return -(sqrt(d2) * sc.inv_h);
}

// K for the four kernels of compact support at dist < h, in sklearn's own operations and their order (dist = sqrt(d2), then
// 1 - (dist dist) / (h h) | 1 - dist / h | cos(0.5 pi dist / h)): near the edge of the support K is a difference of nearly equal
// numbers, and a reciprocal in place of the division would show in log K at 1e-13.  Few pairs are in reach; the divisions cost
// little.
template <int KERNEL>
__device__ __forceinline__ double kde_compact_k(double dist, const KdeScale& sc) {
    if constexpr (KERNEL == MVF_KDE_TOPHAT) {
        return 1.0;
    } else if constexpr (KERNEL == MVF_KDE_EPANECHNIKOV) {
        return 1.0 - (dist * dist) / sc.h2;
    } else if constexpr (KERNEL == MVF_KDE_LINEAR) {
        return 1.0 - dist / sc.h;
    } else {
        return cos(1.5707963267948966 * dist / sc.h);
    }
}

constexpr bool kde_is_compact(int kernel) { return kernel != MVF_KDE_GAUSSIAN && kernel != MVF_KDE_EXPONENTIAL; }

// One tile of sources, compacted in source order to those of column `col` with w > 0.  sv: the weight (compact kernels) or its
// log (the others).  Returns the number kept; every thread of the workgroup must call it.
template <typename T, bool LOGW>
__device__ __forceinline__ int kde_load_tile(const typename Vec4<T>::type* __restrict__ s4, const double* __restrict__ weight,
                                             const int32_t* __restrict__ group, int col, int64_t base, int64_t hi, double* sx,
                                             double* sy, double* sz, double* sv, int* wcnt) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t j = base + tid;
    bool keep = false;
    double w = 1.0;
    if (j < hi) {
        const int g = group ? group[j] : 0;
        if (weight) w = weight[j];
        keep = (g == col) && (w > 0.0);
    }
    const unsigned long long b = __ballot(keep);
    __syncthreads();  // the readers of the previous tile are done
    if (lane == 0) wcnt[wv] = __popcll(b);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int k = 0; k < KDE_THREADS / 64; ++k) {
        const int c = wcnt[k];
        if (k < wv) off += c;
        total += c;
    }
    if (keep) {
        const int pos = off + __popcll(b & ((1ull << lane) - 1ull));
        const typename Vec4<T>::type s = s4[j];
        sx[pos] = (double)s.x, sy[pos] = (double)s.y, sz[pos] = (double)s.z;
        sv[pos] = LOGW ? log(w) : w;
    }
    __syncthreads();
    return total;
}

// pass 1: part[split][i][col] = the largest log term (gaussian, exponential) or the largest weight in reach (compact kernels)
// of this split; -inf / 0 when it holds none
template <typename T, int KERNEL>
__global__ __launch_bounds__(KDE_THREADS) void kde_shift_kernel(const typename Vec4<T>::type* __restrict__ t4, int64_t n,
                                                                const typename Vec4<T>::type* __restrict__ s4, int64_t N,
                                                                const double* __restrict__ weight, const int32_t* __restrict__ group,
                                                                int C, int64_t chunk, KdeScale sc, double* __restrict__ part) {
    constexpr bool COMPACT = kde_is_compact(KERNEL);
    __shared__ double sx[KDE_THREADS], sy[KDE_THREADS], sz[KDE_THREADS], sv[KDE_THREADS];
    __shared__ int wcnt[KDE_THREADS / 64];
    const int64_t i = (int64_t)blockIdx.x * KDE_THREADS + threadIdx.x;
    const int col = blockIdx.z;
    const int64_t lo = (int64_t)blockIdx.y * chunk, hi = min(lo + chunk, N);
    double tx = 0.0, ty = 0.0, tz = 0.0;
    if (i < n) {
        const typename Vec4<T>::type t = t4[i];
        tx = (double)t.x, ty = (double)t.y, tz = (double)t.z;
    }
    double best = COMPACT ? 0.0 : -INFINITY;
    for (int64_t base = lo; base < hi; base += KDE_THREADS) {
        const int cnt = kde_load_tile<T, !COMPACT>(s4, weight, group, col, base, hi, sx, sy, sz, sv, wcnt);
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const double dx = tx - sx[j], dy = ty - sy[j], dz = tz - sz[j];
            const double d2 = dx * dx + dy * dy + dz * dz;
            if constexpr (COMPACT) {
                if (d2 <= sc.h2_up && sqrt(d2) < sc.h) best = fmax(best, sv[j]);
            } else {
                best = fmax(best, sv[j] + kde_log_k<KERNEL>(d2, sc));
            }
        }
    }
    if (i < n) part[((int64_t)blockIdx.y * n + i) * C + col] = best;
}

// shift[i][c] = max over the splits (what pass 2 reads)
__global__ __launch_bounds__(KDE_THREADS) void kde_shift_combine_kernel(const double* __restrict__ part, int64_t total, int64_t splits,
                                                                        double* __restrict__ shift) {
    const int64_t e = (int64_t)blockIdx.x * KDE_THREADS + threadIdx.x;
    if (e >= total) return;
    double m = part[e];
    for (int64_t s = 1; s < splits; ++s) m = fmax(m, part[s * total + e]);
    shift[e] = m;
}

// pass 2: part[split][i][col] = this split's sum of exp(log w + log K - shift) (gaussian, exponential) or of (w / shift) K
// (compact kernels; shift == NULL: unit weights, no scaling), in source order
template <typename T, int KERNEL>
__global__ __launch_bounds__(KDE_THREADS) void kde_sum_kernel(const typename Vec4<T>::type* __restrict__ t4, int64_t n,
                                                              const typename Vec4<T>::type* __restrict__ s4, int64_t N,
                                                              const double* __restrict__ weight, const int32_t* __restrict__ group, int C,
                                                              int64_t chunk, KdeScale sc, const double* __restrict__ shift,
                                                              double* __restrict__ part) {
    constexpr bool COMPACT = kde_is_compact(KERNEL);
    __shared__ double sx[KDE_THREADS], sy[KDE_THREADS], sz[KDE_THREADS], sv[KDE_THREADS];
    __shared__ int wcnt[KDE_THREADS / 64];
    const int64_t i = (int64_t)blockIdx.x * KDE_THREADS + threadIdx.x;
    const int col = blockIdx.z;
    const int64_t lo = (int64_t)blockIdx.y * chunk, hi = min(lo + chunk, N);
    double tx = 0.0, ty = 0.0, tz = 0.0;
    double m = COMPACT ? 1.0 : 0.0;  // the scale 1 / shift (compact kernels) or the shift itself
    if (i < n) {
        const typename Vec4<T>::type t = t4[i];
        tx = (double)t.x, ty = (double)t.y, tz = (double)t.z;
        if (shift) {
            const double s = shift[i * C + col];
            m = COMPACT ? (s > 0.0 ? 1.0 / s : 0.0) : s;
        }
    }
    double acc = 0.0;
    for (int64_t base = lo; base < hi; base += KDE_THREADS) {
        const int cnt = kde_load_tile<T, !COMPACT>(s4, weight, group, col, base, hi, sx, sy, sz, sv, wcnt);
#pragma unroll 2
        for (int j = 0; j < cnt; ++j) {
            const double dx = tx - sx[j], dy = ty - sy[j], dz = tz - sz[j];
            const double d2 = dx * dx + dy * dy + dz * dz;
            if constexpr (COMPACT) {
                if (d2 <= sc.h2_up) {
                    const double dist = sqrt(d2);
                    if (dist < sc.h) acc += (sv[j] * m) * fmax(kde_compact_k<KERNEL>(dist, sc), 0.0);
                }
            } else {
                // the same expression as pass 1 (no contraction: -ffp-contract=off), so the largest term is exp(0) and a <= 0
                const double a = (sv[j] + kde_log_k<KERNEL>(d2, sc)) - m;
                if (a > -746.0) acc += exp(a);  // below it exp gives 0: a wave whose lanes are all that far skips the exp
            }
        }
    }
    if (i < n) part[((int64_t)blockIdx.y * n + i) * C + col] = acc;
}

// out[i][c] = shift + log(sum of the splits' partials, in split order); -inf when nothing was in reach
template <bool COMPACT>
__global__ __launch_bounds__(KDE_THREADS) void kde_finish_kernel(const double* __restrict__ part, int64_t total, int64_t splits,
                                                                 const double* __restrict__ shift, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * KDE_THREADS + threadIdx.x;
    if (e >= total) return;
    double s = part[e];
    for (int64_t k = 1; k < splits; ++k) s += part[k * total + e];
    double r = -INFINITY;
    if (s > 0.0) {
        const double m = shift ? shift[e] : (COMPACT ? 1.0 : 0.0);
        r = (COMPACT ? log(m) : m) + log(s);
    }
    out[e] = r;
}

__global__ __launch_bounds__(KDE_THREADS) void kde_fill_kernel(double* __restrict__ out, int64_t total, double v) {
    const int64_t e = (int64_t)blockIdx.x * KDE_THREADS + threadIdx.x;
    if (e < total) out[e] = v;
}

template <typename T, int KERNEL>
static void kde_launch(hipStream_t st, const void* t4, int64_t n, const void* s4, int64_t N, const double* weight, const int32_t* group,
                       int C, KdeScale sc, double* out, double* ws) {
    using V = typename Vec4<T>::type;
    constexpr bool COMPACT = kde_is_compact(KERNEL);
    const int64_t chunk = kde_chunk(n, N), splits = cdiv(N, chunk), total = n * (int64_t)C;
    double* part = ws;
    double* shift = ws + splits * total;
    const dim3 grid((unsigned)cdiv(n, KDE_THREADS), (unsigned)splits, (unsigned)C), block(KDE_THREADS);
    const dim3 flat((unsigned)cdiv(total, KDE_THREADS));
    const bool pass1 = !COMPACT || weight;  // unit weights on a compact kernel: the shift is 1
    if (pass1) {
        hipLaunchKernelGGL((kde_shift_kernel<T, KERNEL>), grid, block, 0, st, (const V*)t4, n, (const V*)s4, N, weight, group, C, chunk, sc,
                           part);
        hipLaunchKernelGGL(kde_shift_combine_kernel, flat, block, 0, st, part, total, splits, shift);
    }
    hipLaunchKernelGGL((kde_sum_kernel<T, KERNEL>), grid, block, 0, st, (const V*)t4, n, (const V*)s4, N, weight, group, C, chunk, sc,
                       pass1 ? shift : nullptr, part);
    hipLaunchKernelGGL(kde_finish_kernel<COMPACT>, flat, block, 0, st, part, total, splits, pass1 ? shift : nullptr, out);
}

template <typename T>
static void kde_dispatch(int kernel, hipStream_t st, const void* t4, int64_t n, const void* s4, int64_t N, const double* weight,
                         const int32_t* group, int C, KdeScale sc, double* out, double* ws) {
    switch (kernel) {
        case MVF_KDE_GAUSSIAN: return kde_launch<T, MVF_KDE_GAUSSIAN>(st, t4, n, s4, N, weight, group, C, sc, out, ws);
        case MVF_KDE_EXPONENTIAL: return kde_launch<T, MVF_KDE_EXPONENTIAL>(st, t4, n, s4, N, weight, group, C, sc, out, ws);
        case MVF_KDE_TOPHAT: return kde_launch<T, MVF_KDE_TOPHAT>(st, t4, n, s4, N, weight, group, C, sc, out, ws);
        case MVF_KDE_EPANECHNIKOV: return kde_launch<T, MVF_KDE_EPANECHNIKOV>(st, t4, n, s4, N, weight, group, C, sc, out, ws);
        case MVF_KDE_LINEAR: return kde_launch<T, MVF_KDE_LINEAR>(st, t4, n, s4, N, weight, group, C, sc, out, ws);
        default: return kde_launch<T, MVF_KDE_COSINE>(st, t4, n, s4, N, weight, group, C, sc, out, ws);
    }
}

}  // namespace mvf

using namespace mvf;

extern "C" size_t mvf_kde_workspace_bytes(int64_t n, int64_t N, int C) {
    if (n <= 0 || N <= 0 || C <= 0 || C > KDE_MAX_COLUMNS) return 0;
    return kde_ws_bytes(n, N, C);
}

extern "C" int mvf_kde(const void* t4, int64_t n, const void* s4, int64_t N, int d, int kernel, double h, const double* weight,
                       const int32_t* group, int C, double* out, void* workspace, size_t workspace_bytes, int dtype, void* stream) {
    if (n == 0 || C == 0) return 0;
    MVF_REQUIRE(n > 0 && N >= 0 && C > 0 && C <= KDE_MAX_COLUMNS && d >= 1 && d <= 3,
                "mvf_kde: bad shape (n=%lld, N=%lld, d=%d, C=%d; d must be 1, 2 or 3, C at most %d)", (long long)n, (long long)N, d, C,
                KDE_MAX_COLUMNS);
    MVF_REQUIRE(n < ((int64_t)1 << 38) && N < ((int64_t)1 << 38), "mvf_kde: bad shape (too many rows)");
    MVF_REQUIRE(h > 0.0 && std::isfinite(h), "mvf_kde: bad shape (the bandwidth must be positive and finite, got %g)", h);
    MVF_REQUIRE(kernel >= MVF_KDE_GAUSSIAN && kernel <= MVF_KDE_COSINE, "mvf_kde: bad kernel %d", kernel);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "mvf_kde: bad dtype %d", dtype);
    MVF_REQUIRE(t4 && out && (N == 0 || s4), "mvf_kde: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = n * (int64_t)C;
    MVF_REQUIRE(cdiv(total, KDE_THREADS) < ((int64_t)1 << 31), "mvf_kde: bad shape (n x C exceeds one launch)");
    if (N == 0) {  // no source at all: every density is log 0
        hipLaunchKernelGGL(kde_fill_kernel, dim3((unsigned)cdiv(total, KDE_THREADS)), dim3(KDE_THREADS), 0, st, out, total, -INFINITY);
        MVF_LAUNCH_CHECK();
        return 0;
    }
    const size_t need = kde_ws_bytes(n, N, C);
    MVF_REQUIRE(workspace, "mvf_kde: null pointer (workspace)");
    MVF_REQUIRE(((uintptr_t)workspace & 7) == 0, "mvf_kde: the workspace must be 8-byte aligned");
    MVF_REQUIRE(workspace_bytes >= need, "mvf_kde: workspace too small (%zu < %zu)", workspace_bytes, need);
    KdeScale sc;
    sc.h = h, sc.h2 = h * h, sc.h2_up = sc.h2 * (1.0 + 8.8817841970012523e-16), sc.inv_h = 1.0 / h, sc.half_inv_h2 = 0.5 / (h * h);
    if (dtype == MVF_F32)
        kde_dispatch<float>(kernel, st, t4, n, s4, N, weight, group, C, sc, out, (double*)workspace);
    else
        kde_dispatch<double>(kernel, st, t4, n, s4, N, weight, group, C, sc, out, (double*)workspace);
    MVF_LAUNCH_CHECK();
    return 0;
}
