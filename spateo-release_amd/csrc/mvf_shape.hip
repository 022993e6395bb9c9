// Shape of the cloud: mvf_shape_descriptors, the per-subspace descriptors of `model_eigenvector`
// (spateo/tdr/morphometrics/shape_similarity.py:164-177) - `rough_subspace` (15-56), `subspace_surface_fitting` (59-110),
// `dist_global_centroid_to_subspace` (113-120) and `cos_global_centroid_to_subspace` (123-133) - without the Python loop over
// n_subspace^3 voxels.  gfx950 only, float64 throughout: the fit is a polynomial in RAW monomials whose condition number
// sits at 1 / eps, and float32 storage of the coordinates would decide its rank.
//
//   bin       one lane per point: the candidate floor((x - min) / size) and its two neighbours are tested against the host's
//             interval tables with the reference's `lo <= x` and `x < hi`; the voxel id, or -1 when no interval holds the point
//             (an upper face of the cuboid when ceil(ptp) == ptp).  A point two intervals of an axis hold goes to the lower one
//             and is counted (n_overlap: the one deviation - the reference would count it twice).
//   group     the stable radix sort of mvf_prep.hip on the voxel id: a voxel's points in original-index order.  Segment ends,
//             then the voxels with at least two points compacted in voxel order by one workgroup.  No row order and no
//             float sum is decided by an atomic (the two counters are integer sums): two calls give equal bits.
//   fit       one workgroup per kept voxel.  The rows of A are generated from the grouped points, 64 at a time per wave, and
//             folded into the wave's p x (p + 1) triangle [R | Q^T z] by Householder reflections (the triangle's row j lives on
//             lane j); the four triangles are folded into one the same way.  A one-sided Jacobi SVD of R in one wave, singular
//             values at or below eps sigma_max dropped (gelsd's cond=None), the minimum-norm coefficients; no normal equations,
//             no column scaling or centring (neither the minimum-norm solution nor the cut-off survives them).  Then the
//             voxel's centroid and cosine, the 20 x 20 surface and its mean distance from the global centroid, every sum in an
//             order fixed by the count alone.
#include "mvf_common.h"

namespace mvf {

constexpr int SHAPE_THREADS = 256;
constexpr int SHAPE_WAVES = SHAPE_THREADS / 64;
constexpr int SHAPE_MAX_NSUB = MVF_SHAPE_MAX_NSUB;
constexpr int SHAPE_GRID = 20;                       // `np.linspace(mn, mx, 20)` (shape_similarity.py:68)
constexpr double SHAPE_EPS = 2.220446049250313e-16;  // 2^-52: lstsq's cond=None
constexpr double SHAPE_JACOBI_TOL = 8.881784197001252e-16;
constexpr int SHAPE_JACOBI_SWEEPS = 60;

struct ShapePlan {
    int64_t nvox, cap;
    size_t off_start, off_end, off_kstart, total;
};

static ShapePlan shape_plan(int64_t n, int nsub) {
    ShapePlan p;
    p.nvox = (int64_t)nsub * nsub * nsub;
    p.cap = std::min<int64_t>(p.nvox, n / 2);  // a kept voxel holds two points at least
    size_t o = align_up(sort_pairs_bytes(n), 256);
    p.off_start = o, o += align_up((size_t)p.nvox * 4, 256);
    p.off_end = o, o += align_up((size_t)p.nvox * 4, 256);
    p.off_kstart = o, o += align_up((size_t)std::max<int64_t>(p.cap, 1) * 4, 256);
    p.total = o;
    return p;
}

struct ShapeCentroid {
    double x, y, z;
};

// every lane gets the sum, and the same bits of it: lanes l and l ^ o add the same two numbers
__device__ __forceinline__ double wave_allsum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_allmin(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_allmax(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- bin ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SHAPE_THREADS) void shape_bin_kernel(const double* __restrict__ pts, int64_t n, const double* __restrict__ lo,
                                                                  const double* __restrict__ hi, int nsub, int32_t* __restrict__ point_voxel,
                                                                  unsigned long long* __restrict__ keys, long long* __restrict__ vals,
                                                                  unsigned long long* __restrict__ counts) {
    __shared__ double slo[3 * SHAPE_MAX_NSUB], shi[3 * SHAPE_MAX_NSUB];
    __shared__ unsigned int sdrop, sover;
    const int tid = threadIdx.x;
    for (int t = tid; t < 3 * nsub; t += SHAPE_THREADS) slo[t] = lo[t], shi[t] = hi[t];
    if (tid == 0) sdrop = 0, sover = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * SHAPE_THREADS + tid;
    if (i < n) {
        int id[3];
        bool over = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = pts[3 * i + a];
            const double* l = slo + a * nsub;
            const double* h = shi + a * nsub;
            const double t = floor((x - l[0]) / (h[0] - l[0]));
            const int c = (t >= 0.0) ? (t < (double)nsub ? (int)t : nsub - 1) : 0;  // (a NaN of a zero size: 0; no interval holds x then)
            int found = -1, hits = 0;
            for (int j = max(c - 1, 0); j <= min(c + 1, nsub - 1); ++j)
                if (l[j] <= x && x < h[j]) {
                    if (found < 0) found = j;
                    ++hits;
                }
            id[a] = found;
            over = over || hits > 1;
        }
        const int v = (id[0] < 0 || id[1] < 0 || id[2] < 0) ? -1 : (id[2] * nsub + id[1]) * nsub + id[0];
        point_voxel[i] = v;
        keys[i] = v < 0 ? (unsigned long long)nsub * nsub * nsub : (unsigned long long)v;  // the dropped points sort behind every voxel
        vals[i] = i;
        if (v < 0) atomicAdd(&sdrop, 1u);  // integer atomics: sums that do not depend on the order
        if (over) atomicAdd(&sover, 1u);
    }
    __syncthreads();
    if (tid == 0) {
        if (sdrop) atomicAdd(&counts[1], (unsigned long long)sdrop);
        if (sover) atomicAdd(&counts[2], (unsigned long long)sover);
    }
}

// ---- group ----------------------------------------------------------------------------------------------------------------
// seg_start[v] .. seg_end[v]: the positions of voxel v in the sorted order (both 0, as memset, for a voxel without a point)
__global__ __launch_bounds__(SHAPE_THREADS) void shape_segments_kernel(const unsigned long long* __restrict__ keys, int64_t n, int64_t nvox,
                                                                       int32_t* __restrict__ seg_start, int32_t* __restrict__ seg_end) {
    const int64_t i = (int64_t)blockIdx.x * SHAPE_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    if (k >= (unsigned long long)nvox) return;
    if (i == 0 || keys[i - 1] != k) seg_start[k] = (int32_t)i;
    if (i == n - 1 || keys[i + 1] != k) seg_end[k] = (int32_t)(i + 1);
}

// the voxels with two points or more, in voxel order: one workgroup, each thread a contiguous range of voxels (at most 2048 of
// them at nsub = 128)
__global__ __launch_bounds__(1024) void shape_compact_kernel(const int32_t* __restrict__ seg_start, const int32_t* __restrict__ seg_end,
                                                             int64_t nvox, int32_t* __restrict__ voxel, int64_t* __restrict__ count,
                                                             int32_t* __restrict__ kstart, unsigned long long* __restrict__ counts) {
    __shared__ unsigned int part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (nvox + 1023) / 1024;
    const int64_t lo = min(nvox, (int64_t)tid * per), hi = min(nvox, lo + per);
    unsigned int c = 0;
    for (int64_t v = lo; v < hi; ++v) c += (seg_end[v] - seg_start[v] >= 2) ? 1u : 0u;
    part[tid] = c;
    __syncthreads();
    if (tid == 0) {
        unsigned int run = 0;
        for (int k = 0; k < 1024; ++k) {
            const unsigned int w = part[k];
            part[k] = run;
            run += w;
        }
        counts[0] = run;
    }
    __syncthreads();
    unsigned int run = part[tid];
    for (int64_t v = lo; v < hi; ++v) {
        const int32_t s = seg_start[v], k = seg_end[v] - s;
        if (k >= 2) {
            voxel[run] = (int32_t)v;
            count[run] = k;
            kstart[run] = s;
            ++run;
        }
    }
}

// ---- fit ------------------------------------------------------------------------------------------------------------------
constexpr int shape_p(int order) { return order == 1 ? 3 : (order == 2 ? 6 : 10); }

// one row of A in the reference's column order (shape_similarity.py:81, 86, 91-101), or the same monomials of a grid point
template <int ORDER>
__device__ __forceinline__ void shape_row(double x, double y, double* a) {
    if constexpr (ORDER == 1) {
        a[0] = x, a[1] = y, a[2] = 1.0;
    } else if constexpr (ORDER == 2) {
        a[0] = 1.0, a[1] = x, a[2] = y, a[3] = x * y, a[4] = x * x, a[5] = y * y;
    } else {
        const double x2 = x * x, y2 = y * y;
        a[0] = 1.0, a[1] = x, a[2] = y, a[3] = x2, a[4] = x * y, a[5] = y2, a[6] = x2 * x, a[7] = x2 * y, a[8] = x * y2, a[9] = y2 * y;
    }
}

// Fold 64 rows [a_0 .. a_{P-1} | a_P] (one per lane; a lane without a row holds zeros) into the wave's triangle, whose row j
// is r[0 .. P] of lane j: column by column, a Householder reflection over the triangle's diagonal entry and the 64 new entries
// (the triangle's rows below j are zero in column j and stay out of it).
template <int P>
__device__ __forceinline__ void shape_qr_block(double (&a)[P + 1], double (&r)[P + 1], int lane) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const double s = wave_allsum(a[j] * a[j]);
        if (s > 0.0) {  // (the same on every lane)
            const double alpha = __shfl(r[j], j, 64);
            const double norm = sqrt(alpha * alpha + s);
            const double beta = alpha > 0.0 ? -norm : norm;
            const double v0 = alpha - beta;  // (no cancellation: beta has the other sign)
            const double vtv = v0 * v0 + s;
#pragma unroll
            for (int c = j + 1; c <= P; ++c) {
                const double dot = v0 * __shfl(r[c], j, 64) + wave_allsum(a[j] * a[c]);
                const double f = 2.0 * dot / vtv;
                if (lane == j) r[c] -= f * v0;
                a[c] -= f * a[j];
            }
            if (lane == j) r[j] = beta;
            a[j] = 0.0;
        }
    }
}

template <int ORDER>
__global__ __launch_bounds__(SHAPE_THREADS) void shape_fit_kernel(const double* __restrict__ pts, const long long* __restrict__ order_idx,
                                                                  const int32_t* __restrict__ kstart, const int64_t* __restrict__ count,
                                                                  const unsigned long long* __restrict__ counts, ShapeCentroid g,
                                                                  double* __restrict__ cosine, double* __restrict__ dist,
                                                                  int32_t* __restrict__ rank, double* __restrict__ sv) {
    constexpr int P = shape_p(ORDER);
    __shared__ double sR[SHAPE_WAVES][P][P + 1];
    __shared__ double sred[SHAPE_WAVES][8];
    __shared__ double scoef[P];
    __shared__ double sinfo[3];
    const int b = blockIdx.x;
    if ((unsigned long long)b >= counts[0]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t start = kstart[b];
    const int64_t k = count[b];
    const int64_t nblocks = (k + 63) / 64;

    double r[P + 1];
#pragma unroll
    for (int c = 0; c <= P; ++c) r[c] = 0.0;
    double sx = 0.0, sy = 0.0, sz = 0.0, xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (int64_t blk = wave; blk < nblocks; blk += SHAPE_WAVES) {
        const int64_t row = blk * 64 + lane;
        double a[P + 1];
#pragma unroll
        for (int c = 0; c <= P; ++c) a[c] = 0.0;
        if (row < k) {
            const int64_t i = order_idx[start + row];
            const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
            shape_row<ORDER>(x, y, a);
            a[P] = z;
            sx += x, sy += y, sz += z;
            xmin = fmin(xmin, x), xmax = fmax(xmax, x), ymin = fmin(ymin, y), ymax = fmax(ymax, y);
        }
        shape_qr_block<P>(a, r, lane);
    }
    sx = wave_allsum(sx), sy = wave_allsum(sy), sz = wave_allsum(sz);
    xmin = wave_allmin(xmin), xmax = wave_allmax(xmax), ymin = wave_allmin(ymin), ymax = wave_allmax(ymax);
    if (lane == 0) {
        sred[wave][0] = sx, sred[wave][1] = sy, sred[wave][2] = sz;
        sred[wave][3] = xmin, sred[wave][4] = xmax, sred[wave][5] = ymin, sred[wave][6] = ymax;
    }
    if (lane < P) {
#pragma unroll
        for (int c = 0; c <= P; ++c) sR[wave][lane][c] = r[c];
    }
    __syncthreads();

    if (wave == 0) {
        // the other waves' triangles as one more block of (SHAPE_WAVES - 1) P <= 30 rows
        double a[P + 1];
#pragma unroll
        for (int c = 0; c <= P; ++c) a[c] = 0.0;
        if (lane < (SHAPE_WAVES - 1) * P) {
#pragma unroll
            for (int c = 0; c <= P; ++c) a[c] = sR[1 + lane / P][lane % P][c];
        }
        shape_qr_block<P>(a, r, lane);

        // one-sided Jacobi on the columns of R: lane i < P holds row i of G = R V and of V
        double G[P], V[P];
#pragma unroll
        for (int c = 0; c < P; ++c) G[c] = lane < P ? r[c] : 0.0, V[c] = lane == c ? 1.0 : 0.0;
        const double d = lane < P ? r[P] : 0.0;
        // A column whose norm is below eps / 64 of the triangle's is rounding of the others - far under the cut-off, dropped
        // whatever its direction - and is left alone: rotating such columns against each other never settles.
        double frob2 = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) frob2 += G[c] * G[c];
        const double tiny = (SHAPE_EPS / 64.0) * (SHAPE_EPS / 64.0) * wave_allsum(frob2);
        for (int sweep = 0; sweep < SHAPE_JACOBI_SWEEPS; ++sweep) {
            bool rotated = false;
#pragma unroll
            for (int i = 0; i < P - 1; ++i) {
#pragma unroll
                for (int j = i + 1; j < P; ++j) {
                    const double aa = wave_allsum(G[i] * G[i]), bb = wave_allsum(G[j] * G[j]), cc = wave_allsum(G[i] * G[j]);
                    if (fmin(aa, bb) > tiny && fabs(cc) > SHAPE_JACOBI_TOL * (sqrt(aa) * sqrt(bb))) {  // (the same on every lane)
                        const double zeta = (bb - aa) / (2.0 * cc);
                        const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                        const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                        const double gi = G[i], gj = G[j], vi = V[i], vj = V[j];
                        G[i] = cs * gi - sn * gj, G[j] = sn * gi + cs * gj;
                        V[i] = cs * vi - sn * vj, V[j] = sn * vi + cs * vj;
                        rotated = true;
                    }
                }
            }
            if (!rotated) break;
        }
        double s2[P], s2max = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            s2[c] = wave_allsum(G[c] * G[c]);
            s2max = fmax(s2max, s2[c]);
        }
        const double smax = sqrt(s2max);
        double coef = 0.0, smin = smax;
        int rk = 0;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const double w = wave_allsum(G[c] * d);
            const double s = sqrt(s2[c]);
            if (s > SHAPE_EPS * smax) {  // gelsd: singular values <= rcond sigma_max count as zero
                coef += V[c] * (w / s2[c]);
                smin = fmin(smin, s);
                ++rk;
            }
        }
        if (lane < P) scoef[lane] = coef;
        if (lane == 0) sinfo[0] = (double)rk, sinfo[1] = smax, sinfo[2] = smax > 0.0 ? smin / smax : 0.0;
    }
    __syncthreads();

    // the voxel's extent and centroid (waves in order), its surface and the mean distance
    double tx = sred[0][0], ty = sred[0][1], tz = sred[0][2], x0 = sred[0][3], x1 = sred[0][4], y0 = sred[0][5], y1 = sred[0][6];
#pragma unroll
    for (int w = 1; w < SHAPE_WAVES; ++w) {
        tx += sred[w][0], ty += sred[w][1], tz += sred[w][2];
        x0 = fmin(x0, sred[w][3]), x1 = fmax(x1, sred[w][4]), y0 = fmin(y0, sred[w][5]), y1 = fmax(y1, sred[w][6]);
    }
    const double stepx = (x1 - x0) / (double)(SHAPE_GRID - 1), stepy = (y1 - y0) / (double)(SHAPE_GRID - 1);
    double coefs[P];
#pragma unroll
    for (int c = 0; c < P; ++c) coefs[c] = scoef[c];
    double acc = 0.0;
    for (int q = tid; q < SHAPE_GRID * SHAPE_GRID; q += SHAPE_THREADS) {
        const int iy = q / SHAPE_GRID, ix = q - iy * SHAPE_GRID;
        // np.linspace: arange(num) * step + start, the last sample set to stop
        const double X = ix == SHAPE_GRID - 1 ? x1 : (double)ix * stepx + x0;
        const double Y = iy == SHAPE_GRID - 1 ? y1 : (double)iy * stepy + y0;
        double m[P];
        shape_row<ORDER>(X, Y, m);
        double Z;
        if constexpr (ORDER == 1) {
            Z = coefs[0] * X + coefs[1] * Y + coefs[2];
        } else {
            Z = coefs[0] * m[0];
#pragma unroll
            for (int c = 1; c < P; ++c) Z += coefs[c] * m[c];
        }
        const double dx = X - g.x, dy = Y - g.y, dz = Z - g.z;
        acc += sqrt(dx * dx + dy * dy + dz * dz);
    }
    acc = wave_allsum(acc);
    __syncthreads();
    if (lane == 0) sred[wave][7] = acc;
    __syncthreads();
    if (tid == 0) {
        double total = sred[0][7];
#pragma unroll
        for (int w = 1; w < SHAPE_WAVES; ++w) total += sred[w][7];
        const double kk = (double)k;
        const double cx = tx / kk - g.x, cy = ty / kk - g.y, cz = tz / kk - g.z;
        cosine[b] = fabs(cz / sqrt(cx * cx + cy * cy + cz * cz));
        dist[b] = total / (double)(SHAPE_GRID * SHAPE_GRID);
        rank[b] = (int32_t)sinfo[0];
        sv[2 * (int64_t)b] = sinfo[1];
        sv[2 * (int64_t)b + 1] = sinfo[2];
    }
}

}  // namespace mvf

using namespace mvf;

extern "C" size_t mvf_shape_descriptors_workspace_bytes(int64_t n, int nsub) {
    if (n < 1 || n >= ((int64_t)1 << 31) || nsub < 1 || nsub > SHAPE_MAX_NSUB) return 0;
    return shape_plan(n, nsub).total;
}

extern "C" int mvf_shape_descriptors(const double* pts, int64_t n, const double* lo, const double* hi, int nsub, int order,
                                     const double* centroid, int32_t* point_voxel, int32_t* voxel, int64_t* count, double* cosine,
                                     double* dist, int32_t* rank, double* sv, int64_t* counts, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    MVF_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "mvf_shape_descriptors: bad shape (n=%lld; need 1 <= n < 2^31)", (long long)n);
    MVF_REQUIRE(nsub >= 1 && nsub <= SHAPE_MAX_NSUB, "mvf_shape_descriptors: bad shape (nsub=%d; need 1 <= nsub <= %d)", nsub,
                SHAPE_MAX_NSUB);
    MVF_REQUIRE(order >= 1 && order <= 3, "mvf_shape_descriptors: bad order %d (1 linear, 2 quadratic, 3 cubic)", order);
    MVF_REQUIRE(pts && lo && hi && centroid && point_voxel && counts, "mvf_shape_descriptors: null pointer");
    const ShapePlan p = shape_plan(n, nsub);
    MVF_REQUIRE(p.cap == 0 || (voxel && count && cosine && dist && rank && sv), "mvf_shape_descriptors: null pointer (outputs)");
    MVF_REQUIRE(workspace, "mvf_shape_descriptors: null pointer (workspace)");
    MVF_REQUIRE(((uintptr_t)workspace & 255) == 0, "mvf_shape_descriptors: the workspace must be 256-byte aligned");
    MVF_REQUIRE(workspace_bytes >= p.total, "mvf_shape_descriptors: workspace too small (%zu < %zu)", workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int32_t* seg_start = (int32_t*)(ws + p.off_start);
    int32_t* seg_end = (int32_t*)(ws + p.off_end);
    int32_t* kstart = (int32_t*)(ws + p.off_kstart);
    unsigned long long* cnt = (unsigned long long*)counts;
    unsigned long long* keys;
    long long* vals;
    sort_pairs_input(ws, n, &keys, &vals);
    MVF_CHECK_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), st));
    MVF_CHECK_HIP(hipMemsetAsync(seg_start, 0, p.off_kstart - p.off_start, st));
    const dim3 grid((unsigned)cdiv(n, SHAPE_THREADS)), block(SHAPE_THREADS);
    hipLaunchKernelGGL(shape_bin_kernel, grid, block, 0, st, pts, n, lo, hi, nsub, point_voxel, keys, vals, cnt);
    int bits = 8;
    while (bits < 64 && ((unsigned long long)p.nvox >> bits) != 0) bits += 8;  // the largest key is nvox itself
    sort_pairs(st, ws, n, bits, &keys, &vals);
    hipLaunchKernelGGL(shape_segments_kernel, grid, block, 0, st, keys, n, p.nvox, seg_start, seg_end);
    hipLaunchKernelGGL(shape_compact_kernel, dim3(1), dim3(1024), 0, st, seg_start, seg_end, p.nvox, voxel, count, kstart, cnt);
    if (p.cap > 0) {
        ShapeCentroid g{centroid[0], centroid[1], centroid[2]};
        const dim3 fit((unsigned)p.cap);  // the kept voxels are at most this many; a workgroup past their number returns at once
        if (order == 1)
            hipLaunchKernelGGL(shape_fit_kernel<1>, fit, block, 0, st, pts, vals, kstart, count, cnt, g, cosine, dist, rank, sv);
        else if (order == 2)
            hipLaunchKernelGGL(shape_fit_kernel<2>, fit, block, 0, st, pts, vals, kstart, count, cnt, g, cosine, dist, rank, sv);
        else
            hipLaunchKernelGGL(shape_fit_kernel<3>, fit, block, 0, st, pts, vals, kstart, count, cnt, g, cosine, dist, rank, sv);
    }
    MVF_LAUNCH_CHECK();
    return 0;
}
