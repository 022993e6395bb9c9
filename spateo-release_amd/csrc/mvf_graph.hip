// A kernel along the tissue: the exact k nearest neighbours of every point (mvf_knn) and shortest-path distances through a
// weighted graph from many sources at once (mvf_graph_sssp).  gfx950 only, float64 throughout whatever the cell dtype.
//
// Reference: `construct_knn_graph` and `con_K_graph` (spateo/alignment/methods/utils.py:1161-1217), the `kernel_type="geodist"`
// branch of `Morpho_pairwise._construct_kernel` (spateo/alignment/methods/morpho_class.py:865-871): sklearn's
// `kneighbors_graph(points, knn, mode="distance", include_self=False)` densified to N x N and walked in a Python double loop,
// then one networkx Dijkstra per inducing variable.
//
//   knn    a uniform grid, not all pairs.  The bounding box on the device (two launches); the cell edge from the box's volume over
//          the axes the cloud extends along, h = (V k / n)^(1/d'), so that a cell holds about k points where the cloud fills its
//          box - a thin slab included, whose short axis gets one or two cells -, doubled until the grid has at most `cap` cells
//          (what the offsets in the workspace hold); the points ordered by cell with the stable radix sort of mvf_prep.hip,
//          the cell offsets, the coordinates gathered in that order.  One query per lane -
//          a wave holds queries of neighbouring cells - walks the cells in growing Chebyshev rings around its own; a ring is
//          one contiguous run of sorted points per grid row (its two end cells where the row is inside the ring).  The lane's
//          k-list, ascending by (distance, index), sits in LDS as list[j * 64 + lane].  After ring r a lane stops when its list
//          is full and its k-th distance is below the distance from the query to the nearest face of the cells not yet visited,
//          less a margin for the rounding of the cell index; with every cell visited there is no such face.  A cloud in one
//          cell (a zero extent, n < 2 k) is the all-pairs sweep: exact, merely slow.
//          The distance is sklearn's KD-tree's: explicit differences, squares added in axis order, then sqrt; the library is
//          built with -ffp-contract=off, so no multiply-add is fused.  A point is left out of its own list by index: a
//          duplicate of it is a neighbour at distance 0.  Ties go to the smaller index.
//   sssp   Bellman-Ford sweeps over dist (n x ld, one row per node: lanes of a wave hold consecutive sources of one node and
//          load a neighbour's row coalesced).  Entry (v, s) has one writer, which pulls min(d[v], d[u] + w) over the edges of
//          v in place: every stored value is the left-to-right sum along a real path, and at the fixed point d[v] <= d[u] + w
//          holds on every edge, so the fixed point is the minimum over all paths of that sum - unique whatever the order of the
//          relaxations, and what Dijkstra returns.  Each sweep adds the number of entries it lowered to the status block
//          (an integer sum); a sweep that finds the sweep before it at zero returns at once.  Values short of the fixed point
//          depend on the scheduling; the fixed point does not.
#include "mvf_common.h"

namespace mvf {

constexpr int KNN_MAX_K = MVF_KNN_MAX_K;
constexpr int KNN_LANES = 64;            // queries per workgroup: one wave, its lists in LDS
constexpr int KNN_RED_BLOCKS = 1024;     // partial bounding boxes
constexpr int64_t KNN_MAX_CELLS = (int64_t)1 << 24;

struct KnnGrid {  // written by the device (knn_grid_kernel), 256 bytes of the workspace
    double lo[3];
    double h;       // cell edge
    double margin;  // what the rounding of a cell index can move a face by
    int g[3];       // cells per axis (1 along an axis the data does not have)
    int ncells;     // g[0] g[1] g[2] <= cap
};

struct KnnPlan {
    int64_t cap;  // the most cells the grid may have: the cell offsets hold cap + 1 entries
    size_t off_part, off_grid, off_xs, off_ord, off_offs, total;
};

static KnnPlan knn_plan(int64_t n, int d, int k) {
    KnnPlan p;
    // about n / k cells where the cloud fills its box; floor(e / h) + 1 cells per axis round that up by a factor below 2 an axis
    p.cap = std::min<int64_t>(KNN_MAX_CELLS, 8 * (n / k) + 8);
    size_t o = align_up(sort_pairs_bytes(n), 256);
    p.off_part = o, o += align_up((size_t)KNN_RED_BLOCKS * 6 * 8, 256);
    p.off_grid = o, o += 256;
    p.off_xs = o, o += align_up((size_t)n * 3 * 8, 256);
    p.off_ord = o, o += align_up((size_t)n * 4, 256);
    p.off_offs = o, o += align_up((size_t)(p.cap + 1) * 4, 256);
    p.total = o;
    return p;
}

// ---- bounding box ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void knn_bounds_kernel(const double* __restrict__ X, int64_t n, int d, double* __restrict__ part) {
    __shared__ double red[4];
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        for (int a = 0; a < d; ++a) {
            const double x = X[i * d + a];
            mn[a] = fmin(mn[a], x), mx[a] = fmax(mx[a], x);
        }
    for (int a = 0; a < 3; ++a) {
        const double lo = block_min<256>(mn[a], red);
        const double hi = -block_min<256>(-mx[a], red);
        if (threadIdx.x == 0) part[blockIdx.x * 6 + a] = lo, part[blockIdx.x * 6 + 3 + a] = hi;
    }
}

__global__ __launch_bounds__(256) void knn_grid_kernel(const double* __restrict__ part, int nblocks, int d, int64_t n, int k, int64_t cap,
                                                       KnnGrid* __restrict__ grid) {
    __shared__ double red[4];
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        double mn = INFINITY, mx = -INFINITY;
        for (int b = threadIdx.x; b < nblocks; b += 256) mn = fmin(mn, part[b * 6 + a]), mx = fmax(mx, part[b * 6 + 3 + a]);
        lo[a] = block_min<256>(mn, red);
        hi[a] = -block_min<256>(-mx, red);
    }
    if (threadIdx.x != 0) return;
    double emax = 0.0, vol = 1.0;
    int active = 0;  // the axes the cloud extends along
    for (int a = 0; a < d; ++a) {
        const double e = hi[a] - lo[a];
        emax = fmax(emax, e);
        if (e > 0.0) vol *= e, ++active;
    }
    const bool one_cell = !(emax > 0.0) || !isfinite(emax) || !isfinite(vol) || !(vol > 0.0) || n < 2 * (int64_t)k;
    double h = one_cell ? 1.0 : pow(vol * (double)k / (double)n, 1.0 / (double)active);
    if (!one_cell && (!(h > 0.0) || !isfinite(h))) h = emax;
    int g[3] = {1, 1, 1};
    for (int it = 0; it < 64 && !one_cell; ++it) {  // (h doubles until the grid fits: at h > emax it is one cell)
        double cells = 1.0;
        for (int a = 0; a < d; ++a) {
            const double t = floor((hi[a] - lo[a]) / h) + 1.0;
            g[a] = t < 1048576.0 ? (t >= 1.0 ? (int)t : 1) : 1048576;
            cells *= (double)g[a];
        }
        if (cells <= (double)cap) break;
        h *= 2.0;
        g[0] = g[1] = g[2] = 1;
    }
    if ((double)g[0] * (double)g[1] * (double)g[2] > (double)cap) g[0] = g[1] = g[2] = 1;  // (never: 64 doublings pass any extent)
    for (int a = 0; a < 3; ++a) {
        grid->g[a] = (a < d && !one_cell) ? g[a] : 1;
        grid->lo[a] = (a < d && isfinite(lo[a])) ? lo[a] : 0.0;
    }
    grid->ncells = grid->g[0] * grid->g[1] * grid->g[2];
    grid->h = h;
    // a cell index is floor((x - lo) / h) of two roundings: relative 2^-52 of at most emax / h cells, and the faces m * h carry one more
    grid->margin = one_cell ? 0.0 : emax * 0x1p-48;
}

// the cell of a coordinate along one axis: floor((x - lo) / h) clamped into the grid (a NaN goes to cell 0)
__device__ __forceinline__ int knn_cell(double x, double lo, double h, int g) {
    const double t = floor((x - lo) / h);
    return t >= 0.0 ? (t < (double)g ? (int)t : g - 1) : 0;
}

__global__ __launch_bounds__(256) void knn_bin_kernel(const double* __restrict__ X, int64_t n, int d, const KnnGrid* __restrict__ grid,
                                                      unsigned long long* __restrict__ keys, long long* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const KnnGrid g = *grid;
    int c[3] = {0, 0, 0};
    for (int a = 0; a < d; ++a) c[a] = knn_cell(X[i * d + a], g.lo[a], g.h, g.g[a]);
    keys[i] = (unsigned long long)(((int64_t)c[2] * g.g[1] + c[1]) * g.g[0] + c[0]);
    vals[i] = i;
}

// the sorted order as int32, the coordinates in that order (x, y, z; z = 0 in 2-D), and offs[c] = the first sorted position whose
// cell is >= c, for every c in [0, ncells]: position t writes the cells (key[t - 1], key[t]], the last one those behind its own
__global__ __launch_bounds__(256) void knn_gather_kernel(const double* __restrict__ X, int64_t n, int d, const unsigned long long* __restrict__ keys,
                                                         const long long* __restrict__ vals, const KnnGrid* __restrict__ grid, double* __restrict__ xs,
                                                         int32_t* __restrict__ ord, uint32_t* __restrict__ offs) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int64_t i = vals[t];
    ord[t] = (int32_t)i;
    xs[3 * t] = X[i * d], xs[3 * t + 1] = X[i * d + 1], xs[3 * t + 2] = d == 3 ? X[i * d + 2] : 0.0;
    const int64_t cap = grid->ncells;  // (<= the plan's cap: the offsets read are 0 .. ncells)
    const int64_t key = (int64_t)min(keys[t], (unsigned long long)(cap - 1));
    const int64_t prev = t == 0 ? -1 : (int64_t)min(keys[t - 1], (unsigned long long)(cap - 1));
    for (int64_t c = prev + 1; c <= key; ++c) offs[c] = (uint32_t)t;
    if (t == n - 1)
        for (int64_t c = key + 1; c <= cap; ++c) offs[c] = (uint32_t)n;
}

// ---- the search -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KNN_LANES) void knn_search_kernel(const double* __restrict__ xs, const int32_t* __restrict__ ord,
                                                               const uint32_t* __restrict__ offs, const KnnGrid* __restrict__ grid, int64_t n,
                                                               int k, int32_t* __restrict__ idx, double* __restrict__ dist) {
    extern __shared__ double lds[];
    double* ldist = lds;                                   // [k][64]
    int32_t* lidx = (int32_t*)(lds + (size_t)k * KNN_LANES);  // [k][64]
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * KNN_LANES + lane;
    if (t >= n) return;  // (no barrier below: a lane works on its own list)
    const KnnGrid g = *grid;
    const double qx = xs[3 * t], qy = xs[3 * t + 1], qz = xs[3 * t + 2];
    const int32_t self = ord[t];
    const int cq[3] = {knn_cell(qx, g.lo[0], g.h, g.g[0]), knn_cell(qy, g.lo[1], g.h, g.g[1]), knn_cell(qz, g.lo[2], g.h, g.g[2])};
    const double rel[3] = {qx - g.lo[0], qy - g.lo[1], qz - g.lo[2]};
    int rmax = 0;
    for (int a = 0; a < 3; ++a) rmax = max(rmax, max(cq[a], g.g[a] - 1 - cq[a]));

    int cnt = 0;
    double kth = INFINITY;  // the k-th distance once the list is full
    int32_t kth_i = 0x7fffffff;
    for (int r = 0; r <= rmax; ++r) {
        const int z0 = max(cq[2] - r, 0), z1 = min(cq[2] + r, g.g[2] - 1);
        const int y0 = max(cq[1] - r, 0), y1 = min(cq[1] + r, g.g[1] - 1);
        const int x0 = max(cq[0] - r, 0), x1 = min(cq[0] + r, g.g[0] - 1);
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const int64_t row = ((int64_t)z * g.g[1] + y) * g.g[0];
                const bool whole = (z - cq[2] == r) || (cq[2] - z == r) || (y - cq[1] == r) || (cq[1] - y == r);
                // the ring's cells of this grid row: all of [x0, x1], or the two end cells at distance r where they are in the grid
                const int nruns = whole ? 1 : 2;
                for (int run = 0; run < nruns; ++run) {
                    int xa, xb;
                    if (whole) {
                        xa = x0, xb = x1;
                    } else {
                        xa = xb = run == 0 ? cq[0] - r : cq[0] + r;
                        if (xa < 0 || xa >= g.g[0] || (run == 1 && r == 0)) continue;
                    }
                    const uint32_t p0 = offs[row + xa], p1 = offs[row + xb + 1];
                    for (uint32_t p = p0; p < p1; ++p) {
                        const int32_t j = ord[p];
                        if (j == self) continue;
                        const double dx = qx - xs[3 * (int64_t)p], dy = qy - xs[3 * (int64_t)p + 1], dz = qz - xs[3 * (int64_t)p + 2];
                        const double dd = sqrt((dx * dx + dy * dy) + dz * dz);  // (2-D: dz * dz = +0 adds nothing)
                        if (cnt == k && !(dd < kth || (dd == kth && j < kth_i))) continue;
                        // insert into the ascending list; the last entry falls off a full list
                        int pos = cnt < k ? cnt : k - 1;
                        while (pos > 0) {
                            const double pd = ldist[(pos - 1) * KNN_LANES + lane];
                            const int32_t pi = lidx[(pos - 1) * KNN_LANES + lane];
                            if (pd < dd || (pd == dd && pi < j)) break;
                            ldist[pos * KNN_LANES + lane] = pd, lidx[pos * KNN_LANES + lane] = pi;
                            --pos;
                        }
                        ldist[pos * KNN_LANES + lane] = dd, lidx[pos * KNN_LANES + lane] = j;
                        if (cnt < k) ++cnt;
                        if (cnt == k) kth = ldist[(k - 1) * KNN_LANES + lane], kth_i = lidx[(k - 1) * KNN_LANES + lane];
                    }
                }
            }
        if (cnt == k) {
            // the nearest face of the cells outside ring r, along the axes that still have cells there
            double face = INFINITY;
            for (int a = 0; a < 3; ++a) {
                if (cq[a] - r > 0) face = fmin(face, rel[a] - (double)(cq[a] - r) * g.h);
                if (cq[a] + r < g.g[a] - 1) face = fmin(face, (double)(cq[a] + r + 1) * g.h - rel[a]);
            }
            if (kth < face - g.margin) break;
        }
    }
    // (k < n: with every cell visited the list is full)
    for (int j = 0; j < cnt; ++j) {
        idx[(int64_t)self * k + j] = lidx[j * KNN_LANES + lane];
        dist[(int64_t)self * k + j] = ldist[j * KNN_LANES + lane];
    }
}

// ---- shortest paths -------------------------------------------------------------------------------------------------------
// status: [0] entries lowered since the call began, [1] entries the sweep before lowered, [2] entries this sweep lowers
__global__ void sssp_begin_kernel(unsigned long long* __restrict__ status) {
    status[0] = 0, status[1] = 1, status[2] = 0, status[3] = 0;
}
__global__ void sssp_advance_kernel(unsigned long long* __restrict__ status) {
    status[0] += status[2], status[1] = status[2], status[2] = 0;
    status[3] += 1;  // sweeps queued since the call began (those that returned at once included)
}

__global__ __launch_bounds__(256) void sssp_init_kernel(double* __restrict__ dist, int64_t n, int64_t m, int64_t ld) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n * m) dist[(e / m) * ld + e % m] = INFINITY;
}
__global__ __launch_bounds__(256) void sssp_sources_kernel(double* __restrict__ dist, int64_t n, int64_t m, int64_t ld,
                                                           const int32_t* __restrict__ sources) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= m) return;
    const int64_t v = sources[s];
    if (v >= 0 && v < n) dist[v * ld + s] = 0.0;
}

__global__ __launch_bounds__(256) void sssp_sweep_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                         const double* __restrict__ weights, int64_t n, int64_t m, int64_t ld,
                                                         int64_t nnz, double* dist, unsigned long long* __restrict__ status) {
    __shared__ unsigned int lowered;
    if (status[1] == 0) return;  // the sweep before this one changed nothing: the fixed point (the same on every lane)
    if (threadIdx.x == 0) lowered = 0;
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n * m) {
        const int64_t v = e / m, s = e - v * m;
        const int64_t b = max(indptr[v], (int64_t)0), t = min(indptr[v + 1], nnz);
        const double old = dist[v * ld + s];
        double best = old;
        for (int64_t q = b; q < t; ++q) {
            const int64_t u = indices[q];
            if (u < 0 || u >= n) continue;
            const double c = dist[u * ld + s] + weights[q];
            best = c < best ? c : best;
        }
        if (best < old) {
            dist[v * ld + s] = best;
            atomicAdd(&lowered, 1u);  // integer atomics: a sum that does not depend on the order
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && lowered) atomicAdd(&status[2], (unsigned long long)lowered);
}

}  // namespace mvf

using namespace mvf;

extern "C" size_t mvf_knn_workspace_bytes(int64_t n, int d, int k) {
    if ((d != 2 && d != 3) || k < 1 || k > KNN_MAX_K || n <= k || n >= ((int64_t)1 << 31)) return 0;
    return knn_plan(n, d, k).total;
}

extern "C" int mvf_knn(const double* points, int64_t n, int d, int k, int32_t* idx, double* dist, void* workspace,
                       size_t workspace_bytes, void* stream) {
    MVF_REQUIRE(d == 2 || d == 3, "mvf_knn: bad shape (d=%d; need 2 or 3)", d);
    MVF_REQUIRE(k >= 1 && k <= KNN_MAX_K, "mvf_knn: bad shape (k=%d; need 1 <= k <= %d)", k, KNN_MAX_K);
    MVF_REQUIRE(n > k && n < ((int64_t)1 << 31), "mvf_knn: bad shape (n=%lld, k=%d; need k < n < 2^31)", (long long)n, k);
    MVF_REQUIRE(points && idx && dist && workspace, "mvf_knn: null pointer");
    MVF_REQUIRE(((uintptr_t)workspace & 255) == 0, "mvf_knn: the workspace must be 256-byte aligned");
    const KnnPlan p = knn_plan(n, d, k);
    MVF_REQUIRE(workspace_bytes >= p.total, "mvf_knn: workspace too small (%zu < %zu)", workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double* part = (double*)(ws + p.off_part);
    KnnGrid* grid = (KnnGrid*)(ws + p.off_grid);
    double* xs = (double*)(ws + p.off_xs);
    int32_t* ord = (int32_t*)(ws + p.off_ord);
    uint32_t* offs = (uint32_t*)(ws + p.off_offs);
    const int nred = (int)std::min<int64_t>(cdiv(n, 256), KNN_RED_BLOCKS);
    const dim3 grid_n((unsigned)cdiv(n, 256));
    unsigned long long* keys;
    long long* vals;
    sort_pairs_input(ws, n, &keys, &vals);
    hipLaunchKernelGGL(knn_bounds_kernel, dim3(nred), dim3(256), 0, st, points, n, d, part);
    hipLaunchKernelGGL(knn_grid_kernel, dim3(1), dim3(256), 0, st, part, nred, d, n, k, p.cap, grid);
    hipLaunchKernelGGL(knn_bin_kernel, grid_n, dim3(256), 0, st, points, n, d, grid, keys, vals);
    int bits = 8;
    while (bits < 64 && ((unsigned long long)p.cap >> bits) != 0) bits += 8;
    sort_pairs(st, ws, n, bits, &keys, &vals);
    hipLaunchKernelGGL(knn_gather_kernel, grid_n, dim3(256), 0, st, points, n, d, keys, vals, grid, xs, ord, offs);
    hipLaunchKernelGGL(knn_search_kernel, dim3((unsigned)cdiv(n, KNN_LANES)), dim3(KNN_LANES), (size_t)k * KNN_LANES * 12, st, xs, ord, offs, grid,
                       n, k, idx, dist);
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" int mvf_graph_sssp(const int64_t* indptr, const int32_t* indices, const double* weights, int64_t n, int64_t nnz,
                              const int32_t* sources, int64_t m, double* dist, int64_t ld, int init, int sweeps, int64_t* status,
                              void* stream) {
    MVF_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && nnz >= 0, "mvf_graph_sssp: bad shape (n=%lld nnz=%lld; need 1 <= n < 2^31)", (long long)n,
                (long long)nnz);
    MVF_REQUIRE(m >= 1 && ld >= m && m <= ((int64_t)1 << 20) && n * m <= ((int64_t)1 << 39) - 256,  // (grid.x = cdiv(n m, 256) < 2^31)
                "mvf_graph_sssp: bad shape (m=%lld ld=%lld; need 1 <= m <= ld, m <= 2^20, n m <= 2^39 - 256)",
                (long long)m, (long long)ld);
    MVF_REQUIRE(sweeps >= 0 && sweeps <= 65536, "mvf_graph_sssp: bad sweeps %d (0 .. 65536 per call)", sweeps);
    MVF_REQUIRE(indptr && sources && dist && status && (nnz == 0 || (indices && weights)), "mvf_graph_sssp: null pointer");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* stat = (unsigned long long*)status;
    const dim3 grid((unsigned)cdiv(n * m, 256));
    if (init) {
        hipLaunchKernelGGL(sssp_init_kernel, grid, dim3(256), 0, st, dist, n, m, ld);
        hipLaunchKernelGGL(sssp_sources_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, st, dist, n, m, ld, sources);
    }
    hipLaunchKernelGGL(sssp_begin_kernel, dim3(1), dim3(1), 0, st, stat);
    for (int s = 0; s < sweeps; ++s) {
        hipLaunchKernelGGL(sssp_sweep_kernel, grid, dim3(256), 0, st, indptr, indices, weights, n, m, ld, nnz, dist, stat);
        hipLaunchKernelGGL(sssp_advance_kernel, dim3(1), dim3(1), 0, st, stat);
    }
    MVF_LAUNCH_CHECK();
    return 0;
}
