// Mesh correction: batched 2-D ICP between contours, and the cut of a transformed surface mesh at the slice heights that feeds it.
// Float64 throughout, whatever the package's cell dtype: the results are counts, ratios of counts and coordinates.
//
// Reference: spateo/alignment/methods/mesh_correction_utils.py - `ICP` (:404-498: a KD-tree query and an SVD per round, one
// problem at a time), `_calculate_loss` (:371-401: one mesh copy, one VTK contour filter and one ICP per slice, per candidate
// transformation), `_transform_points` (:27-85), `_extract_contours_from_mesh` (:224-238).
//   * icp_core: ONE workgroup of 256 lanes per problem.  The data contour lives in LDS (every lane reads the same point: a
//     broadcast), the model points in registers, two per lane at the cap of 512.  A round is a brute-force nearest-neighbour
//     pass - candidates in rising index and a strict `<`, so the lower index wins among equal distances -, one block sum of six
//     values (count, the two means, the distance), one of four (the 2 x 2 covariance), and the closed-form orthogonal polar
//     factor R = V U^T of the covariance's transpose: a rotation when its determinant is >= 0, the reflection otherwise (the
//     reference's loop corrects no determinant).  The workgroup waits on nothing another workgroup writes.
//   * every sum: a lane adds its own points in rising index, the 64 lanes of a wave fold by halving (lane i += lane i + 32,
//     16, .. 1), the four waves add in wave order.  No atomics, no fused multiply-add (-ffp-contract=off): two runs give the
//     same bits, and tests/_icp_cases.py restates the order.
//   * the cut: a lane per edge, 256 edges at a time in edge order; an edge crosses the plane when its ends classify differently
//     under z >= h (VTK's rule: a vertex on the plane is above it); a ballot and a four-entry scan give every crossing edge its
//     ordinal, so the contour comes out in edge-index order.  Only z is computed for an edge that does not cross.  In the loss
//     kernel the cut runs twice - the count decides which ordinals the thinning keeps, then the kept points go to LDS -, which
//     costs about 1 % of the ICP that follows and spares a global buffer of contours (profiles/mesh_correction.md).
#include <cmath>

#include "mvf_common.h"

namespace mvf {

constexpr int ICP_MAX = MVF_ICP_MAX_POINTS;
constexpr int ICP_THREADS = 256;
constexpr int ICP_WAVES = ICP_THREADS / WAVE;
constexpr int ICP_PER = ICP_MAX / ICP_THREADS;  // model points per lane at the cap
constexpr int64_t ICP_LAUNCH = 4096;            // problems per launch of icp_batch_kernel: what the record workspace holds
constexpr int64_t MESH_T_CHUNK = 4096;          // transformations per launch of mesh_loss_kernel (grid.y)
static_assert(ICP_MAX % ICP_THREADS == 0, "the cap is a whole number of points per lane");

struct IcpParams {
    int max_iter, subsample, allow_rotation;
    double error_threshold, inlier_threshold, gamma_threshold;
};

struct IcpShared {
    double2 A[ICP_MAX];  // contour 1, the data
    double2 B[ICP_MAX];  // contour 2, the model: raw in, T_contour_2 out
    double red[8][ICP_WAVES];
    int scan[ICP_WAVES];
};

// the row of a contour of n points that slot j of its thinned copy takes
__device__ __forceinline__ int64_t thin_row(int64_t j, int64_t n, int subsample) {
    return (subsample > 0 && n > subsample) ? (j * n) / subsample : j;
}
__host__ __device__ static inline int64_t thin_size(int64_t n, int subsample) { return (subsample > 0 && n > subsample) ? subsample : n; }

// v[i] summed over the workgroup, in every lane: lanes fold by halving inside a wave, the waves add in order
template <int NV>
__device__ __forceinline__ void block_sum_n(double (&v)[NV], IcpShared& sm) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) sm.red[i][w] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double t = sm.red[i][0];
#pragma unroll
        for (int k = 1; k < ICP_WAVES; ++k) t = t + sm.red[i][k];
        v[i] = t;
    }
}
template <int NV>
__device__ __forceinline__ void block_min_n(double (&v)[NV], IcpShared& sm) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[i] = fmin(v[i], __shfl_xor(v[i], o, 64));
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) sm.red[i][w] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double t = sm.red[i][0];
#pragma unroll
        for (int k = 1; k < ICP_WAVES; ++k) t = fmin(t, sm.red[i][k]);
        v[i] = t;
    }
}

// `ICP` (:436-492) on the N data points sm.A and the M model points sm.B (1 <= N, M <= ICP_MAX, raw coordinates, visible to the
// whole workgroup).  Leaves T_contour_2 in sm.B (visible after the caller's barrier); the results in every lane.  shift: the
// `translation` the reference returns without rotation (:494): the LAST round's, scale t + centre_1 - centre_2.
__device__ void icp_core(IcpShared& sm, int N, int M, const IcpParams& par, double& gamma, int& iters, int& ninl, double2& shift) {
    const int tid = threadIdx.x;
    double mn[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) mn[i] = INFINITY;
    for (int i = tid; i < N; i += ICP_THREADS) {
        const double2 a = sm.A[i];
        mn[0] = fmin(mn[0], a.x), mn[1] = fmin(mn[1], a.y), mn[2] = fmin(mn[2], -a.x), mn[3] = fmin(mn[3], -a.y);
    }
    for (int i = tid; i < M; i += ICP_THREADS) {
        const double2 b = sm.B[i];
        mn[4] = fmin(mn[4], b.x), mn[5] = fmin(mn[5], b.y), mn[6] = fmin(mn[6], -b.x), mn[7] = fmin(mn[7], -b.y);
    }
    block_min_n<8>(mn, sm);
    const double m1x = (-mn[2] + mn[0]) / 2, m1y = (-mn[3] + mn[1]) / 2;  // the mid-range: (max + min) / 2
    const double m2x = (-mn[6] + mn[4]) / 2, m2y = (-mn[7] + mn[5]) / 2;
    double ss[2] = {0.0, 0.0};
    for (int i = tid; i < N; i += ICP_THREADS) {
        double2 a = sm.A[i];
        a.x = a.x - m1x, a.y = a.y - m1y;
        sm.A[i] = a;
        ss[0] = ss[0] + (a.x * a.x + a.y * a.y);
    }
    double2 b[ICP_PER];
#pragma unroll
    for (int q = 0; q < ICP_PER; ++q) {
        const int j = tid + q * ICP_THREADS;
        b[q] = make_double2(0.0, 0.0);
        if (j < M) {
            b[q] = sm.B[j];
            b[q].x = b[q].x - m2x, b[q].y = b[q].y - m2y;
            ss[1] = ss[1] + (b[q].x * b[q].x + b[q].y * b[q].y);
        }
    }
    block_sum_n<2>(ss, sm);
    const double scale = (sqrt(ss[0] / (double)N) + sqrt(ss[1] / (double)M)) / 2;
    for (int i = tid; i < N; i += ICP_THREADS) {  // (each lane rewrites the points it demeaned)
        double2 a = sm.A[i];
        a.x = a.x / scale, a.y = a.y / scale;
        sm.A[i] = a;
    }
#pragma unroll
    for (int q = 0; q < ICP_PER; ++q) b[q].x = b[q].x / scale, b[q].y = b[q].y / scale;
    __syncthreads();

    double dist[ICP_PER], prev = INFINITY;
#pragma unroll
    for (int q = 0; q < ICP_PER; ++q) dist[q] = INFINITY;
    iters = 0, ninl = 0;
    double ltx = 0.0, lty = 0.0;  // the last round's translation: 0 when it found fewer than 3 inliers (:458)
    for (int it = 0; it < par.max_iter; ++it) {
        iters = it + 1;
        double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double2 nr[ICP_PER];
        bool inl[ICP_PER];
#pragma unroll
        for (int q = 0; q < ICP_PER; ++q) {
            const int j = tid + q * ICP_THREADS;
            inl[q] = false;
            nr[q] = make_double2(0.0, 0.0);
            if (j < M) {
                double best = INFINITY;
                int bi = 0;
#pragma unroll 4
                for (int i = 0; i < N; ++i) {
                    const double2 a = sm.A[i];
                    const double dx = b[q].x - a.x, dy = b[q].y - a.y;
                    const double d2 = dx * dx + dy * dy;
                    if (d2 < best) best = d2, bi = i;
                }
                dist[q] = sqrt(best);
                if (dist[q] < par.inlier_threshold) {
                    inl[q] = true;
                    nr[q] = sm.A[bi];
                    s[0] = s[0] + 1.0, s[1] = s[1] + b[q].x, s[2] = s[2] + b[q].y;
                    s[3] = s[3] + nr[q].x, s[4] = s[4] + nr[q].y, s[5] = s[5] + dist[q];
                }
            }
        }
        block_sum_n<6>(s, sm);
        ninl = (int)s[0];
        if (ninl < 3) {  // identity, and T_contour_2 stays (:457-460)
            ltx = 0.0, lty = 0.0;
            break;
        }
        const double cnt = s[0];
        const double bmx = s[1] / cnt, bmy = s[2] / cnt, amx = s[3] / cnt, amy = s[4] / cnt;
        double r00 = 1.0, r01 = 0.0, r10 = 0.0, r11 = 1.0, tx, ty;
        if (par.allow_rotation) {
            double h[4] = {0.0, 0.0, 0.0, 0.0};  // H = (T_corr - mean)^T (c1_corr - mean), row-major
#pragma unroll
            for (int q = 0; q < ICP_PER; ++q) {
                if (inl[q]) {
                    const double ux = b[q].x - bmx, uy = b[q].y - bmy, vx = nr[q].x - amx, vy = nr[q].y - amy;
                    h[0] = h[0] + ux * vx, h[1] = h[1] + ux * vy, h[2] = h[2] + uy * vx, h[3] = h[3] + uy * vy;
                }
            }
            block_sum_n<4>(h, sm);
            // R = V U^T of H = U S V^T: the orthogonal polar factor of H^T = [[pa, pb], [pc, pd]]
            const double pa = h[0], pb = h[2], pc = h[1], pd = h[3];
            const double det = pa * pd - pb * pc;
            if (det >= 0.0) {
                const double p = pa + pd, q2 = pc - pb, nrm = sqrt(p * p + q2 * q2);
                if (nrm > 0.0) r00 = p / nrm, r01 = -(q2 / nrm), r10 = q2 / nrm, r11 = p / nrm;
            } else {
                const double p = pa - pd, q2 = pb + pc, nrm = sqrt(p * p + q2 * q2);
                r00 = p / nrm, r01 = q2 / nrm, r10 = q2 / nrm, r11 = -(p / nrm);
            }
            tx = amx - (r00 * bmx + r01 * bmy), ty = amy - (r10 * bmx + r11 * bmy);
        } else {
            tx = amx - bmx, ty = amy - bmy;
        }
#pragma unroll
        for (int q = 0; q < ICP_PER; ++q) {
            const double x = b[q].x, y = b[q].y;
            b[q].x = (r00 * x + r01 * y) + tx, b[q].y = (r10 * x + r11 * y) + ty;
        }
        ltx = tx, lty = ty;
        const double err = s[5] / cnt;
        if (fabs(prev - err) < par.error_threshold) break;
        prev = err;
    }
    double g[1] = {0.0};
#pragma unroll
    for (int q = 0; q < ICP_PER; ++q)
        if (tid + q * ICP_THREADS < M && dist[q] < par.gamma_threshold) g[0] = g[0] + 1.0;
    block_sum_n<1>(g, sm);
    gamma = g[0] / (double)M;
    shift = make_double2((scale * ltx + m1x) - m2x, (scale * lty + m1y) - m2y);
#pragma unroll
    for (int q = 0; q < ICP_PER; ++q) {
        const int j = tid + q * ICP_THREADS;
        if (j < M) sm.B[j] = make_double2(scale * b[q].x + m1x, scale * b[q].y + m1y);  // (:492)
    }
}

__global__ __launch_bounds__(ICP_THREADS) void icp_batch_kernel(const mvf_icp_problem* __restrict__ recs, IcpParams par) {
    __shared__ IcpShared sm;
    const mvf_icp_problem pr = recs[blockIdx.x];
    const int tid = threadIdx.x;
    const int N = (int)thin_size(pr.n1, par.subsample), M = (int)thin_size(pr.n2, par.subsample);
    for (int i = tid; i < N; i += ICP_THREADS) {
        const int64_t r = thin_row(i, pr.n1, par.subsample);
        sm.A[i] = make_double2(pr.contour_1[2 * r], pr.contour_1[2 * r + 1]);
    }
    for (int i = tid; i < M; i += ICP_THREADS) {
        const int64_t r = thin_row(i, pr.n2, par.subsample);
        sm.B[i] = make_double2(pr.contour_2[2 * r], pr.contour_2[2 * r + 1]);
    }
    __syncthreads();
    double gamma;
    int iters, ninl;
    double2 shift;
    icp_core(sm, N, M, par, gamma, iters, ninl, shift);
    if (tid == 0) {
        if (pr.translation) pr.translation[0] = shift.x, pr.translation[1] = shift.y;
        pr.gamma[0] = gamma;
        pr.stats[0] = iters;
        pr.stats[1] = ninl;
    }
    if (pr.T_contour_2) {  // (every lane reads back the points it wrote itself)
        for (int j = tid; j < M; j += ICP_THREADS) {
            pr.T_contour_2[2 * j] = sm.B[j].x;
            pr.T_contour_2[2 * j + 1] = sm.B[j].y;
        }
    }
}

// ---- the mesh: `_transform_points` with the translation on z of every vertex, and the cut ----
struct MeshXf {
    double R[9], scale, tz, mean[3];
};
struct Mean3 {
    double v[3];
};
struct Par5 {
    double v[5];
};

__device__ __forceinline__ void mat3_mul(const double* a, const double* b, double* c) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[i * 3 + j] = (a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j]) + a[i * 3 + 2] * b[6 + j];
}

// par: {rx, ry, rz in degrees, z translation, scale}
__device__ __forceinline__ MeshXf mesh_xf(const double* par, const Mean3& mean) {
    const double k = 3.14159265358979323846 / 180.0;
    const double ex = par[0] * k, ey = par[1] * k, ez = par[2] * k;
    const double cx = cos(ex), sx = sin(ex), cy = cos(ey), sy = sin(ey), cz = cos(ez), sz = sin(ez);
    const double Rx[9] = {1.0, 0.0, 0.0, 0.0, cx, -sx, 0.0, sx, cx};
    const double Ry[9] = {cy, 0.0, sy, 0.0, 1.0, 0.0, -sy, 0.0, cy};
    const double Rz[9] = {cz, -sz, 0.0, sz, cz, 0.0, 0.0, 0.0, 1.0};
    double T[9];
    MeshXf xf;
    mat3_mul(Ry, Rx, T);
    mat3_mul(Rz, T, xf.R);
    xf.tz = par[3], xf.scale = par[4];
    xf.mean[0] = mean.v[0], xf.mean[1] = mean.v[1], xf.mean[2] = mean.v[2];
    return xf;
}
// coordinate c (0, 1, 2) of the transformed vertex p
__device__ __forceinline__ double xf_coord(const MeshXf& xf, const double* __restrict__ p, int c) {
    const double c0 = p[0] - xf.mean[0], c1 = p[1] - xf.mean[1], c2 = p[2] - xf.mean[2];
    const double r = (c0 * xf.R[c * 3] + c1 * xf.R[c * 3 + 1]) + c2 * xf.R[c * 3 + 2];
    const double v = xf.scale * r + xf.mean[c];
    return c == 2 ? v + xf.tz : v;
}
__device__ __forceinline__ int64_t clamp_vertex(int32_t v, int64_t V) { return v < 0 ? 0 : (v >= V ? V - 1 : (int64_t)v); }

// Every edge that crosses z = h, in edge order: sink(ordinal, a, b, za, zb).  Returns their number, in every lane.
template <typename Sink>
__device__ __forceinline__ int cut_pass(const MeshXf& xf, const double* __restrict__ verts, int64_t V, const int32_t* __restrict__ edges,
                                        int64_t E, double h, int* scan, Sink sink) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int base = 0;
    for (int64_t e0 = 0; e0 < E; e0 += ICP_THREADS) {
        const int64_t e = e0 + tid;
        bool f = false;
        int64_t a = 0, b = 0;
        double za = 0.0, zb = 0.0;
        if (e < E) {
            a = clamp_vertex(edges[2 * e], V), b = clamp_vertex(edges[2 * e + 1], V);
            za = xf_coord(xf, verts + 3 * a, 2), zb = xf_coord(xf, verts + 3 * b, 2);
            f = (za >= h) != (zb >= h);
        }
        const unsigned long long bal = __ballot(f);
        const int pre = __popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) scan[w] = __popcll(bal);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int i = 0; i < ICP_WAVES; ++i) {
            if (i < w) off += scan[i];
            tot += scan[i];
        }
        if (f) sink(off + pre, a, b, za, zb);
        base += tot;
    }
    return base;
}
// the point of edge (a, b) on the plane: linear in z, x and y only
__device__ __forceinline__ double2 cut_point(const MeshXf& xf, const double* __restrict__ verts, int64_t a, int64_t b, double za, double zb,
                                             double h) {
    const double t = (h - za) / (zb - za);
    const double xa = xf_coord(xf, verts + 3 * a, 0), ya = xf_coord(xf, verts + 3 * a, 1);
    const double xb = xf_coord(xf, verts + 3 * b, 0), yb = xf_coord(xf, verts + 3 * b, 1);
    return make_double2(xa + t * (xb - xa), ya + t * (yb - ya));
}

// grid (n_S, transformations of this chunk): gamma and the uncut contour size of every (transformation, slice)
__global__ __launch_bounds__(ICP_THREADS) void mesh_loss_kernel(const double* __restrict__ verts, int64_t V, const int32_t* __restrict__ edges,
                                                                int64_t E, Mean3 mean, const double* __restrict__ params,
                                                                const double* __restrict__ heights, const double* __restrict__ contours,
                                                                const int64_t* __restrict__ offsets, int64_t total, int64_t n_S,
                                                                IcpParams par, double* __restrict__ gam, int32_t* __restrict__ cnt) {
    __shared__ IcpShared sm;
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x, t = blockIdx.y;
    const MeshXf xf = mesh_xf(params + t * 5, mean);
    const double h = heights[s];
    const int n = cut_pass(xf, verts, V, edges, E, h, sm.scan, [](int, int64_t, int64_t, double, double) {});
    const int sub = par.subsample;
    const int M = n > sub ? sub : n;
    if (M > 0) {
        cut_pass(xf, verts, V, edges, E, h, sm.scan, [&](int k, int64_t a, int64_t b, double za, double zb) {
            int64_t slot = k;
            if (n > sub) {  // kept when k == floor(j n / sub) for a j: the only candidate is j = ceil(k sub / n)
                slot = ((int64_t)k * sub + n - 1) / n;
                if (slot >= sub || (slot * n) / sub != k) slot = -1;
            }
            if (slot >= 0) sm.B[slot] = cut_point(xf, verts, a, b, za, zb, h);
        });
    }
    int64_t lo = offsets[s], hi = offsets[s + 1];  // clamped into the packed array before they are used as addresses
    lo = lo < 0 ? 0 : (lo > total ? total : lo);
    hi = hi < lo ? lo : (hi > total ? total : hi);
    const int64_t n1 = hi - lo;
    const int N = (int)(n1 > sub ? sub : n1);
    for (int i = tid; i < N; i += ICP_THREADS) {
        const int64_t r = lo + thin_row(i, n1, sub);
        sm.A[i] = make_double2(contours[2 * r], contours[2 * r + 1]);
    }
    __syncthreads();
    double gamma = 0.0;
    int iters, ninl;
    double2 shift;
    if (M > 0 && N > 0) icp_core(sm, N, M, par, gamma, iters, ninl, shift);
    if (tid == 0) {
        gam[t * n_S + s] = gamma;
        cnt[t * n_S + s] = n;
    }
}

// `_calculate_loss` (:387-399): one lane per transformation, the slices in order
__global__ __launch_bounds__(256) void mesh_loss_sum_kernel(const double* __restrict__ gam, const int32_t* __restrict__ cnt, int64_t nt,
                                                            int64_t n_S, double* __restrict__ loss, double* __restrict__ gamma_out,
                                                            int32_t* __restrict__ count_out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    double cost = 0.0;
    bool cut = true;
    for (int64_t s = 0; s < n_S; ++s) {
        const double g = gam[t * n_S + s];
        const int32_t c = cnt[t * n_S + s];
        if (c == 0) cut = false;
        cost = cost + (1.0 - g);
        if (gamma_out) gamma_out[t * n_S + s] = g;
        if (count_out) count_out[t * n_S + s] = c;
    }
    loss[t] = (cut ? cost : 1e6) / (double)n_S;
}

// grid n_S: the contour of one transformation at every height, the first `cap` points of each
__global__ __launch_bounds__(ICP_THREADS) void mesh_contours_kernel(const double* __restrict__ verts, int64_t V, const int32_t* __restrict__ edges,
                                                                    int64_t E, Mean3 mean, Par5 par5, const double* __restrict__ heights,
                                                                    int64_t cap, double* __restrict__ points, int32_t* __restrict__ counts) {
    __shared__ int scan[ICP_WAVES];
    const int64_t s = blockIdx.x;
    const MeshXf xf = mesh_xf(par5.v, mean);
    const double h = heights[s];
    double* out = points + s * cap * 2;
    const int n = cut_pass(xf, verts, V, edges, E, h, scan, [&](int k, int64_t a, int64_t b, double za, double zb) {
        if (k < cap) {
            const double2 p = cut_point(xf, verts, a, b, za, zb, h);
            out[2 * (int64_t)k] = p.x, out[2 * (int64_t)k + 1] = p.y;
        }
    });
    if (threadIdx.x == 0) counts[s] = n;
}

static int check_icp_params(const char* who, int max_iter, double error_threshold, double inlier_threshold, double gamma_threshold) {
    MVF_REQUIRE(max_iter >= 1, "%s: max_iter must be at least 1, got %d", who, max_iter);
    MVF_REQUIRE(error_threshold == error_threshold && inlier_threshold == inlier_threshold && gamma_threshold == gamma_threshold,
                "%s: a threshold is NaN", who);
    return 0;
}

static int check_mesh(const char* who, const void* verts, int64_t V, const void* edges, int64_t E, const double* mean, int64_t n_S,
                      const void* heights) {
    MVF_REQUIRE(V >= 1 && V < ((int64_t)1 << 31), "%s: need 1 <= V < 2^31 vertices, got %lld", who, (long long)V);
    MVF_REQUIRE(E >= 1 && E < ((int64_t)1 << 31) - ICP_THREADS, "%s: need 1 <= E < 2^31 - 256 edges, got %lld", who, (long long)E);
    // (n_S is grid.x of 256-lane workgroups: the launch holds fewer than 2^32 lanes in x)
    MVF_REQUIRE(n_S >= 1 && n_S < ((int64_t)1 << 24), "%s: need 1 <= n_S < 2^24 slice heights, got %lld", who, (long long)n_S);
    MVF_REQUIRE(verts && edges && mean && heights, "%s: null pointer", who);
    MVF_REQUIRE(std::isfinite(mean[0]) && std::isfinite(mean[1]) && std::isfinite(mean[2]), "%s: the vertex mean is not finite", who);
    return 0;
}

static inline size_t mesh_loss_ws(int64_t n_T, int64_t n_S) {
    const int64_t c = std::min(n_T, MESH_T_CHUNK);
    return align_up((size_t)c * (size_t)n_S * 8, 16) + align_up((size_t)c * (size_t)n_S * 4, 16);
}

}  // namespace mvf

using namespace mvf;

extern "C" size_t mvf_icp_batch_workspace_bytes(int64_t nproblems) {
    if (nproblems <= 0) return 0;
    return (size_t)std::min(nproblems, ICP_LAUNCH) * sizeof(mvf_icp_problem);
}

extern "C" int mvf_icp_batch(const mvf_icp_problem* problems, int64_t nproblems, int max_iter, double error_threshold,
                             double inlier_threshold, double gamma_threshold, int subsample, int allow_rotation, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (nproblems == 0) return 0;
    MVF_REQUIRE(nproblems > 0 && problems, "mvf_icp_batch: %lld problems at a null pointer", (long long)nproblems);
    if (int rc = check_icp_params("mvf_icp_batch", max_iter, error_threshold, inlier_threshold, gamma_threshold)) return rc;
    MVF_REQUIRE(subsample <= ICP_MAX, "mvf_icp_batch: subsample = %d, at most %d (MVF_ICP_MAX_POINTS) are supported", subsample, ICP_MAX);
    for (int64_t i = 0; i < nproblems; ++i) {
        const mvf_icp_problem& p = problems[i];
        MVF_REQUIRE(p.n1 >= 1 && p.n2 >= 1, "mvf_icp_batch: problem %lld: both contours need at least one point", (long long)i);
        MVF_REQUIRE(p.n1 < ((int64_t)1 << 40) && p.n2 < ((int64_t)1 << 40), "mvf_icp_batch: problem %lld: too many points", (long long)i);
        MVF_REQUIRE(thin_size(p.n1, subsample) <= ICP_MAX && thin_size(p.n2, subsample) <= ICP_MAX,
                    "mvf_icp_batch: problem %lld: %lld and %lld points with subsample = %d, at most %d (MVF_ICP_MAX_POINTS) fit",
                    (long long)i, (long long)p.n1, (long long)p.n2, subsample, ICP_MAX);
        MVF_REQUIRE(p.contour_1 && p.contour_2 && p.gamma && p.stats, "mvf_icp_batch: problem %lld: null pointer", (long long)i);
    }
    const size_t need = mvf_icp_batch_workspace_bytes(nproblems);
    MVF_REQUIRE(workspace, "mvf_icp_batch: null workspace");
    MVF_REQUIRE(((uintptr_t)workspace & 7) == 0, "mvf_icp_batch: the workspace must be 8-byte aligned");
    MVF_REQUIRE(workspace_bytes >= need, "mvf_icp_batch: workspace too small (%zu < %zu)", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const IcpParams par{max_iter, subsample, allow_rotation != 0, error_threshold, inlier_threshold, gamma_threshold};
    for (int64_t lo = 0; lo < nproblems; lo += ICP_LAUNCH) {
        const int64_t nb = std::min(ICP_LAUNCH, nproblems - lo);
        MVF_CHECK_HIP(hipMemcpyAsync(workspace, problems + lo, (size_t)nb * sizeof(mvf_icp_problem), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(icp_batch_kernel, dim3((unsigned)nb), dim3(ICP_THREADS), 0, st, (const mvf_icp_problem*)workspace, par);
        MVF_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" size_t mvf_mesh_loss_workspace_bytes(int64_t n_T, int64_t n_S) {
    if (n_T <= 0 || n_S <= 0) return 0;
    return mesh_loss_ws(n_T, n_S);
}

extern "C" int mvf_mesh_loss(const double* verts, int64_t V, const int32_t* edges, int64_t E, const double* mean, const double* params,
                             int64_t n_T, const double* heights, const double* contours, const int64_t* offsets, int64_t contour_total,
                             int64_t n_S, int max_iter, double error_threshold, double inlier_threshold, double gamma_threshold,
                             int subsample, double* loss, double* gamma, int32_t* count, void* workspace, size_t workspace_bytes,
                             void* stream) {
    if (n_T == 0) return 0;
    MVF_REQUIRE(n_T > 0, "mvf_mesh_loss: n_T must not be negative, got %lld", (long long)n_T);
    if (int rc = check_mesh("mvf_mesh_loss", verts, V, edges, E, mean, n_S, heights)) return rc;
    if (int rc = check_icp_params("mvf_mesh_loss", max_iter, error_threshold, inlier_threshold, gamma_threshold)) return rc;
    MVF_REQUIRE(subsample >= 1 && subsample <= ICP_MAX, "mvf_mesh_loss: subsample must be 1 .. %d (MVF_ICP_MAX_POINTS), got %d", ICP_MAX,
                subsample);
    MVF_REQUIRE(contour_total >= 1, "mvf_mesh_loss: the packed contours are empty");
    MVF_REQUIRE(params && contours && offsets && loss, "mvf_mesh_loss: null pointer");
    const size_t need = mesh_loss_ws(n_T, n_S);
    MVF_REQUIRE(workspace, "mvf_mesh_loss: null workspace");
    MVF_REQUIRE(((uintptr_t)workspace & 15) == 0, "mvf_mesh_loss: the workspace must be 16-byte aligned");
    MVF_REQUIRE(workspace_bytes >= need, "mvf_mesh_loss: workspace too small (%zu < %zu)", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const IcpParams par{max_iter, subsample, 1, error_threshold, inlier_threshold, gamma_threshold};
    const Mean3 m3{{mean[0], mean[1], mean[2]}};
    const int64_t chunk = std::min(n_T, MESH_T_CHUNK);
    double* gws = (double*)workspace;
    int32_t* cws = (int32_t*)((char*)workspace + align_up((size_t)chunk * (size_t)n_S * 8, 16));
    for (int64_t t0 = 0; t0 < n_T; t0 += chunk) {
        const int64_t nt = std::min(chunk, n_T - t0);
        hipLaunchKernelGGL(mesh_loss_kernel, dim3((unsigned)n_S, (unsigned)nt), dim3(ICP_THREADS), 0, st, verts, V, edges, E, m3,
                           params + t0 * 5, heights, contours, offsets, contour_total, n_S, par, gws, cws);
        MVF_LAUNCH_CHECK();
        hipLaunchKernelGGL(mesh_loss_sum_kernel, dim3((unsigned)cdiv(nt, 256)), dim3(256), 0, st, (const double*)gws, (const int32_t*)cws,
                           nt, n_S, loss + t0, gamma ? gamma + t0 * n_S : nullptr, count ? count + t0 * n_S : nullptr);
        MVF_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int mvf_mesh_contours(const double* verts, int64_t V, const int32_t* edges, int64_t E, const double* mean, const double* param,
                                 const double* heights, int64_t n_S, int64_t capacity, double* points, int32_t* counts, void* stream) {
    if (int rc = check_mesh("mvf_mesh_contours", verts, V, edges, E, mean, n_S, heights)) return rc;
    MVF_REQUIRE(param && counts, "mvf_mesh_contours: null pointer");
    MVF_REQUIRE(capacity >= 0 && capacity < ((int64_t)1 << 31), "mvf_mesh_contours: capacity must be 0 .. 2^31 - 1, got %lld",
                (long long)capacity);
    MVF_REQUIRE(capacity == 0 || points, "mvf_mesh_contours: null points with a capacity of %lld", (long long)capacity);
    for (int i = 0; i < 5; ++i) MVF_REQUIRE(std::isfinite(param[i]), "mvf_mesh_contours: parameter %d is not finite", i);
    const Mean3 m3{{mean[0], mean[1], mean[2]}};
    Par5 p5;
    for (int i = 0; i < 5; ++i) p5.v[i] = param[i];
    hipLaunchKernelGGL(mesh_contours_kernel, dim3((unsigned)n_S), dim3(ICP_THREADS), 0, (hipStream_t)stream, verts, V, edges, E, m3, p5,
                       heights, capacity, points, counts);
    MVF_LAUNCH_CHECK();
    return 0;
}
