// The assignment step of Spateo's alignment, fused: every weight the other updates consume (K_NA, K_NB, K_NA_spatial,
// K_NA_sigma2, sum P_sigma2 d, P @ coordsB) without the NA x NB matrix P.
//
// Reference: `Morpho_pairwise._update_assignment_P` (spateo/alignment/methods/morpho_class.py:1071-1200) = `calc_distance`
// (methods/utils.py:647-788, 866-941) + `get_P_core` (:993-1096), which materialise P and three more NA x NB matrices.
//
// Every supported layer metric is d_ij = a_i + b_j - s <X'_i, Y'_j> (optionally clamped at 0 / square-rooted):
//   euc     X' = x, Y' = y, a = |x|^2, b = |y|^2, s = 2, clamped (the reference's "euc" IS the squared distance)
//   kl      X' = p, Y' = log(q + 1e-8), a = sum p log(p + 1e-8), b = 0, s = 1        (p, q: x + 0.01, row-normalised)
//   sym_kl  X' = [p, log p'], Y' = [log q', q], a = sum p log p' / 2, b = sum q log q' / 2, s = 1/2   (2 G features)
//   cos     X' = x / max(|x|, 1e-8), Y' likewise, a = 1/2, b = 0, s = 1/2
// The one metric that is no product of features is "label" (`_label_distance_backend`, utils.py:791-832): d_ij = T[la_i][lb_j],
// a look-up in the K x L label-transfer table (float64 whatever the cell dtype) with the cells' labels travelling as
// integers held in a / b.  layer_product takes that branch per layer (label_distances): 8 row labels, 2 column labels and 16
// table reads per lane and 32 x 32 block, through the cache (the table is a few hundred bytes and every wave reads it; no LDS
// is spent on it, of which assign_pass1_topk_kernel<., 64> has none to spare).  No clamp, no square root; the probability is
// formed by the code that forms it for every other layer.
// mvf_assign_prepare builds X' / Y' (cell dtype, rows zero-padded to a multiple of 16 features) and a / b (float64) in O(N G);
// the pairwise part is one tile routine: the layer dot products as v_mfma_f64_16x16x4_f64 (operands widened from the cell
// dtype, float64 accumulation), the spatial distance from the coordinates and all exponent arithmetic in float64 on VALU.
//
// Two passes over the tiles, flash-attention style (the column normalisers must be known before a row sum can be formed):
//   pass 1  per B column j, over the A rows i:  S0 = sum e1, S1 = sum e1 m_i, S2 = sum e2 m_i, S3 = sum e2 m_i q_ij
//           (e1 = exp(-d sigma2_variance / 2 sigma2), e2 = exp(-d / 2 sigma2), q = product of the layer probabilities)
//   factors in_j = 1 - o / (o + S0), c1 = 1 / (o + S1), c2 = in_j / (S2 + 1e-8), c3 = in_j / (S3 + 1e-8), K_NB_j = c3 S3
//   pass 2  per A row i, over the B columns j:  K_NA_spatial = m_i sum e1 c1, K_NA_sigma2 = m_i sum e2 c2,
//           K_NA = m_i sum e2 q c3, PXB = m_i sum e2 q c3 y_j, and sum_ij m_i e2 c2 d
// No max-subtraction before exp, as in the reference: a column whose terms all underflow has S = 0, in_j = 0 and gives
// exactly 0 everywhere.  A workgroup is 4 waves on a 64 x 64 tile (each wave 32 x 32: 2 x 2 MFMA blocks); the rows (pass 1) /
// columns (pass 2) are split over workgroups, every split writes its partial sums to the workspace and a small kernel adds
// them in split order: no floating-point atomics, two calls give the same bits.
//
// mvf_assign_topk (the reference's sparse_calculation_mode: `_dense_to_sparse(axis=0, descending=True)`, methods/utils.py:
// 1085-1094, 1369-1404) keeps the k largest entries of every column of P.  Within a column P_ij = c3_j u_ij with u_ij = e2_ij m_i
// q_ij, the summand of S3, and c3_j >= 0: the k largest of a column of P are the k largest of u over the rows.  Pass 1 keeps,
// per workgroup, a sorted (value, row) list of k per column in LDS in the total order (value descending, row ascending); a
// wave per column merges the row splits' lists, applies c3 and writes rows / vals / K_NB; pass 2 adds an entry to K_NA / PXB
// only if its row index is in the column's list.  The k largest of a set under a total order do not depend on the order of
// insertion: the lists, and with them every output, are the same bits on every call.
//
// mvf_assign_layer_stats (what the reference computes in front of its loop from three more materialised matrices:
// `_init_guess_sigma2`, `_init_probability_parameters`, the nearest voxels of `_coarse_rigid_alignment`) reduces ONE layer's
// distance matrix, on the same tile routine and with pass 1's grid, to per-column minima, per-column lists of the k smallest
// entries (the lists of mvf_assign_topk with the order turned round) and the sums of d and d^2; the statistics of the rows are
// the same call with the operands exchanged.
//
// mvf_assign_best (the reference's cell mapping, `get_optimal_mapping_relationship` / `mapping_aligned_coords`,
// spateo/alignment/utils.py:157-255, which takes row and column maxima of the dense P) runs pass 1 and the factors as they are
// and then one sweep per direction on the same tile routine: per row and per column of P the largest entry and its index
// under the reference's two tie rules, from states that combine in any order (see struct Best).
//
// mvf_assign_apply (what the reference's users form from the dense P of `Morpho_pairwise.run()`: P.T @ onehot(labels), P @ X_B,
// the row-normalised forms) runs pass 1 and the factors as they are and then, per direction and 64-column chunk of the
// features, one sweep whose tile entries feed the same MFMA straight from the accumulator layout they are formed in (see
// assign_apply_kernel); P @ FB is that sweep on the exchanged operands.
#include <climits>

#include "mvf_common.h"

namespace mvf {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int AT = 64;            // tile edge (rows of A and columns of B per workgroup step)
constexpr int AKS = 16;           // features per k-step: 4 lane groups x 4 consecutive features (one 16 / 32-byte load)
constexpr int MAX_LAYERS = 4;
constexpr int MAX_SPLITS = 64;
constexpr int TARGET_WGS = 1024;  // workgroups a pass aims for (4 per CU)
constexpr double ASSIGN_EPS = 1e-8;
constexpr int TOPK_MAX = MVF_ASSIGN_TOPK_MAX;
constexpr int TOPK_STAGE = 16;    // candidates a column stages per round (more wait for the next round)
constexpr double TOPK_PREFILTER = 1e-6;  // pass 2 looks a row up in a column's list from this far below its last value on
static_assert(MAX_SPLITS <= 64, "the merge of the row splits' lists gives every split one lane of a wave");

struct DevLayer {
    const void* X;
    const void* Y;
    const double* a;
    const double* b;
    int64_t ld;
    double s;       // d = a_i + b_j - s dot
    double nparam;  // gauss: -1 / (2 p)
    int post;       // 0 none, 1 clamp at 0, 2 clamp at 0 and square root, POST_LABEL: d = X[a_i][b_j], X the float64 table
    int prob;       // mvf_assign_prob
};

constexpr int POST_LABEL = 3;

struct DevLayers {
    DevLayer l[MAX_LAYERS];
    int n;
};

struct Plan {
    int64_t rtiles, ctiles, na_pad, nb_pad, rsplit, csplit;
    size_t off_part1, off_fac, off_part2, off_rows, total;  // in bytes
};

Plan make_plan(int64_t na, int64_t nb) {
    Plan p;
    p.rtiles = cdiv(na, AT), p.ctiles = cdiv(nb, AT);
    p.na_pad = p.rtiles * AT, p.nb_pad = p.ctiles * AT;
    p.rsplit = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(p.rtiles, MAX_SPLITS), cdiv(TARGET_WGS, p.ctiles)));
    p.csplit = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(p.ctiles, MAX_SPLITS), cdiv(TARGET_WGS, p.rtiles)));
    size_t o = 0;
    p.off_part1 = o, o += align_up((size_t)p.rsplit * 4 * p.nb_pad * sizeof(double), 256);
    p.off_fac = o, o += align_up((size_t)p.nb_pad * 4 * sizeof(double), 256);
    p.off_part2 = o, o += align_up((size_t)p.csplit * p.na_pad * 8 * sizeof(double), 256);
    p.off_rows = o, o += align_up((size_t)p.na_pad * sizeof(double), 256);
    p.total = o;
    return p;
}

template <typename T>
__device__ __forceinline__ void load4(const T* p, double (&v)[4]) {
    const typename Vec4<T>::type u = *reinterpret_cast<const typename Vec4<T>::type*>(p);
    v[0] = (double)u.x, v[1] = (double)u.y, v[2] = (double)u.z, v[3] = (double)u.w;
}

__device__ __forceinline__ double layer_probability(const DevLayer& ly, double d) {
    if (ly.prob == MVF_ASSIGN_GAUSS) return exp(d * ly.nparam);
    if (ly.prob == MVF_ASSIGN_COS_PROB) return 1.0 - d;
    return d;
}

// d[a][b][r] = the layer's distance d(row i0 + 16 a + lk + 4 r, column j0 + 16 b + li) for the wave's 32 x 32 block at (i0, j0),
// a product layer: d = a_i + b_j - s <X'_i, Y'_j>, clamped at 0 / square-rooted as the metric has it.  Rows / columns beyond the
// arrays are clamped to the last one (finite values, masked by the callers).
template <typename T>
__device__ __forceinline__ void product_distances(const DevLayer& ly, int64_t i0, int64_t j0, int64_t na, int64_t nb, int li, int lk,
                                                  f64x4 (&acc)[2][2]) {
    const int64_t ld = ly.ld;
    // A operand of the MFMA: row li of block a, features 4 lk .. 4 lk + 3 of the k-step; B operand: column li of block b
    const T* pa[2];
    const T* pb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        pa[h] = (const T*)ly.X + std::min<int64_t>(i0 + 16 * h + li, na - 1) * ld + 4 * lk;
        pb[h] = (const T*)ly.Y + std::min<int64_t>(j0 + 16 * h + li, nb - 1) * ld + 4 * lk;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
    double na_[2][4], nb_[2][4];  // the next k-step's operands fly during this step's MFMAs
#pragma unroll
    for (int h = 0; h < 2; ++h) load4(pa[h], na_[h]), load4(pb[h], nb_[h]);
    for (int64_t k0 = 0; k0 < ld; k0 += AKS) {
        double fa[2][4], fb[2][4];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int t = 0; t < 4; ++t) fa[h][t] = na_[h][t], fb[h][t] = nb_[h][t];
        if (k0 + AKS < ld) {
#pragma unroll
            for (int h = 0; h < 2; ++h) load4(pa[h] + k0 + AKS, na_[h]), load4(pb[h] + k0 + AKS, nb_[h]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a][t], fb[b][t], acc[a][b], 0, 0, 0);
    }
    // D[row lk + 4 r of block a][column li of block b] sits in acc[a][b][r] of lane (li, lk)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double ai = ly.a[std::min<int64_t>(i0 + 16 * a + lk + 4 * r, na - 1)];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const double bj = ly.b[std::min<int64_t>(j0 + 16 * b + li, nb - 1)];
                double d = (ai + bj) - ly.s * acc[a][b][r];
                if (ly.post >= 1) d = fmax(d, 0.0);
                if (ly.post == 2) d = sqrt(d);
                acc[a][b][r] = d;
            }
        }
}

// The same for a label layer: d = T[la_i][lb_j], T = ly.X (float64, row length ly.ld), the labels integers held in ly.a / ly.b.
// 8 row labels, 2 column labels and 16 table reads per lane; no clamp, no square root.  TR: the caller sweeps the TRANSPOSED
// problem (rows = B cells, columns = A cells; ly.a / ly.b already exchanged) and the table is read as T[column label][row label].
template <bool TR = false>
__device__ __forceinline__ void label_distances(const DevLayer& ly, int64_t i0, int64_t j0, int64_t na, int64_t nb, int li, int lk,
                                                f64x4 (&acc)[2][2]) {
    const double* tab = (const double*)ly.X;
    int64_t cj[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) cj[b] = (int64_t)ly.b[std::min<int64_t>(j0 + 16 * b + li, nb - 1)] * (TR ? ly.ld : 1);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double* row = tab + (int64_t)ly.a[std::min<int64_t>(i0 + 16 * a + lk + 4 * r, na - 1)] * (TR ? 1 : ly.ld);
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b][r] = row[cj[b]];
        }
}

// q[a][b][r] = product over the layers of the probability of d(row i0 + 16 a + lk + 4 r, column j0 + 16 b + li), for the
// wave's 32 x 32 block at (i0, j0).  The branch between the two kinds of layer is the same on every lane; the probability is
// formed by one piece of code for both.  TR: see label_distances.
template <typename T, bool TR = false>
__device__ __forceinline__ void layer_product(const DevLayers& L, int64_t i0, int64_t j0, int64_t na, int64_t nb, int li, int lk,
                                              f64x4 (&q)[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) q[a][b] = f64x4{1.0, 1.0, 1.0, 1.0};
    for (int l = 0; l < L.n; ++l) {
        const DevLayer& ly = L.l[l];
        f64x4 acc[2][2];
        if (ly.post == POST_LABEL)
            label_distances<TR>(ly, i0, j0, na, nb, li, lk, acc);
        else
            product_distances<T>(ly, i0, j0, na, nb, li, lk, acc);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int b = 0; b < 2; ++b) q[a][b][r] *= layer_probability(ly, acc[a][b][r]);
    }
}

struct Point {
    double x, y, z, n2;
};

// workspace of mvf_assign_topk behind mvf_assign's: the row splits' lists, lv / lr[split][k][nb_pad]
struct TopkPlan {
    int k;  // min(k, na)
    size_t off_lv, off_lr, total;
};

TopkPlan make_topk_plan(const Plan& p, int64_t na, int k) {
    TopkPlan t;
    t.k = (int)std::min<int64_t>(k, na);
    size_t o = p.total;
    t.off_lv = o, o += align_up((size_t)p.rsplit * t.k * p.nb_pad * sizeof(double), 256);
    t.off_lr = o, o += align_up((size_t)p.rsplit * t.k * p.nb_pad * sizeof(int), 256);
    t.total = o;
    return t;
}

// the total order of a column's entries: value descending, row ascending
__device__ __forceinline__ bool topk_before(double v, int r, double w, int s) { return v > w || (v == w && r < s); }

template <typename T>
__device__ __forceinline__ Point load_point(const T* x4, int64_t i) {
    double v[4];
    load4(x4 + 4 * i, v);
    Point p;
    p.x = v[0], p.y = v[1], p.z = v[2];
    p.n2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    return p;
}

// the reference's squared distance: |x|^2 + |y|^2 - 2 x.y, clamped at 0 (methods/utils.py:780-783)
__device__ __forceinline__ double sq_dist(const Point& p, const Point& c) {
    const double dot = (p.x * c.x + p.y * c.y) + p.z * c.z;
    return fmax((p.n2 + c.n2) - 2.0 * dot, 0.0);
}

// ---- pass 1: column sums.  grid (column tiles, row splits); part1[split][S0..S3][nb_pad]
template <typename T>
__global__ __launch_bounds__(256) void assign_pass1_kernel(const T* __restrict__ xa4, int64_t na, const T* __restrict__ xb4,
                                                           int64_t nb, DevLayers L, const double* __restrict__ mm, double h1,
                                                           double h2, int64_t rtiles, int64_t nb_pad,
                                                           double* __restrict__ part1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4, wi = wave >> 1, wj = wave & 1;
    const int64_t j0 = (int64_t)blockIdx.x * AT + 32 * wj;
    const int64_t t_lo = rtiles * blockIdx.y / gridDim.y, t_hi = rtiles * (blockIdx.y + 1) / gridDim.y;
    Point cb[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) cb[b] = load_point(xb4, std::min<int64_t>(j0 + 16 * b + li, nb - 1));
    double s[4][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    for (int64_t t = t_lo; t < t_hi; ++t) {
        const int64_t i0 = t * AT + 32 * wi;
        f64x4 q[2][2];
        layer_product<T>(L, i0, j0, na, nb, li, lk, q);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = i0 + 16 * a + lk + 4 * r;
                const bool live = i < na;
                const Point pa = load_point(xa4, live ? i : na - 1);
                const double m = live ? mm[i] : 0.0, one = live ? 1.0 : 0.0;
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const double d = sq_dist(pa, cb[b]);
                    const double e1 = exp(d * h1), e2m = exp(d * h2) * m;
                    s[0][b] += e1 * one;
                    s[1][b] += e1 * m;
                    s[2][b] += e2m;
                    s[3][b] += e2m * q[a][b][r];
                }
            }
    }
    // the 8 (row half, lane group) partials of every column, added in a fixed order
    __shared__ double red[4][8][AT];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int b = 0; b < 2; ++b) red[k][wi * 4 + lk][32 * wj + 16 * b + li] = s[k][b];
    __syncthreads();
    const int k = threadIdx.x >> 6, c = threadIdx.x & 63;
    double tot = 0.0;
#pragma unroll
    for (int g = 0; g < 8; ++g) tot += red[k][g][c];
    part1[((int64_t)blockIdx.y * 4 + k) * nb_pad + (int64_t)blockIdx.x * AT + c] = tot;
}

// ---- pass 1 of mvf_assign_topk: the column sums as above and, per column, the k largest u = e2 m q of this row split.
// lval / lrow[p][c]: the list of column c, sorted, always k long (unused places hold (-inf, INT_MAX), which every entry
// beats).  Per tile a lane compares its 16 values with its columns' last entries; the ones that beat them are staged through
// per-column integer counters (at most TOPK_STAGE a round, the rest wait) and thread c inserts column c's.
template <typename T, int KC>
__global__ __launch_bounds__(256) void assign_pass1_topk_kernel(const T* __restrict__ xa4, int64_t na, const T* __restrict__ xb4,
                                                                int64_t nb, DevLayers L, const double* __restrict__ mm, double h1,
                                                                double h2, int64_t rtiles, int64_t nb_pad, int k,
                                                                double* __restrict__ part1, double* __restrict__ lv,
                                                                int* __restrict__ lr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4, wi = wave >> 1, wj = wave & 1;
    const int64_t j0 = (int64_t)blockIdx.x * AT + 32 * wj;
    const int64_t t_lo = rtiles * blockIdx.y / gridDim.y, t_hi = rtiles * (blockIdx.y + 1) / gridDim.y;
    __shared__ double lval[KC][AT];
    __shared__ int lrow[KC][AT];
    __shared__ double red[4][8][AT];  // after the tiles: the partial sums; between them: the staged candidates
    __shared__ int scnt[AT];
    double(*sval)[AT] = reinterpret_cast<double(*)[AT]>(&red[0][0][0]);  // [TOPK_STAGE][AT]
    int(*srow)[AT] = reinterpret_cast<int(*)[AT]>(&red[2][0][0]);        // [TOPK_STAGE][AT]
    static_assert(TOPK_STAGE * AT * sizeof(double) <= 2 * 8 * AT * sizeof(double) &&
                      TOPK_STAGE * AT * sizeof(int) <= 2 * 8 * AT * sizeof(double),
                  "the staged values lie in red[0..1], their rows in red[2..3]");
    for (int e = threadIdx.x; e < k * AT; e += 256) lval[e / AT][e % AT] = -HUGE_VAL, lrow[e / AT][e % AT] = INT_MAX;
    if (threadIdx.x < AT) scnt[threadIdx.x] = 0;
    __syncthreads();
    Point cb[2];
    int col[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) cb[b] = load_point(xb4, std::min<int64_t>(j0 + 16 * b + li, nb - 1)), col[b] = 32 * wj + 16 * b + li;
    double s[4][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    for (int64_t t = t_lo; t < t_hi; ++t) {
        const int64_t i0 = t * AT + 32 * wi;
        f64x4 q[2][2];
        layer_product<T>(L, i0, j0, na, nb, li, lk, q);
        double u[2][4][2];
        unsigned pend = 0;  // bit 8 a + 2 r + b: u[a][r][b] beats the last entry of its column's list and is not staged yet
        double tv[2];
        int tr[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) tv[b] = lval[k - 1][col[b]], tr[b] = lrow[k - 1][col[b]];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = i0 + 16 * a + lk + 4 * r;
                const bool live = i < na;
                const Point pa = load_point(xa4, live ? i : na - 1);
                const double m = live ? mm[i] : 0.0, one = live ? 1.0 : 0.0;
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const double d = sq_dist(pa, cb[b]);
                    const double e1 = exp(d * h1), e2m = __dmul_rn(exp(d * h2), m);
                    const double uu = __dmul_rn(e2m, q[a][b][r]);  // the selection key: a product, stored as rounded
                    s[0][b] += e1 * one;
                    s[1][b] += e1 * m;
                    s[2][b] += e2m;
                    s[3][b] += uu;
                    u[a][r][b] = uu;
                    if (live && topk_before(uu, (int)i, tv[b], tr[b])) pend |= 1u << (8 * a + 2 * r + b);
                }
            }
        while (__syncthreads_or(pend != 0)) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const unsigned bit = 1u << (8 * a + 2 * r + b);
                        if (pend & bit) {
                            const int slot = atomicAdd(&scnt[col[b]], 1);
                            if (slot < TOPK_STAGE) {
                                sval[slot][col[b]] = u[a][r][b];
                                srow[slot][col[b]] = (int)(i0 + 16 * a + lk + 4 * r);
                                pend &= ~bit;
                            }
                        }
                    }
            __syncthreads();
            if (threadIdx.x < AT) {
                const int c = threadIdx.x, n = min(scnt[c], TOPK_STAGE);
                for (int e = 0; e < n; ++e) {
                    const double v = sval[e][c];
                    const int row = srow[e][c];
                    if (!topk_before(v, row, lval[k - 1][c], lrow[k - 1][c])) continue;
                    int p = k - 1;
                    while (p > 0 && topk_before(v, row, lval[p - 1][c], lrow[p - 1][c])) {
                        lval[p][c] = lval[p - 1][c], lrow[p][c] = lrow[p - 1][c];
                        --p;
                    }
                    lval[p][c] = v, lrow[p][c] = row;
                }
                scnt[c] = 0;
            }
            __syncthreads();
            if (pend) {  // what waits for the next round is compared with the lists as they are now
#pragma unroll
                for (int b = 0; b < 2; ++b) tv[b] = lval[k - 1][col[b]], tr[b] = lrow[k - 1][col[b]];
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int b = 0; b < 2; ++b) {
                            const unsigned bit = 1u << (8 * a + 2 * r + b);
                            if ((pend & bit) && !topk_before(u[a][r][b], (int)(i0 + 16 * a + lk + 4 * r), tv[b], tr[b])) pend &= ~bit;
                        }
            }
        }
    }
    // (the loop's last barrier lies behind the last insertion)
    for (int e = threadIdx.x; e < k * AT; e += 256) {
        const int64_t o = ((int64_t)blockIdx.y * k + e / AT) * nb_pad + (int64_t)blockIdx.x * AT + e % AT;
        lv[o] = lval[e / AT][e % AT], lr[o] = lrow[e / AT][e % AT];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int b = 0; b < 2; ++b) red[kk][wi * 4 + lk][32 * wj + 16 * b + li] = s[kk][b];
    __syncthreads();
    const int kk = threadIdx.x >> 6, c = threadIdx.x & 63;
    double tot = 0.0;
#pragma unroll
    for (int g = 0; g < 8; ++g) tot += red[kk][g][c];
    part1[((int64_t)blockIdx.y * 4 + kk) * nb_pad + (int64_t)blockIdx.x * AT + c] = tot;
}

// ---- the row splits' lists of a column merged by one wave (lane = split, its list's head in registers; k rounds pick the
// first of the heads in the total order): rows / vals[j][k] = the kept entries of P, K_NB[j] = their sum in stored order
__global__ __launch_bounds__(256) void assign_topk_merge_kernel(const double* __restrict__ lv, const int* __restrict__ lr,
                                                                int64_t rsplit, int k, int64_t nb, int64_t nb_pad,
                                                                const double* __restrict__ fac, int* __restrict__ rows,
                                                                double* __restrict__ vals, double* __restrict__ K_NB) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= nb) return;
    const double c3 = fac[4 * j + 2];
    int ptr = 0;
    double hv = -HUGE_VAL;
    int hr = INT_MAX;
    if (lane < rsplit) hv = lv[((int64_t)lane * k) * nb_pad + j], hr = lr[((int64_t)lane * k) * nb_pad + j];
    double sum = 0.0;
    for (int p = 0; p < k; ++p) {
        double bv = hv;
        int br = hr, bs = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64);
            const int orow = __shfl_xor(br, o, 64), os = __shfl_xor(bs, o, 64);
            if (topk_before(ov, orow, bv, br) || (ov == bv && orow == br && os < bs)) bv = ov, br = orow, bs = os;
        }
        if (lane == bs) {
            ++ptr;
            hv = -HUGE_VAL, hr = INT_MAX;
            if (ptr < k && lane < rsplit) hv = lv[((int64_t)lane * k + ptr) * nb_pad + j], hr = lr[((int64_t)lane * k + ptr) * nb_pad + j];
        }
        if (lane == 0) {
            // (na >= k rows were offered, so a place holder can only come first behind non-finite values: kept in range)
            const bool real = br != INT_MAX;
            const double v = real ? __dmul_rn(c3, bv) : 0.0;
            rows[j * k + p] = real ? br : p;
            vals[j * k + p] = v;
            sum += v;
        }
    }
    if (lane == 0) K_NB[j] = sum;
}

// ---- mvf_assign_layer_stats: column statistics of ONE layer's distance matrix, for the alignment's start state (what
// `_init_guess_sigma2`, `_init_probability_parameters` and `_coarse_rigid_alignment` reduce their na x nb matrices to).  Pass 1's
// tiling, row split and workgroup shape; per column and row split: the minimum, the sum and the sum of squares of d over the
// live rows and, for KC > 0, the k SMALLEST entries as pass 1 of mvf_assign_topk keeps the k largest: the same sorted lists in
// LDS and the same staging, in the total order (value ascending, row ascending); unused places hold (+inf, INT_MAX).
// part[split][{min, sum, sum of squares}][nb_pad]
__device__ __forceinline__ bool stats_before(double v, int r, double w, int s) { return v < w || (v == w && r < s); }

template <typename T, int KC>
__global__ __launch_bounds__(256) void layer_stats_kernel(DevLayer ly, int64_t na, int64_t nb, int64_t rtiles, int64_t nb_pad,
                                                          int k, double* __restrict__ part, double* __restrict__ lv,
                                                          int* __restrict__ lr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4, wi = wave >> 1, wj = wave & 1;
    const int64_t j0 = (int64_t)blockIdx.x * AT + 32 * wj;
    const int64_t t_lo = rtiles * blockIdx.y / gridDim.y, t_hi = rtiles * (blockIdx.y + 1) / gridDim.y;
    __shared__ double lval[KC ? KC : 1][AT];
    __shared__ int lrow[KC ? KC : 1][AT];
    __shared__ double red[4][8][AT];  // after the tiles: the partial statistics; between them: the staged candidates
    __shared__ int scnt[AT];
    double(*sval)[AT] = reinterpret_cast<double(*)[AT]>(&red[0][0][0]);  // [TOPK_STAGE][AT]
    int(*srow)[AT] = reinterpret_cast<int(*)[AT]>(&red[2][0][0]);        // [TOPK_STAGE][AT]
    static_assert(TOPK_STAGE * AT * sizeof(double) <= 2 * 8 * AT * sizeof(double) &&
                      TOPK_STAGE * AT * sizeof(int) <= 2 * 8 * AT * sizeof(double),
                  "the staged values lie in red[0..1], their rows in red[2..3]");
    if (KC) {
        for (int e = threadIdx.x; e < k * AT; e += 256) lval[e / AT][e % AT] = HUGE_VAL, lrow[e / AT][e % AT] = INT_MAX;
        if (threadIdx.x < AT) scnt[threadIdx.x] = 0;
        __syncthreads();
    }
    int col[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) col[b] = 32 * wj + 16 * b + li;
    double mn[2] = {HUGE_VAL, HUGE_VAL}, s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
    for (int64_t t = t_lo; t < t_hi; ++t) {
        const int64_t i0 = t * AT + 32 * wi;
        f64x4 d[2][2];
        if (ly.post == POST_LABEL)
            label_distances(ly, i0, j0, na, nb, li, lk, d);
        else
            product_distances<T>(ly, i0, j0, na, nb, li, lk, d);
        unsigned pend = 0;  // bit 8 a + 2 r + b: d[a][b][r] beats the last entry of its column's list and is not staged yet
        double tv[2] = {0.0, 0.0};
        int tr[2] = {0, 0};
        if (KC) {
#pragma unroll
            for (int b = 0; b < 2; ++b) tv[b] = lval[k - 1][col[b]], tr[b] = lrow[k - 1][col[b]];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = i0 + 16 * a + lk + 4 * r;
                if (i >= na) continue;  // a padded row (clamped to the last one by the tile routine) is in no statistic
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const double v = d[a][b][r];
                    mn[b] = fmin(mn[b], v);
                    s1[b] += v;
                    s2[b] += v * v;
                    if (KC && stats_before(v, (int)i, tv[b], tr[b])) pend |= 1u << (8 * a + 2 * r + b);
                }
            }
        while (KC && __syncthreads_or(pend != 0)) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const unsigned bit = 1u << (8 * a + 2 * r + b);
                        if (pend & bit) {
                            const int slot = atomicAdd(&scnt[col[b]], 1);
                            if (slot < TOPK_STAGE) {
                                sval[slot][col[b]] = d[a][b][r];
                                srow[slot][col[b]] = (int)(i0 + 16 * a + lk + 4 * r);
                                pend &= ~bit;
                            }
                        }
                    }
            __syncthreads();
            if (threadIdx.x < AT) {
                const int c = threadIdx.x, n = min(scnt[c], TOPK_STAGE);
                for (int e = 0; e < n; ++e) {
                    const double v = sval[e][c];
                    const int row = srow[e][c];
                    if (!stats_before(v, row, lval[k - 1][c], lrow[k - 1][c])) continue;
                    int p = k - 1;
                    while (p > 0 && stats_before(v, row, lval[p - 1][c], lrow[p - 1][c])) {
                        lval[p][c] = lval[p - 1][c], lrow[p][c] = lrow[p - 1][c];
                        --p;
                    }
                    lval[p][c] = v, lrow[p][c] = row;
                }
                scnt[c] = 0;
            }
            __syncthreads();
            if (pend) {  // what waits for the next round is compared with the lists as they are now
#pragma unroll
                for (int b = 0; b < 2; ++b) tv[b] = lval[k - 1][col[b]], tr[b] = lrow[k - 1][col[b]];
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int b = 0; b < 2; ++b) {
                            const unsigned bit = 1u << (8 * a + 2 * r + b);
                            if ((pend & bit) && !stats_before(d[a][b][r], (int)(i0 + 16 * a + lk + 4 * r), tv[b], tr[b])) pend &= ~bit;
                        }
            }
        }
    }
    if (KC) {  // (the loop's last barrier lies behind the last insertion)
        for (int e = threadIdx.x; e < k * AT; e += 256) {
            const int64_t o = ((int64_t)blockIdx.y * k + e / AT) * nb_pad + (int64_t)blockIdx.x * AT + e % AT;
            lv[o] = lval[e / AT][e % AT], lr[o] = lrow[e / AT][e % AT];
        }
        __syncthreads();
    }
    // the 8 (row half, lane group) partials of every column, combined in a fixed order
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        red[0][wi * 4 + lk][col[b]] = mn[b];
        red[1][wi * 4 + lk][col[b]] = s1[b];
        red[2][wi * 4 + lk][col[b]] = s2[b];
    }
    __syncthreads();
    const int kk = threadIdx.x >> 6, c = threadIdx.x & 63;
    if (kk == 3) return;
    double tot = red[kk][0][c];
#pragma unroll
    for (int g = 1; g < 8; ++g) tot = kk == 0 ? fmin(tot, red[kk][g][c]) : tot + red[kk][g][c];
    part[((int64_t)blockIdx.y * 3 + kk) * nb_pad + (int64_t)blockIdx.x * AT + c] = tot;
}

// the row splits' statistics of a column combined in split order: cmin[j], and the column's two sums colsum[{0, 1}][nb_pad]
__global__ __launch_bounds__(256) void layer_stats_columns_kernel(const double* __restrict__ part, int64_t rsplit, int64_t nb,
                                                                  int64_t nb_pad, double* __restrict__ cmin,
                                                                  double* __restrict__ colsum) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nb) return;  // a padded column (clamped to the last one by the tile routine) is in no statistic
    double mn = HUGE_VAL, s1 = 0.0, s2 = 0.0;
    for (int64_t sp = 0; sp < rsplit; ++sp) {
        mn = fmin(mn, part[(sp * 3 + 0) * nb_pad + j]);
        s1 += part[(sp * 3 + 1) * nb_pad + j];
        s2 += part[(sp * 3 + 2) * nb_pad + j];
    }
    cmin[j] = mn, colsum[j] = s1, colsum[nb_pad + j] = s2;
}

// the row splits' lists of a column merged by one wave, as assign_topk_merge_kernel does it, in stats_before's order:
// rows / vals[j][k] = the column's k smallest entries
__global__ __launch_bounds__(256) void layer_stats_merge_kernel(const double* __restrict__ lv, const int* __restrict__ lr,
                                                                int64_t rsplit, int k, int64_t nb, int64_t nb_pad,
                                                                int* __restrict__ rows, double* __restrict__ vals) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= nb) return;
    int ptr = 0;
    double hv = HUGE_VAL;
    int hr = INT_MAX;
    if (lane < rsplit) hv = lv[((int64_t)lane * k) * nb_pad + j], hr = lr[((int64_t)lane * k) * nb_pad + j];
    for (int p = 0; p < k; ++p) {
        double bv = hv;
        int br = hr, bs = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64);
            const int orow = __shfl_xor(br, o, 64), os = __shfl_xor(bs, o, 64);
            if (stats_before(ov, orow, bv, br) || (ov == bv && orow == br && os < bs)) bv = ov, br = orow, bs = os;
        }
        if (lane == bs) {
            ++ptr;
            hv = HUGE_VAL, hr = INT_MAX;
            if (ptr < k && lane < rsplit) hv = lv[((int64_t)lane * k + ptr) * nb_pad + j], hr = lr[((int64_t)lane * k + ptr) * nb_pad + j];
        }
        if (lane == 0) {
            // (na >= k rows were offered, so a place holder can only come first behind non-finite values: kept in range)
            const bool real = br != INT_MAX;
            rows[j * k + p] = real ? br : p;
            vals[j * k + p] = real ? bv : 0.0;
        }
    }
}

// ---- column factors: fac[j] = {c1, c2, c3, 0}, K_NB[j] = c3 S3 (the splits added in order)
__global__ __launch_bounds__(256) void assign_factors_kernel(const double* __restrict__ part1, int64_t rsplit, int64_t nb,
                                                             int64_t nb_pad, double outlier, double* __restrict__ fac,
                                                             double* __restrict__ K_NB) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nb_pad) return;
    double S[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t sp = 0; sp < rsplit; ++sp)
#pragma unroll
        for (int k = 0; k < 4; ++k) S[k] += part1[(sp * 4 + k) * nb_pad + j];
    double c1 = 0.0, c2 = 0.0, c3 = 0.0;
    if (j < nb) {
        const double inl = 1.0 - outlier / (outlier + S[0]);
        c1 = 1.0 / (outlier + S[1]);
        c2 = inl / (S[2] + ASSIGN_EPS);
        c3 = inl / (S[3] + ASSIGN_EPS);
        K_NB[j] = c3 * S[3];
    }
    fac[4 * j + 0] = c1, fac[4 * j + 1] = c2, fac[4 * j + 2] = c3, fac[4 * j + 3] = 0.0;  // columns >= nb: zero weight
}

// ---- pass 2: row sums.  grid (row tiles, column splits); part2[split][na_pad][8] = {sum e1 c1, sum e2 c2, sum e2 q c3,
// PXB x, y, z, sum e2 c2 d, 0} (the row factor m_i is applied by the reduction).  MODE P2_DENSE writes P as well; P2_TOPK
// (mvf_assign_topk) adds to sum e2 q c3 and to PXB only the entries whose row is in the column's list trows[j][k]: the
// comparison with the list's last value tvals[j][k - 1] only spares the look-up, the row indices decide
enum { P2_PLAIN = 0, P2_DENSE = 1, P2_TOPK = 2 };

template <typename T, int MODE>
__global__ __launch_bounds__(256) void assign_pass2_kernel(const T* __restrict__ xa4, int64_t na, const T* __restrict__ xb4,
                                                           int64_t nb, DevLayers L, const double* __restrict__ mm, double h1,
                                                           double h2, const double* __restrict__ fac, int64_t ctiles,
                                                           int64_t na_pad, double* __restrict__ part2, double* __restrict__ P,
                                                           const int* __restrict__ trows, const double* __restrict__ tvals,
                                                           int tk) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4, wi = wave >> 1, wj = wave & 1;
    const int64_t i0 = (int64_t)blockIdx.x * AT + 32 * wi;
    const int64_t t_lo = ctiles * blockIdx.y / gridDim.y, t_hi = ctiles * (blockIdx.y + 1) / gridDim.y;
    Point pa[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) pa[a][r] = load_point(xa4, std::min<int64_t>(i0 + 16 * a + lk + 4 * r, na - 1));
    double acc[2][4][7];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < 7; ++k) acc[a][r][k] = 0.0;
    double mi[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) mi[a][r] = MODE == P2_TOPK ? mm[std::min<int64_t>(i0 + 16 * a + lk + 4 * r, na - 1)] : 0.0;
    for (int64_t t = t_lo; t < t_hi; ++t) {
        const int64_t j0 = t * AT + 32 * wj;
        f64x4 q[2][2];
        layer_product<T>(L, i0, j0, na, nb, li, lk, q);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int64_t j = j0 + 16 * b + li;  // < nb_pad: fac is zero for nb <= j
            const Point cb = load_point(xb4, std::min<int64_t>(j, nb - 1));
            double f[4];
            load4(fac + 4 * j, f);
            double last = 0.0;
            if (MODE == P2_TOPK && j < nb) last = tvals[j * tk + tk - 1];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double d = sq_dist(pa[a][r], cb);
                    const double e1 = exp(d * h1), e2 = exp(d * h2);
                    const double t2 = e2 * f[1];
                    double t3 = (e2 * q[a][b][r]) * f[2];
                    if (MODE == P2_TOPK) {
                        // (an entry that is exactly 0 adds nothing whether it is kept or not: not looked up)
                        bool keep = false;
                        const int64_t i = i0 + 16 * a + lk + 4 * r;
                        if (j < nb && i < na && t3 != 0.0 && mi[a][r] * t3 >= last - TOPK_PREFILTER * fabs(last)) {
                            const int* lst = trows + j * tk;
                            for (int p = 0; p < tk; ++p) keep = keep || lst[p] == (int)i;
                        }
                        if (!keep) t3 = 0.0;
                    }
                    acc[a][r][0] += e1 * f[0];
                    acc[a][r][1] += t2;
                    acc[a][r][2] += t3;
                    acc[a][r][3] += t3 * cb.x;
                    acc[a][r][4] += t3 * cb.y;
                    acc[a][r][5] += t3 * cb.z;
                    acc[a][r][6] += t2 * d;
                    if (MODE == P2_DENSE) {
                        const int64_t i = i0 + 16 * a + lk + 4 * r;
                        if (i < na && j < nb) P[i * nb + j] = mm[i] * t3;
                    }
                }
        }
    }
    // sum over the 16 column lanes (a butterfly inside each group of 16 lanes: the same order on every lane), then over the
    // two column halves of the tile through LDS
    __shared__ double red[2][AT][8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                double v = acc[a][r][k];
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (li == 0) red[wj][32 * wi + 16 * a + lk + 4 * r][k] = v;
            }
    __syncthreads();
    for (int e = threadIdx.x; e < AT * 8; e += 256) {
        const int row = e >> 3, k = e & 7;
        const double v = k < 7 ? red[0][row][k] + red[1][row][k] : 0.0;
        part2[((int64_t)blockIdx.y * na_pad + (int64_t)blockIdx.x * AT + row) * 8 + k] = v;
    }
}

// ---- rows: the column splits added in order, times m_i
__global__ __launch_bounds__(256) void assign_rows_kernel(const double* __restrict__ part2, int64_t csplit, int64_t na,
                                                          int64_t na_pad, const double* __restrict__ mm,
                                                          double* __restrict__ K_NA, double* __restrict__ K_NA_spatial,
                                                          double* __restrict__ K_NA_sigma2, double* __restrict__ PXB,
                                                          double* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= na) return;
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t sp = 0; sp < csplit; ++sp)
#pragma unroll
        for (int k = 0; k < 7; ++k) v[k] += part2[(sp * na_pad + i) * 8 + k];
    const double m = mm[i];
    K_NA_spatial[i] = m * v[0];
    K_NA_sigma2[i] = m * v[1];
    K_NA[i] = m * v[2];
    PXB[3 * i + 0] = m * v[3], PXB[3 * i + 1] = m * v[4], PXB[3 * i + 2] = m * v[5];
    rows[i] = m * v[6];
}

// one workgroup: out[0] = sum of v[0 .. n) in a fixed order
__global__ __launch_bounds__(256) void assign_sum_kernel(const double* __restrict__ v, int64_t n, double* __restrict__ out) {
    __shared__ double red[4];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += v[i];
    const double t = block_sum<256>(s, red);
    if (threadIdx.x == 0) out[0] = t;
}

// ---- operand preparation: one wave per cell
__device__ __forceinline__ double wave_all_sum(double v) { return __shfl(wave_sum(v), 0, 64); }

// one row of one side of one product layer, by the 64 lanes of one wave: x (g float64) -> o (ld, cell dtype; the tail zero);
// returns the row constant on every lane.  Sums run lane-strided over k and then across the wave: every caller gets the
// same bits for the same x.
template <typename T>
__device__ __forceinline__ double assign_prepare_row(const double* x, int64_t g, int metric, int side, T* o, int64_t ld, int lane) {
    double cst = 0.0;
    if (metric == MVF_ASSIGN_EUC || metric == MVF_ASSIGN_SQRT_EUC) {
        double s = 0.0;
        for (int64_t k = lane; k < g; k += 64) {
            const T v = (T)x[k];
            o[k] = v;
            s += (double)v * (double)v;
        }
        cst = wave_all_sum(s);
    } else if (metric == MVF_ASSIGN_COS) {
        double s = 0.0;
        for (int64_t k = lane; k < g; k += 64) s += x[k] * x[k];
        const double nrm = fmax(sqrt(wave_all_sum(s)), ASSIGN_EPS);
        for (int64_t k = lane; k < g; k += 64) o[k] = (T)(x[k] / nrm);
        cst = side == 0 ? 0.5 : 0.0;
    } else {  // kl / sym_kl
        double s = 0.0;
        for (int64_t k = lane; k < g; k += 64) s += x[k] + 0.01;
        const double tot = wave_all_sum(s);
        const bool sym = metric == MVF_ASSIGN_SYM_KL;
        double e = 0.0;
        for (int64_t k = lane; k < g; k += 64) {
            const T p = (T)((x[k] + 0.01) / tot);
            const double lp = log((double)p + ASSIGN_EPS);
            e += (double)p * lp;
            // A side: [p, log p] ; B side: [log q, q]  (kl keeps the first half only)
            if (side == 0) {
                o[k] = p;
                if (sym) o[g + k] = (T)lp;
            } else {
                o[k] = (T)lp;
                if (sym) o[g + k] = p;
            }
        }
        e = wave_all_sum(e);
        cst = sym ? 0.5 * e : (side == 0 ? e : 0.0);
    }
    const int64_t gp = metric == MVF_ASSIGN_SYM_KL ? 2 * g : g;
    for (int64_t k = gp + lane; k < ld; k += 64) o[k] = (T)0;
    return cst;
}

template <typename T>
__global__ __launch_bounds__(256) void assign_prepare_kernel(const double* __restrict__ Lraw, int64_t n, int64_t g, int metric,
                                                             int side, T* __restrict__ Lp, int64_t ld, double* __restrict__ ab) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const double cst = assign_prepare_row<T>(Lraw + i * g, g, metric, side, Lp + i * ld, ld, lane);
    if (lane == 0) ab[i] = cst;
}

// ---- the same from CSR: each wave owns one staging row of g float64 (all zero between rows), scatters a CSR row into it,
// runs assign_prepare_row on it and takes its entries out again; a block walks rows blockIdx.x * 4 + wave, + 4 gridDim.x, ...
// An entry whose column is outside [0, g) is skipped, never used as an address.  The barriers order the stores and loads of
// different lanes on one staging row (the loop's trip count is uniform over the block; a wave past n only idles).
template <typename T, typename V>
__global__ __launch_bounds__(256) void assign_prepare_csr_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                                 const V* __restrict__ data, int64_t n, int64_t g, int metric, int side,
                                                                 T* Lp, int64_t ld, double* ab, double* stage) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* x = stage + ((int64_t)blockIdx.x * 4 + wave) * g;
    for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
        const int64_t i = base + wave;
        const bool active = i < n;
        const int64_t e0 = active ? indptr[i] : 0, e1 = active ? indptr[i + 1] : 0;
        for (int64_t e = e0 + lane; e < e1; e += 64) {
            const int64_t c = indices[e];
            if (c >= 0 && c < g) x[c] = (double)data[e];
        }
        __syncthreads();
        if (active) {
            const double cst = assign_prepare_row<T>(x, g, metric, side, Lp + i * ld, ld, lane);
            if (lane == 0) ab[i] = cst;
        }
        __syncthreads();
        for (int64_t e = e0 + lane; e < e1; e += 64) {
            const int64_t c = indices[e];
            if (c >= 0 && c < g) x[c] = 0.0;
        }
        __syncthreads();
    }
}

// labels as the label branch reads them: integers held in float64, clamped into the table
__global__ __launch_bounds__(256) void assign_label_prepare_kernel(const int32_t* __restrict__ labels, int64_t n, int classes,
                                                                   double* __restrict__ ab) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) ab[i] = (double)min(max(labels[i], 0), classes - 1);
}

constexpr int CSR_MAX_BLOCKS = 4096;  // staging blocks of mvf_assign_prepare_csr: 16 per CU of a 256-CU device

int64_t padded_features(int64_t g, int metric) { return cdiv(metric == MVF_ASSIGN_SYM_KL ? 2 * g : g, AKS) * AKS; }

template <typename T>
int run_assign(hipStream_t st, const Plan& p, const void* xa4, int64_t na, const void* xb4, int64_t nb, const DevLayers& L,
               const double* mm, double h1, double h2, double outlier, double* K_NA, double* K_NB, double* K_NA_spatial,
               double* K_NA_sigma2, double* PXB, double* scalars, double* P, const TopkPlan* tp, int* trows, double* tvals,
               char* ws) {
    double* part1 = (double*)(ws + p.off_part1);
    double* fac = (double*)(ws + p.off_fac);
    double* part2 = (double*)(ws + p.off_part2);
    double* rows = (double*)(ws + p.off_rows);
    const dim3 grid1((unsigned)p.ctiles, (unsigned)p.rsplit), grid2((unsigned)p.rtiles, (unsigned)p.csplit);
    double* lv = tp ? (double*)(ws + tp->off_lv) : nullptr;
    int* lr = tp ? (int*)(ws + tp->off_lr) : nullptr;
    const int k = tp ? tp->k : 0;
#define MVF_PASS1_TOPK(KC)                                                                                                     \
    hipLaunchKernelGGL((assign_pass1_topk_kernel<T, KC>), grid1, dim3(256), 0, st, (const T*)xa4, na, (const T*)xb4, nb, L, mm, \
                       h1, h2, p.rtiles, p.nb_pad, k, part1, lv, lr)
    if (!tp)
        hipLaunchKernelGGL((assign_pass1_kernel<T>), grid1, dim3(256), 0, st, (const T*)xa4, na, (const T*)xb4, nb, L, mm, h1, h2,
                           p.rtiles, p.nb_pad, part1);
    else if (k <= 4)  // the lists' LDS is sized by the template: 3 KiB, 12 KiB or 48 KiB
        MVF_PASS1_TOPK(4);
    else if (k <= 16)
        MVF_PASS1_TOPK(16);
    else
        MVF_PASS1_TOPK(TOPK_MAX);
#undef MVF_PASS1_TOPK
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(assign_factors_kernel, dim3((unsigned)cdiv(p.nb_pad, 256)), dim3(256), 0, st, part1, p.rsplit, nb, p.nb_pad,
                       outlier, fac, K_NB);
    MVF_LAUNCH_CHECK();
    if (tp) {  // K_NB is written again: the sum of the column's kept entries
        hipLaunchKernelGGL(assign_topk_merge_kernel, dim3((unsigned)cdiv(nb, 4)), dim3(256), 0, st, lv, lr, p.rsplit, k, nb, p.nb_pad,
                           fac, trows, tvals, K_NB);
        MVF_LAUNCH_CHECK();
        hipLaunchKernelGGL((assign_pass2_kernel<T, P2_TOPK>), grid2, dim3(256), 0, st, (const T*)xa4, na, (const T*)xb4, nb, L, mm,
                           h1, h2, fac, p.ctiles, p.na_pad, part2, P, trows, tvals, k);
    } else if (P)
        hipLaunchKernelGGL((assign_pass2_kernel<T, P2_DENSE>), grid2, dim3(256), 0, st, (const T*)xa4, na, (const T*)xb4, nb, L, mm,
                           h1, h2, fac, p.ctiles, p.na_pad, part2, P, nullptr, nullptr, 0);
    else
        hipLaunchKernelGGL((assign_pass2_kernel<T, P2_PLAIN>), grid2, dim3(256), 0, st, (const T*)xa4, na, (const T*)xb4, nb, L, mm,
                           h1, h2, fac, p.ctiles, p.na_pad, part2, P, nullptr, nullptr, 0);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(assign_rows_kernel, dim3((unsigned)cdiv(na, 256)), dim3(256), 0, st, part2, p.csplit, na, p.na_pad, mm, K_NA,
                       K_NA_spatial, K_NA_sigma2, PXB, rows);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(assign_sum_kernel, dim3(1), dim3(256), 0, st, rows, na, scalars);
    MVF_LAUNCH_CHECK();
    return 0;
}

// one host layer validated and translated for the kernels; `probability`: the layer's prob / param are read (the passes of
// mvf_assign*) or ignored (mvf_assign_layer_stats)
int check_layer(const char* who, int l, const mvf_assign_layer& s, bool probability, DevLayer& d) {
    MVF_REQUIRE(s.metric >= MVF_ASSIGN_EUC && s.metric <= MVF_ASSIGN_LABEL, "%s: layer %d: bad metric %d", who, l, s.metric);
    const bool label = s.metric == MVF_ASSIGN_LABEL;  // Xp: the table, ld its row length, Yp NULL
    // (a layer that carries prepared B rows is a product layer: with the label code its Xp / a / b would be read as table
    // and labels, unchecked - refused before anything is launched)
    MVF_REQUIRE(!label || !s.Yp, "%s: layer %d: bad metric %d for a layer with Yp set (a label layer has no Yp: pass NULL)", who, l,
                s.metric);
    MVF_REQUIRE(s.Xp && (s.Yp || label) && s.a && s.b, "%s: null pointer in layer %d", who, l);
    if (label)
        MVF_REQUIRE(s.ld >= 1 && s.ld < ((int64_t)1 << 31), "%s: layer %d: a label layer's ld is the table's row length L >= 1", who, l);
    else
        MVF_REQUIRE(s.ld >= AKS && s.ld % AKS == 0, "%s: layer %d: ld must be a positive multiple of %d", who, l, AKS);
    if (probability) {
        MVF_REQUIRE(s.prob >= MVF_ASSIGN_GAUSS && s.prob <= MVF_ASSIGN_PROB, "%s: layer %d: bad probability type %d", who, l, s.prob);
        MVF_REQUIRE(s.prob != MVF_ASSIGN_GAUSS || s.param > 0.0, "%s: layer %d: a gauss layer needs a parameter > 0", who, l);
    }
    d.X = s.Xp, d.Y = s.Yp, d.a = s.a, d.b = s.b, d.ld = s.ld, d.prob = probability ? s.prob : MVF_ASSIGN_PROB;
    d.nparam = probability && s.prob == MVF_ASSIGN_GAUSS ? -1.0 / (2.0 * s.param) : 0.0;
    d.s = s.metric <= MVF_ASSIGN_SQRT_EUC ? 2.0 : (s.metric == MVF_ASSIGN_KL ? 1.0 : 0.5);
    d.post = label ? POST_LABEL : (s.metric == MVF_ASSIGN_EUC ? 1 : (s.metric == MVF_ASSIGN_SQRT_EUC ? 2 : 0));
    return 0;
}

int assign_entry(const char* who, const void* xa4, int64_t na, const void* xb4, int64_t nb, const mvf_assign_layer* layers,
                 int nlayers, const double* model_mul, double sigma2, double sigma2_variance, double spatial_outlier,
                 double* K_NA, double* K_NB, double* K_NA_spatial, double* K_NA_sigma2, double* PXB, double* scalars, double* P,
                 bool dense, int k, int* trows, double* tvals, void* workspace, size_t workspace_bytes, mvf_dtype dtype,
                 void* stream) {
    const bool topk = trows || tvals || k;  // (mvf_assign and mvf_assign_dense pass 0 and null pointers)
    if (topk) MVF_REQUIRE(k >= 1 && k <= TOPK_MAX, "%s: need 1 <= k <= %d, got %d", who, TOPK_MAX, k);
    if (na == 0 || nb == 0) return 0;
    MVF_REQUIRE(na > 0 && nb > 0, "%s: negative size", who);
    MVF_REQUIRE(na < ((int64_t)1 << 31) && nb < ((int64_t)1 << 31), "%s: too many cells", who);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "%s: bad dtype %d", who, (int)dtype);
    MVF_REQUIRE(nlayers >= 1 && nlayers <= MAX_LAYERS, "%s: need 1 .. %d layers, got %d", who, MAX_LAYERS, nlayers);
    MVF_REQUIRE(xa4 && xb4 && layers && model_mul && K_NA && K_NB && K_NA_spatial && K_NA_sigma2 && PXB && scalars && workspace &&
                    (P || !dense) && ((trows && tvals) || !topk),
                "%s: null pointer", who);
    MVF_REQUIRE(sigma2 > 0.0 && sigma2_variance > 0.0 && spatial_outlier >= 0.0, "%s: need sigma2 > 0, sigma2_variance > 0, outlier >= 0", who);
    const Plan p = make_plan(na, nb);
    TopkPlan tp;
    if (topk) tp = make_topk_plan(p, na, k);
    const size_t need = topk ? tp.total : p.total;
    MVF_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
    DevLayers L;
    L.n = nlayers;
    for (int l = 0; l < nlayers; ++l)
        if (const int rc = check_layer(who, l, layers[l], true, L.l[l])) return rc;
    for (int l = nlayers; l < MAX_LAYERS; ++l) L.l[l] = L.l[0];
    const double h1 = -1.0 / (2.0 * (sigma2 / sigma2_variance)), h2 = -1.0 / (2.0 * sigma2);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MVF_F32)
        return run_assign<float>(st, p, xa4, na, xb4, nb, L, model_mul, h1, h2, spatial_outlier, K_NA, K_NB, K_NA_spatial,
                                 K_NA_sigma2, PXB, scalars, P, topk ? &tp : nullptr, trows, tvals, (char*)workspace);
    return run_assign<double>(st, p, xa4, na, xb4, nb, L, model_mul, h1, h2, spatial_outlier, K_NA, K_NB, K_NA_spatial,
                              K_NA_sigma2, PXB, scalars, P, topk ? &tp : nullptr, trows, tvals, (char*)workspace);
}

// workspace of mvf_assign_layer_stats: part[rsplit][3][nb_pad], colsum[2][nb_pad], the row splits' lists lv / lr[split][k][nb_pad]
struct StatsPlan {
    Plan p;
    int k;  // min(k, na)
    size_t off_part, off_col, off_lv, off_lr, total;
};

StatsPlan make_stats_plan(int64_t na, int64_t nb, int k) {
    StatsPlan t;
    t.p = make_plan(na, nb);
    t.k = (int)std::min<int64_t>(k, na);
    size_t o = 0;
    t.off_part = o, o += align_up((size_t)t.p.rsplit * 3 * t.p.nb_pad * sizeof(double), 256);
    t.off_col = o, o += align_up((size_t)2 * t.p.nb_pad * sizeof(double), 256);
    t.off_lv = o, o += align_up((size_t)t.p.rsplit * t.k * t.p.nb_pad * sizeof(double), 256);
    t.off_lr = o, o += align_up((size_t)t.p.rsplit * t.k * t.p.nb_pad * sizeof(int), 256);
    t.total = o;
    return t;
}

template <typename T>
int run_layer_stats(hipStream_t st, const StatsPlan& t, const DevLayer& ly, int64_t na, int64_t nb, double* cmin, int* rows,
                    double* vals, double* sums, char* ws) {
    const Plan& p = t.p;
    double* part = (double*)(ws + t.off_part);
    double* colsum = (double*)(ws + t.off_col);
    double* lv = (double*)(ws + t.off_lv);
    int* lr = (int*)(ws + t.off_lr);
    const dim3 grid((unsigned)p.ctiles, (unsigned)p.rsplit);
#define MVF_LAYER_STATS(KC) \
    hipLaunchKernelGGL((layer_stats_kernel<T, KC>), grid, dim3(256), 0, st, ly, na, nb, p.rtiles, p.nb_pad, t.k, part, lv, lr)
    if (t.k == 0)
        MVF_LAYER_STATS(0);
    else if (t.k <= 4)  // the lists' LDS is sized by the template, as in pass 1 of mvf_assign_topk
        MVF_LAYER_STATS(4);
    else if (t.k <= 16)
        MVF_LAYER_STATS(16);
    else
        MVF_LAYER_STATS(TOPK_MAX);
#undef MVF_LAYER_STATS
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(layer_stats_columns_kernel, dim3((unsigned)cdiv(nb, 256)), dim3(256), 0, st, part, p.rsplit, nb, p.nb_pad, cmin,
                       colsum);
    MVF_LAUNCH_CHECK();
    for (int q = 0; q < 2; ++q) {
        hipLaunchKernelGGL(assign_sum_kernel, dim3(1), dim3(256), 0, st, colsum + q * p.nb_pad, nb, sums + q);
        MVF_LAUNCH_CHECK();
    }
    if (t.k) {
        hipLaunchKernelGGL(layer_stats_merge_kernel, dim3((unsigned)cdiv(nb, 4)), dim3(256), 0, st, lv, lr, p.rsplit, t.k, nb, p.nb_pad,
                           rows, vals);
        MVF_LAUNCH_CHECK();
    }
    return 0;
}

// ---- mvf_assign_best: the mapping (`get_optimal_mapping_relationship` / `mapping_aligned_coords`, spateo/alignment/utils.py:
// 157-255) without P: per row and per column of P the largest entry and its index under the reference's two tie rules.
// The entry is v_ij = m_i ((e2_ij q_ij) c3_j), the value and the product order of assign_pass2_kernel<T, P2_DENSE>; d_ij is
// sq_dist's.  A state is the head of its set in two total orders at once:
//   nearest  (v descending, d ascending, index ascending)     keep_all=False: among equal maxima the nearest partner
//   first    (v descending, index ascending)                  keep_all=True after the reference's sort and drop-duplicates
// The empty state (-inf, +inf, INT_MAX, INT_MAX) loses against every entry.  Taking the head of a union from the heads of
// its parts is associative and commutative: lanes, halves, tiles and splits may be combined in any order, the bits are the
// same on every call.  Only live rows / columns are ever offered, so an index is in range or INT_MAX (nothing offered, or
// nothing but NaN), which the merge turns into index 0, value 0.
struct Best {
    double v, d;
    int in, ifirst;
};

__device__ __forceinline__ Best best_empty() { return Best{-HUGE_VAL, HUGE_VAL, INT_MAX, INT_MAX}; }

__device__ __forceinline__ void best_combine(Best& s, double v, double d, int in, int ifirst) {
    if (v > s.v) {
        s.v = v, s.d = d, s.in = in, s.ifirst = ifirst;
    } else if (v == s.v) {
        if (d < s.d || (d == s.d && in < s.in)) s.d = d, s.in = in;
        s.ifirst = min(s.ifirst, ifirst);
    }
}

// workspace of mvf_assign_best behind mvf_assign's: K_NB of the factor kernel (not returned), the column splits' row states
// rv / rd [csplit][na_pad], ri [csplit][na_pad][2] and the row splits' column states cv / cd [rsplit][nb_pad], ci [..][2]
struct BestPlan {
    size_t off_knb, off_rv, off_rd, off_ri, off_cv, off_cd, off_ci, total;
};

BestPlan make_best_plan(const Plan& p) {
    BestPlan t;
    size_t o = p.total;
    const size_t nr = (size_t)p.csplit * p.na_pad, nc = (size_t)p.rsplit * p.nb_pad;
    t.off_knb = o, o += align_up((size_t)p.nb_pad * sizeof(double), 256);
    t.off_rv = o, o += align_up(nr * sizeof(double), 256);
    t.off_rd = o, o += align_up(nr * sizeof(double), 256);
    t.off_ri = o, o += align_up(nr * 2 * sizeof(int), 256);
    t.off_cv = o, o += align_up(nc * sizeof(double), 256);
    t.off_cd = o, o += align_up(nc * sizeof(double), 256);
    t.off_ci = o, o += align_up(nc * 2 * sizeof(int), 256);
    t.total = o;
    return t;
}

// ---- the rows' best columns.  Pass 2's grid (row tiles, column splits) and tile walk; a lane keeps the states of its 8 rows
// over the column tiles of its split; bv / bd [split][na_pad], bi [split][na_pad][2]
template <typename T>
__global__ __launch_bounds__(256) void assign_best_rows_kernel(const T* __restrict__ xa4, int64_t na, const T* __restrict__ xb4,
                                                               int64_t nb, DevLayers L, const double* __restrict__ mm, double h2,
                                                               const double* __restrict__ fac, int64_t ctiles, int64_t na_pad,
                                                               double* __restrict__ bv, double* __restrict__ bd,
                                                               int* __restrict__ bi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4, wi = wave >> 1, wj = wave & 1;
    const int64_t i0 = (int64_t)blockIdx.x * AT + 32 * wi;
    const int64_t t_lo = ctiles * blockIdx.y / gridDim.y, t_hi = ctiles * (blockIdx.y + 1) / gridDim.y;
    Point pa[2][4];
    double mi[2][4];
    Best st[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t i = std::min<int64_t>(i0 + 16 * a + lk + 4 * r, na - 1);
            pa[a][r] = load_point(xa4, i), mi[a][r] = mm[i], st[a][r] = best_empty();
        }
    for (int64_t t = t_lo; t < t_hi; ++t) {
        const int64_t j0 = t * AT + 32 * wj;
        f64x4 q[2][2];
        layer_product<T>(L, i0, j0, na, nb, li, lk, q);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int64_t j = j0 + 16 * b + li;  // < nb_pad
            if (j >= nb) continue;               // a padded column is never offered
            const Point cb = load_point(xb4, j);
            const double c3 = fac[4 * j + 2];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double d = sq_dist(pa[a][r], cb);
                    const double v = mi[a][r] * ((exp(d * h2) * q[a][b][r]) * c3);  // P_ij as mvf_assign_dense stores it
                    best_combine(st[a][r], v, d, (int)j, (int)j);
                }
        }
    }
    // the 16 column lanes of a row by a butterfly (the combination is commutative: every lane ends with the same state), then
    // the two column halves of the tile through LDS
    __shared__ double rv[2][AT], rd[2][AT];
    __shared__ int ri[2][AT][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Best s = st[a][r];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                const double ov = __shfl_xor(s.v, o, 64), od = __shfl_xor(s.d, o, 64);
                const int on = __shfl_xor(s.in, o, 64), of = __shfl_xor(s.ifirst, o, 64);
                best_combine(s, ov, od, on, of);
            }
            if (li == 0) {
                const int row = 32 * wi + 16 * a + lk + 4 * r;
                rv[wj][row] = s.v, rd[wj][row] = s.d, ri[wj][row][0] = s.in, ri[wj][row][1] = s.ifirst;
            }
        }
    __syncthreads();
    if (threadIdx.x < AT) {
        const int row = threadIdx.x;
        Best s{rv[0][row], rd[0][row], ri[0][row][0], ri[0][row][1]};
        best_combine(s, rv[1][row], rd[1][row], ri[1][row][0], ri[1][row][1]);
        const int64_t o = (int64_t)blockIdx.y * na_pad + (int64_t)blockIdx.x * AT + row;
        bv[o] = s.v, bd[o] = s.d, bi[2 * o] = s.in, bi[2 * o + 1] = s.ifirst;
    }
}

// ---- the columns' best rows.  Pass 1's grid (column tiles, row splits) and tile walk; a lane keeps the states of its 2
// columns over the row tiles of its split; bv / bd [split][nb_pad], bi [split][nb_pad][2]
template <typename T>
__global__ __launch_bounds__(256) void assign_best_cols_kernel(const T* __restrict__ xa4, int64_t na, const T* __restrict__ xb4,
                                                               int64_t nb, DevLayers L, const double* __restrict__ mm, double h2,
                                                               const double* __restrict__ fac, int64_t rtiles, int64_t nb_pad,
                                                               double* __restrict__ bv, double* __restrict__ bd,
                                                               int* __restrict__ bi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4, wi = wave >> 1, wj = wave & 1;
    const int64_t j0 = (int64_t)blockIdx.x * AT + 32 * wj;
    const int64_t t_lo = rtiles * blockIdx.y / gridDim.y, t_hi = rtiles * (blockIdx.y + 1) / gridDim.y;
    Point cb[2];
    double c3[2];
    Best st[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int64_t j = j0 + 16 * b + li;  // < nb_pad: fac is zero for nb <= j (those columns are not merged)
        cb[b] = load_point(xb4, std::min<int64_t>(j, nb - 1)), c3[b] = fac[4 * j + 2], st[b] = best_empty();
    }
    for (int64_t t = t_lo; t < t_hi; ++t) {
        const int64_t i0 = t * AT + 32 * wi;
        f64x4 q[2][2];
        layer_product<T>(L, i0, j0, na, nb, li, lk, q);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = i0 + 16 * a + lk + 4 * r;
                if (i >= na) continue;  // a padded row is never offered
                const Point pa = load_point(xa4, i);
                const double m = mm[i];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const double d = sq_dist(pa, cb[b]);
                    const double v = m * ((exp(d * h2) * q[a][b][r]) * c3[b]);  // P_ij as mvf_assign_dense stores it
                    best_combine(st[b], v, d, (int)i, (int)i);
                }
            }
    }
    // the 8 (row half, lane group) states of every column through LDS, as pass 1 adds its partial sums
    __shared__ double rv[8][AT], rd[8][AT];
    __shared__ int ri[8][AT][2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int g = wi * 4 + lk, c = 32 * wj + 16 * b + li;
        rv[g][c] = st[b].v, rd[g][c] = st[b].d, ri[g][c][0] = st[b].in, ri[g][c][1] = st[b].ifirst;
    }
    __syncthreads();
    if (threadIdx.x < AT) {
        const int c = threadIdx.x;
        Best s{rv[0][c], rd[0][c], ri[0][c][0], ri[0][c][1]};
#pragma unroll
        for (int g = 1; g < 8; ++g) best_combine(s, rv[g][c], rd[g][c], ri[g][c][0], ri[g][c][1]);
        const int64_t o = (int64_t)blockIdx.y * nb_pad + (int64_t)blockIdx.x * AT + c;
        bv[o] = s.v, bd[o] = s.d, bi[2 * o] = s.in, bi[2 * o + 1] = s.ifirst;
    }
}

// ---- the splits' states of one row / column combined: idx[e] = {nearest, first}, val[e] = the maximum.  `limit`: the size
// of the other side; an index outside [0, limit) - nothing comparable was offered - becomes index 0 with value 0
__global__ __launch_bounds__(256) void assign_best_merge_kernel(const double* __restrict__ bv, const double* __restrict__ bd,
                                                                const int* __restrict__ bi, int64_t nsplit, int64_t n,
                                                                int64_t n_pad, int limit, int* __restrict__ idx,
                                                                double* __restrict__ val) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    Best s = best_empty();
    for (int64_t sp = 0; sp < nsplit; ++sp) {
        const int64_t o = sp * n_pad + e;
        best_combine(s, bv[o], bd[o], bi[2 * o], bi[2 * o + 1]);
    }
    const bool real = s.in >= 0 && s.in < limit && s.ifirst >= 0 && s.ifirst < limit;
    idx[2 * e] = real ? s.in : 0, idx[2 * e + 1] = real ? s.ifirst : 0;
    val[e] = real ? s.v : 0.0;
}

template <typename T>
int run_assign_best(hipStream_t st, const Plan& p, const BestPlan& bp, const void* xa4, int64_t na, const void* xb4, int64_t nb,
                    const DevLayers& L, const double* mm, double h1, double h2, double outlier, int* row_idx, double* row_val,
                    int* col_idx, double* col_val, char* ws) {
    double* part1 = (double*)(ws + p.off_part1);
    double* fac = (double*)(ws + p.off_fac);
    double* K_NB = (double*)(ws + bp.off_knb);
    const dim3 grid1((unsigned)p.ctiles, (unsigned)p.rsplit), grid2((unsigned)p.rtiles, (unsigned)p.csplit);
    hipLaunchKernelGGL((assign_pass1_kernel<T>), grid1, dim3(256), 0, st, (const T*)xa4, na, (const T*)xb4, nb, L, mm, h1, h2,
                       p.rtiles, p.nb_pad, part1);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(assign_factors_kernel, dim3((unsigned)cdiv(p.nb_pad, 256)), dim3(256), 0, st, part1, p.rsplit, nb, p.nb_pad,
                       outlier, fac, K_NB);
    MVF_LAUNCH_CHECK();
    if (row_idx) {
        double* bv = (double*)(ws + bp.off_rv);
        double* bd = (double*)(ws + bp.off_rd);
        int* bi = (int*)(ws + bp.off_ri);
        hipLaunchKernelGGL((assign_best_rows_kernel<T>), grid2, dim3(256), 0, st, (const T*)xa4, na, (const T*)xb4, nb, L, mm, h2,
                           fac, p.ctiles, p.na_pad, bv, bd, bi);
        MVF_LAUNCH_CHECK();
        hipLaunchKernelGGL(assign_best_merge_kernel, dim3((unsigned)cdiv(na, 256)), dim3(256), 0, st, bv, bd, bi, p.csplit, na,
                           p.na_pad, (int)nb, row_idx, row_val);
        MVF_LAUNCH_CHECK();
    }
    if (col_idx) {
        double* bv = (double*)(ws + bp.off_cv);
        double* bd = (double*)(ws + bp.off_cd);
        int* bi = (int*)(ws + bp.off_ci);
        hipLaunchKernelGGL((assign_best_cols_kernel<T>), grid1, dim3(256), 0, st, (const T*)xa4, na, (const T*)xb4, nb, L, mm, h2,
                           fac, p.rtiles, p.nb_pad, bv, bd, bi);
        MVF_LAUNCH_CHECK();
        hipLaunchKernelGGL(assign_best_merge_kernel, dim3((unsigned)cdiv(nb, 256)), dim3(256), 0, st, bv, bd, bi, p.rsplit, nb,
                           p.nb_pad, (int)na, col_idx, col_val);
        MVF_LAUNCH_CHECK();
    }
    return 0;
}

// ---- mvf_assign_apply: P @ FB and P^T @ FA without P.  One sweep kernel for both directions, on pass 1's tile walk: grid
// (column tiles, row splits) of a SWEEP problem whose rows carry the features and whose columns receive the product,
//   SWAP = false  rows = A cells, columns = B cells:  out^T = FA^T P      (to_B = P^T @ FA; pass 1's grid as it is)
//   SWAP = true   rows = B cells, columns = A cells:  out^T = FB^T P^T    (to_A = P @ FB; the operands exchanged - layers
//                 Xp <-> Yp and a <-> b, a label layer's table read transposed - as mvf_assign_layer_stats' row statistics are).
// layer_product and the spatial factor leave p = P[row i0 + 16 a + lk + 4 r][column j0 + 16 b + li] in lane (li, lk), which for
// fixed (a, r) IS the B operand B[k = lk][n = li] of v_mfma_f64_16x16x4_f64 over the 4 rows i0 + 16 a + 4 r + (0 .. 3); the A
// operand A[m = li][k = lk] = F[that row][16 c + li] is 16 consecutive doubles per lane group, and the accumulator
// D[m = lk + 4 r'][n = li] = out^T[feature 16 c + lk + 4 r'][column j0 + 16 b + li]: no shuffle, no transpose of P.  CB column
// blocks of 16 features (at most 4: 32 accumulator doubles per lane).  The entry is the value mvf_assign_dense stores,
// m ((e2 q) c3), in that product order under either SWAP.  A padded row has p = 0 and F = 0; a padded column has factor 0.
// The two row halves of the workgroup meet in LDS, which also turns the tile round: part[split][column][16 CB] is written in
// whole rows.  ksum (may be NULL): the columns' sums of p, kpart[split][nc_pad] - K_NA under SWAP.
template <typename T, int CB, bool SWAP>
__global__ __launch_bounds__(256) void assign_apply_kernel(const T* __restrict__ xr4, int64_t nr, const T* __restrict__ xc4,
                                                           int64_t nc, DevLayers L, const double* __restrict__ rowfac,
                                                           int64_t rstride, const double* __restrict__ colfac, int64_t cstride,
                                                           double h2, const double* __restrict__ F, int64_t ldf, int cw,
                                                           int64_t rtiles, int64_t nc_pad, double* __restrict__ part,
                                                           double* __restrict__ kpart) {
    constexpr int W = 16 * CB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4, wi = wave >> 1, wj = wave & 1;
    const int64_t j0 = (int64_t)blockIdx.x * AT + 32 * wj;
    const int64_t t_lo = rtiles * blockIdx.y / gridDim.y, t_hi = rtiles * (blockIdx.y + 1) / gridDim.y;
    Point cb[2];
    double cf[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int64_t j = j0 + 16 * b + li;
        cb[b] = load_point(xc4, std::min<int64_t>(j, nc - 1));
        cf[b] = j < nc ? colfac[j * cstride] : 0.0;
    }
    f64x4 acc[CB][2];
#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[c][b] = f64x4{0.0, 0.0, 0.0, 0.0};
    double ks[2] = {0.0, 0.0};
    for (int64_t t = t_lo; t < t_hi; ++t) {
        const int64_t i0 = t * AT + 32 * wi;
        f64x4 q[2][2];
        if (SWAP)
            layer_product<T, true>(L, i0, j0, nr, nc, li, lk, q);
        else
            layer_product<T, false>(L, i0, j0, nr, nc, li, lk, q);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = i0 + 16 * a + lk + 4 * r;
                const bool live = i < nr;
                const int64_t ic = live ? i : nr - 1;
                const Point pa = load_point(xr4, ic);
                const double rf = live ? rowfac[ic * rstride] : 0.0;
                double f[CB];
#pragma unroll
                for (int c = 0; c < CB; ++c) f[c] = live && 16 * c + li < cw ? F[ic * ldf + 16 * c + li] : 0.0;
                double p[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const double d = sq_dist(pa, cb[b]);
                    const double eq = exp(d * h2) * q[a][b][r];
                    p[b] = SWAP ? cf[b] * (eq * rf) : rf * (eq * cf[b]);  // P_ij as mvf_assign_dense stores it
                    ks[b] += p[b];
                }
#pragma unroll
                for (int c = 0; c < CB; ++c)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[c][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[c], p[b], acc[c][b], 0, 0, 0);
            }
    }
    __shared__ double red[AT][W + 1];
    __shared__ double kred[8][AT];
#pragma unroll
    for (int b = 0; b < 2; ++b) kred[wi * 4 + lk][32 * wj + 16 * b + li] = ks[b];
    if (wi == 1) {
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[32 * wj + 16 * b + li][16 * c + lk + 4 * r] = acc[c][b][r];
    }
    __syncthreads();
    if (wi == 0) {
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double& x = red[32 * wj + 16 * b + li][16 * c + lk + 4 * r];
                    x = acc[c][b][r] + x;
                }
    }
    __syncthreads();
    double* out = part + ((int64_t)blockIdx.y * nc_pad + (int64_t)blockIdx.x * AT) * W;
    for (int e = threadIdx.x; e < AT * W; e += 256) out[e] = red[e / W][e % W];
    if (kpart && threadIdx.x < AT) {
        double tot = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) tot += kred[g][threadIdx.x];
        kpart[(int64_t)blockIdx.y * nc_pad + (int64_t)blockIdx.x * AT + threadIdx.x] = tot;
    }
}

// the splits' partial products added in split order: out[j][c0 + c] for j < n, c < cw (part[split][n_pad][W])
__global__ __launch_bounds__(256) void assign_apply_reduce_kernel(const double* __restrict__ part, int64_t nsplit, int64_t n,
                                                                  int64_t n_pad, int W, int cw, double* __restrict__ out,
                                                                  int64_t ldo) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * cw) return;
    const int64_t j = e / cw;
    const int c = (int)(e % cw);
    double s = 0.0;
    for (int64_t sp = 0; sp < nsplit; ++sp) s += part[(sp * n_pad + j) * W + c];
    out[j * ldo + c] = s;
}

// the splits' column sums added in split order
__global__ __launch_bounds__(256) void assign_apply_ksum_kernel(const double* __restrict__ kpart, int64_t nsplit, int64_t n,
                                                                int64_t n_pad, double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int64_t sp = 0; sp < nsplit; ++sp) s += kpart[sp * n_pad + j];
    out[j] = s;
}

constexpr int APPLY_CHUNK = 64;  // feature columns per sweep

int apply_width(int c) { return 16 * (int)std::min<int64_t>(APPLY_CHUNK / 16, cdiv(c, 16)); }  // 0 for c == 0

// workspace of mvf_assign_apply: pass 1's partials and the factors (mvf_assign's offsets), K_NB when it is not returned, the
// sweeps' partial products (one buffer, both directions and every chunk in turn) and the partial K_NA
struct ApplyPlan {
    size_t off_knb, off_part, off_kpart, total;
};

ApplyPlan make_apply_plan(const Plan& p, int cb, int ca) {
    ApplyPlan t;
    size_t o = p.off_part2;  // (pass 2's partials are not needed)
    t.off_knb = o, o += align_up((size_t)p.nb_pad * sizeof(double), 256);
    const size_t to_a = (size_t)p.csplit * p.na_pad * apply_width(cb), to_b = (size_t)p.rsplit * p.nb_pad * apply_width(ca);
    t.off_part = o, o += align_up(std::max(to_a, to_b) * sizeof(double), 256);
    t.off_kpart = o, o += align_up((size_t)p.csplit * p.na_pad * sizeof(double), 256);
    t.total = o;
    return t;
}

// one direction: the chunks of F (n_rows x c, ld ldf) swept one after the other into out (n_cols x c, dense)
template <typename T, bool SWAP>
int run_apply_direction(hipStream_t st, const void* xr4, int64_t nr, const void* xc4, int64_t nc, const DevLayers& L,
                        const double* rowfac, int64_t rstride, const double* colfac, int64_t cstride, double h2, const double* F,
                        int c, int64_t ldf, double* out, int64_t rtiles, int64_t ctiles, int64_t nsplit, int64_t nc_pad,
                        double* part, double* kpart, double* ksum) {
    const dim3 grid((unsigned)ctiles, (unsigned)nsplit);
    for (int c0 = 0; c0 < c; c0 += APPLY_CHUNK) {
        const int cw = std::min(APPLY_CHUNK, c - c0), W = apply_width(cw);
        double* kp = c0 == 0 && ksum ? kpart : nullptr;
#define MVF_APPLY(CB)                                                                                                          \
    hipLaunchKernelGGL((assign_apply_kernel<T, CB, SWAP>), grid, dim3(256), 0, st, (const T*)xr4, nr, (const T*)xc4, nc, L, rowfac, \
                       rstride, colfac, cstride, h2, F + c0, ldf, cw, rtiles, nc_pad, part, kp)
        if (W == 16)
            MVF_APPLY(1);
        else if (W == 32)
            MVF_APPLY(2);
        else if (W == 48)
            MVF_APPLY(3);
        else
            MVF_APPLY(4);
#undef MVF_APPLY
        MVF_LAUNCH_CHECK();
        hipLaunchKernelGGL(assign_apply_reduce_kernel, dim3((unsigned)cdiv(nc * cw, 256)), dim3(256), 0, st, part, nsplit, nc, nc_pad,
                           W, cw, out + c0, (int64_t)c);
        MVF_LAUNCH_CHECK();
        if (kp) {
            hipLaunchKernelGGL(assign_apply_ksum_kernel, dim3((unsigned)cdiv(nc, 256)), dim3(256), 0, st, kp, nsplit, nc, nc_pad, ksum);
            MVF_LAUNCH_CHECK();
        }
    }
    return 0;
}

template <typename T>
int run_assign_apply(hipStream_t st, const Plan& p, const ApplyPlan& ap, const void* xa4, int64_t na, const void* xb4, int64_t nb,
                     const DevLayers& L, const double* mm, double h1, double h2, double outlier, const double* FB, int cb,
                     int64_t ldfb, double* to_A, const double* FA, int ca, int64_t ldfa, double* to_B, double* K_NA, double* K_NB,
                     char* ws) {
    double* part1 = (double*)(ws + p.off_part1);
    double* fac = (double*)(ws + p.off_fac);
    double* part = (double*)(ws + ap.off_part);
    double* kpart = (double*)(ws + ap.off_kpart);
    if (!K_NB) K_NB = (double*)(ws + ap.off_knb);
    hipLaunchKernelGGL((assign_pass1_kernel<T>), dim3((unsigned)p.ctiles, (unsigned)p.rsplit), dim3(256), 0, st, (const T*)xa4, na,
                       (const T*)xb4, nb, L, mm, h1, h2, p.rtiles, p.nb_pad, part1);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(assign_factors_kernel, dim3((unsigned)cdiv(p.nb_pad, 256)), dim3(256), 0, st, part1, p.rsplit, nb, p.nb_pad,
                       outlier, fac, K_NB);
    MVF_LAUNCH_CHECK();
    if (to_B)  // rows = A cells (factor m_i), columns = B cells (factor c3_j = fac[4 j + 2]; zero for the padded ones)
        if (const int rc = run_apply_direction<T, false>(st, xa4, na, xb4, nb, L, mm, 1, fac + 2, 4, h2, FA, ca, ldfa, to_B, p.rtiles,
                                                         p.ctiles, p.rsplit, p.nb_pad, part, kpart, nullptr))
            return rc;
    if (to_A) {  // the operands exchanged: rows = B cells (factor c3_j), columns = A cells (factor m_i)
        DevLayers Ls = L;
        for (int l = 0; l < MAX_LAYERS; ++l) {
            if (Ls.l[l].post != POST_LABEL) std::swap(Ls.l[l].X, Ls.l[l].Y);  // (a label layer: X stays the table, read transposed)
            std::swap(Ls.l[l].a, Ls.l[l].b);
        }
        if (const int rc = run_apply_direction<T, true>(st, xb4, nb, xa4, na, Ls, fac + 2, 4, mm, 1, h2, FB, cb, ldfb, to_A, p.ctiles,
                                                        p.rtiles, p.csplit, p.na_pad, part, kpart, K_NA))
            return rc;
    }
    return 0;
}

}  // namespace
}  // namespace mvf

using namespace mvf;

extern "C" int64_t mvf_assign_padded_features(int64_t g, int metric) {
    if (g <= 0 || metric < MVF_ASSIGN_EUC || metric > MVF_ASSIGN_COS) return 0;
    return padded_features(g, metric);
}

extern "C" int mvf_assign_prepare(const double* layer, int64_t n, int64_t g, int metric, int side, void* Lp, int64_t ld,
                                  double* ab, mvf_dtype dtype, void* stream) {
    if (n == 0) return 0;
    MVF_REQUIRE(n > 0 && g > 0, "mvf_assign_prepare: need n >= 0 and g > 0");
    MVF_REQUIRE(metric >= MVF_ASSIGN_EUC && metric <= MVF_ASSIGN_COS, "mvf_assign_prepare: bad metric %d", metric);
    MVF_REQUIRE(side == 0 || side == 1, "mvf_assign_prepare: side must be 0 (A) or 1 (B)");
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "mvf_assign_prepare: bad dtype %d", (int)dtype);
    MVF_REQUIRE(ld == padded_features(g, metric), "mvf_assign_prepare: ld must be mvf_assign_padded_features(g, metric)");
    MVF_REQUIRE(layer && Lp && ab, "mvf_assign_prepare: null pointer");
    MVF_REQUIRE(cdiv(n, 4) < ((int64_t)1 << 31), "mvf_assign_prepare: too many cells");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MVF_F32)
        hipLaunchKernelGGL(assign_prepare_kernel<float>, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, st, layer, n, g, metric, side,
                           (float*)Lp, ld, ab);
    else
        hipLaunchKernelGGL(assign_prepare_kernel<double>, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, st, layer, n, g, metric, side,
                           (double*)Lp, ld, ab);
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t mvf_assign_prepare_csr_min_workspace_bytes(int64_t g) {
    if (g <= 0) return 0;
    return (size_t)g * 4 * sizeof(double);  // one block: four waves, one staging row each
}

extern "C" int mvf_assign_prepare_csr(const int64_t* indptr, const int32_t* indices, const void* data, int data_is_f32, int64_t n,
                                      int64_t g, int metric, int side, void* Lp, int64_t ld, double* ab, void* workspace,
                                      size_t workspace_bytes, mvf_dtype dtype, void* stream) {
    if (n == 0) return 0;
    MVF_REQUIRE(n > 0 && g > 0, "mvf_assign_prepare_csr: need n >= 0 and g > 0");
    MVF_REQUIRE(g < ((int64_t)1 << 31), "mvf_assign_prepare_csr: column indices are int32, g must be below 2^31");
    MVF_REQUIRE(metric >= MVF_ASSIGN_EUC && metric <= MVF_ASSIGN_COS, "mvf_assign_prepare_csr: bad metric %d", metric);
    MVF_REQUIRE(side == 0 || side == 1, "mvf_assign_prepare_csr: side must be 0 (A) or 1 (B)");
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "mvf_assign_prepare_csr: bad dtype %d", (int)dtype);
    MVF_REQUIRE(ld == padded_features(g, metric), "mvf_assign_prepare_csr: ld must be mvf_assign_padded_features(g, metric)");
    MVF_REQUIRE(indptr && indices && data && Lp && ab && workspace, "mvf_assign_prepare_csr: null pointer");
    const size_t row_bytes = (size_t)g * sizeof(double);
    MVF_REQUIRE(workspace_bytes >= 4 * row_bytes, "mvf_assign_prepare_csr: workspace of %zu bytes, need %zu", workspace_bytes,
                4 * row_bytes);
    MVF_REQUIRE(((uintptr_t)workspace & 7) == 0, "mvf_assign_prepare_csr: the workspace must be 8-byte aligned");
    // as many blocks (of four staging rows) as fit, no more than the rows ask for and than keep the device busy
    int64_t blocks = (int64_t)(workspace_bytes / (4 * row_bytes));
    blocks = std::min(blocks, std::min(cdiv(n, 4), (int64_t)CSR_MAX_BLOCKS));
    hipStream_t st = (hipStream_t)stream;
    MVF_CHECK_HIP(hipMemsetAsync(workspace, 0, (size_t)blocks * 4 * row_bytes, st));
    const dim3 grid((unsigned)blocks), block(256);
#define MVF_PREPARE_CSR(T, V)                                                                                                    \
    hipLaunchKernelGGL((assign_prepare_csr_kernel<T, V>), grid, block, 0, st, indptr, indices, (const V*)data, n, g, metric, side, \
                       (T*)Lp, ld, ab, (double*)workspace)
    if (dtype == MVF_F32) {
        if (data_is_f32)
            MVF_PREPARE_CSR(float, float);
        else
            MVF_PREPARE_CSR(float, double);
    } else {
        if (data_is_f32)
            MVF_PREPARE_CSR(double, float);
        else
            MVF_PREPARE_CSR(double, double);
    }
#undef MVF_PREPARE_CSR
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" int mvf_assign_label_prepare(const int32_t* labels, int64_t n, int64_t classes, double* ab, void* stream) {
    if (n == 0) return 0;
    MVF_REQUIRE(n > 0 && cdiv(n, 256) < ((int64_t)1 << 31), "mvf_assign_label_prepare: bad cell count");
    MVF_REQUIRE(classes >= 1 && classes < ((int64_t)1 << 31), "mvf_assign_label_prepare: need 1 <= classes < 2^31, got %lld",
                (long long)classes);
    MVF_REQUIRE(labels && ab, "mvf_assign_label_prepare: null pointer");
    hipLaunchKernelGGL(assign_label_prepare_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, labels, n,
                       (int)classes, ab);
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t mvf_assign_workspace_bytes(int64_t na, int64_t nb) {
    if (na <= 0 || nb <= 0) return 0;
    return make_plan(na, nb).total;
}

extern "C" int mvf_assign(const void* xa4, int64_t na, const void* xb4, int64_t nb, const mvf_assign_layer* layers, int nlayers,
                          const double* model_mul, double sigma2, double sigma2_variance, double spatial_outlier, double* K_NA,
                          double* K_NB, double* K_NA_spatial, double* K_NA_sigma2, double* PXB, double* scalars, void* workspace,
                          size_t workspace_bytes, mvf_dtype dtype, void* stream) {
    return assign_entry("mvf_assign", xa4, na, xb4, nb, layers, nlayers, model_mul, sigma2, sigma2_variance, spatial_outlier, K_NA,
                        K_NB, K_NA_spatial, K_NA_sigma2, PXB, scalars, nullptr, false, 0, nullptr, nullptr, workspace, workspace_bytes,
                        dtype, stream);
}

extern "C" int mvf_assign_dense(const void* xa4, int64_t na, const void* xb4, int64_t nb, const mvf_assign_layer* layers,
                                int nlayers, const double* model_mul, double sigma2, double sigma2_variance,
                                double spatial_outlier, double* K_NA, double* K_NB, double* K_NA_spatial, double* K_NA_sigma2,
                                double* PXB, double* scalars, double* P, void* workspace, size_t workspace_bytes, mvf_dtype dtype,
                                void* stream) {
    return assign_entry("mvf_assign_dense", xa4, na, xb4, nb, layers, nlayers, model_mul, sigma2, sigma2_variance, spatial_outlier,
                        K_NA, K_NB, K_NA_spatial, K_NA_sigma2, PXB, scalars, P, true, 0, nullptr, nullptr, workspace, workspace_bytes,
                        dtype, stream);
}

extern "C" size_t mvf_assign_topk_workspace_bytes(int64_t na, int64_t nb, int k) {
    if (na <= 0 || nb <= 0 || k < 1 || k > TOPK_MAX) return 0;
    return make_topk_plan(make_plan(na, nb), na, k).total;
}

extern "C" int mvf_assign_topk(const void* xa4, int64_t na, const void* xb4, int64_t nb, const mvf_assign_layer* layers,
                               int nlayers, const double* model_mul, double sigma2, double sigma2_variance,
                               double spatial_outlier, int k, double* K_NA, double* K_NB, double* K_NA_spatial,
                               double* K_NA_sigma2, double* PXB, double* scalars, int32_t* rows, double* vals, void* workspace,
                               size_t workspace_bytes, mvf_dtype dtype, void* stream) {
    MVF_REQUIRE(k >= 1 && k <= TOPK_MAX, "mvf_assign_topk: need 1 <= k <= %d, got %d", TOPK_MAX, k);
    return assign_entry("mvf_assign_topk", xa4, na, xb4, nb, layers, nlayers, model_mul, sigma2, sigma2_variance, spatial_outlier,
                        K_NA, K_NB, K_NA_spatial, K_NA_sigma2, PXB, scalars, nullptr, false, k, rows, vals, workspace,
                        workspace_bytes, dtype, stream);
}

extern "C" size_t mvf_assign_layer_stats_workspace_bytes(int64_t na, int64_t nb, int k) {
    if (na <= 0 || nb <= 0 || k < 0 || k > TOPK_MAX) return 0;
    return make_stats_plan(na, nb, k).total;
}

extern "C" int mvf_assign_layer_stats(const mvf_assign_layer* layer, int64_t na, int64_t nb, int k, double* cmin, int32_t* rows,
                                      double* vals, double* sums, void* workspace, size_t workspace_bytes, mvf_dtype dtype,
                                      void* stream) {
    const char* who = "mvf_assign_layer_stats";
    MVF_REQUIRE(k >= 0 && k <= TOPK_MAX, "%s: need 0 <= k <= %d, got %d", who, TOPK_MAX, k);
    MVF_REQUIRE(na >= 1 && nb >= 1, "%s: need na >= 1 and nb >= 1", who);
    MVF_REQUIRE(na < ((int64_t)1 << 31) && nb < ((int64_t)1 << 31), "%s: too many cells", who);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "%s: bad dtype %d", who, (int)dtype);
    MVF_REQUIRE(layer && cmin && sums && workspace && ((rows && vals) || k == 0), "%s: null pointer", who);
    DevLayer ly;
    if (const int rc = check_layer(who, 0, *layer, false, ly)) return rc;
    const StatsPlan t = make_stats_plan(na, nb, k);
    MVF_REQUIRE(workspace_bytes >= t.total, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, t.total);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MVF_F32) return run_layer_stats<float>(st, t, ly, na, nb, cmin, rows, vals, sums, (char*)workspace);
    return run_layer_stats<double>(st, t, ly, na, nb, cmin, rows, vals, sums, (char*)workspace);
}

extern "C" size_t mvf_assign_best_workspace_bytes(int64_t na, int64_t nb) {
    if (na <= 0 || nb <= 0) return 0;
    return make_best_plan(make_plan(na, nb)).total;
}

extern "C" int mvf_assign_best(const void* xa4, int64_t na, const void* xb4, int64_t nb, const mvf_assign_layer* layers,
                               int nlayers, const double* model_mul, double sigma2, double sigma2_variance,
                               double spatial_outlier, int32_t* row_idx, double* row_val, int32_t* col_idx, double* col_val,
                               void* workspace, size_t workspace_bytes, mvf_dtype dtype, void* stream) {
    const char* who = "mvf_assign_best";
    MVF_REQUIRE((row_idx != nullptr) == (row_val != nullptr), "%s: row_idx and row_val must both be given or both be NULL", who);
    MVF_REQUIRE((col_idx != nullptr) == (col_val != nullptr), "%s: col_idx and col_val must both be given or both be NULL", who);
    MVF_REQUIRE(row_idx || col_idx, "%s: nothing to compute: the row pair and the column pair are both NULL", who);
    if (na == 0 || nb == 0) return 0;
    MVF_REQUIRE(na > 0 && nb > 0, "%s: negative size", who);
    MVF_REQUIRE(na < ((int64_t)1 << 31) && nb < ((int64_t)1 << 31), "%s: too many cells", who);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "%s: bad dtype %d", who, (int)dtype);
    MVF_REQUIRE(nlayers >= 1 && nlayers <= MAX_LAYERS, "%s: need 1 .. %d layers, got %d", who, MAX_LAYERS, nlayers);
    MVF_REQUIRE(xa4 && xb4 && layers && model_mul && workspace, "%s: null pointer", who);
    MVF_REQUIRE(sigma2 > 0.0 && sigma2_variance > 0.0 && spatial_outlier >= 0.0, "%s: need sigma2 > 0, sigma2_variance > 0, outlier >= 0", who);
    const Plan p = make_plan(na, nb);
    const BestPlan bp = make_best_plan(p);
    MVF_REQUIRE(workspace_bytes >= bp.total, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, bp.total);
    DevLayers L;
    L.n = nlayers;
    for (int l = 0; l < nlayers; ++l)
        if (const int rc = check_layer(who, l, layers[l], true, L.l[l])) return rc;
    for (int l = nlayers; l < MAX_LAYERS; ++l) L.l[l] = L.l[0];
    const double h1 = -1.0 / (2.0 * (sigma2 / sigma2_variance)), h2 = -1.0 / (2.0 * sigma2);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MVF_F32)
        return run_assign_best<float>(st, p, bp, xa4, na, xb4, nb, L, model_mul, h1, h2, spatial_outlier, row_idx, row_val, col_idx,
                                      col_val, (char*)workspace);
    return run_assign_best<double>(st, p, bp, xa4, na, xb4, nb, L, model_mul, h1, h2, spatial_outlier, row_idx, row_val, col_idx,
                                   col_val, (char*)workspace);
}

extern "C" size_t mvf_assign_apply_workspace_bytes(int64_t na, int64_t nb, int cb, int ca) {
    if (na <= 0 || nb <= 0 || cb < 0 || ca < 0) return 0;
    return make_apply_plan(make_plan(na, nb), cb, ca).total;
}

extern "C" int mvf_assign_apply(const void* xa4, int64_t na, const void* xb4, int64_t nb, const mvf_assign_layer* layers,
                                int nlayers, const double* model_mul, double sigma2, double sigma2_variance,
                                double spatial_outlier, const double* FB, int cb, int64_t ldfb, double* to_A, const double* FA,
                                int ca, int64_t ldfa, double* to_B, double* K_NA, double* K_NB, void* workspace,
                                size_t workspace_bytes, mvf_dtype dtype, void* stream) {
    const char* who = "mvf_assign_apply";
    const bool row_dir = FB && to_A && cb >= 1, col_dir = FA && to_B && ca >= 1;
    MVF_REQUIRE(row_dir || (!FB && !to_A && cb == 0), "%s: FB, cb >= 1 and to_A must all be given, or NULL / 0 to skip P @ FB", who);
    MVF_REQUIRE(col_dir || (!FA && !to_B && ca == 0), "%s: FA, ca >= 1 and to_B must all be given, or NULL / 0 to skip P^T @ FA", who);
    MVF_REQUIRE(row_dir || col_dir, "%s: nothing to compute: both directions are skipped", who);
    MVF_REQUIRE(!K_NA || row_dir, "%s: K_NA rides with P @ FB, which is skipped", who);
    MVF_REQUIRE((!row_dir || ldfb >= cb) && (!col_dir || ldfa >= ca), "%s: a feature matrix's ld is below its column count", who);
    if (na == 0 || nb == 0) return 0;
    MVF_REQUIRE(na > 0 && nb > 0, "%s: negative size", who);
    MVF_REQUIRE(na < ((int64_t)1 << 31) && nb < ((int64_t)1 << 31), "%s: too many cells", who);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "%s: bad dtype %d", who, (int)dtype);
    MVF_REQUIRE(nlayers >= 1 && nlayers <= MAX_LAYERS, "%s: need 1 .. %d layers, got %d", who, MAX_LAYERS, nlayers);
    MVF_REQUIRE(xa4 && xb4 && layers && model_mul && workspace, "%s: null pointer", who);
    MVF_REQUIRE(sigma2 > 0.0 && sigma2_variance > 0.0 && spatial_outlier >= 0.0, "%s: need sigma2 > 0, sigma2_variance > 0, outlier >= 0", who);
    const Plan p = make_plan(na, nb);
    const ApplyPlan ap = make_apply_plan(p, cb, ca);
    MVF_REQUIRE(workspace_bytes >= ap.total, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, ap.total);
    DevLayers L;
    L.n = nlayers;
    for (int l = 0; l < nlayers; ++l)
        if (const int rc = check_layer(who, l, layers[l], true, L.l[l])) return rc;
    for (int l = nlayers; l < MAX_LAYERS; ++l) L.l[l] = L.l[0];
    const double h1 = -1.0 / (2.0 * (sigma2 / sigma2_variance)), h2 = -1.0 / (2.0 * sigma2);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MVF_F32)
        return run_assign_apply<float>(st, p, ap, xa4, na, xb4, nb, L, model_mul, h1, h2, spatial_outlier, FB, cb, ldfb, to_A, FA, ca,
                                       ldfa, to_B, K_NA, K_NB, (char*)workspace);
    return run_assign_apply<double>(st, p, ap, xa4, na, xb4, nb, L, model_mul, h1, h2, spatial_outlier, FB, cb, ldfb, to_A, FA, ca,
                                    ldfa, to_B, K_NA, K_NB, (char*)workspace);
}
