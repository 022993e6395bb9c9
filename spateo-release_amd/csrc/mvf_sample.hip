// Down-sampling of a slice to n representative cells: the topology-representing network (TRN), k-means, and the exact nearest
// row that turns either's nodes into cell indices.  Float64 throughout, whatever the package's cell dtype: the samplers return
// INDICES, and one wrong rank or label moves a node by a visible fraction of a cell spacing.
//
// Reference: spateo/alignment/methods/sampling.py - `TRNET.run` / `runOnce` (:103-155: a Python loop over the nodes inside a
// loop of 200 n steps), `trn` (:196-222), `sample_by_kmeans` (:243-260: scipy.cluster.vq.kmeans2 + a nearest-neighbour query).
//   * trn_kernel: ONE workgroup per problem, every step of it inside the kernel.  The nodes live in registers (four per lane at
//     4096 nodes), the squared distances to the step's sample go to LDS as order-preserving 64-bit keys, a bitonic network sorts
//     the (key, node) pairs there - a strict total order, the lower node first among equal distances, so the network's
//     instability cannot show - and every node reads its rank back.  (A variant that kept the pairs in registers - partners
//     inside a wave by shuffles, in the same lane directly, only the distances 64 .. 512 through LDS - compares every pair twice
//     and measured 29.1 us per step against this one's 27.0 at 2000 nodes: fewer barriers did not pay.
//     profiles/downsampling.md.)  Only X[p_idx[t]] and three schedule values are fetched per step, one step ahead
//     (the row index two steps ahead).  The workgroup waits on nothing another workgroup writes.
//   * nearest_kernel: one lane per query row, the candidate rows streamed through LDS in tiles (every lane reads the same row:
//     a broadcast); candidates in rising index and a strict `<`, so the smallest index wins among equal distances.  Candidates
//     are cut into at most NEAR_MAX_CHUNKS chunks (grid.y); with more than one chunk the per-chunk winners are combined in chunk
//     order by nearest_reduce_kernel.  k-means' assignment is the same kernel with the cells as queries and the centroids as rows.
//   * k-means' update: ksum_kernel has one lane per CLUSTER scan the labels of a fixed block of rows (a function of N alone) in
//     row order and add its members; kupdate_kernel adds the blocks in block order and divides.  No atomics: two runs give the
//     same bits.  A cluster without members keeps its centroid.
// Every sum of squares is ((d0 d0) + d1 d1) + d2 d2 with -ffp-contract=off: the reference's column order, no fused multiply-add.
#include <cmath>

#include "mvf_common.h"

namespace mvf {

constexpr int TRN_MAX_NODES = MVF_TRN_MAX_NODES;
constexpr int TRN_THREADS = 1024;
constexpr int TRN_PER = TRN_MAX_NODES / TRN_THREADS;  // nodes per lane at the cap
constexpr int TRN_MAX_BATCH = 32;                     // problems per launch: their records travel as the kernel's argument
constexpr int NEAR_THREADS = 256;                     // queries per workgroup == rows per LDS tile
constexpr int64_t NEAR_MIN_CHUNK = 4096;              // candidate rows per chunk at least
constexpr int64_t NEAR_MAX_CHUNKS = 1024;
constexpr int64_t KM_MIN_ROWS = 1024;                 // rows per partial cluster sum at least (== the LDS tile of ksum_kernel)
constexpr int64_t KM_MAX_BLOCKS = 256;

struct TrnBatch {
    mvf_trn_problem p[TRN_MAX_BATCH];
};

__device__ __forceinline__ int64_t clamp_row(int64_t r, int64_t N) { return r < 0 ? 0 : (r >= N ? N - 1 : r); }

__global__ __launch_bounds__(TRN_THREADS) void trn_kernel(TrnBatch batch) {
    __shared__ unsigned long long key[TRN_MAX_NODES];
    __shared__ unsigned short node[TRN_MAX_NODES];
    __shared__ unsigned short rank[TRN_MAX_NODES];
    const mvf_trn_problem& pr = batch.p[blockIdx.x];
    const double* __restrict__ X = pr.X;
    const int64_t* __restrict__ p_idx = pr.p_idx;
    const double* __restrict__ sl = pr.l;
    const double* __restrict__ sep = pr.ep;
    const double* __restrict__ skc = pr.kc;
    const int64_t N = pr.N, T = pr.T;
    const int n = (int)pr.n, d = (int)pr.d, tid = threadIdx.x;
    int P = 2;  // the network's size: the power of two that holds the nodes
    while (P < n) P <<= 1;

    double w[TRN_PER][3], D[TRN_PER][3];
#pragma unroll
    for (int q = 0; q < TRN_PER; ++q) {
        const int i = tid + q * TRN_THREADS;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            w[q][c] = 0.0;  // (columns d .. 2 stay zero: they add +0 to the sum of squares and nothing to the node)
            D[q][c] = 0.0;
        }
        if (i < n) {
            const int64_t r = clamp_row(pr.w_idx[i], N);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (c < d) w[q][c] = X[r * d + c];
        }
    }
    double pn[3] = {0.0, 0.0, 0.0};  // the sample of the step to come
    int64_t r2 = 0;                  // ... and the row of the one after it
    if (T > 0) {
        const int64_t r1 = clamp_row(p_idx[0], N);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (c < d) pn[c] = X[r1 * d + c];
    }
    if (T > 1) r2 = clamp_row(p_idx[1], N);

    for (int64_t t = 0; t < T; ++t) {
        const double p0 = pn[0], p1 = pn[1], p2 = pn[2];
        const double l = sl[t], ep = sep[t], kc = skc ? skc[t] : 0.0;
        if (t + 1 < T) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (c < d) pn[c] = X[r2 * d + c];
        }
        if (t + 2 < T) r2 = clamp_row(p_idx[t + 2], N);
#pragma unroll
        for (int q = 0; q < TRN_PER; ++q) {
            const int i = tid + q * TRN_THREADS;
            if (i < P) {
                unsigned long long kbits = ~0ull;  // padding sorts behind every node
                if (i < n) {
                    D[q][0] = p0 - w[q][0];
                    D[q][1] = p1 - w[q][1];
                    D[q][2] = p2 - w[q][2];
                    double s = D[q][0] * D[q][0];
                    s = s + D[q][1] * D[q][1];
                    s = s + D[q][2] * D[q][2];
                    kbits = (unsigned long long)__double_as_longlong(s);  // s >= +0: the bit pattern orders like the value
                }
                key[i] = kbits;
                node[i] = (unsigned short)i;
            }
        }
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int e = tid; e < (P >> 1); e += TRN_THREADS) {
                    const int a = ((e & ~(j - 1)) << 1) | (e & (j - 1)), b = a | j;
                    const unsigned long long ka = key[a], kb = key[b];
                    const unsigned short na = node[a], nb = node[b];
                    const bool greater = ka > kb || (ka == kb && na > nb);
                    if (greater == ((a & k) == 0)) {
                        key[a] = kb;
                        key[b] = ka;
                        node[a] = nb;
                        node[b] = na;
                    }
                }
                __syncthreads();
            }
        }
        for (int r = tid; r < n; r += TRN_THREADS) rank[node[r]] = (unsigned short)r;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < TRN_PER; ++q) {
            const int i = tid + q * TRN_THREADS;
            if (i < n) {
                const double k = (double)rank[i];
                if (!skc || k < kc) {
                    const double f = ep * exp(-k / l);
                    w[q][0] += f * D[q][0];
                    w[q][1] += f * D[q][1];
                    w[q][2] += f * D[q][2];
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < TRN_PER; ++q) {
        const int i = tid + q * TRN_THREADS;
        if (i < n) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (c < d) pr.W[(int64_t)i * d + c] = w[q][c];
        }
    }
}

static inline int64_t near_chunk(int64_t nr) { return std::max(NEAR_MIN_CHUNK, cdiv(cdiv(nr, NEAR_MAX_CHUNKS), NEAR_THREADS) * NEAR_THREADS); }
static inline int64_t near_chunks(int64_t nr) { return cdiv(nr, near_chunk(nr)); }
static inline size_t near_ws_bytes(int64_t nr, int64_t nq) {
    const int64_t nc = near_chunks(nr);
    return nc > 1 ? (size_t)nc * (size_t)nq * 16 : 0;
}

// queries Q (nq x D), candidate rows R (nr x D): chunk blockIdx.y of the rows against queries blockIdx.x * 256 ..
template <int D, typename OutT>
__global__ __launch_bounds__(NEAR_THREADS) void nearest_kernel(const double* __restrict__ Q, int64_t nq, const double* __restrict__ R,
                                                               int64_t nr, int64_t chunk, double* __restrict__ part_d,
                                                               int64_t* __restrict__ part_i, OutT* __restrict__ out) {
    __shared__ double tile[NEAR_THREADS * D];
    const int tid = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * NEAR_THREADS + tid;
    const int64_t lo = (int64_t)blockIdx.y * chunk, hi = min(lo + chunk, nr);
    double x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = q < nq ? Q[q * D + c] : 0.0;
    double best = INFINITY;
    int64_t bi = lo;
    for (int64_t base = lo; base < hi; base += NEAR_THREADS) {
        const int cnt = (int)min((int64_t)NEAR_THREADS, hi - base);
        __syncthreads();
        for (int e = tid; e < cnt * D; e += NEAR_THREADS) tile[e] = R[base * D + e];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            double df = x[0] - tile[j * D];
            double s = df * df;
#pragma unroll
            for (int c = 1; c < D; ++c) {
                df = x[c] - tile[j * D + c];
                s = s + df * df;
            }
            if (s < best) {
                best = s;
                bi = base + j;
            }
        }
    }
    if (q >= nq) return;
    if (gridDim.y == 1) {
        out[q] = (OutT)bi;
    } else {
        part_d[(int64_t)blockIdx.y * nq + q] = best;
        part_i[(int64_t)blockIdx.y * nq + q] = bi;
    }
}

template <typename OutT>
__global__ __launch_bounds__(NEAR_THREADS) void nearest_reduce_kernel(const double* __restrict__ part_d, const int64_t* __restrict__ part_i,
                                                                      int64_t nq, int64_t nchunks, OutT* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * NEAR_THREADS + threadIdx.x;
    if (q >= nq) return;
    double best = part_d[q];
    int64_t bi = part_i[q];
    for (int64_t c = 1; c < nchunks; ++c) {
        const double v = part_d[c * nq + q];
        if (v < best) {
            best = v;
            bi = part_i[c * nq + q];
        }
    }
    out[q] = (OutT)bi;
}

template <typename OutT>
static void launch_nearest(hipStream_t st, const double* Q, int64_t nq, const double* R, int64_t nr, int d, void* ws, OutT* out) {
    const int64_t chunk = near_chunk(nr), nc = near_chunks(nr);
    double* pd = (double*)ws;
    int64_t* pi = (int64_t*)(pd + (nc > 1 ? nc * nq : 0));
    const dim3 grid((unsigned)cdiv(nq, NEAR_THREADS), (unsigned)nc), block(NEAR_THREADS);
    if (d == 1)
        hipLaunchKernelGGL((nearest_kernel<1, OutT>), grid, block, 0, st, Q, nq, R, nr, chunk, pd, pi, out);
    else if (d == 2)
        hipLaunchKernelGGL((nearest_kernel<2, OutT>), grid, block, 0, st, Q, nq, R, nr, chunk, pd, pi, out);
    else
        hipLaunchKernelGGL((nearest_kernel<3, OutT>), grid, block, 0, st, Q, nq, R, nr, chunk, pd, pi, out);
    if (nc > 1)
        hipLaunchKernelGGL(nearest_reduce_kernel<OutT>, dim3((unsigned)cdiv(nq, NEAR_THREADS)), block, 0, st, pd, pi, nq, nc, out);
}

static inline int64_t km_rows(int64_t N) { return std::max(KM_MIN_ROWS, cdiv(cdiv(N, KM_MAX_BLOCKS), KM_MIN_ROWS) * KM_MIN_ROWS); }
static inline int64_t km_blocks(int64_t N) { return cdiv(N, km_rows(N)); }

// partial[b][c][0 .. 2] = sum of the rows of block b = blockIdx.y with label c, in row order; [3] = their number
template <int D>
__global__ __launch_bounds__(256) void ksum_kernel(const double* __restrict__ X, int64_t N, const int32_t* __restrict__ labels,
                                                   int64_t n, int64_t rows, double* __restrict__ partial) {
    __shared__ double tx[KM_MIN_ROWS * D];
    __shared__ int32_t tl[KM_MIN_ROWS];
    const int tid = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * 256 + tid;
    const int64_t lo = (int64_t)blockIdx.y * rows, hi = min(lo + rows, N);
    double s[3] = {0.0, 0.0, 0.0}, cnt = 0.0;
    for (int64_t base = lo; base < hi; base += KM_MIN_ROWS) {
        const int m = (int)min(KM_MIN_ROWS, hi - base);
        __syncthreads();
        for (int e = tid; e < m * D; e += 256) tx[e] = X[base * D + e];
        for (int e = tid; e < m; e += 256) tl[e] = labels[base + e];
        __syncthreads();
        for (int j = 0; j < m; ++j) {
            if (tl[j] == (int32_t)c) {
#pragma unroll
                for (int k = 0; k < D; ++k) s[k] += tx[j * D + k];
                cnt += 1.0;
            }
        }
    }
    if (c >= n) return;
    double* o = partial + ((int64_t)blockIdx.y * n + c) * 4;
    o[0] = s[0];
    o[1] = s[1];
    o[2] = s[2];
    o[3] = cnt;
}

__global__ __launch_bounds__(256) void kupdate_kernel(const double* __restrict__ partial, int64_t nblocks, int64_t n, int d,
                                                      double* __restrict__ C, int64_t* __restrict__ counts) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    double s[3] = {0.0, 0.0, 0.0}, cnt = 0.0;
    for (int64_t b = 0; b < nblocks; ++b) {
        const double* o = partial + (b * n + c) * 4;
        s[0] += o[0];
        s[1] += o[1];
        s[2] += o[2];
        cnt += o[3];
    }
    counts[c] = (int64_t)cnt;
    if (cnt > 0.0)
        for (int k = 0; k < d; ++k) C[c * d + k] = s[k] / cnt;
}

static size_t kmeans_ws_bytes(int64_t N, int64_t n) { return (size_t)km_blocks(N) * (size_t)n * 32 + near_ws_bytes(n, N); }

static int check_points(const char* who, const void* X, int64_t N, int d, const void* Q, int64_t n, const void* out) {
    MVF_REQUIRE(N > 0 && n > 0, "%s: need N > 0 and n > 0", who);
    MVF_REQUIRE(d >= 1 && d <= 3, "%s: d must be 1, 2 or 3, got %d", who, d);
    MVF_REQUIRE(N < ((int64_t)1 << 38) && n < ((int64_t)1 << 38), "%s: too many rows", who);
    MVF_REQUIRE(X && Q && out, "%s: null pointer", who);
    return 0;
}

}  // namespace mvf

using namespace mvf;

extern "C" int mvf_trn(const mvf_trn_problem* problems, int nproblems, void* stream) {
    if (nproblems == 0) return 0;
    MVF_REQUIRE(nproblems > 0 && problems, "mvf_trn: %d problems at a null pointer", nproblems);
    for (int i = 0; i < nproblems; ++i) {
        const mvf_trn_problem& p = problems[i];
        MVF_REQUIRE(p.n >= 0 && p.n <= TRN_MAX_NODES, "mvf_trn: problem %d has %lld nodes, at most %d are supported", i, (long long)p.n,
                    TRN_MAX_NODES);
        if (p.n == 0) continue;
        MVF_REQUIRE(p.N > 0 && p.T >= 0, "mvf_trn: problem %d needs N > 0 and T >= 0", i);
        MVF_REQUIRE(p.d >= 1 && p.d <= 3, "mvf_trn: problem %d: d must be 1, 2 or 3, got %lld", i, (long long)p.d);
        MVF_REQUIRE(p.X && p.w_idx && p.W, "mvf_trn: problem %d: null pointer", i);
        MVF_REQUIRE(p.T == 0 || (p.p_idx && p.l && p.ep), "mvf_trn: problem %d: null schedule", i);
    }
    hipStream_t st = (hipStream_t)stream;
    TrnBatch batch;
    int nb = 0;
    for (int i = 0; i <= nproblems; ++i) {
        if (i < nproblems && problems[i].n > 0) batch.p[nb++] = problems[i];
        if (nb == TRN_MAX_BATCH || (i == nproblems && nb > 0)) {
            hipLaunchKernelGGL(trn_kernel, dim3((unsigned)nb), dim3(TRN_THREADS), 0, st, batch);
            MVF_LAUNCH_CHECK();
            nb = 0;
        }
    }
    return 0;
}

extern "C" size_t mvf_nearest_rows_workspace_bytes(int64_t N, int64_t n) {
    if (N <= 0 || n <= 0) return 0;
    return near_ws_bytes(N, n);
}

extern "C" int mvf_nearest_rows(const double* X, int64_t N, int d, const double* Q, int64_t n, int64_t* idx, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (n == 0) return 0;
    if (int rc = check_points("mvf_nearest_rows", X, N, d, Q, n, idx)) return rc;
    const size_t need = near_ws_bytes(N, n);
    MVF_REQUIRE(need == 0 || workspace, "mvf_nearest_rows: null workspace");
    MVF_REQUIRE(((uintptr_t)workspace & 7) == 0, "mvf_nearest_rows: the workspace must be 8-byte aligned");
    MVF_REQUIRE(workspace_bytes >= need, "mvf_nearest_rows: workspace too small (%zu < %zu)", workspace_bytes, need);
    launch_nearest<int64_t>((hipStream_t)stream, Q, n, X, N, d, workspace, idx);
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t mvf_kmeans_workspace_bytes(int64_t N, int64_t n) {
    if (N <= 0 || n <= 0) return 0;
    return kmeans_ws_bytes(N, n);
}

extern "C" int mvf_kmeans(const double* X, int64_t N, int d, double* C, int64_t n, int iter, int32_t* labels, int64_t* counts,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (N == 0 || n == 0) return 0;
    if (int rc = check_points("mvf_kmeans", X, N, d, C, n, labels)) return rc;
    MVF_REQUIRE(iter >= 1, "mvf_kmeans: iter must be at least 1, got %d", iter);
    MVF_REQUIRE(n < ((int64_t)1 << 31), "mvf_kmeans: labels are int32, n must be below 2^31");
    MVF_REQUIRE(cdiv(n, 256) <= 0x7fffffff && km_blocks(N) <= 65535, "mvf_kmeans: too many rows");
    MVF_REQUIRE(counts && workspace, "mvf_kmeans: null pointer");
    MVF_REQUIRE(((uintptr_t)workspace & 7) == 0, "mvf_kmeans: the workspace must be 8-byte aligned");
    const size_t need = kmeans_ws_bytes(N, n);
    MVF_REQUIRE(workspace_bytes >= need, "mvf_kmeans: workspace too small (%zu < %zu)", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const int64_t rows = km_rows(N), nb = km_blocks(N);
    double* partial = (double*)workspace;
    void* near_ws = partial + nb * n * 4;
    const dim3 sgrid((unsigned)cdiv(n, 256), (unsigned)nb);
    for (int it = 0; it < iter; ++it) {
        launch_nearest<int32_t>(st, X, N, C, n, d, near_ws, labels);
        if (d == 1)
            hipLaunchKernelGGL(ksum_kernel<1>, sgrid, dim3(256), 0, st, X, N, labels, n, rows, partial);
        else if (d == 2)
            hipLaunchKernelGGL(ksum_kernel<2>, sgrid, dim3(256), 0, st, X, N, labels, n, rows, partial);
        else
            hipLaunchKernelGGL(ksum_kernel<3>, sgrid, dim3(256), 0, st, X, N, labels, n, rows, partial);
        hipLaunchKernelGGL(kupdate_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, partial, nb, n, d, C, counts);
        MVF_LAUNCH_CHECK();
    }
    return 0;
}
