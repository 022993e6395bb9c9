// PCA across slices on the kernel-value cache: the cache Ublk[g/16][n][16] of mvf_gram.hip filled from DATA (a cells x genes
// matrix, centred by its column means) instead of from con_K, so that mvf_gram_cached (TILES | REDUCE, P = 1) is the
// covariance's Gram matrix Xc^T Xc and mvf_apply_cached (C = the leading eigenvectors) the scores Xc V.
//
// Reference: `group_pca` (spateo/alignment/utils.py:88-149) concatenates the slices and runs scanpy's PCA on them; here the
// slices are packed one behind the other into ONE cache (rows offset by `row0`), no concatenated copy is made.
//   * colsum_kernel: per-column sums over fixed blocks of CM_ROWS GLOBAL rows (row0 + i), one lane per (block, column), the
//     rows of a block added in row order; a slice that starts inside a block continues the block's partial sum where the
//     previous slice left it.  colmean_kernel adds the blocks in block order.  So the means depend on the stacked matrix
//     alone - not on where it is cut into slices or CSR staging chunks -, there are no atomics, and two calls give the same bits.
//   * ublk_pack_kernel: (T)((double)x[i][j] - mu[j]) at cache position ((j / 16) * n_pad + row0 + i) * 16 + j % 16; one 16-byte
//     store per lane, 16 / 8 cells x 64 / 128 contiguous bytes per store instruction.  Columns g .. roundup(g, 128) are written
//     as zeros with the rows; the call that ends at n_total also zeroes the rows n_total .. roundup(n_total, 256).
//   * CSR input: chunks of rows are expanded into a caller-provided staging area (zeroed, then one wave per row scatters its
//     entries; a column outside [0, g) is skipped, never used as an address) and go through the two dense kernels above with
//     the chunk's row offset: the same bits as the dense entry points give for the densified matrix, whatever the staging size.
#include "mvf_common.h"

namespace mvf {

constexpr int PUB = 16;         // == UB of mvf_gram.hip: columns per cache block
constexpr int PCHUNK = 256;     // == GCHUNK: the cache pads the rows to a multiple of this
constexpr int PGT = 128;        // == GT: ... and the columns to a multiple of this
constexpr int CM_ROWS = 1024;   // global rows per partial column sum
constexpr int64_t CSR_CHUNK_MAX_ROWS = 1 << 20;  // rows per staging chunk at most (bounds the expansion's grid)

static inline int64_t pca_npad(int64_t n) { return cdiv(n, PCHUNK) * PCHUNK; }
static inline int64_t pca_mpad(int64_t g) { return cdiv(g, PGT) * PGT; }

// partial[b][col] for the global row blocks b = row0 / CM_ROWS + blockIdx.x that this slice (global rows row0 .. row0 + n) meets
template <typename V>
__global__ __launch_bounds__(256) void colsum_kernel(const V* __restrict__ x, int64_t n, int64_t g, int64_t row0,
                                                     double* __restrict__ partial) {
    const int64_t col = (int64_t)blockIdx.y * 256 + threadIdx.x;
    if (col >= g) return;
    const int64_t b = row0 / CM_ROWS + blockIdx.x;
    const int64_t lo = max(b * CM_ROWS, row0), hi = min((b + 1) * CM_ROWS, row0 + n);  // global rows of this block in this slice
    if (lo >= hi) return;
    double acc = lo > b * CM_ROWS ? partial[b * g + col] : 0.0;  // an earlier slice began this block
    const V* p = x + (lo - row0) * g + col;
    int64_t r = lo;
    for (; r + 8 <= hi; r += 8, p += 8 * g) {  // eight loads in flight, added in row order
        V v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = p[q * g];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc += (double)v[q];
    }
    for (; r < hi; ++r, p += g) acc += (double)p[0];
    partial[b * g + col] = acc;
}

__global__ __launch_bounds__(256) void colmean_kernel(const double* __restrict__ partial, int64_t nblocks, int64_t g, int64_t n_total,
                                                      double* __restrict__ mean) {
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= g) return;
    double acc = 0.0;
    for (int64_t b = 0; b < nblocks; ++b) acc += partial[b * g + col];
    mean[col] = acc / (double)n_total;
}

// cache rows row0 .. cell_end (cell_end = row0 + n, or n_pad for the slice that ends the matrix), all padded columns
template <typename T, typename V>
__global__ __launch_bounds__(256) void ublk_pack_kernel(const V* __restrict__ x, int64_t n, int64_t g, const double* __restrict__ mu,
                                                        int64_t row0, int64_t cell_end, int64_t n_pad, T* __restrict__ ublk) {
    constexpr int PER = 16 / sizeof(T);  // elements per 16-byte store
    constexpr int LPC = PUB / PER;       // lanes per cell and cache block
    constexpr int CPB = 256 / LPC;       // cells per workgroup
    typedef T vec_t __attribute__((ext_vector_type(PER)));
    const int part = threadIdx.x % LPC;
    const int64_t i = (int64_t)blockIdx.x * CPB + threadIdx.x / LPC;  // row of this slice
    const int64_t cell = row0 + i;
    if (cell >= cell_end) return;
    const int64_t cb = blockIdx.y, col0 = cb * PUB + part * PER;
    vec_t o;
#pragma unroll
    for (int jj = 0; jj < PER; ++jj) {
        const int64_t col = col0 + jj;
        T v = T(0);
        if (i < n && col < g) {
            double d = (double)x[i * g + col];
            if (mu) d -= mu[col];
            v = (T)d;
        }
        o[jj] = v;
    }
    *reinterpret_cast<vec_t*>(ublk + (cb * n_pad + cell) * PUB + part * PER) = o;
}

// rows r0 .. r0 + rows of the CSR matrix into stage[rows][g] (zeroed by the caller): one wave per row
template <typename V>
__global__ __launch_bounds__(256) void csr_expand_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                         const V* __restrict__ data, int64_t r0, int64_t rows, int64_t g,
                                                         V* __restrict__ stage) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= rows) return;
    const int64_t e0 = indptr[r0 + k], e1 = indptr[r0 + k + 1];
    for (int64_t e = e0 + lane; e < e1; e += 64) {
        const int64_t c = indices[e];
        if (c >= 0 && c < g) stage[k * g + c] = data[e];
    }
}

static size_t colmeans_ws_bytes(int64_t n_total, int64_t g) { return (size_t)cdiv(n_total, CM_ROWS) * (size_t)g * sizeof(double); }

// the arguments both mean entry points share; `who` names the caller in the message
static int check_colmeans(const char* who, int64_t n, int64_t g, int64_t n_total, int64_t row0, const double* mean,
                          const void* workspace, size_t workspace_bytes) {
    MVF_REQUIRE(n > 0 && g > 0, "%s: need n > 0 and g > 0", who);
    MVF_REQUIRE(row0 >= 0 && n_total > 0 && row0 <= n_total - n, "%s: rows %lld .. %lld are not inside 0 .. n_total = %lld", who,
                (long long)row0, (long long)(row0 + n), (long long)n_total);
    MVF_REQUIRE(cdiv(g, 256) <= 65535, "%s: g too large", who);
    MVF_REQUIRE(cdiv(n_total, CM_ROWS) < ((int64_t)1 << 31), "%s: n_total too large", who);
    MVF_REQUIRE(workspace && (row0 + n < n_total || mean), "%s: null pointer", who);
    MVF_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: the workspace must be 8-byte aligned", who);
    MVF_REQUIRE(workspace_bytes >= colmeans_ws_bytes(n_total, g), "%s: workspace too small (%zu < %zu)", who, workspace_bytes,
                colmeans_ws_bytes(n_total, g));
    return 0;
}

static int check_pack(const char* who, int64_t n, int64_t g, int64_t n_total, int64_t row0, const void* ublk, size_t ublk_bytes,
                      mvf_dtype dtype) {
    MVF_REQUIRE(n > 0 && g > 0, "%s: need n > 0 and g > 0", who);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "%s: bad dtype %d", who, (int)dtype);
    MVF_REQUIRE(row0 >= 0 && n_total > 0 && row0 <= n_total - n, "%s: rows %lld .. %lld are not inside 0 .. n_total = %lld", who,
                (long long)row0, (long long)(row0 + n), (long long)n_total);
    MVF_REQUIRE(pca_mpad(g) / PUB <= 65535, "%s: g too large", who);
    MVF_REQUIRE(pca_npad(n_total) / 32 < ((int64_t)1 << 31), "%s: n_total too large", who);
    MVF_REQUIRE(ublk, "%s: null pointer", who);
    MVF_REQUIRE(((uintptr_t)ublk & 15) == 0, "%s: the cache must be 16-byte aligned", who);
    const size_t need = mvf_ublk_bytes(n_total, g, dtype);
    MVF_REQUIRE(ublk_bytes >= need, "%s: buffer too small (%zu < %zu)", who, ublk_bytes, need);
    return 0;
}

template <typename V>
static void launch_colsum(hipStream_t st, const V* x, int64_t n, int64_t g, int64_t row0, double* partial) {
    const int64_t nb = (row0 + n - 1) / CM_ROWS - row0 / CM_ROWS + 1;
    hipLaunchKernelGGL(colsum_kernel<V>, dim3((unsigned)nb, (unsigned)cdiv(g, 256)), dim3(256), 0, st, x, n, g, row0, partial);
}

static void launch_colmean(hipStream_t st, const double* partial, int64_t g, int64_t n_total, double* mean) {
    hipLaunchKernelGGL(colmean_kernel, dim3((unsigned)cdiv(g, 256)), dim3(256), 0, st, partial, cdiv(n_total, CM_ROWS), g, n_total,
                       mean);
}

template <typename T, typename V>
static void launch_pack(hipStream_t st, const V* x, int64_t n, int64_t g, const double* mu, int64_t n_total, int64_t row0, T* ublk) {
    constexpr int CPB = 256 / (PUB / (16 / (int)sizeof(T)));
    const int64_t n_pad = pca_npad(n_total);
    const int64_t cell_end = row0 + n == n_total ? n_pad : row0 + n;
    hipLaunchKernelGGL((ublk_pack_kernel<T, V>), dim3((unsigned)cdiv(cell_end - row0, CPB), (unsigned)(pca_mpad(g) / PUB)), dim3(256),
                       0, st, x, n, g, mu, row0, cell_end, n_pad, ublk);
}

template <typename V>
static void launch_pack_any(hipStream_t st, const V* x, int64_t n, int64_t g, const double* mu, int64_t n_total, int64_t row0,
                            void* ublk, mvf_dtype dtype) {
    if (dtype == MVF_F32)
        launch_pack<float, V>(st, x, n, g, mu, n_total, row0, (float*)ublk);
    else
        launch_pack<double, V>(st, x, n, g, mu, n_total, row0, (double*)ublk);
}

// rows of one staging chunk: what fits, at most CSR_CHUNK_MAX_ROWS
static int64_t staging_rows(size_t staging_bytes, int64_t g, size_t itemsize) {
    return std::min<int64_t>(CSR_CHUNK_MAX_ROWS, (int64_t)(staging_bytes / ((size_t)g * itemsize)));
}

static int check_csr(const char* who, const void* indptr, const void* indices, const void* data, int64_t g, const void* staging,
                     size_t staging_bytes, size_t itemsize) {
    MVF_REQUIRE(g < ((int64_t)1 << 31), "%s: column indices are int32, g must be below 2^31", who);
    MVF_REQUIRE(indptr && indices && data && staging, "%s: null pointer", who);
    MVF_REQUIRE(((uintptr_t)staging & 7) == 0, "%s: the staging area must be 8-byte aligned", who);
    MVF_REQUIRE(staging_bytes >= (size_t)g * itemsize, "%s: staging area of %zu bytes, one expanded row needs %zu", who, staging_bytes,
                (size_t)g * itemsize);
    return 0;
}

template <typename V, typename F>
static int for_each_csr_chunk(hipStream_t st, const int64_t* indptr, const int32_t* indices, const V* data, int64_t n, int64_t g,
                              V* stage, size_t staging_bytes, F&& body) {
    const int64_t rows_max = staging_rows(staging_bytes, g, sizeof(V));
    for (int64_t r0 = 0; r0 < n; r0 += rows_max) {
        const int64_t rows = std::min(rows_max, n - r0);
        MVF_CHECK_HIP(hipMemsetAsync(stage, 0, (size_t)rows * (size_t)g * sizeof(V), st));
        hipLaunchKernelGGL(csr_expand_kernel<V>, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, st, indptr, indices, data, r0, rows, g,
                           stage);
        body(r0, rows);
        MVF_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace mvf

using namespace mvf;

extern "C" size_t mvf_colmeans_workspace_bytes(int64_t n_total, int64_t g) {
    if (n_total <= 0 || g <= 0) return 0;
    return colmeans_ws_bytes(n_total, g);
}

extern "C" int mvf_colmeans(const void* x, int x_is_f32, int64_t n, int64_t g, int64_t n_total, int64_t row0, double* mean,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_colmeans("mvf_colmeans", n, g, n_total, row0, mean, workspace, workspace_bytes)) return rc;
    MVF_REQUIRE(x, "mvf_colmeans: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (x_is_f32)
        launch_colsum<float>(st, (const float*)x, n, g, row0, (double*)workspace);
    else
        launch_colsum<double>(st, (const double*)x, n, g, row0, (double*)workspace);
    if (row0 + n == n_total) launch_colmean(st, (const double*)workspace, g, n_total, mean);
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" int mvf_ublk_pack(const void* x, int x_is_f32, int64_t n, int64_t g, const double* mu, int64_t n_total, int64_t row0,
                             void* ublk, size_t ublk_bytes, mvf_dtype dtype, void* stream) {
    if (int rc = check_pack("mvf_ublk_pack", n, g, n_total, row0, ublk, ublk_bytes, dtype)) return rc;
    MVF_REQUIRE(x, "mvf_ublk_pack: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (x_is_f32)
        launch_pack_any<float>(st, (const float*)x, n, g, mu, n_total, row0, ublk, dtype);
    else
        launch_pack_any<double>(st, (const double*)x, n, g, mu, n_total, row0, ublk, dtype);
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" int mvf_colmeans_csr(const int64_t* indptr, const int32_t* indices, const void* data, int data_is_f32, int64_t n,
                                int64_t g, int64_t n_total, int64_t row0, double* mean, void* workspace, size_t workspace_bytes,
                                void* staging, size_t staging_bytes, void* stream) {
    if (int rc = check_colmeans("mvf_colmeans_csr", n, g, n_total, row0, mean, workspace, workspace_bytes)) return rc;
    if (int rc = check_csr("mvf_colmeans_csr", indptr, indices, data, g, staging, staging_bytes, data_is_f32 ? 4 : 8)) return rc;
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)workspace;
    int rc;
    if (data_is_f32)
        rc = for_each_csr_chunk<float>(st, indptr, indices, (const float*)data, n, g, (float*)staging, staging_bytes,
                                       [&](int64_t r0, int64_t rows) { launch_colsum<float>(st, (const float*)staging, rows, g, row0 + r0, partial); });
    else
        rc = for_each_csr_chunk<double>(st, indptr, indices, (const double*)data, n, g, (double*)staging, staging_bytes,
                                        [&](int64_t r0, int64_t rows) { launch_colsum<double>(st, (const double*)staging, rows, g, row0 + r0, partial); });
    if (rc) return rc;
    if (row0 + n == n_total) launch_colmean(st, partial, g, n_total, mean);
    MVF_LAUNCH_CHECK();
    return 0;
}

extern "C" int mvf_ublk_pack_csr(const int64_t* indptr, const int32_t* indices, const void* data, int data_is_f32, int64_t n,
                                 int64_t g, const double* mu, int64_t n_total, int64_t row0, void* ublk, size_t ublk_bytes,
                                 void* staging, size_t staging_bytes, mvf_dtype dtype, void* stream) {
    if (int rc = check_pack("mvf_ublk_pack_csr", n, g, n_total, row0, ublk, ublk_bytes, dtype)) return rc;
    if (int rc = check_csr("mvf_ublk_pack_csr", indptr, indices, data, g, staging, staging_bytes, data_is_f32 ? 4 : 8)) return rc;
    hipStream_t st = (hipStream_t)stream;
    // a chunk is a slice of its own: rows row0 + r0 .. of n_total (the chunk that ends the matrix zeroes the padding rows)
    if (data_is_f32)
        return for_each_csr_chunk<float>(st, indptr, indices, (const float*)data, n, g, (float*)staging, staging_bytes,
                                         [&](int64_t r0, int64_t rows) { launch_pack_any<float>(st, (const float*)staging, rows, g, mu, n_total, row0 + r0, ublk, dtype); });
    return for_each_csr_chunk<double>(st, indptr, indices, (const double*)data, n, g, (double*)staging, staging_bytes,
                                      [&](int64_t r0, int64_t rows) { launch_pack_any<double>(st, (const double*)staging, rows, g, mu, n_total, row0 + r0, ublk, dtype); });
}
