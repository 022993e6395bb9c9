/*
 * mvf.h -- C ABI of libmvf.so, the MI355X (gfx950) morphometric vector-field engine.
 *
 * This is the drop-in boundary for ONE hot path of aristoteleo/spateo-release: the SparseVFC kernel regression
 * under spateo.tdr (con_K -> EM loop -> coefficient solve -> differential-geometry evaluators).  The reference has
 * no native code and no FFI for this path (SURVEY.md "Three facts", section 8b): its arithmetic lives in Python
 * (third-party `dynamo` + in-tree twins).  Each entry point below therefore cites the reference *Python* interface
 * it replaces (file:line under /root/reference); INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.  All data pointers are DEVICE pointers
 *     (hipMalloc'd by the caller, e.g. torch tensors' data_ptr()); the library never allocates or frees memory
 *     and never takes ownership.  Workspaces are caller-provided and sized by the *_workspace_bytes queries.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Every call is asynchronous on it.
 *   - `dtype` selects the arithmetic of the cell-sized arrays: MVF_F32 or MVF_F64.  Reductions, the Gram matrix,
 *     the coefficient solve and the coefficients C are always float64.
 *   - Row-major, dense, no strides.  Cell coordinates / displacements use the padded layout "x4": n rows of
 *     4 elements (x, y, z, 0) so that one lane loads one cell with a single 16/32-byte access; 2-D data sets z = 0.
 *   - Return value: 0 = ok; non-zero = error, message in mvf_last_error() (thread-local).  No exceptions cross
 *     the boundary.  The Python host raises RuntimeError on a non-zero status.
 *   - State: the library has no global or per-process state (mvf_last_error's thread-local buffer, a per-device cache
 *     of the CU count and the developer options of mvf_debug_option - all at their defaults unless that entry point is
 *     called - aside), and it never reads the environment.  Whatever must survive between calls lives in CALLER-provided memory and is named at
 *     the entry point that uses it: the workspace of mvf_solve_minnorm_lr keeps the pivot order of its last finished
 *     factorisation (the next call's hint), the workspaces of the two minimum-norm solves keep their decomposition for
 *     `reuse` calls and mvf_pinv_diag, `basis` keeps the eigenvectors of mvf_solve_minnorm for its warm start.  A fresh
 *     (or overwritten) workspace simply means no hint / no reuse.  The one opaque object is the `mvf_comm` handle of the
 *     multi-GPU exchange (an RCCL communicator, created and destroyed by the caller; libmvf.so links librccl for it).
 */
#ifndef MVF_H
#define MVF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { MVF_F32 = 0, MVF_F64 = 1 } mvf_dtype;

/* evaluator output selection flags for mvf_eval */
enum {
    MVF_EVAL_V = 1,        /* v(x)                      n x 3            */
    MVF_EVAL_JAC = 2,      /* Jacobian                  (3, 3, n) layout */
    MVF_EVAL_DIV = 4,      /* divergence = trace J      n                */
    MVF_EVAL_CURL = 8,     /* curl 3-vector             n x 3            */
    MVF_EVAL_ACC = 16,     /* acceleration a = J v      n x 3            */
    MVF_EVAL_CURV = 32,    /* curvature vector (f. 2)   n x 3            */
    MVF_EVAL_TORS = 64,    /* torsion 3-vector          n x 3            */
    MVF_EVAL_JDET = 128    /* det J                     n                */
};

/* ---- library ------------------------------------------------------------------------------------------------ */
const char* mvf_last_error(void);
int mvf_version(void);                 /* ABI version, currently 7 */
/* mvf_read_back (ABI 7): blocking device -> host copy of a small status block on `stream` (everything enqueued on the stream
 * before it is complete when it returns) - the one host read of an EM iteration (statistics, solver status, sum P r). */
int mvf_read_back(void* dst_host, const void* src_device, size_t nbytes, void* stream);
/* Developer options, process-wide: which kernel variant / launch plan is taken in A/B measurements and in the tests that
 * compare the variants bit for bit.  The library NEVER reads the environment (rounds 1 - 3 had getenv knobs in launch
 * paths); nothing but this call changes its behaviour.  value 0 = default.  Ten names (round 6 removed four that no test
 * or measurement used any more): "conk_form" (1 rows, 2 flat, 3 2d), "slice_len" (cells per Gram slice), "solve_small_off"
 * (1: the blocked multi-launch Cholesky at every m), "lr_no_deflate" (1: mvf_solve_minnorm_lrd always takes the Jacobi path),
 * "defl_block" (64 / 128 / 256: mvf_solve_minnorm_lrd tries that block size alone), "defl_apps" (1 .. 8: applications of
 * S2^-1 in its block inverse iteration), "lr_no_direct" (1: mvf_solve_minnorm_lrd never takes its direct form),
 * "direct_accept" (v > 0: the direct form accepts at most v - 1 deflated directions), "lr_timing" (1: phase times of
 * mvf_solve_minnorm_lr on stderr), "gram_reg_cols" (1: the float32 cached Gram tile stage takes gram_cached_kernel<float>, every
 * wave widening its own column operands, instead of the kernel that shares them through LDS; 2 / 3: the sharing kernel with one
 * workgroup per job / with persistent workgroups, whatever the number of jobs).  Unknown name: non-zero return.  mvf_debug_option_get returns -1 for an unknown name. */
int mvf_debug_option(const char* name, long long value);
long long mvf_debug_option_get(const char* name);
int mvf_device_count(int* count);      /* number of visible HIP devices (0 without a GPU) */

/* ---- preprocessing: sorted unique rows -------------------------------------------------------------------------------
 * Replaces: `tmp_X, uid = np.unique(X, axis=0, return_index=True)` of dynamo SparseVFC (same
 * call in-tree: spateo/alignment/methods/morpho_class.py:845).  X: n x d float64 row-major (finite).  Outputs (device,
 * caller-allocated for n rows): uid[0..count) = index of the FIRST occurrence of each distinct row, in lexicographic row
 * order; rows[0..count) = those rows; count[0] = number of distinct rows.  Stable LSD radix sort over the columns
 * (hand-written from round 4 on: 8-bit passes of per-chunk histograms, a table scan and a ballot-ranked stable scatter;
 * rounds 2 - 3 called rocPRIM here) + run flags + a ballot-ranked compaction; bit-identical to NumPy for finite input. */
size_t mvf_unique_rows_workspace_bytes(int64_t n, int d);
int mvf_unique_rows(const double* X, int64_t n, int d, int64_t* uid, double* rows, int64_t* count, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- preprocessing: kNN bandwidth -------------------------------------------------------------------------------------
 * Replaces the neighbour search of dynamo `bandwidth_selector` (exact kNN with
 * k = max(2, int(0.2 m)) neighbours incl. the point itself, `d = mean(dist[:, 1:]) / 1.5`, `h = sqrt(2) d`).
 * X: m x d float64 row-major (device), 1 <= m <= 8192, d <= 8.  rowsum[i] (device, m float64) = sum of the distances from
 * point i to its k - 1 nearest OTHER points; the caller takes mean = sum(rowsum) / (m (k - 1)).  One workgroup per point:
 * all m squared distances in LDS, bitonic sort, fixed-order sum (deterministic). */
int mvf_knn_rowsum(const double* X, int64_t m, int d, int k, double* rowsum, void* stream);

/* ---- grid preparation: convex-hull mask --------------------------------------------------------------------------------
 * Replaces: `grid_in_hull = in_hull(Grid, hull.points[hull.vertices, :])` of `get_X_Y_grid`
 * (spateo/tdr/interpolations/utils.py:48-53; `in_hull` = Delaunay(...).find_simplex(p) >= 0, spateo/tools/utils.py:205-221).
 * A point lies in a convex hull iff it is on the inner side of every facet: inside[i] = (max_f n_f . p_i + d_f <= tol).
 * points: n x 3 float64 row-major; equations: nfacets x 4 float64 = SciPy `ConvexHull(X).equations` (built on the host
 * with Qhull, as the reference does); inside: n bytes (0 / 1).  tol: the caller passes 100 eps x the hull's extent,
 * the scale of find_simplex's own barycentric tolerance.  A point at margin exactly tol is inside; a point with a NaN or
 * infinite coordinate is outside.  Limit: the equations must be finite - a facet whose value at a point is NaN does not
 * constrain that point (fmax drops a NaN operand), so a row of NaN acts as if it were not in the list. */
int mvf_hull_mask(const double* points, int64_t n, const double* equations, int64_t nfacets, double tol,
                  unsigned char* inside, void* stream);

/* ---- con_K ----------------------------------------------------------------------------------------------------
 * K[i, j] = exp(-beta * ||x_i - y_j||^2), materialised n x m row-major.
 * Replaces: dynamo `con_K` / in-tree twin `_con_K` spateo/tdr/morphometrics/morphofield/gaussian_process.py:16-36
 * (cdist path :21-24).  x: n x d, y: m x d, plain row-major (NOT x4), 1 <= d <= 8.  HBM-write-bound. */
int mvf_con_k(const void* x, int64_t n, const void* y, int64_t m, int d, double beta, void* K, mvf_dtype dtype,
              void* stream);
/* return_d=True variant (gaussian_process.py:25-29): also D[n, :, m] = x_n - y_m as n x d x m.  At most 65535 rows per call;
 * K is computed first, so a call refused for its row count or a null D has already written K and leaves D alone. */
int mvf_con_k_d(const void* x, int64_t n, const void* y, int64_t m, int d, double beta, void* K, void* D,
                mvf_dtype dtype, void* stream);

/* ---- field evaluation:  V = con_K(x, ctrl, beta) @ C  ---------------------------------------------------------
 * Replaces: dynamo `vector_field_function` (call site differential_geometry.py:67-68; twin `_gp_velocity`
 * gaussian_process.py:102-127), `V = U.dot(C)` and `grid_V = grid_U.dot(C)` of SparseVFC.
 * U is never materialised: kernel values are recomputed from x and ctrl.  x4: n x 4, ctrl4: m x 4 (dtype),
 * C: m x 3 float64 (unused columns zero), V4 out: n x 4 (dtype, 4th = 0).
 * If y4 != NULL also writes r[i] = ||y_i - V_i||^2 (dtype) and, if P != NULL (dtype, n), accumulates
 * stats[0] += sum_i P_i r_i  (float64; caller zeroes stats).  Reductions over cells are DETERMINISTIC everywhere in
 * this library: per-workgroup partials go to `scratch` (caller-provided, >= mvf_reduce_scratch_doubles(n) float64,
 * needed whenever P != NULL) and are summed in workgroup order by one workgroup - no floating-point atomics. */
size_t mvf_reduce_scratch_doubles(int64_t n);
int mvf_apply(const void* x4, int64_t n, const void* ctrl4, int64_t m, double beta, const double* C, void* V4,
              const void* y4, const void* P, void* r, double* stats, double* scratch, mvf_dtype dtype, void* stream);

/* ---- E-step ---------------------------------------------------------------------------------------------------
 * Replaces: dynamo `get_P` + the `P = max(P, minP)` / numcorr lines of SparseVFC.
 * Input r (dtype, n) = ||Y - V||^2.  Two phases so that the min-non-zero rule `temp1[temp1 == 0] =
 * min(temp1[temp1 != 0])` can be made global across ranks between them:
 *   mvf_estep_min : mins[0] = min non-zero exp(-r/(2 sigma2)) (float64, +inf if none), mins[1] = #zeros;
 *                   `mins` must hold MVF_ESTEP_MIN_DOUBLES float64 (the tail is block-partial scratch)
 *   mvf_estep_p   : P_out (dtype, n) = max(P, minP) with P = t1/(t1+t2);  stats (float64[5], caller zeroes):
 *                   [0] += sum P_unfloored * r, [1] += sum P_unfloored, [2] += sum P_floored, [3] += #(P_floored > theta),
 *                   [4] += #(t1 == 0), the cells that took the fill.  The fill is t1_zero_fill_dev[0] when that
 *                   DEVICE pointer is non-NULL (mins[0] of mvf_estep_min, MIN-all-reduced across ranks by the host; +inf
 *                   -> 0): the two phases then chain on the stream with no host round trip; else t1_zero_fill.
 *                   scratch: >= mvf_reduce_scratch_doubles(n) float64 (deterministic two-level sums).
 * All arithmetic in float64 regardless of dtype. */
#define MVF_ESTEP_MIN_DOUBLES 4098
int mvf_estep_min(const void* r, int64_t n, double sigma2, double* mins, mvf_dtype dtype, void* stream);
int mvf_estep_p(const void* r, int64_t n, double sigma2, double gamma, double a, int dy, double minP, double theta,
                double t1_zero_fill, const double* t1_zero_fill_dev, void* P_out, double* stats, double* scratch,
                mvf_dtype dtype, void* stream);
/* mvf_estep (ABI 7): mvf_estep_min followed by mvf_estep_p with the fill taken from mins[0] on the device - the E-step of ONE
 * process (no MIN all-reduce between the phases) in one call.  `stats` is OVERWRITTEN (no memset by the caller).  n >= 1. */
int mvf_estep(const void* r, int64_t n, double sigma2, double gamma, double a, int dy, double minP, double theta, double* mins,
              void* P_out, double* stats, double* scratch, mvf_dtype dtype, void* stream);

/* ---- M-step assembly:  G = U^T diag(P) U (m x m),  R = U^T diag(P) Y (m x 3)  --------------------------------
 * Replaces: `UP = U.T * repmat(P.T, M, 1); lhs = UP.dot(U) ...; rhs = UP.dot(Y)` of SparseVFC (App. A 5c; same
 * shape in-tree at spateo/alignment/methods/morpho_class.py:1266-1293).  MFMA kernel; the kernel values (cell dtype)
 * are regenerated from x4/ctrl4 in registers and accumulated with v_mfma_f64_16x16x4_f64 in both dtypes, so G is the
 * exact Gram matrix of those values; per-slice partial tiles are summed in a fixed order (deterministic).  No
 * process-global state: the library's behaviour depends on its arguments only.
 * Outputs are float64: G (m x m, full symmetric), R (m x 3).  They hold THIS rank's partial sums; the exchange is
 * mvf_allreduce_stats (below) or the host's own collective on the same device pointers: the packed triangle of G is
 * all-reduced asynchronously while the rhs kernels run, then [R | scalars]. */
size_t mvf_gram_workspace_bytes(int64_t n, int64_t m, mvf_dtype dtype);
int mvf_gram(const void* x4, const void* P, const void* y4, int64_t n, const void* ctrl4, int64_t m, double beta,
             double* G, double* R, void* workspace, size_t workspace_bytes, mvf_dtype dtype, void* stream);
/* Same, one stage at a time (mask of MVF_GRAM_STAGE_*): TILES = the MFMA kernel writing per-slice partial tiles into
 * the workspace, RHS = the U^T P Y kernel (partials), REDUCE / REDUCE_RHS = fixed-order sums of the partials into G /
 * into R.  mvf_gram == all four.  Lets a caller bracket the dominant kernel with HIP events on `stream` (bench.py's
 * roofline) and lets a wide Y (Dy > 3, kernel_interpolation) reuse one G for several 3-column rhs groups. */
enum { MVF_GRAM_STAGE_TILES = 1, MVF_GRAM_STAGE_RHS = 2, MVF_GRAM_STAGE_REDUCE = 4, MVF_GRAM_STAGE_REDUCE_RHS = 8 };
int mvf_gram_stages(int stages, const void* x4, const void* P, const void* y4, int64_t n, const void* ctrl4,
                    int64_t m, double beta, double* G, double* R, void* workspace, size_t workspace_bytes,
                    mvf_dtype dtype, void* stream);

/* Cached-U variant of the Gram kernel.  U = con_K(x, ctrl) is constant across EM iterations (only P changes), so when
 * HBM has room (mvf_ublk_bytes = sizeof(dtype) * roundup(n,256) * roundup(m,128) bytes; 98 GB at 8 M x 3000 float32)
 * the kernel values are materialised once per fit in the MFMA-operand-shaped layout Ublk[m/16][n][16] and the Gram
 * kernel streams them (9 coalesced loads per 16 MFMAs) instead of regenerating them - VALU work is additive to f64
 * MFMA time on gfx950, and in float64 mode the regenerated exp alone makes the kernel VALU-bound.  Same values, same
 * float64 accumulation, bit-identical outputs to mvf_gram; `stages` as in mvf_gram_stages. */
size_t mvf_ublk_bytes(int64_t n, int64_t m, mvf_dtype dtype);
int mvf_ublk_build(const void* x4, int64_t n, const void* ctrl4, int64_t m, double beta, void* ublk, size_t ublk_bytes,
                   mvf_dtype dtype, void* stream);
int mvf_gram_cached(int stages, const void* ublk, const void* x4, const void* P, const void* y4, int64_t n,
                    const void* ctrl4, int64_t m, double beta, double* G, double* R, void* workspace,
                    size_t workspace_bytes, mvf_dtype dtype, void* stream);

/* ---- wide right-hand sides (Dy > 3) on the cached kernel values (ABI 6) -------------------------------------------
 * Replaces: dynamo's `rhs = UP.dot(Y)` and `V = U.dot(C)` when Y has many columns - what
 * `kernel_interpolation` passes (spateo/tdr/interpolations/interpolation_sparseVFC.py:13-85: Y = the expression of Dy genes).
 * Both stream the cache of mvf_ublk_build ONCE for all columns, as v_mfma_f64_16x16x4_f64 products:
 *   mvf_rhs_cached  : R[j][d] = sum_n U[n][j] P_n Y[n][d]        R: m x dy float64, leading dimension ldr >= dy
 *   mvf_apply_cached: V[n][d] = sum_j U[n][j] C[j][d],  r_n = sum_d (Y[n][d] - V[n][d])^2 (against V as stored),
 *                     stats[0] += sum_n P_n r_n (P may be NULL: no sum)
 * Yd / Vd: n rows x ldy columns of the cell dtype, row-major, ldy a multiple of 16 and >= dy; Yd must be READABLE for
 * mvf_ublk_npad rows (n rounded up to 256) and zero (or any finite value) beyond row n and column dy.  C: float64,
 * leading dimension ldc (a multiple of 16, >= dy), readable for m rounded up to 128 rows (the cache holds zeros for the
 * padded control points and cells, so the padding's values only have to be finite).  r: n values of the cell dtype.
 * workspace: mvf_wide_workspace_bytes(n, m).  Deterministic (fixed summation orders). */
size_t mvf_wide_workspace_bytes(int64_t n, int64_t m);
int mvf_rhs_cached(const void* ublk, const void* P, const void* Yd, int64_t n, int64_t m, int dy, int64_t ldy, double* R,
                   int64_t ldr, void* workspace, size_t workspace_bytes, mvf_dtype dtype, void* stream);
int mvf_apply_cached(const void* ublk, int64_t n, int64_t m, const double* C, int64_t ldc, int dy, const void* Yd, int64_t ldy,
                     const void* P, void* Vd, void* r, double* stats, void* workspace, size_t workspace_bytes,
                     mvf_dtype dtype, void* stream);

/* ---- coefficient solve ------------------------------------------------------------------------------------------
 * Replaces: dynamo `lstsq_solver(lhs, rhs, "scipy")` as Spateo calls it (sparsevfc.py:110,194,250) =
 * scipy.linalg.lstsq = LAPACK gelsd: the MINIMUM-NORM solution with singular values below eps * s_max dropped
 * (in-tree analogue: `_pinv(SigmaInv)` spateo/alignment/methods/morpho_class.py:1287).  lhs = G + lambda_sigma2 * K is
 * symmetric, numerically positive SEMI-definite and, at Spateo's default lambda_ = 0.02, rank deficient.  Two entry
 * points; the host (vectorfield.py) uses the first when it certifies full numerical rank and the second otherwise:
 *
 * mvf_solve: (G + lambda_sigma2 K + jitter * mean(diag) * I) C = R by blocked right-looking Cholesky in float64 (f64
 *   MFMA trailing update) + forward/back substitution.  With jitter = 0 and a matrix of full numerical rank this IS
 *   the gelsd solution (nothing is truncated).  info[0] = 0 on success, or 1 + index of the first non-positive pivot.
 *   pivots (may be NULL): [0] = min_j L_jj^2, [1] = max_j L_jj^2 - min L_jj^2 is an upper bound of lambda_min, the
 *   host's rank certificate.  G, K: m x m float64 (read-only), R: m x nrhs, C out: m x nrhs, nrhs <= 8.
 *
 * mvf_solve_minnorm: C = sum_{|lambda_i| > rcond max|lambda|} q_i (q_i^T R) / lambda_i over the eigenpairs of
 *   G + lambda_sigma2 K (for a symmetric matrix exactly gelsd's SVD-truncated minimum-norm solution; rcond =
 *   DBL_EPSILON reproduces scipy's default).  Hand-written symmetric eigensolver: Cholesky of the matrix shifted by
 *   delta = shift * mean(diag) (0 < shift < 1; the shift only makes the factorisation exist and is subtracted from the
 *   eigenvalues again), then one-sided block Jacobi (f64 MFMA Gram and update tiles, 64 x 64 subproblems in LDS) on
 *   the factor's columns until a whole sweep applies no rotation.  info[0] != 0: the shift was too small for this
 *   matrix (the caller retries with a larger one); C is then not written.  einfo (12 float64, device): [0] = sweeps
 *   (x.5 if max_sweeps was hit first), [1] = kept rank, [2] = max|lambda|, [3] = min kept |lambda|, [4] = delta,
 *   [5] = min lambda.  NOT asynchronous: it synchronises `stream` once per sweep to read the rotation counter.
 *   reuse != 0: the decomposition of the previous call on this workspace (same matrix) is applied to another R (a
 *   wide Y is solved in groups of <= 8 columns); asynchronous, einfo must hold 12 float64 ([6..11] = this call's).
 *   basis (may be NULL; mvf_solve_minnorm_basis_bytes, caller-owned): on exit the orthonormal eigenvectors (row i =
 *   eigenvector i).  warm != 0: on entry it holds the eigenvectors of a NEARBY matrix (the previous EM iteration's):
 *   the matrix is first transformed to that basis (f64 MFMA GEMMs), where its well-determined part is already
 *   diagonal - same result, about half the sweeps (measured 27 -> 13 at m = 3000, 18 -> 4 at m = 500; the eigenvectors
 *   of eigenvalues near the rounding level of the matrix are re-resolved against each factorisation's own rounding
 *   noise, which is what the remaining sweeps do). */
size_t mvf_solve_workspace_bytes(int64_t m, int nrhs);
int mvf_solve(const double* G, const double* K, double lambda_sigma2, double jitter, const double* R, int64_t m,
              int nrhs, double* C, int* info, double* pivots, void* workspace, size_t workspace_bytes, void* stream);
size_t mvf_solve_minnorm_workspace_bytes(int64_t m, int nrhs);
int mvf_solve_minnorm(const double* G, const double* K, double lambda_sigma2, double shift, double rcond,
                      const double* R, int64_t m, int nrhs, double* C, int* info, double* einfo, int max_sweeps,
                      int reuse, double* basis, int warm, void* workspace, size_t workspace_bytes, void* stream);
size_t mvf_solve_minnorm_basis_bytes(int64_t m);

/* mvf_solve_minnorm_lr: the same truncated minimum-norm solve (same reference semantics: scipy.linalg.lstsq = gelsd,
 * spateo/tdr/morphometrics/morphofield/sparsevfc.py:110,194,250; `_pinv`, spateo/alignment/methods/morpho_class.py:1287)
 * through a RANK-REVEALING factor: greedy diagonally pivoted Cholesky  A = L L^T + E  (L m x r), stopped when every
 * remaining diagonal entry is <= tolf * DBL_EPSILON * lambda_max (lambda_max from 8 power-iteration steps; trace(E)
 * bounds ||E|| and sits at the rounding level of A), then one-sided block Jacobi on the r columns of L only, then
 * C = sum over sigma_i^2 > rcond max sigma^2 of u_i (u_i^T R) / sigma_i^2.  In the EM's steady state r ~ 0.3 m at
 * m = 3000 and the graded pivoted factor halves the sweep count; no shift, no retry ladder: info[0] != 0 only for
 * non-finite input.  einfo (12 float64, device): [0] = sweeps (x.5 if max_sweeps was hit first), [1] = kept rank,
 * [2] = max lambda, [3] = min kept lambda, [4] = 0, [5] = min lambda of the factor, [6] = r (columns of L).
 * rank_hint (0 = none): einfo[6] of the previous call ON THIS WORKSPACE for a nearby matrix (the previous EM iteration):
 * the factorisation then first follows the pivot order that call left in the workspace, 64 columns per three launches
 * (64 x 64 Cholesky of the gathered block, forward substitution of the gathered rows, trailing update) instead of one
 * launch per pivot, accepting a pivot only while it exceeds max(2^-10 x the largest remaining diagonal entry, the
 * stopping tolerance); the first rejected column ends the use of the hint and the greedy steps finish.  The result does
 * not depend on the hint being good: a stale or foreign order is rejected column by column, a workspace without a
 * finished order ignores the hint.  reuse != 0: apply the decomposition of the previous call on this workspace to another
 * R (einfo[7..11] = this call's).  reuse reads the workspace's state record first and is refused, with a non-zero return and
 * before anything is launched, unless the record carries the mark of a finished factorisation with 0 <= r <= m columns - the
 * same test mvf_lr_pivot_order and mvf_pinv_diag apply; mvf_solve_minnorm_lrd's reuse likewise.  That turns away a fresh,
 * zeroed or overwritten workspace and one whose last call stopped in the factorisation (non-finite input: the mark is
 * cleared when a factorisation starts and set when it ends).  It is not a proof that the record belongs to this matrix or
 * this m: the caller passes the workspace of the previous call, as for the rank hint.
 * NOT asynchronous (status reads during the factorisation, one per Jacobi sweep). */
size_t mvf_solve_minnorm_lr_workspace_bytes(int64_t m, int nrhs);
int mvf_solve_minnorm_lr(const double* G, const double* K, double lambda_sigma2, double tolf, double rcond,
                         const double* R, int64_t m, int nrhs, double* C, int* info, double* einfo, int max_sweeps,
                         int reuse, int rank_hint, void* workspace, size_t workspace_bytes, void* stream);

/* mvf_solve_minnorm_lrd: the same truncated minimum-norm solve (same reference call, same eps * lambda_max cut-off, same
 * arguments, same pivot-order / rank_hint / reuse behaviour and the same einfo layout as mvf_solve_minnorm_lr) WITHOUT the
 * eigendecomposition of the whole factor: after the pivoted Cholesky has dropped everything below tolf * eps * lambda_max,
 * the eigenvalues gelsd truncates are the few smallest ones of S2 = L^T L (r x r) and lie within 1 / tolf of the cut.
 * S2 = Rc Rc^T (Cholesky; the inverse factor rides along as extra rows), block inverse iteration on 256 vectors started on
 * the smallest pivots (three applications of S2^-1, Cholesky-QR in between), Rayleigh-Ritz on the 256 x 256 projection (the
 * Jacobi kernels; einfo[0] = ITS sweeps), W = Ritz vectors with theta <= rcond * lambda_max, Pc = I - W^T W, and
 *     C = L Pc S2^-1 Pc S2^-1 Pc L^T R
 * (the projections between the inverse applications keep the amplified rounding error of the dropped directions out).
 * lambda_max (einfo[2]) is the Rayleigh quotient of 12 power-iteration steps (relative error ~1e-8), einfo[3] the smallest
 * Ritz value above the cut inside the block, einfo[7] the block size used (256; 128 when the
 * previous call on this workspace - rank_hint > 0 - deflated at most 72 directions, repeated with 256 if it then finds more
 * than 80; 64 for factors of 128 .. 511 columns, accepted while at most 40 Ritz values lie below the cut; 0 when the Jacobi
 * path answered).  When the factor has fewer than 128 columns, when more than 224 (block 256) Ritz values
 * fall below the cut, or a factorisation meets a non-positive pivot, the call continues on mvf_solve_minnorm_lr's Jacobi
 * path and returns its result.  Measured at m = 3000 in the EM's steady state (r = 869): 6.7 ms against 22.9 ms, the field
 * within 1e-6 of the Jacobi path's on the same factor.  The workspace is larger (the r x r scratch); mvf_pinv_diag does not
 * accept a workspace left by this call (it needs every eigenpair): use mvf_solve_minnorm_lr for that.  No reference
 * interface changes: this is how `lstsq_solver(lhs, rhs, "scipy")` is evaluated.
 * Direct form (ABI 5; m <= 640, rank_hint == m, i.e. the previous call on this workspace kept ALL m columns - what m = 500
 * control points give): the pivoted factorisation of the next matrix in that order is an ordinary Cholesky of the permuted
 * matrix, A_perm = Rc Rc^T, and the blocked factorisation with the identity riding along yields E = Rc^-T in the same pass;
 * block inverse iteration on 64 vectors (continued from the previous call's block when that call had this form), Rayleigh-Ritz
 * through the factor (H = (Z Rc)(Z Rc)^T, one 64 x 64 Jacobi tile diagonalised in one launch), and
 *     C = Pi^T Pc E E^T Pc Pi R
 * with the inverse applied as its two triangular factors (the product E E^T would lose the factor's grading: 3 - 4 digits of
 * the field).  Accepted only if every pivot clears tolf * eps * lambda_max, lambda_max has converged and at most 40 Ritz values
 * lie below the cut; anything else re-runs the call in the factor form above.  The workspace then holds the unchanged pivot
 * order (mvf_lr_pivot_order works), einfo[0] = Rayleigh-Ritz launches (1), einfo[6] = m, einfo[7] = 64; reuse works.  Measured
 * at m = 500: 1.5 ms against 2.5 ms for the factor form and 3.6 ms for mvf_solve_minnorm (round 6: 0.9 ms).
 * einfo[8] (ABI 6) names the form that answered: 0 = the Jacobi path, 1 = the factor form, 2 = the direct form; einfo[9] = 0.
 *
 * mvf_solve_minnorm_lrd_async (ABI 6): the direct form WITHOUT a single host synchronisation - the synchronous entry point
 * reads the workspace state before it launches, the Rayleigh-Ritz counter and the acceptance numbers after (three round
 * trips of ~40 us in a 0.9 ms call, and the host cannot run ahead of the device across any of them).  The caller says what it
 * knows from the previous call's einfo ON THIS WORKSPACE: form_hint = 1: that call returned einfo[6] == m (all m columns
 * kept) through the factor form, 2: through the direct form (its block is continued); + 4 (that is 5 or 6): the matrix
 * moved since that call (the caller's sigma^2 changed by more than a few per cent): 13 warm power steps for lambda_max
 * instead of 5, as the synchronous entry adds them after reading the Rayleigh quotient.  The device verifies the state
 * (a stale or foreign workspace, a pending cool-down: not accepted) and takes the acceptance decision itself (every pivot
 * above the tolerance, lambda_max settled after the five warm power steps, the 64 x 64 Rayleigh-Ritz converged inside its one
 * launch, at most 40 directions below the cut): einfo[9] = 0: accepted - C, einfo[0..8] and the workspace exactly as the
 * synchronous direct form leaves them; einfo[9] = 1: NOT accepted - C is undefined and the caller must repeat the call
 * through mvf_solve_minnorm_lrd (the workspace carries the cool-down mark, so that call goes to the factor form at once).
 * Asynchronous on `stream`; einfo / info are read by the caller in its own device -> host copy.  128 <= m <= 640. */
size_t mvf_solve_minnorm_lrd_workspace_bytes(int64_t m, int nrhs);
int mvf_solve_minnorm_lrd(const double* G, const double* K, double lambda_sigma2, double tolf, double rcond,
                          const double* R, int64_t m, int nrhs, double* C, int* info, double* einfo, int max_sweeps,
                          int reuse, int rank_hint, void* workspace, size_t workspace_bytes, void* stream);
int mvf_solve_minnorm_lrd_async(const double* G, const double* K, double lambda_sigma2, double tolf, double rcond,
                                const double* R, int64_t m, int nrhs, double* C, int* info, double* einfo, int form_hint,
                                void* workspace, size_t workspace_bytes, void* stream);

/* The pivot order of the factorisation the last mvf_solve_minnorm_lr call left in `workspace` (same m): order_out (HOST,
 * room for m ints) receives the r pivots in the order they were taken, *r_out = r.  These are the control points that
 * carry the numerical rank of  U^T P U + lambda sigma^2 K;  the host's optional "pivot" Gram mode restricts the rest of
 * a fit to them.  pivots_out (HOST, m float64, may be NULL): the diagonal value each pivot had when it was taken (falling,
 * the last ones at the stopping tolerance); tol_out (HOST, may be NULL): that tolerance, tolf * eps * lambda_max.
 * Synchronises `stream`. */
int mvf_lr_pivot_order(const void* workspace, size_t workspace_bytes, int64_t m, int* order_out, double* pivots_out,
                       double* tol_out, int64_t* r_out, void* stream);

/* diag_out[n] = (U pinv(A) U^T)_nn, U = con_K(x, ctrl, beta), with the decomposition of A that the previous
 * mvf_solve_minnorm_lr (lowrank != 0) / mvf_solve_minnorm (lowrank == 0) call left in `workspace` (same m, same rcond
 * semantics: eigenvalues below rcond * max|lambda| dropped).  Replaces the last statement of
 * `Morpho_pairwise._update_nonrigid`, spateo/alignment/methods/morpho_class.py:1295-1297:
 * `SigmaDiag = sigma2 * einsum("ij->i", einsum("ij,ji->ij", U, dot(Sigma, U.T)))` (the caller multiplies by sigma2).
 * x4: n x 4 (dtype), ctrl4: m x 4 (dtype), diag_out: n float64.  Synchronises `stream` once on the lowrank path. */
int mvf_pinv_diag(const void* x4, int64_t n, const void* ctrl4, int64_t m, double beta, double rcond, int lowrank,
                  double* diag_out, void* workspace, size_t workspace_bytes, mvf_dtype dtype, void* stream);

/* out[i] = a A[i] + b B[i] + c C[i], n float64 (B, C may be NULL; out may alias an input).  The compositions of
 * `Morpho_pairwise._update_nonrigid`'s SVI and guidance branches (spateo/alignment/methods/morpho_class.py:1269-1288):
 * `SigmaInv = step SigmaInv_new + (1 - step) SigmaInv_prev`, `SigmaInv += w U_I^T U_I`, `UPXB_term += w U_I^T (X_BI - R_AI)`. */
int mvf_lincomb3(double* out, double a, const double* A, double b, const double* B, double c, const double* C,
                 int64_t n, void* stream);

/* trace(C^T K C) -> out[0] (float64), the regulariser of the energy (App. A 5b). K: m x m, C: m x nrhs;
 * scratch >= m float64 (row partials, summed in row order). */
int mvf_quadform(const double* K, const double* C, int64_t m, int nrhs, double* out, double* scratch, void* stream);

/* Packed upper triangle (row-major, row i = columns i..m-1, m (m + 1) / 2 float64) <-> full symmetric m x m: the
 * multi-GPU host all-reduces the packed triangle of G (36 MB instead of 72 MB at m = 3000). */
int mvf_sym_pack(const double* G, int64_t m, double* tri, void* stream);
int mvf_sym_unpack(const double* tri, int64_t m, double* G, void* stream);

/* ---- the EM step's exchange: all-reduce of the sufficient statistics over RCCL (xGMI) -------------------------------
 * cells are block-sharded over the GPUs of one node, one process per GPU; per EM step every rank
 * contributes its partial  [tri(G) | R | sum P, sum P r, #(P > theta), ...]  (contiguous float64, caller-owned) and all
 * ranks continue with the sums.  The reference has no counterpart (single process, NumPy); the statement it distributes
 * is `lhs = UP.dot(U) ...; rhs = UP.dot(Y)` of SparseVFC (App. A 5c; call site
 * spateo/tdr/morphometrics/morphofield/sparsevfc.py:189-198) - sums over cells, hence an all-reduce of the partials.
 *   mvf_comm_unique_id : id_out = MVF_COMM_ID_BYTES host bytes (ncclGetUniqueId).  ONE rank calls it and hands the bytes to
 *                        the others out of band (the Python host broadcasts them with torch.distributed / its store).
 *   mvf_comm_create    : collective over all `nranks` ranks (ncclCommInitRank) on the CURRENT HIP device, which becomes the
 *                        communicator's device; nranks = 1 is valid (a single-rank communicator: how the one-GPU tests
 *                        execute this path on RCCL).  The handle owns nothing but the RCCL communicator.
 *   mvf_comm_destroy   : frees it (NULL is a no-op).
 *   mvf_comm_info      : nranks / rank / device of a handle AS RCCL REPORTS THEM (ncclCommCount / ncclCommUserRank /
 *                        ncclCommCuDevice; any pointer may be NULL) - what bench.py records as `rccl_ranks`.
 *   mvf_allreduce_stats: buf[0..count) (DEVICE float64, in place) <- elementwise SUM (MVF_RED_SUM) or MIN (MVF_RED_MIN: the
 *                        E-step's global min-non-zero rule) over the ranks; asynchronous on `stream` (ordered with the
 *                        kernels the caller launched there: pass a second stream + events to overlap it with compute, as
 *                        the host does for tri(G)).  The current device must be the communicator's.  Every rank must call
 *                        with the same count / op in the same order.  RCCL's sums are in a fixed ring order: every rank
 *                        receives bit-identical results, which the redundant coefficient solve relies on. */
typedef struct mvf_comm mvf_comm;
#define MVF_COMM_ID_BYTES 128
enum { MVF_RED_SUM = 0, MVF_RED_MIN = 1 };
int mvf_comm_unique_id(void* id_out);
int mvf_comm_create(mvf_comm** comm_out, int nranks, int rank, const void* id);
int mvf_comm_destroy(mvf_comm* comm);
int mvf_comm_info(const mvf_comm* comm, int* nranks, int* rank, int* device);
int mvf_allreduce_stats(mvf_comm* comm, double* buf, int64_t count, int op, void* stream);

/* ---- differential-geometry evaluators -------------------------------------------------------------------------
 * Replaces: dynamo `Jacobian_rkhs_gaussian` and `compute_{acceleration,curvature,curl,torsion,divergence}` =
 * in-tree twins spateo/tdr/morphometrics/morphofield_dg/GPVectorField.py:143-190 and :12-121 (wrappers
 * differential_geometry.py:42-341).  One fused kernel: per query point, one pass over the control points
 * accumulates v (3) and J (3x3) in float64, then derives the requested quantities in registers.
 * x4: n x 4 (dtype), ctrl4: m x 4 (dtype), C: m x 3 float64.  Outputs are float64, NULL if not requested:
 * v, curl, acc, curv, tors: n x 3;  jac: (3, 3, n) = J[f][i][n];  div, jdet: n.  `flags` = MVF_EVAL_* bits. */
int mvf_eval(const void* x4, int64_t n, const void* ctrl4, int64_t m, double beta, const double* C, int flags,
             double* v, double* jac, double* div, double* curl, double* acc, double* curv, double* tors,
             double* jdet, mvf_dtype dtype, void* stream);

/* Same with an affine epilogue, for the Gaussian-process morphofield variant:
 *   v_out[f] = alpha[f] * (K @ C)[f] + (A q + b)[f],   J_out = jmul * J,   q = the query point as passed in x4 (unscaled);
 * every derived quantity (div, curl, acc, curvature, torsion, det) is computed from v_out / J_out.
 * `affine` is a HOST array of 16 doubles {alpha[3], jmul, A[9] row-major, b[3]} read at call time (NULL = identity);
 * alpha is per output component since ABI 6 (a per-axis `scale_fixed` of the GP variant's norm_dict).
 * Replaces: `_gp_velocity` spateo/tdr/morphometrics/morphofield/gaussian_process.py:102-127 and
 * `Jacobian_GP_gaussian_kernel` / `GPVectorField` morphofield_dg/GPVectorField.py:143-266 (norm_dict + rigid part). */
int mvf_eval_affine(const void* x4, int64_t n, const void* ctrl4, int64_t m, double beta, const double* C,
                    const double* affine, int flags, double* v, double* jac, double* div, double* curl, double* acc,
                    double* curv, double* tors, double* jdet, mvf_dtype dtype, void* stream);

/* ---- fields in 4 to 8 dimensions (ABI 7) ----------------------------------------------------------------------
 * The points are plain row-major n x d arrays of the cell dtype (NOT x4), centred by the caller, 4 <= d <= 8 (the bound of
 * mvf_con_k).  K(x, c) is bit-identical to mvf_con_k at the same d.  Arguments are validated before any HIP call.
 *
 * mvf_ublk_build_d: the kernel-value cache of mvf_ublk_build (same layout Ublk[m/16][n][16], same zero padding, same size
 * mvf_ublk_bytes) for d-dimensional cells x (n x d) and control points ctrl (m x d).  mvf_gram_cached's TILES and REDUCE
 * stages, mvf_rhs_cached, mvf_apply_cached and the E-step read only the cache, P, Y and the coefficients, so an EM
 * iteration runs unchanged on it.
 * Replaces: `U = con_K(X, ctrl_pts, beta)` of dynamo SparseVFC with `_con_K`
 * spateo/tdr/morphometrics/morphofield/gaussian_process.py:16-36 on d-column `obsm` coordinates
 * (interpolations/interpolation_sparseVFC.py:45,63). */
int mvf_ublk_build_d(const void* x, int64_t n, const void* ctrl, int64_t m, int d, double beta, void* ublk,
                     size_t ublk_bytes, mvf_dtype dtype, void* stream);
/* mvf_eval_d: the fused evaluator of mvf_eval for x (n x d), ctrl (m x d) and C (m x dy float64, row-major), 1 <= dy <= 8.
 * Outputs float64, NULL if not requested: v n x dy;  jac (dy, d, n) = J[f][i][q] (the reference's layout);  and, for
 * dy == d only, div n, acc = J v n x d, curv (formula 2) n x d.  flags: MVF_EVAL_V | _JAC | _DIV | _ACC | _CURV (curl,
 * torsion and det are not defined here).  Deterministic; v alone is one 16-column MFMA product.
 * Replaces: dynamo `vector_field_function` / `Jacobian_rkhs_gaussian` and compute_{acceleration,curvature,divergence} =
 * morphofield_dg/GPVectorField.py:143-190 and :12-52, 97-121 at 4 <= d <= 8. */
int mvf_eval_d(const void* x, int64_t n, const void* ctrl, int64_t m, int d, double beta, const double* C, int dy,
               int flags, double* v, double* jac, double* div, double* acc, double* curv, mvf_dtype dtype, void* stream);

/* ---- wide fields at new points: values and spatial gradients (mvf_eval_wide.hip) ----------------------------------------
 * One addition to the table (mvf_version stays 7 by the addition rule stated at mvf_align_moments).
 * v = K @ C and J[f][i][q] = d v_f / d x_i = -2 beta sum_m K(x_q, c_m) C[m, f] (x_q - c_m)_i for a field of ANY number of
 * output columns dy at d = 1, 2 or 3: the field `kernel_interpolation` fits (Y = the selected obs columns and genes).
 * x4: n x 4 and ctrl4: m x 4 (dtype), as mvf_eval takes them: centred by the caller, unused coordinates zero; K(x, c) is the
 * value mvf_eval sees.  C: m x dy float64, row-major, row stride ldc >= dy (so a column panel is `C + f0` with the same ldc).
 * flags: a non-empty subset of MVF_EVAL_V | MVF_EVAL_JAC.  v: n x dy float64 with row stride ldv >= dy, the columns
 * dy .. ldv - 1 are not touched;  jac: (dy, d, n) contiguous float64 = J[f][i][q], the reference's layout.  An output that
 * is not requested may be NULL.  1 + d matrix-core products of a generated n x m operand with C (float64 accumulation), one
 * workgroup over all m per tile: no atomics, two calls give identical bits.  Arguments are validated before any HIP call;
 * n == 0 or dy == 0 launches nothing, m == 0 writes zeros.
 * Replaces: dynamo `vector_field_function` / `Jacobian_rkhs_gaussian` for Dy = #keys on the field fitted at
 * spateo/tdr/interpolations/interpolation_sparseVFC.py:63 (Jacobian twin: morphofield_dg/GPVectorField.py:143-190). */
int mvf_eval_wide(const void* x4, int64_t n, const void* ctrl4, int64_t m, int d, double beta, const double* C, int64_t ldc,
                  int dy, int flags, double* v, int64_t ldv, double* jac, mvf_dtype dtype, void* stream);

/* ---- trajectory integration (morphopath) ------------------------------------------------------------------------
 * Integrates dx/dt = v(x), v as in mvf_eval_affine, from the n start points x4 with classical RK4: n_out samples per
 * trajectory, `dt` apart, `substeps` RK4 steps between samples; traj (float64) = [n][n_out][3], traj[:, 0] = start.
 * One launch, one lane per trajectory, control points staged in LDS.  A negative dt integrates backwards.
 * Replaces the field evaluations inside dynamo `fate` as driven by `morphopath`
 * (spateo/tdr/morphometrics/morphofield/trajectory.py:61-109).  The integrator itself is this repo's (fixed-step RK4,
 * uniform time sampling); mvf_integrate_rk45 below is the adaptive RK45 + arc-length resampling dynamo `fate` runs. */
int mvf_integrate(const void* x4, int64_t n, const void* ctrl4, int64_t m, double beta, const double* C,
                  const double* affine, double dt, int substeps, int n_out, double* traj, mvf_dtype dtype, void* stream);

/* Sampling of mvf_integrate_rk45 */
typedef enum { MVF_RK45_UNIFORM_TIME = 0, MVF_RK45_ARC_LENGTH = 1 } mvf_rk45_sampling;

/* Adaptive integration of dx/dt = v(x), v as in mvf_integrate, with SciPy 1.15.3's RK45 (`solve_ivp(method="RK45")`)
 * step for step: Dormand-Prince 5(4) with FSAL, select_initial_step, the step-size controller (SAFETY 0.9, factors
 * [0.2, 10], h in [10 ulp(t), max_step], clipped to t_bound), the RMS error norm over the first `d` components, the
 * quartic dense output, and a terminal event where every |v_i| (i < d) < 1e-5, detected between accepted steps as a
 * change of the event's sign and located on the dense output to 4 EPS; the path then ends at (root, sol(root)).
 * Step control, the event and the arc length run in WORLD coordinates y = q * scale + offset per axis (q = the point as
 * x4 holds it): `world` is a HOST array {scale[3], offset[3]} (scale non-zero).  t_bound is signed (< 0 = backwards),
 * rtol / atol > 0, max_step > 0 (may be +inf), max_steps >= 1 caps the step attempts (accepted + rejected) per trajectory.
 * sampling: MVF_RK45_UNIFORM_TIME = n_out samples at k t_bound / (n_out - 1) on the dense output (after a terminal event
 * the remaining samples hold the event state); MVF_RK45_ARC_LENGTH = n_out points equally spaced in arc length along the
 * polyline of accepted step points, their times by linear interpolation along it (np.interp; uniform times over
 * [0, t_end] when the path has length 0), their states on the dense output (two passes over the same steps, no workspace).
 * Outputs (DEVICE, float64 unless stated): t = [n][n_out], traj = [n][n_out][3] (world coordinates, sample 0 = start),
 * stats = int32 [n][4] = {accepted steps, rejected steps, field evaluations, status}; status 0 = reached t_bound,
 * 1 = terminal event, -1 = step size below the spacing of t (SciPy's failure; the partial path is kept and the remaining
 * samples hold its last point), -2 = max_steps reached (same), -3 = non-finite start row (t and traj are NaN).
 * n == 0 launches nothing; invalid arguments are rejected before any HIP call.
 * Replaces: dynamo `fate` as `morphopath` drives it, spateo/tdr/morphometrics/morphofield/trajectory.py:61-110
 * (solve_ivp RK45 per cell, max_step = t_end / interpolation_num, dense output, arc-length resampling). */
int mvf_integrate_rk45(const void* x4, int64_t n, const void* ctrl4, int64_t m, double beta, const double* C,
                       const double* affine, int d, const double* world, double t_bound, double rtol, double atol,
                       double max_step, int max_steps, int sampling, int n_out, double* t, double* traj, int* stats,
                       mvf_dtype dtype, void* stream);

/* ---- alignment: the assignment step, fused (no NA x NB matrix) ----------------------------------------------------------
 * Replaces: `Morpho_pairwise._update_assignment_P` (spateo/alignment/methods/morpho_class.py:1071-1200), i.e. `calc_distance`
 * (spateo/alignment/methods/utils.py:647-788, 866-941), `calc_probability` (:944-985) and `get_P_core` (:993-1096) on the
 * dense path, for the metrics and probability types below.  Every metric is d_ij = a_i + b_j - s <X'_i, Y'_j>, optionally
 * clamped at 0 / square-rooted; mvf_assign_prepare builds the operands of one side of one layer, mvf_assign runs the two
 * tile passes (layer products as f64 MFMA, exponent arithmetic in float64 whatever the dtype; `dtype` is the storage of
 * the coordinates and of X' / Y').  Partial sums go through the workspace and are added in a fixed order: two calls give
 * bit-identical results. */
typedef enum {
    MVF_ASSIGN_EUC = 0,       /* "euc" / "euclidean": the SQUARED distance, clamped at 0 (the reference's naming) */
    MVF_ASSIGN_SQRT_EUC = 1,  /* "square_euc" / "square_euclidean": its square root                               */
    MVF_ASSIGN_KL = 2,        /* "kl": rows + 0.01, normalised, log(. + 1e-8)                                     */
    MVF_ASSIGN_SYM_KL = 3,    /* "sym_kl": (kl(x, y) + kl(y, x)) / 2 as one product over 2 g features             */
    MVF_ASSIGN_COS = 4,       /* "cos" / "cosine": 1/2 - 1/2 cosine similarity, norms floored at 1e-8             */
    MVF_ASSIGN_LABEL = 5      /* "label": d_ij = T[la_i][lb_j], a look-up in the label-transfer table (see below) */
} mvf_assign_metric;
typedef enum { MVF_ASSIGN_GAUSS = 0, MVF_ASSIGN_COS_PROB = 1, MVF_ASSIGN_PROB = 2 } mvf_assign_prob;
#define MVF_ASSIGN_MAX_LAYERS 4
/* one expression / representation layer (a HOST struct of DEVICE pointers): Xp (na x ld) and Yp (nb x ld) in `dtype`, a (na)
 * and b (nb) float64, all from mvf_assign_prepare; prob: exp(-d / (2 param)) | 1 - d | d  (calc_probability, :974-983).
 * A LABEL layer (metric MVF_ASSIGN_LABEL; `_label_distance_backend`, utils.py:791-832, 908-910) travels in the same fields:
 *   Xp  the label-transfer table T, K x L FLOAT64 row-major whatever `dtype`;   ld = L >= 1 (any value, not a multiple of 16);
 *   a (na) / b (nb)  the cells' labels as integers held in float64, 0 <= a_i < K and 0 <= b_j < L, from
 *       mvf_assign_label_prepare (the kernels read T[a_i ld + b_j] UNCHECKED: that entry point is what puts them in range);
 *   Yp  NULL (a label layer has no rows per B cell; a non-null Yp under this metric code is refused as a product layer with
 *       the wrong code, before its Xp / a / b could be read as table and labels).   d_ij = T[a_i][b_j], no clamp, no square root; prob / param as for every other layer.
 * K is no field: it is an argument of mvf_assign_label_prepare, which rejects K < 1; mvf_assign, mvf_assign_dense,
 * mvf_assign_topk and mvf_align_gather reject ld < 1 and null Xp / a / b (the gather: b; it does not look at Yp).  Several label layers may share one
 * table.  (An addition behind version 7: the struct's layout and every signature are unchanged.) */
typedef struct {
    const void* Xp;
    const void* Yp;
    const double* a;
    const double* b;
    int64_t ld;
    int metric;
    int prob;
    double param;
} mvf_assign_layer;
/* features per prepared row: g (2 g for sym_kl) rounded up to a multiple of 16; 0 for g <= 0, an unknown metric or
 * MVF_ASSIGN_LABEL (a label layer has no prepared rows) */
int64_t mvf_assign_padded_features(int64_t g, int metric);
/* Replaces the per-cell part of `_kl_distance_backend` / `_cosine_distance_backend` / `_euc_distance_backend`
 * (utils.py:683-695, 736-739, 780).  layer: n x g float64 (device); side 0 = the A cells (rows of P), 1 = the B cells.
 * Out: Lp (n x ld, dtype; ld = mvf_assign_padded_features(g, metric), the tail of each row zero) and ab (n float64): the
 * row constant a_i (side 0) or b_j (side 1), formed from the operands as stored.  n == 0 launches nothing. */
int mvf_assign_prepare(const double* layer, int64_t n, int64_t g, int metric, int side, void* Lp, int64_t ld, double* ab,
                       mvf_dtype dtype, void* stream);
/* The same from the CSR arrays of a sparse layer (device): indptr (n + 1 int64, non-decreasing, indptr[0] >= 0 - the CALLER
 * checks that, spateo_amd does on the host), indices (int32) and data (float32 if data_is_f32, else float64), n rows and
 * g < 2^31 columns.  Lp and ab are, bit for bit, what mvf_assign_prepare writes for the dense float64 matrix
 * M[i][indices[e]] = (double)data[e], zeros elsewhere: one wave per row expands the row into a staging row of g float64
 * inside `workspace` and runs the dense entry point's row routine on it, so no n x g buffer exists on the device either.
 * The column indices of a row must be distinct (any order); an entry whose index lies outside [0, g) is skipped, never
 * used as an address.  workspace: at least mvf_assign_prepare_csr_min_workspace_bytes(g) (four staging rows), 8-byte
 * aligned; more rows are used when they fit, and the result does not depend on the size.  No atomics: two calls give the
 * same bits.  n == 0 launches nothing.  (An addition behind version 7.) */
size_t mvf_assign_prepare_csr_min_workspace_bytes(int64_t g);
int mvf_assign_prepare_csr(const int64_t* indptr, const int32_t* indices, const void* data, int data_is_f32, int64_t n, int64_t g,
                           int metric, int side, void* Lp, int64_t ld, double* ab, void* workspace, size_t workspace_bytes,
                           mvf_dtype dtype, void* stream);
/* One side of a label layer: labels (n int32, device) -> ab (n float64, device) = min(max(label, 0), classes - 1), the
 * representation mvf_assign_layer's a (classes = K) / b (classes = L) hold.  The clamp only keeps the table look-up inside
 * the table; a label outside 0 .. classes - 1 is the CALLER's error to report (spateo_amd.align does, on the host).
 * classes < 1 is an error; n == 0 launches nothing. */
int mvf_assign_label_prepare(const int32_t* labels, int64_t n, int64_t classes, double* ab, void* stream);
size_t mvf_assign_workspace_bytes(int64_t na, int64_t nb);
/* xa4 (na x 4) = XAHat, xb4 (nb x 4) = coordsB in the x4 layout (dtype); layers: 1 .. MVF_ASSIGN_MAX_LAYERS host structs;
 * model_mul (na float64) = alpha exp(-SigmaDiag / sigma2) (morpho_class.py:1087); spatial_outlier as get_P_core forms it
 * (:1051-1053).  Outputs (device float64): K_NA, K_NA_spatial, K_NA_sigma2 (na), K_NB (nb), PXB = P @ coordsB (na x 3, the
 * unused columns 0), scalars[0] = sum_ij P_sigma2 d_ij (`sigma2_related` before its division, :1075).  Sp = sum K_NB.
 * na == 0 or nb == 0 returns 0 without touching the device. */
int mvf_assign(const void* xa4, int64_t na, const void* xb4, int64_t nb, const mvf_assign_layer* layers, int nlayers,
               const double* model_mul, double sigma2, double sigma2_variance, double spatial_outlier, double* K_NA,
               double* K_NB, double* K_NA_spatial, double* K_NA_sigma2, double* PXB, double* scalars, void* workspace,
               size_t workspace_bytes, mvf_dtype dtype, void* stream);
/* The same, and the dense P (na x nb float64, row-major) as well: `self.P` of the reference (:1167), for label transfer and
 * debugging - the one variant that writes na nb values. */
int mvf_assign_dense(const void* xa4, int64_t na, const void* xb4, int64_t nb, const mvf_assign_layer* layers, int nlayers,
                     const double* model_mul, double sigma2, double sigma2_variance, double spatial_outlier, double* K_NA,
                     double* K_NB, double* K_NA_spatial, double* K_NA_sigma2, double* PXB, double* scalars, double* P,
                     void* workspace, size_t workspace_bytes, mvf_dtype dtype, void* stream);
/* The reference's `sparse_calculation_mode` (`get_P_core` -> `_dense_to_sparse(axis=0, descending=True)`, utils.py:1085-1094,
 * 1369-1404): the k_eff = min(k, na) largest entries of every column of P are kept, 1 <= k <= MVF_ASSIGN_TOPK_MAX (the
 * per-column lists of a 64-column workgroup live in LDS: 64 x 64 x 12 bytes = 48 KiB at the cap); any other k is an error.
 * rows (nb x k_eff int32) / vals (nb x k_eff float64): column j's kept entries in the total order (value descending, row
 * ascending); a column whose terms all underflow has vals = 0 and rows = 0 .. k_eff - 1.  K_NB[j] = the sum of vals[j][.] in
 * stored order; K_NA and PXB are summed over the kept entries only; K_NA_spatial, K_NA_sigma2 and scalars[0] are the dense
 * quantities, the same sums as mvf_assign's.  No floating-point atomics: two calls give the same bits, rows included.
 * (An addition behind version 7: no existing signature or layout changes.) */
#define MVF_ASSIGN_TOPK_MAX 64
size_t mvf_assign_topk_workspace_bytes(int64_t na, int64_t nb, int k); /* 0 for an empty side or k outside the range */
int mvf_assign_topk(const void* xa4, int64_t na, const void* xb4, int64_t nb, const mvf_assign_layer* layers, int nlayers,
                    const double* model_mul, double sigma2, double sigma2_variance, double spatial_outlier, int k,
                    double* K_NA, double* K_NB, double* K_NA_spatial, double* K_NA_sigma2, double* PXB, double* scalars,
                    int32_t* rows, double* vals, void* workspace, size_t workspace_bytes, mvf_dtype dtype, void* stream);
/* The cell mapping of the reference (`get_optimal_mapping_relationship` / `mapping_aligned_coords`, spateo/alignment/utils.py:
 * 157-255) without P: the best partner of every A cell (the maximum of its row of P) and of every B cell (of its column).
 * With v_ij the value mvf_assign_dense stores in P[i][j] and d_ij the clamped squared spatial distance, per row i over j < nb:
 *   row_val[i]        max_j v_ij;
 *   row_idx[2 i]      "nearest": the j first in the total order (v descending, d ascending, j ascending) - keep_all=False,
 *                     where the reference takes the nearest coordinate among equal maxima (an all-zero row: the nearest B cell);
 *   row_idx[2 i + 1]  "first": the j first in (v descending, j ascending) - what keep_all=True keeps after its sort and
 *                     drop-duplicates (an all-zero row: 0);
 * and the same per column j over i < na in col_idx (nb x 2) / col_val (nb).  Both orders are total and the head of a union is
 * the head of the heads of its parts, so tiles and splits combine in any order: no floating-point atomics, two calls give the
 * same bits.  Indices always lie in [0, nb) / [0, na): padding is never offered, and a row or column without one comparable
 * (non-NaN) entry gets index 0 and value 0.  Arguments, checks and the empty-side return are mvf_assign's.  row_idx / row_val
 * are both NULL or both given, and so are col_idx / col_val; a NULL pair skips that direction's kernel, both pairs NULL is an
 * error.  Workspace: mvf_assign's with the splits' states behind it.  (An addition behind version 7.) */
size_t mvf_assign_best_workspace_bytes(int64_t na, int64_t nb); /* 0 for an empty side */
int mvf_assign_best(const void* xa4, int64_t na, const void* xb4, int64_t nb, const mvf_assign_layer* layers, int nlayers,
                    const double* model_mul, double sigma2, double sigma2_variance, double spatial_outlier,
                    int32_t* row_idx, double* row_val, int32_t* col_idx, double* col_val, void* workspace,
                    size_t workspace_bytes, mvf_dtype dtype, void* stream);
/* P applied to cell features without P: what the reference's users form from `Morpho_pairwise.run()`'s dense result -
 * `P.T @ onehot(labels_A)` (an annotation carried to the next slice), `P @ X_B` (expression or an embedding carried across),
 * and with the sums the row-normalised, barycentric forms.  With P[i][j] the value mvf_assign_dense stores, m_i e2_ij q_ij c3_j:
 *   to_A (na x cb, ld = cb) = P   @ FB,   FB nb x cb (ld ldfb >= cb);
 *   to_B (nb x ca, ld = ca) = P^T @ FA,   FA na x ca (ld ldfa >= ca);
 *   K_NA (na) / K_NB (nb)   the row / column sums of P, each may be NULL (K_NB is the factor kernel's, K_NA rides with P @ FB).
 * Features and outputs are DEVICE float64 row-major whatever `dtype` (the storage of the coordinates and layer operands).  A
 * direction whose F and output are NULL and whose c is 0 is skipped; any other mix, both directions skipped, and K_NA without
 * P @ FB are errors.  Any c >= 1: a sweep takes up to 64 columns (in blocks of 16), wider F is worked in 64-column chunks
 * behind ONE pass 1 and one factor launch.  Pass 1 and the factors as mvf_assign runs them, then per direction and chunk one
 * sweep of the tiles whose entries feed v_mfma_f64_16x16x4_f64 straight from the accumulator layout the tile routine leaves
 * them in (P @ FB: the same sweep on the exchanged operands), and a kernel that adds the splits' partial products in split
 * order: no floating-point atomics, two calls give the same bits.  Arguments, checks and the empty-side return (0, nothing
 * touched) are mvf_assign's; every error is reported before anything is launched.  (An addition behind version 7.) */
size_t mvf_assign_apply_workspace_bytes(int64_t na, int64_t nb, int cb, int ca); /* 0 for an empty side */
int mvf_assign_apply(const void* xa4, int64_t na, const void* xb4, int64_t nb, const mvf_assign_layer* layers, int nlayers,
                     const double* model_mul, double sigma2, double sigma2_variance, double spatial_outlier,
                     const double* FB, int cb, int64_t ldfb, double* to_A, const double* FA, int ca, int64_t ldfa, double* to_B,
                     double* K_NA, double* K_NB, void* workspace, size_t workspace_bytes, mvf_dtype dtype, void* stream);

/* Column statistics of ONE layer's na x nb distance matrix d_ij, which is never written: what the code in front of the
 * reference's loop reduces its matrices to (`_init_guess_sigma2`, utils.py:1339-1354; `_init_probability_parameters`,
 * morpho_class.py:771-820; the mutual nearest neighbours of `_coarse_rigid_alignment`, :898-1041).  layer: ONE host struct as
 * mvf_assign_prepare / mvf_assign_label_prepare fill it (prob and param are not read); spatial distances are an "euc" layer
 * of the D coordinates.  Out (device, float64 whatever `dtype`), per column j over the rows i < na:
 *   cmin (nb)          min_i d_ij;
 *   rows / vals        for k > 0 (nb x k_eff int32 / float64, k_eff = min(k, na), mvf_assign_topk's layout): column j's k_eff
 *                      smallest entries in the total order (value ascending, row ascending); not touched for k == 0 (may be NULL);
 *   sums (2)           sum_ij d_ij and sum_ij d_ij^2 over the na x nb entries.
 * 0 <= k <= MVF_ASSIGN_TOPK_MAX.  The statistics of every ROW are the same call with the operands exchanged (Xp <-> Yp, a <-> b,
 * na <-> nb; a label layer: the transposed table and its row length): both kinds of distance are symmetric in how their
 * operands enter, and "kl" keeps its asymmetry because the operands are prepared per side.  Pass 1's tiling and row split;
 * every split writes partials that are combined in split order, minima and lists do not depend on the order: no
 * floating-point atomics, two calls give the same bits.  na < 1, nb < 1, k outside the range, a null pointer, a bad layer and a
 * small workspace are errors, reported before anything is launched.  (An addition behind version 7.) */
size_t mvf_assign_layer_stats_workspace_bytes(int64_t na, int64_t nb, int k); /* 0 for an empty side or k outside the range */
int mvf_assign_layer_stats(const mvf_assign_layer* layer, int64_t na, int64_t nb, int k, double* cmin, int32_t* rows,
                           double* vals, double* sums, void* workspace, size_t workspace_bytes, mvf_dtype dtype, void* stream);

/* ---- alignment: the O(N) glue of one iteration between the assignment and the non-rigid update (mvf_align.hip) ----------
 * With mvf_assign, mvf_gram, mvf_solve_minnorm*, mvf_apply and mvf_pinv_diag these three make the loop of
 * `Morpho_pairwise.run` (spateo/alignment/methods/morpho_class.py:280-294) device resident: per iteration the host reads
 * ONE block of MVF_ALIGN_MOMENT_DOUBLES float64 and does the 3 x 3 SVDs and the scalar updates.  Float64 arithmetic
 * whatever `dtype` (the storage of the x4 arrays), no floating-point atomics, partial sums added in a fixed order: two
 * calls give bit-identical results.  coordsA / coordsB / PXB / RnA / XAHat / PXB_term are n x 3 float64 (2-D data: third
 * column 0, R and t embedded in 3 x 3 / 3).  ABI version rule: entry points that only ADD to the table leave mvf_version
 * unchanged (as mvf_assign* did at 7); the version moves when an existing signature or layout changes. */
#define MVF_ALIGN_MOMENT_DOUBLES 64
/* Replaces: `_update_alpha` (morpho_class.py:1250-1252) and the `model_mul` of the next `_update_assignment_P` (:1087).
 * alpha_i = exp(psi(kappa_i + K_NA_spatial_i) - psi(kappa_i na + Sp_spatial)), model_mul_i = alpha_i exp(-SigmaDiag_i /
 * sigma2); psi = digamma for positive arguments (recurrence up to 10, then the asymptotic series through x^-14).
 * na == 0 launches nothing. */
int mvf_align_alpha(const double* kappa, const double* K_NA_spatial, const double* SigmaDiag, int64_t na, double Sp_spatial,
                    double sigma2, double* alpha, double* model_mul, void* stream);
size_t mvf_align_workspace_bytes(int64_t na, int64_t nb);
/* Replaces the reductions of `_update_rigid` (:1312-1318, 1343-1358), `_update_sigma2` (:1427) and `_get_optimal_R`
 * (:1451-1461), without P.  VnA4: x4 in `dtype` (mvf_apply's output; zeros before the non-rigid update has run); PXB = P
 * (coordsB - origin) as mvf_assign returns it for xb4 = coordsB - origin (origin: HOST double[3], NULL = 0); extra: optional
 * device scalar copied to out[50] (mvf_assign's `scalars`).  out (device, all 64 written):
 *   [0..2] K_NA.coordsA  [3..5] K_NA.VnA  [6..8] K_NB.coordsB  [9] Sp = sum K_NB  [10] sum K_NA  [11] Sp_spatial
 *   [12] Sp_sigma2  [13] sum K_NA_sigma2 SigmaDiag  [14..16] mu_XA  [17..19] mu_Vn  [20..22] mu_XB  (= [0..8] / Sp; 0 if Sp == 0)
 *   with xc = coordsA - mu_XA, vc = VnA - mu_Vn, pc = PXB - K_NA (mu_XB - origin) per row:
 *   [23..31] sum K_NA xc vc^T   [32..40] sum xc pc^T  (= XA_hat^T P XB_hat of :1357; its transpose is `A` of :1461)
 *   [41..43] sum K_NA xc   [44..46] sum K_NA vc   [47..49] sum pc   [50] extra   [51..63] 0
 * The second-order sums are taken on rows centred by the device's means; the host moves them to other means (the inlier
 * terms of :1328-1337) with the first-order centred sums [41..49], which is exact algebra on small numbers.
 * na == 0 or nb == 0 launches nothing. */
int mvf_align_moments(const double* coordsA, const void* VnA4, const double* K_NA, const double* K_NA_spatial,
                      const double* K_NA_sigma2, const double* SigmaDiag, const double* PXB, int64_t na, const double* coordsB,
                      const double* K_NB, int64_t nb, const double* origin, const double* extra, double* out, void* workspace,
                      size_t workspace_bytes, mvf_dtype dtype, void* stream);
/* Replaces: `RnA = coordsA R^T + t` (:1404), `XAHat = VnA + RnA` (:293), `PXB_term` (:1276) and the division that turns it
 * into the Gram stage's right-hand side.  Rt: HOST double[12] = R row-major, t.  Per cell, in this operation order:
 *   RnA_d = ((x_0 R[d][0] + x_1 R[d][1]) + x_2 R[d][2]) + t_d;  XAHat_d = VnA_d + RnA_d;  xa4_d = (dtype)(XAHat_d - origin_d);
 *   PXB_term_d = PXB_d - (RnA_d - origin_d) K_NA;  Y_d = K_NA != 0 ? PXB_term_d / K_NA : 0;  Y4 = (dtype)Y;  Pw = (dtype)K_NA.
 * Outputs may be NULL (skipped): RnA, XAHat, PXB_term (n x 3 float64), xa4, Y4 (n x 4, dtype), Pw (n, dtype).  VnA4 NULL = 0.
 * na == 0 launches nothing. */
int mvf_align_transform(const double* coordsA, const void* VnA4, const double* PXB, const double* K_NA, int64_t na,
                        const double* Rt, const double* origin, double* RnA, double* XAHat, void* xa4, double* PXB_term,
                        void* Y4, void* Pw, mvf_dtype dtype, void* stream);

/* ---- alignment, SVI mode: one batch of the B slice per iteration, running averages with step_size (:749-760, 894-896) ----
 * Three additions to the table (mvf_version stays 7 by the rule above).  Float64 arithmetic whatever `dtype`, no atomics,
 * every output element written by one lane: two calls give bit-identical results. */
/* Replaces: `self.coordsB[self.batch_idx, :]` and `layer[self.batch_idx]` (:1105-1107, 1149, 1161, 1270, 1315, 1345) for
 * batch_idx[j] = perm[(start + j) mod nb], j < bs - with start = (-iter bs) mod nb the batch `_update_batch` (:894-896) draws
 * at iteration `iter` from the initial `batch_perm`.  One launch copies, bit for bit, into contiguous batch buffers: the rows
 * of xb4 (nb x 4, dtype) -> xb4_out (bs x 4), of coordsB (nb x 3 float64) -> coordsB_out (bs x 3) and, per layer l < nlayers
 * (0 .. MVF_ASSIGN_MAX_LAYERS host structs; only Yp, b, ld and metric are read), of layers[l].Yp (nb x ld, dtype) -> Yp_out[l]
 * (bs x ld) and layers[l].b -> b_out[l] (bs float64).  For a layer with metric MVF_ASSIGN_LABEL only b (the B labels) is
 * gathered: Yp and Yp_out[l] are not read and may be NULL, ld >= 1 is the table's row length.  Yp_out / b_out: HOST arrays of nlayers DEVICE pointers.  The prepared
 * rows move as 16-byte chunks, consecutive lanes on consecutive chunks of a row; xb4, xb4_out, Yp and Yp_out must be 16-byte
 * aligned and ld a multiple of 16.  perm: DEVICE int32, a permutation of 0 .. nb - 1 - the CALLER guarantees it (the kernel
 * reads row perm[.] unchecked); 0 <= start < nb, bs <= nb < 2^31.  bs == 0 launches nothing. */
int mvf_align_gather(const int32_t* perm, int64_t nb, int64_t start, int64_t bs, const void* xb4, void* xb4_out,
                     const double* coordsB, double* coordsB_out, const mvf_assign_layer* layers, int nlayers,
                     void* const* Yp_out, double* const* b_out, mvf_dtype dtype, void* stream);
/* Replaces: `_update_alpha` in SVI mode (:1240-1247) and the `model_mul` of the next `_update_assignment_P` (:1087).
 *   a_i = exp(psi(kappa_i + K_NA_spatial_i) - psi(kappa_i na + Sp_spatial))        (mvf_align_alpha's expression and psi)
 *   alpha_i = step < 1 ? (step a_i) + ((1 - step) alpha_i) : a_i;   model_mul_i = alpha_i exp(-SigmaDiag_i / sigma2)
 * alpha is read and overwritten; Sp_spatial is the BLENDED sum; 0 < step <= 1.  step == 1 gives mvf_align_alpha's bits. */
int mvf_align_alpha_svi(const double* kappa, const double* K_NA_spatial, const double* SigmaDiag, int64_t na, double Sp_spatial,
                        double sigma2, double step, double* alpha, double* model_mul, void* stream);
/* Replaces: the blended `PXB_term` of `_update_nonrigid` in SVI mode (:1270-1274).  Per cell, d = 0, 1, 2, in this order:
 *   now_d = PXB_d - (RnA_d - origin_d) K_NA;   PXB_term_d = (step now_d) + ((1 - step) PXB_term_d)        (in place, float64)
 *   Y4_d = (dtype)PXB_term_d, Y4_3 = 0;   Pw = (dtype)K_NA
 * RnA (na x 3 float64) as mvf_align_transform wrote it; PXB = P (coordsB[batch] - origin); origin: HOST double[3], NULL = 0.
 * Rows with K_NA == 0 keep the earlier batches' share, so Y4 is the right-hand side for UNIT weights (mvf_gram_stages with
 * MVF_GRAM_STAGE_RHS | MVF_GRAM_STAGE_REDUCE_RHS, P = 1) and Pw the weights of the Gram matrix.  PXB_term must hold finite values (zeros before the first
 * non-rigid update, :760); 0 < step <= 1.  na == 0 launches nothing. */
int mvf_align_transform_svi(const double* RnA, const double* PXB, const double* K_NA, int64_t na, const double* origin,
                            double step, double* PXB_term, void* Y4, void* Pw, mvf_dtype dtype, void* stream);

/* ---- PCA across slices: the cache of mvf_ublk_build filled from data (mvf_pca.hip) ----------------------------------------
 * Five additions to the table (mvf_version stays 7 by the rule above).  A PCA of the stacked n_total x g matrix X of several
 * slices is  means -> cache of Xc = X - mean -> G = Xc^T Xc -> eigenvectors V -> scores Xc V;  the entry points here do the
 * first two, the rest runs UNCHANGED on the cache: mvf_gram_cached(MVF_GRAM_STAGE_TILES | MVF_GRAM_STAGE_REDUCE) with m = g and
 * P = 1 (x4 / ctrl4: any non-NULL pointer, neither stage reads them; y4, R: NULL), mvf_apply_cached with C = V (Yd: zeros).
 * A slice is n rows of the stacked matrix starting at global row `row0`; the slices are handed in by rising row0, from 0, on
 * one stream, and the call with row0 + n == n_total finishes the job (n_total = n, row0 = 0: one matrix, one call).  Input
 * matrices are row-major n x g, float32 (x_is_f32 / data_is_f32 != 0) or float64.  Arguments are validated before any HIP call.
 *
 * Replaces: `group_pca` (spateo/alignment/utils.py:88-149: `ad.concat` of the slices + `sc.tl.pca`), each of them. */
/* mvf_colmeans: mean[j] = (sum_i X[i][j]) / n_total, g float64, written by the call that ends at n_total.  The sum runs over
 * fixed blocks of 1024 global rows, the rows of a block in row order, then the blocks in order - float64, no atomics: the
 * result depends on the stacked matrix only (not on where it is cut into slices), and two calls give the same bits.
 * workspace: mvf_colmeans_workspace_bytes(n_total, g), 8-byte aligned, the same buffer for every slice of a matrix.
 * Replaces: the centring inside `sc.tl.pca(..., zero_center=True)` of alignment/utils.py:88-149. */
size_t mvf_colmeans_workspace_bytes(int64_t n_total, int64_t g);
int mvf_colmeans(const void* x, int x_is_f32, int64_t n, int64_t g, int64_t n_total, int64_t row0, double* mean,
                 void* workspace, size_t workspace_bytes, void* stream);
/* mvf_ublk_pack: (dtype)((double)X[i][j] - mu[j]) into the cache of mvf_ublk_build - same layout Ublk[g/16][n_total][16], same
 * size mvf_ublk_bytes(n_total, g, dtype) - at rows row0 .. row0 + n; mu (g float64, device) NULL = no centring.  The columns
 * g .. roundup(g, 128) of those rows are written as zeros, and the call that ends at n_total zeroes the rows n_total ..
 * roundup(n_total, 256): after the last slice every element of the cache has been written once.  ublk: 16-byte aligned.
 * Replaces: the operand of the SVD inside `sc.tl.pca` of alignment/utils.py:88-149 (the centred, concatenated matrix). */
int mvf_ublk_pack(const void* x, int x_is_f32, int64_t n, int64_t g, const double* mu, int64_t n_total, int64_t row0,
                  void* ublk, size_t ublk_bytes, mvf_dtype dtype, void* stream);
/* The same two from CSR: indptr (n + 1 int64), indices (int32), data (float32 / float64), all on the device.  The contract is
 * mvf_assign_prepare_csr's: distinct column indices within a row; an entry whose column is outside [0, g) is skipped, never
 * used as an address; indptr is the caller's to validate.  Chunks of rows are expanded into `staging` (>= one row = g elements
 * of the data's type, 8-byte aligned; as many rows per chunk as it holds) and go through the dense kernels: bit for bit what
 * the dense entry points give for the densified matrix, whatever the staging size.  No n x g copy of the input is made.
 * Replaces: `.X` of the concatenated slices as `sc.tl.pca` reads it when it is sparse (alignment/utils.py:88-149). */
int mvf_colmeans_csr(const int64_t* indptr, const int32_t* indices, const void* data, int data_is_f32, int64_t n, int64_t g,
                     int64_t n_total, int64_t row0, double* mean, void* workspace, size_t workspace_bytes, void* staging,
                     size_t staging_bytes, void* stream);
int mvf_ublk_pack_csr(const int64_t* indptr, const int32_t* indices, const void* data, int data_is_f32, int64_t n, int64_t g,
                      const double* mu, int64_t n_total, int64_t row0, void* ublk, size_t ublk_bytes, void* staging,
                      size_t staging_bytes, mvf_dtype dtype, void* stream);

/* ---- down-sampling: TRN, nearest row, k-means (mvf_sample.hip) -------------------------------------------------------------
 * Five additions to the table (mvf_version stays 7 by the rule above).  Float64 arithmetic whatever the package's cell dtype -
 * the samplers return indices -, every sum of squares ((d0 d0) + d1 d1) + d2 d2 without fused multiply-add, no atomics, every
 * output element written by one lane with ordinary vector stores: two calls give bit-identical results.  Rows have 1 <= d <= 3
 * float64 columns, row-major, no padding.  Arguments are validated before any HIP call. */
#define MVF_TRN_MAX_NODES 4096
/* One TRN problem: every pointer a DEVICE pointer.  X (N x d); w_idx (n int64): the start draw, W starts as X[w_idx]; p_idx
 * (T int64): the sample of every step; l, ep (T float64): the step's schedule values, computed by the HOST as the reference
 * computes them; kc (T float64, NULL when the cutoff c is 0): -l log(c / ep); W (n x d): the nodes, out.  A row index outside
 * [0, N) is clamped into it before it is used as an address. */
typedef struct mvf_trn_problem {
    const double* X;
    int64_t N;
    int64_t d;
    int64_t n;
    int64_t T;
    const int64_t* w_idx;
    const int64_t* p_idx;
    const double* l;
    const double* ep;
    const double* kc;
    double* W;
} mvf_trn_problem;
/* Replaces: `TRNET.run` / `TRNET.runOnce` (spateo/alignment/methods/sampling.py:103-155) for `nproblems` slices at once.
 * problems: HOST array.  One workgroup per problem runs all T steps, strictly in order, the nodes in registers; per step
 *   D = p - W;  sD_i = ((D_i0 D_i0) + D_i1 D_i1) + D_i2 D_i2;  k_i = #{j : (sD_j, j) < (sD_i, i)}  (the stable rank: the lower
 *   node first among equal distances);  W_i += (ep exp(-k_i / l)) D_i  for every node (kc NULL) or for k_i < kc.
 * Up to 32 problems share a launch (more: one launch per 32); no workgroup waits on another.  n <= MVF_TRN_MAX_NODES; a problem
 * with n == 0 is skipped, nproblems == 0 launches nothing. */
int mvf_trn(const mvf_trn_problem* problems, int nproblems, void* stream);
/* Replaces: the nearest-neighbour query that turns nodes into cells - `k_nearest_neighbors(X, query_X=W, k=0)` of `trn`
 * (sampling.py:214-222) and `nearest_neighbors(C, X, k=1)` of `sample_by_kmeans` (:255).  idx[i] (n int64) = the row of X
 * (N x d) nearest to Q[i] (n x d): exact, the smallest index among equal squared distances.  workspace:
 * mvf_nearest_rows_workspace_bytes(N, n) (0 up to 4096 rows), 8-byte aligned.  n == 0 launches nothing. */
size_t mvf_nearest_rows_workspace_bytes(int64_t N, int64_t n);
int mvf_nearest_rows(const double* X, int64_t N, int d, const double* Q, int64_t n, int64_t* idx, void* workspace,
                     size_t workspace_bytes, void* stream);
/* Replaces: `scipy.cluster.vq.kmeans2(X, C0, iter, minit="matrix", missing="warn")` of `sample_by_kmeans` (sampling.py:254).
 * C (n x d): the start matrix in, the centroids out.  `iter` >= 1 Lloyd steps are queued on the stream with no host round trip
 * between them: labels (N int32) = argmin of the squared distance, the first centroid among equal ones (vq's rule); centroid =
 * sum of its members / their number, the sum taken over fixed blocks of rows (a function of N alone) in row order and the
 * blocks in order; a cluster without members keeps its centroid.  labels are those of the last step's assignment (made with the
 * centroids BEFORE its update, as kmeans2 returns them), counts (n int64) their histogram.  workspace:
 * mvf_kmeans_workspace_bytes(N, n), 8-byte aligned.  N == 0 or n == 0 launches nothing. */
size_t mvf_kmeans_workspace_bytes(int64_t N, int64_t n);
int mvf_kmeans(const double* X, int64_t N, int d, double* C, int64_t n, int iter, int32_t* labels, int64_t* counts,
               void* workspace, size_t workspace_bytes, void* stream);

/* ---- mesh correction: batched 2-D ICP, the cut of a transformed surface mesh (mvf_icp.hip) -------------------------------
 * Five additions to the table (mvf_version stays 7 by the rule above).  The conventions are the sampling section's: float64
 * arithmetic whatever the package's cell dtype, no fused multiply-add, no atomics, every output element written by one lane
 * with ordinary vector stores, two calls give bit-identical results, the lower index wins among equal distances.  Every sum
 * over points is taken in one fixed order: a lane of the 256 adds its points j = lane, lane + 256 in that order, the 64 lanes
 * of a wave fold by halving (i += i + 32, 16, .. 1), the four waves add in wave order.  Arguments are validated before any HIP
 * call.  Contours are row-major n x 2 float64 and must hold finite numbers.
 *
 * Thinning: a contour of n > subsample points (subsample > 0) is reduced to the rows floor(j n / subsample), j = 0 ..
 * subsample - 1.  A deviation: the reference draws `np.random.choice(n, subsample, replace=False)` from the global generator,
 * which cannot be pinned; a caller that wants that draw passes contours it has thinned itself. */
#define MVF_ICP_MAX_POINTS 512
/* One ICP problem: every pointer a DEVICE pointer.  contour_1 (n1 x 2): the data; contour_2 (n2 x 2): the model, the one that
 * moves; gamma (1 float64), stats (2 int32: the rounds run, the inliers of the last query): out; T_contour_2 (min(n2,
 * subsample) x 2 float64, may be NULL): the transformed - thinned - model points in the frame of contour_1, out; translation
 * (2 float64, may be NULL): what the reference returns for allow_rotation == 0 (:494), scale t + centre_1 - centre_2 with the t
 * of the LAST round (0 when that round found fewer than 3 inliers), out. */
typedef struct mvf_icp_problem {
    const double* contour_1;
    int64_t n1;
    const double* contour_2;
    int64_t n2;
    double* gamma;
    int32_t* stats;
    double* T_contour_2;
    double* translation;
} mvf_icp_problem;
/* Replaces: `ICP` (spateo/alignment/methods/mesh_correction_utils.py:404-498) up to its line 492, for D = 2 and `nproblems`
 * pairs of contours at once; the closing `solve_RT_by_correspondence` (:496) stays with the host.  problems: HOST array, copied
 * to `workspace` on the stream (it must stay untouched until the stream has passed the call).  One workgroup per problem, both
 * thinned contours in LDS:
 *   centre each at its mid-range (max + min) / 2, divide both by scale = (rms_1 + rms_2) / 2;  T = the model;  up to max_iter
 *   rounds:  d_j = the distance from T_j to its exact nearest data point;  inliers: d_j < inlier_threshold;  fewer than 3 of
 *   them: stop, T stays;  else the means of the inliers and of their partners, the translation between them
 *   (allow_rotation == 0) or R = V U^T of the 2 x 2 covariance H = U S V^T - the closed-form orthogonal polar factor of H^T, a
 *   reflection when det H < 0: the reference's loop corrects no determinant - and t = mean_1 - R mean_T;  T = R T + t;  stop
 *   when the mean inlier distance moved by less than error_threshold.
 *   gamma = #{d_j < gamma_threshold} / M with the distances of the last query;  T_contour_2 = scale T + centre_1.
 * max_iter >= 1; n1, n2 >= 1; min(n, subsample) <= MVF_ICP_MAX_POINTS (subsample <= 0: no thinning).  Up to 4096 problems share
 * a launch; no workgroup waits on another.  workspace: mvf_icp_batch_workspace_bytes(nproblems), 8-byte aligned.  nproblems == 0
 * launches nothing. */
size_t mvf_icp_batch_workspace_bytes(int64_t nproblems);
int mvf_icp_batch(const mvf_icp_problem* problems, int64_t nproblems, int max_iter, double error_threshold,
                  double inlier_threshold, double gamma_threshold, int subsample, int allow_rotation, void* workspace,
                  size_t workspace_bytes, void* stream);
/* Replaces: `_calculate_loss` (mesh_correction_utils.py:371-401) with `_transform_points` (:27-85),
 * `_extract_contours_from_mesh` (:224-238) and one `ICP(c, m_c, allow_rotation=True)` per slice under it, for n_T candidate
 * transformations at once (`_get_binary_values`, :350-367, calls it label_num^2 times per pair of parameters).
 * verts (V x 3 float64), edges (E x 2 int32: the unique edges of the triangles, built once by the host; an index outside
 * [0, V) is clamped into it), params (n_T x 5 float64: rotation about x, y, z in degrees, z translation, scale), heights (n_S),
 * contours (contour_total x 2: the slices' contours packed), offsets (n_S + 1 int64: slice s owns the rows offsets[s] ..
 * offsets[s + 1], clamped into [0, contour_total]): DEVICE.  mean: HOST double[3], the vertex mean.  Per transformation:
 *   p' = scale ((p - mean) (R_z R_y R_x)^T) + mean;  p'_z += translation - on z of EVERY vertex, what the reference's docstring
 *   says (its line :83 adds it to the first two rows instead);
 *   per height h: one point per edge whose ends classify differently under z >= h (VTK's contour rule: a vertex on the plane is
 *   above it), a + ((h - z_a) / (z_b - z_a)) (b - a) in x and y, in edge-index order; thinned; the ICP above with that slice's
 *   contour as the data;
 *   loss = (sum over slices, in order, of (1 - gamma)) / n_S, or 1e6 / n_S when any height cuts no edge (:397-399).
 * One workgroup per (transformation, slice), at most 4096 transformations per launch.  loss (n_T); gamma (n_T x n_S, 0 where
 * nothing is cut) and count (n_T x n_S int32: the contour sizes before thinning) may be NULL.  1 <= subsample <=
 * MVF_ICP_MAX_POINTS; 1 <= n_S < 2^24.  workspace: mvf_mesh_loss_workspace_bytes(n_T, n_S), 16-byte aligned, bounded by the launch chunk.
 * n_T == 0 launches nothing. */
size_t mvf_mesh_loss_workspace_bytes(int64_t n_T, int64_t n_S);
int mvf_mesh_loss(const double* verts, int64_t V, const int32_t* edges, int64_t E, const double* mean, const double* params,
                  int64_t n_T, const double* heights, const double* contours, const int64_t* offsets, int64_t contour_total,
                  int64_t n_S, int max_iter, double error_threshold, double inlier_threshold, double gamma_threshold,
                  int subsample, double* loss, double* gamma, int32_t* count, void* workspace, size_t workspace_bytes,
                  void* stream);
/* Replaces: `_extract_contours_from_mesh` (mesh_correction_utils.py:224-238: `mesh.contour(isosurfaces=z_values)`) after
 * `_transform_points`, for one transformation.  param: HOST double[5] as a row of params above; mean: HOST double[3].  Slice s
 * gets counts[s] (int32) = the number of crossing edges and its first min(counts[s], capacity) points at points[s][0 ..]
 * (n_S x capacity x 2 float64; 1 <= n_S < 2^24), the rest of the row untouched: the same points, in the same order, the loss kernel cuts. */
int mvf_mesh_contours(const double* verts, int64_t V, const int32_t* edges, int64_t E, const double* mean, const double* param,
                      const double* heights, int64_t n_S, int64_t capacity, double* points, int32_t* counts, void* stream);

/* ---- density of the cloud: the fused log of a kernel sum per (target, group of sources) (mvf_kde.hip) -------------------
 * Two additions to the table (mvf_version stays 7 by the rule above).  The six kernels of sklearn.neighbors.KernelDensity, with
 * r = dist / h and sklearn's strict support dist < h for the four compact ones:  log K = -r^2 / 2 | -r | 0 | log(1 - r^2) |
 * log(1 - r) | log cos(pi r / 2). */
enum {
    MVF_KDE_GAUSSIAN = 0,
    MVF_KDE_EXPONENTIAL = 1,
    MVF_KDE_TOPHAT = 2,
    MVF_KDE_EPANECHNIKOV = 3,
    MVF_KDE_LINEAR = 4,
    MVF_KDE_COSINE = 5
};
#define MVF_KDE_MAX_COLUMNS 64
/* Replaces: `KernelDensity(kernel=kernel, bandwidth=bandwidth).fit(coords).score_samples(coords)` of `pc_KDE`
 * (spateo/tdr/morphometrics/morphology.py:109), without its normalising constants: the caller adds log_norm(h, d, kernel) -
 * log(sum of the group's weights).  t4 (n x 4 targets), s4 (N x 4 sources): x4 layout of `dtype`, both centred by the caller
 * with the same centre; d in {1, 2, 3} (the unused coordinates are 0).  weight (N float64; NULL = 1): finite, zero or a normal
 * positive number.  group (N int32; NULL = every source in column 0): a source whose group lies outside [0, C) belongs to no
 * column.  1 <= C <= MVF_KDE_MAX_COLUMNS (the caller runs more columns in chunks).
 *   out[i, c] (n x C float64) = log sum_{j: group[j] == c, w_j > 0} w_j K(|t_i - s_j| / h), -inf when no such source is in
 *   reach (an empty group, all weights zero, a compact kernel with every distance >= h).
 * Every distance is formed from the coordinate differences in float64 whatever `dtype` (the storage of the coordinates only);
 * exponent, sum and logarithm are float64.  Two passes over tiles of 256 sources: the largest log term log w_j + log K_ij per
 * (target, column) first - log K at the nearest source when the weights are equal -, then sum_j exp(log w_j + log K_ij - that),
 * whose largest term is 1: a target 40 bandwidths from every source gets -800 - .., not log 0.  The compact kernels take the
 * largest weight in reach as their shift and add (w_j / shift) K_ij without an exp.  No atomics: the sources are split over
 * workgroups (a number fixed by n and N alone: at least 4096 sources each, about 1024 workgroups per column), the partials go to the workspace and are folded in split order; within a split a target's
 * terms are added in source order; two calls give equal bits.  workspace: mvf_kde_workspace_bytes(n, N, C), 8-byte aligned.
 * Refused: "bad shape" (n, N < 0, d outside 1 .. 3, C outside 1 .. 64, h <= 0 or not finite), "bad kernel", "bad dtype", "null
 * pointer", "workspace too small".  n == 0 or C == 0 returns 0 before anything is looked at; N == 0 fills out with -inf. */
int mvf_kde(const void* t4, int64_t n, const void* s4, int64_t N, int d, int kernel, double h, const double* weight,
            const int32_t* group, int C, double* out, void* workspace, size_t workspace_bytes, int dtype, void* stream);
/* Replaces: the memory `score_samples` (morphology.py:109) takes for itself.  (splits + 1) x n x C float64: the splits' partials
 * and the shifts; 0 for an empty or refused shape. */
size_t mvf_kde_workspace_bytes(int64_t n, int64_t N, int C);

/* ---- shape of the cloud: the per-subspace descriptors of the shape similarity (mvf_shape.hip) -----------------------------
 * Two additions to the table (mvf_version stays 7 by the rule above). */
#define MVF_SHAPE_MAX_NSUB 128
/* Replaces: the loop of `model_eigenvector` (spateo/tdr/morphometrics/shape_similarity.py:164-177) over `rough_subspace`
 * (15-56), `subspace_surface_fitting` (59-110), `dist_global_centroid_to_subspace` (113-120) and
 * `cos_global_centroid_to_subspace` (123-133).  float64 throughout and no dtype argument: the fit is a polynomial in raw
 * monomials whose condition number sits at 1 / eps, and float32 storage of the coordinates would decide its rank.
 *   pts (n x 3 float64, device), 1 <= n < 2^31.  lo, hi (3 x nsub float64 each, device; axis-major): the interval ends of the
 *   voxels, computed by the host with the reference's own expressions `min + j * size` and `(min + j * size) + size`.
 *   1 <= nsub <= MVF_SHAPE_MAX_NSUB.  order: 1 linear [x, y, 1], 2 quadratic [1, x, y, xy, x^2, y^2], 3 cubic
 *   [1, x, y, x^2, xy, y^2, x^3, x^2 y, x y^2, y^3].  centroid (3 float64, HOST): the mean of all points.
 * Outputs (device):
 *   point_voxel (n int32): the voxel (layer nsub^2 + line nsub + piece; piece x, line y, layer z) whose intervals hold the
 *     point with `lo <= x` and `x < hi`, or -1 when none does (an upper face of the cuboid when ceil(ptp) == ptp).  A point
 *     two intervals of one axis hold goes to the lower one - the reference would count it twice.
 *   per kept voxel (count >= 2), in voxel order, min(nsub^3, n / 2) entries each: voxel (int32), count (int64), cosine
 *     (|c_z - g_z| / |c - g|, c the voxel's centroid), dist (the mean distance from the global centroid to the 20 x 20
 *     surface of the fit over the voxel's own x, y extent), rank (int32: singular values above 2^-52 sigma_max, gelsd's
 *     cond=None; the coefficients are the minimum-norm solution), sv (2 float64: sigma_max, and the smallest kept singular
 *     value over sigma_max).
 *   counts (3 int64): the number of kept voxels, of points with voxel -1 (n_dropped), and of points two intervals of one axis
 *     hold (n_overlap).
 * The points are grouped by a stable sort on the voxel id, each voxel is fitted by one workgroup (Householder QR of the
 * streamed rows, one-sided Jacobi SVD of the triangle), every sum in an order fixed by the counts: two calls give equal bits.
 * workspace: mvf_shape_descriptors_workspace_bytes(n, nsub), 256-byte aligned.  Refused: "bad shape" (n, nsub), "bad order",
 * "null pointer", "workspace too small". */
int mvf_shape_descriptors(const double* pts, int64_t n, const double* lo, const double* hi, int nsub, int order,
                          const double* centroid, int32_t* point_voxel, int32_t* voxel, int64_t* count, double* cosine,
                          double* dist, int32_t* rank, double* sv, int64_t* counts, void* workspace, size_t workspace_bytes,
                          void* stream);
/* Replaces: the copies `rough_subspace` (shape_similarity.py:46-51) makes of the cloud.  The sort buffers of the grouping
 * and two int32 per voxel; 0 for a refused shape. */
size_t mvf_shape_descriptors_workspace_bytes(int64_t n, int nsub);

/* ---- digitization: the two Jacobi relaxations of the heat equation, whole loops on the device (mvf_heat.hip) -------------
 * Four additions to the table (mvf_version stays 7 by the rule above).  float64 throughout, no floating-point atomics: two calls
 * give equal bits.  Both entries run the whole loop, read the device's status block every few batches and return when it has
 * stopped: they block.  The stop rule is the reference's `while (err > max_err) and (itr <= max_itr)`, evaluated like that: a NaN
 * err (an all-zero field gives 0 / 0) ends the loop after one sweep, and floor(max_itr) + 1 sweeps run at most.
 * Host outputs of both: sweeps (the reference's `itr`), err (the last one; 1 when no sweep ran), hit_max_itr (1 when
 * err > max_err still held at the end: the sweep budget ended the loop). */
#define MVF_HEAT_MAX_STEPS 8
/* Replaces: the loop of `domain_heat_eqn_solver` (spateo/digitization/utils.py:508-522) with `effective_L2_error` (445-461).
 *   init (H x W float64, device): the heat field with the four boundary lines written (`init_field`); border, mask (H x W
 *   float64 each, device): `field_border` and `field_mask` as the reference takes them - a pixel is fixed when border != 0 or
 *   when it lies on the array's outer rows or columns, and the mask is a weight (its values multiply).  3 <= H, W < 2^20.
 *   One sweep: new[y, x] = 0.25 * (((old[y, x+1] + old[y, x-1]) + old[y+1, x]) + old[y-1, x]) on every pixel that is not fixed, the
 *   whole array over; S1 = sum (new - old)^2 mask, S0 = sum old^2 mask, err = sqrt(S1 / S0).
 *   block_steps: the sweeps one launch runs in LDS, 1 .. MVF_HEAT_MAX_STEPS (1: the plain one-sweep kernel), or 0 for the
 *   dispatcher's choice (MVF_HEAT_MAX_STEPS: faster at every raster measured).  The field does not depend on it, bit for bit.
 *   out (H x W float64, device): field * mask.
 * workspace: mvf_heat_grid_workspace_bytes(H, W), 256-byte aligned.  Refused, with nothing launched: "bad shape", "bad
 * block_steps", "null pointer", "workspace too small". */
int mvf_heat_grid(const double* init, const double* border, const double* mask, int64_t H, int64_t W, double max_err,
                  double max_itr, int block_steps, double* out, int64_t* sweeps, double* err, int* hit_max_itr,
                  void* workspace, size_t workspace_bytes, void* stream);
/* Replaces: the copies the loop makes per sweep (utils.py:512-516).  The status block, two fields, MVF_HEAT_MAX_STEPS pairs of
 * partial sums per 32 x 64 tile and one byte per pixel; 0 for a refused shape. */
size_t mvf_heat_grid_workspace_bytes(int64_t H, int64_t W);
/* Replaces: the loop of `digitize_general` (spateo/digitization/utils.py:553-575) and its dense N x N `adj_mtx`.
 *   indptr (n + 1 int64), indices (nnz int32), values (nnz float64): the CSC arrays of `adj_mtx`, on the HOST - for node j the
 *   rows i with A_ij != 0 in ascending i; they are checked here and copied into the workspace.  fixed_value (n float64, HOST):
 *   the reference's `mask_field`, which is also the starting field.  1 <= n < 2^31.
 *   One sweep: new_j = sum_i old_i A_ij, added one after the other in ascending i from 0; a node with fixed_value != 0 then takes
 *   fixed_value (heat 0 is not held).  S1 = sum (new - old)^2, S0 = sum new^2, err = sqrt(S1 / S0).  One launch per sweep.
 *   out (n float64, device): the field.
 * workspace: mvf_heat_graph_workspace_bytes(n, nnz), 256-byte aligned.  Refused, with nothing launched: "bad shape", "null
 * pointer", "bad indptr" (not from 0, or falling), "index out of range", "workspace too small". */
int mvf_heat_graph(const int64_t* indptr, const int32_t* indices, const double* values, const double* fixed_value, int64_t n,
                   double max_err, double max_itr, double* out, int64_t* sweeps, double* err, int* hit_max_itr, void* workspace,
                   size_t workspace_bytes, void* stream);
/* Replaces: the dense `adj_mtx` (n x n float64) of `digitize_general`.  The status block, three vectors, the partial sums and the
 * CSC arrays; 0 for a refused shape. */
size_t mvf_heat_graph_workspace_bytes(int64_t n, int64_t nnz);

/* ---- a kernel along the tissue: exact k nearest neighbours and graph distances on the device (mvf_graph.hip) ---------------
 * Four additions to the table (mvf_version stays 7 by the rule above).  float64 throughout whatever the cell dtype, no
 * floating-point atomics: two calls give equal bits.  mvf_knn and mvf_graph_sssp are asynchronous on `stream` and never block. */
#define MVF_KNN_MAX_K 64
#define MVF_SSSP_STATUS 4
/* Replaces: `kneighbors_graph(points, knn, mode="distance", include_self=False)` of `construct_knn_graph`
 * (spateo/alignment/methods/utils.py:1176), sklearn's KD-tree query on the host.
 *   points (n x d float64 row-major, device, finite): d = 2 or 3, 1 <= k <= MVF_KNN_MAX_K, k < n < 2^31.
 *   idx (n x k int32), dist (n x k float64): the k nearest OTHER points of each point, every row ascending by (distance, index).
 *   A point is left out of its own list by index, not by distance: a duplicate of it is a neighbour at distance 0.  The distance
 *   is sqrt((dx dx + dy dy) + dz dz) of explicit differences, no fused multiply-add: what sklearn's KD-tree computes.  Among
 *   equal distances the smaller index wins (sklearn's order there is unspecified).
 *   A uniform grid of about n / k cells (at most 2^24), the points ordered by cell with the radix sort of mvf_unique_rows; one
 *   query per lane walks Chebyshev rings of cells until its k-th distance lies inside the region visited.  A cloud that falls
 *   into one cell (n < 2 k, or a zero extent) is searched exactly all the same, merely slowly.  The cell edge comes from the
 *   box's volume over the axes the cloud extends along, (V k / n)^(1/d'): a thin slab or a line keeps about k points per cell.
 * workspace: mvf_knn_workspace_bytes(n, d, k), 256-byte aligned.  Refused, with nothing launched: "bad shape", "null pointer",
 * "256-byte aligned", "workspace too small". */
int mvf_knn(const double* points, int64_t n, int d, int k, int32_t* idx, double* dist, void* workspace, size_t workspace_bytes,
            void* stream);
/* Replaces: the dense N x N array `A.toarray()` of `construct_knn_graph` (utils.py:1177).  The sort buffers, the points in cell
 * order with their indices, and one offset per cell; 0 for a refused shape. */
size_t mvf_knn_workspace_bytes(int64_t n, int d, int k);
/* Replaces: the loop of `networkx.single_source_dijkstra` calls of `con_K_graph` (utils.py:1207-1213), one per inducing variable.
 *   indptr (n + 1 int64), indices (nnz int32), weights (nnz float64, >= 0): the CSR arrays of an undirected graph, on the device
 *   (both directions of every edge stored); an index outside 0 .. n - 1 is skipped.  1 <= n < 2^31, m <= 2^20, n m <= 2^39 - 256.
 *   sources (m int32, device, repeats allowed; one outside 0 .. n - 1 sets nothing), dist (n x ld float64, ld >= m): column s
 *   holds the distances from sources[s], one row per node.  init != 0: +inf everywhere and 0 at (sources[s], s) first.
 *   sweeps: the Bellman-Ford sweeps this call queues (0 .. 65536).  A sweep replaces every entry in place by
 *   min(d[v], min over the edges (v, u) of d[u] + w): every stored value is the left-to-right sum along a path, and the fixed
 *   point - the minimum of that sum over all paths, which is what Dijkstra returns - does not depend on the order of the
 *   relaxations; values short of it do.  An unreachable node keeps +inf.
 *   status (MVF_SSSP_STATUS int64, device, overwritten): [0] the entries lowered by the sweeps of this call, [1] those of its
 *   last sweep, [3] the sweeps queued.  Only zero or non-zero means anything: a sweep that finds the sweep before it at zero
 *   returns at once, and a caller that reads [0] == 0 (mvf_read_back) has the fixed point.  A path has at most n - 1 edges, so
 *   n sweeps in all reach it.
 * Refused, with nothing launched: "bad shape", "bad sweeps", "null pointer". */
int mvf_graph_sssp(const int64_t* indptr, const int32_t* indices, const double* weights, int64_t n, int64_t nnz,
                   const int32_t* sources, int64_t m, double* dist, int64_t ld, int init, int sweeps, int64_t* status,
                   void* stream);
/* Replaces: the same statement as mvf_pinv_diag (`SigmaDiag`, morpho_class.py:1295-1297) when U is not con_K of coordinates -
 * the `kernel_type="geodist"` branch, where U = con_K_graph(graph, inducing_idx) (morpho_class.py:865-871).
 *   diag_out[n] = (U pinv(A) U^T)_nn with the rows of U read from the operand cache `ublk` (mvf_ublk_build / mvf_ublk_pack for
 *   these n and m, of `dtype`; ublk_bytes >= mvf_ublk_bytes(n, m, dtype)) instead of regenerated: the one consumer of U that had
 *   no cache-reading form.  One kernel with mvf_pinv_diag behind the point where the kernel value is formed: on a cache that
 *   mvf_ublk_build made of (x4, ctrl4, beta) the two give equal bits.  workspace, rcond, lowrank and the synchronisation on the
 *   lowrank path as mvf_pinv_diag. */
int mvf_pinv_diag_cached(const void* ublk, size_t ublk_bytes, int64_t n, int64_t m, double rcond, int lowrank, double* diag_out,
                         void* workspace, size_t workspace_bytes, mvf_dtype dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVF_H */
