"""Inputs, references, bounds and case tables of the kernel-level edge tests of csrc/mvf_gram.hip
(tests/test_gpu_gram_kernels.py on the device, tests/test_gram_kernel_refs.py without one).

What is compared
----------------
The Gram stage computes  G = U^T diag(P) U  (m x m)  and  R = U^T diag(P) Y  (m x 3)  with U the n x m kernel values in the
cell dtype T.  The kernel values themselves are NOT under test here (mvf_con_k is pinned elsewhere, and the GPU module asserts
that the cache holds mvf_con_k's bits): the references are built from the kernel values THE DEVICE PRODUCED, so what is left
is accumulation, indexing, masking, slices, phases and the two reductions, and the bound follows from summation theory instead
of from the cell dtype.

  G_ref[i, j] = sum_n P_n U_ni U_nj          in np.longdouble (80-bit on x86, eps 1.08e-19), P and U widened exactly from T
  R_ref[j, c] = sum_n U_nj w_nc              w = (T)(y * p): NumPy's multiply in the cell dtype is the IEEE multiply the
                                             rhs kernel stages, so w holds the kernel's bits

The bound
---------
Let u = 2^-53.  A term of G is t_n = P_n U_ni U_nj >= 0.  float32 mode: (double)U_ni (double)P_n has 48 significant bits and
is exact; it enters v_mfma_f64_16x16x4_f64 / fma with (double)U_nj, where the product is not rounded before the add.  float64
mode: (double)A pd = U_ni P_n is rounded once (1 + d), |d| <= u, and then enters the same chain.  So every term is rounded at
most once when it is formed and every addition rounds once.  The accumulators start at an exact 0, padded cells and padded
control points add exact zeros, and the slice / phase folds (eight interleaved sums combined pairwise, `acc += G` between
phases) only change the ORDER: the whole sum is a summation tree over the n live terms, in which a term passes through at most
n - 1 rounded additions.  Hence, for any order (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2),

  |G - G_exact| <= gamma_n sum_n |t_n| = gamma_n G_exact,      gamma_k = k u / (1 - k u),

and with the reference's own error (<= n 1.08e-19 relative, three decimal digits below u) and (n + 2) u >= gamma_n (1 + ...)
for every n used here (n u < 1e-11):

  |G - G_ref| <= (n + 2) u G_ref                               per element (all terms are >= 0)
  |R - R_ref| <= (n + 2) u sum_n |U_nj w_nc|                   per element (fma(k, w, r): exact product, one rounding)

About 5e-13 relative at n = 4097 in BOTH cell dtypes.  Underflow: float32 kernel values are >= 2^-149, so no product of a float32
mode underflows in float64.  In float64 mode U_ni P_n and the sums can fall below 2^-1022; there a rounding is an ABSOLUTE error
of at most 2^-1075 (half the smallest subnormal; additions of subnormals are exact), times U_nj <= 1, once per term: the bound
gets the absolute term n 2^-1074 per element (`abs_term`), which is what the derivation gives and 4e-320 at n = 8193.

Sampled reference (above FULL_COST = 1.6e8 terms n m^2, of which the longdouble matmul does the upper half in about a second):
all elements of 40 rows (`sample_rows`: first and last row of every tile, 16-block edges, the last live row - with the exact
symmetry of G that is every tile pair's first and last live row and column) from float64 BLAS, asserted at 2 x the bound since
the reference's own error obeys the same gamma_n, and 64 single elements (`sample_elements`) whose terms are split into exact
float64 pieces (Dekker's two-product) and summed by math.fsum, which is exact: asserted at 1 x the bound.

Mirrored constants: the boundaries the case tables sit on follow these constants of mvf_gram.hip; tests/test_gram_kernel_refs.py
::test_cases_sit_on_every_boundary computes from them that every boundary is hit and says which constant moves which."""
import math

import numpy as np

L = np.longdouble
U_ROUND = 2.0 ** -53

# ---- constants of csrc/mvf_gram.hip (mirrored; a change there moves the boundaries below) ----
GT = 128              # Gram tile edge                                            (GT)
UB = 16               # control points per cached block, one MFMA block           (UB)
GCHUNK = 256          # cells per LDS stage = granularity of slices and of n_pad  (GCHUNK)
KSTEP = 4             # cells per v_mfma_f64_16x16x4_f64
EDGE_COLS = 4 * UB    # last tile column with <= 64 live points: edge shape / edge2 (live_cols <= 4 * UB; GT / 2 in make_plan)
SUPER_CELLS = {"float32": 64, "float64": 32}  # 4096 / (UB * sizeof(T)): cells per superblock of the cached kernels (SUPER * UGT * 4)
RHS_COLS = 512        # control points per rhs workgroup                          (RHS_COLS = 256 * RHS_CPT)
UBLK_COLS = 512       # control points per ublk_build workgroup column            (cb_per_block * UB)
REDUCE_WAYS = 8       # interleaved partial sums of gram_reduce_kernel
RHS_LANES = 16        # slice lanes of rhs_reduce_kernel; also its control points per workgroup
RHS_WANT = 1024       # rhs jobs make_plan aims at (want_r)
MIN_BUFFER_BYTES = 3e9                                     # smallest partial-tile budget (make_plan: std::max(3e9, ...))
MIN_TILES = int(MIN_BUFFER_BYTES // (GT * GT * 8))         # = 22 888 partial tiles

BETA = 0.003
SPREAD = 30.0
UNDERFLOW_BETA = 0.05
MUTATION_FACTOR = 100.0
FULL_COST = 1.6e8     # n m^2 up to which the longdouble reference is computed in full (513^3 = 1.35e8, 4097 x 193^2 = 1.53e8)


def cdiv(a, b):
    return -(-int(a) // int(b))


def np_dtype(dtype):
    return np.float32 if dtype == "float32" else np.float64


def pads(n, m):
    """(n_pad, m_pad) of the cache Ublk[m_pad / 16][n_pad][16]."""
    return cdiv(n, GCHUNK) * GCHUNK, cdiv(m, GT) * GT


def align_up(x, a=256):
    return cdiv(x, a) * a


def rhs_plan(n, m):
    """(rslice_len, rslices) of make_plan: independent of the device."""
    rcolblocks = cdiv(m, RHS_COLS)
    want = max(1, cdiv(RHS_WANT, max(1, rcolblocks)))
    rsl = max(cdiv(cdiv(n, want), GCHUNK) * GCHUNK, GCHUNK)
    return rsl, max(1, cdiv(n, rsl))


def forced_plan(n, m, dtype, slice_len):
    """make_plan with the developer option slice_len set (then nothing depends on the device): a dict of nt, npairs, edge2,
    nslices, fit, nphases, phase_slices and the three parts of mvf_gram_workspace_bytes."""
    nt = cdiv(m, GT)
    npairs = nt * (nt + 1) // 2
    cache_bytes = float(n) * float(m) * (8.0 if dtype == "float64" else 4.0)
    budget = min(20e9, max(MIN_BUFFER_BYTES, 0.1 * cache_bytes))
    fit = max(1, max(npairs, int(budget // (GT * GT * 8))) // npairs)
    sl = max(GCHUNK, slice_len // GCHUNK * GCHUNK)
    nslices = max(1, cdiv(n, sl))
    nphases = cdiv(nslices, fit)
    phase_slices = cdiv(nslices, nphases)
    rsl, rslices = rhs_plan(n, m)
    wide = align_up(8 * min(pads(n, m)[0], phase_slices * sl)) if dtype == "float32" else 0
    return dict(nt=nt, npairs=npairs, edge2=int(dtype == "float64" and nt >= 2 and m - (nt - 1) * GT <= GT // 2), slice_len=sl,
                nslices=nslices, fit=fit, nphases=nphases, phase_slices=phase_slices, gram_bytes=phase_slices * npairs * GT * GT * 8,
                rhs_bytes=rslices * m * 4 * 8, widened_p_bytes=wide)


# ------------------------------------------------------------------------------------------------------------ inputs
P_KINDS = ("uniform", "zero", "one", "holes", "floor")


def inputs(n, m, p_kind="uniform", seed=None):
    """Host float64 X (n, 3), ctrl (m, 3), Y (n, 3), P (n,) and the centre both point sets are shifted by.  Control points of
    their own (m may exceed n).  P: "uniform" in [1e-5, 1]; "zero"; "one"; "holes" = exact zeros over the whole k-steps 1 and
    the last full one, over cells 9 .. 10 inside a k-step and over the whole second 256-cell slice; "floor" = the E-step's
    floor 1e-5 on every seventh cell and exact zeros on every third, next to ordinary weights."""
    rng = np.random.default_rng(100003 * n + 17 * m + 1 if seed is None else seed)
    X = rng.uniform(-1, 1, (n, 3)) * SPREAD
    ctrl = rng.uniform(-1, 1, (m, 3)) * SPREAD
    Y = rng.standard_normal((n, 3))
    P = rng.uniform(1e-5, 1.0, n)
    if p_kind == "zero":
        P[:] = 0.0
    elif p_kind == "one":
        P[:] = 1.0
    elif p_kind == "holes":
        P[KSTEP:2 * KSTEP] = 0.0
        P[9:11] = 0.0
        P[GCHUNK:2 * GCHUNK] = 0.0
        last = (n // KSTEP - 1) * KSTEP
        if last >= 0:
            P[last:last + KSTEP] = 0.0
    elif p_kind == "floor":
        P[::3] = 0.0
        P[1::7] = 1e-5
    elif p_kind != "uniform":
        raise ValueError(p_kind)
    center = ctrl.mean(0) if m else np.zeros(3)
    return dict(X=X, ctrl=ctrl, Y=Y, P=P, center=center)


def host_cell_inputs(case_inputs, dtype):
    """What HipKernels.to_x4 / a cast of P hand the kernels, restated on the host: centred in float64, rounded to the cell dtype."""
    T = np_dtype(dtype)
    c = case_inputs["center"][None, :]
    return ((case_inputs["X"] - c).astype(T), (case_inputs["ctrl"] - c).astype(T), case_inputs["Y"].astype(T),
            case_inputs["P"].astype(T))


def host_kernel_values(x3, c3, beta):
    """Kernel values in the cell dtype of x3 by the kernels' recipe (coordinates pre-scaled by sqrt(beta log2 e), exp2 of the
    negated squared distance), in NumPy arithmetic of that dtype: the census arithmetic of tests/test_gpu_gram_shared_cols.py.
    Not the device's bits (no fma, another exp2) - the host module needs kernel values LIKE the device's, not the same ones."""
    T = x3.dtype.type
    s = T(np.sqrt(beta * np.log2(np.e)))
    xs, cs = x3 * s, c3 * s
    d = xs[:, None, :] - cs[None, :, :]
    e = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).astype(T)
    with np.errstate(under="ignore"):
        return np.exp2(-e).astype(T)


def census(kv):
    """(normal, denormal, zero) counts of kernel values in their own dtype."""
    tiny = np.finfo(kv.dtype).tiny
    return int((kv >= tiny).sum()), int(((kv > 0) & (kv < tiny)).sum()), int((kv == 0).sum())


def rhs_weights(y3, P):
    """w = (T)(y * p), the weights rhs_kernel stages: one IEEE multiply in the cell dtype."""
    assert y3.dtype == P.dtype
    return y3 * P[:, None]


# ------------------------------------------------------------------------------------------------------------ references
def gram_reference(U, P):
    """G_ref (m x m, np.longdouble) from kernel values U (n x m) and P (n) in the cell dtype, widened exactly.  Only the tile
    rows' upper parts are multiplied (the longdouble matmul is ~15 ns per term); the rest is the mirror image."""
    n, m = U.shape
    G = np.zeros((m, m), dtype=L)
    if n == 0 or m == 0:
        return G
    Ul = U.astype(L)
    A = Ul * P.astype(L)[:, None]
    for i0 in range(0, m, GT):
        i1 = min(m, i0 + GT)
        G[i0:i1, i0:] = A[:, i0:i1].T @ Ul[:, i0:]
    iu = np.triu_indices(m, 1)
    G.T[iu] = G[iu]
    return G


def rhs_reference(U, W):
    """(R_ref, S) in np.longdouble: R_ref = U^T W and S = U^T |W|, the sum of the absolute terms the bound is relative to."""
    Ul, Wl = U.astype(L), W.astype(L)
    if U.shape[0] == 0:
        z = np.zeros((U.shape[1], W.shape[1]), dtype=L)
        return z, z.copy()
    return Ul.T @ Wl, Ul.T @ np.abs(Wl)


def abs_term(n):
    return np.ldexp(L(n), -1074)


def bound(scale, n):
    """(n + 2) u scale + n 2^-1074 per element (module docstring); `scale` = G_ref, or sum |U w| for R."""
    return L((n + 2) * U_ROUND) * np.abs(np.asarray(scale, dtype=L)) + abs_term(n)


def ratio(got, ref, bnd):
    """Largest |got - ref| / bound over the elements; an exact match counts 0 whatever its bound (n = 0: bound 0)."""
    diff = np.abs(np.asarray(got).astype(L) - np.asarray(ref, dtype=L))
    if diff.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, L(0), diff / np.asarray(bnd, dtype=L))
    return float(np.max(r))


def full_reference_affordable(n, m):
    return float(n) * m * m <= FULL_COST


def sample_rows(m, count=40):
    """`count` rows of G (fewer when m is smaller): the first and last row of every tile, the last live row, then 16-block
    edges inside the first, the middle and the last tile.  With G exactly symmetric (asserted bit for bit) all elements of
    these rows are every tile pair's first and last live row AND column."""
    nt = cdiv(m, GT)
    rows = []
    for t in range(nt):
        rows += [t * GT, min(m, (t + 1) * GT) - 1]
    rows.append(m - 1)
    for t in (0, nt // 2, nt - 1):
        for b in (1, 4, 7):
            rows += [t * GT + b * UB - 1, t * GT + b * UB]
    out = []
    for r in rows:
        if 0 <= r < m and r not in out:
            out.append(r)
    return np.array(sorted(out[:count]), dtype=np.int64)


def sample_elements(m, count=64, seed=5):
    """`count` single elements (i <= j): the four corners of the upper triangle's tile grid, then random ones."""
    nt = cdiv(m, GT)
    rng = np.random.default_rng(seed)
    el = [(0, 0), (0, m - 1), (m - 1, m - 1), ((nt - 1) * GT - 1, m - 1), ((nt - 1) * GT, m - 1), (GT - 1, GT), (GT, GT)]
    el = [(i, j) for i, j in el if 0 <= i <= j < m]
    while len(el) < count:
        i, j = sorted(int(v) for v in rng.integers(0, m, 2))
        el.append((i, j))
    return el[:count]


def gram_rows_blas(U, P, rows):
    """Rows `rows` of G from float64 BLAS (the sampled reference; its own error obeys gamma_n: compare at 2 x the bound)."""
    U64 = U.astype(np.float64, copy=False)
    A = U64[:, rows] * P.astype(np.float64)[:, None]
    return A.T @ U64


def _split(a):
    c = 134217729.0 * a  # 2^27 + 1 (Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    """p + e == a b exactly (Dekker; no underflow / overflow in the ranges used)."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def gram_element_exact(Ui, Uj, P):
    """sum_n P_n U_ni U_nj correctly rounded: every term as four exact float64 pieces, summed by math.fsum."""
    a, ae = _two_prod(P.astype(np.float64), Ui.astype(np.float64))
    p1, e1 = _two_prod(a, Uj.astype(np.float64))
    p2, e2 = _two_prod(ae, Uj.astype(np.float64))
    return math.fsum(np.concatenate([p1, e1, p2, e2]).tolist())


# ------------------------------------------------------------------------------------------------------------ emulation
def emulate_gram(U, P, slice_len):
    """G in float64 in the kernels' summation order: per slice a chain over its cells in k-steps of 4 (term = (U_i P) U_j,
    the row operand rounded once as `(double)A * pd`), slices folded into eight interleaved sums (slice s -> sum s % 8) and
    those combined pairwise, as gram_reduce_kernel does."""
    n, m = U.shape
    U64 = U.astype(np.float64)
    A = U64 * P.astype(np.float64)[:, None]
    sums = [np.zeros((m, m)) for _ in range(REDUCE_WAYS)]
    for s, n0 in enumerate(range(0, max(n, 1), slice_len)):
        acc = np.zeros((m, m))
        for k0 in range(n0, min(n, n0 + slice_len), KSTEP):
            for k in range(k0, min(n, k0 + KSTEP)):
                acc += A[k][:, None] * U64[k][None, :]
        sums[s % REDUCE_WAYS] += acc
    a = sums
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))


def emulate_rhs(U, W, rslice_len):
    """R in float64 in the kernels' order: per rhs slice a chain over its cells, slice s on lane s % 16 of rhs_reduce_kernel,
    the 16 lanes added in lane order."""
    n, m = U.shape
    U64, W64 = U.astype(np.float64), W.astype(np.float64)
    lanes = [np.zeros((m, W.shape[1])) for _ in range(RHS_LANES)]
    for s, n0 in enumerate(range(0, max(n, 1), rslice_len)):
        acc = np.zeros((m, W.shape[1]))
        for k in range(n0, min(n, n0 + rslice_len)):
            acc += U64[k][:, None] * W64[k][None, :]
        lanes[s % RHS_LANES] += acc
    t = np.zeros((m, W.shape[1]))
    for q in range(RHS_LANES):
        t = t + lanes[q]
    return t


# ------------------------------------------------------------------------------------------------------------ mutations
def _g64(U, P):
    U64 = U.astype(np.float64)
    return (U64 * P.astype(np.float64)[:, None]).T @ U64


def _r64(U, W):
    return U.astype(np.float64).T @ W.astype(np.float64)


def mutations(U, P, Y3, slice_len, rslice_len, dtype, p_kind):
    """{name: (G or None, R or None)}: what G / R would be with each targeted defect, in float64 BLAS (its own error is within
    2 x the bound; a mutation has to move an element by >= 100 x).  Only the mutations that apply to the case are returned;
    tests/test_gram_kernel_refs.py asserts which those are."""
    n, m = U.shape
    W = rhs_weights(Y3, P)
    G0, R0 = _g64(U, P), _r64(U, W)
    out = {}
    if p_kind == "zero":
        return out  # (every sum is exactly 0 whatever the defect; this case pins the exact zeros)
    if n >= 1 and P[n - 1] != 0:
        out["drop_last_cell"] = (_g64(U[:-1], P[:-1]), _r64(U[:-1], W[:-1]))
    if n > KSTEP:
        # the last whole k-step whose P is not all zero
        for q in range(n // KSTEP - 1, -1, -1):
            if P[q * KSTEP:(q + 1) * KSTEP].any():
                keep = np.r_[0:q * KSTEP, (q + 1) * KSTEP:n]
                out["drop_k_step"] = (_g64(U[keep], P[keep]), None)
                break
    nsl = cdiv(n, slice_len)
    if nsl >= 2:
        s = nsl - 2  # a whole slice (the last one may hold a single cell)
        if p_kind == "holes":
            s = 0  # (slice 1 of this P is all zero by design)
        keep = np.r_[0:s * slice_len, (s + 1) * slice_len:n]
        out["drop_slice"] = (_g64(U[keep], P[keep]), None)
    if nsl > REDUCE_WAYS:
        keep = np.r_[0:REDUCE_WAYS * slice_len, min(n, (REDUCE_WAYS + 1) * slice_len):n]
        out["reduce_skips_slice_8"] = (_g64(U[keep], P[keep]), None)
    if cdiv(n, rslice_len) > REDUCE_WAYS:
        keep = np.r_[0:REDUCE_WAYS * rslice_len, min(n, (REDUCE_WAYS + 1) * rslice_len):n]
        out["rhs_reduce_skips_slice_8"] = (None, _r64(U[keep], W[keep]))
    if m > GT:
        # tile (0, 1) stored transposed: element (r, c) of the 128 x 128 tile takes (c, r), padded columns being 0
        k = min(GT, m - GT)
        tile = np.zeros((GT, GT))
        tile[:, :k] = G0[0:GT, GT:GT + k]
        G = G0.copy()
        G[0:GT, GT:GT + k] = tile.T[:, :k]
        G[GT:GT + k, 0:GT] = G[0:GT, GT:GT + k].T
        out["transpose_off_diagonal_tile"] = (G, None)
    if m >= 2:
        G, R = G0.copy(), R0.copy()
        G[:, m - 1] = G0[:, m - 2]
        G[m - 1, :] = G[:, m - 1]
        R[m - 1] = R0[m - 2]
        out["last_column_from_its_neighbour"] = (G, R)
    if dtype == "float64" and p_kind in ("uniform", "floor", "holes"):
        P32 = P.astype(np.float32).astype(np.float64)
        out["p_rounded_to_float32"] = (_g64(U, P32), None)
    if dtype == "float32" and p_kind in ("uniform", "floor", "holes") and n >= 1:
        Wx = Y3.astype(np.float64) * P.astype(np.float64)[:, None]  # exact: not rounded to float32
        out["rhs_weights_not_rounded"] = (None, U.astype(np.float64).T @ Wx)
    return out


def padded_point_value(x3, beta):
    """Largest kernel value a padded control point would show if it were not masked: ublk_build_kernel stages it as the
    point (0, 0, 0), the centre of the shifted frame, and zeroes its column through the flag w = 0 alone."""
    return float(host_kernel_values(x3, np.zeros((1, 3), dtype=x3.dtype), beta).max()) if len(x3) else 0.0


# ------------------------------------------------------------------------------------------------------------ case tables
# Control points (at n = 257 and n = 65) and what each m reaches
M_TABLE = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 192, 193, 257, 385, 440, 511, 512, 513]
M_TABLE_NS = [257, 65]
# Cells (at m = 17 and m = 193)
N_TABLE = [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513]
N_TABLE_MS = [17, 193]
# Gram slices: slice_len forced to 256 at m = 130, n = 256 (k - 1) + 1 for k slices
SLICE_M = 130
SLICE_LEN = 256
SLICE_KS = [7, 8, 9, 16, 17]
# rhs slices are 256 cells at these sizes without any option: 15, 16, 17, 33 of them on the 16 lanes of rhs_reduce_kernel
RHS_SLICE_NS = [3840, 3841, 4097, 8193]
RHS_SLICE_M = 17
# P variants (forced 256-cell slices so that "holes" empties a whole slice)
P_CASE = (1025, 130)
# float32 underflow case (the shape and beta of tests/test_gpu_gram_shared_cols.py)
UNDERFLOW_CASE = (4097, 193)
# three phases
PHASE_CASE = (76289, 2049)
# dead work / stage masks / raw ABI
DEAD_MS = [129, 193, 257, 385]
DEAD_N = 300


def case(family, n, m, beta=BETA, p_kind="uniform", slice_len=0):
    return dict(family=family, n=n, m=m, beta=beta, p_kind=p_kind, slice_len=slice_len)


def case_id(c):
    return f"{c['family']}-n{c['n']}-m{c['m']}" + ("" if c["p_kind"] == "uniform" else f"-{c['p_kind']}")


M_CASES = [case("control points", n, m) for n in M_TABLE_NS for m in M_TABLE]
N_CASES = [case("cells", n, m) for m in N_TABLE_MS for n in N_TABLE]
SLICE_CASES = [case("gram slices", SLICE_LEN * (k - 1) + 1, SLICE_M, slice_len=SLICE_LEN) for k in SLICE_KS]
RHS_SLICE_CASES = [case("rhs slices", n, RHS_SLICE_M) for n in RHS_SLICE_NS]
P_CASES = [case("P", *P_CASE, p_kind=p, slice_len=SLICE_LEN) for p in ("zero", "one", "holes", "floor")]
UNDERFLOW = case("underflow", *UNDERFLOW_CASE, beta=UNDERFLOW_BETA)
SMALL_CASES = M_CASES + N_CASES + SLICE_CASES + RHS_SLICE_CASES + P_CASES + [UNDERFLOW]
PHASE = case("three phases", *PHASE_CASE, slice_len=SLICE_LEN)


def emulated_slice_len(c):
    """Slice length the host emulation uses: the forced one, else one slice of whole 256-cell chunks (any order obeys the
    bound; the device's plan picks its own)."""
    return c["slice_len"] or max(GCHUNK, cdiv(c["n"], GCHUNK) * GCHUNK)
