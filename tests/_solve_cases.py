"""Cases, references and bounds of the coefficient-solve edge suite (csrc/mvf_solve.hip, csrc/mvf_minnorm.hip,
csrc/mvf_chol_dev.h).  No torch, no GPU: tests/test_solve_kernel_refs.py proves the references and the bounds on the CPU,
tests/test_gpu_solve_kernels.py runs the device kernels against them.

Matrices have a spectrum known BY CONSTRUCTION: A = Q diag(lambda) Q^T with Q a product of Householder reflectors of random
unit vectors, formed in np.longdouble, rounded to float64 and symmetrised.  The reference coefficient is
C* = Q_keep diag(1 / lambda_keep) Q_keep^T R in np.longdouble, where "keep" is decided on the DESIGNED lambda (the cut-off
rcond * max|lambda| lies at least 10 x away from every designed eigenvalue and at least 10^3 separates kept from dropped
ones, so the kept set is unambiguous after rounding).  A is split into G and K with a non-trivial lambda_sigma2
(G = A - ls2 K in longdouble, then rounded), so the device's assembly kernels see both operands.

The bound on max|C - C*| / max|C*| per column is  C_BOUND m eps kappa_kept  (kappa_kept = lambda_max / min kept |lambda|
from the design).  C_BOUND is not invented: it is 16 x the largest ratio deviation / (m eps kappa_kept) of the float64
LAPACK route (np.linalg.eigh truncated solve, scipy.linalg.cho_solve) on the same rounded matrices over every case of this
module, rounded up to a power of two - profiles/solve_kernel_edges.md holds the measured ratios, and
tests/test_solve_kernel_refs.py asserts that they still fit.  The factor 16: the device diagonalises a Cholesky factor with
one-sided Jacobi, LAPACK a tridiagonal form with QR; both are backward stable with error constants that differ by O(1) to
O(10).  The defect tests of test_solve_kernel_refs.py show that the bound still separates a wrong kernel by >= 100 x."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
PAD = 64            # the drivers pad m to a multiple of 64 (mp)
LAMBDA_MAX = 3.7    # largest designed |eigenvalue| of every case (not a power of two)
# 16 x the largest measured ratio (2.15, np.linalg.eigh's truncated solve on the 2 x 2 "cluster" case: at m = 1 and 2 the
# rounding of the matrix itself is the whole error; from m = 63 on the LAPACK ratios are <= 0.03) = 34.4, rounded up to a
# power of two: profiles/solve_kernel_edges.md, "CPU-measured ratios"
C_BOUND = 64.0
# mvf_pinv_diag with float32 cells, by m: the measured deviation (relative to the largest leverage) of the longdouble
# leverage reference - same A, same eigenpairs - with U evaluated from float32-rounded coordinates against float64 ones on
# pinv_case(257, m); it grows with kappa_kept (a U that is not the one A was formed from leaves e^T pinv(A) e).  The GPU
# bound is 4 x this (profiles/solve_kernel_edges.md, "mvf_pinv_diag"; tests/test_solve_kernel_refs.py re-measures it)
FLOAT32_PINV_FLOOR = {1: 1.9e-8, 127: 2.3e-6, 128: 3.3e-6, 129: 4.1e-6, 257: 1.02e-4}
MARGIN_MIN = 2.0 ** -20     # smallest relative gap between a greedy pivot and the runner-up in every pivot-order case
SHIFT = 1e-8                # mvf_solve_minnorm's shift on the semi-definite families (delta = SHIFT mean(diag))


def pad(m):
    return -(-m // PAD) * PAD


# ---------------------------------------------------------------------------------------------------- construction
def _unit(v):
    v = np.asarray(v, dtype=LD)
    return v / np.sqrt(v @ v)


def _reflect_sym(A, w):
    """H A H, H = I - 2 w w^T (longdouble, O(m^2))."""
    Aw = A @ w
    return A - 2 * np.outer(w, Aw) - 2 * np.outer(Aw, w) + 4 * (w @ Aw) * np.outer(w, w)


def _reflect_rows(T, w):
    """H T."""
    return T - 2 * np.outer(w, w @ T)


def q_times(refl, T):
    """Q T, Q = H_1 H_2 ... H_k."""
    for w in reversed(refl):
        T = _reflect_rows(T, w)
    return T


def qt_times(refl, T):
    """Q^T T."""
    for w in refl:
        T = _reflect_rows(T, w)
    return T


def q_matrix(refl, m):
    return q_times(refl, np.eye(m, dtype=LD))


def designed_matrix(lam, refl):
    """Q diag(lam) Q^T in longdouble, symmetrised."""
    A = np.diag(np.asarray(lam, dtype=LD))
    for w in reversed(refl):
        A = _reflect_sym(A, w)
    return (A + A.T) / 2


def reflectors(m, seed, ortho_ones=False):
    """Two random unit vectors; ortho_ones: chosen so that Q e_0 (the dominant eigenvector) is orthogonal to the all-ones
    vector, the start of the cold power iteration."""
    rng = np.random.default_rng(seed)
    u, v = _unit(rng.standard_normal(m)), _unit(rng.standard_normal(m))
    if ortho_ones and m >= 3:
        e0 = np.zeros(m, dtype=LD)
        e0[0] = 1
        y = _reflect_rows(e0[:, None], v)[:, 0]
        t = np.asarray(rng.standard_normal(m), dtype=LD)
        t = _unit(t - t.mean())  # unit, orthogonal to ones
        u = _unit(y - t)         # H_u y = t
    return [u, v]


def small_rotation(m, seed, angle=1e-2):
    """Two reflectors of nearly parallel vectors: H_a H_b is a rotation by ~2 angle in one plane (the "nearby" basis)."""
    rng = np.random.default_rng(seed)
    a = _unit(rng.standard_normal(m))
    b = _unit(a + angle * _unit(rng.standard_normal(m)))
    return [a, b]


# ---------------------------------------------------------------------------------------------------- spectra
def spectrum(family, m):
    """(lambda[m] descending in |.|, rcond) of a family, or None where the family does not fit m."""
    def geo(hi, lo, n):
        return np.ones(1) * 10.0 ** hi if n == 1 else np.logspace(hi, lo, n)

    def top(n):
        """kappa = 10^2 with a separated largest eigenvalue (lambda_2 / lambda_1 = 0.32): the power iterations of the
        rank-revealing drivers settle in their fixed number of steps, as they do on kernel Gram matrices (0.45)."""
        return np.ones(1) if n == 1 else np.concatenate([np.ones(1), geo(-2, -2, 1) if n == 2 else geo(-0.5, -2, n - 1)])

    if family == "well":
        lam, rcond = top(m), 1e-12
    elif family == "graded":
        if m < 2:
            return None
        lam, rcond = geo(0, -8, m), 1e-12
    elif family in ("rank1", "rankhalf", "rankm1"):
        r = {"rank1": 1, "rankhalf": m // 2, "rankm1": m - 1}[family]
        if m < 2 or (family == "rankhalf" and r < 2) or (family == "rankm1" and r <= max(1, m // 2)):
            return None  # (the three ranks coincide at m = 2, two of them at m = 3)
        # (one dominant eigenvalue, the others <= 1e-2 of it: the entries of A - and with them the rounding of the matrix,
        # which is what an "exact" null space turns into in float64 - are small against lambda_max, so that what remains on
        # the diagonal after r pivots lies far below the factor's stopping tolerance 0.25 eps lambda_max and the factor has
        # exactly r columns; tests/test_solve_kernel_refs.py asserts that margin)
        lam, rcond = np.concatenate([np.ones(1), geo(-2, -3, r - 1) if r > 1 else np.zeros(0), np.zeros(m - r)]), 1e-12
    elif family == "cluster":  # kept >= 1e-6, dropped <= 1e-9, the cut between them
        if m < 2:
            return None
        k = (m + 1) // 2
        lam, rcond = np.concatenate([geo(0, -6, k), geo(-9, -10, m - k)]), 3e-8
    elif family == "ortho":  # dominant eigenvector orthogonal to ones; second-largest 1e-3, dropped at 1e-9
        if m < 3:
            return None
        k = max(2, m // 2)
        lam, rcond = np.concatenate([np.ones(1), geo(-3, -5, k - 1), np.full(m - k, 1e-9)]), 1e-8
    elif family == "indef":  # two negative eigenvalues at -1e-4 lambda_max
        if m < 3:
            return None
        lam, rcond = np.concatenate([top(m - 2), [-1e-4, -1e-4]]), 1e-12
    else:
        raise ValueError(family)
    return LAMBDA_MAX * lam, rcond


FAMILIES = ["well", "graded", "rank1", "rankhalf", "rankm1", "cluster", "ortho", "indef"]
# Exact-rank cases whose first seed leaves a remaining diagonal entry above EXACT_RANK_RESIDUAL_MAX x the stopping tolerance
# after the designed rank - in longdouble or in a plain float64 factorisation (which cannot resolve the Schur complement
# below eps x its entries): the first seed offset that does not (tests/test_solve_kernel_refs.py asserts the condition)
EXACT_RANK_SEED_OFFSET = {("rankhalf", 65): 1, ("rankhalf", 128): 1, ("rankhalf", 512): 1, ("rankhalf", 513): 1}
_CACHE = {}


def make_case(family, m, lam=None, rcond=None, refl=None, seed=None, tag=""):
    """One system.  Keys: A_ld (designed, longdouble), G, K, ls2 (float64 operands), A (float64: G + ls2 K exactly as the
    device assembles it), R (m x 8; tests take leading columns), lam, keep, rcond, kappa, refl, rank."""
    key = (family, m, tag)
    if lam is None and key in _CACHE:
        return _CACHE[key]
    if lam is None:
        sp = spectrum(family, m)
        if sp is None:
            return None
        lam, rcond = sp
    seed = (1000 * FAMILIES.index(family) + m + 100000 * EXACT_RANK_SEED_OFFSET.get((family, m), 0)) if seed is None else seed
    if refl is None:
        # (2 x 2 of exact rank 1: a Q close to the identity keeps the second diagonal entry, and the rounding it carries,
        # small against lambda_max - see the exact-rank spectrum)
        refl = small_rotation(m, seed, 0.05) if (family == "rank1" and m == 2) else reflectors(m, seed, ortho_ones=family == "ortho")
    lam = np.asarray(lam, dtype=LD)
    A_ld = designed_matrix(lam, refl)
    rng = np.random.default_rng(seed + 7)
    B = rng.standard_normal((m, m))
    K = B @ B.T / m + 0.5 * np.eye(m)
    K = (K + K.T) / 2
    # (exact-rank families: a split 100 x smaller, for the same reason as their spectrum - the rounding of G + ls2 K is the
    # "null space" the factor sees, and it scales with ls2 K)
    ls2 = (1e-3 if family.startswith("rank") else 0.1) * LAMBDA_MAX
    G = np.asarray(A_ld - LD(ls2) * K.astype(LD), dtype=np.float64)
    G = (G + G.T) / 2
    A = G + ls2 * K  # float64, one multiply and one add per entry: the device's assembly
    absl = np.abs(lam)
    cut = LD(rcond) * absl.max()
    keep = absl > cut
    # the design keeps clear of the cut: 10 x on either side (9 x after the 1 % perturbation of a "nearby" matrix), about
    # 10^3 between kept and dropped
    clear = 9 if tag else 10
    assert absl[keep].min() >= clear * cut and (not (~keep).any() or absl[~keep].max() * clear <= cut * (1 + 1e-12)), (family, m)
    assert not (~keep).any() or absl[keep].min() * (1 + 1e-12) >= (clear ** 3) * absl[~keep].max(), (family, m)
    c = dict(family=family, m=m, tag=tag, id=f"{family}{tag}-m{m}", lam=lam, rcond=float(rcond), keep=keep, refl=refl,
             A_ld=A_ld, G=G, K=K, ls2=ls2, A=A, R=rng.standard_normal((m, 8)), rank=int(keep.sum()),
             kappa=float(absl.max() / absl[keep].min()), lmax=float(absl.max()), seed=seed)
    if tag == "" and family in FAMILIES:
        _CACHE[key] = c
    return c


def nearby_case(c, seed=5):
    """The matrix of the next EM iteration: lambda perturbed by 1 % (zeros stay zero), Q turned by a small rotation."""
    rng = np.random.default_rng(c["seed"] + seed)
    lam = c["lam"] * np.asarray(1 + 0.01 * rng.uniform(-1, 1, c["m"]), dtype=LD)
    lam[0] = c["lam"][0]  # lambda_max stays the designed one
    refl = small_rotation(c["m"], c["seed"] + seed + 1) + c["refl"]
    return make_case(c["family"], c["m"], lam=lam, rcond=c["rcond"], refl=refl, seed=c["seed"], tag="-near")


def c_star(c, R):
    """Q_keep diag(1 / lambda_keep) Q_keep^T R in longdouble."""
    g = np.zeros(c["m"], dtype=LD)
    g[c["keep"]] = 1 / c["lam"][c["keep"]]
    return q_times(c["refl"], g[:, None] * qt_times(c["refl"], np.asarray(R, dtype=LD)))


def bound(c):
    """Bound on max|C - C*| / max|C*| per column."""
    return C_BOUND * c["m"] * EPS * c["kappa"]


def eig_bound(c):
    """Bound on the absolute error of einfo[2], [3], [5]."""
    return C_BOUND * c["m"] * EPS * c["lmax"]


def col_dev(C, Cs):
    """max over columns of max|C - C*| / max|C*| (longdouble arithmetic, float result)."""
    C, Cs = np.asarray(C, dtype=LD), np.asarray(Cs, dtype=LD)
    d = np.abs(C - Cs).max(0) / np.maximum(np.abs(Cs).max(0), LD(1e-300))
    return float(d.max())


def ratio(C, Cs, c):
    return col_dev(C, Cs) / bound(c)


# ---------------------------------------------------------------------------------------------------- references
def cholesky_ld(A, jitter=0.0):
    """Plain longdouble Cholesky of A + jitter mean(diag) I (row loop).  Returns (L, pivots L_jj^2, bad) with bad = index of
    the first non-positive pivot or -1; behind a bad pivot nothing is computed (L and pivots are cut there)."""
    A = np.asarray(A, dtype=LD)
    m = len(A)
    if jitter:
        A = A + LD(jitter) * (np.trace(A) / m) * np.eye(m, dtype=LD)
    L = np.zeros((m, m), dtype=LD)
    piv = np.zeros(m, dtype=LD)
    for j in range(m):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        piv[j] = d
        if not d > 0:
            return L[:j, :j], piv[: j + 1], j
        L[j, j] = np.sqrt(d)
        if j + 1 < m:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L, piv, -1


def cholesky_solve_ld(A, R, jitter=0.0):
    """(C, [min L_jj^2, max L_jj^2]) of the longdouble Cholesky solve; the matrix must be positive definite."""
    L, piv, bad = cholesky_ld(A, jitter)
    assert bad < 0
    m = len(L)
    Y = np.array(R, dtype=LD)
    for i in range(m):
        Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    for i in range(m - 1, -1, -1):
        Y[i] = (Y[i] - L[i + 1:, i] @ Y[i + 1:]) / L[i, i]
    return Y, np.array([piv.min(), piv.max()], dtype=LD)


def greedy_pivoted_cholesky_ld(A, tol, max_steps=None, dtype=LD):
    """Greedy diagonally pivoted Cholesky in longdouble: largest remaining diagonal entry first (ties: lowest index), stopped
    when it is <= tol - the rule of _greedy_pivoted_cholesky in tests/test_gpu_kernels.py.  Returns (order, pivot values,
    margins): margins[j] = (chosen - runner-up) / chosen of step j (1 when nothing else remains).  dtype = np.float64: the
    same steps in float64, for the rounding a float64 factorisation adds on its own."""
    A = np.asarray(A, dtype=dtype)
    m = len(A)
    d = np.diag(A).copy()
    L = np.zeros((m, m), dtype=dtype)
    alive = np.ones(m, dtype=bool)
    order, piv, margins = [], [], []
    for j in range(m if max_steps is None else min(m, max_steps)):
        dm = np.where(alive, d, -np.inf)
        p = int(np.argmax(dm))
        if not dm[p] > tol:
            break
        dm[p] = -np.inf
        second = dm.max()
        margins.append(1.0 if not np.isfinite(second) else float((d[p] - second) / d[p]))
        col = (A[:, p] - L[:, :j] @ L[p, :j]) / np.sqrt(d[p])
        col[~alive] = 0
        order.append(p)
        piv.append(d[p])
        L[:, j] = col
        d = d - col * col
        alive[p] = False
    return np.asarray(order, dtype=np.int64), np.asarray(piv, dtype=dtype), np.asarray(margins)


def lapack_minnorm(c, nrhs=8):
    """The float64 reference route of the minimum-norm entry points on the rounded matrix: eigh, truncated at rcond max|w|."""
    w, q = np.linalg.eigh((c["A"] + c["A"].T) / 2)
    keep = np.abs(w) > c["rcond"] * np.abs(w).max()
    return (q[:, keep] / w[keep]) @ (q[:, keep].T @ c["R"][:, :nrhs]), w, keep


def lapack_solve(c, jitter=0.0, nrhs=8):
    """The float64 reference route of mvf_solve: scipy's Cholesky solve."""
    import scipy.linalg

    A = c["A"] + jitter * np.trace(c["A"]) / c["m"] * np.eye(c["m"])
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True), c["R"][:, :nrhs])


# ---------------------------------------------------------------------------------------------------- case lists
SOLVE_M_SMALL = [1, 2, 63, 64, 65, 127, 128]
SOLVE_M_BLOCKED = SOLVE_M_SMALL + [129, 191, 192, 193, 257]
SOLVE_FAMILIES = ["well", "graded"]  # positive definite ones
MINNORM_M = [1, 2, 63, 64, 65, 128, 129, 257]
LR_M = [1, 2, 64, 65, 127, 129, 511, 512, 513]
LR_FAMILIES = [f for f in FAMILIES if f != "indef"]  # the rank-revealing factor needs a semi-definite matrix
LR_LARGE_FAMILIES = ["well", "rank1", "rankhalf", "rankm1"]  # m >= 511: to stay within seconds
LRD_M = [127, 128, 129, 511, 512, 513, 640, 641]
PIVOT_M = [65, 512, 513]


def solve_nrhs(m):
    return list(range(1, 9)) if m in (65, 129) else [1, 3, 8]


def solve_cases(ms=SOLVE_M_BLOCKED):
    return [c for m in ms for f in SOLVE_FAMILIES for c in [make_case(f, m)] if c is not None]


def minnorm_cases(ms=MINNORM_M):
    return [c for m in ms for f in FAMILIES for c in [make_case(f, m)] if c is not None]


def lr_cases(ms=LR_M):
    return [c for m in ms for f in (LR_LARGE_FAMILIES if m >= 511 else LR_FAMILIES) for c in [make_case(f, m)]
            if c is not None]


def lrd_cases(ms=LRD_M):
    """Deflated form: the number of directions between the factor's stopping tolerance and the cut must fit the block, so
    the well-conditioned and exact-rank families (nothing, or rounding-level columns only, below the cut)."""
    return [c for m in ms for f in ["well", "rankhalf", "rankm1"] for c in [make_case(f, m)] if c is not None]


def all_cases():
    seen, out = set(), []
    for c in solve_cases() + minnorm_cases() + lr_cases() + lrd_cases():
        if c["id"] not in seen:
            seen.add(c["id"])
            out.append(c)
    return out


def indefinite_for_solve(m, bad):
    """A matrix whose Cholesky factorisation meets its first non-positive pivot at index `bad`: the well-conditioned case
    with A[bad][bad] lowered by twice the pivot the longdouble factorisation finds there (pivots before it are untouched).
    Returns (G, K, ls2, A)."""
    c = make_case("well", m)
    _, piv, none = cholesky_ld(c["A"])
    assert none < 0
    G = c["G"].copy()
    G[bad, bad] -= 2.0 * float(piv[bad])
    A = G + c["ls2"] * c["K"]
    _, piv2, first = cholesky_ld(A)
    assert first == bad and piv2[bad] < -0.5 * piv[bad]  # clearly negative, not a rounding-level sign
    return G, c["K"], c["ls2"], A


def minnorm_shift(c):
    """The shift of mvf_solve_minnorm for a case: SHIFT on semi-definite matrices, delta = 10 |lambda_min| on the indefinite
    one."""
    if c["family"] != "indef":
        return SHIFT
    s = 10 * 1e-4 * c["lmax"] / (np.trace(c["A"]) / c["m"])
    assert 0 < s < 1
    return float(s)


EXACT_RANK_RESIDUAL_MAX = 1.0 / 8  # largest remaining diagonal entry after the designed rank, in units of the stopping tolerance


def exact_rank_cases():
    seen, out = set(), []
    for c in lr_cases() + lrd_cases():
        if c["family"].startswith("rank") and c["id"] not in seen:
            seen.add(c["id"])
            out.append(c)
    return out


def pivot_case(m):
    """Graded full-rank matrix for the pivot-order comparison: the seed is the first whose longdouble greedy margin is
    >= MARGIN_MIN at every step (asserted in tests/test_solve_kernel_refs.py)."""
    key = ("pivot", m)
    if key not in _CACHE:
        # graded over six decades below a separated largest eigenvalue (lambda_2 / lambda_1 = 0.1): the factor's stopping
        # tolerance comes from 8 power steps started at 1 / sqrt(m), which then settle lambda_max to 1e-7
        lam = LAMBDA_MAX * np.concatenate([np.ones(1), np.logspace(-1, -6, m - 1)])
        _CACHE[key] = make_case("graded", m, lam=lam, rcond=1e-12, seed=PIVOT_SEEDS[m], tag="-pivot")
    return _CACHE[key]


PIVOT_SEEDS = {65: 0, 512: 0, 513: 0}


# ---------------------------------------------------------------------------------------------------- leverage cases
def power_estimate(A, steps=8):
    """lambda_max as the rank-revealing drivers estimate it for the stopping tolerance: `steps` power steps from 1 / sqrt(m),
    the last Rayleigh quotient, and at least the largest diagonal entry."""
    x = np.full(len(A), 1.0 / np.sqrt(len(A)))
    est = 0.0
    for _ in range(steps):
        y = A @ x
        est = float(x @ y)
        x = y / np.sqrt(y @ y)
    return max(est, float(np.diag(A).max()))


def pinv_case(n, m, seed=None):
    """Point cloud of the mvf_pinv_diag cases: n cells in [-30, 30]^3, m control points among / beside them."""
    rng = np.random.default_rng(7000 + m if seed is None else seed)
    ctrl = rng.uniform(-1, 1, (m, 3)) * 30.0
    X = rng.uniform(-1, 1, (n, 3)) * 30.0
    k = min(n, m)
    X[:k] = ctrl[:k]  # some cells sit on control points (kernel value exactly 1)
    return dict(n=n, m=m, X=X, ctrl=ctrl, beta=0.004, rcond=1e-10, center=ctrl.mean(0))


def leverage_reference(pc, dtype):
    """A = U^T U from the float64 coordinates (one float64 eigh, cut at rcond), and the longdouble leverage
    sum over the kept eigenpairs of (U_d q)^2 / lambda with U_d evaluated in float64 at the coordinates rounded to `dtype`.
    Keys: A, X, ctrl (centred, in dtype), ref, rank, kappa."""
    from oracle import sparsevfc_oracle as svo

    X64, c64 = pc["X"] - pc["center"], pc["ctrl"] - pc["center"]
    U = svo.con_K(X64, c64, pc["beta"]).reshape(len(X64), len(c64))
    A = U.T @ U
    A = (A + A.T) / 2
    w, q = np.linalg.eigh(A)
    keep = w > pc["rcond"] * w.max()
    X, ctrl = X64.astype(dtype), c64.astype(dtype)
    Ud = svo.con_K(X.astype(np.float64), ctrl.astype(np.float64), pc["beta"]).reshape(len(X), len(ctrl))
    Z = Ud.astype(LD) @ q[:, keep].astype(LD)
    return dict(pc=pc, A=A, U=Ud, X=X, ctrl=ctrl, ref=(Z * Z / w[keep].astype(LD)).sum(1), rank=int(keep.sum()),
                kappa=float(w.max() / w[keep].min()))
