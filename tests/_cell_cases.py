"""Shared by tests/test_gpu_cell_kernels.py (the HIP kernels on the device) and tests/test_cell_kernel_refs.py (no GPU): the
seeded inputs of the evaluator / RK4 / E-step / quadform / lincomb3 / sym_pack edge cases, the shape lists, the tolerances and
the high-precision references.  The CPU module proves on exactly these inputs that the float64 restatements of
tests/_cpu_kernels.py are accurate, that the quantities are well conditioned (so a plain max-norm relative error over ALL
queries means something) and that each targeted off-by-one would be a gross error; the GPU module then compares the kernels
with the restatements.

Input design (beta = 0.004, control points in a +-30 cloud as ``_cloud`` of test_gpu_kernels.py draws them):
  * coefficients are strictly positive (0.5 .. 1.5 x COEF), so that no sum over control points cancels;
  * the LAST control point, and the last point of the first staging chunk where the list is longer than one chunk (index 255
    for the evaluator's 256-point chunks, index cap - 1 for mvf_integrate's LDS cap), carry coefficients of BIG = 50 x COEF and
    sit 3 units on either side of ANCHOR; the first and the last query / start point sit within 1.5 .. 4 units of ANCHOR, so a
    dropped tail row, a dropped chunk-end row or a last lane that repeats its neighbour is a gross error even at n = 1;
  * every other query is drawn 1.5 .. 14 units from ANCHOR: inside the cloud, where the two big points are felt with a kernel
    value of at least 0.3, so that |v| and |a| = |J v| (which goes with the SQUARE of the coefficients) stay within a factor
    of 30 / 200 over the queries while the ordinary control points still contribute their share;
  * lists of fewer than 16 control points are drawn within +-6 of ANCHOR and their queries 0.5 .. 8 units beyond that box
    along every axis: each (x - c) is positive in every component, so with one control point a = J v cannot vanish on the
    plane (x - c) . C = 0.
"""
import math

import numpy as np

EVAL_V, EVAL_JAC, EVAL_DIV, EVAL_CURL, EVAL_ACC, EVAL_CURV, EVAL_TORS, EVAL_JDET = 1, 2, 4, 8, 16, 32, 64, 128
EVAL_FLAGS = (EVAL_V, EVAL_JAC, EVAL_DIV, EVAL_CURL, EVAL_ACC, EVAL_CURV, EVAL_TORS, EVAL_JDET)
EVAL_ALL = 255
EVAL_NAMES = {EVAL_V: "v", EVAL_JAC: "jac", EVAL_DIV: "div", EVAL_CURL: "curl", EVAL_ACC: "acc", EVAL_CURV: "curv",
              EVAL_TORS: "tors", EVAL_JDET: "jdet"}
EVAL_SHAPES = {EVAL_V: lambda n: (n, 3), EVAL_JAC: lambda n: (3, 3, n), EVAL_DIV: lambda n: (n,), EVAL_CURL: lambda n: (n, 3),
               EVAL_ACC: lambda n: (n, 3), EVAL_CURV: lambda n: (n, 3), EVAL_TORS: lambda n: (n, 3), EVAL_JDET: lambda n: (n,)}

BETA = 0.004
COEF = 0.02
BIG = 50.0
ANCHOR = np.array([5.0, -4.0, 3.0])

# relative to each quantity's maximum (the existing evaluator tests' tolerances); torsion 10 x (test_evaluators_golden)
TOL = {"float64": 1e-10, "float32": 2e-4}
MUTATION_FACTOR = 1000.0  # a targeted off-by-one must move a compared quantity by this many float32 tolerances


def eval_tol(dtype, flag):
    return TOL[dtype] * (10.0 if flag == EVAL_TORS else 1.0)


def relmax(got, ref):
    """max |got - ref| over ALL entries, relative to max |ref|."""
    got, ref = np.asarray(got), np.asarray(ref)
    if ref.size == 0:
        return 0.0
    return float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), 1e-300))


def eval_errors(got, ref):
    """flag -> max |got - ref| over ALL queries relative to the quantity's maximum.  det J is a cubic form in J whose rounding
    error scales with max |J|^3 whatever its own size (with one or two control points J has rank <= 2 and det J is 0 but for
    rounding), so its error is taken relative to max |J|^3, as test_jacobian_determinant_on_the_device_and_one_fused_pass does."""
    out = {}
    for f in ref:
        if f == EVAL_JDET:
            out[f] = float(np.abs(np.asarray(got[f]) - ref[f]).max() / float(np.abs(ref[EVAL_JAC]).max()) ** 3)
        else:
            out[f] = relmax(got[f], ref[f])
    return out


# ------------------------------------------------------------------------------------------------------ evaluator
EVAL_NS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000)   # 16-query tile, 64-query wave, 256-query workgroup edges
EVAL_MS = (1, 2, 3, 4, 5, 255, 256, 257, 259, 513, 1023)     # k-step of 4, 256-point chunk: m % 4 = 1, 2, 3 and 256 +- 1
EVAL_SWEEP = sorted(set([(n, m) for n in EVAL_NS for m in (259, 1023)] + [(n, m) for m in EVAL_MS for n in (17, 257)]))
EVAL_AFFINE_SHAPES = [(65, 5), (257, 259), (1000, 513)]
# one control point without the affine part: a = J v is parallel to v, the curvature (a (v.v) - v (v.a)) / |v|^4 is 0 but for
# rounding and cannot be compared relative to its own size; with 2 .. 5 points the big one dominates and it nearly is.  Those
# shapes run with the constant b (not parallel to the big coefficients)
EVAL_CASES = ([("affine" if m < 16 else "positive", n, m) for n, m in EVAL_SWEEP]
              + [("affine", n, m) for n, m in EVAL_AFFINE_SHAPES])
EVAL_CHUNK = 256  # EM_CHUNK of csrc/mvf_eval.hip


def _unit(rng, k):
    d = rng.standard_normal((k, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _points(rng, n, m, chunk_end, coef=COEF, signed=False):
    """Control points, their coefficients and n queries / start points as the module docstring describes them.  chunk_end:
    indices (besides m - 1) that carry the big coefficients when they exist below m - 1."""
    if m < 16:
        ctrl = ANCHOR + rng.uniform(-6.0, 6.0, (m, 3))
    else:
        ctrl = rng.uniform(-30.0, 30.0, (m, 3))
    C = (rng.standard_normal((m, 3)) if signed else rng.uniform(0.5, 1.5, (m, 3))) * coef
    if m:
        ctrl[m - 1] = ANCHOR + np.array([3.0, 0.0, 0.0])
        C[m - 1] = BIG * coef * np.array([1.0, 0.6, 0.8])
    places = [np.array([-3.0, 0.0, 0.0]), np.array([0.0, 3.0, 0.0]), np.array([0.0, 0.0, -3.0])]
    dirs = [np.array([0.7, 1.0, 0.5]), np.array([0.5, 0.8, 1.0]), np.array([0.9, 0.5, 0.7])]
    for t, j in enumerate(chunk_end):
        if j < m - 1:
            ctrl[j] = ANCHOR + places[t]
            C[j] = BIG * coef * dirs[t]
    if m < 16:
        X = ANCHOR + 6.0 + rng.uniform(0.5, 8.0, (n, 3))
    else:
        X = ANCHOR + _unit(rng, n) * rng.uniform(1.5, 14.0, (n, 1))
    near = ANCHOR + _unit(rng, 2) * rng.uniform(1.5, 4.0, (2, 1))
    if n and m >= 16:
        X[0] = near[0]
        X[n - 1] = near[1]
    return X, ctrl, C


def eval_case(n, m, family="positive"):
    """family "positive": no affine epilogue; "affine": a full A (entries ~1e-2), a constant b of the field's magnitude, a
    per-axis alpha and jmul != 1."""
    rng = np.random.default_rng(1000 * n + m + (7 if family == "affine" else 0))
    X, ctrl, C = _points(rng, n, m, (EVAL_CHUNK - 1,))
    affine = None
    if family == "affine":
        A = 1e-2 * rng.standard_normal((3, 3))
        b = BIG * COEF * np.array([1.0, 0.8, 1.2])
        affine = (np.array([0.9, 1.3, 1.1]), 1.7, A, b)
    return {"X": X, "ctrl": ctrl, "C": C, "beta": BETA, "affine": affine}


def eval_case_empty(n, family="positive"):
    """No control points.  Queries, A and b are small dyadic rationals (k / 8, k / 1024, k / 16): every product and every
    partial sum of alpha * 0 + A q + b is exact in float32 and float64, so the expected v does not depend on the order or
    on the contraction into fused multiply-adds the compiler chose for the epilogue."""
    rng = np.random.default_rng(n + (7 if family == "affine" else 0))
    X = rng.integers(-240, 241, (n, 3)) / 8.0
    affine = None
    if family == "affine":
        affine = (np.array([0.9, 1.3, 1.1]), 1.7, rng.integers(-32, 33, (3, 3)) / 1024.0, rng.integers(-64, 65, 3) / 16.0)
    return {"X": X, "ctrl": np.zeros((0, 3)), "C": np.zeros((0, 3)), "beta": BETA, "affine": affine}


def eval_mutations(case):
    """name -> mutated INPUTS (the off-by-one each shape exists to catch); "dup_last_query" acts on the outputs instead."""
    m = len(case["ctrl"])
    out = {}
    if m:
        out["drop_last_ctrl"] = dict(case, ctrl=case["ctrl"][:-1], C=case["C"][:-1])
    if m > EVAL_CHUNK:
        keep = np.arange(m) != EVAL_CHUNK - 1
        out["drop_chunk_end"] = dict(case, ctrl=case["ctrl"][keep], C=case["C"][keep])
    return out


def dup_last_query(outs):
    """What a last lane that repeats its neighbour's result would return."""
    res = {}
    for f, a in outs.items():
        a = np.array(a, copy=True)
        if f == EVAL_JAC:
            a[:, :, -1] = a[:, :, -2]
        else:
            a[-1] = a[-2]
        res[f] = a
    return res


def eval_reference(xp, X, ctrl, C, beta, affine=None, flags=EVAL_ALL):
    """All evaluator outputs pair by pair in the floating-point type `xp` (np.float64 or np.longdouble)."""
    X, ctrl, C = np.asarray(X, dtype=xp), np.asarray(ctrl, dtype=xp).reshape(-1, 3), np.asarray(C, dtype=xp).reshape(-1, 3)
    beta = xp(beta)
    n = len(X)
    D = X[:, None, :] - ctrl[None, :, :]                      # (n, m, 3)
    K = np.exp(-beta * np.sum(D * D, axis=2))                 # (n, m)
    v = K @ C
    J = -2 * beta * np.einsum("nm,mf,nmi->fin", K, C, D)      # J[f][i][n]
    if affine is not None:
        alpha, jmul, A, b = affine
        alpha = np.broadcast_to(np.asarray(alpha, dtype=xp).reshape(-1), (3,))
        v = alpha[None, :] * v + X @ np.asarray(A, dtype=xp).T + np.asarray(b, dtype=xp)[None, :]
        J = xp(jmul) * J
    a = np.einsum("fin,ni->nf", J, v)
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        if flags & EVAL_V:
            out[EVAL_V] = v
        if flags & EVAL_JAC:
            out[EVAL_JAC] = J
        if flags & EVAL_DIV:
            out[EVAL_DIV] = J[0, 0] + J[1, 1] + J[2, 2]
        if flags & EVAL_CURL:
            out[EVAL_CURL] = np.stack([J[2, 1] - J[1, 2], J[0, 2] - J[2, 0], J[1, 0] - J[0, 1]], axis=1)
        if flags & EVAL_ACC:
            out[EVAL_ACC] = a
        if flags & EVAL_CURV:
            vv, va = np.sum(v * v, 1), np.sum(v * a, 1)
            out[EVAL_CURV] = (a * vv[:, None] - v * va[:, None]) / (vv * vv)[:, None]
        if flags & EVAL_TORS:
            Ja = np.einsum("fin,ni->nf", J, a)
            out[EVAL_TORS] = v * (np.sum(a * Ja, 1) / (np.sum(v * v, 1) * np.sum(a * a, 1)))[:, None]
        if flags & EVAL_JDET:
            out[EVAL_JDET] = (J[0, 0] * (J[1, 1] * J[2, 2] - J[1, 2] * J[2, 1]) - J[0, 1] * (J[1, 0] * J[2, 2] - J[1, 2] * J[2, 0])
                              + J[0, 2] * (J[1, 0] * J[2, 1] - J[1, 1] * J[2, 0]))
    assert all(o.shape == EVAL_SHAPES[f](n) for f, o in out.items())
    return out


# ------------------------------------------------------------------------------------------------------ RK4
# mvf_integrate stages at most cap = 144 KiB / (sizeof(vec4<T>) + 32 B) control points at once: 3072 (float32) / 2304 (float64)
RK4_CAP = {"float32": (144 * 1024) // (16 + 32), "float64": (144 * 1024) // (32 + 32)}
RK4_MS = (15, 2303, 2304, 2305, 3071, 3072, 3073, 4613, 6200)
RK4_NS = (1, 255, 257, 600)
RK4_SHAPES = [(600, m) for m in RK4_MS] + [(n, m) for n in (1, 255, 257) for m in (2305, 15)]
RK4_AFFINE_SHAPE = (257, 2305)
RK4_DT, RK4_SUBSTEPS, RK4_NOUT = 2.0, 2, 6
# ordinary coefficients are N(0, RK4_COEF^2): with thousands of control points a positive background would carry every start
# point across the cloud, a signed one adds up to ~sqrt(0.1 m) RK4_COEF and the big points (50 x) stay the gross term
RK4_COEF = 0.01
RK4_STEPPING = [(1, 2), (4, 2), (1, 6), (4, 6), (2, 1), (4, 1)]   # (substeps, n_out) besides the default (2, 6)


def rk4_chunks(m, dtype):
    return -(-m // RK4_CAP[dtype])


def rk4_case(n, m, affine=False):
    """Start points, control points and coefficients on the float32 grid (both cell dtypes then integrate the SAME field
    from the same points, and one float64 reference serves both; the state leaves that grid with the first step)."""
    rng = np.random.default_rng(77 * n + m + (3 if affine else 0))
    X, ctrl, C = _points(rng, n, m, tuple(c - 1 for c in sorted(RK4_CAP.values())), coef=RK4_COEF, signed=True)
    X, ctrl = X.astype(np.float32).astype(np.float64), ctrl.astype(np.float32).astype(np.float64)
    aff = None
    if affine:  # GP style: one alpha, a small linear part and a constant drift
        aff = (0.8, 1.0, 2e-3 * rng.standard_normal((3, 3)), np.array([0.05, -0.08, 0.04]))
    return {"X": X, "ctrl": ctrl, "C": C, "beta": BETA, "affine": aff}


def rk4_mutations(case):
    m = len(case["ctrl"])
    out = {"drop_last_ctrl": dict(case, ctrl=case["ctrl"][:-1], C=case["C"][:-1])}
    for dtype, cap in RK4_CAP.items():
        if m > cap:
            keep = np.arange(m) != cap - 1
            out[f"drop_chunk_end_{dtype}"] = dict(case, ctrl=case["ctrl"][keep], C=case["C"][keep])
    return out


def rk4_reference(xp, X, ctrl, C, beta, dt, substeps, n_out, affine=None):
    """Classical RK4, the device kernel's scheme and step count, in the floating-point type `xp`."""
    X, ctrl, C = np.asarray(X, dtype=xp), np.asarray(ctrl, dtype=xp).reshape(-1, 3), np.asarray(C, dtype=xp).reshape(-1, 3)
    beta = xp(beta)
    if affine is not None:
        alpha, _, A, b = affine
        alpha = np.broadcast_to(np.asarray(alpha, dtype=xp).reshape(-1), (3,))
        A, b = np.asarray(A, dtype=xp), np.asarray(b, dtype=xp)

    def f(q):
        D = q[:, None, :] - ctrl[None, :, :]
        v = np.exp(-beta * np.sum(D * D, axis=2)) @ C
        return v if affine is None else alpha[None, :] * v + q @ A.T + b[None, :]

    traj = np.empty((len(X), n_out, 3), dtype=xp)
    x = X.copy()
    traj[:, 0] = x
    h = xp(dt) / xp(substeps)
    for t in range(1, n_out):
        for _ in range(substeps):
            k1 = f(x); k2 = f(x + h / 2 * k1); k3 = f(x + h / 2 * k2); k4 = f(x + h * k3)
            x = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        traj[:, t] = x
    return traj


def extent(traj):
    """max |x(t) - x(0)|: the scale the trajectory errors are relative to."""
    return float(np.abs(traj - traj[:, :1]).max())


# ------------------------------------------------------------------------------------------------------ E-step
ESTEP_NS = (1, 255, 256, 257, 1023, 1025, 5000, 2048 * 1024 + 257)   # the last: some lanes take two cells (grid-stride loop)
ESTEP_DYS = (1, 2, 3, 5, 8)
ESTEP_GAMMAS = (1e-6, 0.5, 1 - 1e-6)
ESTEP_SIGMA2, ESTEP_A, ESTEP_MINP = 0.05, 5.0, 1e-5
ESTEP_SUM_RTOL = 1e-12   # >= 0 summands, <= ceil(n / (nb 256)) per lane + log2(256) + log2(2048) tree levels: ~30 x 2^-53
ESTEP_MAX_BLOCKS = 2048


# (n, kind, dy, gamma): every n at dy = 3, gamma = 0.5; dy x gamma at n = 1025; the underflow families at three sizes
ESTEP_CASES = ([(n, "mixed", 3, 0.5) for n in ESTEP_NS] + [(1025, "mixed", dy, g) for dy in ESTEP_DYS for g in ESTEP_GAMMAS]
               + [(n, kind, 3, 0.5) for kind in ("all", "none", "one") for n in (257, 5000)]
               + [(ESTEP_NS[-1], "all", 5, 0.5)])
ESTEP_CASES = list(dict.fromkeys(ESTEP_CASES))


def estep_blocks(n):
    return min(ESTEP_MAX_BLOCKS, max(1, -(-n // 1024)))


def estep_residuals(n, kind, dtype):
    """r as the device holds it (float64 values of the cell dtype's numbers).  kind: "mixed" = inliers, a spread of moderate
    residuals and 1 % cells whose t1 underflows (r / 2 sigma2 = 900 .. 1000; everything else stays below ~30, far from the
    subnormal range 708 .. 745 where exp's last bits decide whether t1 is 0, and the smallest non-zero t1 is large enough
    against t2 that a fill left at 0 changes P and the sums grossly); "none" = no underflow; "all" = every cell
    underflows (r / 2 sigma2 > 800); "one" = every cell but one underflows."""
    rng = np.random.default_rng(n % 100003 + {"mixed": 0, "none": 1, "all": 2, "one": 3}[kind])
    s2 = 2 * ESTEP_SIGMA2
    if kind in ("mixed", "none"):
        r = s2 * np.where(rng.uniform(size=n) < 0.7, rng.chisquare(3, n) * 0.5, rng.uniform(0.0, 12.0, n))
        if kind == "mixed":
            far = rng.uniform(size=n) < 0.01
            if n >= 2:
                far[n - 1] = True   # the last cell takes the fill
                far[0] = False
            r[far] = s2 * rng.uniform(900.0, 1000.0, int(far.sum()))
    else:
        r = s2 * rng.uniform(810.0, 1000.0, n)
        if kind == "one":
            r[n // 2] = s2 * 3.25
    npdt = np.float32 if dtype == "float32" else np.float64
    return r.astype(npdt).astype(np.float64)


def estep_reference(r, sigma2, gamma, a, dy, minP, dtype, zero_fill=None):
    """The restatement (CpuKernels.estep_min / estep_p: same formulas) on the device's residuals, with P as the device stores
    it (rounded to the cell dtype) and the five sums taken with math.fsum.  zero_fill None = the min-non-zero rule."""
    r = np.asarray(r, dtype=np.float64)
    t1 = np.exp(-r / (2 * sigma2))
    zero = t1 == 0
    nz = t1[~zero]
    mins = (float(nz.min()) if len(nz) else np.inf, float(zero.sum()))
    fill = zero_fill if zero_fill is not None else (mins[0] if np.isfinite(mins[0]) else 0.0)
    t1 = np.where(zero, fill, t1)
    t2 = (2 * np.pi * sigma2) ** (dy / 2) * (1 - gamma) / (gamma * a)
    p = t1 / (t1 + t2)
    pf = np.maximum(p, minP)
    stored = pf.astype(np.float32).astype(np.float64) if dtype == "float32" else pf
    return {"mins": mins, "p": p, "pf": pf, "stored": stored, "t2": t2,
            "sums": (math.fsum(p * r), math.fsum(p), math.fsum(stored)), "nzero": float(zero.sum())}


def pick_theta(stored, lo=0.6, hi=0.9):
    """A threshold inside [lo, hi] in the middle of the widest gap between the stored posteriors there, so that the count
    of P > theta does not hang on a last bit; returns (theta, distance to the nearest P)."""
    s = np.sort(stored[(stored > lo) & (stored < hi)])
    edges = np.concatenate([[lo], s, [hi]])
    g = int(np.argmax(np.diff(edges)))
    theta = 0.5 * (edges[g] + edges[g + 1])
    return float(theta), float(np.abs(stored - theta).min())


def blocked_sum(x):
    """float64 sum of x in the order of estep_p_kernel + sum_partials_kernel: a lane adds its grid-stride cells in sequence,
    256 lanes of a workgroup are combined by a binary tree, a lane of the final workgroup adds every 256th partial in
    sequence and a second tree finishes."""
    x = np.asarray(x, dtype=np.float64)
    nb = estep_blocks(len(x))
    stride = nb * 256
    k = -(-len(x) // stride)
    buf = np.zeros(k * stride)
    buf[: len(x)] = x
    lanes = np.zeros(stride)
    for row in buf.reshape(k, stride):
        lanes = lanes + row

    def tree(a):  # over the last axis (256)
        while a.shape[-1] > 1:
            h = a.shape[-1] // 2
            a = a[..., :h] + a[..., h:]
        return a[..., 0]

    part = tree(lanes.reshape(nb, 256))
    fin = np.zeros(256)
    pad = np.zeros(-(-nb // 256) * 256)
    pad[:nb] = part
    for row in pad.reshape(-1, 256):
        fin = fin + row
    return float(tree(fin))


# ------------------------------------------------------------------------------------------------------ small kernels
QUADFORM_MS = (1, 255, 256, 257, 1000, 3000)
QUADFORM_NRHS = (1, 3, 6, 8, 16)
QUADFORM_SHAPES = [(m, 3) for m in QUADFORM_MS] + [(257, k) for k in QUADFORM_NRHS] + [(3000, 16), (1, 1)]
LINCOMB_NS = (1, 255, 256, 257, 100003)
SYM_MS = (1, 2, 255, 256, 257, 3000)


def quadform_case(m, nrhs):
    """A Gaussian Gram matrix (every entry positive) and positive coefficients: the sum is well conditioned."""
    rng = np.random.default_rng(31 * m + nrhs)
    p = rng.uniform(-30.0, 30.0, (m, 3))
    d2 = np.zeros((m, m))
    for i in range(3):
        d2 += (p[:, None, i] - p[None, :, i]) ** 2
    return np.exp(-BETA * d2), rng.uniform(0.5, 1.5, (m, nrhs))


def quadform_reference(K, C):
    Kl, Cl = K.astype(np.longdouble), C.astype(np.longdouble)
    return float(np.sum(Cl * (Kl @ Cl)))


def lincomb3_case(n):
    """a A in [1/16, 0.08), b B in [1/4, 0.3), c C in [1, 1.25): every partial and final sum of any subset of the terms
    stays inside one binade, and the kernel's roundings (a A, then one fma per further term) are bounded by 1/2 ulp of a
    term at most 1/4 (B present) or 1/16 (B absent) of the result plus 1/2 ulp of the result: under 1.4 ulp from the
    exact value, hence at most 1 ulp from its correctly rounded float64."""
    rng = np.random.default_rng(n)
    return (0.0625, rng.uniform(1.0, 1.28, n)), (0.25, rng.uniform(1.0, 1.2, n)), (1.0, rng.uniform(1.0, 1.25, n))


def lincomb3_reference(a, A, b=0.0, B=None, c=0.0, C=None):
    L = np.longdouble
    v = L(a) * A.astype(L)
    if B is not None:
        v = v + L(b) * B.astype(L)
    if C is not None:
        v = v + L(c) * C.astype(L)
    return v.astype(np.float64)


def sym_case(m):
    """A full matrix with garbage in the strict lower triangle: sym_pack must read the upper triangle only."""
    rng = np.random.default_rng(m)
    G = rng.standard_normal((m, m))
    G[np.tril_indices(m, -1)] = 1e300
    return G


def sym_completion(tri, m):
    g = np.zeros((m, m))
    g[np.triu_indices(m)] = tri
    return g + np.triu(g, 1).T
