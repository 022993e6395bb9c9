"""Shared by tests/test_gpu_highd_kernels.py (``ublk_build_d_kernel`` / ``eval_d_kernel`` of csrc/mvf_highd.hip and
``mvf_con_k`` at d = 4 .. 8 on the device) and tests/test_highd_kernel_refs.py (no GPU): the seeded inputs, the shape
lists, the tolerances and the high-precision references.  The CPU module proves on exactly these inputs that the float64
call of ``eval_d_reference`` (the restatement the GPU module compares with) is accurate, that the compared quantities are
well conditioned over ALL queries and that each targeted off-by-one would be a gross error.

Input design: the 3-D design of tests/_cell_cases.py lifted to d columns (beta = 0.004):
  * control points uniform in +-30 sqrt(3 / d) per axis, so that a typical squared distance - and with it a typical kernel
    value - stays what it is in 3-D; coefficients strictly positive (0.5 .. 1.5 x COEF): no sum over control points cancels;
  * the LAST control point, and the last point of the first 64-point staging chunk (index 63) where m > 64, carry
    coefficients of BIG = 50 x COEF along two non-parallel direction vectors and sit 3 units from ANCHOR along two
    different axes (lists of 16 .. 64 points carry the second one at index 0: with ONE dominant point a = J v vanishes on
    the plane (x - c) . v = 0, with two along non-parallel directions only where both terms do); the first and the last
    query sit within 1.5 .. 4 units of ANCHOR, the last but one 12 .. 14 units (a last lane that repeats its neighbour is
    a gross error in v alone), every other one 1.5 .. 14 units;
  * lists of fewer than 16 control points are drawn within +-6 sqrt(3 / d) of ANCHOR and their queries beyond that box on
    the positive side of every axis: every (x - c) is positive in every component; the last query sits at the near end of
    that range and the last but one at the far end.
"""
import numpy as np

from _cell_cases import BETA, BIG, COEF, MUTATION_FACTOR, TOL, relmax  # noqa: F401  (the 3-D suite's values)

EVAL_V, EVAL_JAC, EVAL_DIV, EVAL_CURL, EVAL_ACC, EVAL_CURV, EVAL_TORS, EVAL_JDET = 1, 2, 4, 8, 16, 32, 64, 128
HD_FLAGS = (EVAL_V, EVAL_JAC, EVAL_DIV, EVAL_ACC, EVAL_CURV)   # what mvf_eval_d defines, in the order of its arguments
HD_ALL = EVAL_V | EVAL_JAC | EVAL_DIV | EVAL_ACC | EVAL_CURV
HD_NAMES = {EVAL_V: "v", EVAL_JAC: "jac", EVAL_DIV: "div", EVAL_ACC: "acc", EVAL_CURV: "curv"}
ANCHOR = np.array([5.0, -4.0, 3.0, -2.0, 4.0, -3.0, 2.0, -5.0])
DIR_LAST = np.array([1.0, 0.6, 0.8, 0.9, 0.5, 0.7, 1.0, 0.6])    # the big coefficients' directions over the dy columns
DIR_CHUNK = np.array([0.7, 1.0, 0.5, 0.6, 0.9, 1.0, 0.5, 0.8])
HD_CHUNK = 64        # ED_CHUNK of csrc/mvf_highd.hip
FEW = 5              # up to here one control point dominates: curvature is compared on the scale of `curv_scale`
CONK_TOL = {"float64": 1e-11, "float32": 2e-5}   # DTYPES of test_gpu_kernels.py::test_con_k_vs_oracle (absolute: K <= 1)

HD_NS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)   # 16-query tiles; QB = 64 / 128 / 256 edges
# the k-step of 4 and the 64-point chunk: m % 4 = 1, 2, 3 inside one chunk and (65, 66, 67) in the tail of a second one
HD_MS = (1, 2, 3, 4, 5, 63, 64, 65, 66, 67, 129, 259)
HD_SWEEP = sorted(set([(n, m) for n in HD_NS for m in (67, 259)] + [(n, m) for m in HD_MS for n in (17, 257)]))
# (d, dy, flags): NCT 2 / QB 128, NCT 4 / QB 64, NCT 5 / QB 64, NCT 1 / QB 256
HD_SWEEP_DIMS = ((4, 4, HD_ALL), (7, 7, HD_ALL), (8, 8, HD_ALL), (5, 8, EVAL_V))
HD_GRID_SHAPE = (257, 67)
HD_GRID = [(d, dy) for d in range(4, 9) for dy in range(1, 9)]
HD_FLAG_DIMS = (4, 7, 8)           # d = dy of the flag-subset cases at (257, 259)
HD_PREFIXES = (1, 17, 65, 129)
HD_GUARD_DIMS = ((4, 4), (7, 3), (8, 8), (6, 8))
HD_GUARD_NS = (257, 1000)

CONK_DS = (4, 5, 6, 7, 8)
CONK_SHAPES = ((1, 7), (33, 1), (257, 129), (130, 1030))
UBLK_SHAPES = ([(n, 129) for n in (1, 63, 64, 65, 255, 256, 257, 1000)]
               + [(257, m) for m in (1, 15, 16, 17, 127, 128, 129, 511, 512, 513, 1025)])
UBLK_BETA = 0.004
# how far the queries of the cache's underflow case are moved out of the cloud (whose radius is up to ~50 units): the kernel
# value is denormal for beta r^2 = 87.3 .. 103.3 (float32) / 708.4 .. 744.4 (float64), r = 148 .. 161 / 421 .. 431 units
UBLK_FAR = {"float32": (100.0, 180.0), "float64": (380.0, 480.0)}
UBLK_FAR_SHAPE = (257, 129)
UBLK_FAR_DS = (4, 8)


def grid_flags(d, dy):
    return HD_ALL if dy == d else EVAL_V | EVAL_JAC


def ncols(d, dy, flags):
    """Columns of the evaluator's product [v | W]: v alone, or v and the dy x d block W."""
    return dy * (1 + d) if flags & ~EVAL_V else dy


def nct(d, dy, flags):
    """Column tiles of 16: cdiv(ncols, 16) of mvf_eval_d, the NCT of eval_d_kernel<T, D, NCT>."""
    return -(-ncols(d, dy, flags) // 16)


def out_shapes(n, d, dy):
    return {EVAL_V: (n, dy), EVAL_JAC: (dy, d, n), EVAL_DIV: (n,), EVAL_ACC: (n, d), EVAL_CURV: (n, d)}


def _unit(rng, k, d):
    u = rng.standard_normal((k, d))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def eval_case(n, m, d, dy):
    """Queries X (n, d), control points (m, d) and coefficients C (m, dy) as the module docstring describes them."""
    rng = np.random.default_rng(100000 * d + 10000 * dy + 1000 * n + m)
    s = np.sqrt(3.0 / d)
    anchor = ANCHOR[:d]
    few = m < 16
    ctrl = anchor + rng.uniform(-6.0 * s, 6.0 * s, (m, d)) if few else rng.uniform(-30.0 * s, 30.0 * s, (m, d))
    C = rng.uniform(0.5, 1.5, (m, dy)) * COEF
    if m:
        ctrl[m - 1] = anchor
        ctrl[m - 1, 0] += 3.0
        C[m - 1] = BIG * COEF * DIR_LAST[:dy]
    second = HD_CHUNK - 1 if m > HD_CHUNK else (0 if m >= 16 else None)
    if second is not None:
        ctrl[second] = anchor
        ctrl[second, 1] -= 3.0
        C[second] = BIG * COEF * DIR_CHUNK[:dy]
    if few:
        X = anchor + (6.0 + rng.uniform(0.5, 8.0, (n, d))) * s
        ends = anchor + (6.0 + np.stack([rng.uniform(7.0, 8.0, d), rng.uniform(0.5, 1.5, d)])) * s
    else:
        X = anchor + _unit(rng, n, d) * rng.uniform(1.5, 14.0, (n, 1))
        ends = anchor + _unit(rng, 2, d) * np.array([[rng.uniform(12.0, 14.0)], [rng.uniform(1.5, 4.0)]])
        if n:
            X[0] = anchor + _unit(rng, 1, d)[0] * rng.uniform(1.5, 4.0)
    if n >= 3:
        X[n - 2] = ends[0]
    if n >= 2:
        X[n - 1] = ends[1]
    return {"X": X, "ctrl": ctrl, "C": C, "beta": BETA}


def eval_d_reference(xp, X, ctrl, C, beta, flags=HD_ALL):
    """Every output of mvf_eval_d pair by pair in the floating-point type `xp` (np.float64: the restatement the device is
    compared with; np.longdouble: what tests/test_highd_kernel_refs.py ties it to).  K = exp(-beta |x - c|^2), v = K C
    (n, dy), J[f][i][q] = -2 beta sum_m K C_mf (x - c)_i (dy, d, n); for dy == d: div = trace J, acc = J v and
    curv = (a (v.v) - v (v.a)) / |v|^4.  An empty sum is 0, 0 / 0 is NumPy's NaN."""
    X = np.asarray(X, dtype=xp)
    n, d = X.shape
    ctrl = np.asarray(ctrl, dtype=xp).reshape(-1, d)
    C = np.asarray(C, dtype=xp)
    dy = C.shape[1]
    beta = xp(beta)
    D = X[:, None, :] - ctrl[None, :, :]                      # (n, m, d)
    K = np.exp(-beta * np.sum(D * D, axis=2))                 # (n, m)
    v = K @ C
    out = {}
    if flags & EVAL_V:
        out[EVAL_V] = v
    if not flags & ~EVAL_V:
        return out
    J = np.empty((dy, d, n), dtype=xp)
    for f in range(dy):
        J[f] = -2 * beta * np.einsum("nm,nmi->in", K * C[None, :, f], D)
    if flags & EVAL_JAC:
        out[EVAL_JAC] = J
    if flags & (EVAL_DIV | EVAL_ACC | EVAL_CURV):
        assert dy == d, "divergence / acceleration / curvature need dy == d"
        a = np.einsum("fin,ni->nf", J, v)
        if flags & EVAL_DIV:
            out[EVAL_DIV] = np.einsum("iin->n", J)
        if flags & EVAL_ACC:
            out[EVAL_ACC] = a
        if flags & EVAL_CURV:
            vv, va = np.sum(v * v, 1), np.sum(v * a, 1)
            with np.errstate(invalid="ignore", divide="ignore"):
                out[EVAL_CURV] = (a * vv[:, None] - v * va[:, None]) / (vv * vv)[:, None]
    shapes = out_shapes(n, d, dy)
    assert all(o.shape == shapes[f] for f, o in out.items())
    return out


def curv_scale(ref):
    """max_q |a| / min_q |v|^2: the size of the two terms a (v.v) / |v|^4 and v (v.a) / |v|^4 whose difference the
    curvature is."""
    vn, an = np.linalg.norm(ref[EVAL_V], axis=1), np.linalg.norm(ref[EVAL_ACC], axis=1)
    return float(an.max() / vn.min() ** 2)


def eval_errors(got, ref, m):
    """flag -> max |got - ref| over ALL queries relative to the quantity's maximum.  With m <= FEW control points the
    curvature is taken relative to `curv_scale` instead: one control point dominates, a = J v is parallel to v and the true
    curvature is 0 but for rounding (the 3-D suite escapes through the affine constant b, which mvf_eval_d does not have),
    so its rounding error goes with the terms it is the difference of, not with its own size - as det J of the 3-D
    evaluator is taken relative to max |J|^3 (_cell_cases.eval_errors).  `ref` must then hold v and acc."""
    out = {}
    for f in ref:
        if f == EVAL_CURV and m <= FEW:
            out[f] = float(np.abs(np.asarray(got[f]) - ref[f]).max() / curv_scale(ref))
        else:
            out[f] = relmax(got[f], ref[f])
    return out


# ------------------------------------------------------------------------------------------------------ mutations
def input_mutations(case):
    """name -> mutated INPUTS: the control point a dropped k-step tail / a dropped chunk end would lose."""
    m = len(case["ctrl"])
    out = {}
    if m:
        out["drop_last_ctrl"] = dict(case, ctrl=case["ctrl"][:-1], C=case["C"][:-1])
    if m > HD_CHUNK:
        keep = np.arange(m) != HD_CHUNK - 1
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


def swap_jac_axes(outs):
    """J[f][i] <-> J[i][f] (dy == d): the epilogue reading W transposed."""
    return {**outs, EVAL_JAC: np.swapaxes(outs[EVAL_JAC], 0, 1).copy()}


def shift_w_column(outs):
    """J[f][i] <- J[f][(i + 1) % d]: the W column of the product off by one."""
    return {**outs, EVAL_JAC: np.roll(outs[EVAL_JAC], -1, axis=1)}


# ------------------------------------------------------------------------------------------------------ con_K, cache
def conk_case(n, m, d, far=None):
    """x (n, d) and y (m, d) from the same +-30 sqrt(3 / d) cloud: most kernel values are far from underflow.  far = (lo, hi):
    every row of x is moved lo .. hi units away instead (UBLK_FAR: to where part of the cell dtype's kernel values are
    denormal and part are 0)."""
    rng = np.random.default_rng(1000003 * d + 1009 * n + m + (5 if far else 0))
    s = np.sqrt(3.0 / d)
    x, y = rng.uniform(-30.0 * s, 30.0 * s, (n, d)), rng.uniform(-30.0 * s, 30.0 * s, (m, d))
    if far:
        x = x + _unit(rng, n, d) * rng.uniform(far[0], far[1], (n, 1))
    return x, y


def conk_reference(xp, x, y, beta):
    x, y = np.asarray(x, dtype=xp), np.asarray(y, dtype=xp)
    D = x[:, None, :] - y[None, :, :]
    return np.exp(-xp(beta) * np.sum(D * D, axis=2))
