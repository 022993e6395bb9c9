"""Shared by tests/test_gpu_eval_wide_kernels.py (mvf_eval_wide on the device), tests/test_eval_wide_refs.py and
tests/test_eval_wide_host.py (no GPU): the seeded inputs, the shape lists and the NumPy reference of the wide evaluator - values
v = K @ C (n x dy) and the Jacobian J[f][i][q] = -2 beta sum_m K(x_q, c_m) C[m, f] (x_q - c_m)_i (dy, d, n) of a field with any
number of output columns dy at d = 1, 2, 3.

Tolerances and conventions are tests/_cell_cases.py's (TOL, relmax, BETA, COEF, BIG, ANCHOR; nothing new): control points in a
+-30 cloud, strictly positive coefficients, the LAST control point and the last one of the first staging chunk (index CHUNK - 1)
carry BIG x COEF coefficients 3 units on either side of ANCHOR, the first and the last query sit 1.5 .. 4 units from ANCHOR and
every other one 1.5 .. 14 units; fewer than 16 control points are drawn within +-6 of ANCHOR with the queries 0.5 .. 8 beyond that
box (here the first and the last query at its near corner and the last one's neighbour at its far corner, so that a last query
that repeats its neighbour is a gross error with one control point too).  Here the coefficients have dy columns and column f carries the factor COLUMN_FACTORS[f % 3], so that a column written one
place off is a gross error; in d < 3 dimensions only the first d coordinates are used.  The points are centred on the control
points' mean before they meet the kernel, as the product's to_x4(..., center) does: |p| stays within the data's radius and
p v - W does not cancel beyond what _cell_cases' evaluator cases see."""
import functools

import numpy as np

from _cell_cases import ANCHOR, BETA, BIG, COEF, EVAL_JAC, EVAL_V

PANEL = 64   # EW_PANEL of csrc/mvf_eval_wide.hip: columns of C per workgroup
CHUNK = 64   # EW_CHUNK: control points staged per pass
COLUMN_FACTORS = (1.0, 2.0, 3.0)

BASE = (65, 259, 65, 3)  # (n, m, dy, d)
NS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257)                       # 16-query tile, 64-query workgroup, several workgroups
MS = (1, 2, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 1023)               # k-step of 4 and the staging chunk
DYS = (1, 4, 15, 16, 17, PANEL - 1, PANEL, PANEL + 1, 2 * PANEL + 2)  # 16-column tile and the 64-column panel
DS = (1, 2, 3)
SWEEP = list(dict.fromkeys([BASE] + [(n, BASE[1], BASE[2], BASE[3]) for n in NS] + [(BASE[0], m, BASE[2], BASE[3]) for m in MS]
                           + [(BASE[0], BASE[1], dy, BASE[3]) for dy in DYS] + [(BASE[0], BASE[1], BASE[2], d) for d in DS]))


def _unit(rng, k, d):
    u = rng.standard_normal((k, d))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def wide_case(n, m, dy, d):
    """{"X" (n, d), "ctrl" (m, d), "C" (m, dy), "beta", "d"}: centred points, read-only arrays (one instance per shape)."""
    rng = np.random.default_rng(100003 * n + 1009 * m + 17 * dy + d)
    anchor = ANCHOR[:d]
    ctrl = (anchor + rng.uniform(-6.0, 6.0, (m, d))) if m < 16 else rng.uniform(-30.0, 30.0, (m, d))
    col = np.array([COLUMN_FACTORS[f % 3] for f in range(dy)])
    C = rng.uniform(0.5, 1.5, (m, dy)) * COEF * col[None, :]
    first = np.zeros(d)
    first[0] = 3.0
    if m:
        ctrl[m - 1] = anchor + first
        C[m - 1] = BIG * COEF * col * np.resize([1.0, 0.6, 0.8], dy)
    if CHUNK - 1 < m - 1:
        ctrl[CHUNK - 1] = anchor - first
        C[CHUNK - 1] = BIG * COEF * col * np.resize([0.7, 1.0, 0.5], dy)
    if m < 16:
        X = anchor + 6.0 + rng.uniform(0.5, 8.0, (n, d))
        if n:  # the first and the last query at the near corner of that box, the last one's neighbour at the far corner
            X[0] = X[n - 1] = anchor + 6.5
        if n > 2:
            X[n - 2] = anchor + 13.5
    else:
        X = anchor + _unit(rng, n, d) * rng.uniform(1.5, 14.0, (n, 1))
        near = anchor + _unit(rng, 2, d) * rng.uniform(1.5, 4.0, (2, 1))
        if n:
            X[0] = near[0]
            X[n - 1] = near[1]
    center = ctrl.mean(0) if m else np.zeros(d)
    out = {"X": X - center, "ctrl": ctrl - center, "C": C, "beta": BETA, "d": d}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def round_cell(a, dtype):
    """The values the kernel reads: rounded to the cell dtype, as float64."""
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) if dtype == "float32" else a


def wide_reference(X, ctrl, C, beta, flags=EVAL_V | EVAL_JAC, dtype="float64"):
    """{EVAL_V: v (n, dy), EVAL_JAC: J (dy, d, n)} in float64 from points and control points rounded to the cell dtype `dtype`
    (everything else float64), pair by pair as _cell_cases.eval_reference does."""
    X, ctrl = round_cell(X, dtype), round_cell(ctrl, dtype)
    d = X.shape[1]
    ctrl = ctrl.reshape(-1, d)
    C = np.asarray(C, dtype=np.float64)  # (m, dy)
    D = X[:, None, :] - ctrl[None, :, :]                        # (n, m, d)
    K = np.exp(-beta * np.sum(D * D, axis=2))                   # (n, m)
    out = {}
    if flags & EVAL_V:
        out[EVAL_V] = K @ C
    if flags & EVAL_JAC:
        out[EVAL_JAC] = -2.0 * beta * np.stack([(K * D[:, :, i]) @ C for i in range(d)], axis=0).transpose(2, 0, 1)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(n, m, dy, d, dtype):
    """wide_reference of wide_case(n, m, dy, d) at cell dtype `dtype`: computed once, shared, read-only."""
    c = wide_case(n, m, dy, d)
    ref = wide_reference(c["X"], c["ctrl"], c["C"], c["beta"], dtype=dtype)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def pad4(a):
    """(k, d <= 3) -> (k, 4) zero padded: the x4 layout."""
    a = np.asarray(a, dtype=np.float64)
    out = np.zeros((len(a), 4))
    out[:, : a.shape[1]] = a
    return out


def wide_mutations(case):
    """name -> outputs of the one-off slip each edge of the sweep exists to catch (computed with the float64 reference):
    the last control point dropped, the chunk-end control point dropped, every column written one place off, the last query
    repeating its neighbour."""
    X, ctrl, C, beta = case["X"], case["ctrl"], case["C"], case["beta"]
    m, dy, n = len(ctrl), C.shape[1], len(X)
    good = wide_reference(X, ctrl, C, beta)
    out = {}
    if m:
        out["drop_last_ctrl"] = wide_reference(X, ctrl[:-1], C[:-1], beta)
    if m > CHUNK:
        keep = np.arange(m) != CHUNK - 1
        out["drop_chunk_end"] = wide_reference(X, ctrl[keep], C[keep], beta)
    if dy > 1:
        out["shift_column"] = {EVAL_V: np.roll(good[EVAL_V], 1, axis=1), EVAL_JAC: np.roll(good[EVAL_JAC], 1, axis=0)}
    if n > 1:
        v, J = good[EVAL_V].copy(), good[EVAL_JAC].copy()
        v[-1], J[:, :, -1] = v[-2], J[:, :, -2]
        out["shift_query"] = {EVAL_V: v, EVAL_JAC: J}
    return good, out
