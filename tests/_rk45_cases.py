"""Shared by tests/test_gpu_rk45_kernels.py (``rk45_kernel`` on the device, through HipKernels.integrate_rk45 and the C entry
point) and tests/test_rk45_kernel_refs.py (no GPU): the seeded inputs of the adaptive integrator's edge cases, the SciPy
reference on a float64 NumPy restatement of the kernel's field, the stability filter, the resampling rules and the tolerances.

Reference: ``scipy.integrate.solve_ivp(method="RK45", rtol=1e-3, atol=1e-6, max_step=..., dense_output=True, events=<at rest,
terminal>)`` exactly as tests/test_gpu_rk45.py::_scipy states it, on ``field()`` of csrc/mvf_rk45.hip in world coordinates:
v = scale * (alpha * K(q) @ C + A q + b) with q = (y - offset) / scale, the state holding the field's own d components (its
RMS norm is over d).  Status -2 (this library's cap on step attempts) has no solve_ivp counterpart: ``capped_reference``
drives the public ``scipy.integrate.RK45`` by hand for the capped number of attempts.

Input design.  All coordinates sit on the float32 grid, so both cell dtypes integrate the same field from the same points.
  * "moving" cases: control points in a +-30 cloud with signed coefficients N(0, COEF^2) (fewer than 16 points: within +-6 of
    ANCHOR, every coefficient of size BIG), starts 1.5 .. 6 units from ANCHOR, t_bound = +-40 with max_step = 1 or inf.  A
    Gaussian field alone pushes a start away and lets it coast: at rtol = 1e-3 SciPy then takes steps of 6 and more, max_step
    sets every step and nothing is ever rejected.  So the affine part carries a rotation about the origin (SWIRL, one turn
    in 6.3 time units): the paths keep circling through the bumps, the error control sets the steps (44 .. 49 per path, up to
    9 rejected) with or without max_step.  In 1-D there is no rotation; that case has 6 or 7 free steps.
    PLANTED points carry coefficients of BIG and sit 3 units from ANCHOR, each on its own side: the last control point, and
    the last point of every full LDS stage with the first point of the next (indices j cap - 1 and j cap).  A random extra
    control point barely moves a trajectory (dropping the last of 2305 random points: 7e-8 of a unit); a dropped planted
    point moves the compared samples by whole units (test_rk45_kernel_refs.py: >= 5e7 tolerances).
  * "event" cases: ONE control point at the origin, C = (0.05, 0, 0), beta = 0.02, |t_bound| = 1e5, max_step = |t_bound| / 50.
    A start at |x| = 20.9 on the inflow side is at rest (|v| = 8e-6) and LEAVES rest (the event fires with the root on the
    start side of the bracket); one at |x| = 20.0 on the outflow side ENTERS rest; one at |x| = 60 never moves (the path has
    length exactly 0: |v| 1e5 = 3e-28 is absorbed by 60.0).

Stability filter.  Step-for-step equality with SciPy means something only where the step sequence does not hang on the last
bits of the field, so every distinct start is solved three times: as is and with the field scaled by 1 +- 1e-13 (the device's
exp2 on pre-scaled coordinates against NumPy's exp: a few ulp of an exponent argument of at most ~60, about 2e-14).  A start is
KEPT where the three runs agree on len(sol.t), sol.nfev and sol.status; dropped starts leave the SciPy comparisons only.
Condition (not a measurement): >= 90 % of every case's starts are kept - with the seeds here, all of them.

Tolerances.  float64: states 1e-9 x the extent of the field's data (tests/test_gpu_rk45.py), arc-length times 1e-8 |t_bound|,
step counts / field evaluations / status exact on kept starts.  float32: no counts; states within 10 x D32 x the extent of
motion, D32 = the largest deviation between SciPy on the float64 field and SciPy on the float32 restatement of the field
(``field32``) over all float32 cases, at the samples of the sampling mode compared (``d32(sampling)``), status where those
two CPU routes agree.
"""
import functools

import numpy as np
from scipy.integrate import RK45, OdeSolution, solve_ivp

# LDS per staged control point = sizeof(vec4<T>) + 32 B, 144 KiB in all (csrc/mvf_rk45.hip:428-430)
CAP = {"float32": (144 * 1024) // (16 + 32), "float64": (144 * 1024) // (32 + 32)}
DTYPES = ("float64", "float32")
RTOL, ATOL = 1e-3, 1e-6
LOG2E = 1.4426950408889634074

TOL_X64 = 1e-9       # x extent of the field's data
TOL_T64 = 1e-8       # x |t_bound| (arc_length times)
D32_FACTOR = 10.0
MUTATION_FACTOR = 1000.0
FILTER_EPS = 1e-13
KEEP_MIN = 0.9
FIELD32_RTOL = 2e-5  # |float32 restatement - float64 field| <= this x max |v| over a case's starts (test_rk45_kernel_refs.py)
BISECT_MAX = 100     # brentq's maxiter as the kernel restates it: at most 100 + 1 evaluations of one event's bisection

BETA = 0.02
COEF = 0.04
BIG = 1.0
ANCHOR = np.array([5.0, -4.0, 3.0])
T_MOVING, STEP_MOVING = 40.0, 1.0
SWIRL = 1.0
_PLACES = np.array([[3.0, 0, 0], [-3.0, 0, 0], [0, 3.0, 0], [0, -3.0, 0], [0, 0, 3.0], [0, 0, -3.0]])
_DIRS = np.array([[1.0, 0.6, 0.8], [0.7, -1.0, 0.5], [-0.5, 0.8, 1.0], [0.9, 0.5, -0.7], [-0.8, -0.6, 1.0], [1.0, -0.5, -0.9]])

LANE_NS = (1, 63, 64, 65, 255, 256, 257, 513)
LANE_CHUNKED_NS = (257, 513)
LANE_M, LANE_STARTS = 40, 19
COUNT_N = 70
NOUTS = (2, 3, 101)
SAMPLINGS = ("uniform_time", "arc_length")
BAD_LANES = (0, 63, 64, 255, 256, 299)
WORLD_SCALE, WORLD_OFFSET = np.array([1.0, -1.3, 0.8]), np.array([12.5, -7.25, 3.0])


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def count_ms(dtype):
    """Control-point counts of the sweep: the affine part alone, the remainders of the loop unrolled by 4, and the LDS stage
    boundary (one chunk, a tail of one point, two full chunks, two and a tail of one)."""
    cap = CAP[dtype]
    return (0, 1, 3, 4, 5, cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1)


def planted(m, cap):
    """Indices that carry the big coefficients (module docstring)."""
    idx = {m - 1} if m else set()
    for j in range(1, m // cap + 1):
        idx.update(i for i in (j * cap - 1, j * cap) if i < m)
    return sorted(idx)


# ------------------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def moving_case(m, cap, d=3, affine=False, world=False, nstarts=8, t_bound=T_MOVING, max_step=STEP_MOVING, swirl=True):
    rng = np.random.default_rng(100003 * d + 17 * m + 5 * nstarts + (3 if affine else 0) + (1 if world else 0) + (11 if swirl else 0))
    if m < 16:
        ctrl = ANCHOR + rng.uniform(-6.0, 6.0, (m, 3))
        C = BIG * rng.uniform(0.5, 1.5, (m, 3)) * np.array([1.0, -0.7, 0.8])
    else:
        ctrl = rng.uniform(-30.0, 30.0, (m, 3))
        C = COEF * rng.standard_normal((m, 3))
    for t, j in enumerate(planted(m, cap)):
        ctrl[j] = ANCHOR + _PLACES[t % 6] * (1.0 + 0.25 * (t // 6))
        C[j] = BIG * _DIRS[t % 6]
    u = rng.standard_normal((nstarts, 3))
    u[:, d:] = 0.0
    starts = ANCHOR + u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(1.5, 6.0, (nstarts, 1))
    ctrl[:, d:] = 0.0      # what to_x4 pads an (m, d) array with
    starts[:, d:] = 0.0
    alpha, A, b = np.ones(3), np.zeros((3, 3)), np.zeros(3)
    if affine:  # GP style: per-axis alpha, a small linear part and a constant drift
        alpha, A, b = np.array([0.9, 1.3, 1.1]), 2e-3 * rng.standard_normal((3, 3)), np.array([0.05, -0.08, 0.04])
    if swirl:   # a rotation about the origin keeps the paths among the bumps: the error control, not max_step, sets the steps
        A = A + SWIRL * np.array([[0.0, -1.0, 0.3], [1.0, 0.0, -0.2], [-0.3, 0.2, 0.0]])
    aff = (alpha, 1.0, A, b) if affine or swirl else None
    scale, offset = np.ones(3), np.zeros(3)
    if world:
        scale, offset = WORLD_SCALE.copy(), WORLD_OFFSET.copy()
        offset[d:] = 0.0
    return {"name": f"moving m={m} d={d} T={t_bound:g} h<={max_step:g}" + (" affine" if affine else "") + (" world" if world else "")
                    + (" swirl" if swirl else ""),
            "ctrl": _f32(ctrl), "C": C, "beta": BETA, "affine": aff, "d": d, "scale": scale, "offset": offset,
            "starts": _f32(starts), "t_bound": float(t_bound), "max_step": float(max_step), "cap": cap}


@functools.lru_cache(maxsize=None)
def event_case(d=3, sign=1.0, t_bound=1e5, max_step=None):
    """Starts by kind for the direction `sign`: leaving rest, entering rest, never moving (two or more of each)."""
    x = np.array([-20.9, -20.85, -20.95, 20.0, 20.1, 19.9, -60.0, 60.0, -60.0]) * sign
    yz = np.array([[0.3, -0.2], [-0.2, 0.1], [0.1, 0.4], [0.3, -0.2], [-0.4, 0.2], [0.0, 0.0], [0.3, -0.2], [5.0, 1.0],
                   [-30.0, 40.0]])
    starts = np.concatenate([x[:, None], yz], axis=1)
    starts[:, d:] = 0.0
    C = np.array([[0.05, 0.0, 0.0]])
    return {"name": f"event d={d} T={sign * t_bound:g}", "ctrl": np.zeros((1, 3)), "C": C, "beta": BETA,
            "affine": None, "d": d, "scale": np.ones(3), "offset": np.zeros(3), "starts": _f32(starts),
            "t_bound": float(sign * t_bound), "max_step": float(t_bound / 50 if max_step is None else max_step), "cap": CAP["float64"]}


def with_garbage(case, value=7.0):
    """What the dimension test feeds the kernel: `value` in the unused components of the starts and the unused columns of C."""
    d = case["d"]
    starts, C = case["starts"].copy(), case["C"].copy()
    starts[:, d:] = value
    C[:, d:] = value
    return dict(case, starts=starts, C=C)


def capped_case():
    """Status -2: the event field over |t_bound| = 2000 with max_step >= |t_bound|.  The rows at rest near |x| = 20.9 (and the
    slowest movers) grow their step tenfold per attempt and arrive within 5 attempts; the faster movers need more and meet a
    rejection on the way; the row at |x| = 60 starts from h = 1e-6 and is capped at t = 0.011 on a path of length 0."""
    case = event_case(3, 1.0, 2000.0, np.inf)
    starts = _f32(np.array([[-20.9, 0.3, -0.2], [-15.0, 1.0, 0.5], [-20.8, -0.2, 0.1], [-12.0, -2.0, 1.0], [-8.0, 0.5, 0.5],
                            [-60.0, 0.3, -0.2], [-17.0, 0.0, 3.0], [-3.0, 0.5, -0.5], [-10.0, 3.0, 0.0]]))
    return dict(case, name="capped", starts=starts)


CAPPED_STEPS, CAPPED_NOUT = 5, 30


def world_starts(case, starts=None):
    """y = q * scale + offset on the field's own d components."""
    q = case["starts"] if starts is None else starts
    return (q * case["scale"] + case["offset"])[:, : case["d"]]


def data_extent(case):
    """The extent of the field's data (control points and starts) in world coordinates: what the float64 tolerance is relative to."""
    pts = np.concatenate([case["ctrl"], case["starts"]]) * case["scale"] + case["offset"]
    return float(np.ptp(pts[:, : case["d"]], axis=0).max())


# ------------------------------------------------------------------------------------------------------ fields
def _affine_parts(case):
    if case["affine"] is None:
        return np.ones(3), np.zeros((3, 3)), np.zeros(3)
    alpha, _, A, b = case["affine"]
    return np.broadcast_to(np.asarray(alpha, dtype=np.float64).reshape(-1), (3,)), np.asarray(A, float), np.asarray(b, float)


def field64(case, gain=1.0, drop=None, components=None):
    """y (d,) or (3,) world -> v.  drop: control-point indices left out (mutations); components: how many components of v
    are returned (default d; 3 = what a kernel that forgot d would see: alpha K @ C of the unused columns)."""
    d = case["d"]
    keep = np.ones(len(case["ctrl"]), dtype=bool)
    if drop is not None:
        keep[list(drop)] = False
    ctrl, C = case["ctrl"][keep], case["C"][keep]
    alpha, A, b = _affine_parts(case)
    scale, offset, beta = case["scale"], case["offset"], case["beta"]
    assert not offset[d:].any()
    nc = d if components is None else components

    def f(y):
        q = np.zeros(3)
        q[:d] = (np.asarray(y, dtype=np.float64)[:d] - offset[:d]) / scale[:d]
        D = q - ctrl
        k = np.exp(-beta * np.sum(D * D, axis=1))
        return gain * (scale * (alpha * (k @ C) + A @ q + b))[:nc]

    return f


def field32(case):
    """The float32 kernel's field: coordinates and s = sqrt(beta log2e) rounded to float32, differences, squares and exp2 in
    float32, the sum with C in float64 (no fused multiply-adds, NumPy's exp2 for v_exp_f32)."""
    d = case["d"]
    s = np.float32(np.sqrt(case["beta"] * LOG2E))
    cs = case["ctrl"].astype(np.float32) * s
    C = case["C"]
    alpha, A, b = _affine_parts(case)
    scale, offset = case["scale"], case["offset"]

    def f(y):
        q = np.zeros(3)
        q[:d] = (np.asarray(y, dtype=np.float64)[:d] - offset[:d]) / scale[:d]
        D = q.astype(np.float32) * s - cs
        e = D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1] + D[:, 2] * D[:, 2]
        k = np.exp2(-e).astype(np.float64)
        assert e.dtype == np.float32
        return (scale * (alpha * (k @ C) + A @ q + b))[:d]

    return f


def solve(f, y0, t_bound, max_step, threshold=1e-5, rest_field=None):
    """tests/test_gpu_rk45.py::_scipy with the tolerances spelled out; `threshold` / `rest_field` for the event's mutations."""
    g = f if rest_field is None else rest_field
    ev = lambda t, y: float(np.all(np.abs(g(y)) < threshold)) - 1 + 1e-12  # noqa: E731
    ev.terminal = True
    return solve_ivp(lambda t, y: f(y), (0.0, t_bound), y0, method="RK45", rtol=RTOL, atol=ATOL, max_step=max_step,
                     dense_output=True, events=ev)


def signature(sol):
    return len(sol.t), sol.nfev, sol.status


def _ident(case):
    return (case["name"], case["ctrl"].tobytes(), case["C"].tobytes(), case["starts"].tobytes(), case["t_bound"], case["max_step"],
            case["scale"].tobytes(), case["offset"].tobytes(), case["d"], repr(case["affine"]))


_SOLS, _KEPT, _SOLS32 = {}, {}, {}


def reference(case):
    """The SciPy solution on the float64 field for every distinct start.  Computed once per case and shared (nothing may
    change it)."""
    key = _ident(case)
    if key not in _SOLS:
        _SOLS[key] = [solve(field64(case), y0, case["t_bound"], case["max_step"]) for y0 in world_starts(case)]
    return _SOLS[key]


def kept(case):
    """The stability filter (module docstring): one flag per distinct start."""
    key = _ident(case)
    if key not in _KEPT:
        flags = []
        for y0, sol in zip(world_starts(case), reference(case)):
            others = [solve(field64(case, g), y0, case["t_bound"], case["max_step"]) for g in (1 - FILTER_EPS, 1 + FILTER_EPS)]
            flags.append(len({signature(s) for s in [sol] + others}) == 1)
        _KEPT[key] = np.array(flags)
    return _KEPT[key]


def reference32(case):
    """SciPy on the float32 restatement of the field: the second CPU route of the float32 yardstick."""
    key = _ident(case)
    if key not in _SOLS32:
        f = field32(case)
        _SOLS32[key] = [solve(f, y0, case["t_bound"], case["max_step"]) for y0 in world_starts(case)]
    return _SOLS32[key]


def rejected(sol):
    """Rejected attempts of a solve_ivp run: every attempt costs 6 evaluations, RungeKutta.__init__ and select_initial_step one each."""
    return (sol.nfev - 2) // 6 - (len(sol.t) - 1)


# ------------------------------------------------------------------------------------------------------ sampling
def resample(ts, xs, dense, t_bound, n_out, sampling):
    """The n_out samples of one path (ts (k,), xs (k, d) its step points, dense(t) -> (d, len(t)) its dense output).
    uniform_time: sign * linspace(0, |t_bound|), the dense output up to the path's end and its end state after it
    (tests/test_gpu_rk45.py::test_kernel_steps_as_scipy); arc_length: oracle.trajectory_oracle.fate_arclength's rule on the same
    solution (equal steps of arc length along the polyline of step points, times by np.interp, states on the dense output; a
    path of length 0: uniform times up to its end)."""
    sign = 1.0 if t_bound > 0 else -1.0
    if sampling == "uniform_time":
        tq = sign * np.linspace(0, abs(t_bound), n_out)
        inside = sign * (tq - ts[-1]) <= 0
        x = np.broadcast_to(xs[-1], (n_out, xs.shape[1])).copy()
        if inside.any():
            x[inside] = dense(tq[inside]).T
        return tq, x
    seg = np.linalg.norm(np.diff(xs, axis=0), axis=1)
    s = np.concatenate([[0.0], np.cumsum(seg)])
    sq = np.linspace(0.0, s[-1], n_out)
    tq = np.interp(sq, s, ts) if s[-1] > 0 else np.linspace(ts[0], ts[-1], n_out)
    return tq, dense(tq).T


def resample_sol(sol, t_bound, n_out, sampling):
    return resample(sol.t, sol.y.T, sol.sol, t_bound, n_out, sampling)


def chords(x):
    return np.linalg.norm(np.diff(x, axis=0), axis=1)


def motion(x):
    """max |x(t) - x(0)| of one sampled path."""
    return float(np.abs(x - x[:1]).max())


def capped_reference(f, y0, t_bound, max_step, max_attempts):
    """scipy.integrate.RK45 stepped by hand until `max_attempts` step attempts (accepted + rejected; every one costs 6
    evaluations) are spent: the accepted steps that fit, their dense outputs, and the final status (0 when t_bound was
    reached within the cap, else -2).  Events are not looked at: the caller asserts that no start changes its at-rest state."""
    solver = RK45(lambda t, y: f(y), 0.0, np.asarray(y0, dtype=np.float64), t_bound, max_step=max_step, rtol=RTOL, atol=ATOL)
    ts, xs, dense = [0.0], [np.array(y0, dtype=np.float64)], []
    status, attempts = -2, 0
    while True:
        msg = solver.step()
        assert msg is None, msg
        now = (solver.nfev - 2) // 6
        if now > max_attempts:   # this accepted step came after the cap: the attempts before it were rejections
            break
        attempts = now
        ts.append(solver.t)
        xs.append(solver.y.copy())
        dense.append(solver.dense_output())
        if solver.status == "finished":
            status = 0
            break
        if attempts == max_attempts:
            break
    n_acc = len(ts) - 1
    n_rej = (attempts if status == 0 else max_attempts) - n_acc
    ts, xs = np.array(ts), np.array(xs)
    sol = OdeSolution(ts, dense) if dense else (lambda t: np.repeat(xs[0][:, None], len(np.atleast_1d(t)), axis=1))
    return {"t": ts, "x": xs, "dense": sol, "status": status, "accepted": n_acc, "rejected": n_rej}


_CAPPED = {}


def capped_references(case, field=field64):
    """capped_reference per start of the -2 case, and the stability filter on (accepted, rejected, status)."""
    key = (_ident(case), field.__name__)
    if key not in _CAPPED:
        run = lambda f: [capped_reference(f, y0, case["t_bound"], case["max_step"], CAPPED_STEPS)  # noqa: E731
                         for y0 in world_starts(case)]
        refs = run(field(case))
        sig = lambda r: (r["accepted"], r["rejected"], r["status"])  # noqa: E731
        flags = np.ones(len(refs), dtype=bool)
        if field is field64:
            for g in (1 - FILTER_EPS, 1 + FILTER_EPS):
                flags &= np.array([sig(a) == sig(b) for a, b in zip(refs, run(field64(case, g)))])
        _CAPPED[key] = (refs, flags)
    return _CAPPED[key]


# ------------------------------------------------------------------------------------------------------ float32 yardstick
def lane_case(dtype, sign=1.0):
    return moving_case(LANE_M, CAP[dtype], nstarts=LANE_STARTS, t_bound=sign * T_MOVING)


def count_case(dtype, m):
    return moving_case(m, CAP[dtype])


def empty_cases(dtype):
    """No control points: the rotation alone, and the GP-style affine part on top of it."""
    return [moving_case(0, CAP[dtype]), moving_case(0, CAP[dtype], affine=True)]


def dim_case(dtype, d):
    """max_step = inf: with the steps set by the error norm alone, a norm over 3 components changes every one of them."""
    return moving_case(LANE_M, CAP[dtype], d=d, max_step=np.inf)


def free_case(dtype):
    return moving_case(LANE_M, CAP[dtype], max_step=np.inf)


def world_cases(dtype):
    """One negative world scale axis, non-zero offsets on the used axes; in 3-D with the GP-style affine part."""
    return [moving_case(LANE_M, CAP[dtype], world=True, affine=True), moving_case(LANE_M, CAP[dtype], d=2, world=True)]


def sweep_cases(dtype):
    """Every case the GPU module runs in `dtype` against SciPy (the -2 case has its own hand-stepped reference)."""
    cases = [lane_case(dtype, s) for s in (1.0, -1.0)] + [count_case(dtype, m) for m in count_ms(dtype)] + empty_cases(dtype)
    cases += [dim_case(dtype, d) for d in (1, 2, 3)] + [event_case(d, 1.0) for d in (1, 2)]
    cases += [event_case(3, s) for s in (1.0, -1.0)] + [free_case(dtype)] + world_cases(dtype)
    return list({c["name"]: c for c in cases}.values())


def float32_cases():
    return sweep_cases("float32")


D32_NOUTS = (2, 3, 7, 40, 101)   # the sample counts the GPU module compares float32 states at


def float32_deviation(case, sampling="uniform_time"):
    """max over the case's starts and over D32_NOUTS of |SciPy(float64 field) - SciPy(float32 restatement)| at the samples of
    `sampling`, as a fraction of the path's extent of motion (paths that do not move: of 1)."""
    worst = 0.0
    for s64, s32 in zip(reference(case), reference32(case)):
        for n_out in D32_NOUTS:
            _, a = resample_sol(s64, case["t_bound"], n_out, sampling)
            _, b = resample_sol(s32, case["t_bound"], n_out, sampling)
            worst = max(worst, float(np.abs(a - b).max()) / (motion(a) or 1.0))
    return worst


@functools.lru_cache(maxsize=None)
def d32(sampling="uniform_time"):
    """The float32 yardstick of one sampling mode.  The modes differ: uniform_time samples sit on the dense output, where a
    shifted accept / reject decision moves them by the integration error; arc_length samples are placed by the polyline of
    the step points themselves, so the same shift moves them by the polyline's distance from the curve."""
    return max(float32_deviation(c, sampling) for c in float32_cases())


@functools.lru_cache(maxsize=None)
def d32_capped(sampling="uniform_time"):
    """The same yardstick for the status -2 case, from the two hand-stepped CPU routes at its own CAPPED_NOUT samples (rows on
    which the routes agree in accepted steps and status).  Kept apart from d32(): five attempts that grow the step tenfold
    each time run at an error norm near 1, where a float32-sized change of the field moves the size of the step after a
    rejection by 0.3 %; folded into d32() this case would widen every other float32 bound tenfold."""
    case = capped_case()
    worst = 0.0
    for a, b in zip(capped_references(case)[0], capped_references(case, field32)[0]):
        if (a["accepted"], a["status"]) != (b["accepted"], b["status"]):
            continue
        _, xa = resample(a["t"], a["x"], a["dense"], case["t_bound"], CAPPED_NOUT, sampling)
        _, xb = resample(b["t"], b["x"], b["dense"], case["t_bound"], CAPPED_NOUT, sampling)
        worst = max(worst, float(np.abs(xa - xb).max()) / (motion(xa) or 1.0))
    return worst
