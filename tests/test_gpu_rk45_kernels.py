"""Kernel-level edge tests of ``rk45_kernel<float|double>`` (csrc/mvf_rk45.hip, mvf_integrate_rk45), the adaptive trajectory
integrator: HipKernels.integrate_rk45 called directly on ``cuda:0`` in both cell dtypes (the guard test calls the C entry point
with its own buffers), against SciPy's own ``solve_ivp(method="RK45")`` on a float64 NumPy restatement of the kernel's field
(tests/_rk45_cases.py: inputs, reference, stability filter, resampling rules, tolerances).

tests/test_rk45_kernel_refs.py proves without a GPU that the filter keeps every start, that each planted control point and each
targeted mistake (norm / at-rest test over 3 components for d < 3, event threshold) is a gross error (>= 1000 tolerances) on
the cases meant to catch it, and computes the float32 yardstick D32.

What is compared.  float64, on the starts the filter keeps: states within 1e-9 of the extent of the field's data, arc-length
times within 1e-8 |t_bound|, chords within twice the state tolerance, uniform times bit for bit, and the four stats columns
exactly (accepted steps, rejected steps = (nfev - 2) / 6 - accepted, field evaluations = nfev, status; a fired event adds its
bisection, at most 101 evaluations).  float32: states within 10 x D32 (of the sampling mode) of the extent of motion, status where SciPy on the
float64 field and SciPy on the float32 restatement agree; no counts and no arc-length times (a float32-sized change of the
field moves the time of a slowly approached event by whole steps); a fired float32 path must end on the event surface of
the float64 field, max |v_c| = 1e-5 to 2e-4.  Bit-equality checks carry no tolerance in either dtype.
No expected value comes from the kernel: every one is SciPy's, the restated field's, or the bits of a differently shaped call.
Run with ``-s`` to see the largest deviation of every case family (profiles/rk45_kernel_edges.md records them)."""
import ctypes

import numpy as np
import pytest
import torch

import _rk45_cases as rc
from _kernel_scaffold import (DEV, MODES, bits as _bits, called as _called, dev as _dev, deviation_table, kernel_cache,
                              Out as _Out, same_bits, under as _under, x4 as _sx4)

pytestmark = pytest.mark.gpu

DTYPES = list(rc.DTYPES)
MAX_STEPS = 100_000
_k = kernel_cache()
_note, _deviation_table = deviation_table("| case family | dtype | largest deviation |")


def _x4(k, a):
    """(n, 3) kernel coordinates (on the float32 grid, or non-finite) -> device (n, 4) of the cell dtype, fourth column 0."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    buf = np.zeros((len(a), 4))
    buf[:, :3] = a
    return torch.from_numpy(buf).to(k.tdtype).to(DEV)


def _inputs(dtype, case, starts=None):
    from spateo_amd import _lib

    k = _k(dtype)
    q = case["starts"] if starts is None else starts
    Cd = torch.from_numpy(np.ascontiguousarray(case["C"], dtype=np.float64).reshape(-1, 3)).to(DEV)
    return k, _x4(k, q), _x4(k, case["ctrl"]), Cd, {"uniform_time": _lib.RK45_UNIFORM_TIME, "arc_length": _lib.RK45_ARC_LENGTH}


def _run(dtype, case, starts=None, n_out=101, sampling="uniform_time", max_steps=MAX_STEPS):
    k, x4, c4, Cd, code = _inputs(dtype, case, starts)
    return k.integrate_rk45(x4, c4, case["beta"], Cd, case["d"], (case["scale"], case["offset"]), case["t_bound"], rc.RTOL,
                            rc.ATOL, case["max_step"], max_steps, code[sampling], n_out, affine=case["affine"])


def _tile(case, n):
    idx = np.arange(n) % len(case["starts"])
    return case["starts"][idx], idx


def _all_same_bits(a, b):
    """Two tuples of outputs, array for array."""
    return all(same_bits(x, y) for x, y in zip(a, b))


def _check_rows_repeat(out, idx):
    """Every row carries the bits of the first copy of its start."""
    first = {j: int(np.flatnonzero(idx == j)[0]) for j in np.unique(idx)}
    src = np.array([first[j] for j in idx])
    for a in out:
        assert np.array_equal(_bits(a), _bits(a[src]))


def _check_path(dtype, family, case, j, t, x, et, ex, sampling, kept=True, d32=None):
    """One sampled path of start j (t (n_out,), x (n_out, 3)) against its expected samples (et, ex (n_out, d))."""
    d32 = rc.d32 if d32 is None else d32
    d, T = case["d"], abs(case["t_bound"])
    assert not x[:, d:].any(), (case["name"], j)
    assert np.all(np.diff(t) * np.sign(case["t_bound"]) >= 0)
    if sampling == "uniform_time":
        np.testing.assert_array_equal(t, et)
    dev = float(np.abs(x[:, :d] - ex).max())
    if dtype == "float64":
        if not kept:
            return
        extent = rc.data_extent(case)
        _note(f"{family}: states / extent", dtype, dev / extent)
        assert dev <= rc.TOL_X64 * extent, (case["name"], j, dev / extent)
        if sampling == "arc_length":
            _note(f"{family}: arc-length times / |t_bound|", dtype, np.abs(t - et).max() / T)
            assert np.abs(t - et).max() <= rc.TOL_T64 * T, (case["name"], j, np.abs(t - et).max() / T)
            assert np.abs(rc.chords(x[:, :d]) - rc.chords(ex)).max() <= 2 * rc.TOL_X64 * extent, (case["name"], j)
    else:
        scale = rc.motion(ex) or 1.0
        _note(f"{family}: states / motion", dtype, dev / scale)
        assert dev <= rc.D32_FACTOR * d32(sampling) * scale, (case["name"], j, dev / scale, d32(sampling))


def _check_stats(dtype, case, j, row, sol, s32=None, kept=True):
    if dtype == "float64":
        if not kept:
            return
        attempts = (sol.nfev - 2) // 6
        assert row[0] == len(sol.t) - 1 and row[1] == rc.rejected(sol) and row[3] == sol.status, (case["name"], j, row, rc.signature(sol))
        if sol.status == 1:
            assert 2 + 6 * attempts < row[2] <= 2 + 6 * attempts + rc.BISECT_MAX + 1, (case["name"], j, row)
        else:
            assert row[2] == sol.nfev, (case["name"], j, row, sol.nfev)
    elif s32.status == sol.status:
        assert row[3] == sol.status, (case["name"], j, row)


def _check_scipy(dtype, family, case, out, n_out, sampling, rows=None):
    """rows[j] = the output row of distinct start j (default: row j)."""
    t, x, stats = out
    sols = rc.reference(case)
    kept = rc.kept(case) if dtype == "float64" else np.ones(len(sols), dtype=bool)
    s32 = rc.reference32(case) if dtype == "float32" else [None] * len(sols)
    assert kept.sum() >= rc.KEEP_MIN * len(kept), (case["name"], kept)
    for j, sol in enumerate(sols):
        r = j if rows is None else rows[j]
        if r is None:
            continue
        et, ex = rc.resample_sol(sol, case["t_bound"], n_out, sampling)
        _check_path(dtype, family, case, j, t[r], x[r], et, ex, sampling, kept[j])
        _check_stats(dtype, case, j, stats[r], sol, s32[j], kept[j])
        if sampling == "arc_length" and sol.status == 1 and dtype == "float64" and kept[j]:   # a fired path ends at the event state
            assert np.abs(x[r, -1, : case["d"]] - sol.y[:, -1]).max() <= rc.TOL_X64 * rc.data_extent(case)
        if dtype == "float32" and stats[r, 3] == 1:
            # a fired float32 path ends ON the event surface max |v_c| = 1e-5 of its own field (bisected to 4 eps of t), and
            # that field is the float64 one to FIELD32_RTOL (CPU-proved for the restatement; x 10 as for D32)
            v_end = np.abs(rc.field64(case)(x[r, -1, : case["d"]])).max()
            _note(f"{family}: |v| at the event state / 1e-5 - 1", dtype, abs(v_end / 1e-5 - 1))
            assert abs(v_end - 1e-5) <= rc.D32_FACTOR * rc.FIELD32_RTOL * 1e-5, (case["name"], j, v_end)


def _first_rows(idx, k):
    return [int(np.flatnonzero(idx == j)[0]) if (idx == j).any() else None for j in range(k)]


# ------------------------------------------------------------------------------------------------------ a. lane position
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,chunked", [(n, False) for n in rc.LANE_NS] + [(n, True) for n in rc.LANE_CHUNKED_NS])
def test_lane_position(dtype, n, chunked):
    """Wave and workgroup edges, live lanes beside dead ones: every row has the bits of the first copy of its start."""
    case = rc.count_case(dtype, rc.CAP[dtype] + 1) if chunked else rc.lane_case(dtype)
    assert (len(case["ctrl"]) > rc.CAP[dtype]) == chunked and len(case["starts"]) <= 19
    starts, idx = _tile(case, n)
    for sampling, n_out in (("uniform_time", 101), ("arc_length", 40)):
        out = _run(dtype, case, starts, n_out, sampling)
        assert out[0].shape == (n, n_out) and out[1].shape == (n, n_out, 3) and out[2].shape == (n, 4)
        assert _all_same_bits(out, _run(dtype, case, starts, n_out, sampling))
        _check_rows_repeat(out, idx)
        _check_scipy(dtype, "lanes" + (" (chunked)" if chunked else ""), case, out, n_out, sampling,
                     rows=_first_rows(idx, len(case["starts"])))


# ------------------------------------------------------------------------------------------------------ b. control points
def _count_params():
    return [pytest.param(dt, m, id=f"{dt}-m={m}") for dt in DTYPES for m in rc.count_ms(dt)]


@pytest.mark.parametrize("dtype,m", _count_params())
def test_control_point_counts(dtype, m):
    """The unrolled loop's remainders and the LDS stage boundary, with weight planted where an off-by-one would lose it."""
    case = rc.count_case(dtype, m)
    assert len(case["ctrl"]) == m
    starts, idx = _tile(case, rc.COUNT_N)
    for sampling, n_out in (("uniform_time", 101), ("arc_length", 40)):
        out = _run(dtype, case, starts, n_out, sampling)
        _check_rows_repeat(out, idx)
        _check_scipy(dtype, "control-point counts", case, out, n_out, sampling)


@pytest.mark.parametrize("dtype", DTYPES)
def test_affine_part_without_control_points(dtype):
    for case in rc.empty_cases(dtype):
        assert case["ctrl"].shape == (0, 3) and case["affine"] is not None
        starts, _ = _tile(case, rc.COUNT_N)
        for sampling in rc.SAMPLINGS:
            _check_scipy(dtype, "m = 0, affine", case, _run(dtype, case, starts, 40, sampling), 40, sampling)


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_field_at_all(dtype):
    """m = 0 without an affine part: v = 0, status 0, every sample is the start, uniform times in both sampling modes."""
    case = rc.moving_case(0, rc.CAP[dtype], swirl=False)
    assert case["affine"] is None and len(case["ctrl"]) == 0
    starts, _ = _tile(case, rc.COUNT_N)
    for sign in (1.0, -1.0):
        c = dict(case, t_bound=sign * case["t_bound"])
        for sampling in rc.SAMPLINGS:
            for n_out in (2, 33):
                t, x, stats = _run(dtype, c, starts, n_out, sampling)
                np.testing.assert_array_equal(t, np.broadcast_to(sign * np.linspace(0, rc.T_MOVING, n_out), t.shape))
                np.testing.assert_array_equal(x, np.broadcast_to(starts[:, None, :], x.shape))
                assert (stats[:, 3] == 0).all() and (stats[:, 1] == 0).all()
    _check_scipy(dtype, "m = 0, no field", case, _run(dtype, case, starts, 33, "uniform_time"), 33, "uniform_time")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chunks", [1, 2])
def test_zero_coefficient_tail_gives_the_bits_of_the_shorter_list(dtype, chunks):
    """m = chunks * cap + 1 with a last coefficient row of zeros runs one more LDS stage (for chunks = 1: the chunked path
    against the unchunked one) and must give the bits of m = chunks * cap: fma(k, 0, a) == a."""
    cap = rc.CAP[dtype]
    case = rc.count_case(dtype, chunks * cap)
    longer = dict(case, ctrl=np.concatenate([case["ctrl"], case["ctrl"][:1] + 1.0]), C=np.concatenate([case["C"], np.zeros((1, 3))]))
    assert len(longer["ctrl"]) == chunks * cap + 1
    starts, _ = _tile(case, rc.COUNT_N)
    for sampling in rc.SAMPLINGS:
        assert _all_same_bits(_run(dtype, case, starts, 40, sampling), _run(dtype, longer, starts, 40, sampling))


# ------------------------------------------------------------------------------------------------------ c. dimension
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [1, 2, 3])
def test_dimension(dtype, d):
    """d = 1, 2, 3 on a moving field and on the event field: garbage in the unused components of the starts and the unused
    columns of C changes no bit, the unused output components are 0, and the norm / the at-rest test are over d components."""
    for case in (rc.dim_case(dtype, d), rc.event_case(d, 1.0)):
        assert not case["offset"][d:].any() and not case["ctrl"][:, d:].any()
        for sampling in rc.SAMPLINGS:
            out = _run(dtype, case, None, 40, sampling)
            _check_scipy(dtype, f"d = {d}", case, out, 40, sampling)
            assert not out[1][:, :, d:].any()
            if d < 3:
                g = rc.with_garbage(case)
                assert (g["starts"][:, d:] == 7.0).all() and (g["C"][:, d:] == 7.0).all()
                assert _all_same_bits(out, _run(dtype, g, None, 40, sampling))


# ------------------------------------------------------------------------------------------------------ d. sampling
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["forward", "backward"])
@pytest.mark.parametrize("sampling", rc.SAMPLINGS)
@pytest.mark.parametrize("n_out", rc.NOUTS)
def test_sample_counts_and_sampling(dtype, n_out, sampling, sign):
    """n_out = 2 (the minimum; k == n_out - 1 is special in both target functions), 3 and 101, on the event field (events that
    fire on leaving and on entering rest, paths of length exactly 0) and on a moving field."""
    for family, case in (("event field", rc.event_case(3, sign)), ("moving field", rc.lane_case(dtype, sign))):
        out = _run(dtype, case, None, n_out, sampling)
        _check_scipy(dtype, f"{family}, {sampling}", case, out, n_out, sampling)
        t, x, _ = out
        for j, sol in enumerate(rc.reference(case)):
            if rc.motion(sol.y.T) == 0.0:   # a path of length 0: uniform times over [0, t_bound], a constant state
                np.testing.assert_array_equal(t[j], sign * np.linspace(0, abs(case["t_bound"]), n_out))
                np.testing.assert_array_equal(x[j], np.broadcast_to(case["starts"][j], (n_out, 3)))


# ------------------------------------------------------------------------------------------------------ e. stats
@pytest.mark.parametrize("dtype", DTYPES)
def test_stats_columns(dtype):
    """Accepted, rejected, field evaluations and status on cases whose reference holds rejections, fired and unfired paths
    (_check_stats; in arc_length mode the stats are those of ONE pass)."""
    rej = fired = unfired = 0
    for case in (rc.lane_case(dtype), rc.free_case(dtype), rc.event_case(3, 1.0), rc.event_case(3, -1.0)):
        sols = rc.reference(case)
        rej += sum(rc.rejected(s) > 0 for s in sols)
        fired += sum(s.status == 1 for s in sols)
        unfired += sum(s.status == 0 for s in sols)
        outs = {s: _run(dtype, case, None, 7, s) for s in rc.SAMPLINGS}
        for sampling, out in outs.items():
            _check_scipy(dtype, "stats", case, out, 7, sampling)
        np.testing.assert_array_equal(outs["uniform_time"][2], outs["arc_length"][2])
    assert rej >= 10 and fired >= 10 and unfired >= 20


# ------------------------------------------------------------------------------------------------------ f. status -2
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sampling", rc.SAMPLINGS)
def test_step_cap(dtype, sampling):
    """max_steps = 5: a capped row has spent exactly 5 attempts, its samples follow the hand-stepped scipy.integrate.RK45 up to
    the last point reached and hold that point afterwards; rows that finish within 5 attempts keep their normal status.
    The float32 yardstick of this case is its own (_rk45_cases.d32_capped)."""
    case = rc.capped_case()
    n_out, d = rc.CAPPED_NOUT, case["d"]
    refs, kept = rc.capped_references(case)
    refs32, _ = rc.capped_references(case, rc.field32)
    t, x, stats = _run(dtype, case, None, n_out, sampling, max_steps=rc.CAPPED_STEPS)
    free = _run(dtype, case, None, n_out, sampling)
    assert (free[2][:, 3] >= 0).all()
    assert {r["status"] for r in refs} == {0, -2} and kept.sum() >= rc.KEEP_MIN * len(kept)
    for j, r in enumerate(refs):
        sig = (r["accepted"], r["status"])
        if dtype == "float32" and sig != (refs32[j]["accepted"], refs32[j]["status"]):
            continue
        if dtype == "float64" and not kept[j]:
            continue
        assert stats[j, 3] == r["status"], (j, stats[j])
        if r["status"] == -2:
            assert stats[j, 0] + stats[j, 1] == rc.CAPPED_STEPS
        else:   # unaffected by the cap: the bits of the uncapped call
            assert _all_same_bits([a[j] for a in (t, x, stats)], [a[j] for a in free])
        if dtype == "float64":
            assert stats[j, 0] == r["accepted"] and stats[j, 1] == r["rejected"] and stats[j, 2] == 2 + 6 * (r["accepted"] + r["rejected"])
        et, ex = rc.resample(r["t"], r["x"], r["dense"], case["t_bound"], n_out, sampling)
        _check_path(dtype, f"status -2, {sampling}", case, j, t[j], x[j], et, ex, sampling, d32=rc.d32_capped)
        if r["status"] == -2:   # the trailing samples hold the last point reached
            late = np.sign(case["t_bound"]) * (et - r["t"][-1]) >= 0
            assert late[-1]
            tol = rc.TOL_X64 * rc.data_extent(case) if dtype == "float64" else rc.D32_FACTOR * rc.d32_capped(sampling) * (rc.motion(ex) or 1.0)
            assert np.abs(x[j, late, :d] - r["x"][-1]).max() <= tol
            if sampling == "arc_length" and dtype == "float64":
                assert abs(t[j, -1] - r["t"][-1]) <= rc.TOL_T64 * abs(case["t_bound"])


# ------------------------------------------------------------------------------------------------------ g. status -3
@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_rows_in_a_chunked_block(dtype):
    """NaN / +inf / -inf starts in a block whose field evaluations hold barriers: status -3 and NaN outputs for those rows,
    the bits of the clean call for every other row (the lane keeps taking the barriers on a harmless point)."""
    case = rc.count_case(dtype, rc.CAP[dtype] + 1)
    starts, idx = _tile(case, 300)
    bad = starts.copy()
    for i, (lane, v) in enumerate(zip(rc.BAD_LANES, [np.nan, np.inf, -np.inf] * 2)):
        bad[lane, i % 3] = v
    lanes = np.array(rc.BAD_LANES)
    ok = np.setdiff1d(np.arange(300), lanes)
    for sampling in rc.SAMPLINGS:
        clean = _run(dtype, case, starts, 12, sampling)
        t, x, stats = _run(dtype, case, bad, 12, sampling)
        assert (stats[lanes, 3] == -3).all() and np.isnan(t[lanes]).all() and np.isnan(x[lanes]).all()
        assert (clean[2][:, 3] == 0).all()
        assert _all_same_bits([t[ok], x[ok], stats[ok]], [a[ok] for a in clean])
        _check_rows_repeat([a[ok] for a in (t, x, stats)], idx[ok])


# ------------------------------------------------------------------------------------------------------ h. max_step, world
@pytest.mark.parametrize("dtype", DTYPES)
def test_infinite_max_step_and_a_negative_world_scale(dtype):
    free = rc.free_case(dtype)
    assert np.isinf(free["max_step"])
    for sampling in rc.SAMPLINGS:
        _check_scipy(dtype, "max_step = inf", free, _run(dtype, free, None, 40, sampling), 40, sampling)
    for case in rc.world_cases(dtype):
        d = case["d"]
        assert (case["scale"] == rc.WORLD_SCALE).all() and case["scale"][1] < 0 and case["offset"][:d].all() and not case["offset"][d:].any()
        for sampling in rc.SAMPLINGS:
            out = _run(dtype, case, None, 40, sampling)
            np.testing.assert_array_equal(out[1][:, 0, :d], rc.world_starts(case))
            _check_scipy(dtype, "world map", case, out, 40, sampling)


# ------------------------------------------------------------------------------------------------------ i. guards
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("chunked", [False, True], ids=["one stage", "chunked"])
def test_writes_nothing_around_its_buffers(dtype, n, chunked):
    """The C entry point with caller-owned t, traj and stats, each between two sentinel regions: the 255 dead lanes of the
    last block write nothing, the live rows are written completely."""
    from spateo_amd import _lib

    case = rc.count_case(dtype, rc.CAP[dtype] + 1) if chunked else rc.lane_case(dtype)
    starts, _ = _tile(case, n)
    k, x4, c4, Cd, code = _inputs(dtype, case, starts)
    for sampling, n_out in (("uniform_time", 9), ("arc_length", 2)):
        want = _run(dtype, case, starts, n_out, sampling)
        tb, xb, sb = _Out(n * n_out), _Out(3 * n * n_out), _Out(4 * n, dtype=torch.int32)  # t, traj: float64 in both cell dtypes
        w = (ctypes.c_double * 6)(*case["scale"], *case["offset"])
        _lib.check(k.lib.mvf_integrate_rk45(x4.data_ptr(), n, c4.data_ptr(), c4.shape[0], float(case["beta"]), Cd.data_ptr(),
                                            k._affine_buf(case["affine"]), case["d"], w, case["t_bound"], rc.RTOL, rc.ATOL,
                                            case["max_step"], MAX_STEPS, code[sampling], n_out, tb.ptr, xb.ptr, sb.ptr,
                                            k.cdtype, k._stream()), "mvf_integrate_rk45")
        torch.cuda.synchronize()
        for o, ref in ((tb, want[0]), (xb, want[1]), (sb, want[2])):
            assert o.guards_intact()
            got = o.host()
            assert not (got == o.sent).any()
            assert np.array_equal(_bits(got), _bits(ref.reshape(-1)))


CONVENTION_COVERS = {"mvf_integrate_rk45": MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("chunked", [False, True], ids=["one stage", "chunked"])
def test_calling_conventions(dtype, chunked, mode):
    """Times, trajectories and statistics of 257 starts: the plain call's bits on a side stream behind poisoned inputs, at
    displaced pointers, and with the inputs unchanged."""
    from spateo_amd import _lib

    case = rc.count_case(dtype, rc.CAP[dtype] + 1) if chunked else rc.lane_case(dtype)
    (starts, _), k, n, n_out = _tile(case, 257), _k(dtype), 257, 9
    w = (ctypes.c_double * 6)(*case["scale"], *case["offset"])

    def call():
        x4, c4 = _sx4(np.asarray(starts).reshape(-1, 3), dtype), _sx4(np.asarray(case["ctrl"]).reshape(-1, 3), dtype)
        Cd = _dev(np.ascontiguousarray(case["C"], dtype=np.float64).reshape(-1, 3))
        tb, xb, sb = _Out(n * n_out), _Out(3 * n * n_out), _Out(4 * n, dtype=torch.int32)
        _lib.check(k.lib.mvf_integrate_rk45(x4.data_ptr(), n, c4.data_ptr(), c4.shape[0], float(case["beta"]), Cd.data_ptr(),
                                            k._affine_buf(case["affine"]), case["d"], w, case["t_bound"], rc.RTOL, rc.ATOL,
                                            case["max_step"], MAX_STEPS, _lib.RK45_UNIFORM_TIME, n_out, tb.ptr, xb.ptr, sb.ptr,
                                            k.cdtype, k._stream()), "mvf_integrate_rk45")
        _called()
        torch.cuda.synchronize()
        assert tb.guards_intact() and xb.guards_intact() and sb.guards_intact()
        return tb.host(), xb.host(), sb.host()

    plain, got = _under(mode, call)
    assert all(same_bits(a, b) for a, b in zip(plain, got))
