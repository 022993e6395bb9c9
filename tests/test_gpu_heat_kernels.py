"""GPU: ``mvf_heat_grid`` / ``mvf_heat_graph`` through the raw C ABI against the restatements of tests/_heat_cases.py (which
tests/test_heat_kernel_refs.py pins to the real reference functions on the CPU).

Grid: for every case and every dispatch (one sweep per launch, T sweeps per launch, the library's choice) the field is bit-equal
to the restatement and the sweep count equal; err within 1e-12 (relative) or NaN on both sides - the kernels add the error sums
in another order than NumPy, which is why every case is decidable.  The blocked kernel at every ``steps`` in 1 .. T is bit-equal
to ``steps`` one-sweep launches.  Two calls give equal bits.  Graph: the same checks.  Outputs and workspaces are guarded."""
import ctypes

import numpy as np
import pytest

import _heat_cases as hc
from _kernel_scaffold import MODES, Out, Ws, called, dev, same_bits, stream, under

pytestmark = pytest.mark.gpu
ERR_RTOL = 1e-12


def lib():
    from spateo_amd import _lib

    return _lib.load()


def check(rc):
    from spateo_amd import _lib

    _lib.check(rc, "mvf_heat")


def run_grid(init, border, mask, max_err, max_itr, block):
    H, W = init.shape
    di, db, dm = dev(init), dev(border), dev(mask)
    out, ws = Out(H, W), Ws(lib().mvf_heat_grid_workspace_bytes(H, W))
    sweeps, err, hit = ctypes.c_int64(-1), ctypes.c_double(-1.0), ctypes.c_int(-1)
    check(lib().mvf_heat_grid(di.data_ptr(), db.data_ptr(), dm.data_ptr(), H, W, float(max_err), float(max_itr), block, out.ptr,
                              ctypes.byref(sweeps), ctypes.byref(err), ctypes.byref(hit), ws.ptr, ws.nbytes, stream()))
    called()
    assert out.guards_intact() and ws.guards_intact()
    return out.host(), sweeps.value, err.value, hit.value


def run_grid_case(case, block, **over):
    c = dict(case, **over)
    return run_grid(hc.grid_init(c), c["border"], c["mask"], c["max_err"], c["max_itr"], block)


def close_or_both_nan(a, b):
    if np.isnan(a) or np.isnan(b):
        return np.isnan(a) and np.isnan(b)
    return abs(a - b) <= ERR_RTOL * abs(b)


@pytest.mark.parametrize("name", hc.GRID_NAMES)
def test_grid_case_meets_the_restatement_bit_for_bit(name):
    case = hc.grid_case(name)
    ref, itr, errs = hc.grid_reference(name)
    want_err = errs[-1] if errs else 1.0
    for block in (1, hc.T, 0):
        got, sweeps, err, hit = run_grid_case(case, block)
        print(f"{name} block {block}: {sweeps} sweeps (restatement {itr}), err {err!r} (restatement {want_err!r})")
        assert sweeps == itr, (block, sweeps, itr)
        assert same_bits(got, np.asarray(ref)), block
        assert close_or_both_nan(err, want_err), (block, err, want_err)
        assert hit == int(want_err > case["max_err"]), block


@pytest.mark.parametrize("name", ("edge_41x73", "open_border", "edge_32x64"))
def test_blocked_kernel_equals_one_sweep_launches_at_every_steps(name):
    case = hc.grid_case(name)
    for steps in range(1, hc.T + 1):
        f, itr, _ = hc.grid_loop(case, max_sweeps=steps)
        assert itr == steps
        blocked = run_grid_case(case, steps, max_itr=steps - 1)
        single = run_grid_case(case, 1, max_itr=steps - 1)
        assert blocked[1] == single[1] == steps and blocked[3] == single[3] == 1
        assert same_bits(blocked[0], single[0]) and same_bits(blocked[0], f * case["mask"]), steps
        assert blocked[2] == single[2]        # the same partial sums in the same order: the same err, bit for bit
    # the host's repeat of the stopping batch: T sweeps per launch, the budget ends inside the second batch
    for sweeps in (hc.T + 1, hc.T + 3, 2 * hc.T - 1):
        f, _, _ = hc.grid_loop(case, max_sweeps=sweeps)
        assert same_bits(run_grid_case(case, 3, max_itr=sweeps - 1)[0], f * case["mask"])
        assert same_bits(run_grid_case(case, hc.T, max_itr=sweeps - 1)[0], f * case["mask"])


def test_grid_two_calls_give_equal_bits():
    case = hc.grid_case("edge_41x73")
    a, b = run_grid_case(case, 0), run_grid_case(case, 0)
    assert same_bits(a[0], b[0]) and a[1:] == b[1:]
    a, b = run_grid_case(case, hc.T, max_err=1e-3), run_grid_case(case, hc.T, max_err=1e-3)
    assert same_bits(a[0], b[0]) and a[1:] == b[1:]


def test_grid_refusals_on_real_buffers_leave_the_output_alone():
    case = hc.grid_case("rect_12x15")
    init = hc.grid_init(case)
    di, db, dm = dev(init), dev(case["border"]), dev(case["mask"])
    out, need = Out(12, 15), lib().mvf_heat_grid_workspace_bytes(12, 15)
    ws = Ws(need)
    sweeps, err, hit = ctypes.c_int64(-1), ctypes.c_double(-1.0), ctypes.c_int(-1)
    for H, W, block, nbytes in ((2, 15, 0, need), (12, 15, hc.T + 1, need), (12, 15, 0, need - 8)):
        rc = lib().mvf_heat_grid(di.data_ptr(), db.data_ptr(), dm.data_ptr(), H, W, 1e-20, 1e6, block, out.ptr, ctypes.byref(sweeps),
                                 ctypes.byref(err), ctypes.byref(hit), ws.ptr, nbytes, stream())
        assert rc != 0 and b"mvf_heat_grid" in lib().mvf_last_error()
    assert out.untouched() and out.guards_intact() and sweeps.value == -1


# --------------------------------------------------------------------------------------------------------------- graph
def run_graph(case):
    indptr, indices, data = hc.graph_csc(case)
    fv = hc.graph_fixed_value(case)
    n = len(fv)
    out, ws = Out(n), Ws(lib().mvf_heat_graph_workspace_bytes(n, len(data)))
    sweeps, err, hit = ctypes.c_int64(-1), ctypes.c_double(-1.0), ctypes.c_int(-1)
    hp = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    check(lib().mvf_heat_graph(hp(indptr), hp(indices), hp(data), hp(fv), n, float(case["max_err"]), float(case["max_itr"]), out.ptr,
                               ctypes.byref(sweeps), ctypes.byref(err), ctypes.byref(hit), ws.ptr, ws.nbytes, stream()))
    called()
    assert out.guards_intact() and ws.guards_intact()
    return out.host(), sweeps.value, err.value, hit.value


# ------------------------------------------------------------------------------------------------- calling conventions
CONVENTION_COVERS = {"mvf_heat_grid": MODES, "mvf_heat_graph": MODES}


def _same(a, b):
    return same_bits(a[0], b[0]) and a[1] == b[1] and a[3] == b[3] and (a[2] == b[2] or (np.isnan(a[2]) and np.isnan(b[2])))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("block", (1, hc.T), ids=("one-sweep", "blocked"))
def test_grid_calling_conventions(block, mode):
    """The plain call's field, sweep count and err on a side stream behind poisoned inputs, at displaced pointers, and with the
    inputs unchanged.  Both heat entries block (include/mvf.h): the side stream protects the launches of the first batch."""
    plain, got = under(mode, lambda: run_grid_case(hc.grid_case("rect_12x15"), block), synchronising=True)
    assert _same(plain, got)


@pytest.mark.parametrize("mode", MODES)
def test_graph_calling_conventions(mode):
    """As for the grid; the graph's arrays are host arrays, which the entry copies into its workspace on the stream."""
    plain, got = under(mode, lambda: run_graph(hc.graph_case("n63")), synchronising=True)
    assert _same(plain, got)


@pytest.mark.parametrize("name", hc.GRAPH_NAMES)
def test_graph_case_meets_the_restatement_bit_for_bit(name):
    case = hc.graph_case(name)
    ref, itr, errs = hc.graph_reference(name)
    got, sweeps, err, hit = run_graph(case)
    print(f"{name}: {sweeps} sweeps (restatement {itr}), err {err!r} (restatement {errs[-1]!r})")
    assert sweeps == itr
    assert same_bits(got, np.asarray(ref))
    assert close_or_both_nan(err, errs[-1])
    assert hit == int(errs[-1] > case["max_err"])
    again = run_graph(case)
    assert same_bits(again[0], got) and again[1] == sweeps and (again[2] == err or (np.isnan(err) and np.isnan(again[2])))


def test_graph_zero_sweeps_and_refusal():
    case = dict(hc.graph_case("n63"), max_itr=-1)
    got, sweeps, err, hit = run_graph(case)
    assert sweeps == 0 and err == 1.0 and hit == 1 and same_bits(got, hc.graph_fixed_value(case))
    indptr, indices, data = hc.graph_csc(case)
    bad = indices.copy()
    bad[7] = 63
    fv = hc.graph_fixed_value(case)
    out, ws = Out(63), Ws(lib().mvf_heat_graph_workspace_bytes(63, len(data)))
    s, e, h = ctypes.c_int64(-1), ctypes.c_double(-1.0), ctypes.c_int(-1)
    rc = lib().mvf_heat_graph(indptr.ctypes.data, bad.ctypes.data, data.ctypes.data, fv.ctypes.data, 63, 1e-5, 1e6, out.ptr,
                              ctypes.byref(s), ctypes.byref(e), ctypes.byref(h), ws.ptr, ws.nbytes, stream())
    assert rc != 0 and b"index out of range" in lib().mvf_last_error() and out.untouched() and s.value == -1
