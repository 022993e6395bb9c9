"""No GPU: what tests/test_gpu_eval_wide_kernels.py relies on.  The NumPy reference of the wide evaluator
(tests/_eval_wide_cases.py) equals the oracle's ``vector_field_function`` / ``Jacobian_rkhs_gaussian(vectorize=True)`` for
Dy != D, its Jacobian is the derivative of its values, the float32-operand reference stays within the float32 tolerance of the
float64 one on every case of the sweep (so ONE tolerance, _cell_cases.TOL, serves both cell dtypes), and each targeted one-off
slip moves a compared quantity by at least MUTATION_FACTOR float32 tolerances."""
import numpy as np
import pytest

import _eval_wide_cases as wc
from _cell_cases import EVAL_JAC, EVAL_V, MUTATION_FACTOR, TOL, relmax
from oracle import dg_oracle as dgo
from oracle import sparsevfc_oracle as svo

ORACLE_SHAPES = [(65, 259, 65, 3), (17, 65, 17, 2), (16, 5, 4, 1), (1, 259, 130, 3)]


@pytest.mark.parametrize("n,m,dy,d", ORACLE_SHAPES)
def test_reference_equals_the_oracle_for_wide_fields(n, m, dy, d):
    c = wc.wide_case(n, m, dy, d)
    ref = wc.case_reference(n, m, dy, d, "float64")
    vf = {"X_ctrl": c["ctrl"], "C": c["C"], "beta": c["beta"]}
    v = np.asarray(svo.vector_field_function(c["X"], vf)).reshape(n, dy)
    J = dgo.Jacobian_rkhs_gaussian(c["X"], vf, vectorize=True)
    assert ref[EVAL_V].shape == (n, dy) and ref[EVAL_JAC].shape == (dy, d, n) == np.asarray(J).shape
    assert relmax(ref[EVAL_V], v) <= 1e-12
    assert relmax(ref[EVAL_JAC], J) <= 1e-12


@pytest.mark.parametrize("n,m,dy,d", [(65, 259, 65, 3), (17, 65, 17, 2), (16, 5, 4, 1)])
def test_reference_jacobian_is_the_derivative_of_the_values(n, m, dy, d):
    """Central differences with h = 1e-4: the truncation error h^2 / 6 |v'''| is ~(2 beta)^(3/2) h^2 ~ 1e-11 of |v|, the rounding
    error eps |v| / h ~ 1e-12 |v|; against max |J| ~ 2 beta r |v| with r ~ 10 both stay far below 1e-7."""
    c = wc.wide_case(n, m, dy, d)
    J = wc.case_reference(n, m, dy, d, "float64")[EVAL_JAC]
    h = 1e-4
    for i in range(d):
        e = np.zeros(d)
        e[i] = h
        vp = wc.wide_reference(c["X"] + e, c["ctrl"], c["C"], c["beta"], EVAL_V)[EVAL_V]
        vm = wc.wide_reference(c["X"] - e, c["ctrl"], c["C"], c["beta"], EVAL_V)[EVAL_V]
        fd = ((vp - vm) / (2 * h)).T  # (dy, n)
        assert np.abs(fd - J[:, i, :]).max() <= 1e-7 * np.abs(J).max(), i


@pytest.mark.parametrize("n,m,dy,d", wc.SWEEP)
def test_float32_operands_stay_within_the_float32_tolerance(n, m, dy, d):
    r64, r32 = wc.case_reference(n, m, dy, d, "float64"), wc.case_reference(n, m, dy, d, "float32")
    for f in (EVAL_V, EVAL_JAC):
        assert np.all(np.isfinite(r64[f])) and np.abs(r64[f]).max() > 0
        assert relmax(r32[f], r64[f]) <= TOL["float32"], f


@pytest.mark.parametrize("n,m,dy,d", wc.SWEEP)
def test_every_targeted_slip_is_a_gross_error(n, m, dy, d):
    good, muts = wc.wide_mutations(wc.wide_case(n, m, dy, d))
    want = {"drop_last_ctrl"} | ({"drop_chunk_end"} if m > wc.CHUNK else set()) | ({"shift_column"} if dy > 1 else set()) | \
        ({"shift_query"} if n > 1 else set())
    assert set(muts) == want
    for name, bad in muts.items():
        moved = max(relmax(bad[f], good[f]) for f in (EVAL_V, EVAL_JAC))
        assert moved >= MUTATION_FACTOR * TOL["float32"], (name, moved)


def test_sweep_covers_the_edges_the_kernel_has():
    ns, ms, dys, ds = (sorted({s[i] for s in wc.SWEEP}) for i in range(4))
    assert {1, 15, 16, 17, 63, 64, 65, 255, 256, 257} <= set(ns)
    assert {1, 2, 3, 4, 5, wc.CHUNK - 1, wc.CHUNK, wc.CHUNK + 1, 1023} <= set(ms)
    assert {1, 4, 15, 16, 17, wc.PANEL - 1, wc.PANEL, wc.PANEL + 1, 2 * wc.PANEL + 2} <= set(dys)
    assert ds == [1, 2, 3]
    src = open(__file__.replace("tests/test_eval_wide_refs.py", "spateo-release_amd/csrc/mvf_eval_wide.hip")).read()
    assert f"EW_PANEL = {wc.PANEL};" in src and f"EW_CHUNK = {wc.CHUNK};" in src
