"""No GPU: the references and the input designs of tests/test_gpu_highd_kernels.py, on exactly the inputs that module runs
(tests/_highd_cases.py builds them for both).

  * the float64 call of ``eval_d_reference`` / ``conk_reference`` (the restatement the GPU module compares the kernels with)
    against the 80-bit np.longdouble call: <= 1e-12 on the scale the GPU module uses (each quantity's maximum; curvature with
    m <= 5 control points on ``curv_scale``), two digits below the tightest tolerance asserted there (1e-10);
  * conditioning: |v| and |a| bounded away from 0 relative to their maxima, and from 16 control points on no query whose
    curvature towers over the rest - a max-norm relative error over ALL queries is meaningful, nothing has to be masked;
  * mutation sensitivity: the last control point dropped, the last point of the first 64-point staging chunk dropped, the
    last query repeating its neighbour, the Jacobian transposed, the W column off by one - each moves a compared quantity by
    >= 1000 float32 tolerances;
  * coverage: the grid and the sweep reach every (D, NCT) instantiation ``launch_eval_d`` dispatches to, the column counts
    that fill their last tile exactly, and every n and m of the shape lists at least twice."""
import numpy as np
import pytest

import _highd_cases as hc

L = np.longdouble
REF_TOL = 1e-12

GRID_CASES = [(*hc.HD_GRID_SHAPE, d, dy, hc.grid_flags(d, dy)) for d, dy in hc.HD_GRID]
SWEEP_CASES = [(n, m, d, dy, flags) for d, dy, flags in hc.HD_SWEEP_DIMS for n, m in hc.HD_SWEEP]


@pytest.mark.parametrize("n,m,d,dy,flags", GRID_CASES + SWEEP_CASES)
def test_evaluator_restatement_conditioning_and_mutations(n, m, d, dy, flags):
    case = hc.eval_case(n, m, d, dy)
    assert case["X"].shape == (n, d) and case["ctrl"].shape == (m, d) and case["C"].shape == (m, dy) and (case["C"] > 0).all()
    ref = hc.eval_d_reference(np.float64, case["X"], case["ctrl"], case["C"], case["beta"], flags)
    hp = hc.eval_d_reference(L, case["X"], case["ctrl"], case["C"], case["beta"], flags)
    assert set(ref) == set(hp) == {f for f in hc.HD_FLAGS if flags & f}
    for f, e in hc.eval_errors(ref, hp, m).items():
        assert e <= REF_TOL, (hc.HD_NAMES[f], e)
    vn = np.linalg.norm(ref[hc.EVAL_V], axis=1)
    assert vn.min() / vn.max() >= 0.03
    if flags & hc.EVAL_ACC:
        an = np.linalg.norm(ref[hc.EVAL_ACC], axis=1)
        assert an.min() / an.max() >= 5e-3
    if flags & hc.EVAL_CURV:
        qn = np.linalg.norm(ref[hc.EVAL_CURV], axis=1)
        assert np.isfinite(qn).all()
        if m >= 16:
            assert qn.max() <= 20 * np.median(qn)
        else:
            assert m <= hc.FEW  # (nothing between: curv_scale is what the curvature of these shapes is compared on)
    muts = {name: hc.eval_d_reference(np.float64, mc["X"], mc["ctrl"], mc["C"], mc["beta"], flags)
            for name, mc in hc.input_mutations(case).items()}
    if n >= 2:
        muts["dup_last_query"] = hc.dup_last_query(ref)
    if flags & hc.EVAL_JAC:
        muts["shift_w_column"] = hc.shift_w_column(ref)
        if dy == d:
            muts["swap_jac_axes"] = hc.swap_jac_axes(ref)
    assert ("drop_last_ctrl" in muts) and (("drop_chunk_end" in muts) == (m > hc.HD_CHUNK))
    for name, mut in muts.items():
        # (a mutated curvature is compared on the true reference's scale, as the device's would be)
        moved = max(e / hc.TOL["float32"] for e in hc.eval_errors(mut, ref, m).values())
        assert moved >= hc.MUTATION_FACTOR, (name, moved)


@pytest.mark.parametrize("d", hc.CONK_DS)
def test_conk_reference_in_float64_is_the_longdouble_one(d):
    for n, m in hc.CONK_SHAPES:
        x, y = hc.conk_case(n, m, d)
        K = hc.conk_reference(np.float64, x, y, hc.UBLK_BETA)
        assert K.shape == (n, m) and np.abs(K - hc.conk_reference(L, x, y, hc.UBLK_BETA)).max() <= REF_TOL
        if n * m >= 1000:  # most values are far from underflow
            assert np.median(K) > 1e-6


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("d", hc.UBLK_FAR_DS)
def test_underflow_case_of_the_cache_has_normals_denormals_and_zeros(d, dtype):
    npdt = np.float32 if dtype == "float32" else np.float64
    x, y = hc.conk_case(*hc.UBLK_FAR_SHAPE, d, far=hc.UBLK_FAR[dtype])
    K = hc.conk_reference(L, x.astype(npdt), y.astype(npdt), hc.UBLK_BETA)
    tiny, least = L(np.finfo(npdt).tiny), L(np.finfo(npdt).smallest_subnormal)
    for part in (K > 4 * tiny, (K < tiny / 4) & (K > 4 * least), K < least / 4):
        assert part.mean() >= 0.05


def test_cases_cover_what_they_claim():
    reached = {(d, hc.nct(d, dy, hc.grid_flags(d, dy))) for d, dy in hc.HD_GRID}
    reached |= {(d, hc.nct(d, dy, flags)) for d, dy, flags in hc.HD_SWEEP_DIMS}
    # the dispatcher of launch_eval_d: NCT 1 .. 3 at every d, 4 from d = 6, 5 at d = 8
    want = {(d, t) for d in range(4, 9) for t in (1, 2, 3)} | {(d, 4) for d in (6, 7, 8)} | {(8, 5)}
    assert reached == want
    assert [hc.nct(*e) for e in hc.HD_SWEEP_DIMS] == [2, 4, 5, 1]
    full = {hc.ncols(d, dy, hc.grid_flags(d, dy)) for d, dy in hc.HD_GRID}
    assert {16, 32, 48, 64} <= full
    assert {(d, dy) for d, dy in hc.HD_GRID if hc.ncols(d, dy, hc.EVAL_JAC) % 16 == 0} == {(7, 2), (7, 4), (5, 8), (7, 6), (7, 8)}
    assert len(hc.HD_GRID) == 40 and any(dy != d for d, dy in hc.HD_GRID)
    assert {n for n, _ in hc.HD_SWEEP} == set(hc.HD_NS) and {m for _, m in hc.HD_SWEEP} == set(hc.HD_MS)
    for n in hc.HD_NS:
        assert sum(1 for a, _ in hc.HD_SWEEP if a == n) >= 2
    for m in hc.HD_MS:
        assert sum(1 for _, b in hc.HD_SWEEP if b == m) >= 2
    assert {m % 4 for _, m in hc.HD_SWEEP if m > hc.HD_CHUNK} >= {1, 2, 3}
    # cache shapes: one, two and three block columns of 512 control points, the last one short
    assert {-(-(-(-m // 128) * 128) // 512) for _, m in hc.UBLK_SHAPES} == {1, 2, 3}
