"""``spateo_amd.align.morpho_iterate_svi`` on ``cuda:0`` against tests/golden/ref_align_svi.npz: the real reference methods
with ``SVI_mode=True`` run for 30 iterations of 150-cell batches on cases 1 - 3 of the dense fixture and on case 3 with a late
non-rigid start (tests/golden/make_golden_align_svi.py), in both cell dtypes, per iteration and per quantity, relative to the
quantity's maximum, with the dense loop's rule (tests/test_gpu_align_loop.py):

* float64: ``1e-10 max(1, 1.25 g_k)``;
* float32: ``max(1.25 x the reference's own float32 floor, 1e-5 max(1, 1.25 g_k))``, ``Coff`` asserted in float64 only.  On
  case 1 this float32 bound is WEAK and is left so: the reference's own float32 twin is poor there - its sigma2 is off by
  1.1e-2 relative once it reaches the 1e-2 floor, its ``VnA`` by 0.12 and its ``Coff`` by 0.9 - so the floor, not the
  1e-5 term, sets the bound on that case.

Also: ``return_mapping=True`` against its stored ``optimal_R`` / ``optimal_t`` / ``Sp`` with ``K_NB`` of the whole B slice; two
calls give equal bits in everything returned; with ``batch_size = NB``, the identity permutation and 8 iterations (every step
1) the result agrees with ``morpho_iterate`` within the float64 bound of the dense fixture (the gather and the unit-weight
right-hand side against the dense path); a small ``origin`` agrees with ``origin=None``; ``BA_transform(vecfld, coordsA)``
reproduces ``XAHat`` and ``optimal_RnA``.  Run with ``-s`` for the worst ratio per quantity."""
import numpy as np
import pytest

import _align_loop_case as lc
import _align_svi_case as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = sc.load()
TAGS = sc.case_tags(G)
_RUNS, _WORST = {}, {}


def _run(tag, dtype, return_mapping=False):
    key = (tag, dtype, return_mapping)
    if key not in _RUNS:
        from spateo_amd import align

        args, kw = sc.case_inputs(G, tag)
        _RUNS[key] = align.morpho_iterate_svi(*args, dtype=dtype, device=DEV, record="arrays", return_mapping=return_mapping, **kw)
    return _RUNS[key]


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    yield
    print("\n| quantity | dtype | worst deviation / bound |\n|---|---|---|")
    for (q, dtype), v in sorted(_WORST.items()):
        print(f"| {q} | {dtype} | {v:.3g} |")


def _checked(dev, tol, what, dtype):
    try:
        ratio = sc.check(dev, tol, what)
    finally:
        for q in tol:
            _WORST[(q, dtype)] = max(_WORST.get((q, dtype), 0.0), float((dev[q] / tol[q]).max()))
    assert max(ratio.values()) <= 1.0


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tag", TAGS)
def test_svi_loop_against_the_reference(tag, dtype):
    out = _run(tag, dtype)
    got = dict(out["history"], optimal_R=out["optimal_R"], optimal_t=out["optimal_t"])
    f32 = dtype == "float32"
    tol = sc.bounds(G, tag, sc.F32_BASE if f32 else sc.F64_TOL, f32=f32, skip=("Coff",) if f32 else ())
    _checked(sc.deviations(got, G, tag), tol, f"case {tag} {dtype}", dtype)
    bs, iters = int(G["batch_size"]), int(G["iters"])
    np.testing.assert_array_equal(out["history"]["step_size"], G[f"{tag}_step_size"])
    assert out["batch_size"] == bs and out["step_size"] == 1.0 / 3.0 and len(out["K_NB"]) == bs
    np.testing.assert_array_equal(out["batch_perm"], G[f"{tag}_batch_perm"])
    assert np.array_equal(out["XAHat"], out["history"]["XAHat"][-1]) and out["sigma2"] == out["history"]["sigma2"][-1]
    assert out["Sp"] == out["history"]["Sp"][-1] and len(out["history"]["Sp"]) == iters
    # K_NB belongs to the last batch: its sum is that batch's unblended Sp, which the running value is not
    assert abs(out["K_NB"].sum() - out["K_NA"].sum()) <= 1e-9 * out["K_NA"].sum() and out["K_NB"].sum() != out["Sp"]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tag", TAGS)
def test_return_mapping_against_the_reference(tag, dtype):
    out = _run(tag, dtype, return_mapping=True)
    NB = len(G[f"{tag}_batch_perm"])
    assert len(out["K_NB"]) == NB and len(out["K_NA"]) == len(out["XAHat"])
    assert abs(out["K_NB"].sum() - out["Sp"]) <= 1e-12 * out["Sp"]      # the unblended Sp of the whole slice
    got = dict(optimal_R_map=out["optimal_R"], optimal_t_map=out["optimal_t"], Sp_map=out["Sp"])
    f32 = dtype == "float32"
    tol = sc.bounds(G, tag, sc.F32_BASE if f32 else sc.F64_TOL, f32=f32, finals=sc.FINALS_MAP)
    tol = {q: tol[q] for q in sc.FINALS_MAP}
    dev = {q: lc.rel(np.asarray(got[q], dtype=np.float64)[None], G[f"{tag}_{q}"][None]) for q in sc.FINALS_MAP}
    _checked(dev, tol, f"case {tag} {dtype} return_mapping", dtype)
    # the loop itself does not depend on return_mapping
    plain = _run(tag, dtype)
    for q in ("R", "t", "XAHat", "Coff", "alpha"):
        assert np.array_equal(out[q], plain[q]), q
    assert out["sigma2"] == plain["sigma2"]


def _equal(a, b, path=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for key in a:
            _equal(a[key], b[key], f"{path}/{key}")
    elif isinstance(a, np.ndarray) and a.dtype.kind == "f":
        assert a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)), path
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    else:
        assert a == b or (a is None and b is None), path


@pytest.mark.parametrize("return_mapping", [False, True])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_two_calls_give_equal_bits(dtype, return_mapping):
    from spateo_amd import align

    args, kw = sc.case_inputs(G, "2")
    kw.update(max_iter=14, return_mapping=return_mapping, sigma2_end=0.02)    # steps below 1 included
    a = align.morpho_iterate_svi(*args, dtype=dtype, device=DEV, **kw)
    b = align.morpho_iterate_svi(*args, dtype=dtype, device=DEV, **kw)
    assert set(a) >= {"R", "t", "Coff", "VnA", "RnA", "XAHat", "optimal_R", "optimal_t", "optimal_RnA", "sigma2", "gamma", "alpha",
                      "SigmaDiag", "sigma2_variance", "K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2", "Sp", "Sp_spatial",
                      "Sp_sigma2", "history", "vecfld", "batch_size", "batch_perm", "step_size"}
    assert set(a["history"]) == {"sigma2", "gamma", "R", "t", "Sp", "step_size"} and len(a["history"]["Sp"]) == 14
    assert a["sigma2"] == 0.02 and a["step_size"] == 10.0 / 14.0
    _equal(a, b)


def test_seeded_permutation_is_reproducible():
    from spateo_amd import align

    args, kw = sc.case_inputs(G, "3")
    kw.update(max_iter=2, batch_perm=None, record=False)
    a = align.morpho_iterate_svi(*args, device=DEV, seed=11, **kw)
    NB = len(args[1])
    np.testing.assert_array_equal(a["batch_perm"], np.random.default_rng(11).permutation(NB))
    assert "history" not in a
    b = align.morpho_iterate_svi(*args, device=DEV, **dict(kw, batch_perm=a["batch_perm"]))
    assert np.array_equal(a["XAHat"], b["XAHat"])


@pytest.mark.parametrize("tag", ["1", "2", "3"])
def test_full_batches_agree_with_the_dense_loop(tag):
    """batch_size = NB, batch_perm = arange(NB), 8 iterations: every step is 1 and every batch the whole slice in its own
    order, so the SVI loop computes what morpho_iterate computes - through the gathered buffers and the unit-weight
    right-hand side.  Bound: the dense fixture's float64 bound at its iteration 7 (both sides are this product)."""
    from spateo_amd import align

    D = lc.load()
    args, kw = lc.case_inputs(D, tag)
    kw.update(max_iter=8)
    NB = len(args[1])
    dense = align.morpho_iterate(*args, device=DEV, **kw)
    svi = align.morpho_iterate_svi(*args, device=DEV, batch_size=NB, batch_perm=np.arange(NB), **kw)
    assert np.all(svi["history"]["step_size"] == 1.0) and len(svi["K_NB"]) == NB
    tol = lc.bounds(D, tag, lc.F64_TOL)
    at = {q: float(tol[q][7]) for q in lc.SCALARS}
    at.update({q: float(tol[q][2]) for q in lc.ARRAYS})        # the stored iteration 7 of the arrays
    at.update({q: float(tol[q][0]) for q in lc.FINALS})
    worst = {}
    for q in lc.SCALARS:
        worst[q] = float(lc.rel(svi["history"][q], dense["history"][q]).max())
    for q in ("alpha", "XAHat", "VnA", "K_NA", "Coff", "optimal_R", "optimal_t"):
        worst[q] = float(lc.rel(svi[q][None], dense[q][None])[0])
    worst["K_NB"] = float(lc.rel(svi["K_NB"][None], dense["K_NB"][None])[0])
    at["K_NB"] = at["K_NA"]
    print(f"  case {tag}: SVI with full batches vs the dense loop: " + ", ".join(f"{q} {v:.2e}" for q, v in worst.items()))
    for q, v in worst.items():
        assert v <= at[q], (q, v, at[q])


@pytest.mark.parametrize("tag", ["1", "3"])
def test_small_origin_agrees_with_none(tag):
    """origin = mean(coordsB) (order 1 here) only re-centres the assignment's operands: same result within the bound."""
    from spateo_amd import align

    args, kw = sc.case_inputs(G, tag)
    plain = _run(tag, "float64")
    moved = align.morpho_iterate_svi(*args, device=DEV, record="arrays", origin=np.asarray(args[1]).mean(0), **kw)
    got = dict(moved["history"], optimal_R=moved["optimal_R"], optimal_t=moved["optimal_t"])
    ref = dict(plain["history"], optimal_R=plain["optimal_R"], optimal_t=plain["optimal_t"])
    tol = sc.bounds(G, tag, sc.F64_TOL)
    arr = [int(i) for i in G["arr_iters"]]
    for q in tol:
        a, b = np.asarray(got[q]), np.asarray(ref[q])
        if q in sc.ARRAYS:
            a, b = a[arr], b[arr]
        elif q in sc.FINALS:
            a, b = a[None], b[None]
        dev = lc.rel(a, b)
        assert np.all(dev <= tol[q]), (q, dev, tol[q])


@pytest.mark.parametrize("tag", ["1", "3n"])
def test_vecfld_feeds_BA_transform(tag):
    from spateo_amd import align

    out = _run(tag, "float64")
    coordsA = sc.case_inputs(G, tag)[0][0]
    hat, vel, opt = align.BA_transform(out["vecfld"], coordsA, dtype="float64", device=DEV)
    tol = sc.bounds(G, tag, sc.F64_TOL)
    d_hat = np.abs(hat - out["XAHat"]).max() / np.abs(out["XAHat"]).max()
    d_opt = np.abs(opt - out["optimal_RnA"]).max() / np.abs(out["optimal_RnA"]).max()
    d_vel = np.abs(vel - out["VnA"]).max() / np.abs(out["VnA"]).max()
    print(f"  case {tag}: BA_transform vs morpho_iterate_svi: XAHat {d_hat:.2e}, optimal_RnA {d_opt:.2e}, VnA {d_vel:.2e}")
    assert d_hat <= tol["XAHat"][-1] and d_opt <= tol["optimal_t"][-1] and d_vel <= tol["VnA"][-1]
