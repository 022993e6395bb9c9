"""``spateo_amd.align.morpho_iterate`` on ``cuda:0`` against tests/golden/ref_align_loop.npz: the real reference methods run
for 12 iterations on four cases (tests/golden/make_golden_align_loop.py), in both cell dtypes, per iteration and per
quantity, relative to the quantity's maximum.

* float64: ``1e-10 max(1, 1.25 g_k)`` - 1e-10 is the assignment step's own bound (tests/test_gpu_assign.py), g_k the
  amplification the maker measured on the reference with its perturbed twin;
* float32: ``max(1.25 x the reference's own float32 floor, 1e-5 max(1, 1.25 g_k))``; ``Coff`` is asserted in float64 only
  (the reference's own float32 ``Coff`` is off by 0.9: ``pinv`` leaves it poorly determined) - in float32 the field is
  asserted through ``VnA`` and ``XAHat``.

Also: two calls give equal bits in everything returned; with ``max_iter=1`` the returned ``K_NA``, ``K_NB``, ``K_NA_spatial``,
``K_NA_sigma2`` equal ``update_assignment``'s on the initial state bit for bit (the same kernel on the same operands);
``BA_transform(vecfld, coordsA)`` reproduces ``XAHat`` and ``optimal_RnA``.  Run with ``-s`` for the worst ratio per quantity."""
import numpy as np
import pytest

import _align_loop_case as lc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = lc.load()
TAGS = lc.case_tags(G)
_RUNS, _WORST = {}, {}


def _run(tag, dtype):
    if (tag, dtype) not in _RUNS:
        from spateo_amd import align

        args, kw = lc.case_inputs(G, tag)
        _RUNS[(tag, dtype)] = align.morpho_iterate(*args, dtype=dtype, device=DEV, record="arrays", **kw)
    return _RUNS[(tag, dtype)]


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    yield
    print("\n| quantity | dtype | worst deviation / bound |\n|---|---|---|")
    for (q, dtype), v in sorted(_WORST.items()):
        print(f"| {q} | {dtype} | {v:.3g} |")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tag", TAGS)
def test_loop_against_the_reference(tag, dtype):
    out = _run(tag, dtype)
    got = dict(out["history"], optimal_R=out["optimal_R"], optimal_t=out["optimal_t"])
    dev = lc.deviations(got, G, tag)
    f32 = dtype == "float32"
    tol = lc.bounds(G, tag, lc.F32_BASE if f32 else lc.F64_TOL, f32=f32, skip=("Coff",) if f32 else ())
    try:
        ratio = lc.check(dev, tol, f"case {tag} {dtype}")
    finally:
        for q in tol:
            _WORST[(q, dtype)] = max(_WORST.get((q, dtype), 0.0), float((dev[q] / tol[q]).max()))
    assert max(ratio.values()) <= 1.0
    # the state returned is the last iteration's
    assert np.array_equal(out["XAHat"], out["history"]["XAHat"][-1]) and out["sigma2"] == out["history"]["sigma2"][-1]
    assert abs(out["sigma2_variance"] - float(G[f"{tag}_sigma2_variance"])) <= 1e-12 * out["sigma2_variance"]


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


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_two_calls_give_equal_bits(dtype):
    from spateo_amd import align

    args, kw = lc.case_inputs(G, "2")
    kw.update(max_iter=6)
    a = align.morpho_iterate(*args, dtype=dtype, device=DEV, **kw)
    b = align.morpho_iterate(*args, dtype=dtype, device=DEV, **kw)
    assert set(a) >= {"R", "t", "Coff", "VnA", "RnA", "XAHat", "optimal_R", "optimal_t", "optimal_RnA", "sigma2", "gamma", "alpha",
                      "SigmaDiag", "sigma2_variance", "K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2", "Sp", "Sp_spatial",
                      "Sp_sigma2", "history", "vecfld"}
    assert set(a["history"]) == {"sigma2", "gamma", "R", "t", "Sp"} and len(a["history"]["Sp"]) == 6
    _equal(a, b)
    assert "history" not in align.morpho_iterate(*args, dtype=dtype, device=DEV, record=False, **dict(kw, max_iter=1))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tag", ["2", "3"])
def test_first_assignment_is_update_assignment_bit_for_bit(tag, dtype):
    from spateo_amd import align

    args, kw = lc.case_inputs(G, tag)
    one = align.morpho_iterate(*args, dtype=dtype, device=DEV, **dict(kw, max_iter=1))
    NA = len(args[0])
    ref = align.update_assignment(*args, dissimilarity=kw["dissimilarity"], probability_type=kw["probability_type"],
                                  probability_parameters=kw["probability_parameters"], sigma2=kw["sigma2"], alpha=np.ones(NA),
                                  SigmaDiag=np.zeros(NA), gamma=0.5, samples_s=kw["samples_s"], sigma2_variance=1.0, dtype=dtype,
                                  device=DEV)
    for q in ("K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2"):
        assert np.array_equal(one[q].view(np.int64), ref[q].view(np.int64)), q


@pytest.mark.parametrize("tag", ["1", "3", "4"])
def test_vecfld_feeds_BA_transform(tag):
    from spateo_amd import align

    out = _run(tag, "float64")
    coordsA = lc.case_inputs(G, tag)[0][0]
    hat, vel, opt = align.BA_transform(out["vecfld"], coordsA, dtype="float64", device=DEV)
    tol = lc.bounds(G, tag, lc.F64_TOL)
    d_hat = np.abs(hat - out["XAHat"]).max() / np.abs(out["XAHat"]).max()
    d_opt = np.abs(opt - out["optimal_RnA"]).max() / np.abs(out["optimal_RnA"]).max()
    d_vel = np.abs(vel - out["VnA"]).max() / np.abs(out["VnA"]).max()
    print(f"  case {tag}: BA_transform vs morpho_iterate: XAHat {d_hat:.2e}, optimal_RnA {d_opt:.2e}, VnA {d_vel:.2e}")
    assert d_hat <= tol["XAHat"][-1] and d_opt <= tol["optimal_t"][-1] and d_vel <= tol["VnA"][-1]
