"""CPU proof that the restatement of tests/_kde_cases.py - what the GPU suites compare ``csrc/mvf_kde.hip`` against - is sklearn's
``KernelDensity.score_samples``, and the derivation of the bounds those suites use (printed, recorded in profiles/kde.md):

  * the restatement against sklearn itself where it is installed, and against its recorded output (tests/golden/ref_kde.npz)
    everywhere, for all six kernels, with weights, groups and -inf entries;
  * the normalising constants for d = 1, 2, 3 against sklearn's value at a single point;
  * every compact case decidable: no pair distance within 1e-9 (relative) of the bandwidth;
  * the bound formula: forward against reversed summation, the recorded sklearn deviation, the floor."""
import numpy as np
import pytest

import _kde_cases as kc


@pytest.fixture(scope="module")
def G():
    return kc.load()


def _sklearn_scores(case):
    from sklearn.neighbors import KernelDensity

    T, X, w, g, C = case["T"], case["X"], case["w"], case["g"], case["C"]
    out = np.full((len(T), C), -np.inf)
    for c in range(C):
        sel = np.ones(len(X), dtype=bool) if g is None else g == c
        wc = None if w is None else w[sel]
        if sel.any() and (wc is None or (wc > 0).any()):
            out[:, c] = KernelDensity(kernel=case["kernel"], bandwidth=case["h"]).fit(X[sel], sample_weight=wc).score_samples(T)
    return out


@pytest.mark.parametrize("name", kc.GOLDEN_FULL)
def test_restatement_equals_the_recorded_sklearn_scores(G, name):
    case = kc.CASES[name]
    assert np.array_equal(G[f"{name}_T"], case["T"]) and np.array_equal(G[f"{name}_X"], case["X"])   # the case is the recorded one
    if case["w"] is not None:
        assert np.array_equal(G[f"{name}_w"], case["w"])
    if case["g"] is not None:
        assert np.array_equal(G[f"{name}_g"], case["g"])
    score, ref = G[f"{name}_score"], kc.log_density(case)
    dev = kc.deviation(ref, score, score)          # (asserts the -inf patterns equal)
    assert dev == float(G[f"skdev_{name}"])
    print(f"{name}: |restatement - sklearn| / max(1, |ref|) = {dev:.3e}")
    assert dev < 1e-11 or name in kc.TIGHT


@pytest.mark.parametrize("kernel", kc.KERNELS)
@pytest.mark.parametrize("d", (1, 2, 3))
def test_restatement_equals_sklearn(G, kernel, d):
    pytest.importorskip("sklearn")
    import sklearn

    name = f"{kernel}_d{d}"
    case = kc.CASES[name]
    score, ref = _sklearn_scores(case), kc.log_density(case)
    empty = ~np.isfinite(ref)
    assert (np.isneginf(score[empty]) | (score[empty] < score[~empty].max() - 27.0)).all()   # -inf, or the residue of sklearn's bounds
    score[empty] = -np.inf
    dev = kc.deviation(ref, score, score)
    assert dev < 1e-12
    if sklearn.__version__ == str(G["sklearn_version"]):
        assert dev == float(G[f"skdev_{name}"])


@pytest.mark.parametrize("d", (1, 2, 3))
def test_normalising_constants(d):
    pytest.importorskip("sklearn")
    from sklearn.neighbors import KernelDensity

    from spateo_amd.tdr.morphometrics.morphology import kde_log_norm

    X = np.zeros((1, d))
    for kernel in kc.KERNELS:
        for h in (0.3, 1.0, 17.5):
            want = KernelDensity(kernel=kernel, bandwidth=h).fit(X).score_samples(X)[0]     # one point on itself: log K(0) = 0
            assert abs(kc.log_norm(h, d, kernel) - want) <= 8 * kc.EPS * max(1.0, abs(want)), (kernel, h)
            assert abs(kde_log_norm(h, d, kernel) - want) <= 8 * kc.EPS * max(1.0, abs(want)), (kernel, h)


def test_constants_without_sklearn():
    """The closed forms against their integrals by quadrature (d = 2 cosine: sklearn's own value, not the integral)."""
    from spateo_amd.tdr.morphometrics.morphology import kde_log_norm

    r = (np.arange(200000) + 0.5) / 200000
    K = {"tophat": np.ones_like(r), "epanechnikov": 1 - r * r, "linear": 1 - r, "cosine": np.cos(0.5 * np.pi * r)}
    surface = {1: 2.0, 2: 2 * np.pi, 3: 4 * np.pi}
    for d in (1, 2, 3):
        for kernel, k in K.items():
            if (kernel, d) == ("cosine", 2):
                continue
            want = -np.log(surface[d] * np.mean(k * r ** (d - 1))) - d * np.log(0.7)
            assert abs(kc.log_norm(0.7, d, kernel) - want) < 1e-9 and abs(kde_log_norm(0.7, d, kernel) - want) < 1e-9
        assert abs(kc.log_norm(0.7, d, "gaussian") + 0.5 * d * np.log(2 * np.pi) + d * np.log(0.7)) < 1e-14
    assert kc.log_norm(1.0, 2, "cosine") == kde_log_norm(1.0, 2, "cosine")


@pytest.mark.parametrize("name", [n for n in kc.NAMES if kc.CASES[n]["kernel"] in kc.COMPACT])
def test_compact_cases_are_decidable(name):
    kc.assert_decidable(kc.CASES[name])


def test_cases_cover_what_they_claim():
    C = kc.CASES
    sizes = {(len(c["T"]), len(c["X"])) for c in C.values()}
    for n in (1, kc.TILE - 1, kc.TILE, kc.TILE + 1):
        assert any(s[0] == n for s in sizes) and any(s[1] == n for s in sizes), n
    assert kc.splits(40, kc.MIN_CHUNK) == 1 and kc.splits(40, kc.MIN_CHUNK + 1) == 2 and kc.splits(300, 12290) >= 3
    assert {(40, 4096), (40, 4097), (300, 12290)} <= sizes
    assert {(c["kernel"], c["d"]) for c in C.values()} >= {(k, d) for k in kc.KERNELS for d in (1, 2, 3)}
    assert {1, 2, 17, 65} <= {c["C"] for c in C.values()}
    grouped = [c for c in C.values() if c["g"] is not None]
    assert any(len(np.unique(c["g"])) < c["C"] for c in grouped)                                  # an id without a source
    assert any(c["w"] is not None and any(c["w"][c["g"] == k].max() == 0 for k in np.unique(c["g"])) for c in grouped)
    assert any(c["w"] is not None and ((c["w"] == 0).any() and (c["w"] > 0).any()) for c in C.values())
    assert any(c["w"] is not None and c["w"][c["w"] > 0].min() < 1e-290 and c["w"].max() > 1e290 for c in C.values())
    for c in C.values():
        if c["far"]:
            ref = kc.log_density(c)[-c["far"]:]
            if c["kernel"] in kc.COMPACT:
                assert np.isneginf(ref).all(), c["name"]
            else:
                assert np.isfinite(ref).all() and (ref < -790).all(), c["name"]     # far below log(min double) = -745
    dup = C["gaussian_d3"]
    assert (kc.pair_dist(dup["T"][:300], dup["X"]) == 0).sum() > 300                              # duplicates: dist == 0 off the diagonal
    two = C["C2_shift_gauss"]
    ref = kc.log_density(two)
    near0 = np.flatnonzero(ref[:, 0] > -20)
    assert len(near0) > 20 and (ref[near0, 1] < -700).all()                                        # one group near, the other far


@pytest.mark.parametrize("name", ("gaussian_d3", "n300_N12290_epan", "C17_gauss", "wide_gauss", "C2_shift_gauss"))
def test_bound_formula(G, name):
    ref, b, tight, dev_order, dev_sk = kc.reference(name)
    rev = kc.log_density(kc.CASES[name], reverse=True)
    fin = np.isfinite(ref)
    assert dev_order == kc.deviation(ref, rev, ref) and dev_sk == float(G[f"skdev_{name}"])
    rel = max(kc.ALLOW * max(dev_order, dev_sk), kc.FLOOR_ULP * kc.EPS)
    assert np.array_equal(b[fin], rel * np.maximum(1.0, np.abs(ref[fin])))
    assert (np.abs(rev[fin] - ref[fin]) <= b[fin] / kc.ALLOW + 1e-300).all()     # the reversed sum itself sits 64 x inside
    print(f"{name}: dev_order {dev_order:.3e}, dev_sklearn {dev_sk:.3e}, dev_extended {float(G[f'xdev_{name}']):.3e}, "
          f"relative bound {rel:.3e}")
    if tight is not None:
        assert (tight[fin] <= b[fin]).all() and float(G[f"xdev_{name}"]) < 1e-12
    assert kc.compare(ref.copy(), ref, b) == 0.0
    worse = ref.copy()
    worse[fin] += 2 * b[fin]
    assert kc.compare(worse, ref, b) > 1.0
    if (~fin).any():
        broken = ref.copy()
        broken[~fin] = -1e308
        with pytest.raises(AssertionError):
            kc.compare(broken, ref, b)
