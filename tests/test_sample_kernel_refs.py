"""CPU proof that the restatements of tests/_sample_cases.py - what the GPU suites compare ``csrc/mvf_sample.hip`` against - equal
the real thing, and the derivation of the two bounds those suites use (printed, and recorded in profiles/downsampling.md):

  * TRN restatement vs the goldens of the reference's own ``TRNET`` (tests/golden/ref_downsampling.npz): bit-equal element for
    element where the start draw has no repeat, bit-equal as a sorted multiset of rows where it has (two nodes start identical
    and the reference's unstable ``argsort`` decides which is which);
  * k-means restatement vs ``scipy.cluster.vq.kmeans2(minit="matrix")``: bit-equal centroids, equal labels;
  * nearest row vs a brute-force ``argmin``;
  * the stored deviations of the tmax = 20 series are what the restatement gives today."""
import warnings

import numpy as np
import pytest

import _sample_cases as sc


@pytest.fixture(scope="module")
def G():
    return sc.load()


@pytest.mark.parametrize("tag", sc.TRN_TAGS)
def test_trn_restatement_equals_the_reference(G, tag):
    X, n, seed, kw, W_ref, repeat = sc.golden_case(G, tag)
    W = sc.trn_restate(X, n, seed=seed, **kw)
    assert W.shape == W_ref.shape == (n, X.shape[1])
    if repeat:
        assert np.array_equal(sc.sort_rows(W), sc.sort_rows(W_ref))
    else:
        assert np.array_equal(W, W_ref)
    assert np.array_equal(np.sort(sc.nearest_restate(X, W)), np.sort(sc.nearest_restate(X, W_ref)))


def test_golden_cases_cover_what_they_claim(G):
    cases = {t: sc.golden_case(G, t) for t in sc.TRN_TAGS}
    shapes = {(c[0].shape[0], c[0].shape[1], c[1]) for c in cases.values()}
    assert {(1500, 3, 48), (3000, 2, 33), (1500, 2, 48), (400, 3, 64), (200, 2, 40)} <= shapes
    assert any(c[5] for c in cases.values()) and any(not c[5] for c in cases.values())        # with and without a repeat
    assert any("c" in c[3] for c in cases.values()) and any(c[3].get("tmax") == 20 for c in cases.values())
    assert any(c[1] == 1 for c in cases.values()) and any(c[1] == c[0].shape[0] for c in cases.values())
    assert any(c[2] != 19491001 for c in cases.values()) and all(c[1] <= 64 for c in cases.values())
    for t, c in cases.items():   # the flag is the draw's own property
        w_idx, _ = sc.trn_draws(c[0], c[1], c[2], c[3].get("tmax", 200))
        assert (len(np.unique(w_idx)) < c[1]) == c[5], t


@pytest.mark.parametrize("tag", ("b", "e", "f", "g"))
def test_trn_bound_is_rounding_sized_and_changes_no_cell(G, tag):
    X, n, seed, kw, _, _ = sc.golden_case(G, tag)
    bound, W0 = sc.trn_bound(X, n, seed=seed, **kw)
    print(f"TRN case {tag} {X.shape} n={n}: 4-ulp deviation / extent = {bound / sc.ALLOW:.3e}, GPU bound = {bound:.3e}")
    assert 0 < bound < 1e-12                                  # rounding, far below a cell spacing (extent / sqrt(N) ~ 1e-2)
    W4 = sc.trn_restate(X, n, seed=seed, jitter_ulp=4, **kw)
    assert np.array_equal(sc.nearest_restate(X, W4), sc.nearest_restate(X, W0))


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257))
def test_series_goldens_are_the_restatement(G, n):
    X = sc.series_coordinates(n)
    W = sc.trn_restate(X, n, tmax=20)
    assert np.array_equal(W, G[f"s{n}_W"])
    dev = float(np.abs(sc.trn_restate(X, n, tmax=20, jitter_ulp=4) - W).max() / np.abs(X).max())
    assert dev == float(G[f"s{n}_dev"])


def test_series_deviations_are_rounding_sized(G):
    for n in sc.SERIES:
        dev = float(G[f"s{n}_dev"])
        print(f"TRN series n={n} {sc.SERIES[n]}: 4-ulp deviation / extent = {dev:.3e}, GPU bound = {sc.ALLOW * dev:.3e}")
        assert G[f"s{n}_W"].shape == (n, sc.SERIES[n][1]) and 0 < dev < 1e-13


KMEANS_CASES = [(5000, 3, 64, 10), (20000, 2, 200, 10), (3000, 3, 130, 10), (300, 2, 100, 10), (1, 2, 1, 3), (65, 3, 2, 10)]


@pytest.mark.parametrize("N,d,n,iters", KMEANS_CASES)
def test_kmeans_restatement_equals_kmeans2(N, d, n, iters):
    from scipy.cluster.vq import kmeans2

    X = sc.uniform_cloud(N, d, seed=N + n)
    C0 = X[np.random.default_rng(n).choice(N, n, replace=False)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        C_ref, lab_ref = kmeans2(X, C0.copy(), iter=iters, minit="matrix")
    C, lab, counts = sc.kmeans_restate(X, C0, iters)
    assert np.array_equal(C, C_ref) and np.array_equal(lab, lab_ref)
    assert np.array_equal(counts, np.bincount(lab_ref, minlength=n))
    bound = sc.kmeans_bound(X, C0, iters, C)
    print(f"k-means ({N}, {d}, {n}): shuffled-sum deviation / extent = {bound / sc.ALLOW:.3e}, GPU bound = {bound:.3e}")
    assert bound < 1e-11
    order = np.random.default_rng(5).permutation(N)
    _, lab_sh, _ = sc.kmeans_restate(X, C0, iters, order=order)
    assert np.array_equal(lab_sh, lab)


def test_kmeans_restatement_keeps_the_centroid_of_an_empty_cluster():
    from scipy.cluster.vq import kmeans2

    X = sc.uniform_cloud(400, 2, seed=3)
    C0 = np.vstack([X[:5], [[1e6, 1e6]]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        C_ref, lab_ref = kmeans2(X, C0.copy(), iter=4, minit="matrix")
    C, lab, counts = sc.kmeans_restate(X, C0, 4)
    assert np.array_equal(C, C_ref) and np.array_equal(lab, lab_ref)
    assert counts[5] == 0 and np.array_equal(C[5], [1e6, 1e6])


@pytest.mark.parametrize("N,d,n", [(1, 2, 3), (63, 1, 10), (1000, 3, 40), (5000, 2, 7)])
def test_nearest_restatement_equals_brute_force(N, d, n):
    rng = np.random.default_rng(N + d)
    X = np.round(rng.random((N, d)) * 20)      # a coarse lattice: many equal distances, many duplicated rows
    Q = np.vstack([np.round(rng.random((n, d)) * 20), X[-1:]])
    want = sc.sq_dist(Q, X).argmin(1)
    assert np.array_equal(sc.nearest_restate(X, Q, block=64), want)
    assert np.array_equal(sc.nearest_restate(X, Q), want)
