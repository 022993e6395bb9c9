"""``st.align``'s reference-model route on ``cuda:0``: ``trn`` and ``sample_by_kmeans`` from host arrays against the goldens of the
real reference / SciPy (bounds of tests/_sample_cases.py), ``downsampling`` with its three methods, ``morpho_align_ref`` against
``morpho_align`` of the reference slices and ``BA_transform`` of each pair's field, and ``morpho_align_transformation`` +
``morpho_align_apply_transformation`` against the rigid chain.  The slices are those of tests/_morpho_align_case.py's series."""
import warnings

import numpy as np
import pytest

import _morpho_align_case as mc
import _sample_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def G():
    return sc.load()


@pytest.fixture(scope="module")
def MG():
    return mc.load()


@pytest.fixture(scope="module")
def series(MG):
    """Three 2-D slices of 503 cells, their 150-cell reference slices and the alignment's arguments (a few iterations)."""
    from spateo_amd import align

    models = [mc.sample(MG, f"4_slice{i}") for i in range(3)]
    kw = dict(mc.CASE_KW["4"], genes=[str(g) for g in MG["4_genes"]], max_iter=4, dtype="float64", device=DEV, verbose=False)
    refs = align.downsampling(models, n_sampling=150, sampling_method="random")
    return models, refs, kw


@pytest.mark.parametrize("tag", ("a", "c", "f", "i", "j"))
def test_trn_from_host_arrays_against_the_reference(G, tag):
    from spateo_amd import align

    X, n, seed, kw, W_ref, repeat = sc.golden_case(G, tag)
    np.random.seed(4242)
    W = align.trn(X, n, return_index=False, seed=seed, device=DEV, **kw)
    assert np.array_equal(np.random.random(3), G[f"{tag}_next"])
    bound, _ = sc.trn_bound(X, n, W0=sc.trn_restate(X, n, seed=seed, **kw) if repeat else W_ref, seed=seed, **kw)
    a, b = (sc.sort_rows(W), sc.sort_rows(W_ref)) if repeat else (W, W_ref)
    assert float(np.abs(a - b).max() / np.abs(X).max()) <= bound
    idx = align.trn(X, n, seed=seed, device=DEV, **kw)
    assert idx.dtype == np.int64 and np.array_equal(np.sort(idx), np.sort(sc.nearest_restate(X, W_ref)))
    both = align.trn([X, X[: len(X) // 2]], [n, min(n, 9)], seed=seed, device=DEV, **kw)          # a list: one launch
    assert np.array_equal(both[0], idx) and len(both[1]) == min(n, 9)


def test_sample_by_kmeans_from_host_arrays_against_scipy():
    from scipy.cluster.vq import kmeans2

    from spateo_amd import align

    X = sc.uniform_cloud(6000, 3, seed=21)
    C0 = X[np.random.default_rng(0).choice(6000, 300, replace=False)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        C_ref, _ = kmeans2(X, C0.copy(), iter=10, minit="matrix")
    want = sc.nearest_restate(X, C_ref)
    idx = align.sample_by_kmeans(X, 300, return_index=True, device=DEV)
    assert np.array_equal(idx, want)
    assert np.array_equal(align.sample_by_kmeans(X, 300, init=C0, device=DEV), X[want])
    with pytest.warns(UserWarning, match="One of the clusters is empty"):
        align.sample_by_kmeans(X, 4, init=np.vstack([C0[:3], [[9e6, 9e6, 9e6]]]), iter=2, device=DEV)


def test_downsampling_with_all_three_methods():
    from spateo_amd import AnnDataLite, align

    rng = np.random.default_rng(3)
    models = [AnnDataLite(X=rng.poisson(1.0, (n, 5)).astype(np.float64), obsm={"spatial": sc.uniform_cloud(n, d, seed=n)},
                          obs={"row": np.arange(n)}) for n, d in ((900, 2), (400, 3), (650, 2))]
    for method in ("trn", "kmeans", "random"):
        out = align.downsampling(models, n_sampling=500, sampling_method=method)
        assert [m.n_obs for m in out] == [500, 400, 400]                       # the clamp of the second slice stays
        for m, o in zip(models, out):
            rows = np.asarray(o.obs["row"])
            assert np.array_equal(o.obsm["spatial"], m.obsm["spatial"][rows]) and np.array_equal(o.X, m.X[rows])
            if method == "random":
                assert len(np.unique(rows)) == len(rows)
        if method == "trn":
            for m, o in zip(models, out):
                assert np.array_equal(np.asarray(o.obs["row"]), align.trn(m.obsm["spatial"], o.n_obs, device=DEV))
        if method == "kmeans":
            assert np.array_equal(np.asarray(out[2].obs["row"]), align.sample_by_kmeans(models[2].obsm["spatial"], 400, True))


@pytest.mark.parametrize("mode", ("SN-S", "SN-N"))
def test_morpho_align_ref_against_morpho_align_and_BA_transform(series, mode):
    from spateo_amd import align

    models, refs, kw = series
    out, out_ref, pis, pis_ref = align.morpho_align_ref(models, models_ref=refs, mode=mode, **kw)
    want_ref, want_pis = align.morpho_align(refs, mode=mode, **kw)
    picked = "align_spatial_rigid" if mode == "SN-S" else "align_spatial_nonrigid"
    assert len(out) == len(out_ref) == 3 and len(pis) == len(pis_ref) == 2
    for i in range(3):
        assert out_ref[i].n_obs == 150 and out[i].n_obs == 503
        for key in ("align_spatial", "align_spatial_rigid", "align_spatial_nonrigid"):
            assert np.array_equal(out_ref[i].obsm[key], want_ref[i].obsm[key]), (i, key)
        assert np.array_equal(out_ref[i].obsm["align_spatial"], out_ref[i].obsm[picked])
        assert np.array_equal(out[i].obsm["align_spatial"], out[i].obsm[picked])
    assert np.array_equal(out[0].obsm["align_spatial"], models[0].obsm["spatial"]) and "align_spatial" not in models[1].obsm
    for i in (1, 2):
        vecfld = out[i].uns["VecFld_morpho"]
        assert vecfld is out_ref[i].uns["VecFld_morpho"] and out[i].uns["iter_spatial"] is out_ref[i].uns["iter_spatial"]
        hat, _, opt = align.BA_transform(vecfld, models[i].obsm["spatial"], dtype="float64", device=DEV)
        assert np.array_equal(out[i].obsm["align_spatial_nonrigid"], hat) and np.array_equal(out[i].obsm["align_spatial_rigid"], opt)
        assert not np.array_equal(hat, opt)                                     # mode "SN-N" really picks another array
        P, Pw = pis[i - 1], want_pis[i - 1]
        assert P is pis_ref[i - 1] and (P is None) == (Pw is None)
        if P is not None:
            assert np.array_equal(np.asarray(P), np.asarray(Pw).T)              # morpho_align returns P.T, this route P


def test_morpho_align_ref_draws_its_own_reference_slices(series):
    from spateo_amd import align

    models, refs, kw = series
    a = align.morpho_align_ref(models, n_sampling=150, sampling_method="random", **kw)
    b = align.morpho_align_ref(models, models_ref=refs, **kw)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        for key in ("spatial", "align_spatial", "align_spatial_rigid", "align_spatial_nonrigid"):
            assert np.array_equal(x.obsm[key], y.obsm[key])


def test_transformation_list_reproduces_the_rigid_chain(series):
    from spateo_amd import align

    models, _, kw = series
    small = [m.select_obs(np.arange(0, m.n_obs, 2)) for m in models]
    trans = align.morpho_align_transformation(small, **kw)
    assert len(trans) == 2 and all(t["Rotation"].shape == (2, 2) and t["Translation"].shape == (2,) for t in trans)
    done = align.morpho_align_apply_transformation([m.copy() for m in small], transformation=trans)
    assert np.array_equal(done[0].obsm["align_spatial"], small[0].obsm["spatial"])
    cur = [np.eye(2), np.zeros(2)]
    eps = np.finfo(np.float64).eps
    for i in (1, 2):
        # the pair's own rigid map, refitted: optimal_RnA of slice i + 1 against the raw slice i
        m = align.Morpho_pairwise(sampleA=small[i], sampleB=small[i - 1], spatial_key="spatial", key_added="align_spatial", **kw)
        m.run()
        R, t = align.solve_RT_by_correspondence(m.optimal_RnA[:, :2], small[i].obsm["spatial"][:, :2])
        assert np.array_equal(R, trans[i - 1]["Rotation"]) and np.array_equal(t, trans[i - 1]["Translation"])
        xy = small[i].obsm["spatial"]
        # R is the least-squares fit of a map that IS rigid: it reproduces optimal_RnA to rounding of the fit's sums
        scale = np.abs(m.optimal_RnA).max()
        assert np.abs(xy @ R.T + t - m.optimal_RnA).max() <= 64 * len(xy) * eps * scale
        cur = [cur[0] @ R, t @ cur[0].T + cur[1]]
        chain = xy @ cur[0].T + cur[1]
        assert np.abs(done[i].obsm["align_spatial"] - chain).max() <= 16 * eps * np.abs(chain).max()
