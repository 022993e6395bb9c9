"""Host tests (no GPU) of the reference-model route of ``st.align``: the C ABI's refusals without a launch, ``sample``'s dispatch
and error text, the ``"random"`` draw against ``np.random`` itself, ``trn``'s draws / schedules / global-generator state against
the goldens of the real reference through the NumPy stand-in of the kernels (tests/_sample_cpu_kernels.py behind the kernel seam),
the clamp quirk of ``downsampling``, ``AnnDataLite`` row subsets, ``solve_RT_by_correspondence`` and the composition of
``morpho_align_apply_transformation`` against the goldens, the named refusals, ``__all__``, and ``morpho_align_ref``'s
bookkeeping with a stubbed ``Morpho_pairwise``."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import _sample_cases as sc
from _sample_cpu_kernels import SampleCpuKernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def G():
    return sc.load()


@pytest.fixture
def seam(monkeypatch):
    from spateo_amd import _runtime as rt

    made = []
    monkeypatch.setattr(rt, "_make_kernels", lambda device, dtype: made.append(SampleCpuKernels(device, dtype)) or made[-1])
    monkeypatch.setattr(rt, "_shared_kernels", lambda device, dtype: rt._make_kernels(device, dtype))
    return made


@pytest.fixture
def no_kernels(monkeypatch):
    from spateo_amd import _runtime as rt

    def refuse(device, dtype):
        raise AssertionError("the kernels were bound before the arguments were refused")

    monkeypatch.setattr(rt, "_make_kernels", refuse)
    monkeypatch.setattr(rt, "_shared_kernels", refuse)


# ------------------------------------------------------------------------------------------------- C ABI without a launch
def test_sampler_entry_points_reject_bad_arguments_without_launching():
    from spateo_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(16)
    assert _lib.TRN_MAX_NODES == 4096
    assert "#define MVF_TRN_MAX_NODES 4096" in open(os.path.join(ROOT, "include", "mvf.h")).read()
    assert lib.mvf_nearest_rows_workspace_bytes(4096, 10) == 0 and lib.mvf_nearest_rows_workspace_bytes(4097, 10) == 2 * 10 * 16
    assert lib.mvf_nearest_rows_workspace_bytes(0, 10) == 0 and lib.mvf_kmeans_workspace_bytes(10, 0) == 0
    assert lib.mvf_kmeans_workspace_bytes(1000, 7) == 7 * 32 and lib.mvf_kmeans_workspace_bytes(1 << 20, 7) == 256 * 7 * 32

    def near(X=p, N=100, d=3, Q=p, n=5, idx=p, ws=None, ws_bytes=0):
        return lib.mvf_nearest_rows(X, N, d, Q, n, idx, ws, ws_bytes, None)

    def km(X=p, N=100, d=3, C=p, n=5, iters=10, labels=p, counts=p, ws=p, ws_bytes=5 * 32):
        return lib.mvf_kmeans(X, N, d, C, n, iters, labels, counts, ws, ws_bytes, None)

    for fn, name, cases in [
        (near, b"mvf_nearest_rows", [dict(X=None), dict(Q=None), dict(idx=None), dict(N=0), dict(n=-1), dict(d=0), dict(d=4),
                                     dict(N=5000), dict(N=5000, ws=p, ws_bytes=2 * 5 * 16 - 1), dict(ws=ctypes.c_void_p(4))]),
        (km, b"mvf_kmeans", [dict(X=None), dict(C=None), dict(labels=None), dict(counts=None), dict(ws=None), dict(N=-1), dict(d=4),
                             dict(iters=0), dict(ws_bytes=5 * 32 - 1), dict(ws=ctypes.c_void_p(4)), dict(n=1 << 31, ws_bytes=1 << 40)]),
    ]:
        for kw in cases:
            assert fn(**kw) != 0 and name in lib.mvf_last_error(), (name, kw, lib.mvf_last_error())
    assert near(n=0) == 0 and km(N=0) == 0 and km(n=0) == 0          # empty problems launch nothing

    def trn(count=1, **over):
        rec = _lib.TrnProblem(X=16, N=100, d=2, n=8, T=4, w_idx=16, p_idx=16, l=16, ep=16, kc=None, W=16)
        for k, v in over.items():
            setattr(rec, k, v)
        return lib.mvf_trn((_lib.TrnProblem * 1)(rec), count, None)

    for kw in [dict(n=4097), dict(n=-1), dict(N=0), dict(d=0), dict(d=4), dict(T=-1), dict(X=None), dict(w_idx=None), dict(W=None),
               dict(p_idx=None), dict(l=None), dict(ep=None), dict(count=-1)]:
        assert trn(**kw) != 0 and b"mvf_trn" in lib.mvf_last_error(), (kw, lib.mvf_last_error())
    assert trn(n=4097) != 0 and b"at most 4096" in lib.mvf_last_error()
    assert lib.mvf_trn(None, 0, None) == 0 and trn(n=0) == 0 and lib.mvf_trn(None, 1, None) != 0


# ------------------------------------------------------------------------------------------------- sample / trn / kmeans
def test_all_lists_the_new_names():
    import spateo_amd as st

    for name in ("trn", "sample_by_kmeans", "sample", "downsampling", "solve_RT_by_correspondence", "morpho_align_transformation",
                 "morpho_align_apply_transformation", "morpho_align_ref"):
        assert name in st.align.__all__ and callable(getattr(st.align, name))


def test_sample_dispatch_error_text_and_the_random_draw(seam):
    import spateo_amd as st

    arr = np.arange(500) * 3
    np.random.seed(19491001)
    want = arr[np.random.choice(500, size=40, replace=False)]
    nxt = np.random.random(3)
    np.random.seed(1)
    assert np.array_equal(st.align.sample(arr, 40), want) and np.array_equal(np.random.random(3), nxt)
    np.random.seed(77)
    want = arr[np.random.choice(500, size=40, replace=False)]
    assert np.array_equal(st.align.sample(arr, 40, method="random", seed=77), want)
    for kw in (dict(method="trn"), dict(method="velocity"), dict(method="lhs", X=np.zeros((500, 2)))):
        with pytest.raises(NotImplementedError) as e:
            st.align.sample(arr, 40, **kw)
        assert str(e.value) == f"The sampling method {kw['method']} is not implemented or relevant data are not provided."
    V = np.random.default_rng(0).standard_normal((500, 3))
    from spateo_amd.preprocess import sample_by_velocity

    assert np.array_equal(st.align.sample(arr, 30, method="velocity", V=V), arr[sample_by_velocity(V, 30)])
    X = sc.uniform_cloud(500, 2, seed=1)
    got = st.align.sample(arr, 12, method="trn", X=X, tmax=5)
    assert np.array_equal(got, arr[st.align.trn(X, 12, tmax=5)]) and seam[-1].calls["trn"] == 1
    got = st.align.sample(arr, 12, method="kmeans", X=X)
    assert np.array_equal(got, arr[st.align.sample_by_kmeans(X, 12, return_index=True)])


@pytest.mark.parametrize("tag", ("e", "f", "g", "h", "i", "j"))
def test_trn_host_side_against_the_reference(G, seam, tag):
    """Draws, schedules, the cutoff and the state the global generator is left in: through the stand-in's steps the nodes are
    the real TRNET's."""
    import spateo_amd as st

    X, n, seed, kw, W_ref, repeat = sc.golden_case(G, tag)
    np.random.seed(4242)
    W = st.align.trn(X, n, return_index=False, seed=seed, **kw)
    assert np.array_equal(np.random.random(3), G[f"{tag}_next"])
    if repeat:
        assert np.array_equal(sc.sort_rows(W), sc.sort_rows(W_ref))
    else:
        assert np.array_equal(W, W_ref)
    idx = st.align.trn(X, n, seed=seed, **kw)
    assert idx.dtype == np.int64 and np.array_equal(np.sort(idx), np.sort(sc.nearest_restate(X, W_ref)))


def test_trn_takes_a_list_as_one_call_and_refuses_by_name(seam):
    import spateo_amd as st
    from spateo_amd import _lib

    Xs = [sc.uniform_cloud(N, d, seed=N) for N, d in ((300, 2), (200, 3), (150, 1))]
    got = st.align.trn(Xs, [10, 7, 5], return_index=False, tmax=4)
    assert seam[-1].calls == {"trn": 1, "trn_problems": 3, "nearest_rows": 0, "kmeans": 0}
    for x, n, w in zip(Xs, (10, 7, 5), got):
        assert np.array_equal(w, st.align.trn(x, n, return_index=False, tmax=4))
    with pytest.raises(NotImplementedError, match="TRN_MAX_NODES"):
        st.align.trn(sc.uniform_cloud(5000, 2, seed=1), _lib.TRN_MAX_NODES + 1)
    with pytest.raises(TypeError, match="unsupported arguments"):
        st.align.trn(Xs[0], 5, k0=3)
    with pytest.raises(ValueError, match="d <= 3"):
        st.align.trn(np.zeros((10, 4)), 5)
    with pytest.raises(ValueError, match="non-finite"):
        st.align.trn(np.full((10, 2), np.nan), 5)


def test_refusals_come_before_the_kernels_are_bound(no_kernels):
    import spateo_amd as st
    from spateo_amd import _lib

    with pytest.raises(NotImplementedError, match="TRN_MAX_NODES"):
        st.align.trn(np.zeros((5000, 2)), _lib.TRN_MAX_NODES + 1)
    with pytest.raises(ValueError, match="distinct start cells"):
        st.align.sample_by_kmeans(np.zeros((5, 2)), 6)
    with pytest.raises(ValueError, match="init must be"):
        st.align.sample_by_kmeans(np.zeros((5, 2)), 2, init=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="iter must be"):
        st.align.sample_by_kmeans(np.zeros((5, 2)), 2, iter=0)


def test_sample_by_kmeans_start_draw_warning_and_outputs(seam):
    import spateo_amd as st

    X = sc.uniform_cloud(600, 3, seed=9)
    C0 = X[np.random.default_rng(0).choice(600, 20, replace=False)]
    idx = st.align.sample_by_kmeans(X, 20, return_index=True)
    C, _, _ = sc.kmeans_restate(X, C0, 10)
    assert np.array_equal(idx, sc.nearest_restate(X, C))                       # the documented start: default_rng(seed=0)
    assert np.array_equal(st.align.sample_by_kmeans(X, 20), X[idx])
    assert np.array_equal(st.align.sample_by_kmeans(X, 20, return_index=True, init=C0, iter=10), idx)
    assert not np.array_equal(st.align.sample_by_kmeans(X, 20, return_index=True, seed=1), idx)
    far = np.vstack([C0[:4], [[1e7, 1e7, 1e7]]])
    with pytest.warns(UserWarning, match="One of the clusters is empty") as rec:
        st.align.sample_by_kmeans(X, 5, init=far, iter=3)
    assert len(rec) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        st.align.sample_by_kmeans(X, 4, init=C0[:4], iter=3)


# ------------------------------------------------------------------------------------------------- AnnDataLite, downsampling
def _slice(n, seed, genes=6):
    import pandas as pd

    from spateo_amd import AnnDataLite

    rng = np.random.default_rng(seed)
    X = sp.csr_matrix(rng.poisson(0.7, (n, genes)).astype(np.float64))
    return AnnDataLite(X=X, var_names=[f"g{i}" for i in range(genes)], layers={"smooth": rng.random((n, genes))},
                       obs={"celltype": pd.Series(pd.Categorical.from_codes(rng.integers(0, 3, n), categories=["a", "b", "c"])),
                            "depth": rng.random(n)},
                       var={"highly_variable": rng.random(genes) > 0.5}, obsm={"spatial": rng.random((n, 2)) * 100},
                       uns={"note": {"k": 1}})


def test_anndata_lite_row_subset():
    a = _slice(30, 0)
    idx = np.array([4, 4, 29, 0, 17])
    b = a.select_obs(idx)
    assert b.n_obs == 5 and sp.issparse(b.X) and np.array_equal(b.X.toarray(), a.X.toarray()[idx])
    assert np.array_equal(b.layers["smooth"], a.layers["smooth"][idx]) and np.array_equal(b.obsm["spatial"], a.obsm["spatial"][idx])
    assert np.array_equal(b.obs["depth"], a.obs["depth"][idx])
    assert list(b.obs["celltype"]) == list(a.obs["celltype"].iloc[idx]) and list(b.obs["celltype"].cat.categories) == ["a", "b", "c"]
    assert b.var_names == a.var_names and np.array_equal(b.var["highly_variable"], a.var["highly_variable"])
    b.uns["note"]["k"] = 2
    b.obsm["spatial"][0] = -1
    assert a.uns["note"]["k"] == 1 and a.obsm["spatial"][4, 0] >= 0
    with pytest.raises(IndexError):
        a.select_obs([30])
    assert a.select_obs([]).n_obs == 0


def test_downsampling_keeps_the_clamp_quirk(seam):
    import spateo_amd as st

    models = [_slice(n, n) for n in (50, 20, 40)]
    for method in ("random", "trn", "kmeans"):
        out = st.align.downsampling(models, n_sampling=30, sampling_method=method)
        assert [m.n_obs for m in out] == [30, 20, 20], method                   # clamped by the second slice, kept for the third
        assert [m.n_obs for m in models] == [50, 20, 40]
        for m, o in zip(models, out):
            pos = [int(np.flatnonzero((m.obsm["spatial"] == r).all(1))[0]) for r in o.obsm["spatial"]]
            assert np.array_equal(o.X.toarray(), m.X.toarray()[pos]) and np.array_equal(o.obs["depth"], m.obs["depth"][pos])
    assert seam[-1].calls["trn_problems"] in (0, 3)
    one = st.align.downsampling(models[0], n_sampling=10, sampling_method="random")
    assert isinstance(one, list) and one[0].n_obs == 10
    np.random.seed(19491001)
    pick = np.random.choice(50, size=10, replace=False)
    assert np.array_equal(one[0].obsm["spatial"], models[0].obsm["spatial"][pick])
    with pytest.raises(NotImplementedError, match="The sampling method lhs is not implemented"):
        st.align.downsampling(models, n_sampling=10, sampling_method="lhs")


# ------------------------------------------------------------------------------------------------- rigid helpers
@pytest.mark.parametrize("tag", ("rt2", "rt3", "rtf"))
def test_solve_rt_by_correspondence_against_the_reference(G, tag):
    import spateo_amd as st

    R, t, s = st.align.solve_RT_by_correspondence(G[f"{tag}_X"], G[f"{tag}_Y"], return_scale=True)
    assert np.array_equal(R, G[f"{tag}_R"]) and np.array_equal(t, G[f"{tag}_t"]) and s == float(G[f"{tag}_s"])
    R2, t2 = st.align.solve_RT_by_correspondence(G[f"{tag}_X"], G[f"{tag}_Y"])
    assert np.array_equal(R2, R) and np.array_equal(t2, t)
    assert (np.linalg.det(R) < 0) == (tag == "rtf")                            # the reflection is not corrected


def test_apply_transformation_composition_against_the_reference(G):
    import spateo_amd as st
    from spateo_amd import AnnDataLite

    models = [AnnDataLite(obsm={"spatial": G[f"ap_spatial{i}"].copy()}) for i in range(3)]
    trans = [{"Rotation": G[f"ap_R{i}"], "Translation": G[f"ap_t{i}"]} for i in range(2)]
    out = st.align.morpho_align_apply_transformation(models, transformation=trans)
    assert out[0] is models[0]
    for i, m in enumerate(out):
        assert np.array_equal(m.obsm["align_spatial"], G[f"ap_aligned{i}"]) and np.array_equal(m.obsm["spatial"], G[f"ap_spatial{i}"])
    with pytest.raises(AssertionError, match="len\\(models\\) - 1"):
        st.align.morpho_align_apply_transformation(models, transformation=trans[:1])


def test_on_disk_forms_are_refused_by_name(no_kernels):
    import spateo_amd as st
    from spateo_amd import AnnDataLite

    models = [AnnDataLite(obsm={"spatial": np.zeros((3, 2))}) for _ in range(2)]
    t = [{"Rotation": np.eye(2), "Translation": np.zeros(2)}]
    for fn, kw, name in [
        (st.align.morpho_align_transformation, dict(models_path="/data"), "models_path"),
        (st.align.morpho_align_transformation, dict(save_transformation=True), "save_transformation"),
        (st.align.morpho_align_transformation, dict(resume=True), "resume"),
        (st.align.morpho_align_apply_transformation, dict(models_path="/data", transformation=t), "models_path"),
        (st.align.morpho_align_apply_transformation, dict(save_models_path="/out", transformation=t), "save_models_path"),
        (st.align.morpho_align_apply_transformation, dict(), "transformation_path"),
    ]:
        with pytest.raises(NotImplementedError, match=name):
            fn(models, **kw)
    with pytest.raises(NotImplementedError, match="models_path"):
        st.align.morpho_align_transformation(["a.h5ad", "b.h5ad"])


# ------------------------------------------------------------------------------------------------- morpho_align_ref bookkeeping
class _FakePair:
    """Stands in for Morpho_pairwise: the "alignment" shifts sampleA by +1 (rigid) / +2 (non-rigid) per call."""
    made = []

    def __init__(self, sampleA, sampleB, **kw):
        self.A, self.B, self.kw = sampleA, sampleB, kw
        _FakePair.made.append(self)

    def run(self):
        k = len(_FakePair.made)
        xy = np.asarray(self.A.obsm[self.kw["spatial_key"]])
        self.optimal_RnA, self.XAHat = xy + 1.0, xy + 2.0
        self.vecfld, self.iter_added = {"pair": k}, {"iters": k}
        return None if self.kw.get("no_P") else np.full((self.A.n_obs, self.B.n_obs), float(k))


@pytest.fixture
def fake_pair(monkeypatch):
    from spateo_amd import _morpho_pairwise, align

    _FakePair.made = []
    monkeypatch.setattr(_morpho_pairwise, "Morpho_pairwise", _FakePair)
    calls = []

    def ba(vecfld, quary_points, device=None, dtype="float64"):
        calls.append((vecfld, np.array(quary_points), device, dtype))
        q = np.asarray(quary_points)
        return q + 20.0 * vecfld["pair"], None, q + 10.0 * vecfld["pair"]

    monkeypatch.setattr(align, "BA_transform", ba)
    return calls


@pytest.mark.parametrize("mode", ("SN-S", "SN-N"))
def test_morpho_align_ref_bookkeeping(seam, fake_pair, mode):
    import spateo_amd as st

    models = [_slice(n, n) for n in (40, 30, 50)]
    raw = [m.obsm["spatial"].copy() for m in models]
    out, out_ref, pis, pis_ref = st.align.morpho_align_ref(models, n_sampling=12, mode=mode, max_iter=3, device="0", dtype="float64",
                                                           beta=0.5)
    ref0 = st.align.downsampling([m.copy() for m in models], n_sampling=12, sampling_method="random")
    assert len(out) == len(out_ref) == 3 and len(pis) == len(pis_ref) == 2 and len(_FakePair.made) == 2
    for i, p in enumerate(_FakePair.made):                                     # B is aligned onto A = the ALIGNED previous one
        assert p.A is out_ref[i + 1] and p.B is out_ref[i] and p.kw["spatial_key"] == p.kw["key_added"] == "align_spatial"
        assert p.kw["max_iter"] == 3 and p.kw["beta"] == 0.5 and p.kw["device"] == "0" and p.kw["dtype"] == "float64"
    shift = 1.0 if mode == "SN-S" else 2.0
    big = 10.0 if mode == "SN-S" else 20.0
    for i in range(3):
        assert np.array_equal(models[i].obsm["spatial"], raw[i]) and "align_spatial" not in models[i].obsm
        assert np.array_equal(out_ref[i].obsm["spatial"], ref0[i].obsm["spatial"])
        if i == 0:
            for key in ("align_spatial", "align_spatial_rigid", "align_spatial_nonrigid"):
                assert np.array_equal(out[0].obsm[key], raw[0]) and np.array_equal(out_ref[0].obsm[key], ref0[0].obsm["spatial"])
            continue
        r = ref0[i].obsm["spatial"]
        assert np.array_equal(out_ref[i].obsm["align_spatial_rigid"], r + 1.0)
        assert np.array_equal(out_ref[i].obsm["align_spatial_nonrigid"], r + 2.0)
        assert np.array_equal(out_ref[i].obsm["align_spatial"], r + shift)
        vec, q, dev, dt = fake_pair[i - 1]
        assert vec == {"pair": i} and np.array_equal(q, raw[i]) and dev == "cuda:0" and dt == "float64"
        assert np.array_equal(out[i].obsm["align_spatial_rigid"], raw[i] + 10.0 * i)
        assert np.array_equal(out[i].obsm["align_spatial_nonrigid"], raw[i] + 20.0 * i)
        assert np.array_equal(out[i].obsm["align_spatial"], raw[i] + big * i)
        for m in (out[i], out_ref[i]):
            assert m.uns["VecFld_morpho"] == {"pair": i} and m.uns["iter_spatial"] == {"iters": i}
        assert pis[i - 1] is pis_ref[i - 1] and pis[i - 1].shape == (12, 12) and pis[i - 1][0, 0] == i
    assert "VecFld_morpho" not in out[0].uns


def test_morpho_align_ref_explicit_reference_none_P_and_keys(seam, fake_pair):
    import spateo_amd as st

    models = [_slice(n, n) for n in (25, 35)]
    refs = [m.select_obs(np.arange(0, m.n_obs, 5)) for m in models]
    out, out_ref, pis, pis_ref = st.align.morpho_align_ref(models, models_ref=refs, iter_key_added=None, vecfld_key_added=None,
                                                           key_added="al", no_P=True)
    assert pis == [None] and pis_ref == [None]
    assert "VecFld_morpho" not in out[1].uns and "iter_spatial" not in out[1].uns and "al_rigid" in out[1].obsm
    assert out_ref[1].n_obs == 7 and "al" not in refs[1].obsm
    with pytest.raises(ValueError, match="mode"):
        st.align.morpho_align_ref(models, models_ref=refs, mode="N-N")


def test_morpho_align_transformation_pairs_raw_slices(fake_pair):
    import spateo_amd as st

    models = [_slice(n, n) for n in (20, 20, 20)]
    trans = st.align.morpho_align_transformation(models, max_iter=2)
    assert len(trans) == 2 and len(_FakePair.made) == 2
    for i, (p, tr) in enumerate(zip(_FakePair.made, trans)):
        assert p.A is models[i + 1] and p.B is models[i] and p.kw["spatial_key"] == "spatial"
        # optimal_RnA = raw + 1: the transformation that maps the raw slice onto it is the identity and a shift by one
        assert np.allclose(tr["Rotation"], np.eye(2), atol=1e-12) and np.allclose(tr["Translation"], [1.0, 1.0], atol=1e-10)
