"""Host tests of ``align.pca`` / ``align.group_pca`` (no GPU): the argument errors of the new entry points through
``mvf_last_error`` without a launch, every refusal, the gene and HVG selection rules, the sign rule and the clipping of
``n_comps``, and the Python on the NumPy stand-in of the kernels (``tests/_pca_cpu_kernels.py`` behind the kernel seam):
``group_pca`` on ``AnnDataLite``, a list of slices against the stacked matrix, and the whole call against the restatement of
``tests/_pca_case.py`` inside its derived bounds."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import _pca_case as pc
from _pca_cpu_kernels import PcaCpuKernels


@pytest.fixture
def seam(monkeypatch):
    """The stand-in behind the kernel seam; `made` lists the kernel objects the calls created."""
    from spateo_amd import _runtime as rt

    made = []
    monkeypatch.setattr(rt, "_make_kernels", lambda device, dtype: made.append(PcaCpuKernels(device, dtype)) or made[-1])
    return made


@pytest.fixture
def no_kernels(monkeypatch):
    """A seam that fails the test when a refusal comes too late (after the kernels were bound)."""
    from spateo_amd import _runtime as rt

    def refuse(device, dtype):
        raise AssertionError("the kernels were bound before the arguments were refused")

    monkeypatch.setattr(rt, "_make_kernels", refuse)


# ------------------------------------------------------------------------------------------------- C ABI without a launch
def test_new_entry_points_reject_bad_arguments_without_launching():
    from spateo_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(16)
    n, g = 300, 20
    ws = lib.mvf_colmeans_workspace_bytes(n, g)
    assert ws == 1 * g * 8 and lib.mvf_colmeans_workspace_bytes(1025, g) == 2 * g * 8
    assert lib.mvf_colmeans_workspace_bytes(0, g) == 0 and lib.mvf_colmeans_workspace_bytes(n, 0) == 0
    ub = lib.mvf_ublk_bytes(n, g, _lib.MVF_F32)
    assert ub == 512 * 128 * 4

    def means(x=p, n=n, g=g, n_total=n, row0=0, mean=p, wsp=p, ws_bytes=ws):
        return lib.mvf_colmeans(x, 1, n, g, n_total, row0, mean, wsp, ws_bytes, None)

    def pack(x=p, n=n, g=g, n_total=n, row0=0, ublk=p, ub_bytes=ub, dtype=_lib.MVF_F32):
        return lib.mvf_ublk_pack(x, 0, n, g, None, n_total, row0, ublk, ub_bytes, dtype, None)

    def means_csr(indptr=p, n=n, g=g, n_total=n, row0=0, mean=p, wsp=p, ws_bytes=ws, stage=p, st_bytes=g * 8):
        return lib.mvf_colmeans_csr(indptr, p, p, 0, n, g, n_total, row0, mean, wsp, ws_bytes, stage, st_bytes, None)

    def pack_csr(indptr=p, n=n, g=g, n_total=n, row0=0, ublk=p, ub_bytes=ub, stage=p, st_bytes=g * 4, dtype=_lib.MVF_F64):
        return lib.mvf_ublk_pack_csr(indptr, p, p, 1, n, g, None, n_total, row0, ublk, ub_bytes, stage, st_bytes, dtype, None)

    refused = [
        (means, b"mvf_colmeans", [dict(x=None), dict(n=0), dict(g=0), dict(n_total=n - 1), dict(row0=1), dict(row0=-1), dict(mean=None),
                                  dict(wsp=None), dict(ws_bytes=ws - 1), dict(wsp=ctypes.c_void_p(4))]),
        (pack, b"mvf_ublk_pack", [dict(x=None), dict(n=0), dict(g=0), dict(n_total=n - 1), dict(row0=1), dict(ublk=None),
                                  dict(ub_bytes=ub - 1), dict(dtype=7), dict(ublk=ctypes.c_void_p(8))]),
        (means_csr, b"mvf_colmeans_csr", [dict(indptr=None), dict(n=0), dict(row0=1), dict(mean=None), dict(ws_bytes=ws - 1),
                                          dict(stage=None), dict(st_bytes=g * 8 - 1), dict(g=1 << 31, ws_bytes=1 << 40)]),
        (pack_csr, b"mvf_ublk_pack_csr", [dict(indptr=None), dict(n=0), dict(row0=1), dict(ublk=None), dict(ub_bytes=ub - 1),
                                          dict(stage=None), dict(st_bytes=g * 4 - 1), dict(dtype=-1)]),
    ]
    for fn, name, cases in refused:
        for kw in cases:
            assert fn(**kw) != 0 and name in lib.mvf_last_error(), (name, kw, lib.mvf_last_error())
    assert pack(ub_bytes=ub - 1) != 0 and b"buffer too small" in lib.mvf_last_error()
    assert means(ws_bytes=0) != 0 and b"workspace too small" in lib.mvf_last_error()
    # a slice that does not end the matrix needs no `mean`; the error here is the null input, found before any launch
    assert means(x=None, n=100, mean=None) != 0 and b"null pointer" in lib.mvf_last_error()
    with pytest.raises(_lib.MVFError, match="mvf_ublk_pack_csr"):
        _lib.check(pack_csr(dtype=-1), "mvf_ublk_pack_csr")


def test_limits_are_the_code_s_own():
    """PCA_MAX_FEATURES: the Gram stage reduces with one grid row per pair of 128-wide tiles, nt (nt + 1) / 2 <= 65535;
    PCA_MAX_COMPS: mvf_apply_cached takes 128 columns per pass over the cache."""
    from spateo_amd import _lib

    nt = _lib.PCA_MAX_FEATURES // 128
    assert _lib.PCA_MAX_FEATURES % 128 == 0 and nt * (nt + 1) // 2 <= 65535 < (nt + 1) * (nt + 2) // 2
    assert _lib.PCA_MAX_COMPS == 128


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_the_kernels_are_bound(no_kernels):
    import spateo_amd as st
    from spateo_amd import _lib

    rng = np.random.default_rng(0)
    X = rng.standard_normal((40, 6))
    bad = X.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        st.align.pca([X, bad])
    inf = sp.csr_matrix(X)
    inf.data[5] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        st.align.pca([inf])
    with pytest.raises(ValueError, match="at least 2 cells"):
        st.align.pca([X[:1]])
    with pytest.raises(ValueError, match="at least 2 cells"):
        st.align.pca([X[:0], X[:1]])
    with pytest.raises(ValueError, match="at least 2 features"):
        st.align.pca([X[:, :1]])
    with pytest.raises(ValueError, match="columns"):
        st.align.pca([X, X[:, :5]])
    with pytest.raises(ValueError, match="n_comps"):
        st.align.pca([X], n_comps=0)
    with pytest.raises(ValueError, match="dtype"):
        st.align.pca([X], dtype="float16")
    with pytest.raises(ValueError, match="no slices"):
        st.align.pca([])
    wide = np.zeros((2, _lib.PCA_MAX_FEATURES + 1), dtype=np.float32)
    with pytest.raises(NotImplementedError, match=str(_lib.PCA_MAX_FEATURES)):
        st.align.pca([wide])
    many = rng.standard_normal((_lib.PCA_MAX_COMPS + 2, _lib.PCA_MAX_COMPS + 2))
    with pytest.raises(NotImplementedError, match="PCA_MAX_COMPS"):
        st.align.pca([many], n_comps=_lib.PCA_MAX_COMPS + 1)


def test_a_cache_larger_than_the_free_memory_is_refused_with_its_size(seam, monkeypatch):
    import spateo_amd as st
    from spateo_amd import _lib

    X = np.random.default_rng(1).standard_normal((300, 20))
    monkeypatch.setattr(PcaCpuKernels, "free_bytes", 512 * 128 * 4)  # exactly the float32 cache: not enough
    with pytest.raises(_lib.MVFError, match=rf"kernel-value cache \({512 * 128 * 4} bytes"):
        st.align.pca([X], dtype="float32")
    assert seam[-1].calls == []  # nothing was opened, nothing launched
    monkeypatch.setattr(PcaCpuKernels, "free_bytes", 512 * 128 * 4 + 1)
    st.align.pca([X], n_comps=3, dtype="float32")
    assert seam[-1].calls == ["open", "means", "pack", "gram", "scores", "close"]


# ------------------------------------------------------------------------------------------------- sign rule, k
def test_sign_rule_and_clipping(seam):
    import spateo_amd as st

    V = np.array([[0.1, -0.5, 0.5], [-0.9, 0.5, -0.5], [0.2, 0.1, 0.1]])
    flipped, signs = st.align.pca_sign(V)
    assert signs.tolist() == [-1.0, -1.0, 1.0]      # column 1: |-0.5| == |0.5|, the lowest index decides
    assert np.array_equal(flipped, V * signs) and np.array_equal(flipped, pc.sign_rule(V))
    rng = np.random.default_rng(2)
    for (n, g), n_comps, k in (((30, 7), 50, 6), ((5, 9), 50, 4), ((30, 7), 3, 3), ((2, 2), 50, 1)):
        res = st.align.pca([rng.standard_normal((n, g))], n_comps=n_comps, dtype="float64")
        assert k == pc.clip_k(n_comps, n, g)
        assert res["PCs"].shape == (g, k) and res["X_pca"][0].shape == (n, k)
        assert res["variance"].shape == (k,) and res["variance_ratio"].shape == (k,) and res["mean"].shape == (g,)
        top = np.argmax(np.abs(res["PCs"]), axis=0)
        assert (res["PCs"][top, np.arange(k)] > 0).all()
        assert (np.diff(res["variance"]) <= 0).all()


# ------------------------------------------------------------------------------------------------- the call on the stand-in
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("zero_center", [True, False])
def test_pca_on_the_stand_in_matches_the_restatement(seam, dtype, zero_center):
    import spateo_amd as st

    k = 5
    X = pc.planted(257, 17, k, seed=3)
    res = st.align.pca([X], n_comps=k, zero_center=zero_center, dtype=dtype)
    Xc = X - res["mean"] if zero_center else X
    if dtype == "float32":
        Xc = Xc.astype(np.float32).astype(np.float64)
    dof = len(X) - 1 if zero_center else len(X)
    pc.check_against(res["PCs"], res["X_pca"][0], res["variance"], Xc, k, dof, score_extra=2.0 ** -24 if dtype == "float32" else 0.0,
                     label=f"stand-in {dtype} zero_center={zero_center}")
    if zero_center:
        assert np.abs(res["mean"] - X.mean(0)).max() <= len(X) * pc.EPS * np.abs(X).max()
    else:
        assert not res["mean"].any()
    orc, _, _, var_tol = pc.bounds(Xc, k, dof)
    assert np.abs(res["variance_ratio"] - orc["variance_ratio"]).max() <= 2 * var_tol / orc["lam_all"][0]
    assert res["variance_ratio"].sum() < 1.0
    assert np.abs(res["PCs"].T @ res["PCs"] - np.eye(k)).max() < 1e-12


def test_a_list_of_slices_equals_the_stacked_matrix(seam):
    import spateo_amd as st

    X = pc.planted(1000, 24, 6, seed=4)
    X[np.abs(X) < 0.7] = 0.0
    parts = [X[:400], sp.csr_matrix(X[400:750]), X[750:750], X[750:].astype(np.float32).astype(np.float64)]
    stacked = np.vstack([X[:750], parts[3]])
    a = st.align.pca(parts, n_comps=6)
    b = st.align.pca(stacked, n_comps=6)
    assert [s.shape for s in a["X_pca"]] == [(400, 6), (350, 6), (0, 6), (250, 6)]
    assert np.array_equal(np.vstack(a["X_pca"]), b["X_pca"][0])
    for q in ("PCs", "variance", "variance_ratio", "mean"):
        assert np.array_equal(a[q], b[q]), q


# ------------------------------------------------------------------------------------------------- group_pca
def _slices(seed=5, sparse_one=True, hvg=True):
    from spateo_amd import AnnDataLite

    rng = np.random.default_rng(seed)
    genes = [f"g{i}" for i in range(12)]
    orders = [genes, genes[::-1], genes[2:] + ["only_c"]]
    marks = [set(genes[:9]), set(genes[1:10]), set(genes[2:11]) | {"only_c"}]
    out = []
    for i, (names, n) in enumerate(zip(orders, (40, 35, 25))):
        X = rng.poisson(2.0, (n, len(names))).astype(np.float64)
        var = {"highly_variable": np.array([g in marks[i] for g in names])} if hvg else {}
        out.append(AnnDataLite(X=sp.csr_matrix(X) if (sparse_one and i == 1) else X, var_names=names, var=var,
                               obsm={"spatial": rng.standard_normal((n, 2))}))
    return out


def test_gene_and_hvg_selection_rules():
    from spateo_amd.align import _pca_genes

    ads = _slices()
    # marked in EVERY slice, in the first slice's order
    assert _pca_genes(ads, True, "highly_variable", None) == [f"g{i}" for i in range(2, 9)]
    # without HVG: the genes every slice carries, first slice's order
    assert _pca_genes(ads, False, "highly_variable", None) == [f"g{i}" for i in range(2, 12)]
    # genes=: restricted to the allowed ones, in ITS order, duplicates dropped
    assert _pca_genes(ads, True, "highly_variable", ["g8", "g0", "g3", "g8", "nope"]) == ["g8", "g3"]
    with pytest.raises(ValueError, match="No highly variable genes were found"):
        _pca_genes(ads, True, "highly_variable", ["g0", "g11"])
    for a in ads:
        a.var["hv2"] = np.zeros(len(a.var_names), dtype=bool)
    with pytest.raises(ValueError, match="No highly variable genes were found"):
        _pca_genes(ads, True, "hv2", None)
    del ads[1].var["highly_variable"]
    with pytest.raises(NotImplementedError, match=r"scanpy.*genes=.*use_hvg=False"):
        _pca_genes(ads, True, "highly_variable", None)
    ads[2].var_names = ["x", "y"]
    with pytest.raises(ValueError, match="common gene"):
        _pca_genes(ads, False, "highly_variable", None)


def test_group_pca_on_anndata_lite(seam):
    import spateo_amd as st

    ads = _slices()
    assert st.align.group_pca(ads, n_comps=4, dtype="float64") is None
    assert [a.obsm["X_pca"].shape for a in ads] == [(40, 4), (35, 4), (25, 4)]
    assert all(a.obsm["X_pca"].dtype == np.float64 for a in ads)
    # what it ran on: the HVG-in-every-slice genes, each slice's columns brought into the first slice's order
    use = [f"g{i}" for i in range(2, 9)]
    mats = [np.asarray(a.X.todense() if sp.issparse(a.X) else a.X)[:, a.var_index(use)] for a in ads]
    ref = st.align.pca(mats, n_comps=4, dtype="float64")
    for a, s in zip(ads, ref["X_pca"]):
        assert np.array_equal(a.obsm["X_pca"], s)
    # pca_key, use_hvg=False and genes=
    st.align.group_pca(ads, pca_key="pcs", use_hvg=False, genes=["g5", "g2", "g9"], n_comps=2, dtype="float64")
    mats = [np.asarray(a.X.todense() if sp.issparse(a.X) else a.X)[:, a.var_index(["g5", "g2", "g9"])] for a in ads]
    ref = st.align.pca(mats, n_comps=2, dtype="float64")
    assert all(np.array_equal(a.obsm["pcs"], s) for a, s in zip(ads, ref["X_pca"]))
    # the reference's errors
    ads[1].obs["batch"] = np.zeros(35)
    with pytest.raises(ValueError, match="batch_key 'batch' already exists in adata.obs for dataset 1"):
        st.align.group_pca(ads)
    st.align.group_pca(ads, batch_key="slice", n_comps=2)
    with pytest.raises(TypeError, match="svd_solver"):
        st.align.group_pca(ads, batch_key="slice", svd_solver="arpack")
    with pytest.raises(NotImplementedError, match="scanpy"):
        st.align.group_pca(_slices(hvg=False))
    assert {"pca", "group_pca"} <= set(st.align.__all__)
