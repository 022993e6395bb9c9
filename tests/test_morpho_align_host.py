"""Host side of ``spateo_amd.align.Morpho_pairwise`` / ``morpho_align`` and of the sparse layers (no GPU): the restated
``_check`` and ``_align_preprocess`` of the reference against what the real class recorded in
tests/golden/ref_morpho_align.npz (tests/golden/make_golden_morpho_align.py) - the constructor touches no device -, every
refusal by its message, the CSR host validation, ``AnnDataLite`` with sparse matrices and the ``return_P`` arguments."""
import numpy as np
import pytest
import scipy.sparse as sp

import _morpho_align_case as mc

G = mc.load()


def _model(tag, **over):
    from spateo_amd import align

    A, B = mc.pair_samples(G, tag)
    return align.Morpho_pairwise(A, B, dtype="float64", verbose=False, **mc.pair_kwargs(G, tag, **over))


@pytest.fixture(scope="module")
def models():
    return {tag: _model(tag) for tag in ("1", "2", "3")}


# ---- _check ----
@pytest.mark.parametrize("tag", ["1", "2", "3"])
def test_check_gives_the_reference_lists(models, tag):
    m = models[tag]
    for q in ("rep_layer", "rep_field", "dissimilarity", "probability_type"):
        assert list(getattr(m, q)) == [str(v) for v in G[f"{tag}_{q}"]], q
    assert len(m.probability_parameters) == len(m.rep_layer)
    if tag == "3":   # rep_field="obs" forces "label" / "prob"
        assert m.dissimilarity[1] == "label" and m.probability_type[1] == "prob" and m.obs_key == "celltype"
        assert m.label_transfer.shape == (5, 5)
        want = G["3_label_transfer_values"].astype(np.float32).astype(np.float64)
        assert np.array_equal(m.label_transfer, want)


def test_check_errors():
    from spateo_amd import align

    A, B = mc.pair_samples(G, "3")
    kw = dict(dtype="float64", verbose=False)
    with pytest.raises(ValueError, match="representation 'nope' not found in the 'layer' attribute"):
        align.Morpho_pairwise(A, B, rep_layer="nope", **kw)
    with pytest.raises(ValueError, match="representation 'nope' not found in the 'obsm' attribute"):
        align.Morpho_pairwise(A, B, rep_layer="nope", rep_field="obsm", **kw)
    with pytest.raises(ValueError, match="rep_field must be either"):
        align.Morpho_pairwise(A, B, rep_layer="X", rep_field="varm", **kw)
    with pytest.raises(ValueError, match="'obs' occurs more than once"):
        align.Morpho_pairwise(A, B, rep_layer=["celltype", "celltype"], rep_field=["obs", "obs"], **kw)
    with pytest.raises(ValueError, match="No representation input"):
        align.Morpho_pairwise(A, B, rep_layer=None, **kw)
    with pytest.raises(KeyError, match="Spatial key 'where' not found in sampleA"):
        align.Morpho_pairwise(A, B, spatial_key="where", **kw)
    with pytest.raises(ValueError, match="Invalid `metric` value: manhattan"):
        align.Morpho_pairwise(A, B, dissimilarity="manhattan", **kw)
    with pytest.raises(ValueError, match="Invalid `metric` value: laplace"):
        align.Morpho_pairwise(A, B, probability_type="laplace", **kw)
    with pytest.raises(ValueError, match="Invalid `guidance_effect` value: sideways"):
        align.Morpho_pairwise(A, B, guidance_effect="sideways", **kw)
    with pytest.raises(ValueError, match="not found in the 'layer' attribute"):   # the coarse alignment's layer is checked too
        align.Morpho_pairwise(A, B, init_layer="nope", **kw)
    C = A.copy()
    C.obs["plain"] = np.arange(C.n_obs)
    with pytest.raises(ValueError, match="'plain' found in the 'obs' attribute should be categorical"):
        align.Morpho_pairwise(C, C, rep_layer="plain", rep_field="obs", **kw)
    ltd = mc.label_transfer_dict(G, "3")
    del ltd["T2"]
    with pytest.raises(KeyError, match="Category 'T2' from catA not found"):
        align.Morpho_pairwise(A, B, rep_layer=["X", "celltype"], rep_field=["layer", "obs"], label_transfer_dict=ltd, **kw)
    ltd = mc.label_transfer_dict(G, "3")
    del ltd["T1"]["T4"]
    with pytest.raises(KeyError, match="Category 'T4' from catB not found in label_transfer_dict for category 'T1'"):
        align.Morpho_pairwise(A, B, rep_layer=["X", "celltype"], rep_field=["layer", "obs"], label_transfer_dict=ltd, **kw)
    with pytest.raises(ValueError, match="dtype must be"):
        align.Morpho_pairwise(A, B, dtype="float16", verbose=False)
    # a string becomes a list, a missing field "layer"
    m = align.Morpho_pairwise(A, B, rep_layer="X", rep_field=None, nn_init=False, **kw)
    assert m.rep_layer == ["X"] and m.rep_field == ["layer"] and m.dissimilarity == ["kl"] and m.probability_type == ["gauss"]
    assert m.probability_parameters == [None]


# ---- genes ----
def test_gene_selection_and_order(models):
    from spateo_amd import _morpho_pairwise as mp

    A, B = mc.pair_samples(G, "1")
    ref = [str(g) for g in G["1_genes"]]
    # genes= given: its order
    assert models["1"].genes == ref
    # none given: the same SET (highly_variable honoured: fewer than the 40 common genes), in sample A's var order
    own = mp.common_genes(A, B, use_hvg=True)
    assert set(own) == set(ref) and len(ref) < 40
    order = {g: i for i, g in enumerate(A.var_names)}
    assert own == sorted(own, key=order.__getitem__)
    every = mp.common_genes(A, B, use_hvg=False)
    assert len(every) == 40 and set(ref) < set(every)
    assert mp.common_genes(A, B, use_hvg=False, genes=["g003", "zzz", "g001", "g003"]) == ["g003", "g001"]
    with pytest.raises(ValueError, match="None of `genes`"):
        mp.common_genes(A, B, genes=["zzz"])
    C = A.select_vars([g for g in A.var_names if g.startswith("a")])
    with pytest.raises(ValueError, match="number of common gene between all samples is 0"):
        mp.common_genes(C, B)


def test_column_selection_on_csr_equals_dense(models):
    A, _ = mc.pair_samples(G, "1")
    Ad, _ = mc.pair_samples(G, "1", dense=True)
    from spateo_amd import align

    kw = mc.pair_kwargs(G, "1")
    sparse = models["1"].exp_layers_A[0]
    dense = align.Morpho_pairwise(Ad, Ad, dtype="float64", verbose=False, **kw).exp_layers_A[0]
    assert sp.issparse(sparse) and sparse.format == "csr" and isinstance(dense, np.ndarray) and dense.dtype == np.float64
    assert np.array_equal(sparse.toarray(), dense) and dense.shape == (A.n_obs, len(kw["genes"]))
    # ... and equals picking the genes by name from the full matrix
    where = {g: i for i, g in enumerate(A.var_names)}
    assert np.array_equal(dense, Ad.X[:, [where[g] for g in kw["genes"]]])
    assert np.array_equal(A.select_vars(kw["genes"]).X.toarray(), dense)


# ---- coordinates and normalisation ----
@pytest.mark.parametrize("tag", ["1", "2", "3"])
def test_normalisation_parameters(models, tag):
    m = models[tag]
    assert m.D == (2 if tag == "1" else 3)          # case 1: three columns stored, z constant -> a 2-D problem
    scales, means = G[f"{tag}_normalize_scales"], G[f"{tag}_normalize_means"]
    assert np.shape(m.normalize_scales) == scales.shape and np.shape(m.normalize_means) == means.shape
    assert np.abs(m.normalize_scales - scales).max() <= mc.HOST_TOL * np.abs(scales).max()
    assert np.abs(m.normalize_means - means).max() <= mc.HOST_TOL * np.abs(means).max()
    if tag == "2":   # separate_scale
        assert m.normalize_scales[0] != m.normalize_scales[1]
    if tag == "3":   # separate_mean=False: the reference's (2 D,) repeat, one scalar for both slices
        assert means.shape == (6,) and m.normalize_means[0] == m.normalize_means[1]
    # de-normalisation is the inverse for the fixed slice
    assert np.abs(m._denormalize(m.coordsB) - m.raw_coordsB).max() <= mc.HOST_TOL * np.abs(m.raw_coordsB).max()


def test_expression_normalisation(models):
    m = models["2"]
    assert list(m.exp_scales) == [1]                # the "euc" layer, not the "kl" one
    assert abs(m.exp_scales[1] - float(G["2_exp_scale"])) <= mc.HOST_TOL * float(G["2_exp_scale"])
    A, B = mc.pair_samples(G, "2")
    assert sp.issparse(m.exp_layers_A[1]) and sp.issparse(m.exp_layers_A[0])
    raw = A.select_vars(m.genes)
    assert np.array_equal(m.exp_layers_A[0].toarray(), raw.X.toarray())                       # kl: untouched
    assert np.allclose(m.exp_layers_A[1].toarray() * m.exp_scales[1], raw.layers["smooth"].toarray(), rtol=1e-14, atol=0)
    assert np.array_equal(A.layers["smooth"].toarray(), mc.pair_samples(G, "2")[0].layers["smooth"].toarray())   # the sample is left alone
    # the same scale from dense layers
    from spateo_amd import align

    Ad, Bd = mc.pair_samples(G, "2", dense=True)
    md = align.Morpho_pairwise(Ad, Bd, dtype="float64", verbose=False, **mc.pair_kwargs(G, "2"))
    assert abs(md.exp_scales[1] - m.exp_scales[1]) <= mc.HOST_TOL * m.exp_scales[1]


def test_check_spatial_coords():
    from spateo_amd import AnnDataLite
    from spateo_amd import _morpho_pairwise as mp

    rng = np.random.default_rng(0)
    s = AnnDataLite(obsm={"spatial": np.column_stack([rng.random(9), np.full(9, 2.0), rng.random(9)])})
    assert mp.check_spatial_coords(s).shape == (9, 2)
    s.obsm["spatial"] = np.column_stack([rng.random(9), np.full(9, 2.0)])
    with pytest.raises(ValueError, match="should only has 2 / 3 dimension"):
        mp.check_spatial_coords(s)
    s.obsm["spatial"] = rng.random((9, 4))
    with pytest.raises(ValueError, match="should only has 2 / 3 dimension"):
        mp.check_spatial_coords(s)
    with pytest.raises(KeyError, match="Spatial key 'other'"):
        mp.check_spatial_coords(s, "other")


# ---- output ----
def test_wrap_output_keys_and_denormalisation(models):
    from spateo_amd import _morpho_pairwise as mp
    from spateo_amd import align

    assert sorted(mp.VECFLD_KEYS) == [str(k) for k in G["1_vecfld_keys"]]
    assert sorted(mp.NORM_DICT_KEYS) == [str(k) for k in G["1_norm_dict_keys"]]
    m = _model("1", iter_key_added="iter_spatial")
    rng = np.random.default_rng(1)
    NA, D, K, iters = m.NA, m.D, 16, 3
    start = align._Start(probability_parameters=[0.3], sigma2=0.7, inducing_variables=rng.random((K, D)), samples_s=1.0, inliers=None)
    start.coordsA, start.init_R, start.init_t = rng.random((NA, D)), np.eye(D), np.zeros(D)
    start.inducing_rows = np.arange(K)
    hist = dict(XAHat=rng.random((iters, NA, D)), sigma2=np.array([0.5, 0.4, 0.3]))
    out = dict(R=np.eye(D), t=np.zeros(D), optimal_R=np.eye(D), optimal_t=np.zeros(D), sigma2=0.3, gamma=0.9, sigma2_variance=1.1,
               Coff=rng.random((K, D)), VnA=np.zeros((NA, D)), alpha=np.ones(NA), SigmaDiag=np.zeros(NA), K_NA=np.ones(NA),
               K_NB=np.ones(m.NB), XAHat=hist["XAHat"][-1], RnA=rng.random((NA, D)), optimal_RnA=rng.random((NA, D)), history=hist)
    m._wrap_output(start, out)
    assert sorted(m.vecfld) == sorted(mp.VECFLD_KEYS) and sorted(m.vecfld["norm_dict"]) == sorted(mp.NORM_DICT_KEYS)
    s, mean = m.normalize_scales[1], m.normalize_means[1]
    for q in ("XAHat", "RnA", "optimal_RnA"):
        assert np.array_equal(getattr(m, q), out[q] * s + mean), q
    assert m.P is None and m.probability_parameters == [0.3]
    assert np.array_equal(m.inducing_variables, m.coordsA[:K])          # the rows as they were before the coarse transform
    # _save_iter: the state at the START of every iteration
    frames, sig = m.iter_added["align_spatial"], m.iter_added["sigma2"]
    assert sorted(frames) == [0, 1, 2] and sorted(sig) == [0, 1, 2]
    assert np.array_equal(frames[0], start.coordsA * s + mean) and np.array_equal(frames[2], hist["XAHat"][1] * s + mean)
    assert [float(sig[i]) for i in range(3)] == [0.7, 0.5, 0.4]
    assert np.array_equal(m.vecfld["norm_dict"]["mean_fixed"], m.normalize_means[1])
    assert np.array_equal(m.vecfld["norm_dict"]["scale_transformed"], m.normalize_scales[0])


def test_device_argument():
    from spateo_amd import _morpho_pairwise as mp

    assert mp._device_argument("cpu") is None and mp._device_argument(None) is None
    assert mp._device_argument("0") == "cuda:0" and mp._device_argument("3") == "cuda:3" and mp._device_argument("cuda:1") == "cuda:1"


# ---- refusals ----
def test_refusals_by_name():
    from spateo_amd import align

    A, B = mc.pair_samples(G, "1")
    kw = dict(dtype="float64", verbose=False, nn_init=False)
    pair = [np.zeros((3, 2)), np.zeros((3, 2))]
    with pytest.raises(NotImplementedError, match="guidance_pair"):
        align.Morpho_pairwise(A, B, guidance_pair=pair, guidance_effect="both", **kw)
    align.Morpho_pairwise(A, B, guidance_pair=pair, guidance_effect=False, **kw)               # no effect asked for: accepted
    align.Morpho_pairwise(A, B, guidance_pair=pair, guidance_effect="rigid", guidance_weight=0.0, **kw)
    with pytest.raises(NotImplementedError, match="kernel_type='geodist'"):
        align.Morpho_pairwise(A, B, kernel_type="geodist", **kw)
    with pytest.raises(NotImplementedError, match="graph="):
        align.Morpho_pairwise(A, B, graph=object(), **kw)
    with pytest.raises(NotImplementedError, match=r"sparse_top_k = 1024.*at most 64.*1024 is only the reference"):
        align.Morpho_pairwise(A, B, sparse_calculation_mode=True, **kw)
    align.Morpho_pairwise(A, B, sparse_calculation_mode=True, sparse_top_k=64, **kw)
    align.Morpho_pairwise(A, B, sparse_top_k=1024, **kw)                                        # the default, dense mode: unused
    with pytest.raises(NotImplementedError, match="at most 4 layers"):
        align.Morpho_pairwise(A, B, rep_layer=["X"] * 5, **kw)
    # accepted with no effect
    m = align.Morpho_pairwise(A, B, use_chunk=True, chunk_capacity=2.0, pre_compute_dist=False, save_concrete_iter=True, **kw)
    assert m.use_chunk and m.chunk_capacity == 2.0


def test_morpho_align_mode_is_checked():
    from spateo_amd import align

    with pytest.raises(ValueError, match="mode must be"):
        align.morpho_align([], mode="SN")
    assert align.morpho_align([]) == ([], [])


# ---- CSR host validation ----
def test_csr_arrays():
    from spateo_amd._kernels import csr_arrays, is_sparse

    # duplicates and unsorted indices: summed on a copy
    m = sp.csr_matrix((np.array([1, 2, 3, 4], dtype=np.int64), np.array([2, 0, 2, 1], dtype=np.int32), np.array([0, 3, 4])),
                      shape=(2, 3))
    assert not m.has_canonical_format
    indptr, indices, data, n, g = csr_arrays(m)
    assert (n, g) == (2, 3) and indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float64
    assert indptr.tolist() == [0, 2, 3] and indices.tolist() == [0, 2, 1] and data.tolist() == [2.0, 4.0, 4.0]
    assert m.nnz == 4                                                       # the caller's matrix is left alone
    # float32 stays float32; csc / coo are converted
    f = sp.random(5, 7, 0.4, format="csc", random_state=0, dtype=np.float32)
    assert csr_arrays(f)[2].dtype == np.float32 and np.array_equal(sp.csr_matrix(csr_arrays(f)[:3][::-1], shape=(5, 7)).toarray(), f.toarray())
    # a decreasing indptr raises before anything is launched
    bad = sp.csr_matrix((3, 4))
    bad.indptr = np.array([0, 2, 1, 2], dtype=np.int32)
    bad.indices, bad.data = np.array([0, 1], dtype=np.int32), np.array([1.0, 2.0])
    with pytest.raises(ValueError, match="malformed CSR layer"):
        csr_arrays(bad)
    neg = sp.csr_matrix((2, 4))
    neg.indptr = np.array([-1, 0, 0], dtype=np.int32)
    with pytest.raises(ValueError, match="malformed CSR layer"):
        csr_arrays(neg)
    with pytest.raises(ValueError, match="at most 2\\^31 - 1 columns"):
        csr_arrays(sp.csr_matrix((1, 2 ** 31)))
    assert is_sparse(m) and not is_sparse(np.zeros((2, 2))) and not is_sparse([[1.0]])


def test_sparse_layers_pass_validation():
    """_assignment_arguments and _start_layers read .shape: a sparse layer is neither converted nor measured with len()."""
    from spateo_amd import align

    rng = np.random.default_rng(0)
    A, B = sp.random(9, 5, 0.5, format="csr", random_state=1), sp.random(7, 5, 0.5, format="coo", random_state=2)
    XA, XB, LA, LB, codes, _ = align._assignment_arguments(rng.random((9, 3)), rng.random((7, 3)), [A], [B], ["kl"], ["gauss"], [0.1],
                                                           False)
    assert sp.issparse(LA[0]) and LB[0].format == "csr" and codes[0][0] == 2
    with pytest.raises(ValueError, match="one row per cell"):
        align._assignment_arguments(rng.random((8, 3)), rng.random((7, 3)), [A], [B], ["kl"], ["gauss"], [0.1], False)
    with pytest.raises(AssertionError, match="same number of features"):
        align._assignment_arguments(rng.random((9, 3)), rng.random((7, 3)), [A], [B.tocsr()[:, :4]], ["kl"], ["gauss"], [0.1], False)
    LA, LB, codes, _, params, estimate = align._start_layers([A], [B], ["kl"], ["gauss"], None, None, "morpho_start")
    assert sp.issparse(LA[0]) and estimate == [0]
    # the voxel means of the coarse stage from a sparse layer: a sparse product, the dense result's bits
    coords = rng.random((200, 2))
    dense = rng.poisson(0.3, (200, 11)).astype(np.float64)
    v1, g1 = align._voxel_data(coords, dense, 100)
    v2, g2 = align._voxel_data(coords, sp.csr_matrix(dense), 100)
    assert np.array_equal(v1, v2) and np.array_equal(g1, g2) and isinstance(g2, np.ndarray)


def test_anndata_lite_keeps_sparse_matrices():
    from spateo_amd import AnnDataLite

    X = sp.random(6, 4, 0.5, format="csr", random_state=0)
    a = AnnDataLite(X=X, layers={"l": X.tocoo()}, var_names=list("wxyz"), var={"highly_variable": [True, False, True, True]})
    assert a.X is X and sp.issparse(a.layers["l"]) and a.n_obs == 6
    b = a.copy()
    assert sp.issparse(b.X) and b.X is not X and np.array_equal(b.X.toarray(), X.toarray())
    c = a.select_vars(["z", "w"])
    assert sp.issparse(c.X) and c.X.format == "csr" and np.array_equal(c.X.toarray(), X.toarray()[:, [3, 0]])
    assert c.var_names == ["z", "w"] and c.var["highly_variable"].tolist() == [True, True] and c.layers["l"].shape == (6, 2)
    with pytest.raises(KeyError, match="genes not in var_names"):
        a.select_vars(["q"])
    d = AnnDataLite(X=np.arange(6.0).reshape(3, 2))                      # a dense X as before
    assert isinstance(d.X, np.ndarray) and d.var_names == ["0", "1"] and d.n_obs == 3


# ---- return_P of the loops ----
def test_return_P_arguments(monkeypatch):
    from spateo_amd import align

    rng = np.random.default_rng(0)
    XA, XB = rng.random((12, 2)), rng.random((9, 2))
    LA, LB = rng.random((12, 4)), rng.random((9, 4))
    kw = dict(dissimilarity="kl", probability_type="gauss", probability_parameters=0.1, inducing_variables=XA[:4], beta=1.0,
              lambdaVF=1.0, sigma2=0.1, max_iter=2)
    with pytest.raises(ValueError, match="exclude each other"):
        align.morpho_iterate(XA, XB, LA, LB, return_P=True, sparse_calculation_mode=True, sparse_top_k=4, **kw)
    with pytest.raises(ValueError, match="exclude each other"):
        align.morpho_iterate_svi(XA, XB, LA, LB, return_P=True, sparse_calculation_mode=True, sparse_top_k=4, **kw)
    monkeypatch.setattr(align, "RETURN_P_MAX_ENTRIES", 12 * 9 - 1)
    with pytest.raises(ValueError, match="return_P=True materialises 12 x 9"):
        align.morpho_iterate(XA, XB, LA, LB, return_P=True, **kw)
    with pytest.raises(ValueError, match="return_P=True materialises 12 x 9"):
        align.morpho_iterate_svi(XA, XB, LA, LB, return_P=True, return_mapping=True, batch_size=3, **kw)
    assert align._return_P_argument(True, None, 12, 3) is True        # the SVI batch alone fits
    assert align._return_P_argument(False, 4, 12, 9) is False
    # the class: above the cap P is not asked for (run() then warns and returns None)
    m = _model("1")
    monkeypatch.setattr(align, "RETURN_P_MAX_ENTRIES", m.NA * m.NB)
    assert m._P_fits()
    monkeypatch.setattr(align, "RETURN_P_MAX_ENTRIES", m.NA * m.NB - 1)
    assert not m._P_fits()
    svi = _model("2")                                                   # SVI without return_mapping: NA x batch_size
    monkeypatch.setattr(align, "RETURN_P_MAX_ENTRIES", svi.NA * 150)
    assert svi._P_fits()
