"""CPU tests of the alignment's assignment step (``spateo_amd.align.update_assignment``, ``mvf_assign*``): the NumPy
restatement the GPU suite compares large cases with is pinned to goldens of the real ``_update_assignment_P``
(tests/golden/make_golden_assign.py); argument validation and every refusal of the public function; the identities
that connect its outputs to the other updates; the C ABI's symbols and its no-launch paths."""
import ctypes

import numpy as np
import pytest

import _assign_case as ac


@pytest.fixture(scope="module")
def g():
    return ac.load()


def test_restatement_reproduces_the_reference_goldens(g):
    """Same arithmetic, same precision: 1e-12 relative to each quantity's maximum (the reference's own chunked run sits
    <= 1.5e-15 from its dense run: what its reorderings cost)."""
    assert len(ac.case_tags(g)) >= 5
    for tag in ac.case_tags(g):
        args, kw = ac.case_inputs(g, tag)
        for chunk in (None, 100):
            dev = ac.deviations(ac.restatement(*args, chunk=chunk, **kw), ac.golden_ref(g, tag))
            assert max(dev.values()) <= 1e-12, (tag, chunk, dev)
        assert float(g[f"{tag}_floor_chunk"].max()) <= 1e-14
    args, kw = ac.case_inputs(g, "p")
    P = ac.restatement(*args, return_P=True, **kw)["P"]
    assert np.abs(P - g["p_P"]).max() <= 1e-12 * g["p_P"].max()


def test_goldens_cover_the_cases_the_step_is_used_on(g):
    mets = {str(m) for t in ac.case_tags(g) for m in g[f"{t}_dissimilarity"]}
    assert {"kl", "cos", "euc", "sym_kl"} <= mets
    assert any(len(g[f"{t}_dissimilarity"]) == 2 for t in ac.case_tags(g))
    assert any(g[f"{t}_XAHat"].shape[1] == 2 for t in ac.case_tags(g))
    assert any(float(g[f"{t}_sigma2_variance"]) != 1.0 for t in ac.case_tags(g))
    for t in ac.case_tags(g):
        NA, NB = len(g[f"{t}_XAHat"]), len(g[f"{t}_coordsB"])
        assert NA % 16 and NB % 16   # exact tile multiples, 1-cell sides and the split plans: tests/_assign_edge_cases.py
        far = g[f"{t}_far"]
        assert len(far) >= 0.05 * NB and np.all(g[f"{t}_K_NB"][far] == 0.0)  # columns whose terms all underflow: exactly 0
        assert all(np.isfinite(g[f"{t}_{q}"]).all() for q in ac.QUANTITIES)


def test_identities_between_the_outputs(g):
    """K_NB.sum() == Sp; XA_hat^T P XB_hat (what _update_rigid needs) from PXB and K_NA alone."""
    args, kw = ac.case_inputs(g, "p")
    r = ac.restatement(*args, return_P=True, **kw)
    XA, XB, P = args[0], args[1], g["p_P"]
    assert abs(g["p_K_NB"].sum() - float(g["p_Sp"])) <= 1e-12 * float(g["p_Sp"])
    assert abs(g["p_K_NA"].sum() - float(g["p_Sp"])) <= 1e-12 * float(g["p_Sp"])
    mu_XB = XB.T @ g["p_K_NB"] / float(g["p_Sp"])
    mu_XA = XA.T @ g["p_K_NA"] / float(g["p_Sp"])
    dense = (XA - mu_XA).T @ P @ (XB - mu_XB)
    fused = (XA - mu_XA).T @ r["PXB"] - np.outer((XA - mu_XA).T @ r["K_NA"], mu_XB)
    assert np.abs(fused - dense).max() <= 1e-12 * np.abs(dense).max()


def _call(**over):
    from spateo_amd import align

    rng = np.random.default_rng(0)
    kw = dict(XAHat=rng.standard_normal((20, 3)), coordsB=rng.standard_normal((15, 3)),
              exp_layers_A=[rng.random((20, 7))], exp_layers_B=[rng.random((15, 7))], dissimilarity=["kl"],
              probability_type=["gauss"], probability_parameters=[0.1], sigma2=0.1, alpha=np.ones(20),
              SigmaDiag=np.zeros(20), gamma=0.5, samples_s=1.0)
    kw.update(over)
    pos = [kw.pop(k) for k in ("XAHat", "coordsB", "exp_layers_A", "exp_layers_B")]
    return align.update_assignment(*pos, **kw)


def test_refusals_name_their_reason():
    rng = np.random.default_rng(1)
    from spateo_amd import align

    assert "update_assignment" in align.__all__
    with pytest.raises(NotImplementedError, match="label"):
        _call(dissimilarity=["label"])
    with pytest.raises(NotImplementedError, match="sparse_calculation_mode"):
        _call(sparse_calculation_mode=True)
    with pytest.raises(NotImplementedError, match="at most 4 layers"):
        _call(exp_layers_A=[rng.random((20, 7))] * 5, exp_layers_B=[rng.random((15, 7))] * 5, dissimilarity=["kl"] * 5,
              probability_type=["gauss"] * 5, probability_parameters=[0.1] * 5)
    for D in (1, 4):
        with pytest.raises(NotImplementedError, match="2-D or 3-D"):
            _call(XAHat=rng.random((20, D)), coordsB=rng.random((15, D)))
    with pytest.raises(ValueError, match="probability_parameter must be provided for 'Gauss' probability type."):
        _call(probability_parameters=None)
    with pytest.raises(ValueError, match="probability_parameter must be provided"):
        _call(probability_parameters=[None])
    with pytest.raises(AssertionError, match="X and Y do not have the same number of features."):
        _call(exp_layers_B=[rng.random((15, 8))])
    with pytest.raises(AssertionError, match="X and Y do not have the same number of features."):
        _call(coordsB=rng.random((15, 2)))
    with pytest.raises(ValueError, match="Unsupported probability type"):
        _call(probability_type=["laplace"])
    with pytest.raises(ValueError, match="Unsupported dissimilarity"):
        _call(dissimilarity=["jaccard"])
    with pytest.raises(ValueError, match="dtype"):
        _call(dtype="float16")
    with pytest.raises(ValueError, match="one row per cell"):
        _call(exp_layers_A=[rng.random((19, 7))])
    with pytest.raises(ValueError, match=r"alpha and SigmaDiag must be \(NA,\)"):
        _call(alpha=np.ones(19))
    with pytest.raises(ValueError, match="same .* number of layers"):
        _call(dissimilarity=["kl", "cos"])
    big = np.zeros((align.RETURN_P_MAX_ENTRIES // 1024 + 1, 3))
    with pytest.raises(ValueError, match="return_P=True materialises"):
        _call(XAHat=big, coordsB=np.zeros((1024, 3)), exp_layers_A=[np.zeros((len(big), 2))],
              exp_layers_B=[np.zeros((1024, 2))], alpha=np.ones(len(big)), SigmaDiag=np.zeros(len(big)), return_P=True)


def test_empty_slices_return_zeros_without_a_device():
    r = _call(coordsB=np.zeros((0, 3)), exp_layers_B=[np.zeros((0, 7))], return_P=True)
    assert r["K_NA"].shape == (20,) and r["K_NB"].shape == (0,) and r["PXB"].shape == (20, 3) and r["P"].shape == (20, 0)
    assert r["Sp"] == 0.0 and not r["K_NA"].any()


def test_c_abi_symbols_and_no_launch_paths():
    from spateo_amd import _lib

    lib = _lib.load()
    for name in ("mvf_assign_padded_features", "mvf_assign_prepare", "mvf_assign_workspace_bytes", "mvf_assign",
                 "mvf_assign_dense"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.mvf_version() == 7
    # padded feature counts: multiples of 16; sym_kl carries 2 g features
    assert [lib.mvf_assign_padded_features(g_, 2) for g_ in (1, 16, 17, 50, 2000)] == [16, 16, 32, 64, 2000]
    assert lib.mvf_assign_padded_features(24, 3) == 48 and lib.mvf_assign_padded_features(0, 2) == 0
    assert lib.mvf_assign_padded_features(24, 9) == 0
    # zero sizes return 0 and touch nothing
    assert lib.mvf_assign_workspace_bytes(0, 10) == 0 and lib.mvf_assign_workspace_bytes(10, 0) == 0
    assert lib.mvf_assign_prepare(None, 0, 5, 2, 0, None, 16, None, _lib.MVF_F64, None) == 0
    tail = (None, 0, _lib.MVF_F64, None)
    assert lib.mvf_assign(None, 0, None, 5, None, 1, None, 0.1, 1.0, 0.0, None, None, None, None, None, None, *tail) == 0
    assert lib.mvf_assign_dense(None, 5, None, 0, None, 1, None, 0.1, 1.0, 0.0, None, None, None, None, None, None, None,
                                *tail) == 0
    # the workspace holds the split partials: pass 1 rsplit x 4 x nb_pad, factors 4 x nb_pad, pass 2 csplit x na_pad x 8, na_pad
    ws = lib.mvf_assign_workspace_bytes(600, 450)  # 10 x 8 tiles: 10 row splits, 8 column splits
    assert ws == 8 * (10 * 4 * 512 + 4 * 512 + 8 * 640 * 8 + 640)
    big = lib.mvf_assign_workspace_bytes(100_000, 100_000)  # 1563 tiles each way: one split
    assert big == 8 * (4 * 100_032 + 4 * 100_032 + 100_032 * 8 + 100_032)
    # refusals report through the status + mvf_last_error channel before any HIP call
    p = ctypes.c_void_p(256)
    lay = (_lib.AssignLayer * 1)()
    lay[0].Xp = lay[0].Yp = lay[0].a = lay[0].b = 256
    lay[0].ld, lay[0].metric, lay[0].prob, lay[0].param = 16, 2, 0, 0.1

    def run(na=600, nb=450, layers=lay, nl=1, sigma2=0.1, ws_bytes=ws, dtype=_lib.MVF_F64, mm=p):
        return lib.mvf_assign(p, na, p, nb, layers, nl, mm, sigma2, 1.0, 0.0, p, p, p, p, p, p, p, ws_bytes, dtype, None)

    for kw, msg in ((dict(ws_bytes=ws - 1), b"workspace too small"), (dict(dtype=7), b"bad dtype"), (dict(nl=0), b"layers"),
                    (dict(nl=5), b"layers"), (dict(mm=None), b"null pointer"), (dict(sigma2=0.0), b"sigma2 > 0"),
                    (dict(na=-1), b"negative size"), (dict(layers=None), b"null pointer")):
        assert run(**kw) != 0 and msg in lib.mvf_last_error() and b"mvf_assign" in lib.mvf_last_error(), (kw, lib.mvf_last_error())
    for field, val, msg in (("ld", 24, b"multiple of 16"), ("metric", 5, b"bad metric"), ("prob", 3, b"bad probability type"),
                            ("param", 0.0, b"gauss layer needs a parameter"), ("a", None, b"null pointer in layer 0")):
        old = getattr(lay[0], field)
        setattr(lay[0], field, val)
        assert run() != 0 and msg in lib.mvf_last_error(), (field, lib.mvf_last_error())
        setattr(lay[0], field, old)
    assert lib.mvf_assign_prepare(p, 10, 5, 2, 0, p, 24, p, _lib.MVF_F64, None) != 0 and b"ld must be" in lib.mvf_last_error()
    assert lib.mvf_assign_prepare(p, 10, 5, 7, 0, p, 16, p, _lib.MVF_F64, None) != 0 and b"bad metric" in lib.mvf_last_error()
    assert lib.mvf_assign_prepare(p, 10, 5, 2, 2, p, 16, p, _lib.MVF_F64, None) != 0 and b"side" in lib.mvf_last_error()


def test_layer_record_and_layer_array():
    """`Layer` and `layer_array` (spateo_amd._kernels) on host tensors: every field of mvf_assign_layer set from a record and
    from a plain 8-sequence, NULL for a label layer's Yp, max(n, 1) entries; exchanged() and with_columns() against the tuple
    expressions they replace, field by field on objects with distinct identities."""
    import torch

    from spateo_amd import _lib
    from spateo_amd._kernels import Layer, layer_array

    Xp, Yp, a, b, T, la, lb, Y2, b2 = (torch.zeros(4, dtype=torch.float64) for _ in range(9))
    assert len({t.data_ptr() for t in (Xp, Yp, a, b, T, la, lb, Y2, b2)}) == 9
    product = Layer(Xp, Yp, a, b, 16, _lib.ASSIGN_METRICS["kl"], _lib.ASSIGN_PROBS["gauss"], 0.25)
    label = Layer(T, None, la, lb, 3, _lib.ASSIGN_LABEL, _lib.ASSIGN_PROBS["prob"], 0.0)
    assert Layer._fields == ("Xp", "Yp", "a", "b", "ld", "metric", "prob", "param")
    assert label.is_label and not product.is_label
    for layers in ([product, label], [tuple(product), tuple(label)]):
        arr = layer_array(layers)
        assert len(arr) == 2 and isinstance(arr[0], _lib.AssignLayer)
        for s, L in zip(arr, (product, label)):
            assert (s.Xp, s.a, s.b) == (L.Xp.data_ptr(), L.a.data_ptr(), L.b.data_ptr())
            assert s.Yp == (None if L.Yp is None else L.Yp.data_ptr())
            assert (s.ld, s.metric, s.prob, s.param) == (L.ld, L.metric, L.prob, L.param)
    assert len(layer_array([])) == 1 and len(layer_array([product])) == 1
    p0, p1, p2, p3, ld, metric, prob, param = product
    for got, want in ((product.exchanged(), (p1, p0, p3, p2, ld, metric, prob, param)),
                      (product.with_columns(Y2, b2), (product[0], Y2, product[2], b2) + tuple(product[4:])),
                      (label.with_columns(None, b2), (label[0], None, label[2], b2) + tuple(label[4:]))):
        assert isinstance(got, Layer) and len(got) == len(want) == 8
        for x, y in zip(got, want):
            assert x is y if torch.is_tensor(y) or y is None else x == y
