"""Kernel-level edge tests of the label branch of the fused assignment step (``csrc/mvf_assign.hip``) through the raw C ABI -
``mvf_assign_label_prepare``, ``mvf_assign``, ``mvf_assign_dense``, ``mvf_assign_topk``, ``mvf_align_gather`` - on ``cuda:0`` in
both cell dtypes, against the NumPy restatement of tests/_assign_label_case.py fed with the coordinates as the cell dtype
stores them (the look-up and every sum are float64 in both modes, so both are held to 1e-10, ``_assign_case.F64_TOL``).

Shapes (NA x NB; K x L): 1 x 1 (1 x 1), 63 x 65 (5 x 4), 64 x 64 (K = 1), 65 x 129 (L = 1) and 65 x 129 (7 x 9) - the tile
edges, tables of one row and of one column, and in the last two the smallest sizes at which both passes split their work
(``_assign_edge_cases.plan``).  Every case draws the last row and the last column of its table.  Every output sits in front of
a guard, the workspace is filled with NaN bit patterns, and every call is made twice: the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import _assign_case as ac
import _assign_edge_cases as ec
import _assign_label_case as lab
import _assign_topk_case as tk
from _align_kernel_scaffold import LABEL, PROBS, label_prepare as _label_prepare, LabelCase as _Case
from _kernel_scaffold import DTYPES, dev as _dev, guarded as _guarded, intact as _intact

pytestmark = pytest.mark.gpu


def _compare(case, out, what):
    ref, D = case.ref, case.XA.shape[1]
    dev = {}
    for q in ("K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2"):
        dev[q] = float(np.abs(out[q] - ref[q]).max() / np.abs(ref[q]).max())
    dev["PXB"] = float(np.abs(out["PXB"][:, :D] - ref["PXB"]).max() / np.abs(ref["PXB"]).max())
    raw = ref["sigma2_related"] * D * ref["Sp_sigma2"]
    dev["scalar"] = float(abs(out["scalar"][0] - raw) / abs(raw))
    print(f"  {what}: " + ", ".join(f"{q} {v:.2e}" for q, v in dev.items()))
    for q, v in dev.items():
        assert v <= ac.F64_TOL, (what, q, v)
    assert not out["PXB"][:, D:].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", lab.EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_label_branch_at_the_tile_and_table_edges(shape, dtype):
    NA, NB, K, L = shape
    if (NA, NB) == (65, 129):
        rt, ct, rs, cs = ec.plan(NA, NB)
        assert rs > 1 and cs > 1 and ec.plan(64, 129)[2] == 1 and ec.plan(65, 64)[3] == 1   # the smallest sizes that split both passes
    for expression in (True, False):
        case = _Case(shape, dtype, expression)
        c = case.c
        assert c["layers_A"][-1].max() == K - 1 and c["layers_B"][-1].max() == L - 1
        what = f"{NA} x {NB}, table {K} x {L}, {'euc + label' if expression else 'label alone'}, {dtype}"
        _, plain = case.call()
        _compare(case, plain, what)
        _, dense = case.call("dense")
        _compare(case, dense, what + " (dense)")
        assert np.abs(dense["P"] - case.ref["P"]).max() <= ac.F64_TOL * case.ref["P"].max()
        _, again = case.call()
        for q in plain:
            assert plain[q].tobytes() == again[q].tobytes() == dense[q].tobytes(), q


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,par", [("gauss", 0.25), ("cos", None)])
def test_probability_types_on_a_label_layer(kind, par, dtype):
    """gauss and cos on the look-up, with the label layer FIRST."""
    case = _Case((63, 65, 5, 4), dtype)
    c = case.c
    order = [1, 0]
    for key in ("layers_A", "layers_B", "dissimilarity", "probability_type", "probability_parameters"):
        c[key] = [c[key][i] for i in order]
    c["probability_type"][0], c["probability_parameters"][0] = kind, par
    T, _, a, b, L, _, _, _ = case.layers[1]
    layers = [(T, None, a, b, L, LABEL, PROBS[kind], 0.0 if par is None else par), case.layers[0]]
    Xp, Yp = case.layers[0][0], case.layers[0][1]
    g = c["layers_A"][1].shape[1]
    case.ref = lab.restatement(case.XA, case.XB, [c["layers_A"][0], Xp.double().cpu().numpy()[:, :g]],
                               [c["layers_B"][0], Yp.double().cpu().numpy()[:, :g]], dissimilarity=c["dissimilarity"],
                               probability_type=c["probability_type"], probability_parameters=c["probability_parameters"],
                               sigma2=c["sigma2"], alpha=None, SigmaDiag=None, gamma=None, samples_s=None,
                               sigma2_variance=c["sigma2_variance"], label_transfer=c["label_transfer"], return_P=True,
                               model_mul=case.mm_host, outlier=case.outlier)
    _, out = case.call(layers=layers)
    _compare(case, out, f"label ({kind}) + euc, {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 8, 64])
def test_top_k_through_the_raw_abi(k, dtype):
    case = _Case((65, 129, 7, 9), dtype)
    _, out = case.call("topk", k)
    tk.check(out, case.ref["P"], case.XB, k, ac.F64_TOL, what=f"65 x 129 k {k} {dtype}")
    _, again = case.call("topk", k)
    for q in out:
        assert out[q].tobytes() == again[q].tobytes(), q


def test_malformed_label_layers_are_rejected():
    """Null pointers and ld < 1 in the four entry points that take the layer, classes < 1 in the preparation: the error code
    and message style of the neighbouring checks, nothing launched."""
    case = _Case((63, 65, 5, 4), "float64", expression=False)
    k, lib = case.k, case.k.lib
    T, _, a, b, L, metric, prob, param = case.layers[0]
    bad = {"a null table": (None, None, a, b, L), "null A labels": (T, None, None, b, L), "null B labels": (T, None, a, None, L),
           "L = 0": (T, None, a, b, 0), "L < 0": (T, None, a, b, -4), "Yp set: a product layer with the label code": (T, T, a, b, L)}
    for mode, kk in (("plain", 0), ("dense", 0), ("topk", 8)):
        for what, (t_, y_, a_, b_, l_) in bad.items():
            status, _ = case.call(mode, kk, layers=[(t_, y_, a_, b_, l_, metric, prob, param)])
            msg = lib.mvf_last_error().decode()
            assert status != 0 and ("null pointer in layer 0" in msg or "ld" in msg or "bad metric 5" in msg), (mode, what, status, msg)
        status, _ = case.call(mode, kk, layers=[(T, None, a, b, L, 6, prob, param)])
        assert status != 0 and "bad metric" in lib.mvf_last_error().decode()
        status, _ = case.call(mode, kk, layers=[(T, None, a, b, L, metric, 0, 0.0)])   # gauss on a label layer needs its parameter
        assert status != 0 and "gauss" in lib.mvf_last_error().decode()
    # mvf_align_gather: b and b_out are needed, Yp / Yp_out are not read
    nb, bs = case.nb, 16
    perm = _dev(np.random.default_rng(0).permutation(nb), torch.int32)
    xb4_out, B, B_out, b_out = k.empty(bs, 4), k.zeros(nb, 3, dtype=torch.float64), k.empty(bs, 3, dtype=torch.float64), _guarded(bs)
    vp = ctypes.c_void_p * 1

    def gather(layer, bo):
        return lib.mvf_align_gather(perm.data_ptr(), nb, 3, bs, case.xb4.data_ptr(), xb4_out.data_ptr(), B.data_ptr(),
                                    B_out.data_ptr(), case.struct([layer]), 1, vp(None), vp(bo), k.cdtype, k._stream())

    assert gather(case.layers[0], b_out.data_ptr()) == 0
    torch.cuda.synchronize()
    idx = perm.cpu().numpy()[(3 + np.arange(bs)) % nb]
    assert np.array_equal(b_out[:bs].cpu().numpy(), c_labels(case)[idx]) and _intact(b_out, bs)
    assert gather((T, None, a, None, L, metric, prob, param), b_out.data_ptr()) != 0 and b"null pointer" in lib.mvf_last_error()
    assert gather(case.layers[0], None) != 0 and b"null pointer" in lib.mvf_last_error()
    assert gather((T, None, a, b, 0, metric, prob, param), b_out.data_ptr()) != 0 and b"ld" in lib.mvf_last_error()
    # the preparation
    lab32 = _dev(np.zeros(8), torch.int32)
    out = _guarded(8)
    assert lib.mvf_assign_label_prepare(lab32.data_ptr(), 8, 0, out.data_ptr(), None) != 0 and b"classes" in lib.mvf_last_error()
    assert lib.mvf_assign_label_prepare(None, 8, 3, out.data_ptr(), None) != 0 and b"null pointer" in lib.mvf_last_error()
    assert lib.mvf_assign_label_prepare(lab32.data_ptr(), 8, 3, None, None) != 0
    assert lib.mvf_assign_label_prepare(None, 0, 3, None, None) == 0                     # n == 0 launches nothing
    assert lib.mvf_assign_padded_features(7, LABEL) == 0                                  # a label layer has no prepared rows
    # labels outside the table are clamped into it: the look-up cannot leave the table
    wild = _label_prepare(k, np.array([-3, 0, 2, 3, 99]), 3)
    assert np.array_equal(wild.cpu().numpy(), [0.0, 0.0, 2.0, 2.0, 2.0])


def c_labels(case):
    return np.asarray(case.c["layers_B"][-1], dtype=np.float64)
