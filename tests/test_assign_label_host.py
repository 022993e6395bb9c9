"""Host tests (no GPU) of the ``"label"`` layer of the alignment: the validation of ``update_assignment`` / ``morpho_iterate`` /
``morpho_iterate_svi``, ``label_transfer_matrix`` against values recorded from the reference's ``check_label_transfer``, and
the NumPy restatement of tests/_assign_label_case.py against the goldens of the real ``_update_assignment_P``
(tests/golden/make_golden_assign_label.py) at 1e-12, the project's figure for its reference proofs."""
import numpy as np
import pytest

import _assign_case as ac
import _assign_label_case as lab
import _assign_topk_case as tk

REF_TOL = 1e-12
G = lab.load()


# ---- the restatement against the real reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", lab.case_tags(G))
def test_restatement_against_the_goldens(tag):
    args, kw = lab.case_inputs(G, tag)
    got = lab.restatement(*args, return_P=tag == "a", **kw)
    ac.check(got, lab.golden_ref(G, tag), {q: REF_TOL for q in lab.QUANTITIES}, f"restatement {tag}")
    far = lab.far_columns(G, tag)
    assert np.all(got["K_NB"][far] == 0.0)
    if tag == "a":
        assert got["P"].shape == (149, 117) and G["a_label_transfer"].shape == (5, 4)
        assert np.abs(got["P"] - G["a_P"]).max() <= REF_TOL * G["a_P"].max()


def test_a_transposed_or_reordered_lookup_would_show():
    """The step cases tell T from its transpose (where that can be read at all) and the label layer from its absence."""
    args, kw = lab.case_inputs(G, "b")
    ref = lab.golden_ref(G, "b")
    T = kw["label_transfer"]
    swapped = lab.restatement(*args, **dict(kw, label_transfer=np.ascontiguousarray(T.T).reshape(T.shape)))   # T^T's memory read as K x L
    assert ac.deviations(swapped, ref)["K_NA"] > 1e-3
    without = lab.restatement(args[0], args[1], args[2][:1], args[3][:1], **dict(
        kw, dissimilarity=kw["dissimilarity"][:1], probability_type=kw["probability_type"][:1],
        probability_parameters=kw["probability_parameters"][:1]))
    assert ac.deviations(without, ref)["K_NA"] > 1e-3


def test_columns_without_any_transfer_are_exactly_zero():
    args, kw = lab.case_inputs(G, "z")
    got = lab.restatement(*args, return_P=True, **kw)
    dead, rare = G["z_dead_columns"], G["z_rare_columns"]
    assert len(dead) and np.all(got["P"][:, dead] == 0.0) and np.all(got["K_NB"][dead] == 0.0)
    assert np.all(G["z_K_NB"][dead] == 0.0)                       # ... and so says the reference
    positives = (got["P"][:, rare] > 0).sum(0)
    assert len(rare) and positives.max() < 64 and positives.min() >= 1


@pytest.mark.parametrize("k", [int(k) for k in G["z_ks"]])
def test_masked_restatement_against_the_sparse_goldens(k):
    args, kw = lab.case_inputs(G, "z")
    d = lab.restatement(*args, return_P=True, **kw)
    rows, vals = tk.top_lists(d["P"], k)
    NB = len(args[1])
    grow, gval = G[f"z_k{k}_row"].reshape(NB, k).astype(np.int32), G[f"z_k{k}_data"].reshape(NB, k)
    assert np.abs(vals - gval).max() <= REF_TOL * gval.max()
    decided = (gval > 0) & (G[f"z_k{k}_colgap"] > 0)[:, None]       # zeros tie exactly: the reference's sort is free there
    assert decided.any() and np.array_equal(rows[decided], grow[decided])
    sums = tk.masked_sums(d["P"], rows, np.asarray(args[1], dtype=np.float64))
    for q in tk.SUMS:
        assert np.abs(sums[q] - G[f"z_k{k}_{q}"]).max() <= REF_TOL * np.abs(G[f"z_k{k}_{q}"]).max(), q


# ---- label_transfer_matrix ---------------------------------------------------------------------------------------------------
def test_label_transfer_matrix_against_the_recorded_reference_values():
    from spateo_amd import align

    catA, catB = [str(c) for c in G["lt_catA"]], [str(c) for c in G["lt_catB"]]
    T = align.label_transfer_matrix(catA, catB)
    assert T.dtype == np.float64 and T.shape == (5, 4) and np.array_equal(T, G["lt_default"])
    assert np.array_equal(T, T.astype(np.float32))                  # the reference's float32 rounding
    assert T[1, 0] > T[1, 1] and T[0].min() == T[0].max()           # "T cell" -> "T cell"; "B cell" has no partner
    given = {ca: {cb: float(G["lt_given_values"][i, j]) for j, cb in enumerate(catB)} for i, ca in enumerate(catA)}
    assert np.array_equal(align.label_transfer_matrix(catA, catB, given), G["lt_given"])
    with pytest.raises(ValueError, match="label_transfer_dict should be"):
        align.label_transfer_matrix(catA, catB, [given])
    with pytest.raises(KeyError):
        align.label_transfer_matrix(catA + ["other"], catB, given)


# ---- validation (nothing here reaches a device) --------------------------------------------------------------------------------
def _call(fn, **changes):
    from spateo_amd import align

    args, kw = lab.case_inputs(G, "b")
    XA, XB, LA, LB = args
    LA, LB = list(LA), list(LB)
    kw = dict(kw)
    for key, v in changes.items():
        if key == "labels_A":
            LA[1] = v
        elif key == "labels_B":
            LB[1] = v
        else:
            kw[key] = v
    if fn == "update_assignment":
        return align.update_assignment(XA, XB, LA, LB, device="cuda:0", **kw)
    for q in ("alpha", "SigmaDiag", "gamma", "sigma2_variance"):
        kw.pop(q)
    kw.update(inducing_variables=XA[:8], beta=0.5, lambdaVF=1.0, max_iter=2)
    return getattr(align, fn)(XA, XB, LA, LB, device="cuda:0", **kw)


@pytest.mark.parametrize("fn", ["update_assignment", "morpho_iterate", "morpho_iterate_svi"])
def test_validation_errors(fn):
    _, kw = lab.case_inputs(G, "b")
    args = lab.case_inputs(G, "b")[0]
    labA, labB, T = np.asarray(args[2][1]), np.asarray(args[3][1]), kw["label_transfer"]
    with pytest.raises(AssertionError, match="label_transfer must be provided"):
        _call(fn, label_transfer=None)
    with pytest.raises(AssertionError, match="should contain integer values"):
        _call(fn, labels_A=labA.astype(np.float64))
    with pytest.raises(AssertionError, match="should contain integer values"):
        _call(fn, labels_B=labB.astype(np.float32))
    with pytest.raises(AssertionError, match="X should be a 1-dimensional array"):
        _call(fn, labels_A=labA[:, None])
    with pytest.raises(AssertionError, match="Y should be a 1-dimensional array"):
        _call(fn, labels_B=labB[None, :])
    with pytest.raises(ValueError, match="one row per cell"):
        _call(fn, labels_A=labA[:-1])
    with pytest.raises(ValueError, match="one row per cell"):
        _call(fn, labels_B=np.concatenate([labB, labB[:1]]))
    bad = labA.copy()
    bad[3] = T.shape[0]
    with pytest.raises(ValueError, match="A labels must lie in 0 .. 4"):
        _call(fn, labels_A=bad)
    bad[3] = -1
    with pytest.raises(ValueError, match="A labels must lie in"):
        _call(fn, labels_A=bad)
    bad = labB.copy()
    bad[0] = T.shape[1]
    with pytest.raises(ValueError, match="B labels must lie in 0 .. 3"):
        _call(fn, labels_B=bad)
    with pytest.raises(ValueError, match="B labels must lie in"):
        _call(fn, label_transfer=T[:, :3])              # a table too narrow for the labels that occur
    with pytest.raises(ValueError, match="finite 2-D"):
        _call(fn, label_transfer=T.reshape(-1))
    with pytest.raises(ValueError, match="finite 2-D"):
        _call(fn, label_transfer=np.where(T == T[0, 0], np.nan, T))
    with pytest.raises(ValueError, match="finite 2-D"):
        _call(fn, label_transfer=np.zeros((0, 4)))
    with pytest.raises(ValueError, match="probability_parameter must be provided"):
        _call(fn, probability_type=["gauss", "gauss"], probability_parameters=[0.05, None])
    with pytest.raises(ValueError, match="Unsupported dissimilarity metric"):
        _call(fn, dissimilarity=["kl", "labels"])


def test_the_codes_of_a_label_layer():
    from spateo_amd import _lib, align

    args, kw = lab.case_inputs(G, "c")
    XA, XB, LA, LB, codes, T = align._assignment_arguments(*args, kw["dissimilarity"], kw["probability_type"],
                                                           kw["probability_parameters"], False, kw["label_transfer"])
    assert codes[0] == (_lib.ASSIGN_LABEL, 2, 0.0) and codes[1][0] == _lib.ASSIGN_METRICS["kl"] and _lib.ASSIGN_LABEL == 5
    assert LA[0].dtype == np.int64 and LA[0].shape == (len(XA),) and LB[0].shape == (len(XB),) and LA[1].dtype == np.float64
    assert T.dtype == np.float64 and T.flags.c_contiguous and T.shape == (5, 4)
    # without a label layer the table is not needed and, when given, not looked at beyond its shape
    a2, kw2 = lab.case_inputs(G, "b")
    out = align._assignment_arguments(a2[0], a2[1], a2[2][:1], a2[3][:1], ["kl"], ["gauss"], [0.05], False, None)
    assert out[5] is None
