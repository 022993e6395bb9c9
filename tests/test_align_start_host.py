"""The alignment's start state without a GPU: the NumPy restatement of ``tests/_align_start_case.py`` against the goldens the
reference itself wrote (``tests/golden/ref_align_start.npz``), two wrong variants of it that the goldens must reject, the
host logic of ``spateo_amd.align.init_sigma2`` / ``init_probability_parameters`` / ``coarse_rigid_alignment`` / ``morpho_start``
through the kernel seam (``_runtime._make_kernels`` replaced by the restatement of the kernel), their validation before any
device is touched, the public names, and the C ABI of ``mvf_assign_layer_stats``: exported, every argument error returned as
a status before a launch."""
import ctypes

import numpy as np
import pytest

import _align_start_case as sc
import _assign_case as ac
import _assign_edge_cases as ec

G = sc.load()
TAGS = sc.case_tags(G)
NAMES = {v: k for k, v in ec.METRICS.items()}


# ---- the goldens and the restatement ------------------------------------------------------------------------------------------
def test_goldens_cover_what_the_issue_names():
    assert TAGS == ["1", "2", "3", "4"]
    c = {t: sc.case_inputs(G, t) for t in TAGS}
    assert c["1"]["coordsA"].shape[1] == 3 and len(c["1"]["subsample_A"]) < len(c["1"]["coordsA"])        # a draw on both sides
    assert len(c["1"]["subsample_B"]) < len(c["1"]["coordsB"]) and c["1"]["dissimilarity"] == ["kl"]
    assert c["2"]["coordsA"].shape[1] == 2 and sorted(c["2"]["dissimilarity"]) == ["cos", "euc"]
    assert len(c["2"]["subsample_A"]) == len(c["2"]["coordsA"]) != len(c["2"]["coordsB"]) == len(c["2"]["subsample_B"])
    assert sum(p is None for p in c["2"]["probability_parameters"]) == 1
    assert c["3"]["allow_flip"] and bool(G["3_flipped"]) and np.linalg.det(G["3_init_R"]) < 0
    assert not any(bool(G[f"{t}_flipped"]) for t in "124")
    assert 0.01 in G["4_parameters"] and all(np.all(G[f"{t}_parameters"] > 0.01) for t in "123")
    for t in TAGS:
        assert np.linalg.norm(G[f"{t}_init_R"] - G[f"{t}_R0"]) <= 0.05
        assert all(float(G[f"{t}_g_{q}"]) <= 100.0 for q in sc.QUANTITIES)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference_goldens(tag):
    out = sc.restate_case(sc.case_inputs(G, tag))
    sc.check(out, G, tag, sc.tolerances(G, tag, "float64"), "restatement")
    assert out["flipped"] == bool(G[f"{tag}_flipped"])


@pytest.mark.parametrize("tag,wrong", [(t, "single_square") for t in TAGS] + [("2", "nanb"), ("4", "nanb")])
def test_the_goldens_reject_what_the_reference_does_not_do(tag, wrong):
    """The distance squared once, and the sum over D nA nB (the cases whose sides differ in size after the draw)."""
    c = sc.case_inputs(G, tag)
    assert wrong != "nanb" or len(c["subsample_A"]) != len(c["subsample_B"])
    got = sc.init_sigma2(G[f"{tag}_coordsA"], c["coordsB"], c["subsample_A"], c["subsample_B"], wrong=wrong)
    right = sc.init_sigma2(G[f"{tag}_coordsA"], c["coordsB"], c["subsample_A"], c["subsample_B"])
    ref, tol = float(G[f"{tag}_sigma2"]), sc.tolerances(G, tag, "float64")["sigma2"]
    assert abs(right - ref) <= tol * ref and abs(got - ref) > 1e3 * tol * ref, (got, right, ref)


def test_the_kernel_restatement_orders_ties_by_row_and_masks_nothing_live():
    d = np.array([[3.0, 1.0], [1.0, 1.0], [1.0, 0.5], [2.0, 1.0]])
    st = sc.layer_stats(d, 3)
    assert st["rows"].tolist() == [[1, 2, 3], [2, 0, 1]] and st["vals"].tolist() == [[1.0, 1.0, 2.0], [0.5, 1.0, 1.0]]
    assert st["cmin"].tolist() == [1.0, 0.5] and st["sums"].tolist() == [10.5, 18.25]
    assert sc.layer_stats(d, 64)["rows"].shape == (2, 4) and set(sc.layer_stats(d, 0)) == {"cmin", "sums"}
    assert sc.list_gap(d, 1) == 0.0 and sc.list_gap(np.array([[1.0], [4.0], [2.0]]), 2) == 0.25


# ---- the host logic through the kernel seam -----------------------------------------------------------------------------------
class _SeamKernels:
    """What align's start state asks of HipKernels, stated in NumPy: mvf_assign_prepare (prepare_reference) and
    mvf_assign_layer_stats (layer_stats on the stored operands' distance)."""

    def __init__(self, dtype):
        self.npdt = np.float32 if dtype == "float32" else np.float64
        self.calls = []

    def assign_prepare(self, layer, metric, side):
        Xp, ab = ec.prepare_reference(layer, NAMES[metric], side, self.npdt)
        return Xp, ab, Xp.shape[1]

    def assign_layer_stats(self, layer, na, nb, k=0):
        Xp, Yp, a, b, ld, metric, _, _ = layer
        assert Xp.shape == (na, ld) and Yp.shape == (nb, ld) and a.shape == (na,) and b.shape == (nb,)
        self.calls.append((na, nb, k))
        return sc.layer_stats(sc.stored_distance(Xp, Yp, a, b, NAMES[metric]), k)


def _seam(monkeypatch):
    from spateo_amd import _runtime as rt

    made = []
    monkeypatch.setattr(rt, "_make_kernels", lambda device, dtype: made.append(_SeamKernels(dtype)) or made[-1])
    monkeypatch.setattr(rt, "_to_host", lambda k, tensors: [np.asarray(t) for t in tensors])
    return made


def start_of_case(align, c, dtype, **kw):
    """morpho_start and coarse_rigid_alignment on a golden case with the recorded indices -> the compared quantities."""
    common = dict(nn_init_top_K=c["top_K"], allow_flip=c["allow_flip"], subsample_A=c["subsample_A"], subsample_B=c["subsample_B"],
                  dtype=dtype, **kw)
    st = align.morpho_start(c["coordsA"], c["coordsB"], c["layers_A"], c["layers_B"], dissimilarity=c["dissimilarity"],
                            probability_type=c["probability_type"], probability_parameters=c["probability_parameters"],
                            inducing_variables_num=40, init_metric=c["init_metric"], **common)
    co = align.coarse_rigid_alignment(c["coordsA"], c["coordsB"], c["layers_A"][0], c["layers_B"][0], metric=c["init_metric"], **common)
    for a, b in zip(st["inliers"], co["inliers"]):
        assert np.array_equal(a, b)
    assert np.array_equal(st.coordsA, co["coordsA"]) and np.array_equal(st.init_R, co["init_R"])
    got = dict(sigma2=st["sigma2"], parameters=np.array(st["probability_parameters"], dtype=np.float64), init_R=st.init_R,
               init_t=st.init_t, coordsA=st.coordsA, inlier_A=st["inliers"][0], inlier_B=st["inliers"][1], inlier_P=st["inliers"][2],
               inlier_pairs=co["inlier_pairs"])
    return st, got


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tag", TAGS)
def test_the_public_functions_through_the_seam(tag, dtype, monkeypatch):
    from spateo_amd import align

    made = _seam(monkeypatch)
    c = sc.case_inputs(G, tag)
    st, got = start_of_case(align, c, dtype)
    sc.check(got, G, tag, sc.tolerances(G, tag, dtype), f"seam {dtype}")
    assert set(st) == {"inliers", "sigma2", "probability_parameters", "inducing_variables", "samples_s"}   # morpho_iterate's keywords
    # the inducing variables: rows of coordsA, moved with it
    moved = c["coordsA"] @ st.init_R.T + st.init_t
    assert st["inducing_variables"].shape == (40, c["coordsA"].shape[1])
    assert all(np.abs(moved - u).sum(1).min() < 1e-12 for u in st["inducing_variables"])
    assert st["samples_s"] == max(np.prod(np.ptp(st.coordsA, axis=0)), np.prod(np.ptp(c["coordsB"], axis=0)))
    # the stand-alone functions give the same numbers
    s2 = align.init_sigma2(st.coordsA, c["coordsB"], subsample_A=c["subsample_A"], subsample_B=c["subsample_B"], dtype=dtype)
    pp = align.init_probability_parameters(c["layers_A"], c["layers_B"], dissimilarity=c["dissimilarity"],
                                           probability_type=c["probability_type"], probability_parameters=c["probability_parameters"],
                                           subsample_A=c["subsample_A"], subsample_B=c["subsample_B"], dtype=dtype)
    assert s2 == st["sigma2"] and pp == st["probability_parameters"]
    assert align.init_sigma2(st.coordsA, c["coordsB"], sigma2_init_scale=2.5, subsample_A=c["subsample_A"],
                             subsample_B=c["subsample_B"], dtype=dtype) == 2.5 * s2
    # the row statistics are asked for as the exchanged call: (nB_sub, nA_sub)
    nA, nB = len(c["subsample_A"]), len(c["subsample_B"])
    assert sum(m.calls.count((nB, nA, 0)) for m in made) >= 2        # morpho_start's and init_probability_parameters'


@pytest.mark.parametrize("loop", ["morpho_iterate", "morpho_iterate_svi"])
def test_the_loops_start_from_morpho_start_through_the_seams(loop, monkeypatch):
    """``loop(start.coordsA, coordsB, LA, LB, ..., **start)`` on case 1 (the loops' own NumPy stand-ins): the rotation put in
    comes back within the maker's 0.05."""
    import _align_svi_case as svc
    from spateo_amd import align

    c = sc.case_inputs(G, "1")
    _seam(monkeypatch)
    st, _ = start_of_case(align, c, "float64")
    monkeypatch.undo()
    svc.cpu_loop_kernels(monkeypatch, 3)
    extra = dict(batch_size=200, seed=0) if loop.endswith("svi") else {}
    out = getattr(align, loop)(st.coordsA, c["coordsB"], c["layers_A"], c["layers_B"], dissimilarity=c["dissimilarity"],
                               probability_type=c["probability_type"], beta=0.5, lambdaVF=100.0, max_iter=6, record=False, **extra, **st)
    assert np.linalg.norm(out["R"] @ st.init_R - c["R0"]) <= 0.05


def test_parameters_that_were_given_and_other_types_pass_through(monkeypatch):
    from spateo_amd import align

    made = _seam(monkeypatch)
    c = sc.case_inputs(G, "2")
    out = align.init_probability_parameters(c["layers_A"], c["layers_B"], dissimilarity=c["dissimilarity"],
                                            probability_type=["gauss", "cos"], probability_parameters=[7.0, None])
    assert out == [7.0, None] and not made                           # nothing to estimate: no device
    # a draw of our own: seeded, reproducible, the subsample's size
    kw = dict(dissimilarity=c["dissimilarity"], probability_type=c["probability_type"], subsample=100)
    one = align.init_probability_parameters(c["layers_A"], c["layers_B"], seed=3, **kw)
    assert one == align.init_probability_parameters(c["layers_A"], c["layers_B"], seed=3, **kw)
    assert one != align.init_probability_parameters(c["layers_A"], c["layers_B"], seed=4, **kw)
    assert [c for m in made for c in m.calls] == [(100, 100, 0)] * 3


# ---- validation before a device is touched --------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    from spateo_amd import _runtime as rt

    def refuse(device, dtype):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(rt, "_make_kernels", refuse)


def test_validation_needs_no_device(monkeypatch):
    from spateo_amd import align

    _no_device(monkeypatch)
    rng = np.random.default_rng(0)
    XA, XB = rng.standard_normal((50, 2)), rng.standard_normal((40, 2))
    LA, LB = rng.random((50, 6)), rng.random((40, 6))
    kw = dict(dissimilarity="kl", probability_type="gauss")
    bad = [
        (AssertionError, lambda: align.init_sigma2(XA, XB[:, :1])),
        (AssertionError, lambda: align.init_sigma2(XA[0], XB)),
        (NotImplementedError, lambda: align.init_sigma2(rng.random((5, 4)), rng.random((5, 4)))),
        (ValueError, lambda: align.init_sigma2(XA, XB, subsample_A=[0, 50])),                  # out of range
        (ValueError, lambda: align.init_sigma2(XA, XB, subsample_B=[3, 3])),                   # repeated
        (ValueError, lambda: align.init_sigma2(XA, XB, subsample_A=[-1])),
        (ValueError, lambda: align.init_sigma2(XA, XB, subsample_A=[0.5, 1.0])),
        (ValueError, lambda: align.init_sigma2(XA, XB, subsample=0)),
        (ValueError, lambda: align.init_sigma2(XA, XB, dtype="float16")),
        (NotImplementedError, lambda: align.init_probability_parameters([LA] * 5, [LB] * 5, **kw)),
        (ValueError, lambda: align.init_probability_parameters([LA, LA], [LB], **kw)),
        (ValueError, lambda: align.init_probability_parameters([LA], [LB], dissimilarity=["kl", "kl"], probability_type="gauss")),
        (ValueError, lambda: align.init_probability_parameters(LA, LB, dissimilarity="manhattan", probability_type="gauss")),
        (AssertionError, lambda: align.init_probability_parameters(LA, LB[:, :5], **kw)),
        (ValueError, lambda: align.init_probability_parameters(LA, LB, subsample_A=[50], **kw)),
        (ValueError, lambda: align.coarse_rigid_alignment(XA, XB, LA, LB, metric="kl", nn_init_top_K=0)),
        (ValueError, lambda: align.coarse_rigid_alignment(XA, XB, LA, LB, metric="label")),
        (NotImplementedError, lambda: align.coarse_rigid_alignment(XA, XB, LA, LB, metric="kl", nn_init_top_K=65)),
        (NotImplementedError, lambda: align.morpho_start(XA, XB, LA, LB, nn_init_top_K=65, **kw)),
        (ValueError, lambda: align.coarse_rigid_alignment(XA, XB, LA[:49], LB, metric="kl")),
        (AssertionError, lambda: align.coarse_rigid_alignment(XA, XB, LA, LB[:, :5], metric="kl")),
        (ValueError, lambda: align.coarse_rigid_alignment(XA, XB, LA, LB, metric="kl", subsample_B=[1, 1])),
        (NotImplementedError, lambda: align.coarse_rigid_alignment(rng.random((50, 4)), rng.random((40, 4)), LA, LB, metric="kl")),
        (ValueError, lambda: align.morpho_start(XA, XB, LA[:49], LB, **kw)),
        (ValueError, lambda: align.morpho_start(XA, XB, LA, LB, nn_init_top_K=0, **kw)),
        (ValueError, lambda: align.morpho_start(XA, XB, LA, LB, inducing_variables_num=0, **kw)),
        (ValueError, lambda: align.morpho_start(XA, XB, LA, LB, subsample_A=[0, 0], nn_init=False, **kw)),
        (NotImplementedError, lambda: align.morpho_start(XA, XB, [LA] * 5, [LB] * 5, **kw)),
    ]
    for exc, call in bad:
        with pytest.raises(exc):
            call()


def test_refusals_name_the_function_that_was_called(monkeypatch):
    from spateo_amd import align

    _no_device(monkeypatch)
    rng = np.random.default_rng(3)
    LA, LB = rng.random((30, 4)), rng.random((20, 4))
    kw = dict(dissimilarity="kl", probability_type="gauss")
    with pytest.raises(NotImplementedError, match="^init_probability_parameters: at most 4 layers"):
        align.init_probability_parameters([LA] * 5, [LB] * 5, **kw)
    with pytest.raises(NotImplementedError, match="^morpho_start: at most 4 layers"):
        align.morpho_start(rng.random((30, 2)), rng.random((20, 2)), [LA] * 5, [LB] * 5, **kw)
    with pytest.raises(NotImplementedError, match="^coarse_rigid_alignment: nn_init_top_K = 65"):
        align.coarse_rigid_alignment(rng.random((30, 2)), rng.random((20, 2)), LA, LB, metric="kl", nn_init_top_K=65)


def test_morpho_starts_own_draw_is_one_stream(monkeypatch):
    """Without index arrays: A is drawn before B from ONE generator, so equally sized slices get different rows, and the
    stand-alone functions called with the same seed draw the same rows."""
    from spateo_amd import align

    _seam(monkeypatch)
    c = sc.case_inputs(G, "2")
    n = min(len(c["coordsA"]), len(c["coordsB"]))
    XA, XB = c["coordsA"][:n], c["coordsB"][:n]
    LA, LB = [a[:n] for a in c["layers_A"]], [b[:n] for b in c["layers_B"]]
    kw = dict(dissimilarity=c["dissimilarity"], probability_type=c["probability_type"], probability_parameters=c["probability_parameters"])
    st = align.morpho_start(XA, XB, LA, LB, init_metric=c["init_metric"], subsample=150, n_sampling=150, seed=11,
                            inducing_variables_num=30, **kw)
    rng = np.random.default_rng(11)
    iA, iB = rng.choice(n, 150, replace=False), rng.choice(n, 150, replace=False)
    assert not np.array_equal(iA, iB)
    assert st["sigma2"] == align.init_sigma2(st.coordsA, XB, subsample=150, seed=11) == align.init_sigma2(st.coordsA, XB, subsample_A=iA, subsample_B=iB)
    assert st["probability_parameters"] == align.init_probability_parameters(LA, LB, subsample=150, seed=11, **kw)
    import copy
    import pickle

    for twin in (st.copy(), copy.copy(st), copy.deepcopy(st), pickle.loads(pickle.dumps(st))):     # the attributes travel
        assert type(twin) is type(st) and dict(twin).keys() == dict(st).keys()
        assert np.array_equal(twin.coordsA, st.coordsA) and np.array_equal(twin.init_R, st.init_R) and np.array_equal(twin.init_t, st.init_t)
    again = align.morpho_start(XA, XB, LA, LB, init_metric=c["init_metric"], subsample=150, n_sampling=150, seed=11,
                               inducing_variables_num=30, **kw)
    assert again["sigma2"] == st["sigma2"] and np.array_equal(again["inducing_variables"], st["inducing_variables"])
    other = align.morpho_start(XA, XB, LA, LB, init_metric=c["init_metric"], subsample=150, n_sampling=150, seed=12,
                               inducing_variables_num=30, **kw)
    assert other["sigma2"] != st["sigma2"]


def test_morpho_start_refuses_too_few_pairs_before_the_device(monkeypatch):
    """The coarse stage's refusal through morpho_start: no kernels object and no device unique_rows before it."""
    from spateo_amd import align, preprocess

    _no_device(monkeypatch)
    monkeypatch.setattr(preprocess, "unique_rows", lambda *a, **k: (_ for _ in ()).throw(AssertionError("unique_rows ran first")))
    rng = np.random.default_rng(2)
    centres = np.array([[0.2, 0.2], [0.5, 0.7], [0.8, 0.3]])

    def slice_(n):
        X = centres[rng.integers(0, 3, n)] + 1e-3 * rng.standard_normal((n, 2))
        X[0], X[1] = (0.0, 0.0), (1.0, 1.0)
        return X, rng.random((n, 5))

    (XA, LA), (XB, LB) = slice_(2000), slice_(2000)
    with pytest.raises(ValueError, match="fewer than 22 matched pairs"):
        align.morpho_start(XA, XB, LA, LB, dissimilarity="kl", probability_type="gauss", probability_parameters=[0.1], nn_init_top_K=1)


def test_a_label_layer_that_would_need_estimating_is_named(monkeypatch):
    from spateo_amd import align

    _no_device(monkeypatch)
    rng = np.random.default_rng(1)
    LA, LB = rng.random((30, 4)), rng.random((20, 4))
    labA, labB = rng.integers(0, 3, 30), rng.integers(0, 3, 20)
    kw = dict(dissimilarity=["kl", "label"], probability_type=["gauss", "gauss"], label_transfer=np.ones((3, 3)))
    with pytest.raises(ValueError, match="layer 1 is a 'label' layer"):
        align.init_probability_parameters([LA, labA], [LB, labB], probability_parameters=[0.1, None], **kw)
    with pytest.raises(ValueError, match="layer 1 is a 'label' layer"):
        align.morpho_start(rng.random((30, 2)), rng.random((20, 2)), [LA, labA], [LB, labB], probability_parameters=[0.1, None], **kw)
    # with its parameter, or as a "prob" layer, it passes through
    assert align.init_probability_parameters([LA, labA], [LB, labB], probability_parameters=[0.1, 0.5], **kw) == [0.1, 0.5]


def test_fewer_than_22_pairs_are_refused_before_the_device(monkeypatch):
    """Three tight clusters and one corner point per slice: four occupied voxels a side, top_K capped at 3 -> 1 asked: 8 pairs."""
    from spateo_amd import align

    _no_device(monkeypatch)
    rng = np.random.default_rng(2)

    def slice_(n):
        centres = np.array([[0.2, 0.2], [0.5, 0.7], [0.8, 0.3]])
        X = centres[rng.integers(0, 3, n)] + 1e-3 * rng.standard_normal((n, 2))
        X[0], X[1] = (0.0, 0.0), (1.0, 1.0)
        return X, rng.random((n, 5))

    (XA, LA), (XB, LB) = slice_(2000), slice_(2000)
    vA, _ = align._voxel_data(XA, LA, 100)
    assert len(vA) == 4
    with pytest.raises(ValueError, match="fewer than 22 matched pairs"):
        align.coarse_rigid_alignment(XA, XB, LA, LB, metric="kl", nn_init_top_K=1)


@pytest.mark.parametrize("D", [2, 3])
def test_the_grid_voxelisation_is_the_loop_over_all_voxels(D):
    """align._voxel_data (every point visits the nodes in reach) against the restatement (every node tests every point)."""
    from spateo_amd import align

    rng = np.random.default_rng(D)
    X, F = rng.standard_normal((700, D)) * [1.0, 2.0, 0.5][:D], rng.random((700, 7))
    for voxel_num in (100, 400):
        v, m = align._voxel_data(X, F, voxel_num)
        rv, rm = sc.voxel_data(X, F, voxel_num)
        assert np.array_equal(v, rv) and np.abs(m - rm).max() <= 1e-14


# ---- the public names -------------------------------------------------------------------------------------------------------------
def test_public_names_and_docstrings():
    import inspect

    import spateo_amd as st
    from spateo_amd import align

    for name in ("init_sigma2", "init_probability_parameters", "coarse_rigid_alignment", "morpho_start"):
        assert name in align.__all__ and getattr(st.align, name) is getattr(align, name)
        doc = getattr(align, name).__doc__
        assert "NOT the reference's stream" in doc and "subsample_A" in doc, name
        assert {"subsample_A", "subsample_B", "seed", "dtype", "device"} <= set(inspect.signature(getattr(align, name)).parameters)
    assert "utils.py:1339-1354" in align.init_sigma2.__doc__ and "nA_sub * nA_sub" in align.init_sigma2.__doc__
    assert ":813-817" in align.init_probability_parameters.__doc__ and "ValueError" in align.init_probability_parameters.__doc__
    assert "inlier_from_NN" in align.coarse_rigid_alignment.__doc__ and "22 pairs" in align.coarse_rigid_alignment.__doc__
    assert "rigid motion" in align.morpho_start.__doc__ and "**start" in align.morpho_start.__doc__
    # the loops' signatures did not move
    for fn in (align.morpho_iterate, align.morpho_iterate_svi):
        assert {"probability_parameters", "inducing_variables", "sigma2", "samples_s", "inliers"} <= set(inspect.signature(fn).parameters)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_c_abi_symbols_and_argument_errors():
    from spateo_amd import _lib
    from spateo_amd._kernels import HipKernels

    lib = _lib.load()
    for name in ("mvf_assign_layer_stats", "mvf_assign_layer_stats_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert hasattr(HipKernels, "assign_layer_stats")
    assert lib.mvf_version() == 7                                            # an addition: the ABI version is unchanged
    size = lib.mvf_assign_layer_stats_workspace_bytes
    # 600 x 450: 10 row splits, 512 padded columns: 3 partials per split, 2 column sums, the splits' lists
    assert size(600, 450, 0) == 10 * 3 * 512 * 8 + 2 * 512 * 8
    assert size(600, 450, 8) == size(600, 450, 0) + 10 * 8 * 512 * (8 + 4)
    assert size(5, 450, 64) == size(5, 450, 0) + 5 * 512 * (8 + 4)          # k_eff = min(k, na)
    assert size(0, 450, 8) == 0 and size(600, 0, 8) == 0 and size(600, 450, -1) == 0 and size(600, 450, 65) == 0
    p = ctypes.c_void_p(256)
    ws = size(600, 450, 8)

    def run(na=600, nb=450, k=8, ws_bytes=ws, cmin=p, rows=p, vals=p, sums=p, work=p, layer=True, dtype=_lib.MVF_F64, **fields):
        lay = (_lib.AssignLayer * 1)()
        lay[0].Xp = lay[0].Yp = lay[0].a = lay[0].b = 256
        lay[0].ld, lay[0].metric, lay[0].prob, lay[0].param = 16, 2, 7, -1.0    # prob / param are not read
        for f, v in fields.items():
            setattr(lay[0], f, v)
        return lib.mvf_assign_layer_stats(lay if layer else None, na, nb, k, cmin, rows, vals, sums, work, ws_bytes, dtype, None)

    # refusals report through the status + mvf_last_error channel before any HIP call
    for kw, msg in ((dict(k=-1), b"0 <= k <= 64"), (dict(k=65), b"0 <= k <= 64"), (dict(na=0), b"na >= 1"), (dict(nb=0), b"nb >= 1"),
                    (dict(na=-3), b"na >= 1"), (dict(na=1 << 31), b"too many cells"), (dict(ws_bytes=ws - 1), b"workspace too small"),
                    (dict(cmin=None), b"null pointer"), (dict(sums=None), b"null pointer"), (dict(work=None), b"null pointer"),
                    (dict(rows=None), b"null pointer"), (dict(vals=None), b"null pointer"), (dict(layer=False), b"null pointer"),
                    (dict(Xp=None), b"null pointer in layer"), (dict(Yp=None), b"null pointer in layer"),
                    (dict(a=None), b"null pointer in layer"), (dict(b=None), b"null pointer in layer"),
                    (dict(ld=0), b"ld must be"), (dict(ld=17), b"ld must be"), (dict(metric=6), b"bad metric"),
                    (dict(metric=-1), b"bad metric"), (dict(metric=5), b"a label layer has no Yp"),
                    (dict(metric=5, Yp=None, ld=0), b"row length L >= 1"), (dict(dtype=2), b"bad dtype")):
        assert run(**kw) != 0, kw
        assert msg in lib.mvf_last_error() and b"mvf_assign_layer_stats" in lib.mvf_last_error(), (kw, lib.mvf_last_error())
