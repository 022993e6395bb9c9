"""CPU suite of the cell mapping from the fused assignment: the restatement of the two tie rules against the goldens of the real
``mapping_aligned_coords`` (tests/golden/ref_assign_best.npz), ``st.align.optimal_mapping`` / ``mapping_from_best``, the
``optimal_mapping=True`` of both loops and of ``Morpho_pairwise`` on the NumPy stand-in of ``HipKernels.assign_best``,
``st.tdr.cell_directions(mapping=)``, every new ``ValueError`` and the C ABI's refusals.  No GPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import _align_loop_case as lc
import _align_svi_case as sc
import _assign_best_case as bc
import _assign_case as ac
import _assign_edge_cases as ec
import _assign_label_case as lab
import _morpho_align_case as mc

G = bc.load()
TAGS = bc.case_tags(G)
HERE = os.path.dirname(os.path.abspath(__file__))


def _numpy_P(tag):
    args, kw = bc.case_inputs(G, tag)
    fn = lab.restatement if "label_transfer" in kw else ac.restatement
    return np.asarray(fn(*args, return_P=True, **kw)["P"]), args


def _golden_best(tag):
    return bc.golden_best(G, tag)


# ---- the goldens and the restatement ------------------------------------------------------------------------------------
def test_goldens_cover_the_tie_rules():
    assert TAGS == ["a", "b", "c", "l", "p"]
    dims = {t: G[f"{t}_XAHat"].shape[1] for t in TAGS}
    assert 2 in dims.values() and 3 in dims.values() and "label" in [str(m) for m in G["l_dissimilarity"]]
    assert G["p_XAHat"].shape == (149, 3) and G["p_coordsB"].shape == (117, 3) and G["p_P"].shape == (149, 117)
    for t in TAGS:
        na, nb = len(G[f"{t}_XAHat"]), len(G[f"{t}_coordsB"])
        g = _golden_best(t)
        for keep_all in (False, True):
            (iA, vA), (iB, vB) = bc.golden_mapping(G, t, keep_all)
            assert iA.shape == (na, 2) and iB.shape == (nb, 2) and vA.shape == (na,) and vB.shape == (nb,)
            assert np.array_equal(iA[:, 0], np.arange(na)) and np.array_equal(iB[:, 1], np.arange(nb))   # sorted, one per cell
        # far cells: an all-zero row / column maps to the nearest cell (keep_all=False) and to index 0 (keep_all=True)
        far_A, far_B = G[f"{t}_far_A"], G[f"{t}_far"]
        assert len(far_A) >= 3 and len(far_B) >= 0.05 * nb
        assert not g["row_values"][far_A].any() and not g["col_values"][far_B].any()
        assert not g["rows"][far_A, 1].any() and not g["cols"][far_B, 1].any()
        X, Y = G[f"{t}_XAHat"], G[f"{t}_coordsB"]
        assert np.array_equal(g["rows"][far_A, 0], ((Y[None] - X[far_A, None]) ** 2).sum(2).argmin(1))
        assert np.array_equal(g["cols"][far_B, 0], ((X[None] - Y[far_B, None]) ** 2).sum(2).argmin(1))
        assert (g["rows"][far_A, 0] != 0).any()
        assert float(G[f"{t}_near_rows"]) <= bc.MAX_LEFT_OUT and float(G[f"{t}_near_cols"]) <= bc.MAX_LEFT_OUT


def test_restatement_reproduces_the_goldens_exactly():
    """On the reference's own P (case p stores it) the restatement gives the real function's indices and values, bit for bit,
    for both ``keep_all``."""
    got = bc.best_of(G["p_P"], G["p_XAHat"], G["p_coordsB"])
    want = _golden_best("p")
    for q in bc.KEYS:
        assert got[q].dtype == want[q].dtype and np.array_equal(got[q], want[q]), q
    assert (got["rows"][:, 0] != got["rows"][:, 1]).any()          # the rules differ in this fixture


@pytest.mark.parametrize("tag", TAGS)
def test_goldens_against_the_numpy_assignment(tag):
    """The restatement on the P of the NumPy restatement of the step against the real mapping: every case's inputs reproduce
    its stored indices wherever the reference's P and this one decide them at the float64 bound, and its values."""
    P, args = _numpy_P(tag)
    ours = bc.best_of(P, args[0], args[1])
    gold = bc.check_golden_indices(ours, P, G, tag, ac.F64_TOL, what=f"golden {tag}")
    for q in ("row_values", "col_values"):
        assert np.abs(ours[q] - gold[q]).max() <= ac.F64_TOL * P.max(), q
    fig = bc.check(ours, P, args[0], args[1], ac.F64_TOL, what=f"restatement {tag}")
    assert fig["rows"]["zero"] == len(G[f"{tag}_far_A"]) and fig["cols"]["zero"] >= len(G[f"{tag}_far"])
    # exact ties of a positive maximum (the matrix product may leave a case's copies an ulp apart in one direction)
    assert fig["rows"]["tied"] + fig["cols"]["tied"] > fig["rows"]["zero"] + fig["cols"]["zero"]


def test_the_checker_rejects_each_wrong_answer():
    P, X, Y = G["p_P"], G["p_XAHat"], G["p_coordsB"]
    good = bc.best_of(P, X, Y)
    bc.check(good, P, X, Y, ac.F64_TOL, "good")
    far = int(G["p_far_A"][0])

    def bad(**edit):
        b = {q: v.copy() for q, v in good.items()}
        for q, (i, c, v) in edit.items():
            if c is None:
                b[q][i] = v
            else:
                b[q][i, c] = v
        return b

    second = int(np.argsort(-P[7])[1])
    for what, b in (("an index out of range", bad(rows=(3, 0, P.shape[1]))),
                    ("the runner-up", bad(rows=(7, 0, second))),
                    ("index 0 for the nearest partner of a far cell", bad(rows=(far, 0, 0))),
                    ("the nearest partner under the first rule", bad(rows=(far, 1, good["rows"][far, 0]))),
                    ("a value from elsewhere", bad(row_values=(7, None, good["row_values"][7] * (1 + 1e-6)))),
                    ("a wrong row of a column", bad(cols=(5, 1, int(np.argsort(-P[:, 5])[1]))))):
        with pytest.raises(AssertionError):
            bc.check(b, P, X, Y, ac.F64_TOL, what)


def test_the_planted_ties_of_the_kernel_tests():
    """What tests/test_gpu_assign_best_kernels.py relies on, proven on the reference of the host-prepared operands."""
    c = bc.tie_case()
    P = ec.reference_for(c, np.float64)["P"]
    b = bc.best_of(P, c["XA"], c["XB"])
    zr, zc = c["zero_rows"], c["far"]
    assert ec.plan(*bc.TIE_SHAPE) == (4, 5, 4, 5)
    assert sorted(set(zr // ec.TILE)) == [0, 1, 2, 3] and not P[zr].any() and not P[:, zc].any()
    assert (b["rows"][zr, 0] // ec.TILE != 0).all() and not b["rows"][zr, 1].any()
    assert (b["cols"][zc, 0] // ec.TILE != 0).all() and not b["cols"][zc, 1].any()
    assert len(c["copies_B"]) >= 2 and len(c["copies_A"]) >= 2
    # (NumPy's matrix product may leave the copies' entries an ulp apart; the device forms them by the same operations in the
    # same order, so there they tie exactly - the kernel test demands the smallest copy wherever a copy heads the row)
    for group, Q in [(g, P) for g in c["copies_B"]] + [(g, P.T) for g in c["copies_A"]]:
        assert len({i // ec.TILE for i in group}) >= 3 and group == sorted(group)
        headed = [i for i in range(len(Q)) if Q[i, group].max() == Q[i].max() > 0]
        assert len(headed) >= 2
        for i in headed:
            assert np.ptp(Q[i, group]) <= ec.REF_TOL * Q[i].max()
    assert all(g[1] == g[0] + 1 for g in c["copies_B"])                  # the next lane


# ---- mapping_from_best and optimal_mapping ----------------------------------------------------------------------------------
def test_mapping_from_best_layouts_and_dtypes():
    from spateo_amd import align

    P, X, Y = G["p_P"], G["p_XAHat"], G["p_coordsB"]
    best = bc.best_of(P, X, Y)
    for keep_all in (False, True):
        by_A, by_B = align.mapping_from_best(best, X, Y, keep_all)
        (iA, vA), (iB, vB) = bc.golden_mapping(G, "p", keep_all)
        for m, idx, val, n in ((by_A, iA, vA, len(X)), (by_B, iB, vB, len(Y))):
            assert sorted(m) == ["mapping_X", "mapping_Y", "pi_index", "pi_value"]
            assert m["pi_index"].dtype == np.int32 and m["pi_index"].shape == (n, 2) and m["pi_value"].dtype == np.float64
            assert np.array_equal(m["pi_index"], idx) and np.array_equal(m["pi_value"], val)
            assert np.array_equal(m["mapping_X"], X[idx[:, 0]]) and np.array_equal(m["mapping_Y"], Y[idx[:, 1]])
        assert np.array_equal(by_A["pi_index"][:, 0], np.arange(len(X))) and np.array_equal(by_B["pi_index"][:, 1], np.arange(len(Y)))
    # torch tensors and plain lists are taken as they come back from the device
    import torch

    t = {q: torch.from_numpy(v) for q, v in best.items()}
    assert np.array_equal(align.mapping_from_best(t, X, Y)[0]["pi_index"], align.mapping_from_best(best, X, Y)[0]["pi_index"])
    empty_A, empty_B = align.mapping_from_best(best, X[:0], Y)
    for m in (empty_A, empty_B):
        assert m["pi_index"].shape == (0, 2) and m["pi_index"].dtype == np.int32 and m["mapping_X"].shape == (0, 3) \
            and m["mapping_Y"].shape == (0, 3) and m["pi_value"].shape == (0,)


def test_mapping_from_best_errors():
    from spateo_amd import align

    P, X, Y = G["p_P"], G["p_XAHat"], G["p_coordsB"]
    best = bc.best_of(P, X, Y)
    with pytest.raises(ValueError, match="missing: cols"):
        align.mapping_from_best({q: v for q, v in best.items() if q != "cols"}, X, Y)
    with pytest.raises(ValueError, match="best must be a dict"):
        align.mapping_from_best(None, X, Y)
    with pytest.raises(ValueError, match="same D"):
        align.mapping_from_best(best, X, Y[:, :2])
    with pytest.raises(ValueError, match="rows side"):
        align.mapping_from_best(dict(best, rows=best["rows"][:-1]), X, Y)
    with pytest.raises(ValueError, match="cols side"):
        align.mapping_from_best(dict(best, cols=best["cols"].astype(np.float64)), X, Y)
    wrong = best["rows"].copy()
    wrong[3, 0] = len(Y)
    with pytest.raises(ValueError, match=f"outside \\[0, {len(Y)}\\)"):
        align.mapping_from_best(dict(best, rows=wrong), X, Y)


@pytest.mark.parametrize("tag", ["p", "c"])
@pytest.mark.parametrize("keep_all", [False, True])
def test_optimal_mapping_through_the_seam(tag, keep_all, monkeypatch):
    from spateo_amd import align

    args, kw = bc.case_inputs(G, tag)
    bc.cpu_best_kernels(monkeypatch, args[0].shape[1])
    by_A, by_B = align.optimal_mapping(*args, keep_all=keep_all, **kw)
    (kind, call), = bc.CpuBestKernels.CALLS                     # one call, on the whole of both slices
    assert kind == "assign_best" and call["P"].shape == (len(args[0]), len(args[1]))
    want = align.mapping_from_best(bc.best_of(call["P"], args[0], args[1]), args[0], args[1], keep_all)
    for got, ref in zip((by_A, by_B), want):
        assert sorted(got) == sorted(ref)
        for q in ref:
            assert got[q].dtype == ref[q].dtype and np.array_equal(got[q], ref[q]), q
    # and against the NumPy restatement of the step on the arguments as given
    best = bc.best_from_mappings(align.optimal_mapping(*args, keep_all=False, **kw), align.optimal_mapping(*args, keep_all=True, **kw))
    bc.check(best, _numpy_P(tag)[0], args[0], args[1], ac.F64_TOL, what=f"seam {tag}")


def test_optimal_mapping_empty_sides_and_argument_errors():
    from spateo_amd import align

    args, kw = bc.case_inputs(G, "p")
    XA, XB, LA, LB = args
    for a in ((XA[:0], XB, [L[:0] for L in LA], LB), (XA, XB[:0], LA, [L[:0] for L in LB])):
        k2 = dict(kw, alpha=kw["alpha"][: len(a[0])], SigmaDiag=kw["SigmaDiag"][: len(a[0])])
        by_A, by_B = align.optimal_mapping(*a, **k2)
        for m in (by_A, by_B):
            assert m["pi_index"].shape == (0, 2) and m["pi_index"].dtype == np.int32 and m["pi_value"].shape == (0,)
            assert m["mapping_X"].shape == (0, 3) and m["mapping_Y"].shape == (0, 3)
    # update_assignment's refusals, in its order, named after this function where it names itself
    with pytest.raises(ValueError, match="dtype must be"):
        align.optimal_mapping(*args, **dict(kw, dtype="float16"))
    with pytest.raises(NotImplementedError, match="optimal_mapping: spatial coordinates must be 2-D or 3-D"):
        align.optimal_mapping(np.zeros((5, 4)), np.zeros((6, 4)), LA, LB, **kw)
    with pytest.raises(NotImplementedError, match="optimal_mapping: at most 4 layers"):
        align.optimal_mapping(XA, XB, [LA[0]] * 5, [LB[0]] * 5, **dict(kw, dissimilarity="kl", probability_type="gauss",
                                                                   probability_parameters=0.1))
    with pytest.raises(ValueError, match="Unsupported dissimilarity metric"):
        align.optimal_mapping(*args, **dict(kw, dissimilarity=["manhattan", "cos"]))
    with pytest.raises(ValueError, match="alpha and SigmaDiag"):
        align.optimal_mapping(*args, **dict(kw, alpha=kw["alpha"][:-1]))
    with pytest.raises(AssertionError, match="label_transfer must be provided"):
        align.optimal_mapping(XA, XB, [np.zeros(len(XA), dtype=np.int64)], [np.zeros(len(XB), dtype=np.int64)],
                              **dict(kw, dissimilarity=["label"], probability_type=["prob"], probability_parameters=[None]))
    with pytest.raises(TypeError):
        align.optimal_mapping(*args, return_P=True, **kw)
    with pytest.raises(TypeError):
        align.optimal_mapping(*args, sparse_calculation_mode=True, **kw)


# ---- the loops ------------------------------------------------------------------------------------------------------------
def _equal(a, b, path=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), (path, sorted(a), sorted(b))
        for key in a:
            _equal(a[key], b[key], f"{path}/{key}")
    elif isinstance(a, np.ndarray) and a.dtype.kind == "f":
        assert a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)), path
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    elif hasattr(a, "toarray"):
        assert np.array_equal(a.toarray(), b.toarray()), path
    else:
        assert a == b or (a is None and b is None), path


def _same_state(a, b):
    for q in a:
        if q == "P":
            continue
        if isinstance(a[q], list):
            assert len(a[q]) == len(b[q]) and all(np.array_equal(x, y) for x, y in zip(a[q], b[q])), q
        else:
            assert np.array_equal(a[q], b[q]), q


@pytest.mark.parametrize("sparse", [False, True])
def test_morpho_iterate_gains_best_and_keeps_every_other_bit(sparse, monkeypatch):
    from spateo_amd import align

    D = lc.load()
    args, kw = lc.case_inputs(D, "3")
    kw = dict(kw, max_iter=4, record=True)
    if sparse:
        kw.update(sparse_calculation_mode=True, sparse_top_k=8)
    bc.cpu_best_kernels(monkeypatch, 2)
    plain = align.morpho_iterate(*args, **kw)
    del bc.CpuBestKernels.CALLS[:]
    out = align.morpho_iterate(*args, optimal_mapping=True, **kw)
    best = out.pop("best")
    _equal(out, plain)
    # one mvf_assign_best, right behind the LAST assignment and on its operands and state
    kinds = [k for k, _ in bc.CpuBestKernels.CALLS]
    assert kinds == ["assign_topk" if sparse else "assign"] * 4 + ["assign_best"]
    _same_state(bc.CpuBestKernels.CALLS[-1][1], bc.CpuBestKernels.CALLS[-2][1])
    call = bc.CpuBestKernels.CALLS[-1][1]
    assert sorted(best) == sorted(bc.KEYS) and best["rows"].shape == (len(args[0]), 2) and best["cols"].shape == (len(args[1]), 2)
    assert best["rows"].dtype == best["cols"].dtype == np.int32 and best["row_values"].dtype == np.float64
    for q, v in bc.best_of(call["P"], call["xa4"][:, :2], call["xb4"][:, :2]).items():     # the DENSE P, also in the sparse mode
        assert np.array_equal(best[q], v), q
    by_A, _ = align.mapping_from_best(best, out["XAHat"], args[1])
    assert np.array_equal(by_A["mapping_X"], out["XAHat"]) and np.array_equal(by_A["pi_index"][:, 1], best["rows"][:, 0])


@pytest.mark.parametrize("return_mapping", [False, True])
def test_morpho_iterate_svi_runs_the_closing_assignment(return_mapping, monkeypatch):
    from spateo_amd import align

    S = sc.load()
    args, kw = sc.case_inputs(S, "3")
    kw = dict(kw, max_iter=4, record=True)
    bc.cpu_best_kernels(monkeypatch, 2)
    mapped = align.morpho_iterate_svi(*args, return_mapping=True, **kw)
    del bc.CpuBestKernels.CALLS[:]
    out = align.morpho_iterate_svi(*args, return_mapping=return_mapping, optimal_mapping=True, **kw)
    best = out.pop("best")
    _equal(out, mapped)                       # with or without return_mapping: the bits of the call with return_mapping=True
    assert [k for k, _ in bc.CpuBestKernels.CALLS] == ["assign"] * 5 + ["assign_best"]      # 4 batches, the closing full one
    _same_state(bc.CpuBestKernels.CALLS[-1][1], bc.CpuBestKernels.CALLS[-2][1])
    call = bc.CpuBestKernels.CALLS[-1][1]
    assert call["P"].shape == (len(args[0]), len(args[1]))                                   # every B cell, not the batch
    assert best["rows"].shape == (len(args[0]), 2) and best["cols"].shape == (len(args[1]), 2)
    for q, v in bc.best_of(call["P"], call["xa4"][:, :2], call["xb4"][:, :2]).items():
        assert np.array_equal(best[q], v), q


def test_the_loops_share_the_keyword_and_document_it():
    import spateo_amd as st

    for fn in (st.align.morpho_iterate, st.align.morpho_iterate_svi):
        p = inspect.signature(fn).parameters["optimal_mapping"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
        assert "optimal_mapping=True" in fn.__doc__ and "mvf_assign_best" in fn.__doc__
    for name in ("optimal_mapping", "mapping_from_best"):
        assert name in st.align.__all__ and callable(getattr(st.align, name))
    doc = st.align.optimal_mapping.__doc__
    for word in ("get_optimal_mapping_relationship", "mapping_aligned_coords", "keep_all", "sorted by cell", "every tied pair",
                 "cell_directions"):
        assert word in doc, word
    sig = inspect.signature(st.align.optimal_mapping).parameters
    upd = inspect.signature(st.align.update_assignment).parameters
    assert [p for p in upd if p not in ("return_P", "sparse_calculation_mode", "sparse_top_k")] + ["keep_all"] == list(sig)
    assert list(inspect.signature(st.align.mapping_from_best).parameters) == ["best", "X", "Y", "keep_all"]
    assert "mapping=" in st.tdr.cell_directions.__doc__ or "``mapping``" in st.tdr.cell_directions.__doc__


def test_the_unchanged_refusals_still_come_first():
    from spateo_amd import align

    D = lc.load()
    args, kw = lc.case_inputs(D, "3")
    with pytest.raises(NotImplementedError, match="guidance"):
        align.morpho_iterate(*args, optimal_mapping=True, **dict(kw, guidance=dict(X_AI=np.zeros((2, 2)))))
    with pytest.raises(NotImplementedError, match="geodist"):
        align.morpho_iterate_svi(*args, optimal_mapping=True, **dict(kw, kernel_type="geodist"))
    with pytest.raises(NotImplementedError, match="sparse_top_k = 1024"):
        align.morpho_iterate(*args, optimal_mapping=True, sparse_calculation_mode=True, **kw)
    with pytest.raises(ValueError, match="exclude each other"):
        align.morpho_iterate_svi(*args, optimal_mapping=True, return_P=True, sparse_calculation_mode=True, sparse_top_k=4, **kw)


# ---- Morpho_pairwise and morpho_align ---------------------------------------------------------------------------------------
def test_morpho_pairwise_optimal_mapping(monkeypatch):
    from spateo_amd import _morpho_pairwise as mp
    from spateo_amd import align

    M = mc.load()
    A, B = mc.pair_samples(M, "1")
    make = lambda **over: align.Morpho_pairwise(A, B, dtype="float64", verbose=False, **mc.pair_kwargs(M, "1", **over))  # noqa: E731
    p = inspect.signature(align.Morpho_pairwise.__init__).parameters["optimal_mapping"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    off = make()
    with pytest.raises(ValueError, match="optimal_mapping=True"):
        off.optimal_mapping()
    m = make(optimal_mapping=True)
    with pytest.raises(ValueError, match="run\\(\\) first"):
        m.optimal_mapping()
    # run() hands the keyword to the loop
    seen = {}
    rng = np.random.default_rng(3)
    NA, NB, D, K = m.NA, m.NB, m.D, 8
    P = rng.random((NA, NB)) ** 8
    P[4] = 0.0
    start = align._Start(probability_parameters=[0.3], sigma2=0.7, inducing_variables=rng.random((K, D)), samples_s=1.0, inliers=None)
    start.coordsA, start.init_R, start.init_t, start.inducing_rows = m.coordsA.copy(), np.eye(D), np.zeros(D), np.arange(K)
    XAHat = rng.random((NA, D))
    best = bc.best_of(P, XAHat, m.coordsB)

    def loop(*a, **kw):
        seen.update(kw)
        return dict(R=np.eye(D), t=np.zeros(D), optimal_R=np.eye(D), optimal_t=np.zeros(D), sigma2=0.3, gamma=0.9, sigma2_variance=1.1,
                    Coff=rng.random((K, D)), VnA=np.zeros((NA, D)), alpha=np.ones(NA), SigmaDiag=np.zeros(NA), K_NA=np.ones(NA),
                    K_NB=np.ones(NB), XAHat=XAHat, RnA=XAHat, optimal_RnA=XAHat, P=P if kw["return_P"] else None,
                    **({"best": best} if kw["optimal_mapping"] else {}))

    monkeypatch.setattr(mp._al, "morpho_start", lambda *a, **kw: start)
    monkeypatch.setattr(mp._al, "morpho_iterate", loop)
    assert m.run() is P and seen["optimal_mapping"] is True
    for keep_all in (False, True):
        by_A, by_B = m.optimal_mapping(keep_all=keep_all)
        want = align.mapping_from_best(best, m.XAHat, m.raw_coordsB, keep_all)        # de-normalised XAHat, B as it came in
        for got, ref in zip((by_A, by_B), want):
            for q in ref:
                assert np.array_equal(got[q], ref[q]), q
        assert np.array_equal(by_A["mapping_X"], m._denormalize(XAHat))
        assert m.raw_coordsB.shape == (NB, D) and np.array_equal(by_B["mapping_Y"], m.raw_coordsB)   # not the normalised ones
    assert by_A["pi_index"][4, 1] == 0                                                 # keep_all=True: the zero row says 0
    off.run()
    assert seen["optimal_mapping"] is False and off.best is None
    # SVI: the dense P is sized for the closing full assignment that the keyword brings
    svi = align.Morpho_pairwise(*mc.pair_samples(M, "2"), dtype="float64", verbose=False, **mc.pair_kwargs(M, "2", optimal_mapping=True))
    monkeypatch.setattr(align, "RETURN_P_MAX_ENTRIES", svi.NA * 150)
    assert not svi._P_fits()


def test_morpho_align_passes_the_keyword_through(monkeypatch):
    from spateo_amd import _morpho_pairwise as mp

    seen = []

    class Recorder:
        def __init__(self, **kw):
            seen.append(kw)
            self.optimal_RnA = self.XAHat = np.array(kw["sampleA"].obsm["spatial"])
            self.iter_added = self.vecfld = None

        def run(self):
            return None

    M = mc.load()
    A, B = mc.pair_samples(M, "1")
    monkeypatch.setattr(mp, "Morpho_pairwise", Recorder)
    mp.morpho_align([A, B], optimal_mapping=True, iter_key_added=None)
    mp.morpho_align([A, B], iter_key_added=None)
    assert seen[0]["optimal_mapping"] is True and "optimal_mapping" not in seen[1]


# ---- cell_directions(mapping=) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_all, tag", [(False, "nearest"), (True, "all")])
def test_cell_directions_takes_the_mapping(keep_all, tag):
    import spateo_amd as st

    with np.load(os.path.join(HERE, "golden", "ref_celldir.npz")) as z:
        g = {k: z[k] for k in z.files}
    mapping = st.align.mapping_from_best(bc.best_of(g["pi"], g["XA"], g["XB"]), g["XA"], g["XB"], keep_all)
    for given in (mapping[0], mapping):
        A = st.AnnDataLite(obsm={"align_spatial": g["XA"].copy()})
        B = st.AnnDataLite(obsm={"align_spatial": g["XB"].copy()})
        ret, back = st.tdr.cell_directions(A, B, mapping=given)
        assert ret is None and back is given
        np.testing.assert_array_equal(A.obsm["X_mapping"], g[f"{tag}_X_mapping"])
        np.testing.assert_array_equal(A.obsm["V_mapping"], g[f"{tag}_V_mapping"])
    A2, _ = st.tdr.cell_directions(A, B, mapping=mapping, inplace=False, key_added="m2")
    assert "X_m2" in A2.obsm and "X_m2" not in A.obsm


def test_cell_directions_mapping_errors():
    import spateo_amd as st

    with np.load(os.path.join(HERE, "golden", "ref_celldir.npz")) as z:
        g = {k: z[k] for k in z.files}
    A = st.AnnDataLite(obsm={"align_spatial": g["XA"].copy()})
    B = st.AnnDataLite(obsm={"align_spatial": g["XB"].copy()})
    by_A, by_B = st.align.mapping_from_best(bc.best_of(g["pi"], g["XA"], g["XB"]), g["XA"], g["XB"])
    with pytest.raises(ValueError, match="not both"):
        st.tdr.cell_directions(A, B, pi=g["pi"], mapping=by_A)
    with pytest.raises(NotImplementedError, match="optimal-transport"):
        st.tdr.cell_directions(A, B)                                       # with neither: what it raised before
    with pytest.raises(ValueError, match="by_A dict"):
        st.tdr.cell_directions(A, B, mapping=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="\\(n_A, 2\\)"):
        st.tdr.cell_directions(A, B, mapping=by_B)                         # the B side: n_B entries
    shuffled = dict(by_A, pi_index=by_A["pi_index"][::-1].copy())
    with pytest.raises(ValueError, match="arange\\(n_A\\)"):
        st.tdr.cell_directions(A, B, mapping=shuffled)
    twice = by_A["pi_index"].copy()
    twice[1, 0] = 0
    with pytest.raises(ValueError, match="arange\\(n_A\\)"):
        st.tdr.cell_directions(A, B, mapping=dict(by_A, pi_index=twice))
    beyond = by_A["pi_index"].copy()
    beyond[2, 1] = len(g["XB"])
    with pytest.raises(ValueError, match="\\[0, n_B\\)"):
        st.tdr.cell_directions(A, B, mapping=dict(by_A, pi_index=beyond))
    with pytest.raises(ValueError, match="integer array"):
        st.tdr.cell_directions(A, B, mapping=dict(by_A, pi_index=by_A["pi_index"].astype(np.float64)))
    assert "X_mapping" not in A.obsm


# ---- the C ABI, as far as it goes without a device ------------------------------------------------------------------------
def test_c_abi_symbols_and_argument_errors():
    from spateo_amd import _lib

    lib = _lib.load()
    for name in ("mvf_assign_best", "mvf_assign_best_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.mvf_version() == 7                                            # an addition: the ABI version is unchanged
    plain = lib.mvf_assign_workspace_bytes(600, 450)                        # 10 x 8 tiles: 10 row splits, 8 column splits
    assert lib.mvf_assign_best_workspace_bytes(600, 450) == plain + 512 * 8 + 8 * 640 * 24 + 10 * 512 * 24
    assert lib.mvf_assign_best_workspace_bytes(0, 450) == 0 and lib.mvf_assign_best_workspace_bytes(600, 0) == 0
    p = ctypes.c_void_p(256)
    lay = (_lib.AssignLayer * 1)()
    lay[0].Xp = lay[0].Yp = lay[0].a = lay[0].b = 256
    lay[0].ld, lay[0].metric, lay[0].prob, lay[0].param = 16, 2, 0, 0.1
    ws = lib.mvf_assign_best_workspace_bytes(600, 450)

    def run(na=600, nb=450, ws_bytes=ws, outs=(p, p, p, p), mm=p, nl=1, sigma2=0.1):
        return lib.mvf_assign_best(p, na, p, nb, lay, nl, mm, sigma2, 1.0, 0.0, *outs, p, ws_bytes, _lib.MVF_F64, None)

    # refusals report through the status + mvf_last_error channel before any HIP call
    for kw, msg in ((dict(ws_bytes=ws - 1), b"workspace too small"), (dict(ws_bytes=plain), b"workspace too small"),
                    (dict(mm=None), b"null pointer"), (dict(outs=(None, None, None, None)), b"both NULL"),
                    (dict(outs=(p, None, p, p)), b"row_idx and row_val"), (dict(outs=(None, p, p, p)), b"row_idx and row_val"),
                    (dict(outs=(p, p, p, None)), b"col_idx and col_val"), (dict(outs=(None, None, None, None), na=0), b"both NULL"),
                    (dict(nl=0), b"layers"), (dict(nl=5), b"layers"), (dict(sigma2=0.0), b"sigma2 > 0"), (dict(na=-1), b"negative size")):
        assert run(**kw) != 0 and msg in lib.mvf_last_error() and b"mvf_assign_best" in lib.mvf_last_error(), (kw, lib.mvf_last_error())
    assert run(na=0) == 0 and run(nb=0) == 0                                 # an empty side: nothing to do
