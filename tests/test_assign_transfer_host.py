"""CPU tests of the assignment applied to cell features (``mvf_assign_apply`` / ``align.apply_assignment``): the checker of
tests/_assign_transfer_case.py and a NumPy restatement against the golden products of the real ``_update_assignment_P``'s ``P``;
the checker against two stated wrong kernels; the one-hot expansion; every argument error of the Python layer, raised before a
device is touched; and the C entry point's argument rejections, which launch nothing (no GPU needed)."""
import ctypes

import numpy as np
import pytest

import _assign_case as ac
import _assign_edge_cases as ec
import _assign_transfer_case as tc

G = tc.load()
GA = ac.load()
CASES = tc.cases(G)


def test_the_golden_covers_what_it_should():
    assert ("p", 5) in CASES and ("p", 70) in CASES and {c for _, c in CASES} == {5, 70}
    assert any(len(GA[f"{t}_dissimilarity"]) == 2 for t, _ in CASES)            # a case with two layers
    for tag, c in CASES:
        F_A, F_B = tc.features(G, tag, c)
        for F in (F_A, F_B):                                                   # half one-hot, half standard normal
            hot = F[:, : c // 2]
            assert set(np.unique(hot)) == {0.0, 1.0} and (hot.sum(1) == 1).all()
            assert 0.8 < F[:, c // 2:].std() < 1.2
        ref = tc.golden_ref(G, tag, c)
        assert 9 <= int((ref["K_NB"] == 0).sum()) <= 33                        # the far B cells: zero columns of P
        assert not ref["to_B_norm"][ref["K_NB"] == 0].any() and not ref["to_B_raw"][ref["K_NB"] == 0].any()


@pytest.mark.parametrize("tag,c", CASES)
def test_restatement_against_the_golden(tag, c):
    """P of tests/_assign_case.restatement times F: the reference's products at the float64 bound, on the checker's scales."""
    args, kw = ac.case_inputs(GA, tag)
    P = ac.restatement(*args, return_P=True, **kw)["P"]
    F_A, F_B = tc.features(G, tag, c)
    got = tc.products(P, F_A, F_B)
    ref = tc.golden_ref(G, tag, c)
    tc.check(got, ref, tc.tolerances(G, tag, c, "float64"), what=f"restatement {tag} C {c}")
    for q in tc.QUANTITIES:                                                    # and the scales as the file states them
        assert abs(got["scale"][q] - ref["scale"][q]) <= 1e-12 * ref["scale"][q]
    # the stored floors leave the float32 bound where the issue puts it: near 1e-5, never below
    tols = tc.tolerances(G, tag, c, "float32")
    assert all(1e-5 <= tols[q] <= 1e-4 for q in tc.QUANTITIES)


@pytest.mark.parametrize("tag,c", [("p", 70), ("b", 5)])
def test_the_checker_rejects_two_wrong_kernels(tag, c):
    args, kw = ac.case_inputs(GA, tag)
    P = ac.restatement(*args, return_P=True, **kw)["P"]
    F_A, F_B = tc.features(G, tag, c)
    ref = tc.golden_ref(G, tag, c)
    wrong = tc.mutations(P, F_A, F_B)
    assert [n for n, _ in wrong] == ["rows of F permuted inside one 16-row block"] + (["the last 64-column chunk dropped"] if c > 64 else [])
    loosest = tc.tolerances(G, tag, c, "float32")
    for name, got in wrong:
        dev = tc.deviations({q: got[q] for q in tc.QUANTITIES}, ref)
        print(f"  {tag} C {c}: {name}: " + ", ".join(f"{q} {v:.1e}" for q, v in dev.items()))
        for q in tc.QUANTITIES:                                                # every quantity gives it away, in either dtype
            assert dev[q] > 100 * loosest[q], (name, q, dev[q])
        with pytest.raises(AssertionError):
            tc.check({q: got[q] for q in tc.QUANTITIES}, ref, loosest, what=name)


def test_the_checker_wants_zero_rows_for_cells_without_partners():
    ref = tc.golden_ref(G, "p", 5)
    got = {q: ref[q].copy() for q in tc.QUANTITIES}
    got["to_B_norm"][np.flatnonzero(ref["K_NB"] == 0)[0], 0] = 1e-300
    with pytest.raises(AssertionError, match="zero row"):
        tc.deviations(got, ref)


def test_one_hot_expansion():
    from spateo_amd import align

    lab = np.array([2, 0, 0, 3, 1], dtype=np.int32)
    F = align._transfer_features(lab, 5, "features_A")
    assert F.dtype == np.float64 and F.shape == (5, 4) and np.array_equal(F.argmax(1), lab) and (F.sum(1) == 1).all()
    assert align._transfer_features(np.array([0, 0]), 2, "features_B").shape == (2, 1)
    assert align._transfer_features(np.zeros(0, dtype=np.int64), 0, "features_B").shape == (0, 1)
    # a 1-D FLOAT vector is no label vector, an (n, 1) integer matrix is a feature column
    with pytest.raises(ValueError, match="one row per cell"):
        align._transfer_features(np.array([0.0, 1.0]), 2, "features_A")
    one = align._transfer_features(np.array([[3], [4]]), 2, "features_A")
    assert one.dtype == np.float64 and np.array_equal(one, [[3.0], [4.0]])
    assert align._transfer_features(None, 7, "features_A") is None


def _no_device(monkeypatch):
    from spateo_amd import _runtime as rt

    def touched(*a, **k):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(rt, "_make_kernels", touched)
    monkeypatch.setattr(rt, "_shared_kernels", touched)


def test_argument_errors_come_before_any_device(monkeypatch):
    import scipy.sparse as sp
    from spateo_amd import align

    _no_device(monkeypatch)
    args, kw = ac.case_inputs(GA, "p")
    NA, NB = len(args[0]), len(args[1])
    F_A, F_B = tc.features(G, "p", 5)
    call = lambda **over: align.apply_assignment(*args, **dict(kw, **over))  # noqa: E731
    with pytest.raises(ValueError, match="features_A or features_B"):
        call()
    with pytest.raises(ValueError, match="one row per cell"):
        call(features_A=F_A[:-1])
    with pytest.raises(ValueError, match="one row per cell"):
        call(features_B=F_B[:, 0])                       # a 1-D float vector
    with pytest.raises(ValueError, match="one row per cell"):
        call(features_B=F_A)                              # the other slice's
    with pytest.raises(ValueError, match="one entry per cell"):
        call(features_A=np.zeros(NA + 1, dtype=np.int64))
    with pytest.raises(ValueError, match="non-negative"):
        call(features_A=np.full(NA, -1))
    with pytest.raises(ValueError, match="at least one column"):
        call(features_B=np.zeros((NB, 0)))
    for bad in (np.nan, np.inf):
        F = F_B.copy()
        F[3, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            call(features_B=F)
    with pytest.raises(ValueError, match="numeric"):
        call(features_A=np.array([["a"]] * NA))
    with pytest.raises(NotImplementedError, match="scipy.sparse features_A"):
        call(features_A=sp.csr_matrix(F_A))
    with pytest.raises(NotImplementedError, match="scipy.sparse features_B"):
        call(features_B=sp.coo_matrix(F_B))
    # update_assignment's own errors
    with pytest.raises(ValueError, match="dtype"):
        call(features_A=F_A, dtype="float16")
    with pytest.raises(ValueError, match="alpha and SigmaDiag"):
        call(features_A=F_A, alpha=kw["alpha"][:-1])
    with pytest.raises(ValueError, match="Unsupported dissimilarity"):
        call(features_A=F_A, dissimilarity=["nope", "cos"])
    with pytest.raises(NotImplementedError, match="apply_assignment: spatial coordinates"):
        align.apply_assignment(np.zeros((4, 4)), np.zeros((3, 4)), [np.ones((4, 2))], [np.ones((3, 2))], features_A=np.ones((4, 1)),
                               **dict(kw, dissimilarity=["kl"], probability_type=["gauss"], probability_parameters=[1.0],
                                      alpha=np.ones(4), SigmaDiag=np.zeros(4)))
    # an empty side: zeros of the right shape, and still no device
    small = dict(kw, dissimilarity=["kl"], probability_type=["gauss"], probability_parameters=[1.0])
    out = align.apply_assignment(np.zeros((0, 3)), np.zeros((4, 3)), [np.zeros((0, 2))], [np.ones((4, 2))],
                                 features_A=np.zeros((0, 3)), features_B=np.ones((4, 2)),
                                 **dict(small, alpha=np.zeros(0), SigmaDiag=np.zeros(0)))
    assert sorted(out) == ["K_NA", "K_NB", "to_A", "to_B"]
    assert out["to_A"].shape == (0, 2) and out["to_B"].shape == (4, 3) and out["K_NA"].shape == (0,) and out["K_NB"].shape == (4,)
    assert not out["to_B"].any() and not out["K_NB"].any()
    out = align.apply_assignment(np.zeros((5, 3)), np.zeros((0, 3)), [np.ones((5, 2))], [np.zeros((0, 2))],
                                 features_A=np.arange(5) % 3, **dict(small, alpha=np.ones(5), SigmaDiag=np.zeros(5)))
    assert sorted(out) == ["K_NB", "to_B"] and out["to_B"].shape == (0, 3)


def test_the_loops_validate_apply_before_any_device(monkeypatch):
    import _align_loop_case as lc
    from spateo_amd import align

    _no_device(monkeypatch)
    args, kw = lc.case_inputs(lc.load(), "3")
    kw = dict(kw, max_iter=2)
    NA, NB = len(args[0]), len(args[1])
    for loop in (align.morpho_iterate, align.morpho_iterate_svi):
        with pytest.raises(ValueError, match="apply must be a dict"):
            loop(*args, apply=np.ones((NA, 2)), **kw)
        with pytest.raises(ValueError, match="apply must be a dict"):
            loop(*args, apply=dict(features=np.ones((NA, 2))), **kw)
        with pytest.raises(ValueError, match="needs features_A or features_B"):
            loop(*args, apply=dict(normalize=False), **kw)
        with pytest.raises(ValueError, match=f"{loop.__name__}: features_B must have one row per cell"):
            loop(*args, apply=dict(features_B=np.ones((NB + 1, 2))), **kw)
    ok = align._apply_argument(dict(features_A=np.arange(NA) % 4), NA, NB, "x")
    assert ok["FA"].shape == (NA, 4) and ok["FB"] is None and ok["normalize"] is True


def test_the_sparse_modes_host_product():
    """sparse_calculation_mode: `applied` is the returned coo_matrix times F - the kept entries, their sums beside them."""
    from scipy.sparse import coo_matrix
    from spateo_amd import align

    rng = np.random.default_rng(5)
    dense = rng.random((7, 5)) * (rng.random((7, 5)) < 0.4)
    dense[:, 2] = 0.0                                                           # a column without partners
    P = coo_matrix(dense)
    FA, FB = rng.standard_normal((7, 3)), rng.standard_normal((5, 2))
    raw = align._applied_from_coo(P, dense.sum(1), dense.sum(0), FA, FB, False)
    assert np.allclose(raw["to_A"], dense @ FB, rtol=0, atol=1e-15) and np.allclose(raw["to_B"], dense.T @ FA, rtol=0, atol=1e-15)
    norm = align._applied_from_coo(P, dense.sum(1), dense.sum(0), FA, FB, True)
    want = tc.products(dense, FA, FB)
    assert np.allclose(norm["to_A"], want["to_A_norm"], rtol=0, atol=1e-14) and np.allclose(norm["to_B"], want["to_B_norm"], rtol=0, atol=1e-14)
    assert not norm["to_B"][2].any()
    only = align._applied_from_coo(P, dense.sum(1), dense.sum(0), FA, None, True)
    assert sorted(only) == ["K_NB", "to_B"]


# ---- the C entry point: every refusal is reported before anything is launched (none of the pointers is ever dereferenced)
def test_workspace_size_function():
    from spateo_amd import _lib

    lib = _lib.load()
    for na, nb in [(1, 1), (65, 63), (129, 257), (4417, 50), (50, 4417), (2500, 2500), (100000, 100000)]:
        for cb, ca in [(1, 0), (0, 1), (5, 70), (64, 64), (17, 129), (200, 3)]:
            assert int(lib.mvf_assign_apply_workspace_bytes(na, nb, cb, ca)) == tc.workspace_bytes(na, nb, cb, ca), (na, nb, cb, ca)
    for na, nb in ((0, 5), (5, 0), (0, 0), (-1, 5)):
        assert int(lib.mvf_assign_apply_workspace_bytes(na, nb, 4, 4)) == 0
    assert int(lib.mvf_assign_apply_workspace_bytes(5, 5, -1, 4)) == 0
    # 100 000 x 100 000 cells, 64 columns either way: a few hundred MB, against the 80 GB of P
    assert tc.workspace_bytes(100000, 100000, 64, 64) < 200e6


def test_the_c_entry_rejects_bad_arguments_without_a_launch():
    from spateo_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(1)
    na, nb, cb, ca = 70, 66, 5, 70
    need = int(lib.mvf_assign_apply_workspace_bytes(na, nb, cb, ca))
    arr = (_lib.AssignLayer * 1)()
    arr[0].Xp, arr[0].Yp, arr[0].a, arr[0].b, arr[0].ld = 1, 1, 1, 1, 32
    arr[0].metric, arr[0].prob, arr[0].param = _lib.ASSIGN_METRICS["kl"], _lib.ASSIGN_PROBS["gauss"], 0.5

    def call(xa4=p, na=na, nb=nb, layers=arr, nlayers=1, mm=p, sigma2=0.1, variance=1.0, outlier=0.01, FB=p, cb=cb, ldfb=cb, to_A=p,
             FA=p, ca=ca, ldfa=ca, to_B=p, K_NA=p, K_NB=p, ws=p, ws_bytes=need, dtype=_lib.MVF_F64):
        rc = lib.mvf_assign_apply(xa4, na, p, nb, layers, nlayers, mm, sigma2, variance, outlier, FB, cb, ldfb, to_A, FA, ca, ldfa,
                                  to_B, K_NA, K_NB, ws, ws_bytes, dtype, None)
        return rc, lib.mvf_last_error().decode("utf-8", "replace")

    refused = [
        (dict(FB=None, cb=0, to_A=None, K_NA=None, FA=None, ca=0, to_B=None), "both directions are skipped"),
        (dict(to_A=None), "to skip P @ FB"), (dict(FB=None), "to skip P @ FB"), (dict(cb=0), "to skip P @ FB"),
        (dict(FB=None, to_A=None, K_NA=None), "to skip P @ FB"),                   # cb still 5
        (dict(to_B=None), "to skip P^T @ FA"), (dict(FA=None), "to skip P^T @ FA"), (dict(ca=-3), "to skip P^T @ FA"),
        (dict(FB=None, cb=0, to_A=None), "K_NA rides with P @ FB"),
        (dict(ldfb=cb - 1), "ld is below"), (dict(ldfa=ca - 1), "ld is below"),
        (dict(ws_bytes=need - 1), "workspace too small"), (dict(ws=None), "null pointer"), (dict(xa4=None), "null pointer"),
        (dict(mm=None), "null pointer"), (dict(layers=None), "null pointer"),
        (dict(dtype=7), "bad dtype"), (dict(nlayers=0), "layers"), (dict(nlayers=5), "layers"),
        (dict(sigma2=0.0), "sigma2 > 0"), (dict(variance=-1.0), "sigma2 > 0"), (dict(outlier=-1.0), "outlier >= 0"),
        (dict(na=-1), "negative size"), (dict(na=1 << 31), "too many cells"),
    ]
    for kw, text in refused:
        rc, msg = call(**kw)
        assert rc != 0 and "mvf_assign_apply" in msg and text in msg, (kw, msg)
    bad = (_lib.AssignLayer * 1)()
    bad[0].Xp, bad[0].Yp, bad[0].a, bad[0].b, bad[0].ld = 1, 1, 1, 1, 30           # ld no multiple of 16
    bad[0].metric, bad[0].prob, bad[0].param = _lib.ASSIGN_METRICS["kl"], _lib.ASSIGN_PROBS["gauss"], 0.5
    rc, msg = call(layers=bad)
    assert rc != 0 and "multiple of 16" in msg
    # an empty side: nothing to do, nothing launched - but a wrong mix of the direction's arguments is still an error
    assert call(na=0)[0] == 0 and call(nb=0)[0] == 0
    assert call(na=0, to_A=None)[0] != 0
    # K_NA / K_NB may be NULL, one direction may be skipped: accepted up to the first thing that needs a device - checked on
    # an empty side, where the call returns before it
    assert call(na=0, K_NA=None, K_NB=None)[0] == 0
    assert call(na=0, FB=None, cb=0, to_A=None, K_NA=None)[0] == 0
    assert call(na=0, FA=None, ca=0, to_B=None)[0] == 0
    assert ec.TILE == 64 and tc.CHUNK == 64


# ---- Morpho_pairwise(apply=): the strings are looked up at construction, before anything runs
def test_morpho_pairwise_resolves_the_strings():
    import _morpho_align_case as mc
    from spateo_amd import align

    M = mc.load()
    A, B = mc.pair_samples(M, "1")
    make = lambda **over: align.Morpho_pairwise(A, B, dtype="float64", verbose=False, **mc.pair_kwargs(M, "1", **over))  # noqa: E731
    m = make(apply=dict(features_A="celltype", features_B="spatial", normalize=False))
    cats = list(A.obs["celltype"].cat.categories)
    assert m._apply_categories == {"categories_A": cats} and m._apply["normalize"] is False
    assert np.array_equal(m._apply["features_A"], np.eye(len(cats))[np.asarray(A.obs["celltype"].cat.codes)])   # category order
    assert np.array_equal(m._apply["features_B"], B.obsm["spatial"]) and m.applied is None
    assert m._P_fits()
    arrays = make(apply=dict(features_B=np.ones((m.NB, 3))))
    assert arrays._apply_categories == {} and "features_A" not in arrays._apply
    assert make()._apply is None
    with pytest.raises(KeyError, match="neither an obs column nor an obsm key"):
        make(apply=dict(features_A="nope"))
    with pytest.raises(ValueError, match="apply must be a dict"):
        make(apply="celltype")
    with pytest.raises(ValueError, match="one row per cell"):
        make(apply=dict(features_A=np.ones((m.NA + 1, 2))))
    A.obs["depth"] = np.linspace(0, 1, m.NA)
    with pytest.raises(ValueError, match="not categorical"):
        make(apply=dict(features_A="depth"))
