"""CPU tests of the alignment's ``sparse_calculation_mode`` (``mvf_assign_topk``; ``update_assignment``, ``morpho_iterate`` and
``morpho_iterate_svi`` with ``sparse_calculation_mode=True``): the masked restatement the GPU suite compares with is pinned to
goldens of the real ``_update_assignment_P`` in that mode (tests/golden/make_golden_assign_topk.py,
make_golden_align_loop_topk.py); the public functions run through the kernel seam on NumPy stand-ins
(``_assign_topk_case.CpuTopkKernels``) against the same goldens; the coo layout, the argument errors, the clamp to NA,
``top_k = 1``; and the checker of ``_assign_topk_case`` is shown to reject the wrong answers it exists for."""
import ctypes

import numpy as np
import pytest

import _align_loop_case as lc
import _align_svi_case as sc
import _assign_case as ac
import _assign_topk_case as tk

G = tk.load()
KEYS = tk.case_keys(G)
API_KEYS = [(t, k) for t, k in KEYS if k <= 64]   # (the golden with k above NA = 149 pins the restatement's clamp; the public
# functions refuse a k above the device's cap of 64, and their clamp is tested on a 5-row slice of that case)


def _positive_lists_agree(rows, vals, grows, gvals, tol):
    """The reference's lists against ours: equal shapes, values within tol of the largest, the same rows wherever the value
    is positive (among exact zeros the reference's sort keeps no particular row)."""
    assert rows.shape == grows.shape and vals.shape == gvals.shape
    assert np.abs(vals - gvals).max() <= tol * gvals.max()
    pos = gvals > 0
    assert np.array_equal(rows[pos], grows[pos])
    assert not vals[~pos].any()


# ---- the goldens and the restatement --------------------------------------------------------------------------------------
def test_goldens_cover_the_mode():
    ks = {k for _, k in KEYS}
    assert {1, 8, 64} <= ks and len(KEYS) >= 6
    shapes = {t: (len(G[f"{t}_XAHat"]), len(G[f"{t}_coordsB"])) for t, _ in KEYS}
    assert any(k > shapes[t][0] for t, k in KEYS)                        # one k above NA: the clamp
    assert any(na < 200 for na, _ in shapes.values()) and sum(na > 500 for na, _ in shapes.values()) >= 2
    assert any(G[f"{t}_XAHat"].shape[1] == 2 for t, _ in KEYS) and any(len(G[f"{t}_dissimilarity"]) == 2 for t, _ in KEYS)
    for t, k in KEYS:
        assert float(G[f"{t}_k{k}_gap"]) >= 1000 * ac.F64_TOL               # no selection hangs on a near tie
        assert float(G[f"{t}_k{k}_near"]) <= tk.MAX_LEFT_OUT                # a float32 comparison leaves out <= 5 % columns
        assert float(G[f"{t}_k{k}_floor_chunk"].max()) <= 1e-13
        far = G[f"{t}_far"]
        assert len(far) >= 0.05 * shapes[t][1] and not G[f"{t}_k{k}_K_NB"][far].any()
    L = tk.load_loop()
    assert [str(t) for t in L["cases"]] == lc.case_tags() and int(L["top_k"]) == 16 and int(L["iters"]) == int(lc.load()["iters"])
    for t in lc.case_tags():
        assert float(L[f"{t}_gap"]) >= 1000 * ac.F64_TOL
        assert max(float(L[f"{t}_chunk_{q}"].max()) for q in lc.SCALARS + lc.ARRAYS + lc.FINALS) <= 1e-9
        assert not np.allclose(L[f"{t}_Sp"], lc.load()[f"{t}_Sp"], rtol=1e-6)   # the mode changes the numbers


@pytest.mark.parametrize("tag,k", KEYS)
def test_masked_restatement_reproduces_the_reference_goldens(tag, k):
    """Same arithmetic, same precision: 1e-12 relative to each quantity's maximum; the lists are the reference's."""
    args, kw = ac.case_inputs(G, tag)
    r = tk.restatement(*args, k=k, **kw)
    dev = ac.deviations(r, tk.golden_ref(G, tag, k))
    assert max(dev.values()) <= 1e-12, (tag, k, dev)
    _positive_lists_agree(r["rows"], r["vals"], *tk.golden_lists(G, tag, k), 1e-12)
    dense = ac.restatement(*args, **kw)
    for q in ("K_NA_spatial", "K_NA_sigma2", "sigma2_related", "Sp_spatial", "Sp_sigma2"):
        assert np.array_equal(r[q], dense[q]), q                            # what stays dense
    assert r["Sp"] <= dense["Sp"] and np.all(r["K_NA"] <= dense["K_NA"])
    # the restatement's own result passes the checker (and the reference's selection is the one the checker calls optimal)
    XB = np.asarray(args[1], dtype=np.float64)
    tk.check(r, r["P"], XB, k, ac.F64_TOL, what=f"restatement {tag} k {k}")


# ---- the public functions through the seam --------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,k", API_KEYS)
def test_update_assignment_through_the_seam(tag, k, monkeypatch):
    from scipy.sparse import coo_matrix

    from spateo_amd import align

    args, kw = ac.case_inputs(G, tag)
    NA, D = args[0].shape
    NB = len(args[1])
    tk.cpu_topk_kernels(monkeypatch, D)
    got = align.update_assignment(*args, sparse_calculation_mode=True, sparse_top_k=k, **kw)
    ac.check(got, tk.golden_ref(G, tag, k), tk.tolerances(G, tag, k, "float64"), f"update_assignment {tag} k {k} on stand-ins")
    # the coo layout is the reference's: col = repeat(arange(NB), k_eff), rows and values from the lists
    P, ke = got["P"], min(k, NA)
    assert isinstance(P, coo_matrix) and P.shape == (NA, NB) and P.data.dtype == np.float64
    assert np.array_equal(P.col, G[f"{tag}_k{k}_col"]) and np.array_equal(P.col, np.repeat(np.arange(NB), ke))
    rows, vals = tk.coo_lists(P, NB)
    assert np.array_equal(rows, got["topk_rows"]) and np.array_equal(vals, got["topk_values"])
    assert got["topk_rows"].dtype == np.int32 and got["topk_rows"].shape == (NB, ke)
    _positive_lists_agree(rows, vals, *tk.golden_lists(G, tag, k), ac.F64_TOL)
    dense = ac.restatement(*args, return_P=True, **kw)
    tk.check(dict(rows=rows, vals=vals, K_NA=got["K_NA"], K_NB=got["K_NB"], PXB=got["PXB"]), dense["P"], args[1], k, ac.F64_TOL,
             what=f"update_assignment {tag} k {k}")
    assert abs(P.sum() - got["Sp"]) <= 1e-12 * got["Sp"]


def test_k_above_na_is_the_dense_result_and_k_1_the_column_argmax(monkeypatch):
    from spateo_amd import align

    args, kw = ac.case_inputs(G, "s")
    NA, NB = len(args[0]), len(args[1])
    tk.cpu_topk_kernels(monkeypatch, args[0].shape[1])
    dense = ac.restatement(*args, return_P=True, **kw)
    full = align.update_assignment(*args, sparse_calculation_mode=True, sparse_top_k=64, **dict(kw))   # (64 < NA = 149: sparse)
    assert full["topk_rows"].shape == (NB, 64) and full["Sp"] < dense["Sp"]
    a5 = [args[0][:5], args[1], [a[:5] for a in args[2]], args[3]]
    kw5 = dict(kw, alpha=kw["alpha"][:5], SigmaDiag=kw["SigmaDiag"][:5])
    clamp = align.update_assignment(*a5, sparse_calculation_mode=True, sparse_top_k=64, **kw5)             # 64 > NA = 5: the clamp
    assert clamp["topk_rows"].shape == (NB, 5) and clamp["P"].shape == (5, NB)
    ac.check(clamp, ac.restatement(*a5, **kw5), {q: 1e-12 for q in ac.QUANTITIES}, "k above NA against the dense result")
    one = align.update_assignment(*args, sparse_calculation_mode=True, sparse_top_k=1, **kw)
    live = dense["P"].max(0) > 0
    assert live.sum() >= 0.9 * NB
    assert np.array_equal(one["topk_rows"][live, 0], dense["P"].argmax(0)[live])
    assert np.abs(one["K_NB"] - dense["P"].max(0)).max() <= 1e-12 * dense["P"].max()
    assert not one["topk_rows"][~live].any()                                # an all-zero column: row 0


@pytest.mark.parametrize("tag", lc.case_tags())
def test_morpho_iterate_through_the_seam(tag, monkeypatch):
    """`morpho_iterate(sparse_calculation_mode=True, sparse_top_k=16)` on the stand-ins against the real reference loop in
    that mode: per iteration and quantity within the float64 bound 1e-10 max(1, 1.25 g_k) of the GPU suite."""
    from spateo_amd import align

    L = tk.load_loop()
    args, kw = lc.case_inputs(lc.load(), tag)
    NA, NB = len(args[0]), len(args[1])
    tk.cpu_topk_kernels(monkeypatch, args[0].shape[1])
    out = align.morpho_iterate(*args, record="arrays", sparse_calculation_mode=True, sparse_top_k=int(L["top_k"]), **kw)
    got = dict(out["history"], optimal_R=out["optimal_R"], optimal_t=out["optimal_t"])
    tol = lc.bounds(L, tag, lc.F64_TOL)
    lc.check(lc.deviations(got, L, tag), tol, f"case {tag} top-k loop on stand-ins")
    rows, vals = tk.coo_lists(out["P"], NB)
    assert out["P"].shape == (NA, NB) and rows.shape == (NB, 16)
    _positive_lists_agree(rows, vals, L[f"{tag}_P_row"].reshape(NB, 16), L[f"{tag}_P_data"].reshape(NB, 16), float(tol["K_NA"][-1]))
    assert np.abs(np.asarray(out["P"].sum(1)).ravel() - out["K_NA"]).max() <= 1e-12 * out["K_NA"].max()


@pytest.mark.parametrize("tag", sc.case_tags(tk.load_svi()))
def test_morpho_iterate_svi_through_the_seam_against_the_fixture(tag, monkeypatch):
    """`morpho_iterate_svi(sparse_calculation_mode=True, sparse_top_k=16, return_mapping=True)` on the stand-ins against the
    real reference SVI loop in that mode, at the float64 bound of the GPU suite; P is the closing full assignment's."""
    from spateo_amd import align

    S = tk.load_svi()
    args, kw = sc.case_inputs(S, tag)
    NA, NB = len(args[0]), len(args[1])
    tk.cpu_topk_kernels(monkeypatch, args[0].shape[1])
    out = align.morpho_iterate_svi(*args, record="arrays", return_mapping=True, sparse_calculation_mode=True,
                                   sparse_top_k=int(S["top_k"]), **kw)
    got = dict(out["history"], optimal_R_map=out["optimal_R"], optimal_t_map=out["optimal_t"], Sp_map=out["Sp"])
    tol = sc.bounds(S, tag, sc.F64_TOL, finals=sc.FINALS_MAP)
    sc.check(sc.deviations(got, S, tag, sc.FINALS_MAP), tol, f"case {tag} top-k SVI loop on stand-ins")
    np.testing.assert_array_equal(out["history"]["step_size"], S[f"{tag}_step_size"])
    rows, vals = tk.coo_lists(out["P"], NB)
    assert out["P"].shape == (NA, NB) and rows.shape == (NB, 16) and float(S[f"{tag}_gap"]) >= 1000 * ac.F64_TOL
    _positive_lists_agree(rows, vals, S[f"{tag}_P_row"].reshape(NB, 16), S[f"{tag}_P_data"].reshape(NB, 16), float(tol["K_NA"][-1]))


def test_morpho_iterate_svi_routes_every_assignment_through_assign_topk(monkeypatch):
    """The SVI loop in the mode: every assignment goes through assign_topk (never assign), the batches' lists are clamped to
    NA and have batch_size columns, and P comes back only from the closing full assignment."""
    from spateo_amd import _runtime as rt
    from spateo_amd import align

    S = sc.load()
    args, kw = sc.case_inputs(S, sc.case_tags(S)[0])
    NA, NB = len(args[0]), len(args[1])
    tk.cpu_topk_kernels(monkeypatch, args[0].shape[1])
    calls = []
    make = rt._make_kernels

    def counting(device, dtype):
        k = make(device, dtype)
        inner = k.assign_topk

        def assign_topk(xa4, xb4, *a):
            r = inner(xa4, xb4, *a)
            calls.append((len(xb4), tuple(r["rows"].shape), a[-1]))
            return r

        k.assign_topk = assign_topk
        k.assign = None   # the dense kernel must not be reached
        return k

    monkeypatch.setattr(rt, "_make_kernels", counting)
    kw = dict(kw, max_iter=4)
    out = align.morpho_iterate_svi(*args, record=True, return_mapping=True, sparse_calculation_mode=True, sparse_top_k=16, **kw)
    bs = out["batch_size"]
    assert calls == [(bs, (bs, 16), 16)] * 4 + [(NB, (NB, 16), 16)]
    rows, vals = tk.coo_lists(out["P"], NB)
    assert out["P"].shape == (NA, NB) and rows.shape == (NB, 16)
    assert np.abs(np.asarray(out["P"].sum(1)).ravel() - out["K_NA"]).max() <= 1e-12 * out["K_NA"].max()
    assert np.abs(np.asarray(out["P"].sum(0)).ravel() - out["K_NB"]).max() <= 1e-12 * out["K_NB"].max()
    assert abs(out["P"].sum() - out["Sp"]) <= 1e-12 * out["Sp"]
    del calls[:]
    plain = align.morpho_iterate_svi(*args, record=False, sparse_calculation_mode=True, sparse_top_k=16, **kw)
    assert "P" not in plain and len(calls) == 4 and len(plain["K_NB"]) == bs
    dense = sc.CpuLoopKernels   # and with the mode off the loop is the one it was: assign, never assign_topk
    monkeypatch.setattr(rt, "_make_kernels", lambda device, dtype: _with_D(dense(device, dtype), args[0].shape[1]))
    off = align.morpho_iterate_svi(*args, record=False, **kw)
    assert "P" not in off and not np.allclose(off["K_NA"], plain["K_NA"], rtol=1e-9)


def _with_D(k, D):
    k.D = D
    return k


# ---- arguments ------------------------------------------------------------------------------------------------------------
def _call(fn="update_assignment", **over):
    from spateo_amd import align

    if fn == "update_assignment":
        args, kw = ac.case_inputs(G, "s")
    else:
        args, kw = lc.case_inputs(lc.load(), "1")
    kw.update(over)
    return getattr(align, fn)(*args, **kw)


@pytest.mark.parametrize("fn", ["update_assignment", "morpho_iterate", "morpho_iterate_svi"])
def test_argument_errors_of_the_public_functions(fn):
    import inspect

    from spateo_amd import _lib, align

    assert inspect.signature(getattr(align, fn)).parameters["sparse_top_k"].default == 1024    # morpho_class.py:140
    assert "sparse_calculation_mode" in getattr(align, fn).__doc__ and "sparse_top_k" in getattr(align, fn).__doc__
    cap = _lib.ASSIGN_TOPK_MAX
    assert cap == 64
    for k in (cap + 1, 1024, 10**6):   # the requested value is tested, before the clamp to NA
        with pytest.raises(NotImplementedError, match=rf"sparse_calculation_mode.*{k}.*{cap}"):
            _call(fn, sparse_calculation_mode=True, sparse_top_k=k)
    with pytest.raises(NotImplementedError, match="sparse_calculation_mode"):
        _call(fn, sparse_calculation_mode=True)                               # the default, 1024
    for k in (0, -3, 2.5):
        with pytest.raises(ValueError, match="sparse_top_k"):
            _call(fn, sparse_calculation_mode=True, sparse_top_k=k)
    if fn == "update_assignment":
        with pytest.raises(ValueError, match="return_P"):
            _call(fn, sparse_calculation_mode=True, sparse_top_k=8, return_P=True)
    with pytest.raises(NotImplementedError, match="label"):                    # the other refusals come first as before
        _call(fn, sparse_calculation_mode=True, sparse_top_k=8, dissimilarity=["label"])


def test_empty_slices_in_the_mode_return_an_empty_mapping():
    from spateo_amd import align

    args, kw = ac.case_inputs(G, "s")

    out = align.update_assignment(args[0], np.zeros((0, 3)), args[2], [np.zeros((0, a.shape[1])) for a in args[3]],
                                  sparse_calculation_mode=True, sparse_top_k=8, **kw)
    assert out["P"].shape == (len(args[0]), 0) and out["topk_rows"].shape == (0, 8) and out["Sp"] == 0.0


def test_c_abi_symbols_and_argument_errors():
    from spateo_amd import _lib

    lib = _lib.load()
    for name in ("mvf_assign_topk", "mvf_assign_topk_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.mvf_version() == 7                                            # an addition: the ABI version is unchanged
    plain = lib.mvf_assign_workspace_bytes(600, 450)                        # 10 x 8 tiles: 10 row splits
    assert lib.mvf_assign_topk_workspace_bytes(600, 450, 8) == plain + 10 * 8 * 512 * (8 + 4)   # + the splits' lists
    assert lib.mvf_assign_topk_workspace_bytes(5, 450, 64) == lib.mvf_assign_workspace_bytes(5, 450) + 5 * 512 * (8 + 4)
    for k in (0, -1, 65):
        assert lib.mvf_assign_topk_workspace_bytes(600, 450, k) == 0
    assert lib.mvf_assign_topk_workspace_bytes(0, 450, 8) == 0 and lib.mvf_assign_topk_workspace_bytes(600, 0, 8) == 0
    p = ctypes.c_void_p(256)
    lay = (_lib.AssignLayer * 1)()
    lay[0].Xp = lay[0].Yp = lay[0].a = lay[0].b = 256
    lay[0].ld, lay[0].metric, lay[0].prob, lay[0].param = 16, 2, 0, 0.1
    ws = lib.mvf_assign_topk_workspace_bytes(600, 450, 8)

    def run(na=600, nb=450, k=8, ws_bytes=ws, rows=p, vals=p, nl=1):
        return lib.mvf_assign_topk(p, na, p, nb, lay, nl, p, 0.1, 1.0, 0.0, k, p, p, p, p, p, p, rows, vals, p, ws_bytes,
                                   _lib.MVF_F64, None)

    # refusals report through the status + mvf_last_error channel before any HIP call
    for kw, msg in ((dict(k=0), b"1 <= k <= 64"), (dict(k=65), b"1 <= k <= 64"), (dict(k=-1), b"1 <= k <= 64"),
                    (dict(k=0, na=0), b"1 <= k <= 64"), (dict(ws_bytes=ws - 1), b"workspace too small"),
                    (dict(ws_bytes=lib.mvf_assign_workspace_bytes(600, 450)), b"workspace too small"),
                    (dict(rows=None), b"null pointer"), (dict(vals=None), b"null pointer"), (dict(nl=0), b"layers")):
        assert run(**kw) != 0 and msg in lib.mvf_last_error() and b"mvf_assign_topk" in lib.mvf_last_error(), (kw, lib.mvf_last_error())
    assert run(na=0) == 0 and run(nb=0) == 0                                 # an empty side with a valid k: nothing to do


# ---- the checker rejects what it exists for -------------------------------------------------------------------------------
def test_the_checker_rejects_each_wrong_answer():
    args, kw = ac.case_inputs(G, "s")
    k = 8
    r = tk.restatement(*args, k=k, **kw)
    P, XB = r["P"], np.asarray(args[1], dtype=np.float64)
    NA, NB = P.shape
    good = {q: r[q] for q in ("rows", "vals", "K_NA", "K_NB", "PXB")}
    tk.check(good, P, XB, k, ac.F64_TOL, what="the right answer")

    def with_lists(rows, vals=None):
        rows = np.asarray(rows, dtype=np.int32)
        vals = P[rows.astype(np.int64), np.arange(NB)[:, None]] if vals is None else vals
        out = dict(rows=rows, vals=vals)
        out.update(tk.masked_sums(P, rows, XB))   # (sums consistent with the wrong lists: the selection alone is wrong)
        return out

    wrong = {}
    # selection along the wrong axis: the k largest of every ROW, handed back in the (NB, k) layout
    by_row = np.argsort(-P, axis=1, kind="stable")[:, :k]
    wrong["the wrong axis"] = with_lists(np.resize(by_row, (NB, k)) % NA)
    wrong["k - 1 entries"] = with_lists(r["rows"][:, :k - 1])
    wrong["k + 1 entries"] = with_lists(tk.top_lists(P, k + 1)[0])
    gap, _ = tk.reference_gaps(P, k)
    j = int(np.argmax(gap * (P.max(0) > 0)))                 # the column whose k-th entry stands clearest above the rest
    swapped = r["rows"].copy()
    swapped[j, -1] = np.argsort(-P[:, j], kind="stable")[k]   # its (k + 1)-th row in the k-th place
    wrong["one swapped sub-optimal row"] = with_lists(swapped)
    wrong["unsorted lists"] = with_lists(r["rows"][:, ::-1])
    rep = r["rows"].copy()
    rep[:, 1] = rep[:, 0]
    wrong["repeated rows"] = with_lists(rep, r["vals"])
    dense = ac.restatement(*args, **kw)
    wrong["K_NA taken from the dense P"] = dict(good, K_NA=dense["K_NA"])
    for name, bad in wrong.items():
        with pytest.raises(AssertionError):
            tk.check(bad, P, XB, k, ac.F64_TOL, what=name)
        print(f"  rejected: {name}")
    assert len(wrong) == 7
