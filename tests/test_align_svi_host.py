"""CPU proofs around the SVI mode of the alignment loop (``spateo_amd.align.morpho_iterate_svi``): the NumPy restatement of
tests/_align_svi_case.py against the fixture tests/golden/ref_align_svi.npz (real reference code with ``SVI_mode=True``, 30
iterations of 150-cell batches, cases 1 - 3 of the dense fixture and case 3 with a late non-rigid start), the batch schedule,
the default ``batch_size``, the host half of an SVI iteration, and the validation / refusals of ``morpho_iterate_svi`` (no
device needed).

Bound of the restatement: ``1e-12 max(1, 1.25 g_k)`` per case, iteration and quantity, as for the dense loop
(tests/test_align_loop_host.py)."""
import numpy as np
import pytest

import _align_loop_case as lc
import _align_svi_case as sc

G = sc.load()
TAGS = sc.case_tags(G)
_RUNS = {}


def _run(tag):
    if tag not in _RUNS:
        args, kw = sc.case_inputs(G, tag)
        _RUNS[tag] = sc.restatement(*args, return_mapping=True, **kw)
    return _RUNS[tag]


@pytest.mark.parametrize("q", sc.SCALARS + sc.ARRAYS + sc.FINALS + sc.FINALS_MAP)
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_fixture(tag, q):
    finals = sc.FINALS + sc.FINALS_MAP
    dev = sc.deviations(_run(tag), G, tag, finals)
    tol = sc.bounds(G, tag, sc.HOST_TOL, finals=finals)
    sc.check({q: dev[q]}, {q: tol[q]}, f"case {tag} SVI restatement")


def test_fixture_conditions():
    iters, bs = int(G["iters"]), int(G["batch_size"])
    assert iters == 30 and bs == 150 and TAGS == ["1", "2", "3", "3n"] and list(G["arr_iters"]) == [0, 9, 19, 29]
    for tag in TAGS:
        NB = len(G[f"{tag}_batch_perm"])
        assert bs % 64 != 0 and NB % bs != 0 and bs * iters > NB          # the roll wraps, several times
        for q in sc.SCALARS + sc.ARRAYS + sc.FINALS + sc.FINALS_MAP:
            assert np.isfinite(G[f"{tag}_{q}"]).all(), (tag, q)
            assert float(G[f"{tag}_g_{q}"].max()) <= 100.0, (tag, q)
        assert int(G[f"{tag}_nonrigid_runs"]) >= 8
        assert np.linalg.norm(G[f"{tag}_R"][-1] - lc.load()[f"{G[f'{tag}_inputs_of']}_R0"]) <= 0.05
        np.testing.assert_array_equal(G[f"{tag}_step_size"], np.minimum(1.0, 10.0 / (np.arange(iters) + 1.0)))
        assert G[f"{tag}_step_size"][-1] == 1.0 / 3.0
    # case 3n: the first non-rigid update (iteration 12, step 10/13) is blended against zeros
    assert int(G["3n_nonrigid_start_iter"]) == 11 and int(G["3n_nonrigid_runs"]) == 18
    assert np.abs(G["3n_VnA"][1]).max() == 0.0 and np.abs(G["3n_VnA"][2]).max() > 0.0


@pytest.mark.parametrize("tag", TAGS)
def test_batch_schedule_formula(tag):
    """batch_idx[j] of iteration it = perm0[(j - it bs) mod NB]: the product's formula and the tests' equal what the
    reference's head-then-roll drew at every iteration; every batch is bs distinct cells."""
    from spateo_amd.align import _svi_schedule

    perm, bs = G[f"{tag}_batch_perm"], int(G["batch_size"])
    for it in range(int(G["iters"])):
        want = G[f"{tag}_batch_idx"][it]
        np.testing.assert_array_equal(_svi_schedule(perm, bs, it), want)
        np.testing.assert_array_equal(sc.schedule(perm, bs, it), want)
        start = (-it * bs) % len(perm)                         # what mvf_align_gather is handed
        np.testing.assert_array_equal(perm[(start + np.arange(bs)) % len(perm)], want)
        assert len(np.unique(want)) == bs


@pytest.mark.parametrize("NB, want", [(500, 500), (5_000, 1000), (20_000, 2000)])
def test_default_batch_size_rule(NB, want):
    from spateo_amd.align import _svi_arguments, _svi_batch_size

    assert _svi_batch_size(NB) == want == sc.default_batch_size(NB)
    assert _svi_batch_size(NB, 300) == 300 and _svi_batch_size(NB, 10 * NB) == NB
    bs, perm = _svi_arguments(NB, None, None, 3)
    assert bs == want and perm.dtype == np.int32 and np.array_equal(np.sort(perm), np.arange(NB))
    np.testing.assert_array_equal(perm, np.random.default_rng(3).permutation(NB))


def test_svi_rigid_update_from_the_block_matches_the_formulas():
    """The host half of an SVI iteration: `_rigid_from_block` / `_optimal_from_block` on a block built by the NumPy reference
    of mvf_align_moments, with a blended Sp that differs from the batch's, give the R, t of the direct formulas (means over
    the blended Sp, R blended before the translation reads it, t blended after)."""
    from spateo_amd.align import _optimal_from_block, _rigid_from_block

    rng = np.random.default_rng(6)
    for D, with_inliers, step in ((3, False, 1.0), (3, False, 0.4), (3, True, 0.4), (2, True, 10 / 13)):
        n, nb = 300, 120
        A, B = np.zeros((n, 3)), np.zeros((nb, 3))
        A[:, :D], B[:, :D] = rng.standard_normal((n, D)) + 2.0, rng.standard_normal((nb, D)) + 2.0
        P = rng.random((n, nb)) * (rng.random((n, nb)) < 0.1)
        V = np.zeros((n, 3))
        V[:, :D] = 0.1 * rng.standard_normal((n, D))
        K, KB = P.sum(1), P.sum(0)
        val, _ = lc.moments_reference(A, V, K, K, K, np.zeros(n), P @ B, B, KB, np.zeros(3))
        blk = np.zeros(64)
        blk[:50] = val
        Sp = 1.3 * P.sum()                                      # the running value, not this batch's
        inl = None
        if with_inliers:
            inl = (A[:20, :D] + 0.0, B[:20, :D] + 0.3, rng.uniform(0.5, 1, (20, 1)))
        R_prev, t_prev = lc._rotation(rng.standard_normal((D, D))), rng.standard_normal(D)
        R, t = _rigid_from_block(blk, D, 0.3, inl, 1.5, R_prev, True, Sp_blend=Sp, step=step, t_prev=t_prev)
        XA, XB, Vn = A[:, :D], B[:, :D], V[:, :D]
        S_A, S_V, S_B, deno, w = K @ XA, K @ Vn, KB @ XB, Sp, 0.0
        if inl:
            w = 0.3 * 1.5 * Sp / inl[2].sum()
            S_B, S_A, deno = S_B + w * (inl[2].T @ inl[1])[0], S_A + w * (inl[2].T @ inl[0])[0], Sp + w * inl[2].sum()
        mB, mA, mV = S_B / deno, S_A / deno, S_V / Sp
        Am = -(((XA - mA).T @ ((Vn - mV) * K[:, None])) - (XA - mA).T @ P @ (XB - mB)).T
        if inl:
            Am = Am - w * ((inl[0] - mA) * inl[2]).T.dot(-(inl[1] - mB)).T
        R_ref = lc._rotation(Am)
        if step < 1:
            R_ref = step * R_ref + (1 - step) * R_prev
        t_ref = (S_B - S_V - S_A @ R_ref.T + (w * (inl[2].T @ (inl[1] - inl[0] @ R_ref.T))[0] if inl else 0.0)) / deno
        if step < 1:
            t_ref = step * t_ref + (1 - step) * t_prev
        assert np.abs(R - R_ref).max() <= 1e-12 and np.abs(t - t_ref).max() <= 1e-12 * max(1.0, np.abs(t_ref).max())
        # _get_optimal_R on the last batch: means over the blended Sp
        oR, ot = _optimal_from_block(blk, D, Sp)
        mu_A, mu_B = (K @ XA) / Sp, (KB @ XB) / Sp
        oR_ref = lc._rotation((P @ (XB - mu_B)).T @ (XA - mu_A))
        assert np.abs(oR - oR_ref).max() <= 1e-12 and np.abs(ot - (mu_B - mu_A @ oR_ref.T)).max() <= 1e-12
        # and on the device's own means (dense loop, return_mapping) it is the block's matrix as it stands
        oR2, _ = _optimal_from_block(blk, D)
        mu_A, mu_B = (K @ XA) / P.sum(), (KB @ XB) / P.sum()
        assert np.abs(oR2 - lc._rotation((P @ (XB - mu_B)).T @ (XA - mu_A))).max() <= 1e-12


@pytest.mark.parametrize("tag", TAGS)
def test_loop_on_cpu_stand_in_kernels_reproduces_the_fixture(tag, monkeypatch):
    """`morpho_iterate_svi` itself - its schedule, the order of its stages, the host's blends and its rigid update from the
    block - with NumPy stand-ins in place of the kernels (tests/_align_svi_case.CpuLoopKernels), against the fixture, with
    `return_mapping=True`: per iteration and quantity within the GPU suite's float64 bound 1e-10 max(1, 1.25 g_k)."""
    from spateo_amd import align

    args, kw = sc.case_inputs(G, tag)
    sc.cpu_loop_kernels(monkeypatch, args[0].shape[1])
    out = align.morpho_iterate_svi(*args, record="arrays", return_mapping=True, **kw)
    got = dict(out["history"], optimal_R_map=out["optimal_R"], optimal_t_map=out["optimal_t"], Sp_map=out["Sp"])
    tol = sc.bounds(G, tag, sc.F64_TOL, finals=sc.FINALS_MAP)
    sc.check(sc.deviations(got, G, tag, sc.FINALS_MAP), tol, f"case {tag} loop on stand-ins")
    np.testing.assert_array_equal(out["history"]["step_size"], G[f"{tag}_step_size"])
    assert len(out["K_NB"]) == len(args[1]) and out["batch_size"] == int(G["batch_size"])
    plain = align.morpho_iterate_svi(*args, record=False, **dict(kw, max_iter=12))
    assert len(plain["K_NB"]) == int(G["batch_size"]) and plain["step_size"] == 10.0 / 12.0 and "history" not in plain


def test_dense_loop_on_cpu_stand_in_kernels_keeps_its_fixture(monkeypatch):
    """The shared loop body still computes the dense loop: `morpho_iterate` on the same stand-ins against ref_align_loop.npz
    (case 3: 2-D, inliers)."""
    from spateo_amd import align

    D = lc.load()
    args, kw = lc.case_inputs(D, "3")
    sc.cpu_loop_kernels(monkeypatch, 2)
    out = align.morpho_iterate(*args, record="arrays", **kw)
    got = dict(out["history"], optimal_R=out["optimal_R"], optimal_t=out["optimal_t"])
    lc.check(lc.deviations(got, D, "3"), lc.bounds(D, "3", lc.F64_TOL), "dense case 3 on stand-ins")
    assert set(out["history"]) == {"sigma2", "gamma", "R", "t", "Sp", "alpha", "XAHat", "VnA", "K_NA", "Coff"}


# ---- morpho_iterate_svi: validation and refusals (no device) -------------------------------------------------------------
def _call(**over):
    from spateo_amd import align

    args, kw = sc.case_inputs(G, "1")
    kw.update(over)
    pos = list(args)
    for i, name in enumerate(("coordsA", "coordsB", "exp_layers_A", "exp_layers_B")):
        if name in kw:
            pos[i] = kw.pop(name)
    return align.morpho_iterate_svi(*pos, **kw)


def test_morpho_iterate_svi_is_public():
    import inspect

    import spateo_amd as st

    assert "morpho_iterate_svi" in st.align.__all__ and callable(st.align.morpho_iterate_svi)
    doc = st.align.morpho_iterate_svi.__doc__
    for word in ("batch_size", "batch_perm", "return_mapping", "step_size", "morpho_class.py:136"):
        assert word in doc, word
    mine, dense = (inspect.signature(f).parameters for f in (st.align.morpho_iterate_svi, st.align.morpho_iterate))
    assert set(dense) - set(mine) == {"SVI_mode"}               # every argument of morpho_iterate but the refused mode
    assert set(mine) - set(dense) == {"batch_size", "batch_perm", "seed", "return_mapping"}
    # morpho_iterate still refuses the mode, and says where it lives
    with pytest.raises(NotImplementedError, match="SVI_mode") as e:
        args, kw = lc.case_inputs(lc.load(), "1")
        st.align.morpho_iterate(*args, SVI_mode=True, **kw)
    assert "morpho_iterate_svi" in str(e.value)


@pytest.mark.parametrize("over, match", [
    (dict(guidance=dict(X_AI=np.zeros((2, 3)))), "guidance"),
    (dict(sparse_calculation_mode=True), "sparse_calculation_mode"),
    (dict(dissimilarity=["label"]), "label"),
    (dict(kernel_type="geodist"), "geodist"),
    (dict(coordsA=np.zeros((607, 4)), coordsB=np.zeros((451, 4))), "2-D or 3-D"),
    (dict(exp_layers_A=[np.ones((607, 3))] * 5, exp_layers_B=[np.ones((451, 3))] * 5, dissimilarity=["kl"] * 5,
          probability_type=["gauss"] * 5, probability_parameters=[0.1] * 5), "at most 4 layers"),
])
def test_morpho_iterate_svi_refusals(over, match):
    with pytest.raises(NotImplementedError, match=match):
        _call(**over)


def _perm(kind):
    p = np.arange(451)
    if kind == "repeated":
        p[7] = p[8]
    elif kind == "out_of_range":
        p[0] = 451
    elif kind == "negative":
        p[3] = -1
    elif kind == "short":
        p = p[:-1]
    elif kind == "float":
        p = p.astype(np.float64)
    elif kind == "2d":
        p = p[None]
    return p


@pytest.mark.parametrize("over", [
    dict(batch_perm=_perm("repeated")),      # one index twice, so another is missing
    dict(batch_perm=_perm("out_of_range")),
    dict(batch_perm=_perm("negative")),
    dict(batch_perm=_perm("short")),
    dict(batch_perm=_perm("float")),
    dict(batch_perm=_perm("2d")),
    dict(batch_size=0),
    dict(batch_size=-5),
    dict(batch_size=12.5),
    dict(dtype="float16"),
    dict(max_iter=0),
    dict(sigma2=0.0),
    dict(kappa=-1.0),
    dict(coordsB=np.zeros((0, 3))),
])
def test_morpho_iterate_svi_validation_needs_no_device(over):
    with pytest.raises(ValueError):
        _call(**over)
