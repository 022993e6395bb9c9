"""CPU proofs around the alignment loop (``spateo_amd.align.morpho_iterate``): the NumPy restatement of
tests/_align_loop_case.py against the fixture tests/golden/ref_align_loop.npz (real reference code, 12 iterations, four
cases), the fixture's own conditions, the Python digamma, the targeted wrong answers, and the validation / refusals of
``morpho_iterate`` (no device needed).

Bound of the restatement: ``1e-12 max(1, 1.25 g_k)`` per case, iteration and quantity (1e-12: the project's figure for its
reference proofs; g_k: the amplification the maker measured with its perturbed twin).  Measured with this file
(``pytest -s``): the restatement reproduces every stored quantity of all four cases and all twelve iterations with deviation
0 - the same float64 operations in the same order, once its digamma is ``scipy.special.psi`` and ``diag(U Sigma U^T)`` is
summed row by row in index order.  That is not a coincidence to rely on but it is informative: with the project's own digamma
formula (2.3e-13 from scipy's on ``exp(psi(a) - psi(b))``, proven below) in its place the same restatement deviates by up to
1.4e-12 on ``t``, 1.4e-11 on ``VnA`` and 2e-10 on ``Coff`` (case 4) - cond(SigmaInv) = 3.6e5 turns the last place of one
digamma value into 1e-11 of ``Coff`` a few iterations later, which is also the size of the reference's own ``use_chunk`` twin."""
import numpy as np
import pytest

import _align_loop_case as lc

G = lc.load()
TAGS = lc.case_tags(G)
_RUNS = {}


def _run(tag):
    if tag not in _RUNS:
        args, kw = lc.case_inputs(G, tag)
        _RUNS[tag] = lc.restatement(*args, **kw)
    return _RUNS[tag]


@pytest.mark.parametrize("q", lc.SCALARS + lc.ARRAYS + lc.FINALS)
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_fixture(tag, q):
    dev = lc.deviations(_run(tag), G, tag)
    tol = lc.bounds(G, tag, lc.HOST_TOL)
    lc.check({q: dev[q]}, {q: tol[q]}, f"case {tag} restatement")


def test_fixture_conditions():
    iters = int(G["iters"])
    assert iters == 12 and TAGS == ["1", "2", "3", "4"]
    for tag in TAGS:
        for q in lc.SCALARS + lc.ARRAYS + lc.FINALS:
            assert np.isfinite(G[f"{tag}_{q}"]).all(), (tag, q)
            assert float(G[f"{tag}_g_{q}"].max()) <= 100.0, (tag, q)
        assert int(G[f"{tag}_nonrigid_runs"]) >= 8
        # the non-rigid update really ran: VnA is non-zero from the first stored iteration after nonrigid_start_iter
        stored = [int(i) for i in G["arr_iters"]]
        for i, it in enumerate(stored):
            assert (np.abs(G[f"{tag}_VnA"][i]).max() > 0) == (it > int(G[f"{tag}_nonrigid_start_iter"]))
        assert np.linalg.norm(G[f"{tag}_R"][-1] - G[f"{tag}_R0"]) <= 0.05
        assert len(G[f"{tag}_sigma2"]) == iters and G[f"{tag}_sigma2"][-1] < G[f"{tag}_sigma2"][0]
    gam = G["2_gamma"]
    assert np.sum((gam > 0.01) & (gam < 0.99)) >= iters // 2
    assert len(G["2_far"]) >= 0.05 * len(G["2_coordsB"])
    assert len(G["2_dissimilarity"]) == 2 and G["3_coordsA"].shape[1] == 2 and "3_inlier_P" in G.files
    assert float(G["3_partial_robust_level"]) != 1.0
    np.testing.assert_array_equal(G["4_origin"], np.full(3, 1e4))
    assert np.abs(G["4_coordsA"] - G["4_origin"] - G["1_coordsA"]).max() < 4e-12


def test_python_digamma_against_scipy():
    from scipy.special import psi

    from spateo_amd.align import _digamma

    a = np.concatenate([np.logspace(-3, 6, 400), [1e-3, 0.5, 1.0, 9.999999, 10.0, 10.000001, 1e6]])
    b = np.concatenate([np.logspace(0, 9, 300), [1.0, 10.0, 1e9]])
    pa, pb = np.array([_digamma(x) for x in a]), np.array([_digamma(x) for x in b])
    # got / ref - 1 with got = exp(pa - pb), ref = exp(psi(a) - psi(b)): formed from the exponents, so that the pairs whose
    # exponential underflows (psi(1e-3) = -1000.4) are measured too
    worst = float(np.abs(np.expm1((pa - psi(a))[:, None] - (pb - psi(b))[None, :])).max())
    print(f"  exp(psi(a) - psi(b)): largest relative deviation from scipy.special.psi {worst:.2e}")
    assert worst <= 1e-12
    # the vectorised twin the restatement uses is the same formula
    assert np.array_equal(lc.digamma(a), pa) or float(np.abs(lc.digamma(a) - pa).max()) <= 1e-13
    with pytest.raises(ValueError):
        _digamma(0.0)


def _moved(ref, got, tag, quantities):
    """largest deviation / float64 bound over the quantities (inf when the wrong answer is not even finite)."""
    if got is None:
        return np.inf
    tol = lc.bounds(G, tag, lc.F64_TOL)
    dev = lc.deviations(got, G, tag) if ref is None else {q: lc.rel(got[q], ref[q]) for q in quantities}
    return max(float(dev[q].max() / tol[q].max()) for q in quantities)


def test_targeted_wrong_answers_move_a_compared_quantity():
    """Each wrong answer moves a compared quantity by at least 1000 x the float64 bound of the GPU suite."""
    q = ("sigma2", "R", "t")
    # raw instead of centred moments, on the case that sits 1e4 from the origin
    args, kw = lc.case_inputs(G, "4")
    moved = _moved(None, lc.restatement(*args, wrong="raw_moments", **kw), "4", q + ("optimal_R", "optimal_t"))
    print(f"  raw moments on case 4: {moved:.3g} x the bound")
    assert moved >= 1000
    # kappa NA taken as the scalar sum of kappa: the same number for a constant kappa, so kappa varies over the cells
    args, kw = lc.case_inputs(G, "1")
    kw.update(max_iter=3, kappa=np.linspace(0.5, 2.0, len(args[0])))
    right, wrong = lc.restatement(*args, **kw), lc.restatement(*args, wrong="kappa_sum", **kw)
    moved = _moved(right, wrong, "1", ("alpha", "sigma2"))
    print(f"  kappa NA as a scalar sum: {moved:.3g} x the bound")
    assert moved >= 1000
    # sigma2's 1e-2 floor applied after iteration 100 instead of below it: a state whose sigma2 falls under the floor
    args, kw = lc.case_inputs(G, "1")
    tight = (args[0], args[0][: len(args[1])] @ np.eye(3), args[2], [a[: len(args[1])] for a in args[2]])
    kw.update(max_iter=6, sigma2=0.02)
    right, wrong = lc.restatement(*tight, **kw), lc.restatement(*tight, wrong="late_floor", **kw)
    assert min(right["sigma2"]) == 1e-2, right["sigma2"]
    moved = _moved(right, wrong, "1", ("sigma2",))
    print(f"  late sigma2 floor: {moved:.3g} x the bound")
    assert moved >= 1000
    # the K_NA == 0 rule dropped: three A cells so far away that their rows of P underflow to exactly 0
    args, kw = lc.case_inputs(G, "2")
    XA = args[0].copy()
    XA[[5, 77, 300], 0] += 1e3
    kw.update(max_iter=5)
    right = lc.restatement(XA, *args[1:], **kw)
    assert np.all(right["K_NA"][-1][[5, 77, 300]] == 0.0) and all(np.isfinite(right[k]).all() for k in right if k != "sigma2_variance")
    assert lc.restatement(XA, *args[1:], wrong="no_zero_rule", **kw) is None   # 0 / 0: not one finite entry of U^T Y is left


# ---- morpho_iterate: validation and refusals (no device) ----------------------------------------------------------------
def _call(**over):
    from spateo_amd import align

    args, kw = lc.case_inputs(G, "1")
    kw.update(over)
    pos = list(args)
    for i, name in enumerate(("coordsA", "coordsB", "exp_layers_A", "exp_layers_B")):
        if name in kw:
            pos[i] = kw.pop(name)
    return align.morpho_iterate(*pos, **kw)


def test_morpho_iterate_is_public():
    import spateo_amd as st

    assert "morpho_iterate" in st.align.__all__ and callable(st.align.morpho_iterate)
    doc = st.align.morpho_iterate.__doc__
    for word in ("SVI_mode", "guidance", "sparse_calculation_mode", '"label"', "geodist", "morpho_class.py:133-152"):
        assert word in doc, word


@pytest.mark.parametrize("over, match", [
    (dict(SVI_mode=True), "SVI_mode"),
    (dict(guidance=dict(X_AI=np.zeros((2, 3)))), "guidance"),
    (dict(sparse_calculation_mode=True), "sparse_calculation_mode"),
    (dict(dissimilarity=["label"]), "label"),
    (dict(kernel_type="geodist"), "geodist"),
    (dict(coordsA=np.zeros((607, 4)), coordsB=np.zeros((451, 4))), "2-D or 3-D"),
])
def test_morpho_iterate_refusals(over, match):
    with pytest.raises(NotImplementedError, match=match):
        _call(**over)


@pytest.mark.parametrize("over, exc", [
    (dict(dtype="float16"), ValueError),
    (dict(max_iter=0), ValueError),
    (dict(sigma2=0.0), ValueError),
    (dict(kappa="one"), ValueError),
    (dict(kappa=np.ones(5)), ValueError),
    (dict(kappa=-1.0), ValueError),
    (dict(record="everything"), ValueError),
    (dict(inducing_variables=np.zeros((40, 2))), AssertionError),
    (dict(inliers=(np.zeros((3, 3)), np.zeros((4, 3)), np.ones(3))), ValueError),
    (dict(inliers=(np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3))), ValueError),
    (dict(samples_s=0.0), ValueError),
    (dict(probability_type=["nothing"]), ValueError),
    (dict(coordsB=np.zeros((0, 3))), ValueError),
])
def test_morpho_iterate_validation_needs_no_device(over, exc):
    with pytest.raises(exc):
        _call(**over)


def test_rigid_update_from_the_block_matches_the_formulas():
    """The host half of an iteration: `_rigid_from_block` on a block built by the NumPy reference of mvf_align_moments gives
    the R, t of the direct formulas, with and without inliers, for means that differ from the device's."""
    from spateo_amd.align import _rigid_from_block

    rng = np.random.default_rng(5)
    for D, with_inliers in ((3, False), (3, True), (2, True)):
        n, nb = 300, 200
        A, B = np.zeros((n, 3)), np.zeros((nb, 3))
        A[:, :D], B[:, :D] = rng.standard_normal((n, D)) + 50.0, rng.standard_normal((nb, D)) + 50.0
        P = rng.random((n, nb)) * (rng.random((n, nb)) < 0.1)
        V = np.zeros((n, 3))
        V[:, :D] = 0.1 * rng.standard_normal((n, D))
        K, KB = P.sum(1), P.sum(0)
        val, _ = lc.moments_reference(A, V, K, K, K, np.zeros(n), P @ B, B, KB, np.zeros(3))
        blk = np.zeros(64)
        blk[:50] = val
        inl = None
        if with_inliers:
            iA, iB = A[:20, :D] + 0.0, B[:20, :D] + 0.3
            inl = (iA, iB, rng.uniform(0.5, 1, (20, 1)))
        R, t = _rigid_from_block(blk, D, 0.3, inl, 1.5, np.eye(D), True)
        # direct formulas
        XA, XB, Vn = A[:, :D], B[:, :D], V[:, :D]
        Sp = P.sum()
        S_A, S_V, S_B, deno, w = K @ XA, K @ Vn, KB @ XB, Sp, 0.0
        if inl:
            w = 0.3 * 1.5 * Sp / inl[2].sum()
            S_B, S_A, deno = S_B + w * (inl[2].T @ inl[1])[0], S_A + w * (inl[2].T @ inl[0])[0], Sp + w * inl[2].sum()
        mB, mA, mV = S_B / deno, S_A / deno, S_V / Sp
        Am = -(((XA - mA).T @ ((Vn - mV) * K[:, None])) - (XA - mA).T @ P @ (XB - mB)).T
        if inl:
            Am = Am - w * ((inl[0] - mA) * inl[2]).T.dot(-(inl[1] - mB)).T
        R_ref = lc._rotation(Am)
        t_num = S_B - S_V - S_A @ R_ref.T + (w * (inl[2].T @ (inl[1] - inl[0] @ R_ref.T))[0] if inl else 0.0)
        assert np.abs(R - R_ref).max() <= 1e-12 and np.abs(t - t_num / deno).max() <= 1e-12 * np.abs(t_num / deno).max()
