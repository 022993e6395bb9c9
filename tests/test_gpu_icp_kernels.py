"""Kernel-level tests of ``mvf_icp_batch`` (csrc/mvf_icp.hip) through the raw C ABI on ``cuda:0``, and of ``st.align.icp`` /
``icp_batch`` above it.  References and bounds come from tests/_icp_cases.py (proved against the real reference by
tests/test_icp_kernel_refs.py): ``gamma``, the rounds run and the inliers of the last query equal the restatement's; ``T_contour_2``
and the translation within 64 x the restatement's own 4-ulp deviation.  Every output sits in front of a guard, and two runs must
give identical bits."""
import ctypes

import numpy as np
import pytest
import torch

import _icp_cases as ic
from _kernel_scaffold import (DEV, MODES, called as _called, dev as _dev, guarded as _guarded, intact as _intact,
                              same_bits as _same_bits, stream as _stream, take as _take, under as _under)

pytestmark = pytest.mark.gpu

PAR = dict(max_iter=20, error_threshold=1e-6, inlier_threshold=0.1, gamma_threshold=0.05, subsample=500, allow_rotation=False)


@pytest.fixture(scope="module")
def lib():
    from spateo_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


@pytest.fixture(scope="module")
def G():
    return ic.load()


def run_batch(lib, pairs, want_T=True, **kw):
    """mvf_icp_batch on the pairs [(c1, c2), ...]: list of dict(gamma, iters, inliers, translation, T) from guarded outputs."""
    from spateo_amd import _lib

    par = dict(PAR, **kw)
    P = len(pairs)
    sub = par["subsample"]
    m2 = [min(len(b), sub) if sub > 0 else len(b) for _, b in pairs]
    keep, outs = [], []
    recs = (_lib.IcpProblem * P)()
    for rec, (a, b), m in zip(recs, pairs, m2):
        da, db = _dev(a), _dev(b)
        o = dict(gamma=_guarded(1, torch.float64), stats=_guarded(2, torch.int32), shift=_guarded(2, torch.float64),
                 T=_guarded(2 * m, torch.float64) if want_T else None)
        rec.contour_1, rec.n1, rec.contour_2, rec.n2 = da.data_ptr(), len(a), db.data_ptr(), len(b)
        rec.gamma, rec.stats, rec.translation = o["gamma"].data_ptr(), o["stats"].data_ptr(), o["shift"].data_ptr()
        rec.T_contour_2 = o["T"].data_ptr() if want_T else None
        keep.append((da, db))
        outs.append(o)
    need = int(lib.mvf_icp_batch_workspace_bytes(P))
    assert need == min(P, 4096) * ctypes.sizeof(_lib.IcpProblem)
    ws = _guarded(need // 8, fill=0.0)
    rc = lib.mvf_icp_batch(recs, P, par["max_iter"], par["error_threshold"], par["inlier_threshold"], par["gamma_threshold"],
                           par["subsample"], int(par["allow_rotation"]), ws.data_ptr(), need, _stream())
    assert rc == 0, lib.mvf_last_error()
    _called()
    torch.cuda.synchronize()
    assert _intact(ws, need // 8), "wrote past the end of the workspace"
    res = []
    for o, m in zip(outs, m2):
        st = _take(o["stats"], 2)
        res.append(dict(gamma=float(_take(o["gamma"], 1)[0]), iters=int(st[0]), inliers=int(st[1]), translation=_take(o["shift"], 2),
                        T=_take(o["T"], 2 * m).reshape(m, 2) if want_T else None))
    return res


def check(got, c1, c2, **kw):
    """One device result against the restatement; returns the restatement's result."""
    par = dict(PAR, **kw)
    bound, want = ic.icp_bound(c1, c2, **par)
    err = float(np.abs(got["T"] - want["T"]).max()) if np.isfinite(want["T"]).all() else 0.0
    print(f"({len(c1)}, {len(c2)}) {kw}: gamma {got['gamma']} rounds {got['iters']} inliers {got['inliers']} "
          f"|T - T_restated| = {err:.3e} (bound {bound:.3e})")
    assert got["gamma"] == want["gamma"] and got["iters"] == want["iters"] and got["inliers"] == want["inliers"]
    assert got["T"].shape == want["T"].shape and err <= bound
    assert np.abs(got["translation"] - want["translation"]).max() <= bound
    return want


CONVENTION_COVERS = {"mvf_icp_batch": MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rot", (False, True))
def test_calling_conventions(lib, rot, mode):
    """The plain call's bits on a side stream behind poisoned inputs, at displaced pointers, and with the inputs unchanged."""
    pairs = [ic.icp_pair(n1, n2, 100 + n1 + 3 * n2) for n1, n2 in ((7, 2), (63, 64), (65, 63))]
    plain, got = _under(mode, lambda: run_batch(lib, pairs, allow_rotation=rot))
    for p, g in zip(plain, got):
        assert (p["gamma"], p["iters"], p["inliers"]) == (g["gamma"], g["iters"], g["inliers"])
        assert _same_bits(p["T"], g["T"]) and _same_bits(p["translation"], g["translation"])


# sizes: the fewer-than-3-inliers exit (M < 3), around a wave, around the cap of a lane's first point, N != M both ways
SMALL = [(7, 1), (7, 2), (7, 3), (1, 7), (2, 7), (3, 7), (63, 64), (64, 65), (65, 63), (257, 255), (120, 300)]


@pytest.mark.parametrize("rot", (False, True))
def test_small_sizes_in_one_batch(lib, rot):
    pairs = [ic.icp_pair(n1, n2, 100 + n1 + 3 * n2) for n1, n2 in SMALL]
    res = run_batch(lib, pairs, allow_rotation=rot)
    wants = [check(r, a, b, allow_rotation=rot) for r, (a, b) in zip(res, pairs)]
    assert all(w["inliers"] < 3 and w["iters"] == 1 for w, (_, n2) in zip(wants, SMALL) if n2 < 3)
    assert any(w["inliers"] >= 3 for w in wants)
    again = run_batch(lib, pairs, allow_rotation=rot)
    for r, s in zip(res, again):   # two calls, identical bits
        assert r["gamma"] == s["gamma"] and np.array_equal(r["T"], s["T"]) and np.array_equal(r["translation"], s["translation"])


@pytest.mark.parametrize("n1,n2", [(500, 501), (501, 500), (1203, 500), (500, 1203)])
def test_thinning(lib, n1, n2):
    c1, c2 = ic.icp_pair(n1, n2, 7 * n1 + n2, angle=2.0, shift=(0.6, -0.4))
    (got,) = run_batch(lib, [(c1, c2)], allow_rotation=True)
    check(got, c1, c2, allow_rotation=True)
    assert got["T"].shape == (500, 2)
    # the same contours thinned by the caller, with no thinning asked of the kernel: the same bits
    (own,) = run_batch(lib, [(c1[ic.thin_rows(n1, 500)], c2[ic.thin_rows(n2, 500)])], allow_rotation=True, subsample=0)
    assert own["gamma"] == got["gamma"] and np.array_equal(own["T"], got["T"])


def test_smaller_subsample_and_the_cap(lib):
    c1, c2 = ic.icp_pair(300, 200, 17)
    (got,) = run_batch(lib, [(c1, c2)], subsample=64, allow_rotation=True)
    check(got, c1, c2, subsample=64, allow_rotation=True)
    c1, c2 = ic.icp_pair(512, 512, 19, angle=1.0, shift=(0.2, 0.2))   # MVF_ICP_MAX_POINTS on both sides, nothing thinned
    (got,) = run_batch(lib, [(c1, c2)], subsample=512)
    check(got, c1, c2, subsample=512)


def test_rounds(lib, G):
    """max_iter = 1; a case the error test stops; one that runs all rounds."""
    c1, c2 = G["icp_a_c1"], G["icp_a_c2"]
    (one,) = run_batch(lib, [(c1, c2)], max_iter=1)
    assert check(one, c1, c2, max_iter=1)["iters"] == 1
    (early,) = run_batch(lib, [(c1, c2)])
    assert 1 < check(early, c1, c2)["iters"] < 20
    g1, g2 = G["icp_g_c1"], G["icp_g_c2"]
    (full,) = run_batch(lib, [(g1, g2)], allow_rotation=True)
    assert check(full, g1, g2, allow_rotation=True)["iters"] == 20
    (never,) = run_batch(lib, [(c1, c2)], error_threshold=0.0, max_iter=5)   # |prev - err| < 0 never holds
    assert check(never, c1, c2, error_threshold=0.0, max_iter=5)["iters"] == 5


def test_a_covariance_with_negative_determinant_gives_the_reflection(lib, G):
    c1, c2 = G["icp_h_c1"], G["icp_h_c2"]
    (got,) = run_batch(lib, [(c1, c2)], allow_rotation=True)
    want = check(got, c1, c2, allow_rotation=True)
    assert want["dets"][0] < 0 and got["gamma"] == float(G["icp_h_1_gamma"]) == 1.0
    # the real reference's reflected result: it lies within the rule of the restatement too, so twice the bound covers both
    assert np.abs(got["T"] - G["icp_h_1_T"]).max() <= 2 * ic.icp_bound(c1, c2, **dict(PAR, allow_rotation=True))[0]
    (plain,) = run_batch(lib, [(c1, c2)])
    assert check(plain, c1, c2)["gamma"] == float(G["icp_h_0_gamma"]) == 0.0


@pytest.mark.parametrize("tag", list("abcdefgh"))
def test_goldens_of_the_real_reference(lib, G, tag):
    c1, c2 = G[f"icp_{tag}_c1"], G[f"icp_{tag}_c2"]
    for rot in (0, 1):
        (got,) = run_batch(lib, [(c1, c2)], allow_rotation=bool(rot))
        check(got, c1, c2, allow_rotation=bool(rot))
        assert got["gamma"] == float(G[f"icp_{tag}_{rot}_gamma"])
        # (the golden lies within the rule of the restatement as well - tests/test_icp_kernel_refs.py -: twice the bound)
        assert np.abs(got["T"] - G[f"icp_{tag}_{rot}_T"]).max() <= 2 * ic.icp_bound(c1, c2, **dict(PAR, allow_rotation=bool(rot)))[0]


def test_more_problems_than_one_launch_holds(lib):
    """4096 problems share a launch: 4101 tiny ones cross it; without T_contour_2 the pointer may be NULL."""
    kinds = [ic.icp_pair(5 + k, 4 + (3 * k) % 7, 900 + k) for k in range(8)]
    pairs = [kinds[i % 8] for i in range(4101)]
    res = run_batch(lib, pairs, want_T=False, allow_rotation=True)
    wants = [ic.icp(a, b, **dict(PAR, allow_rotation=True)) for a, b in kinds]
    for i, r in enumerate(res):
        w = wants[i % 8]
        assert (r["gamma"], r["iters"], r["inliers"]) == (w["gamma"], w["iters"], w["inliers"]), i
    for i in (0, 4095, 4096, 4100):   # ... and all of them computed the same thing as the first of their kind
        assert np.array_equal(res[i]["translation"], res[i % 8]["translation"])


def test_refusals_on_real_buffers(lib):
    from spateo_amd import _lib

    a = _dev(ic.closed_curve(20, 1))
    out = _guarded(8, torch.float64)
    st = _guarded(2, torch.int32)
    ws = torch.zeros(64, dtype=torch.float64, device=DEV)

    def call(n1=20, n2=20, max_iter=20, subsample=500, ws_bytes=512, gamma=out.data_ptr(), nprob=1):
        rec = _lib.IcpProblem(contour_1=a.data_ptr(), n1=n1, contour_2=a.data_ptr(), n2=n2, gamma=gamma, stats=st.data_ptr(),
                              T_contour_2=None, translation=None)
        recs = (_lib.IcpProblem * 1)(rec)
        return lib.mvf_icp_batch(recs, nprob, max_iter, 1e-6, 0.1, 0.05, subsample, 0, ws.data_ptr(), ws_bytes, _stream())

    for kw in (dict(n1=0), dict(n2=0), dict(max_iter=0), dict(subsample=513), dict(subsample=0, n1=513), dict(ws_bytes=8),
               dict(gamma=None), dict(nprob=-1)):
        assert call(**kw) != 0 and b"mvf_icp_batch" in lib.mvf_last_error(), kw
    assert call(nprob=0) == 0
    torch.cuda.synchronize()
    assert _intact(out, 0) and _intact(st, 0)   # nothing was launched


# ---- the API ----
def _closing_bound(c1, c2, **par):
    """64 x the 4-ulp deviation of the closing solve's (R, t) on the restated T, in coordinate units."""
    from spateo_amd import _mesh_correction as mc

    mag = float(max(np.abs(c1).max(), np.abs(c2).max()))
    flat = lambda a, b: np.concatenate([x.reshape(-1) for x in mc._closing_solve(ic.icp(a, b, **par)["T"], b[ic.thin_rows(len(b), par["subsample"])])[:2]])  # noqa: E731
    return ic.ALLOW * max(ic.deviation(flat, (c1, c2), mag), 2.0 ** -52) * mag


def check_api(res, c1, c2, **kw):
    """One tuple of st.align.icp / icp_batch against the restatement, by the rule of check(): gamma equal, T_contour_2 and the
    translation within 64 x the restatement's own 4-ulp deviation; with rotation (R, t) of the closing solve on the restated T."""
    from spateo_amd import _mesh_correction as mc

    par = dict(PAR, **kw)
    gamma, zero, t, k1, T, R = res
    bound, want = ic.icp_bound(c1, c2, **par)
    k2 = c2[ic.thin_rows(len(c2), par["subsample"])]
    assert gamma == want["gamma"] and zero == 0 and np.array_equal(k1, c1[ic.thin_rows(len(c1), par["subsample"])])
    assert T.shape == want["T"].shape and np.abs(T - want["T"]).max() <= bound
    if par["allow_rotation"]:
        R_want, t_want = mc._closing_solve(want["T"], k2)[:2]
        rb = _closing_bound(c1, c2, **par)
        assert np.linalg.det(R) > 0 and np.abs(R - R_want).max() <= rb and np.abs(t - t_want).max() <= rb
    else:
        assert np.array_equal(R, np.eye(2)) and np.abs(t - want["translation"]).max() <= bound
    return want, bound


@pytest.mark.parametrize("tag", ("a", "h"))
def test_icp_returns_the_reference_tuple(G, tag):
    """Against the restatement by the 64 x rule, and against the real reference's own return values (case h: a round reflects,
    the closing solve returns the proper rotation all the same)."""
    import spateo_amd as st

    c1, c2 = G[f"icp_{tag}_c1"], G[f"icp_{tag}_c2"]
    for rot in (False, True):
        res = st.align.icp(c1, c2, allow_rotation=rot)
        _, bound = check_api(res, c1, c2, allow_rotation=rot)
        gamma, _, t, _, T, R = res
        r = int(rot)
        # the goldens lie within the same rule of the restatement (tests/test_icp_kernel_refs.py): twice the bound covers both
        rb = _closing_bound(c1, c2, **dict(PAR, allow_rotation=True)) if rot else bound
        assert gamma == float(G[f"icp_{tag}_{r}_gamma"]) and np.abs(T - G[f"icp_{tag}_{r}_T"]).max() <= 2 * bound
        assert np.abs(R - G[f"icp_{tag}_{r}_R"]).max() <= 2 * rb and np.abs(t - G[f"icp_{tag}_{r}_t"]).max() <= 2 * rb


def test_icp_batch_thins_and_refuses(G):
    import spateo_amd as st
    from spateo_amd import _lib

    c1, c2 = ic.icp_pair(1203, 640, 23)
    pairs = [(c1, c2), (G["icp_c_c1"], G["icp_c_c2"]), (G["icp_f_c1"], G["icp_f_c2"])]   # three sizes: every offset differs
    for rot in (True, False):
        res = st.align.icp_batch([p[0] for p in pairs], [p[1] for p in pairs], allow_rotation=rot)
        for r, (a, b) in zip(res, pairs):
            check_api(r, a, b, allow_rotation=rot)
    assert st.align.icp_batch([], []) == []
    with pytest.raises(NotImplementedError, match="D != 2"):
        st.align.icp(np.zeros((5, 3)), np.zeros((5, 3)))
    with pytest.raises(NotImplementedError, match="ICP_MAX_POINTS"):
        st.align.icp(c1, c2, subsample=_lib.ICP_MAX_POINTS + 1)
    with pytest.raises(NotImplementedError, match="ICP_MAX_POINTS"):
        st.align.icp(c1, c2, subsample=0)
    with pytest.raises(ValueError, match="finite"):
        st.align.icp(np.full((5, 2), np.nan), c2)
