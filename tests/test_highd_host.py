"""CPU tests of the 4- to 8-dimensional path: the oracle reproduces the reference executed at D = 4, 5, 8
(``tests/golden/ref_highd.npz``, written by ``make_golden_highd.py``), and the two new C-ABI entry points are exported and
reject bad arguments through the status + mvf_last_error channel without launching anything."""
import ctypes
import os

import numpy as np
import pytest

from oracle import dg_oracle as dgo
from oracle import sparsevfc_oracle as svo

HERE = os.path.dirname(os.path.abspath(__file__))
RT = dict(rtol=1e-12, atol=1e-13)
DIMS = (4, 5, 8)


@pytest.fixture(scope="module")
def hd():
    with np.load(os.path.join(HERE, "golden", "ref_highd.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("d", DIMS)
def test_oracle_con_k_matches_the_reference_in_d_dimensions(hd, d):
    x, y, beta = hd[f"d{d}_conk_x"], hd[f"d{d}_conk_y"], float(hd["beta_conk"])
    np.testing.assert_allclose(svo.con_K(x, y, beta), hd[f"d{d}_conk_K"], **RT)
    K, D = svo.con_K(x, y, beta, return_d=True)
    np.testing.assert_allclose(K, hd[f"d{d}_conk_K_diff"], **RT)
    np.testing.assert_array_equal(D, hd[f"d{d}_conk_D"])


@pytest.mark.parametrize("d", DIMS)
def test_oracle_evaluators_match_the_reference_in_d_dimensions(hd, d):
    vfd = {"X_ctrl": hd[f"d{d}_Xc"], "C": hd[f"d{d}_C"], "beta": float(hd["beta_dg"])}
    Xq = hd[f"d{d}_Xq"]
    vf = lambda x: svo.vector_field_function(x, vfd)  # noqa: E731
    fj = lambda x: dgo.Jacobian_rkhs_gaussian(x, vfd)  # noqa: E731
    np.testing.assert_allclose(vf(Xq), hd[f"d{d}_v"], **RT)
    np.testing.assert_allclose(fj(Xq), hd[f"d{d}_J_loop"], **RT)
    np.testing.assert_allclose(dgo.Jacobian_rkhs_gaussian(Xq, vfd, vectorize=True), hd[f"d{d}_J_vec"], **RT)
    J1 = fj(Xq[3])
    assert J1.shape == (d, d)
    np.testing.assert_allclose(J1, hd[f"d{d}_J_1d"], **RT)
    acc, acc_mat = dgo.compute_acceleration(vf, fj, Xq)
    np.testing.assert_allclose(acc, hd[f"d{d}_acc"], **RT)
    np.testing.assert_allclose(acc_mat, hd[f"d{d}_acc_mat"], **RT)
    c2, c2m = dgo.compute_curvature(vf, fj, Xq, formula=2)
    np.testing.assert_allclose(c2, hd[f"d{d}_curv2"], **RT)
    np.testing.assert_allclose(c2m, hd[f"d{d}_curv2_mat"], **RT)
    c1, _ = dgo.compute_curvature(vf, fj, Xq, formula=1)
    np.testing.assert_allclose(c1, hd[f"d{d}_curv1"], **RT)
    np.testing.assert_allclose(dgo.compute_divergence(fj, Xq, vectorize_size=4), hd[f"d{d}_div"], **RT)
    # the reference's exceptions beyond 3 dimensions
    assert str(hd[f"d{d}_curl_exc"]) == "ValueError" and str(hd[f"d{d}_torsion_exc"]) == "Exception"
    with pytest.raises(ValueError):
        dgo.compute_curl(fj, Xq)
    with pytest.raises(Exception, match="torsion is only defined in 3 dimension"):
        dgo.compute_torsion(vf, fj, Xq)


def test_oracle_fit_matches_the_reference_wrapper_in_5_dimensions(hd):
    # the wrapper golden's field was fitted by the oracle under the reference's morphofield_sparsevfc (one restart, seed 0)
    X, V, NX = hd["a5_X"], hd["a5_V"], hd["a5_NX"]
    res = svo.SparseVFC(X, V, NX, M=20, MaxIter=20, seed=0, lambda_=0.02, lstsq_method="scipy")
    np.testing.assert_array_equal(res["X_ctrl"], hd["a5_vf_X_ctrl"])
    for k in ("V", "grid_V"):
        np.testing.assert_allclose(res[k], hd[f"a5_vf_{k}"], rtol=1e-9, atol=1e-12)
    assert abs(res["sigma2"] - float(hd["a5_vf_sigma2"])) <= 1e-9 * float(hd["a5_vf_sigma2"])
    vfd = {"X_ctrl": hd["a5_vf_X_ctrl"], "C": hd["a5_vf_C"], "beta": float(hd["a5_vf_beta"])}
    J = dgo.Jacobian_rkhs_gaussian(X, vfd)
    np.testing.assert_allclose(J, hd["a5_jacobian_uns"], **RT)
    np.testing.assert_allclose(np.trace(J), hd["a5_divergence_obs"], **RT)


def _lib():
    from spateo_amd import _lib

    return _lib, _lib.load()


def test_highd_entry_points_are_exported():
    _l, lib = _lib()
    for name in ("mvf_ublk_build_d", "mvf_eval_d"):
        assert hasattr(lib, name) and name in _l.SIGNATURES
    assert lib.mvf_version() == 7


def test_highd_entry_points_reject_bad_arguments_without_launching():
    _l, lib = _lib()
    dummy = ctypes.c_void_p(1)  # never dereferenced: every call below fails its argument checks first
    buf = 1 << 30
    for d in (3, 9, 0):
        assert lib.mvf_ublk_build_d(dummy, 100, dummy, 10, d, 0.1, dummy, buf, _l.MVF_F32, None) != 0
        assert b"d must be in 4 .. 8" in lib.mvf_last_error()
    assert lib.mvf_ublk_build_d(None, 100, dummy, 10, 5, 0.1, dummy, buf, _l.MVF_F32, None) != 0
    assert b"null pointer" in lib.mvf_last_error()
    assert lib.mvf_ublk_build_d(dummy, 100, dummy, 10, 5, 0.1, dummy, 16, _l.MVF_F64, None) != 0
    assert b"buffer too small" in lib.mvf_last_error()
    assert lib.mvf_ublk_build_d(dummy, 100, dummy, 10, 5, 0.1, dummy, buf, 7, None) != 0
    assert b"bad dtype" in lib.mvf_last_error()
    V = _l.EVAL_V
    args = lambda d, dy, flags, v=dummy, jac=None, x=dummy: (x, 50, dummy, 10, d, 0.1, dummy, dy, flags, v, jac, None,  # noqa: E731
                                                           None, None, _l.MVF_F32, None)
    for d in (3, 9):
        assert lib.mvf_eval_d(*args(d, 4, V)) != 0 and b"d must be in 4 .. 8" in lib.mvf_last_error()
    for dy in (0, 9):
        assert lib.mvf_eval_d(*args(5, dy, V)) != 0 and b"dy must be in 1 .. 8" in lib.mvf_last_error()
    assert lib.mvf_eval_d(*args(5, 5, _l.EVAL_CURL)) != 0 and b"only V, JAC" in lib.mvf_last_error()
    assert lib.mvf_eval_d(*args(5, 4, _l.EVAL_DIV)) != 0 and b"dy == d" in lib.mvf_last_error()
    assert lib.mvf_eval_d(*args(5, 5, V, v=None)) != 0 and b"v requested but null" in lib.mvf_last_error()
    assert lib.mvf_eval_d(*args(5, 5, _l.EVAL_JAC)) != 0 and b"jac requested but null" in lib.mvf_last_error()
    assert lib.mvf_eval_d(*args(5, 5, V, x=None)) != 0 and b"null input" in lib.mvf_last_error()
    # an empty query set launches nothing
    assert lib.mvf_eval_d(None, 0, None, 10, 5, 0.1, None, 5, V, dummy, None, None, None, None, _l.MVF_F32, None) == 0


def test_the_engine_and_the_evaluators_name_the_supported_range():
    import spateo_amd as st

    X = np.zeros((10, 9))
    with pytest.raises(NotImplementedError, match="1-8 spatial dimensions"):
        st.SparseVFC(X, X, None, M=5)
    vfd = {"X_ctrl": np.zeros((4, 9)), "C": np.zeros((4, 9)), "beta": 0.1}
    with pytest.raises(NotImplementedError, match="1 to 8 dimensions"):
        st.vector_field_function(np.zeros((3, 9)), vfd)
