"""GPU tests of SparseVFC fields in 4 to 8 dimensions: the kernel-value cache of mvf_ublk_build_d against mvf_con_k (bit for
bit), whole fits against the float64 oracle (tests/_floors.py criterion), the evaluators of mvf_eval_d against the reference
executed at D = 4, 5, 8 (tests/golden/ref_highd.npz), the Spateo wrappers on a 5-D AnnData, and what stays refused."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sparsevfc_oracle as svo  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = {"float64": 1e-5, "float32": 1e-3}
EVAL_TOL = {"float64": 1e-10, "float32": 1e-4}  # the 3-D twin test's (test_gpu_kernels.py::test_evaluators_golden)


@pytest.fixture(scope="module")
def st():
    import spateo_amd

    assert torch.cuda.is_available()
    return spateo_amd


@pytest.fixture(scope="module")
def hd():
    with np.load(os.path.join(HERE, "golden", "ref_highd.npz")) as z:
        return {k: z[k] for k in z.files}


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def lifted_c2(n, d, dy=None, seed=0, n_grid=1500):
    """The C2 generator lifted to d dimensions: points in an ellipsoid with axes 300 .. 120, a field that rotates in the
    (0, 1) and (2, 3) coordinate planes, grows radially and carries a sinusoidal shear; unit rms, noise 0.05, 5 % gross
    outliers.  dy columns (default d): the first min(dy, d) are the field, further ones smooth functions of the points.
    Returns (X, Y, Grid) with Grid drawn inside the data's bounding box."""
    rng = np.random.default_rng(seed)
    axes = np.linspace(300.0, 120.0, d)
    g = rng.standard_normal((n, d))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    X = g * (rng.random(n) ** (1.0 / d))[:, None] * axes
    L = float(np.abs(X).max())
    A = 0.02 * np.eye(d)
    A[0, 1], A[1, 0] = -0.01, 0.01
    A[2, 3], A[3, 2] = -0.015, 0.015
    V = X @ A.T + 2.0 * np.sin(2 * np.pi * np.roll(X, 1, axis=1) / L)
    dy = d if dy is None else dy
    extra = [np.cos(2 * np.pi * X[:, j % d] / L + j) * X[:, (j + 1) % d] / L for j in range(max(0, dy - d))]
    Y = np.column_stack([V[:, : min(dy, d)]] + extra) if extra else V[:, :dy].copy()
    Y /= np.sqrt(np.mean(Y**2))
    Y += 0.05 * rng.standard_normal(Y.shape)
    out = rng.choice(n, size=n // 20, replace=False)
    Y[out] = 2.0 * rng.standard_normal((len(out), dy))
    lo, hi = X.min(0), X.max(0)
    Grid = lo + (hi - lo) * rng.random((n_grid, d))
    return X, Y, Grid


# ------------------------------------------------------------------------------------------------ 1. cache == con_K
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("d", [4, 5, 8])
def test_ublk_build_d_is_con_k_bit_for_bit(st, d, dtype):
    from spateo_amd._kernels import HipKernels

    k = HipKernels("cuda:0", dtype)
    rng = np.random.default_rng(d)
    n, m, beta = 1000, 300, 0.013  # off the 256 / 128 padding
    X = rng.standard_normal((n, d)) * 6.0
    ctrl = X[rng.choice(n, m, replace=False)]
    c = ctrl.mean(0)
    xd, cd = k.to_xd(X, c), k.to_xd(ctrl, c)
    k.build_ublk_d(xd, cd, beta)
    n_pad, m_pad = k.wide_pads(n, m)
    assert k._ublk.numel() == n_pad * m_pad == k.ublk_bytes(n, m) // (4 if dtype == "float32" else 8)
    U = k._ublk.view(m_pad // 16, n_pad, 16).permute(1, 0, 2).reshape(n_pad, m_pad)
    K = k.con_k(xd, cd, beta)
    torch.cuda.synchronize()
    assert torch.equal(U[:n, :m], K)  # the same bits: C is fitted to the U the Gram kernel saw
    assert not U[n:].any() and not U[:, m:].any()  # the padding is zero
    k.drop_ublk()


# ------------------------------------------------------------------------------------------------ 2. whole fits
_FLOORS = {}


def _fit_case(X, Y, Grid, kw):
    """(oracle result, floor table, near mask) of one case, computed once for both dtypes."""
    import _floors as F

    key = (X.shape, Y.shape, float(X[0, 0]), tuple(sorted(kw.items())))
    if key not in _FLOORS:
        ref = svo.SparseVFC(X, Y, Grid, **kw)
        near = F.near_mask(X, Grid)
        _FLOORS[key] = (ref, F.floor_table(X, Y, Grid, ref, kw, near=near), near)
    return _FLOORS[key]


def _check_fit(st, X, Y, Grid, kw, dtype):
    import _floors as F

    ref, table, near = _fit_case(X, Y, Grid, kw)
    got = st.SparseVFC(X, Y, Grid, dtype=dtype, device="cuda:0", **kw)
    assert got["V"].shape == Y.shape and got["grid_V"].shape == (len(Grid), Y.shape[1])
    assert got["iteration"] == ref["iteration"]
    dev = F.deviations(got, ref, near=near)
    t = TOL[dtype]
    base = {"V": t, "grid12": t, "sigma2": t, "E": t, "P999": 10 * t}
    col = 0 if dtype == "float64" else 1
    print(f"{dtype}: " + "; ".join(f"{k} gpu {dev[k]:.2e} / floor {table[k][col]:.2e}" for k in base))
    print(F.fmt(table))
    for q in base:
        assert dev[q] <= F.tol(dtype, table, q, base[q]), (q, dev[q], table[q])
    assert dev["P"] <= F.cap(dtype, table, "P", 10 * t), ("P", dev["P"], table["P"])
    return got


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("M", [100, 500])
@pytest.mark.parametrize("d", [4, 5, 8])
def test_fit_in_d_dimensions_against_the_oracle(st, d, M, dtype):
    X, Y, Grid = lifted_c2(20_000, d, seed=d)
    kw = dict(M=M, lambda_=0.02, MaxIter=10, ecr=0.0, seed=0, lstsq_method="scipy")
    _check_fit(st, X, Y, Grid, kw, dtype)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_fit_in_5_dimensions_through_the_deflated_solve(st, dtype):
    X, Y, Grid = lifted_c2(20_000, 5, seed=55)
    kw = dict(M=800, lambda_=0.02, MaxIter=8, ecr=0.0, seed=0, lstsq_method="scipy")
    _check_fit(st, X, Y, Grid, kw, dtype)


@pytest.mark.parametrize("dtype,dy", [("float64", 1), ("float64", 2), ("float64", 3), ("float64", 12), ("float32", 1),
                                      ("float32", 12)])
def test_fit_in_4_dimensions_any_number_of_output_columns(st, dtype, dy):
    """Dy <= 3 runs the wide (cached) rhs / apply kernels too (mvf_wide.hip: ldy = 16 >= dy); Dy = 12: grid_V in two
    evaluator launches of at most 8 columns."""
    X, Y, Grid = lifted_c2(20_000, 4, dy=dy, seed=40 + dy)
    kw = dict(M=100, lambda_=0.02, MaxIter=10, ecr=0.0, seed=0, lstsq_method="scipy")
    _check_fit(st, X, Y, Grid, kw, dtype)


# ------------------------------------------------------------------------------------------------ 3. evaluators
def _svc(st, hd, d, dtype):
    vfd = {"X_ctrl": hd[f"d{d}_Xc"], "C": hd[f"d{d}_C"], "beta": float(hd["beta_dg"])}
    vf = st.SvcVectorField(dtype=dtype, device="cuda:0")
    vf.vf_dict = vfd
    vf.func = lambda x: st.vector_field_function(x, vfd, dtype=dtype, device="cuda:0")
    return vf, vfd


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("d", [4, 5, 8])
def test_evaluators_against_the_reference_in_d_dimensions(st, hd, d, dtype):
    tol = EVAL_TOL[dtype]
    vf, vfd = _svc(st, hd, d, dtype)
    Xq = hd[f"d{d}_Xq"]
    assert _rel(vf.compute_velocity(Xq), hd[f"d{d}_v"]) < tol
    J = vf.get_Jacobian()(Xq)
    assert J.shape == (d, d, len(Xq)) and _rel(J, hd[f"d{d}_J_loop"]) < tol
    J1 = vf.get_Jacobian()(Xq[3])
    assert J1.shape == (d, d) and _rel(J1, hd[f"d{d}_J_1d"]) < tol
    Jw, det = vf.jacobian_with_det(Xq)
    assert _rel(Jw, hd[f"d{d}_J_vec"]) < tol
    ref_det = np.array([np.linalg.det(hd[f"d{d}_J_loop"][:, :, i]) for i in range(len(Xq))])
    assert _rel(det, ref_det) < 100 * tol
    acc, acc_mat = vf.compute_acceleration(Xq)
    assert _rel(acc, hd[f"d{d}_acc"]) < tol and _rel(acc_mat, hd[f"d{d}_acc_mat"]) < tol
    c2, c2m = vf.compute_curvature(Xq, formula=2)
    assert _rel(c2, hd[f"d{d}_curv2"]) < tol and _rel(c2m, hd[f"d{d}_curv2_mat"]) < tol
    c1, c1m = vf.compute_curvature(Xq, formula=1)
    assert c1m is None and _rel(c1, hd[f"d{d}_curv1"]) < tol
    assert _rel(vf.compute_divergence(Xq, vectorize_size=4), hd[f"d{d}_div"]) < tol
    v1 = st.vector_field_function(Xq[2], vfd, dtype=dtype, device="cuda:0")
    assert v1.shape == (d,) and _rel(v1, hd[f"d{d}_v"][2]) < tol


@pytest.mark.parametrize("d", [4, 5, 8])
def test_jacobian_against_central_differences_of_the_field(st, hd, d):
    vf, vfd = _svc(st, hd, d, "float64")
    Xq = hd[f"d{d}_Xq"]
    J = vf.get_Jacobian()(Xq)
    h = 1e-4
    num = np.empty_like(J)
    for i in range(d):
        e = np.zeros(d)
        e[i] = h
        vp = st.vector_field_function(Xq + e, vfd, dtype="float64", device="cuda:0")
        vm = st.vector_field_function(Xq - e, vfd, dtype="float64", device="cuda:0")
        num[:, i, :] = ((vp - vm) / (2 * h)).T
    assert _rel(J, num) < 1e-6


def test_v_alone_launches_v_alone_and_the_kernel_wrappers_check_their_inputs(st, hd):
    """vector_field_function at D > 3 runs the 16-column v-only product (no Jacobian columns, nothing else kept); the first
    Jacobian-family call then keeps the rest of that family.  HipKernels.eval_d / gram refuse what mvf_eval_d would misread."""
    from spateo_amd import _lib
    from spateo_amd._kernels import HipKernels

    st.vectorfield.clear_eval_cache()
    vf, vfd = _svc(st, hd, 8, "float64")
    Xq = hd["d8_Xq"]
    assert _rel(vf.compute_velocity(Xq), hd["d8_v"]) < EVAL_TOL["float64"]
    assert st.vectorfield._TLS.fused.flags == _lib.EVAL_V
    assert _rel(vf.compute_divergence(Xq), hd["d8_div"]) < EVAL_TOL["float64"]
    assert st.vectorfield._TLS.fused.flags == _lib.EVAL_V | _lib.EVAL_JAC | _lib.EVAL_DIV | _lib.EVAL_ACC | _lib.EVAL_CURV
    st.vectorfield.clear_eval_cache()

    k = HipKernels("cuda:0", "float64")
    c = hd["d8_Xc"].mean(0)
    xd, cd = k.to_xd(Xq, c), k.to_xd(hd["d8_Xc"], c)
    C = torch.from_numpy(hd["d8_C"]).to("cuda:0")
    cd5 = k.to_xd(hd["d5_Xc"], hd["d5_Xc"].mean(0))
    with pytest.raises(ValueError, match="disagree"):
        k.eval_d(xd, cd5, 0.02, C, _lib.EVAL_V)
    with pytest.raises(TypeError):
        k.eval_d(xd.float(), cd, 0.02, C, _lib.EVAL_V)
    P = torch.ones(len(Xq), dtype=torch.float64, device="cuda:0")
    G = torch.zeros(len(cd), len(cd), dtype=torch.float64, device="cuda:0")
    with pytest.raises(_lib.MVFError, match="cache"):
        k.gram(xd, P, None, cd, 0.02, G, None, tiles_only=True, cache_only=True)


# ------------------------------------------------------------------------------------------------ 4. Spateo wrappers
def test_morphofield_wrappers_in_5_dimensions(st, hd):
    g = hd
    X = g["a5_X"]
    ad = st.AnnDataLite(obsm={"align_spatial": X, "V_mapping": g["a5_V"]})
    assert st.tdr.morphofield_sparsevfc(ad, NX=g["a5_NX"], M=20, MaxIter=20, restart_num=1, restart_seed=[0],
                                        dtype="float64", device="cuda:0") is None
    vf = ad.uns["VecFld_morpho"]
    np.testing.assert_array_equal(vf["X_ctrl"], g["a5_vf_X_ctrl"])
    assert vf["beta"] == pytest.approx(float(g["a5_vf_beta"]), rel=1e-12)
    assert vf["iteration"] == int(g["a5_vf_iteration"])
    assert _rel(vf["V"], g["a5_vf_V"]) < 1e-5 and _rel(vf["grid_V"], g["a5_vf_grid_V"]) < 1e-5
    assert abs(vf["sigma2"] - float(g["a5_vf_sigma2"])) < 1e-5 * float(g["a5_vf_sigma2"])
    # the evaluators on the REFERENCE's coefficients: evaluator parity not mixed with fit parity
    vf["C"] = g["a5_vf_C"]
    st.tdr.morphofield_velocity(ad)
    st.tdr.morphofield_acceleration(ad)
    st.tdr.morphofield_curvature(ad)
    st.tdr.morphofield_divergence(ad)
    st.tdr.morphofield_jacobian(ad)
    tol = 1e-8
    assert _rel(ad.obsm["velocity"], g["a5_velocity"]) < tol
    assert _rel(ad.obs["acceleration"], g["a5_acceleration_obs"]) < tol
    assert _rel(ad.obsm["acceleration"], g["a5_acceleration_obsm"]) < tol
    assert _rel(ad.obs["curvature"], g["a5_curvature_obs"]) < tol
    assert _rel(ad.obsm["curvature"], g["a5_curvature_obsm"]) < tol
    assert _rel(ad.obs["divergence"], g["a5_divergence_obs"]) < tol
    assert ad.uns["jacobian"].shape == g["a5_jacobian_uns"].shape == (5, 5, len(X))
    assert _rel(ad.uns["jacobian"], g["a5_jacobian_uns"]) < tol
    assert _rel(ad.obs["jacobian"], g["a5_jacobian_obs"]) < 1e-6
    # curl and torsion raise as the reference's wrappers did
    assert str(g["a5_curl_exc"]) == "ValueError" and str(g["a5_torsion_exc"]) == "Exception"
    with pytest.raises(ValueError):
        st.tdr.morphofield_curl(ad)
    with pytest.raises(Exception, match="torsion is only defined in 3 dimension"):
        st.tdr.morphofield_torsion(ad)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_kernel_interpolation_on_5_dimensional_coordinates(st, dtype):
    """kernel_interpolation passes obsm[spatial_key] with any number of columns to SparseVFC (interpolation_sparseVFC.py:45,63)."""
    import spateo_amd.vectorfield as vfm

    X, Y, _ = lifted_c2(4000, 5, dy=4, seed=7)
    ad = st.AnnDataLite(X=Y, var_names=["g0", "g1", "g2", "g3"], obsm={"spatial": X})
    tgt = X[:200] * 0.9
    kw = dict(M=80, MaxIter=10, seed=0)
    old = vfm._DEFAULT_DTYPE
    vfm.set_default_dtype(dtype)
    try:
        out = st.tdr.kernel_interpolation(ad, target_points=tgt, keys=["g0", "g1", "g2", "g3"], lambda_=3.0, **kw)
    finally:
        vfm.set_default_dtype(old)
    ref = svo.SparseVFC(X, Y, tgt, lambda_=3.0, lstsq_method="scipy", **kw)["grid_V"]
    assert np.asarray(out.X).shape == (200, 4)
    assert _rel(np.asarray(out.X), ref) < TOL[dtype]


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_what_stays_refused_in_higher_dimensions(st):
    from spateo_amd._lib import MVFError
    from spateo_amd.engine import SparseVFCEngine

    X9 = np.random.default_rng(0).standard_normal((300, 9))
    with pytest.raises(NotImplementedError, match="1-8 spatial dimensions"):
        st.SparseVFC(X9, X9, None, M=20, dtype="float64", device="cuda:0")
    X, Y, _ = lifted_c2(2000, 5, seed=3)
    res = st.SparseVFC(X, Y, None, M=30, MaxIter=5, dtype="float64", device="cuda:0")
    vf = st.SvcVectorField(dtype="float64", device="cuda:0")
    vf.vf_dict, vf.data["X"] = res, X
    with pytest.raises(ValueError):
        vf.compute_curl(X[:10])
    with pytest.raises(Exception, match="torsion is only defined in 3 dimension"):
        vf.compute_torsion(X[:10])
    # the GP variant and the trajectories stay at <= 3 dimensions
    gpd = {"norm_dict": {"scale_fixed": 1.0, "scale_transformed": 1.0, "mean_transformed": np.zeros(5),
                         "mean_fixed": np.zeros(5)}, "kernel_type": "euc", "inducing_variables": res["X_ctrl"],
           "beta": res["beta"], "Coff": res["C"], "R": np.eye(5), "t": np.zeros(5)}
    with pytest.raises(NotImplementedError):
        st.vectorfield.gp_velocity(X[:10], gpd, dtype="float64", device="cuda:0")
    vfd = {"X_ctrl": res["X_ctrl"], "C": res["C"], "beta": res["beta"], "method": "sparsevfc"}
    with pytest.raises(NotImplementedError):
        st.vectorfield.integrate_field(vfd, X[:4], t_end=1.0, interpolation_num=5, dtype="float64", device="cuda:0")
    with pytest.raises(NotImplementedError):
        st.vectorfield.genesis_states(vfd, X[:4], [0.1, 0.1], dtype="float64", device="cuda:0")
    # no regenerating Gram kernel at D > 3: without the cache the fit is refused, naming the bytes it needs
    with pytest.raises(MVFError, match=r"kernel-value cache \(\d+ bytes"):
        SparseVFCEngine(X, Y, X[:30], 0.01, dtype="float64", device="cuda:0", cache_u=False)
