"""GPU parity tests of the EM loop and the drop-in API against the float64 NumPy oracle.

Parity quantity = the learned FIELD (V, grid_V), sigma^2, P - not the coefficients C, which the reference's own
solver only determines up to the numerical null space of the Gram system (DESIGN.md "Solve parity").
Tolerances: float64 mode 1e-5 relative, float32 mode 1e-3 relative (BASELINE.json north_star)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sparsevfc_oracle as svo  # noqa: E402

TOL = {"float64": 1e-5, "float32": 1e-3}


@pytest.fixture(scope="module")
def st():
    import spateo_amd

    assert torch.cuda.is_available()
    return spateo_amd


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _c2(n, noise=0.05):
    from spateo_amd._synthetic import make_config

    X, V, _ = make_config("C2", N=n, noise=noise)
    return X, V


# ------------------------------------------------------------------------------------------- single EM step
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("lambda_", [3.0, 0.02])
def test_single_em_step_from_same_state(st, dtype, lambda_):
    """One EM iteration from the identical state (V = 0): P, G-derived field, sigma^2, gamma, energy."""
    from spateo_amd.vectorfield import SparseVFCEngine, sparsevfc_preprocess

    X, V = _c2(6000)
    valid, Xv, Yv, idx, ctrl, beta = sparsevfc_preprocess(X, V, M=200, seed=0)
    eng = SparseVFCEngine(Xv, Yv, ctrl, beta, dtype=dtype, device="cuda:0")
    eng.init_state(gamma=0.9)
    K = svo.con_K(ctrl, ctrl, beta)
    U = svo.con_K(Xv, ctrl, beta)
    N, D = Yv.shape
    s2 = np.sum(Yv**2) / (N * D)
    np.testing.assert_allclose(eng.sigma2, s2, rtol=1e-6)
    Pr, Er, tecr_r, Cr, Vr, s2r, gr = svo.em_step(
        U, K, Yv, np.zeros_like(Yv), np.zeros((len(ctrl), D)), s2, 0.9, 1, a=5, lambda_=lambda_, minP=1e-5,
        theta=0.75, lstsq_method="scipy")
    E, tecr = eng.em_step(a=5, lambda_=lambda_, minP=1e-5, theta=0.75)
    Vg, Pg, Cg = eng.results()
    tol = TOL[dtype]
    # the first step is well regularised (sigma^2 is large) for both lambdas
    assert _rel(Vg, Vr) < tol
    np.testing.assert_allclose(Pg, Pr, rtol=tol, atol=1e-9)
    np.testing.assert_allclose(eng.sigma2, s2r, rtol=tol)
    assert eng.gamma == pytest.approx(gr, abs=1e-12 if dtype == "float64" else 1e-3)
    np.testing.assert_allclose(E, Er, rtol=tol)
    np.testing.assert_allclose(tecr, tecr_r, rtol=tol)


# ------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sparsevfc_end_to_end_well_regularised(st, dtype):
    """Full fits in the regime where the reference's own solve is stable (lambda_ = 3, dynamo's default)."""
    X, V = _c2(8000)
    Grid = X[::40] + 1.0
    kw = dict(M=300, lambda_=3.0, lstsq_method="scipy", MaxIter=25, seed=0)
    ref = svo.SparseVFC(X, V, Grid, **kw)
    got = st.SparseVFC(X, V, Grid, dtype=dtype, device="cuda:0", **kw)
    tol = TOL[dtype]
    assert got["iteration"] == ref["iteration"]
    assert set(got.keys()) == set(ref.keys()) | {"tecr_vec"}  # + the docstring's name of tecr_traj (sparsevfc.py:155)
    np.testing.assert_array_equal(got["tecr_vec"], got["tecr_traj"])
    for key in ("X", "Y", "valid_ind", "X_ctrl", "ctrl_idx", "grid"):
        np.testing.assert_array_equal(got[key], ref[key])
    assert got["beta"] == pytest.approx(ref["beta"], rel=1e-12)
    assert got["V"].dtype == np.float64 and got["P"].shape == ref["P"].shape == (len(X), 1)
    assert got["C"].shape == ref["C"].shape
    assert _rel(got["V"], ref["V"]) < tol
    assert _rel(got["grid_V"], ref["grid_V"]) < tol
    np.testing.assert_allclose(got["P"], ref["P"], rtol=10 * tol, atol=10 * tol)
    np.testing.assert_allclose(got["sigma2"], ref["sigma2"], rtol=tol)
    np.testing.assert_allclose(got["E_traj"], ref["E_traj"], rtol=tol)
    np.testing.assert_allclose(got["tecr_traj"], ref["tecr_traj"], rtol=5e-2, atol=tol)
    # VFCIndex may differ only for cells whose P sits at the threshold
    diff = set(got["VFCIndex"]) ^ set(ref["VFCIndex"])
    assert all(abs(ref["P"][i, 0] - 0.75) < 10 * tol for i in diff)


@pytest.mark.parametrize("n,M", [(6000, 300), (10000, 800)])
def test_sparsevfc_default_lambda_within_reference_noise_floor(st, n, M):
    """lambda_ = 0.02 (Spateo's default): lambda sigma^2 K becomes negligible, the normal equations are numerically
    singular and the reference's own result moves by O(1e-3) under changes that leave its mathematics untouched (LAPACK
    driver swapped, Gram summed in another order: tests/_floors.py).  The GPU field, sigma^2, P and energy must each sit
    within 1.25x of that measured floor (or inside the north-star tolerance where the floor is below it).  M = 300: the
    deflated solve with its 64-vector block (and the direct form when the factor keeps all 300 columns); M = 800: the
    deflated rank-revealing solve with the 128 / 256-vector blocks."""
    import _floors as F

    X, V = _c2(n)
    kw = dict(M=M, lambda_=0.02, MaxIter=12, seed=0, lstsq_method="scipy")
    if M == 800:
        kw.update(MaxIter=8, ecr=0.0)  # a fixed number of iterations: the reference's own eigh variant stops elsewhere here
    ref = svo.SparseVFC(X, V, None, **kw)
    table = F.floor_table(X, V, None, ref, kw, f32=False)
    got = st.SparseVFC(X, V, None, dtype="float64", device="cuda:0", **kw)
    assert got["iteration"] == ref["iteration"]
    dev = F.deviations(got, ref)
    base = {"V": 1e-5, "sigma2": 1e-5, "E": 1e-5, "P999": 1e-4}
    print("; ".join(f"{k} gpu {dev[k]:.2e} / floor {table[k][0]:.2e}" for k in dev))
    print(F.fmt(table))
    for k in base:  # the 99.9th percentile of |dP| carries the 1.25 x; max |dP| ("P") the loose hard cap (tests/_floors.py)
        assert dev[k] <= F.tol("float64", table, k, base[k]), (k, dev[k], table[k])
    assert dev["P"] <= F.cap("float64", table, "P", 1e-4), ("P", dev["P"], table["P"])


def test_sparsevfc_2d_config1(st):
    """BASELINE config 1 geometry (2-D, N = 1000, M = 100) through the GPU path."""
    rng = np.random.default_rng(1)
    n = 1000
    X = rng.uniform(0, 1, (n, 2)) * 100
    th = np.deg2rad(30)
    Rm = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    V = 0.05 * (X - 50) @ (Rm - np.eye(2)).T + 0.1 * rng.standard_normal((n, 2))
    out = rng.choice(n, n // 10, replace=False)
    V[out] = 5 * rng.standard_normal((len(out), 2))
    gx, gy = np.meshgrid(np.linspace(0, 100, 20), np.linspace(0, 100, 20))
    NX = np.column_stack([gx.ravel(), gy.ravel()])
    kw = dict(M=100, lambda_=3.0, lstsq_method="scipy", MaxIter=30)
    ref = svo.SparseVFC(X, V, NX, **kw)
    got = st.SparseVFC(X, V, NX, dtype="float64", device="cuda:0", **kw)
    assert got["V"].shape == (n, 2) and got["C"].shape == (100, 2) and got["grid_V"].shape == (400, 2)
    assert got["iteration"] == ref["iteration"]
    assert _rel(got["V"], ref["V"]) < 1e-5 and _rel(got["grid_V"], ref["grid_V"]) < 1e-5


def test_sparsevfc_non_finite_rows_and_duplicates(st):
    X, V = _c2(3000)
    V[[5, 100, 2999]] = np.nan
    X[10] = X[11]  # duplicate coordinates: np.unique path
    kw = dict(M=150, lambda_=3.0, lstsq_method="scipy", MaxIter=6)
    ref = svo.SparseVFC(X, V, None, **kw)
    got = st.SparseVFC(X, V, None, dtype="float64", device="cuda:0", **kw)
    np.testing.assert_array_equal(got["valid_ind"], ref["valid_ind"])
    assert got["V"].shape == ref["V"].shape == (2997, 3)
    assert got["grid_V"] is None
    assert _rel(got["V"], ref["V"]) < 1e-5


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("dy", [1, 5, 16, 31])
def test_sparsevfc_wide_and_narrow_outputs(st, dtype, dy):
    """Dy != D (kernel_interpolation's call shape): 3-column groups sharing one Gram matrix per EM step.  Dy = 16 and 31: the
    column counts at which 3 x the number of groups overshoots the 16-column padding of the wide path's buffers (a fit with 16
    genes raised a shape error until the re-entry of round 6: found by tools/api_stall_probe.py, no test had that width)."""
    rng = np.random.default_rng(dy)
    X, _ = _c2(5000)
    Y = np.column_stack([np.sin(X[:, 0] / 80 + j) + 0.3 * np.cos(X[:, 1] / 60 * (j + 1)) for j in range(dy)])
    Y += 0.02 * rng.standard_normal(Y.shape)
    kw = dict(M=150, lambda_=3.0, lstsq_method="scipy", MaxIter=10, seed=0)
    ref = svo.SparseVFC(X, Y, X[::50], **kw)
    got = st.SparseVFC(X, Y, X[::50], dtype=dtype, device="cuda:0", **kw)
    assert got["V"].shape == (5000, dy) and got["C"].shape == (150, dy) and got["grid_V"].shape == (100, dy)
    assert got["iteration"] == ref["iteration"]
    assert _rel(got["V"], ref["V"]) < TOL[dtype] and _rel(got["grid_V"], ref["grid_V"]) < TOL[dtype]
    np.testing.assert_allclose(got["sigma2"], ref["sigma2"], rtol=TOL[dtype])


def test_sparsevfc_tiny_inputs(st):
    """Fewer cells than one 128-wide tile / one 256-cell stage; M clipped to the unique rows; explicit beta."""
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((5, 3)), rng.standard_normal((5, 3)) * 0.1
    kw = dict(lambda_=3.0, lstsq_method="scipy", MaxIter=3)
    for Xi, Yi, M, extra in ((X, Y, 3, {}), (X[:2], Y[:2], 5, {}), (X, Y, 2, {"beta": 0.3})):
        ref = svo.SparseVFC(Xi, Yi, Xi, M=M, **kw, **extra)
        for dtype, tol in (("float64", 1e-6), ("float32", 1e-3)):
            got = st.SparseVFC(Xi, Yi, Xi, M=M, dtype=dtype, device="cuda:0", **kw, **extra)
            assert got["iteration"] == ref["iteration"] and got["V"].shape == ref["V"].shape
            np.testing.assert_allclose(got["V"], ref["V"], rtol=tol, atol=tol * np.abs(ref["V"]).max())
            np.testing.assert_allclose(got["grid_V"], ref["grid_V"], rtol=tol, atol=tol * np.abs(ref["V"]).max())


def test_sparsevfc_errors(st):
    X, V = _c2(100)
    with pytest.raises(NotImplementedError):
        st.SparseVFC(X, V, None, div_cur_free_kernels=True)
    with pytest.raises(ValueError):
        st.SparseVFC(X, V[:50], None)
    with pytest.raises(ValueError):
        st.SparseVFC(X, np.full_like(V, np.nan), None)


# ------------------------------------------------------------------------------------------- wrappers
def test_morphofield_wrappers_against_reference_goldens(st, golden):
    """The AnnData wrappers driven exactly like the reference wrappers were when the goldens were generated
    (tests/golden/make_golden.py): fit, then the seven morphofield_* evaluators."""
    g = golden
    ad = st.AnnDataLite(obsm={"align_spatial": g["a_X"], "V_mapping": g["a_V"]})
    out = st.tdr.morphofield_sparsevfc(ad, NX=g["a_X"][:5], M=15, MaxIter=20, restart_num=1, restart_seed=[0],
                                       dtype="float64", device="cuda:0")
    assert out is None
    vf = ad.uns["VecFld_morpho"]
    assert vf["method"] == "sparsevfc"
    np.testing.assert_array_equal(vf["X_ctrl"], g["a_vf_X_ctrl"])
    assert vf["beta"] == pytest.approx(float(g["a_vf_beta"]), rel=1e-12)
    assert _rel(vf["V"], g["a_vf_V"]) < 1e-5
    assert _rel(vf["grid_V"], g["a_vf_grid_V"]) < 1e-5
    # evaluators on the REFERENCE's coefficients, so that evaluator parity is not mixed with fit parity
    vf["C"] = g["a_vf_C"]
    st.tdr.morphofield_velocity(ad)
    st.tdr.morphofield_acceleration(ad)
    st.tdr.morphofield_curvature(ad)
    st.tdr.morphofield_curl(ad)
    st.tdr.morphofield_torsion(ad)
    st.tdr.morphofield_divergence(ad)
    st.tdr.morphofield_jacobian(ad)
    tol = 1e-8
    assert _rel(ad.obsm["velocity"], g["a_velocity"]) < tol
    assert _rel(ad.obs["acceleration"], g["a_acceleration_obs"]) < tol
    assert _rel(ad.obsm["acceleration"], g["a_acceleration_obsm"]) < tol
    assert _rel(ad.obs["curvature"], g["a_curvature_obs"]) < tol
    assert _rel(ad.obsm["curvature"], g["a_curvature_obsm"]) < tol
    assert ad.obsm["curl"].shape == g["a_curl_obsm"].shape == (len(g["a_X"]), 3, 3)
    assert _rel(ad.obs["curl"], g["a_curl_obs"]) < tol and _rel(ad.obsm["curl"], g["a_curl_obsm"]) < tol
    assert _rel(ad.obs["torsion"], g["a_torsion_obs"]) < 1e-6
    assert _rel(ad.uns["torsion"], g["a_torsion_uns"]) < 1e-6
    assert _rel(ad.obs["divergence"], g["a_divergence_obs"]) < tol
    assert ad.uns["jacobian"].shape == g["a_jacobian_uns"].shape
    assert _rel(ad.uns["jacobian"], g["a_jacobian_uns"]) < tol
    assert _rel(ad.obs["jacobian"], g["a_jacobian_obs"]) < 1e-6


def test_morphofield_restart_loop_golden(st, golden):
    """_morphofield_sparsevfc with grid generation + restart loop, vs the reference wrapper's golden output."""
    g = golden
    res = st.tdr._morphofield_sparsevfc(
        g["w_X"][:300], g["w_V"][:300], NX=None, grid_num=[5, 4, 3], M=30, lambda_=0.02, lstsq_method="scipy",
        min_vel_corr=0.5, restart_num=3, restart_seed=[0, 100, 200], MaxIter=30, dtype="float64", device="cuda:0")
    assert res["method"] == "sparsevfc"
    np.testing.assert_array_equal(res["X_ctrl"], g["w1_X_ctrl"])
    np.testing.assert_allclose(res["grid"], g["w1_grid"], rtol=1e-13)
    assert res["iteration"] == int(g["w1_iteration"])
    assert _rel(res["V"], g["w1_V"]) < 1e-5
    assert _rel(res["grid_V"], g["w1_grid_V"]) < 1e-5
    np.testing.assert_allclose(res["sigma2"], float(g["w1_sigma2"]), rtol=1e-5)
    # forced restarts (unreachable threshold) + the default seed-length quirk: best-of fallback
    Xf, Vf = g["w_X"][300:], g["w_V"][300:]
    res2 = st.tdr._morphofield_sparsevfc(Xf, Vf, NX=Xf[:10], M=12, min_vel_corr=2.0, restart_num=2,
                                         restart_seed=(0, 100, 200, 300, 400), MaxIter=8, dtype="float64",
                                         device="cuda:0")
    np.testing.assert_array_equal(res2["X_ctrl"], g["w2_X_ctrl"])
    assert _rel(res2["V"], g["w2_V"]) < 1e-5 and _rel(res2["grid_V"], g["w2_grid_V"]) < 1e-5


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-9), ("float32", 2e-4)])
def test_gp_variant_against_reference_goldens(st, golden, dtype, tol):
    """Gaussian-process morphofield variant on the GPU (fused evaluator with the affine epilogue) against the outputs
    of the real reference wrappers (morphofield_gp, GPVectorField, differential_geometry)."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _gp_case import gp_dict, run_and_check

    st.set_default_dtype(dtype)
    try:
        g = golden
        v = st.vectorfield.gp_velocity(g["gp_Xq"], gp_dict(g))
        assert _rel(v, g["gp_vel"]) < tol
        assert _rel(st.vectorfield.gp_velocity(g["gp_Xq"], gp_dict(g), nonrigid_only=True), g["gp_vel_nonrigid"]) < tol
        run_and_check(st, g, tol)
    finally:
        st.set_default_dtype("float64")


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-9), ("float32", 2e-4)])
def test_gp_variant_per_axis_scales_and_2d_fields(st, dtype, tol):
    """Per-axis ``norm_dict`` scales (per-component alpha of the affine epilogue, ABI 6) and 2-D GP fields (zero-padded 3-D
    points) on the fused evaluator, against goldens of the real reference functions (tests/golden/ref_gp_axes.npz)."""
    import os, sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    from _gp_case import check_axes_and_2d

    g = dict(np.load(os.path.join(here, "golden", "ref_gp_axes.npz")))
    check_axes_and_2d(st, g, tol, dtype=dtype, device="cuda:0")


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-6), ("float32", 2e-4)])  # RK4 truncation at 4 substeps ~3e-7
def test_morphopath_fused_rk4_vs_dop853(st, golden, dtype, tol):
    """The fused RK4 integration kernel against SciPy DOP853 on the float64 oracle field (sparsevfc and GP fields)."""
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _gp_case import gp_dict
    from oracle import trajectory_oracle as tro
    from spateo_amd.vectorfield import integrate_field

    g = golden
    vf = {k: g[f"a_vf_{k}"] for k in ["X_ctrl", "C", "V"]}
    vf.update(X=g["a_X"], beta=float(g["a_vf_beta"]), method="sparsevfc")
    x0 = g["a_X"][:40]
    tq = np.linspace(0, 30, 16)
    t, pred = integrate_field(vf, x0, t_end=30.0, interpolation_num=16, dtype=dtype, device="cuda:0",
                            sampling="uniform_time")
    ref = tro.integrate(vf, x0, tq)
    assert np.abs(np.stack(pred) - ref).max() / np.abs(ref).max() < tol
    np.testing.assert_allclose(t[0], tq)
    # GP field (norm_dict scaling + rigid part): the oracle field is the reference twin's formula
    gd = gp_dict(g)
    gd.update(X=g["gpw_X"], V=g["gpw_full_V"], method="gaussian_process")

    def gp_field(x):
        nd = gd["norm_dict"]
        xn = (np.atleast_2d(x) - nd["mean_transformed"]) / nd["scale_transformed"]
        vel = svo.con_K(xn, gd["inducing_variables"], gd["beta"]).reshape(len(xn), -1) @ gd["Coff"]
        q = (vel + xn @ gd["R"].T + gd["t"]) * nd["scale_fixed"] + nd["mean_fixed"]
        return (q - np.atleast_2d(x)) / 10000

    np.testing.assert_allclose(gp_field(g["gp_Xq"]), g["gp_vel"], rtol=1e-10)  # the restated field == the twin
    tq2 = np.linspace(0, 2000.0, 11)
    t2, pred2 = integrate_field(gd, g["gpw_X"][:10], t_end=2000.0, interpolation_num=11, dtype=dtype, device="cuda:0",
                              sampling="uniform_time")
    ref2 = tro.integrate(gd, g["gpw_X"][:10], tq2, field=gp_field)
    assert np.abs(np.stack(pred2) - ref2).max() / np.abs(ref2).max() < tol


def test_many_independent_fits_on_streams(st):
    """BASELINE config 5 shape (independent organs, one per HIP stream): concurrent fits == sequential fits == the
    oracle's fits."""
    from spateo_amd.vectorfield import SparseVFC_many
    from spateo_amd._synthetic import ellipsoid_cloud, displacement_field

    data = []
    for k in range(6):
        rng = np.random.default_rng(100 + k)
        X = ellipsoid_cloud(rng, 3000 + 200 * k, rng.uniform(100, 400, 3))
        V = displacement_field(X)
        V = V / np.sqrt(np.mean(V**2)) + 0.05 * rng.standard_normal(X.shape)
        data.append((X, V, X[:20]))
    kw = dict(M=100, lambda_=3.0, MaxIter=8, dtype="float64")
    seq = [st.SparseVFC(X, V, G, device="cuda:0", **kw) for X, V, G in data]
    par = SparseVFC_many(data, n_streams=3, device="cuda:0", **kw)
    assert len(par) == 6
    for a, b in zip(seq, par):
        np.testing.assert_array_equal(a["X_ctrl"], b["X_ctrl"])
        assert _rel(b["V"], a["V"]) < 1e-10 and _rel(b["grid_V"], a["grid_V"]) < 1e-10
        assert a["iteration"] == b["iteration"]
    # ... and the concurrent fits are the ORACLE's fits (M = 100: the single-launch solve path), not only each other's
    okw = dict(M=100, lambda_=3.0, MaxIter=8, lstsq_method="scipy")  # what the device solve implements (also for "drouin")
    for (X, V, G), b in zip(data[:3], par[:3]):
        ref = svo.SparseVFC(X, V, G, **okw)
        assert b["iteration"] == ref["iteration"]
        assert _rel(b["V"], ref["V"]) < 1e-5 and _rel(b["grid_V"], ref["grid_V"]) < 1e-5
        np.testing.assert_allclose(b["sigma2"], ref["sigma2"], rtol=1e-5)


def test_morphofield_missing_key_errors(st):
    ad = st.AnnDataLite(obsm={"align_spatial": np.zeros((3, 3))})
    ad.uns["bad"] = {"method": "nope"}
    with pytest.raises(Exception, match="is not in ``anndata.uns"):
        st.tdr.morphofield_velocity(ad, vf_key="bad")
    with pytest.raises(KeyError):
        st.tdr.morphofield_velocity(ad, vf_key="absent")


# ------------------------------------------------------------------------------------------- size-independent
def test_large_n_properties_float32(st):
    """Properties that hold at any size (checked at N = 400k, M = 1000 - the oracle cannot run here in seconds):
    linearity of the rhs in Y, symmetry/PSD-ness of G, agreement of the recompute path with a materialised con_K,
    and V == U C on a sample of rows."""
    from spateo_amd._kernels import HipKernels
    from spateo_amd._synthetic import make_config

    X, V, _ = make_config("C3", N=400_000)
    rng = np.random.default_rng(0)
    ctrl = X[rng.choice(len(X), 1000, replace=False)]
    from spateo_amd.vectorfield import bandwidth_selector

    beta = 1 / bandwidth_selector(ctrl) ** 2
    k = HipKernels("cuda:0", "float32")
    c = ctrl.mean(0)
    x4, c4 = k.to_x4(X, c), k.to_x4(ctrl, c)
    P = torch.rand(len(X), device="cuda:0") * 0.99 + 0.01
    m = 1000
    G = torch.empty(m, m, dtype=torch.float64, device="cuda:0")
    R1, R2, R12 = (torch.empty(m, 3, dtype=torch.float64, device="cuda:0") for _ in range(3))
    Y1, Y2 = V, rng.standard_normal(V.shape)
    k.gram(x4, P, k.to_x4(Y1), c4, beta, G, R1)
    k.gram(x4, P, k.to_x4(Y2), c4, beta, G, R2)
    k.gram(x4, P, k.to_x4(Y1 + Y2), c4, beta, G, R12)
    assert float((R12 - R1 - R2).abs().max() / R12.abs().max()) < 1e-5  # linearity in Y
    Gh = G.cpu().numpy()
    assert np.array_equal(Gh, Gh.T)
    ev = np.linalg.eigvalsh(Gh)
    assert ev.min() > -1e-12 * ev.max()  # float64-accumulated Gram: PSD up to round-off
    # Gram from a materialised float32 con_K on a row sample == recompute path restricted to that sample
    sel = np.sort(rng.choice(len(X), 20000, replace=False))
    xs = torch.from_numpy((X[sel] - c).astype(np.float32)).to("cuda:0")
    cs = torch.from_numpy((ctrl - c).astype(np.float32)).to("cuda:0")
    U = k.con_k(xs, cs, beta).double()
    Ps = P[torch.from_numpy(sel).to("cuda:0")].double()
    Gs_ref = (U * Ps[:, None]).T @ U
    Gs = torch.empty_like(G)
    Rs = torch.empty_like(R1)
    k.gram(k.to_x4(X[sel], c), Ps.float(), k.to_x4(Y1[sel]), c4, beta, Gs, Rs)
    assert float((Gs - Gs_ref).abs().max() / Gs_ref.abs().max()) < 1e-5
    # V == U C on the sample
    C = torch.from_numpy(rng.standard_normal((m, 3))).to("cuda:0")
    V4, _ = k.apply(k.to_x4(X[sel], c), c4, beta, C)
    assert float((V4[:, :3].double() - U @ C).abs().max() / (U @ C).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------- multi-rank on one GPU
def _two_rank_worker(rank, world, port, out_dir, case):
    import os
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (root, os.path.join(root, "spateo-release_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    # gloo moves the (device) tensors of the collectives through the host: both ranks can share cuda:0, which RCCL
    # refuses; everything else - sharding, HIP kernels per shard, the all-reduced [tri(G) | R | stats] buffer - is the
    # production path
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import spateo_amd as st
        from spateo_amd._synthetic import make_config
        from spateo_amd.vectorfield import SparseVFC_many

        X, V, _ = make_config("C2", N=9001)
        kw = dict(M=200, lambda_=3.0, lstsq_method="scipy", MaxIter=8, seed=0, device="cuda:0")
        if case == "many":  # replicas only: organ i is fitted by rank i % world, results exchanged as objects
            data = [(X[i::3], V[i::3], None) for i in range(3)]
            res = SparseVFC_many(data, distributed=True, dtype="float64", **kw)
            np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **{f"V{i}": r_["V"] for i, r_ in enumerate(res)})
            return
        dtype = "float32" if case == "float32" else "float64"
        if case == "minnorm4":  # Spateo's default lambda_: every rank runs the eigensolver redundantly, in step
            kw.update(M=300, lambda_=0.02)
        if case == "wide":
            V = np.column_stack([V, np.sin(X[:, 0] / 70), np.cos(X[:, 1] / 50)])
        if case == "own_shards":  # uneven: 6001 + 3000 rows, each rank passes only its own
            lo, hi = (0, 6001) if rank == 0 else (6001, 9001)
            got = st.SparseVFC(X[lo:hi], V[lo:hi], X[::50], dtype=dtype, distributed=True, sharded_input=True, **kw)
        else:
            got = st.SparseVFC(X, V, X[::50], dtype=dtype, distributed=True, gather="all", **kw)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), V=got["V"], P=got["P"], grid_V=got["grid_V"],
                 sigma2=got["sigma2"], iteration=got["iteration"], E=got["E_traj"])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", ["float64", "float32", "wide", "own_shards", "many"])
def test_two_ranks_sharing_one_gpu_match_the_oracle(st, tmp_path, case):
    """Cells sharded over 2 processes (both on cuda:0, gloo collectives on device tensors) == single oracle fit:
    float64 / float32 cells, a wide Y (two column groups), every rank bringing its own uneven shard (root gather), and
    SparseVFC_many's replicas-only distribution."""
    import socket

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_two_rank_worker, args=(2, port, str(tmp_path), case), nprocs=2, join=True)
    X, V = _c2(9001)
    kw = dict(M=200, lambda_=3.0, lstsq_method="scipy", MaxIter=8, seed=0)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    if case == "many":
        for i in range(3):
            ref = svo.SparseVFC(X[i::3], V[i::3], None, **kw)
            np.testing.assert_array_equal(r0[f"V{i}"], r1[f"V{i}"])
            assert _rel(r0[f"V{i}"], ref["V"]) < 1e-5
        return
    if case == "wide":
        V = np.column_stack([V, np.sin(X[:, 0] / 70), np.cos(X[:, 1] / 50)])
    ref = svo.SparseVFC(X, V, X[::50], **kw)
    tol = 1e-3 if case == "float32" else 1e-5
    if case == "own_shards":
        np.testing.assert_array_equal(r1["V"], r0["V"][6001:])  # rank 1 kept its own rows of the root's gathered result
    else:
        for k in ("V", "P"):
            np.testing.assert_array_equal(r0[k], r1[k])
    for k in ("grid_V", "sigma2", "E"):
        np.testing.assert_array_equal(r0[k], r1[k])
    assert int(r0["iteration"]) == ref["iteration"]
    assert _rel(r0["V"], ref["V"]) < tol and _rel(r0["grid_V"], ref["grid_V"]) < tol
    np.testing.assert_allclose(r0["E"], ref["E_traj"], rtol=max(tol / 10, 1e-6))


def test_four_ranks_sharing_one_gpu_minimum_norm_path(st, tmp_path):
    """4 ranks (all on cuda:0, gloo collectives), lambda_ = 0.02: the system goes numerically rank deficient, every rank
    runs the minimum-norm eigensolver redundantly on the all-reduced Gram system and the per-step agreement check
    (SparseVFCEngine._finish_step) passes on every step; all ranks end bit-identical and at the reference's floor."""
    import socket

    import _floors as F
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_two_rank_worker, args=(4, port, str(tmp_path), "minnorm4"), nprocs=4, join=True)
    X, V = _c2(9001)
    kw = dict(M=300, lambda_=0.02, lstsq_method="scipy", MaxIter=8, seed=0)
    ref = svo.SparseVFC(X, V, X[::50], **kw)
    table = F.floor_table(X, V, X[::50], ref, kw, f32=False)
    rs = [np.load(tmp_path / f"rank{r}.npz") for r in range(4)]
    for r in rs[1:]:
        for k in ("V", "P", "grid_V", "sigma2", "E"):
            np.testing.assert_array_equal(rs[0][k], r[k])
    assert int(rs[0]["iteration"]) == ref["iteration"]
    err = _rel(rs[0]["V"], ref["V"])
    print(f"4 ranks, lambda 0.02: V err {err:.2e}, floor {table['V'][0]:.2e}")
    assert err <= F.tol("float64", table, "V", 1e-5)


# ------------------------------------------------------------------------------------------- BASELINE full size
def test_full_size_c4_invariants_float32(st):
    """BASELINE config 4 at FULL size on one GPU (8 M cells x 3000 control points, float32 cells) - where the oracle
    cannot run - through size-independent properties: the cached-U and the recompute Gram kernels agree bit for bit,
    G is symmetric PSD (up to round-off), the EM statistics are consistent, and V == con_K(X, ctrl) @ C on sampled rows
    (materialised kernel rows x float64 coefficients)."""
    from spateo_amd._kernels import HipKernels
    from spateo_amd._synthetic import make_config
    from spateo_amd.vectorfield import SparseVFCEngine, sparsevfc_preprocess

    X, V, M = make_config("C4")
    valid, Xv, Yv, idx, ctrl, beta = sparsevfc_preprocess(X, V, M=M, seed=0)
    N = len(Xv)
    assert N == 8_000_000 and len(ctrl) == 3000
    kern = HipKernels("cuda:0", "float32")
    eng = SparseVFCEngine(Xv, Yv, ctrl, beta, dtype="float32", device="cuda:0", kernels=kern, cache_u=True)
    assert eng.cached_u
    eng.init_state(0.9)
    np.testing.assert_allclose(eng.sigma2, np.sum(Yv**2) / (N * 3), rtol=1e-5)
    E, tecr = eng.em_step(lambda_=0.02)
    assert np.isfinite(E) and eng.sigma2 > 0 and 0.05 <= eng.gamma <= 0.95
    st_ = eng.st.cpu().numpy()
    assert 1e-5 * N * 0.999 <= st_[2] <= N and st_[3] <= N  # sum of floored P, #inliers
    G_cached = eng.G.clone()
    # the same Gram through the recompute kernel (cache dropped): identical bits
    kern.drop_ublk()
    G2 = torch.empty_like(eng.G)
    R2 = torch.empty_like(eng.R[0])
    kern.gram(eng.x4, eng.P, eng.y4[0], eng.ctrl4, eng.beta, G2, R2)
    assert torch.equal(G2, G_cached)
    assert torch.equal(R2, eng.R[0])
    assert torch.equal(G2, G2.T)
    ev = torch.linalg.eigvalsh(G2)
    assert float(ev.min()) > -1e-10 * float(ev.max())
    # V == U C on a sample of rows
    rng = np.random.default_rng(0)
    sel = torch.from_numpy(np.sort(rng.choice(N, 4096, replace=False))).to("cuda:0")
    xs = eng.x4[sel][:, :3].contiguous()
    cs = eng.ctrl4[:, :3].contiguous()
    U = kern.con_k(xs, cs, eng.beta).double()
    Vs = U @ eng.C[0]
    got = eng.V4[0][sel][:, :3].double()
    assert float((got - Vs).abs().max() / Vs.abs().max()) < 2e-4  # float32 storage of V + per-kernel K rounding
    # residuals and sigma^2 are consistent with V
    r_s = ((eng.y4[0][sel][:, :3].double() - got) ** 2).sum(1)
    assert float((eng.r[sel].double() - r_s).abs().max() / r_s.abs().max()) < 1e-5


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-12), ("float32", 1e-5)])
def test_ba_transform_against_reference_goldens(st, golden_align, dtype, tol):
    """Alignment-side caller: BA_transform on the GPU against the outputs of the real
    spateo/alignment/transform.py, and con_K against the alignment module's ||x||^2+||y||^2-2x.y formulation."""
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _align_case import check_ba

    g = golden_align
    check_ba(st.align.BA_transform, g, tol, dtype=dtype)
    K = st.con_K(g["ak_x"], g["ak_y"], float(g["ak_beta"]), dtype=dtype)
    assert _rel(K, g["ak_K"]) < (1e-13 if dtype == "float64" else 1e-6)


# ------------------------------------------------------------------------------------------- kernel_interpolation
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_kernel_interpolation_wrapper_on_the_gpu(st, dtype):
    """``st.tdr.kernel_interpolation`` itself (interpolation_sparseVFC.py:13-85: obs keys + genes -> wide Y -> grid_V split
    back) on the real kernels, against the oracle at the SparseVFC seam."""
    import spateo_amd.vectorfield as vfm

    rng = np.random.default_rng(3)
    n = 5000
    S = rng.uniform(-1, 1, (n, 3)) * 50
    genes = np.column_stack([np.sin(S[:, 0] / 20), np.cos(S[:, 1] / 15), S[:, 2] / 50, np.sin(S[:, 0] / 9) ** 2,
                             np.cos(S[:, 2] / 11) * np.sin(S[:, 1] / 13)])
    genes += 0.01 * rng.standard_normal(genes.shape)
    score = np.cos(S[:, 2] / 25)
    ad = st.AnnDataLite(X=genes, var_names=["g0", "g1", "g2", "g3", "g4"], obs={"score": score}, obsm={"spatial": S})
    tgt = rng.uniform(-1, 1, (300, 3)) * 45
    kw = dict(M=120, MaxIter=10, seed=0)
    old = vfm._DEFAULT_DTYPE
    vfm.set_default_dtype(dtype)
    try:
        out = st.tdr.kernel_interpolation(ad, target_points=tgt, keys=["g2", "score", "g0", "g3", "g4"], lambda_=3.0, **kw)
    finally:
        vfm.set_default_dtype(old)
    info = np.column_stack([score, genes[:, [2, 0, 3, 4]]])  # obs keys first, then genes, each in `keys` order
    ref = svo.SparseVFC(S, info, tgt, lambda_=3.0, lstsq_method="scipy", **kw)["grid_V"]
    got = np.column_stack([np.asarray(out.obs["score"], dtype=float), np.asarray(out.X)])
    assert got.shape == (300, 5) and list(out.var_names) == ["g2", "g0", "g3", "g4"]
    assert _rel(got, ref) < TOL[dtype]
    np.testing.assert_array_equal(np.asarray(out.obsm["spatial"]), tgt)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_wide_y_through_the_cached_kernel_values(st, dtype):
    """Dy = 48 (kernel_interpolation with 48 genes): R = U^T P Y and V = U C run as MFMA products that stream the cached U
    once for all columns (mvf_rhs_cached / mvf_apply_cached, round 6).  Against the oracle within the mode's tolerance, and
    against this repository's own three-columns-at-a-time path (the VALU kernels of rounds 1 - 5: same mathematics, other
    summation order) far inside it; the fit takes the same number of iterations either way."""
    import spateo_amd.vectorfield as vfm

    rng = np.random.default_rng(11)
    n, dy = 6000, 48
    S = rng.uniform(-1, 1, (n, 3)) * 60
    f = np.column_stack([np.sin(S[:, 0] / (9 + j)) * np.cos(S[:, 1] / (7 + 0.5 * j)) + 0.02 * j * S[:, 2] / 60 for j in range(dy)])
    f += 0.01 * rng.standard_normal(f.shape)
    f[rng.choice(n, n // 20, replace=False)] += rng.standard_normal((n // 20, dy))   # 5 % outliers
    tgt = rng.uniform(-1, 1, (200, 3)) * 55
    kw = dict(M=150, lambda_=3.0, lstsq_method="scipy", MaxIter=12, seed=0)
    ref = svo.SparseVFC(S, f, tgt, **kw)
    got = st.SparseVFC(S, f, tgt, dtype=dtype, device="cuda:0", **kw)
    old = vfm.SparseVFCEngine.wide_y
    vfm.SparseVFCEngine.wide_y = False
    try:
        narrow = st.SparseVFC(S, f, tgt, dtype=dtype, device="cuda:0", **kw)
    finally:
        vfm.SparseVFCEngine.wide_y = old
    assert got["V"].shape == (n, dy) and got["C"].shape == (150, dy) and got["grid_V"].shape == (200, dy)
    assert got["iteration"] == ref["iteration"] == narrow["iteration"]
    tol = TOL[dtype]
    print(f"wide Dy = {dy} {dtype}: V vs oracle {_rel(got['V'], ref['V']):.2e}, grid {_rel(got['grid_V'], ref['grid_V']):.2e}, "
          f"sigma2 {abs(got['sigma2'] / ref['sigma2'] - 1):.2e}; vs the three-column path V {_rel(got['V'], narrow['V']):.2e}, "
          f"P {np.abs(got['P'] - narrow['P']).max():.2e}")
    assert _rel(got["V"], ref["V"]) < tol and _rel(got["grid_V"], ref["grid_V"]) < tol
    assert abs(got["sigma2"] / ref["sigma2"] - 1) < tol and np.abs(got["P"] - ref["P"]).max() < 10 * tol
    assert _rel(got["V"], narrow["V"]) < 0.1 * tol and np.abs(got["P"] - narrow["P"]).max() < tol


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_wide_y_beyond_one_column_chunk(st, dtype):
    """Dy = 130: mvf_rhs_cached / mvf_apply_cached take their columns 128 at a time, so this fit runs the second trip of both
    loops (the partial-tile buffer with another leading dimension, r read back and added to, sum P r formed by the last launch
    only).  Against the oracle at the mode's tolerance, against the three-column path at a tenth of it, same iteration count all
    three ways - the assertions of the Dy = 48 test above."""
    import spateo_amd.vectorfield as vfm

    rng = np.random.default_rng(13)
    n, dy = 3000, 130
    S = rng.uniform(-1, 1, (n, 3)) * 60
    f = np.column_stack([np.sin(S[:, 0] / (9 + j)) * np.cos(S[:, 1] / (7 + 0.5 * j)) + 0.02 * j * S[:, 2] / 60 for j in range(dy)])
    f += 0.01 * rng.standard_normal(f.shape)
    f[rng.choice(n, n // 20, replace=False)] += rng.standard_normal((n // 20, dy))   # 5 % outliers
    tgt = rng.uniform(-1, 1, (200, 3)) * 55
    kw = dict(M=100, lambda_=3.0, lstsq_method="scipy", MaxIter=8, seed=0)
    ref = svo.SparseVFC(S, f, tgt, **kw)
    got = st.SparseVFC(S, f, tgt, dtype=dtype, device="cuda:0", **kw)
    old = vfm.SparseVFCEngine.wide_y
    vfm.SparseVFCEngine.wide_y = False
    try:
        narrow = st.SparseVFC(S, f, tgt, dtype=dtype, device="cuda:0", **kw)
    finally:
        vfm.SparseVFCEngine.wide_y = old
    assert got["V"].shape == (n, dy) and got["C"].shape == (100, dy) and got["grid_V"].shape == (200, dy)
    assert got["iteration"] == ref["iteration"] == narrow["iteration"]
    tol = TOL[dtype]
    print(f"wide Dy = {dy} {dtype}: V vs oracle {_rel(got['V'], ref['V']):.2e}, grid {_rel(got['grid_V'], ref['grid_V']):.2e}, "
          f"sigma2 {abs(got['sigma2'] / ref['sigma2'] - 1):.2e}; vs the three-column path V {_rel(got['V'], narrow['V']):.2e}, "
          f"P {np.abs(got['P'] - narrow['P']).max():.2e}")
    assert _rel(got["V"], ref["V"]) < tol and _rel(got["grid_V"], ref["grid_V"]) < tol
    assert abs(got["sigma2"] / ref["sigma2"] - 1) < tol and np.abs(got["P"] - ref["P"]).max() < 10 * tol
    assert _rel(got["V"], narrow["V"]) < 0.1 * tol and np.abs(got["P"] - narrow["P"]).max() < tol


# ------------------------------------------------------------------------------------------- alignment M-step
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_update_nonrigid_against_reference_goldens(st, golden_em, dtype):
    """mvf_gram + mvf_solve_minnorm + mvf_apply against the outputs of the REAL Morpho_pairwise._construct_kernel +
    _update_nonrigid (tests/golden/make_golden_em.py): the in-tree reference statement of the M-step arithmetic."""
    from _align_case import check_update_nonrigid

    errs = check_update_nonrigid(st.align.update_nonrigid, golden_em, dtype, device="cuda:0")
    print(f"update_nonrigid {dtype}: (SigmaInv, VnA) errors vs reference: {errs}")
    from _align_case import check_update_nonrigid_branches

    errs = check_update_nonrigid_branches(st.align.update_nonrigid, golden_em, dtype, device="cuda:0")
    print(f"update_nonrigid {dtype}, guidance / SVI / both branches vs reference: {errs}")


# ------------------------------------------------------------------------------------------- morphopath: fate semantics
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_morphopath_fate_semantics_and_genesis_on_the_gpu(st, golden, dtype):
    """``st.tdr.morphopath`` with dynamo fate's default arc-length sampling and ``construct_genesis_states`` on the real
    kernels (mvf_integrate + mvf_eval), against the restated dynamo procedure / SciPy odeint."""
    from _fate_case import _fate_case, check_fate_semantics
    from oracle import trajectory_oracle as tro

    if dtype == "float64":
        check_fate_semantics(golden, dtype=dtype, device="cuda:0")
    vf = _fate_case(golden)
    ad = st.AnnDataLite(obsm={"align_spatial": golden["a_X"][:5]}, uns={"VecFld_morpho": vf})
    st.tdr.morphopath(ad, interpolation_num=12, t_end=40.0, dtype=dtype, device="cuda:0")
    stages, tv = st.tdr.construct_genesis_states(ad, n_steps=5, dtype=dtype, device="cuda:0")
    ref = tro.genesis_states(vf, ad.uns["fate_morpho"]["init_states"], tv)
    for a, b in zip(stages, ref):
        assert _rel(a, b) < (1e-5 if dtype == "float64" else 1e-3)
