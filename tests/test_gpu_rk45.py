"""GPU tests of the opt-in RK45 integrator (``mvf_integrate_rk45``; ``integrate_field(..., integrator="rk45")``): SciPy's
own ``solve_ivp(method="RK45")`` on the float64 oracle field is the yardstick, step count for step count."""
import os
import sys

import numpy as np
import pytest
from scipy.integrate import solve_ivp

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def st():
    import torch

    import spateo_amd

    assert torch.cuda.is_available()
    return spateo_amd


def _vf(golden):
    g = golden
    vf = {k: g[f"a_vf_{k}"] for k in ["X_ctrl", "C", "V"]}
    vf.update(X=g["a_X"], beta=float(g["a_vf_beta"]), method="sparsevfc")
    return vf


def _scipy(field, p, t_bound, max_step):
    """solve_ivp as dynamo fate runs it, with the event fate_arclength defines (restated: it is local there)."""
    f = lambda t, y: np.asarray(field(y)).reshape(-1)  # noqa: E731
    ev = lambda t, y: float(np.all(np.abs(f(t, y)) < 1e-5)) - 1 + 1e-12  # noqa: E731
    ev.terminal = True
    return solve_ivp(f, (0.0, t_bound), p, method="RK45", max_step=max_step, dense_output=True, events=ev)


def _kernel_run(golden, starts, t_bound, n_out, max_step, dtype="float64", sampling=None, world=None, vf=None):
    from spateo_amd import _lib
    from spateo_amd._kernels import HipKernels
    import torch

    vf = vf or _vf(golden)
    k = HipKernels("cuda:0", dtype)
    ctrl = np.asarray(vf["X_ctrl"], dtype=float)
    d = ctrl.shape[1]
    center = ctrl.mean(0)
    C3 = np.zeros((len(ctrl), 3))
    C3[:, :d] = vf["C"]
    c4, x4 = k.to_x4(ctrl, center), k.to_x4(starts, center)
    Cd = torch.from_numpy(C3).to("cuda:0")
    world = world or (np.ones(3), np.concatenate([center, np.zeros(3 - d)]))
    return k.integrate_rk45(x4, c4, vf["beta"], Cd, d, world, t_bound, 1e-3, 1e-6, max_step, 100_000,
                            _lib.RK45_UNIFORM_TIME if sampling is None else sampling, n_out)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_kernel_steps_as_scipy(golden, sign):
    """uniform_time samples of the kernel == SciPy's dense output, the same accepted steps and the same statuses."""
    from oracle import sparsevfc_oracle as svo

    vf = _vf(golden)
    X = golden["a_X"]
    c = X.mean(0)
    starts = np.concatenate([X[:48], c + (X[48:64] - c) * 2.0])  # data points and points on the field's fringe
    t_end, n_out = 1000.0, 101
    max_step = t_end / 250
    t, traj, stats = _kernel_run(golden, starts, sign * t_end, n_out, max_step)
    tq = sign * np.linspace(0, t_end, n_out)
    np.testing.assert_array_equal(t, np.broadcast_to(tq, t.shape))
    extent = np.ptp(X, axis=0).max()
    fired = 0
    for i, p in enumerate(starts):
        sol = _scipy(lambda y: svo.vector_field_function(y, vf), p, sign * t_end, max_step)
        assert stats[i, 0] == len(sol.t) - 1, (i, stats[i], len(sol.t))
        assert stats[i, 3] == sol.status, (i, stats[i], sol.status)
        inside = sign * (tq - sol.t[-1]) <= 0
        np.testing.assert_allclose(traj[i, inside], sol.sol(tq[inside]).T, rtol=0, atol=1e-9 * extent)
        if sol.status == 1:
            fired += 1
            np.testing.assert_allclose(traj[i, ~inside], np.broadcast_to(sol.y[:, -1], traj[i, ~inside].shape),
                                       rtol=0, atol=1e-9 * extent)
    if sign < 0:
        assert fired >= len(starts) // 4, fired


def _check_vs_fate(t_got, x_got, T, Y, t_end, n_out, direction, extent, ttol, xtol):
    for i in range(len(T)):
        x, t = x_got[i], t_got[i]
        assert x.shape == (n_out, Y[i].shape[1]) and t.shape == (n_out,)
        assert np.all(np.diff(t) * (-1 if direction == "backward" else 1) >= 0)
        # equally spaced in arc length along the polyline of step points: the chords between samples are the oracle's
        chords = lambda z: np.linalg.norm(np.diff(z, axis=0), axis=1)  # noqa: E731
        assert np.abs(chords(x) - chords(Y[i])).max() / extent < 2 * xtol
        assert np.abs(t - T[i]).max() / t_end < ttol, (i, np.abs(t - T[i]).max())
        assert np.abs(x - Y[i]).max() / extent < xtol, (i, np.abs(x - Y[i]).max())


@pytest.mark.parametrize("dtype,tol,t_end", [("float64", 1e-8, 60.0), ("float64", 1e-8, 1000.0),
                                              ("float32", 2e-3, 60.0)])
def test_morphopath_rk45_vs_fate(st, golden, dtype, tol, t_end):
    """morphopath(integrator="rk45") against the restated dynamo fate (arc-length sampling on SciPy's RK45)."""
    from oracle import sparsevfc_oracle as svo
    from oracle import trajectory_oracle as tro

    vf = _vf(golden)
    vf.update(X=golden["a_X"][:12], V=vf["V"][:12])
    extent = np.ptp(golden["a_X"], axis=0).max()
    for n_t in (30, 250):
        for direction in ("forward", "backward", "both"):
            ad = st.AnnDataLite(obsm={"align_spatial": vf["X"]}, uns={"VecFld_morpho": vf})
            st.tdr.morphopath(ad, interpolation_num=n_t, t_end=t_end, direction=direction, integrator="rk45",
                              dtype=dtype, device="cuda:0")
            fate = ad.uns["fate_morpho"]
            T, Y = tro.fate_arclength(lambda x: svo.vector_field_function(x, vf), vf["X"], t_end, n_t, direction)
            n_out = 2 * n_t if direction == "both" else n_t
            _check_vs_fate(fate["t"], fate["prediction"], T, Y, t_end, n_out, direction, extent, tol, tol)


def test_gp_field_world_coordinates(st, golden):
    """The GP field (per-axis norm_dict, rigid part): step control must run in world coordinates to match SciPy."""
    from _gp_case import gp_dict
    from oracle import sparsevfc_oracle as svo
    from oracle import trajectory_oracle as tro

    g = golden
    gd = gp_dict(g)
    nd = gd["norm_dict"]
    nd["scale_transformed"] = nd["scale_transformed"] * np.array([1.0, 1.3, 0.8])  # per axis
    gd.update(X=g["gpw_X"][:8], V=g["gpw_full_V"][:8], method="gaussian_process")

    def gp_field(x):
        xn = (np.atleast_2d(x) - nd["mean_transformed"]) / nd["scale_transformed"]
        vel = svo.con_K(xn, gd["inducing_variables"], gd["beta"]).reshape(len(xn), -1) @ gd["Coff"]
        q = (vel + xn @ gd["R"].T + gd["t"]) * nd["scale_fixed"] + nd["mean_fixed"]
        return (q - np.atleast_2d(x)) / 10000

    extent = np.ptp(g["gpw_X"], axis=0).max()
    for direction in ("forward", "both"):
        ad = st.AnnDataLite(obsm={"align_spatial": gd["X"]}, uns={"VecFld_morpho": gd})
        st.tdr.morphopath(ad, interpolation_num=40, t_end=2000.0, direction=direction, integrator="rk45",
                          dtype="float64", device="cuda:0")
        fate = ad.uns["fate_morpho"]
        T, Y = tro.fate_arclength(gp_field, gd["X"], 2000.0, 40, direction)
        n_out = 80 if direction == "both" else 40
        _check_vs_fate(fate["t"], fate["prediction"], T, Y, 2000.0, n_out, direction, extent, 1e-8, 1e-8)


def test_two_dimensional_field(st):
    """A 2-D field: the error norm is the RMS over 2 components (dividing by 3 changes the step sequence)."""
    from oracle import sparsevfc_oracle as svo
    from oracle import trajectory_oracle as tro
    from spateo_amd.vectorfield import integrate_field

    rng = np.random.default_rng(11)
    vf = dict(X_ctrl=rng.uniform(-20, 20, (25, 2)), C=rng.standard_normal((25, 2)), beta=0.01, method="sparsevfc")
    P = rng.uniform(-20, 20, (10, 2))
    for direction in ("forward", "backward"):
        t, x = integrate_field(vf, P, t_end=500.0, interpolation_num=120, direction=direction, integrator="rk45",
                               dtype="float64", device="cuda:0")
        T, Y = tro.fate_arclength(lambda y: svo.vector_field_function(y, vf), P, 500.0, 120, direction)
        _check_vs_fate(t, x, T, Y, 500.0, 120, direction, 40.0, 1e-8, 1e-8)


def test_chunked_control_points_mixed_blocks(st):
    """M = 3000 float64 control points exceed one LDS stage: the step loop and the event bisection must stay
    block-uniform while event-terminated and full-length trajectories share blocks."""
    from oracle import sparsevfc_oracle as svo
    from spateo_amd.vectorfield import integrate_field

    rng = np.random.default_rng(7)
    M = 3000
    Xc = rng.standard_normal((M, 3))
    Xc = Xc / np.linalg.norm(Xc, axis=1, keepdims=True) * 25 * rng.uniform(0, 1, (M, 1)) ** (1 / 3)
    Cc = 0.01 * Xc / np.linalg.norm(Xc, axis=1, keepdims=True) + 0.01 * rng.standard_normal((M, 3))
    vf = dict(X_ctrl=Xc, C=Cc, beta=0.02, method="sparsevfc")
    u = rng.standard_normal((300, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    P = u * np.where(np.arange(300) % 2 == 0, 15.0, 80.0)[:, None]  # inside (escapes, fires) / far out (at rest)
    t_end, n_t = 300.0, 50
    t, x = integrate_field(vf, P, t_end=t_end, interpolation_num=n_t, direction="backward", integrator="rk45",
                           sampling="uniform_time", dtype="float64", device="cuda:0")
    tq = -np.linspace(0, t_end, n_t)
    fired = 0
    for i in rng.choice(300, 16, replace=False):
        sol = _scipy(lambda y: svo.vector_field_function(y, vf), P[i], -t_end, t_end / n_t)
        fired += sol.status == 1
        inside = tq >= sol.t[-1]
        np.testing.assert_allclose(x[i][inside], sol.sol(tq[inside]).T, rtol=0, atol=1e-8 * 80)
    assert 0 < fired < 16


def test_status_nonfinite_row_and_step_cap(st, golden):
    """A non-finite start gives status -3 and a NaN path without touching its neighbours; a tiny max_steps raises."""
    from spateo_amd import _lib
    from spateo_amd.vectorfield import integrate_field

    vf = _vf(golden)
    P = golden["a_X"][:9].copy()
    Pn = P.copy()
    Pn[4, 1] = np.nan
    t_ok, x_ok, s_ok = _kernel_run(golden, P, 60.0, 30, 60.0 / 30, sampling=_lib.RK45_ARC_LENGTH)
    t_bad, x_bad, s_bad = _kernel_run(golden, Pn, 60.0, 30, 60.0 / 30, sampling=_lib.RK45_ARC_LENGTH)
    assert s_bad[4, 3] == -3 and np.isnan(x_bad[4]).all() and np.isnan(t_bad[4]).all()
    keep = np.arange(9) != 4
    np.testing.assert_array_equal(x_bad[keep], x_ok[keep])
    np.testing.assert_array_equal(t_bad[keep], t_ok[keep])
    np.testing.assert_array_equal(s_bad[keep], s_ok[keep])
    assert (s_ok[:, 3] == 0).all()
    with pytest.raises(_lib.MVFError, match="max_steps"):
        integrate_field(vf, P, t_end=60.0, interpolation_num=30, integrator="rk45", max_steps=5, dtype="float64",
                        device="cuda:0")


def test_default_integrator_unchanged(st, golden):
    """integrator="rk4" is the default: the same outputs, bit for bit, as a call without the argument."""
    from spateo_amd.vectorfield import integrate_field

    vf = _vf(golden)
    for sampling in ("arc_length", "uniform_time"):
        a = integrate_field(vf, golden["a_X"][:10], t_end=60.0, interpolation_num=30, sampling=sampling,
                            dtype="float64", device="cuda:0")
        b = integrate_field(vf, golden["a_X"][:10], t_end=60.0, interpolation_num=30, sampling=sampling,
                            integrator="rk4", dtype="float64", device="cuda:0")
        for u, v in zip(a[0] + a[1], b[0] + b[1]):
            np.testing.assert_array_equal(u, v)
