"""Generate ``tests/golden/ref_highd.npz`` by EXECUTING the real reference code in 4, 5 and 8 dimensions.

Run in the build container only (``/root/reference`` does not exist on the GPU box):

    python tests/golden/make_golden_highd.py

Same loading and stubs as ``make_golden.py`` (the reference modules by file path; ``anndata`` and ``dynamo`` stubbed with
this repo's float64 oracle).  Executed at D = 4, 5, 8:

* ``gaussian_process.py``  -> ``_con_K`` (cdist path and ``return_d``)
* ``GPVectorField.py``     -> ``Jacobian_GP_gaussian_kernel`` (identity ``norm_dict``, looped and vectorised, a 1-D query),
  ``compute_acceleration``, ``compute_curvature`` (formulas 1 and 2), ``compute_divergence``, and the exceptions of
  ``compute_torsion`` / ``compute_curl``
* ``sparsevfc.py`` / ``differential_geometry.py`` -> ``_morphofield_sparsevfc(NX=...)`` and
  ``morphofield_{velocity,jacobian,divergence,acceleration,curvature}`` on a 5-D AnnData
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import load_reference  # noqa: E402  (also puts the repository root on sys.path)
from spateo_amd._anndata_lite import AnnDataLite  # noqa: E402

DIMS = (4, 5, 8)


def synth_field_d(rng, n, d):
    """A smooth d-dimensional displacement field: rotation in the (0, 1) and (2, 3) planes, radial growth, noise, 5 %
    gross outliers."""
    X = rng.uniform(-1.0, 1.0, size=(n, d)) * np.linspace(30.0, 12.0, d)
    A = 0.02 * np.eye(d)
    A[0, 1], A[1, 0] = -0.05, 0.05
    A[2, 3], A[3, 2] = -0.03, 0.03
    V = X @ A.T + 0.3 * np.sin(X / 7.0) + 0.05 * rng.standard_normal((n, d))
    out = rng.choice(n, size=max(1, n // 20), replace=False)
    V[out] = 3.0 * rng.standard_normal((len(out), d))
    return X, V


def _exception(fn):
    try:
        fn()
    except Exception as exc:  # noqa: BLE001 - the TYPE is what is pinned
        return type(exc).__name__
    return ""


def main():
    iu, gp, gvf, svfc, dg = load_reference()
    rng = np.random.default_rng(20261016)
    out = {}
    for d in DIMS:
        # ---- con_K (gaussian_process.py:16-36) ----
        x = rng.standard_normal((7, d)) * 3.0
        y = rng.standard_normal((5, d)) * 3.0
        beta = 0.041
        out[f"d{d}_conk_x"], out[f"d{d}_conk_y"] = x, y
        out[f"d{d}_conk_K"] = gp._con_K(x, y, beta)
        Kd, Dd = gp._con_K(x, y, beta, return_d=True)
        out[f"d{d}_conk_K_diff"], out[f"d{d}_conk_D"] = Kd, Dd

        # ---- Jacobian + evaluators with an identity norm_dict == dynamo's sparsevfc formulas ----
        M, n = 11, 13
        Xc = rng.standard_normal((M, d)) * 4.0
        C = rng.standard_normal((M, d)) * 0.7
        Xq = rng.standard_normal((n, d)) * 4.0
        beta_j = 0.023
        ident = {"scale_fixed": 1.0, "scale_transformed": 1.0, "mean_transformed": np.zeros(d), "mean_fixed": np.zeros(d)}
        vfd = {"norm_dict": ident, "kernel_type": "euc", "inducing_variables": Xc, "beta": beta_j, "Coff": C}
        out.update({f"d{d}_Xc": Xc, f"d{d}_C": C, f"d{d}_Xq": Xq})
        out[f"d{d}_J_loop"] = gvf.Jacobian_GP_gaussian_kernel(Xq, vfd, vectorize=False)
        out[f"d{d}_J_vec"] = gvf.Jacobian_GP_gaussian_kernel(Xq, vfd, vectorize=True)
        out[f"d{d}_J_1d"] = gvf.Jacobian_GP_gaussian_kernel(Xq[3], vfd)
        vf = lambda xx, Xc=Xc, C=C: gp._con_K(xx, Xc, beta_j) @ C  # noqa: E731  == vector_field_function
        fj = lambda xx, vfd=vfd: gvf.Jacobian_GP_gaussian_kernel(xx, vfd)  # noqa: E731
        out[f"d{d}_v"] = vf(Xq)
        out[f"d{d}_acc"], out[f"d{d}_acc_mat"] = gvf.compute_acceleration(vf, fj, Xq)
        out[f"d{d}_curv2"], out[f"d{d}_curv2_mat"] = gvf.compute_curvature(vf, fj, Xq, formula=2)
        out[f"d{d}_curv1"], _ = gvf.compute_curvature(vf, fj, Xq, formula=1)
        out[f"d{d}_div"] = gvf.compute_divergence(fj, Xq, vectorize_size=4)
        out[f"d{d}_curl_exc"] = _exception(lambda: gvf.compute_curl(fj, Xq))
        out[f"d{d}_torsion_exc"] = _exception(lambda: gvf.compute_torsion(vf, fj, Xq))
    out["beta_conk"], out["beta_dg"] = 0.041, 0.023

    # ---- the reference wrappers on a 5-D AnnData, the oracle engine injected ----
    Xa, Va = synth_field_d(rng, 160, 5)
    NX = Xa[:7] + 0.5
    ad = AnnDataLite(obsm={"align_spatial": Xa, "V_mapping": Va})
    svfc.morphofield_sparsevfc(ad, NX=NX, M=20, MaxIter=20, restart_num=1, restart_seed=[0])
    out.update(a5_X=Xa, a5_V=Va, a5_NX=NX)
    for k in ["X_ctrl", "ctrl_idx", "C", "beta", "V", "P", "sigma2", "grid", "grid_V", "iteration"]:
        out[f"a5_vf_{k}"] = np.asarray(ad.uns["VecFld_morpho"][k])
    dg.morphofield_velocity(ad)
    dg.morphofield_acceleration(ad)
    dg.morphofield_curvature(ad)
    dg.morphofield_divergence(ad)
    dg.morphofield_jacobian(ad)
    out["a5_velocity"] = ad.obsm["velocity"]
    out["a5_acceleration_obs"], out["a5_acceleration_obsm"] = ad.obs["acceleration"], ad.obsm["acceleration"]
    out["a5_curvature_obs"], out["a5_curvature_obsm"] = ad.obs["curvature"], ad.obsm["curvature"]
    out["a5_divergence_obs"] = ad.obs["divergence"]
    out["a5_jacobian_obs"], out["a5_jacobian_uns"] = ad.obs["jacobian"], ad.uns["jacobian"]
    out["a5_curl_exc"] = _exception(lambda: dg.morphofield_curl(ad))
    out["a5_torsion_exc"] = _exception(lambda: dg.morphofield_torsion(ad))

    path = os.path.join(HERE, "ref_highd.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)/1024:.1f} KiB")


if __name__ == "__main__":
    main()
