"""``kernel_interpolation`` with the reference's signature (``spateo/tdr/interpolations/interpolation_sparseVFC.py:13-85``):
the second call site of the SparseVFC engine, with ``Y`` = the selected obs / gene columns (Dy = #keys) instead of a
displacement field.  The fit runs on the GPU; wide ``Y`` is processed in 3-column groups sharing one Gram matrix.

``kernel_interpolation(..., return_model=True)`` also hands back the fitted field, and ``kernel_interpolation_predict`` reads
it at any other point set - values and, with ``gradient=True``, the spatial gradient of every key - without a refit."""
from __future__ import annotations

from typing import Optional, Union

import numpy as np

from ... import _lib
from ...logging import logger_manager as lm
from ...vectorfield import SparseVFC, _field_on_device


def _dense(a):
    return a.toarray() if hasattr(a, "toarray") else np.asarray(a)


def _interpolated_adata(target, target_points, obs_keys, var_keys, spatial_key, grads=None):
    """The AnnData (``anndata.AnnData`` when installed, else ``AnnDataLite``) of interpolated values ``target`` (n x
    (#obs keys + #genes), obs columns first).  grads: per spatial axis i an array like ``target`` = d value / d x_i, stored as
    ``layers["grad_i"]`` (genes) and ``obs[f"{key}_grad_{i}"]`` (obs keys)."""
    no = len(obs_keys)
    obs_part = target[:, :no]
    x_part = target[:, no:] if var_keys else None
    obs_cols = {k: obs_part[:, i] for i, k in enumerate(obs_keys)}
    layers = {}
    for i, g in enumerate(grads or []):
        for j, k in enumerate(obs_keys):
            obs_cols[f"{k}_grad_{i}"] = g[:, j]
        if var_keys:
            layers[f"grad_{i}"] = g[:, no:]
    try:
        import pandas as pd
        from anndata import AnnData

        out = AnnData(
            X=x_part,
            obs=pd.DataFrame(obs_cols) if obs_cols else None,
            obsm={spatial_key: np.asarray(target_points)},
            var=pd.DataFrame(index=var_keys) if var_keys else None,
            **({"layers": layers} if layers else {}),
        )
    except ImportError:
        from ..._anndata_lite import AnnDataLite

        out = AnnDataLite(X=x_part, var_names=var_keys, obs=obs_cols, obsm={spatial_key: np.asarray(target_points)},
                          n_obs=len(target), layers=layers)
    return out


def kernel_interpolation(
    source_adata,
    target_points: Optional[np.ndarray] = None,
    keys: Union[str, list] = None,
    spatial_key: str = "spatial",
    layer: str = "X",
    lambda_: float = 0.02,
    lstsq_method: str = "scipy",
    return_model: bool = False,
    **kwargs,
):
    """Learn a continuous mapping from space to the ``keys`` (obs columns first, then genes) with SparseVFC and
    evaluate it at ``target_points``.  Returns an AnnData (``anndata.AnnData`` when installed, else ``AnnDataLite``)
    with ``obs[obs_keys]``, ``X`` / ``var_names`` = the interpolated genes and ``obsm[spatial_key] = target_points``.
    ``return_model=True`` (not in the reference) returns ``(adata, model)``: ``model`` is the ``SparseVFC`` dict plus
    ``obs_keys``, ``var_keys`` and ``spatial_key``, what ``kernel_interpolation_predict`` takes."""
    assert keys is not None, "`keys` cannot be None."
    keys = [keys] if isinstance(keys, str) else list(keys)
    Xmat = source_adata.X if layer == "X" else source_adata.layers[layer]
    spatial = np.asarray(source_adata.obsm[spatial_key], dtype=float)
    var_names = [str(v) for v in list(source_adata.var_names)]
    obs_keys = [k for k in keys if k in source_adata.obs.keys()]
    var_keys = [k for k in keys if k in var_names]
    cols = []
    if obs_keys:
        cols.append(np.column_stack([np.asarray(source_adata.obs[k], dtype=float) for k in obs_keys]))
    if var_keys:
        idx = [var_names.index(k) for k in var_keys]
        cols.append(_dense(Xmat[:, idx]).astype(float))
    if not cols:
        raise ValueError(f"none of the keys {keys} is an obs column or a gene of source_adata")
    info_data = np.concatenate(cols, axis=1)

    res = SparseVFC(spatial, info_data, target_points, lambda_=lambda_, lstsq_method=lstsq_method, **kwargs)
    target = res["grid_V"]
    lm.main_info("Creating an adata object with the interpolated expression...")
    out = _interpolated_adata(target, target_points, obs_keys, var_keys, spatial_key)
    lm.main_finish_progress(progress_name="KernelInterpolation")
    if return_model:
        return out, {**res, "obs_keys": list(obs_keys), "var_keys": list(var_keys), "spatial_key": spatial_key}
    return out


def kernel_interpolation_predict(model, target_points, gradient: bool = False, dtype=None, device=None):
    """Evaluate the field of ``kernel_interpolation(..., return_model=True)`` at ``target_points`` (n x d) without a refit: one
    more pass of ``con_K @ C``, as the reference would pay.  Returns the AnnData ``kernel_interpolation`` builds for its own
    targets.  ``gradient=True`` adds the spatial gradient of every key: ``layers["grad_0"] .. layers[f"grad_{d-1}"]`` (n x
    genes each, d gene / d x_i) and ``obs[f"{key}_grad_{i}"]`` for the obs keys."""
    for key in ("X_ctrl", "C", "beta", "obs_keys", "var_keys", "spatial_key"):
        if key not in model:
            raise ValueError(f"not a kernel_interpolation model: {key!r} is missing (fit with return_model=True)")
    pts = np.asarray(target_points, dtype=np.float64)
    if pts.ndim != 2:
        raise ValueError(f"target_points must be an (n, d) array, got shape {pts.shape}")
    obs_keys, var_keys = list(model["obs_keys"]), list(model["var_keys"])
    dy = np.asarray(model["C"]).shape[1]
    d = np.asarray(model["X_ctrl"]).shape[1]
    if dy != len(obs_keys) + len(var_keys):
        raise ValueError(f"the model's coefficients have {dy} columns for {len(obs_keys)} obs keys + {len(var_keys)} genes")
    flags = _lib.EVAL_V | (_lib.EVAL_JAC if gradient else 0)
    o = _field_on_device(pts, model, flags, dtype, device)
    target = np.ascontiguousarray(o[_lib.EVAL_V][:, :dy])
    grads = None
    if gradient:
        J = o[_lib.EVAL_JAC][:dy, :d, :]  # (dy, d, n)
        grads = [np.ascontiguousarray(J[:, i, :].T) for i in range(d)]
    return _interpolated_adata(target, target_points, obs_keys, var_keys, model["spatial_key"], grads)
