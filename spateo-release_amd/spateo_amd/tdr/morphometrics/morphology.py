"""``spateo.tdr.morphometrics.morphology``: the kernel density of a reconstructed point cloud on the device.

``pc_KDE`` (``spateo/tdr/morphometrics/morphology.py:74-121``) is one line on ``sklearn.neighbors.KernelDensity(kernel,
bandwidth).fit(coords).score_samples(coords)``.  Here the N x N reduction is ``mvf_kde`` (``csrc/mvf_kde.hip``): the pairwise
kernel is generated in registers and reduced in log space, so a cell 40 bandwidths from its neighbours gets sklearn's -4303 and
not ``log 0``.  ``kernel_density`` is the general form (other targets, ``sample_weight``, one column per group of sources),
``pc_KDE`` the reference's signature on any object with ``.points``, ``.copy()`` and ``.point_data`` (pyvista is never imported),
``cell_density`` the same on an AnnData.

Not here, by name: d > 3; sklearn's ``atol`` / ``rtol`` (the device result is the exact sum); ``bandwidth="scott"`` /
``"silverman"``; metrics other than the Euclidean.  ``model_morphology`` of the same reference module lives in
``model_morphology.py``.
"""
from __future__ import annotations

import math

import numpy as np

from ... import _lib
from ... import _runtime as _rt

__all__ = ["kernel_density", "pc_KDE", "cell_density"]

KERNELS = tuple(_lib.KDE_KERNELS)
MAX_DIM = 3


def _log_vn(n):
    """log of the volume of the unit n-ball."""
    return 0.5 * n * math.log(math.pi) - math.lgamma(0.5 * n + 1)


def _log_sn(n):
    """log of the surface of the unit n-sphere (in n + 1 dimensions)."""
    return math.log(2 * math.pi) + _log_vn(n - 1)


def kde_log_norm(bandwidth, d, kernel):
    """sklearn's ``_log_kernel_norm(h, d, kernel)``: the log of 1 / (h^d x the integral of K over R^d), closed form for the six
    kernels (d = 1, 2, 3 is what the device kernel takes)."""
    if kernel not in KERNELS:
        raise ValueError(f"kernel must be one of {list(KERNELS)}, got {kernel!r}")
    if kernel == "gaussian":
        factor = 0.5 * d * math.log(2 * math.pi)
    elif kernel == "tophat":
        factor = _log_vn(d)
    elif kernel == "epanechnikov":
        factor = _log_vn(d) + math.log(2.0 / (d + 2.0))
    elif kernel == "exponential":
        factor = _log_sn(d - 1) + math.lgamma(d)
    elif kernel == "linear":
        factor = _log_vn(d) - math.log(d + 1.0)
    else:  # cosine: S_{d-1} x the integral of cos(pi r / 2) r^(d-1) over [0, 1], by parts
        factor, tmp = 0.0, 2.0 / math.pi
        for k in range(1, d + 1, 2):
            factor += tmp
            tmp *= -(d - k) * (d - k - 1) * (2.0 / math.pi) ** 2
        factor = math.log(factor) + _log_sn(d - 1)
    return -factor - d * math.log(bandwidth)


def _is_sparse(a):
    return hasattr(a, "tocsr") and hasattr(a, "nnz")


def _coords(a, name):
    if _is_sparse(a):
        raise NotImplementedError(f"kernel_density: `{name}` is a scipy.sparse matrix; dense coordinates with 1 <= d <= {MAX_DIM} only")
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2:
        raise ValueError(f"kernel_density: `{name}` must be an (n, d) array, got shape {a.shape}")
    if not (1 <= a.shape[1] <= MAX_DIM):
        raise NotImplementedError(f"kernel_density: `{name}` has d = {a.shape[1]}; 1 <= d <= {MAX_DIM} only")
    if not np.isfinite(a).all():
        raise ValueError(f"kernel_density: `{name}` holds non-finite values")
    return a


def _centre(points):
    """The source mean, rounded to 2^-20 of the cloud's extent.  Any common centre leaves the differences unchanged; this one
    makes `x - centre` exact for coordinates that carry no more than some 30 bits below the extent (pixel grids, float32
    data), so that the result does not depend on WHICH set of points the mean was taken of: a per-group call and the
    group's column of a grouped call see the same differences bit for bit."""
    mean = points.mean(axis=0)
    extent = float((points.max(axis=0) - points.min(axis=0)).max())
    if not (extent > 0.0 and np.isfinite(extent)):
        return mean
    q = math.ldexp(1.0, math.frexp(extent)[1] - 1 - 20)
    return np.round(mean / q) * q


def kernel_density(points, targets=None, *, kernel="gaussian", bandwidth=1.0, sample_weight=None, groups=None, dtype="float64",
                   device=None):
    """Log-density of the cloud ``points`` (N, d), d <= 3, at ``targets`` (n, d; None: at the points themselves).

    Returns host float64: (n,) without ``groups``; with a 1-D integer ``groups`` (N,) an (n, C) matrix, C = max + 1, whose
    column c equals ``KernelDensity(kernel=kernel, bandwidth=bandwidth).fit(points[groups == c], sample_weight=w[groups ==
    c]).score_samples(targets)``.  A group without sources, or whose weights are all zero, gives a column of -inf.

    kernel: "gaussian", "exponential", "tophat", "epanechnikov", "linear" or "cosine" (sklearn's definitions, the compact ones
    with its strict support dist < bandwidth).  ``dtype`` is the storage of the centred coordinates on the device only; every
    distance, exponent and sum is float64 in both modes.  The result is the exact sum (no ``atol`` / ``rtol``)."""
    if kernel not in KERNELS:
        raise ValueError(f"kernel_density: kernel must be one of {list(KERNELS)}, got {kernel!r}")
    if isinstance(bandwidth, str):
        raise NotImplementedError(f"kernel_density: bandwidth={bandwidth!r} is not supported; pass a positive number")
    h = float(bandwidth)
    if not (h > 0.0 and math.isfinite(h)):
        raise ValueError(f"kernel_density: bandwidth must be positive and finite, got {bandwidth!r}")
    if dtype not in ("float32", "float64"):
        raise ValueError(f"kernel_density: dtype must be 'float32' or 'float64', got {dtype!r}")
    X = _coords(points, "points")
    N, d = X.shape
    if N == 0:
        raise ValueError("kernel_density: `points` is empty")
    T = X if targets is None else _coords(targets, "targets")
    if T.shape[1] != d:
        raise ValueError(f"kernel_density: `targets` has d = {T.shape[1]}, `points` d = {d}")
    w = None
    if sample_weight is not None:
        w = np.asarray(sample_weight, dtype=np.float64)
        if w.shape != (N,):
            raise ValueError(f"kernel_density: sample_weight must have shape ({N},), got {w.shape}")
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("kernel_density: sample_weight must be finite and non-negative")
        if ((w > 0) & (w < np.finfo(np.float64).tiny)).any():
            raise ValueError("kernel_density: sample_weight holds subnormal numbers")
    g, C = None, 1
    if groups is not None:
        g = np.asarray(groups)
        if g.shape != (N,):
            raise ValueError(f"kernel_density: groups must have shape ({N},), got {g.shape}")
        if g.dtype == bool or not np.issubdtype(g.dtype, np.integer):
            gf = np.asarray(g, dtype=np.float64) if np.issubdtype(g.dtype, np.number) and g.dtype != bool else None
            if gf is None or not (np.isfinite(gf).all() and (gf == np.floor(gf)).all()):
                raise ValueError("kernel_density: groups must be integers")
            g = gf.astype(np.int64)
        if (g < 0).any():
            raise ValueError("kernel_density: groups must be non-negative")
        C = int(g.max()) + 1
        if C >= 2**31:
            raise ValueError("kernel_density: group ids must be below 2^31")
    with np.errstate(over="ignore"):
        if g is None:
            totals = np.array([float(N) if w is None else float(w.sum())])
        else:
            totals = np.bincount(g, weights=w, minlength=C).astype(np.float64)
    if not np.isfinite(totals).all():
        raise ValueError("kernel_density: the sum of the weights is not finite")
    if T.shape[0] == 0:
        return np.zeros((0,) if g is None else (0, C), dtype=np.float64)
    centre = _centre(X)
    k = _rt._shared_kernels(device, dtype)
    out = np.asarray(k.kde(T - centre, X - centre, kernel, h, weight=w, group=g, C=C), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = out + (kde_log_norm(h, d, kernel) - np.log(totals))[None, :]   # (-inf column + inf of an empty group: set below)
    out[:, totals == 0] = -np.inf
    return out[:, 0] if g is None else out


def pc_KDE(pc, key_added="kde", kernel="gaussian", bandwidth=1.0, colormap="hot_r", alphamap=1.0, inplace=False, dtype="float64",
           device=None):
    """Kernel density of a 3-D point cloud model: the reference's ``pc_KDE`` (``morphology.py:74-121``) with its return value
    ``(pc or None, plot_cmap)``.  ``pc``: any object with ``.points``, ``.copy()`` and a ``point_data`` mapping.  The
    log-densities are numeric labels, for which the reference's ``add_model_labels`` (``label_utils.py:98-106``) stores the
    labels under ``point_data[key_added]`` and returns the colormap as ``plot_cmap`` (``alphamap`` is not used on that branch)."""
    pc = pc.copy() if not inplace else pc
    pc_kde = kernel_density(np.asarray(pc.points), kernel=kernel, bandwidth=bandwidth, dtype=dtype, device=device)
    pc.point_data[key_added] = np.asarray(pc_kde).flatten()
    plot_cmap = colormap
    return (pc if not inplace else None), plot_cmap


def cell_density(adata, spatial_key="spatial", group_key=None, key_added="kde", **kw):
    """``kernel_density`` on an AnnData (``AnnDataLite`` or anything with ``obsm`` / ``obs`` / ``uns``) at its own cells:
    writes ``obs[key_added]``; with a categorical ``obs[group_key]`` instead ``obsm[key_added]`` (n x C, one column per
    category: the density of THAT cell type at every cell) and ``uns[key_added] = {"categories": [...], "group_key": ...}``.
    ``kw`` goes to ``kernel_density`` (kernel, bandwidth, sample_weight, dtype, device).  Returns None."""
    if spatial_key not in adata.obsm:
        raise KeyError(f"cell_density: obsm has no '{spatial_key}'")
    X = adata.obsm[spatial_key]
    for bad in ("groups", "targets"):
        if bad in kw:
            raise TypeError(f"cell_density: `{bad}` is set by group_key / the cells themselves")
    if group_key is None:
        adata.obs[key_added] = kernel_density(X, **kw)
        return None
    col = adata.obs[group_key]
    if not hasattr(col, "cat"):
        raise ValueError(f"cell_density: obs column '{group_key}' is not categorical")
    cats, codes = col.cat.categories.tolist(), np.asarray(col.cat.codes, dtype=np.int64)
    if (codes < 0).any():
        raise ValueError(f"cell_density: obs column '{group_key}' has cells without a category")
    dens = kernel_density(X, groups=codes, **kw)
    if dens.shape[1] < len(cats):  # trailing categories without a cell: columns of -inf, as for any empty group
        dens = np.hstack([dens, np.full((dens.shape[0], len(cats) - dens.shape[1]), -np.inf)])
    adata.obsm[key_added] = dens
    adata.uns[key_added] = {"categories": cats, "group_key": group_key}
    return None
