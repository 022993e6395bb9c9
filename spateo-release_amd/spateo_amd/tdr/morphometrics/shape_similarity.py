"""``spateo.tdr.morphometrics.shape_similarity``: the shape similarity of two point cloud models (Hu Xiaotong, Wang Jiandong:
similarity analysis of three-dimensional point clouds based on the eigenvector of subspaces) with the per-subspace work on
the device.

The reference (``spateo/tdr/morphometrics/shape_similarity.py``) visits each of the ``n_subspace^3`` voxels in a Python loop,
masks the whole cloud six times per voxel and runs one ``scipy.linalg.lstsq`` per voxel.  Here ``mvf_shape_descriptors``
(``csrc/mvf_shape.hip``) bins the points once, groups them by voxel and fits every kept voxel in a workgroup of its own;
``subspace_descriptors`` is that call, ``model_eigenvector`` / ``calculate_eigenvector`` / ``pairwise_shape_similarity`` have the
reference's signatures and return values, and ``shape_similarity_matrix`` computes each model's eigenvector once.

The reference's quirks are kept, because they decide the numbers: the cuboid is ``ceil(ptp)`` long, so a point on an upper
face belongs to no voxel whenever ``ceil(ptp) == ptp`` (integer pixel coordinates); a voxel counts only with more than one
point; the surface is fitted in RAW monomials by the minimum-norm solution with the cut-off ``eps sigma_max``; a cosine of
exactly 1 falls into no bin.  One deviation: a point that two intervals of one axis hold (an ulp-wide overlap of ``hi[j]`` and
``lo[j + 1]``) is put into the lower one and counted in ``n_overlap``, where the reference would count it twice.

Everything is float64 and there is no ``dtype`` argument: at realistic coordinates (hundreds of units away from the origin)
the cubic's singular values reach down to ``eps sigma_max`` in most voxels, the rank decision is marginal, and float32 storage
of the coordinates would decide it.  In that regime the reference itself moves by 1e-5 relative when LAPACK's driver is
swapped (gelsd for gelss); results agree with it to that, not to rounding.
"""
from __future__ import annotations

import math

import numpy as np
from numpy.linalg import norm

from ... import _lib
from ... import _runtime as _rt

__all__ = ["subspace_descriptors", "calculate_eigenvector", "model_eigenvector", "pairwise_shape_similarity",
           "shape_similarity_matrix"]

ORDERS = tuple(_lib.SHAPE_ORDERS)


def _cloud(pcs, who):
    pcs = np.asarray(pcs, dtype=np.float64)
    if pcs.ndim != 2 or pcs.shape[1] != 3 or pcs.shape[0] < 1:
        raise ValueError(f"{who}: a point cloud is an (n >= 1, 3) array, got shape {pcs.shape}")
    if not np.isfinite(pcs).all():
        raise ValueError(f"{who}: the point cloud holds non-finite values")
    return np.ascontiguousarray(pcs)


def _n_subspace(n_subspace, who):
    n = int(n_subspace)
    if n != n_subspace or n < 1:
        raise ValueError(f"{who}: n_subspace must be a positive integer, got {n_subspace!r}")
    if n > _lib.SHAPE_MAX_NSUB:
        raise NotImplementedError(f"{who}: n_subspace = {n} is not supported; at most {_lib.SHAPE_MAX_NSUB} voxels per axis")
    return n


def voxel_tables(pcs, n):
    """The interval ends of ``rough_subspace`` (shape_similarity.py:19-44) per axis, ``lo[a, j] = min + j * size`` and
    ``hi[a, j] = lo[a, j] + size`` with ``size = ceil(ptp) / n``, in the reference's own float64 operations: (3, n) each."""
    start = np.min(pcs, axis=0)
    ptp = np.ptp(pcs, axis=0)
    lo, hi = np.empty((3, n)), np.empty((3, n))
    j = np.arange(n)
    for a in range(3):
        size = math.ceil(ptp[a]) / n
        lo[a] = start[a] + j * size
        hi[a] = lo[a] + size
    return lo, hi


def _queue(k, pcs, n, order):
    lo, hi = voxel_tables(pcs, n)
    return k.shape_queue(pcs, lo, hi, _lib.SHAPE_ORDERS[order], np.mean(pcs, axis=0))


def _checked(desc, n, who):
    if len(desc["voxel"]) == 0:
        raise ValueError(f"{who}: no subspace of the {n}^3 holds more than one point ({desc['n_dropped']} of "
                         f"{len(desc['point_voxel'])} points lie in no subspace), so there is nothing to fit; use a smaller n_subspace")
    return desc


def subspace_descriptors(pcs, n_subspace=20, order="cubic", device=None):
    """The descriptors of every subspace that holds more than one point, in the reference's voxel order
    (``layer n^2 + line n + piece``; piece x, line y, layer z): a dict with ``voxel`` (ids), ``count``, ``cosine``, ``dist``
    and ``rank`` per kept subspace, ``point_voxel`` (the voxel of every point, -1 for a point in none), ``n_dropped`` (their
    number) and ``n_overlap`` (points two intervals of one axis hold; they go to the lower one).  ``sigma_max`` and
    ``sigma_min_ratio`` (the smallest kept singular value over the largest) describe the fit.  ``order``: "linear",
    "quadratic" or "cubic", the surfaces of ``subspace_surface_fitting``; ``model_eigenvector`` always uses "cubic".
    float64 throughout (see the module's docstring)."""
    if order not in ORDERS:
        raise ValueError("``order`` value is wrong.")
    n = _n_subspace(n_subspace, "subspace_descriptors")
    pcs = _cloud(pcs, "subspace_descriptors")
    k = _rt._shared_kernels(device, "float64")
    return _checked(k.shape_read([_queue(k, pcs, n, order)])[0], n, "subspace_descriptors")


def calculate_eigenvector(vetorspaces, m=10, s=5):
    """The subspace eigenvector of ``calculate_eigenvector`` (shape_similarity.py:136-161), on the host: m bins on the cosine,
    ``[(i - 1) / m, i / m)``, each split into s bins on the distance against fractions of the bin's ``ptp``; the entry is
    ``mean(dist) / max(dist)``, the weight the number of subspaces.  Returns (eigenvector, weight vector / its sum)."""
    vetorspaces = np.asarray(vetorspaces)
    eigenvector, weightvector = [], []
    for i in range(1, m + 1):
        w_i1, w_i2 = (i - 1) / m, i / m
        i_vetorspaces = vetorspaces[vetorspaces[:, 0] >= w_i1, :]
        i_vetorspaces = i_vetorspaces[i_vetorspaces[:, 0] < w_i2, :]
        if i_vetorspaces.shape[0] == 0:
            eigenvector.extend([0] * s)
            weightvector.extend([0] * s)
            continue
        max_dist_i, ptp_dist_i = np.max(i_vetorspaces[:, 1]), np.ptp(i_vetorspaces[:, 1])
        for j in range(1, s + 1):
            w_ptp_i1, w_ptp_i2 = ptp_dist_i * (j - 1) / s, ptp_dist_i * j / s
            j_vetorspaces = i_vetorspaces[i_vetorspaces[:, 1] >= w_ptp_i1, :]
            j_vetorspaces = j_vetorspaces[j_vetorspaces[:, 1] < w_ptp_i2, :]
            if j_vetorspaces.shape[0] == 0:
                dist_rat_j, segma_i = 0, 0
            else:
                segma_i = j_vetorspaces.shape[0]
                dist_rat_j = np.mean(j_vetorspaces[:, 1]) / max_dist_i
            eigenvector.append(dist_rat_j)
            weightvector.append(segma_i)
    return np.asarray(eigenvector), np.asarray(weightvector) / np.sum(weightvector)


def _eigenvector(desc, m, s):
    return calculate_eigenvector(np.c_[desc["cosine"], desc["dist"]], m=m, s=s)


def model_eigenvector(model_pcs, n_subspace=20, m=10, s=5, device=None):
    """The subspace eigenvector of a 3-D point cloud model (shape_similarity.py:164-177): (eigenvector, weight vector), m s
    entries each."""
    desc = subspace_descriptors(model_pcs, n_subspace=n_subspace, order="cubic", device=device)
    return _eigenvector(desc, m, s)


def _score(e1, w1, e2, w2):
    """shape_similarity.py:199-201."""
    w = np.max(np.c_[w1, w2], axis=1)
    similarity_score = np.sum(w * e1 * e2) / (norm((np.sqrt(w) * e1)) * norm((np.sqrt(w) * e2)))
    return round(float(similarity_score), 4)


def pairwise_shape_similarity(model1_pcs, model2_pcs, n_subspace=20, m=10, s=5, device=None):
    """The shape similarity score of two 3-D point cloud models (shape_similarity.py:180-201): a Python float rounded to 4
    decimals, 1 for equal shapes."""
    return float(shape_similarity_matrix([model1_pcs, model2_pcs], n_subspace=n_subspace, m=m, s=s, device=device)[0, 1])


def shape_similarity_matrix(models, n_subspace=20, m=10, s=5, device=None):
    """The symmetric k x k matrix of ``pairwise_shape_similarity`` over k models.  Each model's eigenvector is computed once
    (the pairwise call computes it once per pair): the descriptor calls are queued on one stream and read back together.
    Entry (i, j), i < j, is ``pairwise_shape_similarity(models[i], models[j])`` bit for bit, and (j, i) is its copy."""
    n = _n_subspace(n_subspace, "shape_similarity_matrix")
    clouds = [_cloud(pcs, "shape_similarity_matrix") for pcs in models]
    if not clouds:
        return np.zeros((0, 0))
    k = _rt._shared_kernels(device, "float64")
    descs = k.shape_read([_queue(k, pcs, n, "cubic") for pcs in clouds])
    vectors = [_eigenvector(_checked(d, n, f"shape_similarity_matrix (model {i})"), m, s) for i, d in enumerate(descs)]
    out = np.empty((len(clouds), len(clouds)))
    for i, (e1, w1) in enumerate(vectors):
        for j in range(i, len(clouds)):
            out[i, j] = out[j, i] = _score(e1, w1, *vectors[j])
    return out
