"""The reference-model route of ``spateo.alignment`` for large slices: align a down-sampled copy of every slice, then carry the
transformation to the full-resolution slices - ``downsampling`` (``spateo/alignment/utils.py:25-47``), ``morpho_align_ref``,
``morpho_align_transformation``, ``morpho_align_apply_transformation`` (``morpho_alignment.py:114-454``),
``solve_RT_by_correspondence`` (``utils.py:350-402``) - and the samplers under it (``alignment/methods/sampling.py``): ``sample``,
``trn``, ``sample_by_kmeans``.

The samplers' hot loops run on the device in float64 (``mvf_trn``, ``mvf_kmeans``, ``mvf_nearest_rows``; csrc/mvf_sample.hip);
every random draw is made on the host from the generator the reference draws from, and NumPy's GLOBAL generator is left in the
state the reference leaves it in (the way ``preprocess.sample_by_velocity`` treats it).  ``align.py`` re-exports the names.
"""
from __future__ import annotations

import warnings

import numpy as np

from . import _lib
from . import _runtime as _rt
from .preprocess import _RNG_LOCK, sample_by_velocity

__all__ = ["trn", "sample_by_kmeans", "sample", "downsampling", "solve_RT_by_correspondence", "morpho_align_transformation",
           "morpho_align_apply_transformation", "morpho_align_ref"]

TRN_DEFAULTS = dict(tmax=200, li=0.2, lf=0.01, ei=0.3, ef=0.05, c=0)  # TRNET.run's (sampling.py:133-135)


def _coords(X, who):
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or not (1 <= X.shape[1] <= 3) or X.shape[0] < 1:
        raise ValueError(f"{who}: X must be (N >= 1, 1 <= d <= 3), got shape {X.shape}")
    if not np.isfinite(X).all():
        raise ValueError(f"{who}: non-finite coordinates")
    return X


def _count(n, who):
    if isinstance(n, (bool, np.bool_)) or int(n) != n or n < 0:
        raise ValueError(f"{who}: n must be a non-negative integer, got {n!r}")
    return int(n)


def _leave_global_rng(rs):
    with _RNG_LOCK:
        np.random.set_state(rs.get_state())


def trn_schedule(n, tmax=200, li=0.2, lf=0.01, ei=0.3, ef=0.05, c=0):
    """``(T, l, ep, kc)`` of ``TRNET.run`` (sampling.py:146-153) for n nodes: ``T = int(tmax n)`` steps and per step the scalar
    expressions of the reference, evaluated one by one as it evaluates them (NumPy's array ``power`` may round differently
    from its scalar one); ``kc = -l log(c / ep)`` (:128), None when ``c == 0``."""
    T = int(tmax * n)
    li = li * n
    l, ep = np.empty(T), np.empty(T)
    for t in range(1, T + 1):
        tt = t / T
        l[t - 1] = li * np.power(lf / li, tt)
        ep[t - 1] = ei * np.power(ef / ei, tt)
    kc = None
    if c != 0:
        kc = np.array([-lt * np.log(c / et) for lt, et in zip(l.tolist(), ep.tolist())], dtype=np.float64).reshape(T)
    return T, l, ep, kc


def trn(X, n, return_index=True, seed=19491001, device=None, **kwargs):
    """``trn`` of ``spateo/alignment/methods/sampling.py:196-222``: n nodes of a topology-representing network on the cells
    ``X`` (N, d <= 3), every step of ``TRNET.run`` on the device (``mvf_trn``, float64).

    ``kwargs``: ``tmax, li, lf, ei, ef, c`` of ``TRNET.run``.  The start draw and the sample draw are the reference's -
    ``np.random.seed(seed); np.random.randint(0, N, n)`` and the same again for ``int(tmax n)`` samples -, made on the host, and
    the global generator is left where the reference leaves it.  ``return_index=False`` returns the nodes ``W`` (n, d);
    ``True`` the nearest cell of every node: the exact nearest one, the smallest index among equally near ones (dynamo's
    ``k_nearest_neighbors`` may answer approximately for large N); duplicates are kept.

    A list of ``X`` (``n`` one number or one per slice) runs as ONE launch, one workgroup per slice, and returns a list.
    Deviation: when the start draw holds a cell twice, two nodes start identical and the reference's unstable ``argsort``
    decides which is which; here the lower node ranks first.  The set of nodes, and of cells, is the same.

    ``n`` above ``_lib.TRN_MAX_NODES`` (the nodes of a slice live in one workgroup): ``NotImplementedError``."""
    unknown = set(kwargs) - set(TRN_DEFAULTS)
    if unknown:
        raise TypeError(f"trn: unsupported arguments {sorted(unknown)} ({', '.join(TRN_DEFAULTS)} are)")
    par = dict(TRN_DEFAULTS, **kwargs)
    many = isinstance(X, (list, tuple))
    Xs = [_coords(x, "trn") for x in (X if many else [X])]
    ns = list(n) if isinstance(n, (list, tuple, np.ndarray)) else [n] * len(Xs)
    if len(ns) != len(Xs):
        raise ValueError(f"trn: {len(Xs)} slices but {len(ns)} node counts")
    ns = [_count(v, "trn") for v in ns]
    for v in ns:
        if v > _lib.TRN_MAX_NODES:
            raise NotImplementedError(f"trn: n = {v} nodes are not supported: at most {_lib.TRN_MAX_NODES} "
                                      f"(_lib.TRN_MAX_NODES; the nodes of a slice live in one workgroup's registers and LDS)")
    problems, schedules, rs = [], {}, None
    for x, v in zip(Xs, ns):
        if v not in schedules:
            schedules[v] = trn_schedule(v, **par)
        T, l, ep, kc = schedules[v]
        rs = np.random.RandomState(seed)
        w_idx = rs.randint(0, x.shape[0], v)
        rs = np.random.RandomState(seed)          # (TRNET.run draws through draw_sample, which seeds again)
        p_idx = rs.randint(0, x.shape[0], T)
        problems.append(dict(X=x, w_idx=w_idx, p_idx=p_idx, l=l, ep=ep, kc=kc))
    if rs is not None:
        _leave_global_rng(rs)
    k = _rt._shared_kernels(device, "float64")
    Ws = k.trn(problems) if problems else []
    out = [k.nearest_rows(x, W) if len(W) else np.zeros(0, dtype=np.int64) for x, W in zip(Xs, Ws)] if return_index else Ws
    return out if many else out[0]


def sample_by_kmeans(X, n, return_index=False, *, init=None, seed=0, iter=10, device=None):
    """``sample_by_kmeans`` of ``sampling.py:243-260``: ``iter`` Lloyd steps of k-means with n clusters on the device
    (``mvf_kmeans``: ``scipy.cluster.vq.kmeans2(X, start, iter, minit="matrix")``), then the cell nearest to every centroid
    (``mvf_nearest_rows``: exact, the smallest index among equally near cells).  Returns the indices, or ``X`` at them.

    ``init``: the (n, d) start matrix.  Without it the start is n distinct cells drawn with ``np.random.default_rng(seed)`` - a
    deviation: the reference lets ``kmeans2`` draw its start from the unseeded global generator, so its result is not
    reproducible.  A cluster that loses all members keeps its centroid, and one ``UserWarning`` with SciPy's text says so after
    the run."""
    X = _coords(X, "sample_by_kmeans")
    n = _count(n, "sample_by_kmeans")
    if int(iter) < 1:
        raise ValueError(f"sample_by_kmeans: iter must be at least 1, got {iter}")
    if init is None:
        if n > X.shape[0]:
            raise ValueError(f"sample_by_kmeans: n = {n} distinct start cells from {X.shape[0]} cells")
        init = X[np.random.default_rng(seed).choice(X.shape[0], size=n, replace=False)]
    init = np.ascontiguousarray(init, dtype=np.float64)
    if init.shape != (n, X.shape[1]) or not np.isfinite(init).all():
        raise ValueError(f"sample_by_kmeans: init must be a finite ({n}, {X.shape[1]}) matrix, got shape {init.shape}")
    if n == 0:
        nbrs = np.zeros(0, dtype=np.int64)
    else:
        k = _rt._shared_kernels(device, "float64")
        C, _, counts = k.kmeans(X, init, int(iter))
        if (np.asarray(counts) == 0).any():
            warnings.warn("One of the clusters is empty. Re-run kmeans with a different initialization.", UserWarning, stacklevel=2)
        nbrs = k.nearest_rows(X, C)
    return nbrs if return_index else X[nbrs]


def sample(arr, n, method="random", X=None, V=None, seed=19491001, **kwargs):
    """The dispatcher ``sample`` of ``sampling.py:17-59``: ``arr`` at the rows a method picks - ``"random"``
    (``np.random.seed(seed); np.random.choice(N, n, replace=False)``), ``"velocity"`` (needs ``V``), ``"trn"`` (needs ``X``),
    ``"kmeans"``; anything else, or a method without its data, is the reference's ``NotImplementedError``."""
    arr = np.asarray(arr)
    if method == "random":
        rs = np.random.RandomState(seed)
        idx = rs.choice(arr.shape[0], size=n, replace=False)
        _leave_global_rng(rs)
        return arr[idx]
    if method == "velocity" and V is not None:
        return arr[sample_by_velocity(V=V, n=n, seed=seed, **kwargs)]
    if method == "trn" and X is not None:
        return arr[trn(X=X, n=n, return_index=True, seed=seed, **kwargs)]
    if method == "kmeans":
        return arr[sample_by_kmeans(X, n, return_index=True)]
    raise NotImplementedError(f"The sampling method {method} is not implemented or relevant data are not provided.")


def _n_cells(model):
    return int(model.n_obs) if hasattr(model, "n_obs") else int(model.shape[0])


def _take_cells(model, idx):
    """``model[idx, :]``: ``AnnDataLite.select_obs`` or, by duck typing, AnnData's own indexing."""
    return model.select_obs(idx) if hasattr(model, "select_obs") else model[idx, :]


def downsampling(models, n_sampling=2000, sampling_method="trn", spatial_key="spatial"):
    """``downsampling`` of ``spateo/alignment/utils.py:25-47``: every slice reduced to ``n_sampling`` of its cells, picked by
    ``sample(..., method=sampling_method, X=obsm[spatial_key])``; always returns a list.  The reference's quirk is kept:
    ``n_sampling``, once clamped to a small slice, stays clamped for the slices after it.  With ``"trn"`` all slices run as one
    launch (the draws, and the state the global generator is left in, are those of the slice-by-slice loop).

    ``models``: ``AnnDataLite`` (subset by ``select_obs``) or ``anndata.AnnData`` (``adata[idx, :]``)."""
    models = list(models) if isinstance(models, (list, tuple)) else [models]
    counts = []
    for m in models:
        n_sampling = min(n_sampling, _n_cells(m))
        counts.append(n_sampling)
    coords = [np.asarray(m.obsm[spatial_key]) for m in models]
    if sampling_method == "trn":
        picks = trn(coords, counts, return_index=True) if models else []
    else:
        picks = [sample(np.arange(_n_cells(m)), c, method=sampling_method, X=x) for m, c, x in zip(models, counts, coords)]
    return [_take_cells(m.copy(), np.asarray(idx)) for m, idx in zip(models, picks)]


def solve_RT_by_correspondence(X, Y, return_scale=False):
    """``solve_RT_by_correspondence`` of ``spateo/alignment/utils.py:350-402``: the orthogonal ``R`` and the ``t`` with
    ``X ~ Y R^T + t`` from corresponding rows, by the SVD of ``(Y - mean Y)^T (X - mean X)``.  As in the reference a reflection
    is NOT corrected (``det R`` may be -1).  ``return_scale``: also the reference's scale expression."""
    X, Y = np.asarray(X), np.asarray(Y)
    tX, tY = np.mean(X, axis=0), np.mean(Y, axis=0)
    Xc, Yc = X - tX, Y - tY
    H = np.dot(Yc.T, Xc)
    U, _, Vt = np.linalg.svd(H)
    R = np.dot(Vt.T, U.T)
    t = tX - np.dot(tY, R.T)
    if return_scale:
        s = np.trace(np.dot(Xc.T, Xc) - np.dot(R.T, np.dot(Yc.T, Xc))) / np.trace(np.dot(Yc.T, Yc))
        return R, t, s
    return R, t


def _in_memory(who, models, **forms):
    """The on-disk forms of the reference need h5ad I/O: refused by name."""
    for name, (value, default) in forms.items():
        if value is not default and value != default:
            raise NotImplementedError(f"{who}: {name}={value!r} is not supported: the on-disk forms of the reference (h5ad "
                                      f"slices, saved transformations) are not implemented, pass the slices and the "
                                      f"transformation as in-memory lists")
    if any(isinstance(m, str) for m in models):
        raise NotImplementedError(f"{who}: models_path / file names are not supported: pass the slices as in-memory objects")


def morpho_align_transformation(models, models_path=None, save_transformation=False, transformation_path="./Spateo_transformation",
                                resume=False, rep_layer="X", rep_field="layer", genes=None, spatial_key="spatial",
                                key_added="align_spatial", iter_key_added="iter_spatial", vecfld_key_added="VecFld_morpho",
                                dissimilarity="kl", max_iter=200, dtype="float32", device="cpu", verbose=True, **kwargs):
    """``morpho_align_transformation`` of ``morpho_alignment.py:114-218`` on in-memory slices: every slice i + 1 aligned to the
    RAW slice i (``spatial_key`` on both sides), and per pair ``{"Rotation": R, "Translation": t}`` from
    ``solve_RT_by_correspondence(optimal_RnA[:, :2], obsm[spatial_key][:, :2])``.  ``models_path``, ``save_transformation`` and
    ``resume`` (h5ad slices, ``.npy`` files under ``transformation_path``): ``NotImplementedError``."""
    from ._morpho_pairwise import Morpho_pairwise

    models = list(models)
    _in_memory("morpho_align_transformation", models, models_path=(models_path, None),
               save_transformation=(save_transformation, False), resume=(resume, False))
    transformation = []
    for i in range(len(models) - 1):
        modelA, modelB = models[i], models[i + 1]
        morpho_model = Morpho_pairwise(sampleA=modelB, sampleB=modelA, rep_layer=rep_layer, rep_field=rep_field,
                                       dissimilarity=dissimilarity, genes=genes, spatial_key=spatial_key, key_added=key_added,
                                       iter_key_added=iter_key_added, vecfld_key_added=vecfld_key_added, max_iter=max_iter,
                                       dtype=dtype, device=device, verbose=verbose, **kwargs)
        morpho_model.run()
        R, t = solve_RT_by_correspondence(np.asarray(morpho_model.optimal_RnA)[:, :2], np.asarray(modelB.obsm[spatial_key])[:, :2])
        transformation.append({"Rotation": R, "Translation": t})
    return transformation


def morpho_align_apply_transformation(models, models_path=None, transformation=None, transformation_path="./Spateo_transformation",
                                      spatial_key="spatial", key_added="align_spatial", save_models_path=None, verbose=True):
    """``morpho_align_apply_transformation`` of ``morpho_alignment.py:221-314`` on in-memory slices: the pairwise
    transformations chained along the series, as the reference writes it -
    ``cur_t = t_i @ cur_R.T + cur_t; cur_R = cur_R @ R_i; obsm[key_added] = obsm[spatial_key] @ cur_R.T + cur_t`` - on 2-D
    coordinates; the slices are changed in place and returned.  ``models_path``, ``save_models_path`` and ``transformation=None``
    (read from ``transformation_path``): ``NotImplementedError``."""
    models = list(models)
    _in_memory("morpho_align_apply_transformation", models, models_path=(models_path, None), save_models_path=(save_models_path, None))
    if transformation is None:
        raise NotImplementedError("morpho_align_apply_transformation: transformation=None (read from transformation_path) is not "
                                  "supported: pass the list morpho_align_transformation returned")
    assert len(transformation) == len(models) - 1, "The length of transformation should be len(models) - 1."
    cur_R, cur_t = np.diag((1, 1)), np.zeros((2,))
    models[0].obsm[key_added] = np.array(models[0].obsm[spatial_key]).copy()
    for i in range(len(models) - 1):
        cur_model = models[i + 1]
        cur_t = transformation[i]["Translation"] @ cur_R.T + cur_t
        cur_R = cur_R @ transformation[i]["Rotation"]
        cur_model.obsm[key_added] = np.array(cur_model.obsm[spatial_key]).copy() @ cur_R.T + cur_t
    return models


def morpho_align_ref(models, models_ref=None, n_sampling=2000, sampling_method="random", rep_layer="X", rep_field="layer",
                     genes=None, spatial_key="spatial", key_added="align_spatial", iter_key_added="iter_spatial",
                     vecfld_key_added="VecFld_morpho", mode="SN-S", dissimilarity="kl", max_iter=200, dtype="float32",
                     device="cpu", verbose=True, **kwargs):
    """``morpho_align_ref`` of ``morpho_alignment.py:318-454`` with its signature: the reference slices ``models_ref`` (None:
    ``downsampling(models, n_sampling, sampling_method, spatial_key)``) are aligned pair by pair exactly as ``morpho_align``
    aligns them, and the full-resolution slice i + 1 takes ``obsm[f"{key_added}_nonrigid"]`` / ``_rigid`` from
    ``BA_transform(vecfld, obsm[key_added])`` with that pair's ``vecfld``; ``key_added`` takes the rigid result in mode
    ``"SN-S"``, the non-rigid one in ``"SN-N"``.  ``uns[iter_key_added]`` / ``uns[vecfld_key_added]`` are set on both slices.

    Returns ``(align_models, align_models_ref, pis, pis_ref)``; as in the reference both lists hold the pair's ``P`` (not
    transposed), ``None`` where ``Morpho_pairwise.run()`` returns ``None`` (see ``morpho_align``)."""
    from ._morpho_pairwise import Morpho_pairwise, _device_argument
    from .align import BA_transform

    if mode not in ("SN-S", "SN-N"):
        raise ValueError(f"mode must be 'SN-S' or 'SN-N', got {mode!r}")
    if models_ref is None:
        models_ref = downsampling([m.copy() for m in models], n_sampling=n_sampling, sampling_method=sampling_method,
                                  spatial_key=spatial_key)
    pis, pis_ref = [], []
    align_models, align_models_ref = [m.copy() for m in models], [m.copy() for m in models_ref]
    for m in align_models + align_models_ref:
        m.obsm[key_added] = np.array(m.obsm[spatial_key]).copy()
        m.obsm[f"{key_added}_rigid"] = np.array(m.obsm[spatial_key]).copy()
        m.obsm[f"{key_added}_nonrigid"] = np.array(m.obsm[spatial_key]).copy()
    picked = f"{key_added}_rigid" if mode == "SN-S" else f"{key_added}_nonrigid"
    for i in range(len(align_models) - 1):
        modelA_ref, modelB_ref = align_models_ref[i], align_models_ref[i + 1]
        morpho_model = Morpho_pairwise(sampleA=modelB_ref, sampleB=modelA_ref, rep_layer=rep_layer, rep_field=rep_field,
                                       dissimilarity=dissimilarity, genes=genes, spatial_key=key_added, key_added=key_added,
                                       iter_key_added=iter_key_added, vecfld_key_added=vecfld_key_added, max_iter=max_iter,
                                       dtype=dtype, device=device, verbose=verbose, **kwargs)
        P = morpho_model.run()
        modelB_ref.obsm[f"{key_added}_rigid"] = morpho_model.optimal_RnA.copy()
        modelB_ref.obsm[f"{key_added}_nonrigid"] = morpho_model.XAHat.copy()
        modelB_ref.obsm[key_added] = modelB_ref.obsm[picked]
        pis_ref.append(P)
        modelB = align_models[i + 1]
        vecfld = morpho_model.vecfld
        if iter_key_added is not None:
            modelB_ref.uns[iter_key_added] = modelB.uns[iter_key_added] = morpho_model.iter_added
        if vecfld_key_added is not None:
            modelB_ref.uns[vecfld_key_added] = modelB.uns[vecfld_key_added] = vecfld
        modelB.obsm[f"{key_added}_nonrigid"], _, modelB.obsm[f"{key_added}_rigid"] = BA_transform(
            vecfld=vecfld, quary_points=modelB.obsm[key_added], device=_device_argument(device), dtype=dtype)
        modelB.obsm[key_added] = modelB.obsm[picked]
        pis.append(P)
    return align_models, align_models_ref, pis, pis_ref
