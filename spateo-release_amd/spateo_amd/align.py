"""Alignment-side callers of the same Gaussian kernel and M-step: ``BA_transform``,
``update_nonrigid`` (the non-rigid update of ``Morpho_pairwise``: the SparseVFC M-step with Gamma <-> K, K_NA <-> P) and
``update_assignment`` (its assignment step, fused: every weight the other updates consume, without the NA x NB matrix).

Mirror of ``spateo/alignment/transform.py:61-116``: the learned non-rigid alignment ``vecfld`` (output of
``st.align.morpho_align``) applied to query points.  The N x M kernel contraction ``con_K(x, ctrl, beta) @ Coff`` runs
on the MI355X through ``libmvf`` (``mvf_apply``); the three 3 x 3 similarity maps around it are O(N) host NumPy.
``dtype`` selects the device cell dtype like the reference's ``dtype`` selects its backend dtype; outputs are host
float64 arrays ``(XAHat, quary_velocities, quary_optimal_similarity)``.
"""
from __future__ import annotations

import numpy as np

import torch

from . import _lib
from . import _runtime as _rt
from ._graph import (GraphKernel, KnnGraph, check_graph_kernel as _check_graph_kernel, con_K_graph, construct_knn_graph,  # noqa: F401
                     graph_distances, graph_kernel, knn)
from ._kernels import Layer, is_sparse
from .engine import _consistent_K
from .vectorfield import vector_field_function

__all__ = ["BA_transform", "update_nonrigid", "update_assignment", "morpho_iterate", "morpho_iterate_svi",
           "optimal_mapping", "mapping_from_best", "apply_assignment", "label_transfer_matrix", "init_sigma2", "init_probability_parameters", "coarse_rigid_alignment", "morpho_start",
           "Morpho_pairwise", "morpho_align", "pca", "group_pca", "trn", "sample_by_kmeans", "sample", "downsampling",
           "solve_RT_by_correspondence", "morpho_align_transformation", "morpho_align_apply_transformation", "morpho_align_ref",
           "icp", "icp_batch", "mesh_contours", "mesh_correction_loss", "Mesh_correction",
           "knn", "construct_knn_graph", "graph_distances", "con_K_graph", "graph_kernel", "KnnGraph", "GraphKernel"]

RETURN_P_MAX_ENTRIES = 1 << 27  # return_P=True: at most this many entries of P (1 GiB of float64 on the device and the host)


def _sparse_top_k(sparse_calculation_mode, sparse_top_k, return_P=False):
    """None (the dense path) or the validated ``sparse_top_k`` of ``sparse_calculation_mode``: the test against the device's
    cap is made on the requested value, before the reference's clamp to NA."""
    if not sparse_calculation_mode:
        return None
    if isinstance(sparse_top_k, bool) or int(sparse_top_k) != sparse_top_k or sparse_top_k < 1:
        raise ValueError(f"sparse_top_k must be a positive integer, got {sparse_top_k!r}")
    if sparse_top_k > _lib.ASSIGN_TOPK_MAX:
        raise NotImplementedError(f"update_assignment: sparse_calculation_mode with sparse_top_k = {int(sparse_top_k)} is not "
                                  f"supported: the device keeps at most {_lib.ASSIGN_TOPK_MAX} entries per column of P "
                                  f"(_lib.ASSIGN_TOPK_MAX; the per-column lists live in LDS)")
    if return_P:
        raise ValueError("return_P=True (the dense P) and sparse_calculation_mode=True (P as a scipy.sparse.coo_matrix) "
                         "exclude each other")
    return int(sparse_top_k)


def label_transfer_matrix(catA, catB, label_transfer_dict=None):
    """The K x L label-transfer table of a ``"label"`` layer from the two slices' category lists, as the reference builds it
    (``check_label_transfer`` / ``generate_label_transfer_dict``, ``spateo/alignment/methods/utils.py:264-312, 376-436``):
    ``T[j, k] = label_transfer_dict[catA[j]][catB[k]]``, rounded to float32 as there and returned as float64.  Without a
    dictionary the default one is used: 10 where both slices carry the same category and 1 elsewhere, every row divided by
    its sum ``+ 1e-8``.  Labels are then the positions in ``catA`` / ``catB`` (``.cat.codes`` of the ``obs`` column)."""
    if label_transfer_dict is not None and not isinstance(label_transfer_dict, dict):
        raise ValueError("label_transfer_dict should be a list or a dictionary.")  # (utils.py:300)
    catA, catB = list(catA), list(catB)
    if label_transfer_dict is None:
        raw = np.array([[10.0 if ca == cb else 1.0 for cb in catB] for ca in catA], dtype=np.float64).reshape(len(catA), len(catB))
        table = raw / (raw.sum(1, keepdims=True) + 1e-8)
    else:
        for ca in catA:
            if ca not in label_transfer_dict:
                raise KeyError(f"Category '{ca}' from catA not found in label_transfer_dict.")
            for cb in catB:
                if cb not in label_transfer_dict[ca]:
                    raise KeyError(f"Category '{cb}' from catB not found in label_transfer_dict['{ca}'].")
        table = np.array([[label_transfer_dict[ca][cb] for cb in catB] for ca in catA], dtype=np.float64).reshape(len(catA), len(catB))
    return table.astype(np.float32).astype(np.float64)


class LabelTransferRequired(AssertionError, NotImplementedError):
    """A ``"label"`` layer without ``label_transfer``: the reference's assertion (``calc_distance``, ``utils.py:909``) with its
    text.  Also a ``NotImplementedError``, which is what this call - a label layer and no table, the only one earlier versions
    could be given - raised when the metric was refused: callers that catch it to fall back keep working."""


def _label_arguments(A, B, NA, NB, table):
    """One label layer's two label vectors (validated, int64).  `table`: the validated K x L table or None."""
    A, B = np.asarray(A), np.asarray(B)
    if table is None:
        raise LabelTransferRequired("label_transfer must be provided for metric 'label'.")  # calc_distance (utils.py:909)
    assert A.ndim == 1, "X should be a 1-dimensional array."                            # _label_distance_backend (:818-828)
    assert B.ndim == 1, "Y should be a 1-dimensional array."
    assert np.issubdtype(A.dtype, np.integer) and np.issubdtype(B.dtype, np.integer), "X should contain integer values."
    if len(A) != NA or len(B) != NB:
        raise ValueError("every layer must have one row per cell of its slice")
    K, L = table.shape
    if len(A) and (A.min() < 0 or A.max() >= K):
        raise ValueError(f"a label layer's A labels must lie in 0 .. {K - 1}, the rows of label_transfer")
    if len(B) and (B.min() < 0 or B.max() >= L):
        raise ValueError(f"a label layer's B labels must lie in 0 .. {L - 1}, the columns of label_transfer")
    return A.astype(np.int64), B.astype(np.int64)


def _assignment_arguments(XAHat, coordsB, exp_layers_A, exp_layers_B, dissimilarity, probability_type,
                          probability_parameters, return_P, label_transfer=None, who="update_assignment"):
    """Validation of update_assignment (no device needed; `who`: the public function named in a refusal): the arrays as float64 (a label layer's as int64), the per-layer
    (metric, probability type, parameter) codes of include/mvf.h and the label-transfer table as float64 (K, L) or None."""
    XA, XB = np.asarray(XAHat, dtype=np.float64), np.asarray(coordsB, dtype=np.float64)
    if XA.ndim != 2 or XB.ndim != 2 or XA.shape[1] != XB.shape[1]:
        raise AssertionError("X and Y do not have the same number of features.")  # _euc_distance_backend (utils.py:775)
    if XA.shape[1] not in (2, 3):
        raise NotImplementedError(f"{who}: spatial coordinates must be 2-D or 3-D, got D = {XA.shape[1]}")
    LA = list(exp_layers_A) if isinstance(exp_layers_A, (list, tuple)) else [exp_layers_A]
    LB = list(exp_layers_B) if isinstance(exp_layers_B, (list, tuple)) else [exp_layers_B]
    n_layers = len(LA)
    table = None
    if label_transfer is not None:
        table = np.ascontiguousarray(label_transfer, dtype=np.float64)
        if table.ndim != 2 or table.shape[0] < 1 or table.shape[1] < 1 or not np.isfinite(table).all():
            raise ValueError("label_transfer must be a finite 2-D (K, L) array with K, L >= 1")
    as_list = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n_layers  # noqa: E731
    metrics, kinds = as_list(dissimilarity), as_list(probability_type)
    params = [None] * n_layers if probability_parameters is None else as_list(probability_parameters)
    if n_layers < 1 or not (len(LB) == len(metrics) == len(kinds) == len(params) == n_layers):
        raise ValueError("exp_layers_A, exp_layers_B, dissimilarity, probability_type and probability_parameters must list "
                         "the same (non-zero) number of layers")
    if n_layers > _lib.ASSIGN_MAX_LAYERS:
        raise NotImplementedError(f"{who}: at most {_lib.ASSIGN_MAX_LAYERS} layers are supported, got {n_layers}")
    codes = []
    for l, (met, kind, par) in enumerate(zip(metrics, kinds, params)):
        if met not in _lib.ASSIGN_METRICS:
            raise ValueError(f"Unsupported dissimilarity metric: {met}")
        if met == "label":
            LA[l], LB[l] = _label_arguments(LA[l], LB[l], len(XA), len(XB), table)
        else:
            # a scipy.sparse layer stays sparse (HipKernels.assign_prepare expands its CSR arrays on the device)
            A, B = LA[l], LB[l] = [v.tocsr() if is_sparse(v) else np.asarray(v, dtype=np.float64) for v in (LA[l], LB[l])]
            if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1]:
                raise AssertionError("X and Y do not have the same number of features.")
            if A.shape[0] != len(XA) or B.shape[0] != len(XB):
                raise ValueError("every layer must have one row per cell of its slice")
        if str(kind).lower() not in _lib.ASSIGN_PROBS:
            raise ValueError(f"Unsupported probability type: {kind}")  # calc_probability (utils.py:983)
        prob = _lib.ASSIGN_PROBS[str(kind).lower()]
        if prob == 0 and par is None:
            raise ValueError("probability_parameter must be provided for 'Gauss' probability type.")  # (utils.py:976)
        codes.append((_lib.ASSIGN_METRICS[met], prob, 0.0 if par is None else float(par)))
    if return_P and len(XA) * len(XB) > RETURN_P_MAX_ENTRIES:
        raise ValueError(f"return_P=True materialises NA x NB = {len(XA) * len(XB)} entries; the cap is "
                         f"{RETURN_P_MAX_ENTRIES} (align.RETURN_P_MAX_ENTRIES)")
    return XA, XB, LA, LB, codes, table


def _n_rows(layer):
    """Rows of a layer as handed in: a scipy.sparse matrix is asked for its shape, never converted."""
    return layer.shape[0] if is_sparse(layer) else len(np.asarray(layer))


def _spatial_outlier(sigma2, gamma, samples_s, NA, D):
    return float(np.power(2 * np.pi * sigma2, D / 2) * (1 - gamma) / (gamma * (samples_s * NA)))  # utils.py:1051-1053


def _prepare_layers(k, LA, LB, codes, table=None):
    """Upload and prepare both sides of every layer (mvf_assign_prepare; a label layer: mvf_assign_label_prepare and the
    one float64 table its kind shares): the operands no iteration changes, one `Layer` record each."""
    layers = []
    T = None
    for A, B, (metric, prob, param) in zip(LA, LB, codes):
        if metric == _lib.ASSIGN_LABEL:
            T = k.h2d(table) if T is None else T
            K, L = table.shape
            layers.append(Layer(T, None, k.assign_label_prepare(A, K), k.assign_label_prepare(B, L), L, metric, prob, param))
            continue
        layers.append(_product_layer(k, A, B, metric, prob, param))
    return layers


def _assignment_stage(who, XAHat, coordsB, exp_layers_A, exp_layers_B, dissimilarity, probability_type, probability_parameters,
                      sigma2, alpha, SigmaDiag, gamma, samples_s, sigma2_variance, dtype, label_transfer, return_P=False,
                      features=None):
    """The prelude update_assignment, optimal_mapping and apply_assignment share, on the host: ``dtype``, the arrays and layers
    (_assignment_arguments, refusals under the name ``who``), ``features`` = (features_A, features_B) where the stage takes
    them, ``alpha`` / ``SigmaDiag``, the scalars.  Returns (XA, XB, FA, FB, upload); nothing touches the device before
    ``upload(device)``: the layers prepared, then XAHat, coordsB and model_mul uploaded, it returns (k, the seven arguments
    every assignment entry point of HipKernels takes)."""
    if dtype not in ("float32", "float64"):
        raise ValueError("dtype must be 'float32' or 'float64'")
    XA, XB, LA, LB, codes, table = _assignment_arguments(XAHat, coordsB, exp_layers_A, exp_layers_B, dissimilarity,
                                                         probability_type, probability_parameters, return_P, label_transfer,
                                                         who=who)
    NA, D = XA.shape
    FA = FB = None
    if features is not None:
        FA, FB = _transfer_features(features[0], NA, "features_A"), _transfer_features(features[1], len(XB), "features_B")
        if FA is None and FB is None:
            raise ValueError(f"{who}: features_A or features_B must be given")
    al, sd = np.asarray(alpha, dtype=np.float64).reshape(-1), np.asarray(SigmaDiag, dtype=np.float64).reshape(-1)
    if len(al) != NA or len(sd) != NA:
        raise ValueError("alpha and SigmaDiag must be (NA,)")
    sigma2, gamma, samples_s, sigma2_variance = float(sigma2), float(gamma), float(samples_s), float(sigma2_variance)

    def upload(device):
        model_mul = al * np.exp(-sd / sigma2)                                               # morpho_class.py:1087
        outlier = _spatial_outlier(sigma2, gamma, samples_s, NA, D)
        k = _rt._make_kernels(device, dtype)
        layers = _prepare_layers(k, LA, LB, codes, table)
        return k, (k.to_x4(XA), k.to_x4(XB), layers, k.h2d(model_mul), sigma2, sigma2_variance, outlier)

    return XA, XB, FA, FB, upload


def _coo_from_lists(rows, vals, NA):
    """The reference's sparse P (`_dense_to_sparse`, utils.py:1369-1404) from the device's lists (NB, k_eff): entries in its
    order, col = repeat(arange(NB), k_eff)."""
    from scipy.sparse import coo_matrix

    rows, vals = np.asarray(rows), np.asarray(vals, dtype=np.float64)
    NB, ke = rows.shape
    col = np.repeat(np.arange(NB), ke)
    return coo_matrix((vals.reshape(-1), (rows.reshape(-1).astype(np.int64), col)), shape=(NA, NB))


def update_assignment(XAHat, coordsB, exp_layers_A, exp_layers_B, *, dissimilarity, probability_type,
                      probability_parameters, sigma2, alpha, SigmaDiag, gamma, samples_s, sigma2_variance=1.0,
                      dtype: str = "float64", device=None, return_P=False, sparse_calculation_mode=False, sparse_top_k=1024,
                      label_transfer=None):
    """The assignment step of Spateo's alignment, ``Morpho_pairwise._update_assignment_P``
    (``spateo/alignment/methods/morpho_class.py:1071-1200``) followed by ``get_P_core`` on the dense path
    (``spateo/alignment/methods/utils.py:993-1096``; ``use_chunk`` changes nothing mathematically), on the MI355X as one
    fused two-pass kernel (``mvf_assign``): the NA x NB matrix ``P`` is never written.  For SVI the caller passes the
    batch's rows of ``coordsB`` and of the B layers and blends the three ``Sp*`` scalars itself.

    ``XAHat`` (NA, D) and ``coordsB`` (NB, D) with D in {2, 3}; 1 to 4 layers ``exp_layers_A[l]`` (NA, G_l) /
    ``exp_layers_B[l]`` (NB, G_l) with ``dissimilarity[l]`` in ``"kl"``, ``"sym_kl"``, ``"euc"`` / ``"euclidean"`` (the
    SQUARED distance clamped at 0, as the reference has it), ``"square_euc"`` / ``"square_euclidean"`` (its square root),
    ``"cos"`` / ``"cosine"``; ``probability_type[l]`` in ``"gauss"`` (``exp(-d / (2 probability_parameters[l]))``),
    ``"cos"`` (``1 - d``), ``"prob"`` (``d``); ``alpha`` and ``SigmaDiag`` (NA,); the rest scalars.  ``dtype`` is the
    storage of the coordinates and of the prepared layer operands; distances, exponents and every sum are float64 in
    both modes.

    ``dissimilarity[l] = "label"`` (what the reference forces for ``rep_field="obs"``, ``morpho_class.py:412-415``, usually
    with ``probability_type[l] = "prob"``): ``exp_layers_A[l]`` (NA,) and ``exp_layers_B[l]`` (NB,) are 1-D INTEGER arrays,
    one label per cell, and the layer's distance is ``label_transfer[labelA_i, labelB_j]`` (``_label_distance_backend``,
    ``utils.py:791-832``) - ``label_transfer`` (K, L), finite, required then (``label_transfer_matrix`` builds the reference's
    from the category lists); several label layers share it, as in ``calc_distance``.  The table stays float64 in both modes.
    A float or 2-D label array, a missing table: the reference's ``AssertionError``; a label outside the table, a table that
    is not 2-D and finite: ``ValueError``.  The three probability types apply to it as to any distance; ``"gauss"`` needs its
    parameter.

    Not supported (``NotImplementedError``): ``sparse_calculation_mode`` with
    ``sparse_top_k`` above ``_lib.ASSIGN_TOPK_MAX`` = 64 (the reference constructor's default, 1024, among them), more than
    4 layers, D outside {2, 3}.

    ``sparse_calculation_mode=True`` with ``1 <= sparse_top_k <= 64`` (``get_P_core`` -> ``_dense_to_sparse(axis=0,
    descending=True)``, ``utils.py:1085-1094, 1369-1404``; ``mvf_assign_topk``): the ``k_eff = min(sparse_top_k, NA)`` largest
    entries of every column of ``P`` are kept - on equal values the smaller row - and ``K_NA``, ``K_NB``, ``Sp`` and ``PXB``
    are formed from them (``morpho_class.py:1171-1198``); ``K_NA_spatial``, ``K_NA_sigma2`` and ``sigma2_related`` stay the
    dense ones.  The result gains ``P``, a ``scipy.sparse.coo_matrix`` (NA, NB) with the entries in the reference's order
    (``col = repeat(arange(NB), k_eff)``), and ``topk_rows`` / ``topk_values`` (NB, k_eff): column j's entries, value
    descending.  ``sparse_top_k < 1`` and ``return_P=True`` in this mode are ``ValueError``.

    Returns host float64: ``K_NA``, ``K_NA_spatial``, ``K_NA_sigma2`` (NA,), ``K_NB`` (NB,), ``Sp``, ``Sp_spatial``,
    ``Sp_sigma2``, ``sigma2_related`` (already divided by ``Dim * Sp_sigma2``, ``:1200``), ``PXB = P @ coordsB`` (NA, D)
    and, with ``return_P=True``, the dense ``P`` (NA, NB) - label transfer and debugging only; ``ValueError`` above
    ``RETURN_P_MAX_ENTRIES`` entries (``apply_assignment`` forms ``P @ F`` and ``P.T @ F`` at any size, without ``P``).  Two calls
    give bit-identical results.

    What the other updates take from it:

    * ``update_nonrigid``'s ``PXB_term`` is ``PXB - RnA * K_NA[:, None]``;
    * ``_update_rigid``'s ``XA_hat^T P XB_hat`` (``:1300-1408``) is ``XA_hat^T PXB - (XA_hat^T K_NA) mu_XB``, from
      ``PXB`` and ``K_NA``."""
    if dtype not in ("float32", "float64"):                   # (before the stage's own check: dtype is refused first)
        raise ValueError("dtype must be 'float32' or 'float64'")
    top_k = _sparse_top_k(sparse_calculation_mode, sparse_top_k, return_P)
    XA, XB, _, _, upload = _assignment_stage("update_assignment", XAHat, coordsB, exp_layers_A, exp_layers_B, dissimilarity,
                                             probability_type, probability_parameters, sigma2, alpha, SigmaDiag, gamma,
                                             samples_s, sigma2_variance, dtype, label_transfer, return_P=return_P)
    (NA, D), NB = XA.shape, len(XB)
    names = ("K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2")
    if NA == 0 or NB == 0:
        out = {q: np.zeros(NB if q == "K_NB" else NA) for q in names}
        out.update(Sp=0.0, Sp_spatial=0.0, Sp_sigma2=0.0, sigma2_related=float("nan"), PXB=np.zeros((NA, D)))
        if return_P:
            out["P"] = np.zeros((NA, NB))
        if top_k is not None:
            ke = min(top_k, NA)
            out["topk_rows"], out["topk_values"] = np.zeros((NB, ke), dtype=np.int32), np.zeros((NB, ke))
            out["P"] = _coo_from_lists(out["topk_rows"], out["topk_values"], NA)
        return out
    k, common = upload(device)
    dev = k.assign_topk(*common, top_k) if top_k is not None else k.assign(*common, dense=bool(return_P))
    keys = list(names) + ["PXB", "scalars"] + (["P"] if return_P else []) + (["rows", "vals"] if top_k is not None else [])
    host = dict(zip(keys, _rt._to_host(k, [dev[q] for q in keys])))
    out = {q: np.array(host[q], dtype=np.float64) for q in names}
    out["Sp"], out["Sp_spatial"], out["Sp_sigma2"] = (float(out[q].sum()) for q in ("K_NB", "K_NA_spatial", "K_NA_sigma2"))
    out["sigma2_related"] = float(host["scalars"][0]) / (D * out["Sp_sigma2"])
    out["PXB"] = np.array(host["PXB"][:, :D], dtype=np.float64)
    if return_P:
        out["P"] = np.array(host["P"], dtype=np.float64)
    if top_k is not None:
        out["topk_rows"], out["topk_values"] = np.array(host["rows"], dtype=np.int32), np.array(host["vals"], dtype=np.float64)
        out["P"] = _coo_from_lists(out["topk_rows"], out["topk_values"], NA)
    return out


BEST_KEYS = ("rows", "row_values", "cols", "col_values")


def _best_to_host(k, dev):
    """HipKernels.assign_best's dict of device tensors as host arrays: rows / cols int32 (n, 2), the values float64."""
    host = dict(zip(BEST_KEYS, _rt._to_host(k, [dev[q] for q in BEST_KEYS])))
    return {q: np.array(host[q], dtype=np.float64 if q.endswith("values") else np.int32) for q in BEST_KEYS}


def _empty_mapping(D):
    return {"mapping_X": np.zeros((0, D)), "mapping_Y": np.zeros((0, D)), "pi_index": np.zeros((0, 2), dtype=np.int32),
            "pi_value": np.zeros(0)}


def mapping_from_best(best, X, Y, keep_all=False):
    """The two dicts of the reference's ``mapping_aligned_coords(X, Y, P, keep_all)`` (``spateo/alignment/utils.py:196-255``)
    from the best partners ``mvf_assign_best`` found, without ``P``.

    ``best``: ``rows`` (NA, 2) / ``cols`` (NB, 2) integer - per cell its partner under the "nearest" rule (column 0: among
    equal maxima the nearest coordinate, ``keep_all=False``) and under the "first" rule (column 1: the smallest index,
    ``keep_all=True``) - and ``row_values`` (NA,) / ``col_values`` (NB,), the maxima: the ``best`` of ``morpho_iterate(...,
    optimal_mapping=True)``, or ``HipKernels.assign_best``'s result brought to the host.  ``X`` (NA, D) and ``Y`` (NB, D): the
    coordinates the dicts quote (``XAHat`` and ``coordsB``).

    Returns ``(by_A, by_B)``, each ``{"mapping_X", "mapping_Y", "pi_index" (n, 2) int32 = (index_x, index_y), "pi_value" (n,)
    float64}``: ``by_A`` has one entry per A cell in index order, ``by_B`` one per B cell.  An empty side gives empty dicts."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    if X.ndim != 2 or Y.ndim != 2 or X.shape[1] != Y.shape[1]:
        raise ValueError("mapping_from_best: X (NA, D) and Y (NB, D) must be 2-D with the same D")
    missing = [q for q in BEST_KEYS if not isinstance(best, dict) or q not in best]
    if missing:
        raise ValueError(f"mapping_from_best: best must be a dict with {', '.join(BEST_KEYS)}; missing: {', '.join(missing)}")
    NA, NB = len(X), len(Y)
    if NA == 0 or NB == 0:
        return _empty_mapping(X.shape[1]), _empty_mapping(X.shape[1])
    col = 1 if keep_all else 0
    out = []
    for idx, val, n, limit, own in ((best["rows"], best["row_values"], NA, NB, 0), (best["cols"], best["col_values"], NB, NA, 1)):
        idx, val = np.asarray(idx), np.asarray(val, dtype=np.float64).reshape(-1)
        if idx.shape != (n, 2) or idx.dtype.kind not in "iu" or val.shape != (n,):
            raise ValueError(f"mapping_from_best: the {'rows' if own == 0 else 'cols'} side must be an integer (n, 2) array with "
                             f"(n,) values, n = {n}; got {idx.shape} {idx.dtype} and {val.shape}")
        partner = idx[:, col].astype(np.int64)
        if partner.min() < 0 or partner.max() >= limit:
            raise ValueError(f"mapping_from_best: a partner index lies outside [0, {limit})")
        pair = np.empty((n, 2), dtype=np.int32)
        pair[:, own], pair[:, 1 - own] = np.arange(n), partner
        out.append({"mapping_X": X[pair[:, 0]], "mapping_Y": Y[pair[:, 1]], "pi_index": pair, "pi_value": val.copy()})
    return out[0], out[1]


def optimal_mapping(XAHat, coordsB, exp_layers_A, exp_layers_B, *, dissimilarity, probability_type, probability_parameters,
                    sigma2, alpha, SigmaDiag, gamma, samples_s, sigma2_variance=1.0, dtype: str = "float64", device=None,
                    label_transfer=None, keep_all=False):
    """The cell mapping after an alignment - ``mapping_aligned_coords(XAHat, coordsB, P, keep_all)`` of the reference
    (``spateo/alignment/utils.py:196-255``, on ``get_optimal_mapping_relationship``, ``:157-193``) for the ``P`` that
    ``update_assignment`` would form from the same arguments - without ``P``: ``mvf_assign_best`` reduces the tiles of the fused
    assignment to the largest entry of every row and of every column, so two slices of 100 000 cells (a dense ``P`` of 80 GB)
    get their mapping in about the time of an assignment step and a half.

    Arguments as ``update_assignment`` takes them (``"label"`` layers with ``label_transfer`` included), without ``return_P``
    and the sparse pair; errors are ``update_assignment``'s.  ``keep_all=False``: among equal maxima the partner with the
    nearest coordinate - so a cell whose row (column) of ``P`` is all zero, every far or outlying cell, maps to its nearest
    neighbour, as in the reference; ``keep_all=True``: the smallest index among equal maxima.

    Returns ``(by_A, by_B)``: ``by_A`` maps every A cell to its best B cell (the maximum of its row of ``P``), ``by_B`` every B
    cell to its best A cell (of its column); each ``{"mapping_X": XAHat[index_x], "mapping_Y": coordsB[index_y], "pi_index"
    (n, 2) int32 = (index_x, index_y), "pi_value" (n,) float64}``.  ``st.tdr.cell_directions(adataA, adataB, mapping=by_A)``
    turns ``by_A`` into ``V_mapping``.  Two calls give equal bits.

    Where this differs from ``get_optimal_mapping_relationship`` / ``mapping_aligned_coords``: the entries are sorted by cell
    index and there is ONE per cell also for ``keep_all=True``.  The reference appends the cells with tied maxima at the end
    of its index arrays and, with ``keep_all=True``, returns every tied pair; its ``mapping_aligned_coords`` then sorts and
    drops the duplicates, which is what is returned here."""
    XA, XB, _, _, upload = _assignment_stage("optimal_mapping", XAHat, coordsB, exp_layers_A, exp_layers_B, dissimilarity,
                                             probability_type, probability_parameters, sigma2, alpha, SigmaDiag, gamma,
                                             samples_s, sigma2_variance, dtype, label_transfer)
    if len(XA) == 0 or len(XB) == 0:
        return _empty_mapping(XA.shape[1]), _empty_mapping(XA.shape[1])
    k, common = upload(device)
    return mapping_from_best(_best_to_host(k, k.assign_best(*common)), XA, XB, keep_all)


def _transfer_features(features, n, name, who="apply_assignment"):
    """``features_A`` / ``features_B`` of apply_assignment validated (no device needed): None, or host float64 (n, c >= 1).  A
    1-D integer array is a label vector and becomes its one-hot matrix (n, max + 1)."""
    if features is None:
        return None
    if is_sparse(features):
        raise NotImplementedError(f"{who}: scipy.sparse {name} is not supported: the sweep reads dense float64 rows; pass "
                                  f"{name}.toarray(), a block of columns at a time if it is wide")
    F = np.asarray(features)
    if F.ndim == 1 and F.dtype.kind in "iu":
        if len(F) != n:
            raise ValueError(f"{who}: {name} must have one entry per cell of its slice ({n}), got {len(F)}")
        if len(F) and F.min() < 0:
            raise ValueError(f"{who}: a label vector {name} must be non-negative")
        out = np.zeros((n, int(F.max()) + 1 if len(F) else 1))
        out[np.arange(n), F.astype(np.int64)] = 1.0
        return out
    if F.dtype.kind not in "fiub":
        raise ValueError(f"{who}: {name} must be numeric (n, c) or a 1-D integer label vector, got dtype {F.dtype}")
    F = np.ascontiguousarray(F, dtype=np.float64)
    if F.ndim != 2 or F.shape[0] != n:
        raise ValueError(f"{who}: {name} must have one row per cell of its slice ({n}), got shape {F.shape}")
    if F.shape[1] < 1:
        raise ValueError(f"{who}: {name} needs at least one column")
    if not np.isfinite(F).all():
        raise ValueError(f"{who}: {name} must be finite")
    return F


def _normalized_rows(M, K):
    """Every row of M divided by its cell's sum K; a cell whose sum is 0 (no partner within reach) keeps a zero row."""
    K = np.asarray(K, dtype=np.float64)
    out = np.zeros_like(M)
    live = K != 0.0
    out[live] = M[live] / K[live, None]
    return out


def _normalize_applied(out, normalize):
    if normalize:
        if "to_A" in out:
            out["to_A"] = _normalized_rows(out["to_A"], out["K_NA"])
        if "to_B" in out:
            out["to_B"] = _normalized_rows(out["to_B"], out["K_NB"])
    return out


def _applied_to_host(k, dev, normalize):
    """HipKernels.assign_apply's dict of device tensors as apply_assignment's host result."""
    keys = [q for q in ("to_A", "to_B", "K_NA", "K_NB") if q in dev]
    out = {q: np.array(v, dtype=np.float64) for q, v in zip(keys, _rt._to_host(k, [dev[q] for q in keys]))}
    return _normalize_applied(out, normalize)


def _applied_from_coo(P, K_NA, K_NB, FA, FB, normalize):
    """The same from the kept entries of sparse_calculation_mode: the returned coo_matrix times F, on the host."""
    P = P.tocsr()
    out = {}
    if FB is not None:
        out["to_A"], out["K_NA"] = np.asarray(P @ FB, dtype=np.float64), np.array(K_NA, dtype=np.float64)
    if FA is not None:
        out["to_B"] = np.asarray(P.T @ FA, dtype=np.float64)
    out["K_NB"] = np.array(K_NB, dtype=np.float64)
    return _normalize_applied(out, normalize)


def _apply_argument(apply, NA, NB, who):
    """``apply=`` of the loops validated (no device needed): None or dict(FA=, FB=, normalize=)."""
    if apply is None:
        return None
    if not isinstance(apply, dict) or not set(apply) <= {"features_A", "features_B", "normalize"}:
        raise ValueError(f"{who}: apply must be a dict with features_A and / or features_B and, optionally, normalize")
    FA = _transfer_features(apply.get("features_A"), NA, "features_A", who)
    FB = _transfer_features(apply.get("features_B"), NB, "features_B", who)
    if FA is None and FB is None:
        raise ValueError(f"{who}: apply needs features_A or features_B")
    return dict(FA=FA, FB=FB, normalize=bool(apply.get("normalize", True)))


def apply_assignment(XAHat, coordsB, exp_layers_A, exp_layers_B, *, features_A=None, features_B=None, normalize=True,
                     dissimilarity, probability_type, probability_parameters, sigma2, alpha, SigmaDiag, gamma, samples_s,
                     sigma2_variance=1.0, dtype: str = "float64", device=None, label_transfer=None):
    """The assignment applied to cell features - what the reference's users form from the dense ``P`` that
    ``Morpho_pairwise.run()`` returns - for the ``P`` that ``update_assignment`` would form from the same arguments, without
    ``P`` (``mvf_assign_apply``): the tiles of the fused step feed a matrix product as they are formed, so two slices of
    100 000 cells (a dense ``P`` of 80 GB) are served like any other size.

    * ``features_B`` (NB, CB): ``to_A = P @ features_B`` (NA, CB) - expression or an embedding of slice B carried to the A
      cells; with ``normalize`` each A cell's barycentre of its partners' rows.
    * ``features_A`` (NA, CA): ``to_B = P.T @ features_A`` (NB, CA) - an annotation of slice A carried to the B cells.

    A 1-D INTEGER ``features_*`` is a label vector and is expanded on the host to its one-hot matrix (n, max + 1):
    ``to_B`` of ``features_A=labels_A`` is every B cell's class distribution.  Anything else must be a finite numeric (n, c >= 1)
    array (``ValueError``); ``scipy.sparse`` features are ``NotImplementedError``.  One of the two must be given.

    ``normalize=True`` divides every output row by its cell's sum of ``P`` - ``K_NA[i]`` for ``to_A``, ``K_NB[j]`` for ``to_B``;
    a cell whose sum is 0 (a B cell out of reach of every A cell, an A cell whose weight is 0) gets a zero row.
    ``normalize=False`` returns the raw products.

    The other arguments and their errors are ``update_assignment``'s (``"label"`` layers with ``label_transfer`` included),
    without ``return_P`` and the sparse pair.  ``dtype`` is the storage of the coordinates and of the prepared layer operands;
    the features, the products and every sum are float64 in both modes.

    Returns host float64 ``{"to_A", "K_NA"}`` (with ``features_B``), ``{"to_B"}`` (with ``features_A``) and ``"K_NB"``; an empty
    side gives zeros of the right shape.  Two calls give equal bits."""
    XA, XB, FA, FB, upload = _assignment_stage("apply_assignment", XAHat, coordsB, exp_layers_A, exp_layers_B, dissimilarity,
                                               probability_type, probability_parameters, sigma2, alpha, SigmaDiag, gamma,
                                               samples_s, sigma2_variance, dtype, label_transfer,
                                               features=(features_A, features_B))
    NA, NB = len(XA), len(XB)
    if NA == 0 or NB == 0:
        out = {"K_NB": np.zeros(NB)}
        if FB is not None:
            out["to_A"], out["K_NA"] = np.zeros((NA, FB.shape[1])), np.zeros(NA)
        if FA is not None:
            out["to_B"] = np.zeros((NB, FA.shape[1]))
        return out
    k, common = upload(device)
    dev = k.assign_apply(*common, features_B=None if FB is None else k.h2d(FB), features_A=None if FA is None else k.h2d(FA))
    return _applied_to_host(k, dev, bool(normalize))


def _nonrigid_solve(k, G, Gamma, reg, R, indefinite=None):
    """The device-resident solve of update_nonrigid (and of morpho_iterate): C = pinv(G + reg Gamma) R with scipy.linalg.pinv's
    cut-off.  Returns (C (m x 3 float64 device), rcond, lowrank); the decomposition stays in k's workspace for pinv_diag.

    ``indefinite`` (the geodesic kernel): exp(-beta D^2) of a graph distance is no positive semi-definite kernel - Gamma of the
    3-D golden case has eigenvalues down to -0.13 against 8.0, and SigmaInv six negative ones down to -4.1 against 1040 - and the
    reference's ``pinv`` (an SVD) keeps such eigenpairs with their sign.  So does mvf_solve_minnorm (|lambda| against the cut-off)
    once its shift makes the factorisation exist: the ladder of shifts then goes on past 2^-12 of the mean diagonal, by factors
    of 4 up to 1/2, and the rank-revealing path, which needs a semi-definite matrix, is not taken.  ``indefinite`` is a dict the
    caller keeps for its loop: the ladder starts at the shift that worked last time (``indefinite["shift"]``) instead of climbing
    through a dozen failed factorisations, each a host read, in every iteration."""
    m = G.shape[0]
    f64 = torch.float64
    C, info, einfo = k.zeros(m, 3, dtype=f64), k.zeros(1, dtype=torch.int32), k.zeros(_lib.EINFO_DOUBLES, dtype=f64)
    rcond = m * float(np.finfo(np.float64).eps)
    lowrank = m >= 1024 and hasattr(k, "solve_minnorm_lr") and indefinite is None
    if lowrank:
        # rank-revealing factor + Jacobi on its columns (the faster path once the factor drops most columns)
        k.solve_minnorm_lr(G, Gamma, reg, R, C, info, einfo, rcond=rcond)
        if int(info.cpu()[0]) != 0:
            raise _lib.MVFError("update_nonrigid: SigmaInv has non-finite entries")
        _lib.check_converged(float(einfo.cpu()[_lib.EINFO_SWEEPS]))
    else:
        shift = 2.0 ** -36 if indefinite is None else indefinite.get("shift", 2.0 ** -36)
        while True:
            k.solve_minnorm(G, Gamma, reg, shift, R, C, info, einfo, rcond=rcond)
            if int(info.cpu()[0]) == 0:
                _lib.check_converged(float(einfo.cpu()[_lib.EINFO_SWEEPS]))
                if indefinite is not None:
                    indefinite["shift"] = shift
                break
            shift *= 16.0 if shift < 2.0 ** -12 else 4.0
            if shift > (0.5 if indefinite is not None else 2.0 ** -12):
                raise _lib.MVFError("update_nonrigid: SigmaInv is not numerically positive semi-definite")
    return C, rcond, lowrank


def update_nonrigid(coordsA, inducing_variables, beta, K_NA, PXB_term, sigma2, lambdaVF, dtype: str = "float64",
                    device=None, *, guidance=None, svi=None, kernel_type="euc", graph_kernel=None):
    """The non-rigid update of Spateo's alignment, ``Morpho_pairwise._update_nonrigid``
    (``spateo/alignment/methods/morpho_class.py:1254-1298``), on the MI355X with the kernels of the SparseVFC M-step - it
    is the same computation (``SigmaInv = sigma2 lambdaVF Gamma + U^T diag(K_NA) U``,
    ``Coff = pinv(SigmaInv) U^T PXB_term``, ``VnA = U Coff``; Gamma = con_K(ctrl, ctrl), U = con_K(coordsA, ctrl) as
    ``_construct_kernel`` builds them, ``:825-875``):

    * ``U^T diag(K_NA) U`` and ``U^T PXB_term``  -> ``mvf_gram`` (f64 MFMA; U is never materialised),
    * ``pinv(SigmaInv) @ rhs``                   -> ``mvf_solve_minnorm`` / ``_lr`` with scipy.linalg.pinv's default cut-off
      ``max(M, M) * eps * s_max`` (what ``_pinv`` resolves to on the NumPy backend, ``methods/utils.py:11,1435``),
    * ``U @ Coff``                               -> ``mvf_apply``.

    ``PXB_term`` (n x D) is the reference's ``P @ coordsB - RnA * K_NA[:, None]`` of THIS batch (O(n nb) host work that
    belongs to the assignment step, not to this one).

    ``svi`` (the ``SVI_mode`` branch, ``:1269-1275``): ``dict(step_size=, SigmaInv_prev=, PXB_prev=)`` - the running
    averages of the previous batches; ``SigmaInv`` and ``PXB_term`` are blended ``step new + (1 - step) prev`` before the
    solve (``mvf_lincomb3``) and returned for the next call.
    ``guidance`` (the ``guidance_effect in ("nonrigid", "both")`` branch, ``:1282-1288,1293-1294``):
    ``dict(X_AI=, X_BI=, R_AI=, weight=, Sp=)`` - ``U_I = con_K(X_AI, ctrl)``; ``SigmaInv += w U_I^T U_I``,
    ``rhs += w U_I^T (X_BI - R_AI)`` with ``w = sigma2 weight Sp / n_I`` (a second ``mvf_gram`` with unit weights) and
    ``V_AI = U_I Coff`` (``mvf_apply``) is returned too.

    Returns ``{"SigmaInv", "PXB_term", "Coff", "VnA", "SigmaDiag"[, "V_AI"]}`` as host float64; ``SigmaDiag`` =
    ``sigma2 diag(U pinv(SigmaInv) U^T)`` (the n-vector feeding the alignment's variational sigma^2, ``:1295-1297``) comes
    from the decomposition the solve left on the device (``mvf_pinv_diag``).

    ``kernel_type="geodist"`` with ``graph_kernel=`` (what ``st.align.graph_kernel(coordsA, inducing_idx, beta)`` returns; pass
    ``inducing_variables=graph_kernel.inducing_variables``): U and Gamma are the graph kernel's (``morpho_class.py:865-871``)
    instead of con_K of the coordinates.  U is packed once into the Gram kernel's operand cache (``mvf_ublk_pack``) and the four
    consumers read it there: ``mvf_gram_cached``, ``mvf_rhs_cached``, ``mvf_apply_cached``, ``mvf_pinv_diag_cached``.
    ``ValueError`` unless the kernel fits the call (cells, inducing variables, ``beta``); ``guidance`` is refused with it (the
    reference sets ``U_I = None`` in this branch)."""
    if dtype not in ("float32", "float64"):
        raise ValueError("dtype must be 'float32' or 'float64'")
    _kernel_type_argument("update_nonrigid", kernel_type, graph_kernel)
    if graph_kernel is not None:
        _check_graph_kernel(graph_kernel, kernel_type, len(coordsA), len(inducing_variables), beta, "update_nonrigid")
        if guidance is not None:
            raise NotImplementedError("update_nonrigid: guidance pairs have no graph distance to the inducing variables "
                                      "(the reference sets U_I = None with kernel_type='geodist')")
    X = np.asarray(coordsA, dtype=np.float64)
    ctrl = np.asarray(inducing_variables, dtype=np.float64)
    w = np.asarray(K_NA, dtype=np.float64).reshape(-1)
    B = np.asarray(PXB_term, dtype=np.float64)
    if X.ndim != 2 or ctrl.ndim != 2 or X.shape[1] != ctrl.shape[1]:
        raise AssertionError("X and Y do not have the same number of features.")  # con_K's assertion (utils.py:1150)
    if len(w) != len(X) or B.shape[0] != len(X) or B.ndim != 2 or not (1 <= B.shape[1] <= 3):
        raise ValueError("K_NA must be (n,) and PXB_term (n, D) with D <= 3")
    n, m, D = len(X), len(ctrl), B.shape[1]
    k = _rt._make_kernels(device, dtype)
    npdt = np.float32 if dtype == "float32" else np.float64
    center = ctrl.mean(0)
    x4, c4 = k.to_x4(X, center), k.to_x4(ctrl, center)
    f64 = torch.float64
    gk = graph_kernel
    if gk is None:
        Gamma = _consistent_K(k, ctrl, center, float(beta))  # generated like U (see SparseVFCEngine)

        def gram(P, Y, rhs_only=False):
            k.gram(x4, P, k.to_x4(Y), c4, float(beta), G, R, rhs_only=rhs_only)
    else:
        Gamma = k.h2d(np.ascontiguousarray(gk.Gamma, dtype=np.float64))
        k.pack_ublk(gk.device_U(k))

        def gram(P, Y, rhs_only=False):
            if not rhs_only:
                k.gram_on_cache(P, G)
            k.rhs_on_cache(P, k.to_x4(Y), R)
    G, R = k.zeros(m, m, dtype=f64), k.zeros(m, 3, dtype=f64)
    Pw = k.h2d(w.astype(npdt))
    ls2 = float(sigma2) * float(lambdaVF)
    step = 1.0
    if svi is None:
        # rhs = U^T PXB = U^T diag(K_NA) Y with Y = PXB / K_NA (rows with K_NA == 0 have PXB == 0: cells without a partner)
        Y = np.divide(B, w[:, None], out=np.zeros_like(B), where=w[:, None] != 0)
        gram(Pw, Y)
    else:
        step = float(svi["step_size"])
        S_prev = np.ascontiguousarray(svi["SigmaInv_prev"], dtype=np.float64)
        B_prev = np.asarray(svi["PXB_prev"], dtype=np.float64)
        if S_prev.shape != (m, m) or B_prev.shape != B.shape or not (0.0 < step <= 1.0):
            raise ValueError("svi needs 0 < step_size <= 1, SigmaInv_prev (M, M) and PXB_prev shaped like PXB_term")
        B = step * B + (1.0 - step) * B_prev  # the blended n x D term (host, O(n)): rows without a partner NOW may carry
        # the previous batches' share, so its rhs is taken with unit weights
        gram(Pw, np.zeros_like(B))
        ones = torch.ones(n, dtype=Pw.dtype, device=k.device)
        gram(ones, B, rhs_only=True)
        # G <- step G + (1 - step) (SigmaInv_prev);  the regulariser enters the solve as (step ls2) Gamma
        k.lincomb3(G, step, G, 1.0 - step, k.h2d(S_prev))
    x4_I = None
    if guidance is not None:
        X_AI = np.asarray(guidance["X_AI"], dtype=np.float64)
        dXI = np.asarray(guidance["X_BI"], dtype=np.float64) - np.asarray(guidance["R_AI"], dtype=np.float64)
        if X_AI.ndim != 2 or X_AI.shape[1] != X.shape[1] or dXI.shape != X_AI.shape:
            raise ValueError("guidance needs X_AI, X_BI, R_AI of one (n_I, D) shape")
        n_i = len(X_AI)
        wg = float(sigma2) * float(guidance["weight"]) * float(guidance["Sp"]) / n_i
        x4_I = k.to_x4(X_AI, center)
        G_I, R_I = k.zeros(m, m, dtype=f64), k.zeros(m, 3, dtype=f64)
        k.gram(x4_I, torch.ones(n_i, dtype=Pw.dtype, device=k.device), k.to_x4(dXI), c4, float(beta), G_I, R_I)
        k.lincomb3(G, 1.0, G, wg, G_I)
        k.lincomb3(R, 1.0, R, wg, R_I)
    C, rcond, lowrank = _nonrigid_solve(k, G, Gamma, step * ls2, R, indefinite=None if gk is None else {})
    SigmaInv = _rt._d2h(k, G) + step * ls2 * _rt._d2h(k, Gamma)
    # SigmaDiag = sigma2 diag(U pinv(SigmaInv) U^T) (morpho_class.py:1295-1297) from the decomposition the solve left
    if gk is None:
        V4, _ = k.apply(x4, c4, float(beta), C)
        diag = k.pinv_diag(x4, c4, float(beta), rcond=rcond, lowrank=lowrank) if hasattr(k, "pinv_diag") else None
    else:
        V4 = k.apply_on_cache(C)
        diag = k.pinv_diag_cached(rcond=rcond, lowrank=lowrank)
        k.drop_ublk()
    out = {"SigmaInv": SigmaInv, "PXB_term": B, "Coff": _rt._d2h(k, C)[:, :D].copy(),
           "VnA": _rt._d2h(k, V4[:, :D].to(f64))}
    if diag is not None:
        out["SigmaDiag"] = float(sigma2) * _rt._d2h(k, diag)
    if x4_I is not None:
        out["V_AI"] = _rt._d2h(k, k.apply(x4_I, c4, float(beta), C)[0][:, :D].to(f64))
    return out


def BA_transform(vecfld, quary_points, deformation_scale: int = 1, dtype: str = "float64", device=None):
    if dtype not in ("float32", "float64"):
        raise ValueError("dtype must be 'float32' or 'float64'")
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    if vecfld.get("kernel_type", "euc") == "geodist":
        raise ValueError("BA_transform: this vecfld was fitted with kernel_type='geodist' - a new point has no graph distance to "
                         "the inducing variables, and the Euclidean kernel (what the reference evaluates here) is not the fitted "
                         "field; the fitted positions are the loop's XAHat and VnA")
    scale = f(vecfld["norm_dict"]["scale_transformed"])
    mean_ref = f(vecfld["norm_dict"]["mean_fixed"])
    mean_q = f(vecfld["norm_dict"]["mean_transformed"])
    XA = f(quary_points)
    if XA.ndim != 2:
        raise ValueError("quary_points must be (n, d)")
    if vecfld["normalize_c"]:
        XA = (XA - mean_q) / scale
    ctrl = f(vecfld["inducing_variables"])
    if XA.shape[1] != ctrl.shape[1]:  # the reference's con_K assertion (alignment/methods/utils.py:1150)
        raise AssertionError("X and Y do not have the same number of features.")
    field = {"X_ctrl": ctrl, "C": f(vecfld["Coff"]), "beta": float(vecfld["beta"])}
    vel = vector_field_function(XA, field, dtype=dtype, device=device) * deformation_scale
    XA = XA @ f(vecfld["init_R"]).T + f(vecfld["init_t"])
    sim = XA @ f(vecfld["R"]).T + f(vecfld["t"])
    opt = XA @ f(vecfld["optimal_R"]).T + f(vecfld["optimal_t"])
    hat = vel + sim
    if vecfld["normalize_c"]:
        hat = hat * scale + mean_ref
        vel = vel * scale
        opt = opt * scale + mean_ref
    return hat, vel, opt


def _digamma(x):
    """Digamma for a positive float, the formula of mvf_align_alpha's device function (recurrence up to 10, then the
    asymptotic series through x^-14) in Python float64: what gamma's update needs once per iteration."""
    import math

    x = float(x)
    if not x > 0.0:
        raise ValueError("digamma is implemented for positive arguments only")
    s = 0.0
    while x < 10.0:
        s += 1.0 / x
        x += 1.0
    r = 1.0 / x
    r2 = r * r
    p = 1.0 / 12.0
    for c in (-691.0 / 32760.0, 1.0 / 132.0, -1.0 / 240.0, 1.0 / 252.0, -1.0 / 120.0, 1.0 / 12.0):
        p = p * r2 + c
    return ((math.log(x) - 0.5 * r) - p * r2) - s


def _kernel_type_argument(who, kernel_type, graph_kernel):
    """The kernels the loops and update_nonrigid know: 'euc', and 'geodist' when the kernel is handed over built."""
    if kernel_type == "geodist" and graph_kernel is None:
        raise NotImplementedError(f"{who}: kernel_type='geodist' needs graph_kernel=: the kernel is built first, from the indices "
                                  f"of the inducing variables in slice A and the graph (gk = st.align.graph_kernel(coordsA, "
                                  f"inducing_idx, beta)), and handed over with inducing_variables=gk.inducing_variables")
    if kernel_type not in ("euc", "geodist"):
        raise NotImplementedError(f"{who}: kernel_type={kernel_type!r} is not supported (the Euclidean 'euc' kernel, or 'geodist' "
                                  f"with graph_kernel=)")
    if graph_kernel is not None and kernel_type != "geodist":
        raise ValueError(f"{who}: graph_kernel= goes with kernel_type='geodist' (got kernel_type={kernel_type!r})")


def _iterate_arguments(coordsA, coordsB, exp_layers_A, exp_layers_B, dissimilarity, probability_type, probability_parameters,
                       inducing_variables, beta, lambdaVF, sigma2, max_iter, nonrigid_start_iter, kappa, gamma_a, gamma_b,
                       partial_robust_level, sigma2_end, samples_s, inliers, nn_init_weight, dtype, record, SVI_mode, guidance,
                       sparse_calculation_mode, kernel_type, origin, sparse_top_k=1024, label_transfer=None, graph_kernel=None):
    """Validation of morpho_iterate (no device needed).  Returns the arguments as float64 arrays / floats."""
    if dtype not in ("float32", "float64"):
        raise ValueError("dtype must be 'float32' or 'float64'")
    if SVI_mode:
        raise NotImplementedError("morpho_iterate: SVI_mode (stochastic batches of B with blended running averages) is what "
                                  "morpho_iterate_svi runs; this function is the SVI_mode=False loop")
    if guidance is not None and guidance is not False:
        raise NotImplementedError("morpho_iterate: guidance pairs are not supported (update_nonrigid(guidance=) is the stage)")
    _kernel_type_argument("morpho_iterate", kernel_type, graph_kernel)
    top_k = _sparse_top_k(sparse_calculation_mode, sparse_top_k)
    XA, XB, LA, LB, codes, table = _assignment_arguments(coordsA, coordsB, exp_layers_A, exp_layers_B, dissimilarity,
                                                         probability_type, probability_parameters, False, label_transfer)
    NA, D = XA.shape
    if NA == 0 or len(XB) == 0:
        raise ValueError("morpho_iterate: both slices need at least one cell")
    ctrl = np.asarray(inducing_variables, dtype=np.float64)
    if ctrl.ndim != 2 or ctrl.shape[1] != D or len(ctrl) == 0:
        raise AssertionError("X and Y do not have the same number of features.")  # con_K's assertion (utils.py:1150)
    if graph_kernel is not None:
        _check_graph_kernel(graph_kernel, kernel_type, NA, len(ctrl), beta, "morpho_iterate")
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError("max_iter must be a positive integer")
    if record not in (False, True, "arrays"):
        raise ValueError("record must be False, True or 'arrays'")
    if not (float(sigma2) > 0.0 and float(beta) > 0.0 and float(lambdaVF) >= 0.0):
        raise ValueError("sigma2 and beta must be positive and lambdaVF non-negative")
    if not (float(gamma_a) > 0.0 and float(gamma_b) > 0.0 and float(partial_robust_level) > 0.0):
        raise ValueError("gamma_a, gamma_b and partial_robust_level must be positive")
    if isinstance(kappa, (float, int)):
        kap = np.full(NA, float(kappa))
    elif isinstance(kappa, np.ndarray):
        kap = np.asarray(kappa, dtype=np.float64).reshape(-1)
    else:
        raise ValueError("kappa should be a float or a numpy array.")  # morpho_class.py:722
    if len(kap) != NA or not np.all(kap > 0.0):
        raise ValueError("kappa must be positive, a float or one value per A cell")
    inl = None
    if inliers is not None:
        iA, iB, iP = (np.asarray(a, dtype=np.float64) for a in inliers)
        iP = iP.reshape(-1, 1)
        if iA.ndim != 2 or iA.shape != iB.shape or iA.shape[1] != D or len(iP) != len(iA) or len(iA) == 0 or not iP.sum() > 0:
            raise ValueError("inliers must be (inlier_A (k, D), inlier_B (k, D), inlier_P (k,) or (k, 1)) with a positive sum")
        inl = (iA, iB, iP)
    if samples_s is None:  # morpho_class.py:738-741
        samples_s = max(np.prod(XA.max(0) - XA.min(0)), np.prod(XB.max(0) - XB.min(0)))
    if not float(samples_s) > 0.0:
        raise ValueError("samples_s must be positive")
    org = np.zeros(3)
    if origin is not None:
        org[:D] = np.asarray(origin, dtype=np.float64).reshape(D)
    return dict(XA=XA, XB=XB, LA=LA, LB=LB, codes=codes, table=table, ctrl=ctrl, kappa=kap, inliers=inl, samples_s=float(samples_s),
                origin=org, sigma2_end=None if sigma2_end is None else float(sigma2_end), top_k=top_k, graph_kernel=graph_kernel)


def _moved_sums(blk, D, mu_XA, mu_Vn, mu_XB, move_Vn):
    """The block's centred second-order sums moved from the device's means (blk[14:23]) to the means given, through the
    first-order centred sums (exact algebra, include/mvf.h): (sum K_NA xc vc^T, sum xc pc^T) as 3 x 3."""
    dA, dV, dB = np.zeros(3), np.zeros(3), np.zeros(3)
    dA[:D], dB[:D] = mu_XA - blk[14:14 + D], mu_XB - blk[20:20 + D]
    sumK = blk[10]
    c1, c2, c3 = blk[41:44], blk[44:47], blk[47:50]
    M1 = blk[23:32].reshape(3, 3) - np.outer(dA, c2)
    if move_Vn:
        dV[:D] = mu_Vn - blk[17:17 + D]
        M1 = M1 - np.outer(c1, dV) + np.outer(dA, dV) * sumK
    M2 = blk[32:41].reshape(3, 3) - np.outer(dA, c3) - np.outer(c1, dB) + np.outer(dA, dB) * sumK
    return M1, M2


def _rigid_from_block(blk, D, sigma2, inliers, nn_init_weight, R_prev, update_R, Sp_blend=None, step=1.0, t_prev=None):
    """`_update_rigid` (morpho_class.py:1300-1408) from the block of mvf_align_moments, in host float64: the means, the
    D x D matrix ``A``, its SVD, R and t.  The block's second-order sums are centred on the device's means (K_NA . coordsA /
    Sp, ...); with inliers the reference's means move by the O(pairs) inlier terms, and the sums are moved with them through
    the first-order centred sums (exact algebra, include/mvf.h).  The reference's ``mu_XB += ...`` acts in place on the
    arrays its translation reads afterwards (``mu_XB`` IS ``PXB`` there): the translation's numerator is formed from the
    augmented sums, as there.

    ``Sp_blend`` (SVI): the running ``Sp`` that the reference divides this batch's sums by (``:1321, 1339-1341, 1382``) and
    weighs the inliers with - the means differ from the device's by ``Sp_now / Sp_blend``, the same move with another
    ``mu`` (and ``mu_Vn`` moves too); ``step < 1`` blends R before the translation reads it and t afterwards
    (``:1375-1376, 1399-1400``)."""
    svi = Sp_blend is not None
    Sp = Sp_blend if svi else blk[9]
    PXA, PVA, PXB = blk[0:D].copy(), blk[3:3 + D].copy(), blk[6:6 + D].copy()
    deno = Sp
    w = 0.0
    if inliers is not None:
        iA, iB, iP = inliers
        w = sigma2 * nn_init_weight * Sp / iP.sum()
        PXB = PXB + w * (iP.T @ iB)[0]
        PXA = PXA + w * (iP.T @ iA)[0]
        deno = Sp + w * iP.sum()
    mu_XB, mu_XA = PXB / deno, PXA / deno
    if svi or inliers is not None:
        M1, M2 = _moved_sums(blk, D, mu_XA, PVA / Sp, mu_XB, svi)
    else:  # (the device's means ARE the reference's: the same sums and the same division)
        M1, M2 = blk[23:32].reshape(3, 3), blk[32:41].reshape(3, 3)
    A = -((M1 - M2)[:D, :D]).T
    if inliers is not None:
        A = A - w * ((iA - mu_XA) * iP).T.dot(-(iB - mu_XB)).T
    svdU, _, svdV = np.linalg.svd(A)
    C = np.eye(D)
    C[-1, -1] = np.linalg.det(svdU @ svdV)
    R = (svdU @ C @ svdV) if update_R else R_prev
    if svi and update_R and step < 1:
        R = step * R + (1 - step) * R_prev
    t_num = PXB - PVA - PXA @ R.T
    if inliers is not None:
        t_num = t_num + w * (iP.T @ (iB - iA @ R.T))[0]
    t = t_num / deno
    if svi and step < 1:
        t = step * t + (1 - step) * t_prev
    return R, t


def _optimal_from_block(blk, D, Sp_blend=None):
    """`_get_optimal_R` (:1437-1469) from a block: A = (sum xc pc^T)^T on the means K_NA . coordsA / Sp, K_NB . coordsB / Sp -
    the device's, or (SVI without the final full assignment) the last batch's sums over the running ``Sp``."""
    if Sp_blend is None:
        mu_XnA, mu_XnB = blk[14:14 + D], blk[20:20 + D]
        M2 = blk[32:41].reshape(3, 3)
    else:
        mu_XnA, mu_XnB = blk[0:D] / Sp_blend, blk[6:6 + D] / Sp_blend
        _, M2 = _moved_sums(blk, D, mu_XnA, None, mu_XnB, False)
    svdU, _, svdV = np.linalg.svd(M2[:D, :D].T)
    C = np.eye(D)
    C[-1, -1] = np.linalg.det(svdU @ svdV)
    optimal_R = svdU @ C @ svdV
    return optimal_R, mu_XnB - mu_XnA @ optimal_R.T


def _embed(R, t):
    """D x D rotation and D translation as the 3 x 3 / 3 the kernels take (2-D data: the third axis untouched)."""
    R3, t3 = np.eye(3), np.zeros(3)
    D = len(t)
    R3[:D, :D], t3[:D] = R, t
    return R3, t3


def morpho_iterate(coordsA, coordsB, exp_layers_A, exp_layers_B, *, dissimilarity, probability_type, probability_parameters,
                   inducing_variables, beta, lambdaVF, sigma2, max_iter, nonrigid_start_iter=0, kappa=1.0, gamma_a=1.0,
                   gamma_b=1.0, partial_robust_level=10, sigma2_end=None, samples_s=None, inliers=None, nn_init_weight=1.0,
                   update_R=True, dtype: str = "float64", device=None, record=True, origin=None, SVI_mode=False, guidance=None,
                   sparse_calculation_mode=False, kernel_type="euc", sparse_top_k=1024, label_transfer=None, return_P=False,
                   optimal_mapping=False, apply=None, graph_kernel=None):
    """The iteration loop of Spateo's pairwise alignment on the MI355X: the non-SVI, dense-path body of
    ``Morpho_pairwise.run`` (``spateo/alignment/methods/morpho_class.py:280-294``: assignment -> gamma -> alpha -> non-rigid
    -> rigid -> ``XAHat`` -> sigma2) for ``max_iter`` iterations from the state ``_initialize_variational_variables`` sets
    (``:700-747``: alpha = 1, gamma = 0.5, ``VnA = 0``, ``XAHat = RnA = coordsA``, ``SigmaDiag = 0``, R = I, ``sigma2_variance``
    from 1 towards ``partial_robust_level`` by ``_get_anneling_factor`` over 100 iterations), followed by ``_get_optimal_R``
    (``:1437-1469``) and the ``vecfld`` of ``_wrap_output`` (``:1507-1528``, ``normalize_c=False``).

    Both slices' layers are uploaded and prepared once; between the first upload and the result nothing of size NA or NB
    crosses the link.  Per iteration the device runs ``mvf_assign``, ``mvf_align_transform``, the non-rigid update's
    ``mvf_gram`` / ``mvf_solve_minnorm`` / ``mvf_apply`` / ``mvf_pinv_diag`` (from iteration ``nonrigid_start_iter + 1`` on, as
    ``:289``), ``mvf_align_moments`` and ``mvf_align_alpha``; the host reads one block of 64 float64 (page-locked) next to
    the solve's status words and does, in float64, the 3 x 3 SVD, gamma with its clamp to [0.01, 0.99] (``:1220-1224``),
    sigma2 with its floors 1e-3 and, below iteration 100, 1e-2 (``:1426-1435``), and ``sigma2_variance``.

    ``coordsA`` (NA, D) / ``coordsB`` (NB, D), D in {2, 3}, as the caller has normalised them; layers, ``dissimilarity``,
    ``probability_type``, ``probability_parameters`` and ``label_transfer`` (for ``"label"`` layers: 1-D integer label arrays, prepared
    once with the other layers) as ``update_assignment`` takes them; ``inducing_variables`` (M, D) and
    ``beta`` as ``update_nonrigid``; ``sigma2`` the initial value (``_init_guess_sigma2`` in the reference).  Defaults are the
    reference constructor's (``morpho_class.py:133-152``: ``nn_init_weight=1.0``, ``gamma_a = gamma_b = 1.0``, ``kappa=1.0``,
    ``partial_robust_level=10``); ``kappa`` is a float or an (NA,) array; ``samples_s`` defaults to the larger bounding-box
    volume (``:738-741``).  ``inliers = (inlier_A, inlier_B, inlier_P)``: the pairs of the coarse alignment (``nn_init``);
    their terms of ``_update_rigid`` (``:1328-1337, 1352-1368, 1390-1396``) are O(pairs) host float64 work.
    ``sigma2_end`` replaces sigma2 after the loop (``:296-297``).  ``origin`` (D,), optional and not in the reference: a point
    near the data that the coordinates handed to the assignment kernel are taken relative to - distances are formed as
    |x|^2 + |y|^2 - 2 x.y, which loses digits when both slices sit far from the origin; None leaves the operands as
    ``update_assignment`` has them.  ``record``: True keeps per-iteration ``sigma2``, ``gamma``, ``R``, ``t``, ``Sp`` in
    ``history``; ``"arrays"`` (debugging: it crosses the link every iteration) also ``alpha``, ``XAHat``, ``VnA``, ``K_NA``,
    ``Coff``.

    ``sparse_calculation_mode=True`` with ``1 <= sparse_top_k <= 64``: every iteration's assignment keeps the ``sparse_top_k``
    largest entries of each column of ``P`` (``mvf_assign_topk`` in place of ``mvf_assign``, as ``update_assignment`` describes
    it); nothing else of the iteration changes, the other updates read ``K_NA``, ``K_NB``, ``PXB`` and the scalars.  The result
    gains ``P``, the last assignment's, as a ``scipy.sparse.coo_matrix`` (NA, NB).

    ``return_P=True`` (the dense path only; ``ValueError`` with ``sparse_calculation_mode`` and above
    ``RETURN_P_MAX_ENTRIES`` entries): the last iteration's assignment runs through ``mvf_assign_dense`` and the result gains
    its ``P`` (NA, NB), the reference's ``self.P`` after ``run()``.  Every other output keeps its bits.

    ``optimal_mapping=True`` (dense and sparse mode, any size): the last iteration's assignment is followed by
    ``mvf_assign_best`` on the same device operands and state, and the result gains ``best`` - host ``rows`` (NA, 2) / ``cols``
    (NB, 2) int32 and ``row_values`` / ``col_values`` float64, the best partner of every cell in the last assignment's DENSE
    ``P`` under both tie rules; ``mapping_from_best(best, XAHat, coordsB, keep_all)`` makes the reference's two mapping dicts
    of it.  Every other output keeps its bits.

    ``apply=dict(features_A=, features_B=, normalize=True)`` (features as ``apply_assignment`` takes them, validated before
    anything runs): the last iteration's assignment is followed by ``mvf_assign_apply`` on the same device operands and state,
    and the result gains ``applied``, ``apply_assignment``'s dict for that assignment.  With ``sparse_calculation_mode`` the kept
    entries are applied instead: the returned ``coo_matrix`` times the features, on the host.  Every other output keeps its bits.

    Not supported (``NotImplementedError``): ``SVI_mode`` (``morpho_iterate_svi`` runs it), ``guidance``,
    ``sparse_calculation_mode`` with ``sparse_top_k`` above 64 (the default, 1024, is the reference constructor's,
    ``morpho_class.py:140``), ``kernel_type="geodist"`` without ``graph_kernel=`` (and any ``kernel_type`` but these two), and what
    ``update_assignment`` / ``update_nonrigid`` refuse (more than 4 layers, D outside {2, 3}).

    ``kernel_type="geodist", graph_kernel=gk`` with ``gk = st.align.graph_kernel(coordsA, inducing_idx, beta)`` and
    ``inducing_variables=gk.inducing_variables``: the non-rigid field's kernel is ``exp(-beta D^2)`` of the shortest-path distance
    through a k-nearest-neighbour graph of slice A (``morpho_class.py:865-871``) - the kernel for folded tissue, where two cells
    close in space lie far apart along the tissue.  The loop receives the inducing variables as coordinates, the geodesic kernel
    needs their indices in slice A and the graph, so it is built first and handed over.  ``gk.U`` is packed once into the Gram
    kernel's operand cache (``mvf_ublk_pack``) and read there by ``mvf_gram_cached``, ``mvf_rhs_cached``, ``mvf_apply_cached`` and
    ``mvf_pinv_diag_cached``; ``gk.Gamma`` is the regulariser; nothing else of the loop changes, and without ``graph_kernel`` every
    launch is as before.  ``ValueError`` unless ``kernel_type="geodist"``, ``len(gk.U) == NA``, one inducing variable per column and
    ``gk.beta == beta``.  The returned ``vecfld`` carries ``kernel_type="geodist"`` and ``BA_transform`` refuses it (a new point has
    no graph distance): the fitted positions are ``XAHat`` and ``VnA``.

    Returns a dict of host float64: ``R``, ``t``, ``Coff``, ``VnA``, ``RnA``, ``XAHat``, ``optimal_R``, ``optimal_t``,
    ``optimal_RnA``, ``sigma2``, ``gamma``, ``alpha``, ``SigmaDiag``, ``sigma2_variance``, the last assignment's ``K_NA``,
    ``K_NB``, ``K_NA_spatial``, ``K_NA_sigma2``, ``Sp``, ``Sp_spatial``, ``Sp_sigma2``, ``history`` (if recorded) and
    ``vecfld``: ``BA_transform(vecfld, coordsA)`` reproduces ``XAHat`` and ``optimal_RnA``.  Two calls give equal bits."""
    a = _iterate_arguments(coordsA, coordsB, exp_layers_A, exp_layers_B, dissimilarity, probability_type,
                           probability_parameters, inducing_variables, beta, lambdaVF, sigma2, max_iter, nonrigid_start_iter,
                           kappa, gamma_a, gamma_b, partial_robust_level, sigma2_end, samples_s, inliers, nn_init_weight, dtype,
                           record, SVI_mode, guidance, sparse_calculation_mode, kernel_type, origin, sparse_top_k, label_transfer,
                           graph_kernel)
    return_P = _return_P_argument(return_P, a["top_k"], len(a["XA"]), len(a["XB"]))
    apply = _apply_argument(apply, len(a["XA"]), len(a["XB"]), "morpho_iterate")
    return _iterate(a, dissimilarity, beta, lambdaVF, sigma2, max_iter, nonrigid_start_iter, gamma_a, gamma_b,
                    partial_robust_level, nn_init_weight, update_R, dtype, device, record, return_P=return_P,
                    best=bool(optimal_mapping), apply=apply)


def _return_P_argument(return_P, top_k, NA, NB_last):
    """``return_P`` of the loops, validated: the dense P of the last assignment (NA x NB_last) excludes the top-k mode and
    is capped like update_assignment's."""
    if not return_P:
        return False
    if top_k is not None:
        raise ValueError("return_P=True (the dense P) and sparse_calculation_mode=True (P as a scipy.sparse.coo_matrix) "
                         "exclude each other")
    if NA * NB_last > RETURN_P_MAX_ENTRIES:
        raise ValueError(f"return_P=True materialises {NA} x {NB_last} = {NA * NB_last} entries; the cap is "
                         f"{RETURN_P_MAX_ENTRIES} (align.RETURN_P_MAX_ENTRIES)")
    return True


def _iterate(a, dissimilarity, beta, lambdaVF, sigma2, max_iter, nonrigid_start_iter, gamma_a, gamma_b, partial_robust_level,
             nn_init_weight, update_R, dtype, device, record, svi=None, return_P=False, best=False, apply=None):
    """The loop of morpho_iterate and, with ``svi = dict(batch_size=, batch_perm= (int32, validated), return_mapping=)``, of
    morpho_iterate_svi, on validated arguments ``a`` (_iterate_arguments).  ``return_P``: the LAST assignment executed - the
    last iteration's, or the closing full one - runs through mvf_assign_dense.  ``best``: the same assignment is followed by
    mvf_assign_best on its operands, before the iteration moves them on.  ``apply`` (_apply_argument): and, on the dense
    path, by mvf_assign_apply there; in the top-k mode the kept entries are applied on the host."""
    XA, XB, ctrl, org, top_k = a["XA"], a["XB"], a["ctrl"], a["origin"], a["top_k"]
    NA, D = XA.shape
    NB, m = len(XB), len(ctrl)
    beta, lambdaVF, sigma2, samples_s = float(beta), float(lambdaVF), float(sigma2), a["samples_s"]
    k = _rt._make_kernels(device, dtype)
    f64 = torch.float64
    ph = _rt._Phases(k.device)   # {setup, assign, nonrigid, glue, result: seconds} in last_fit_profile() under PROFILE_FITS
    # ---- uploaded / built once ----
    layers = _prepare_layers(k, a["LA"], a["LB"], a["codes"], a["table"])
    has_origin = bool(np.any(org != 0.0))
    xa4 = k.to_x4(XA, org[:D] if has_origin else None)       # XAHat of iteration 0 = coordsA, as update_assignment uploads it
    xb4 = k.to_x4(XB, org[:D] if has_origin else None)
    A64, B64 = k.h2d_padded(XA, 3, f64), k.h2d_padded(XB, 3, f64)
    center = ctrl.mean(0)
    x4c, c4 = k.to_x4(XA, center), k.to_x4(ctrl, center)     # what the Gram / apply / pinv_diag kernels read (update_nonrigid)
    gk = a.get("graph_kernel")
    if gk is None:
        Gamma = _consistent_K(k, ctrl, center, beta)
    else:                                                      # U along the tissue: packed once, read from the cache below
        Gamma = k.h2d(np.ascontiguousarray(gk.Gamma, dtype=np.float64))
        k.pack_ublk(gk.device_U(k))
    ladder = None if gk is None else {}                        # the shift of the last solve that worked (_nonrigid_solve)
    kap = k.h2d(a["kappa"])
    # ---- the state that stays on the device ----
    alpha, model_mul = (torch.ones(NA, dtype=f64, device=k.device) for _ in range(2))   # alpha = 1, SigmaDiag = 0 (:723, :734)
    SigmaDiag = k.zeros(NA, dtype=f64)
    V4 = k.zeros(NA, 4)
    Y4, Pw = k.empty(NA, 4), k.empty(NA)
    Pw_dtype = Pw.dtype
    RnA, XAHat, PXB_term = k.empty(NA, 3, dtype=f64), k.empty(NA, 3, dtype=f64), k.empty(NA, 3, dtype=f64)
    if svi is not None:
        # the batch schedule (:894-896) follows from the initial permutation: batch_idx[j] = perm[(j - it bs) mod NB]; the
        # permutation is uploaded once and every batch is gathered on the device into these buffers
        bs, NB_eff = int(svi["batch_size"]), int(svi["batch_size"])
        perm = k.h2d(svi["batch_perm"])
        xb4_b, B64_b = k.empty(bs, 4), k.empty(bs, 3, dtype=f64)
        # (a label layer has no rows per B cell: its batch is the gathered labels b alone)
        Yp_b = [None if L.is_label else k.empty(bs, L.ld) for L in layers]
        b_b = [k.empty(bs, dtype=f64) for L in layers]
        layers_b = [L.with_columns(Yb, bb) for L, Yb, bb in zip(layers, Yp_b, b_b)]
        PXB_term.zero_()                                       # the running PXB_term and SigmaInv start at 0 (:759-760)
        S_run = k.zeros(m, m, dtype=f64)
        ones = torch.ones(NA, dtype=Pw_dtype, device=k.device)
        Sp_run = Sp_spatial_run = Sp_sigma2_run = 0.0
        xb_cur, layers_cur, B_cur = xb4_b, layers_b, B64_b     # the B operands of every iteration: the batch buffers
    else:
        NB_eff = NB
        xb_cur, layers_cur, B_cur = xb4, layers, B64
    step = 1.0
    G, Rhs = k.zeros(m, m, dtype=f64), k.zeros(m, 3, dtype=f64)
    Coff = k.zeros(m, 3, dtype=f64)
    block = k.empty(_lib.ALIGN_MOMENT_DOUBLES, dtype=f64)
    R, t = np.eye(D), np.zeros(D)
    gamma, sigma2_variance = 0.5, 1.0
    variance_step = float(np.power(float(partial_robust_level) / 1.0, 1.0 / 100))  # _get_anneling_factor (utils.py:1357-1365)
    nonrigid = False
    history = {q: [] for q in ("sigma2", "gamma", "R", "t", "Sp") + (("step_size",) if svi is not None else ())}
    if record == "arrays":
        history.update({q: [] for q in ("alpha", "XAHat", "VnA", "K_NA", "Coff")})
    R3, t3 = _embed(R, t)
    k.align_transform(A64, V4, None, None, R3, t3, RnA=RnA, XAHat=XAHat)
    dev = blk = None
    extras = {}                                                # best / applied of the last assignment executed
    if apply is not None and top_k is None:                    # the features go up once, with the layers
        FA_dev = None if apply["FA"] is None else k.h2d(apply["FA"])
        FB_dev = None if apply["FB"] is None else k.h2d(apply["FB"])

    def assignment(xb, lay, last):
        """One assignment on the B operands given, at the state as it is now; the ``last`` one executed carries the extras."""
        common = (xa4, xb, lay, model_mul, sigma2, sigma2_variance, _spatial_outlier(sigma2, gamma, samples_s, NA, D))
        dev = k.assign_topk(*common, top_k) if top_k is not None else k.assign(*common, dense=last and bool(return_P))
        if last and best:                                      # on the operands of the assignment itself
            extras["best"] = k.assign_best(*common)
        if last and apply is not None and top_k is None:
            # the features cover the WHOLE B slice, never a batch: the SVI loop applies after its closing full assignment
            extras["applied"] = k.assign_apply(xa4, xb4, layers, *common[3:], features_B=FB_dev, features_A=FA_dev)
        return dev

    def moments(dev, B):
        """The block of reductions of an assignment over the B rows it saw: the one host read, 64 float64, page-locked."""
        k.align_moments(A64, V4, dev["K_NA"], dev["K_NA_spatial"], dev["K_NA_sigma2"], SigmaDiag, dev["PXB"], B, dev["K_NB"],
                        block, origin=org, extra=dev["scalars"])
        return np.array(k.to_host([block])[0], dtype=np.float64)

    def field_and_variance(Coff, rcond, lowrank):
        """After the solve, in both modes: V4 = U Coff, SigmaDiag = sigma2 diag(U pinv(SigmaInv) U^T)  (:1296).  (Coff, V4)."""
        if gk is None:
            V4, _ = k.apply(x4c, c4, beta, Coff)
            diag = k.pinv_diag(x4c, c4, beta, rcond=rcond, lowrank=lowrank)
        else:
            V4 = k.apply_on_cache(Coff)
            diag = k.pinv_diag_cached(rcond=rcond, lowrank=lowrank)
        k.lincomb3(SigmaDiag, sigma2, diag)
        return Coff, V4

    def gram(P, tiles_only=False, rhs_only=False):
        """G = U^T diag(P) U and / or Rhs = U^T diag(P) Y4: U regenerated from the coordinates, or read from the packed cache."""
        if gk is None:
            k.gram(x4c, P, Y4, c4, beta, G, Rhs, tiles_only=tiles_only, rhs_only=rhs_only)
            return
        if not rhs_only:
            k.gram_on_cache(P, G)
        if not tiles_only:
            k.rhs_on_cache(P, Y4, Rhs)

    ph.mark("setup")
    closing = svi is not None and svi["return_mapping"]       # a full assignment follows the loop
    for it in range(int(max_iter)):
        if svi is not None:
            step = min(1.0, 10.0 / (it + 1.0))                 # :894, SVI_deacy = 10
            k.align_gather(perm, (-it * bs) % NB, bs, xb4, B64, layers, xb4_b, B64_b, Yp_b, b_b)
        dev = assignment(xb_cur, layers_cur, last=not closing and it == int(max_iter) - 1)
        ph.mark("assign")
        if it > nonrigid_start_iter or nonrigid:               # morpho_class.py:289
            nonrigid = True
            if svi is not None:
                # PXB_term <- step (P coordsB[batch] - RnA K_NA) + (1 - step) PXB_term; rows without a partner in THIS batch keep
                # the earlier batches' share, so the right-hand side is U^T PXB_term with unit weights (:1270-1279)
                k.align_transform_svi(RnA, dev["PXB"], dev["K_NA"], step, PXB_term, Y4, Pw, origin=org)
                gram(Pw, tiles_only=True)
                gram(ones, rhs_only=True)
                # SigmaInv <- step (sigma2 lambdaVF Gamma + U^T diag(K_NA) U) + (1 - step) SigmaInv (:1273): G takes the blend
                # without the regulariser, which enters the solve as (step sigma2 lambdaVF) Gamma and the stored value after it
                k.lincomb3(G, step, G, 1.0 - step, S_run)
                solved = _nonrigid_solve(k, G, Gamma, step * sigma2 * lambdaVF, Rhs, indefinite=ladder)
                k.lincomb3(S_run, 1.0, G, step * sigma2 * lambdaVF, Gamma)
            else:
                # PXB_term = P coordsB - RnA K_NA with the RnA of the previous iteration's R, t; Y = PXB_term / K_NA; Pw = K_NA
                k.align_transform(A64, V4, dev["PXB"], dev["K_NA"], R3, t3, origin=org, PXB_term=PXB_term, Y4=Y4, Pw=Pw)
                gram(Pw)
                solved = _nonrigid_solve(k, G, Gamma, sigma2 * lambdaVF, Rhs, indefinite=ladder)
            Coff, V4 = field_and_variance(*solved)
            ph.mark("nonrigid")
        blk = moments(dev, B_cur)
        Sp, Sp_spatial, Sp_sigma2 = float(blk[9]), float(blk[11]), float(blk[12])
        if svi is not None:                                    # :1178-1181
            Sp_run = Sp = step * Sp + (1 - step) * Sp_run
            Sp_spatial_run = Sp_spatial = step * Sp_spatial + (1 - step) * Sp_spatial_run
            Sp_sigma2_run = Sp_sigma2 = step * Sp_sigma2 + (1 - step) * Sp_sigma2_run
        if not (Sp > 0.0 and Sp_sigma2 > 0.0 and np.isfinite(blk).all()):
            raise _lib.MVFError(f"morpho_iterate: iteration {it}: the assignment is empty or not finite (Sp = {Sp}, Sp_sigma2 = "
                                f"{Sp_sigma2}): no B cell lies within reach of the A slice at sigma2 = {sigma2}")
        gamma = float(np.exp(_digamma(gamma_a + Sp_spatial) - _digamma(gamma_a + gamma_b + NB_eff)))   # :1214-1222
        gamma = max(min(gamma, 0.99), 0.01)
        R, t = _rigid_from_block(blk, D, sigma2, a["inliers"], float(nn_init_weight), R, update_R,
                                 Sp_blend=None if svi is None else Sp, step=step, t_prev=t)
        R3, t3 = _embed(R, t)
        k.align_transform(A64, V4, None, None, R3, t3, origin=org, RnA=RnA, XAHat=XAHat, xa4=xa4)
        sigma2_related = float(blk[50]) / (D * Sp_sigma2)     # :1200
        sigma2 = max(sigma2_related + float(blk[13]) / Sp_sigma2, 1e-3)                            # :1426-1429
        sigma2_variance = min(sigma2_variance * variance_step, float(partial_robust_level))        # :1431-1433
        if it < 100:
            sigma2 = max(sigma2, 1e-2)
        # alpha of this iteration (:1250-1252) and the NEXT assignment's model_mul, which needs this iteration's sigma2
        if svi is None:
            k.align_alpha(kap, dev["K_NA_spatial"], SigmaDiag, Sp_spatial, sigma2, alpha, model_mul)
        else:                                                  # :1240-1247, with the blended Sp_spatial
            k.align_alpha_svi(kap, dev["K_NA_spatial"], SigmaDiag, Sp_spatial, sigma2, step, alpha, model_mul)
        ph.mark("glue")
        if record:
            for q, v in (("sigma2", sigma2), ("gamma", gamma), ("R", R.copy()), ("t", t.copy()), ("Sp", Sp)):
                history[q].append(v)
            if svi is not None:
                history["step_size"].append(step)
        if record == "arrays":
            h = k.to_host([alpha, XAHat, V4, dev["K_NA"], Coff], own_pinned=False)
            for q, v in zip(("alpha", "XAHat", "VnA", "K_NA", "Coff"), h):
                history[q].append(np.array(v[:, :D] if v.ndim == 2 else v, dtype=np.float64))
    if a["sigma2_end"] is not None:
        sigma2 = a["sigma2_end"]
    if svi is not None and svi["return_mapping"]:
        # the full, non-SVI assignment on the final state (:300-302): K_NA, K_NB and the Sp* of the whole B slice, unblended
        if a["sigma2_end"] is not None:                        # model_mul of :1087 with the replaced sigma2: once, on the host
            al, sd = k.to_host([alpha, SigmaDiag], own_pinned=False)
            model_mul = k.h2d(np.array(al, dtype=np.float64) * np.exp(-np.array(sd, dtype=np.float64) / sigma2))
        dev = assignment(xb4, layers, last=True)
        blk = moments(dev, B64)
        Sp_run, Sp_spatial_run, Sp_sigma2_run = float(blk[9]), float(blk[11]), float(blk[12])
        if not (Sp_run > 0.0 and np.isfinite(blk).all()):
            raise _lib.MVFError(f"morpho_iterate_svi: the final full assignment is empty or not finite (Sp = {Sp_run})")
    # ---- _get_optimal_R (:1437-1469) from the last block: A = (sum xc pc^T)^T on the device's means, or (SVI, last batch) on
    # the batch's sums over the running Sp ----
    optimal_R, optimal_t = _optimal_from_block(blk, D, None if svi is None or svi["return_mapping"] else Sp_run)
    oRnA = k.empty(NA, 3, dtype=f64)
    k.align_transform(A64, None, None, None, *_embed(optimal_R, optimal_t), RnA=oRnA)
    names = ("K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2")
    host = k.to_host([RnA, XAHat, V4, oRnA, Coff, alpha, SigmaDiag] + [dev[q] for q in names], own_pinned=False)
    out = {q: np.array(v[:, :D], dtype=np.float64) for q, v in zip(("RnA", "XAHat", "VnA", "optimal_RnA", "Coff"), host)}
    out.update({q: np.array(v, dtype=np.float64) for q, v in zip(("alpha", "SigmaDiag") + names, host[5:])})
    out.update(R=R, t=t, optimal_R=optimal_R, optimal_t=optimal_t, sigma2=sigma2, gamma=gamma, sigma2_variance=sigma2_variance,
               Sp=float(blk[9]), Sp_spatial=float(blk[11]), Sp_sigma2=float(blk[12]))
    if svi is not None:
        out.update(Sp=Sp_run, Sp_spatial=Sp_spatial_run, Sp_sigma2=Sp_sigma2_run, batch_size=bs,
                   batch_perm=np.array(svi["batch_perm"], dtype=np.int64), step_size=step)
    if top_k is not None and (svi is None or svi["return_mapping"]):   # the mapping: the last (full) assignment's sparse P
        rows, vals = k.to_host([dev["rows"], dev["vals"]], own_pinned=False)
        out["P"] = _coo_from_lists(rows, vals, NA)
    if return_P:
        out["P"] = np.array(k.to_host([dev["P"]], own_pinned=False)[0], dtype=np.float64)
    if best:
        out["best"] = _best_to_host(k, extras["best"])
    if apply is not None:
        if top_k is None:
            out["applied"] = _applied_to_host(k, extras["applied"], apply["normalize"])
        else:
            out["applied"] = _applied_from_coo(out["P"], out["K_NA"], out["K_NB"], apply["FA"], apply["FB"], apply["normalize"])
    if record:
        out["history"] = {q: np.array(v) for q, v in history.items()}
    ph.mark("result")
    ph.done()
    out["vecfld"] = {
        "R": R, "t": t, "optimal_R": optimal_R, "optimal_t": optimal_t, "init_R": np.eye(D), "init_t": np.zeros(D), "beta": beta,
        "Coff": out["Coff"], "inducing_variables": ctrl, "normalize_scales": None, "normalize_means": None, "normalize_c": False,
        "dissimilarity": list(dissimilarity) if isinstance(dissimilarity, (list, tuple)) else dissimilarity, "sigma2": sigma2,
        "gamma": gamma, "NA": NA, "sigma2_variance": sigma2_variance, "method": "Spateo",
        "norm_dict": {"mean_transformed": np.zeros(D), "mean_fixed": np.zeros(D), "scale": 1.0, "scale_transformed": 1.0,
                      "scale_fixed": 1.0},
        "kernel_type": "euc" if gk is None else "geodist",
    }
    if gk is not None:
        k.drop_ublk()
    return out


def _svi_batch_size(NB, batch_size=None):
    """The reference's rule (morpho_class.py:753-756): a tenth of the B slice, at least 1000 cells, at most all of them."""
    if batch_size is None:
        return min(max(int(NB / 10), 1000), NB)
    if int(batch_size) != batch_size or batch_size < 1:
        raise ValueError("batch_size must be a positive integer")
    return min(int(batch_size), NB)


def _svi_schedule(batch_perm, batch_size, it):
    """batch_idx of iteration ``it`` (:895-896: the head of the permutation, which is then rolled by batch_size):
    ``batch_perm[(j - it batch_size) mod NB]``, j < batch_size - what mvf_align_gather reads with start = (-it bs) mod NB."""
    perm = np.asarray(batch_perm)
    return perm[(np.arange(batch_size) - it * batch_size) % len(perm)]


def _svi_arguments(NB, batch_size, batch_perm, seed):
    """Validation of morpho_iterate_svi's own arguments (no device needed): (batch_size, batch_perm as int32).  The kernel
    reads row batch_perm[.] of every B array unchecked, so the permutation is proven here, before any launch."""
    if NB >= 1 << 31:
        raise ValueError("morpho_iterate_svi: the B slice must have fewer than 2^31 cells")
    bs = _svi_batch_size(NB, batch_size)
    if batch_perm is None:
        perm = np.random.default_rng(seed).permutation(NB)
    else:
        perm = np.asarray(batch_perm)
        if perm.ndim != 1 or len(perm) != NB or perm.dtype.kind not in "iu":
            raise ValueError(f"batch_perm must be a 1-D integer array with one entry per B cell ({NB})")
        if perm.min() < 0 or perm.max() >= NB or not np.array_equal(np.sort(perm), np.arange(NB)):
            raise ValueError("batch_perm must be a permutation of range(NB): every index exactly once")
    return bs, np.ascontiguousarray(perm, dtype=np.int32)


def morpho_iterate_svi(coordsA, coordsB, exp_layers_A, exp_layers_B, *, dissimilarity, probability_type, probability_parameters,
                       inducing_variables, beta, lambdaVF, sigma2, max_iter, nonrigid_start_iter=0, kappa=1.0, gamma_a=1.0,
                       gamma_b=1.0, partial_robust_level=10, sigma2_end=None, samples_s=None, inliers=None, nn_init_weight=1.0,
                       update_R=True, dtype: str = "float64", device=None, record=True, origin=None, batch_size=None,
                       batch_perm=None, seed=None, return_mapping=False, guidance=None, sparse_calculation_mode=False,
                       kernel_type="euc", sparse_top_k=1024, label_transfer=None, return_P=False, optimal_mapping=False, apply=None,
                       graph_kernel=None):
    """The SVI mode of the same loop - the reference constructor's default, ``SVI_mode=True``
    (``spateo/alignment/methods/morpho_class.py:136, 283-284, 749-760, 894-896``): every iteration sees ``batch_size`` cells
    of the B slice and blends what it learns into running averages with ``step_size = min(1, 10 / (iter + 1))``.

    ``batch_size``: None takes the reference's rule ``min(max(int(NB / 10), 1000), NB)``, a number is capped at NB.
    ``batch_perm``: the initial permutation of ``range(NB)`` (``ValueError`` unless every index occurs exactly once); None
    draws one from ``np.random.default_rng(seed)``.  Iteration ``it`` takes ``batch_perm[(j - it batch_size) mod NB]``,
    ``j < batch_size`` - the reference's head-then-``roll``.  Everything else as ``morpho_iterate`` takes it.

    What differs from the dense loop, per iteration: the assignment runs on NA x the batch (``mvf_align_gather`` copies the
    batch's rows of the coordinates and of every prepared B layer - of a ``"label"`` layer the B labels - on the device,
    ``mvf_assign`` follows); ``Sp``,
    ``Sp_spatial``, ``Sp_sigma2`` are blended (``:1178-1181``) and divide this batch's sums in ``_update_rigid`` and
    ``_update_sigma2``; gamma counts ``batch_size`` cells (``:1214-1218``); alpha (``mvf_align_alpha_svi``, ``:1240-1247``),
    ``PXB_term`` (``mvf_align_transform_svi``) and ``SigmaInv`` (``mvf_lincomb3``, on the device) are blended with their
    running values, which start at zero (``:758-760``) - also when the first non-rigid update comes at ``iter >= 10``, as in
    the reference; R and t are blended once ``step_size < 1`` (``:1375-1376, 1399-1400``), so ``R`` is no rotation then.
    The host reads the same one block of 64 float64 per iteration; nothing of size NA, NB or ``batch_size`` crosses the link
    between the first upload and the result.  After the loop ``sigma2_end`` replaces sigma2; ``return_mapping=True`` runs
    one full, non-SVI assignment on the final state (``:300-302``), whose ``K_NA``, ``K_NB`` (NB,) and unblended ``Sp*`` are
    returned and feed ``_get_optimal_R``; otherwise ``_get_optimal_R`` sees the last batch over the running ``Sp``
    (``:1451-1461``).  The reference's SVI result is not translation covariant (the blended ``Sp`` divides the batch's
    sums): ``origin`` only re-centres the assignment's operands, as in ``morpho_iterate``.

    ``sparse_calculation_mode=True`` with ``1 <= sparse_top_k <= 64``: as in ``morpho_iterate``, on every batch (the clamp is
    to NA, the columns are the batch's); ``P`` (``scipy.sparse.coo_matrix`` (NA, NB)) is returned only with
    ``return_mapping=True``, from the closing full assignment (``:299-302``).

    ``return_P=True`` (dense path only, capped as in ``morpho_iterate``): the last assignment executed runs through
    ``mvf_assign_dense`` and its ``P`` is returned - the last batch's, (NA, ``batch_size``) with the columns in the batch's
    order, or with ``return_mapping=True`` the closing full one's, (NA, NB).  Every other output keeps its bits.

    ``optimal_mapping=True``: a mapping needs every B cell, so the closing full assignment runs exactly as with
    ``return_mapping=True`` and is followed by ``mvf_assign_best``; the result gains ``best`` as in ``morpho_iterate`` (``cols``
    has NB rows).  Every other output has the bits of the same call with ``return_mapping=True``.

    ``apply=dict(...)`` as in ``morpho_iterate``: the closing full assignment runs in the same way and is followed by
    ``mvf_assign_apply``; the result gains ``applied`` (``to_B`` has NB rows).

    Not supported (``NotImplementedError``): what ``morpho_iterate`` refuses but ``SVI_mode``.  ``kernel_type="geodist"`` with
    ``graph_kernel=`` as in ``morpho_iterate``.

    Returns ``morpho_iterate``'s dict - ``K_NA``, ``K_NB`` (``batch_size``,), ``K_NA_spatial``, ``K_NA_sigma2`` of the last
    batch, ``Sp``, ``Sp_spatial``, ``Sp_sigma2`` the running values (or all of them the full assignment's) - plus
    ``batch_size``, ``batch_perm``, ``step_size`` (the last); ``history`` gains ``step_size``.  Two calls give equal bits."""
    a = _iterate_arguments(coordsA, coordsB, exp_layers_A, exp_layers_B, dissimilarity, probability_type,
                           probability_parameters, inducing_variables, beta, lambdaVF, sigma2, max_iter, nonrigid_start_iter,
                           kappa, gamma_a, gamma_b, partial_robust_level, sigma2_end, samples_s, inliers, nn_init_weight, dtype,
                           record, False, guidance, sparse_calculation_mode, kernel_type, origin, sparse_top_k, label_transfer,
                           graph_kernel)
    bs, perm = _svi_arguments(len(a["XB"]), batch_size, batch_perm, seed)
    apply = _apply_argument(apply, len(a["XA"]), len(a["XB"]), "morpho_iterate_svi")
    return_mapping = bool(return_mapping) or bool(optimal_mapping) or apply is not None
    return_P = _return_P_argument(return_P, a["top_k"], len(a["XA"]), len(a["XB"]) if return_mapping else bs)
    return _iterate(a, dissimilarity, beta, lambdaVF, sigma2, max_iter, nonrigid_start_iter, gamma_a, gamma_b,
                    partial_robust_level, nn_init_weight, update_R, dtype, device, record,
                    svi=dict(batch_size=bs, batch_perm=perm, return_mapping=bool(return_mapping)), return_P=return_P,
                    best=bool(optimal_mapping), apply=apply)


# ---- the start state: what the reference computes in front of the loop (morpho_class.py:700-747, 771-820, 845-852, 898-1041) ----
def _draw(n, idx, subsample, rng, name):
    """The rows of one side a start-state function works on: the indices given (validated) or, above ``subsample`` rows, a
    draw without replacement from ``rng`` - np.arange(n) otherwise, as the reference has it."""
    if idx is not None:
        raw = np.asarray(idx)
        if raw.ndim != 1 or len(raw) == 0 or not np.issubdtype(raw.dtype, np.integer):
            raise ValueError(f"{name} must be a non-empty 1-D integer array")
        if raw.min() < 0 or raw.max() >= n:
            raise ValueError(f"{name}: indices must lie in 0 .. {n - 1}")
        if len(np.unique(raw)) != len(raw):
            raise ValueError(f"{name}: indices must not repeat (the reference draws without replacement)")
        return raw.astype(np.int64)
    if isinstance(subsample, bool) or int(subsample) != subsample or subsample < 1:
        raise ValueError(f"the subsample size must be a positive integer, got {subsample!r}")
    return rng.choice(n, int(subsample), replace=False) if n > subsample else np.arange(n)


def _coords_pair(coordsA, coordsB, who):
    XA, XB = np.asarray(coordsA, dtype=np.float64), np.asarray(coordsB, dtype=np.float64)
    if XA.ndim != 2 or XB.ndim != 2 or XA.shape[1] != XB.shape[1]:
        raise AssertionError("X and Y do not have the same number of features.")  # _euc_distance_backend (utils.py:775)
    if XA.shape[1] not in (2, 3):
        raise NotImplementedError(f"{who}: spatial coordinates must be 2-D or 3-D, got D = {XA.shape[1]}")
    if len(XA) == 0 or len(XB) == 0:
        raise ValueError(f"{who}: both slices need at least one cell")
    return XA, XB


def _product_layer(k, A, B, metric, prob=_lib.ASSIGN_PROBS["prob"], param=0.0):
    """Both sides of one product layer prepared (mvf_assign_prepare): a `Layer` (mvf_assign_layer_stats reads no prob / param)."""
    Xp, a, ld = k.assign_prepare(A, metric, 0)
    Yp, b, _ = k.assign_prepare(B, metric, 1)
    return Layer(Xp, Yp, a, b, ld, metric, prob, param)


def init_sigma2(coordsA, coordsB, *, sigma2_init_scale=1.0, subsample=20000, subsample_A=None, subsample_B=None, seed=0,
                dtype: str = "float64", device=None):
    """The loop's initial ``sigma2``: ``sigma2_init_scale * _init_guess_sigma2(coordsA, coordsB)`` of the reference
    (``spateo/alignment/methods/utils.py:1339-1354``, ``morpho_class.py:710``), from the sum of squares that
    ``mvf_assign_layer_stats`` forms over the spatial distance matrix (the coordinates as an ``"euc"`` layer of D features):
    the matrix is never written.  ``coordsA`` are the coordinates AFTER the coarse alignment, as in the reference.

    Two things are the reference's and are reproduced: its ``"euc"`` distance already is the squared distance and is squared
    once more (``:1352``), and the sum is divided by ``D * nA_sub * nA_sub``, not by ``D * nA_sub * nB_sub`` (``:1353``).

    Above ``subsample`` cells a side is subsampled: ``subsample_A`` / ``subsample_B`` are the row indices to use (what the
    reference draws with ``np.random.choice``); without them the draw is ``np.random.default_rng(seed).choice``, A first -
    NOT the reference's stream.  Returns a float."""
    if dtype not in ("float32", "float64"):
        raise ValueError("dtype must be 'float32' or 'float64'")
    XA, XB = _coords_pair(coordsA, coordsB, "init_sigma2")
    rng = np.random.default_rng(seed)
    iA = _draw(len(XA), subsample_A, subsample, rng, "subsample_A")
    iB = _draw(len(XB), subsample_B, subsample, rng, "subsample_B")
    k = _rt._shared_kernels(device, dtype)
    stats = k.assign_layer_stats(_product_layer(k, XA[iA], XB[iB], _lib.ASSIGN_METRICS["euc"]), len(iA), len(iB))
    sum_sq = float(_rt._to_host(k, [stats["sums"]])[0][1])
    # utils.py:1352-1353: SpatialDistMat**2 of the already squared distance, over D * nA_sub * nA_sub
    return float(sigma2_init_scale) * (sum_sq / (XA.shape[1] * len(iA) * len(iA)))


def _start_layers(exp_layers_A, exp_layers_B, dissimilarity, probability_type, probability_parameters, label_transfer, who):
    """The layer lists validated as update_assignment validates them, a missing Gaussian parameter allowed.  Returns (LA,
    LB, codes, table, params, estimate): params the parameters as given, estimate the layers whose parameter is to be found."""
    LA = list(exp_layers_A) if isinstance(exp_layers_A, (list, tuple)) else [exp_layers_A]
    LB = list(exp_layers_B) if isinstance(exp_layers_B, (list, tuple)) else [exp_layers_B]
    if len(LA) < 1 or len(LA) != len(LB):
        raise ValueError("exp_layers_A and exp_layers_B must list the same (non-zero) number of layers")
    n = len(LA)
    as_list = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n  # noqa: E731
    metrics, kinds = as_list(dissimilarity), as_list(probability_type)
    params = [None] * n if probability_parameters is None else as_list(probability_parameters)
    if not (len(metrics) == len(kinds) == len(params) == n):
        raise ValueError("exp_layers_A, exp_layers_B, dissimilarity, probability_type and probability_parameters must list "
                         "the same (non-zero) number of layers")
    estimate = [l for l in range(n) if params[l] is None and str(kinds[l]).lower() == "gauss"]   # morpho_class.py:803-805
    for l in estimate:
        if metrics[l] == "label":  # the reference calls calc_distance without a table there (:813) and fails
            raise ValueError(f"{who}: layer {l} is a 'label' layer with probability type 'gauss' and no parameter; the "
                             f"reference cannot estimate it either - pass probability_parameters[{l}]")
    NA, NB = _n_rows(LA[0]), _n_rows(LB[0])
    filled = [1.0 if l in estimate else params[l] for l in range(n)]
    _, _, LA, LB, codes, table = _assignment_arguments(np.zeros((NA, 2)), np.zeros((NB, 2)), LA, LB, metrics, kinds, filled, False,
                                                       label_transfer, who)
    return LA, LB, codes, table, params, estimate


def _estimate_parameters(k, LA, LB, codes, estimate, iA, iB):
    """`_init_probability_parameters` (morpho_class.py:813-817) for the layers `estimate` on the rows iA / iB."""
    found = {}
    for l in estimate:
        layer = _product_layer(k, LA[l][iA], LB[l][iB], codes[l][0])
        # the minima over B for every A cell: the column minima of the exchanged call
        stats = k.assign_layer_stats(layer.exchanged(), len(iB), len(iA))
        row_min = np.sort(np.asarray(_rt._to_host(k, [stats["cmin"]])[0], dtype=np.float64))
        found[l] = max(float(row_min[int(len(iA) * 0.05)]) / 5, 0.01)
    return found


def init_probability_parameters(exp_layers_A, exp_layers_B, *, dissimilarity, probability_type, probability_parameters=None,
                                subsample=20000, subsample_A=None, subsample_B=None, seed=0, label_transfer=None,
                                dtype: str = "float64", device=None):
    """The per-layer Gaussian parameters the reference estimates in front of the loop,
    ``Morpho_pairwise._init_probability_parameters`` (``spateo/alignment/methods/morpho_class.py:771-820``): for every
    ``"gauss"`` layer whose parameter is ``None``, the minimum over the (subsampled) B cells of the layer distance of every
    (subsampled) A cell - ``mvf_assign_layer_stats`` with the operands exchanged, no matrix is written -, sorted, the entry at
    index ``int(nA_sub * 0.05)``, divided by 5 and floored at 0.01 (``:813-817``).  Parameters that were given and layers of
    another probability type pass through.  A ``"label"`` layer that would need estimating is a ``ValueError`` (the reference
    fails there: it calls ``calc_distance`` without the table).

    Layers and lists as ``update_assignment`` takes them.  ``subsample_A`` / ``subsample_B``: the row indices to use (one set
    for every estimated layer; the reference draws per layer with ``np.random.choice``); without them the draw is
    ``np.random.default_rng(seed).choice``, A first - NOT the reference's stream.  Returns the list of parameters."""
    if dtype not in ("float32", "float64"):
        raise ValueError("dtype must be 'float32' or 'float64'")
    LA, LB, codes, _, params, estimate = _start_layers(exp_layers_A, exp_layers_B, dissimilarity, probability_type,
                                                       probability_parameters, label_transfer, "init_probability_parameters")
    rng = np.random.default_rng(seed)
    iA = _draw(_n_rows(LA[0]), subsample_A, subsample, rng, "subsample_A")
    iB = _draw(_n_rows(LB[0]), subsample_B, subsample, rng, "subsample_B")
    out = list(params)
    if estimate:
        k = _rt._shared_kernels(device, dtype)
        for l, v in _estimate_parameters(k, LA, LB, codes, estimate, iA, iB).items():
            out[l] = v
    return out


def _voxel_data(coords, gene_exp, voxel_num):
    """``voxel_data`` (utils.py:1283-1336) without its loop over all voxels: a point can lie within ``voxel_size / 2`` only of
    the grid nodes whose index along every axis is within reach, so every point visits those few and the reference's own test
    ``sqrt(sum((coords - voxel_coord)**2)) < voxel_size / 2`` decides.  Returns (voxel_coords, voxel_gene_exps) of the
    occupied voxels in the reference's order (``np.meshgrid``'s).  ``gene_exp`` may be a scipy.sparse matrix (float64)."""
    from scipy.sparse import csr_matrix

    N, D = coords.shape
    lo, hi = coords.min(0), coords.max(0)
    voxel_size = np.sqrt(np.prod(hi - lo)) / (np.sqrt(N) / 5)
    steps = (hi - lo) / int(np.sqrt(voxel_num))
    axes = [np.arange(a, b, s) for a, b, s in zip(lo, hi, steps)]
    grid = np.stack(np.meshgrid(*axes), axis=-1)          # (n1, n0[, n2], D): meshgrid's "xy" order
    nodes = grid.reshape(-1, D)
    index_of = np.arange(len(nodes)).reshape(grid.shape[:-1])
    radius = voxel_size / 2
    first = [np.floor((coords[:, d] - radius - lo[d]) / steps[d]).astype(np.int64) - 1 for d in range(D)]
    span = [int(np.max(np.floor((coords[:, d] + radius - lo[d]) / steps[d]).astype(np.int64) + 1 - first[d])) + 1 for d in range(D)]
    vox, pts = [], []
    every = np.arange(N)
    for off in np.ndindex(*span):
        idx = [first[d] + off[d] for d in range(D)]
        ok = np.ones(N, dtype=bool)
        for d in range(D):
            ok &= (idx[d] >= 0) & (idx[d] < len(axes[d]))
        p = every[ok]
        ax = [idx[d][ok] for d in range(D)]
        v = index_of[(ax[1], ax[0]) + tuple(ax[2:])]     # meshgrid puts the second axis first
        dists = np.sqrt(np.sum((coords[p] - nodes[v]) ** 2, axis=1))
        keep = dists < radius
        vox.append(v[keep]), pts.append(p[keep])
    vox, pts = np.concatenate(vox), np.concatenate(pts)
    member = csr_matrix((np.ones(len(vox)), (vox, pts)), shape=(len(nodes), N))
    count = np.asarray(member.sum(1)).reshape(-1)
    used = count > 0
    sums = member[used] @ gene_exp                     # a sparse layer: a sparse product, dense only as voxels x g
    means = (sums.toarray() if is_sparse(sums) else np.asarray(sums)) / count[used][:, None]
    return nodes[used], means


PAIR_FIT_ITERATIONS = 100   # utils.py:1238
PAIR_FIT_ANNEAL_AFTER = 20  # the expression weights flatten from the iteration after this one on (:1268-1271)


def _weighted_rigid_fit(src, dst, w, total):
    """The proper rotation R and translation t that minimise sum_i w_i |dst_i - R src_i - t|^2 (weighted Kabsch; the last
    singular direction takes the sign that keeps det R = +1).  src, dst (n, D), w (n, 1); ``total`` is what the weighted
    centroids are divided by - the caller's sum of w before its floor, as in the reference (:1247-1248, 1263-1265)."""
    c_src, c_dst = (w * src).sum(0) / total, (w * dst).sum(0) / total
    U, _, Vt = np.linalg.svd((dst - c_dst).T @ (w * (src - c_src)))
    sign = np.ones(src.shape[1])
    sign[-1] = np.linalg.det(U @ Vt)
    R = (U * sign) @ Vt
    return R, c_dst - c_src @ R.T


def _inlier_posterior(resid2, w, sigma2, gamma, volume, D):
    """Per pair, the probability of being an inlier: an isotropic Gaussian of the squared residual, weighted by the pair's
    expression weight, against a uniform outlier density over ``volume`` carrying the largest weight (:1258-1260)."""
    inlier = np.exp(-resid2 / (2 * sigma2)) * w
    outlier = w.max() * (1 - gamma) * (2 * np.pi * sigma2) ** (D / 2) / (gamma * volume)
    return inlier / (inlier + outlier)


def _pair_inlier_fit(src, dst, expr_dist):
    """What the reference's ``inlier_from_NN`` (``utils.py:1220-1280``) computes, in this project's own form: an EM fit of one
    rigid motion to matched pairs src -> dst (n, D) that may be wrong.  Every pair carries an expression weight
    ``exp(-temper * d)`` with d its expression distance scaled so that the largest becomes 2 ln 10; per iteration a weighted
    rigid fit, the inlier posteriors (floored at 1e-6 once their sum is taken), the inlier fraction clamped to [0.01, 0.99]
    and the residual variance; after the first 21 iterations ``temper`` falls geometrically towards 0.1 and the weights are
    renormalised to a maximum of 1.  The posteriors returned are evaluated once more at variance 1e-2 and inlier fraction
    0.1 (:1273-1279).  Returns (posterior (n, 1), R, t, inlier fraction of that last evaluation)."""
    n, D = src.shape
    d = np.maximum(expr_dist, 0)
    d = d / (d.max() / (np.log(10) * 2))
    volume = max(np.prod(np.ptp(src, axis=0)), np.prod(np.ptp(dst, axis=0)))
    temper = 1.0
    cooling = (0.1 / temper) ** (1 / (PAIR_FIT_ITERATIONS - PAIR_FIT_ANNEAL_AFTER))
    w = np.exp(-d * temper)
    post, mass = w.copy(), w.sum()
    sigma2, fraction = ((src - dst) ** 2).sum() / (D * n), 0.5
    for it in range(PAIR_FIT_ITERATIONS):
        R, t = _weighted_rigid_fit(src, dst, post, mass)
        resid2 = ((dst - (src @ R.T + t)) ** 2).sum(1, keepdims=True)
        post = _inlier_posterior(resid2, w, sigma2, fraction, volume, D)
        mass = post.sum()
        fraction = min(max(mass / n, 0.01), 0.99)
        post = np.maximum(post, 1e-6)
        sigma2 = (resid2 * post).sum() / (D * mass)
        if it > PAIR_FIT_ANNEAL_AFTER:
            temper *= cooling
            w = np.exp(-d * temper)
            w = w / w.max()
    post = _inlier_posterior(resid2, w, 1e-2, 0.1, volume, D)
    return post, R, t, min(max(post.sum() / n, 0.01), 0.99)


INLIER_RANK = 20  # morpho_class.py:1020: the inlier threshold is the 21st largest P (at most 0.5), so 22 pairs are the least


def _coarse_arguments(coordsA, coordsB, init_A, init_B, metric, nn_init_top_K, n_sampling, subsample_A, subsample_B, rng, dtype):
    if dtype not in ("float32", "float64"):
        raise ValueError("dtype must be 'float32' or 'float64'")
    XA, XB = _coords_pair(coordsA, coordsB, "coarse_rigid_alignment")
    if metric not in _lib.ASSIGN_METRICS or metric == "label":
        raise ValueError(f"coarse_rigid_alignment: metric must be one of the product metrics (the reference uses 'kl' for "
                         f"init_field='layer' and 'euc' otherwise), got {metric!r}")
    FA, FB = (v.tocsr() if is_sparse(v) else np.asarray(v, dtype=np.float64) for v in (init_A, init_B))
    if FA.ndim != 2 or FB.ndim != 2 or FA.shape[1] != FB.shape[1] or FA.shape[1] < 1:
        raise AssertionError("X and Y do not have the same number of features.")
    if FA.shape[0] != len(XA) or FB.shape[0] != len(XB):
        raise ValueError("init_A and init_B must have one row per cell of their slice")
    if isinstance(nn_init_top_K, bool) or int(nn_init_top_K) != nn_init_top_K or nn_init_top_K < 1:
        raise ValueError(f"nn_init_top_K must be a positive integer, got {nn_init_top_K!r}")
    if nn_init_top_K > _lib.ASSIGN_TOPK_MAX:
        raise NotImplementedError(f"coarse_rigid_alignment: nn_init_top_K = {int(nn_init_top_K)} is not supported: the device "
                                  f"keeps at most {_lib.ASSIGN_TOPK_MAX} neighbours per voxel (_lib.ASSIGN_TOPK_MAX)")
    iA = _draw(len(XA), subsample_A, n_sampling, rng, "subsample_A")
    iB = _draw(len(XB), subsample_B, n_sampling, rng, "subsample_B")
    return XA, XB, FA, FB, iA, iB


def coarse_rigid_alignment(coordsA, coordsB, init_A, init_B, *, metric, nn_init_top_K=10, allow_flip=False, init_transform=True,
                           n_sampling=20000, subsample_A=None, subsample_B=None, seed=0, dtype: str = "float64", device=None):
    """The coarse rigid alignment of the reference's ``nn_init``, ``Morpho_pairwise._coarse_rigid_alignment``
    (``spateo/alignment/methods/morpho_class.py:898-1041``): both slices (subsampled above ``n_sampling`` cells) are
    voxelised (``voxel_data``, ``utils.py:1283-1336``, with ``voxel_num = max(min(int(N / 20), 1000), 100)``), the voxels'
    mean representations ``init_A`` (NA, G) / ``init_B`` (NB, G) are compared with ``metric`` (the reference: ``"kl"`` for
    ``init_field="layer"``, ``"euc"`` otherwise), the ``nn_init_top_K`` nearest voxels of every voxel either way make the
    matched pairs (``:976-998``), and the fit of ``inlier_from_NN`` (``utils.py:1220-1280``) gives R, t and the pairs' inlier
    probabilities; with ``allow_flip`` the mirrored fit replaces it when its gamma is larger (``:1007-1019``).

    The voxelisation and ``inlier_from_NN`` (100 iterations on a few thousand pairs) are host NumPy; the voxel x voxel
    distance matrix is never written: both lists of nearest voxels come from two ``mvf_assign_layer_stats`` calls with
    ``k = top_K``, the second with the operands exchanged.  Within a voxel's list the pairs are ordered by distance where
    ``np.argpartition`` leaves them unordered; every sum over the pairs is the same set of terms.  ``top_K`` is capped at the
    smaller voxel count minus one (the reference counts down after an exception); ``nn_init_top_K`` above 64 is refused
    (``NotImplementedError``: the lists' cap); at least 22 pairs are needed for the inlier threshold (``:1020``), fewer is a
    ``ValueError``.

    ``subsample_A`` / ``subsample_B``: the row indices to use; without them the draw is
    ``np.random.default_rng(seed).choice``, A first - NOT the reference's stream.

    Returns ``inliers = (inlier_A, inlier_B, inlier_P)`` as ``morpho_iterate`` takes them (``inlier_A`` transformed when
    ``init_transform``), ``inlier_pairs`` (n, 2) (the pairs' B voxel and A voxel), ``init_R`` (D, D), ``init_t`` (D,) and
    ``coordsA``, transformed by ``coordsA @ init_R.T + init_t`` when ``init_transform`` (``:1033-1035``)."""
    rng = np.random.default_rng(seed)
    XA, XB, FA, FB, iA, iB = _coarse_arguments(coordsA, coordsB, init_A, init_B, metric, nn_init_top_K, n_sampling, subsample_A,
                                               subsample_B, rng, dtype)
    D = XA.shape[1]
    vA, gA = _voxel_data(XA[iA], FA[iA], max(min(int(len(iA) / 20), 1000), 100))
    vB, gB = _voxel_data(XB[iB], FB[iB], max(min(int(len(iB) / 20), 1000), 100))
    N, M = len(vA), len(vB)
    top_K = min(int(nn_init_top_K), min(N, M) - 1)
    if top_K < 1 or top_K * (N + M) < INLIER_RANK + 2:
        raise ValueError(f"coarse_rigid_alignment: {N} x {M} occupied voxels with top_K = {top_K} give fewer than "
                         f"{INLIER_RANK + 2} matched pairs; the inlier threshold needs that many")
    k = _rt._shared_kernels(device, dtype)
    layer = _product_layer(k, gA, gB, _lib.ASSIGN_METRICS[metric])
    cols = k.assign_layer_stats(layer, N, M, top_K)                  # per B voxel: its top_K A voxels
    rows = k.assign_layer_stats(layer.exchanged(), M, N, top_K)      # per A voxel: its top_K B voxels
    c_rows, c_vals, r_rows, r_vals = _rt._to_host(k, [cols["rows"], cols["vals"], rows["rows"], rows["vals"]])
    # the pair list (B voxel, A voxel) in the reference's order (:976-998): every B voxel's neighbours, then every A voxel's
    NN1 = np.stack([np.repeat(np.arange(M), top_K), np.asarray(c_rows, dtype=np.int64).reshape(-1)], axis=1)
    NN2 = np.stack([np.asarray(r_rows, dtype=np.int64).reshape(-1), np.repeat(np.arange(N), top_K)], axis=1)
    NN = np.vstack((NN1, NN2))
    distance = np.r_[np.asarray(c_vals, dtype=np.float64).reshape(-1), np.asarray(r_vals, dtype=np.float64).reshape(-1)][:, None]
    src, dst = vA[NN[:, 1], :], vB[NN[:, 0], :]
    post, R, t, fraction = _pair_inlier_fit(src, dst, distance)
    if allow_flip:
        # the same fit to the slice mirrored in its last axis; kept when it explains more pairs (morpho_class.py:1007-1019)
        mirror = np.diag([1.0] * (D - 1) + [-1.0])
        m_post, m_R, m_t, m_fraction = _pair_inlier_fit(src @ mirror, dst, distance)
        if m_fraction > fraction:
            post, R, t = m_post, m_R @ mirror, m_t
    # inliers: the pairs above the 21st largest posterior, or above 0.5 where that is larger (:1020-1023)
    cut = min(np.sort(post[:, 0])[-(INLIER_RANK + 1)], 0.5)
    keep = np.flatnonzero(post[:, 0] > cut)
    inlier_A, inlier_B, out_A = src[keep], dst[keep], XA
    if init_transform:
        inlier_A, out_A = inlier_A @ R.T + t, XA @ R.T + t
    return dict(inliers=(inlier_A, inlier_B, post[keep]), inlier_pairs=NN[keep], init_R=R, init_t=np.asarray(t).reshape(-1),
                coordsA=out_A)


class _Start(dict):
    """What morpho_start returns: the keyword arguments of morpho_iterate / morpho_iterate_svi it computed, as a dict, and
    beside them - as attributes, so that ``**start`` stays what the loops take - ``coordsA`` (after the coarse transform),
    ``init_R`` and ``init_t``.  ``copy()``, ``copy.copy`` and pickling keep the attributes; ``dict(start)`` is the plain
    keyword dict."""

    def copy(self):
        return self.__copy__()

    def __copy__(self):
        new = _Start(self)
        new.__dict__.update(self.__dict__)
        return new

    def __reduce__(self):
        return (_Start, (dict(self),), dict(self.__dict__))


def morpho_start(coordsA, coordsB, exp_layers_A, exp_layers_B, *, dissimilarity, probability_type, probability_parameters=None,
                 inducing_variables_num=300, nn_init=True, init_layer_A=None, init_layer_B=None, init_metric="kl",
                 nn_init_top_K=10, allow_flip=False, init_transform=True, n_sampling=20000, subsample=20000,
                 sigma2_init_scale=1.0, subsample_A=None, subsample_B=None, inducing_idx=None, seed=0, label_transfer=None,
                 dtype: str = "float64", device=None):
    """Everything ``Morpho_pairwise`` computes in front of its loop, in the reference's order: the inducing variables
    (``_construct_kernel``, ``morpho_class.py:845-852``: unique rows of ``coordsA``, ``inducing_variables_num`` of them - the
    reference constructor's ``K``), with ``nn_init`` the coarse rigid alignment of ``init_layer_A`` / ``init_layer_B`` under
    ``init_metric`` (``coarse_rigid_alignment``; default: the first layer), and then, on the transformed ``coordsA``,
    ``sigma2`` (``init_sigma2``), the missing Gaussian parameters (``init_probability_parameters``) and ``samples_s``, the
    larger bounding-box volume (``:738-741``).

    Returns ``start``, a dict of ``probability_parameters``, ``inducing_variables``, ``sigma2``, ``samples_s`` and ``inliers``
    (None without ``nn_init``) with the attributes ``start.coordsA`` (the transformed coordinates), ``start.init_R`` and
    ``start.init_t`` (and ``start.inducing_rows``, the rows of ``coordsA`` the inducing variables were taken from):
    ``morpho_iterate(start.coordsA, coordsB, exp_layers_A, exp_layers_B, dissimilarity=, probability_type=,
    beta=, lambdaVF=, max_iter=, **start)`` runs the loop from it, and likewise ``morpho_iterate_svi``.

    The reference builds ``U`` and ``GammaSparse`` from ``coordsA`` BEFORE the coarse transform and lets the transform move
    ``coordsA`` alone.  Here the inducing variables are returned moved by the same ``init_R``, ``init_t``: the Gaussian
    kernel depends on distances only and a rigid motion, a flip included, keeps them, so ``U = con_K(coordsA,
    inducing_variables)`` and ``GammaSparse`` are the reference's.

    ``subsample_A`` / ``subsample_B`` (used by all three subsampled stages) and ``inducing_idx`` (rows of the unique
    ``coordsA``) pin what the reference draws with ``np.random.choice``; without them the draws are
    ``np.random.default_rng(seed)``'s - NOT the reference's stream."""
    from .preprocess import unique_rows

    XA, XB = _coords_pair(coordsA, coordsB, "morpho_start")
    LA, LB, codes, _, params, estimate = _start_layers(exp_layers_A, exp_layers_B, dissimilarity, probability_type,
                                                       probability_parameters, label_transfer, "morpho_start")
    if _n_rows(LA[0]) != len(XA) or _n_rows(LB[0]) != len(XB):
        raise ValueError("every layer must have one row per cell of its slice")
    if isinstance(inducing_variables_num, bool) or int(inducing_variables_num) != inducing_variables_num or inducing_variables_num < 1:
        raise ValueError("inducing_variables_num must be a positive integer")
    # one stream for every draw of our own, A before B: the rows of sigma2 and of the parameters first (what init_sigma2 and
    # init_probability_parameters draw from the same seed), then the coarse alignment's, then the inducing variables
    rng = np.random.default_rng(seed)
    iA = _draw(len(XA), subsample_A, subsample, rng, "subsample_A")
    iB = _draw(len(XB), subsample_B, subsample, rng, "subsample_B")
    FA = LA[0] if init_layer_A is None else init_layer_A
    FB = LB[0] if init_layer_B is None else init_layer_B
    out = _Start(inliers=None)
    R, t = np.eye(XA.shape[1]), np.zeros(XA.shape[1])
    moved = XA
    if nn_init:
        if init_layer_A is None and codes[0][0] == _lib.ASSIGN_LABEL:
            raise ValueError("morpho_start: nn_init needs init_layer_A / init_layer_B when the first layer is a label layer")
        cA, cB = (iA, iB) if n_sampling == subsample else (subsample_A, subsample_B)
        _, _, _, _, cA, cB = _coarse_arguments(XA, XB, FA, FB, init_metric, nn_init_top_K, n_sampling, cA, cB, rng, dtype)
        # (its refusals - fewer than 22 pairs among them - come before the device is touched: unique_rows follows it)
        c = coarse_rigid_alignment(XA, XB, FA, FB, metric=init_metric, nn_init_top_K=nn_init_top_K, allow_flip=allow_flip,
                                   init_transform=init_transform, subsample_A=cA, subsample_B=cB, dtype=dtype, device=device)
        out["inliers"], R, t = c["inliers"], c["init_R"], c["init_t"]
        if init_transform:
            moved = c["coordsA"]
    elif dtype not in ("float32", "float64"):
        raise ValueError("dtype must be 'float32' or 'float64'")
    # ---- _construct_kernel's draw (:845-852), on coordsA as given; the chosen rows move with the slice ----
    uniq, uniq_idx = unique_rows(XA, device=device)
    pick = _draw(len(uniq), inducing_idx, int(inducing_variables_num), rng, "inducing_idx")
    ctrl, XA = moved[uniq_idx[pick], :], moved
    out["sigma2"] = init_sigma2(XA, XB, sigma2_init_scale=sigma2_init_scale, subsample_A=iA, subsample_B=iB, dtype=dtype,
                                device=device)
    out["probability_parameters"] = list(params)
    if estimate:
        k = _rt._shared_kernels(device, dtype)
        for l, v in _estimate_parameters(k, LA, LB, codes, estimate, iA, iB).items():
            out["probability_parameters"][l] = v
    out["inducing_variables"] = ctrl
    out["samples_s"] = float(max(np.prod(XA.max(0) - XA.min(0)), np.prod(XB.max(0) - XB.min(0))))   # :738-741
    out.coordsA, out.init_R, out.init_t = XA, R, t
    out.inducing_rows = np.asarray(uniq_idx[pick], dtype=np.int64)   # the rows of coordsA the inducing variables are
    return out


# =====================================================================================================================
# PCA across slices (`group_pca`, spateo/alignment/utils.py:88-149): from counts to the 50 features the assignment likes
# =====================================================================================================================

def pca_sign(PCs):
    """The sign rule of ``pca``: every column of ``PCs`` (G, k) scaled by +-1 so that its loading of largest magnitude is
    positive, the lowest index on ties.  Returns (PCs flipped, the (k,) signs)."""
    PCs = np.asarray(PCs, dtype=np.float64)
    top = np.argmax(np.abs(PCs), axis=0)                      # (np.argmax returns the first of equal maxima)
    signs = np.where(PCs[top, np.arange(PCs.shape[1])] < 0, -1.0, 1.0)
    return PCs * signs, signs


def pca(mats, n_comps=50, zero_center=True, dtype="float32", device=None):
    """One PCA over all slices of a series, on the MI355X: what ``group_pca`` (``spateo/alignment/utils.py:88-149``) gets
    from ``sc.tl.pca`` on the concatenated slices.

    ``mats``: a list of per-slice matrices (n_i, G) with equal G, each dense or ``scipy.sparse`` (a single matrix is a list
    of one).  With N = sum n_i the stacked matrix is never formed on the host: the slices are packed one behind the other
    into one device cache of the centred values in ``dtype`` ("float32" | "float64"; the difference ``x - mean`` is taken in
    float64 and then rounded), laid out as the Gram kernel's operand (``mvf_colmeans`` / ``mvf_ublk_pack`` and their CSR
    twins).  ``G = Xc^T Xc`` is the cached Gram kernel with unit weights (float64 accumulation in both modes), the G x G
    symmetric eigenproblem runs ONCE on the host (``scipy.linalg.eigh`` with ``subset_by_index``: the top k pairs,
    independent of N) and the scores ``Xc V`` are ``mvf_apply_cached`` on the same cache.

    Returns a dict: ``X_pca`` - list of float64 (n_i, k) arrays (computed with float64 accumulation and stored in ``dtype``
    on the device, so in float32 mode they carry a float32 rounding); ``PCs`` (G, k), orthonormal columns; ``variance`` (k,)
    = eigenvalues / (N - 1); ``variance_ratio`` (k,) = eigenvalues / trace, the trace taken from the Gram diagonal;
    ``mean`` (G,) float64.  ``k = min(n_comps, min(N, G) - 1)``, components by decreasing variance.

    Sign rule: in every component the loading of largest magnitude is positive (the lowest index on ties) - sklearn's
    ``svd_flip(u_based_decision=False)``; with the fixed summation orders of the kernels it makes two calls bit-identical.
    The column means, and with them every output, depend on the stacked matrix only: a list of slices and their stacked
    matrix give the same bits.

    ``zero_center=False``: no means are taken (``mean`` is zeros), the raw values are packed and ``variance`` divides by N.

    Refused before anything is launched (``ValueError``): non-finite input, N < 2, G < 2, unequal column counts,
    ``n_comps < 1``; (``NotImplementedError``): G above ``_lib.PCA_MAX_FEATURES`` (what the Gram stage's reduction covers),
    k above ``_lib.PCA_MAX_COMPS`` (one pass of ``mvf_apply_cached``); (``_lib.MVFError``): a cache larger than the free
    device memory."""
    from ._kernels import pca_slices

    if dtype not in ("float32", "float64"):
        raise ValueError("dtype must be 'float32' or 'float64'")
    if is_sparse(mats) or (isinstance(mats, np.ndarray) and mats.ndim == 2):
        mats = [mats]
    mats = list(mats)
    if len(mats) == 0:
        raise ValueError("pca: no slices")
    if int(n_comps) < 1:
        raise ValueError(f"pca: n_comps must be at least 1, got {n_comps}")
    slices, G = pca_slices(mats)
    counts = [sl[4] if sl[0] == "csr" else sl[1].shape[0] for sl in slices]
    N = int(sum(counts))
    if N < 2:
        raise ValueError(f"pca: needs at least 2 cells over all slices, got {N}")
    if G < 2:
        raise ValueError(f"pca: needs at least 2 features, got {G}")
    if G > _lib.PCA_MAX_FEATURES:
        raise NotImplementedError(f"pca: at most {_lib.PCA_MAX_FEATURES} features are supported (_lib.PCA_MAX_FEATURES, the "
                                  f"extent of the Gram stage's tile reduction), got {G}; select genes first")
    k_comp = min(int(n_comps), min(N, G) - 1)
    if k_comp > _lib.PCA_MAX_COMPS:
        raise NotImplementedError(f"pca: at most {_lib.PCA_MAX_COMPS} components are supported (_lib.PCA_MAX_COMPS, one pass "
                                  f"of mvf_apply_cached), got {k_comp}")
    k = _rt._make_kernels(device, dtype)
    need, free = k.ublk_bytes(N, G), k.mem_free()
    if need >= free:
        raise _lib.MVFError(f"pca: the kernel-value cache ({need} bytes of HBM for {N} cells x {G} features in {dtype}) does "
                            f"not fit the {free} bytes free on the device")
    live = [sl for sl, c in zip(slices, counts) if c > 0]
    k.pca_open(N, G)
    try:
        mean = np.array(k.pca_means(live), dtype=np.float64) if zero_center else np.zeros(G)
        k.pca_pack(live, centred=bool(zero_center))
        gram = k.pca_gram()
        import scipy.linalg

        # ascending eigenvalues of the top k_comp pairs (the lower triangle is read; the Gram stage writes both, equal)
        lam, vec = scipy.linalg.eigh(gram, subset_by_index=[G - k_comp, G - 1])
        lam, vec = lam[::-1], vec[:, ::-1]
        PCs, _ = pca_sign(vec)
        scores = k.pca_scores(PCs)
    finally:
        k.pca_close()
    trace = float(np.trace(gram))
    bounds = np.concatenate([[0], np.cumsum(counts)])
    return {"X_pca": [np.array(scores[bounds[i] : bounds[i + 1]], dtype=np.float64) for i in range(len(counts))],
            "PCs": np.ascontiguousarray(PCs), "variance": lam / (N - 1 if zero_center else N),
            "variance_ratio": lam / trace if trace > 0 else np.zeros_like(lam), "mean": mean}


def _pca_genes(adatas, use_hvg, hvg_key, genes):
    """The genes ``group_pca`` runs on: those every slice carries - with ``use_hvg`` only the ones ``var[hvg_key]`` marks in
    EVERY slice -, in the first slice's order; restricted to ``genes`` (in its order) when given."""
    from ._morpho_pairwise import _var_column, var_names

    names = [var_names(a) for a in adatas]
    if use_hvg:
        marks = [_var_column(a, hvg_key) for a in adatas]
        lacking = [i for i, m in enumerate(marks) if m is None]
        if lacking:
            raise NotImplementedError(
                f"group_pca(use_hvg=True): slices {lacking} have no var['{hvg_key}'] column, and scanpy's highly-variable-gene "
                f"selection (sc.pp.highly_variable_genes, which the reference runs here) is not restated in this package. "
                f"Remedies: pass genes=[...], pass use_hvg=False, or mark the column yourself.")
        names = [[g for g, keep in zip(nm, np.asarray(m).astype(bool)) if keep] for nm, m in zip(names, marks)]
    common = names[0]
    for nm in names[1:]:
        have = set(nm)
        common = [g for g in common if g in have]
    if genes is not None:
        allowed, seen, picked = set(common), set(), []
        for g in np.asarray(genes).tolist():
            if g in allowed and g not in seen:
                seen.add(g)
                picked.append(g)
        common = picked
    if len(common) == 0:
        if use_hvg:
            raise ValueError("No highly variable genes were found. Please check your data or parameters for highly variable "
                             "gene selection.")
        raise ValueError("The number of common gene between all samples is 0.")
    return common


def group_pca(adatas, batch_key="batch", pca_key="X_pca", use_hvg=True, hvg_key="highly_variable", genes=None, **args):
    """``st.align.group_pca`` (``spateo/alignment/utils.py:88-149``): one PCA over the ``.X`` of all slices, written back as
    ``adatas[i].obsm[pca_key]`` (float64 (n_i, k)) - the representation ``Morpho_pairwise(rep_layer="X_pca",
    rep_field="obsm")`` then aligns on.  Returns None, like the reference.

    ``adatas``: ``AnnDataLite`` or, by duck typing, ``anndata.AnnData``.  ``batch_key`` is only checked: the reference's
    ``ValueError`` when it is already an ``obs`` column (the slices are not concatenated here, so nothing is labelled).
    The PCA runs on the genes common to all slices, in the first slice's order; ``genes=`` (an extension) restricts them.
    ``use_hvg=True`` uses the genes ``var[hvg_key]`` marks in EVERY slice (the rule of ``common_genes``); none left: the
    reference's "No highly variable genes were found" ``ValueError``; a slice without the column: ``NotImplementedError`` -
    the reference computes the column with scanpy's ``highly_variable_genes`` at this point, which is not restated here.
    ``**args``: ``n_comps`` (50), ``zero_center`` (True), ``dtype`` ("float32"), ``device`` of ``pca``; anything else
    (``sc.tl.pca``'s solver options) is a ``TypeError``."""
    from ._morpho_pairwise import _gene_positions, select_columns

    unknown = set(args) - {"n_comps", "zero_center", "dtype", "device"}
    if unknown:
        raise TypeError(f"group_pca: unsupported arguments {sorted(unknown)} (n_comps, zero_center, dtype, device are)")
    adatas = list(adatas)
    for i, adata in enumerate(adatas):
        obs = adata.obs
        if batch_key in (obs.columns if hasattr(obs, "columns") else obs.keys()):
            raise ValueError(f"batch_key '{batch_key}' already exists in adata.obs for dataset {i}. Please choose a different key.")
    use = _pca_genes(adatas, use_hvg, hvg_key, genes)
    mats = []
    for a in adatas:
        idx = _gene_positions(a, use)
        whole = len(idx) == a.X.shape[1] and np.array_equal(idx, np.arange(len(idx)))
        mats.append(a.X if whole else select_columns(a.X, idx))  # (all genes in place: the slice's own matrix, no copy)
    res = pca(mats, **args)
    for a, s in zip(adatas, res["X_pca"]):
        a.obsm[pca_key] = s


# the reference's top-level API on the stages above (its module reads this one's names at call time)
from ._morpho_pairwise import Morpho_pairwise, morpho_align  # noqa: E402
# ... and its reference-model route with the samplers under it
from ._downsampling import (downsampling, morpho_align_apply_transformation, morpho_align_ref,  # noqa: E402
                            morpho_align_transformation, sample, sample_by_kmeans, solve_RT_by_correspondence, trn)
# ... and the correction of the aligned stack against a surface mesh
from ._mesh_correction import Mesh_correction, icp, icp_batch, mesh_contours, mesh_correction_loss  # noqa: E402
