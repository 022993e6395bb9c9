"""``Morpho_pairwise`` and ``morpho_align``: the reference's top-level alignment API
(``spateo/alignment/methods/morpho_class.py``, ``spateo/alignment/morpho_alignment.py:22-111``) on this engine, AnnData in
and AnnData out.  Exported from ``spateo_amd.align``.

What runs where: the checks, the gene selection, the extraction of the layers and the normalisation of coordinates and
expression are host NumPy / SciPy in float64, O(N D) and O(nnz) - a ``scipy.sparse`` layer is column-selected, scaled and
row-indexed as CSR and never densified on the host; ``HipKernels.assign_prepare`` expands its CSR arrays on the device.  The
start state is ``align.morpho_start``, the loop ``align.morpho_iterate`` / ``align.morpho_iterate_svi``; the de-normalisation
of the three coordinate arrays and the ``vecfld`` dict are host work again.
"""
from __future__ import annotations

import warnings

import numpy as np

from . import _lib
from . import align as _al
from ._kernels import is_sparse
from .logging import logger_manager as lm

VALID_DISSIMILARITY = ["kl", "sym_kl", "euc", "euclidean", "square_euc", "square_euclidean", "cos", "cosine", "label"]
VALID_PROBABILITY = ["gauss", "gaussian", "cos", "cosine", "prob"]
VALID_GUIDANCE = ["nonrigid", "rigid", "both"]
VECFLD_KEYS = ("R", "t", "optimal_R", "optimal_t", "init_R", "init_t", "beta", "Coff", "inducing_variables", "normalize_scales",
               "normalize_means", "normalize_c", "dissimilarity", "sigma2", "gamma", "NA", "sigma2_variance", "method", "norm_dict",
               "kernel_type")
NORM_DICT_KEYS = ("mean_transformed", "mean_fixed", "scale", "scale_transformed", "scale_fixed")


# ---- duck-typed access to an AnnData / AnnDataLite ----
def var_names(sample):
    """The gene names of a sample as a list: ``.var_names``, else ``.var.index``."""
    names = getattr(sample, "var_names", None)
    if names is None:
        names = sample.var.index
    return [g for g in names]


def _var_column(sample, name):
    """A column of ``.var`` (a DataFrame or a dict of columns) as an array, or None when it is not there."""
    var = getattr(sample, "var", None)
    if var is None:
        return None
    columns = var.columns if hasattr(var, "columns") else var.keys()
    return np.asarray(var[name]) if name in columns else None


def _categorical(sample, key):
    """(categories, codes) of the categorical ``.obs`` column ``key``."""
    col = sample.obs[key]
    return col.cat.categories.tolist(), np.asarray(col.cat.codes, dtype=np.int64)


def _is_categorical(col):
    return hasattr(col, "cat")


def select_columns(matrix, idx):
    """Columns ``idx`` of an expression matrix: a ``scipy.sparse`` matrix as CSR (``X[:, idx]``, O(nnz)), anything else as a
    float64 array."""
    if is_sparse(matrix):
        return matrix.tocsr()[:, idx]
    return np.asarray(matrix, dtype=np.float64)[:, idx]


def check_rep_layer(samples, rep_layer, rep_field):
    """``check_rep_layer`` (``utils.py:174-224``), errors included."""
    for sample in samples:
        for rep, rep_f in zip(rep_layer, rep_field):
            missing = f"The specified representation '{rep}' not found in the '{rep_f}' attribute of some of the AnnData objects."
            if rep_f == "layer":
                if (rep != "X") and (rep not in sample.layers):
                    raise ValueError(missing)
            elif rep_f == "obsm":
                if rep not in sample.obsm:
                    raise ValueError(missing)
            elif rep_f == "obs":
                if rep not in sample.obs:
                    raise ValueError(missing)
                if not _is_categorical(sample.obs[rep]):
                    raise ValueError(f"The specified representation '{rep}' found in the '{rep_f}' attribute should be categorical.")
            else:
                raise ValueError("rep_field must be either 'layer', 'obsm' or 'obs'")
    return True


def check_obs(rep_layer, rep_field):
    """``check_obs`` (``utils.py:139-170``): the one ``obs`` layer's key, None without one, ``ValueError`` for more."""
    keys = [rep for rep, rep_f in zip(rep_layer, rep_field) if rep_f == "obs"]
    if len(keys) > 1:
        raise ValueError("'obs' occurs more than once in the list. Currently Spateo only support one label consistency.")
    return keys[0] if keys else None


def check_label_transfer_dict(catA, catB, label_transfer_dict):
    """``check_label_transfer_dict`` (``utils.py:228-260``)."""
    for ca in catA:
        if ca not in label_transfer_dict.keys():
            raise KeyError(f"Category '{ca}' from catA not found in label_transfer_dict.")
        for cb in catB:
            if cb not in label_transfer_dict[ca].keys():
                raise KeyError(f"Category '{cb}' from catB not found in label_transfer_dict for category '{ca}' from catA.")


def check_spatial_coords(sample, spatial_key="spatial"):
    """``check_spatial_coords`` (``utils.py:70-108``): the coordinates without the columns that hold a single value (a
    3-column ``spatial`` with constant z is a 2-D problem), float64; ``ValueError`` outside 2 / 3 dimensions."""
    if spatial_key not in sample.obsm:
        raise KeyError(f"Spatial key '{spatial_key}' not found in AnnData object.")
    coordinates = sample.obsm[spatial_key]
    coordinates = np.array(getattr(coordinates, "values", coordinates), dtype=np.float64)
    mask = []
    for i in range(coordinates.shape[1]):
        if len(np.unique(coordinates[:, i])) == 1:
            lm.main_info(f"The {i}-th dimension of the spatial coordinate has single value, which will be ignored.", indent_level=2)
        else:
            mask.append(i)
    coordinates = coordinates[:, mask]
    if coordinates.shape[1] > 3 or coordinates.shape[1] < 2:
        raise ValueError(f"The spatial coordinate '{spatial_key}' should only has 2 / 3 dimension")
    return np.ascontiguousarray(coordinates)


def common_genes(sampleA, sampleB, use_hvg=True, genes=None):
    """The genes both samples carry (``_align_preprocess``, ``morpho_class.py:471-484``): with ``use_hvg`` and a
    ``highly_variable`` column in both ``.var`` only those it marks.  The ORDER is that of ``genes`` when given, otherwise
    sample A's ``var`` order (the reference's is the iteration order of a ``set``)."""
    namesA, namesB = var_names(sampleA), var_names(sampleB)
    hvA, hvB = _var_column(sampleA, "highly_variable"), _var_column(sampleB, "highly_variable")
    if use_hvg and hvA is not None and hvB is not None:
        namesA = [g for g, keep in zip(namesA, hvA.astype(bool)) if keep]
        namesB = [g for g, keep in zip(namesB, hvB.astype(bool)) if keep]
    inB = set(namesB)
    common = [g for g in namesA if g in inB]
    if len(common) == 0:
        raise ValueError("The number of common gene between all samples is 0.")
    if genes is None:
        return common
    allowed, seen, out = set(common), set(), []
    for g in (g for g in np.asarray(genes).tolist()):
        if g in allowed and g not in seen:
            seen.add(g)
            out.append(g)
    if len(out) == 0:
        raise ValueError("None of `genes` is among the common genes of the samples.")
    return out


def _gene_positions(sample, genes):
    where = {g: i for i, g in enumerate(var_names(sample))}
    return np.array([where[g] for g in genes], dtype=np.int64)


def get_rep(sample, rep, rep_field, genes):
    """``get_rep`` (``utils.py:441-486``) without the densification: a ``layer`` is ``.X`` / ``.layers[rep]`` restricted to
    ``genes`` (CSR stays CSR), ``obsm`` a float64 array, ``obs`` the category codes."""
    if rep_field == "layer":
        if rep != "X" and rep not in sample.layers:
            raise KeyError(f"Layer '{rep}' not found in AnnData object.")
        return select_columns(sample.X if rep == "X" else sample.layers[rep], _gene_positions(sample, genes))
    if rep_field == "obs":
        return _categorical(sample, rep)[1]
    if rep_field == "obsm":
        rep_ = sample.obsm[rep]
        return np.array(getattr(rep_, "values", rep_), dtype=np.float64)
    raise ValueError("rep_field must be either 'layer', 'obsm' or 'obs'")


def normalize_coords(coordsA, coordsB, separate_mean=True, separate_scale=False):
    """``_normalize_coords`` (``morpho_class.py:589-641``) in float64: (coordsA, coordsB normalised, normalize_scales (2,),
    normalize_means).  ``separate_mean=False`` is the reference's to the letter: its ``repeat(global_mean, 2, axis=0)`` makes
    ``normalize_means`` the (2 D,) vector [m0, m0, m1, m1, ...], so BOTH slices have the SCALAR ``normalize_means[i]`` = m0, the
    global mean of the first axis, subtracted from every coordinate - a common translation, which the alignment does not mind
    and which de-normalisation (``normalize_means[1]``) and ``BA_transform`` undo with the same scalar."""
    coords = [np.array(coordsA, dtype=np.float64), np.array(coordsB, dtype=np.float64)]
    D = coords[0].shape[1]
    normalize_scales, normalize_means = np.zeros(2), np.zeros((2, D))
    for i in range(2):
        normalize_means[i] = np.einsum("ij->j", coords[i]) / coords[i].shape[0]
    if not separate_mean:
        normalize_means = np.repeat(np.mean(normalize_means, axis=0), 2, axis=0)
    for i in range(2):
        coords[i] -= normalize_means[i]
        normalize_scales[i] = np.sqrt(np.einsum("ij->", np.einsum("ij,ij->ij", coords[i], coords[i])) / coords[i].shape[0])
    if not separate_scale:
        normalize_scales = np.full((2,), np.mean(normalize_scales))
    for i in range(2):
        coords[i] /= normalize_scales[i]
    return coords[0], coords[1], normalize_scales, normalize_means


def _sum_of_squares(layer):
    if is_sparse(layer):
        d = np.asarray(layer.data, dtype=np.float64)
        return float(np.einsum("i,i->", d, d))                   # the stored entries are all that is not zero
    return float(np.einsum("ij->", np.einsum("ij,ij->ij", layer, layer)))


def _scaled(layer, scale):
    if is_sparse(layer):
        out = layer.astype(np.float64)                           # (a copy: the sample's own matrix is left alone)
        out.data = out.data / scale
        return out
    return layer / scale


def normalize_exps(layers_A, layers_B, rep_field, dissimilarity):
    """``_normalize_exps`` (``morpho_class.py:643-680``): every ``layer`` field whose metric is not ``kl`` is divided by the
    mean over the two slices of sqrt(sum of squares / cells).  Returns the scales ({layer index: scale}); the lists are
    updated in place.  For a sparse layer the sum is over ``.data`` and the division scales ``.data``."""
    scales = {}
    for i, (rep_f, d_s) in enumerate(zip(rep_field, dissimilarity)):
        if rep_f == "layer" and d_s != "kl":
            scale = 0.0
            for L in (layers_A, layers_B):
                scale += np.sqrt(_sum_of_squares(L[i]) / L[i].shape[0])
            scale /= 2
            layers_A[i], layers_B[i] = _scaled(layers_A[i], scale), _scaled(layers_B[i], scale)
            scales[i] = float(scale)
    return scales


def _device_argument(device):
    """The reference's ``device`` strings: ``"cpu"`` / None -> the default HIP device (there is no CPU path), ``"0"`` ->
    ``"cuda:0"``; anything else is handed on."""
    if device is None or str(device).lower() == "cpu":
        return None
    if str(device).isdigit():
        return f"cuda:{int(device)}"
    return device


class Morpho_pairwise:
    """Spateo's pairwise alignment, ``spateo.alignment.methods.Morpho_pairwise`` (``morpho_class.py:110-167``): the same
    constructor - names and defaults, ``dtype="float32"`` and ``SVI_mode=True`` included - and, after ``run()``, the same
    attributes: ``P``, ``XAHat``, ``RnA``, ``optimal_RnA``, ``optimal_R``, ``optimal_t``, ``R``, ``t``, ``sigma2``, ``gamma``,
    ``Coff``, ``inducing_variables``, ``normalize_scales``, ``normalize_means``, ``probability_parameters``, ``genes``,
    ``iter_added``, ``vecfld``.  ``sampleA`` is the slice that moves, ``sampleB`` the fixed one.

    The constructor runs the reference's ``_check`` (``:316-441``, errors included) and ``_align_preprocess`` (``:443-558``):
    common genes (``use_hvg`` with a ``highly_variable`` column, ``genes=``; exposed as ``.genes`` - in the order of ``genes=``
    when given, otherwise sample A's ``var`` order, where the reference has a ``set``'s), the layers per ``rep_field``
    (``layer``: ``.X`` / ``.layers[...]`` column-selected, a ``scipy.sparse`` matrix stays CSR and is never densified on the
    host; ``obsm``; ``obs``: category codes and the label-transfer table), ``check_spatial_coords`` (columns with a single
    value are dropped), ``_normalize_coords`` and ``_normalize_exps`` - all on the host in float64.  ``run()`` computes the
    start state (``align.morpho_start``; the reference draws its inducing variables in the constructor), runs the loop
    (``align.morpho_iterate_svi`` or, with ``SVI_mode=False``, ``align.morpho_iterate``) and wraps the output as
    ``_wrap_output`` does (``:1471-1528``): ``XAHat``, ``RnA`` and ``optimal_RnA`` de-normalised with the fixed slice's scale
    and mean, and ``vecfld`` with every key of the reference's, so that ``align.BA_transform(model.vecfld, raw_coordsA)``
    reproduces ``XAHat`` and ``optimal_RnA``.  ``vecfld`` is built whether or not ``vecfld_key_added`` is given.

    ``run()`` returns ``P`` like the reference: the dense ``P`` (NA x NB; in SVI mode without ``return_mapping`` the last
    batch's, NA x ``batch_size``) when it has at most ``align.RETURN_P_MAX_ENTRIES`` entries - above that ``None``, with one
    warning that names ``sparse_calculation_mode`` -, and in ``sparse_calculation_mode`` the ``scipy.sparse.coo_matrix`` of the
    last full assignment (in SVI mode that needs ``return_mapping=True``; without it the loop keeps no batch's mapping: None).

    ``iter_key_added`` (not None): ``iter_added[key_added][iter]`` is the de-normalised ``XAHat`` at the start of iteration
    ``iter`` and ``iter_added["sigma2"][iter]`` sigma2 there, as ``_save_iter`` records them (``:1043-1065``).  This uses the
    loop's ``record="arrays"``, which crosses the link every iteration: leave it None for speed.

    The reference draws from ``np.random``; that stream cannot be reproduced here.  Keyword-only and beyond the reference's
    signature, the pinning arguments of the stages: ``seed`` (our own draws), ``inducing_idx`` (rows of the unique
    ``coordsA``), ``subsample_A`` / ``subsample_B`` (the rows of the subsampled stages, the coarse alignment's included) and
    ``batch_perm`` (the initial SVI permutation).  Also keyword-only: ``optimal_mapping=True`` has the loop follow its last
    assignment with ``mvf_assign_best`` (in SVI mode the closing full assignment runs as with ``return_mapping=True``); after
    ``run()`` the method ``optimal_mapping(keep_all=False)`` returns the reference's ``mapping_aligned_coords(XAHat, coordsB, P,
    keep_all)`` - ``(by_A, by_B)``, see ``align.optimal_mapping`` - for slices of any size, with or without a ``P``.
    ``apply=dict(features_A=, features_B=, normalize=True)`` is forwarded to the loop (``align.morpho_iterate``'s ``apply``:
    the last assignment applied to cell features without ``P``; in SVI mode the closing full assignment runs); a string
    names a categorical ``obs`` column of that sample - expanded to one-hot columns in category order - or an ``obsm`` key.
    After ``run()`` the result is ``self.applied``, ``align.apply_assignment``'s dict, with ``categories_A`` / ``categories_B``
    beside it where an ``obs`` column was named.

    Accepted with no effect: ``use_chunk``, ``chunk_capacity`` and ``pre_compute_dist`` (memory layouts of the reference; the
    fused assignment writes no NA x NB matrix at all), ``save_concrete_iter``, ``graph_knn``, and ``verbose`` beyond logging.
    ``device``: ``"cpu"`` / None -> the default HIP device, ``"0"`` -> ``"cuda:0"``.

    Refused at construction (``NotImplementedError``): guidance (``guidance_pair`` with a truthy ``guidance_effect`` and
    ``guidance_weight > 0``), ``kernel_type`` other than ``"euc"`` or a ``graph``, ``sparse_calculation_mode`` with
    ``sparse_top_k`` above 64 (1024 is only the reference's default), more than four layers."""

    def __init__(self, sampleA, sampleB, rep_layer="X", rep_field="layer", genes=None, spatial_key="spatial",
                 key_added="align_spatial", iter_key_added=None, save_concrete_iter=False, vecfld_key_added=None,
                 dissimilarity="kl", probability_type="gauss", probability_parameters=None, label_transfer_dict=None,
                 use_hvg=True, nn_init=True, init_transform=True, allow_flip=False, init_layer="X", init_field="layer",
                 nn_init_top_K=10, nn_init_weight=1.0, max_iter=200, nonrigid_start_iter=80, SVI_mode=True, batch_size=None,
                 pre_compute_dist=True, sparse_calculation_mode=False, sparse_top_k=1024, lambdaVF=1e2, beta=0.01, K=15,
                 kernel_type="euc", graph=None, graph_knn=10, sigma2_init_scale=0.1, sigma2_end=None, gamma_a=1.0, gamma_b=1.0,
                 kappa=1.0, partial_robust_level=10, normalize_c=True, normalize_g=False, separate_mean=True,
                 separate_scale=False, dtype="float32", device="cpu", verbose=True, guidance_pair=None, guidance_effect=False,
                 guidance_weight=1.0, use_chunk=False, chunk_capacity=1.0, return_mapping=False, update_R=True, *, seed=0,
                 inducing_idx=None, subsample_A=None, subsample_B=None, batch_perm=None, optimal_mapping=False,
                 apply=None):
        self.verbose = verbose
        self.sampleA, self.sampleB = sampleA, sampleB
        self.rep_layer, self.rep_field, self.genes = rep_layer, rep_field, genes
        self.spatial_key, self.key_added, self.iter_key_added = spatial_key, key_added, iter_key_added
        self.save_concrete_iter, self.vecfld_key_added = save_concrete_iter, vecfld_key_added
        self.dissimilarity, self.probability_type = dissimilarity, probability_type
        self.probability_parameters, self.label_transfer_dict = probability_parameters, label_transfer_dict
        self.use_hvg, self.nn_init, self.init_transform, self.allow_flip = use_hvg, nn_init, init_transform, allow_flip
        self.init_layer, self.init_field, self.nn_init_top_K, self.nn_init_weight = init_layer, init_field, nn_init_top_K, nn_init_weight
        self.max_iter, self.nonrigid_start_iter, self.SVI_mode, self.batch_size = max_iter, nonrigid_start_iter, SVI_mode, batch_size
        self.pre_compute_dist, self.sparse_calculation_mode, self.sparse_top_k = pre_compute_dist, sparse_calculation_mode, sparse_top_k
        self.lambdaVF, self.beta, self.K, self.kernel_type, self.kernel_bandwidth = lambdaVF, beta, K, kernel_type, beta
        self.graph, self.graph_knn = graph, graph_knn
        self.sigma2_init_scale, self.sigma2_end = sigma2_init_scale, sigma2_end
        self.gamma_a, self.gamma_b, self.kappa, self.partial_robust_level = gamma_a, gamma_b, kappa, partial_robust_level
        self.normalize_c, self.normalize_g, self.separate_mean, self.separate_scale = normalize_c, normalize_g, separate_mean, separate_scale
        self.dtype, self.device = dtype, device
        self.guidance_pair, self.guidance_effect, self.guidance_weight = guidance_pair, guidance_effect, guidance_weight
        self.use_chunk, self.chunk_capacity, self.return_mapping, self.update_R = use_chunk, chunk_capacity, return_mapping, update_R
        self.seed, self.inducing_idx, self.subsample_A, self.subsample_B, self.batch_perm = seed, inducing_idx, subsample_A, subsample_B, batch_perm
        self._optimal_mapping, self.best = bool(optimal_mapping), None   # (the name optimal_mapping is the method's)
        self._apply_request, self.applied = apply, None
        if dtype not in ("float32", "float64"):
            raise ValueError("dtype must be 'float32' or 'float64'")
        self._check()
        self._refuse()
        self._align_preprocess()
        self._apply, self._apply_categories = self._resolve_apply()

    # ---- _check (:316-441) ----
    def _check(self):
        if self.rep_layer is None:
            raise ValueError("No representation input is detected, which may not produce meaningful result. Please check the "
                             "rep_layer and rep_field.")
        if self.rep_field is None:
            self.rep_field = "layer"
        if isinstance(self.rep_layer, str):
            self.rep_layer = [self.rep_layer]
        if isinstance(self.rep_field, str):
            self.rep_field = [self.rep_field] * len(self.rep_layer)
        self.rep_layer, self.rep_field = list(self.rep_layer), list(self.rep_field)
        check_rep_layer([self.sampleA, self.sampleB], self.rep_layer, self.rep_field)
        self.obs_key = check_obs(self.rep_layer, self.rep_field)
        if self.spatial_key not in self.sampleA.obsm:
            raise KeyError(f"Spatial key '{self.spatial_key}' not found in sampleA AnnData object.")
        if self.spatial_key not in self.sampleB.obsm:
            raise KeyError(f"Spatial key '{self.spatial_key}' not found in sampleB AnnData object.")
        if self.obs_key is not None and self.label_transfer_dict is not None:
            self.catA = _categorical(self.sampleA, self.obs_key)[0]
            self.catB = _categorical(self.sampleB, self.obs_key)[0]
            check_label_transfer_dict(self.catA, self.catB, self.label_transfer_dict)
        if self.dissimilarity is None:
            self.dissimilarity = "kl"
        if isinstance(self.dissimilarity, str):
            self.dissimilarity = [self.dissimilarity] * len(self.rep_layer)
        self.dissimilarity = [d_s.lower() for d_s in self.dissimilarity]
        for d_s in self.dissimilarity:
            if d_s not in VALID_DISSIMILARITY:
                raise ValueError(f"Invalid `metric` value: {d_s}. Available `metrics` are: {', '.join(VALID_DISSIMILARITY)}.")
        if self.probability_type is None:
            self.probability_type = "gauss"
        if isinstance(self.probability_type, str):
            self.probability_type = [self.probability_type] * len(self.rep_layer)
        self.probability_type = [p_t.lower() for p_t in self.probability_type]
        for p_t in self.probability_type:
            if p_t not in VALID_PROBABILITY:
                raise ValueError(f"Invalid `metric` value: {p_t}. Available `metrics` are: {', '.join(VALID_PROBABILITY)}.")
        for i, r_f in enumerate(self.rep_field):
            if r_f == "obs":
                self.dissimilarity[i] = "label"
                self.probability_type[i] = "prob"
        if self.probability_parameters is None:
            self.probability_parameters = [None] * len(self.rep_layer)
        elif not isinstance(self.probability_parameters, (list, tuple)):
            self.probability_parameters = [self.probability_parameters] * len(self.rep_layer)
        self.probability_parameters = list(self.probability_parameters)
        if self.nn_init:
            check_rep_layer([self.sampleA, self.sampleB], [self.init_layer], [self.init_field])
        if self.guidance_effect:
            if self.guidance_effect not in VALID_GUIDANCE:
                raise ValueError(f"Invalid `guidance_effect` value: {self.guidance_effect}. Available `guidance_effect` values "
                                 f"are: {', '.join(VALID_GUIDANCE)}.")
        if self.sparse_calculation_mode:
            self.pre_compute_dist = False

    def _refuse(self):
        """What this engine does not run, by name, before any data is touched."""
        if (self.guidance_pair is not None) and (self.guidance_effect != False) and (self.guidance_weight > 0):  # noqa: E712 (:551)
            raise NotImplementedError("Morpho_pairwise: guidance_pair (with guidance_effect and guidance_weight > 0) is not "
                                      "supported: the loops on the device take no guidance pairs "
                                      "(align.update_nonrigid(guidance=) is the stage on its own)")
        if self.kernel_type != "euc":
            raise NotImplementedError(f"Morpho_pairwise: kernel_type={self.kernel_type!r} is not supported (only the Euclidean "
                                      f"'euc' kernel; 'geodist' needs the graph distances of the inducing variables)")
        if self.graph is not None:
            raise NotImplementedError("Morpho_pairwise: graph= is not supported (it serves kernel_type='geodist' only)")
        if self.sparse_calculation_mode and not isinstance(self.sparse_top_k, bool) and self.sparse_top_k > _lib.ASSIGN_TOPK_MAX:
            raise NotImplementedError(f"Morpho_pairwise: sparse_calculation_mode with sparse_top_k = {self.sparse_top_k} is not "
                                      f"supported: the device keeps at most {_lib.ASSIGN_TOPK_MAX} entries per column of P "
                                      f"(_lib.ASSIGN_TOPK_MAX). 1024 is only the reference constructor's default: pass "
                                      f"sparse_top_k <= {_lib.ASSIGN_TOPK_MAX}")
        if len(self.rep_layer) > _lib.ASSIGN_MAX_LAYERS:
            raise NotImplementedError(f"Morpho_pairwise: at most {_lib.ASSIGN_MAX_LAYERS} layers are supported, got "
                                      f"{len(self.rep_layer)} in rep_layer")

    # ---- _align_preprocess (:443-558) ----
    def _align_preprocess(self):
        self.genes = common_genes(self.sampleA, self.sampleB, self.use_hvg, self.genes)
        if self.verbose:
            lm.main_info(f"Filtered all samples for common genes. There are {len(self.genes)} common genes.", indent_level=1)
        self.exp_layers_A = [get_rep(self.sampleA, rep, rep_f, self.genes) for rep, rep_f in zip(self.rep_layer, self.rep_field)]
        self.exp_layers_B = [get_rep(self.sampleB, rep, rep_f, self.genes) for rep, rep_f in zip(self.rep_layer, self.rep_field)]
        if self.obs_key is not None:
            catA, catB = _categorical(self.sampleA, self.obs_key)[0], _categorical(self.sampleB, self.obs_key)[0]
            self.label_transfer = _al.label_transfer_matrix(catA, catB, self.label_transfer_dict)
        else:
            self.label_transfer = None
        # the coarse alignment reads its representation from the samples as they are (get_rep in _coarse_rigid_alignment,
        # :934-949): before _normalize_exps
        self.init_layers = None
        if self.nn_init:
            self.init_layers = (get_rep(self.sampleA, self.init_layer, self.init_field, self.genes),
                                get_rep(self.sampleB, self.init_layer, self.init_field, self.genes))
        self.raw_coordsA = check_spatial_coords(self.sampleA, self.spatial_key)
        self.raw_coordsB = check_spatial_coords(self.sampleB, self.spatial_key)
        assert self.raw_coordsA.shape[1] == self.raw_coordsB.shape[1], "Spatial coordinate dimensions are different, please check again."
        self.NA, self.NB, self.D = self.raw_coordsA.shape[0], self.raw_coordsB.shape[0], self.raw_coordsA.shape[1]
        if self.normalize_c:
            self.coordsA, self.coordsB, self.normalize_scales, self.normalize_means = normalize_coords(
                self.raw_coordsA, self.raw_coordsB, self.separate_mean, self.separate_scale)
            if self.verbose:
                lm.main_info("Spatial coordinates normalization params:", indent_level=1)
                lm.main_info(f"Scale: {self.normalize_scales[:2]}...", indent_level=2)
                lm.main_info(f"Mean: {self.normalize_means[:2]}...", indent_level=2)
        else:
            self.coordsA, self.coordsB = self.raw_coordsA.copy(), self.raw_coordsB.copy()
            self.normalize_scales = self.normalize_means = None
        self.exp_scales = {}
        if self.normalize_g:
            self.exp_scales = normalize_exps(self.exp_layers_A, self.exp_layers_B, self.rep_field, self.dissimilarity)
            if self.verbose:
                for scale in self.exp_scales.values():
                    lm.main_info("Gene expression normalization params:", indent_level=1)
                    lm.main_info(f"Scale: {scale}.", indent_level=2)
        self.guidance = False
        if self.verbose:
            lm.main_info("Preprocess finished.", indent_level=1)

    def _resolve_apply(self):
        """``apply=`` with its strings looked up: (the dict the loops take or None, {"categories_A" / "categories_B": list})."""
        req = self._apply_request
        if req is None:
            return None, {}
        if not isinstance(req, dict) or not set(req) <= {"features_A", "features_B", "normalize"}:
            raise ValueError("Morpho_pairwise: apply must be a dict with features_A and / or features_B and, optionally, normalize")
        out, cats = {"normalize": bool(req.get("normalize", True))}, {}
        for side, sample, n in (("A", self.sampleA, self.NA), ("B", self.sampleB, self.NB)):
            F = req.get(f"features_{side}")
            if isinstance(F, str):
                if F in sample.obs:
                    if not _is_categorical(sample.obs[F]):
                        raise ValueError(f"Morpho_pairwise: apply: obs column '{F}' of sample {side} is not categorical")
                    cats[f"categories_{side}"], codes = _categorical(sample, F)
                    if len(codes) and codes.min() < 0:
                        raise ValueError(f"Morpho_pairwise: apply: obs column '{F}' of sample {side} has missing values")
                    F = np.zeros((n, max(len(cats[f"categories_{side}"]), 1)))
                    F[np.arange(n), codes] = 1.0             # one column per category, in category order
                elif F in sample.obsm:
                    F = np.asarray(sample.obsm[F])
                else:
                    raise KeyError(f"Morpho_pairwise: apply: '{F}' is neither an obs column nor an obsm key of sample {side}")
            if F is not None:
                out[f"features_{side}"] = F
        _al._apply_argument(out, self.NA, self.NB, "Morpho_pairwise")   # the loops' own validation, before anything runs
        return out, cats

    def _denormalize(self, X):
        """``X * normalize_scales[1] + normalize_means[1]`` (``_wrap_output``, ``_save_iter``): back to the fixed slice's frame."""
        if not self.normalize_c:
            return np.array(X, dtype=np.float64)
        return X * self.normalize_scales[1] + self.normalize_means[1]

    def _P_fits(self):
        """Whether the dense P of the last assignment is within align.RETURN_P_MAX_ENTRIES."""
        columns = self.NB
        if self.SVI_mode and not (self.return_mapping or self._optimal_mapping or self._apply is not None):
            columns = _al._svi_batch_size(self.NB, self.batch_size)
        return self.NA * columns <= _al.RETURN_P_MAX_ENTRIES

    def run(self):
        """The alignment: start state, loop, optimal rigid transformation, output.  Returns ``P`` (see the class)."""
        device = _device_argument(self.device)
        common = dict(dissimilarity=self.dissimilarity, probability_type=self.probability_type, label_transfer=self.label_transfer,
                      dtype=self.dtype, device=device)
        init = {}
        if self.nn_init:
            init = dict(init_layer_A=self.init_layers[0], init_layer_B=self.init_layers[1],
                        init_metric="kl" if self.init_field == "layer" else "euc")
        start = _al.morpho_start(self.coordsA, self.coordsB, self.exp_layers_A, self.exp_layers_B,
                                 probability_parameters=self.probability_parameters, inducing_variables_num=int(self.K),
                                 nn_init=bool(self.nn_init), nn_init_top_K=self.nn_init_top_K, allow_flip=self.allow_flip,
                                 init_transform=self.init_transform, sigma2_init_scale=self.sigma2_init_scale,
                                 subsample_A=self.subsample_A, subsample_B=self.subsample_B, inducing_idx=self.inducing_idx,
                                 seed=self.seed, **init, **common)
        if self.nn_init and self.verbose:
            lm.main_info("Coarse rigid alignment done.", indent_level=1)
        dense_P = not self.sparse_calculation_mode and self._P_fits()
        if not self.sparse_calculation_mode and not dense_P:
            warnings.warn(f"Morpho_pairwise: the dense P would have more than {_al.RETURN_P_MAX_ENTRIES} entries "
                          f"(align.RETURN_P_MAX_ENTRIES) and is not returned: run() gives None. Use sparse_calculation_mode=True "
                          f"(with sparse_top_k <= {_lib.ASSIGN_TOPK_MAX}) for a mapping of this size.", RuntimeWarning, stacklevel=2)
        loop = dict(beta=self.kernel_bandwidth, lambdaVF=self.lambdaVF, max_iter=self.max_iter,
                    nonrigid_start_iter=self.nonrigid_start_iter, kappa=self.kappa, gamma_a=self.gamma_a, gamma_b=self.gamma_b,
                    partial_robust_level=self.partial_robust_level, sigma2_end=self.sigma2_end, nn_init_weight=self.nn_init_weight,
                    update_R=self.update_R, record="arrays" if self.iter_key_added is not None else False,
                    sparse_calculation_mode=bool(self.sparse_calculation_mode), sparse_top_k=self.sparse_top_k, return_P=dense_P,
                    optimal_mapping=self._optimal_mapping, apply=self._apply, **common, **start)
        if self.SVI_mode:
            out = _al.morpho_iterate_svi(start.coordsA, self.coordsB, self.exp_layers_A, self.exp_layers_B, batch_size=self.batch_size,
                                         batch_perm=self.batch_perm, seed=self.seed, return_mapping=bool(self.return_mapping), **loop)
            self.batch_size, self.batch_perm = out["batch_size"], out["batch_perm"]
        else:
            out = _al.morpho_iterate(start.coordsA, self.coordsB, self.exp_layers_A, self.exp_layers_B, **loop)
        self._wrap_output(start, out)
        if self.verbose:
            lm.main_info(f"Key Parameters: gamma: {self.gamma}; sigma2: {self.sigma2}; probability_parameters: "
                         f"{self.probability_parameters}")
        return self.P

    def optimal_mapping(self, keep_all=False):
        """``(by_A, by_B)`` of ``align.mapping_from_best`` for the last assignment of ``run()``: ``X`` the de-normalised
        ``XAHat``, ``Y`` sample B's coordinates as ``check_spatial_coords`` left them.  Needs the constructor's
        ``optimal_mapping=True`` and a finished ``run()``."""
        if not self._optimal_mapping:
            raise ValueError("Morpho_pairwise.optimal_mapping(): construct the model with optimal_mapping=True, so that run() "
                             "keeps the best partners of its last assignment")
        if self.best is None:
            raise ValueError("Morpho_pairwise.optimal_mapping(): call run() first")
        return _al.mapping_from_best(self.best, self.XAHat, self.raw_coordsB, keep_all)

    # ---- _wrap_output (:1471-1528) and _save_iter (:1043-1065) ----
    def _wrap_output(self, start, out):
        self.probability_parameters = list(start["probability_parameters"])
        self.init_R, self.init_t = np.array(start.init_R), np.array(start.init_t)
        # the reference draws the inducing variables from coordsA BEFORE the coarse transform and keeps them there; the loop
        # got them moved with the slice (the kernel depends on distances only), BA_transform evaluates the field on the
        # points before init_R / init_t: the vecfld holds the rows as they were
        self.inducing_variables = self.coordsA[start.inducing_rows, :].copy()
        self.K = len(self.inducing_variables)
        self.R, self.t, self.optimal_R, self.optimal_t = out["R"], out["t"], out["optimal_R"], out["optimal_t"]
        self.sigma2, self.gamma, self.sigma2_variance = out["sigma2"], out["gamma"], out["sigma2_variance"]
        self.Coff, self.VnA, self.alpha, self.SigmaDiag = out["Coff"], out["VnA"], out["alpha"], out["SigmaDiag"]
        self.K_NA, self.K_NB = out["K_NA"], out["K_NB"]
        self.XAHat = self._denormalize(out["XAHat"])
        self.RnA = self._denormalize(out["RnA"])
        self.optimal_RnA = self._denormalize(out["optimal_RnA"])
        self.P = out.get("P")
        self.best = out.get("best")
        self.applied = dict(out["applied"], **self._apply_categories) if "applied" in out else None
        self.iter_added = None
        if self.iter_key_added is not None:
            hist = out["history"]
            frames = [start.coordsA] + list(hist["XAHat"][:-1])
            sigma2s = [start["sigma2"]] + list(hist["sigma2"][:-1])
            self.iter_added = {self.key_added: {it: self._denormalize(x) for it, x in enumerate(frames)},
                               "sigma2": {it: np.float64(s) for it, s in enumerate(sigma2s)}}
        D = self.D
        if self.normalize_c:
            norm_dict = {"mean_transformed": np.array(self.normalize_means[0]), "mean_fixed": np.array(self.normalize_means[1]),
                         "scale": np.array(self.normalize_scales[0]), "scale_transformed": np.array(self.normalize_scales[0]),
                         "scale_fixed": np.array(self.normalize_scales[1])}
        else:   # (the reference has no norm_dict to give then; BA_transform does not read it)
            norm_dict = {"mean_transformed": np.zeros(D), "mean_fixed": np.zeros(D), "scale": np.array(1.0),
                         "scale_transformed": np.array(1.0), "scale_fixed": np.array(1.0)}
        self.vecfld = {
            "R": self.R, "t": self.t, "optimal_R": self.optimal_R, "optimal_t": self.optimal_t,
            "init_R": self.init_R if self.nn_init else np.eye(D), "init_t": self.init_t if self.nn_init else np.zeros(D),
            "beta": self.beta, "Coff": self.Coff, "inducing_variables": self.inducing_variables,
            "normalize_scales": np.array(self.normalize_scales) if self.normalize_c else None,
            "normalize_means": np.array(self.normalize_means) if self.normalize_c else None,
            "normalize_c": self.normalize_c, "dissimilarity": self.dissimilarity, "sigma2": np.float64(self.sigma2),
            "gamma": np.float64(self.gamma), "NA": self.NA, "sigma2_variance": np.float64(self.sigma2_variance), "method": "Spateo",
            "norm_dict": norm_dict, "kernel_type": self.kernel_type,
        }


def morpho_align(models, rep_layer="X", rep_field="layer", genes=None, spatial_key="spatial", key_added="align_spatial",
                 iter_key_added="iter_spatial", vecfld_key_added="VecFld_morpho", mode="SN-S", dissimilarity="kl", max_iter=200,
                 dtype="float32", device="cpu", verbose=True, **kwargs):
    """Continuous alignment of a list of slices, ``spateo.alignment.morpho_align``
    (``spateo/alignment/morpho_alignment.py:22-111``) with its signature: the models are copied, ``obsm[key_added]``,
    ``obsm[f"{key_added}_rigid"]`` and ``obsm[f"{key_added}_nonrigid"]`` start as the raw coordinates, and every slice is aligned
    to the ALIGNED previous one - ``Morpho_pairwise(sampleA=models[i + 1], sampleB=models[i], spatial_key=key_added, ...)`` -,
    whose ``optimal_RnA`` / ``XAHat`` become ``_rigid`` / ``_nonrigid``; ``key_added`` takes the rigid result in mode
    ``"SN-S"`` and the non-rigid one in ``"SN-N"``.  ``uns[iter_key_added]`` takes ``iter_added`` (per-iteration records cross
    the link every iteration: pass ``iter_key_added=None`` for speed) and ``uns[vecfld_key_added]`` the ``vecfld``.

    ``models``: ``AnnDataLite`` or, by duck typing, ``anndata.AnnData`` - what is touched is ``.X``, ``.layers``, ``.var_names``
    or ``.var.index``, the columns of ``.var``, ``.obs``, ``.obsm``, ``.uns`` and ``.copy()``.  ``**kwargs`` go to
    ``Morpho_pairwise``, the pinning arguments included.  Returns ``(align_models, pis)`` with ``pis[i] = P.T`` of pair i, or
    ``None`` where ``P`` is (see ``Morpho_pairwise``)."""
    if mode not in ("SN-S", "SN-N"):
        raise ValueError(f"mode must be 'SN-S' or 'SN-N', got {mode!r}")
    align_models = [model.copy() for model in models]
    for m in align_models:
        m.obsm[key_added] = np.array(m.obsm[spatial_key]).copy()
        m.obsm[f"{key_added}_rigid"] = np.array(m.obsm[spatial_key]).copy()
        m.obsm[f"{key_added}_nonrigid"] = np.array(m.obsm[spatial_key]).copy()
    pis = []
    for i in range(len(align_models) - 1):
        modelA, modelB = align_models[i], align_models[i + 1]
        morpho_model = Morpho_pairwise(sampleA=modelB, sampleB=modelA, rep_layer=rep_layer, rep_field=rep_field,
                                       dissimilarity=dissimilarity, genes=genes, spatial_key=key_added, key_added=key_added,
                                       iter_key_added=iter_key_added, vecfld_key_added=vecfld_key_added, max_iter=max_iter,
                                       dtype=dtype, device=device, verbose=verbose, **kwargs)
        P = morpho_model.run()
        modelB.obsm[f"{key_added}_rigid"] = morpho_model.optimal_RnA.copy()
        modelB.obsm[f"{key_added}_nonrigid"] = morpho_model.XAHat.copy()
        modelB.obsm[key_added] = modelB.obsm[f"{key_added}_rigid" if mode == "SN-S" else f"{key_added}_nonrigid"]
        if iter_key_added is not None:
            modelB.uns[iter_key_added] = morpho_model.iter_added
        if vecfld_key_added is not None:
            modelB.uns[vecfld_key_added] = morpho_model.vecfld
        pis.append(None if P is None else P.T)
    return align_models, pis
