"""ctypes binding of ``libmvf.so`` (C ABI declared in ``include/mvf.h``).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C spateo-release_amd/csrc`` and is the ONLY
compute path of this package: there is no CPU fallback.  ``load()`` raises if the shared object is missing.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# Developer overrides are honoured ONLY under the explicit gate MVF_DEV_KNOBS=1 (and announced on stderr): MVF_LIB_PATH
# (A/B runs of two builds of the library) and the legacy MVF_* kernel knobs, which are translated into mvf_debug_option
# calls at load time.  Without the gate the environment changes nothing.
DEV_KNOBS = os.environ.get("MVF_DEV_KNOBS") == "1"
LIB_PATH = (DEV_KNOBS and os.environ.get("MVF_LIB_PATH")) or os.path.join(_HERE, "lib", "libmvf.so")
DEBUG_OPTIONS = ("conk_form", "slice_len", "solve_small_off", "lr_timing", "lr_no_deflate", "defl_block", "defl_apps", "lr_no_direct",
                 "direct_accept", "gram_reg_cols")
_LEGACY_ENV = {  # environment name -> (option, value parser)
    "MVF_CONK": ("conk_form", lambda v: {"rows": 1, "flat": 2, "2d": 3}[v]),
    "MVF_SLICE_LEN": ("slice_len", int),
    "MVF_SOLVE_SMALL": ("solve_small_off", lambda v: 1 if v.startswith("0") else 0),
    "MVF_LR_TIMING": ("lr_timing", lambda v: 1),
}

MVF_F32, MVF_F64 = 0, 1
MVF_ESTEP_MIN_DOUBLES = 4098

MVF_COMM_ID_BYTES = 128
RED_SUM, RED_MIN = 0, 1
GRAM_TILES, GRAM_RHS, GRAM_REDUCE, GRAM_REDUCE_RHS = 1, 2, 4, 8
RK45_UNIFORM_TIME, RK45_ARC_LENGTH = 0, 1
ASSIGN_METRICS = {"euc": 0, "euclidean": 0, "square_euc": 1, "square_euclidean": 1, "kl": 2, "sym_kl": 3, "cos": 4, "cosine": 4,
                  "label": 5}
ASSIGN_LABEL = 5  # MVF_ASSIGN_LABEL: the layer is a pair of label vectors and the shared label-transfer table
ASSIGN_PROBS = {"gauss": 0, "gaussian": 0, "cos": 1, "cosine": 1, "prob": 2}
ASSIGN_MAX_LAYERS = 4
ASSIGN_TOPK_MAX = 64  # MVF_ASSIGN_TOPK_MAX: the largest sparse_top_k mvf_assign_topk keeps per column
ALIGN_MOMENT_DOUBLES = 64
# align.pca: the Gram stage reduces its partial tiles with one grid row per pair of 128-wide tiles (gram_reduce_kernel's
# grid.y = nt (nt + 1) / 2 <= 65535  ->  nt <= 361), and mvf_apply_cached projects at most 128 columns per pass over the cache
PCA_MAX_FEATURES = 361 * 128
PCA_MAX_COMPS = 128
TRN_MAX_NODES = 4096  # MVF_TRN_MAX_NODES: mvf_trn keeps the nodes of a problem in one workgroup's registers, their keys in its LDS
ICP_MAX_POINTS = 512  # MVF_ICP_MAX_POINTS: mvf_icp_batch / mvf_mesh_loss keep both (thinned) contours of a problem in one workgroup's LDS
# MVF_KDE_GAUSSIAN .. MVF_KDE_COSINE: the kernels of mvf_kde (sklearn.neighbors.KernelDensity's names)
KDE_KERNELS = {"gaussian": 0, "exponential": 1, "tophat": 2, "epanechnikov": 3, "linear": 4, "cosine": 5}
KDE_MAX_COLUMNS = 64  # MVF_KDE_MAX_COLUMNS: the columns (groups of sources) of one mvf_kde call
SHAPE_MAX_NSUB = 128  # MVF_SHAPE_MAX_NSUB: the voxels per axis of mvf_shape_descriptors
SHAPE_ORDERS = {"linear": 1, "quadratic": 2, "cubic": 3}
HEAT_MAX_STEPS = 8  # MVF_HEAT_MAX_STEPS: the sweeps one launch of mvf_heat_grid's kernel runs in LDS at most
KNN_MAX_K = 64  # MVF_KNN_MAX_K: the neighbours per point of mvf_knn
SSSP_STATUS = 4  # MVF_SSSP_STATUS: int64 entries of mvf_graph_sssp's status block
EVAL_V, EVAL_JAC, EVAL_DIV, EVAL_CURL, EVAL_ACC, EVAL_CURV, EVAL_TORS, EVAL_JDET = 1, 2, 4, 8, 16, 32, 64, 128
# the status record `einfo` of mvf_solve_minnorm / _lr / _lrd / _lrd_async (mvf.h): 12 float64; a `reuse` call writes its own
# values behind the first call's.  SWEEPS is x.5 when the sweep cap was hit (check_converged); DELTA the shift that was
# subtracted again (mvf_solve_minnorm only); FACTOR_RANK the columns of the pivoted factor (the next call's rank_hint);
# BLOCK, FORM, REJECTED: mvf_solve_minnorm_lrd(_async) only
EINFO_DOUBLES = 12
(EINFO_SWEEPS, EINFO_KEPT_RANK, EINFO_LMAX, EINFO_LMIN_KEPT, EINFO_DELTA, EINFO_LMIN, EINFO_FACTOR_RANK, EINFO_BLOCK,
 EINFO_FORM, EINFO_REJECTED) = range(10)
LRD_FORM_JACOBI, LRD_FORM_FACTOR, LRD_FORM_DIRECT = 0, 1, 2  # einfo[EINFO_FORM]: which form of mvf_solve_minnorm_lrd answered
LRD_HINT_MOVED = 4  # added to mvf_solve_minnorm_lrd_async's form_hint: the matrix moved since the previous call

_p, _i64, _i, _d, _sz = C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_size_t



class AssignLayer(C.Structure):
    """mvf_assign_layer of include/mvf.h: one prepared expression / representation layer (device pointers)."""
    _fields_ = [("Xp", C.c_void_p), ("Yp", C.c_void_p), ("a", C.c_void_p), ("b", C.c_void_p), ("ld", C.c_int64),
                ("metric", C.c_int), ("prob", C.c_int), ("param", C.c_double)]


class TrnProblem(C.Structure):
    """mvf_trn_problem of include/mvf.h: one TRN problem (device pointers, sizes)."""
    _fields_ = [("X", C.c_void_p), ("N", C.c_int64), ("d", C.c_int64), ("n", C.c_int64), ("T", C.c_int64), ("w_idx", C.c_void_p),
                ("p_idx", C.c_void_p), ("l", C.c_void_p), ("ep", C.c_void_p), ("kc", C.c_void_p), ("W", C.c_void_p)]


class IcpProblem(C.Structure):
    """mvf_icp_problem of include/mvf.h: one pair of contours (device pointers, sizes) and its outputs."""
    _fields_ = [("contour_1", C.c_void_p), ("n1", C.c_int64), ("contour_2", C.c_void_p), ("n2", C.c_int64), ("gamma", C.c_void_p),
                ("stats", C.c_void_p), ("T_contour_2", C.c_void_p), ("translation", C.c_void_p)]


# name -> (restype, argtypes); mirrors include/mvf.h one to one
SIGNATURES = {
    "mvf_last_error": (C.c_char_p, []),
    "mvf_version": (_i, []),
    "mvf_read_back": (_i, [_p, _p, C.c_size_t, _p]),
    "mvf_debug_option": (_i, [C.c_char_p, C.c_longlong]),
    "mvf_debug_option_get": (C.c_longlong, [C.c_char_p]),
    "mvf_device_count": (_i, [C.POINTER(C.c_int)]),
    "mvf_unique_rows_workspace_bytes": (_sz, [_i64, _i]),
    "mvf_unique_rows": (_i, [_p, _i64, _i, _p, _p, _p, _p, _sz, _p]),
    "mvf_knn_rowsum": (_i, [_p, _i64, _i, _i, _p, _p]),
    "mvf_hull_mask": (_i, [_p, _i64, _p, _i64, _d, _p, _p]),
    "mvf_con_k": (_i, [_p, _i64, _p, _i64, _i, _d, _p, _i, _p]),
    "mvf_con_k_d": (_i, [_p, _i64, _p, _i64, _i, _d, _p, _p, _i, _p]),
    "mvf_reduce_scratch_doubles": (_sz, [_i64]),
    "mvf_apply": (_i, [_p, _i64, _p, _i64, _d, _p, _p, _p, _p, _p, _p, _p, _i, _p]),
    "mvf_estep_min": (_i, [_p, _i64, _d, _p, _i, _p]),
    "mvf_estep_p": (_i, [_p, _i64, _d, _d, _d, _i, _d, _d, _d, _p, _p, _p, _p, _i, _p]),
    "mvf_estep": (_i, [_p, _i64, _d, _d, _d, _i, _d, _d, _p, _p, _p, _p, _i, _p]),
    "mvf_gram_workspace_bytes": (_sz, [_i64, _i64, _i]),
    "mvf_gram": (_i, [_p, _p, _p, _i64, _p, _i64, _d, _p, _p, _p, _sz, _i, _p]),
    "mvf_gram_stages": (_i, [_i, _p, _p, _p, _i64, _p, _i64, _d, _p, _p, _p, _sz, _i, _p]),
    "mvf_ublk_bytes": (_sz, [_i64, _i64, _i]),
    "mvf_ublk_build": (_i, [_p, _i64, _p, _i64, _d, _p, _sz, _i, _p]),
    "mvf_gram_cached": (_i, [_i, _p, _p, _p, _p, _i64, _p, _i64, _d, _p, _p, _p, _sz, _i, _p]),
    "mvf_solve_workspace_bytes": (_sz, [_i64, _i]),
    "mvf_solve": (_i, [_p, _p, _d, _d, _p, _i64, _i, _p, _p, _p, _p, _sz, _p]),
    "mvf_solve_minnorm_workspace_bytes": (_sz, [_i64, _i]),
    "mvf_solve_minnorm": (_i, [_p, _p, _d, _d, _d, _p, _i64, _i, _p, _p, _p, _i, _i, _p, _i, _p, _sz, _p]),
    "mvf_solve_minnorm_basis_bytes": (_sz, [_i64]),
    "mvf_solve_minnorm_lr_workspace_bytes": (_sz, [_i64, _i]),
    "mvf_solve_minnorm_lr": (_i, [_p, _p, _d, _d, _d, _p, _i64, _i, _p, _p, _p, _i, _i, _i, _p, _sz, _p]),
    "mvf_wide_workspace_bytes": (_sz, [_i64, _i64]),
    "mvf_rhs_cached": (_i, [_p, _p, _p, _i64, _i64, _i, _i64, _p, _i64, _p, _sz, _i, _p]),
    "mvf_apply_cached": (_i, [_p, _i64, _i64, _p, _i64, _i, _p, _i64, _p, _p, _p, _p, _p, _sz, _i, _p]),
    "mvf_solve_minnorm_lrd_workspace_bytes": (_sz, [_i64, _i]),
    "mvf_solve_minnorm_lrd": (_i, [_p, _p, _d, _d, _d, _p, _i64, _i, _p, _p, _p, _i, _i, _i, _p, _sz, _p]),
    "mvf_solve_minnorm_lrd_async": (_i, [_p, _p, _d, _d, _d, _p, _i64, _i, _p, _p, _p, _i, _p, _sz, _p]),
    "mvf_lr_pivot_order": (_i, [_p, _sz, _i64, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                C.POINTER(C.c_int64), _p]),
    "mvf_pinv_diag": (_i, [_p, _i64, _p, _i64, _d, _d, _i, _p, _p, _sz, _i, _p]),
    "mvf_lincomb3": (_i, [_p, _d, _p, _d, _p, _d, _p, _i64, _p]),
    "mvf_quadform": (_i, [_p, _p, _i64, _i, _p, _p, _p]),
    "mvf_sym_pack": (_i, [_p, _i64, _p, _p]),
    "mvf_sym_unpack": (_i, [_p, _i64, _p, _p]),
    "mvf_comm_unique_id": (_i, [_p]),
    "mvf_comm_create": (_i, [C.POINTER(_p), _i, _i, _p]),
    "mvf_comm_destroy": (_i, [_p]),
    "mvf_comm_info": (_i, [_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mvf_allreduce_stats": (_i, [_p, _p, _i64, _i, _p]),
    "mvf_eval": (_i, [_p, _i64, _p, _i64, _d, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p]),
    "mvf_eval_affine": (_i, [_p, _i64, _p, _i64, _d, _p, C.POINTER(C.c_double), _i, _p, _p, _p, _p, _p, _p, _p, _p, _i,
                             _p]),
    "mvf_ublk_build_d": (_i, [_p, _i64, _p, _i64, _i, _d, _p, _sz, _i, _p]),
    "mvf_eval_d": (_i, [_p, _i64, _p, _i64, _i, _d, _p, _i, _i, _p, _p, _p, _p, _p, _i, _p]),
    "mvf_eval_wide": (_i, [_p, _i64, _p, _i64, _i, _d, _p, _i64, _i, _i, _p, _i64, _p, _i, _p]),
    "mvf_integrate": (_i, [_p, _i64, _p, _i64, _d, _p, C.POINTER(C.c_double), _d, _i, _i, _p, _i, _p]),
    "mvf_integrate_rk45": (_i, [_p, _i64, _p, _i64, _d, _p, C.POINTER(C.c_double), _i, C.POINTER(C.c_double), _d, _d,
                                _d, _d, _i, _i, _i, _p, _p, _p, _i, _p]),
    "mvf_assign_padded_features": (_i64, [_i64, _i]),
    "mvf_assign_prepare": (_i, [_p, _i64, _i64, _i, _i, _p, _i64, _p, _i, _p]),
    "mvf_assign_prepare_csr_min_workspace_bytes": (_sz, [_i64]),
    "mvf_assign_prepare_csr": (_i, [_p, _p, _p, _i, _i64, _i64, _i, _i, _p, _i64, _p, _p, _sz, _i, _p]),
    "mvf_assign_label_prepare": (_i, [_p, _i64, _i64, _p, _p]),
    "mvf_assign_workspace_bytes": (_sz, [_i64, _i64]),
    "mvf_assign": (_i, [_p, _i64, _p, _i64, C.POINTER(AssignLayer), _i, _p, _d, _d, _d, _p, _p, _p, _p, _p, _p, _p, _sz, _i,
                        _p]),
    "mvf_assign_dense": (_i, [_p, _i64, _p, _i64, C.POINTER(AssignLayer), _i, _p, _d, _d, _d, _p, _p, _p, _p, _p, _p, _p, _p,
                              _sz, _i, _p]),
    "mvf_assign_topk_workspace_bytes": (_sz, [_i64, _i64, _i]),
    "mvf_assign_topk": (_i, [_p, _i64, _p, _i64, C.POINTER(AssignLayer), _i, _p, _d, _d, _d, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                             _sz, _i, _p]),
    "mvf_assign_best_workspace_bytes": (_sz, [_i64, _i64]),
    "mvf_assign_best": (_i, [_p, _i64, _p, _i64, C.POINTER(AssignLayer), _i, _p, _d, _d, _d, _p, _p, _p, _p, _p, _sz, _i, _p]),
    "mvf_assign_apply_workspace_bytes": (_sz, [_i64, _i64, _i, _i]),
    "mvf_assign_apply": (_i, [_p, _i64, _p, _i64, C.POINTER(AssignLayer), _i, _p, _d, _d, _d, _p, _i, _i64, _p, _p, _i, _i64, _p,
                              _p, _p, _p, _sz, _i, _p]),
    "mvf_assign_layer_stats_workspace_bytes": (_sz, [_i64, _i64, _i]),
    "mvf_assign_layer_stats": (_i, [C.POINTER(AssignLayer), _i64, _i64, _i, _p, _p, _p, _p, _p, _sz, _i, _p]),
    "mvf_align_alpha": (_i, [_p, _p, _p, _i64, _d, _d, _p, _p, _p]),
    "mvf_align_workspace_bytes": (_sz, [_i64, _i64]),
    "mvf_align_moments": (_i, [_p, _p, _p, _p, _p, _p, _p, _i64, _p, _p, _i64, C.POINTER(C.c_double), _p, _p, _p, _sz, _i, _p]),
    "mvf_align_transform": (_i, [_p, _p, _p, _p, _i64, C.POINTER(C.c_double), C.POINTER(C.c_double), _p, _p, _p, _p, _p, _p, _i,
                                 _p]),
    "mvf_align_gather": (_i, [_p, _i64, _i64, _i64, _p, _p, _p, _p, C.POINTER(AssignLayer), _i, C.POINTER(_p), C.POINTER(_p), _i,
                              _p]),
    "mvf_align_alpha_svi": (_i, [_p, _p, _p, _i64, _d, _d, _d, _p, _p, _p]),
    "mvf_align_transform_svi": (_i, [_p, _p, _p, _i64, C.POINTER(C.c_double), _d, _p, _p, _p, _i, _p]),
    "mvf_colmeans_workspace_bytes": (_sz, [_i64, _i64]),
    "mvf_colmeans": (_i, [_p, _i, _i64, _i64, _i64, _i64, _p, _p, _sz, _p]),
    "mvf_ublk_pack": (_i, [_p, _i, _i64, _i64, _p, _i64, _i64, _p, _sz, _i, _p]),
    "mvf_colmeans_csr": (_i, [_p, _p, _p, _i, _i64, _i64, _i64, _i64, _p, _p, _sz, _p, _sz, _p]),
    "mvf_ublk_pack_csr": (_i, [_p, _p, _p, _i, _i64, _i64, _p, _i64, _i64, _p, _sz, _p, _sz, _i, _p]),
    "mvf_trn": (_i, [C.POINTER(TrnProblem), _i, _p]),
    "mvf_nearest_rows_workspace_bytes": (_sz, [_i64, _i64]),
    "mvf_nearest_rows": (_i, [_p, _i64, _i, _p, _i64, _p, _p, _sz, _p]),
    "mvf_kmeans_workspace_bytes": (_sz, [_i64, _i64]),
    "mvf_kmeans": (_i, [_p, _i64, _i, _p, _i64, _i, _p, _p, _p, _sz, _p]),
    "mvf_icp_batch_workspace_bytes": (_sz, [_i64]),
    "mvf_icp_batch": (_i, [C.POINTER(IcpProblem), _i64, _i, _d, _d, _d, _i, _i, _p, _sz, _p]),
    "mvf_mesh_loss_workspace_bytes": (_sz, [_i64, _i64]),
    "mvf_mesh_loss": (_i, [_p, _i64, _p, _i64, C.POINTER(C.c_double), _p, _i64, _p, _p, _p, _i64, _i64, _i, _d, _d, _d, _i, _p, _p,
                           _p, _p, _sz, _p]),
    "mvf_mesh_contours": (_i, [_p, _i64, _p, _i64, C.POINTER(C.c_double), C.POINTER(C.c_double), _p, _i64, _i64, _p, _p, _p]),
    "mvf_kde_workspace_bytes": (_sz, [_i64, _i64, _i]),
    "mvf_kde": (_i, [_p, _i64, _p, _i64, _i, _i, _d, _p, _p, _i, _p, _p, _sz, _i, _p]),
    "mvf_shape_descriptors_workspace_bytes": (_sz, [_i64, _i]),
    "mvf_shape_descriptors": (_i, [_p, _i64, _p, _p, _i, _i, C.POINTER(C.c_double), _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "mvf_heat_grid_workspace_bytes": (_sz, [_i64, _i64]),
    "mvf_heat_grid": (_i, [_p, _p, _p, _i64, _i64, _d, _d, _i, _p, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int),
                           _p, _sz, _p]),
    "mvf_heat_graph_workspace_bytes": (_sz, [_i64, _i64]),
    "mvf_heat_graph": (_i, [_p, _p, _p, _p, _i64, _d, _d, _p, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int), _p,
                            _sz, _p]),
    "mvf_knn_workspace_bytes": (_sz, [_i64, _i, _i]),
    "mvf_knn": (_i, [_p, _i64, _i, _i, _p, _p, _p, _sz, _p]),
    "mvf_graph_sssp": (_i, [_p, _p, _p, _i64, _i64, _p, _i64, _p, _i64, _i, _i, _p, _p]),
    "mvf_pinv_diag_cached": (_i, [_p, _sz, _i64, _i64, _d, _i, _p, _p, _sz, _i, _p]),
}

_lib = None


class MVFError(RuntimeError):
    """Raised when a libmvf entry point returns a non-zero status."""


def check_converged(sweeps):
    """mvf_solve_minnorm(_lr) report a sweep count (einfo[EINFO_SWEEPS]) of x.5 when the Jacobi iteration hit its sweep cap
    before a clean sweep: the factor is then not orthogonal and the truncated back-solve is not an eigen-solve - fail loudly."""
    if float(sweeps) % 1.0 != 0.0:
        raise MVFError(f"coefficient solve failed: the Jacobi eigensolver did not converge in {int(sweeps)} "
                       f"sweeps (non-finite or wildly scaled Gram system?)")


def load():
    """Load libmvf.so (once).  Fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (or `make -C spateo-release_amd/csrc`). There is no CPU fallback for this path."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    if DEV_KNOBS:
        import sys

        applied = {}
        for env, (opt, parse) in _LEGACY_ENV.items():
            if env in os.environ:
                applied[opt] = int(parse(os.environ[env]))
                check(lib.mvf_debug_option(opt.encode(), applied[opt]), "mvf_debug_option")
        print(f"[spateo_amd] MVF_DEV_KNOBS=1: library {LIB_PATH}, developer options {applied}", file=sys.stderr, flush=True)
    return lib


OPTION_EPOCH = [0]  # bumped by every debug_option call: what callers key their cached launch-plan sizes with


def debug_option(name, value):
    """Set a developer option of the library (mvf.h: mvf_debug_option); returns the previous value."""
    OPTION_EPOCH[0] += 1
    lib = load()
    old = int(lib.mvf_debug_option_get(name.encode()))
    check(lib.mvf_debug_option(name.encode(), int(value)), "mvf_debug_option")
    return old


def debug_options():
    """{name: value} of the developer options that are not at their default (0)."""
    lib = load()
    vals = {n: int(lib.mvf_debug_option_get(n.encode())) for n in DEBUG_OPTIONS}
    return {n: v for n, v in vals.items() if v != 0}


def check(rc, what=""):
    if rc != 0:
        msg = load().mvf_last_error().decode("utf-8", "replace")
        raise MVFError(f"libmvf {what} failed: {msg}")


def device_count() -> int:
    n = C.c_int(0)
    check(load().mvf_device_count(C.byref(n)), "mvf_device_count")
    return n.value
