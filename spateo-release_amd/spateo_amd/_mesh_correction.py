"""``Mesh_correction`` of ``spateo.alignment`` (``alignment/methods/morpho_mesh_correction.py`` and ``mesh_correction_utils.py``):
the z-stack of aligned slices corrected against a surface mesh of the organ - a discrete search over five parameters of the mesh
(three Euler angles, a z translation, a scale), whose cost is one ICP per slice between the slice's contour and the mesh cut at
the slice's height, then one rigid map per slice onto the corrected mesh.

The hot path runs on the device in float64 (csrc/mvf_icp.hip): ``mvf_mesh_loss`` evaluates all ``10 label_num^2`` candidate
transformations of an optimisation step in one call - transform, cut, thin and ICP inside one workgroup per (transformation,
slice) -, ``mvf_icp_batch`` runs independent ICPs, ``mvf_mesh_contours`` writes the cut out.  ``align.py`` re-exports the names.

The reference's module cannot run as it lies (it imports pyvista, shapely, cv2 and a compiled ``libfastpd`` that is not in its
tree, and ``perform_correction`` calls an ``_eliminate_shift`` defined nowhere): this is a rebuild of its evident design.  What
can be pinned against its code is pinned (``ICP``, the label grid, the pair list, the smoothing, ``_transform_points`` at zero
translation; tests/golden/make_golden_mesh_correction.py).  Four deviations, each documented where it acts:

  1. z translation: added to z of every vertex, as the reference's docstring says; its line adds it to the first two ROWS.
  2. exact labelling: the ``L^5`` labellings are enumerated instead of fastPD's approximate search.
  3. deterministic thinning: a contour above ``subsample`` points keeps the rows ``floor(j n / subsample)`` instead of a draw
     from NumPy's global generator.
  4. ``perform_correction`` completes a function the reference leaves undefined.
"""
from __future__ import annotations

import itertools

import numpy as np

from . import _lib
from . import _runtime as _rt

__all__ = ["icp", "icp_batch", "mesh_contours", "mesh_correction_loss", "Mesh_correction"]

GAMMA_THRESHOLD = 0.05                 # `gamma = np.sum(distances < 0.05) / M` (mesh_correction_utils.py:490)
LABELLING_MAX_BYTES = 64 << 20         # the table of all L^5 labellings, float64
LABEL_NUM_MAX = int((LABELLING_MAX_BYTES // 8) ** 0.2 + 1e-9)  # 24


# ---- meshes ----
class _Mesh:
    """points (V, 3) float64, triangles (F, 3) int64, their unique edges (E, 2) int32: what the kernels read."""

    def __init__(self, points, triangles, edges=None):
        self.points = np.array(points, dtype=np.float64)
        self.triangles = triangles
        self.edges = mesh_edges(triangles) if edges is None else edges

    def copy(self):
        return _Mesh(self.points, self.triangles, self.edges)


def mesh_edges(triangles):
    """The unique edges ``(a < b)`` of the triangles, sorted by ``(a, b)``: int32 (E, 2).  Their order is the order of the cut."""
    t = np.asarray(triangles, dtype=np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    return np.unique(np.sort(e, axis=1), axis=0).astype(np.int32)


def _as_mesh(mesh, who):
    """``(points, triangles)`` or any object with ``.points`` and a pyvista-style flat ``.faces`` (``[3, a, b, c, 3, ...]``;
    pyvista itself is never imported).  Cells that are not triangles are refused by name."""
    if isinstance(mesh, _Mesh):
        return mesh
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        points, tri = mesh
        tri = np.asarray(tri)
        if tri.ndim != 2 or tri.shape[1] != 3:
            raise NotImplementedError(f"{who}: triangles of shape {tri.shape} are not supported: only triangle cells are, pass an "
                                      f"(F, 3) index array (triangulate the surface first)")
    elif hasattr(mesh, "points") and hasattr(mesh, "faces"):
        points, faces = mesh.points, np.asarray(mesh.faces).reshape(-1)
        if len(faces) % 4 or (faces[0::4] != 3).any():
            raise NotImplementedError(f"{who}: the mesh has cells that are not triangles (a flat `faces` array must read "
                                      f"[3, a, b, c, 3, ...]): only triangle cells are supported, triangulate the surface first")
        tri = faces.reshape(-1, 4)[:, 1:]
    else:
        raise TypeError(f"{who}: a mesh is (points, triangles) or an object with .points and a flat .faces, got {type(mesh).__name__}")
    points = np.asarray(points, dtype=np.float64)
    tri = np.asarray(tri, dtype=np.int64)
    if points.ndim != 2 or points.shape[1] != 3 or len(points) < 1 or not np.isfinite(points).all():
        raise ValueError(f"{who}: mesh points must be a finite (V >= 1, 3) array, got shape {points.shape}")
    if len(tri) < 1 or tri.min() < 0 or tri.max() >= len(points):
        raise ValueError(f"{who}: the triangles must index the {len(points)} points and there must be at least one")
    return _Mesh(points, tri)


def _euler_matrix(rotation):
    """``R_z R_y R_x`` for Euler angles in degrees about x, y, z, written out entry by entry."""
    ax, ay, az = np.deg2rad(np.asarray(rotation, dtype=np.float64).reshape(3))
    (cx, sx), (cy, sy), (cz, sz) = ((np.cos(a), np.sin(a)) for a in (ax, ay, az))
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                     [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                     [-sy, cy * sx, cy * cx]])


def _transform_points(points, rotation, translation, scaling):
    """The mesh transform of ``_transform_points`` (mesh_correction_utils.py:27-85): about the vertex mean, rotate by
    ``R_z R_y R_x``, scale, and shift along z.  Deviation 1: ``translation`` moves z of every vertex - what the reference's
    docstring says - where its line ``transformed_points[:2] += translation`` adds it to the first two rows.  At translation 0
    the two agree to rounding, and that is pinned against the real function."""
    points = np.asarray(points, dtype=np.float64)
    centre = points.mean(axis=0)
    moved = scaling * ((points - centre) @ _euler_matrix(rotation).T) + centre
    moved[:, 2] += translation
    return moved


def _param_row(rotation, translation, scaling):
    r = np.asarray(rotation, dtype=np.float64).reshape(-1)
    if r.shape != (3,):
        raise ValueError(f"rotation must hold three Euler angles in degrees, got shape {r.shape}")
    row = np.array([r[0], r[1], r[2], float(translation), float(scaling)])
    if not np.isfinite(row).all():
        raise ValueError("rotation, translation and scaling must be finite")
    return row


# ---- contours ----
def _contour(c, who, what="contour"):
    c = np.ascontiguousarray(c, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != 2:
        d = c.shape[1] if c.ndim == 2 else None
        if d is not None and d > 2:
            raise NotImplementedError(f"{who}: {what} has D = {d} columns: ICP in D != 2 dimensions is not supported, only 2-D "
                                      f"contours are")
        raise ValueError(f"{who}: {what} must be an (n, 2) array, got shape {c.shape}")
    if len(c) < 1 or not np.isfinite(c).all():
        raise ValueError(f"{who}: {what} must hold at least one point and only finite numbers")
    return c


def _icp_args(who, max_iter, error_threshold, inlier_threshold, subsample):
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f"{who}: max_iter must be an integer >= 1, got {max_iter!r}")
    subsample = int(subsample)
    if subsample > _lib.ICP_MAX_POINTS:
        raise NotImplementedError(f"{who}: subsample = {subsample} is not supported: at most {_lib.ICP_MAX_POINTS} "
                                  f"(_lib.ICP_MAX_POINTS; both contours of a problem live in one workgroup's LDS)")
    return int(max_iter), float(error_threshold), float(inlier_threshold), subsample


def _thin(c, subsample):
    n = len(c)
    return c[(np.arange(subsample, dtype=np.int64) * n) // subsample] if 0 < subsample < n else c


def _closing_solve(T_contour_2, contour_2):
    """The solve that closes ``ICP`` with rotation (``solve_RT_by_correspondence`` of mesh_correction_utils.py:501-553, called
    at :496 with ``X = T_contour_2, Y = contour_2``): the PROPER rotation ``R`` - a reflection is corrected by flipping the last
    right singular vector, unlike ``st.align.solve_RT_by_correspondence`` (alignment/utils.py), which is the same ``R`` wherever
    ``det R > 0`` - of the rigid map ``T_contour_2 ~ contour_2 R^T + t_forward``.  Returns ``(R, t_reference, t_forward)``:
    ``t_reference = mean(contour_2) - mean(T_contour_2) R^T`` is the expression the reference returns (it pairs this ``R`` with
    the means the other way round, so it is NOT the translation of that map); ``t_forward = mean(T_contour_2) -
    mean(contour_2) R^T`` is."""
    mean_T, mean_2 = T_contour_2.mean(axis=0), contour_2.mean(axis=0)
    U, _, Vt = np.linalg.svd((contour_2 - mean_2).T @ (T_contour_2 - mean_T))
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt[-1] *= -1
        R = Vt.T @ U.T
    return R, mean_2 - mean_T @ R.T, mean_T - mean_2 @ R.T


def _run_icp(who, contours_1, contours_2, max_iter, error_threshold, inlier_threshold, subsample, allow_rotation, device):
    """Validation and the device call shared by ``icp_batch`` and ``perform_correction``: per pair ``(gamma, shift, kept_1,
    kept_2, T_contour_2)`` - the thinned contours as the kernel saw them, ``shift`` the no-rotation translation."""
    if len(contours_1) != len(contours_2):
        raise ValueError(f"{who}: {len(contours_1)} data contours but {len(contours_2)} model contours")
    max_iter, error_threshold, inlier_threshold, subsample = _icp_args(who, max_iter, error_threshold, inlier_threshold, subsample)
    c1 = [_contour(c, who, f"contour_1[{i}]") for i, c in enumerate(contours_1)]
    c2 = [_contour(c, who, f"contour_2[{i}]") for i, c in enumerate(contours_2)]
    for i, (a, b) in enumerate(zip(c1, c2)):
        if subsample <= 0 and max(len(a), len(b)) > _lib.ICP_MAX_POINTS:
            raise NotImplementedError(f"{who}: pair {i} has {len(a)} and {len(b)} points and subsample = {subsample} thins nothing: "
                                      f"at most {_lib.ICP_MAX_POINTS} points per contour (_lib.ICP_MAX_POINTS) are supported")
    if not c1:
        return []
    k = _rt._shared_kernels(device, "float64")
    gamma, _, shift, Ts = k.icp_batch(c1, c2, max_iter, error_threshold, inlier_threshold, GAMMA_THRESHOLD, subsample, allow_rotation)
    return [(float(gamma[i]), shift[i], _thin(c1[i], subsample), _thin(c2[i], subsample), Ts[i]) for i in range(len(c1))]


def icp_batch(contours_1, contours_2, max_iter=20, error_threshold=1e-6, inlier_threshold=0.1, subsample=500,
              allow_rotation=False, device=None):
    """``icp`` for lists of contour pairs in one call (``mvf_icp_batch``: one workgroup per pair, 4096 pairs per launch).
    Returns the list of ``icp``'s tuples."""
    out = []
    for gamma, shift, kept_1, kept_2, T in _run_icp("icp_batch", contours_1, contours_2, max_iter, error_threshold, inlier_threshold,
                                                    subsample, allow_rotation, device):
        R, t = _closing_solve(T, kept_2)[:2] if allow_rotation else (np.eye(2), shift)
        out.append((gamma, 0, t, kept_1, T, R))
    return out


def icp(contour_1, contour_2, max_iter=20, error_threshold=1e-6, inlier_threshold=0.1, subsample=500, allow_rotation=False,
        device=None):
    """``ICP`` of ``mesh_correction_utils.py:404-498`` with its signature and return tuple ``(gamma, 0, translation, contour_1,
    T_contour_2, Rotation)``, every round on the device (``mvf_icp_batch``, float64): ``contour_1`` (N, 2) is the data,
    ``contour_2`` (M, 2) the model that moves; ``gamma`` the share of model points within 0.05 (normalised units) of the data
    at the last query; ``T_contour_2`` the moved model points in the frame of ``contour_1``.

    ``allow_rotation=False``: ``Rotation`` is the identity and ``translation`` what the reference returns - the LAST round's
    translation, de-normalised.  ``True``: ``(Rotation, translation)`` are the reference's too, from its closing solve restated
    on the host (``_closing_solve``; mesh_correction_utils.py:496, :501-553): ``Rotation`` is the PROPER rotation of the rigid
    map ``T_contour_2 ~ contour_2 R^T + t`` - inside the rounds no determinant is corrected, a round may reflect, and then
    ``T_contour_2`` is a mirror image no proper rotation reproduces -, and ``translation`` is the reference's expression
    ``mean(contour_2) - mean(T_contour_2) R^T``, which is NOT the ``t`` of that map (the reference pairs ``R`` with the means
    the other way round; the map's own is ``mean(T_contour_2) - mean(contour_2) R^T``, what ``perform_correction`` uses).  This
    is the solve of the reference's mesh module, not ``st.align.solve_RT_by_correspondence`` (alignment/utils.py), which
    corrects no reflection and returns the map's own ``t``.

    Deviation 3: a contour above ``subsample`` points is thinned to the rows ``floor(j n / subsample)``, where the reference
    draws ``np.random.choice``; the returned ``contour_1`` and the rows of ``T_contour_2`` are the thinned ones, as there.  Pass
    contours you have thinned yourself to use another draw.  ``subsample`` above ``_lib.ICP_MAX_POINTS`` and contours with
    D != 2 columns: ``NotImplementedError``."""
    return icp_batch([contour_1], [contour_2], max_iter, error_threshold, inlier_threshold, subsample, allow_rotation, device)[0]


def _heights(z_values, who):
    z = np.ascontiguousarray(z_values, dtype=np.float64).reshape(-1)
    if len(z) < 1 or not np.isfinite(z).all():
        raise ValueError(f"{who}: z_values must hold at least one finite height")
    return z


def mesh_contours(mesh, z_values, rotation=(0.0, 0.0, 0.0), translation=0.0, scaling=1.0, device=None):
    """The contours of a triangle mesh at the heights ``z_values`` after ``_transform_points(points, rotation, translation,
    scaling)`` (deviation 1: the translation moves z): per height one (n, 2) array with one point per mesh edge whose ends
    classify differently under ``z >= height`` - VTK's contour rule, a vertex on the plane counts as above it -, the linear
    interpolate in x and y, in the order of the mesh's unique sorted edges; (0, 2) where the plane misses the mesh.  On the
    device (``mvf_mesh_contours``).  Replaces ``_extract_contours_from_mesh`` (``mesh.contour(isosurfaces=z_values)``)."""
    m = _as_mesh(mesh, "mesh_contours")
    z = _heights(z_values, "mesh_contours")
    k = _rt._shared_kernels(device, "float64")
    return k.mesh_contours(k.mesh_upload(m.points, m.edges), m.points.mean(axis=0), _param_row(rotation, translation, scaling), z)


def mesh_correction_loss(contours, mesh, transformations, z_values, max_iter=20, error_threshold=1e-6, inlier_threshold=0.1,
                         subsample=500, return_details=False, device=None):
    """``_calculate_loss`` (mesh_correction_utils.py:371-401) for every row of ``transformations`` (n_T, 5: three Euler angles in
    degrees, z translation, scale) in ONE call (``mvf_mesh_loss``): the mesh transformed, cut at every height of ``z_values``,
    and ``loss = sum_s (1 - gamma_s) / n_slices`` with ``gamma_s`` of ``icp(contours[s], cut_s, allow_rotation=True)``;
    ``1e6 / n_slices`` where any height cuts nothing.  Returns ``loss`` (n_T,) float64 - a float for a single 5-vector -;
    ``return_details``: also ``gamma`` (n_T, n_slices) and the sizes of the cuts before thinning (n_T, n_slices).
    Deviations 1 and 3 apply."""
    who = "mesh_correction_loss"
    m = _as_mesh(mesh, who)
    z = _heights(z_values, who)
    if len(contours) != len(z):
        raise ValueError(f"{who}: {len(contours)} contours but {len(z)} heights")
    cs = [_contour(c, who, f"contours[{i}]") for i, c in enumerate(contours)]
    P = np.asarray(transformations, dtype=np.float64)
    single = P.ndim == 1
    P = np.ascontiguousarray(P.reshape(-1, 5) if P.size else P.reshape(0, 5))
    if not np.isfinite(P).all():
        raise ValueError(f"{who}: non-finite transformation parameters")
    max_iter, error_threshold, inlier_threshold, subsample = _icp_args(who, max_iter, error_threshold, inlier_threshold, subsample)
    if subsample < 1:
        raise ValueError(f"{who}: subsample must be at least 1 (the size of a cut is not known beforehand), got {subsample}")
    k = _rt._shared_kernels(device, "float64")
    loss, gamma, count = k.mesh_loss(k.mesh_upload(m.points, m.edges), m.points.mean(axis=0), P, z, cs, max_iter, error_threshold,
                                     inlier_threshold, GAMMA_THRESHOLD, subsample)
    if single:
        return (float(loss[0]), gamma[0], count[0]) if return_details else float(loss[0])
    return (loss, gamma, count) if return_details else loss


# ---- the discrete optimisation's host side ----
def _generate_labeling(max_value, number_of_steps, scale_type="linear"):
    """The label values of ``_generate_labeling`` (mesh_correction_utils.py:246-284), bit for bit: ``number_of_steps`` values
    ``-max_value + k step`` over ``[-max_value, max_value]`` (linear) or ``exp`` of such a ramp over ``[-log max_value,
    log max_value]`` (log).  The neutral value - 0 or 1, "no change" - goes to position 0: an odd count hits it and it is moved
    there; an even count misses it and position 0 is overwritten with it."""
    if scale_type not in ("linear", "log"):
        raise ValueError(f"Unknown scale_type: {scale_type}")
    log = scale_type == "log"
    half = np.log(max_value) if log else max_value
    step = half * 2.0 / (number_of_steps - 1)
    ramp = [-half + k * step for k in range(number_of_steps)]
    values = [np.exp(v) for v in ramp] if log else ramp
    unit = 1 if log else 0
    labels = [v for v in values if v == unit][::-1] + [v for v in values if v != unit]
    if number_of_steps % 2 == 0:
        labels[0] = unit
    return labels


def _update_parameter(transformation_labels, parameters):
    """The grid recentred on a transformation (``_update_parameter``, :287-293): its angles and translation are added to the
    first four columns, its scale multiplies the fifth.  Returns a new array."""
    shift = np.concatenate([np.asarray(parameters["rotation"], dtype=np.float64).reshape(3), [parameters["translation"], 0.0]])
    factor = np.array([1.0, 1.0, 1.0, 1.0, parameters["scaling"]])
    return (np.asarray(transformation_labels, dtype=np.float64) + shift) * factor


def _make_pairs(nVars=5):
    """``_make_pairs`` (:297-300): the 10 unordered pairs of the 5 parameters, int32."""
    return np.array(list(itertools.combinations(np.arange(nVars), 2)), dtype=np.int32)


def _get_parameters_from_pair(pair, transformation_labels):
    """``_get_parameters_from_pair`` (:307-320): (L, L, 5) - label row 0 ("no change") with parameter ``pair[0]`` set to its
    label i and ``pair[1]`` to its label j."""
    L = transformation_labels.shape[0]
    out = np.broadcast_to(transformation_labels[0], (L, L, 5)).copy()
    out[:, :, pair[0]] = transformation_labels[:, pair[0]][:, None]
    out[:, :, pair[1]] = transformation_labels[:, pair[1]][None, :]
    return out


def _smooth_contours(vertex, window_size=5, iterations=1):
    """The cyclic moving average of ``_smooth_contours`` (:190-221), bit for bit: point i becomes the mean of the ``2
    window_size`` points ``i - window_size .. i + window_size - 1`` of the contour as it stood BEFORE the pass (the window is
    one short of symmetric, as in the reference), the rows added in rising order.  A list of new arrays."""
    w = int(window_size)
    out = []
    for contour in vertex:
        cur = np.array(contour, dtype=np.float64)
        n = len(cur)
        for _ in range(iterations):
            ring = np.concatenate([cur[n - w:], cur, cur[:w]])
            acc = ring[0:n].copy()
            for k in range(1, 2 * w):
                acc += ring[k:k + n]
            cur = acc / (2 * w)
        out.append(cur)
    return out


def solve_labeling(binaries, pairs, n_vars=5):
    """The labelling that minimises ``sum_pairs binaries[p][l[pairs[p, 0]], l[pairs[p, 1]]]`` over all ``L^n_vars`` labellings,
    EXACTLY, by enumeration (deviation 2: the reference hands the tables to fastPD, an approximate solver; its unary terms are
    all 1 and change no argmin).  The tables are added in pair order in float64; among equal sums the lowest flat index wins
    (parameter 0 the slowest digit), so label 0 - "no change" - is preferred.  Returns (labels (n_vars,) int64, the minimum)."""
    binaries = [np.asarray(b, dtype=np.float64) for b in binaries]
    L = binaries[0].shape[0]
    if L ** n_vars * 8 > LABELLING_MAX_BYTES:
        raise NotImplementedError(f"label_num = {L} is not supported: the exact labelling enumerates label_num^{n_vars} float64 sums "
                                  f"and is capped at {LABELLING_MAX_BYTES >> 20} MB, label_num <= {LABEL_NUM_MAX}")
    total = np.zeros((L,) * n_vars)
    for b, (i, j) in zip(binaries, np.asarray(pairs)):
        shape = [1] * n_vars
        shape[i], shape[j] = L, L
        total += b.reshape(shape)
    flat = int(np.argmin(total))
    return np.array(np.unravel_index(flat, total.shape), dtype=np.int64), float(total.reshape(-1)[flat])


def _spatial_2d(model, key):
    return np.asarray(model.obsm[key], dtype=np.float64)[:, :2]


class Mesh_correction:
    """``Mesh_correction`` of ``morpho_mesh_correction.py:39-365`` with its constructor signature and defaults: a 3-D
    reconstruction from slices corrected against a mesh.

    ``slices``: ``AnnDataLite`` or, by duck typing, AnnData (only ``.obsm`` is touched); ``mesh``: ``(points, triangles)`` or an
    object with ``.points`` and a pyvista-style flat ``.faces`` (triangles only; pyvista is never imported).  Beyond the
    reference: ``contours=`` (one (n, 2) array per slice, see ``set_contours``), ``seed=`` for the draw of ``subsample_slices``
    (an index array is taken as the draw itself), ``device=``.  ``fastpd_iter`` and ``multi_processing`` are accepted and
    ignored: the labelling is solved exactly (``solve_labeling``) and all candidates of a step run in one device call.

    Attributes as in the reference: ``losses``, ``transformations``, ``best_loss``, ``best_transformation``, ``contours``; after
    ``perform_correction`` also ``rotations`` and ``translations``."""

    def __init__(self, slices, z_heights, mesh, spatial_key="spatial", key_added="align_spatial", normalize_spatial=False,
                 init_rotation=np.array([0.0, 0.0, 0.0]), init_translation=0.0, init_scaling=1.0, max_rotation_angle=180,
                 max_translation_scale=0.5, max_scaling=1.5, min_rotation_angle=10, min_translation_scale=1, min_scaling=1.1,
                 label_num=15, fastpd_iter=100, max_iter=10, anneal_rate=0.7, multi_processing=False, subsample_slices=None,
                 verbose=False, *, contours=None, seed=None, device=None):
        self.slices = list(slices)
        self.n_slices = len(self.slices)
        if not all(spatial_key in s.obsm.keys() for s in self.slices):
            raise ValueError("All slices must have the same spatial key in the '.obsm' attribute.")
        self.spatial_key = spatial_key
        self.slices_spatial = [np.asarray(s.obsm[spatial_key]) for s in self.slices]
        if z_heights is None:
            raise ValueError("z_heights must be provided.")
        self.z_heights = np.asarray(z_heights, dtype=np.float64).reshape(-1)
        if len(np.unique(self.z_heights)) != len(self.z_heights):
            raise ValueError("z_heights must be unique value.")
        if len(self.z_heights) != self.n_slices:
            raise ValueError("z_heights must have the same length as the number of slices.")
        if int(label_num) != label_num or label_num < 2:
            raise ValueError(f"label_num must be an integer >= 2, got {label_num!r}")
        if label_num > LABEL_NUM_MAX:
            raise NotImplementedError(f"label_num = {label_num} is not supported: the exact labelling enumerates label_num^5 float64 "
                                      f"sums and is capped at {LABELLING_MAX_BYTES >> 20} MB, label_num <= {LABEL_NUM_MAX}")
        self.mesh = _as_mesh(mesh, "Mesh_correction").copy()
        self.key_added = key_added
        self.normalize_spatial = normalize_spatial
        self.set_init_parameters(init_rotation, init_translation, init_scaling)
        self.normalize_mesh_spatial_coordinates()
        self.max_rotation_angle = max_rotation_angle
        self.max_translation_scale = max_translation_scale
        self.max_scaling = max_scaling
        self.min_rotation_angle = min_rotation_angle
        self.min_translation_scale = min_translation_scale
        self.min_scaling = min_scaling
        self.label_num = int(label_num)
        self.fastpd_iter = fastpd_iter
        self.max_iter = max_iter
        self.anneal_rate = anneal_rate
        self.multi_processing = multi_processing
        self.subsample_slices = subsample_slices
        self.verbose = verbose
        self.seed = seed
        self.device = device
        self.contours = [None] * self.n_slices
        self.labels = []
        if contours is not None:
            self.set_contours(contours)

    def set_init_parameters(self, init_rotation=np.array([0.0, 0.0, 0.0]), init_translation=0.0, init_scaling=1.0):
        """The mesh moved by the start transformation (``_transform_points``; deviation 1: the translation moves z)."""
        self.mesh.points = _transform_points(self.mesh.points, init_rotation, init_translation, init_scaling)

    def normalize_mesh_spatial_coordinates(self):
        """``normalize_mesh_spatial_coordinates`` (:147-183): ``slices_scale`` = the range of the z heights; with
        ``normalize_spatial`` the mesh is centred at its mid-range, scaled so that its z range equals it, and moved to the
        mid-range of the slices (x, y) and of the heights (z)."""
        self.slices_scale = self.z_heights.max() - self.z_heights.min()
        if self.normalize_spatial:
            pts = self.mesh.points
            mesh_scale = pts[:, 2].max() - pts[:, 2].min()
            slices_mean_z = (self.z_heights.max() + self.z_heights.min()) / 2
            xy = np.concatenate([np.asarray(s, dtype=np.float64)[:, :2] for s in self.slices_spatial], axis=0)
            slices_mean_xy = (xy.max(axis=0) + xy.min(axis=0)) / 2
            mesh_mean = (pts.max(axis=0) + pts.min(axis=0)) / 2
            pts = (pts - mesh_mean) * self.slices_scale / mesh_scale
            pts[:, :2] += slices_mean_xy
            pts[:, 2] += slices_mean_z
            self.mesh.points = pts

    def set_contours(self, contours):
        """One (n, 2) contour per slice, from any source: what ``extract_contours`` would fill in."""
        contours = list(contours)
        if len(contours) != self.n_slices:
            raise ValueError(f"set_contours: {len(contours)} contours for {self.n_slices} slices")
        self.contours = [_contour(c, "set_contours", f"contours[{i}]") for i, c in enumerate(contours)]

    def extract_contours(self, method="alpha_shape", n_sampling=None, smoothing=True, window_size=5, filter_contours=True,
                         contour_filter_threshold=20, opencv_kwargs=None, alpha_shape_kwargs=None, seed=None):
        """``extract_contours`` (:185-239).  ``alphashape`` + ``shapely`` (``"alpha_shape"``) and ``cv2`` (``"opencv"``) are
        imported lazily: where they are missing an ``ImportError`` names the remedy - ``contours=`` in the constructor or
        ``set_contours(list)``.  ``"alpha_shape"`` takes the exterior of every polygon ``alphashape.alphashape(points, alpha)``
        returns, as the reference does; filtering and smoothing are restated here.  The rasterisation behind ``"opencv"`` is not
        restated: ``NotImplementedError`` (``opencv_kwargs`` is accepted for the signature's sake).  ``n_sampling`` draws with
        ``np.random.default_rng(seed)``.  A slice left without a contour is a ``ValueError`` (the reference would go on with an
        empty array and crash in the first ICP)."""
        if method not in ("opencv", "alpha_shape"):
            raise NotImplementedError(f"Method {method} is not implemented.")
        try:
            if method == "alpha_shape":
                import alphashape
                from shapely.geometry import MultiPolygon, Polygon
            else:
                import cv2
        except ImportError as e:
            raise ImportError(f"extract_contours(method={method!r}) needs {'alphashape and shapely' if method == 'alpha_shape' else 'cv2'}, "
                              f"which cannot be imported ({e}).  Remedy: extract the slice contours by any other means and pass them "
                              f"as `contours=` to the constructor or to `set_contours(list)` - one (n, 2) array per slice.") from e
        if method == "opencv":
            raise NotImplementedError(f"extract_contours(method='opencv'): cv2 {cv2.__version__} is there, but the rasterisation of "
                                      "`_extract_contour_opencv` (mesh_correction_utils.py:95-156) is not restated: use "
                                      "method='alpha_shape', or pass contours from any source to `set_contours(list)`")
        rng = np.random.default_rng(seed)
        found = []
        for index in range(self.n_slices):
            points = np.asarray(self.slices_spatial[index], dtype=np.float64)[:, :2]
            if n_sampling is not None and 0 < n_sampling < points.shape[0]:
                points = points[rng.choice(points.shape[0], n_sampling, replace=False)]
            shape = alphashape.alphashape(points, **dict({"alpha": 0.5}, **(alpha_shape_kwargs or {})))
            polys = [shape] if isinstance(shape, Polygon) else (list(shape.geoms) if isinstance(shape, MultiPolygon) else [])
            cur = [np.array(p.exterior.coords) for p in polys]
            if filter_contours:
                cur = [c for c in cur if c.shape[0] >= contour_filter_threshold]
            if smoothing:
                cur = _smooth_contours(cur, window_size)
            if not cur:
                raise ValueError(f"extract_contours: slice {index} is left without a contour (method {method!r}, "
                                 f"contour_filter_threshold {contour_filter_threshold})")
            found.append(np.concatenate(cur, axis=0))
        self.contours = found

    # -- the optimisation --
    def generate_labels(self):
        """``generate_labels`` (:330-347): (label_num, 5) - the grids of the three angles, the translation and the (log) scale
        around the best transformation so far; row 0 is the best transformation itself."""
        rotation_labels = _generate_labeling(self.max_rotation_angle, self.label_num)
        translation_labels = _generate_labeling(self.max_translation, self.label_num)
        scaling_labels = _generate_labeling(self.max_scaling, self.label_num, "log")
        labels = np.array([rotation_labels, rotation_labels, rotation_labels, translation_labels, scaling_labels], dtype=np.float64).T
        return _update_parameter(labels, self.best_transformation)

    def _evaluate(self, transformations):
        """The loss of every row of ``transformations`` (n, 5) on the (sub-sampled) slices: one device call."""
        return mesh_correction_loss(self.contours_subsample, self.mesh, transformations, self.z_heights_subsample, device=self.device)

    def discrete_optimization_step(self):
        """``discrete_optimization_step`` (:291-328): the label grid, the 10 pairs, the ``10 label_num^2`` parameter sets
        evaluated in ONE ``mesh_correction_loss`` call (duplicates once), the tables cast to float32 as the reference casts
        them, the exact labelling (deviation 2), and the loss of the chosen transformation.  Returns (loss, transformation)."""
        labels = self.generate_labels()
        pairs = _make_pairs()
        L = self.label_num
        sets = np.concatenate([_get_parameters_from_pair(p, labels).reshape(L * L, 5) for p in pairs], axis=0)
        uniq, inverse = np.unique(sets, axis=0, return_inverse=True)
        losses = np.asarray(self._evaluate(uniq), dtype=np.float64)[np.asarray(inverse).reshape(-1)]
        self.binaries = losses.astype(np.float32).reshape(len(pairs), L, L)
        chosen, _ = solve_labeling(self.binaries, pairs)
        self.labels.append(chosen)
        parameters = np.array([labels[chosen[i], i] for i in range(5)])
        loss = float(np.asarray(self._evaluate(parameters[None, :]))[0])
        return loss, {"rotation": parameters[:3], "translation": parameters[3], "scaling": parameters[4]}

    def run_discrete_optimization(self):
        """``run_discrete_optimization`` (:241-289): ``max_iter`` steps, each around the best transformation so far, the search
        ranges annealed by ``anneal_rate`` down to their minima after every step.  ``subsample_slices``: an integer below the
        slice count draws that many slices without replacement with ``np.random.default_rng(seed)`` (the reference draws from
        the global generator); an index array is taken as the draw."""
        if any(c is None for c in self.contours):
            raise ValueError("run_discrete_optimization: the slices have no contours yet: call extract_contours() or set_contours(list)")
        self.max_translation = self.max_translation_scale * self.slices_scale
        sub = self.subsample_slices
        if sub is not None and not np.isscalar(sub):
            self.subsample_slices = np.asarray(sub, dtype=np.int64).reshape(-1)
        elif sub is not None and 0 < sub < self.n_slices:
            self.subsample_slices = np.random.default_rng(self.seed).choice(self.n_slices, int(sub), replace=False)
        if isinstance(self.subsample_slices, np.ndarray):
            self.contours_subsample = [self.contours[i] for i in self.subsample_slices]
            self.z_heights_subsample = self.z_heights[self.subsample_slices]
        else:
            self.contours_subsample = self.contours
            self.z_heights_subsample = self.z_heights
        self.losses, self.transformations, self.labels = [], [], []
        self.best_loss = 1e8
        self.best_transformation = {"rotation": np.array([0.0, 0.0, 0.0]), "translation": 0.0, "scaling": 1.0}
        self.losses.append(self.best_loss)
        self.transformations.append(self.best_transformation)
        for i in range(self.max_iter):
            cur_loss, cur_transformation = self.discrete_optimization_step()
            if self.verbose:
                print(f"Iteration {i + 1}/{self.max_iter}, current loss: {cur_loss}")
            if cur_loss < self.best_loss:
                self.best_loss = cur_loss
                self.best_transformation = cur_transformation
            self.losses.append(cur_loss)
            self.transformations.append(cur_transformation)
            self.max_rotation_angle = max(self.max_rotation_angle * self.anneal_rate, self.min_rotation_angle)
            self.max_translation = max(self.max_translation * self.anneal_rate, self.min_translation_scale * self.slices_scale)
            self.max_scaling = max(self.max_scaling * self.anneal_rate, self.min_scaling)

    def perform_correction(self):
        """The correction itself.  Deviation 4: this COMPLETES a function the reference leaves undefined - its
        ``perform_correction`` (:349-365) transforms the mesh and then calls ``_eliminate_shift``, which exists nowhere.

        The best transformation is applied to the mesh; the mesh is cut at every slice's height; per slice one ICP moves the
        slice's contour (the model) onto the mesh's contour (the data), rotation allowed, and the closing solve
        (``_closing_solve``) gives the rigid map that carries the slice's frame onto the mesh - ``R_s`` always a proper
        rotation, so a slice is never mirrored even where a round of its ICP reflected, and ``t_s = mean(T) - mean(contour)
        R_s^T``, the translation of that map -: ``slices[s].obsm[key_added] = spatial @ R_s.T + t_s``.  ``rotations`` and ``translations`` keep the maps.  A height that
        misses the corrected mesh is a ``ValueError``."""
        if any(c is None for c in self.contours):
            raise ValueError("perform_correction: the slices have no contours yet: call extract_contours() or set_contours(list)")
        best = getattr(self, "best_transformation", None) or {"rotation": np.zeros(3), "translation": 0.0, "scaling": 1.0}
        self.mesh.points = _transform_points(self.mesh.points, best["rotation"], best["translation"], best["scaling"])
        cuts = mesh_contours(self.mesh, self.z_heights, device=self.device)
        empty = [i for i, c in enumerate(cuts) if len(c) == 0]
        if empty:
            raise ValueError(f"perform_correction: the heights of slices {empty} miss the corrected mesh")
        solved = [_closing_solve(T, kept_2) for _, _, _, kept_2, T in
                  _run_icp("perform_correction", cuts, self.contours, 20, 1e-6, 0.1, 500, True, self.device)]
        self.rotations = [R for R, _, _ in solved]
        self.translations = [t_forward for _, _, t_forward in solved]
        for s, R, t in zip(self.slices, self.rotations, self.translations):
            s.obsm[self.key_added] = _spatial_2d(s, self.spatial_key) @ R.T + t
        return self.slices

