"""``spateo.digitization`` (``st.dd``): layer, column and axis coordinates from the heat equation, on the device.

``digitize``, ``gridit`` and ``digitize_general`` of the reference (``spateo/digitization/grid.py``, ``utils.py``) rest on two
Jacobi relaxations written as whole-array NumPy loops: ``domain_heat_eqn_solver`` (``utils.py:464-524``, the 5-point average on
the raster of a slice) and ``digitize_general`` (``utils.py:527-575``, ``field @ adj_mtx`` with a dense N x N adjacency).  Here
both loops run in ``csrc/mvf_heat.hip`` (``mvf_heat_grid``, ``mvf_heat_graph``): the same operations in the same order, the same
stop rule with its quirks, the adjacency as CSC.  There is no CPU fallback.

On the host, restated from the reference: ``add_eh_boundary``, ``add_gh_boundary``, ``effective_L2_error``,
``field_contour_line``, ``field_contours``, ``gridit``.  ``neighbor_adjacency`` is a helper of OUR OWN: the reference gives no
recipe for the adjacency ``digitize_general`` takes.

Two deviations of ``digitize``, both because cv2 is never imported:
  * the rasterisation of the contour is ours - the border is the pixels of the chain ``cv2.findContours(...,
    CHAIN_APPROX_NONE)`` returns, the mask the border plus everything a 4-connected flood fill from outside cannot reach;
    ``cv2.drawContours`` cannot be run beside it to compare.  Any other contour is refused by name: pass ``field_border=`` /
    ``field_mask=``;
  * the mask is drawn with 1 where the reference draws it with ``ctr_idx + 1``, which scales the heat of every contour but the
    first by ``ctr_idx + 1``.

Not here: the borderline route (``get_borderline``, ``grid_borderline``, ``order_borderline``, ``extend_layer``,
``fill_grid_label``, ``draw_seg_grid``) and the cluster-contour functions, which are cv2 / skimage drawing.
"""
from __future__ import annotations

import numpy as np

from . import _runtime as _rt

__all__ = ["domain_heat_eqn_solver", "digitize_general", "digitize", "gridit", "neighbor_adjacency", "add_eh_boundary",
           "add_gh_boundary", "effective_L2_error", "field_contour_line", "field_contours", "rasterize_contour"]


# --------------------------------------------------------------------------------------------- restated from the reference
def add_eh_boundary(heat_field, field_line, value):
    """One heat value on a boundary line (``utils.py:400-417``): every point (x, y) of the line writes ``heat_field[y, x]``."""
    for x, y in field_line:
        heat_field[y, x] = value


def add_gh_boundary(heat_field, field_line, value_s, value_e):
    """Heat rising along a boundary line (``utils.py:420-442``): the k-th point (x, y) of the line writes the k-th sample of
    ``np.linspace(value_s, value_e, len(field_line))`` to ``heat_field[y, x]`` (a point met twice keeps the later sample)."""
    for (x, y), heat in zip(field_line, np.linspace(value_s, value_e, len(field_line))):
        heat_field[y, x] = heat


def effective_L2_error(heat_field_i, heat_field_j, field_mask):
    """``utils.py:445-461`` as written: the masked squared difference of the two fields over the masked square of the SECOND one,
    then the root.  The mask is a weight; an all-zero second field gives 0 / 0."""
    change = np.sum((heat_field_j - heat_field_i) ** 2 * field_mask)
    scale = np.sum(heat_field_j**2 * field_mask)
    return np.sqrt(change / scale)


def field_contour_line(ctr_seq, pnt_pos, min_pnt, max_pnt):
    """The side of the contour from ``min_pnt`` to ``max_pnt`` that passes no other corner (``utils.py:317-357``), as a list of the
    contour's points.  ``ctr_seq``: the contour as a list of (x, y) tuples, ``pnt_pos``: 1 at the four corners, else 0.

    The walk along the contour's own orientation starts at the FIRST occurrence of either point (``list.index``) and is taken
    when no corner lies strictly between the two.  Otherwise the walk against the orientation is taken, from the LAST occurrences
    (the reference searches the reversed list): when the forward walk had no wrap it runs down to the start of the list and on
    from its end, when it had one it runs straight down."""
    n = len(ctr_seq)
    a, b = ctr_seq.index(min_pnt), ctr_seq.index(max_pnt)
    wraps = a > b
    if wraps:
        ahead, between = [*range(a, n), *range(0, b + 1)], [*range(a + 1, n), *range(0, b)]
    else:
        ahead, between = [*range(a, b + 1)], [*range(a + 1, b)]
    if not any(pnt_pos[i] != 0 for i in between):
        return [ctr_seq[i] for i in ahead]
    backwards = ctr_seq[::-1]
    a, b = n - 1 - backwards.index(min_pnt), n - 1 - backwards.index(max_pnt)
    back = [*range(a, b - 1, -1)] if wraps else [*range(a, -1, -1), *range(n - 1, b - 1, -1)]
    return [ctr_seq[i] for i in back]


def _chain(contour):
    """A contour as an (n, 2) integer array of (x, y); (n, 1, 2) as cv2 hands it out, or (n, 2)."""
    c = np.asarray(contour)
    if c.ndim == 3 and c.shape[1] == 1:
        c = c[:, 0]
    if c.ndim != 2 or c.shape[1] != 2 or len(c) == 0:
        raise ValueError(f"a contour must have shape (n, 1, 2) or (n, 2) with n >= 1, got {np.shape(contour)}")
    if not np.issubdtype(c.dtype, np.integer):
        if not (np.issubdtype(c.dtype, np.floating) and np.isfinite(c).all() and (c == np.floor(c)).all()):
            raise ValueError("a contour must hold integer pixel coordinates")
        c = c.astype(np.int64)
    return c


def field_contours(contour, pnt_xy, pnt_Xy, pnt_xY, pnt_XY):
    """The four boundary lines between the corner points (``utils.py:360-397``): (min_line_l, max_line_l, min_line_c,
    max_line_c), lists of (x, y) tuples.  ``ValueError`` when a corner is not a point of the contour."""
    ctr_seq = [tuple(int(v) for v in i) for i in _chain(contour)]
    corners = [tuple(int(v) for v in p) for p in (pnt_xy, pnt_Xy, pnt_xY, pnt_XY)]
    pnt_pos = np.zeros(len(ctr_seq))
    for p in corners:
        pnt_pos[ctr_seq.index(p)] = 1
    pnt_xy, pnt_Xy, pnt_xY, pnt_XY = corners
    min_line_l = field_contour_line(ctr_seq, pnt_pos, pnt_xy, pnt_Xy)
    max_line_l = field_contour_line(ctr_seq, pnt_pos, pnt_xY, pnt_XY)
    min_line_c = field_contour_line(ctr_seq, pnt_pos, pnt_xy, pnt_xY)
    max_line_c = field_contour_line(ctr_seq, pnt_pos, pnt_Xy, pnt_XY)
    return min_line_l, max_line_l, min_line_c, max_line_c


# ------------------------------------------------------------------------------------------------------- the grid solver
def _info(iterations, err, hit):
    return dict(iterations=int(iterations), err=float(err), hit_max_itr=bool(hit))


def _field(a, name, shape=None):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or (shape is not None and a.shape != shape):
        want = "an (H, W) array" if shape is None else f"shape {shape}"
        raise ValueError(f"domain_heat_eqn_solver: `{name}` must have {want}, got {a.shape}")
    return a


def domain_heat_eqn_solver(heat_field, min_line, max_line, edge_line_a, edge_line_b, field_border, field_mask, max_err=1e-20,
                           max_itr=1e6, lh=1, hh=100, device=None, return_info=False):
    """The reference's ``domain_heat_eqn_solver`` (``utils.py:464-524``), same signature and return value, the loop on the
    device: ``min_line`` / ``max_line`` are held at ``lh`` / ``hh``, the two edge lines rise from ``lh`` to ``hh``, every pixel
    with ``field_border != 0`` or on the array's outer rows / columns is fixed, every other pixel of the WHOLE array relaxes
    until ``effective_L2_error`` over ``field_mask`` (a weight) is at most ``max_err`` or ``floor(max_itr) + 1`` sweeps ran.
    Returns ``field * field_mask``; with ``return_info=True`` also ``dict(iterations, err, hit_max_itr)``."""
    heat_field = _field(heat_field, "heat_field")
    H, W = heat_field.shape
    if H < 3 or W < 3:
        raise ValueError(f"domain_heat_eqn_solver: the field must be at least 3 x 3, got {H} x {W}")
    border = _field(field_border, "field_border", (H, W))
    mask = _field(field_mask, "field_mask", (H, W))
    max_err, max_itr = float(max_err), float(max_itr)
    if np.isnan(max_itr):
        raise ValueError("domain_heat_eqn_solver: max_itr is NaN")
    init_field = heat_field.copy()
    add_eh_boundary(init_field, min_line, lh)
    add_eh_boundary(init_field, max_line, hh)
    add_gh_boundary(init_field, edge_line_a, lh, hh)
    add_gh_boundary(init_field, edge_line_b, lh, hh)
    k = _rt._shared_kernels(device, "float64")
    grid_field, sweeps, err, hit = k.heat_grid(init_field, border, mask, max_err, max_itr)
    return (grid_field, _info(sweeps, err, hit)) if return_info else grid_field


# ------------------------------------------------------------------------------------------------------ the graph solver
def _is_sparse(a):
    return hasattr(a, "tocsc") and hasattr(a, "nnz")


DENSE_BLOCK_BYTES = 64 << 20  # rows of a dense adjacency are turned into CSR in blocks of at most this much


def adjacency_csc(adj_mtx, n):
    """``adj_mtx`` (dense (n, n), or any scipy.sparse matrix) -> (indptr int64, indices int32, data float64) of its CSC form:
    per column the rows in ascending order, duplicates summed, explicit zeros dropped (adding 0 changes nothing for a finite
    field).  A sparse matrix stays sparse; a dense one is converted in row blocks."""
    import scipy.sparse as sp

    if _is_sparse(adj_mtx):
        m = adj_mtx.tocsc(copy=True).astype(np.float64)
    else:
        a = np.asarray(adj_mtx)
        if a.ndim != 2:
            raise ValueError(f"digitize_general: adj_mtx must be an (n, n) matrix, got shape {a.shape}")
        rows = max(1, DENSE_BLOCK_BYTES // max(1, a.shape[1] * 8))
        m = sp.vstack([sp.csr_matrix(np.asarray(a[lo : lo + rows], dtype=np.float64)) for lo in range(0, a.shape[0], rows)] or
                      [sp.csr_matrix(a.shape, dtype=np.float64)], format="csr").tocsc()
    if m.shape != (n, n):
        raise ValueError(f"digitize_general: adj_mtx must be ({n}, {n}) for {n} points, got {m.shape}")
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return (np.ascontiguousarray(m.indptr, dtype=np.int64), np.ascontiguousarray(m.indices, dtype=np.int32),
            np.ascontiguousarray(m.data, dtype=np.float64))


def _boundary(idx, n, name):
    idx = np.asarray(idx)
    if idx.size == 0:
        return np.zeros(0, dtype=np.int64)
    if idx.dtype == bool or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"digitize_general: `{name}` must hold integer indices into the point cloud")
    idx = idx.reshape(-1).astype(np.int64)
    if idx.min() < -n or idx.max() >= n:
        raise IndexError(f"digitize_general: `{name}` holds an index outside the {n} points")
    return idx


def digitize_general(pc, adj_mtx, boundary_lower, boundary_upper, max_itr=1e6, lh=1, hh=100, max_err=1e-5, device=None,
                     return_info=False):
    """The reference's ``digitize_general`` (``utils.py:527-575``): the heat of every point of a cloud between a lower boundary
    held at ``lh`` and an upper one held at ``hh`` (index arrays), relaxed over the neighbour network ``adj_mtx`` - dense, or any
    ``scipy.sparse`` matrix, which stays sparse end to end.  One sweep is ``field @ adj_mtx`` followed by the boundary values
    where they are non-zero (a boundary given heat 0 is not held, as in the reference); it stops when
    ``sqrt(sum (new - old)^2 / sum new^2) <= max_err`` (1e-5 hard-wired in the reference) or after ``floor(max_itr) + 1`` sweeps.
    Returns the (n,) float64 field; with ``return_info=True`` also ``dict(iterations, err, hit_max_itr)``."""
    n = len(pc)
    if n < 1:
        raise ValueError("digitize_general: the point cloud is empty")
    if n >= 2**31:
        raise ValueError("digitize_general: at most 2^31 - 1 points")
    max_err, max_itr = float(max_err), float(max_itr)
    if np.isnan(max_itr):
        raise ValueError("digitize_general: max_itr is NaN")
    lower, upper = _boundary(boundary_lower, n, "boundary_lower"), _boundary(boundary_upper, n, "boundary_upper")
    indptr, indices, data = adjacency_csc(adj_mtx, n)
    mask_field = np.zeros(n)
    mask_field[lower] = lh
    mask_field[upper] = hh
    k = _rt._shared_kernels(device, "float64")
    grid_field, sweeps, err, hit = k.heat_graph(indptr, indices, data, mask_field, max_err, max_itr)
    return (grid_field, _info(sweeps, err, hit)) if return_info else grid_field


def neighbor_adjacency(pc, n_neighbors=10):
    """A helper of our own (the reference gives no recipe for ``adj_mtx``): the k-nearest-neighbour graph of the cloud from
    ``scipy.spatial.cKDTree``, symmetrised (i ~ j when either is among the other's ``n_neighbors`` nearest), every column scaled
    to sum 1, as ``scipy.sparse.csc_matrix`` - so that one sweep of ``digitize_general`` replaces the heat of a point by the mean
    over its neighbours.  A point without a neighbour (n = 1) keeps an empty column."""
    import scipy.sparse as sp
    from scipy.spatial import cKDTree

    pc = np.asarray(pc, dtype=np.float64)
    if pc.ndim != 2 or len(pc) == 0:
        raise ValueError(f"neighbor_adjacency: expected an (n, d) array with n >= 1, got shape {pc.shape}")
    n = len(pc)
    k = int(n_neighbors)
    if k < 1:
        raise ValueError("neighbor_adjacency: n_neighbors must be at least 1")
    k = min(k, n - 1)
    if k == 0:
        return sp.csc_matrix((n, n), dtype=np.float64)
    _, nbr = cKDTree(pc).query(pc, k=k + 1)
    rows = np.repeat(np.arange(n), k + 1)
    cols = nbr.reshape(-1)
    keep = rows != cols
    a = sp.csr_matrix((np.ones(int(keep.sum())), (rows[keep], cols[keep])), shape=(n, n))
    a = ((a + a.T) > 0).astype(np.float64).tocsc()
    deg = np.asarray(a.sum(axis=0)).reshape(-1)
    a = (a @ sp.diags(1.0 / np.where(deg > 0, deg, 1.0))).tocsc()
    a.sort_indices()
    return a


# ------------------------------------------------------------------------------------------------------------- digitize
def rasterize_contour(contour, shape):
    """(field_border, field_mask) of a closed pixel chain on an array of ``shape``: the border is the chain's pixels, the mask
    the border plus everything a 4-connected flood fill from outside the array cannot reach, both float64 with ones.

    The chain is what ``cv2.findContours(..., CHAIN_APPROX_NONE)`` returns: (n, 1, 2) or (n, 2) integers (x, y), each point an
    8-neighbour of the next, cyclically.  Any other contour (a compressed chain, a polygon) raises ``NotImplementedError``."""
    from scipy import ndimage

    c = _chain(contour)
    H, W = int(shape[0]), int(shape[1])
    if len(c) > 1:
        step = np.abs(c - np.roll(c, -1, axis=0)).max(axis=1)
        bad = np.nonzero(step != 1)[0]
        if len(bad):
            i = int(bad[0])
            raise NotImplementedError(
                f"digitize: the contour is not a closed pixel chain (point {i} {tuple(c[i])} is no 8-neighbour of the next, "
                f"{tuple(c[(i + 1) % len(c)])}); only what cv2.findContours(..., CHAIN_APPROX_NONE) returns is rasterised here - "
                "pass field_border= / field_mask= for any other contour")
    if c[:, 0].min() < 0 or c[:, 0].max() >= W or c[:, 1].min() < 0 or c[:, 1].max() >= H:
        raise ValueError(f"digitize: the contour leaves the {H} x {W} field (contour points are (x, y) = (column, row))")
    border = np.zeros((H, W), dtype=np.float64)
    border[c[:, 1], c[:, 0]] = 1.0
    free = np.ones((H + 2, W + 2), dtype=bool)      # one ring of outside around the array
    free[1:-1, 1:-1] = border == 0
    labels, _ = ndimage.label(free)                 # 4-connected
    outside = labels == labels[0, 0]
    mask = (~outside[1:-1, 1:-1]).astype(np.float64)
    return border, mask


def digitize(adata, ctrs, ctr_idx, pnt_xy, pnt_Xy, pnt_xY, pnt_XY, spatial_key="spatial", dgl_layer_key="digital_layer",
             dgl_column_key="digital_column", max_itr=1e6, lh=1, hh=100, field_border=None, field_mask=None, device=None):
    """The reference's ``digitize`` (``grid.py:15-106``): the layer and the column heat of every cell inside the contour
    ``ctrs[ctr_idx]``, two solves of the heat equation with the roles of the boundary lines swapped, written to
    ``adata.obs[dgl_layer_key]`` / ``adata.obs[dgl_column_key]`` (a cell reads the field at ``[int(x0), int(x1)]`` of its
    ``obsm[spatial_key]`` row, as in the reference).  The four corners must be points of the contour.

    ``field_border`` / ``field_mask``: the two rasters the reference draws with cv2; without them the contour must be a closed
    pixel chain and is rasterised by ``rasterize_contour`` (the module docstring names the two deviations)."""
    xy = np.asarray(adata.obsm[spatial_key])
    shape = (int(max(xy[:, 0])) + 1, int(max(xy[:, 1])) + 1)
    empty_field = np.zeros(shape)
    contour = ctrs[ctr_idx]
    if field_border is None or field_mask is None:
        border, mask = rasterize_contour(contour, shape)
        field_border = border if field_border is None else field_border
        field_mask = mask if field_mask is None else field_mask
    min_line_l, max_line_l, min_line_c, max_line_c = field_contours(contour, pnt_xy, pnt_Xy, pnt_xY, pnt_XY)
    rows, cols = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)     # int() of the reference: towards zero
    of_layer = domain_heat_eqn_solver(empty_field, min_line_l, max_line_l, min_line_c, max_line_c, field_border, field_mask,
                                      lh=lh, hh=hh, max_itr=max_itr, device=device)
    adata.obs[dgl_layer_key] = of_layer[rows, cols]
    of_column = domain_heat_eqn_solver(empty_field, min_line_c, max_line_c, min_line_l, max_line_l, field_border, field_mask,
                                       lh=lh, hh=hh, max_itr=max_itr, device=device)
    adata.obs[dgl_column_key] = of_column[rows, cols]


def gridit(adata, layer_num, column_num, lh=1, hh=100, dgl_layer_key="digital_layer", dgl_column_key="digital_column",
           layer_border_width=2, column_border_width=2, layer_label_key="layer_label", column_label_key="column_label",
           grid_label_key="grid_label"):
    """The reference's ``gridit`` (``grid.py:110-193``) on ``AnnDataLite`` or anything with the same ``.obs`` item access: cuts
    the heat values into ``layer_num`` / ``column_num`` intervals ``(v_i, v_{i+1}]`` of ``np.linspace(lh, hh, num + 1)`` and writes
    ``obs[layer_label_key]``, ``obs[column_label_key]`` (1-based, 0 outside) and ``obs[grid_label_key]`` ("NA", "Grid Area", or
    "Region Boundary" within half a border width of an interval's lower end)."""
    layer = np.asarray(adata.obs[dgl_layer_key], dtype=np.float64)
    column = np.asarray(adata.obs[dgl_column_key], dtype=np.float64)
    layer_label = np.zeros(len(layer), dtype=np.int64)
    column_label = np.zeros(len(layer), dtype=np.int64)
    grid_label = np.full(len(layer), "NA", dtype=object)
    grid_label[layer != 0] = "Grid Area"
    grid_label[column != 0] = "Grid Area"
    region_mask = grid_label.copy()
    region_mask[region_mask == "Grid Area"] = "Region Boundary"
    value_list = np.linspace(lh, hh, layer_num + 1)
    for i in range(len(value_list) - 1):
        layer_label = np.where((layer > value_list[i]) & (layer <= value_list[i + 1]), i + 1, layer_label)
        grid_label = np.where((layer > (value_list[i] - layer_border_width / 2)) & (layer <= (value_list[i] + layer_border_width / 2)),
                              region_mask, grid_label)
    value_list = np.linspace(lh, hh, column_num + 1)
    for i in range(len(value_list) - 1):
        column_label = np.where((column > value_list[i]) & (column <= value_list[i + 1]), i + 1, column_label)
        grid_label = np.where((column > (value_list[i] - column_border_width / 2)) & (column <= (value_list[i] + column_border_width / 2)),
                              region_mask, grid_label)
    adata.obs[layer_label_key] = layer_label
    adata.obs[column_label_key] = column_label
    adata.obs[grid_label_key] = grid_label
