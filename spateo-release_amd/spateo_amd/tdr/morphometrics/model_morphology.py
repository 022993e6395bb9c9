"""``model_morphology`` of ``spateo.tdr.morphometrics.morphology`` (``morphology.py:11-71``): length, width, height, surface
area, volume, their ratio and the cell density of a reconstructed surface model.

The reference reads pyvista's ``.bounds``, ``.area`` and ``.volume``.  Here the model is a triangle surface as
``Mesh_correction`` takes one and the numbers are O(triangles) sums in float64 NumPy on the host - no kernel is needed: the
bounds from the points, the area as the sum of the triangle areas, the volume as ``|sum det[a, b, c]| / 6`` (the divergence
theorem; what vtkMassProperties computes for a closed surface).  pyvista is not a dependency and is never imported, so area and
volume are not pinned against it; the tests use closed meshes with closed forms.  ``extract_surface`` of a volume mesh is not
here: triangle surfaces only.
"""
from __future__ import annotations

import numpy as np

from ..._mesh_correction import _as_mesh
from ...logging import logger_manager as lm

__all__ = ["model_morphology"]


def _n_points(pc):
    if hasattr(pc, "n_points"):
        return int(pc.n_points)
    if hasattr(pc, "points"):
        return len(pc.points)
    return len(pc)


def _is_closed(triangles):
    """Every edge (as ``mesh_edges`` lists them: unordered vertex pairs) is shared by exactly two triangles."""
    t = np.asarray(triangles, dtype=np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return bool((counts == 2).all())


def model_morphology(model, pc=None):
    """The basic morphological characteristics of a surface model: a dict with ``Length(x)``, ``Width(y)``, ``Height(z)``,
    ``Surface_area``, ``Volume``, ``V/SA_ratio`` and, with ``pc``, ``cell_density`` (the number of points of ``pc`` over the
    volume), each rounded to 5 decimals as in the reference.

    model: ``(points, triangles)`` or an object with ``.points`` and a pyvista-style flat ``.faces``; cells that are not
    triangles are refused by name.  pc: anything with ``.n_points``, ``.points`` or a length.  A surface with an edge that is not
    shared by exactly two triangles is not closed and its volume is not meaningful: that is logged as a warning and the number
    is returned all the same (vtk does not refuse it either)."""
    mesh = _as_mesh(model, "model_morphology")
    points, tri = mesh.points, np.asarray(mesh.triangles, dtype=np.int64)
    morphology = {}

    lengths = np.abs(points.max(axis=0) - points.min(axis=0))
    morphology["Length(x)"], morphology["Width(y)"], morphology["Height(z)"] = (round(float(v), 5) for v in lengths)
    lm.main_info(f"Length (x) of model: {morphology['Length(x)']};", indent_level=1)
    lm.main_info(f"Width (y) of model: {morphology['Width(y)']};", indent_level=1)
    lm.main_info(f"Height (z) of model: {morphology['Height(z)']};", indent_level=1)

    a, b, c = points[tri[:, 0]], points[tri[:, 1]], points[tri[:, 2]]
    model_sa = round(float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()), 5)
    morphology["Surface_area"] = model_sa
    lm.main_info(f"Surface area of model: {morphology['Surface_area']};", indent_level=1)

    if not _is_closed(tri):
        lm.main_warning("The surface is not closed (an edge is not shared by exactly two triangles): the volume of an open "
                        "surface is not meaningful.", indent_level=1)
    model_v = round(float(abs(np.einsum("ij,ij->i", a, np.cross(b, c)).sum()) / 6.0), 5)
    morphology["Volume"] = model_v
    lm.main_info(f"Volume of model: {morphology['Volume']};", indent_level=1)

    model_vsa = round(model_v / model_sa, 5)
    morphology["V/SA_ratio"] = model_vsa
    lm.main_info(f"Volume / surface area ratio of model: {morphology['V/SA_ratio']}.", indent_level=1)

    if pc is not None:
        morphology["cell_density"] = round(_n_points(pc) / model_v, 5)
        lm.main_info(f"Cell density of model: {morphology['cell_density']}.", indent_level=1)
    return morphology
