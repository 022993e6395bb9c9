#!/usr/bin/env python
"""Golden vectors for the mesh correction: the REAL ``spateo/alignment/methods/mesh_correction_utils.py`` is executed, loaded by
file path from the reference checkout with ``shapely.geometry``, ``cv2`` and ``..utils._iteration`` - none of which the pinned
functions touch - stubbed in ``sys.modules``.  Recorded: ``ICP`` (both ``allow_rotation`` values), ``_generate_labeling``
(linear and log, odd and even counts), ``_make_pairs``, ``_get_parameters_from_pair``, ``_smooth_contours``,
``_transform_points`` at translation 0, and ``_calculate_loss`` / ``_get_binary_values`` on a small closed triangulated surface.

Two stand-ins, both stated here because they decide what the last two goldens pin:

  * the mesh handed to ``_calculate_loss`` is a duck-typed object whose ``.contour(isosurfaces=, scalars=)`` is THIS SCRIPT'S OWN
    float64 cut (pyvista / VTK are not installed): one point per unique edge whose ends classify differently under
    ``s >= z`` - VTK's contour rule -, the linear interpolate in x and y, z set to the height itself, in edge-index order.  The
    reference's own line ``points[points[:, 2] == z, :2]`` then picks the slices apart.  What is pinned is everything the
    reference does AROUND the cut: the copy, the transform, the selection by height, one real ``ICP`` per slice, the 1e6 branch,
    the division, the float32 cast and the (L, L) layout of ``_get_binary_values``.
  * for the cases with translation != 0, ``_transform_points`` is replaced by its z-translation restatement (the reference's
    line adds the translation to the first two ROWS; at translation 0 the real function runs and is recorded as such).

ICP inputs are noisy closed curves in general position, never lattices, of at most 500 points, so the reference draws nothing.
Condition, asserted below for every ICP case: under 8 random +-4 ulp perturbations of its inputs the real ``ICP`` returns the
same ``gamma`` and a ``T_contour_2`` within 1e-9 of the contour scale; a case that fails must be replaced, never skipped.

    python tests/golden/make_golden_mesh_correction.py      -> tests/golden/ref_mesh_correction.npz
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402

import _icp_cases as ic  # noqa: E402  (the shared input generators; no reference code)

# (tag, n1, n2, seed, angle, shift, reflect): sizes 2 .. 500, N != M both ways
ICP_CASES = [("a", 120, 90, 3, 3.0, (1.5, -1.0), False), ("b", 500, 500, 11, 2.0, (0.8, 0.6), False),
             ("c", 40, 63, 21, -4.0, (-1.0, 0.5), False), ("d", 65, 64, 33, 5.0, (0.3, 0.3), False),
             ("e", 7, 2, 41, 1.0, (0.1, 0.0), False), ("f", 300, 77, 57, 6.0, (2.0, -2.0), False),
             ("g", 200, 180, 63, 2.0, (0.5, 0.2), True), ("h", 30, 30, 71, 0.0, (0.0, 0.0), False)]  # h: zigzag_pair, a reflection


def load_utils():
    mg._pkg("shapely")
    geo = types.ModuleType("shapely.geometry")
    geo.MultiPolygon = geo.Polygon = type("Polygon", (), {})
    sys.modules["shapely.geometry"] = geo
    sys.modules["cv2"] = types.ModuleType("cv2")
    for name in ("spateo", "spateo.alignment", "spateo.alignment.methods"):
        if name not in sys.modules:
            mg._pkg(name)
    utils = types.ModuleType("spateo.alignment.utils")
    utils._iteration = lambda n, **kw: range(n)
    sys.modules["spateo.alignment.utils"] = utils
    return mg._load("spateo.alignment.methods.mesh_correction_utils", "spateo/alignment/methods/mesh_correction_utils.py")


class CutMesh:
    """The duck-typed mesh of the header: ``.points``, ``.copy()`` and this script's own ``.contour``."""

    def __init__(self, points, edges):
        self.points, self.edges = np.array(points, dtype=np.float64), edges

    def copy(self):
        return CutMesh(self.points, self.edges)

    def contour(self, isosurfaces, scalars):
        out = []
        for z in isosurfaces:
            c = ic.cut(np.column_stack([self.points[:, :2], scalars]), self.edges, float(z))
            out.append(np.column_stack([c, np.full(len(c), z)]))
        return types.SimpleNamespace(points=np.concatenate(out, axis=0))


def main():
    mu = load_utils()
    out = {}
    rng = np.random.default_rng(20261020)
    # ---- ICP
    out["icp_tags"] = np.array([c[0] for c in ICP_CASES])
    for tag, n1, n2, seed, angle, shift, reflect in ICP_CASES:
        c1, c2 = ic.zigzag_pair(n1, seed) if tag == "h" else ic.icp_pair(n1, n2, seed, angle, shift, reflect)
        out[f"icp_{tag}_c1"], out[f"icp_{tag}_c2"] = c1, c2
        scale = float(np.ptp(c1, axis=0).max())
        for rot in (False, True):
            gamma, _, t, k1, T, R = mu.ICP(c1.copy(), c2.copy(), allow_rotation=rot)
            assert k1.shape == c1.shape
            for _ in range(8):
                g4, _, _, _, T4, _ = mu.ICP(ic.jitter(rng, c1), ic.jitter(rng, c2), allow_rotation=rot)
                assert g4 == gamma and np.abs(T4 - T).max() <= 1e-9 * scale, (tag, rot, "replace this case")
            r = int(rot)
            out[f"icp_{tag}_{r}_gamma"], out[f"icp_{tag}_{r}_T"] = np.float64(gamma), T
            out[f"icp_{tag}_{r}_t"], out[f"icp_{tag}_{r}_R"] = np.asarray(t, dtype=np.float64) * np.ones(2), np.asarray(R, dtype=np.float64)
    # ---- the label grid, the pairs, the parameter sets, the smoothing
    grids = [(180.0, 15, "linear"), (180.0, 6, "linear"), (12.5, 5, "linear"), (1.5, 15, "log"), (1.5, 4, "log"), (1.1, 3, "log")]
    out["grid_args"] = np.array([(m, n, t == "log") for m, n, t in grids], dtype=np.float64)
    for i, (m, n, t) in enumerate(grids):
        out[f"grid_{i}"] = np.array(mu._generate_labeling(m, n, t), dtype=np.float64)
    out["pairs"] = mu._make_pairs()
    labels = np.array([mu._generate_labeling(30.0, 5), mu._generate_labeling(30.0, 5), mu._generate_labeling(30.0, 5),
                       mu._generate_labeling(4.0, 5), mu._generate_labeling(1.5, 5, "log")], dtype=np.float64).T
    labels = mu._update_parameter(labels, {"rotation": np.array([2.0, -1.0, 0.5]), "translation": 0.75, "scaling": 1.05})
    out["labels"] = labels
    for p in ((0, 1), (1, 4), (3, 4)):
        out[f"sets_{p[0]}{p[1]}"] = mu._get_parameters_from_pair(np.array(p), labels)
    raw = [ic.closed_curve(57, 5), ic.closed_curve(12, 6), ic.closed_curve(200, 7)]
    out["smooth_in"] = np.concatenate(raw)
    out["smooth_sizes"] = np.array([len(c) for c in raw])
    out["smooth_w5"] = np.concatenate(mu._smooth_contours([c.copy() for c in raw], 5))
    out["smooth_w3_it2"] = np.concatenate(mu._smooth_contours([c.copy() for c in raw], 3, 2))
    # ---- the transform at translation 0, the loss and the binary table
    verts, tri = ic.ellipsoid()
    edges = ic.unique_edges(tri)
    out["mesh_points"], out["mesh_triangles"] = verts, tri
    tf = np.array([[0.0, 0.0, 0.0, 0.0, 1.0], [12.0, -7.0, 31.0, 0.0, 1.1], [-170.0, 95.0, 3.0, 0.0, 0.8]])
    out["tf_params"] = tf
    out["tf_points"] = np.stack([mu._transform_points(verts.copy(), p[:3], p[3], p[4]) for p in tf])
    heights = np.array([30.0, 36.0, 44.0, 50.0])
    truth = np.array([4.0, -3.0, 10.0, 1.0, 1.05])
    contours = ic.slices_of(verts, tri, truth, heights, noise=0.05)
    out["loss_heights"], out["loss_truth"] = heights, truth
    out["loss_contours"] = np.concatenate(contours)
    out["loss_sizes"] = np.array([len(c) for c in contours])
    real_tp = mu._transform_points
    mu._transform_points = lambda pts, rot, tr, sc: ic.transform(pts, np.mean(pts, axis=0), [rot[0], rot[1], rot[2], tr, sc])
    mesh = CutMesh(verts, edges)
    cases = np.array([[0.0, 0.0, 0.0, 0.0, 1.0], truth, [4.0, -3.0, 10.0, 0.0, 1.05], [0.0, 0.0, 0.0, 40.0, 1.0],
                      [8.0, 2.0, -5.0, -2.0, 0.95]])
    out["loss_params"] = cases
    out["loss_values"] = np.array([mu._calculate_loss(contours, mesh, p, heights, "ICP") for p in cases], dtype=np.float64)
    assert out["loss_values"][3] == 1e6 / len(heights) and out["loss_values"][1] < out["loss_values"][0]
    lab3 = np.array([[0.0, 0.0, 0.0, 0.0, 1.0], [-6.0, -6.0, -6.0, -1.5, 1 / 1.1], [6.0, 6.0, 6.0, 1.5, 1.1]])
    lab3 = mu._update_parameter(lab3, {"rotation": truth[:3] * 0.5, "translation": 0.5, "scaling": 1.0})
    out["bin_labels"] = lab3
    for p in ((0, 3), (2, 4)):
        b = mu._get_binary_values(contours, mesh, heights, np.array(p), lab3)
        assert b.dtype == np.float32 and b.shape == (3, 3)
        out[f"bin_{p[0]}{p[1]}"] = b
    mu._transform_points = real_tp
    path = os.path.join(HERE, "ref_mesh_correction.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
