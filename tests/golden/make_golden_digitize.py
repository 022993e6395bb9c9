"""Writes tests/golden/ref_digitize.npz: what the reference's ``spateo/digitization/utils.py`` and ``grid.py`` give on the cases of
tests/_heat_cases.py (built there from code and seeds: the golden holds reference outputs, and the CSC arrays of the graphs).

The two files are loaded by path inside a stand-in package: ``cv2``, ``skimage`` and ``anndata`` are empty stand-in modules (the
pinned functions never call them), ``..configuration.SKM`` a decorator that does nothing, ``..logging.logger_manager`` a logger
that keeps quiet.  Per case:
  ``grid_<name>_out`` / ``_itr``    the real ``domain_heat_eqn_solver`` and its sweep count (a counting wrapper around
                                  ``effective_L2_error``);
  ``graph_<name>_out`` / ``_itr``   the real ``digitize_general`` on the DENSE adjacency (``np.matmul``) and the count it prints;
  ``graph_<name>_indptr`` / ``_indices`` / ``_data``   the CSC arrays of the adjacency;
  ``dev_<name>``                  the largest deviation between that run and the restatement of _heat_cases.py, relative to the
                                  largest heat: what the order of BLAS's sums is worth;
  ``contours_<chain>_<line>``     ``field_contours`` on the hand-made chains and on the probes of ``contour_probes``;  ``gh_field``  ``add_gh_boundary`` / ``add_eh_boundary``;
  ``gridit_*``                    the real ``gridit`` on a small table (pandas ``obs``);
  ``digitize_layer`` / ``_column``  the real solver on the rasters ``st.dd.rasterize_contour`` makes of the L-shaped chain (the
                                  reference draws them with cv2, which is not here), and ``gridit`` on the cells' heat.

Run from the repository root where the reference checkout is readable (its path as the argument; default
``oracle.ref_stage.REFERENCE_TREE``):  python tests/golden/make_golden_digitize.py [<spateo root>]"""
import contextlib
import importlib.util
import io
import os
import re
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), os.path.join(ROOT, "spateo-release_amd")):
    sys.path.insert(0, p)

import _heat_cases as hc  # noqa: E402


def load_reference(root):
    """(utils, grid) of spateo/digitization, loaded by path as ``refdd.digitization.utils`` / ``.grid``."""
    for name in ("cv2", "skimage", "anndata"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["skimage"].morphology = types.ModuleType("skimage.morphology")
    sys.modules["anndata"].AnnData = type("AnnData", (), {})

    class SKM:
        ADATA_UMI_TYPE = "UMI"

        @staticmethod
        def check_adata_is_type(*a, **kw):
            return lambda fn: fn

    class Quiet:
        def __getattr__(self, name):
            return lambda *a, **kw: None

    pkg = types.ModuleType("refdd")
    pkg.__path__ = []
    sub = types.ModuleType("refdd.digitization")
    sub.__path__ = []
    conf = types.ModuleType("refdd.configuration")
    conf.SKM = SKM
    log = types.ModuleType("refdd.logging")
    log.logger_manager = Quiet()
    sys.modules.update({"refdd": pkg, "refdd.digitization": sub, "refdd.configuration": conf, "refdd.logging": log})
    mods = []
    for name in ("utils", "grid"):
        path = os.path.join(root, "spateo", "digitization", name + ".py")
        spec = importlib.util.spec_from_file_location(f"refdd.digitization.{name}", path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def counted_solver(utils, *args, **kw):
    calls = [0]
    real = utils.effective_L2_error

    def counting(*a):
        calls[0] += 1
        return real(*a)

    utils.effective_L2_error = counting
    try:
        with np.errstate(invalid="ignore", divide="ignore"):
            out = utils.domain_heat_eqn_solver(*args, **kw)
    finally:
        utils.effective_L2_error = real
    return out, calls[0]


class Table:
    """What gridit touches of an AnnData: ``.obs`` as a pandas DataFrame."""

    def __init__(self, **cols):
        import pandas as pd

        self.obs = pd.DataFrame(cols)


def run_gridit(grid, layer, column, **kw):
    import warnings

    t = Table(digital_layer=np.asarray(layer, dtype=np.float64), digital_column=np.asarray(column, dtype=np.float64))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        grid.gridit(t, **kw)
    return (np.asarray(t.obs["layer_label"], dtype=np.int64), np.asarray(t.obs["column_label"], dtype=np.int64),
            np.asarray(t.obs["grid_label"]).astype(str))


def main(root):
    import pandas
    import scipy

    utils, grid = load_reference(root)
    out = {"numpy_version": np.array(np.__version__), "scipy_version": np.array(scipy.__version__),
           "pandas_version": np.array(pandas.__version__)}
    for name in hc.GRID_NAMES:
        c = hc.grid_case(name)
        got, itr = counted_solver(utils, c["heat_field"], c["min_line"], c["max_line"], c["edge_a"], c["edge_b"], c["border"], c["mask"],
                                  max_err=c["max_err"], max_itr=c["max_itr"], lh=c["lh"], hh=c["hh"])
        out[f"grid_{name}_out"], out[f"grid_{name}_itr"] = got, np.int64(itr)
        ref, ritr, errs = hc.grid_reference(name)
        same = np.array_equal(got.view(np.int64), np.asarray(ref).view(np.int64))
        print(f"grid {name}: {got.shape}, {itr} sweeps (restatement {ritr}), last err {errs[-1] if errs else None}, bit-equal {same}")
    for name in hc.GRAPH_NAMES:
        c = hc.graph_case(name)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), np.errstate(invalid="ignore", divide="ignore"):
            got = utils.digitize_general(c["pc"], c["adj"].toarray(), c["lower"], c["upper"], max_itr=c["max_itr"], lh=c["lh"], hh=c["hh"])
        itr = int(re.search(r"Total iteration: (\d+)", buf.getvalue()).group(1))
        ref, ritr, errs = hc.graph_reference(name)
        with np.errstate(invalid="ignore"):
            scale = np.abs(ref).max()
            dev = float(np.abs(got - ref).max() / scale) if scale > 0 else float(np.abs(got - ref).max())
        indptr, indices, data = hc.graph_csc(c)
        out[f"graph_{name}_out"], out[f"graph_{name}_itr"], out[f"dev_{name}"] = got, np.int64(itr), np.float64(dev)
        out[f"graph_{name}_indptr"], out[f"graph_{name}_indices"], out[f"graph_{name}_data"] = indptr, indices, data
        print(f"graph {name}: n {len(got)}, nnz {len(data)}, {itr} sweeps (restatement {ritr}), dev {dev:.3g}, last errs {errs[-2:]}")
    # host functions
    chains = {"rect": (hc.chain_rect(2, 9, 3, 14), dict(pnt_xy=(3, 2), pnt_Xy=(14, 2), pnt_xY=(3, 9), pnt_XY=(14, 9))),
              "rect_shifted": (np.roll(hc.chain_rect(2, 9, 3, 14), 11, axis=0), dict(pnt_xy=(3, 2), pnt_Xy=(14, 2), pnt_xY=(3, 9), pnt_XY=(14, 9))),
              "l": (hc.chain_l(), hc.L_CORNERS)}
    for cname, (chain, corners) in chains.items():
        lines = utils.field_contours(chain, **corners)
        for lname, line in zip(("min_l", "max_l", "min_c", "max_c"), lines):
            out[f"contours_{cname}_{lname}"] = np.array(line, dtype=np.int64)
        print(f"field_contours {cname}: lengths {[len(l) for l in lines]}")
    for i, (chain, corners) in enumerate(hc.contour_probes()):
        lines = utils.field_contours(chain, *corners)
        for lname, line in zip(("min_l", "max_l", "min_c", "max_c"), lines):
            out[f"contours_probe{i}_{lname}"] = np.array(line, dtype=np.int64).reshape(-1, 2)
    print(f"field_contours: {len(hc.contour_probes())} probes")
    f = np.zeros((6, 9))
    utils.add_eh_boundary(f, [(1, 1), (2, 1), (3, 1)], 7.0)
    utils.add_gh_boundary(f, [(1, 2), (1, 3), (2, 4), (3, 4), (4, 4), (5, 5), (6, 5)], 1.0, 100.0)
    out["gh_field"] = f
    a, b, m = np.arange(12.0).reshape(3, 4), np.arange(12.0).reshape(3, 4)[::-1] * 0.5 + 1, np.array([[1.0, 2, 0, 1]] * 3)
    out["l2_error"] = np.float64(utils.effective_L2_error(a, b, m))
    rng = np.random.default_rng(5)
    layer, column = rng.random(60) * 120 - 10, rng.random(60) * 120 - 10
    layer[:5], column[:5] = 0.0, 0.0
    layer[5:8], column[8:10] = (1.0, 100.0, 34.0), (0.0, 50.5)
    out["gridit_layer"], out["gridit_column"] = layer, column
    out["gridit_layer_label"], out["gridit_column_label"], out["gridit_grid_label"] = run_gridit(grid, layer, column, layer_num=3,
                                                                                                   column_num=4)
    l2, c2, g2 = run_gridit(grid, layer, column, layer_num=5, column_num=2, lh=0, hh=110, layer_border_width=6, column_border_width=1)
    out["gridit2_layer_label"], out["gridit2_column_label"], out["gridit2_grid_label"] = l2, c2, g2
    # digitize: the real solver on our rasters of the L-shaped chain, the cells' heat, gridit on top
    from spateo_amd import dd

    xy = hc.l_slice_cells()
    shape = (int(max(xy[:, 0])) + 1, int(max(xy[:, 1])) + 1)
    assert shape == (40, 70), shape
    border, mask = dd.rasterize_contour(hc.chain_l(), shape)
    min_l, max_l, min_c, max_c = utils.field_contours(hc.chain_l(), **hc.L_CORNERS)
    of_layer, n1 = counted_solver(utils, np.zeros(shape), min_l, max_l, min_c, max_c, border, mask)
    of_column, n2 = counted_solver(utils, np.zeros(shape), min_c, max_c, min_l, max_l, border, mask)
    rows, cols = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
    out["digitize_layer_field"], out["digitize_column_field"] = of_layer, of_column
    out["digitize_layer"], out["digitize_column"] = of_layer[rows, cols], of_column[rows, cols]
    out["digitize_sweeps"] = np.array([n1, n2], dtype=np.int64)
    out["digitize_layer_label"], out["digitize_column_label"], out["digitize_grid_label"] = run_gridit(
        grid, out["digitize_layer"], out["digitize_column"], layer_num=4, column_num=5)
    print(f"digitize: {n1} + {n2} sweeps, {int((out['digitize_layer'] != 0).sum())} of {len(xy)} cells inside")
    path = os.path.join(HERE, "ref_digitize.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:
        sys.path.insert(0, ROOT)
        from oracle import ref_stage

        main(ref_stage.REFERENCE_TREE)
