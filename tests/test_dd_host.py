"""Host-side tests of ``spateo_amd.dd`` and the ``mvf_heat_*`` C ABI, without a device: the rasterisation of pixel chains and its
named refusal, argument validation before the kernels are bound, the exports, the refusals of the entry points with nothing
launched, and ``digitize`` / ``digitize_general`` end to end over a NumPy stand-in for the kernels (the restatements of
tests/_heat_cases.py behind ``HipKernels.heat_grid`` / ``heat_graph``), which checks what the host adds: boundary lines, the two
solves with swapped roles, the cells' lookup, the CSC conversion."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import _heat_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mvf.h")


class HeatCpuKernels:
    """``HipKernels.heat_grid`` / ``heat_graph`` on the CPU."""

    def __init__(self, device=None, dtype="float64"):
        self.device, self.dtype_name, self.calls = device, dtype, []

    def heat_grid(self, init, border, mask, max_err, max_itr, block_steps=0):
        self.calls.append(("grid", np.array(init), np.array(border), np.array(mask), max_err, max_itr))
        f, itr, errs = hc.grid_loop_arrays(np.asarray(init, dtype=np.float64), np.asarray(border), np.asarray(mask), max_err, max_itr)
        err = errs[-1] if errs else 1.0
        return f * mask, itr, err, bool(err > max_err)

    def heat_graph(self, indptr, indices, data, fixed_value, max_err, max_itr):
        self.calls.append(("graph", np.array(indptr), np.array(indices), np.array(data), np.array(fixed_value), max_err, max_itr))
        f, itr, errs = hc.graph_loop_arrays(indptr, indices, data, np.asarray(fixed_value, dtype=np.float64), max_err, max_itr)
        err = errs[-1] if errs else 1.0
        return f, itr, err, bool(err > max_err)


@pytest.fixture
def seam(monkeypatch):
    from spateo_amd import _runtime as rt

    made = []
    monkeypatch.setattr(rt, "_make_kernels", lambda device, dtype: made.append(HeatCpuKernels(device, dtype)) or made[-1])
    monkeypatch.setattr(rt, "_shared_kernels", lambda device, dtype: rt._make_kernels(device, dtype))
    return made


@pytest.fixture
def no_kernels(monkeypatch):
    from spateo_amd import _runtime as rt

    def refuse(device, dtype):
        raise AssertionError("the kernels were bound before the arguments were refused")

    monkeypatch.setattr(rt, "_make_kernels", refuse)
    monkeypatch.setattr(rt, "_shared_kernels", refuse)


@pytest.fixture(scope="module")
def G():
    return hc.load()


# -------------------------------------------------------------------------------------------------------------- exports
def test_exports():
    import spateo_amd as st
    from spateo_amd import dd

    assert st.dd is dd and "dd" in st.__all__
    assert set(dd.__all__) == {"domain_heat_eqn_solver", "digitize_general", "digitize", "gridit", "neighbor_adjacency",
                               "add_eh_boundary", "add_gh_boundary", "effective_L2_error", "field_contour_line", "field_contours",
                               "rasterize_contour"}
    for name in dd.__all__:
        assert callable(getattr(dd, name))
    for absent in ("get_borderline", "grid_borderline", "order_borderline", "extend_layer", "fill_grid_label", "draw_seg_grid"):
        assert not hasattr(dd, absent)          # the borderline route is not here, and there are no stubs for it
    assert "cv2" not in sys.modules


def test_library_exports_the_four_symbols():
    from spateo_amd import _lib

    lib = _lib.load()
    names = {"mvf_heat_grid", "mvf_heat_grid_workspace_bytes", "mvf_heat_graph", "mvf_heat_graph_workspace_bytes"}
    assert names <= set(_lib.SIGNATURES)
    for name in names:
        assert hasattr(lib, name)
    assert lib.mvf_version() == 7
    text = open(HEADER).read()
    assert int(re.search(r"#define MVF_HEAT_MAX_STEPS (\d+)", text).group(1)) == _lib.HEAT_MAX_STEPS == hc.T
    assert "utils.py:508-522" in text and "utils.py:553-575" in text
    src = open(os.path.join(ROOT, "spateo-release_amd", "csrc", "mvf_heat.hip")).read()
    assert f"HEAT_TX = {hc.TILE_W}, HEAT_TY = {hc.TILE_H}" in src
    for word in ("cooperative_groups", "grid.sync", "hipLaunchCooperativeKernel", "atomicAdd", "atomicCAS", "atomicExch", "volatile",
                 "__threadfence"):
        assert word not in src, word          # no grid-wide barrier, nothing that spins on another workgroup, no atomics


# ------------------------------------------------------------------------------------------- C ABI without a launch
def test_grid_entry_refuses_without_launching():
    from spateo_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(256)     # never dereferenced: every call below returns before a launch
    sweeps, err, hit = ctypes.c_int64(-7), ctypes.c_double(-7.0), ctypes.c_int(-7)

    def call(init=p, border=p, mask=p, H=20, W=30, max_err=1e-20, max_itr=1e6, block=0, out=p, sw=ctypes.byref(sweeps),
             er=ctypes.byref(err), hi=ctypes.byref(hit), ws=p, ws_bytes=1 << 30):
        return lib.mvf_heat_grid(init, border, mask, H, W, max_err, max_itr, block, out, sw, er, hi, ws, ws_bytes, None)

    need = lib.mvf_heat_grid_workspace_bytes(20, 30)
    assert need == 256 + (2 * 600 + 2 * hc.T * 1) * 8 + 600
    assert lib.mvf_heat_grid_workspace_bytes(33, 65) == 256 + (2 * 33 * 65 + 2 * hc.T * 4) * 8 + 2152     # 2145 bytes, 8-aligned
    for H, W in ((2, 30), (20, 2), (0, 0), (-1, 5), (1 << 20, 30)):
        assert lib.mvf_heat_grid_workspace_bytes(H, W) == 0
    for kw, msg in ((dict(H=2), b"bad shape"), (dict(W=2), b"bad shape"), (dict(H=-3), b"bad shape"), (dict(W=1 << 20), b"bad shape"),
                    (dict(block=-1), b"bad block_steps"), (dict(block=hc.T + 1), b"bad block_steps"), (dict(init=None), b"null pointer"),
                    (dict(border=None), b"null pointer"), (dict(mask=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(sw=None), b"null pointer"), (dict(er=None), b"null pointer"), (dict(hi=None), b"null pointer"),
                    (dict(ws=None), b"null pointer"), (dict(ws=ctypes.c_void_p(264)), b"256-byte aligned"),
                    (dict(ws_bytes=need - 1), b"workspace too small")):
        assert call(**kw) != 0, kw
        assert b"mvf_heat_grid" in lib.mvf_last_error() and msg in lib.mvf_last_error(), (kw, lib.mvf_last_error())
    assert (sweeps.value, err.value, hit.value) == (-7, -7.0, -7)
    with pytest.raises(_lib.MVFError, match="bad shape"):
        _lib.check(call(H=1), "mvf_heat_grid")


def test_graph_entry_refuses_without_launching():
    from spateo_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(256)
    sweeps, err, hit = ctypes.c_int64(-7), ctypes.c_double(-7.0), ctypes.c_int(-7)
    good = dict(indptr=np.array([0, 1, 3, 4], dtype=np.int64), indices=np.array([1, 0, 2, 1], dtype=np.int32),
                values=np.array([1.0, 0.5, 0.5, 1.0]), fixed=np.array([1.0, 0.0, 100.0]))

    def call(n=3, out=p, sw=ctypes.byref(sweeps), ws=p, ws_bytes=1 << 30, **arrays):
        a = dict(good, **arrays)
        ptr = lambda v: None if v is None else v.ctypes.data  # noqa: E731
        return lib.mvf_heat_graph(ptr(a["indptr"]), ptr(a["indices"]), ptr(a["values"]), ptr(a["fixed"]), n, 1e-5, 1e6, out, sw,
                                  ctypes.byref(err), ctypes.byref(hit), ws, ws_bytes, None)

    need = lib.mvf_heat_graph_workspace_bytes(3, 4)
    assert need == 256 + (3 * 3 + 2 * 1 + 4 + 4) * 8 + 16
    for n, nnz in ((0, 0), (-1, 3), (1 << 31, 1), (5, -1)):
        assert lib.mvf_heat_graph_workspace_bytes(n, nnz) == 0
    i64, i32 = np.int64, np.int32
    for kw, msg in ((dict(n=0), b"bad shape"), (dict(n=-2), b"bad shape"), (dict(indptr=None), b"null pointer"),
                    (dict(fixed=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(sw=None), b"null pointer"),
                    (dict(indices=None), b"null pointer"), (dict(values=None), b"null pointer"),
                    (dict(indptr=np.array([1, 1, 3, 4], dtype=i64)), b"bad indptr"),
                    (dict(indptr=np.array([0, 3, 1, 4], dtype=i64)), b"bad indptr"),
                    (dict(indptr=np.array([0, 1, 3, -1], dtype=i64)), b"bad indptr"),
                    (dict(indices=np.array([1, 0, 3, 1], dtype=i32)), b"index out of range"),
                    (dict(indices=np.array([1, -1, 2, 1], dtype=i32)), b"index out of range"),
                    (dict(ws=None), b"null pointer"), (dict(ws=ctypes.c_void_p(8)), b"256-byte aligned"),
                    (dict(ws_bytes=need - 1), b"workspace too small")):
        assert call(**kw) != 0, kw
        assert b"mvf_heat_graph" in lib.mvf_last_error() and msg in lib.mvf_last_error(), (kw, lib.mvf_last_error())
    assert (sweeps.value, err.value, hit.value) == (-7, -7.0, -7)


# -------------------------------------------------------------------------------------------------------- rasterisation
def test_rasterisation_of_chains():
    from spateo_amd import dd

    border, mask = dd.rasterize_contour(hc.chain_rect(2, 9, 3, 14), (12, 18))
    want_b, want_m = np.zeros((12, 18)), np.zeros((12, 18))
    want_b[2, 3:15] = want_b[9, 3:15] = want_b[2:10, 3] = want_b[2:10, 14] = 1
    want_m[2:10, 3:15] = 1
    assert np.array_equal(border, want_b) and np.array_equal(mask, want_m) and border.dtype == mask.dtype == np.float64
    # diagonal steps: the 8-connected chain still keeps the 4-connected flood out
    border, mask = dd.rasterize_contour(hc.chain_l(), (40, 70))
    assert border.sum() == len(hc.chain_l()) and (mask[border == 1] == 1).all()
    assert mask[20, 10] == 1 and mask[30, 50] == 1 and mask[10, 50] == 0 and mask[0, 0] == 0 and mask[39, 69] == 0
    assert mask[4, 6] == 1 and mask[3, 5] == 0          # beside the cut corner (5, 4) - (6, 3)
    inside = int(mask.sum() - border.sum())
    assert inside == sum(1 for y in range(40) for x in range(70)
                         if ((4 <= y <= 34 and 6 <= x <= 29) or (20 <= y <= 34 and 6 <= x <= 59) or (x, y) == (30, 19)))
    assert mask[19, 30] == 1 and border[19, 30] == 0      # the diagonal step (31, 19) - (30, 18) leaves this pixel inside
    # (n, 2) input, a chain that touches the array's edge, a single pixel, a two-pixel chain
    b2, m2 = dd.rasterize_contour(hc.chain_rect(0, 5, 0, 7)[:, 0], (6, 8))
    assert m2.all() and b2.sum() == 2 * 8 + 2 * 4
    b3, m3 = dd.rasterize_contour(np.array([[[4, 2]]]), (5, 6))
    assert b3.sum() == 1 and b3[2, 4] == 1 and np.array_equal(b3, m3)
    b4, m4 = dd.rasterize_contour(np.array([[1, 1], [2, 2]]), (4, 4))
    assert b4.sum() == 2 and np.array_equal(b4, m4)


def test_other_contours_are_refused_by_name():
    from spateo_amd import dd

    gap = np.delete(hc.chain_rect(2, 9, 3, 14), 5, axis=0)
    with pytest.raises(NotImplementedError, match=r"field_border= / field_mask="):
        dd.rasterize_contour(gap, (12, 18))
    polygon = np.array([[[3, 2]], [[3, 9]], [[14, 9]], [[14, 2]]])          # CHAIN_APPROX_SIMPLE: the corners alone
    with pytest.raises(NotImplementedError, match="closed pixel chain"):
        dd.rasterize_contour(polygon, (12, 18))
    with pytest.raises(NotImplementedError, match="8-neighbour"):
        dd.rasterize_contour(np.array([[1, 1], [1, 1], [2, 2]]), (4, 4))     # a repeated point
    with pytest.raises(ValueError, match="leaves"):
        dd.rasterize_contour(hc.chain_rect(2, 9, 3, 14), (9, 18))
    with pytest.raises(ValueError, match="integer"):
        dd.rasterize_contour(np.array([[1.5, 1.0], [2.0, 2.0]]), (4, 4))
    with pytest.raises(ValueError, match="shape"):
        dd.rasterize_contour(np.zeros((0, 1, 2), dtype=int), (4, 4))
    with pytest.raises(ValueError, match="shape"):
        dd.rasterize_contour(np.zeros((4, 3), dtype=int), (4, 4))


# ----------------------------------------------------------------------------------------------------------- validation
def test_refusals_come_before_the_kernels(no_kernels):
    import scipy.sparse as sp

    from spateo_amd import AnnDataLite, dd

    c = hc.grid_case("rect_12x15")
    args = (c["heat_field"], c["min_line"], c["max_line"], c["edge_a"], c["edge_b"], c["border"], c["mask"])
    with pytest.raises(ValueError, match="at least 3 x 3"):
        dd.domain_heat_eqn_solver(np.zeros((2, 9)), [], [], [], [], np.zeros((2, 9)), np.zeros((2, 9)))
    with pytest.raises(ValueError, match="field_border"):
        dd.domain_heat_eqn_solver(*args[:5], np.zeros((12, 14)), c["mask"])
    with pytest.raises(ValueError, match="field_mask"):
        dd.domain_heat_eqn_solver(*args[:6], np.zeros((11, 15)))
    with pytest.raises(ValueError, match="heat_field"):
        dd.domain_heat_eqn_solver(np.zeros(15), *args[1:])
    with pytest.raises(ValueError, match="max_itr"):
        dd.domain_heat_eqn_solver(*args, max_itr=float("nan"))
    with pytest.raises(IndexError):
        dd.domain_heat_eqn_solver(*args[:1], [(99, 0)], *args[2:])
    pc, adj = np.zeros((5, 3)), sp.identity(5, format="csr")
    with pytest.raises(ValueError, match="empty"):
        dd.digitize_general(np.zeros((0, 3)), sp.identity(0), [], [])
    with pytest.raises(ValueError, match=r"\(5, 5\)"):
        dd.digitize_general(pc, sp.identity(4), [0], [1])
    with pytest.raises(ValueError, match=r"\(5, 5\)"):
        dd.digitize_general(pc, np.zeros((5, 4)), [0], [1])
    with pytest.raises(ValueError, match="adj_mtx"):
        dd.digitize_general(pc, np.zeros(5), [0], [1])
    with pytest.raises(IndexError, match="boundary_upper"):
        dd.digitize_general(pc, adj, [0], [5])
    with pytest.raises(ValueError, match="boundary_lower"):
        dd.digitize_general(pc, adj, [0.5], [1])
    with pytest.raises(ValueError, match="max_itr"):
        dd.digitize_general(pc, adj, [0], [1], max_itr=float("nan"))
    adata = AnnDataLite(obsm={"spatial": hc.l_slice_cells()})
    gap = np.delete(hc.chain_l(), 7, axis=0)
    with pytest.raises(NotImplementedError, match=r"field_border= / field_mask="):
        dd.digitize(adata, (gap,), 0, **hc.L_CORNERS)
    with pytest.raises(ValueError):
        dd.digitize(adata, (hc.chain_l(),), 0, **dict(hc.L_CORNERS, pnt_XY=(0, 0)))
    with pytest.raises(ValueError, match="n_neighbors"):
        dd.neighbor_adjacency(np.zeros((4, 3)), 0)
    with pytest.raises(ValueError, match="neighbor_adjacency"):
        dd.neighbor_adjacency(np.zeros((0, 3)))


def test_neighbor_adjacency():
    import scipy.sparse as sp

    from spateo_amd import dd

    pc = np.random.default_rng(0).random((257, 3))
    a = dd.neighbor_adjacency(pc, 6)
    assert sp.isspmatrix_csc(a) and a.shape == (257, 257) and a.has_sorted_indices
    assert np.allclose(np.asarray(a.sum(axis=0)).ravel(), 1.0, rtol=0, atol=1e-15) and a.diagonal().sum() == 0
    pattern = (a != 0).astype(int)
    assert (pattern != pattern.T).nnz == 0 and np.diff(a.indptr).min() >= 6
    d2 = ((pc[:, None] - pc[None]) ** 2).sum(-1)
    nearest = np.argsort(d2[0])[1:7]
    assert set(nearest) <= set(a[:, 0].nonzero()[0])
    for j in range(0, 257, 50):                 # a column holds 1 / degree at the node's neighbours
        col = a[:, j].toarray().ravel()
        assert set(np.unique(col[col != 0])) == {1.0 / (col != 0).sum()}
    assert dd.neighbor_adjacency(np.zeros((1, 3)), 10).nnz == 0
    assert dd.neighbor_adjacency(pc[:4], 10).nnz == 12          # k is cut to n - 1


# ------------------------------------------------------------------------------------------------ what the host adds
def test_domain_solver_over_the_stand_in(seam, G):
    from spateo_amd import dd

    for name in ("rect_12x15", "mask_2_and_3", "budget_5", "all_zero", "no_sweep", "stop_1e-3"):
        c = hc.grid_case(name)
        heat = c["heat_field"].copy()
        out, info = dd.domain_heat_eqn_solver(heat, c["min_line"], c["max_line"], c["edge_a"], c["edge_b"], c["border"], c["mask"],
                                              max_err=c["max_err"], max_itr=c["max_itr"], lh=c["lh"], hh=c["hh"], return_info=True)
        assert np.array_equal(out.view(np.int64), G[f"grid_{name}_out"].view(np.int64)), name
        assert info["iterations"] == int(G[f"grid_{name}_itr"]) and set(info) == {"iterations", "err", "hit_max_itr"}
        assert info["hit_max_itr"] == (name in ("budget_5", "no_sweep"))
        assert np.array_equal(heat, c["heat_field"])            # the caller's field is not written
        assert np.array_equal(seam[-1].calls[-1][1], hc.grid_init(c))
    plain = dd.domain_heat_eqn_solver(c["heat_field"], c["min_line"], c["max_line"], c["edge_a"], c["edge_b"], c["border"], c["mask"],
                                      max_err=c["max_err"])
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, out)


def test_digitize_general_over_the_stand_in(seam, G):
    import scipy.sparse as sp

    from spateo_amd import dd

    for name in ("cloud257_k6", "isolated", "self_loop", "lh0", "empty_both", "n1", "graph_budget_3"):
        c = hc.graph_case(name)
        ref = hc.graph_reference(name)
        results = []
        for adj in (c["adj"], sp.csr_matrix(c["adj"]), sp.coo_matrix(c["adj"]), c["adj"].toarray()):
            out, info = dd.digitize_general(c["pc"], adj, c["lower"], c["upper"], max_itr=c["max_itr"], lh=c["lh"], hh=c["hh"],
                                            return_info=True)
            results.append(out)
            assert info["iterations"] == ref[1] == int(G[f"graph_{name}_itr"])
            call = seam[-1].calls[-1]
            for got, want in zip(call[1:4], hc.graph_csc(c)):        # every input form becomes the same CSC arrays
                assert np.array_equal(got, want) and got.dtype == want.dtype
            assert np.array_equal(call[4], hc.graph_fixed_value(c))
        for r in results:
            assert np.array_equal(r, ref[0], equal_nan=True)
    # explicit zeros are dropped, duplicates summed, unsorted indices sorted
    c = hc.graph_case("n63")
    coo = sp.coo_matrix(c["adj"])
    messy = sp.coo_matrix((np.r_[coo.data * 0.25, coo.data * 0.75, 0.0], (np.r_[coo.row, coo.row, 5], np.r_[coo.col, coo.col, 5])),
                          shape=coo.shape)
    dd.digitize_general(c["pc"], messy, c["lower"], c["upper"])
    got = seam[-1].calls[-1]
    assert np.array_equal(got[1], hc.graph_csc(c)[0]) and np.array_equal(got[2], hc.graph_csc(c)[1])
    assert np.allclose(got[3], hc.graph_csc(c)[2], rtol=1e-15, atol=0)
    # a dense matrix is converted in row blocks
    old = dd.DENSE_BLOCK_BYTES
    dd.DENSE_BLOCK_BYTES = 63 * 8 * 5
    try:
        blocks = dd.adjacency_csc(c["adj"].toarray(), 63)
    finally:
        dd.DENSE_BLOCK_BYTES = old
    for got, want in zip(blocks, hc.graph_csc(c)):
        assert np.array_equal(got, want)


def test_digitize_end_to_end_over_the_stand_in(seam, G):
    from spateo_amd import AnnDataLite, dd

    xy = hc.l_slice_cells()
    adata = AnnDataLite(obsm={"spatial": xy})
    assert dd.digitize(adata, (np.zeros((1, 1, 2), dtype=np.int32), hc.chain_l()), 1, **hc.L_CORNERS) is None
    assert np.array_equal(adata.obs["digital_layer"], G["digitize_layer"])
    assert np.array_equal(adata.obs["digital_column"], G["digitize_column"])
    calls = [c for k in seam for c in k.calls][-2:]          # (the seam binds a stand-in per call)
    assert [c[0] for c in calls] == ["grid", "grid"] and calls[0][1].shape == (40, 70)
    assert not np.array_equal(calls[0][1], calls[1][1])          # the two solves have the line roles swapped
    assert calls[0][4] == 1e-20 and calls[0][5] == 1e6
    inside = adata.obs["digital_layer"] != 0
    assert 150 < inside.sum() < 250 and (adata.obs["digital_layer"][inside] >= 1).all() and (adata.obs["digital_layer"] <= 100).all()
    dd.gridit(adata, layer_num=4, column_num=5)
    assert np.array_equal(adata.obs["layer_label"], G["digitize_layer_label"])
    assert np.array_equal(adata.obs["column_label"], G["digitize_column_label"])
    assert np.array_equal(np.asarray(adata.obs["grid_label"]).astype(str), G["digitize_grid_label"])
    # the two rasters handed in: no rasterisation, so any contour that holds the corners will do; other keys
    border, mask = dd.rasterize_contour(hc.chain_l(), (40, 70))
    gap = np.delete(hc.chain_l(), 40, axis=0)
    b = AnnDataLite(obsm={"X": xy})
    dd.digitize(b, (gap,), 0, **hc.L_CORNERS, spatial_key="X", dgl_layer_key="L", dgl_column_key="C", field_border=border,
                field_mask=2 * mask, max_itr=50)
    assert set(b.obs) == {"L", "C"} and seam[-1].calls[-1][5] == 50
    assert np.array_equal(seam[-1].calls[-1][3], 2 * mask)
    assert "cv2" not in sys.modules


@pytest.mark.skipif(torch.cuda.is_available(), reason="a statement about machines WITHOUT a GPU")
def test_no_gpu_means_loud_failure_not_a_fallback():
    from spateo_amd import dd

    c = hc.grid_case("rect_12x15")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dd.domain_heat_eqn_solver(c["heat_field"], c["min_line"], c["max_line"], c["edge_a"], c["edge_b"], c["border"], c["mask"])
    g = hc.graph_case("n63")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dd.digitize_general(g["pc"], g["adj"], g["lower"], g["upper"])
