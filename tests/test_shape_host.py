"""Host-side tests of the shape similarity and ``model_morphology`` without a device: exports, the ``mvf_shape_descriptors``
entries of the header and the ctypes table, every refusal of the entry point (returns before a launch) and of the Python calls
(before the kernels are bound), what the host adds over a NumPy stand-in for the kernels (the restatement of
tests/_shape_cases.py behind ``HipKernels.shape_queue`` / ``shape_read``), and ``model_morphology`` on closed analytic meshes."""
import ctypes
import importlib
import logging
import os
import re

import numpy as np
import pytest

import _shape_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mvf.h")
G = sc.load()
NAMES = ("subspace_descriptors", "calculate_eigenvector", "model_eigenvector", "pairwise_shape_similarity", "shape_similarity_matrix")


class ShapeCpuKernels:
    """``HipKernels.shape_queue`` / ``shape_read`` on the CPU."""

    def __init__(self, device=None, dtype="float64"):
        self.device, self.dtype_name, self.queued, self.reads = device, dtype, [], 0

    def shape_queue(self, pts, lo, hi, order, centroid):
        pts = np.asarray(pts)
        n = np.shape(lo)[1]
        lo2, hi2 = sc.tables(pts, n)
        assert np.array_equal(lo, lo2) and np.array_equal(hi, hi2) and np.array_equal(centroid, np.mean(pts, axis=0))
        self.queued.append((pts, n, {v: k for k, v in sc.ORDERS.items()}[order]))
        return len(self.queued) - 1

    def shape_read(self, queued):
        self.reads += 1
        out = []
        for q in queued:
            r = sc.describe(*self.queued[q])
            out.append({k: r[k] for k in ("voxel", "count", "cosine", "dist", "rank", "point_voxel", "n_dropped", "n_overlap")})
        return out


@pytest.fixture
def seam(monkeypatch):
    from spateo_amd import _runtime as rt

    made = []
    monkeypatch.setattr(rt, "_make_kernels", lambda device, dtype: made.append(ShapeCpuKernels(device, dtype)) or made[-1])
    monkeypatch.setattr(rt, "_shared_kernels", lambda device, dtype: rt._make_kernels(device, dtype))
    return made


@pytest.fixture
def no_kernels(monkeypatch):
    from spateo_amd import _runtime as rt

    def refuse(device, dtype):
        raise AssertionError("the kernels were bound before the arguments were refused")

    monkeypatch.setattr(rt, "_make_kernels", refuse)
    monkeypatch.setattr(rt, "_shared_kernels", refuse)


# --------------------------------------------------------------------------------------------------------- exports, header
def test_exports():
    import spateo_amd as st
    from spateo_amd.tdr import morphometrics
    from spateo_amd.tdr.morphometrics import morphology, shape_similarity

    mm = importlib.import_module("spateo_amd.tdr.morphometrics.model_morphology")     # (the package attribute is the function)
    assert set(shape_similarity.__all__) == set(NAMES) and mm.__all__ == ["model_morphology"]
    for name in NAMES:
        assert getattr(st.tdr, name) is getattr(shape_similarity, name) is getattr(morphometrics, name)
    assert st.tdr.model_morphology is mm.model_morphology is morphometrics.model_morphology
    assert "model_morphology" not in morphology.__all__
    assert "Not here" in morphology.__doc__ and "needs a surface mesh" not in morphology.__doc__


def test_header_and_ctypes_table():
    from spateo_amd import _lib

    text = open(HEADER).read()
    assert int(re.search(r"#define MVF_SHAPE_MAX_NSUB (\d+)", text).group(1)) == _lib.SHAPE_MAX_NSUB == sc.MAX_NSUB
    assert _lib.SHAPE_ORDERS == sc.ORDERS
    assert {"mvf_shape_descriptors", "mvf_shape_descriptors_workspace_bytes"} <= set(_lib.SIGNATURES)
    note = text.split("int mvf_shape_descriptors(")[0].rsplit("/*", 1)[1]
    assert "Replaces:" in note and "shape_similarity.py:164-177" in note and "float32" in note
    res, args = _lib.SIGNATURES["mvf_shape_descriptors"]
    assert res is ctypes.c_int and len(args) == 18 and args[6] == ctypes.POINTER(ctypes.c_double)
    lib = _lib.load()
    assert lib.mvf_version() == 7 and hasattr(lib, "mvf_shape_descriptors")


def test_entry_point_refuses_and_returns_without_launching():
    from spateo_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(256)     # never dereferenced: every call below returns before a launch
    g = (ctypes.c_double * 3)(0.0, 0.0, 0.0)

    def call(pts=p, n=100, lo=p, hi=p, nsub=4, order=3, g=g, pv=p, outs=p, counts=p, ws=p, ws_bytes=1 << 30):
        return lib.mvf_shape_descriptors(pts, n, lo, hi, nsub, order, g, pv, outs, outs, outs, outs, outs, outs, counts, ws, ws_bytes, None)

    for kw, msg in ((dict(nsub=0), b"bad shape"), (dict(nsub=129), b"bad shape"), (dict(n=0), b"bad shape"), (dict(n=-1), b"bad shape"),
                    (dict(n=1 << 31), b"bad shape"), (dict(order=0), b"bad order"), (dict(order=4), b"bad order"),
                    (dict(pts=None), b"null pointer"), (dict(lo=None), b"null pointer"), (dict(hi=None), b"null pointer"),
                    (dict(g=None), b"null pointer"), (dict(pv=None), b"null pointer"), (dict(outs=None), b"null pointer"),
                    (dict(counts=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                    (dict(ws=ctypes.c_void_p(264)), b"256-byte aligned"), (dict(ws_bytes=8), b"workspace too small")):
        assert call(**kw) != 0, kw
        assert b"mvf_shape_descriptors" in lib.mvf_last_error() and msg in lib.mvf_last_error(), (kw, lib.mvf_last_error())
    with pytest.raises(_lib.MVFError, match="bad order"):
        _lib.check(call(order=7), "mvf_shape_descriptors")
    for n, nsub in ((0, 4), (-1, 4), (1 << 31, 4), (100, 0), (100, 129)):
        assert lib.mvf_shape_descriptors_workspace_bytes(n, nsub) == 0
    small, large = lib.mvf_shape_descriptors_workspace_bytes(1000, 1), lib.mvf_shape_descriptors_workspace_bytes(1000, 128)
    assert small % 256 == 0 and small >= 4 * 8 * 1000 and large - small >= 2 * 4 * (128 ** 3 - 1)


# ------------------------------------------------------------------------------------------------------------- validation
def test_refusals_come_before_the_kernels(no_kernels):
    import spateo_amd as st

    X = np.random.default_rng(0).random((50, 3))
    for fn in (st.tdr.subspace_descriptors, st.tdr.model_eigenvector):
        for bad in (np.zeros((5, 2)), np.zeros((5, 4)), np.zeros(5), np.zeros((0, 3)), np.zeros((2, 3, 3))):
            with pytest.raises(ValueError, match=r"\(n >= 1, 3\)"):
                fn(bad)
        for bad in (np.full((4, 3), np.nan), np.array([[0.0, 1.0, np.inf]] * 3)):
            with pytest.raises(ValueError, match="non-finite"):
                fn(bad)
        with pytest.raises(NotImplementedError, match="at most 128"):
            fn(X, n_subspace=129)
        for bad in (0, -2, 2.5):
            with pytest.raises(ValueError, match="positive integer"):
                fn(X, n_subspace=bad)
    with pytest.raises(ValueError, match="``order`` value is wrong."):
        st.tdr.subspace_descriptors(X, order="quartic")
    with pytest.raises(ValueError, match="non-finite"):
        st.tdr.pairwise_shape_similarity(X, np.full((4, 3), np.nan))
    with pytest.raises(ValueError, match=r"\(n >= 1, 3\)"):
        st.tdr.shape_similarity_matrix([X, np.zeros((3, 2))])
    assert st.tdr.shape_similarity_matrix([]).shape == (0, 0)


def test_a_cloud_without_subspaces_is_named(seam):
    import spateo_amd as st

    far = np.array([[0.0, 0.0, 0.0], [1.5, 1.5, 1.5], [4.0, 4.0, 4.0]])
    for call in (lambda: st.tdr.subspace_descriptors(far, n_subspace=4), lambda: st.tdr.model_eigenvector(far, n_subspace=4),
                 lambda: st.tdr.pairwise_shape_similarity(sc.CASES["E_xconst"]["pcs"], far, n_subspace=4)):
        with pytest.raises(ValueError, match="no subspace of the 4\\^3 holds more than one point \\(1 of 3 points lie in no subspace\\)"):
            call()


# ------------------------------------------------------------------------------------------------------- what the host adds
def test_model_eigenvector_and_score_over_the_stand_in(seam):
    import spateo_amd as st

    A, B = sc.CASES["A"], sc.CASES["B4"]
    d = st.tdr.subspace_descriptors(A["pcs"], n_subspace=A["n"])
    assert np.array_equal(d["voxel"], G["A_cubic_voxel"]) and d["n_dropped"] > 0 and d["n_overlap"] == 0
    e, w = st.tdr.model_eigenvector(A["pcs"], n_subspace=A["n"])
    assert np.array_equal(w, G["A_cubic_w"])                      # (the tables and the centroid were checked by the stand-in)
    nz = G["A_cubic_e"] != 0
    assert np.abs(e[nz] / G["A_cubic_e"][nz] - 1.0).max() <= sc.dist_bounds(G, "A")[0]
    score = st.tdr.pairwise_shape_similarity(A["pcs"], B["pcs"], n_subspace=4)
    assert isinstance(score, float) and abs(score - float(G["score_A_B4"])) <= 1e-4 + 1e-12
    assert seam[-1].reads == 1 and len(seam[-1].queued) == 2        # both models queued, one read


def test_similarity_matrix_over_the_stand_in(seam):
    import spateo_amd as st

    models = [sc.CASES["A"]["pcs"], sc.CASES["B"]["pcs"], sc.CASES["C"]["pcs"] * 10.0]
    mat = st.tdr.shape_similarity_matrix(models, n_subspace=4)
    assert seam[-1].reads == 1 and len(seam[-1].queued) == 3      # each eigenvector once, read back together
    assert mat.shape == (3, 3) and np.array_equal(mat, mat.T) and np.array_equal(np.diag(mat), np.ones(3))
    assert np.isfinite(mat).all() and (mat > 0).all()
    for i in range(3):
        for j in range(i + 1, 3):
            assert mat[i, j] == st.tdr.pairwise_shape_similarity(models[i], models[j], n_subspace=4)


# --------------------------------------------------------------------------------------------------------- model_morphology
CUBE_POINTS = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64)
CUBE_TRIANGLES = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6],
                           [3, 0, 4], [3, 4, 7]])


class Faces:
    """What model_morphology touches of a pyvista PolyData."""

    def __init__(self, points, triangles):
        self.points = points
        self.faces = np.c_[np.full(len(triangles), 3), triangles].ravel()
        self.n_points = len(points)


def test_unit_cube_box_and_tetrahedron():
    import spateo_amd as st

    m = st.tdr.model_morphology((CUBE_POINTS, CUBE_TRIANGLES))
    assert list(m) == ["Length(x)", "Width(y)", "Height(z)", "Surface_area", "Volume", "V/SA_ratio"]
    assert m == {"Length(x)": 1.0, "Width(y)": 1.0, "Height(z)": 1.0, "Surface_area": 6.0, "Volume": 1.0, "V/SA_ratio": round(1 / 6, 5)}
    # a scaled, translated box 2 x 3 x 0.5 at (10, -20, 5), as an object with pyvista-style faces, and a cloud of 1234 cells
    box = Faces(CUBE_POINTS * [2.0, 3.0, 0.5] + [10.0, -20.0, 5.0], CUBE_TRIANGLES)
    m = st.tdr.model_morphology(box, pc=np.zeros((1234, 3)))
    area, vol = 2 * (6.0 + 1.0 + 1.5), 3.0
    assert m == {"Length(x)": 2.0, "Width(y)": 3.0, "Height(z)": 0.5, "Surface_area": area, "Volume": vol,
                 "V/SA_ratio": round(vol / area, 5), "cell_density": round(1234 / vol, 5)}
    assert st.tdr.model_morphology(box, pc=box)["cell_density"] == round(8 / 3.0, 5)
    assert st.tdr.model_morphology(box, pc=list(range(7)))["cell_density"] == round(7 / 3.0, 5)
    # a regular tetrahedron of edge a: area sqrt(3) a^2, volume a^3 / (6 sqrt(2))
    a = 2.0 * np.sqrt(2.0)
    tet = (np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64) + 7.0, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]))
    m = st.tdr.model_morphology(tet)
    assert m["Surface_area"] == round(np.sqrt(3.0) * a * a, 5) and m["Volume"] == round(a ** 3 / (6.0 * np.sqrt(2.0)), 5)
    assert m["V/SA_ratio"] == round(m["Volume"] / m["Surface_area"], 5) and m["Length(x)"] == m["Width(y)"] == m["Height(z)"] == 2.0


def test_inside_out_cube_and_open_box(caplog):
    import spateo_amd as st

    with caplog.at_level(logging.INFO, logger="spateo_amd"):
        m = st.tdr.model_morphology((CUBE_POINTS, CUBE_TRIANGLES[:, ::-1]))
    assert m["Volume"] == 1.0 and m["Surface_area"] == 6.0
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING]
    assert sum("of model" in r.getMessage() for r in caplog.records) == 6
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="spateo_amd"):
        m = st.tdr.model_morphology((CUBE_POINTS, CUBE_TRIANGLES[2:]))      # the bottom is missing
    warned = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING]
    assert len(warned) == 1 and "open surface is not meaningful" in warned[0] and m["Surface_area"] == 5.0


def test_model_morphology_refuses_what_is_not_a_triangle_surface():
    import spateo_amd as st

    quads = Faces(CUBE_POINTS, CUBE_TRIANGLES)
    quads.faces = np.array([4, 0, 1, 2, 3, 4, 4, 5, 6, 7])
    with pytest.raises(NotImplementedError, match="not triangles"):
        st.tdr.model_morphology(quads)
    with pytest.raises(NotImplementedError, match="only triangle cells"):
        st.tdr.model_morphology((CUBE_POINTS, np.zeros((2, 4), dtype=int)))
    with pytest.raises(TypeError, match="model_morphology"):
        st.tdr.model_morphology(CUBE_POINTS)
