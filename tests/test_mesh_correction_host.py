"""Host side of the mesh correction, no GPU: the label grid, the pairs, the parameter sets and the smoothing against the goldens of
the real ``mesh_correction_utils.py`` (tests/golden/ref_mesh_correction.npz); the exact labelling against brute force at L = 3 and
against tables with a planted minimum and a planted tie; the mesh argument; every refusal and every argument error of the three
entry points at the C ABI with nothing launched; the exported symbols, ``_lib``'s constants and ``__all__``."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import _icp_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def G():
    return ic.load()


@pytest.fixture(scope="module")
def mc():
    from spateo_amd import _mesh_correction

    return _mesh_correction


def test_label_grid_equals_the_reference(G, mc):
    for i, (m, n, log) in enumerate(G["grid_args"]):
        got = np.array(mc._generate_labeling(float(m), int(n), "log" if log else "linear"), dtype=np.float64)
        assert np.array_equal(got, G[f"grid_{i}"]), (m, n, log)
        assert got[0] == (1.0 if log else 0.0) and len(got) == int(n)      # label 0 is "no change", odd count or even
    with pytest.raises(ValueError, match="Unknown scale_type"):
        mc._generate_labeling(1.0, 3, "cubic")


def test_pairs_and_parameter_sets_equal_the_reference(G, mc):
    pairs = mc._make_pairs()
    assert pairs.dtype == np.int32 and np.array_equal(pairs, G["pairs"]) and pairs.shape == (10, 2)
    labels = np.array([mc._generate_labeling(30.0, 5), mc._generate_labeling(30.0, 5), mc._generate_labeling(30.0, 5),
                       mc._generate_labeling(4.0, 5), mc._generate_labeling(1.5, 5, "log")], dtype=np.float64).T
    labels = mc._update_parameter(labels, {"rotation": np.array([2.0, -1.0, 0.5]), "translation": 0.75, "scaling": 1.05})
    assert np.array_equal(labels, G["labels"])
    for p in ((0, 1), (1, 4), (3, 4)):
        assert np.array_equal(mc._get_parameters_from_pair(np.array(p), labels), G[f"sets_{p[0]}{p[1]}"])


def test_smoothing_equals_the_reference(G, mc):
    raw = np.split(G["smooth_in"], np.cumsum(G["smooth_sizes"])[:-1])
    keep = [c.copy() for c in raw]
    assert np.array_equal(np.concatenate(mc._smooth_contours(raw, 5)), G["smooth_w5"])
    assert np.array_equal(np.concatenate(mc._smooth_contours(raw, 3, 2)), G["smooth_w3_it2"])
    assert all(np.array_equal(a, b) for a, b in zip(raw, keep))            # the input is left alone


def _energy(binaries, pairs, labels):
    return sum(float(np.float64(b[labels[i], labels[j]])) for b, (i, j) in zip(binaries, pairs))


def test_exact_labelling_equals_brute_force(mc):
    rng = np.random.default_rng(4)
    pairs = mc._make_pairs()
    for trial in range(5):
        L = 3
        binaries = rng.random((10, L, L)).astype(np.float32)
        labels, value = mc.solve_labeling(binaries, pairs)
        best = min(itertools.product(range(L), repeat=5), key=lambda l: (_energy(binaries, pairs, l), l))
        assert tuple(labels) == best and abs(value - _energy(binaries, pairs, best)) < 1e-12


def test_exact_labelling_finds_a_planted_minimum_and_breaks_a_tie_towards_label_zero(mc):
    pairs = mc._make_pairs()
    L = 5
    planted = (3, 0, 4, 1, 2)
    binaries = np.ones((10, L, L), dtype=np.float32)
    for b, (i, j) in zip(binaries, pairs):
        b[planted[i], planted[j]] = 0.25                                   # only the planted labelling collects all ten
    labels, value = mc.solve_labeling(binaries, pairs)
    assert tuple(labels) == planted and value == 2.5
    flat = np.full((10, L, L), 0.5, dtype=np.float32)                      # every labelling ties: the lowest flat index wins
    labels, value = mc.solve_labeling(flat, pairs)
    assert tuple(labels) == (0, 0, 0, 0, 0) and value == 5.0
    for b, (i, j) in zip(binaries, pairs):                                 # a second, equal minimum at a HIGHER flat index
        b[4, 4] = 0.25
    assert tuple(mc.solve_labeling(binaries, pairs)[0]) == planted
    assert mc.LABEL_NUM_MAX == 24 and 24 ** 5 * 8 <= mc.LABELLING_MAX_BYTES < 25 ** 5 * 8
    with pytest.raises(NotImplementedError, match="label_num = 25"):
        mc.solve_labeling(np.zeros((10, 25, 25), dtype=np.float32), pairs)


def test_the_mesh_argument(mc):
    verts, tri = ic.ellipsoid()
    m = mc._as_mesh((verts, tri), "t")
    assert np.array_equal(m.edges, ic.unique_edges(tri)) and m.edges.dtype == np.int32 and len(m.edges) == 336
    duck = type("PolyData", (), {})()
    duck.points, duck.faces = verts, np.column_stack([np.full(len(tri), 3), tri]).reshape(-1)
    assert np.array_equal(mc._as_mesh(duck, "t").triangles, tri)
    duck.faces = np.array([3, 0, 1, 2, 4, 0, 1, 2, 3])
    with pytest.raises(NotImplementedError, match="not triangles"):
        mc._as_mesh(duck, "t")
    with pytest.raises(NotImplementedError, match="only triangle cells"):
        mc._as_mesh((verts, np.zeros((4, 4), dtype=int)), "t")
    with pytest.raises(ValueError, match="index"):
        mc._as_mesh((verts, np.array([[0, 1, len(verts)]])), "t")
    with pytest.raises(TypeError, match="a mesh is"):
        mc._as_mesh(verts, "t")
    import sys

    assert "pyvista" not in sys.modules


class _Slice:
    def __init__(self, xy):
        self.obsm = {"spatial": np.array(xy)}


def test_constructor_and_named_refusals(mc, monkeypatch):
    import inspect
    import sys

    for gone in ("alphashape", "cv2"):      # (as on a machine without them: `import` of a None entry is an ImportError)
        monkeypatch.setitem(sys.modules, gone, None)

    import spateo_amd as st

    sig = inspect.signature(st.align.Mesh_correction.__init__)
    names = list(sig.parameters)[1:]
    assert names[:22] == ["slices", "z_heights", "mesh", "spatial_key", "key_added", "normalize_spatial", "init_rotation",
                          "init_translation", "init_scaling", "max_rotation_angle", "max_translation_scale", "max_scaling",
                          "min_rotation_angle", "min_translation_scale", "min_scaling", "label_num", "fastpd_iter", "max_iter",
                          "anneal_rate", "multi_processing", "subsample_slices", "verbose"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["max_rotation_angle"], d["max_translation_scale"], d["max_scaling"], d["min_rotation_angle"], d["min_translation_scale"],
            d["min_scaling"], d["label_num"], d["fastpd_iter"], d["max_iter"], d["anneal_rate"]) == (180, 0.5, 1.5, 10, 1, 1.1, 15, 100,
                                                                                                    10, 0.7)
    verts, tri = ic.ellipsoid()
    heights = [30.0, 44.0]
    slices = [_Slice(ic.closed_curve(40, s)) for s in (1, 2)]
    model = st.align.Mesh_correction(slices, heights, (verts, tri), normalize_spatial=True, label_num=5, fastpd_iter=7, multi_processing=True)
    assert model.slices_scale == 14.0 and model.contours == [None, None]
    z = model.mesh.points[:, 2]
    assert abs((z.max() - z.min()) - 14.0) < 1e-9 and abs((z.max() + z.min()) / 2 - 37.0) < 1e-9
    model.best_transformation = {"rotation": np.array([1.0, 2.0, 3.0]), "translation": 0.5, "scaling": 1.1}
    model.max_translation = 2.0
    labels = model.generate_labels()
    assert labels.shape == (5, 5) and np.array_equal(labels[0], [1.0, 2.0, 3.0, 0.5, 1.1])
    with pytest.raises(ValueError, match="no contours yet"):
        model.run_discrete_optimization()
    with pytest.raises(ImportError, match="set_contours"):
        model.extract_contours()
    with pytest.raises(ImportError, match="contours="):
        model.extract_contours(method="opencv")
    with pytest.raises(NotImplementedError, match="not implemented"):
        model.extract_contours(method="marching")
    with pytest.raises(ValueError, match="2 contours|contours for 2"):
        model.set_contours([np.zeros((3, 2))])
    for bad, exc, match in ((dict(z_heights=[1.0, 1.0]), ValueError, "unique"), (dict(z_heights=[1.0]), ValueError, "same length"),
                            (dict(label_num=25), NotImplementedError, "label_num = 25"), (dict(spatial_key="nope"), ValueError, "spatial key")):
        kw = dict(z_heights=heights)
        kw.update(bad)
        zh = kw.pop("z_heights")
        with pytest.raises(exc, match=match):
            st.align.Mesh_correction(slices, zh, (verts, tri), **kw)


def test_exported_names_and_constants():
    import spateo_amd as st
    from spateo_amd import _lib, _mesh_correction

    for name in ("icp", "icp_batch", "mesh_contours", "mesh_correction_loss", "Mesh_correction"):
        assert name in st.align.__all__ and name in _mesh_correction.__all__ and getattr(st.align, name) is getattr(_mesh_correction, name)
    text = open(os.path.join(ROOT, "include", "mvf.h")).read()
    assert int(re.search(r"#define MVF_ICP_MAX_POINTS (\d+)", text).group(1)) == _lib.ICP_MAX_POINTS == 512
    lib = _lib.load()
    for sym in ("mvf_icp_batch", "mvf_icp_batch_workspace_bytes", "mvf_mesh_loss", "mvf_mesh_loss_workspace_bytes", "mvf_mesh_contours"):
        assert hasattr(lib, sym) and sym in _lib.SIGNATURES
        assert re.search(r"Replaces:[^;]*?mesh_correction_utils\.py[\s\S]*?\b" + sym + r"\(", text), sym
    assert ctypes.sizeof(_lib.IcpProblem) == 64 and lib.mvf_version() == 7
    for k in ("HipKernels.icp_batch", "HipKernels.mesh_loss", "HipKernels.mesh_contours"):
        from spateo_amd import _kernels

        assert callable(getattr(_kernels.HipKernels, k.split(".")[1]))


def test_c_abi_refuses_bad_arguments_without_launching():
    """Every refusal returns a status and names the entry point in mvf_last_error; the pointers are never dereferenced
    (tests/test_gpu_icp_kernels.py and tests/test_gpu_mesh_correction.py repeat some of the calls on real device buffers)."""
    from spateo_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(16)
    m3 = (ctypes.c_double * 3)(1.0, 2.0, 3.0)
    p5 = (ctypes.c_double * 5)(0.0, 0.0, 0.0, 0.0, 1.0)
    # ---- mvf_icp_batch
    assert lib.mvf_icp_batch_workspace_bytes(0) == 0 and lib.mvf_icp_batch_workspace_bytes(-3) == 0
    assert lib.mvf_icp_batch_workspace_bytes(5) == 5 * 64 and lib.mvf_icp_batch_workspace_bytes(45000) == 4096 * 64

    def icp(n1=10, n2=10, nprob=1, max_iter=20, err=1e-6, inl=0.1, gam=0.05, sub=500, ws=p, ws_bytes=64, c1=16, gamma=16, stats=16, recs=True):
        rec = _lib.IcpProblem(contour_1=c1, n1=n1, contour_2=16, n2=n2, gamma=gamma, stats=stats, T_contour_2=None, translation=None)
        arr = (_lib.IcpProblem * 1)(rec)
        return lib.mvf_icp_batch(arr if recs else None, nprob, max_iter, err, inl, gam, sub, 1, ws, ws_bytes, None)

    refused = [dict(n1=0), dict(n2=0), dict(n1=-4), dict(nprob=-1), dict(recs=False), dict(max_iter=0), dict(max_iter=-2),
               dict(err=float("nan")), dict(inl=float("nan")), dict(gam=float("nan")), dict(sub=513), dict(sub=0, n1=513),
               dict(sub=-1, n2=600), dict(c1=None), dict(gamma=None), dict(stats=None), dict(ws=None), dict(ws_bytes=63),
               dict(ws=ctypes.c_void_p(12)), dict(n1=1 << 41)]
    for kw in refused:
        assert icp(**kw) != 0 and b"mvf_icp_batch" in lib.mvf_last_error(), (kw, lib.mvf_last_error())
    assert icp(sub=513) != 0 and b"MVF_ICP_MAX_POINTS" in lib.mvf_last_error()
    assert icp(ws_bytes=63) != 0 and b"workspace too small" in lib.mvf_last_error()
    assert icp(nprob=0) == 0 and icp(nprob=0, recs=False) == 0               # an empty batch launches nothing
    # ---- mvf_mesh_loss
    assert lib.mvf_mesh_loss_workspace_bytes(0, 4) == 0 and lib.mvf_mesh_loss_workspace_bytes(4, 0) == 0
    assert lib.mvf_mesh_loss_workspace_bytes(3, 4) == 96 + 48
    assert lib.mvf_mesh_loss_workspace_bytes(45000, 20) == lib.mvf_mesh_loss_workspace_bytes(4096, 20) == 4096 * 20 * 12
    ws_need = lib.mvf_mesh_loss_workspace_bytes(3, 4)

    def loss(V=100, E=300, mean=m3, nT=3, total=50, nS=4, max_iter=20, inl=0.1, sub=500, verts=p, edges=p, params=p, heights=p, contours=p,
             offsets=p, out=p, ws=p, ws_bytes=ws_need):
        return lib.mvf_mesh_loss(verts, V, edges, E, mean, params, nT, heights, contours, offsets, total, nS, max_iter, 1e-6, inl, 0.05, sub,
                                 out, None, None, ws, ws_bytes, None)

    nan3 = (ctypes.c_double * 3)(1.0, float("nan"), 3.0)
    refused = [dict(V=0), dict(V=1 << 31), dict(E=0), dict(E=1 << 31), dict(mean=None), dict(mean=nan3), dict(nT=-1), dict(total=0), dict(nS=0), dict(nS=1 << 24),
               dict(max_iter=0), dict(inl=float("nan")), dict(sub=0), dict(sub=513), dict(verts=None), dict(edges=None), dict(params=None),
               dict(heights=None), dict(contours=None), dict(offsets=None), dict(out=None), dict(ws=None), dict(ws_bytes=ws_need - 1),
               dict(ws=ctypes.c_void_p(8))]
    for kw in refused:
        assert loss(**kw) != 0 and b"mvf_mesh_loss" in lib.mvf_last_error(), (kw, lib.mvf_last_error())
    assert loss(nT=0) == 0
    # ---- mvf_mesh_contours
    def cont(V=100, E=300, mean=m3, param=p5, nS=4, cap=10, verts=p, edges=p, heights=p, points=p, counts=p):
        return lib.mvf_mesh_contours(verts, V, edges, E, mean, param, heights, nS, cap, points, counts, None)

    inf5 = (ctypes.c_double * 5)(0.0, float("inf"), 0.0, 0.0, 1.0)
    refused = [dict(V=0), dict(E=0), dict(mean=None), dict(mean=nan3), dict(param=None), dict(param=inf5), dict(nS=0), dict(nS=1 << 24), dict(cap=-1),
               dict(cap=1 << 31), dict(verts=None), dict(edges=None), dict(heights=None), dict(points=None), dict(counts=None)]
    for kw in refused:
        assert cont(**kw) != 0 and b"mvf_mesh_contours" in lib.mvf_last_error(), (kw, lib.mvf_last_error())


def test_extract_contours_filters_smooths_and_refuses_an_empty_slice(mc, monkeypatch):
    """The extraction itself belongs to ``alphashape``; stand-ins for it and for ``shapely.geometry`` return prepared polygons,
    so what runs here is the part restated on the host: the sampling, the filter, the smoothing, the concatenation, the refusal."""
    import sys
    import types

    import spateo_amd as st

    class Polygon:
        def __init__(self, xy):
            self.exterior = types.SimpleNamespace(coords=[tuple(p) for p in xy])

    class MultiPolygon:
        def __init__(self, polys):
            self.geoms = polys

    big, small = ic.closed_curve(60, 1), ic.closed_curve(8, 2)
    seen = []

    def alphashape(points, alpha):
        seen.append((len(points), alpha))
        return MultiPolygon([Polygon(big), Polygon(small)]) if len(seen) % 2 else Polygon(big)

    monkeypatch.setitem(sys.modules, "alphashape", types.SimpleNamespace(alphashape=alphashape))
    monkeypatch.setitem(sys.modules, "shapely", types.ModuleType("shapely"))
    monkeypatch.setitem(sys.modules, "shapely.geometry", types.SimpleNamespace(Polygon=Polygon, MultiPolygon=MultiPolygon))
    verts, tri = ic.ellipsoid()
    slices = [_Slice(ic.closed_curve(300, s)) for s in (3, 4)]
    model = st.align.Mesh_correction(slices, [30.0, 44.0], (verts, tri))
    model.extract_contours(n_sampling=100, alpha_shape_kwargs={"alpha": 0.25}, seed=5)
    assert seen == [(100, 0.25), (100, 0.25)]
    want = mc._smooth_contours([big], 5)[0]
    assert all(np.array_equal(c, want) for c in model.contours)                 # the 8-point polygon is filtered out (< 20)
    model.extract_contours(smoothing=False, filter_contours=False)
    assert np.array_equal(model.contours[0], np.concatenate([big, small])) and np.array_equal(model.contours[1], big)
    with pytest.raises(ValueError, match="slice 0 is left without a contour"):
        model.extract_contours(contour_filter_threshold=61)
    monkeypatch.setitem(sys.modules, "cv2", types.SimpleNamespace(__version__="0"))
    with pytest.raises(NotImplementedError, match="not restated"):
        model.extract_contours(method="opencv")
