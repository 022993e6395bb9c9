"""``mvf_mesh_contours`` / ``mvf_mesh_loss`` (csrc/mvf_icp.hip) through the raw C ABI on ``cuda:0`` and ``st.align.mesh_contours``,
``mesh_correction_loss`` and ``Mesh_correction`` above them, against the restatement of tests/_icp_cases.py (proved against the
real reference by tests/test_icp_kernel_refs.py) on a jittered ellipsoid of 224 triangles and 4 - 5 slices.

Bounds: contour counts, cut flags and ``gamma`` are equal; a float64 loss is within ``n_slices 2^-52 max(1, loss)`` of the
restatement's (the only freedom is the order of a sum of n_slices terms); the float32 tables within one float32 ulp; coordinates
within 64 x the restatement's own 4-ulp deviation."""
import ctypes

import numpy as np
import pytest
import torch

import _icp_cases as ic
from _kernel_scaffold import (MODES, SENTINEL, Ws as _Ws, called as _called, dev as _dev, guarded as _guarded, intact as _intact,
                              same_bits as _same_bits, stream as _stream, under as _under)

pytestmark = pytest.mark.gpu

HEIGHTS = np.array([30.0, 36.0, 44.0, 50.0])
TRUTH = np.array([4.0, -3.0, 10.0, 1.0, 1.05])
IDENTITY = np.array([0.0, 0.0, 0.0, 0.0, 1.0])


@pytest.fixture(scope="module")
def lib():
    from spateo_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


@pytest.fixture(scope="module")
def case():
    verts, tri = ic.ellipsoid()
    contours = ic.slices_of(verts, tri, TRUTH, HEIGHTS, noise=0.05)
    return dict(verts=verts, tri=tri, edges=ic.unique_edges(tri), mean=verts.mean(0), contours=contours)


def _loss_bound(loss, n_slices):
    return n_slices * 2.0 ** -52 * np.maximum(1.0, np.abs(loss))


def raw_contours(lib, case, param, heights, cap):
    verts, edges = _dev(case["verts"]), _dev(case["edges"], torch.int32)
    nS = len(heights)
    pts = _guarded(nS * cap * 2)
    cnt = _guarded(nS, torch.int32)
    m3, p5 = (ctypes.c_double * 3)(*case["mean"]), (ctypes.c_double * 5)(*param)
    rc = lib.mvf_mesh_contours(verts.data_ptr(), len(case["verts"]), edges.data_ptr(), len(case["edges"]), m3, p5,
                               _dev(heights).data_ptr(), nS, cap, pts.data_ptr(), cnt.data_ptr(), _stream())
    assert rc == 0, lib.mvf_last_error()
    _called()
    torch.cuda.synchronize()
    assert _intact(pts, nS * cap * 2) and _intact(cnt, nS), "wrote past the end of an output"
    return pts[: nS * cap * 2].cpu().numpy().reshape(nS, cap, 2), cnt[:nS].cpu().numpy()


def raw_loss(lib, case, params, heights, contours, subsample=500, details=True):
    verts, edges = _dev(case["verts"]), _dev(case["edges"], torch.int32)
    params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 5)
    nT, nS = len(params), len(heights)
    flat = np.concatenate(contours)
    off = np.concatenate([[0], np.cumsum([len(c) for c in contours])]).astype(np.int64)
    loss = _guarded(nT)
    gamma = _guarded(nT * nS)
    count = _guarded(nT * nS, torch.int32)
    need = int(lib.mvf_mesh_loss_workspace_bytes(nT, nS))
    ws = _Ws(need, fill=0)   # exactly the bytes asked for, guards either side
    m3 = (ctypes.c_double * 3)(*case["mean"])
    keep = [_dev(params), _dev(heights), _dev(flat), _dev(off, torch.int64)]
    rc = lib.mvf_mesh_loss(verts.data_ptr(), len(case["verts"]), edges.data_ptr(), len(case["edges"]), m3, keep[0].data_ptr(), nT,
                           keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), len(flat), nS, 20, 1e-6, 0.1, 0.05, subsample,
                           loss.data_ptr(), gamma.data_ptr() if details else None, count.data_ptr() if details else None,
                           ws.ptr, need, _stream())
    assert rc == 0, lib.mvf_last_error()
    _called()
    torch.cuda.synchronize()
    assert _intact(loss, nT) and _intact(gamma, nT * nS) and _intact(count, nT * nS)
    assert ws.guards_intact(), "wrote outside the workspace"
    if not details:
        assert _intact(gamma, 0) and _intact(count, 0)
        return loss[:nT].cpu().numpy()
    return loss[:nT].cpu().numpy(), gamma[: nT * nS].cpu().numpy().reshape(nT, nS), count[: nT * nS].cpu().numpy().reshape(nT, nS)


def _coordinate_bound(case, param, heights):
    mag = float(np.abs(case["verts"]).max())
    dev = ic.deviation(lambda v, p: np.concatenate(ic.mesh_contours(v, case["edges"], case["mean"], p, heights)), (case["verts"], param), mag)
    return ic.ALLOW * max(dev, 2.0 ** -52) * mag


@pytest.mark.parametrize("param", [IDENTITY, TRUTH, np.array([-170.0, 95.0, 3.0, -2.0, 0.8])], ids=["identity", "truth", "wide"])
def test_contours_equal_the_restatement(lib, case, param):
    heights = np.append(HEIGHTS, 120.0)                    # the last one misses the mesh
    want = ic.mesh_contours(case["verts"], case["edges"], case["mean"], param, heights)
    cap = len(case["edges"])
    pts, cnt = raw_contours(lib, case, param, heights, cap)
    bound = _coordinate_bound(case, param, heights[:-1])
    assert np.array_equal(cnt, [len(w) for w in want]) and cnt[-1] == 0 and (cnt[:-1] > 0).all()
    for s, w in enumerate(want):
        assert np.abs(pts[s, : len(w)] - w).max(initial=0.0) <= bound
        assert (pts[s, len(w):] == SENTINEL[torch.float64]).all()       # the rest of the row is untouched
    small, cnt2 = raw_contours(lib, case, param, heights, 5)   # a capacity below the counts: the counts stay, 5 points are written
    assert np.array_equal(cnt2, cnt) and np.array_equal(small[:-1], pts[:-1, :5])
    _, cnt0 = raw_contours(lib, case, param, heights, 0)
    assert np.array_equal(cnt0, cnt)


def test_a_vertex_exactly_on_a_cut_plane_counts_as_above(lib, case):
    """Under the identity the device's z of a vertex is the restatement's bit for bit ((z - mean) + mean, sin 0 = 0, cos 0 = 1):
    a plane through a vertex cuts its edges to lower vertices only."""
    P = ic.transform(case["verts"], case["mean"], IDENTITY)
    v = int(np.argsort(P[:, 2])[len(P) // 2])
    h = np.array([P[v, 2]])
    e = case["edges"]
    touching = (e == v).any(axis=1)
    other = np.where(e[touching, 0] == v, e[touching, 1], e[touching, 0])
    want = ic.mesh_contours(case["verts"], e, case["mean"], IDENTITY, h)[0]
    pts, cnt = raw_contours(lib, case, IDENTITY, h, len(e))
    # (the bound is the one of the generic heights: a perturbed vertex would leave this plane, and change the count)
    assert cnt[0] == len(want) and np.abs(pts[0, : cnt[0]] - want).max() <= _coordinate_bound(case, IDENTITY, HEIGHTS)
    below = int((P[other, 2] < h[0]).sum())
    assert 0 < below < len(other)
    on_vertex = np.abs(want - P[v, :2]).max(axis=1) < 1e-9     # the cut points that ARE the vertex: one per lower neighbour
    assert on_vertex.sum() == below
    import spateo_amd as st

    api = st.align.mesh_contours((case["verts"], case["tri"]), h)[0]
    assert np.array_equal(api, pts[0, : cnt[0]])


@pytest.mark.parametrize("n_T", (1, 9))
def test_loss_equals_the_restatement(lib, case, n_T):
    from spateo_amd import _mesh_correction as mc

    if n_T == 1:
        params = TRUTH[None]
    else:   # L = 3: the nine parameter sets of the pair (rotation z, scale)
        labels = np.array([IDENTITY, [-6.0, -6.0, -6.0, -1.5, 1 / 1.1], [6.0, 6.0, 6.0, 1.5, 1.1]])
        labels = mc._update_parameter(labels, {"rotation": TRUTH[:3] * 0.5, "translation": 0.5, "scaling": 1.0})
        params = mc._get_parameters_from_pair(np.array([2, 4]), labels).reshape(9, 5)
    want, wgamma, wcount = ic.mesh_loss(case["verts"], case["edges"], case["mean"], params, HEIGHTS, case["contours"])
    loss, gamma, count = raw_loss(lib, case, params, HEIGHTS, case["contours"])
    print("loss", loss, "restated", want)
    assert np.array_equal(count, wcount) and np.array_equal(gamma, wgamma)
    assert (np.abs(loss - want) <= _loss_bound(want, len(HEIGHTS))).all()
    f32 = loss.astype(np.float32)
    assert (np.abs(f32 - want.astype(np.float32)) <= np.spacing(want.astype(np.float32))).all()
    assert np.array_equal(raw_loss(lib, case, params, HEIGHTS, case["contours"], details=False), loss)   # NULL details; same bits


@pytest.mark.parametrize("details", (True, False), ids=("details", "loss-only"))
def test_more_transformations_than_one_launch_holds(lib, case, details):
    """n_T = 4101 = 4096 + 5: the second chunk of the launch loop, whose pointers are displaced (params + t0 * 5, loss + t0,
    gamma + t0 * n_S, count + t0 * n_S) and which reuses the workspace of the first.  8 distinct parameter sets, tiled: every
    row equals the first of its kind bit for bit (no row depends on its place), and the 8 are the restatement's.  The workspace
    is exactly the queried size between its guards (``raw_loss``)."""
    n_T, heights, contours = 4101, HEIGHTS[:2], case["contours"][:2]
    rng = np.random.default_rng(4101)
    sets = np.concatenate([[IDENTITY, TRUTH], TRUTH + rng.uniform(-1.0, 1.0, (6, 5)) * [3.0, 3.0, 3.0, 1.0, 0.05]])
    assert len(np.unique(sets, axis=0)) == 8
    params = np.tile(sets, (n_T // 8 + 1, 1))[:n_T]
    want, wgamma, wcount = ic.mesh_loss(case["verts"], case["edges"], case["mean"], sets, heights, contours)
    assert int(lib.mvf_mesh_loss_workspace_bytes(n_T, 2)) == int(lib.mvf_mesh_loss_workspace_bytes(4096, 2))  # one chunk's worth
    got = raw_loss(lib, case, params, heights, contours, details=details)
    loss = got[0] if details else got
    assert loss.shape == (n_T,)
    for row in (0, 4095, 4096, 4100):
        assert _same_bits(loss[row], loss[row % 8]), row
    assert _same_bits(loss, np.tile(loss[:8], n_T // 8 + 1)[:n_T])
    print("loss", loss[:8], "restated", want)
    assert (np.abs(loss[:8] - want) <= _loss_bound(want, 2)).all()
    if details:
        gamma, count = got[1], got[2]
        assert np.array_equal(count[:8], wcount) and np.array_equal(gamma[:8], wgamma)
        for row in (0, 4095, 4096, 4100):
            assert _same_bits(gamma[row], gamma[row % 8]) and _same_bits(count[row], count[row % 8]), row
        assert _same_bits(gamma, np.tile(gamma[:8], (n_T // 8 + 1, 1))[:n_T])
        assert _same_bits(count, np.tile(count[:8], (n_T // 8 + 1, 1))[:n_T])


CONVENTION_COVERS = {"mvf_mesh_loss": MODES, "mvf_mesh_contours": MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", ["mvf_mesh_loss", "mvf_mesh_loss:loss-only", "mvf_mesh_contours"])
def test_calling_conventions(lib, case, entry, mode):
    """The plain call's bits on a side stream behind poisoned inputs, at displaced pointers, and with the inputs unchanged."""
    if entry == "mvf_mesh_contours":
        call = lambda: raw_contours(lib, case, TRUTH, HEIGHTS, len(case["edges"]))
    else:
        params = np.stack([IDENTITY, TRUTH, [8.0, 2.0, -5.0, -2.0, 0.95]])
        call = lambda: raw_loss(lib, case, params, HEIGHTS, case["contours"], details=entry == "mvf_mesh_loss")
    plain, got = _under(mode, call)
    plain, got = (plain, got) if isinstance(plain, tuple) else ((plain,), (got,))
    assert len(plain) == len(got) and all(_same_bits(a, b) for a, b in zip(plain, got))


def test_a_height_that_misses_the_mesh_and_thinned_cuts(lib, case):
    heights = np.array([36.0, 120.0, 44.0])
    contours = [case["contours"][1], case["contours"][0], case["contours"][2]]
    params = np.stack([TRUTH, IDENTITY])
    want, wgamma, wcount = ic.mesh_loss(case["verts"], case["edges"], case["mean"], params, heights, contours)
    loss, gamma, count = raw_loss(lib, case, params, heights, contours)
    assert np.array_equal(count, wcount) and (count[:, 1] == 0).all() and np.array_equal(gamma, wgamma) and (gamma[:, 1] == 0).all()
    assert np.array_equal(loss, want) and (loss == 1e6 / 3).all()
    # a subsample below the size of the cuts (28 - 30 points) and of the slice contours: both sides thinned by floor(j n / 12)
    want, wgamma, wcount = ic.mesh_loss(case["verts"], case["edges"], case["mean"], params, HEIGHTS, case["contours"], subsample=12)
    loss, gamma, count = raw_loss(lib, case, params, HEIGHTS, case["contours"], subsample=12)
    assert np.array_equal(count, wcount) and (count > 12).all() and np.array_equal(gamma, wgamma)
    assert (np.abs(loss - want) <= _loss_bound(want, len(HEIGHTS))).all()


def test_api_loss_and_refusals(lib, case):
    import spateo_amd as st

    mesh = (case["verts"], case["tri"])
    params = np.stack([IDENTITY, TRUTH, [8.0, 2.0, -5.0, -2.0, 0.95]])
    want, wgamma, wcount = ic.mesh_loss(case["verts"], case["edges"], case["mean"], params, HEIGHTS, case["contours"])
    loss, gamma, count = st.align.mesh_correction_loss(case["contours"], mesh, params, HEIGHTS, return_details=True)
    assert np.array_equal(gamma, wgamma) and np.array_equal(count, wcount) and (np.abs(loss - want) <= _loss_bound(want, 4)).all()
    assert loss[1] < loss[0]
    assert st.align.mesh_correction_loss(case["contours"], mesh, TRUTH, HEIGHTS) == loss[1]
    faces = np.column_stack([np.full(len(case["tri"]), 3), case["tri"]]).reshape(-1)      # a pyvista-style object
    duck = type("PolyData", (), {})()
    duck.points, duck.faces = case["verts"], faces
    assert np.array_equal(st.align.mesh_correction_loss(case["contours"], duck, params, HEIGHTS), loss)
    duck.faces = np.array([4, 0, 1, 2, 3])
    with pytest.raises(NotImplementedError, match="not triangles"):
        st.align.mesh_contours(duck, HEIGHTS)
    p = ctypes.c_void_p(8)
    assert lib.mvf_mesh_loss(p, 0, p, 5, None, p, 1, p, p, p, 5, 2, 20, 1e-6, 0.1, 0.05, 500, p, None, None, p, 1 << 20, None) != 0
    assert b"mvf_mesh_loss" in lib.mvf_last_error()


# ---- the whole class ----
class _Slice:
    def __init__(self, xy):
        self.obsm = {"spatial": np.array(xy)}


def _model(case, **kw):
    import spateo_amd as st

    args = dict(max_rotation_angle=16, max_translation_scale=0.1, max_scaling=1.2, min_rotation_angle=2, min_translation_scale=0.01,
                min_scaling=1.02, label_num=5, max_iter=3, anneal_rate=0.5)
    args.update(kw)
    return st.align.Mesh_correction([_Slice(c) for c in case["contours"]], HEIGHTS, (case["verts"], case["tri"]),
                                    contours=case["contours"], **args)


def test_whole_run_equals_the_restatement(case):
    """label_num = 5, max_iter = 3 on slices cut from a known rigid transform of the mesh: the same host loop once on the device
    and once with the restated loss in its place - the chosen labels are equal, the losses within the float64 bound -, and the
    search finds something better than the identity."""
    gpu = _model(case)
    gpu.run_discrete_optimization()
    cpu = _model(case)
    # (the mesh as the model holds it after set_init_parameters, and its own mean: what the device path reads)
    cpu._evaluate = lambda P: ic.mesh_loss(cpu.mesh.points, cpu.mesh.edges, cpu.mesh.points.mean(axis=0), P, cpu.z_heights_subsample,
                                           cpu.contours_subsample)[0]
    cpu.run_discrete_optimization()
    print("losses", gpu.losses, "labels", [l.tolist() for l in gpu.labels], "best", gpu.best_transformation)
    assert len(gpu.losses) == 4 and gpu.losses[0] == 1e8 and len(gpu.transformations) == 4
    assert all(np.array_equal(a, b) for a, b in zip(gpu.labels, cpu.labels))
    assert (np.abs(np.array(gpu.losses[1:]) - np.array(cpu.losses[1:])) <= _loss_bound(np.array(cpu.losses[1:]), 4)).all()
    identity = ic.mesh_loss(case["verts"], case["edges"], case["mean"], IDENTITY, HEIGHTS, case["contours"])[0][0]
    assert gpu.best_loss == min(gpu.losses) < identity
    assert gpu.binaries.dtype == np.float32 and gpu.binaries.shape == (10, 5, 5)
    sub = _model(case, subsample_slices=np.array([2, 0]), max_iter=1)     # an index array is the draw
    sub.run_discrete_optimization()
    assert len(sub.contours_subsample) == 2 and np.array_equal(sub.z_heights_subsample, HEIGHTS[[2, 0]])


def test_perform_correction_carries_a_shifted_slice_back(case):
    """Slices whose contours are the mesh's own cut points with noise sigma = 0.02, each then moved by a small rigid motion of
    its own: after the correction every cell is back within 4 sigma of where it was (the rigid fit of ~30 noisy points errs by
    about sigma / sqrt(30) per parameter; 4 sigma leaves room for the lever arm of the rotation error)."""
    import spateo_amd as st

    sigma = 0.02
    rng = np.random.default_rng(31)
    clean = ic.mesh_contours(case["verts"], case["edges"], case["mean"], IDENTITY, HEIGHTS)
    truth, moved = [], []
    for s, c in enumerate(clean):
        c = c + rng.standard_normal(c.shape) * sigma
        a = np.deg2rad([1.5, -2.0, 0.8, -1.0][s])
        R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        ctr = c.mean(0)
        truth.append(c)
        moved.append((c - ctr) @ R.T + ctr + [(0.6, -0.4), (-0.5, 0.5), (0.3, 0.7), (-0.8, -0.2)][s])
    model = st.align.Mesh_correction([_Slice(m) for m in moved], HEIGHTS, (case["verts"], case["tri"]), contours=moved)
    model.best_transformation = {"rotation": np.zeros(3), "translation": 0.0, "scaling": 1.0}
    out = model.perform_correction()
    assert len(model.rotations) == len(model.translations) == 4
    for s, sl in enumerate(out):
        err = np.abs(sl.obsm["align_spatial"] - truth[s]).max()
        before = np.abs(moved[s] - truth[s]).max()
        print(f"slice {s}: off by {before:.3f} before, {err:.4f} after (4 sigma = {4 * sigma})")
        assert err <= 4 * sigma < before
        assert np.allclose(model.rotations[s] @ model.rotations[s].T, np.eye(2), atol=1e-12)
        assert np.array_equal(sl.obsm["align_spatial"], moved[s] @ model.rotations[s].T + model.translations[s])
