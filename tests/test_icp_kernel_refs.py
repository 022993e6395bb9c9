"""CPU proof that the restatements of tests/_icp_cases.py - what the GPU suites compare ``csrc/mvf_icp.hip`` against - equal the
real reference (tests/golden/ref_mesh_correction.npz, written by tests/golden/make_golden_mesh_correction.py from the real
``mesh_correction_utils.py``), and the derivation of the coordinate bound those suites use (printed, and recorded in
profiles/mesh_correction_kernel_edges.md):

  * ``ICP``, both ``allow_rotation`` values: ``gamma`` equal; ``T_contour_2``, the translation (no rotation) and the closing
    ``(R, t)`` (rotation) within 64 x the deviation the restatement itself shows under +-4 ulp perturbations of its inputs;
  * ``_transform_points`` at translation 0: within the same rule;
  * ``_calculate_loss`` / ``_get_binary_values``: equal - the contour counts and every ``gamma`` are, and the sum is taken in the
    same order."""
import numpy as np
import pytest

import _icp_cases as ic


@pytest.fixture(scope="module")
def G():
    return ic.load()


def _tags(G):
    return [str(t) for t in G["icp_tags"]]


def _closing(T, c2):
    """The PRODUCT's closing solve (``_mesh_correction._closing_solve``: what ``st.align.icp`` returns with rotation) on the
    restated T: ``(Rotation, translation)``."""
    from spateo_amd import _mesh_correction as mc

    return mc._closing_solve(T, c2)[:2]


@pytest.mark.parametrize("tag", list("abcdefgh"))
@pytest.mark.parametrize("rot", (0, 1))
def test_icp_restatement_equals_the_reference(G, tag, rot):
    assert tag in _tags(G)
    c1, c2 = G[f"icp_{tag}_c1"], G[f"icp_{tag}_c2"]
    kw = dict(allow_rotation=bool(rot))
    bound, got = ic.icp_bound(c1, c2, **kw)
    mag = float(max(np.abs(c1).max(), np.abs(c2).max()))
    assert got["gamma"] == float(G[f"icp_{tag}_{rot}_gamma"])
    err = float(np.abs(got["T"] - G[f"icp_{tag}_{rot}_T"]).max())
    print(f"ICP case {tag} ({len(c1)}, {len(c2)}) rotation={rot}: rounds {got['iters']}, inliers {got['inliers']}, 4-ulp deviation / "
          f"magnitude = {bound / ic.ALLOW / mag:.3e}, bound = {bound:.3e}, |T - T_ref| = {err:.3e}")
    assert bound < 1e-9 * mag and err <= bound
    if rot:
        R_ref, t_ref = G[f"icp_{tag}_1_R"], G[f"icp_{tag}_1_t"]
        R, t = _closing(got["T"], c2)
        dev = ic.deviation(lambda a, b: np.concatenate([x.reshape(-1) for x in _closing(ic.icp(a, b, **kw)["T"], b)]), (c1, c2), mag)
        rb = ic.ALLOW * max(dev, 2.0 ** -52) * mag
        print(f"    closing solve: det R = {np.linalg.det(R):+.3f}, |R - R_ref| = {np.abs(R - R_ref).max():.3e}, "
              f"|t - t_ref| = {np.abs(t - t_ref).max():.3e} (bound {rb:.3e})")
        assert np.linalg.det(R) > 0 and np.abs(R - R_ref).max() <= rb and np.abs(t - t_ref).max() <= rb
    else:
        assert np.array_equal(G[f"icp_{tag}_0_R"], np.eye(2))
        dev = ic.deviation(lambda a, b: ic.icp(a, b, **kw)["translation"], (c1, c2), mag)
        assert np.abs(got["translation"] - G[f"icp_{tag}_0_t"]).max() <= ic.ALLOW * max(dev, 2.0 ** -52) * mag


def test_golden_cases_cover_what_they_claim(G):
    sizes = {(len(G[f"icp_{t}_c1"]), len(G[f"icp_{t}_c2"])) for t in _tags(G)}
    assert {(500, 500), (65, 64), (40, 63), (7, 2)} <= sizes and max(max(s) for s in sizes) <= 500
    assert any(a > b for a, b in sizes) and any(a < b for a, b in sizes)
    runs = {(t, r): ic.icp(G[f"icp_{t}_c1"], G[f"icp_{t}_c2"], allow_rotation=bool(r)) for t in _tags(G) for r in (0, 1)}
    assert any(v["inliers"] < 3 for v in runs.values())                       # the fewer-than-3-inliers exit
    assert any(v["iters"] < 20 and v["inliers"] >= 3 for v in runs.values())  # stopped by the error test
    assert any(any(d < 0 for d in v["dets"]) for v in runs.values())          # a round that reflects
    for t in _tags(G):   # general position: no two points of a contour coincide
        for c in (G[f"icp_{t}_c1"], G[f"icp_{t}_c2"]):
            assert len(np.unique(c, axis=0)) == len(c)


# The next four tests check the RESTATEMENT'S OWN pieces (block_sum, polar2, thin_rows, cut), which the GPU suites compare the
# kernels against; where the product has a host twin of the piece (``_thin``, ``mesh_edges``) it is held to the same answer.
def test_polar_factor_equals_the_svd():
    rng = np.random.default_rng(2)
    seen = set()
    for _ in range(200):
        H = rng.standard_normal((2, 2))
        U, _, Vt = np.linalg.svd(H)
        R = ic.polar2(H.reshape(-1))
        assert np.abs(R - Vt.T @ U.T).max() < 1e-12 and abs(abs(np.linalg.det(R)) - 1) < 1e-12
        seen.add(np.linalg.det(H) > 0)
    assert seen == {True, False}


def test_block_sum_is_a_sum_in_a_fixed_order():
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 255, 256, 257, 500, 512):
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
        s = ic.block_sum(v)
        assert abs(s - np.sum(v)) <= 64 * 2.0 ** -52 * np.abs(v).sum() and s == ic.block_sum(v.copy())
    assert ic.block_sum(np.arange(512.0)) == 511 * 256.0


def test_thinning_rule():
    assert np.array_equal(ic.thin_rows(7, 500), np.arange(7)) and np.array_equal(ic.thin_rows(500, 500), np.arange(500))
    r = ic.thin_rows(1203, 500)
    assert len(r) == 500 and r[0] == 0 and r[-1] == (499 * 1203) // 500 and (np.diff(r) >= 2).all()
    assert np.array_equal(ic.thin_rows(501, 500)[:3], [0, 1, 2]) and ic.thin_rows(501, 500)[-1] == 499
    assert np.array_equal(ic.thin_rows(9, 0), np.arange(9))
    from spateo_amd import _mesh_correction as mc

    for n, sub in ((7, 500), (500, 500), (501, 500), (1203, 500), (300, 64), (9, 0)):   # the product's host twin of the rule
        c = np.arange(2.0 * n).reshape(n, 2)
        assert np.array_equal(mc._thin(c, sub), c[ic.thin_rows(n, sub)])


def test_transform_restatement_equals_the_reference_at_translation_zero(G):
    from spateo_amd import _mesh_correction as mc

    verts = G["mesh_points"]
    mag = float(np.abs(verts).max())
    for p, want in zip(G["tf_params"], G["tf_points"]):
        got = ic.transform(verts, verts.mean(0), p)
        dev = ic.deviation(lambda v, q: ic.transform(v, v.mean(0), q), (verts, p), mag)
        bound = ic.ALLOW * max(dev, 2.0 ** -52) * mag
        err = float(np.abs(got - want).max())
        print(f"transform {p}: 4-ulp deviation / magnitude = {dev:.3e}, bound = {bound:.3e}, |P - P_ref| = {err:.3e}")
        assert err <= bound < 1e-9
        assert np.abs(mc._transform_points(verts, p[:3], p[3], p[4]) - want).max() <= bound
    # the z translation: every vertex moves by it, in z alone
    base = mc._transform_points(verts, [3.0, 4.0, 5.0], 0.0, 1.2)
    assert np.allclose(mc._transform_points(verts, [3.0, 4.0, 5.0], 2.5, 1.2) - base, [0.0, 0.0, 2.5], atol=1e-12, rtol=0)
    assert np.allclose(ic.transform(verts, verts.mean(0), [3.0, 4.0, 5.0, 2.5, 1.2]) - base, [0.0, 0.0, 2.5], atol=1e-12, rtol=0)


def _loss_case(G):
    verts, tri = G["mesh_points"], G["mesh_triangles"]
    contours = np.split(G["loss_contours"], np.cumsum(G["loss_sizes"])[:-1])
    return verts, ic.unique_edges(tri), contours, G["loss_heights"]


def test_loss_restatement_equals_the_reference(G):
    verts, edges, contours, heights = _loss_case(G)
    loss, gamma, count = ic.mesh_loss(verts, edges, verts.mean(0), G["loss_params"], heights, contours)
    print("loss", loss, "reference", G["loss_values"], "counts", count.tolist())
    assert np.array_equal(loss, G["loss_values"])
    assert (count[3] == 0).any() and loss[3] == 1e6 / len(heights) and (count[[0, 1, 2, 4]] > 0).all()


def test_binary_tables_equal_the_reference(G):
    from spateo_amd import _mesh_correction as mc

    verts, edges, contours, heights = _loss_case(G)
    for p in ((0, 3), (2, 4)):
        sets = mc._get_parameters_from_pair(np.array(p), G["bin_labels"]).reshape(9, 5)
        loss, _, _ = ic.mesh_loss(verts, edges, verts.mean(0), sets, heights, contours)
        assert np.array_equal(loss.astype(np.float32).reshape(3, 3), G[f"bin_{p[0]}{p[1]}"])


def test_cut_follows_the_contour_rule():
    """A vertex exactly on the plane counts as above it: its edges to vertices below cross, those to vertices above do not."""
    P = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 2.0], [1.0, 1.0, 1.0]])
    edges = np.array([[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]], dtype=np.int32)
    c = ic.cut(P, edges, 1.0)
    assert np.array_equal(c, [[0.0, 0.0], [0.5, 0.5], [1.0, 1.0]])       # edges 0-1, 1-2, 1-3; not 0-2, 0-3 (on / above), 2-3
    assert len(ic.cut(P, edges, 2.5)) == 0 and len(ic.cut(P, edges, 0.0)) == 0 and len(ic.cut(P, edges, 2.0)) == 3
    from spateo_amd import _mesh_correction as mc

    tri = np.array([[0, 1, 2], [1, 3, 2], [0, 3, 1], [0, 2, 3]])        # the tetrahedron whose edges these are: the order of the cut
    assert np.array_equal(mc.mesh_edges(tri), edges) and np.array_equal(ic.unique_edges(tri), edges)
