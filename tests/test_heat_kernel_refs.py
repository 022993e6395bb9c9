"""CPU: the restatements of tests/_heat_cases.py against the real reference functions (tests/golden/ref_digitize.npz, written by
tests/golden/make_golden_digitize.py from ``spateo/digitization/utils.py`` and ``grid.py``), and the host functions of
``spateo_amd.dd`` against their goldens.

Grid: the restatement meets the real ``domain_heat_eqn_solver`` bit for bit, in field and sweep count - which also settles the
denominator of ``effective_L2_error`` (the OLD field).  Graph: the real ``digitize_general`` multiplies by a dense matrix with
BLAS, whose order of additions is its own; the sweep counts are equal and the field lies within ALLOW x max(dev, eps) of the
restatement, relative to the largest heat, with dev the deviation the golden recorded where it was made."""
import numpy as np
import pytest

import _heat_cases as hc

ALLOW = 64.0
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def G():
    return hc.load()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("name", hc.GRID_NAMES)
def test_grid_case_is_decidable(name):
    _, itr, errs = hc.grid_reference(name)
    assert len(errs) == itr
    hc.assert_decidable(hc.grid_case(name), errs)


@pytest.mark.parametrize("name", hc.GRAPH_NAMES)
def test_graph_case_is_decidable(name):
    _, itr, errs = hc.graph_reference(name)
    assert len(errs) == itr
    hc.assert_decidable(hc.graph_case(name), errs)


def test_decidable_bites():
    with pytest.raises(AssertionError):
        hc.assert_decidable(dict(max_err=1e-5), [1e-3, 1e-5 * (1 + 5e-10)])
    hc.assert_decidable(dict(max_err=1e-5), [1e-3, 1e-5 * (1 + 5e-9), float("nan")])


def test_case_list_covers_what_it_claims():
    hc.assert_stop_positions_cover_a_batch()
    for name, sweeps in hc.BUDGET_CASES.items():
        assert hc.grid_reference(name)[1] == sweeps, name
    assert np.isnan(hc.grid_reference("all_zero")[2][-1]) and hc.grid_reference("all_zero")[1] == 1
    assert np.isnan(hc.graph_reference("empty_both")[2][-1]) and hc.graph_reference("empty_both")[1] == 1
    for name in ("rect_12x15", "rect_20x27", "rect_40x70", "l_shape", "ring"):      # the default max_err ends at a fixed point
        assert hc.grid_reference(name)[2][-1] == 0.0, name
    assert set(np.unique(hc.grid_case("mask_2_and_3")["mask"])) == {0.0, 2.0, 3.0}
    leak = hc.grid_reference("open_border")[0]          # (the masked result hides the leak; the unmasked field shows it)
    f, _, _ = hc.grid_loop(hc.grid_case("open_border"))
    assert leak.shape == f.shape and (f[:, 27:29] > 0).any()
    lh0 = hc.graph_case("lh0")
    assert not np.array_equal(hc.graph_reference("lh0")[0][lh0["lower"]], np.zeros(len(lh0["lower"])))  # heat 0 is not held
    deg = np.diff(hc.graph_csc(hc.graph_case("hub"))[0])
    assert deg.max() == 300 and deg.min() == 1
    assert np.diff(hc.graph_csc(hc.graph_case("isolated"))[0])[17] == 0
    sl = hc.graph_case("self_loop")["adj"]
    assert sl[21, 21] == 0.5
    sizes = {(hc.grid_case(n)["mask"].shape) for n in hc.GRID_NAMES if n.startswith("edge_")}
    assert sizes == {(hc.TILE_H + a, hc.TILE_W + a) for a in (-1, 0, 1, hc.T - 1, hc.T, hc.T + 1)}


@pytest.mark.parametrize("name", hc.GRID_NAMES)
def test_grid_restatement_is_the_reference_bit_for_bit(G, name):
    out, itr, _ = hc.grid_reference(name)
    assert itr == int(G[f"grid_{name}_itr"])
    assert same_bits(out, G[f"grid_{name}_out"])


@pytest.mark.parametrize("name", hc.GRAPH_NAMES)
def test_graph_restatement_meets_the_reference(G, name):
    out, itr, _ = hc.graph_reference(name)
    assert itr == int(G[f"graph_{name}_itr"])
    for part, got in zip(("indptr", "indices", "data"), hc.graph_csc(hc.graph_case(name))):
        assert np.array_equal(got, G[f"graph_{name}_{part}"]), (name, part)      # the same graph as where the golden was made
    ref = G[f"graph_{name}_out"]
    scale = max(np.abs(ref).max(), np.finfo(np.float64).tiny)
    bound = ALLOW * max(float(G[f"dev_{name}"]), EPS)
    assert np.abs(out - ref).max() / scale <= bound


# ------------------------------------------------------------------------------------------------------ host functions
CORNERS_RECT = dict(pnt_xy=(3, 2), pnt_Xy=(14, 2), pnt_xY=(3, 9), pnt_XY=(14, 9))


@pytest.mark.parametrize("cname", ("rect", "rect_shifted", "l"))
def test_field_contours(G, cname):
    from spateo_amd import dd

    chain, corners = {"rect": (hc.chain_rect(2, 9, 3, 14), CORNERS_RECT),
                      "rect_shifted": (np.roll(hc.chain_rect(2, 9, 3, 14), 11, axis=0), CORNERS_RECT),
                      "l": (hc.chain_l(), hc.L_CORNERS)}[cname]
    lines = dd.field_contours(chain, **corners)
    for lname, line in zip(("min_l", "max_l", "min_c", "max_c"), lines):
        assert np.array_equal(np.array(line, dtype=np.int64), G[f"contours_{cname}_{lname}"]), lname
    assert all(isinstance(p, tuple) for p in lines[0])
    lines2 = dd.field_contours(chain[:, 0], **corners)          # (n, 2) is taken too
    assert [list(l) for l in lines2] == [list(l) for l in lines]
    with pytest.raises(ValueError):
        dd.field_contours(chain, **dict(corners, pnt_xy=(0, 0)))   # a corner that is no point of the contour


def test_field_contours_on_random_corners_and_a_chain_that_repeats_pixels(G):
    from spateo_amd import dd

    probes = hc.contour_probes()
    assert len(probes) == 16
    lengths = set()
    for i, (chain, corners) in enumerate(probes):
        lines = dd.field_contours(chain, *corners)
        for lname, line in zip(("min_l", "max_l", "min_c", "max_c"), lines):
            assert np.array_equal(np.array(line, dtype=np.int64).reshape(-1, 2), G[f"contours_probe{i}_{lname}"]), (i, lname)
            lengths.add(len(line) > len(chain) // 2)
    assert lengths == {True, False}


def test_boundary_writers_and_the_error(G):
    from spateo_amd import dd

    f = np.zeros((6, 9))
    dd.add_eh_boundary(f, [(1, 1), (2, 1), (3, 1)], 7.0)
    dd.add_gh_boundary(f, [(1, 2), (1, 3), (2, 4), (3, 4), (4, 4), (5, 5), (6, 5)], 1.0, 100.0)
    assert same_bits(f, G["gh_field"])
    a, b, m = np.arange(12.0).reshape(3, 4), np.arange(12.0).reshape(3, 4)[::-1] * 0.5 + 1, np.array([[1.0, 2, 0, 1]] * 3)
    assert dd.effective_L2_error(a, b, m) == float(G["l2_error"])
    assert dd.effective_L2_error(a, b, m) != dd.effective_L2_error(b, a, m)    # normalised by the second argument


def test_gridit(G):
    from spateo_amd import AnnDataLite, dd

    for tag, kw in (("gridit", dict(layer_num=3, column_num=4)),
                    ("gridit2", dict(layer_num=5, column_num=2, lh=0, hh=110, layer_border_width=6, column_border_width=1))):
        adata = AnnDataLite(obs={"digital_layer": G["gridit_layer"], "digital_column": G["gridit_column"]}, n_obs=60)
        assert dd.gridit(adata, **kw) is None
        assert np.array_equal(adata.obs["layer_label"], G[f"{tag}_layer_label"])
        assert np.array_equal(adata.obs["column_label"], G[f"{tag}_column_label"])
        assert np.array_equal(np.asarray(adata.obs["grid_label"]).astype(str), G[f"{tag}_grid_label"])
        assert set(G[f"{tag}_grid_label"]) == {"NA", "Grid Area", "Region Boundary"}
    adata = AnnDataLite(obs={"L": G["gridit_layer"], "C": G["gridit_column"]}, n_obs=60)
    dd.gridit(adata, 3, 4, dgl_layer_key="L", dgl_column_key="C", layer_label_key="a", column_label_key="b", grid_label_key="c")
    assert np.array_equal(adata.obs["a"], G["gridit_layer_label"]) and np.array_equal(adata.obs["b"], G["gridit_column_label"])
    assert np.array_equal(np.asarray(adata.obs["c"]).astype(str), G["gridit_grid_label"])
