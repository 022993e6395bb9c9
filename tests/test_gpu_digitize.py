"""GPU: the public ``st.dd`` functions end to end on the device against tests/golden/ref_digitize.npz (the real reference
solver on the same rasters) and the restatements of tests/_heat_cases.py."""
import numpy as np
import pytest

import _heat_cases as hc
from _kernel_scaffold import DEV, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return hc.load()


def test_digitize_on_an_l_shaped_slice_and_gridit_on_top(G):
    import spateo_amd as st

    adata = st.AnnDataLite(obsm={"spatial": hc.l_slice_cells()})
    assert st.dd.digitize(adata, (hc.chain_l(),), 0, **hc.L_CORNERS, device=DEV) is None
    assert same_bits(np.asarray(adata.obs["digital_layer"]), G["digitize_layer"])
    assert same_bits(np.asarray(adata.obs["digital_column"]), G["digitize_column"])
    st.dd.gridit(adata, layer_num=4, column_num=5)
    assert np.array_equal(adata.obs["layer_label"], G["digitize_layer_label"])
    assert np.array_equal(adata.obs["column_label"], G["digitize_column_label"])
    assert np.array_equal(np.asarray(adata.obs["grid_label"]).astype(str), G["digitize_grid_label"])
    # the whole fields, with the sweep counts of the real solver
    border, mask = st.dd.rasterize_contour(hc.chain_l(), (40, 70))
    min_l, max_l, min_c, max_c = st.dd.field_contours(hc.chain_l(), **hc.L_CORNERS)
    layer, info = st.dd.domain_heat_eqn_solver(np.zeros((40, 70)), min_l, max_l, min_c, max_c, border, mask, device=DEV, return_info=True)
    assert same_bits(layer, G["digitize_layer_field"])
    assert info == dict(iterations=int(G["digitize_sweeps"][0]), err=0.0, hit_max_itr=False)
    column, info = st.dd.domain_heat_eqn_solver(np.zeros((40, 70)), min_c, max_c, min_l, max_l, border, mask, device=DEV, return_info=True)
    assert same_bits(column, G["digitize_column_field"]) and info["iterations"] == int(G["digitize_sweeps"][1])


def test_domain_solver_return_info(G):
    import spateo_amd as st

    for name, hit in (("budget_5", True), ("stop_1e-8", False), ("all_zero", False), ("no_sweep", True)):
        c = hc.grid_case(name)
        out, info = st.dd.domain_heat_eqn_solver(c["heat_field"], c["min_line"], c["max_line"], c["edge_a"], c["edge_b"], c["border"],
                                                 c["mask"], max_err=c["max_err"], max_itr=c["max_itr"], lh=c["lh"], hh=c["hh"],
                                                 return_info=True)
        assert same_bits(out, G[f"grid_{name}_out"]) and info["iterations"] == int(G[f"grid_{name}_itr"])
        assert info["hit_max_itr"] is hit and isinstance(info["err"], float)
    assert info["err"] == 1.0       # no sweep ran: the reference's starting err


@pytest.mark.parametrize("name", ("cloud257_k6", "cloud1000_k8", "hub", "lh0"))
def test_digitize_general_dense_csr_csc_give_the_same_bits(G, name):
    import scipy.sparse as sp

    import spateo_amd as st

    c = hc.graph_case(name)
    ref, itr, errs = hc.graph_reference(name)
    outs = []
    for adj in (c["adj"].toarray(), sp.csr_matrix(c["adj"]), sp.csc_matrix(c["adj"])):
        out, info = st.dd.digitize_general(c["pc"], adj, c["lower"], c["upper"], max_itr=c["max_itr"], lh=c["lh"], hh=c["hh"],
                                           device=DEV, return_info=True)
        outs.append(out)
        assert info["iterations"] == itr == int(G[f"graph_{name}_itr"]) and info["hit_max_itr"] is False
        assert abs(info["err"] - errs[-1]) <= 1e-12 * errs[-1]
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2]) and same_bits(outs[0], np.asarray(ref))
    gold = G[f"graph_{name}_out"]
    assert np.abs(outs[0] - gold).max() / np.abs(gold).max() <= 64 * max(float(G[f"dev_{name}"]), np.finfo(np.float64).eps)
    plain = st.dd.digitize_general(c["pc"], c["adj"], c["lower"], c["upper"], lh=c["lh"], hh=c["hh"], device=DEV)
    assert isinstance(plain, np.ndarray) and same_bits(plain, outs[0])


def test_digitize_general_budget_and_max_err():
    import spateo_amd as st

    c = hc.graph_case("graph_budget_3")
    ref, itr, errs = hc.graph_reference("graph_budget_3")
    out, info = st.dd.digitize_general(c["pc"], c["adj"], c["lower"], c["upper"], max_itr=3, device=DEV, return_info=True)
    assert info["iterations"] == itr == 4 and info["hit_max_itr"] is True and same_bits(out, np.asarray(ref))
    loose = dict(hc.graph_case("n65"), max_err=1e-2)
    f, n, _ = hc.graph_loop(loose)
    out, info = st.dd.digitize_general(loose["pc"], loose["adj"], loose["lower"], loose["upper"], max_err=1e-2, device=DEV,
                                       return_info=True)
    assert info["iterations"] == n < hc.graph_reference("n65")[1] and same_bits(out, f)
