"""``st.tdr`` shape similarity on ``cuda:0`` against the golden (the reference's own outputs on the clouds of
tests/_shape_cases.py): ``subspace_descriptors`` through the public call, ``model_eigenvector`` (weight vector exact, eigenvector
within the ``dist`` bound of the case), ``pairwise_shape_similarity`` within max(1e-4 - the reference's own rounding quantum -,
64 x |score_gelss - score_gelsd|), and ``shape_similarity_matrix`` symmetric, with a unit diagonal and equal to the pairwise calls
bit for bit."""
import numpy as np
import pytest
import torch

import _shape_cases as sc

pytestmark = pytest.mark.gpu

G = sc.load()
DEVICE = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def test_subspace_descriptors_through_the_public_call():
    import spateo_amd as st

    case, r = sc.CASES["A"], sc.restated("A")
    d = st.tdr.subspace_descriptors(case["pcs"], n_subspace=case["n"], device=DEVICE)
    assert {"voxel", "count", "cosine", "dist", "rank", "point_voxel", "n_dropped", "n_overlap"} <= set(d)
    assert np.array_equal(d["point_voxel"], r["point_voxel"]) and np.array_equal(d["voxel"], G["A_cubic_voxel"])
    assert np.array_equal(d["count"], G["A_cubic_count"]) and d["n_dropped"] == r["n_dropped"] > 0 and d["n_overlap"] == 0
    bound, _, keep = sc.dist_bounds(G, "A")
    assert (np.abs(d["dist"] - G["A_cubic_vs"][:, 1]) / G["A_cubic_vs"][:, 1])[keep].max() <= bound
    for order in ("linear", "quadratic"):
        case = sc.CASES["B"]
        d = st.tdr.subspace_descriptors(case["pcs"], n_subspace=case["n"], order=order, device=DEVICE)
        bound, _, keep = sc.dist_bounds(G, "B", order)
        assert (np.abs(d["dist"] - G[f"B_{order}_vs"][:, 1]) / G[f"B_{order}_vs"][:, 1])[keep].max() <= bound
        assert d["rank"].max() == sc.P[order]
    with pytest.raises(ValueError, match="no subspace"):
        st.tdr.subspace_descriptors(np.array([[0.0, 0.0, 0.0], [1.5, 1.5, 1.5], [4.0, 4.0, 4.0]]), n_subspace=4, device=DEVICE)


@pytest.mark.parametrize("name", sc.END_TO_END)
def test_model_eigenvector(name):
    import spateo_amd as st

    case = sc.CASES[name]
    e, w = st.tdr.model_eigenvector(case["pcs"], n_subspace=case["n"], m=sc.M, s=sc.S, device=DEVICE)
    e_ref, w_ref = G[f"{name}_cubic_e"], G[f"{name}_cubic_w"]
    assert e.shape == w.shape == (sc.M * sc.S,) and np.array_equal(w, w_ref)
    bound, _, _ = sc.dist_bounds(G, name)
    nz = e_ref != 0
    assert np.array_equal(e != 0, nz)
    dev = float((np.abs(e[nz] - e_ref[nz]) / e_ref[nz]).max())
    print(f"model_eigenvector {name}: {int(nz.sum())} entries, largest relative deviation {dev:.3e} (bound {bound:.3e})")
    assert dev <= bound


@pytest.mark.parametrize("a,b", sc.PAIRS)
def test_pairwise_shape_similarity(a, b):
    import spateo_amd as st

    n = sc.CASES[a]["n"]
    assert sc.CASES[b]["n"] == n
    got = st.tdr.pairwise_shape_similarity(sc.CASES[a]["pcs"], sc.CASES[b]["pcs"], n_subspace=n, m=sc.M, s=sc.S, device=DEVICE)
    want, swapped = float(G[f"score_{a}_{b}"]), float(G[f"score_gelss_{a}_{b}"])
    bound = max(1e-4, sc.ALLOW * abs(swapped - want))
    print(f"pairwise_shape_similarity {a}-{b}: {got} (reference {want}, under gelss {swapped}, bound {bound:.1e})")
    assert isinstance(got, float) and got == round(got, 4)
    assert round(abs(got - want), 8) <= bound          # (both are multiples of 1e-4: their difference is one to rounding)


def test_shape_similarity_matrix():
    import spateo_amd as st

    models = [sc.CASES["A"]["pcs"], sc.CASES["B"]["pcs"], sc.CASES["C"]["pcs"] * 10.0]
    mat = st.tdr.shape_similarity_matrix(models, n_subspace=4, device=DEVICE)
    assert mat.shape == (3, 3) and np.array_equal(mat, mat.T) and np.array_equal(np.diag(mat), np.ones(3))
    for i in range(3):
        for j in range(i + 1, 3):
            assert mat[i, j] == st.tdr.pairwise_shape_similarity(models[i], models[j], n_subspace=4, device=DEVICE)
    assert np.isfinite(mat).all() and (mat > 0).all()
    assert np.array_equal(mat, st.tdr.shape_similarity_matrix(models, n_subspace=4, device=DEVICE))
