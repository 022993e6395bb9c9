"""The NumPy restatements of tests/_graph_cases.py against tests/golden/ref_graph_kernel.npz, on the CPU: what the GPU tests of
the kernel along the tissue rely on.

* the search gives sklearn's neighbour lists (indices equal, distances within D_ULP; the number of unequal entries is printed);
* the union gives the edge set of the reference's ``construct_knn_graph``, a neighbour at distance 0 adding no edge;
* the relaxation gives the ``D`` under the reference's ``con_K_graph`` within 2 ulp (expected: bit-equal) and ``K`` within 4 ulp,
  with 1e5 / exactly 0 across components;
* the fixed-point argument: relaxing in three orders - forward, reversed, a new random order per sweep - gives identical bits,
  and those of ``networkx.single_source_dijkstra``."""
import numpy as np
import pytest

import _graph_cases as gc

G = gc.load()
TAGS = gc.graph_tags(G)
_KNN = {}


def _knn(tag):
    if tag not in _KNN:
        _KNN[tag] = gc.knn_restated(G[f"{tag}_points"], int(G[f"{tag}_knn"]))
    return _KNN[tag]


@pytest.mark.parametrize("tag", TAGS)
def test_search_gives_sklearns_neighbours(tag):
    idx, dist = _knn(tag)
    order = np.argsort(idx, axis=1)
    assert np.array_equal(np.take_along_axis(idx, order, 1), G[f"{tag}_nbr_idx"])
    mine = np.take_along_axis(dist, order, 1)
    print(f"{tag}: {int((mine != G[f'{tag}_nbr_dist']).sum())} of {mine.size} distances differ in bits")
    assert gc.ulps(mine, G[f"{tag}_nbr_dist"]) <= gc.D_ULP
    assert (np.diff(dist, axis=1) >= 0).all()


@pytest.mark.parametrize("tag", TAGS)
def test_union_gives_the_reference_edge_set(tag):
    edges = gc.union_restated(*_knn(tag))
    ref = {(int(i), int(j)): float(w) for (i, j), w in zip(G[f"{tag}_edges_ij"], G[f"{tag}_edges_w"])}
    assert edges.keys() == ref.keys()
    assert gc.ulps([edges[e] for e in sorted(ref)], [ref[e] for e in sorted(ref)]) <= gc.D_ULP
    assert all(w > 0 for w in edges.values())
    indptr, indices, weights = gc.csr_of(edges, len(G[f"{tag}_points"]))
    assert gc.edges_of(indptr, indices, weights) == edges and all((np.diff(indices[a:b]) > 0).all() for a, b in zip(indptr, indptr[1:]))


@pytest.mark.parametrize("tag", TAGS)
def test_relaxation_gives_the_reference_distances_and_kernel(tag):
    n = len(G[f"{tag}_points"])
    ref_edges = {(int(i), int(j)): float(w) for (i, j), w in zip(G[f"{tag}_edges_ij"], G[f"{tag}_edges_w"])}
    csr = gc.csr_of(ref_edges, n)   # the reference's own weights, so that D is compared on equal inputs
    src, beta = G[f"{tag}_inducing_idx"], float(G[f"{tag}_beta"])
    runs = {o: gc.relax_restated(*csr, n, src, order=o, seed=7) for o in ("forward", "reversed", "random")}
    D = runs["forward"][0]
    for o in ("reversed", "random"):
        assert np.array_equal(D.view(np.int64), runs[o][0].view(np.int64)), o
    print(f"{tag}: sweeps forward {runs['forward'][1]}, reversed {runs['reversed'][1]}, random {runs['random'][1]}")
    D5 = np.where(np.isinf(D), gc.UNREACHABLE, D)
    print(f"{tag}: {int((D5 != G[f'{tag}_D']).sum())} of {D5.size} distances differ in bits from the reference's")
    assert np.array_equal(np.isinf(D), G[f"{tag}_D"] == gc.UNREACHABLE)
    assert gc.ulps(D5, G[f"{tag}_D"]) <= gc.D_ULP
    K = gc.kernel_restated(D, beta)
    assert gc.ulps(K, G[f"{tag}_K"]) <= gc.K_ULP and np.array_equal(K == 0, G[f"{tag}_K"] == 0)
    for s in (0, len(src) - 1):
        assert np.array_equal(gc.dijkstra(*csr, n, src[s]).view(np.int64), D[:, s].view(np.int64))


@pytest.mark.parametrize("name", ["path", "star", "two components"])
def test_small_graphs_three_orders_and_dijkstra(name):
    indptr, indices, weights, n = {"path": gc.path_graph, "star": gc.star_graph, "two components": gc.two_components}[name]()
    src = np.array([0, n // 2, n - 1, 0])
    runs = [gc.relax_restated(indptr, indices, weights, n, src, order=o, seed=3) for o in ("forward", "reversed", "random")]
    for D, _ in runs[1:]:
        assert np.array_equal(D.view(np.int64), runs[0][0].view(np.int64))
    for s in range(len(src)):
        assert np.array_equal(gc.dijkstra(indptr, indices, weights, n, src[s]).view(np.int64), runs[0][0][:, s].view(np.int64))
    if name == "path":
        assert runs[1][1] >= 150   # against the edges' order the distances travel one node per sweep
    if name == "two components":
        D = runs[0][0]   # node 160 is isolated and is source 2: nothing but itself reaches it
        assert np.isinf(D[160, [0, 1, 3]]).all() and D[160, 2] == 0 and np.isinf(D[:160, 2]).all() and np.isinf(D[100, 0])


def test_the_clouds_restate_to_sorted_lists_without_the_point_itself():
    for name, (X, k) in gc.clouds().items():
        idx, dist = gc.knn_restated(X, k)
        assert (idx != np.arange(len(X))[:, None]).all() and (np.diff(dist, axis=1) >= 0).all(), name
        ties = np.diff(dist, axis=1) == 0
        assert (np.diff(idx, axis=1)[ties] > 0).all(), name


def test_the_loop_cases_hold_what_the_gpu_tests_read():
    import _align_loop_case as lc
    import _align_svi_case as sc

    for tag in gc.loop_tags(G):
        args, kw = lc.case_inputs(G, tag)
        assert np.array_equal(args[0][G[f"{tag}_inducing_idx"]], kw["inducing_variables"]) and float(G[f"{tag}_U_gap"]) >= 0.1
        tol = lc.bounds(G, tag, lc.F64_TOL)
        assert all(np.isfinite(b).all() and (b >= lc.F64_TOL).all() for b in tol.values())
    S = gc.View(G, "svi_")
    for tag in [str(t) for t in S["cases"]]:
        tol = sc.bounds(S, tag, sc.F64_TOL)
        assert all(np.isfinite(b).all() for b in tol.values()) and int(S["iters"]) == len(S[f"{tag}_sigma2"])
