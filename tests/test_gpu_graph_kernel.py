"""The kernel along the tissue through the API on ``cuda:0`` against tests/golden/ref_graph_kernel.npz (the real
``construct_knn_graph`` / ``con_K_graph`` and the real loop methods on the geodesic kernel; tests/golden/make_golden_graph_kernel.py).

* ``knn`` / ``construct_knn_graph``: sklearn's neighbour lists and the reference's edge set, weights within 2 ulp;
* ``graph_distances`` / ``con_K_graph`` / ``graph_kernel``: ``D`` within 2 ulp (expected bit-equal; the number of unequal entries is
  printed), ``K`` within 4 ulp, 1e5 / exactly 0 across components, ``Gamma = U[inducing_idx]``; a ``networkx.Graph`` input gives the
  ``K`` of the ``KnnGraph`` it came from, bit for bit;
* ``morpho_iterate(graph_kernel=)`` and ``morpho_iterate_svi(graph_kernel=)`` against the golden loops in both cell dtypes with
  exactly the criterion of the Euclidean loop tests: the bounds ``tests/_align_loop_case.py`` / ``_align_svi_case.py`` compute from
  the stored floors and gains (float64 ``1e-10 max(1, 1.25 g_k)``; float32 ``max(1.25 x the reference's own float32 floor, 1e-5
  max(1, 1.25 g_k))``, ``Coff`` in float64 only).  No constant here is fitted to a GPU result;
* ``update_nonrigid(graph_kernel=)`` against the first non-rigid step of the golden loop ``L3`` (iteration 3, a stored one) with
  that iteration's bound of ``VnA`` / ``Coff``; ``SigmaDiag`` is a quadratic form in the same ``pinv(SigmaInv)`` as ``Coff`` and
  takes ``Coff``'s bound;
* with ``graph_kernel=None`` a small existing case gives the bits of a call without the argument; the geodesic result differs
  from the Euclidean one (the kernels differ by up to 0.47 in an entry), and ``BA_transform`` refuses its ``vecfld``."""
import numpy as np
import pytest

import _align_loop_case as lc
import _align_svi_case as sc
import _graph_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = gc.load()
S = gc.View(G, "svi_")
_KERNELS, _RUNS = {}, {}


def _align():
    from spateo_amd import align

    return align


def _gk(tag):
    if tag not in _KERNELS:
        _KERNELS[tag] = _align().graph_kernel(G[f"{tag}_coordsA"], G[f"{tag}_inducing_idx"], float(G[f"{tag}_beta"]),
                                               graph_knn=int(G[f"{tag}_graph_knn"]), device=DEV)
    return _KERNELS[tag]


@pytest.mark.parametrize("tag", gc.graph_tags(G))
def test_graph_and_kernel_against_the_reference(tag):
    align = _align()
    X, knn, src, beta = G[f"{tag}_points"], int(G[f"{tag}_knn"]), G[f"{tag}_inducing_idx"], float(G[f"{tag}_beta"])
    idx, dist = align.knn(X, knn, device=DEV)
    order = np.argsort(idx, axis=1)
    assert np.array_equal(np.take_along_axis(idx, order, 1), G[f"{tag}_nbr_idx"])
    graph = align.construct_knn_graph(X, knn, device=DEV)
    indptr, indices, weights = graph.host_arrays()
    edges = gc.edges_of(indptr, indices, weights)
    ref = {(int(i), int(j)): float(w) for (i, j), w in zip(G[f"{tag}_edges_ij"], G[f"{tag}_edges_w"])}
    assert edges.keys() == ref.keys() and graph.n == len(X) and graph.n_edges == len(ref)
    assert gc.ulps([edges[e] for e in sorted(ref)], [ref[e] for e in sorted(ref)]) <= gc.D_ULP
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and all((np.diff(indices[a:b]) > 0).all() for a, b in zip(indptr, indptr[1:]))
    D = align.graph_distances(graph, src, device=DEV)
    print(f"{tag}: {int((D != G[f'{tag}_D']).sum())} of {D.size} distances differ in bits from the reference's")
    assert np.array_equal(D == gc.UNREACHABLE, G[f"{tag}_D"] == gc.UNREACHABLE) and gc.ulps(D, G[f"{tag}_D"]) <= gc.D_ULP
    K = align.con_K_graph(graph, src, beta=beta, device=DEV)
    assert gc.ulps(K, G[f"{tag}_K"]) <= gc.K_ULP and np.array_equal(K == 0, G[f"{tag}_K"] == 0)
    # a networkx.Graph gives the same K as the KnnGraph it came from
    Kx = align.con_K_graph(graph.to_networkx(), src, beta=beta, device=DEV)
    assert np.array_equal(K.view(np.int64), Kx.view(np.int64))
    gk = align.graph_kernel(X, src, beta, graph_knn=knn, device=DEV)
    assert np.array_equal(gk.U.view(np.int64), K.view(np.int64)) and np.array_equal(gk.Gamma, K[src]) and np.array_equal(gk.inducing_variables, X[src])
    assert gk.n_unreachable == int((G[f"{tag}_D"] == gc.UNREACHABLE).any(1).sum()) and gk.beta == beta


def test_isolated_node_and_seeded_draw():
    align = _align()
    X = np.random.default_rng(4).random((60, 2))
    g = align.construct_knn_graph(X, 4, device=DEV).to_networkx()
    g.remove_edges_from(list(g.edges(7)))                      # node 7 without any edge: kept, isolated
    gk = align.graph_kernel(X, np.array([7, 3]), 0.5, graph=g, device=DEV)
    assert gk.U[7, 0] == 1.0 and (np.delete(gk.U[:, 0], 7) == 0).all() and gk.U[7, 1] == 0 and gk.n_unreachable == 60
    a, b = (align.graph_kernel(X, 9, 0.5, graph_knn=4, seed=11, device=DEV) for _ in range(2))
    assert np.array_equal(a.inducing_idx, b.inducing_idx) and len(set(a.inducing_idx.tolist())) == 9 and np.array_equal(a.U, b.U)


def _loop(tag, dtype):
    if (tag, dtype) not in _RUNS:
        args, kw = lc.case_inputs(G, tag)
        _RUNS[(tag, dtype)] = _align().morpho_iterate(*args, dtype=dtype, device=DEV, record="arrays", kernel_type="geodist",
                                                      graph_kernel=_gk(tag), **kw)
    return _RUNS[(tag, dtype)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tag", gc.loop_tags(G))
def test_loop_on_the_geodesic_kernel_against_the_reference(tag, dtype):
    gk = _gk(tag)
    assert gc.ulps(gk.U[::16], G[f"{tag}_U_sample"]) <= gc.K_ULP and np.array_equal(gk.inducing_variables, G[f"{tag}_inducing_variables"])
    out = _loop(tag, dtype)
    got = dict(out["history"], optimal_R=out["optimal_R"], optimal_t=out["optimal_t"])
    f32 = dtype == "float32"
    tol = lc.bounds(G, tag, lc.F32_BASE if f32 else lc.F64_TOL, f32=f32, skip=("Coff",) if f32 else ())
    ratio = lc.check(lc.deviations(got, G, tag), tol, f"geodist case {tag} {dtype}")
    assert max(ratio.values()) <= 1.0
    assert out["vecfld"]["kernel_type"] == "geodist" and np.array_equal(out["XAHat"], out["history"]["XAHat"][-1])
    with pytest.raises(ValueError, match="geodist"):
        _align().BA_transform(out["vecfld"], G[f"{tag}_coordsA"], device=DEV)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tag", [str(t) for t in S["cases"]])
def test_svi_loop_on_the_geodesic_kernel_against_the_reference(tag, dtype):
    args, kw = lc.case_inputs(G, tag)
    kw.update(max_iter=int(S["iters"]), batch_size=int(S["batch_size"]), batch_perm=S[f"{tag}_batch_perm"].astype(np.int64))
    out = _align().morpho_iterate_svi(*args, dtype=dtype, device=DEV, record="arrays", kernel_type="geodist", graph_kernel=_gk(tag), **kw)
    got = dict(out["history"], optimal_R=out["optimal_R"], optimal_t=out["optimal_t"])
    f32 = dtype == "float32"
    tol = sc.bounds(S, tag, sc.F32_BASE if f32 else sc.F64_TOL, f32=f32, skip=("Coff",) if f32 else ())
    ratio = sc.check(sc.deviations(got, S, tag), tol, f"geodist SVI case {tag} {dtype}")
    assert max(ratio.values()) <= 1.0
    np.testing.assert_array_equal(out["history"]["step_size"], S[f"{tag}_step_size"])
    assert out["vecfld"]["kernel_type"] == "geodist"


def test_update_nonrigid_on_the_geodesic_kernel_is_the_loops_first_step():
    tag, gk = "L3", _gk("L3")
    _, kw = lc.case_inputs(G, tag)
    first = {q: G[f"{tag}_first_{q}"] for q in ("sigma2", "K_NA", "PXB_term", "Coff", "VnA", "SigmaDiag")}
    out = _align().update_nonrigid(G[f"{tag}_coordsA"], gk.inducing_variables, kw["beta"], first["K_NA"], first["PXB_term"],
                                   float(first["sigma2"]), kw["lambdaVF"], dtype="float64", device=DEV, kernel_type="geodist",
                                   graph_kernel=gk)
    tol = lc.bounds(G, tag, lc.F64_TOL)
    at = [int(i) for i in G["arr_iters"]].index(int(G[f"{tag}_nonrigid_start_iter"]) + 1)
    for q, bound in (("Coff", tol["Coff"][at]), ("VnA", tol["VnA"][at]), ("SigmaDiag", tol["Coff"][at])):
        dev = float(lc.rel(out[q][None], first[q][None])[0])
        print(f"update_nonrigid(graph_kernel=) {q}: {dev:.3g} (bound {bound:.3g})")
        assert dev <= bound, q
    assert np.array_equal(first["Coff"], G[f"{tag}_Coff"][at])   # (the step the maker captured is the stored iteration)


def test_without_graph_kernel_the_bits_are_unchanged_and_the_kernels_differ():
    D = lc.load()
    args, kw = lc.case_inputs(D, "3")
    kw["max_iter"] = 5
    a = _align().morpho_iterate(*args, dtype="float64", device=DEV, **kw)
    b = _align().morpho_iterate(*args, dtype="float64", device=DEV, graph_kernel=None, **kw)
    for q in ("XAHat", "VnA", "Coff", "SigmaDiag", "alpha", "R", "t", "K_NA"):
        assert np.array_equal(np.asarray(a[q]).view(np.int64), np.asarray(b[q]).view(np.int64)), q
    assert a["sigma2"] == b["sigma2"] and a["vecfld"]["kernel_type"] == "euc"
    # the geodesic loop is not the Euclidean one: the same case and inducing variables, the other kernel
    args, kw = lc.case_inputs(G, "L3")
    euc = _align().morpho_iterate(*args, dtype="float64", device=DEV, record=False, **kw)
    geo = _loop("L3", "float64")
    assert np.abs(euc["VnA"] - geo["VnA"]).max() > 1e-3 * np.abs(geo["VnA"]).max()
