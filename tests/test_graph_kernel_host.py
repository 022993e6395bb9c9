"""Host logic of the kernel along the tissue (no device needed): the public names, the refusals of ``graph_kernel=`` that do not
fit the call, and what stays pinned - ``kernel_type="geodist"`` without ``graph_kernel=`` is still ``NotImplementedError``, now
naming the way in; ``mvf_version() == 7``."""
import os
import re

import numpy as np
import pytest

import _align_loop_case as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _align():
    from spateo_amd import align

    return align


def _fake_kernel(n=20, m=4, beta=0.5, D=3):
    """A GraphKernel made by hand (no device): enough for the validation in front of every launch."""
    from spateo_amd._graph import GraphKernel, KnnGraph

    rng = np.random.default_rng(0)
    X = rng.random((n, D))
    idx = np.arange(m)
    U = rng.random((n, m))
    graph = KnnGraph(n, host=(np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0)))
    return X, GraphKernel(U, U[idx].copy(), idx, X[idx].copy(), graph, beta, 0, 0)


def _loop_call(fn, X, gk, **over):
    kw = dict(dissimilarity="kl", probability_type="gauss", probability_parameters=[0.1], inducing_variables=gk.inducing_variables,
              beta=gk.beta, lambdaVF=1.0, sigma2=0.1, max_iter=2, kernel_type="geodist", graph_kernel=gk)
    kw.update(over)
    layer = np.ones((len(X), 3))
    return fn(X, X[:7], [layer], [layer[:7]], **kw)


def test_the_names_are_public_and_documented():
    import spateo_amd as st

    align = _align()
    for name in ("knn", "construct_knn_graph", "graph_distances", "con_K_graph", "graph_kernel", "KnnGraph", "GraphKernel"):
        assert name in align.__all__ and getattr(st.align, name).__doc__.strip(), name
    import inspect

    assert list(inspect.signature(align.con_K_graph).parameters)[:3] == ["graph", "inducing_idx", "beta"]
    assert inspect.signature(align.con_K_graph).parameters["beta"].default == 0.01
    assert inspect.signature(align.construct_knn_graph).parameters["knn"].default == 10
    for fn in (align.morpho_iterate, align.morpho_iterate_svi, align.update_nonrigid):
        assert "graph_kernel" in inspect.signature(fn).parameters and "graph_kernel" in fn.__doc__
    assert "geodist" in align.morpho_iterate.__doc__ and "np.random" in align.graph_kernel.__doc__
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "st.align.graph_kernel" in readme and "mvf_graph_sssp" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "A kernel along the tissue" in design


@pytest.mark.parametrize("which", ["morpho_iterate", "morpho_iterate_svi", "update_nonrigid"])
def test_geodist_without_a_graph_kernel_still_refuses_and_names_the_way_in(which):
    align = _align()
    X, gk = _fake_kernel()
    if which == "update_nonrigid":
        call = lambda **kw: align.update_nonrigid(X, gk.inducing_variables, 0.5, np.ones(len(X)), np.zeros((len(X), 3)), 0.1, 1.0, **kw)  # noqa: E731
    else:
        call = lambda **kw: _loop_call(getattr(align, which), X, gk, **dict(dict(graph_kernel=None), **kw))  # noqa: E731
    with pytest.raises(NotImplementedError, match=r"geodist.*graph_kernel"):
        call(kernel_type="geodist")
    with pytest.raises(NotImplementedError, match="kernel_type"):
        call(kernel_type="cosine")


@pytest.mark.parametrize("which", ["morpho_iterate", "morpho_iterate_svi", "update_nonrigid"])
def test_a_graph_kernel_that_does_not_fit_the_call_is_a_value_error(which):
    align = _align()
    X, gk = _fake_kernel()
    if which == "update_nonrigid":
        def call(X_=X, ctrl=gk.inducing_variables, beta=gk.beta, **kw):
            kw = dict(dict(kernel_type="geodist", graph_kernel=gk), **kw)
            return align.update_nonrigid(X_, ctrl, beta, np.ones(len(X_)), np.zeros((len(X_), 3)), 0.1, 1.0, **kw)
    else:
        def call(X_=X, ctrl=gk.inducing_variables, beta=gk.beta, **kw):
            return _loop_call(getattr(align, which), X_, gk, inducing_variables=ctrl, beta=beta, **kw)
    with pytest.raises(ValueError, match="cells"):
        call(X_=X[:-1])                                        # mismatched lengths
    with pytest.raises(ValueError, match="inducing variables"):
        call(ctrl=gk.inducing_variables[:-1])
    with pytest.raises(ValueError, match="beta"):
        call(beta=0.25)                                        # a different beta
    with pytest.raises(ValueError, match="kernel_type='geodist'"):
        call(kernel_type="euc")                                # graph_kernel= with the Euclidean kernel
    with pytest.raises(ValueError, match="st.align.graph_kernel"):
        call(graph_kernel=(gk.inducing_variables, gk.Gamma, gk.U))


def test_graph_arguments_are_refused_with_their_reason():
    import networkx

    align = _align()
    X = np.random.default_rng(1).random((8, 2))
    for fn in (align.construct_knn_graph, align.knn):
        with pytest.raises(ValueError, match="knn >= n"):
            fn(X, 8)
    with pytest.raises(ValueError, match="64"):
        align.knn(np.zeros((100, 2)), 65)
    with pytest.raises(ValueError, match=r"\(n, 2\) or \(n, 3\)"):
        align.knn(np.zeros((100, 4)), 5)
    g = networkx.Graph()
    g.add_edge("a", "b", weight=1.0)
    with pytest.raises(ValueError, match="node label"):
        align.con_K_graph(g, np.array([0]))
    g = networkx.Graph()
    g.add_edge(0, 5, weight=1.0)                               # two nodes, labels not 0 .. 1
    with pytest.raises(ValueError, match="node label"):
        align.graph_distances(g, np.array([0]))
    g = networkx.Graph()
    g.add_edge(0, 1, weight=-1.0)
    with pytest.raises(ValueError, match="negative"):
        align.graph_distances(g, np.array([0]))
    g = networkx.path_graph(4)
    with pytest.raises(ValueError, match="source index"):
        align.graph_distances(g, np.array([4]))
    with pytest.raises(ValueError, match="nodes"):
        align.graph_kernel(X, np.array([0, 1]), 0.5, graph=g)
    with pytest.raises(TypeError, match="KnnGraph"):
        align.graph_distances(np.eye(3), np.array([0]))


def test_networkx_round_trip_on_the_host():
    import networkx
    from spateo_amd._graph import KnnGraph

    g = networkx.Graph()
    g.add_nodes_from(range(6))
    g.add_weighted_edges_from([(0, 1, 0.5), (1, 2, 1.5), (4, 3, 2.0), (2, 2, 9.0)])
    g.add_edge(0, 2)                                           # no weight: 1, as in networkx's Dijkstra
    k = KnnGraph.from_networkx(g)
    indptr, indices, weights = k.host_arrays()
    assert indptr.tolist() == [0, 2, 4, 6, 7, 8, 8] and indices.tolist() == [1, 2, 0, 2, 0, 1, 4, 3] and k.n_edges == 4
    assert weights.tolist() == [0.5, 1.0, 0.5, 1.5, 1.0, 1.5, 2.0, 2.0] and indices.dtype == np.int32 and indptr.dtype == np.int64
    back = k.to_networkx()
    assert back.number_of_nodes() == 6 and sorted(back.edges(data="weight")) == [(0, 1, 0.5), (0, 2, 1.0), (1, 2, 1.5), (3, 4, 2.0)]


def test_BA_transform_refuses_a_geodist_vecfld():
    align = _align()
    vecfld = {"kernel_type": "geodist"}
    with pytest.raises(ValueError, match="geodist"):
        align.BA_transform(vecfld, np.zeros((3, 3)))


def test_the_abi_version_stays_and_the_header_names_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "mvf.h")).read()
    assert re.search(r"ABI version, currently (\d+)", text).group(1) == "7"
    from spateo_amd import _lib

    for name in ("mvf_knn", "mvf_knn_workspace_bytes", "mvf_graph_sssp", "mvf_pinv_diag_cached"):
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", text), name
    if os.path.exists(_lib.LIB_PATH):
        assert _lib.load().mvf_version() == 7
    assert lc.F64_TOL == 1e-10   # the loops' criterion the GPU tests of the geodesic kernel reuse, unchanged
