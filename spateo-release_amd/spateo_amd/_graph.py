"""A kernel along the tissue: the ``kernel_type="geodist"`` branch of ``Morpho_pairwise._construct_kernel``
(``spateo/alignment/methods/morpho_class.py:865-871``) on the MI355X - ``construct_knn_graph`` and ``con_K_graph`` of
``spateo/alignment/methods/utils.py:1161-1217`` without the dense N x N neighbour matrix, the Python double loop over it and the
one ``networkx`` Dijkstra per inducing variable.

* ``knn``                  ``mvf_knn``: the exact k nearest other points on a uniform grid (``csrc/mvf_graph.hip``);
* ``construct_knn_graph``  the undirected union of the neighbour lists as CSR, formed on the device with torch's sort / unique of
                           the n k integer edge keys (not a hot path; no host round trip of the edge list);
* ``graph_distances``      ``mvf_graph_sssp``: Bellman-Ford sweeps from all sources at once, to the fixed point;
* ``con_K_graph``          ``K = exp((-beta) * (D * D))`` with ``D = 1e5`` where there is no path (the reference's initial value);
* ``graph_kernel``         the triple ``(inducing_variables, GammaSparse, U)`` of ``_construct_kernel`` as a ``GraphKernel``, which
                           ``morpho_iterate``, ``morpho_iterate_svi`` and ``update_nonrigid`` take as ``graph_kernel=``.

Reproduced as the reference has it: the edge list is sklearn's ``kneighbors_graph(points, knn, mode="distance",
include_self=False)`` made undirected by ``networkx.Graph.add_edge``; a neighbour at distance exactly 0 (a duplicated
coordinate) takes one of the knn slots but adds no edge (the loop tests ``if connected``); an unreachable pair keeps ``D = 1e5``;
``GammaSparse = U[inducing_idx]``.  Deviations ("A kernel along the tissue"): a node left without any edge
stays in the graph, isolated (the reference's graph loses it and its ``D`` has the wrong number of rows); distances are always
formed from explicit differences (sklearn switches to |x|^2 + |y|^2 - 2 x.y at ``knn >= n // 2``); ties at the k-th distance go
to the smaller index (sklearn's order is unspecified); ``D`` is float64 whatever ``dtype`` (the reference's torch backend gives
float32)."""
from __future__ import annotations

import numpy as np

import torch

from . import _lib
from . import _runtime as _rt

UNREACHABLE = 1e5  # con_K_graph's initial value of D (utils.py:1204): exp(-beta 1e10) == 0 for every beta the alignment uses


class KnnGraph:
    """An undirected weighted graph on the nodes 0 .. n - 1 as CSR - ``indptr`` (n + 1,) int64, ``indices`` int32 ascending per
    row, ``weights`` float64, both directions of every edge stored - on the device and, lazily, on the host."""

    def __init__(self, n, dev=None, host=None):
        self.n = int(n)
        self._dev, self._host = dev, host

    @property
    def n_edges(self):
        return int((self._dev or self._host)[1].shape[0]) // 2

    def host_arrays(self):
        """(indptr, indices, weights) as NumPy arrays."""
        if self._host is None:
            self._host = tuple(t.cpu().numpy() for t in self._dev)
        return self._host

    def device_arrays(self, k):
        """(indptr, indices, weights) as tensors on the device of the kernels object ``k``."""
        if self._dev is None or self._dev[0].device != k.device:
            indptr, indices, weights = self.host_arrays()
            pad = lambda a: a if len(a) else np.zeros(1, dtype=a.dtype)  # noqa: E731  (an edgeless graph still needs an address)
            self._dev = (k.h2d(indptr), k.h2d(pad(indices))[: len(indices)], k.h2d(pad(weights))[: len(weights)])
        return self._dev

    def degrees(self):
        return np.diff(self.host_arrays()[0])

    def to_networkx(self):
        """The graph as a ``networkx.Graph`` with every node 0 .. n - 1, the isolated ones included."""
        import networkx

        indptr, indices, weights = self.host_arrays()
        g = networkx.Graph()
        g.add_nodes_from(range(self.n))
        rows = np.repeat(np.arange(self.n), np.diff(indptr))
        up = rows < indices
        g.add_weighted_edges_from(zip(rows[up].tolist(), indices[up].tolist(), weights[up].tolist()))
        return g

    @classmethod
    def from_networkx(cls, g):
        """CSR on the host from anything with ``number_of_nodes()`` and ``edges(data="weight")`` (an edge without a weight
        counts 1, as in networkx's Dijkstra).  ``ValueError`` for node labels other than 0 .. n - 1 or a negative weight."""
        n = int(g.number_of_nodes())
        edges = list(g.edges(data="weight"))
        labels = list(g.nodes) if hasattr(g, "nodes") else [v for e in edges for v in e[:2]]
        for v in labels:
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) < n:
                raise ValueError(f"graph: node label {v!r} - the nodes must be the integers 0 .. n - 1 = {n - 1} (one per row of the "
                                 f"coordinates)")
        if n >= 1 << 31:
            raise ValueError("graph: fewer than 2^31 nodes")
        a = np.array([(int(i), int(j)) for i, j, _ in edges], dtype=np.int64).reshape(-1, 2)
        w = np.array([1.0 if x is None else float(x) for _, _, x in edges], dtype=np.float64)
        if len(w) and not np.all(w >= 0.0):
            raise ValueError("graph: negative (or NaN) edge weight - shortest paths need weights >= 0")
        keep = a[:, 0] != a[:, 1]
        a, w = a[keep], w[keep]
        src, dst, ww = np.concatenate([a[:, 0], a[:, 1]]), np.concatenate([a[:, 1], a[:, 0]]), np.concatenate([w, w])
        order = np.argsort(src * n + dst, kind="stable")
        indptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int64)
        return cls(n, host=(indptr, dst[order].astype(np.int32), ww[order]))


def _as_graph(graph):
    if isinstance(graph, KnnGraph):
        return graph
    if hasattr(graph, "number_of_nodes") and hasattr(graph, "edges"):
        return KnnGraph.from_networkx(graph)
    raise TypeError("graph must be a KnnGraph (construct_knn_graph) or a networkx.Graph on the nodes 0 .. n - 1")


def _points(points, who):
    X = np.ascontiguousarray(points, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] not in (2, 3):
        raise ValueError(f"{who}: points must be (n, 2) or (n, 3), got shape {X.shape}")
    if not np.isfinite(X).all():
        raise ValueError(f"{who}: non-finite coordinates")
    return X


def _check_knn(n, knn, who):
    if int(knn) != knn or knn < 1:
        raise ValueError(f"{who}: knn must be a positive integer")
    if knn >= n:
        raise ValueError(f"{who}: knn >= n ({int(knn)} >= {n}): a point has only n - 1 other points")
    if knn > _lib.KNN_MAX_K:
        raise ValueError(f"{who}: knn = {int(knn)} is above the {_lib.KNN_MAX_K} neighbours mvf_knn keeps per point")
    if n >= 1 << 31:
        raise ValueError(f"{who}: fewer than 2^31 points")
    return int(knn)


def knn(points, k, device=None):
    """The exact ``k`` nearest OTHER points of every point (``mvf_knn``): host ``(idx (n, k) int32, dist (n, k) float64)``, every
    row ascending by (distance, index).  ``points`` (n, D), D in {2, 3}; 1 <= k <= 64, k < n.  A point is left out of its own
    list by index, so a duplicate of it is a neighbour at distance 0; among equal distances the smaller index wins.  The distance
    is what sklearn's KD-tree computes: explicit differences, squares added in axis order, then the square root."""
    X = _points(points, "knn")
    kk = _check_knn(len(X), k, "knn")
    kern = _rt._shared_kernels(device, "float64")
    idx, dist = kern.knn(kern.h2d(X), kk)
    idx, dist = kern.to_host([idx, dist], own_pinned=False)
    return np.array(idx), np.array(dist)


def _union(kern, idx, dist, n):
    """The undirected union of the neighbour lists as device CSR: an edge {i, j} when either lists the other, edges of weight 0
    dropped.  d(i, j) and d(j, i) are the same bits (the differences change sign, their squares do not)."""
    k = idx.shape[1]
    rows = torch.arange(n, dtype=torch.int64, device=idx.device).repeat_interleave(k)
    cols, w = idx.reshape(-1).to(torch.int64), dist.reshape(-1)
    keep = w != 0
    rows, cols, w = rows[keep], cols[keep], w[keep]
    key = torch.minimum(rows, cols) * n + torch.maximum(rows, cols)     # n < 2^31: below 2^62
    ukey, inv = torch.unique(key, return_inverse=True)
    wu = torch.empty(ukey.shape[0], dtype=torch.float64, device=idx.device)
    wu[inv] = w                                                         # (both copies of an edge carry the same bits)
    lo, hi = ukey // n, ukey % n
    src, dst, ww = torch.cat([lo, hi]), torch.cat([hi, lo]), torch.cat([wu, wu])
    order = torch.argsort(src * n + dst)                                # (keys are distinct: any sort gives this order)
    counts = torch.bincount(src, minlength=n)
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=idx.device)
    indptr[1:] = torch.cumsum(counts, 0)
    return indptr, dst[order].to(torch.int32).contiguous(), ww[order].contiguous()


def construct_knn_graph(points, knn: int = 10, device=None):
    """``construct_knn_graph`` (``spateo/alignment/methods/utils.py:1161-1188``): the k-nearest-neighbour graph of ``points``
    (n, D), D in {2, 3}, made undirected - an edge {i, j} with weight |x_i - x_j| when either point lists the other.  Returns a
    ``KnnGraph`` (CSR on the device; ``to_networkx()`` gives the reference's object).  A neighbour at distance 0 takes one of
    the ``knn`` slots but adds no edge, as in the reference; a node left without any edge stays in the graph, isolated.
    ``ValueError`` when ``knn >= n``."""
    X = _points(points, "construct_knn_graph")
    kk = _check_knn(len(X), knn, "construct_knn_graph")
    kern = _rt._shared_kernels(device, "float64")
    idx, dist = kern.knn(kern.h2d(X), kk)
    return KnnGraph(len(X), dev=_union(kern, idx, dist, len(X)))


def _sources(inducing_idx, n, who):
    src = np.asarray(inducing_idx)
    if src.ndim != 1 or len(src) == 0 or src.dtype.kind not in "iu":
        raise ValueError(f"{who}: the sources must be a non-empty 1-D integer array of node indices")
    if src.min() < 0 or src.max() >= n:
        raise ValueError(f"{who}: source index outside 0 .. n - 1 = {n - 1}")
    return np.ascontiguousarray(src, dtype=np.int32)


def _distances(kern, graph, src):
    """(D on the device, (n, m) float64 with +inf where there is no path; sweeps queued)."""
    indptr, indices, weights = graph.device_arrays(kern)
    return kern.graph_sssp(indptr, indices, weights, graph.n, kern.h2d(src))


def graph_distances(graph, sources, device=None):
    """Shortest-path distances through ``graph`` (a ``KnnGraph`` or a ``networkx.Graph`` on the nodes 0 .. n - 1) from every node
    to each of ``sources`` (m node indices, repeats allowed): host (n, m) float64, ``1e5`` where there is no path - the ``D`` of
    ``con_K_graph``.  ``mvf_graph_sssp``: Bellman-Ford sweeps to the fixed point, which is the minimum over all paths of the
    left-to-right sum of the weights - what ``networkx.single_source_dijkstra`` returns, bit for bit."""
    g = _as_graph(graph)
    src = _sources(sources, g.n, "graph_distances")
    kern = _rt._shared_kernels(device, "float64")
    D, _ = _distances(kern, g, src)
    D = torch.where(torch.isinf(D), torch.full_like(D, UNREACHABLE), D)
    return np.array(kern.to_host([D], own_pinned=False)[0])


def _kernel_values(D, beta):
    """(K = exp((-beta) * (D * D)) with D = 1e5 where there is no path, rows with an unreachable source) on the device."""
    missing = torch.isinf(D)
    D = torch.where(missing, torch.full_like(D, UNREACHABLE), D)
    return torch.exp((-float(beta)) * (D * D)), int(missing.any(1).sum())


def con_K_graph(graph, inducing_idx, beta=0.01, device=None):
    """``con_K_graph`` (``spateo/alignment/methods/utils.py:1191-1217``): ``K[j, i] = exp(-beta D[j, i]^2)`` of the graph distance
    from node j to inducing variable i (``D = 1e5`` where there is no path: K is exactly 0 there).  Host (n, m) float64."""
    g = _as_graph(graph)
    src = _sources(inducing_idx, g.n, "con_K_graph")
    kern = _rt._shared_kernels(device, "float64")
    K, _ = _kernel_values(_distances(kern, g, src)[0], beta)
    return np.array(kern.to_host([K], own_pinned=False)[0])


class GraphKernel:
    """What ``graph_kernel`` returns and the loops take as ``graph_kernel=``: ``U`` (n, m) and ``Gamma = U[inducing_idx]`` (m, m),
    host float64 (``U`` stays on the device until it is read); ``inducing_idx`` (m,); ``inducing_variables = coordsA[inducing_idx]``; ``graph`` (the ``KnnGraph``); ``beta``;
    ``n_unreachable``, the number of nodes that at least one inducing variable cannot reach (their entries of ``U`` are 0)."""

    def __init__(self, U, Gamma, inducing_idx, inducing_variables, graph, beta, n_unreachable, sweeps):
        # U: a host array, or the device tensor it was computed in - kept there for the loops (1.6 GB at 10^6 cells and 200
        # inducing variables), copied to the host only when ``U`` is read
        self._U_dev, self._U = (U, None) if torch.is_tensor(U) else (None, U)
        self.shape = tuple(int(v) for v in U.shape)
        self.Gamma, self.inducing_idx, self.inducing_variables = Gamma, inducing_idx, inducing_variables
        self.graph, self.beta, self.n_unreachable, self.sweeps = graph, float(beta), int(n_unreachable), int(sweeps)

    @property
    def U(self):
        if self._U is None:
            self._U = self._U_dev.cpu().numpy()
        return self._U

    def device_U(self, k):
        """U as a float64 tensor on the device of the kernels object ``k``."""
        if self._U_dev is None or self._U_dev.device != k.device:
            self._U_dev = k.h2d(np.ascontiguousarray(self.U, dtype=np.float64))
        return self._U_dev

    def __repr__(self):
        return (f"GraphKernel(n={self.shape[0]}, m={self.shape[1]}, beta={self.beta}, edges={self.graph.n_edges}, "
                f"n_unreachable={self.n_unreachable})")


def graph_kernel(coordsA, inducing_idx, beta, graph=None, graph_knn: int = 10, dtype: str = "float64", device=None, seed=None):
    """The kernel of the ``kernel_type="geodist"`` branch of ``Morpho_pairwise._construct_kernel`` (``morpho_class.py:865-871``):
    ``U = con_K_graph(graph, inducing_idx, beta)``, ``GammaSparse = U[inducing_idx]``, ``graph = construct_knn_graph(coordsA,
    graph_knn)`` unless one is given (a ``KnnGraph`` or a ``networkx.Graph`` on the nodes 0 .. NA - 1).  Returns a ``GraphKernel``.

    ``inducing_idx``: the indices of the inducing variables in ``coordsA``, or their number - then, as ``_construct_kernel`` does
    (``:845-852``), that many are drawn without replacement from the first occurrences of the unique rows (all of them when there
    are no more) with ``np.random.default_rng(seed)``: our own seeded draw, NOT the reference's global ``np.random`` stream
    (as in ``morpho_start``).  ``beta`` is the ``beta`` the loop is then called with.  ``dtype`` is the cell dtype of the loop it
    is meant for and changes nothing here: ``U`` and ``Gamma`` are float64 (the loop rounds ``U`` once, into its operand cache)."""
    if dtype not in ("float32", "float64"):
        raise ValueError("dtype must be 'float32' or 'float64'")
    if not float(beta) > 0.0:
        raise ValueError("graph_kernel: beta must be positive")
    X = _points(coordsA, "graph_kernel")
    n = len(X)
    if isinstance(inducing_idx, (int, np.integer)) and not isinstance(inducing_idx, bool):
        if inducing_idx < 1:
            raise ValueError("graph_kernel: the number of inducing variables must be positive")
        _, first = np.unique(X, axis=0, return_index=True)
        pick = (np.random.default_rng(seed).choice(len(first), int(inducing_idx), replace=False) if len(first) > inducing_idx
                else np.arange(len(first)))
        inducing_idx = first[pick]
    g = construct_knn_graph(X, graph_knn, device=device) if graph is None else _as_graph(graph)
    if g.n != n:
        raise ValueError(f"graph_kernel: the graph has {g.n} nodes, coordsA {n} rows")
    src = _sources(inducing_idx, n, "graph_kernel")
    kern = _rt._shared_kernels(device, "float64")
    D, sweeps = _distances(kern, g, src)
    K, n_unreachable = _kernel_values(D, beta)
    idx = src.astype(np.int64)
    Gamma = np.array(kern.to_host([K[kern.h2d(idx)].contiguous()], own_pinned=False)[0])
    return GraphKernel(K, Gamma, idx, X[idx].copy(), g, beta, n_unreachable, sweeps)


def check_graph_kernel(gk, kernel_type, NA, m, beta, who):
    """The loops' validation of ``graph_kernel=`` (no device needed)."""
    if not isinstance(gk, GraphKernel):
        raise ValueError(f"{who}: graph_kernel must be what st.align.graph_kernel returns")
    if kernel_type != "geodist":
        raise ValueError(f"{who}: graph_kernel= goes with kernel_type='geodist' (got kernel_type={kernel_type!r})")
    if gk.shape[0] != NA:
        raise ValueError(f"{who}: the graph kernel was built for {gk.shape[0]} cells, coordsA has {NA}")
    if gk.shape[1] != m:
        raise ValueError(f"{who}: the graph kernel has {gk.shape[1]} inducing variables, inducing_variables {m} rows "
                         f"(pass inducing_variables=graph_kernel.inducing_variables)")
    if gk.beta != float(beta):
        raise ValueError(f"{who}: the graph kernel was built with beta = {gk.beta}, the call has beta = {float(beta)}")
