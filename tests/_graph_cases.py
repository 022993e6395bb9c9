"""Shared by the CPU and GPU suites of the kernel along the tissue (``csrc/mvf_graph.hip``, ``spateo_amd/_graph.py``): access to
tests/golden/ref_graph_kernel.npz (tests/golden/make_golden_graph_kernel.py: the real ``construct_knn_graph`` / ``con_K_graph``
and the real loop methods on the geodesic kernel), NumPy restatements of the neighbour search, the union of edges and the
relaxation (test infrastructure, written from the rules below), and the small clouds and graphs of the kernel-level tests.

    search      d(i, j) = sqrt((dx dx + dy dy) + dz dz) of explicit differences, every row ascending by (distance, index), the
                point itself left out by index;
    union       an edge {i, j} with weight d(i, j) when either point lists the other, edges of weight 0 dropped; CSR with both
                directions, indices ascending per row;
    relaxation  d[v, s] <- min(d[v, s], d[u, s] + w) over the edges (v, u), in place, node after node in ANY order, until a whole
                sweep changes nothing: the fixed point is the minimum over all paths of the left-to-right sum, whatever the order.

Bounds (the issue's): neighbour indices and edge sets equal; D within 2 ulp (the expectation is bit-equal; the allowance covers a
contracted multiply-add in a binary we cannot see); K within 4 ulp (the exponent's argument is formed by identical operations,
``exp`` is within 1 ulp on either side)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_graph_kernel.npz")
UNREACHABLE = 1e5
D_ULP, K_ULP = 2, 4
_CACHE = {}


def load():
    if "g" not in _CACHE:
        _CACHE["g"] = np.load(GOLDEN)
    return _CACHE["g"]


class View:
    """The arrays of a golden file whose names start with ``prefix``, under their names without it: what the case modules of
    the loops index (``g["iters"]``, ``g[f"{tag}_sigma2"]``, ``g.files``)."""

    def __init__(self, g, prefix):
        self.g, self.prefix = g, prefix

    def __getitem__(self, key):
        return self.g[self.prefix + key]

    @property
    def files(self):
        return [f[len(self.prefix):] for f in self.g.files if f.startswith(self.prefix)]


def graph_tags(g=None):
    return [str(t) for t in (g or load())["graph_cases"]]


def loop_tags(g=None):
    return [str(t) for t in (g or load())["cases"]]


def ulps(a, b):
    """Largest distance in units of the last place between two float64 arrays of non-negative finite values."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all() and (a >= 0).all() and (b >= 0).all()
    return int(np.abs(a.view(np.int64) - b.view(np.int64)).max()) if a.size else 0


# ---- restatements ---------------------------------------------------------------------------------------------------------
def knn_restated(X, k):
    """(idx (n, k) int32, dist (n, k) float64): all pairs, explicit differences, squares added in axis order."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    idx, dist = np.empty((n, k), dtype=np.int32), np.empty((n, k))
    for i in range(n):
        df = X[i] - X
        s = df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1]
        if d == 3:
            s = s + df[:, 2] * df[:, 2]
        r = np.sqrt(s)
        others = np.delete(np.arange(n), i)
        order = others[np.lexsort((others, r[others]))][:k]
        idx[i], dist[i] = order, r[order]
    return idx, dist


def union_restated(idx, dist):
    """{(i, j): weight, i < j} of the undirected union; a neighbour at distance 0 adds no edge."""
    edges = {}
    for i in range(len(idx)):
        for j, w in zip(idx[i].tolist(), dist[i].tolist()):
            if w != 0:
                edges[(min(i, j), max(i, j))] = w
    return edges


def csr_of(edges, n):
    """(indptr int64, indices int32 ascending per row, weights float64) with both directions of {(i, j): w}."""
    both = sorted([(i, j, w) for (i, j), w in edges.items()] + [(j, i, w) for (i, j), w in edges.items()])
    rows = np.array([e[0] for e in both], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return indptr, np.array([e[1] for e in both], dtype=np.int32), np.array([e[2] for e in both], dtype=np.float64)


def edges_of(indptr, indices, weights):
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return {(int(i), int(j)): float(w) for i, j, w in zip(rows, indices, weights) if i < j}


def relax_restated(indptr, indices, weights, n, sources, order="forward", seed=0):
    """(D (n, m) with +inf where there is no path, sweeps): in-place relaxation, the nodes of every sweep in the given order
    ("forward", "reversed", or "random": a new permutation per sweep)."""
    m = len(sources)
    D = np.full((n, m), np.inf)
    D[np.asarray(sources), np.arange(m)] = 0.0
    rng = np.random.default_rng(seed)
    sweeps = 0
    while True:
        nodes = {"forward": np.arange(n), "reversed": np.arange(n)[::-1]}.get(order)
        if nodes is None:
            nodes = rng.permutation(n)
        changed = False
        for v in nodes:
            lo, hi = indptr[v], indptr[v + 1]
            if lo == hi:
                continue
            cand = (D[indices[lo:hi]] + weights[lo:hi, None]).min(0)
            low = cand < D[v]
            if low.any():
                D[v] = np.where(low, cand, D[v])
                changed = True
        sweeps += 1
        if not changed:
            return D, sweeps


def kernel_restated(D, beta):
    D = np.where(np.isinf(D), UNREACHABLE, D)
    return np.exp((-beta) * (D * D))


def dijkstra(indptr, indices, weights, n, source):
    """networkx.single_source_dijkstra on the CSR graph: distances as an (n,) array, +inf where there is no path."""
    import networkx

    g = networkx.Graph()
    g.add_nodes_from(range(n))
    rows = np.repeat(np.arange(n), np.diff(indptr))
    g.add_weighted_edges_from(zip(rows.tolist(), np.asarray(indices).tolist(), np.asarray(weights).tolist()))
    dist, _ = networkx.single_source_dijkstra(g, source=int(source), weight="weight")
    out = np.full(n, np.inf)
    for node, v in dist.items():
        out[node] = v
    return out


# ---- the clouds and graphs of the kernel-level tests ------------------------------------------------------------------------
def clouds():
    """{name: (points, k)}: the shapes at which the search can go wrong."""
    rng = np.random.default_rng(20261021)
    line = np.zeros((200, 2))
    line[:, 0] = np.cumsum(0.5 + rng.random(200))                   # points on a line in the plane, distinct spacings
    dup = rng.random((300, 3))
    dup[[7, 50, 120, 121, 299]] = dup[[3, 3, 119, 119, 0]]          # duplicates: one point three times, one pair twice over
    tight = 1e3 + 1e-9 * rng.random((150, 3))
    return {
        "n=k+1 (3-D)": (rng.random((11, 3)), 10),
        "n=k+1 (2-D)": (rng.random((65, 2)), 64),
        "257 (3-D)": (rng.standard_normal((257, 3)), 10),
        "257 (2-D)": (rng.standard_normal((257, 2)), 1),
        "1000 (3-D)": (rng.random((1000, 3)) * [4.0, 1.0, 0.25], 10),  # an anisotropic box: the grid has fewer cells along z
        "slab (3-D)": (rng.random((2000, 3)) * [10.0, 10.0, 0.05], 10),  # a tissue section: the short axis gets one cell
        "1000 (2-D)": (rng.random((1000, 2)), 64),
        "1000 (2-D) k=10": (rng.standard_normal((1000, 2)), 10),
        "one cell": (np.concatenate([tight, [[0.0, 0.0, 0.0], [2e3, 2e3, 2e3]]]), 10),  # all but two points inside one cell
        "line": (line, 10),
        "duplicates": (dup, 10),
        "all equal": (np.full((40, 2), 0.25), 3),                    # a zero extent: every distance 0, ties by index
    }


def path_graph(n=300, seed=1):
    w = 0.5 + np.random.default_rng(seed).random(n - 1)
    return csr_of({(i, i + 1): float(w[i]) for i in range(n - 1)}, n) + (n,)


def star_graph(n=130, seed=2):
    w = 0.5 + np.random.default_rng(seed).random(n - 1)
    return csr_of({(0, i + 1): float(w[i]) for i in range(n - 1)}, n) + (n,)


def two_components(seed=3):
    """The kNN graphs of two far blobs of 90 and 70 points, and an isolated node (160): three components."""
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.standard_normal((90, 2)), 50.0 + rng.standard_normal((70, 2))])
    edges = union_restated(*knn_restated(X, 5))
    return csr_of(edges, 161) + (161,)
