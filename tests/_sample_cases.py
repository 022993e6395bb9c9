"""Float64 restatements of the samplers the device runs (``csrc/mvf_sample.hip``) - TRN, k-means, nearest row - that the GPU
suites compare against, the cases they share, and the two bounds of the comparison, DERIVED here (no tolerance is hard-coded):

  * TRN: the deviation of the restatement with every exponential perturbed by +-4 ulp from the unperturbed one, relative to
    the coordinate extent, per case; the GPU assertion is ``ALLOW`` = 64 times that.  One ulp is what a device ``exp`` may
    differ by; 4 ulp and the factor 64 leave room for its error model without admitting a wrong rank, which moves a node by a
    visible fraction of a cell spacing.
  * k-means: the deviation of the centroids when the cluster sums are taken in a shuffled order; the GPU assertion is 64 times
    that (the device adds fixed blocks of rows, then the blocks).

tests/test_sample_kernel_refs.py proves the restatements equal the real thing: TRN against the goldens of the reference's
``TRNET`` (tests/golden/ref_downsampling.npz), k-means against ``scipy.cluster.vq.kmeans2``, nearest row against brute force."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ALLOW = 64.0
ULP = 2.0 ** -52
TRN_TAGS = tuple("abcdefghij")
# the tmax = 20 series of the kernel tests: n -> (N, d); sizes around the wave (64), the workgroup (1024) and the cap (4096)
SERIES = {1: (50, 2), 2: (60, 3), 63: (500, 2), 64: (500, 3), 65: (700, 2), 257: (3000, 3), 1025: (5000, 2), 4096: (9000, 3)}


def load():
    with np.load(os.path.join(HERE, "golden", "ref_downsampling.npz")) as z:
        return {k: z[k] for k in z.files}


def golden_case(G, tag):
    """(X, n, seed, kwargs, W, repeat) of one stored TRN case."""
    seed = int(G[f"{tag}_seed"])
    kw = {}
    if float(G[f"{tag}_tmax"]) != 200:
        kw["tmax"] = float(G[f"{tag}_tmax"])
    if float(G[f"{tag}_c"]) != 0:
        kw["c"] = float(G[f"{tag}_c"])
    return G[f"{tag}_X"], int(G[f"{tag}_n"]), (19491001 if seed < 0 else seed), kw, G[f"{tag}_W"], bool(G[f"{tag}_repeat"])


def series_coordinates(n):
    N, d = SERIES[n]
    return np.random.default_rng(77 * n + d).random((N, d)) * np.array([1500.0, 1100.0, 700.0][:d])


def trn_draws(X, n, seed=19491001, tmax=200):
    """(w_idx, p_idx): the two draws of ``TRNET`` - each after ``np.random.seed(seed)`` - from a private generator."""
    T = int(tmax * n)
    return (np.random.RandomState(seed).randint(0, X.shape[0], n), np.random.RandomState(seed).randint(0, X.shape[0], T))


def trn_schedule(n, tmax=200, li=0.2, lf=0.01, ei=0.3, ef=0.05, c=0):
    """(l, ep, kc or None) per step, scalar by scalar as ``TRNET.run`` / ``runOnce`` evaluate them."""
    T = int(tmax * n)
    li = li * n
    l, ep = np.empty(T), np.empty(T)
    for t in range(1, T + 1):
        tt = t / T
        l[t - 1] = li * np.power(lf / li, tt)
        ep[t - 1] = ei * np.power(ef / ei, tt)
    kc = None if c == 0 else np.array([-a * np.log(c / b) for a, b in zip(l, ep)]).reshape(T)
    return l, ep, kc


def trn_restate(X, n, seed=19491001, tmax=200, li=0.2, lf=0.01, ei=0.3, ef=0.05, c=0, jitter_ulp=0):
    """``TRNET(n, X, seed).run(...)``'s nodes: the squared distance summed in column order, the rank by (distance, node) - the
    lower node first among equal distances -, the update ``(ep exp(-k / l)) D``.  ``jitter_ulp``: every exponential scaled by
    ``1 + j ULP``, j drawn from {-jitter_ulp, 0, +jitter_ulp} (the bound's perturbation)."""
    X = np.asarray(X, dtype=np.float64)
    w_idx, p_idx = trn_draws(X, n, seed, tmax)
    l, ep, kc = trn_schedule(n, tmax, li, lf, ei, ef, c)
    W, P = X[w_idx].copy(), X[p_idx]
    rng = np.random.default_rng(1)
    ranks = np.arange(n)
    K = np.empty(n, dtype=np.int64)
    for t in range(len(p_idx)):
        D = P[t] - W
        sD = D[:, 0] * D[:, 0]
        for j in range(1, X.shape[1]):
            sD = sD + D[:, j] * D[:, j]
        K[np.argsort(sD, kind="stable")] = ranks
        e = np.exp(-K[:, None] / l[t])
        if jitter_ulp:
            e = e * (1 + jitter_ulp * ULP * rng.integers(-1, 2, e.shape))
        if kc is None:
            W += ep[t] * e * D
        else:
            idx = K < kc[t]
            W[idx] += ep[t] * e[idx] * D[idx]
    return W


def sort_rows(W):
    """The rows of W as a sorted multiset (lexicographic): what stays bit-equal when two identical start nodes swap."""
    W = np.asarray(W)
    return W[np.lexsort(W.T[::-1])]


def sq_dist(A, B):
    """(len(A), len(B)) squared distances, ((d0 d0) + d1 d1) + d2 d2."""
    s = (A[:, None, 0] - B[None, :, 0]) ** 2
    for j in range(1, A.shape[1]):
        s = s + (A[:, None, j] - B[None, :, j]) ** 2
    return s


def nearest_restate(X, Q, block=2048):
    """For every row of Q the nearest row of X, the smallest index among equal distances (np.argmin's rule), in blocks of X
    combined with a strict ``<`` in rising order."""
    X, Q = np.asarray(X, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    best = np.full(len(Q), np.inf)
    idx = np.zeros(len(Q), dtype=np.int64)
    for lo in range(0, len(X), block):
        s = sq_dist(Q, X[lo : lo + block])
        j = s.argmin(1)
        v = s[np.arange(len(Q)), j]
        better = v < best
        best[better], idx[better] = v[better], lo + j[better]
    return idx


def kmeans_labels(X, C, block=8192):
    out = np.empty(len(X), dtype=np.int32)
    for lo in range(0, len(X), block):
        out[lo : lo + block] = sq_dist(X[lo : lo + block], C).argmin(1)
    return out


def kmeans_restate(X, C0, iters=10, order=None):
    """``kmeans2(X, C0, iters, minit="matrix", missing="warn")``: labels by the first nearest centroid, centroids the sum of
    their members in row order (``order``: in that order of the rows instead - the bound's perturbation) over their number, a
    cluster without members keeps its centroid.  Returns (centroids, labels of the last assignment, their counts)."""
    X, C = np.asarray(X, dtype=np.float64), np.array(C0, dtype=np.float64)
    rows = np.arange(len(X)) if order is None else np.asarray(order)
    for _ in range(iters):
        labels = kmeans_labels(X, C)
        sums = np.zeros_like(C)
        np.add.at(sums, labels[rows], X[rows])  # unbuffered: one row after the other
        counts = np.bincount(labels, minlength=len(C))
        live = counts > 0
        C[live] = sums[live] / counts[live, None]
    return C, labels, counts.astype(np.int64)


def trn_bound(X, n, W0=None, **kw):
    """ALLOW x the 4-ulp deviation of the restatement, relative to the extent (and the unperturbed nodes)."""
    W0 = trn_restate(X, n, **kw) if W0 is None else W0
    W4 = trn_restate(X, n, jitter_ulp=4, **kw)
    return ALLOW * float(np.abs(W4 - W0).max() / np.abs(X).max()), W0


def kmeans_bound(X, C0, iters, C_ref=None):
    """ALLOW x the deviation of the centroids under a shuffled summation order, relative to the extent."""
    C_ref = kmeans_restate(X, C0, iters)[0] if C_ref is None else C_ref
    C_sh = kmeans_restate(X, C0, iters, order=np.random.default_rng(5).permutation(len(X)))[0]
    return ALLOW * float(np.abs(C_sh - C_ref).max() / np.abs(X).max())


def uniform_cloud(N, d, seed):
    return np.random.default_rng(seed).random((N, d)) * np.array([3000.0, 2000.0, 800.0][:d])
