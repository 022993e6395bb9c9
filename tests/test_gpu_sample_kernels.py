"""Kernel-level tests of ``csrc/mvf_sample.hip`` through the raw C ABI on ``cuda:0``: ``mvf_trn``, ``mvf_nearest_rows``,
``mvf_kmeans``.  References and bounds come from tests/_sample_cases.py (proved against the real reference and SciPy by
tests/test_sample_kernel_refs.py): TRN nodes within 64 x the restatement's own 4-ulp deviation of the coordinate extent and
cell indices equal; k-means labels and counts equal to ``scipy.cluster.vq.kmeans2``'s exactly (uniform random coordinates, no
lattice: the condition under which the reference alone meets that) and centroids within 64 x the shuffled-summation deviation;
nearest rows equal to the brute-force argmin, the smallest index among equal distances.  Every output sits in front of a guard,
and two runs must give identical bits."""
import warnings

import numpy as np
import pytest
import torch

import _sample_cases as sc
from _kernel_scaffold import (MODES, called as _called, dev as _dev, guarded as _guarded, intact as _intact, ptr as _ptr,
                              same_bits as _same_bits, stream as _stream, take as _take, under as _under)

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def lib():
    from spateo_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


@pytest.fixture(scope="module")
def G():
    return sc.load()


class Trn:
    """One problem staged on the device: draws and schedules from the restatement's own helpers."""

    def __init__(self, X, n, seed=19491001, tmax=200, c=0):
        from spateo_amd import _lib

        self.X, self.n, self.d = np.ascontiguousarray(X, dtype=np.float64), n, X.shape[1]
        w_idx, p_idx = sc.trn_draws(self.X, n, seed, tmax)
        l, ep, kc = sc.trn_schedule(n, tmax, c=c)
        self.keep = [_dev(self.X, None), _dev(w_idx, torch.int64), _dev(p_idx, torch.int64), _dev(l, None), _dev(ep, None),
                     None if kc is None else _dev(kc, None)]
        self.W = _guarded(n * self.d, torch.float64)
        k = self.keep
        self.rec = _lib.TrnProblem(X=_ptr(k[0]), N=len(self.X), d=self.d, n=n, T=len(p_idx), w_idx=_ptr(k[1]), p_idx=_ptr(k[2]),
                                   l=_ptr(k[3]), ep=_ptr(k[4]), kc=_ptr(k[5]), W=_ptr(self.W))

    def nodes(self):
        return _take(self.W, self.n * self.d).reshape(self.n, self.d)


def _run_trn(lib, problems):
    from spateo_amd import _lib

    recs = (_lib.TrnProblem * len(problems))(*[p.rec for p in problems])
    assert lib.mvf_trn(recs, len(problems), _stream()) == 0, lib.mvf_last_error()
    _called()
    torch.cuda.synchronize()
    return [p.nodes() for p in problems]


def _nearest(lib, X, Q):
    X, Q = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
    Xd, Qd = _dev(X, None), _dev(Q, None)
    need = int(lib.mvf_nearest_rows_workspace_bytes(len(X), len(Q)))
    ws = _guarded(need // 8, torch.float64)
    idx = _guarded(len(Q), torch.int64)
    rc = lib.mvf_nearest_rows(_ptr(Xd), len(X), X.shape[1], _ptr(Qd), len(Q), _ptr(idx), _ptr(ws), need, _stream())
    assert rc == 0, lib.mvf_last_error()
    _called()
    torch.cuda.synchronize()
    _take(ws, need // 8)
    return _take(idx, len(Q))


def _rel(a, b, X):
    return float(np.abs(a - b).max() / np.abs(X).max())


# ----------------------------------------------------------------------------------------------------------------- mvf_trn
@pytest.mark.parametrize("tag", sc.TRN_TAGS)
def test_trn_golden_cases(lib, G, tag):
    X, n, seed, kw, W_ref, repeat = sc.golden_case(G, tag)
    pr = Trn(X, n, seed=seed, **kw)
    (W,) = _run_trn(lib, [pr])
    bound, _ = sc.trn_bound(X, n, W0=sc.trn_restate(X, n, seed=seed, **kw) if repeat else W_ref, seed=seed, **kw)
    a, b = (sc.sort_rows(W), sc.sort_rows(W_ref)) if repeat else (W, W_ref)
    err = _rel(a, b, X)
    print(f"trn {tag}: |W - W_ref| / extent = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.array_equal(np.sort(_nearest(lib, X, W)), np.sort(sc.nearest_restate(X, W_ref)))
    (W2,) = _run_trn(lib, [pr])
    assert np.array_equal(W2.view(np.uint64), W.view(np.uint64))


@pytest.mark.parametrize("n", tuple(sc.SERIES))
def test_trn_node_counts_around_the_wave_the_workgroup_and_the_cap(lib, G, n):
    X = sc.series_coordinates(n)
    (W,) = _run_trn(lib, [Trn(X, n, tmax=20)])
    W_ref, bound = G[f"s{n}_W"], sc.ALLOW * float(G[f"s{n}_dev"])
    err = _rel(W, W_ref, X)            # (the lower node ranks first on both sides: element for element, repeats or not)
    print(f"trn series n={n}: |W - W_ref| / extent = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.array_equal(_nearest(lib, X, W), sc.nearest_restate(X, W_ref))


def test_trn_batch_equals_single_launches_bit_for_bit(lib):
    shapes = [(400, 2, 33, 0), (1500, 3, 130, 0), (90, 1, 7, 0), (2500, 3, 1030, 0), (700, 2, 64, 0.001)]
    make = lambda: [Trn(sc.uniform_cloud(N, d, seed=N), n, tmax=6, c=c) for N, d, n, c in shapes]  # noqa: E731
    batch = _run_trn(lib, make())
    for (N, d, n, c), pr, Wb in zip(shapes, make(), batch):
        (W1,) = _run_trn(lib, [pr])
        assert np.array_equal(W1.view(np.uint64), Wb.view(np.uint64))
        bound, want = sc.trn_bound(pr.X, n, tmax=6, c=c)
        assert _rel(Wb, want, pr.X) <= bound, (N, d, n, c)


def test_trn_cutoff_moves_only_the_near_nodes(lib):
    X = sc.uniform_cloud(2000, 3, seed=4)
    n, c = 200, 0.01
    (W,) = _run_trn(lib, [Trn(X, n, tmax=10, c=c)])
    want = sc.trn_restate(X, n, tmax=10, c=c)
    bound, _ = sc.trn_bound(X, n, W0=want, tmax=10, c=c)
    assert _rel(W, want, X) <= bound
    assert _rel(want, sc.trn_restate(X, n, tmax=10), X) > 1e-6          # the cutoff matters at this size
    (W0,) = _run_trn(lib, [Trn(X, n, tmax=0)])                           # no steps: the start draw itself
    assert np.array_equal(W0, X[sc.trn_draws(X, n)[0]])


def test_trn_refusals_on_device_buffers(lib):
    from spateo_amd import _lib

    pr = Trn(sc.uniform_cloud(100, 2, seed=1), 8, tmax=2)
    for field, bad in (("n", 4097), ("d", 4), ("N", 0), ("T", -1), ("W", None), ("X", None), ("l", None)):
        rec = _lib.TrnProblem.from_buffer_copy(pr.rec)
        setattr(rec, field, bad)
        assert lib.mvf_trn((_lib.TrnProblem * 1)(rec), 1, _stream()) != 0 and b"mvf_trn" in lib.mvf_last_error(), field
    torch.cuda.synchronize()
    assert _intact(pr.W, 0)                     # nothing was launched


# --------------------------------------------------------------------------------------------------------- mvf_nearest_rows
@pytest.mark.parametrize("N", (1, 63, 64, 65, 1000, 100_003))
@pytest.mark.parametrize("d", (1, 2, 3))
def test_nearest_rows(lib, N, d):
    rng = np.random.default_rng(N * 10 + d)
    X = rng.random((N, d)) * 500
    if N >= 63:
        X[N // 2 :] = X[: N - N // 2][::-1]                              # every row twice: the smaller index must win
    n = 300 if N > 1000 else 70
    Q = rng.random((n, d)) * 500
    Q[::7] = X[rng.integers(0, N, len(Q[::7]))]                          # queries equal to a row (distance exactly 0)
    got = _nearest(lib, X, Q)
    want = sc.nearest_restate(X, Q)
    assert np.array_equal(got, want)
    if N >= 63:
        assert (X[got] == X[N - 1 - got]).all() and (got <= N - 1 - got).all()   # of the two copies of a row, the first
    assert np.array_equal(_nearest(lib, X, Q), got)


def test_nearest_rows_many_queries_and_refusals(lib):
    X = sc.uniform_cloud(5000, 3, seed=2)                                # two chunks of candidates x 1000 queries (4 workgroups)
    Q = sc.uniform_cloud(1000, 3, seed=3)
    assert np.array_equal(_nearest(lib, X, Q), sc.nearest_restate(X, Q))
    Xd, Qd, idx = _dev(X, None), _dev(Q, None), _guarded(1000, torch.int64)
    need = int(lib.mvf_nearest_rows_workspace_bytes(5000, 1000))
    ws = _guarded(need // 8, torch.float64)
    for kw in (dict(d=4), dict(N=0), dict(ws_bytes=need - 1), dict(ws=None), dict(idx=None)):
        a = dict(X=_ptr(Xd), N=5000, d=3, Q=_ptr(Qd), n=1000, idx=_ptr(idx), ws=_ptr(ws), ws_bytes=need)
        a.update(kw)
        rc = lib.mvf_nearest_rows(a["X"], a["N"], a["d"], a["Q"], a["n"], a["idx"], a["ws"], a["ws_bytes"], _stream())
        assert rc != 0 and b"mvf_nearest_rows" in lib.mvf_last_error(), kw
    torch.cuda.synchronize()
    assert _intact(idx, 0) and _intact(ws, 0)


# --------------------------------------------------------------------------------------------------------------- mvf_kmeans
def _kmeans(lib, X, C0, iters):
    X = np.ascontiguousarray(X, dtype=np.float64)
    N, d, n = len(X), X.shape[1], len(C0)
    Xd = _dev(X, None)
    C = _guarded(n * d, torch.float64)
    C[: n * d] = _dev(C0, None).reshape(-1)
    need = int(lib.mvf_kmeans_workspace_bytes(N, n))
    ws = _guarded(need // 8, torch.float64)
    labels, counts = _guarded(N, torch.int32), _guarded(n, torch.int64)
    rc = lib.mvf_kmeans(_ptr(Xd), N, d, _ptr(C), n, iters, _ptr(labels), _ptr(counts), _ptr(ws), need, _stream())
    assert rc == 0, lib.mvf_last_error()
    _called()
    torch.cuda.synchronize()
    _take(ws, need // 8)
    return _take(C, n * d).reshape(n, d), _take(labels, N), _take(counts, n)


# ------------------------------------------------------------------------------------------------------ calling conventions
CONVENTION_COVERS = {"mvf_trn": MODES, "mvf_nearest_rows": MODES, "mvf_kmeans": MODES}


def _trn_call(lib):   # two problems of one launch, one of them with a cutoff table
    return tuple(_run_trn(lib, [Trn(sc.uniform_cloud(N, d, seed=N), n, tmax=6, c=c) for N, d, n, c in ((400, 2, 33, 0), (700, 2, 64, 0.001))]))


def _nearest_call(lib, N):   # 4096 candidates need no workspace, 5000 run in two chunks through one
    return (_nearest(lib, sc.uniform_cloud(N, 3, seed=2), sc.uniform_cloud(300, 3, seed=3)),)


def _kmeans_call(lib, n):   # up to 64 centroids and above: the two assignment kernels
    X = sc.uniform_cloud(1000, 3, seed=n)
    return _kmeans(lib, X, X[:n].copy(), 3)


CONVENTION_CASES = {"mvf_trn": (_trn_call,), "mvf_nearest_rows:N4096": (_nearest_call, 4096), "mvf_nearest_rows:N5000": (_nearest_call, 5000),
                    "mvf_kmeans:n64": (_kmeans_call, 64), "mvf_kmeans:n65": (_kmeans_call, 65)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", list(CONVENTION_CASES))
def test_calling_conventions(lib, entry, mode):
    """The plain call's bits on a side stream behind poisoned inputs, at displaced pointers, and with the inputs unchanged."""
    fn, *args = CONVENTION_CASES[entry]
    plain, got = _under(mode, lambda: fn(lib, *args))
    assert len(plain) == len(got) and all(_same_bits(a, b) for a, b in zip(plain, got))


KMEANS = [(1, 1, 3), (65, 2, 10), (1000, 64, 10), (1000, 65, 10), (100_003, 257, 3), (20_000, 2000, 3)]


@pytest.mark.parametrize("N,n,iters", KMEANS)
@pytest.mark.parametrize("d", (2, 3))
def test_kmeans_against_kmeans2(lib, N, n, iters, d):
    from scipy.cluster.vq import kmeans2

    X = sc.uniform_cloud(N, d, seed=N + n + d)
    C0 = X[np.random.default_rng(n).choice(N, n, replace=False)].copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        C_ref, lab_ref = kmeans2(X, C0.copy(), iter=iters, minit="matrix")
    C, lab, counts = _kmeans(lib, X, C0, iters)
    assert np.array_equal(lab, lab_ref) and np.array_equal(counts, np.bincount(lab_ref, minlength=n))
    bound = sc.kmeans_bound(X, C0, iters, C_ref)
    err = _rel(C, C_ref, X)
    print(f"kmeans ({N}, {n}, d={d}): |C - C_ref| / extent = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    C2, lab2, counts2 = _kmeans(lib, X, C0, iters)
    assert np.array_equal(C2.view(np.uint64), C.view(np.uint64)) and np.array_equal(lab2, lab) and np.array_equal(counts2, counts)


def test_kmeans_empty_cluster_keeps_its_centroid(lib):
    from scipy.cluster.vq import kmeans2

    X = sc.uniform_cloud(3000, 3, seed=8)
    C0 = np.vstack([X[:6], [[1e6, -1e6, 1e6]], X[6:9]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        C_ref, lab_ref = kmeans2(X, C0.copy(), iter=5, minit="matrix")
    C, lab, counts = _kmeans(lib, X, C0, 5)
    assert counts[6] == 0 and np.array_equal(C[6], [1e6, -1e6, 1e6])
    assert np.array_equal(lab, lab_ref) and _rel(C, C_ref, X) <= sc.kmeans_bound(X, C0, 5, C_ref)


def test_kmeans_refusals_on_device_buffers(lib):
    X = sc.uniform_cloud(500, 2, seed=1)
    Xd, C = _dev(X, None), _guarded(8 * 2, torch.float64)
    need = int(lib.mvf_kmeans_workspace_bytes(500, 8))
    ws, labels, counts = _guarded(need // 8, torch.float64), _guarded(500, torch.int32), _guarded(8, torch.int64)
    for kw in (dict(d=0), dict(iters=0), dict(ws_bytes=need - 1), dict(ws=None), dict(labels=None), dict(counts=None), dict(N=-1)):
        a = dict(X=_ptr(Xd), N=500, d=2, C=_ptr(C), n=8, iters=3, labels=_ptr(labels), counts=_ptr(counts), ws=_ptr(ws), ws_bytes=need)
        a.update(kw)
        rc = lib.mvf_kmeans(a["X"], a["N"], a["d"], a["C"], a["n"], a["iters"], a["labels"], a["counts"], a["ws"], a["ws_bytes"],
                            _stream())
        assert rc != 0 and b"mvf_kmeans" in lib.mvf_last_error(), kw
    torch.cuda.synchronize()
    for t in (C, ws, labels, counts):
        assert _intact(t, 0)
