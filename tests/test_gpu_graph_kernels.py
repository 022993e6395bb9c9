"""Kernel-level tests of ``csrc/mvf_graph.hip`` and of ``mvf_pinv_diag_cached`` through the raw C ABI on ``cuda:0``, against the
NumPy restatements of tests/_graph_cases.py (tests/test_graph_kernel_refs.py proves those against the reference's own outputs).

``mvf_knn``: indices equal and distances bit-equal to the all-pairs restatement (the same IEEE operations in the same order) on
every cloud of ``_graph_cases.clouds()`` - n = k + 1, 257 and 1000 points across cell boundaries, a thin slab, all but two points in one cell,
points on a line in the plane, duplicates, a zero extent; k = 1, 3, 10, 64; d = 2, 3 -, two calls on workspaces of different
bytes give equal bits, refused shapes launch nothing.  ``mvf_graph_sssp``: bit-equal to the restated relaxation (which is
bit-equal to networkx's Dijkstra) on a path of 300 nodes (299 sweeps in the worst order: several batches), a star and three
components; m = 1, 64, 65, a repeated source, ld > m; sweeps queued after convergence change nothing and report zero; two calls
bit-equal.  ``mvf_pinv_diag_cached`` against ``mvf_pinv_diag`` on a cache that ``mvf_ublk_build`` made of the same points, at the
(n, m) edges of the existing test of ``mvf_pinv_diag``: bit-equal (one kernel behind the kernel value, and the cache holds
``kernel_value``'s bits).  Every output and workspace sits in front of guards."""
import numpy as np
import pytest
import torch

import _graph_cases as gc
import _solve_cases as sc
from _kernel_scaffold import (MODES, Out, Ws, called as _called, dev as _dev, guarded as _guarded, intact as _intact, kernel_cache,
                              ptr as _ptr, same_bits as _same_bits, settle as _settle, stream as _stream, take as _take, under as _under,
                              x4 as _x4)

pytestmark = pytest.mark.gpu

CLOUDS = gc.clouds()
BATCH = 32
_k = kernel_cache()
_REFS = {}


@pytest.fixture(scope="module")
def lib():
    from spateo_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def _err(lib):
    return lib.mvf_last_error().decode()


# ================================================================================================== raw helpers
def _knn(lib, X, k, ws_fill=0xA5):
    n, d = X.shape
    pts = _dev(X)
    idx, dist = _guarded(n * k, torch.int32), _guarded(n * k)
    need = int(lib.mvf_knn_workspace_bytes(n, d, k))
    assert need > 0 and need % 256 == 0
    ws = Ws(need, fill=ws_fill)
    rc = lib.mvf_knn(_ptr(pts), n, d, k, _ptr(idx), _ptr(dist), ws.ptr, need, _stream())
    assert rc == 0, _err(lib)
    _called()
    torch.cuda.synchronize()
    assert ws.guards_intact(), "wrote outside the workspace"
    return _take(idx, n * k).reshape(n, k), _take(dist, n * k).reshape(n, k)


def _sssp(lib, graph, sources, ld=None, extra_batches=1):
    """To the fixed point in batches of BATCH sweeps, then ``extra_batches`` more: (D (n, m), batches to the fixed point, the
    status blocks read)."""
    indptr, indices, weights, n = graph
    m = len(sources)
    ld = m if ld is None else ld
    dp, di, dw, ds = _dev(indptr, torch.int64), _dev(indices, torch.int32), _dev(weights), _dev(np.asarray(sources), torch.int32)
    dist, status = _guarded(n * ld), _guarded(4, torch.int64)
    blocks, init, done = [], 1, None
    while True:
        rc = lib.mvf_graph_sssp(_ptr(dp), _ptr(di), _ptr(dw), n, len(indices), _ptr(ds), m, _ptr(dist), ld, init, BATCH, _ptr(status),
                                _stream())
        assert rc == 0, _err(lib)
        _called()
        torch.cuda.synchronize()
        blocks.append(_take(status, 4).copy())
        init = 0
        if done is None and blocks[-1][0] == 0:
            done = len(blocks)
        if done is not None and len(blocks) >= done + extra_batches:
            break
        # a path has at most n - 1 edges: the batch that begins after sweep n - 1 lowers nothing
        assert done is not None or len(blocks) * BATCH < n + BATCH, "no fixed point within n sweeps"
    full = _take(dist, n * ld).reshape(n, ld)
    assert ld == m or bool((full[:, m:] == -1.2345e300).all()), "wrote beyond column m"
    return full[:, :m].copy(), done, blocks


def _expected(graph, sources):
    indptr, indices, weights, n = graph
    key = (n, len(indices), tuple(int(s) for s in sources))
    if key not in _REFS:
        _REFS[key] = gc.relax_restated(indptr, indices, weights, n, np.asarray(sources))[0]
    return _REFS[key]


GRAPHS = {"path": gc.path_graph(), "star": gc.star_graph(), "components": gc.two_components()}


# ================================================================================================== calling conventions
CONVENTION_COVERS = {"mvf_knn": MODES, "mvf_graph_sssp": MODES, "mvf_pinv_diag_cached": MODES}


def _conv_knn(lib):
    X, k = CLOUDS["257 (3-D)"]
    return _knn(lib, X, k)


def _conv_sssp(lib):
    """One call (the batches of _sssp synchronise between them): 64 sweeps reach the fixed point of this graph."""
    indptr, indices, weights, n = GRAPHS["components"]
    sources = [0, 100, 160]
    dp, di, dw, ds = _dev(indptr, torch.int64), _dev(indices, torch.int32), _dev(weights), _dev(np.asarray(sources), torch.int32)
    dist, status = _guarded(n * 3), _guarded(4, torch.int64)
    rc = lib.mvf_graph_sssp(_ptr(dp), _ptr(di), _ptr(dw), n, len(indices), _ptr(ds), 3, _ptr(dist), 3, 1, 64, _ptr(status), _stream())
    assert rc == 0, _err(lib)
    _called()
    torch.cuda.synchronize()
    D = _take(dist, n * 3).reshape(n, 3)
    assert _same_bits(D, _expected(GRAPHS["components"], sources)) and _take(status, 4)[1] == 0
    return D, _take(status, 4)[[1, 3]]


def _conv_pinv_cached(lib):
    return (_pinv_pair(lib, 129, 257, "float64", 0, plain=False),)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", ["mvf_knn", "mvf_graph_sssp", "mvf_pinv_diag_cached"])
def test_calling_conventions(lib, entry, mode):
    """The plain call's bits on a side stream behind poisoned inputs, at displaced pointers, and with the inputs unchanged.
    mvf_knn and mvf_graph_sssp must return while the inputs are still in flight; the solve in front of mvf_pinv_diag_cached
    synchronises its stream (include/mvf.h), so the side stream protects that helper's launches up to there."""
    fn = {"mvf_knn": _conv_knn, "mvf_graph_sssp": _conv_sssp, "mvf_pinv_diag_cached": _conv_pinv_cached}[entry]
    plain, got = _under(mode, lambda: fn(lib), synchronising=entry == "mvf_pinv_diag_cached")
    assert len(plain) == len(got) and all(_same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(plain, got))


# ================================================================================================== mvf_knn
@pytest.mark.parametrize("name", list(CLOUDS))
def test_knn_is_the_all_pairs_search_bit_for_bit(lib, name):
    X, k = CLOUDS[name]
    idx, dist = _knn(lib, X, k)
    ridx, rdist = gc.knn_restated(X, k)
    assert np.array_equal(idx, ridx), name
    assert _same_bits(dist, rdist), name
    again = _knn(lib, X, k, ws_fill=0x00)
    assert _same_bits(idx, again[0]) and _same_bits(dist, again[1])


def test_knn_on_the_golden_clouds_gives_sklearns_neighbours(lib):
    G = gc.load()
    for tag in gc.graph_tags(G):
        idx, dist = _knn(lib, G[f"{tag}_points"], int(G[f"{tag}_knn"]))
        order = np.argsort(idx, axis=1)
        assert np.array_equal(np.take_along_axis(idx, order, 1), G[f"{tag}_nbr_idx"]), tag
        mine = np.take_along_axis(dist, order, 1)
        print(f"{tag}: {int((mine != G[f'{tag}_nbr_dist']).sum())} of {mine.size} distances differ in bits from sklearn's")
        assert gc.ulps(mine, G[f"{tag}_nbr_dist"]) <= gc.D_ULP


def test_knn_refusals_launch_nothing(lib):
    X = np.random.default_rng(0).random((70, 3))
    pts = _dev(X)
    idx, dist = _guarded(70 * 64, torch.int32), _guarded(70 * 64)
    need = int(lib.mvf_knn_workspace_bytes(70, 3, 64))
    ws = Ws(need)
    base = dict(pts=_ptr(pts), n=70, d=3, k=10, idx=_ptr(idx), dist=_ptr(dist), ws=ws.ptr, nbytes=need)
    for kw, msg in ((dict(k=70), "bad shape"), (dict(k=71), "bad shape"), (dict(k=65), "bad shape"), (dict(k=0), "bad shape"),
                    (dict(d=4), "bad shape"), (dict(d=1), "bad shape"), (dict(n=10), "bad shape"), (dict(n=1 << 31), "bad shape"),
                    (dict(pts=None), "null pointer"), (dict(idx=None), "null pointer"), (dict(dist=None), "null pointer"),
                    (dict(ws=None), "null pointer"), (dict(ws=ws.ptr + 8), "256-byte aligned"), (dict(nbytes=255), "workspace too small")):
        a = dict(base, **kw)
        rc = lib.mvf_knn(a["pts"], a["n"], a["d"], a["k"], a["idx"], a["dist"], a["ws"], a["nbytes"], _stream())
        assert rc != 0 and "mvf_knn" in _err(lib) and msg in _err(lib), (kw, _err(lib))
    for n, d, k in ((70, 3, 70), (70, 3, 65), (70, 4, 10), (70, 3, 0)):
        assert lib.mvf_knn_workspace_bytes(n, d, k) == 0
    torch.cuda.synchronize()
    assert _intact(idx, 0) and _intact(dist, 0) and ws.guards_intact() and bool((ws.big == 0xA5).all())


# ================================================================================================== mvf_graph_sssp
@pytest.mark.parametrize("name,sources,ld", [("path", [299], None), ("path", [0, 150, 299, 150], 7), ("star", [0, 5], None),
                                             ("star", list(range(64)), None), ("star", list(range(65)), 72),
                                             ("components", [0, 100, 160, 0], None), ("components", list(range(0, 130, 2)), None)])
def test_sssp_is_the_restated_relaxation_bit_for_bit(lib, name, sources, ld):
    graph = GRAPHS[name]
    D, done, blocks = _sssp(lib, graph, sources, ld=ld, extra_batches=2)
    ref = _expected(graph, sources)
    assert np.array_equal(np.isinf(D), np.isinf(ref)) and _same_bits(D, ref), name
    print(f"{name} m {len(sources)}: fixed point read after {done} batches of {BATCH} sweeps")
    # sweeps queued after convergence: nothing lowered, nothing changed (D above was read after them), every sweep counted
    assert all(b[0] == 0 and b[1] == 0 and b[3] == BATCH for b in blocks[done - 1:])
    if name == "path" and sources == [299]:
        # several batches: the 64 nodes of a wave are relaxed by one instruction, every lane loading its neighbour's value before
        # any lane stores, so a distance crosses a wave's nodes one per sweep whatever the order of the waves: 63 sweeps lower
        # something at the least - batches 1 and 2 - and the first batch that reads zero is the third or a later one
        assert done >= 3, "the path was expected to cross several batches"
    again, _, _ = _sssp(lib, graph, sources, ld=ld, extra_batches=0)
    assert _same_bits(D, again)


def test_sssp_edgeless_graph_and_refusals(lib):
    n = 5
    indptr = np.zeros(n + 1, dtype=np.int64)
    dp, ds = _dev(indptr, torch.int64), _dev(np.array([2, 2]), torch.int32)
    dist, status = _guarded(n * 2), _guarded(4, torch.int64)
    rc = lib.mvf_graph_sssp(_ptr(dp), None, None, n, 0, _ptr(ds), 2, _ptr(dist), 2, 1, 3, _ptr(status), _stream())
    torch.cuda.synchronize()
    assert rc == 0, _err(lib)
    D = _take(dist, n * 2).reshape(n, 2)
    assert (D[2] == 0).all() and np.isinf(np.delete(D, 2, 0)).all() and list(_take(status, 4)) == [0, 0, 0, 3]
    dist2, status2 = _guarded(n * 2), _guarded(4, torch.int64)
    base = dict(ip=_ptr(dp), n=n, nnz=0, src=_ptr(ds), m=2, dist=_ptr(dist2), ld=2, sweeps=1, status=_ptr(status2))
    for kw, msg in ((dict(n=0), "bad shape"), (dict(m=0), "bad shape"), (dict(ld=1), "bad shape"), (dict(nnz=-1), "bad shape"),
                    (dict(sweeps=-1), "bad sweeps"), (dict(sweeps=65537), "bad sweeps"), (dict(ip=None), "null pointer"),
                    (dict(src=None), "null pointer"), (dict(dist=None), "null pointer"), (dict(status=None), "null pointer"),
                    (dict(nnz=3), "null pointer")):
        a = dict(base, **kw)
        rc = lib.mvf_graph_sssp(a["ip"], None, None, a["n"], a["nnz"], a["src"], a["m"], a["dist"], a["ld"], 1, a["sweeps"], a["status"],
                                _stream())
        assert rc != 0 and "mvf_graph_sssp" in _err(lib) and msg in _err(lib), (kw, _err(lib))
    torch.cuda.synchronize()
    assert _intact(dist2, 0) and _intact(status2, 0)


# ================================================================================================== mvf_pinv_diag_cached
PINV_N = [0, 1, 7, 8, 9, 257]   # (the sizes of mvf_pinv_diag's test; at n = 0 nothing is launched and no cache is read)


def _leverage_case(m, dtype):
    key = ("pinv", m, dtype)
    if key not in _REFS:
        _REFS[key] = sc.leverage_reference(sc.pinv_case(257, m), np.float32 if dtype == "float32" else np.float64)
    return _REFS[key]


def _pinv_pair(lib, m, n, dtype, lowrank, plain=True):
    """The decomposition of A = U^T U by mvf_solve_minnorm / _lr, the cache of the first n cells by mvf_ublk_build, then
    mvf_pinv_diag_cached - and, with ``plain``, mvf_pinv_diag on the same workspace: (cached[, regenerated])."""
    k, lc = _k(dtype), _leverage_case(m, dtype)
    pc = lc["pc"]
    Ad, Kd, Rd = _dev(lc["A"]), _dev(np.zeros((m, m))), _dev(np.ones((m, 3)))
    C, info, einfo = Out(m, 3), Out(1, dtype=torch.int32), Out(12)
    need = int((lib.mvf_solve_minnorm_lr_workspace_bytes if lowrank else lib.mvf_solve_minnorm_workspace_bytes)(m, 3))
    ws = Ws(need)
    _settle()
    if lowrank:
        rc = lib.mvf_solve_minnorm_lr(_ptr(Ad), _ptr(Kd), 0.0, 0.25, pc["rcond"], _ptr(Rd), m, 3, C.ptr, info.ptr, einfo.ptr, 60, 0, 0,
                                      ws.ptr, need, _stream())
    else:
        rc = lib.mvf_solve_minnorm(_ptr(Ad), _ptr(Kd), 0.0, sc.SHIFT, pc["rcond"], _ptr(Rd), m, 3, C.ptr, info.ptr, einfo.ptr, 60, 0,
                                   None, 0, ws.ptr, need, _stream())
    assert rc == 0, _err(lib)
    _called(synchronising=True)
    xa, ca = _x4(lc["X"][:n], lc["X"].dtype), _x4(lc["ctrl"], lc["ctrl"].dtype)
    nbytes = int(lib.mvf_ublk_bytes(n, m, k.cdtype))
    item = 4 if dtype == "float32" else 8
    cache = _guarded(nbytes // item, torch.float32 if dtype == "float32" else torch.float64, unit=16 // item)
    rc = lib.mvf_ublk_build(_ptr(xa), n, _ptr(ca), m, pc["beta"], _ptr(cache), nbytes, k.cdtype, _stream())
    assert rc == 0, _err(lib)
    out = Out(n)
    rc = lib.mvf_pinv_diag_cached(_ptr(cache), nbytes, n, m, pc["rcond"], lowrank, out.ptr, ws.ptr, need, k.cdtype, _stream())
    assert rc == 0, _err(lib)
    _called(synchronising=bool(lowrank))   # (include/mvf.h: the synchronisation on the lowrank path, as mvf_pinv_diag)
    torch.cuda.synchronize()
    assert int(info.host()[0]) == 0 and out.guards_intact() and ws.guards_intact() and _intact(cache, nbytes // item)
    if not plain:
        return out.host()
    ref = Out(n)
    rc = lib.mvf_pinv_diag(_ptr(xa), n, _ptr(ca), m, pc["beta"], pc["rcond"], lowrank, ref.ptr, ws.ptr, need, k.cdtype, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and ref.guards_intact(), _err(lib)
    return out.host(), ref.host()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("lowrank", [0, 1])
@pytest.mark.parametrize("m", [1, 127, 128, 129, 257])
def test_pinv_diag_cached_is_pinv_diag_bit_for_bit(lib, m, lowrank, dtype):
    for n in PINV_N:
        if n == 0:
            out = Out(1)
            rc = lib.mvf_pinv_diag_cached(None, 0, 0, m, 1e-10, lowrank, out.ptr, None, 0, _k(dtype).cdtype, _stream())
            torch.cuda.synchronize()
            assert rc == 0 and out.untouched() and out.guards_intact(), _err(lib)
            continue
        cached, regenerated = _pinv_pair(lib, m, n, dtype, lowrank)
        assert np.isfinite(cached).all() and _same_bits(cached, regenerated), (m, n, lowrank, dtype)


def test_pinv_diag_cached_refusals(lib):
    k = _k("float64")
    out, cache = Out(9), _guarded(256 * 128)
    ws = Ws(int(lib.mvf_solve_minnorm_lr_workspace_bytes(5, 3)))
    nbytes = int(lib.mvf_ublk_bytes(9, 5, k.cdtype))
    for args, msg in (((_ptr(cache), nbytes, 9, 0, 1e-10, 1), "m > 0"), ((None, nbytes, 9, 5, 1e-10, 1), "null pointer"),
                      ((_ptr(cache), nbytes - 8, 9, 5, 1e-10, 1), "smaller than mvf_ublk_bytes"),
                      ((_ptr(cache), nbytes, 9, 5, -1.0, 1), "bad rcond"), ((_ptr(cache), nbytes, 9, 5, 1e-10, 1), "no finished decomposition")):
        rc = lib.mvf_pinv_diag_cached(*args, out.ptr, ws.ptr, ws.nbytes, k.cdtype, _stream())
        torch.cuda.synchronize()
        assert rc != 0 and "mvf_pinv_diag_cached" in _err(lib) and msg in _err(lib), (msg, _err(lib))
    assert out.untouched() and out.guards_intact() and ws.guards_intact()
