"""Kernel-level tests of ``csrc/mvf_shape.hip`` through the raw C ABI on ``cuda:0``, on the cases of tests/_shape_cases.py against
the golden (the reference's own outputs; tests/test_shape_kernel_refs.py proves the conditions relied on here).

Exact: ``point_voxel``, the kept voxel ids, the counts, ``n_dropped`` and ``n_overlap`` (0 in every case).  The rank equals the
reference's in every subspace that is not marginal.  ``cosine`` within max(64 x the restatement's summation-order deviation,
16 ulp).  ``dist`` as a relative deviation per subspace: within 64 x the case's maximum gelsd-vs-gelss deviation (floor 16 ulp)
with the marginal subspaces - at most 5 % of a case - left out of this one comparison; on the realistic cases (D, D2) nothing is
left out and the median is bounded by 64 x the median swap deviation as well.  Two calls, the second on a workspace of other
bytes, return the same bytes; every output and the workspace sit in front of guards that must stay untouched; refusals launch
nothing."""
import ctypes

import numpy as np
import pytest
import torch

import _shape_cases as sc
from _kernel_scaffold import (MODES, Ws, called as _called, dev as _dev, guarded as _guarded, intact as _intact, ptr as _ptr,
                              same_bits as _same_bits, stream as _stream, take as _take, under as _under)

pytestmark = pytest.mark.gpu

G = sc.load()
CASE_ORDERS = [(name, order) for name in sc.NAMES for order in sc.CASES[name]["orders"]]
OUTS = (("point_voxel", torch.int32), ("voxel", torch.int32), ("count", torch.int64), ("cosine", torch.float64),
        ("dist", torch.float64), ("rank", torch.int32), ("sv", torch.float64), ("counts", torch.int64))


@pytest.fixture(scope="module")
def lib():
    from spateo_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def _sizes(n, nsub):
    cap = max(min(nsub ** 3, n // 2), 1)
    return dict(point_voxel=n, voxel=cap, count=cap, cosine=cap, dist=cap, rank=cap, sv=2 * cap, counts=3)


def _raw(lib, pcs, nsub, order, ws_fill=0xA5):
    """One call on guarded buffers: {name: the whole host array} with the guards checked."""
    n = len(pcs)
    lo, hi = sc.tables(pcs, nsub)
    pts, dlo, dhi = _dev(pcs), _dev(lo), _dev(hi)
    g = (ctypes.c_double * 3)(*np.mean(pcs, axis=0))
    sizes = _sizes(n, nsub)
    bufs = {name: _guarded(sizes[name], dt) for name, dt in OUTS}
    need = int(lib.mvf_shape_descriptors_workspace_bytes(n, nsub))
    assert need > 0 and need % 256 == 0
    ws = Ws(need, fill=ws_fill)
    rc = lib.mvf_shape_descriptors(_ptr(pts), n, _ptr(dlo), _ptr(dhi), nsub, sc.ORDERS[order], g, *[_ptr(bufs[name]) for name, _ in OUTS],
                                   ws.ptr, need, _stream())
    assert rc == 0, lib.mvf_last_error()
    _called()
    torch.cuda.synchronize()
    assert ws.guards_intact(), "wrote outside the workspace"
    return {name: _take(bufs[name], sizes[name]) for name, _ in OUTS}


CONVENTION_COVERS = {"mvf_shape_descriptors": MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,order", [("E_k63", "cubic"), ("E_cubic", "cubic"), ("A", "cubic")])   # 1 voxel (twice); 4^3 voxels
def test_calling_conventions(lib, name, order, mode):
    """The plain call's bits on a side stream behind poisoned inputs, at displaced pointers, and with the inputs unchanged."""
    case = sc.CASES[name]
    plain, got = _under(mode, lambda: _raw(lib, case["pcs"], case["n"], order))
    assert all(_same_bits(plain[k], got[k]) for k, _ in OUTS)


def _kept(raw):
    m = int(raw["counts"][0])
    return m, {k: (raw[k][: 2 * m].reshape(m, 2) if k == "sv" else raw[k][:m]) for k in ("voxel", "count", "cosine", "dist", "rank", "sv")}


@pytest.mark.parametrize("name,order", CASE_ORDERS)
def test_case_against_the_golden_and_bit_stable(lib, name, order):
    case, key, r = sc.CASES[name], f"{name}_{order}", sc.restated(name, order)
    raw = _raw(lib, case["pcs"], case["n"], order)
    m, out = _kept(raw)
    # exact
    assert np.array_equal(raw["point_voxel"], r["point_voxel"])
    assert m == len(G[f"{key}_voxel"]) and np.array_equal(out["voxel"], G[f"{key}_voxel"]) and np.array_equal(out["count"], G[f"{key}_count"])
    assert int(raw["counts"][1]) == r["n_dropped"] == int((r["point_voxel"] < 0).sum()) and int(raw["counts"][2]) == 0
    # rank where the reference's decision is not marginal
    marg = sc.marginal(G[f"{key}_sv"])
    assert np.array_equal(out["rank"][~marg], G[f"{key}_rank"][~marg])
    assert (out["sv"][:, 0] > 0).all() and (out["sv"][:, 1] > sc.EPS).all() and (out["sv"][:, 1] <= 1.0).all()
    # cosine, dist
    vs = G[f"{key}_vs"]
    cos_dev = float((np.abs(out["cosine"] - vs[:, 0]) / np.abs(vs[:, 0])).max())
    cos_bound = sc.cosine_bound(name, order)
    dev = np.abs(out["dist"] - vs[:, 1]) / np.abs(vs[:, 1])
    bound, median_bound, keep = sc.dist_bounds(G, name, order)
    swap = sc.swap_deviation(G, name, order)
    print(f"shape {key} n={len(case['pcs'])} nsub={case['n']} kept={m} marginal={int(marg.sum())} left out={int((~keep).sum())}: "
          f"cosine {cos_dev:.3e} (bound {cos_bound:.3e}), dist max {dev[keep].max():.3e} (bound {bound:.3e}, swap max {swap.max():.3e}), "
          f"median {np.median(dev):.3e} (bound {median_bound if median_bound is None else format(median_bound, '.3e')}, swap median "
          f"{np.median(swap):.3e}), rank mismatches in marginal subspaces {int((out['rank'][marg] != G[f'{key}_rank'][marg]).sum())}")
    assert cos_dev <= cos_bound
    assert dev[keep].max() <= bound
    assert median_bound is None or np.median(dev) <= median_bound
    # the same bytes again, whatever the workspace held
    again = _raw(lib, case["pcs"], case["n"], order, ws_fill=0x00)
    for k, _ in OUTS:
        live = raw[k] if k in ("point_voxel", "counts") else raw[k][: (2 * m if k == "sv" else m)]
        assert np.array_equal(live.view(np.uint8), again[k][: len(live)].view(np.uint8)), k


def test_a_cloud_without_a_kept_voxel_and_a_single_point(lib):
    """Nothing to fit: every voxel holds one point at most (counts[0] == 0, no per-voxel output written); n == 1 has no
    per-voxel capacity at all."""
    pcs = np.array([[0.0, 0.0, 0.0], [1.5, 1.5, 1.5], [2.5, 0.5, 1.5], [4.0, 4.0, 4.0]])   # (the last one on the upper faces)
    raw = _raw(lib, pcs, 4, "cubic")
    assert list(raw["counts"]) == [0, 1, 0] and list(raw["point_voxel"]) == [0, 21, 18, -1]
    assert (raw["voxel"] == -12345).all() and (raw["dist"] == -1.2345e300).all()
    raw = _raw(lib, pcs[:1], 3, "linear")
    assert list(raw["counts"]) == [0, 1, 0] and list(raw["point_voxel"]) == [-1]


def test_refusals_launch_nothing(lib):
    case = sc.CASES["E_k63"]
    pcs, n = case["pcs"], len(case["pcs"])
    lo, hi = sc.tables(pcs, 2)
    pts, dlo, dhi = _dev(pcs), _dev(lo), _dev(hi)
    g = (ctypes.c_double * 3)(*np.mean(pcs, axis=0))
    sizes = _sizes(n, 2)
    bufs = {name: _guarded(sizes[name], dt) for name, dt in OUTS}
    need = int(lib.mvf_shape_descriptors_workspace_bytes(n, 2))
    ws = Ws(need)
    base = dict(pts=_ptr(pts), n=n, lo=_ptr(dlo), hi=_ptr(dhi), nsub=2, order=3, g=g, ws=ws.ptr, ws_bytes=need,
                **{name: _ptr(bufs[name]) for name, _ in OUTS})
    for kw, msg in ((dict(nsub=0), b"bad shape"), (dict(nsub=129), b"bad shape"), (dict(n=0), b"bad shape"), (dict(n=-3), b"bad shape"),
                    (dict(n=1 << 31), b"bad shape"), (dict(order=0), b"bad order"), (dict(order=4), b"bad order"),
                    (dict(pts=None), b"null pointer"), (dict(lo=None), b"null pointer"), (dict(hi=None), b"null pointer"),
                    (dict(g=None), b"null pointer"), (dict(point_voxel=None), b"null pointer"), (dict(counts=None), b"null pointer"),
                    (dict(dist=None), b"null pointer"), (dict(voxel=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                    (dict(ws=ws.ptr + 8), b"256-byte aligned"), (dict(ws_bytes=need - 1), b"workspace too small")):
        a = dict(base, **kw)
        rc = lib.mvf_shape_descriptors(a["pts"], a["n"], a["lo"], a["hi"], a["nsub"], a["order"], a["g"], *[a[name] for name, _ in OUTS],
                                       a["ws"], a["ws_bytes"], _stream())
        assert rc != 0 and b"mvf_shape_descriptors" in lib.mvf_last_error() and msg in lib.mvf_last_error(), (kw, lib.mvf_last_error())
    torch.cuda.synchronize()
    assert all(_intact(bufs[name], 0) for name, _ in OUTS) and ws.guards_intact()
    assert bool((ws.big == 0xA5).all())
