"""Kernel-level tests of ``mvf_assign_topk`` (``csrc/mvf_assign.hip``: the reference's ``sparse_calculation_mode``) through the raw
C ABI on ``cuda:0`` in both cell dtypes.  The reference is ``_assign_edge_cases.pair_reference`` on the operands the device
itself prepared (read back), so float32 storage is held to the float64 bound; the checker is ``_assign_topk_case.check``.
Every call runs on a NaN-filled, guarded workspace with a guard behind every output and is made twice (same bits, ``rows``
included).

Shapes (na, nb, k) sit on the kernel's own edges: the smallest call, the clamp to NA, the tile edges either way, a list that
is exactly full, a single column, 4 and 64 row splits (the merge of 64 lists), 18 column splits in pass 2.  The orderings
stress the per-column lists: every row beats the last (an insertion per row), strictly falling values (none after the first
k), all winners in the last split's last partial tile, exact duplicate A cells 64 rows apart on either side of a split
boundary (the row-ascending rule decides), a block of far columns (all-zero lists: rows 0 .. k - 1).

No bound is fitted to what the device returned."""
import numpy as np
import pytest
import torch

import _assign_case as ac
import _assign_edge_cases as ec
import _assign_topk_case as tk
from _align_kernel_scaffold import assign as _assign, device_case as _case, layer_struct as _layer_array, watch_case as _watch_case
from _kernel_scaffold import (DEV, DTYPES, GUARD, called as _called, guarded as _guarded, intact as _intact,
                              nan_workspace as _nan_workspace, same_bits as _same_bits, under as _under, written as _written)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (5, 3, 64), (63, 65, 1), (64, 64, 64), (65, 63, 8), (129, 1, 16), (200, 50, 8), (4097, 10, 4), (300, 1100, 8)]
ORDERINGS = ("rising", "falling", "last_tile", "duplicates", "far_block")
OUT = ("K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2", "PXB", "scalar", "rows", "vals")


def _shape_case(na, nb):
    layers = [("kl", "gauss", None, 20)] if (na + nb) % 2 else [("cos", "cos", None, 17), ("euc", "gauss", None, 24)]
    return ec.make_case(f"topk-{na}x{nb}", na, nb, layers, far="some")


def _ordering_case(kind, na, nb):
    """Inputs whose per-column order of u = e2 m q over the A rows is known: the A cells sit within 1e-5 of one point with
    one layer profile, so e2 q is the same to ~1e-5 in every row and alpha (= m, SigmaDiag = 0), which moves by >= 2e-3 from
    row to row, alone orders the rows."""
    c = ec.make_case(f"topk-{kind}-{na}x{nb}", na, nb, [("kl", "gauss", None, 20)], far="some" if kind == "far_block" else "none",
                     sigma2=0.5)
    rng = np.random.default_rng(7)
    if kind in ("rising", "falling", "last_tile"):
        c["XA"] = 1e-5 * rng.standard_normal(c["XA"].shape)
        c["XB"] = 0.3 * rng.standard_normal(c["XB"].shape)
        c["layers_A"] = [np.tile(c["layers_A"][0][:1], (na, 1))]
        c["SigmaDiag"] = np.zeros(na)
        i = np.arange(na)
        step = 1.05 if na <= 400 else 1.002          # (1.002^4097 = 3.6e3, 1.05^300 = 2.3e6: far from overflow)
        if kind == "rising":
            c["alpha"] = step ** i
        elif kind == "falling":
            c["alpha"] = step ** (-i.astype(np.float64))
        else:   # only the last 8 rows carry weight: the last partial tile (and, at 4097 rows, the 7 rows in front of it)
            c["alpha"] = np.where(i >= na - 8, 1.0 + 0.01 * i, 1e-6)
    elif kind == "duplicates":
        # rows i and i + 64 identical in every input, for the last 8 rows i of the first tile: the pair straddles the boundary
        # between the first two tiles, which is one between two row splits.  Column j is a near copy of the j-th pair's cell,
        # so the pair heads its list
        src = np.arange(ec.TILE - 8, ec.TILE)
        dst = src + ec.TILE
        c["XA"][dst] = c["XA"][src]
        c["layers_A"][0][dst] = c["layers_A"][0][src]
        c["alpha"][dst], c["SigmaDiag"][dst] = c["alpha"][src], c["SigmaDiag"][src]
        n = min(nb, len(src))
        c["XB"][:n] = c["XA"][src[:n]] + 0.01 * rng.standard_normal((n, c["XA"].shape[1]))
        c["layers_B"][0][:n] = c["layers_A"][0][src[:n]]
        c["pairs"] = list(zip(src.tolist(), dst.tolist()))
    elif kind == "far_block":   # the far columns first, as one block
        order = np.concatenate([c["far"], np.setdiff1d(np.arange(nb), c["far"])])
        c["XB"], c["layers_B"] = c["XB"][order], [L[order] for L in c["layers_B"]]
        c["far"] = np.arange(len(c["far"]))
    return c


def _topk(dc, k, ws=None, ws_bytes=None):
    """mvf_assign_topk through the raw ABI on the current stream; guards behind every output and the workspace (default:
    exactly mvf_assign_topk_workspace_bytes, NaN-filled).  Returns host arrays."""
    from spateo_amd import _lib

    kk, na, nb = dc.k, dc.na, dc.nb
    ke = min(k, na)
    sizes = {"K_NA": na, "K_NB": nb, "K_NA_spatial": na, "K_NA_sigma2": na, "PXB": 3 * na, "scalar": 1, "vals": nb * ke}
    bufs = {q: _guarded(n) for q, n in sizes.items()}
    rows = torch.full((nb * ke + GUARD,), -7, dtype=torch.int32, device=DEV)
    need = int(kk.lib.mvf_assign_topk_workspace_bytes(na, nb, k))
    assert need > int(kk.lib.mvf_assign_workspace_bytes(na, nb)) and need % 8 == 0
    if ws is None:
        ws, ws_bytes = _nan_workspace(need), need
    c = dc.case
    _lib.check(kk.lib.mvf_assign_topk(dc.xa4.data_ptr(), na, dc.xb4.data_ptr(), nb, _layer_array(dc), len(dc.layers),
                                      dc.mm.data_ptr(), float(c["sigma2"]), float(c["sigma2_variance"]), float(dc.outlier), k,
                                      *(bufs[q].data_ptr() for q in ("K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2", "PXB", "scalar")),
                                      rows.data_ptr(), bufs["vals"].data_ptr(), ws.data_ptr(), int(ws_bytes), kk.cdtype,
                                      kk._stream()), "mvf_assign_topk")
    _called()
    torch.cuda.synchronize()
    for q, n in sizes.items():
        assert _intact(bufs[q], n), f"{dc.name}: wrote behind {q}[{n}]"
        assert _written(bufs[q], n), f"{dc.name}: left an element of {q} unwritten"
    assert bool((rows[nb * ke:] == -7).all()), f"{dc.name}: wrote behind rows"
    assert bool((rows[: nb * ke] != -7).all()), f"{dc.name}: left an element of rows unwritten"
    assert _intact(ws, ws_bytes // 8), f"{dc.name}: wrote behind the workspace"
    out = {q: bufs[q][:n].cpu().numpy() for q, n in sizes.items()}
    out["PXB"], out["scalar"] = out["PXB"].reshape(na, 3), out["scalar"].reshape(())
    out["vals"], out["rows"] = out["vals"].reshape(nb, ke), rows[: nb * ke].cpu().numpy().reshape(nb, ke)
    for q in OUT:
        assert np.isfinite(out[q]).all(), f"{dc.name}: {q} is not finite"
    return out


def _same(a, b):
    for q in OUT:
        x, y = np.ascontiguousarray(a[q]), np.ascontiguousarray(b[q])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), q


CONVENTION_COVERS = {"mvf_assign_topk": ("side_stream", "inputs")}


@pytest.mark.parametrize("mode", ["side_stream", "inputs"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("na,nb", [(65, 63), (50, 4417)])   # one tile pair; the split plan
def test_calling_conventions(na, nb, dtype, mode):
    """The plain call's bits with the call on a side stream - the case's operands are made when the case is built, so the
    outputs and the workspace, not the inputs, are in flight there: a launch on another stream is overwritten by their fill -,
    and with every operand unchanged by the call."""
    dc = _case((na, nb), lambda: _shape_case(na, nb), dtype)

    def call():
        _watch_case(dc)
        return _topk(dc, 8)

    plain, got = _under(mode, call)
    _same(plain, got)


def _check(dc, got, k):
    """The checker against pair_reference on the device's own operands at the float64 bound, the dense quantities against
    the reference, the far columns."""
    ref = dc.reference()
    assert "P" in ref
    tk.check(got, ref["P"], dc.xb[:, :3], k, ac.F64_TOL, what=f"{dc.name} {dc.dtype} k {k} plan {ec.plan(dc.na, dc.nb)}")
    for q in ("K_NA_spatial", "K_NA_sigma2", "scalar"):
        top = float(np.abs(ref[q]).max())
        dev = float(np.abs(got[q] - ref[q]).max() / top) if top > 0 else float(np.abs(got[q]).max())
        print(f"  {dc.name}: dense {q} {dev:.1e}")
        assert dev <= ac.F64_TOL, (dc.name, q, dev)
    far = dc.case["far"]
    ke = min(k, dc.na)
    assert not got["K_NB"][far].any() and not got["vals"][far].any()
    assert np.array_equal(got["rows"][far], np.tile(np.arange(ke, dtype=np.int32), (len(far), 1)))   # all-zero lists
    return ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("na,nb,k", SHAPES)
def test_shapes_on_the_kernels_edges(dtype, na, nb, k):
    dc = _case((na, nb), lambda: _shape_case(na, nb), dtype)
    got = _topk(dc, k)
    _check(dc, got, k)
    _same(got, _topk(dc, k))
    if k >= na:   # the clamp: every entry kept, so the sums are the dense ones
        ref = dc.reference()
        assert got["rows"].shape == (nb, na)
        for q in ("K_NA", "K_NB", "PXB"):
            assert np.abs(got[q] - ref[q]).max() <= ac.F64_TOL * np.abs(ref[q]).max(), q


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ORDERINGS)
@pytest.mark.parametrize("na,nb,k", [(200, 50, 8), (4097, 10, 4)])
def test_orderings_that_stress_the_lists(dtype, kind, na, nb, k):
    dc = _case((kind, na, nb), lambda: _ordering_case(kind, na, nb), dtype)
    got = _topk(dc, k)
    _check(dc, got, k)
    _same(got, _topk(dc, k))
    rows = got["rows"]
    if kind == "rising":      # the last k rows, the last first
        assert np.array_equal(rows, np.tile(np.arange(na - 1, na - 1 - k, -1, dtype=np.int32), (nb, 1)))
    elif kind == "falling":   # the first k rows
        assert np.array_equal(rows, np.tile(np.arange(k, dtype=np.int32), (nb, 1)))
    elif kind == "last_tile":
        lo = ec.split_tiles(-(-na // ec.TILE), ec.plan(na, nb)[2], ec.plan(na, nb)[2] - 1)[0] * ec.TILE
        assert rows.min() >= na - 8 >= lo > 0 and na % ec.TILE   # the last row split, which ends in a partial tile
    elif kind == "duplicates":
        # equal bits for the two rows of a pair in every column: next to each other, the smaller row first; a pair cut by
        # the end of the list keeps the smaller row
        vals, both = got["vals"], 0
        rt, _, rs, _ = ec.plan(na, nb)
        assert ec.split_tiles(rt, rs, 0) == (0, 1) and ec.split_tiles(rt, rs, 1)[0] == 1   # tiles 0 and 1: two row splits
        for j in range(nb):
            lst = [int(i) for i in rows[j]]
            for lo, hi in dc.case["pairs"]:
                if vals[j, -1] == 0.0 and (lo in lst or hi in lst) and vals[j, lst.index(lo if lo in lst else hi)] == 0.0:
                    continue   # (a tie among zeros is resolved by the row alone, whatever the pairs)
                if hi in lst:
                    assert lo in lst and lst.index(hi) == lst.index(lo) + 1, (j, lo, hi, lst)
                    assert vals[j, lst.index(hi)] == vals[j, lst.index(lo)], (j, lo, hi)
                    both += 1
                elif lo in lst:
                    assert lst.index(lo) == len(lst) - 1, (j, lo, hi, lst)
        print(f"  duplicates {na}x{nb}: {both} pairs inside the lists")
        assert both >= min(nb, len(dc.case["pairs"]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_contents_and_size_do_not_matter(dtype):
    """A larger workspace, zero-filled, NaN-filled and holding a larger call's partial lists: the same bits."""
    ds = _case((200, 50), lambda: _shape_case(200, 50), dtype)
    dl = _case((300, 1100), lambda: _shape_case(300, 1100), dtype)
    kk = ds.k
    size = max(int(kk.lib.mvf_assign_topk_workspace_bytes(ds.na, ds.nb, 8)),
               int(kk.lib.mvf_assign_topk_workspace_bytes(dl.na, dl.nb, 64))) + 4096
    ws = _guarded(size // 8)
    ws[: size // 8] = 0.0
    zero = _topk(ds, 8, ws=ws, ws_bytes=size)
    ws[: size // 8] = float("nan")
    nan = _topk(ds, 8, ws=ws, ws_bytes=size)
    _topk(dl, 64, ws=ws, ws_bytes=size)
    stale = _topk(ds, 8, ws=ws, ws_bytes=size)
    tight = _topk(ds, 8)
    for other in (nan, stale, tight):
        _same(zero, other)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_call_on_another_stream_gives_the_same_bits(dtype):
    dc = _case((4097, 10), lambda: _shape_case(4097, 10), dtype)
    first = _topk(dc, 4)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        assert dc.k._stream() == stream.cuda_stream != torch.cuda.default_stream(DEV).cuda_stream
        other = _topk(dc, 4)
    torch.cuda.synchronize()
    _same(first, other)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("na,nb,k", [(200, 50, 8), (300, 1100, 64)])
def test_the_dense_quantities_are_mvf_assigns(dtype, na, nb, k):
    """K_NA_spatial, K_NA_sigma2 and scalars[0] against mvf_assign on the same inputs: REF_TOL; whether the bits are equal is
    printed.  The sparse sums lie below the dense ones (entries >= 0 were left out)."""
    dc = _case((na, nb), lambda: _shape_case(na, nb), dtype)
    got = _topk(dc, k)
    dc.name = f"topk-{na}x{nb}"
    plain = _assign(_Plain(dc))
    for q in ("K_NA_spatial", "K_NA_sigma2", "scalar"):
        top = float(np.abs(plain[q]).max())
        dev = float(np.abs(got[q] - plain[q]).max() / top)
        print(f"  {na}x{nb} k {k} {dtype}: {q} against mvf_assign {dev:.1e}, equal bits: {_same_bits(got[q], plain[q])}")
        assert dev <= ec.REF_TOL, (q, dev)
    assert np.all(got["K_NA"] <= plain["K_NA"] * (1 + 1e-12)) and np.all(got["K_NB"] <= plain["K_NB"] * (1 + 1e-12))


class _Plain:
    """What test_gpu_assign_kernels._assign reads of a device case (its workspace-size assertion included)."""

    def __init__(self, dc):
        for q in ("k", "na", "nb", "layers", "case", "xa4", "xb4", "mm", "outlier", "name"):
            setattr(self, q, getattr(dc, q))
