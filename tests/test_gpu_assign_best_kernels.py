"""Kernel-level tests of ``mvf_assign_best`` (``csrc/mvf_assign.hip``: the best partner of every row and column of ``P``, without
``P``) through the raw C ABI on ``cuda:0`` in both cell dtypes.  The reference is the dense ``P`` of
``_assign_edge_cases.pair_reference`` on the operands the device itself prepared (read back), so float32 storage is held to the
float64 bound - the one tests/test_gpu_assign_kernels.py holds ``mvf_assign_dense``'s ``P`` to; the checker is
``_assign_best_case.check``.  Every call runs on a NaN-filled, guarded workspace of exactly the size the library asks for, with
a guard behind every output, and is made twice (same bits).

Shapes sit on the kernels' own edges: the dense shapes of ``_assign_edge_cases`` (one cell, one row, one column, the tile edge
either way), 63 / 64 / 65 / 129 rows against 1 / 65 / 200 columns (tile and lane edges), 64 row splits and 64 column splits,
1 / 16 / 17 features (the k-step), four layers, a label layer, 2-D.  The planted ties - far A and B cells (all-zero rows and
columns, whose nearest partner lies in another tile and split than index 0) and copies of cells in another lane, another tile
and another split - are where the two rules alone decide.

No bound is fitted to what the device returned."""
import numpy as np
import pytest
import torch

import _assign_best_case as bc
import _assign_case as ac
import _assign_edge_cases as ec
from _align_kernel_scaffold import (device_case as _case, kernels as _k, LabelCase as _LabelCase, layer_struct as _layer_array,
                                    watch_case as _watch_case)
from _kernel_scaffold import (DEV, DTYPES, GUARD, SENTINEL, called as _called, guarded as _guarded, intact as _intact,
                              nan_workspace as _nan_workspace, under as _under, written as _written)

pytestmark = pytest.mark.gpu

EDGE_SHAPES = [(na, nb) for na in (63, 64, 65, 129) for nb in (1, 65, 200)]
SPLIT_SHAPES = [(4417, 50), (50, 4417)]
SHAPES = list(ec.DENSE_SHAPES) + EDGE_SHAPES + SPLIT_SHAPES
TIE_SHAPE = bc.TIE_SHAPE
UNSET = -7


def _shape_case(na, nb):
    layers = [("kl", "gauss", None, 20)] if (na + nb) % 2 else [("cos", "cos", None, 17), ("euc", "gauss", None, 24)]
    return ec.make_case(f"best-{na}x{nb}", na, nb, layers, far="some")


def _best(dc, rows=True, cols=True, ws=None, ws_bytes=None, struct=None, nlayers=None):
    """mvf_assign_best through the raw ABI on the current stream; guards behind every output and the workspace (default:
    exactly mvf_assign_best_workspace_bytes, NaN-filled).  Returns host arrays."""
    from spateo_amd import _lib

    kk, na, nb = dc.k, dc.na, dc.nb
    need = int(kk.lib.mvf_assign_best_workspace_bytes(na, nb))
    assert need > int(kk.lib.mvf_assign_workspace_bytes(na, nb)) and need % 8 == 0
    if ws is None:
        ws, ws_bytes = _nan_workspace(need), need
    bufs = {}
    for on, name, n in ((rows, "row", na), (cols, "col", nb)):
        if on:
            bufs[f"{name}_idx"] = torch.full((2 * n + GUARD,), UNSET, dtype=torch.int32, device=DEV)
            bufs[f"{name}_val"] = _guarded(n)
    ptr = lambda q: bufs[q].data_ptr() if q in bufs else None  # noqa: E731
    c = dc.case if hasattr(dc, "case") else dc.c
    arr = _layer_array(dc) if struct is None else struct
    _lib.check(kk.lib.mvf_assign_best(dc.xa4.data_ptr(), na, dc.xb4.data_ptr(), nb, arr, len(dc.layers) if nlayers is None else nlayers,
                                      dc.mm.data_ptr(), float(c["sigma2"]), float(c["sigma2_variance"]), float(dc.outlier),
                                      ptr("row_idx"), ptr("row_val"), ptr("col_idx"), ptr("col_val"), ws.data_ptr(), int(ws_bytes),
                                      kk.cdtype, kk._stream()), "mvf_assign_best")
    _called()
    torch.cuda.synchronize()
    out = {}
    for on, name, n, key, vkey in ((rows, "row", na, "rows", "row_values"), (cols, "col", nb, "cols", "col_values")):
        if not on:
            continue
        idx, val = bufs[f"{name}_idx"], bufs[f"{name}_val"]
        assert bool((idx[2 * n:] == UNSET).all()), f"wrote behind {name}_idx"
        assert bool((idx[: 2 * n] != UNSET).all()), f"left an element of {name}_idx unwritten"
        assert _intact(val, n), f"wrote behind {name}_val"
        assert _written(val, n), f"left an element of {name}_val unwritten"
        out[key], out[vkey] = idx[: 2 * n].cpu().numpy().reshape(n, 2), val[:n].cpu().numpy()
    assert _intact(ws, ws_bytes // 8), "wrote behind the workspace"
    return out


def _same(a, b):
    assert sorted(a) == sorted(b)
    for q in a:
        x, y = np.ascontiguousarray(a[q]), np.ascontiguousarray(b[q])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), q


CONVENTION_COVERS = {"mvf_assign_best": ("side_stream", "inputs")}


@pytest.mark.parametrize("mode", ["side_stream", "inputs"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("na,nb", [(65, 63), (50, 4417)])   # one tile pair; the split plan
def test_calling_conventions(na, nb, dtype, mode):
    """The plain call's bits with the call on a side stream - the case's operands are made when the case is built, so the
    outputs and the workspace, not the inputs, are in flight there: a launch on another stream is overwritten by their fill -,
    and with every operand unchanged by the call."""
    dc = _case(("best", na, nb), lambda: _shape_case(na, nb), dtype)

    def call():
        _watch_case(dc)
        return _best(dc)

    plain, got = _under(mode, call)
    _same(plain, got)


def _check(dc, got, what):
    ref = dc.reference()
    return bc.check(got, ref["P"], dc.xa[:, :3], dc.xb[:, :3], ac.F64_TOL, what=f"{what} {dc.dtype} plan {ec.plan(dc.na, dc.nb)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("na,nb", SHAPES)
def test_shapes_on_the_kernels_edges(dtype, na, nb):
    dc = _case(("best", na, nb), lambda: _shape_case(na, nb), dtype)
    got = _best(dc)
    _check(dc, got, f"{na}x{nb}")
    _same(got, _best(dc))
    if (na, nb) in SPLIT_SHAPES:
        assert ec.plan(na, nb) == ec.SPLIT_PLANS[(na, nb)] and 64 in ec.plan(na, nb)[2:]
    far = dc.case["far"]                     # all-zero columns: value 0, the first rule says row 0
    assert not got["col_values"][far].any() and not got["cols"][far, 1].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", [1, 16, 17])
def test_the_k_step(dtype, g):
    dc = _case(("best-g", g), lambda: ec.make_case(f"best-g{g}", 70, 66, [("kl", "gauss", None, g)]), dtype)
    got = _best(dc)
    _check(dc, got, f"g {g}")
    _same(got, _best(dc))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["four-layers", "2d"])
def test_layers_and_dimensions(dtype, kind):
    make = {"four-layers": lambda: ec.make_case("best-4-layers", 140, 101, list(ec.LAYER_SET)),
            "2d": lambda: ec.make_case("best-2d", 70, 66, [("euc", "gauss", None, 24)], D=2, sigma2_variance=2.5)}[kind]
    dc = _case(("best", kind), make, dtype)
    got = _best(dc)
    _check(dc, got, kind)
    _same(got, _best(dc))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_label_layer(dtype):
    """The label branch of the tile routine (65 x 129, a 7 x 9 table, an expression layer beside it) against the restatement
    of tests/_assign_label_case.py on the coordinates as stored."""
    lc = _LabelCase((65, 129, 7, 9), dtype)
    lc.dtype = dtype
    got = _best(lc, struct=lc.struct())
    bc.check(got, lc.ref["P"], lc.XA, lc.XB, ac.F64_TOL, what=f"label 65x129 {dtype}")
    _same(got, _best(lc, struct=lc.struct()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_ties_are_decided_by_the_rules(dtype):
    dc = _case("best-ties", bc.tie_case, dtype)
    c = dc.case
    na, nb = TIE_SHAPE
    rt, ct, rs, cs = ec.plan(na, nb)
    assert (rs, cs) == (rt, ct) == (4, 5)                       # every tile a split of its own
    got = _best(dc)
    _check(dc, got, "ties")
    _same(got, _best(dc))
    P = dc.reference()["P"]
    rows, cols = got["rows"], got["cols"]
    # all-zero rows: the nearest B cell under the first rule's index 0 - in another tile (= split) than column 0
    zr = c["zero_rows"]
    assert not P[zr].any() and not got["row_values"][zr].any()
    assert not rows[zr, 1].any() and (rows[zr, 0] != 0).all()
    assert (rows[zr, 0] // ec.TILE != 0).any()
    d = ((dc.xb[None, :, :3] - dc.xa[zr, None, :3]) ** 2).sum(2)
    assert np.array_equal(rows[zr, 0], d.argmin(1))
    # all-zero columns likewise
    zc = c["far"]
    assert not P[:, zc].any() and not cols[zc, 1].any() and (cols[zc, 0] != 0).all()
    assert (cols[zc, 0] // ec.TILE != 0).any()
    d = ((dc.xa[None, :, :3] - dc.xb[zc, None, :3]) ** 2).sum(2)
    assert np.array_equal(cols[zc, 0], d.argmin(1))
    # the copies: lanes, tiles and splits apart, the entries tie and both rules return the smallest copy
    # (the reference's matrix product may leave the copies an ulp apart; the device forms them by the same operations in the
    # same order: an exact tie, which the rules give to the smallest copy)
    tied_rows = tied_cols = 0
    for group in c["copies_B"]:
        assert len({j // ec.TILE for j in group}) >= 3 and group[1] == group[0] + 1
        for i in np.flatnonzero(P[:, group].max(1) == P.max(1)):
            if P[i].max() > 0:
                assert np.ptp(P[i, group]) <= ec.REF_TOL * P[i].max()
                assert rows[i, 0] == rows[i, 1] == group[0], (i, group, rows[i])
                tied_rows += 1
    for group in c["copies_A"]:
        assert len({i // ec.TILE for i in group}) >= 3
        for j in np.flatnonzero(P[group].max(0) == P.max(0)):
            if P[:, j].max() > 0:
                assert np.ptp(P[group, j]) <= ec.REF_TOL * P[:, j].max()
                assert cols[j, 0] == cols[j, 1] == group[0], (j, group, cols[j])
                tied_cols += 1
    print(f"  ties {dtype}: rows headed by a copied column {tied_rows}, columns headed by a copied row {tied_cols}")
    assert tied_rows >= len(c["copies_B"]) >= 2 and tied_cols >= len(c["copies_A"]) >= 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_null_pair_skips_its_direction(dtype):
    dc = _case(("best", 129, 200), lambda: _shape_case(129, 200), dtype)
    both = _best(dc)
    only_rows, only_cols = _best(dc, cols=False), _best(dc, rows=False)
    assert sorted(only_rows) == ["row_values", "rows"] and sorted(only_cols) == ["col_values", "cols"]
    _same(only_rows, {q: both[q] for q in only_rows})
    _same(only_cols, {q: both[q] for q in only_cols})


@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_contents_and_size_do_not_matter(dtype):
    """A larger workspace, zero-filled, NaN-filled and holding a larger call's states: the same bits."""
    ds = _case(("best", 129, 200), lambda: _shape_case(129, 200), dtype)
    dl = _case(("best", 50, 4417), lambda: _shape_case(50, 4417), dtype)
    kk = ds.k
    size = max(int(kk.lib.mvf_assign_best_workspace_bytes(ds.na, ds.nb)), int(kk.lib.mvf_assign_best_workspace_bytes(dl.na, dl.nb))) + 4096
    ws = _guarded(size // 8)
    ws[: size // 8] = 0.0
    zero = _best(ds, ws=ws, ws_bytes=size)
    ws[: size // 8] = float("nan")
    nan = _best(ds, ws=ws, ws_bytes=size)
    _best(dl, ws=ws, ws_bytes=size)
    stale = _best(ds, ws=ws, ws_bytes=size)
    tight = _best(ds)
    for other in (nan, stale, tight):
        _same(zero, other)


def _expected_workspace(na, nb):
    """mvf_assign's plan, K_NB of the factor kernel, then per direction two float64 and one int32 pair per (split, padded
    cell); every block rounded up to 256 bytes."""
    rt, ct, rs, cs = ec.plan(na, nb)
    up = lambda n: ec.cdiv(n, 256) * 256  # noqa: E731
    nr, nc = cs * rt * ec.TILE, rs * ct * ec.TILE
    return ec.workspace_bytes(na, nb) + up(8 * ct * ec.TILE) + 3 * up(8 * nr) + 3 * up(8 * nc)


def test_workspace_size_function():
    lib = _k("float64").lib
    for na, nb in SHAPES + [TIE_SHAPE, (100000, 100000)]:
        assert int(lib.mvf_assign_best_workspace_bytes(na, nb)) == _expected_workspace(na, nb), (na, nb)
    for na, nb in ((0, 5), (5, 0), (0, 0), (-1, 5)):
        assert int(lib.mvf_assign_best_workspace_bytes(na, nb)) == 0


def test_argument_errors_are_reported_before_anything_is_launched():
    dc = _case(("best", 65, 63), lambda: _shape_case(65, 63), "float64")
    lib, na, nb, c = dc.k.lib, dc.na, dc.nb, dc.case
    need = int(lib.mvf_assign_best_workspace_bytes(na, nb))
    ws = _nan_workspace(need)
    ri = torch.full((2 * na,), UNSET, dtype=torch.int32, device=DEV)
    ci = torch.full((2 * nb,), UNSET, dtype=torch.int32, device=DEV)
    rv, cv = _guarded(na), _guarded(nb)

    def call(mm=dc.mm.data_ptr(), outs=None, ws_bytes=need, na_=na, nb_=nb):
        outs = (ri.data_ptr(), rv.data_ptr(), ci.data_ptr(), cv.data_ptr()) if outs is None else outs
        rc = lib.mvf_assign_best(dc.xa4.data_ptr(), na_, dc.xb4.data_ptr(), nb_, _layer_array(dc), len(dc.layers), mm,
                                 float(c["sigma2"]), float(c["sigma2_variance"]), float(dc.outlier), *outs, ws.data_ptr(),
                                 int(ws_bytes), dc.k.cdtype, dc.k._stream())
        return rc, lib.mvf_last_error().decode("utf-8", "replace")

    rc, msg = call(ws_bytes=need - 8)
    assert rc != 0 and "workspace too small" in msg
    rc, msg = call(mm=None)
    assert rc != 0 and "null pointer" in msg
    rc, msg = call(outs=(None, None, None, None))
    assert rc != 0 and "both NULL" in msg
    rc, msg = call(outs=(ri.data_ptr(), None, ci.data_ptr(), cv.data_ptr()))
    assert rc != 0 and "row_idx and row_val" in msg
    rc, msg = call(outs=(ri.data_ptr(), rv.data_ptr(), None, cv.data_ptr()))
    assert rc != 0 and "col_idx and col_val" in msg
    torch.cuda.synchronize()
    assert bool((ri == UNSET).all()) and bool((ci == UNSET).all())
    assert bool((rv == SENTINEL[torch.float64]).all()) and bool((cv == SENTINEL[torch.float64]).all())
    assert _intact(ws, need // 8) and bool(torch.isnan(ws[: need // 8]).all())       # nothing was launched
    assert call(na_=0)[0] == 0 and call(nb_=0)[0] == 0                                     # an empty side: nothing to do
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert bool((ri != UNSET).all())
