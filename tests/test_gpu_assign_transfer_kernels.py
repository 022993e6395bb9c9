"""Kernel-level tests of ``mvf_assign_apply`` (``csrc/mvf_assign.hip``: ``P @ FB`` and ``P^T @ FA`` without ``P``) through the raw
C ABI on ``cuda:0`` in both cell dtypes.  The reference is the dense ``P`` of ``_assign_edge_cases.pair_reference`` on the
operands the device itself prepared (read back), times the features in float64, so float32 storage is held to the float64
bound ``F64_TOL`` - as the best-partner kernel tests hold theirs; deviations are taken relative to ``max (P @ |F|)``
(``_assign_transfer_case``).  Every call runs on a NaN-filled, guarded workspace of exactly the size the library asks for, with
a guard behind every output, and is made twice (same bits).  ``K_NA`` / ``K_NB`` are held to ``mvf_assign``'s at ``F64_TOL``.

Shapes sit on the kernels' own edges: the dense shapes of ``_assign_edge_cases``, 63 / 64 / 65 / 129 rows against 1 / 65 / 200
columns, 64 row splits and 64 column splits; feature widths 1, 15, 16, 17 (the MFMA column block), 63, 64, 65, 129 (the
64-column chunk), once with ``ldf > c`` and NaN in the padding; one direction only, each way; NULL sums; four layers; a label
layer with a non-square table (the exchanged sweep must read it transposed); 2-D; far B cells and an A cell of weight 0;
1 / 16 / 17 layer features.

No bound is fitted to what the device returned."""
import numpy as np
import pytest
import torch

import _assign_case as ac
import _assign_edge_cases as ec
import _assign_transfer_case as tc
from _align_kernel_scaffold import (assign as _assign, device_case as _case, LabelCase as _LabelCase,
                                    layer_struct as _layer_array, watch_case as _watch_case)
from _kernel_scaffold import (DEV, DTYPES, SENTINEL, called as _called, dev as _dev, guarded as _guarded, intact as _intact,
                              nan_workspace as _nan_workspace, under as _under, written as _written)

pytestmark = pytest.mark.gpu

EDGE_SHAPES = [(na, nb) for na in (63, 64, 65, 129) for nb in (1, 65, 200)]
SPLIT_SHAPES = [(4417, 50), (50, 4417)]
SHAPES = list(ec.DENSE_SHAPES) + EDGE_SHAPES + SPLIT_SHAPES
WIDTHS = [1, 15, 16, 17, 63, 64, 65, 129]
WIDTH_SHAPE = (129, 200)
OUT = ("to_A", "to_B", "K_NA", "K_NB")


def _shape_case(na, nb):
    layers = [("kl", "gauss", None, 20)] if (na + nb) % 2 else [("cos", "cos", None, 17), ("euc", "gauss", None, 24)]
    return ec.make_case(f"transfer-{na}x{nb}", na, nb, layers, far="some")


def _features(n, c, seed):
    """(n, c) float64: c // 2 one-hot columns, the rest standard normal (the golden's kind)."""
    rng = np.random.default_rng((n, c, seed))
    F = rng.standard_normal((n, c))
    if c // 2:
        F[:, : c // 2] = 0.0
        F[np.arange(n), rng.integers(0, c // 2, n)] = 1.0
    return F


def _strided(F, ld):
    """F on the device in rows of ld >= c doubles, the padding NaN: a kernel that reads it returns NaN."""
    n, c = F.shape
    buf = torch.full((n, ld), float("nan"), dtype=torch.float64, device=DEV)
    buf[:, :c] = _dev(F)
    return buf


def _apply(dc, FB=None, FA=None, ldfb=None, ldfa=None, k_na=True, k_nb=True, ws=None, ws_bytes=None, struct=None):
    """mvf_assign_apply through the raw ABI on the current stream; guards behind every output and the workspace (default:
    exactly mvf_assign_apply_workspace_bytes, NaN-filled).  Returns host arrays."""
    from spateo_amd import _lib

    kk, na, nb = dc.k, dc.na, dc.nb
    cb, ca = (0 if FB is None else FB.shape[1]), (0 if FA is None else FA.shape[1])
    ldfb, ldfa = (cb if ldfb is None else ldfb), (ca if ldfa is None else ldfa)
    need = int(kk.lib.mvf_assign_apply_workspace_bytes(na, nb, cb, ca))
    assert need == tc.workspace_bytes(na, nb, cb, ca) and need % 8 == 0
    if ws is None:
        ws, ws_bytes = _nan_workspace(need), need
    sizes = {}
    if FB is not None:
        sizes["to_A"] = na * cb
        if k_na:
            sizes["K_NA"] = na
    if FA is not None:
        sizes["to_B"] = nb * ca
    if k_nb:
        sizes["K_NB"] = nb
    bufs = {q: _guarded(n) for q, n in sizes.items()}
    dFB = None if FB is None else _strided(FB, ldfb)
    dFA = None if FA is None else _strided(FA, ldfa)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    c = dc.case if hasattr(dc, "case") else dc.c
    arr = _layer_array(dc) if struct is None else struct
    _lib.check(kk.lib.mvf_assign_apply(dc.xa4.data_ptr(), na, dc.xb4.data_ptr(), nb, arr, len(dc.layers), dc.mm.data_ptr(),
                                       float(c["sigma2"]), float(c["sigma2_variance"]), float(dc.outlier), ptr(dFB), cb, ldfb,
                                       ptr(bufs.get("to_A")), ptr(dFA), ca, ldfa, ptr(bufs.get("to_B")), ptr(bufs.get("K_NA")),
                                       ptr(bufs.get("K_NB")), ws.data_ptr(), int(ws_bytes), kk.cdtype, kk._stream()),
               "mvf_assign_apply")
    _called()
    torch.cuda.synchronize()
    for q, n in sizes.items():
        assert _intact(bufs[q], n), f"wrote behind {q}[{n}]"
        assert _written(bufs[q], n), f"left an element of {q} unwritten"
    assert _intact(ws, ws_bytes // 8), "wrote behind the workspace"
    out = {q: bufs[q][:n].cpu().numpy() for q, n in sizes.items()}
    if "to_A" in out:
        out["to_A"] = out["to_A"].reshape(na, cb)
    if "to_B" in out:
        out["to_B"] = out["to_B"].reshape(nb, ca)
    for q, v in out.items():
        assert np.isfinite(v).all(), f"{q} is not finite"
    return out


def _same(a, b):
    assert sorted(a) == sorted(b)
    for q in a:
        x, y = np.ascontiguousarray(a[q]), np.ascontiguousarray(b[q])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), q


CONVENTION_COVERS = {"mvf_assign_apply": ("side_stream", "inputs")}


@pytest.mark.parametrize("mode", ["side_stream", "inputs"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("na,nb", [(65, 63), (50, 4417)])   # one tile pair; the split plan
def test_calling_conventions(na, nb, dtype, mode):
    """The plain call's bits with the call on a side stream - the case's operands are made when the case is built, so the
    outputs and the workspace, not the inputs, are in flight there: a launch on another stream is overwritten by their fill -,
    and with every operand unchanged by the call."""
    dc = _case(("transfer", na, nb), lambda: _shape_case(na, nb), dtype)

    def call():
        _watch_case(dc)
        return _apply(dc, _features(nb, 17, 1), _features(na, 5, 2))

    plain, got = _under(mode, call)
    _same(plain, got)


def _check(got, P, FB, FA, what):
    """The raw products against P times the features at F64_TOL on the scale max (P @ |F|); the sums against P's."""
    ref = tc.products(P, FA, FB)
    tols = {q: ac.F64_TOL for q in tc.QUANTITIES}
    dev = tc.check(tc.quantities_of(got), ref, tols, what=what)
    assert sorted(dev) == sorted(f"{q}_raw" for q in ("to_A", "to_B") if q in got)
    for q in ("K_NA", "K_NB"):
        if q in got:
            top = np.abs(ref[q]).max()
            assert np.abs(got[q] - ref[q]).max() <= ac.F64_TOL * top if top > 0 else not got[q].any(), (what, q)
    return ref


def _sums_are_mvf_assigns(dc, got):
    plain = _assign(dc)
    for q in ("K_NA", "K_NB"):
        top = np.abs(plain[q]).max()
        assert np.abs(got[q] - plain[q]).max() <= ac.F64_TOL * top if top > 0 else not got[q].any(), q


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("na,nb", SHAPES)
def test_shapes_on_the_kernels_edges(dtype, na, nb):
    dc = _case(("transfer", na, nb), lambda: _shape_case(na, nb), dtype)
    cb, ca = (17, 5) if (na + nb) % 2 else (5, 17)
    FB, FA = _features(nb, cb, 1), _features(na, ca, 2)
    got = _apply(dc, FB, FA)
    _check(got, dc.reference()["P"], FB, FA, f"{na}x{nb} {dtype} plan {ec.plan(na, nb)}")
    _same(got, _apply(dc, FB, FA))
    _sums_are_mvf_assigns(dc, got)
    if (na, nb) in SPLIT_SHAPES:
        assert ec.plan(na, nb) == ec.SPLIT_PLANS[(na, nb)] and 64 in ec.plan(na, nb)[2:]
    far = dc.case["far"]                       # B cells out of reach: zero columns of P, zero rows of to_B
    assert not got["to_B"][far].any() and not got["K_NB"][far].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", WIDTHS)
def test_feature_widths_at_the_block_and_chunk_edges(dtype, c):
    na, nb = WIDTH_SHAPE
    dc = _case(("transfer", na, nb), lambda: _shape_case(na, nb), dtype)
    FB, FA = _features(nb, c, 3), _features(na, c, 4)
    ld = c + 7 if c == 17 else None             # once with rows longer than c, NaN behind the columns
    got = _apply(dc, FB, FA, ldfb=ld, ldfa=ld)
    _check(got, dc.reference()["P"], FB, FA, f"C {c} {dtype}")
    _same(got, _apply(dc, FB, FA, ldfb=ld, ldfa=ld))
    if ld is not None:                           # the row length changes nothing
        _same(got, _apply(dc, FB, FA))


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_direction_only_and_null_sums(dtype):
    na, nb = WIDTH_SHAPE
    dc = _case(("transfer", na, nb), lambda: _shape_case(na, nb), dtype)
    FB, FA = _features(nb, 70, 5), _features(na, 33, 6)
    both = _apply(dc, FB, FA)
    only_A, only_B = _apply(dc, FB=FB), _apply(dc, FA=FA)
    assert sorted(only_A) == ["K_NA", "K_NB", "to_A"] and sorted(only_B) == ["K_NB", "to_B"]
    _same(only_A, {q: both[q] for q in only_A})
    _same(only_B, {q: both[q] for q in only_B})
    bare = _apply(dc, FB, FA, k_na=False, k_nb=False)
    assert sorted(bare) == ["to_A", "to_B"]
    _same(bare, {q: both[q] for q in bare})
    _same(_apply(dc, FB, FA, k_nb=False), {q: both[q] for q in ("to_A", "to_B", "K_NA")})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", [1, 16, 17])
def test_the_k_step(dtype, g):
    dc = _case(("transfer-g", g), lambda: ec.make_case(f"transfer-g{g}", 70, 66, [("kl", "gauss", None, g)]), dtype)
    FB, FA = _features(66, 9, 7), _features(70, 20, 8)
    got = _apply(dc, FB, FA)
    _check(got, dc.reference()["P"], FB, FA, f"g {g} {dtype}")
    _same(got, _apply(dc, FB, FA))


def _weightless_cell():
    c = ec.make_case("transfer-weightless", 140, 101, [("kl", "gauss", None, 24)], far="some")
    c["alpha"][[5, 70]] = 0.0                    # model_mul = 0: rows of P that are exactly zero
    return c


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["four-layers", "2d", "weightless"])
def test_layers_dimensions_and_cells_without_partners(dtype, kind):
    make = {"four-layers": lambda: ec.make_case("transfer-4-layers", 140, 101, list(ec.LAYER_SET)),
            "2d": lambda: ec.make_case("transfer-2d", 70, 66, [("euc", "gauss", None, 24)], D=2, sigma2_variance=2.5),
            "weightless": _weightless_cell}[kind]
    dc = _case(("transfer", kind), make, dtype)
    FB, FA = _features(dc.nb, 6, 9), _features(dc.na, 65, 10)
    got = _apply(dc, FB, FA)
    _check(got, dc.reference()["P"], FB, FA, f"{kind} {dtype}")
    _same(got, _apply(dc, FB, FA))
    far = dc.case["far"]
    assert len(far) and not got["to_B"][far].any() and not got["K_NB"][far].any()
    if kind == "weightless":
        assert not got["to_A"][[5, 70]].any() and not got["K_NA"][[5, 70]].any() and got["K_NA"][6] > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_label_layer_with_a_non_square_table(dtype):
    """65 x 129 cells, a 7 x 9 table and an expression layer beside it: P @ FB runs on the exchanged operands and must read
    the table as T[label of the A cell][label of the B cell] all the same (a missed transpose reads other entries, or - 7 x 9
    against 9 x 7 - rows that do not exist)."""
    lc = _LabelCase((65, 129, 7, 9), dtype)
    FB, FA = _features(129, 20, 11), _features(65, 7, 12)
    got = _apply(lc, FB, FA, struct=lc.struct())
    _check(got, lc.ref["P"], FB, FA, f"label 65x129 {dtype}")
    _same(got, _apply(lc, FB, FA, struct=lc.struct()))
    # the label layer alone (no expression layer to mask a slip), the other rectangle
    lo = _LabelCase((65, 129, 4, 1), dtype, expression=False)
    got = _apply(lo, FB, FA, struct=lo.struct())
    _check(got, lo.ref["P"], FB, FA, f"label alone 65x129 {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_contents_and_size_do_not_matter(dtype):
    """A larger workspace, zero-filled, NaN-filled and holding a larger call's partials: the same bits."""
    ds = _case(("transfer", 129, 200), lambda: _shape_case(129, 200), dtype)
    dl = _case(("transfer", 50, 4417), lambda: _shape_case(50, 4417), dtype)
    FB, FA = _features(200, 70, 13), _features(129, 5, 14)
    FBl, FAl = _features(4417, 64, 15), _features(50, 64, 16)
    lib = ds.k.lib
    size = max(int(lib.mvf_assign_apply_workspace_bytes(129, 200, 70, 5)), int(lib.mvf_assign_apply_workspace_bytes(50, 4417, 64, 64))) + 4096
    ws = _guarded(size // 8)
    ws[: size // 8] = 0.0
    zero = _apply(ds, FB, FA, ws=ws, ws_bytes=size)
    ws[: size // 8] = float("nan")
    nan = _apply(ds, FB, FA, ws=ws, ws_bytes=size)
    _apply(dl, FBl, FAl, ws=ws, ws_bytes=size)
    stale = _apply(ds, FB, FA, ws=ws, ws_bytes=size)
    tight = _apply(ds, FB, FA)
    for other in (nan, stale, tight):
        _same(zero, other)


def test_argument_errors_are_reported_before_anything_is_launched():
    dc = _case(("transfer", 65, 63), lambda: _shape_case(65, 63), "float64")
    lib, na, nb, c = dc.k.lib, dc.na, dc.nb, dc.case
    cb, ca = 5, 70
    need = int(lib.mvf_assign_apply_workspace_bytes(na, nb, cb, ca))
    ws = _nan_workspace(need)
    FB, FA = _dev(_features(nb, cb, 17)), _dev(_features(na, ca, 18))
    outs = {"to_A": _guarded(na * cb), "to_B": _guarded(nb * ca), "K_NA": _guarded(na), "K_NB": _guarded(nb)}

    def call(ws_bytes=need, na_=na, nb_=nb, **over):
        a = dict(FB=FB.data_ptr(), cb=cb, ldfb=cb, to_A=outs["to_A"].data_ptr(), FA=FA.data_ptr(), ca=ca, ldfa=ca,
                 to_B=outs["to_B"].data_ptr(), K_NA=outs["K_NA"].data_ptr(), K_NB=outs["K_NB"].data_ptr(), mm=dc.mm.data_ptr())
        a.update(over)
        rc = lib.mvf_assign_apply(dc.xa4.data_ptr(), na_, dc.xb4.data_ptr(), nb_, _layer_array(dc), len(dc.layers), a["mm"],
                                  float(c["sigma2"]), float(c["sigma2_variance"]), float(dc.outlier), a["FB"], a["cb"], a["ldfb"],
                                  a["to_A"], a["FA"], a["ca"], a["ldfa"], a["to_B"], a["K_NA"], a["K_NB"], ws.data_ptr(),
                                  int(ws_bytes), dc.k.cdtype, dc.k._stream())
        return rc, lib.mvf_last_error().decode("utf-8", "replace")

    for kw, text in [(dict(ws_bytes=need - 8), "workspace too small"), (dict(mm=None), "null pointer"),
                     (dict(FB=None, cb=0, to_A=None, K_NA=None, FA=None, ca=0, to_B=None), "both directions are skipped"),
                     (dict(to_A=None), "to skip P @ FB"), (dict(FA=None), "to skip P^T @ FA"),
                     (dict(FB=None, cb=0, to_A=None), "K_NA rides"), (dict(ldfa=ca - 1), "ld is below")]:
        rc, msg = call(**kw)
        assert rc != 0 and text in msg, (kw, msg)
    torch.cuda.synchronize()
    for q, buf in outs.items():
        assert bool((buf == SENTINEL[torch.float64]).all()), q
    assert _intact(ws, need // 8) and bool(torch.isnan(ws[: need // 8]).all())       # nothing was launched
    assert call(na_=0)[0] == 0 and call(nb_=0)[0] == 0                                     # an empty side: nothing to do
    torch.cuda.synchronize()
    assert bool((outs["to_A"] == SENTINEL[torch.float64]).all())
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert _written(outs["to_A"], na * cb) and _written(outs["to_B"], nb * ca)
