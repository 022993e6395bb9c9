"""Kernel-level tests of ``mvf_assign_layer_stats`` (``csrc/mvf_assign.hip``: the column statistics of one layer's distance
matrix, under the alignment's start state) through the raw C ABI on ``cuda:0`` in both cell dtypes.  The reference is
``_align_start_case.layer_stats`` on the distance formed from the operands AS STORED (the device's own prepared operands, read
back), so float32 storage is held to the float64 bound.  Every call runs on a NaN-filled, guarded workspace with a guard
behind every output and is made twice (same bits, ``rows`` included).

Shapes (na, nb) sit on the kernel's edges: the smallest call, the tile edges either way, one full tile, the smallest shape
whose rows split over two workgroups (65 x 1), 4 and 64 row splits (200 x 4, 4097 x 10), a list longer than the column (k > na).  Feature
counts 1, 16 and 17 are the k-step's edges.  ``cmin``, ``vals`` and ``sums`` are held to ``_assign_case.F64_TOL`` relative to
max |d| (the sum of squares: to its square, the scale of a d^2 quantity); ``rows`` must be equal.  The generated product cases keep a gap of 1e-6
max |d| between neighbouring entries of every list (asserted on the reference, so the reference alone decides the order); a
label layer's distances are table entries, equal for equal labels: there the row decides, and ``vals`` are exact.

No bound is fitted to what the device returned."""
import numpy as np
import pytest
import torch

import _align_start_case as sc
import _assign_case as ac
import _assign_edge_cases as ec
from _align_kernel_scaffold import kernels as _k, label_prepare as _label_prepare, prepare as _prepare
from _kernel_scaffold import (DEV, DTYPES, GUARD, MODES, called as _called, dev as _dev, guarded as _guarded, intact as _intact,
                              nan_workspace as _nan_workspace, same_bits as _same_bits, under as _under, watch as _watch,
                              written as _written)

pytestmark = pytest.mark.gpu

KS = (0, 1, 10, 64)
# (na, nb, the k's): a list of 64 is asked for where the columns are few - the more entries the lists of a case hold, the
# closer the closest two of them lie, and the generated cases keep GAP between neighbours
SHAPES = [(1, 1, KS), (63, 65, KS[:3]), (64, 64, KS[:3]), (65, 129, KS[:3]), (65, 1, KS), (5, 3, KS), (200, 4, KS), (4097, 10, KS[:3])]
PRODUCT = ("euc", "square_euc", "kl", "sym_kl", "cos")
GAP = 1e-6
LABEL = 5  # MVF_ASSIGN_LABEL
_CASES = {}


def _features(rng, n, g, metric):
    if metric in ("kl", "sym_kl"):
        return rng.poisson(rng.gamma(0.6, 4.0, (1, g)) * rng.uniform(0.2, 3.0, (n, g))).astype(np.float64)
    return rng.standard_normal((n, g)) * 1.5


def _product_inputs(na, nb, g, metric, dtype, k):
    """Raw layers whose lists keep the gap (checked here on prepare_reference's operands, asserted in the test on the
    device's): the first seed that does."""
    npdt = np.float32 if dtype == "float32" else np.float64
    if g == 1:
        # one feature: d is |x - y| or its square, and among random points the smallest squares lie closer than the gap.  A
        # cells on the integers (shuffled), B cells 0.15 and 0.35 above them: every |x - y| is one of n +- 0.15, n +- 0.35
        rng = np.random.default_rng(na + nb)
        j = np.arange(nb)
        return rng.permutation(na).astype(np.float64)[:, None], ((j // 2) % na + np.where(j % 2, 0.35, 0.15))[:, None]
    for seed in range(200):
        rng = np.random.default_rng(1000 * seed + 7 * na + nb)
        A, B = _features(rng, na, g, metric), _features(rng, nb, g, metric)
        Xp, a = ec.prepare_reference(A, metric, 0, npdt)
        Yp, b = ec.prepare_reference(B, metric, 1, npdt)
        d = sc.stored_distance(Xp, Yp, a, b, metric)
        if min(sc.list_gap(d, k), sc.list_gap(d.T, k)) >= 1.01 * GAP:
            return A, B
    raise AssertionError("no seed keeps the lists' entries apart")


class _Layer:
    """One layer on the device, prepared BY THE DEVICE and read back: `fields` as mvf_assign_layer takes them, `d` the
    distance matrix (na, nb) from the stored operands; `swapped` the same for the exchanged call."""

    def __init__(self, na, nb, g, metric, dtype, k=64):
        kk = _k(dtype)
        self.k, self.na, self.nb, self.metric, self.dtype = kk, na, nb, metric, dtype
        self.name = f"{metric} {na}x{nb} G {g} {dtype}"
        if metric == "label":   # g: (K, L) of the table
            K, L = g
            rng = np.random.default_rng(na + 3 * nb + K + L)
            table = rng.uniform(0.1, 2.0, (K, L))
            la, lb = rng.integers(0, K, na), rng.integers(0, L, nb)
            T, Tt = _dev(table), _dev(table.T.copy())
            a, b = kk.assign_label_prepare(la, K), kk.assign_label_prepare(lb, L)
            self.fields = (T, None, a, b, L, LABEL)
            self.swapped = (Tt, None, b, a, K, LABEL)
            self.d = sc.label_distance(table, la, lb)
            self.keep = (T, Tt, a, b)
        else:
            A, B = _product_inputs(na, nb, g, metric, dtype, k)
            Xp, a, ld = _prepare(kk, A, metric, 0)
            Yp, b, _ = _prepare(kk, B, metric, 1)
            self.fields = (Xp, Yp, a, b, ld, ec.METRICS[metric])
            self.swapped = (Yp, Xp, b, a, ld, ec.METRICS[metric])
            self.d = sc.stored_distance(Xp.double().cpu().numpy(), Yp.double().cpu().numpy(), a.cpu().numpy(), b.cpu().numpy(), metric)


def _layer(key, *args):
    if key not in _CASES:
        if len(_CASES) >= 4:
            _CASES.pop(next(iter(_CASES)))
        _CASES[key] = _Layer(*args)
    return _CASES[key]


def _stats(ly, fields, na, nb, k, ws=None, ws_bytes=None):
    """mvf_assign_layer_stats through the raw ABI; guards behind every output and the workspace (exactly
    mvf_assign_layer_stats_workspace_bytes, NaN-filled).  Returns host arrays."""
    from spateo_amd import _lib
    from spateo_amd._kernels import layer_array

    kk = ly.k
    ke = min(k, na)
    Xp, Yp, a, b, ld, metric = fields
    arr = layer_array([(Xp, Yp, a, b, ld, metric, 0, -1.0)])   # prob / param are not read: a gauss layer without a parameter passes
    sizes = {"cmin": nb, "sums": 2, "vals": nb * ke}
    bufs = {q: _guarded(n) for q, n in sizes.items()}
    rows = torch.full((nb * ke + GUARD,), -7, dtype=torch.int32, device=DEV)
    need = int(kk.lib.mvf_assign_layer_stats_workspace_bytes(na, nb, k))
    assert need > 0 and need % 8 == 0
    if ws is None:
        ws, ws_bytes = _nan_workspace(need), need
    _lib.check(kk.lib.mvf_assign_layer_stats(arr, na, nb, k, bufs["cmin"].data_ptr(), rows.data_ptr() if k else None,
                                             bufs["vals"].data_ptr() if k else None, bufs["sums"].data_ptr(), ws.data_ptr(),
                                             int(ws_bytes), kk.cdtype, kk._stream()), "mvf_assign_layer_stats")
    _called()
    torch.cuda.synchronize()
    for q, n in sizes.items():
        assert _intact(bufs[q], n), f"{ly.name}: wrote behind {q}[{n}]"
        assert _written(bufs[q], n), f"{ly.name}: left an element of {q} unwritten"
    assert bool((rows[nb * ke:] == -7).all()), f"{ly.name}: wrote behind rows"
    assert bool((rows[: nb * ke] != -7).all()), f"{ly.name}: left an element of rows unwritten"
    assert _intact(ws, ws_bytes // 8), f"{ly.name}: wrote behind the workspace"
    out = {q: bufs[q][:n].cpu().numpy() for q, n in sizes.items()}
    out["vals"], out["rows"] = out["vals"].reshape(nb, ke), rows[: nb * ke].cpu().numpy().reshape(nb, ke)
    return out


def _same(a, b):
    for q in ("cmin", "sums", "vals", "rows"):
        x, y = np.ascontiguousarray(a[q]), np.ascontiguousarray(b[q])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), q


# mvf_assign_layer_stats reads a layer that the device prepared when the case was built: no displaced pointers for it, and on
# the side stream its outputs and workspace, not its operands, are in flight.
CONVENTION_COVERS = {"mvf_assign_layer_stats": ("side_stream", "inputs"), "mvf_assign_label_prepare": MODES}


@pytest.mark.parametrize("mode", ["side_stream", "inputs"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("na,nb,g,metric", [(63, 65, 17, "kl"), (200, 4, 16, "cos"), (65, 129, (3, 4), "label")])
def test_layer_stats_calling_conventions(na, nb, g, metric, dtype, mode):
    ly = _layer((na, nb, g, metric, dtype, 10), na, nb, g, metric, dtype, 10)

    def call():
        _watch(*[t for t in ly.fields[:4] if torch.is_tensor(t)])
        return _stats(ly, ly.fields, na, nb, 10)

    plain, got = _under(mode, call)
    _same(plain, got)


@pytest.mark.parametrize("mode", MODES)
def test_label_prepare_calling_conventions(mode):
    labels = np.random.default_rng(3).integers(0, 7, 1025)
    plain, got = _under(mode, lambda: _label_prepare(_k("float64"), labels, 7).cpu().numpy())
    assert np.array_equal(plain, labels.astype(np.float64)) and _same_bits(plain, got)


def _check(ly, d, got, k, what):
    """got against layer_stats(d, k): values at F64_TOL relative to max |d|, rows equal."""
    ref = sc.layer_stats(d, k)
    top = max(float(np.abs(d).max()), 1e-300)
    dev = {"cmin": np.abs(got["cmin"] - ref["cmin"]).max() / top,
           "sums0": abs(got["sums"][0] - ref["sums"][0]) / top,
           # the sum of squares on its own scale, max |d|^2: at max |d| = 228 (euc, 4097 x 10) two float64 summation orders of the
           # REFERENCE differ by 1.1e-8 max |d| (4.8e-11 max |d|^2) - no float64 sum meets 1e-10 max |d| there
           "sums1": abs(got["sums"][1] - ref["sums"][1]) / (top * top)}
    assert np.isfinite(got["cmin"]).all() and np.isfinite(got["sums"]).all()
    if k:
        assert got["rows"].shape == ref["rows"].shape == (d.shape[1], min(k, d.shape[0]))
        if ly.metric == "label":
            assert np.array_equal(got["vals"], ref["vals"]), what          # table entries: exact
        else:
            assert sc.list_gap(d, k) >= GAP, (what, sc.list_gap(d, k))     # the reference alone decides the order
        dev["vals"] = np.abs(got["vals"] - ref["vals"]).max() / top
        assert np.array_equal(got["rows"], ref["rows"]), (what, np.argwhere(got["rows"] != ref["rows"])[:5])
    print(f"  {what} k {k} plan {ec.plan(*d.shape)}: " + ", ".join(f"{q} {v:.1e}" for q, v in dev.items()))
    for q, v in dev.items():
        assert v <= ac.F64_TOL, (what, q, v)


def _both_ways(ly, ks):
    for k in ks:
        got = _stats(ly, ly.fields, ly.na, ly.nb, k)
        _check(ly, ly.d, got, k, ly.name)
        _same(got, _stats(ly, ly.fields, ly.na, ly.nb, k))
        # the statistics of the rows: the exchanged operands against the transposed restatement
        got = _stats(ly, ly.swapped, ly.nb, ly.na, k)
        _check(ly, ly.d.T, got, k, ly.name + " exchanged")
        _same(got, _stats(ly, ly.swapped, ly.nb, ly.na, k))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", PRODUCT)
@pytest.mark.parametrize("na,nb,ks", SHAPES)
def test_shapes_on_the_kernels_edges(dtype, metric, na, nb, ks):
    ly = _layer((na, nb, 20, metric, dtype), na, nb, 20, metric, dtype, max(ks))
    rt, ct, rs, _ = ec.plan(na, nb)
    if (na, nb) == (65, 1):
        assert rs == 2 and ec.plan(64, 1)[2] == 1      # the smallest shape whose rows split
    if na == 4097:
        assert rs == 64
    _both_ways(ly, ks)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric,g", [("euc", 1), ("square_euc", 1)] + [(m, g) for m in PRODUCT for g in (16, 17)])
def test_feature_counts_on_the_k_steps_edges(dtype, metric, g):
    """1 feature (the metrics whose distance a single feature separates), 16 (one full k-step) and 17 (a second one, padded)."""
    ly = _layer((65, 129, g, metric, dtype), 65, 129, g, metric, dtype, 10)
    assert ly.fields[4] == ec.padded_features(g, metric)
    _both_ways(ly, (0, 10))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,L", [(1, 7), (6, 1), (5, 4)])
@pytest.mark.parametrize("na,nb", [(63, 65), (65, 129), (5, 3)])
def test_label_layers(dtype, K, L, na, nb):
    """Tables of one row, of one column and a general one; the exchanged call takes the transposed table and its row length."""
    ly = _layer((na, nb, (K, L), "label", dtype), na, nb, (K, L), "label", dtype)
    _both_ways(ly, KS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_contents_size_and_stream_do_not_matter(dtype):
    ly = _layer((65, 129, 20, "kl", dtype), 65, 129, 20, "kl", dtype, 64)
    big = _layer((4097, 10, 20, "kl", dtype), 4097, 10, 20, "kl", dtype, 10)
    kk = ly.k
    size = max(int(kk.lib.mvf_assign_layer_stats_workspace_bytes(65, 129, 10)),
               int(kk.lib.mvf_assign_layer_stats_workspace_bytes(4097, 10, 10))) + 4096
    ws = _guarded(size // 8)
    ws[: size // 8] = 0.0
    zero = _stats(ly, ly.fields, 65, 129, 10, ws=ws, ws_bytes=size)
    _stats(big, big.fields, 4097, 10, 10, ws=ws, ws_bytes=size)
    stale = _stats(ly, ly.fields, 65, 129, 10, ws=ws, ws_bytes=size)
    tight = _stats(ly, ly.fields, 65, 129, 10)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        other = _stats(ly, ly.fields, 65, 129, 10)
    torch.cuda.synchronize()
    for o in (stale, tight, other):
        _same(zero, o)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_binding_returns_the_raw_calls_bits(dtype):
    """HipKernels.assign_layer_stats against the raw call."""
    ly = _layer((65, 129, 20, "kl", dtype), 65, 129, 20, "kl", dtype, 64)
    raw = _stats(ly, ly.fields, 65, 129, 10)
    got = ly.k.assign_layer_stats(ly.fields + (2, 0.0), 65, 129, 10)
    _same(raw, {q: v.cpu().numpy() for q, v in got.items()})
    assert set(ly.k.assign_layer_stats(ly.fields + (2, 0.0), 65, 129)) == {"cmin", "sums"}
