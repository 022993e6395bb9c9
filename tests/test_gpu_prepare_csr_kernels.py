"""Kernel-level tests of the CSR operand preparation (``csrc/mvf_assign.hip``) through the raw C ABI on ``cuda:0``:
``mvf_assign_prepare_csr`` against ``mvf_assign_prepare`` on the densified matrix, BIT FOR BIT, for the five product metrics,
both sides, both cell dtypes and ``data`` in float32 and float64.

Sizes: n in {1, 3, 4, 5, 257} (the kernel handles four rows a block) x g in {1, 15, 16, 17, 63, 64, 65, 130} (the 16-feature
padding, the 64-lane stride, a row with more than 64 entries).  Rows: empty (leading and trailing), full, a single entry in
the last column, random; the entries of every row are shuffled.  Every case runs once at
``mvf_assign_prepare_csr_min_workspace_bytes(g)`` (one block of four staging rows: n = 5 and n = 257 cross the staging
boundary) and once with room for every row.  Outputs sit in front of guards and are filled with NaN bit patterns, the
workspace is filled with NaN bit patterns and guarded too, and every call is made twice: the same bits."""
import numpy as np
import pytest
import torch

import _assign_edge_cases as ec
from _align_kernel_scaffold import kernels as _k
from _kernel_scaffold import DEV, MODES, called as _called, dev as _dev, guarded, intact as _intact, same_bits as _same_bits, under as _under

pytestmark = pytest.mark.gpu

CELL_DTYPES = ["float64", "float32"]
DATA_DTYPES = [np.float64, np.float32]
PRODUCT_METRICS = ["euc", "square_euc", "kl", "sym_kl", "cos"]
NS = [1, 3, 4, 5, 257]
GS = [1, 15, 16, 17, 63, 64, 65, 130]


def _guarded(n, tdtype=torch.float64):
    """n elements of NaN in front of GUARD sentinels."""
    return guarded(n, tdtype, fill=float("nan"))


def make_csr(n, g, data_dtype, seed):
    """(indptr int64, indices int32, data, dense float64): rows by kind (see the module docstring), entries shuffled."""
    rng = np.random.default_rng(seed)
    if n == 1:
        kinds = ["full"]
    else:
        kinds = ["empty"] + [("full", "last", "random")[i % 3] for i in range(n - 2)] + ["empty"]
    indptr, indices, data = [0], [], []
    for kind in kinds:
        if kind == "empty":
            cols = np.empty(0, dtype=np.int64)
        elif kind == "full":
            cols = np.arange(g)
        elif kind == "last":
            cols = np.array([g - 1])
        else:
            cols = np.flatnonzero(rng.random(g) < 0.4)
        cols = rng.permutation(cols)                       # sortedness is not assumed
        vals = (rng.integers(1, 30, size=len(cols)) + rng.random(len(cols))).astype(data_dtype)
        indices.append(cols), data.append(vals)
        indptr.append(indptr[-1] + len(cols))
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.concatenate(indices).astype(np.int32)
    data = np.concatenate(data).astype(data_dtype)
    dense = np.zeros((n, g))
    for i in range(n):
        sl = slice(indptr[i], indptr[i + 1])
        dense[i, indices[sl]] = data[sl].astype(np.float64)
    return indptr, indices, data, dense


def _dense_prepare(k, dense, metric, side):
    from spateo_amd import _lib

    n, g = dense.shape
    code = ec.METRICS[metric]
    ld = int(k.lib.mvf_assign_padded_features(g, code))
    L = _dev(dense)
    Lp, ab = _guarded(n * ld, k.tdtype), _guarded(n)
    _lib.check(k.lib.mvf_assign_prepare(L.data_ptr(), n, g, code, side, Lp.data_ptr(), ld, ab.data_ptr(), k.cdtype, k._stream()),
               "mvf_assign_prepare")
    _called()
    return Lp[: n * ld].cpu().numpy(), ab[:n].cpu().numpy(), ld


def _csr_call(k, dev, n, g, metric_code, side, ld, ws_bytes, check=True):
    """One mvf_assign_prepare_csr into guarded, NaN-filled buffers: (status, Lp bytes, ab bytes)."""
    indptr, indices, data = dev
    Lp, ab = _guarded(n * ld, k.tdtype), _guarded(n)
    ws = _guarded(ws_bytes // 8)
    status = k.lib.mvf_assign_prepare_csr(indptr.data_ptr(), indices.data_ptr(), data.data_ptr(), int(data.dtype == torch.float32),
                                          n, g, metric_code, side, Lp.data_ptr(), ld, ab.data_ptr(), ws.data_ptr(), ws_bytes,
                                          k.cdtype, k._stream())
    _called()
    torch.cuda.synchronize()
    if status != 0 or not check:
        return status, None, None
    assert _intact(Lp, n * ld) and _intact(ab, n), "mvf_assign_prepare_csr wrote behind an output"
    assert _intact(ws, ws_bytes // 8), "mvf_assign_prepare_csr wrote behind its workspace"
    return status, Lp[: n * ld].cpu().numpy(), ab[:n].cpu().numpy()


def _upload(indptr, indices, data):
    """Device arrays; an empty array still gets an address (one spare element)."""
    def up(a):
        return torch.from_numpy(np.concatenate([a, np.zeros(1, dtype=a.dtype)])).to(DEV)
    return up(indptr)[: len(indptr)], up(indices), up(data)


CONVENTION_COVERS = {"mvf_assign_prepare": MODES, "mvf_assign_prepare_csr": MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", CELL_DTYPES)
@pytest.mark.parametrize("metric,side", [("kl", 0), ("cos", 1)])
def test_calling_conventions(metric, side, dtype, mode):
    """The dense prepare and the CSR prepare (four staging rows) of one 257 x 17 layer: the plain calls' bits on a side stream
    behind poisoned inputs, at displaced pointers, and with the inputs unchanged."""
    k, (n, g), code = _k(dtype), (257, 17), ec.METRICS[metric]
    indptr, indices, data, dense = make_csr(n, g, np.float32, seed=5)

    def call():
        Lp, ab, ld = _dense_prepare(k, dense, metric, side)
        dev = tuple(_dev(a, None) for a in (indptr, indices, data))
        status, Lp2, ab2 = _csr_call(k, dev, n, g, code, side, ld, 4 * g * 8)
        assert status == 0, k.lib.mvf_last_error()
        return Lp, ab, Lp2, ab2

    plain, got = _under(mode, call)
    assert all(_same_bits(a, b) for a, b in zip(plain, got))
    assert _same_bits(plain[0], plain[2]) and _same_bits(plain[1], plain[3])


def _check_case(k, indptr, indices, data, dense, metric, side, what):
    n, g = dense.shape
    code = ec.METRICS[metric]
    want_Lp, want_ab, ld = _dense_prepare(k, dense, metric, side)
    assert not np.isnan(want_Lp).any() and not np.isnan(want_ab).any()
    dev = _upload(indptr, indices, data)
    small = int(k.lib.mvf_assign_prepare_csr_min_workspace_bytes(g))
    assert small == 4 * g * 8
    large = (n + 7) * g * 8
    for ws_bytes in (small, large):
        for rep in range(2):
            status, Lp, ab = _csr_call(k, dev, n, g, code, side, ld, ws_bytes)
            assert status == 0, k.lib.mvf_last_error()
            assert Lp.tobytes() == want_Lp.tobytes(), (what, "Lp", ws_bytes, rep)
            assert ab.tobytes() == want_ab.tobytes(), (what, "ab", ws_bytes, rep)


@pytest.mark.parametrize("data_dtype", DATA_DTYPES, ids=["data64", "data32"])
@pytest.mark.parametrize("dtype", CELL_DTYPES)
@pytest.mark.parametrize("metric", PRODUCT_METRICS)
def test_csr_prepare_equals_dense_prepare_bit_for_bit(metric, dtype, data_dtype):
    k = _k(dtype)
    for n in NS:
        for g in GS:
            indptr, indices, data, dense = make_csr(n, g, data_dtype, seed=1000 * n + g)
            if n >= 3:
                assert indptr[1] == 0 and indptr[-1] == indptr[-2]            # leading and trailing empty rows
                assert indptr[2] - indptr[1] == g                             # a full row
            if g == 130:
                assert (np.diff(indptr) > 64).any()                           # more entries than lanes
            for side in (0, 1):
                _check_case(k, indptr, indices, data, dense, metric, side, f"{metric} side {side} {n} x {g} {dtype}")


@pytest.mark.parametrize("dtype", CELL_DTYPES)
def test_single_rows(dtype):
    """n = 1: an empty row, and a single entry in the last column."""
    k = _k(dtype)
    for g in (1, 17, 65):
        for cols in ([], [g - 1]):
            indptr = np.array([0, len(cols)], dtype=np.int64)
            indices, data = np.asarray(cols, dtype=np.int32), np.full(len(cols), 3.25)
            dense = np.zeros((1, g))
            dense[0, cols] = 3.25
            for metric in PRODUCT_METRICS:
                _check_case(k, indptr, indices, data, dense, metric, 0, f"{metric} 1 x {g} {cols}")


@pytest.mark.parametrize("dtype", CELL_DTYPES)
def test_out_of_range_indices_are_skipped(dtype):
    """Entries with a column outside [0, g) are never used as an address: the result is that of the matrix without them."""
    k = _k(dtype)
    rng = np.random.default_rng(5)
    for n, g in ((5, 17), (257, 65)):
        indptr, indices, data, dense = make_csr(n, g, np.float64, seed=n + g)
        wild = [g, g + 5, -1, np.iinfo(np.int32).max, np.iinfo(np.int32).min]
        ip, ix, dv = [0], [], []
        for i in range(n):
            sl = slice(indptr[i], indptr[i + 1])
            extra = rng.choice(wild, size=i % 3)
            cols, vals = np.concatenate([indices[sl], extra]), np.concatenate([data[sl], 1e30 * np.ones(len(extra))])
            order = rng.permutation(len(cols))
            ix.append(cols[order]), dv.append(vals[order])
            ip.append(ip[-1] + len(cols))
        ip, ix, dv = np.asarray(ip, dtype=np.int64), np.concatenate(ix).astype(np.int32), np.concatenate(dv)
        assert len(ix) > len(indices)
        for metric in PRODUCT_METRICS:
            for side in (0, 1):
                _check_case(k, ip, ix, dv, dense, metric, side, f"wild {metric} side {side} {n} x {g}")


def test_error_returns_and_the_empty_call():
    from spateo_amd import _lib

    k = _k("float64")
    lib = k.lib
    n, g = 5, 17
    indptr, indices, data, _ = make_csr(n, g, np.float64, seed=0)
    dev = _upload(indptr, indices, data)
    ld = int(lib.mvf_assign_padded_features(g, ec.METRICS["kl"]))
    need = int(lib.mvf_assign_prepare_csr_min_workspace_bytes(g))
    assert lib.mvf_assign_prepare_csr_min_workspace_bytes(0) == 0 and lib.mvf_assign_prepare_csr_min_workspace_bytes(-3) == 0
    Lp, ab, ws = _guarded(n * ld), _guarded(n), _guarded(need // 8)

    def call(indptr=dev[0].data_ptr(), indices=dev[1].data_ptr(), data=dev[2].data_ptr(), n=n, metric=ec.METRICS["kl"], side=0,
             Lp=Lp.data_ptr(), ld=ld, ab=ab.data_ptr(), ws=ws.data_ptr(), ws_bytes=need, dtype=_lib.MVF_F64):
        status = lib.mvf_assign_prepare_csr(indptr, indices, data, 0, n, g, metric, side, Lp, ld, ab, ws, ws_bytes, dtype, k._stream())
        return status, lib.mvf_last_error().decode()

    status, msg = call(metric=_lib.ASSIGN_LABEL)
    assert status != 0 and "bad metric 5" in msg
    status, msg = call(ld=ld + 16)
    assert status != 0 and "ld must be" in msg
    status, msg = call(side=2)
    assert status != 0 and "side" in msg
    status, msg = call(dtype=7)
    assert status != 0 and "bad dtype" in msg
    for name in ("indptr", "indices", "data", "Lp", "ab", "ws"):
        status, msg = call(**{name: None})
        assert status != 0 and "null pointer" in msg, name
    status, msg = call(ws_bytes=need - 8)
    assert status != 0 and "workspace" in msg
    torch.cuda.synchronize()
    assert bool(torch.isnan(Lp[: n * ld]).all()) and bool(torch.isnan(ab[:n]).all())      # nothing was launched
    assert call(n=0)[0] == 0 and lib.mvf_assign_prepare_csr(None, None, None, 0, 0, g, 2, 0, None, ld, None, None, 0, _lib.MVF_F64,
                                                            None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(Lp[: n * ld]).all())                                             # n == 0 launches nothing
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(Lp[: n * ld]).any()) and _intact(Lp, n * ld) and _intact(ab, n) and _intact(ws, need // 8)
