"""Kernel-level tests of ``csrc/mvf_kde.hip`` through the raw C ABI on ``cuda:0``.  References and bounds come from
tests/_kde_cases.py (proved against sklearn and the golden by tests/test_kde_kernel_refs.py): every case in both storage dtypes
within its bound - 64 x the larger of the restatement's forward / reversed deviation and its deviation from sklearn, floor
16 ulp of max(1, |ref|); the cases on which sklearn itself is far off within the tighter bound of ``TIGHT`` as well -, the
-inf pattern equal entry for entry, two calls bit-equal, and every output and workspace in front of a guard that must stay
untouched.  More than 64 columns run in chunks of 64, as the host runs them."""
import numpy as np
import pytest
import torch

import _kde_cases as kc
from _kernel_scaffold import (MODES, called as _called, dev as _dev, guarded as _guarded, intact as _intact, ptr as _ptr,
                              same_bits as _same_bits, stream as _stream, take as _take, under as _under, x4 as _x4)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from spateo_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def _raw(lib, case, dtype):
    """Unnormalised (n, C) log sums of a case, the columns in chunks of 64; guards checked."""
    from spateo_amd import _lib

    t4, s4 = _x4(case["T"], dtype), _x4(case["X"], dtype)
    n, N, C = len(case["T"]), len(case["X"]), case["C"]
    w = None if case["w"] is None else _dev(case["w"])
    out = np.empty((n, C))
    for c0 in range(0, C, kc.MAX_COLUMNS):
        cc = min(kc.MAX_COLUMNS, C - c0)
        g = None if case["g"] is None else _dev(case["g"] - c0, torch.int32)
        need = int(lib.mvf_kde_workspace_bytes(n, N, cc))
        assert need == (kc.splits(n, N) + 1) * n * cc * 8
        ws, o = _guarded(need // 8), _guarded(n * cc)
        rc = lib.mvf_kde(_ptr(t4), n, _ptr(s4), N, case["d"], kc.CODES[case["kernel"]], case["h"], _ptr(w), _ptr(g), cc, _ptr(o),
                         _ptr(ws), need, _lib.MVF_F32 if dtype == "float32" else _lib.MVF_F64, _stream())
        assert rc == 0, lib.mvf_last_error()
        _called()
        torch.cuda.synchronize()
        _take(ws, need // 8)
        out[:, c0 : c0 + cc] = _take(o, n * cc).reshape(n, cc)
    return out


@pytest.mark.parametrize("dtype", ("float64", "float32"))
@pytest.mark.parametrize("name", kc.NAMES)
def test_case_within_its_bound_and_bit_stable(lib, name, dtype):
    case = kc.CASES[name]
    ref, bound, tight, dev_order, dev_sk = kc.reference(name, dtype)
    raw = _raw(lib, case, dtype)
    got = kc.normalise(raw, len(case["X"]), case["d"], case["kernel"], case["h"], case["w"], case["g"], case["C"])
    share = kc.compare(got, ref, bound)
    fin = np.isfinite(ref)
    err = float((np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max()) if fin.any() else 0.0
    line = (f"kde {name} [{dtype}] n={len(case['T'])} N={len(case['X'])} C={case['C']} splits={kc.splits(len(case['T']), len(case['X']))}: "
            f"err {err:.3e}, dev_order {dev_order:.3e}, dev_sklearn {dev_sk:.3e}, share of the bound {share:.4f}")
    if tight is not None:
        tshare = kc.compare(got, ref, tight)
        line += f", share of the tight bound {tshare:.4f}"
    print(line)
    assert share <= 1.0
    if tight is not None:
        assert tshare <= 1.0
    if case["far"]:
        far = got[-case["far"] :]
        if case["kernel"] in kc.COMPACT:
            assert np.isneginf(far).all()
        else:
            assert np.isfinite(far).all() and (far < -790.0).all()   # where a plain sum gives log 0 = -inf
    raw2 = _raw(lib, case, dtype)
    assert np.array_equal(raw2.view(np.uint64), raw.view(np.uint64))


CONVENTION_COVERS = {"mvf_kde": MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", ("float64", "float32"))
@pytest.mark.parametrize("name", ["n257_N255", "n40_N4097", "C2_shift_expo"])   # one split; two; weights and groups
def test_calling_conventions(lib, name, dtype, mode):
    """The plain call's bits on a side stream behind poisoned inputs, at displaced pointers, and with the inputs unchanged."""
    assert kc.splits(len(kc.CASES[name]["T"]), len(kc.CASES[name]["X"])) == (2 if name == "n40_N4097" else 1)
    plain, got = _under(mode, lambda: _raw(lib, kc.CASES[name], dtype))
    assert _same_bits(plain, got)


def test_a_column_does_not_depend_on_the_other_columns(lib):
    """The split is a function of (n, N) alone and a source belongs to one column: column c of a grouped call equals the
    single column of a call whose weights keep group c only, bit for bit - here over two splits."""
    case = dict(kc.CASES["C65_N4097"])
    assert kc.splits(len(case["T"]), len(case["X"])) == 2
    full = _raw(lib, case, "float64")
    for c in (0, 7, 63, 64):
        one = dict(case, g=None, C=1, w=(case["g"] == c).astype(np.float64))
        assert np.array_equal(_raw(lib, one, "float64")[:, 0].view(np.uint64), full[:, c].view(np.uint64)), c


def test_no_sources_fills_minus_infinity_and_empty_calls_launch_nothing(lib):
    from spateo_amd import _lib

    t4 = _x4(np.zeros((300, 3)), "float64")
    o = _guarded(300 * 3)
    assert lib.mvf_kde(_ptr(t4), 300, None, 0, 3, 0, 1.0, None, None, 3, _ptr(o), None, 0, _lib.MVF_F64, _stream()) == 0
    torch.cuda.synchronize()
    assert np.isneginf(_take(o, 900)).all()
    o = _guarded(16)
    assert lib.mvf_kde(_ptr(t4), 0, _ptr(t4), 300, 3, 0, 1.0, None, None, 1, _ptr(o), None, 0, _lib.MVF_F64, _stream()) == 0
    assert lib.mvf_kde(_ptr(t4), 300, _ptr(t4), 300, 3, 0, 1.0, None, None, 0, _ptr(o), None, 0, _lib.MVF_F64, _stream()) == 0
    torch.cuda.synchronize()
    assert _intact(o, 0)  # (from element 0 on: nothing at all was written)


def test_refusals_on_device_buffers(lib):
    from spateo_amd import _lib

    case = kc.CASES["n257_N255"]
    t4, s4 = _x4(case["T"], "float64"), _x4(case["X"], "float64")
    n, N = len(case["T"]), len(case["X"])
    need = int(lib.mvf_kde_workspace_bytes(n, N, 1))
    ws, o = _guarded(need // 8), _guarded(n)
    base = dict(t4=_ptr(t4), n=n, s4=_ptr(s4), N=N, d=3, kernel=0, h=0.3, C=1, out=_ptr(o), ws=_ptr(ws), ws_bytes=need, dtype=_lib.MVF_F64)
    for kw, msg in ((dict(d=0), b"bad shape"), (dict(d=4), b"bad shape"), (dict(C=65), b"bad shape"), (dict(h=0.0), b"bad shape"),
                    (dict(h=float("nan")), b"bad shape"), (dict(n=-1), b"bad shape"), (dict(kernel=6), b"bad kernel"),
                    (dict(kernel=-1), b"bad kernel"), (dict(dtype=7), b"bad dtype"), (dict(t4=None), b"null pointer"),
                    (dict(s4=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                    (dict(ws_bytes=need - 1), b"workspace too small")):
        a = dict(base, **kw)
        rc = lib.mvf_kde(a["t4"], a["n"], a["s4"], a["N"], a["d"], a["kernel"], a["h"], None, None, a["C"], a["out"], a["ws"],
                         a["ws_bytes"], a["dtype"], _stream())
        assert rc != 0 and b"mvf_kde" in lib.mvf_last_error() and msg in lib.mvf_last_error(), (kw, lib.mvf_last_error())
    torch.cuda.synchronize()
    assert _intact(o, 0) and _intact(ws, 0)
