"""Kernel-level tests of ``csrc/mvf_conk.hip`` through the raw C ABI on ``cuda:0``: ``mvf_con_k`` in its four kernels (row
form with RS = 1 / 2 / 4 and NP = 1 ... 8, flat form below and above 64 KB of LDS, 2-D form with its scalar tail) and
``mvf_con_k_d``.  Every shape of tests/_prep_cases.py runs under all four settings of the developer option ``conk_form`` (0 the
host's own choice, 1 rows, 2 flat, 3 2-D; a form that does not apply falls through to the next, as launch_conk states it): the
four results are bit-equal, twice in a row, within the project's own 1e-11 (float64) / 2e-5 (float32) of the np.longdouble
reference on the inputs as the kernel sees them, and nothing is written behind K.  ``mvf_con_k_d``'s differences are one IEEE
subtraction each: compared bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import _prep_cases as pc
from _kernel_scaffold import (DTYPES, MODES, Out, called as _called, deviation_table, dev as _dev, option, same_bits as _same_bits,
                              stream as _stream, under as _under)

pytestmark = pytest.mark.gpu

_note, _deviation_table = deviation_table("| case family | dtype: quantity | largest |",
                                          footer=lambda seconds, notes: f"test_gpu_conk_kernels: {seconds:.1f} s")
_T = {"float32": torch.float32, "float64": torch.float64}
FORMS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def lib():
    from spateo_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def _code(dtype):
    from spateo_amd import _lib

    return _lib.MVF_F32 if dtype == "float32" else _lib.MVF_F64


def _err(lib):
    return lib.mvf_last_error() or b""


def _conk_raw(lib, xd, yd, n, m, d, beta, dtype, code=None, x=True, y=True, out=True):
    """(rc, K as an ``Out`` of n m elements of the cell dtype) of one raw call; the guards either side of K checked."""
    K = Out(max(n * m, 1), dtype=_T[dtype])
    rc = lib.mvf_con_k(xd.data_ptr() if x else None, n, yd.data_ptr() if y else None, m, d, ctypes.c_double(beta),
                       K.ptr if out else None, _code(dtype) if code is None else code, _stream())
    _called()
    torch.cuda.synchronize()
    assert K.guards_intact(), "wrote outside K"
    return rc, K


def _all_forms(lib, x, y, beta, dtype):
    """The (n, m) result under conk_form = 3 (2-D) after asserting that every form gives its bits, twice."""
    n, m, d = len(x), len(y), x.shape[1]
    xd, yd = _dev(x, None), _dev(y, None)
    got = {}
    for form in FORMS:
        with option("conk_form", form):
            rc, K = _conk_raw(lib, xd, yd, n, m, d, beta, dtype)
            assert rc == 0, (form, _err(lib))
            rc, K2 = _conk_raw(lib, xd, yd, n, m, d, beta, dtype)
        got[form] = K.host()[:n * m].reshape(n, m)
        assert rc == 0 and _same_bits(K2.host(), K.host()), form
    for form in (0, 1, 2):
        assert _same_bits(got[form], got[3]), f"conk_form = {form} differs from the 2-D form at n = {n}, m = {m}, d = {d}"
    return got[3]


def _note_deviation(family, dtype, err):
    _note(family, f"{dtype}: absolute deviation from np.longdouble", err)
    _note(family, f"{dtype}: share of the bound {pc.CONK_TOL[dtype]:g}", err / pc.CONK_TOL[dtype])


def _check_shape(lib, family, dtype, n, m, d):
    x, y = pc.conk_points(n, m, d, dtype)
    K = _all_forms(lib, x, y, pc.CONK_BETA, dtype)
    err = pc.compare_conk(K, pc.conk_reference(x, y, pc.CONK_BETA))
    _note_deviation(family, dtype, err)
    assert err <= pc.CONK_TOL[dtype], (family, dtype, n, m, d, err)
    return err


@pytest.mark.parametrize("name", tuple(pc.CONK_ROW_CASES) + tuple(pc.CONK_FLAT_CASES))
def test_con_k_forms_are_bit_equal_at_the_edges_of_the_row_and_flat_forms(lib, name):
    case = {**pc.CONK_ROW_CASES, **pc.CONK_FLAT_CASES}[name]
    family = "row form RS = %d" % case["rs"] if "rs" in case else "flat form"
    if "rs" in case and not case["fits"]:
        family = "first m past the row form"
    worst = max(_check_shape(lib, f"con_k d = 3, {family}", case["dtype"], n, case["m"], 3) for n in case["ns"])
    print(f"con_k {name}: n in {case['ns']}, worst {worst:.3g} [{case['branch']}]")


@pytest.mark.parametrize("d", range(1, 9))
@pytest.mark.parametrize("dtype", DTYPES)
def test_con_k_2d_form_tails_and_dimensions(lib, dtype, d):
    """m either side of one vector and of one block of 256 vectors (the scalar tail: m % VEC != 0), n either side of the 32
    rows a workgroup walks, d = 1 ... 8 (templated at 2 and 3, a run-time loop elsewhere)."""
    worst = max(_check_shape(lib, "con_k 2-D form, d = 1 .. 8", dtype, n, m, d) for m in pc.conk_2d_ms(dtype) for n in pc.CONK_2D_NS)
    print(f"con_k 2-D form [{dtype}] d = {d}: m in {pc.conk_2d_ms(dtype)}, n in {pc.CONK_2D_NS}, worst {worst:.3g}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_con_k_exact_properties(lib, dtype):
    rs4 = {"float32": 68, "float64": 66}[dtype]
    for m in (64, 72, rs4, 1 + 256 * pc.VEC[dtype]):
        x, y = pc.conk_points(m, m, 3, dtype)
        ones = _all_forms(lib, x[:5], y, 0.0, dtype)                   # beta = 0: every element exactly 1
        assert (ones == 1.0).all()
        K = _all_forms(lib, y, y, pc.CONK_BETA, dtype)                 # con_k(y, y): unit diagonal, symmetric by bits
        assert (np.diag(K) == 1.0).all() and _same_bits(K, np.ascontiguousarray(K.T))
        assert ((K > 0) & (K <= 1)).all()
    if dtype == "float64":                                              # 0.3 x 100^2 x log2(e) > 1075: exactly zero
        x, y = pc.conk_points(7, 64, 3, dtype)
        far = _all_forms(lib, x + 100.0, y, pc.CONK_BETA, dtype)
        assert (far == 0.0).all() and not np.signbit(far).any()


def test_con_k_empty_calls_and_refusals(lib):
    for dtype in DTYPES:
        x, y = pc.conk_points(5, 68, 3, dtype)
        xd, yd = _dev(x, None), _dev(y, None)
        for n, m in ((0, 68), (5, 0), (0, 0)):
            rc, K = _conk_raw(lib, xd, yd, n, m, 3, 0.3, dtype, x=False, y=False, out=False)
            assert rc == 0, _err(lib)
            rc, K = _conk_raw(lib, xd, yd, n, m, 3, 0.3, dtype)
            assert rc == 0 and K.untouched()
        for kw, msg in ((dict(d=0), b"bad shape"), (dict(d=9), b"bad shape"), (dict(n=-1), b"bad shape"), (dict(m=-1), b"bad shape"),
                        (dict(beta=-1e-300), b"beta"), (dict(beta=float("nan")), b"beta"), (dict(beta=float("inf")), b"beta"),
                        (dict(code=7), b"bad dtype"), (dict(x=False), b"null pointer"), (dict(y=False), b"null pointer"),
                        (dict(out=False), b"null pointer")):
            a = dict(n=5, m=68, d=3, beta=0.3)
            a.update(kw)
            rc, K = _conk_raw(lib, xd, yd, a.pop("n"), a.pop("m"), a.pop("d"), a.pop("beta"), dtype, **a)
            assert rc != 0 and b"mvf_con_k" in _err(lib) and msg in _err(lib), (kw, _err(lib))
            assert K.untouched(), kw


# ============================================================================================================== con_k_d
def _conk_d_raw(lib, xd, yd, n, m, d, beta, dtype, D=True):
    K, Dd = Out(max(n * m, 1), dtype=_T[dtype]), Out(max(n * d * m, 1), dtype=_T[dtype])
    rc = lib.mvf_con_k_d(xd.data_ptr(), n, yd.data_ptr(), m, d, ctypes.c_double(beta), K.ptr, Dd.ptr if D else None, _code(dtype),
                         _stream())
    _called()
    torch.cuda.synchronize()
    assert K.guards_intact() and Dd.guards_intact(), "wrote outside K or D"
    return rc, K, Dd


# ================================================================================================== calling conventions
CONVENTION_COVERS = {"mvf_con_k": MODES, "mvf_con_k_d": MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", (1, 2, 3), ids=("rows", "flat", "2d"))
def test_con_k_calling_conventions(lib, form, dtype, mode):
    """The plain call's bits on a side stream behind poisoned inputs, at displaced pointers (x, y and K one element off: the
    vector stores of every form must not rely on the allocation's alignment), and with the inputs unchanged."""
    n, m, d = 37, 68, 3
    x, y = pc.conk_points(n, m, d, dtype)

    def call():
        rc, K = _conk_raw(lib, _dev(x, None), _dev(y, None), n, m, d, pc.CONK_BETA, dtype)
        assert rc == 0, _err(lib)
        return K.host()

    with option("conk_form", form):
        plain, got = _under(mode, call)
    assert _same_bits(plain, got)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_con_k_d_calling_conventions(lib, dtype, mode):
    n, m, d = 37, 68, 3
    x, y = pc.conk_points(n, m, d, dtype, seed=5)

    def call():
        rc, K, D = _conk_d_raw(lib, _dev(x, None), _dev(y, None), n, m, d, pc.CONK_BETA, dtype)
        assert rc == 0, _err(lib)
        return np.concatenate([K.host(), D.host()])

    plain, got = _under(mode, call)
    assert _same_bits(plain, got)


@pytest.mark.parametrize("d", range(1, 9))
@pytest.mark.parametrize("dtype", DTYPES)
def test_con_k_d_differences_are_bit_exact_and_k_is_con_k(lib, dtype, d):
    for m in pc.CONK_D_MS:
        for n in pc.CONK_D_NS:
            x, y = pc.conk_points(n, m, d, dtype, seed=5)
            xd, yd = _dev(x, None), _dev(y, None)
            rc, K, D = _conk_d_raw(lib, xd, yd, n, m, d, pc.CONK_BETA, dtype)
            assert rc == 0, _err(lib)
            assert _same_bits(D.host()[:n * d * m].reshape(n, d, m), pc.conk_diff_reference(x, y)), (n, m)
            rc, K1 = _conk_raw(lib, xd, yd, n, m, d, pc.CONK_BETA, dtype)
            assert rc == 0 and _same_bits(K.host(), K1.host()), (n, m)
            rc, K2, D2 = _conk_d_raw(lib, xd, yd, n, m, d, pc.CONK_BETA, dtype)
            assert rc == 0 and _same_bits(K2.host(), K.host()) and _same_bits(D2.host(), D.host())
            err = pc.compare_conk(K.host()[:n * m].reshape(n, m), pc.conk_reference(x, y, pc.CONK_BETA))
            _note_deviation("con_k_d: K", dtype, err)
            assert err <= pc.CONK_TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_con_k_d_row_limit_and_empty_calls(lib, dtype):
    x, y = pc.conk_points(65536, 1, 1, dtype)
    xd, yd = _dev(x, None), _dev(y, None)
    rc, K, D = _conk_d_raw(lib, xd, yd, 65535, 1, 1, pc.CONK_BETA, dtype)
    assert rc == 0, _err(lib)
    assert _same_bits(D.host()[:65535].reshape(65535, 1, 1), pc.conk_diff_reference(x[:65535], y))
    assert pc.compare_conk(K.host()[:65535].reshape(65535, 1), pc.conk_reference(x[:65535], y, pc.CONK_BETA)) <= pc.CONK_TOL[dtype]
    rc, K, D = _conk_d_raw(lib, xd, yd, 65536, 1, 1, pc.CONK_BETA, dtype)
    assert rc != 0 and b"mvf_con_k_d" in _err(lib) and b"65535" in _err(lib), _err(lib)
    assert D.untouched()
    rc, K1 = _conk_raw(lib, xd, yd, 65536, 1, 1, pc.CONK_BETA, dtype)           # (K came first, as include/mvf.h states)
    assert rc == 0 and _same_bits(K.host(), K1.host())
    rc, K, D = _conk_d_raw(lib, xd, yd, 3, 1, 1, pc.CONK_BETA, dtype, D=False)
    assert rc != 0 and b"mvf_con_k_d" in _err(lib) and b"null D" in _err(lib)
    for n, m in ((0, 1), (3, 0)):
        rc, K, D = _conk_d_raw(lib, xd, yd, n, m, 1, pc.CONK_BETA, dtype, D=False)
        assert rc == 0 and K.untouched()
    rc, K, D = _conk_d_raw(lib, xd, yd, 3, 1, 9, pc.CONK_BETA, dtype)
    assert rc != 0 and b"bad shape" in _err(lib) and K.untouched() and D.untouched()
