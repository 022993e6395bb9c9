"""Kernel-level edge tests of ``mvf_eval_wide`` (csrc/mvf_eval_wide.hip) through the raw C ABI on ``cuda:0``, both cell dtypes:
values v = K @ C (n x dy) and the Jacobian (dy, d, n) of a field with any number of output columns at d = 1, 2, 3, against the
NumPy reference of tests/_eval_wide_cases.py on the SAME inputs (rounded to the cell dtype), one varied axis at a time around
(n, m, dy, d) = (65, 259, 65, 3): the 16-query tile / 64-query workgroup, the k-step of 4 and the 64-point staging chunk, the
16-column tile and the 64-column panel, every d; the flag subsets with the unrequested pointer NULL; row strides with padding
that must survive; column offsets as the chunked host path passes them; bit-equal repeats; agreement with mvf_eval at dy = 3;
empty problems.  Tolerance: _cell_cases.TOL of each quantity's maximum (tests/test_eval_wide_refs.py shows without a GPU that
the inputs keep it meaningful and that each targeted slip is 1000 tolerances large).  Every output buffer is followed by a guard
that must come back untouched."""
import numpy as np
import pytest
import torch

import _eval_wide_cases as wc
from _cell_cases import EVAL_JAC, EVAL_V, TOL, relmax
from _kernel_scaffold import (DEV, DTYPES, MODES, SENTINEL as _SENTINEL, called as _called, dev as _dev, guarded as _buf,
                              intact as _intact, kernel_cache, same_bits as _same_bits, under as _under, x4 as _sx4)

pytestmark = pytest.mark.gpu

SENTINEL = _SENTINEL[torch.float64]  # (every output of the evaluator is float64: what the host copies below are compared with)
_k = kernel_cache()


def _inputs(dtype, n, m, dy, d):
    k = _k(dtype)
    c = wc.wide_case(n, m, dy, d)
    x4 = k.to_x4(c["X"]) if n else torch.zeros(0, 4, dtype=k.tdtype, device=DEV)
    c4 = k.to_x4(c["ctrl"]) if m else torch.zeros(0, 4, dtype=k.tdtype, device=DEV)
    Cd = torch.from_numpy(np.array(c["C"])).to(DEV)  # (a copy: the shared case is read-only)
    return k, c, x4, c4, Cd


def _run(k, x4, c4, d, beta, C_ptr, ldc, dy, flags, v_ptr, ldv, jac_ptr):
    from spateo_amd import _lib

    with torch.cuda.device(DEV):
        rc = k.lib.mvf_eval_wide(x4.data_ptr() or None, x4.shape[0], c4.data_ptr() or None, c4.shape[0], d, float(beta), C_ptr,
                                 ldc, dy, flags, v_ptr, ldv, jac_ptr, k.cdtype, k._stream())
    _lib.check(rc, "mvf_eval_wide")
    _called()


def _scaffold_inputs(dtype, n, m, dy, d):
    """``_inputs`` from the scaffold's own allocations (not ``HipKernels.to_x4``), so that every calling mode reaches them."""
    c = wc.wide_case(n, m, dy, d)
    return _k(dtype), c, _sx4(c["X"], dtype), _sx4(c["ctrl"], dtype), _dev(np.array(c["C"]))


def _eval(dtype, n, m, dy, d, flags=EVAL_V | EVAL_JAC, inputs=None):
    """One plain call (contiguous C and v): {flag: host array}, guards checked."""
    k, c, x4, c4, Cd = (inputs or _inputs)(dtype, n, m, dy, d)
    vb, jb = _buf(n * dy), _buf(dy * d * n)
    _run(k, x4, c4, d, c["beta"], Cd.data_ptr() or None, dy, dy, flags, vb.data_ptr() if flags & EVAL_V else None, dy,
         jb.data_ptr() if flags & EVAL_JAC else None)
    v, j = vb.cpu().numpy(), jb.cpu().numpy()
    assert np.all(v[n * dy:] == SENTINEL) and np.all(j[dy * d * n:] == SENTINEL), "wrote behind an output"
    out = {}
    if flags & EVAL_V:
        out[EVAL_V] = v[: n * dy].reshape(n, dy)
    else:
        assert np.all(v == SENTINEL)
    if flags & EVAL_JAC:
        out[EVAL_JAC] = j[: dy * d * n].reshape(dy, d, n)
    else:
        assert np.all(j == SENTINEL)
    return out


def _check(got, n, m, dy, d, dtype, what):
    ref = wc.case_reference(n, m, dy, d, dtype)
    for f, a in got.items():
        e = relmax(a, ref[f])
        print(f"eval_wide {what} n={n} m={m} dy={dy} d={d} {dtype} {'v' if f == EVAL_V else 'jac'}: {e:.2e}")
        assert np.all(np.isfinite(a)) and e <= TOL[dtype], (what, f, e)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,dy,d", wc.SWEEP)
def test_values_and_jacobian_at_tile_chunk_and_panel_edges(dtype, n, m, dy, d):
    got = _eval(dtype, n, m, dy, d)
    assert got[EVAL_V].shape == (n, dy) and got[EVAL_JAC].shape == (dy, d, n)
    _check(got, n, m, dy, d, dtype, "sweep")
    again = _eval(dtype, n, m, dy, d)
    for f in got:
        assert got[f].tobytes() == again[f].tobytes(), "two calls differ"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", wc.DS)
@pytest.mark.parametrize("flags", [EVAL_V, EVAL_JAC, EVAL_V | EVAL_JAC])
def test_flag_subsets_with_the_unrequested_pointer_null(dtype, d, flags):
    n, m, dy, _ = wc.BASE
    got = _eval(dtype, n, m, dy, d, flags)
    assert set(got) == {f for f in (EVAL_V, EVAL_JAC) if flags & f}
    _check(got, n, m, dy, d, dtype, f"flags={flags}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dy", [5, 65])
def test_row_strides_with_padding_that_survives(dtype, dy):
    n, m, _, d = wc.BASE
    k, c, x4, c4, Cd = _inputs(dtype, n, m, dy, d)
    plain = _eval(dtype, n, m, dy, d)
    ldc, ldv = dy + 3, dy + 5
    Cp = torch.full((m, ldc), float("nan"), dtype=torch.float64, device=DEV)  # padding the kernel must not read into a sum
    Cp[:, :dy] = Cd
    vb, jb = _buf(n * ldv), _buf(dy * d * n)
    _run(k, x4, c4, d, c["beta"], Cp.data_ptr(), ldc, dy, EVAL_V | EVAL_JAC, vb.data_ptr(), ldv, jb.data_ptr())
    v, j = vb.cpu().numpy(), jb.cpu().numpy()
    assert np.all(v[n * ldv:] == SENTINEL) and np.all(j[dy * d * n:] == SENTINEL)
    v = v[: n * ldv].reshape(n, ldv)
    assert np.all(v[:, dy:] == SENTINEL), "the padding columns of v were touched"
    assert v[:, :dy].tobytes() == plain[EVAL_V].tobytes() and j[: dy * d * n].tobytes() == plain[EVAL_JAC].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("f0,f1", [(0, 64), (64, 130), (3, 20), (129, 130)])
def test_column_offsets_as_the_chunked_host_path_passes_them(dtype, f0, f1):
    """C + f0 with the full ldc, v + f0 with the full ldv, jac[f0:f1]: the same bits as those columns of the whole call."""
    n, m, _, d = wc.BASE
    dy = 130
    k, c, x4, c4, Cd = _inputs(dtype, n, m, dy, d)
    whole = _eval(dtype, n, m, dy, d)
    w = f1 - f0
    vb, jb = _buf(n * dy), _buf(w * d * n)
    _run(k, x4, c4, d, c["beta"], Cd.data_ptr() + 8 * f0, dy, w, EVAL_V | EVAL_JAC, vb.data_ptr() + 8 * f0, dy, jb.data_ptr())
    v, j = vb.cpu().numpy(), jb.cpu().numpy()
    assert np.all(v[n * dy:] == SENTINEL) and np.all(j[w * d * n:] == SENTINEL)
    v = v[: n * dy].reshape(n, dy)
    assert np.all(v[:, :f0] == SENTINEL) and np.all(v[:, f1:] == SENTINEL), "columns outside the chunk were touched"
    assert v[:, f0:f1].tobytes() == whole[EVAL_V][:, f0:f1].tobytes()
    assert j[: w * d * n].tobytes() == whole[EVAL_JAC][f0:f1].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", [(65, 259), (257, 65), (17, 5)])
def test_three_columns_agree_with_mvf_eval(dtype, n, m):
    k, c, x4, c4, Cd = _inputs(dtype, n, m, 3, 3)
    wide = _eval(dtype, n, m, 3, 3)
    narrow = {f: t.cpu().numpy() for f, t in k.eval(x4, c4, c["beta"], Cd, EVAL_V | EVAL_JAC).items()}
    for f in (EVAL_V, EVAL_JAC):
        assert wide[f].shape == narrow[f].shape and relmax(wide[f], narrow[f]) <= TOL[dtype], f


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_problems(dtype):
    k = _k(dtype)
    n, m, dy, d = 17, 5, 9, 3
    _, c, x4, c4, Cd = _inputs(dtype, n, m, dy, d)
    empty4 = torch.zeros(0, 4, dtype=k.tdtype, device=DEV)
    vb, jb = _buf(n * dy), _buf(dy * d * n)
    both = EVAL_V | EVAL_JAC
    _run(k, empty4, c4, d, c["beta"], Cd.data_ptr(), dy, dy, both, vb.data_ptr(), dy, jb.data_ptr())      # n = 0
    _run(k, x4, c4, d, c["beta"], Cd.data_ptr(), dy, 0, both, vb.data_ptr(), dy, jb.data_ptr())           # dy = 0
    torch.cuda.synchronize()
    assert _intact(vb, 0) and _intact(jb, 0), "an empty problem wrote something"
    _run(k, x4, empty4, d, c["beta"], None, dy, dy, both, vb.data_ptr(), dy, jb.data_ptr())               # m = 0: zeros
    v, j = vb.cpu().numpy(), jb.cpu().numpy()
    assert np.all(v[: n * dy] == 0.0) and np.all(j[: dy * d * n] == 0.0)
    assert np.all(v[n * dy:] == SENTINEL) and np.all(j[dy * d * n:] == SENTINEL)


CONVENTION_COVERS = {"mvf_eval_wide": MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dy,d", [(65, 3), (17, 2), (3, 1)])   # two column panels at d = 3; one tile and a partial one; one partial tile
def test_calling_conventions(dtype, dy, d, mode):
    """Values and Jacobian: the plain call's bits on a side stream behind poisoned inputs, at displaced pointers, and with the
    inputs unchanged."""
    plain, got = _under(mode, lambda: _eval(dtype, 65, 259, dy, d, inputs=_scaffold_inputs))
    assert _same_bits(plain[EVAL_V], got[EVAL_V]) and _same_bits(plain[EVAL_JAC], got[EVAL_JAC])
