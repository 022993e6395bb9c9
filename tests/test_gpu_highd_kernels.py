"""Kernel-level edge tests of csrc/mvf_highd.hip: ``eval_d_kernel<T, D, NCT>`` (mvf_eval_d, the fused MFMA evaluator in 4 to 8
dimensions) and ``ublk_build_d_kernel<T, D>`` (mvf_ublk_build_d, the kernel-value cache), with ``mvf_con_k`` at d = 4 .. 8 -
each on ``cuda:0`` in both cell dtypes against the plain NumPy reference of the same operation on the SAME inputs (the device's
own, rounded to the cell dtype where it is float32 and widened exactly), at the tile / workgroup / chunk / column-tile edges.

tests/_highd_cases.py builds the inputs and holds the shape lists and tolerances; tests/test_highd_kernel_refs.py proves without
a GPU that the float64 references are accurate to 1e-12, that the compared quantities are well conditioned over ALL queries,
that each targeted off-by-one moves a compared quantity by >= 1000 tolerances and that the cases reach every (D, NCT)
instantiation of the evaluator.

Tolerances: evaluator 1e-10 (float64) / 2e-4 (float32) of each quantity's maximum (_cell_cases.TOL; curvature with m <= 5 on
_highd_cases.curv_scale); mvf_con_k 1e-11 / 2e-5 (test_gpu_kernels.py::test_con_k_vs_oracle); cache against mvf_con_k,
repeated calls, flag subsets, prefixes of the query list, guards and refusals bit for bit.  Run with ``-s`` to see the largest
deviation of every case family and the module's running time (profiles/highd_kernel_edges.md records them)."""
import numpy as np
import pytest
import torch

import _highd_cases as hc
from _kernel_scaffold import (DEV, DTYPES, GUARD, MODES, bits_equal as _bits_equal, called as _called, dev as _dev,
                              deviation_table, guarded as _guarded, intact as _intact, kernel_cache, same_bits as _same_bits,
                              settle as _settle, take as _take, under as _under, written as _written)

pytestmark = pytest.mark.gpu

_k = kernel_cache()
_note, _deviation_table = deviation_table("| case family | dtype | largest deviation |",
                                           footer=lambda seconds, notes: f"test_gpu_highd_kernels: {seconds:.1f} s")


def _xd(k, a):
    a = np.asarray(a, dtype=np.float64)
    return k.to_xd(a) if len(a) else torch.zeros(0, a.shape[1], dtype=k.tdtype, device=DEV)


def _host(d):
    return {f: t.cpu().numpy() for f, t in d.items()}


def _setup(dtype, case):
    k = _k(dtype)
    return k, _xd(k, case["X"]), _xd(k, case["ctrl"]), _dev(case["C"])


def _ref(xd, cd, Cd, beta, flags):
    """The restatement on the device's inputs (float32 coordinates widened exactly)."""
    return hc.eval_d_reference(np.float64, xd.double().cpu().numpy(), cd.double().cpu().numpy(), Cd.cpu().numpy(), beta, flags)


def _columns(t, f, sl):
    """The queries `sl` of output f (the Jacobian keeps them in its last axis)."""
    return t[:, :, sl] if f == hc.EVAL_JAC else t[sl]


def _check_eval(dtype, family, n, m, d, dy, flags):
    case = hc.eval_case(n, m, d, dy)
    k, xd, cd, Cd = _setup(dtype, case)
    got_d = k.eval_d(xd, cd, case["beta"], Cd, flags)
    again = k.eval_d(xd, cd, case["beta"], Cd, flags)
    want = {f for f in hc.HD_FLAGS if flags & f}
    shapes = hc.out_shapes(n, d, dy)
    assert set(got_d) == want
    for f in want:
        assert got_d[f].shape == shapes[f] and got_d[f].dtype == torch.float64, hc.HD_NAMES[f]
        assert _bits_equal(got_d[f], again[f]), hc.HD_NAMES[f]
    errs = hc.eval_errors(_host(got_d), _ref(xd, cd, Cd, case["beta"], flags), m)
    print(f"eval_d {family} d={d} dy={dy} n={n} m={m} {dtype}: "
          + " ".join(f"{hc.HD_NAMES[f]}={e:.2e}" for f, e in errs.items()))
    for f, e in errs.items():
        on_scale = " (m <= 5, on curv_scale)" if f == hc.EVAL_CURV and m <= hc.FEW else ""
        _note(f"eval_d {family}: {hc.HD_NAMES[f]}{on_scale}", dtype, e)
    for f, e in errs.items():
        assert e <= hc.TOL[dtype], (hc.HD_NAMES[f], e)


# ------------------------------------------------------------------------------------------------------ evaluator
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,dy", hc.HD_GRID)
def test_eval_d_every_dimension_and_column_count(dtype, d, dy):
    """All 40 (d, dy): every (D, NCT) instantiation with the Jacobian columns, dy != d with its (dy, d, n) layout, and the
    column counts 16 / 32 / 48 / 64 where `col < ncols` is all that separates live from padded columns."""
    flags = hc.grid_flags(d, dy)
    _check_eval(dtype, f"grid nct={hc.nct(d, dy, flags)}", *hc.HD_GRID_SHAPE, d, dy, flags)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,dy,flags", hc.HD_SWEEP_DIMS)
@pytest.mark.parametrize("n,m", hc.HD_SWEEP)
def test_eval_d_at_tile_workgroup_chunk_and_k_step_edges(dtype, n, m, d, dy, flags):
    _check_eval(dtype, f"sweep nct={hc.nct(d, dy, flags)}", n, m, d, dy, flags)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", hc.HD_FLAG_DIMS)
def test_eval_d_flag_subsets_return_the_bits_of_the_all_flags_call(dtype, d):
    """Also the v-only product (NCT = 1, four query tiles per wave) against the Jacobian product: column f of [v | W]
    accumulates the same K x C[:, f] terms in the same k order in both."""
    case = hc.eval_case(257, 259, d, d)
    k, xd, cd, Cd = _setup(dtype, case)
    full = k.eval_d(xd, cd, case["beta"], Cd, hc.HD_ALL)
    subsets = [hc.EVAL_V, hc.EVAL_JAC, hc.EVAL_V | hc.EVAL_JAC | hc.EVAL_ACC | hc.EVAL_CURV]
    for flags in list(hc.HD_FLAGS) + subsets:
        part = k.eval_d(xd, cd, case["beta"], Cd, flags)
        assert set(part) == {f for f in hc.HD_FLAGS if flags & f}
        for f, t in part.items():
            assert _bits_equal(t, full[f]), (flags, hc.HD_NAMES[f])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,dy,flags", hc.HD_SWEEP_DIMS)
def test_eval_d_of_a_prefix_of_the_queries_is_the_prefix_of_the_results(dtype, d, dy, flags):
    """A query's result does not depend on its tile, wave or workgroup position, nor on how many queries follow it."""
    case = hc.eval_case(257, 259, d, dy)
    k, xd, cd, Cd = _setup(dtype, case)
    full = k.eval_d(xd, cd, case["beta"], Cd, flags)
    for p in hc.HD_PREFIXES:
        part = k.eval_d(xd[:p].contiguous(), cd, case["beta"], Cd, flags)
        assert set(part) == set(full)
        for f, t in part.items():
            assert _bits_equal(t, _columns(full[f], f, slice(0, p)).contiguous()), (p, hc.HD_NAMES[f])


def _eval_raw(k, xd, cd, Cd, beta, flags, *, n=None, m=None, d=None, dy=None, null=(), elems=None, nullin=False):
    """mvf_eval_d through the raw ABI.  Every output the flags ask for (all five when `elems` is given: elements per buffer)
    is followed by a guard and filled with the sentinel; those in `null` are passed as null.  Returns (rc, buffers)."""
    n = xd.shape[0] if n is None else n
    m = cd.shape[0] if m is None else m
    d = xd.shape[1] if d is None else d
    dy = Cd.shape[1] if dy is None else dy
    shapes = hc.out_shapes(xd.shape[0], xd.shape[1], Cd.shape[1])
    bufs = {}
    for f in hc.HD_FLAGS:
        if elems is not None or flags & f:
            size = int(np.prod(shapes[f])) if elems is None else elems
            bufs[f] = _guarded(size)
    ptr = [bufs[f].data_ptr() if f in bufs and f not in null else None for f in hc.HD_FLAGS]
    _settle()
    rc = k.lib.mvf_eval_d(xd.data_ptr(), n, None if nullin else cd.data_ptr(), m, d, float(beta),
                          None if nullin else Cd.data_ptr(), dy, int(flags), *ptr, k.cdtype, k._stream())
    _called()
    torch.cuda.synchronize()
    return rc, bufs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,dy", hc.HD_GUARD_DIMS)
@pytest.mark.parametrize("n", hc.HD_GUARD_NS)
def test_eval_d_writes_its_buffers_whole_and_nothing_behind_them(dtype, n, d, dy):
    """The live region holds the wrapper's bits (so every element is written, and v has the row stride dy for dy < 8)."""
    case = hc.eval_case(n, 259, d, dy)
    k, xd, cd, Cd = _setup(dtype, case)
    flags = hc.grid_flags(d, dy)
    full = k.eval_d(xd, cd, case["beta"], Cd, flags)
    shapes = hc.out_shapes(n, d, dy)
    for fl in (flags, hc.EVAL_V, hc.EVAL_JAC):
        rc, bufs = _eval_raw(k, xd, cd, Cd, case["beta"], fl)
        assert rc == 0 and set(bufs) == {f for f in hc.HD_FLAGS if fl & f}
        for f, b in bufs.items():
            live = b.numel() - GUARD
            assert _intact(b, live), hc.HD_NAMES[f]
            assert _bits_equal(b[:live].view(shapes[f]), full[f]), hc.HD_NAMES[f]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,dy", hc.HD_GUARD_DIMS)
@pytest.mark.parametrize("n", [17, 300])
def test_eval_d_without_control_points(dtype, n, d, dy):
    """m = 0: the empty sums.  v, J, div and acc hold no non-zero, the curvature is 0 / 0; the same with null ctrl / C."""
    case = hc.eval_case(n, 0, d, dy)
    k, xd, cd, Cd = _setup(dtype, case)
    assert cd.shape == (0, d) and Cd.shape == (0, dy)
    flags = hc.grid_flags(d, dy)
    got = _host(k.eval_d(xd, cd, case["beta"], Cd, flags))
    ref = _ref(xd, cd, Cd, case["beta"], flags)
    shapes = hc.out_shapes(n, d, dy)
    rc, bufs = _eval_raw(k, xd, cd, Cd, case["beta"], flags, nullin=True)
    assert rc == 0 and set(got) == set(ref) == set(bufs)
    for f, g in got.items():
        raw = bufs[f][: g.size].view(shapes[f]).cpu().numpy()
        assert g.shape == shapes[f] and _intact(bufs[f], g.size), hc.HD_NAMES[f]
        if f == hc.EVAL_CURV:
            assert np.isnan(g).all() and np.isnan(ref[f]).all() and np.isnan(raw).all()
        else:
            assert not g.any() and not ref[f].any() and not raw.any(), hc.HD_NAMES[f]


@pytest.mark.parametrize("dtype", DTYPES)
def test_eval_d_without_queries_returns_0_and_writes_nothing(dtype):
    case = hc.eval_case(17, 67, 5, 5)
    k, xd, cd, Cd = _setup(dtype, case)
    rc, bufs = _eval_raw(k, xd, cd, Cd, case["beta"], hc.HD_ALL, n=0)
    assert rc == 0 and len(bufs) == 5
    for f, b in bufs.items():
        assert _intact(b, 0), hc.HD_NAMES[f]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [4, 8])
def test_eval_d_where_every_kernel_value_underflows(dtype, d):
    """45 queries ~1000 units away along every axis: beta r^2 >= 4000 d, every kernel value is exactly 0 in float32 and in
    float64.  v, J, div and acc are exactly 0, the curvature is NumPy's 0 / 0, and the 300 near queries of the same launch
    keep the bits of the call without the far ones."""
    case = hc.eval_case(300, 259, d, d)
    rng = np.random.default_rng(5 + d)
    far = np.resize([1000.0, -900.0, 1100.0], d) * rng.choice([-1.0, 1.0], (45, d)) + rng.uniform(-30, 30, (45, d))
    both = dict(case, X=np.concatenate([case["X"], far]))
    k, xd, cd, Cd = _setup(dtype, both)
    got = k.eval_d(xd, cd, case["beta"], Cd, hc.HD_ALL)
    near = k.eval_d(xd[:300].contiguous(), cd, case["beta"], Cd, hc.HD_ALL)
    ref = _ref(xd, cd, Cd, case["beta"], hc.HD_ALL)
    for f in hc.HD_FLAGS:
        g_far = _columns(got[f], f, slice(300, None)).cpu().numpy()
        r_far = _columns(ref[f], f, slice(300, None))
        assert _bits_equal(_columns(got[f], f, slice(0, 300)).contiguous(), near[f]), hc.HD_NAMES[f]
        if f == hc.EVAL_CURV:
            np.testing.assert_array_equal(np.isnan(g_far), np.isnan(r_far))
            assert np.isnan(r_far).all()
        else:
            assert not g_far.any() and not r_far.any(), hc.HD_NAMES[f]


@pytest.mark.parametrize("dtype", DTYPES)
def test_eval_d_refusals_leave_the_outputs_untouched(dtype):
    """Every input and output buffer is large enough for d = dy = 9, whatever the call claims."""
    n, m = 65, 67
    rng = np.random.default_rng(9)
    k = _k(dtype)
    xd, cd = _dev(rng.uniform(-10, 10, (n, 9)), k.tdtype), _dev(rng.uniform(-10, 10, (m, 9)), k.tdtype)
    Cd = _dev(rng.uniform(0.5, 1.5, (m, 9)))
    V, J = hc.EVAL_V, hc.EVAL_JAC
    calls = {"d = 3": dict(d=3, dy=3, flags=V), "d = 9": dict(d=9, dy=8, flags=V),
             "dy = 0": dict(d=4, dy=0, flags=V), "dy = 9": dict(d=8, dy=9, flags=V),
             "curl": dict(d=4, dy=4, flags=V | hc.EVAL_CURL), "torsion": dict(d=4, dy=4, flags=V | hc.EVAL_TORS),
             "det J": dict(d=4, dy=4, flags=V | J | hc.EVAL_JDET),
             "div with dy != d": dict(d=5, dy=4, flags=V | hc.EVAL_DIV), "acc with dy != d": dict(d=4, dy=5, flags=hc.EVAL_ACC),
             "curv with dy != d": dict(d=8, dy=7, flags=V | J | hc.EVAL_CURV),
             "beta = 0": dict(d=4, dy=4, flags=V, beta=0.0), "beta = inf": dict(d=4, dy=4, flags=V, beta=float("inf")),
             "beta < 0": dict(d=4, dy=4, flags=V, beta=-hc.BETA), "no flags": dict(d=4, dy=4, flags=0)}
    for f in hc.HD_FLAGS:
        calls[f"null {hc.HD_NAMES[f]}"] = dict(d=6, dy=6, flags=hc.HD_ALL, null=(f,))
    for name, kw in calls.items():
        rc, bufs = _eval_raw(k, xd, cd, Cd, kw.get("beta", hc.BETA), kw["flags"], d=kw["d"], dy=kw["dy"],
                             null=kw.get("null", ()), elems=81 * n)
        assert rc != 0 and len(bufs) == 5, name
        for b in bufs.values():
            assert _intact(b, 0), name
    # (the same buffers and claims pass where nothing is wrong: the refusals above are about what they name)
    rc, bufs = _eval_raw(k, xd, cd, Cd, hc.BETA, hc.HD_ALL, d=6, dy=6, elems=81 * n)
    assert rc == 0 and all(_written(b, n) and _intact(b, 81 * n) for b in bufs.values())


# ------------------------------------------------------------------------------------------------------ con_K, cache
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", hc.CONK_SHAPES)
@pytest.mark.parametrize("d", hc.CONK_DS)
def test_con_k_in_4_to_8_dimensions_against_longdouble(dtype, d, n, m):
    x, y = hc.conk_case(n, m, d)
    k = _k(dtype)
    xd, yd = _xd(k, x), _xd(k, y)
    K = k.con_k(xd, yd, hc.UBLK_BETA)
    assert K.shape == (n, m) and K.dtype == k.tdtype
    ref = hc.conk_reference(np.longdouble, xd.double().cpu().numpy(), yd.double().cpu().numpy(), hc.UBLK_BETA)
    err = float(np.abs(K.double().cpu().numpy() - ref).max())  # K <= 1: absolute == relative to max
    print(f"con_k d={d} n={n} m={m} {dtype}: {err:.2e}")
    _note("con_k d = 4 .. 8 (absolute)", dtype, err)
    assert err < hc.CONK_TOL[dtype]


def _build_raw(k, dtype, xd, cd, *, n=None, m=None, d=None, beta=hc.UBLK_BETA, short=0, elems=None):
    """mvf_ublk_build_d into a sentinel-filled buffer of mvf_ublk_bytes(n, m) (of the TRUE shape; `elems` overrides) + a
    guard; the call claims (n, m, d) and ublk_bytes - short.  Returns (rc, buffer, elements of the cache)."""
    tn, tm = xd.shape[0], cd.shape[0]
    item = 4 if dtype == "float32" else 8
    need = k.ublk_bytes(tn, tm)
    live = need // item if elems is None else elems
    buf = _guarded(live, k.tdtype, unit=16 // item)   # (the cache: 16-byte aligned, as include/mvf.h asks at mvf_ublk_pack)
    _settle()
    rc = k.lib.mvf_ublk_build_d(xd.data_ptr(), tn if n is None else n, cd.data_ptr(), tm if m is None else m,
                                xd.shape[1] if d is None else d, float(beta), buf.data_ptr(), need - short, k.cdtype, k._stream())
    _called()
    torch.cuda.synchronize()
    return rc, buf, live


# ------------------------------------------------------------------------------------------------------ calling conventions
CONVENTION_COVERS = {"mvf_eval_d": MODES, "mvf_ublk_build_d": MODES}


def _rows(a, dtype):
    """(n, d) host coordinates as plain rows of the cell dtype, from the scaffold's own allocation (not ``HipKernels.to_xd``)."""
    return _dev(np.ascontiguousarray(a, dtype=np.float64).astype(dtype), None)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,dy", [(4, 1), (5, 3), (8, 8)])
def test_eval_d_calling_conventions(dtype, d, dy, mode):
    """The plain call's bits on a side stream behind poisoned inputs, at displaced pointers (plain rows: one element), and with
    the inputs unchanged."""
    case, k = hc.eval_case(65, 259, d, dy), _k(dtype)

    def call():
        rc, bufs = _eval_raw(k, _rows(case["X"], dtype), _rows(case["ctrl"], dtype), _dev(case["C"]), case["beta"], hc.grid_flags(d, dy))
        assert rc == 0, k.lib.mvf_last_error()
        return [_take(b, b.numel() - GUARD) for _, b in sorted(bufs.items())]

    plain, got = _under(mode, call)
    assert plain and all(_same_bits(a, b) for a, b in zip(plain, got))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [4, 8])
def test_ublk_build_d_calling_conventions(dtype, d, mode):
    case, k = hc.eval_case(65, 259, d, 1), _k(dtype)

    def call():
        rc, buf, live = _build_raw(k, dtype, _rows(case["X"], dtype), _rows(case["ctrl"], dtype))
        assert rc == 0, k.lib.mvf_last_error()
        return _take(buf, live)

    plain, got = _under(mode, call)
    assert _same_bits(plain, got)


def _check_cache(dtype, d, x, y):
    k = _k(dtype)
    xd, yd = _xd(k, x), _xd(k, y)
    n, m = len(x), len(y)
    rc, buf, live = _build_raw(k, dtype, xd, yd)
    n_pad, m_pad = k.wide_pads(n, m)
    assert rc == 0 and live == n_pad * m_pad
    assert _intact(buf, live)  # nothing behind the cache
    U = buf[:live].view(m_pad // 16, n_pad, 16).permute(1, 0, 2).reshape(n_pad, m_pad)
    K = k.con_k(xd, yd, hc.UBLK_BETA)
    torch.cuda.synchronize()
    assert _bits_equal(U[:n, :m].contiguous(), K)
    assert not U[n:].any() and not U[:, m:].any()  # every padded cell row and control-point column, all of n_pad x m_pad
    return K


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", hc.UBLK_SHAPES)
@pytest.mark.parametrize("d", hc.CONK_DS)
def test_ublk_build_d_is_con_k_bit_for_bit_with_zero_padding_and_intact_guard(dtype, d, n, m):
    """n across the 64-cell wave and 256-cell workgroup edges; m across the 16-point block, the 128-point padding and the
    512-point block column (grid.y = 1, 2, 3 with a short last column)."""
    K = _check_cache(dtype, d, *hc.conk_case(n, m, d))
    assert bool((K > 0).any())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", hc.UBLK_FAR_DS)
def test_ublk_build_d_keeps_con_k_bits_where_kernel_values_underflow(dtype, d):
    K = _check_cache(dtype, d, *hc.conk_case(*hc.UBLK_FAR_SHAPE, d, far=hc.UBLK_FAR[dtype]))
    zeros = float((K == 0).double().mean())
    print(f"cache underflow d={d} {dtype}: {zeros:.3f} of the kernel values are 0")
    assert 0.05 <= zeros <= 0.95  # part of them (the CPU module counts the denormals of the exact values)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ublk_build_d_refusals_leave_the_buffer_untouched(dtype):
    """Inputs of 9 columns and a buffer for (n, m) whatever the call claims."""
    n, m = 257, 129
    rng = np.random.default_rng(11)
    k = _k(dtype)
    xd, cd = _dev(rng.uniform(-10, 10, (n, 9)), k.tdtype), _dev(rng.uniform(-10, 10, (m, 9)), k.tdtype)
    calls = {"d = 3": dict(d=3), "d = 9": dict(d=9), "n = 0": dict(d=4, n=0), "m = 0": dict(d=4, m=0),
             "beta < 0": dict(d=4, beta=-hc.UBLK_BETA), "one byte short": dict(d=4, short=1)}
    for name, kw in calls.items():
        rc, buf, _ = _build_raw(k, dtype, xd, cd, **kw)
        assert rc != 0, name
        assert _intact(buf, 0), name
    rc, buf, live = _build_raw(k, dtype, xd, cd, d=4)  # (the same call with nothing wrong passes)
    assert rc == 0 and _written(buf, live) and _intact(buf, live)
