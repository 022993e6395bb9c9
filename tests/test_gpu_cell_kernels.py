"""Kernel-level edge tests of the cell-sized kernels that had none: ``eval_mfma_kernel`` (mvf_eval / mvf_eval_affine),
``integrate_kernel`` (mvf_integrate, the fixed-step RK4), the E-step (mvf_estep_min / mvf_estep_p / mvf_estep), mvf_quadform,
mvf_lincomb3 and mvf_sym_pack / mvf_sym_unpack - each on ``cuda:0`` in both cell dtypes against the plain NumPy restatement
of the same operation (tests/_cpu_kernels.py) on the SAME inputs (the device's own, rounded to the cell dtype where it is
float32), at the tile / wave / workgroup / chunk edges where kernels go wrong.

tests/_cell_cases.py builds the inputs and holds the shape lists and tolerances; tests/test_cell_kernel_refs.py proves without
a GPU that the restatements are accurate to 1e-12, that the compared quantities are well conditioned over ALL queries and
that each targeted off-by-one moves a compared quantity by >= 1000 tolerances.

Tolerances: evaluator and RK4 1e-10 (float64) / 2e-4 (float32) of each quantity's maximum (RK4: of the extent of motion),
torsion 10 x, det J relative to max |J|^3 (_cell_cases.eval_errors says why); E-step sums 1e-12 (derived in _cell_cases), P
1e-12 (float64) / 1 float32 ulp; quadform 1e-11; lincomb3 1 ulp; pack / unpack bit for bit.  Run with ``-s`` to see the
largest deviation of every case family (profiles/cell_kernel_edges.md records them)."""
import numpy as np
import pytest
import torch

import _cell_cases as cc
from _cpu_kernels import CpuKernels
from _kernel_scaffold import (DEV, DTYPES, GUARD, MODES, bits_equal as _bits_equal, called as _called, dev as _dev,
                              deviation_table, guarded as _guarded, intact as _intact, kernel_cache, same_bits as _same_bits,
                              take as _take, under as _under, x4 as _sx4)

pytestmark = pytest.mark.gpu

_k = kernel_cache()
_note, _deviation_table = deviation_table("| case family | dtype | largest deviation |")


def _x4(k, a):
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    return k.to_x4(a) if len(a) else torch.zeros(0, 4, dtype=k.tdtype, device=DEV)


def _host(d):
    return {f: t.cpu().numpy() for f, t in d.items()}


def _eval_setup(dtype, case):
    k = _k(dtype)
    x4, c4 = _x4(k, case["X"]), _x4(k, case["ctrl"])
    Cd = _dev(np.asarray(case["C"], dtype=np.float64).reshape(-1, 3))
    return k, x4, c4, Cd


def _eval_ref(x4, c4, Cd, case, flags=cc.EVAL_ALL):
    """The restatement on the device's inputs (float32 coordinates widened exactly)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        out = CpuKernels().eval(x4.double().cpu(), c4.double().cpu(), case["beta"], Cd.cpu(), flags, affine=case["affine"])
    return {f: o.numpy() for f, o in out.items()}


# ------------------------------------------------------------------------------------------------------ evaluator
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,n,m", cc.EVAL_CASES)
def test_eval_all_outputs_at_tile_wave_workgroup_and_chunk_edges(dtype, family, n, m):
    case = cc.eval_case(n, m, family)
    k, x4, c4, Cd = _eval_setup(dtype, case)
    got_d = k.eval(x4, c4, case["beta"], Cd, cc.EVAL_ALL, affine=case["affine"])
    again = k.eval(x4, c4, case["beta"], Cd, cc.EVAL_ALL, affine=case["affine"])
    assert set(got_d) == set(cc.EVAL_FLAGS)
    for f in cc.EVAL_FLAGS:
        assert got_d[f].shape == cc.EVAL_SHAPES[f](n) and _bits_equal(got_d[f], again[f]), cc.EVAL_NAMES[f]
    errs = cc.eval_errors(_host(got_d), _eval_ref(x4, c4, Cd, case))
    print(f"eval {family} n={n} m={m} {dtype}: " + " ".join(f"{cc.EVAL_NAMES[f]}={e:.2e}" for f, e in errs.items()))
    for f, e in errs.items():
        _note(f"eval {family}: {cc.EVAL_NAMES[f]}", dtype, e)
    for f, e in errs.items():
        assert e <= cc.eval_tol(dtype, f), (cc.EVAL_NAMES[f], e)


@pytest.mark.parametrize("dtype", DTYPES)
def test_eval_without_affine_is_the_identity_affine(dtype):
    case = cc.eval_case(257, 259)
    k, x4, c4, Cd = _eval_setup(dtype, case)
    plain = k.eval(x4, c4, case["beta"], Cd, cc.EVAL_ALL)
    ident = k.eval(x4, c4, case["beta"], Cd, cc.EVAL_ALL, affine=(np.ones(3), 1.0, np.zeros((3, 3)), np.zeros(3)))
    for f in cc.EVAL_FLAGS:
        assert _bits_equal(plain[f], ident[f]), cc.EVAL_NAMES[f]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["positive", "affine"])
@pytest.mark.parametrize("n", [17, 300])
def test_eval_without_control_points(dtype, family, n):
    """m = 0: v = alpha * 0 + A q + b as the epilogue states it, exactly (dyadic inputs: every order of the operations and
    every contraction into fused multiply-adds gives the same, exact, value), J = 0, det = 0."""
    case = cc.eval_case_empty(n, family)
    k, x4, c4, Cd = _eval_setup(dtype, case)
    assert c4.shape == (0, 4) and Cd.shape == (0, 3)
    flags = cc.EVAL_V | cc.EVAL_JAC | cc.EVAL_DIV | cc.EVAL_CURL | cc.EVAL_JDET
    got = _host(k.eval(x4, c4, case["beta"], Cd, flags, affine=case["affine"]))
    assert set(got) == {cc.EVAL_V, cc.EVAL_JAC, cc.EVAL_DIV, cc.EVAL_CURL, cc.EVAL_JDET}
    q = x4.double().cpu().numpy()[:, :3]
    assert np.array_equal(q, case["X"])
    if case["affine"] is None:
        want = np.zeros((n, 3))
    else:
        _, _, A, b = case["affine"]
        want = q @ A.T + b
    np.testing.assert_array_equal(got[cc.EVAL_V], want)
    for f in (cc.EVAL_JAC, cc.EVAL_DIV, cc.EVAL_CURL, cc.EVAL_JDET):
        assert got[f].shape == cc.EVAL_SHAPES[f](n) and not got[f].any(), cc.EVAL_NAMES[f]
    ref = _eval_ref(x4, c4, Cd, case, flags)
    np.testing.assert_array_equal(got[cc.EVAL_V], ref[cc.EVAL_V])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,n,m", [("positive", 257, 259), ("affine", 1000, 513)])
def test_eval_flag_subsets_return_the_bits_of_the_all_flags_call(dtype, family, n, m):
    case = cc.eval_case(n, m, family)
    k, x4, c4, Cd = _eval_setup(dtype, case)
    full = k.eval(x4, c4, case["beta"], Cd, cc.EVAL_ALL, affine=case["affine"])
    product_calls = [cc.EVAL_V, cc.EVAL_JAC | cc.EVAL_JDET, cc.EVAL_V | cc.EVAL_JAC | cc.EVAL_ACC | cc.EVAL_CURV]
    for flags in list(cc.EVAL_FLAGS) + product_calls:
        part = k.eval(x4, c4, case["beta"], Cd, flags, affine=case["affine"])
        assert set(part) == {f for f in cc.EVAL_FLAGS if flags & f}
        for f, t in part.items():
            assert _bits_equal(t, full[f]), (flags, cc.EVAL_NAMES[f])


def _eval_raw(k, x4, c4, Cd, case, flags):
    """mvf_eval_affine through the raw ABI: every requested buffer is followed by a guard, the others are null."""
    n, m = x4.shape[0], c4.shape[0]
    bufs = {}
    for f in cc.EVAL_FLAGS:
        if flags & f:
            bufs[f] = _guarded(int(np.prod(cc.EVAL_SHAPES[f](n))))
    ptr = [bufs[f].data_ptr() if f in bufs else None for f in
           (cc.EVAL_V, cc.EVAL_JAC, cc.EVAL_DIV, cc.EVAL_CURL, cc.EVAL_ACC, cc.EVAL_CURV, cc.EVAL_TORS, cc.EVAL_JDET)]
    from spateo_amd import _lib

    _lib.check(k.lib.mvf_eval_affine(x4.data_ptr(), n, c4.data_ptr(), m, float(case["beta"]), Cd.data_ptr(),
                                     k._affine_buf(case["affine"]), int(flags), *ptr, k.cdtype, k._stream()), "mvf_eval_affine")
    _called()
    torch.cuda.synchronize()
    return bufs


# ------------------------------------------------------------------------------------------------------ calling conventions
CONVENTION_COVERS = {"mvf_eval_affine": MODES, "mvf_eval": MODES, "mvf_integrate": MODES, "mvf_apply": MODES, "mvf_estep_min": MODES,
                     "mvf_estep_p": MODES, "mvf_estep": MODES, "mvf_read_back": MODES}


def _scaffold_inputs(dtype, case):
    """The inputs of a case from the scaffold's own allocations (not ``HipKernels.to_x4``), so that every mode reaches them."""
    return _sx4(case["X"], dtype), _sx4(case["ctrl"], dtype), _dev(np.asarray(case["C"], dtype=np.float64).reshape(-1, 3))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,n,m", [("positive", 257, 259), ("affine", 300, 65)])
def test_eval_calling_conventions(dtype, family, n, m, mode):
    """Every output of mvf_eval_affine: the plain call's bits on a side stream behind poisoned inputs, at displaced pointers
    (coordinates one row, coefficients and outputs one element), and with the inputs unchanged."""
    case = cc.eval_case(n, m, family)
    k = _k(dtype)

    def call():
        bufs = _eval_raw(k, *_scaffold_inputs(dtype, case), case, cc.EVAL_ALL)
        return [_take(b, b.numel() - GUARD) for _, b in sorted(bufs.items())]

    plain, got = _under(mode, call)
    assert len(plain) == len(cc.EVAL_FLAGS) and all(_same_bits(a, b) for a, b in zip(plain, got))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_eval_without_affine_calling_conventions(dtype, mode):
    """mvf_eval, the entry point without the affine epilogue, all outputs."""
    from spateo_amd import _lib

    n, m = 257, 259
    case, k = cc.eval_case(n, m, "positive"), _k(dtype)
    order = (cc.EVAL_V, cc.EVAL_JAC, cc.EVAL_DIV, cc.EVAL_CURL, cc.EVAL_ACC, cc.EVAL_CURV, cc.EVAL_TORS, cc.EVAL_JDET)

    def call():
        x4, c4, Cd = _scaffold_inputs(dtype, case)
        bufs = [_guarded(int(np.prod(cc.EVAL_SHAPES[f](n)))) for f in order]
        _lib.check(k.lib.mvf_eval(x4.data_ptr(), n, c4.data_ptr(), m, float(case["beta"]), Cd.data_ptr(), int(cc.EVAL_ALL),
                                  *[b.data_ptr() for b in bufs], k.cdtype, k._stream()), "mvf_eval")
        _called()
        torch.cuda.synchronize()
        return [_take(b, b.numel() - GUARD) for b in bufs]

    plain, got = _under(mode, call)
    assert all(_same_bits(a, b) for a, b in zip(plain, got))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_and_estep_calling_conventions(dtype, mode):
    """One E-step as a fit chains it, every buffer the scaffold's own: mvf_apply (V, r and sum P r), mvf_estep_min and
    mvf_estep_p with the fill taken on the device, mvf_estep in one call, and the statistics through mvf_read_back - which
    blocks (include/mvf.h): everything in front of it has returned while the inputs were in flight."""
    from spateo_amd import _lib

    n, m = 1000, 259
    case, k = cc.eval_case(n, m, "positive"), _k(dtype)
    rng = np.random.default_rng(7)
    Y, Pw = np.asarray(case["X"]) * 0.01 + rng.standard_normal((n, 3)), rng.uniform(0.0, 1.0, n)
    red = int(k.lib.mvf_reduce_scratch_doubles(n))
    npdt = np.float32 if dtype == "float32" else np.float64

    def call():
        x4, c4, Cd = _scaffold_inputs(dtype, case)
        y4, P = _sx4(Y, dtype), _dev(Pw, k.tdtype)
        V4, r, stats, scratch = _guarded(4 * n, k.tdtype), _guarded(n, k.tdtype), _guarded(1, fill=0.0), _guarded(red)
        _lib.check(k.lib.mvf_apply(x4.data_ptr(), n, c4.data_ptr(), m, float(case["beta"]), Cd.data_ptr(), V4.data_ptr(), y4.data_ptr(),
                                   P.data_ptr(), r.data_ptr(), stats.data_ptr(), scratch.data_ptr(), k.cdtype, k._stream()), "mvf_apply")
        _called()
        mins, P1, st1 = _guarded(4098), _guarded(n, k.tdtype), _guarded(5, fill=0.0)
        _lib.check(k.lib.mvf_estep_min(r.data_ptr(), n, 0.7, mins.data_ptr(), k.cdtype, k._stream()), "mvf_estep_min")
        _called()
        _lib.check(k.lib.mvf_estep_p(r.data_ptr(), n, 0.7, 0.9, 1e-3, 3, 1e-5, 0.75, 0.0, mins.data_ptr(), P1.data_ptr(), st1.data_ptr(),
                                     scratch.data_ptr(), k.cdtype, k._stream()), "mvf_estep_p")
        _called()
        mins2, P2, st2 = _guarded(4098), _guarded(n, k.tdtype), _guarded(5)
        _lib.check(k.lib.mvf_estep(r.data_ptr(), n, 0.7, 0.9, 1e-3, 3, 1e-5, 0.75, mins2.data_ptr(), P2.data_ptr(), st2.data_ptr(),
                                   scratch.data_ptr(), k.cdtype, k._stream()), "mvf_estep")
        _called()
        back = np.full(5, -1.0)
        _lib.check(k.lib.mvf_read_back(back.ctypes.data, st2.data_ptr(), 40, k._stream()), "mvf_read_back")
        _called(synchronising=True)
        torch.cuda.synchronize()
        assert _intact(scratch, red) and _intact(mins, 4098) and _intact(mins2, 4098)
        out = [_take(V4, 4 * n), _take(r, n), _take(stats, 1), mins[:2].cpu().numpy(), _take(P1, n), _take(st1, 5), _take(P2, n),
               _take(st2, 5), back]
        assert out[0].dtype == npdt and _same_bits(out[4], out[6]) and _same_bits(out[5], out[7]) and _same_bits(out[7], back)
        return out

    plain, got = _under(mode, call)
    assert np.isfinite(plain[2]).all() and plain[2][0] > 0 and plain[5][2] > 0
    assert all(_same_bits(a, b) for a, b in zip(plain, got))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("affine", [False, True])
def test_rk4_calling_conventions(dtype, affine, mode):
    from spateo_amd import _lib

    n, m = cc.RK4_SHAPES[0]
    case = cc.rk4_case(n, m, affine)
    k = _k(dtype)

    def call():
        x4, c4, Cd = _scaffold_inputs(dtype, case)
        buf = _guarded(n * cc.RK4_NOUT * 3)
        _lib.check(k.lib.mvf_integrate(x4.data_ptr(), n, c4.data_ptr(), m, float(case["beta"]), Cd.data_ptr(),
                                       k._affine_buf(case["affine"]), float(cc.RK4_DT), int(cc.RK4_SUBSTEPS), int(cc.RK4_NOUT),
                                       buf.data_ptr(), k.cdtype, k._stream()), "mvf_integrate")
        _called()
        torch.cuda.synchronize()
        return _take(buf, n * cc.RK4_NOUT * 3)

    plain, got = _under(mode, call)
    assert _same_bits(plain, got)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [257, 1000])
def test_eval_writes_nothing_behind_its_buffers(dtype, n):
    case = cc.eval_case(n, 259)
    k, x4, c4, Cd = _eval_setup(dtype, case)
    full = k.eval(x4, c4, case["beta"], Cd, cc.EVAL_ALL)
    for flags in (cc.EVAL_ALL, cc.EVAL_V, cc.EVAL_JAC | cc.EVAL_JDET, cc.EVAL_TORS | cc.EVAL_DIV):
        bufs = _eval_raw(k, x4, c4, Cd, case, flags)
        assert set(bufs) == {f for f in cc.EVAL_FLAGS if flags & f}
        for f, b in bufs.items():
            live = b.numel() - GUARD
            assert _intact(b, live), cc.EVAL_NAMES[f]
            assert _bits_equal(b[:live].view(cc.EVAL_SHAPES[f](n)), full[f]), cc.EVAL_NAMES[f]  # (and every element written)


@pytest.mark.parametrize("dtype", DTYPES)
def test_eval_where_every_kernel_value_underflows(dtype):
    """Queries ~1000 units away: beta d^2 ~ 4000, every kernel value is exactly 0 in float32 and in float64.  V, J, div, curl
    and det are exactly 0, curvature and torsion are NumPy's 0 / 0, and the near queries of the same launch keep their bits."""
    case = cc.eval_case(300, 259)
    rng = np.random.default_rng(5)
    far = np.array([1000.0, -900.0, 1100.0]) * rng.choice([-1.0, 1.0], (45, 3)) + rng.uniform(-30, 30, (45, 3))
    both = dict(case, X=np.concatenate([case["X"], far]))
    k, x4, c4, Cd = _eval_setup(dtype, both)
    got = k.eval(x4, c4, case["beta"], Cd, cc.EVAL_ALL)
    near = k.eval(x4[:300].contiguous(), c4, case["beta"], Cd, cc.EVAL_ALL)
    ref = _eval_ref(x4, c4, Cd, both)
    for f in cc.EVAL_FLAGS:
        g = got[f]
        g_far, g_near = (g[:, :, 300:], g[:, :, :300]) if f == cc.EVAL_JAC else (g[300:], g[:300])
        r_far = ref[f][:, :, 300:] if f == cc.EVAL_JAC else ref[f][300:]
        assert _bits_equal(g_near, near[f]), cc.EVAL_NAMES[f]
        if f in (cc.EVAL_CURV, cc.EVAL_TORS, cc.EVAL_ACC):
            np.testing.assert_array_equal(np.isnan(g_far.cpu().numpy()), np.isnan(r_far))
            if f != cc.EVAL_ACC:
                assert np.isnan(r_far).all()
        if f not in (cc.EVAL_CURV, cc.EVAL_TORS):
            assert not g_far.cpu().numpy().any() and not r_far.any(), cc.EVAL_NAMES[f]


# ------------------------------------------------------------------------------------------------------ RK4
_RK4_REF = {}


def _rk4_ref(n, m, affine, dt, substeps, n_out):
    """CpuKernels.integrate on the case's inputs (on the float32 grid: the same for both cell dtypes)."""
    key = (n, m, affine, dt, substeps, n_out)
    if key not in _RK4_REF:
        case = cc.rk4_case(n, m, affine)
        k = CpuKernels()
        _RK4_REF[key] = k.integrate(k.to_x4(case["X"]), k.to_x4(case["ctrl"]), case["beta"], torch.from_numpy(case["C"]), dt,
                                    substeps, n_out, affine=case["affine"]).numpy()
    return _RK4_REF[key]


def _rk4_run(dtype, n, m, affine, dt, substeps, n_out):
    """mvf_integrate through the raw ABI into a guarded buffer, twice: returns the trajectories (host)."""
    from spateo_amd import _lib

    case = cc.rk4_case(n, m, affine)
    k = _k(dtype)
    x4, c4, Cd = _x4(k, case["X"]), _x4(k, case["ctrl"]), _dev(case["C"])
    assert np.array_equal(x4.double().cpu().numpy()[:, :3], case["X"])  # the float32 grid: no rounding on the way in
    outs = []
    for _ in range(2):
        buf = _guarded(n * n_out * 3)
        _lib.check(k.lib.mvf_integrate(x4.data_ptr(), n, c4.data_ptr(), m, float(case["beta"]), Cd.data_ptr(),
                                       k._affine_buf(case["affine"]), float(dt), int(substeps), int(n_out), buf.data_ptr(),
                                       k.cdtype, k._stream()), "mvf_integrate")
        torch.cuda.synchronize()
        assert _intact(buf, n * n_out * 3)
        outs.append(buf[: n * n_out * 3].view(n, n_out, 3))
    assert _bits_equal(outs[0], outs[1])  # deterministic
    via_wrapper = k.integrate(x4, c4, case["beta"], Cd, dt, substeps, n_out, affine=case["affine"])
    assert _bits_equal(via_wrapper, outs[0])
    return outs[0].cpu().numpy(), case


def _rk4_check(dtype, family, n, m, affine=False, dt=cc.RK4_DT, substeps=cc.RK4_SUBSTEPS, n_out=cc.RK4_NOUT):
    got, case = _rk4_run(dtype, n, m, affine, dt, substeps, n_out)
    ref = _rk4_ref(n, m, affine, dt, substeps, n_out)
    np.testing.assert_array_equal(got[:, 0], case["X"])
    ext = cc.extent(ref)
    err = float(np.abs(got - ref).max() / ext)
    print(f"rk4 {family} n={n} m={m} chunks={cc.rk4_chunks(m, dtype)} substeps={substeps} n_out={n_out} dt={dt} {dtype}: "
          f"extent {ext:.3g} err {err:.2e}")
    _note(f"rk4 {family}", dtype, err)
    assert err <= cc.TOL[dtype], err


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", cc.RK4_SHAPES)
def test_rk4_across_the_staging_cap_and_workgroup_edges(dtype, n, m):
    """m = cap - 1, cap, cap + 1 for both dtypes' caps (2304 / 3072), up to three chunks; n = 1, 255, 257, 600: one lane, a
    workgroup with one dead lane, a second workgroup with one live lane, three workgroups with 168 dead lanes in the barriers."""
    chunks = cc.rk4_chunks(m, dtype)
    _rk4_check(dtype, "one chunk" if chunks == 1 else "chunked", n, m)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("substeps,n_out", cc.RK4_STEPPING)
def test_rk4_substeps_and_output_counts(dtype, substeps, n_out):
    n, m = cc.RK4_AFFINE_SHAPE
    if n_out == 1:  # the start points and nothing else (the guard behind them is checked in _rk4_run)
        got, case = _rk4_run(dtype, n, m, False, cc.RK4_DT, substeps, 1)
        np.testing.assert_array_equal(got[:, 0], case["X"])
        return
    _rk4_check(dtype, "stepping", n, m, substeps=substeps, n_out=n_out)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rk4_with_the_affine_part(dtype):
    _rk4_check(dtype, "affine", *cc.RK4_AFFINE_SHAPE, affine=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rk4_backwards(dtype):
    _rk4_check(dtype, "negative dt", *cc.RK4_AFFINE_SHAPE, dt=-cc.RK4_DT)


# ------------------------------------------------------------------------------------------------------ E-step
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,kind,dy,gamma", cc.ESTEP_CASES)
def test_estep_sizes_dimensions_and_underflow_families(dtype, n, kind, dy, gamma):
    s2, a, minP = cc.ESTEP_SIGMA2, cc.ESTEP_A, cc.ESTEP_MINP
    r = cc.estep_residuals(n, kind, dtype)
    ref = cc.estep_reference(r, s2, gamma, a, dy, minP, dtype)
    theta, dist = cc.pick_theta(ref["stored"])
    assert dist >= 1e-6 and np.abs(ref["pf"] - theta).min() >= 1e-6  # the count above theta is determined
    k = _k(dtype)
    rd = _dev(r, k.tdtype)
    assert np.array_equal(rd.double().cpu().numpy(), r)
    f64 = torch.float64
    mins = k.estep_min(rd, s2).clone()
    mh = mins.cpu().numpy()
    # phases apart: statistics ADDED to what the buffer holds
    P0, st0 = torch.full((n,), -1.0, dtype=k.tdtype, device=DEV), torch.zeros(5, dtype=f64, device=DEV)
    k.estep_p(rd, s2, gamma, a, dy, minP, theta, mins, P0, st0)
    prefill = torch.tensor([3.0, 0.5, 1e3, 7.0, 11.0], dtype=f64, device=DEV)
    P1, st1 = torch.full((n,), -1.0, dtype=k.tdtype, device=DEV), prefill.clone()
    k.estep_p(rd, s2, gamma, a, dy, minP, theta, mins, P1, st1)
    assert torch.equal(P1, P0) and torch.equal(st1, prefill + st0)
    # the host's fill is the device's
    P2, st2 = torch.full((n,), -1.0, dtype=k.tdtype, device=DEV), torch.zeros(5, dtype=f64, device=DEV)
    k.estep_p(rd, s2, gamma, a, dy, minP, theta, float(mh[0]) if np.isfinite(mh[0]) else 0.0, P2, st2)
    assert torch.equal(P2, P0) and torch.equal(st2, st0)
    # one call: statistics OVERWRITTEN, the bits of estep_min followed by estep_p on zeroed statistics
    P3, st3 = torch.full((n,), -1.0, dtype=k.tdtype, device=DEV), prefill.clone()
    k._mins[:2] = -5.0
    k.estep(rd, s2, gamma, a, dy, minP, theta, P3, st3)
    assert torch.equal(P3, P0) and torch.equal(st3, st0) and torch.equal(k._mins[:2], mins)
    # against the restatement
    assert mh[1] == ref["mins"][1] == ref["nzero"]
    if np.isfinite(ref["mins"][0]):
        np.testing.assert_allclose(mh[0], ref["mins"][0], rtol=1e-12)
    else:
        assert mh[0] == np.inf
    P = P0.cpu().numpy()
    if dtype == "float64":
        np.testing.assert_allclose(P, ref["pf"], rtol=1e-12, atol=0)
        prel = float((np.abs(P - ref["pf"]) / ref["pf"]).max())
    else:
        want = ref["pf"].astype(np.float32)
        ulps = np.abs(P.astype(np.float64) - want.astype(np.float64)) / np.spacing(want).astype(np.float64)
        assert ulps.max() <= 1.0
        prel = float(ulps.max())
    s = st0.cpu().numpy()
    serr = max(abs(s[i] - ref["sums"][i]) / ref["sums"][i] if ref["sums"][i] else abs(s[i]) for i in range(3))
    print(f"estep n={n} {kind} dy={dy} gamma={gamma} {dtype}: sums {serr:.2e}  P {prel:.2e} ({'rel' if dtype == 'float64' else 'ulp'})")
    _note("estep sums (rel)", dtype, serr)
    _note("estep P (float64: rel, float32: ulp)", dtype, prel)
    np.testing.assert_allclose(s[:3], ref["sums"], rtol=cc.ESTEP_SUM_RTOL, atol=0)
    assert s[3] == float((ref["stored"] > theta).sum()) and s[4] == ref["nzero"]
    if kind == "all":
        assert mh[0] == np.inf and mh[1] == n and s[4] == n and s[3] == 0 and bool((P0 == torch.tensor(minP, dtype=k.tdtype)).all())
    if kind == "one":  # every filled cell holds the one live cell's t1
        assert mh[1] == n - 1 and len(np.unique(np.delete(P, n // 2))) == 1 and P[0] > minP
    if kind == "none":
        assert mh[1] == 0 and s[4] == 0


# ------------------------------------------------------------------------------------------------------ small kernels
@pytest.mark.parametrize("m,nrhs", cc.QUADFORM_SHAPES)
def test_quadform_shapes(m, nrhs):
    K, C = cc.quadform_case(m, nrhs)
    k = _k("float64")
    out = _guarded(1)
    k.quadform(_dev(K), _dev(C), out)
    ref = cc.quadform_reference(K, C)
    got = float(out[0])
    err = abs(got - ref) / ref
    print(f"quadform m={m} nrhs={nrhs}: {err:.2e}")
    _note("quadform", "float64", err)
    assert _intact(out, 1)
    np.testing.assert_allclose(got, ref, rtol=1e-11)


@pytest.mark.parametrize("n", cc.LINCOMB_NS)
def test_lincomb3_lengths_absent_terms_and_aliasing(n):
    (a, A), (b, B), (c, C) = cc.lincomb3_case(n)
    k = _k("float64")
    worst = 0.0
    for kw in ({}, {"b": b, "B": B}, {"c": c, "C": C}, {"b": b, "B": B, "c": c, "C": C}):
        ref = cc.lincomb3_reference(a, A, **kw)
        for alias in [None, "A"] + [key for key in kw if key in "BC"]:
            dev = {"A": _dev(A)}
            dev.update({key: _dev(v) for key, v in kw.items() if key in "BC"})
            if alias is None:
                buf = _guarded(n)
                out = buf[:n]
            else:
                buf, out = None, dev[alias]
            k.lincomb3(out, a, dev["A"], kw.get("b", 0.0), dev.get("B"), kw.get("c", 0.0), dev.get("C"))
            got = out.cpu().numpy()
            ulps = np.abs(got - ref) / np.spacing(ref)
            worst = max(worst, float(ulps.max()))
            assert ulps.max() <= 1.0, (sorted(kw), alias)
            if buf is not None:
                assert _intact(buf, n)
            for key, t in dev.items():  # inputs that are not the output are untouched
                if key != alias:
                    assert np.array_equal(t.cpu().numpy(), {"A": A, "B": B, "C": C}[key])
    print(f"lincomb3 n={n}: {worst:.2f} ulp")
    _note("lincomb3 (ulp)", "float64", worst)


@pytest.mark.parametrize("m", cc.SYM_MS)
def test_sym_pack_and_unpack_bit_for_bit(m):
    G = cc.sym_case(m)
    k = _k("float64")
    nt = m * (m + 1) // 2
    tri = _guarded(nt)
    k.sym_pack(_dev(G), tri[:nt])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tri[:nt].cpu().numpy(), G[np.triu_indices(m)])
    assert _intact(tri, nt)
    full = _guarded(m * m)
    k.sym_unpack(tri[:nt], full[: m * m].view(m, m))
    torch.cuda.synchronize()
    F = full[: m * m].view(m, m).cpu().numpy()
    np.testing.assert_array_equal(F, cc.sym_completion(G[np.triu_indices(m)], m))
    assert _intact(full, m * m) and _intact(tri, nt)
    np.testing.assert_array_equal(tri[:nt].cpu().numpy(), G[np.triu_indices(m)])  # unpack leaves the packed values alone
