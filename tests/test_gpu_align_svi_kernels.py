"""Kernel-level tests of what the SVI mode adds to ``csrc/mvf_align.hip`` - ``mvf_align_gather``, ``mvf_align_alpha_svi``,
``mvf_align_transform_svi`` - through the raw C ABI on ``cuda:0``.  tests/_align_svi_case.py holds the NumPy references.

* gather: batches of 1, 63, 64, 65 and 1000 rows out of NB = bs (the whole slice, permuted) and NB = 3 bs + 7, start offsets
  0, in the middle and such that the batch wraps past the end of the permutation; rows of 16, 48 and 2000 features, 1 and 4
  layers, both cell dtypes.  Every output equals NumPy indexing bit for bit, the guard words behind every output stay
  intact, two calls give the same bits, ``bs = 0`` touches nothing.
* alpha: n = 1, 255, 256, 257, 70 001; ``step = 1`` gives ``mvf_align_alpha``'s bits whatever ``alpha`` held; ``step = 0.37`` is
  within 1e-12 (relative) of the blend formed with ``scipy.special.psi``.
* transform: the same n; the float64 ``PXB_term`` bit for bit against the operation order ``include/mvf.h`` states, in place,
  the cell-dtype stores equal to NumPy's rounding; ``step = 1`` on a zero ``PXB_term`` and ``step < 1`` on a running one."""
import ctypes

import numpy as np
import pytest
import torch

import _align_svi_case as sc
from _align_kernel_scaffold import kernels as _k
from _kernel_scaffold import (DEV, DTYPES, MODES, called as _called, dev as _dev, guarded as _guarded, intact as _intact,
                              same_bits as _same_bits, take as _take, under as _under)

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 70001]


# ---- gather ----------------------------------------------------------------------------------------------------------
_SLICES = {}


def _slice(nb, lds, dtype):
    """A B slice of nb cells on the device (built once per shape): xb4, coordsB, and per layer Yp (nb x ld) and b."""
    key = (nb, lds, dtype)
    if key not in _SLICES:
        _SLICES.clear()   # one slice at a time on the device: the 2000-feature ones are tens of MB
        tdt = torch.float32 if dtype == "float32" else torch.float64
        g = torch.Generator(device="cpu").manual_seed(nb + 7 * len(lds))
        xb4 = torch.randn(nb, 4, generator=g, dtype=torch.float64).to(tdt).to(DEV)
        B = torch.randn(nb, 3, generator=g, dtype=torch.float64).to(DEV)
        Yp = [torch.randn(nb, ld, generator=g, dtype=torch.float32).to(tdt).to(DEV) for ld in lds]
        b = [torch.randn(nb, generator=g, dtype=torch.float64).to(DEV) for _ in lds]
        perm = torch.from_numpy(np.random.default_rng(nb).permutation(nb).astype(np.int32)).to(DEV)
        _SLICES[key] = (xb4, B, Yp, b, perm)
    return _SLICES[key]


def _gather(lib, k, perm, nb, start, bs, xb4, B, Yp, b, lds, outs):
    from spateo_amd._kernels import layer_array

    arr = layer_array([(None, y, None, c, ld, 0, 0, 0.0) for y, c, ld in zip(Yp, b, lds)])   # (Yp, b, ld are what it reads)
    vp = ctypes.c_void_p * max(len(lds), 1)
    return lib.mvf_align_gather(perm.data_ptr(), nb, start, bs, xb4.data_ptr(), outs["xb4"].data_ptr(), B.data_ptr(),
                                outs["B"].data_ptr(), arr, len(lds), vp(*[o.data_ptr() for o in outs["Yp"]]),
                                vp(*[o.data_ptr() for o in outs["b"]]), k.cdtype, k._stream())


GATHER_CASES = [(bs, lds) for bs in (1, 63, 64, 65, 1000) for lds in ((16,), (48,), (16, 48, 16, 48))] + \
               [(1, (2000,)), (65, (2000,)), (1000, (2000, 16, 48, 16))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs, lds", GATHER_CASES)
def test_gather(bs, lds, dtype):
    k, lib = _k(dtype), _k(dtype).lib
    tdt = torch.float32 if dtype == "float32" else torch.float64
    for nb in (bs, 3 * bs + 7):
        xb4, B, Yp, b, perm = _slice(nb, lds, dtype)
        hp = perm.cpu().numpy().astype(np.int64)
        host = dict(xb4=xb4.cpu().numpy(), B=B.cpu().numpy(), Yp=[y.cpu().numpy() for y in Yp], b=[c.cpu().numpy() for c in b])
        for start in sorted({0, nb // 2, nb - 1, (nb - bs // 2) % nb, (-5 * bs) % nb}):
            idx = hp[(start + np.arange(bs)) % nb]
            runs = []
            for rep in range(2):
                outs = dict(xb4=_guarded(4 * bs, tdt), B=_guarded(3 * bs), Yp=[_guarded(bs * ld, tdt) for ld in lds],
                            b=[_guarded(bs) for _ in lds])
                rc = _gather(lib, k, perm, nb, start, bs, xb4, B, Yp, b, lds, outs)
                assert rc == 0, lib.mvf_last_error()
                torch.cuda.synchronize()
                assert _intact(outs["xb4"], 4 * bs) and _intact(outs["B"], 3 * bs)
                assert all(_intact(o, bs * ld) for o, ld in zip(outs["Yp"], lds)) and all(_intact(o, bs) for o in outs["b"])
                runs.append(dict(xb4=outs["xb4"][: 4 * bs].cpu().numpy().reshape(bs, 4), B=outs["B"][: 3 * bs].cpu().numpy().reshape(bs, 3),
                                 Yp=[o[: bs * ld].cpu().numpy().reshape(bs, ld) for o, ld in zip(outs["Yp"], lds)],
                                 b=[o[:bs].cpu().numpy() for o in outs["b"]]))
            got = runs[0]
            assert _same_bits(got["xb4"], host["xb4"][idx]) and _same_bits(got["B"], host["B"][idx]), (nb, start)
            for l in range(len(lds)):
                assert _same_bits(got["Yp"][l], host["Yp"][l][idx]) and _same_bits(got["b"][l], host["b"][l][idx]), (nb, start, l)
                assert _same_bits(got["Yp"][l], runs[1]["Yp"][l]) and _same_bits(got["b"][l], runs[1]["b"][l])
            assert _same_bits(got["xb4"], runs[1]["xb4"]) and _same_bits(got["B"], runs[1]["B"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_through_the_binding_and_empty_batch(dtype):
    """HipKernels.align_gather (what the loop calls) on layers as assign_prepare returns them; bs = 0 is a no-op."""
    from spateo_amd._kernels import Layer

    k, lib = _k(dtype), _k(dtype).lib
    rng = np.random.default_rng(3)
    nb, bs = 457, 150
    XB = rng.standard_normal((nb, 3))
    layers = []
    for g, metric in ((40, 2), (24, 4)):
        Yp, b, ld = k.assign_prepare(rng.random((nb, g)) + 0.1, metric, 1)
        layers.append((None, Yp, None, b, ld, metric, 0, 0.1))   # plain 8-sequences: the binding takes them
    xb4, B = k.to_x4(XB), k.h2d_padded(XB, 3, torch.float64)
    perm = rng.permutation(nb).astype(np.int32)
    outs = (k.empty(bs, 4), k.empty(bs, 3, dtype=torch.float64), [k.empty(bs, Layer(*L).ld) for L in layers],
            [k.empty(bs, dtype=torch.float64) for L in layers])
    for it in (0, 3, 4):
        k.align_gather(_dev(perm, None), (-it * bs) % nb, bs, xb4, B, layers, *outs)
        idx = torch.from_numpy(sc.schedule(perm, bs, it).astype(np.int64)).to(DEV)
        assert torch.equal(outs[0], xb4[idx]) and torch.equal(outs[1], B[idx])
        for l, L in enumerate(layers):
            assert torch.equal(outs[2][l], Layer(*L).Yp[idx]) and torch.equal(outs[3][l], Layer(*L).b[idx])
    with pytest.raises(ValueError):
        k.align_gather(_dev(perm.astype(np.int64), None), 0, bs, xb4, B, layers, *outs)
    # bs == 0: nothing is launched, whatever the pointers
    assert lib.mvf_align_gather(None, nb, 0, 0, None, None, None, None, None, 0, None, None, k.cdtype, None) == 0
    p = xb4.data_ptr()
    vp = (ctypes.c_void_p * 1)(p)
    assert lib.mvf_align_gather(p, nb, nb, 5, p, p, p, p, None, 0, vp, vp, k.cdtype, None) != 0 and b"start" in lib.mvf_last_error()
    assert lib.mvf_align_gather(p, nb, 0, nb + 1, p, p, p, p, None, 0, vp, vp, k.cdtype, None) != 0
    assert lib.mvf_align_gather(p, nb, 0, 5, p, p, p, p, None, 5, vp, vp, k.cdtype, None) != 0 and b"layers" in lib.mvf_last_error()
    assert lib.mvf_align_gather(p, 1 << 31, 0, 5, p, p, p, p, None, 0, vp, vp, k.cdtype, None) != 0


# ---- alpha -----------------------------------------------------------------------------------------------------------
def _alpha_inputs(n):
    rng = np.random.default_rng(n)
    Ks = rng.uniform(0.0, 2.0, n) * (rng.random(n) < 0.9)
    return dict(kappa=rng.uniform(0.5, 1.5, n), Ks=Ks, sd=rng.uniform(0.0, 0.1, n), old=rng.uniform(0.0, 1.2, n),
                Sp_spatial=0.8 * float(Ks.sum()), sigma2=0.3)


@pytest.mark.parametrize("n", SIZES)
def test_alpha_svi(n):
    k, lib = _k("float64"), _k("float64").lib
    inp = _alpha_inputs(n)
    d = {q: _dev(inp[q]) for q in ("kappa", "Ks", "sd")}
    head = (d["kappa"].data_ptr(), d["Ks"].data_ptr(), d["sd"].data_ptr(), n, inp["Sp_spatial"], inp["sigma2"])
    # step == 1: mvf_align_alpha's bits, whatever alpha held (here: the sentinel)
    al0, mm0, al1, mm1 = _guarded(n), _guarded(n), _guarded(n), _guarded(n)
    assert lib.mvf_align_alpha(*head, al0.data_ptr(), mm0.data_ptr(), k._stream()) == 0, lib.mvf_last_error()
    assert lib.mvf_align_alpha_svi(*head, 1.0, al1.data_ptr(), mm1.data_ptr(), k._stream()) == 0, lib.mvf_last_error()
    torch.cuda.synchronize()
    assert _intact(al1, n) and _intact(mm1, n)
    assert _same_bits(al0[:n].cpu().numpy(), al1[:n].cpu().numpy()) and _same_bits(mm0[:n].cpu().numpy(), mm1[:n].cpu().numpy())
    # step < 1: the blend with the old alpha, in place, against scipy.special.psi
    step = 0.37
    runs = []
    for rep in range(2):
        al, mm = _guarded(n), _guarded(n)
        al[:n] = _dev(inp["old"])
        assert lib.mvf_align_alpha_svi(*head, step, al.data_ptr(), mm.data_ptr(), k._stream()) == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        assert _intact(al, n) and _intact(mm, n)
        runs.append((al[:n].cpu().numpy(), mm[:n].cpu().numpy()))
    assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1])
    ra, rm = sc.alpha_svi_reference(inp["kappa"], inp["Ks"], inp["sd"], inp["Sp_spatial"], inp["sigma2"], step, inp["old"])
    worst = max(float((np.abs(runs[0][0] - ra) / np.abs(ra)).max()), float((np.abs(runs[0][1] - rm) / np.abs(rm)).max()))
    print(f"  n = {n}: alpha / model_mul at step {step}: largest relative deviation from scipy.special.psi {worst:.2e}")
    assert worst <= 1e-12


# ---- transform -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_transform_svi(n, dtype):
    k, lib = _k(dtype), _k(dtype).lib
    tdt, npdt = (torch.float32, np.float32) if dtype == "float32" else (torch.float64, np.float64)
    rng = np.random.default_rng(n + 1)
    RnA = rng.standard_normal((n, 3)) + 3.0
    K = rng.uniform(0.1, 1.5, n) * (rng.random(n) < 0.8)          # cells without a partner in this batch
    PXB = K[:, None] * (RnA + 0.05 * rng.standard_normal((n, 3)))
    running = 0.1 * rng.standard_normal((n, 3))
    d = {"RnA": _dev(RnA), "K": _dev(K), "PXB": _dev(PXB)}
    for origin in (None, np.array([0.5, -0.25, 3.0])):
        org = None if origin is None else (ctypes.c_double * 3)(*origin)
        o = np.zeros(3) if origin is None else origin
        for step, start in ((1.0, np.zeros((n, 3))), (10.0 / 13.0, np.zeros((n, 3))), (0.37, running)):
            runs = []
            for rep in range(2):
                term, Y4, Pw = _guarded(3 * n), _guarded(4 * n, tdt), _guarded(n, tdt)
                term[: 3 * n] = _dev(start.reshape(-1))
                rc = lib.mvf_align_transform_svi(d["RnA"].data_ptr(), d["PXB"].data_ptr(), d["K"].data_ptr(), n, org, step,
                                                 term.data_ptr(), Y4.data_ptr(), Pw.data_ptr(), k.cdtype, k._stream())
                assert rc == 0, lib.mvf_last_error()
                torch.cuda.synchronize()
                assert _intact(term, 3 * n) and _intact(Y4, 4 * n) and _intact(Pw, n)
                runs.append((term[: 3 * n].cpu().numpy().reshape(n, 3), Y4[: 4 * n].cpu().numpy().reshape(n, 4), Pw[:n].cpu().numpy()))
            ref = sc.transform_svi_reference(RnA, PXB, K, o, step, start, npdt)
            for got, again, want in zip(runs[0], runs[1], ref):
                assert _same_bits(got, np.ascontiguousarray(want)) and _same_bits(got, again), (step, origin)
            if step < 1.0 and start is running:                   # rows without a partner keep the earlier batches' share
                assert np.array_equal(runs[0][0][K == 0], ((1.0 - step) * running)[K == 0] + 0.0)


CONVENTION_COVERS = {"mvf_align_gather": MODES, "mvf_align_alpha_svi": MODES, "mvf_align_transform_svi": MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_calling_conventions(dtype, mode):
    """A batch of 65 of 202 cells that wraps around the end, two layers: the plain call's bits on a side stream behind poisoned
    inputs, at displaced pointers (the rows of xb4 and of the layers 16 bytes, as the entry point asks; coordsB, b and the
    permutation one element), and with the inputs unchanged."""
    k, lib = _k(dtype), _k(dtype).lib
    tdt, npdt, item = (torch.float32, np.float32, 4) if dtype == "float32" else (torch.float64, np.float64, 8)
    nb, bs, lds, start = 202, 65, (16, 48), 170
    rng = np.random.default_rng(202)
    host = dict(xb4=rng.standard_normal((nb, 4)).astype(npdt), B=rng.standard_normal((nb, 3)),
                Yp=[rng.standard_normal((nb, ld)).astype(npdt) for ld in lds], b=[rng.standard_normal(nb) for _ in lds],
                perm=rng.permutation(nb).astype(np.int32))

    def call():
        xb4, B, perm = _dev(host["xb4"], None, unit=16 // item), _dev(host["B"]), _dev(host["perm"], None)
        Yp, b = [_dev(y, None, unit=16 // item) for y in host["Yp"]], [_dev(c) for c in host["b"]]
        outs = dict(xb4=_guarded(4 * bs, tdt, unit=16 // item), B=_guarded(3 * bs), Yp=[_guarded(bs * ld, tdt, unit=16 // item) for ld in lds],
                    b=[_guarded(bs) for _ in lds])
        rc = _gather(lib, k, perm, nb, start, bs, xb4, B, Yp, b, lds, outs)
        _called()
        assert rc == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        return [_take(outs["xb4"], 4 * bs), _take(outs["B"], 3 * bs)] + [_take(o, bs * ld) for o, ld in zip(outs["Yp"], lds)] + \
               [_take(o, bs) for o in outs["b"]]

    plain, got = _under(mode, call)
    idx = host["perm"].astype(np.int64)[(start + np.arange(bs)) % nb]
    assert _same_bits(plain[0].reshape(bs, 4), host["xb4"][idx]) and _same_bits(plain[3].reshape(bs, 48), host["Yp"][1][idx])
    assert all(_same_bits(a, b) for a, b in zip(plain, got))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_alpha_and_transform_svi_calling_conventions(dtype, mode):
    """mvf_align_alpha_svi and mvf_align_transform_svi at a step below 1 on running values of 257 cells; ``alpha`` and the
    running term are read and overwritten (not ``const`` in include/mvf.h): they are left out of the input check."""
    k, lib = _k(dtype), _k(dtype).lib
    tdt = torch.float32 if dtype == "float32" else torch.float64
    n = 257
    inp = _alpha_inputs(n)
    rng = np.random.default_rng(n + 1)
    RnA = rng.standard_normal((n, 3)) + 3.0
    K = rng.uniform(0.1, 1.5, n) * (rng.random(n) < 0.8)
    PXB, running = K[:, None] * (RnA + 0.05 * rng.standard_normal((n, 3))), 0.1 * rng.standard_normal((n, 3))
    org = (ctypes.c_double * 3)(0.5, -0.25, 3.0)

    def call():
        d = {q: _dev(inp[q]) for q in ("kappa", "Ks", "sd")}
        al, mm = _guarded(n), _guarded(n)
        al[:n] = _dev(inp["old"])
        rc = lib.mvf_align_alpha_svi(d["kappa"].data_ptr(), d["Ks"].data_ptr(), d["sd"].data_ptr(), n, inp["Sp_spatial"], inp["sigma2"],
                                     0.37, al.data_ptr(), mm.data_ptr(), k._stream())
        _called()
        assert rc == 0, lib.mvf_last_error()
        t = {"RnA": _dev(RnA), "K": _dev(K), "PXB": _dev(PXB)}
        term, Y4, Pw = _guarded(3 * n), _guarded(4 * n, tdt), _guarded(n, tdt)
        term[: 3 * n] = _dev(running.reshape(-1))
        rc = lib.mvf_align_transform_svi(t["RnA"].data_ptr(), t["PXB"].data_ptr(), t["K"].data_ptr(), n, org, 0.37, term.data_ptr(),
                                         Y4.data_ptr(), Pw.data_ptr(), k.cdtype, k._stream())
        _called()
        assert rc == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        return [_take(al, n), _take(mm, n), _take(term, 3 * n), _take(Y4, 4 * n), _take(Pw, n)]

    plain, got = _under(mode, call)
    assert all(_same_bits(a, b) for a, b in zip(plain, got))


def test_empty_and_refusals():
    lib = _k("float64").lib
    p = torch.zeros(64, dtype=torch.float64, device=DEV).data_ptr()
    assert lib.mvf_align_alpha_svi(None, None, None, 0, 0.0, 1.0, 0.5, None, None, None) == 0
    assert lib.mvf_align_transform_svi(None, None, None, 0, None, 0.5, None, None, None, 1, None) == 0
    assert lib.mvf_align_alpha_svi(p, p, p, 5, 1.0, 1.0, 0.0, p, p, None) != 0 and b"step" in lib.mvf_last_error()
    assert lib.mvf_align_alpha_svi(p, p, p, 5, 1.0, 1.0, 1.5, p, p, None) != 0
    assert lib.mvf_align_transform_svi(p, p, p, 5, None, 0.0, p, p, p, 1, None) != 0 and b"step" in lib.mvf_last_error()
    assert lib.mvf_align_transform_svi(p, p, p, 5, None, 0.5, None, p, p, 1, None) != 0 and b"null pointer" in lib.mvf_last_error()
    assert lib.mvf_align_transform_svi(p, p, p, 5, None, 0.5, p, p, p, 7, None) != 0 and b"bad dtype" in lib.mvf_last_error()
