"""Kernel-level edge tests of the alignment loop's glue (``csrc/mvf_align.hip``) through the raw C ABI - ``mvf_align_alpha``,
``mvf_align_moments``, ``mvf_align_transform`` - on ``cuda:0`` in both cell dtypes, at n = 1, the wave and workgroup edges
(63 / 64 / 65, 255 / 256 / 257), one reduction block +- 1 (1023 / 1024 / 1025 cells) and 70 001 cells (several partial blocks
and a tail).  tests/_align_loop_case.py holds the NumPy references.

Every call has guard words behind every output and behind the workspace, runs on a workspace filled with NaN bit patterns,
and is made twice (same bits).  Bounds, none fitted to what the device returned:

* moments: 1e-12 of sum |terms| against the same sums in ``math.fsum``, the second-order sums on rows centred by the means
  the device formed (read back), the means themselves against the fsum'd sums; for denormal weights an absolute slack of
  n denormal spacings (each product of a denormal weight is rounded to the denormal grid);
* transform: the float64 outputs bit for bit against the NumPy evaluation in the operation order the kernel's header
  states, the cell-dtype stores equal to NumPy's rounding of the float64 value;
* alpha / model_mul: 1e-12 relative against ``scipy.special.psi``.

Run with ``-s`` for the largest deviation of every family."""
import numpy as np
import pytest
import torch

import _align_loop_case as lc
from _align_kernel_scaffold import kernels as _k
from _kernel_scaffold import (DEV, DTYPES, GUARD, MODES, SENTINEL, called as _called, dev as _dev, deviation_table,
                              guarded as _guarded, intact as _intact, same_bits as _same_bits, take as _take, under as _under,
                              x4 as _sx4)

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 70001]
VARIANTS = ["zero_K", "one_K", "denormal_K", "kappa_small", "kappa_large", "zero_Ks", "offset", "reflection"]
_note, _deviation_table = deviation_table("| family | dtype | largest deviation / bound |")


def make_inputs(n, variant, seed=0):
    """One A slice of n cells and a B slice of max(1, 3 n // 4) cells; every array float64 on the host."""
    rng = np.random.default_rng(1000 * seed + n)
    nb = max(1, (3 * n) // 4)
    off = 1e4 if variant == "offset" else 0.0
    A, B = rng.standard_normal((n, 3)) + off, rng.standard_normal((nb, 3)) + off
    V = 0.1 * rng.standard_normal((n, 3))
    K = rng.uniform(0.1, 1.5, n) * (rng.random(n) < 0.9)          # some cells without a partner
    KB = rng.uniform(0.1, 1.5, nb)
    if variant == "zero_K":
        K[:] = 0.0
    elif variant == "one_K":
        K[:] = 0.0
        K[n // 2] = 0.7
    elif variant == "denormal_K":
        K = K * 1e-310
    Ks = np.zeros(n) if variant == "zero_Ks" else rng.uniform(0.0, 2.0, n)
    K2 = rng.uniform(0.0, 1.0, n)
    sd = rng.uniform(0.0, 0.1, n)
    origin = np.full(3, off)
    PXB = K[:, None] * (B[rng.integers(0, nb, n)] - origin + 0.05 * rng.standard_normal((n, 3)))
    kappa = np.full(n, {"kappa_small": 1e-3, "kappa_large": 1e3}.get(variant, 1.0)) * rng.uniform(1.0, 1.5, n)
    th = 0.4
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.2), -np.sin(0.2)], [0, np.sin(0.2), np.cos(0.2)]])
    if variant == "reflection":
        R = R @ np.diag([1.0, 1.0, -1.0])
    t = rng.standard_normal(3) + off * (1.0 - R.sum(1))
    return dict(n=n, nb=nb, A=A, B=B, V=V, K=K, KB=KB, Ks=Ks, K2=K2, sd=sd, PXB=PXB, kappa=kappa, R=R, t=t, origin=origin,
                sigma2=0.3, Sp_spatial=float(Ks.sum()))


CASES = [(n, "base") for n in SIZES] + [(n, v) for v in VARIANTS for n in (257, 1025)]


def _v4(inp, dtype):
    """VnA as the x4 tensor of the cell dtype, and widened back to float64 (what the kernels see)."""
    tdt = torch.float32 if dtype == "float32" else torch.float64
    V4 = torch.zeros(inp["n"], 4, dtype=tdt, device=DEV)
    V4[:, :3] = _dev(inp["V"]).to(tdt)
    return V4, V4[:, :3].to(torch.float64).cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n, variant", CASES)
def test_moments(n, variant, dtype):
    k, lib = _k(dtype), _k(dtype).lib
    inp = make_inputs(n, variant)
    nb = inp["nb"]
    V4, Vw = _v4(inp, dtype)
    d = {q: _dev(inp[q]) for q in ("A", "B", "K", "KB", "Ks", "K2", "sd", "PXB")}
    extra = _dev(np.array([3.25]))
    need = int(lib.mvf_align_workspace_bytes(n, nb))
    assert need > 0 and need % 8 == 0
    import ctypes

    org = (ctypes.c_double * 3)(*inp["origin"])
    outs = []
    for rep in range(2):
        ws = torch.full((need // 8 + GUARD,), float("nan"), dtype=torch.float64, device=DEV)
        ws[need // 8:] = SENTINEL[torch.float64]
        out = _guarded(64)
        rc = lib.mvf_align_moments(d["A"].data_ptr(), V4.data_ptr(), d["K"].data_ptr(), d["Ks"].data_ptr(), d["K2"].data_ptr(),
                                   d["sd"].data_ptr(), d["PXB"].data_ptr(), n, d["B"].data_ptr(), d["KB"].data_ptr(), nb, org,
                                   extra.data_ptr(), out.data_ptr(), ws.data_ptr(), need, k.cdtype, k._stream())
        assert rc == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        assert _intact(out, 64) and _intact(ws, need // 8)
        outs.append(out[:64].cpu().numpy())
    assert _same_bits(outs[0], outs[1])
    got = outs[0]
    assert np.isfinite(got).all() and got[50] == 3.25 and np.all(got[51:] == 0.0)
    val, mag = lc.moments_reference(inp["A"], Vw, inp["K"], inp["Ks"], inp["K2"], inp["sd"], inp["PXB"], inp["B"], inp["KB"],
                                    inp["origin"], mu=got[14:23])
    slack = n * 5e-324 * 64 if variant == "denormal_K" else 0.0   # products of denormal weights land on the denormal grid
    worst = 0.0
    for i in list(range(14)) + list(range(23, 50)):
        bound = 1e-12 * mag[i] + slack
        assert abs(got[i] - val[i]) <= bound, (i, got[i], val[i], mag[i])
        worst = max(worst, abs(got[i] - val[i]) / bound if bound > 0 else 0.0)
    Sp = val[9]
    for i in range(9):   # the means against the fsum'd first-order sums
        bound = 2e-12 * mag[i] / Sp + slack / Sp
        assert abs(got[14 + i] - val[i] / Sp) <= bound, (i, got[14 + i], val[i] / Sp)
    _note(f"moments {variant}", dtype, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n, variant", CASES)
def test_transform(n, variant, dtype):
    import ctypes

    k, lib = _k(dtype), _k(dtype).lib
    inp = make_inputs(n, variant)
    tdt, npdt = (torch.float32, np.float32) if dtype == "float32" else (torch.float64, np.float64)
    V4, Vw = _v4(inp, dtype)
    d = {q: _dev(inp[q]) for q in ("A", "K", "PXB")}
    Rt = (ctypes.c_double * 12)(*inp["R"].reshape(9), *inp["t"])
    org = (ctypes.c_double * 3)(*inp["origin"])
    runs = []
    for rep in range(2):
        bufs = {"RnA": _guarded(3 * n), "XAHat": _guarded(3 * n), "xa4": _guarded(4 * n, tdt), "PXB_term": _guarded(3 * n),
                "Y4": _guarded(4 * n, tdt), "Pw": _guarded(n, tdt)}
        rc = lib.mvf_align_transform(d["A"].data_ptr(), V4.data_ptr(), d["PXB"].data_ptr(), d["K"].data_ptr(), n, Rt, org,
                                     *(bufs[q].data_ptr() for q in ("RnA", "XAHat", "xa4", "PXB_term", "Y4", "Pw")), k.cdtype,
                                     k._stream())
        assert rc == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        sizes = {"RnA": 3 * n, "XAHat": 3 * n, "xa4": 4 * n, "PXB_term": 3 * n, "Y4": 4 * n, "Pw": n}
        assert all(_intact(bufs[q], sizes[q]) for q in bufs)
        runs.append({q: bufs[q][: sizes[q]].cpu().numpy() for q in bufs})
    assert all(_same_bits(runs[0][q], runs[1][q]) for q in runs[0])
    ref = dict(zip(("RnA", "XAHat", "xa4", "PXB_term", "Y4", "Pw"),
                   lc.transform_reference(inp["A"], Vw, inp["PXB"], inp["K"], inp["R"], inp["t"], inp["origin"], npdt)))
    for q, r in ref.items():
        assert _same_bits(runs[0][q], np.ascontiguousarray(r).reshape(-1)), (q, np.abs(runs[0][q] - r.reshape(-1)).max())
    if variant in ("zero_K", "one_K"):
        Y = runs[0]["Y4"].reshape(n, 4)
        assert np.all(Y[inp["K"] == 0] == 0.0)          # update_nonrigid's rule: rows with K_NA == 0 give 0
    # a subset of the outputs: the others are not touched
    only = _guarded(3 * n)
    rc = lib.mvf_align_transform(d["A"].data_ptr(), None, None, None, n, Rt, None, only.data_ptr(), None, None, None, None, None,
                                 k.cdtype, k._stream())
    assert rc == 0, lib.mvf_last_error()
    torch.cuda.synchronize()
    r0 = lc.transform_reference(inp["A"], np.zeros((n, 3)), inp["PXB"], inp["K"], inp["R"], inp["t"], np.zeros(3), npdt)[0]
    assert _intact(only, 3 * n) and _same_bits(only[: 3 * n].cpu().numpy(), r0.reshape(-1))
    _note(f"transform {variant}", dtype, 0.0)


@pytest.mark.parametrize("n, variant", CASES)
def test_alpha(n, variant):
    k, lib = _k("float64"), _k("float64").lib
    inp = make_inputs(n, variant)
    d = {q: _dev(inp[q]) for q in ("kappa", "Ks", "sd")}
    runs = []
    for rep in range(2):
        al, mm = _guarded(n), _guarded(n)
        rc = lib.mvf_align_alpha(d["kappa"].data_ptr(), d["Ks"].data_ptr(), d["sd"].data_ptr(), n, inp["Sp_spatial"],
                                 inp["sigma2"], al.data_ptr(), mm.data_ptr(), k._stream())
        assert rc == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        assert _intact(al, n) and _intact(mm, n)
        runs.append((al[:n].cpu().numpy(), mm[:n].cpu().numpy()))
    assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1])
    ra, rm = lc.alpha_reference(inp["kappa"], inp["Ks"], inp["sd"], inp["Sp_spatial"], inp["sigma2"])
    assert np.all(np.abs(runs[0][0] - ra) <= 1e-12 * np.abs(ra)) and np.all(np.abs(runs[0][1] - rm) <= 1e-12 * np.abs(rm))
    pos = ra > 0
    if pos.any():
        _note(f"alpha {variant}", "float64", float((np.abs(runs[0][0] - ra)[pos] / ra[pos]).max() / 1e-12))


CONVENTION_COVERS = {"mvf_align_alpha": MODES, "mvf_align_moments": MODES, "mvf_align_transform": MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [257, 1025])   # one workgroup and a partial one; more than one block of partial sums
def test_calling_conventions(n, dtype, mode):
    """mvf_align_alpha, mvf_align_moments and mvf_align_transform of one slice pair: the plain calls' bits on a side stream
    behind poisoned inputs, at displaced pointers (VnA one row, every other array one element), and with the inputs unchanged."""
    import ctypes

    k, lib = _k(dtype), _k(dtype).lib
    inp = make_inputs(n, "base")
    nb, tdt = inp["nb"], torch.float32 if dtype == "float32" else torch.float64
    need = int(lib.mvf_align_workspace_bytes(n, nb))
    org = (ctypes.c_double * 3)(*inp["origin"])
    Rt = (ctypes.c_double * 12)(*inp["R"].reshape(9), *inp["t"])

    def call():
        d = {q: _dev(inp[q]) for q in ("A", "B", "K", "KB", "Ks", "K2", "sd", "PXB", "kappa")}
        V4, extra = _sx4(inp["V"], dtype), _dev(np.array([3.25]))
        al, mm = _guarded(n), _guarded(n)
        rc = lib.mvf_align_alpha(d["kappa"].data_ptr(), d["Ks"].data_ptr(), d["sd"].data_ptr(), n, inp["Sp_spatial"], inp["sigma2"],
                                 al.data_ptr(), mm.data_ptr(), k._stream())
        _called()
        assert rc == 0, lib.mvf_last_error()
        ws, out = _guarded(need // 8, fill=float("nan")), _guarded(64)
        rc = lib.mvf_align_moments(d["A"].data_ptr(), V4.data_ptr(), d["K"].data_ptr(), d["Ks"].data_ptr(), d["K2"].data_ptr(),
                                   d["sd"].data_ptr(), d["PXB"].data_ptr(), n, d["B"].data_ptr(), d["KB"].data_ptr(), nb, org,
                                   extra.data_ptr(), out.data_ptr(), ws.data_ptr(), need, k.cdtype, k._stream())
        _called()
        assert rc == 0, lib.mvf_last_error()
        sizes = {"RnA": 3 * n, "XAHat": 3 * n, "xa4": 4 * n, "PXB_term": 3 * n, "Y4": 4 * n, "Pw": n}
        bufs = {q: _guarded(sizes[q], tdt if q in ("xa4", "Y4", "Pw") else torch.float64) for q in sizes}
        rc = lib.mvf_align_transform(d["A"].data_ptr(), V4.data_ptr(), d["PXB"].data_ptr(), d["K"].data_ptr(), n, Rt, org,
                                     *(bufs[q].data_ptr() for q in sizes), k.cdtype, k._stream())
        _called()
        assert rc == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        assert _intact(ws, need // 8)
        return [_take(al, n), _take(mm, n), _take(out, 64)] + [_take(bufs[q], sizes[q]) for q in sizes]

    plain, got = _under(mode, call)
    assert np.isfinite(plain[2]).all() and plain[2][50] == 3.25
    assert all(_same_bits(a, b) for a, b in zip(plain, got))


def test_empty_and_refusals():
    lib = _k("float64").lib
    p = torch.zeros(64, dtype=torch.float64, device=DEV).data_ptr()
    assert lib.mvf_align_workspace_bytes(0, 5) == 0 and lib.mvf_align_workspace_bytes(5, 0) == 0
    assert lib.mvf_align_alpha(None, None, None, 0, 0.0, 1.0, None, None, None) == 0
    assert lib.mvf_align_transform(None, None, None, None, 0, None, None, None, None, None, None, None, None, 1, None) == 0
    assert lib.mvf_align_moments(None, None, None, None, None, None, None, 0, None, None, 3, None, None, None, None, 0, 1, None) == 0
    assert lib.mvf_align_alpha(p, p, p, 5, 1.0, 0.0, p, p, None) != 0 and b"sigma2" in lib.mvf_last_error()
    assert lib.mvf_align_moments(p, p, p, p, p, p, p, 5, p, p, 5, None, None, p, p, 8, 1, None) != 0
    assert b"workspace too small" in lib.mvf_last_error()
    assert lib.mvf_align_transform(p, None, None, None, 5, None, None, p, None, None, None, None, None, 1, None) != 0
    assert lib.mvf_align_transform(p, None, None, None, 5, (__import__("ctypes").c_double * 12)(), None, None, None, None, p, None,
                                   None, 1, None) != 0 and b"need PXB and K_NA" in lib.mvf_last_error()
