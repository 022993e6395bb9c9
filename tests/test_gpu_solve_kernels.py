"""Kernel-level edge tests of the coefficient-solve family - csrc/mvf_solve.hip, csrc/mvf_minnorm.hip, csrc/mvf_chol_dev.h -
through the raw C ABI on ``cuda:0``: mvf_solve, mvf_solve_minnorm (with ``reuse``, ``basis`` and ``warm``),
mvf_solve_minnorm_lr, mvf_lr_pivot_order, mvf_solve_minnorm_lrd, mvf_solve_minnorm_lrd_async and mvf_pinv_diag, at m = 1 and
on either side of every padding and switch of the drivers (64, 128, 512, 640).

Matrices have a spectrum known by construction and the references are np.longdouble (tests/_solve_cases.py); the bound on
max|C - C*| / max|C*| per column is C_BOUND m eps kappa_kept with C_BOUND measured on the CPU, and
tests/test_solve_kernel_refs.py proves without a GPU that the float64 LAPACK route stays within a 16th of it while each
targeted defect leaves it by >= 100 x.

Every output (C, info, einfo, pivots, basis, diag) sits inside a larger tensor with a sentinel in 4096 elements either side;
the workspace is exactly *_workspace_bytes long inside 4096 guard bytes and starts filled with 0xA5 (zero where a test says
so), so a kernel that reads a word it never wrote, or writes one element past an output, does not pass.  Repeated calls are
bit-identical.  Two checks that the code does not meet are kept as strict expected failures, one case each, with their
figures: the warm start's sweep count on the rank-1 family on a moved matrix, and einfo[3] / einfo[5] of the deflated forms of
mvf_solve_minnorm_lrd (block Ritz values, 5e-7 ... 4e-4 above the eigenvalue).  Run with ``-s`` for the largest |deviation| / bound per (entry point, family):
profiles/solve_kernel_edges.md records them."""
import ctypes

import numpy as np
import pytest
import torch

import _solve_cases as sc
from _kernel_scaffold import (MODES, SENTINEL as _SENTINEL, WS_FILL, called as _called, dev as _dev, deviation_table, kernel_cache,
                              option as _option, Out as _Out, same_bits as _same_bits, settle as _settle, stream as _stream,
                              under as _under, Ws as _Ws, x4 as _x4)

pytestmark = pytest.mark.gpu

LD = np.longdouble
SENTINEL, ISENTINEL = _SENTINEL[torch.float64], _SENTINEL[torch.int32]  # what untouched float64 / int32 outputs hold
_REFS = {}
_k = kernel_cache()
_note, _deviation_table = deviation_table(
    "| entry point | family | largest |deviation| / bound |",
    footer=lambda seconds, notes: f"test_gpu_solve_kernels: {seconds:.1f} s, {notes} reference comparisons")


def _lib():
    return _k().lib


def _last_error():
    return _lib().mvf_last_error().decode("utf-8", "replace")


_DEVICE_CASES = {}


def _operands(c):
    """G, K on the device (kept for the module: the cases are shared and never written)."""
    if c["id"] not in _DEVICE_CASES:
        _DEVICE_CASES[c["id"]] = (_dev(c["G"]), _dev(c["K"]))
    return _DEVICE_CASES[c["id"]]


class _Result:
    pass


def _call(entry, Gd, Kd, ls2, R, *, jitter=0.0, shift=sc.SHIFT, rcond=2.0 ** -52, tolf=0.25, max_sweeps=60, reuse=0,
          rank_hint=0, form_hint=1, basis=None, warm=0, ws=None, ws_bytes=None, einfo=None, want_pivots=True):
    """One raw-ABI call of a solve entry point inside guards.  Returns the outputs (host copies), the return code and the
    workspace; asserts the guards around every output and the workspace."""
    lib, m, nrhs = _lib(), Gd.shape[0], R.shape[1]
    Rd = _dev(R)
    need = {"solve": lib.mvf_solve_workspace_bytes, "minnorm": lib.mvf_solve_minnorm_workspace_bytes,
            "lr": lib.mvf_solve_minnorm_lr_workspace_bytes, "lrd": lib.mvf_solve_minnorm_lrd_workspace_bytes,
            "lrd_async": lib.mvf_solve_minnorm_lrd_workspace_bytes}[entry](m, nrhs)
    if ws is None:
        ws = _Ws(need)
    nbytes = ws.nbytes if ws_bytes is None else ws_bytes
    C, info, piv = _Out(m, nrhs), _Out(1, dtype=torch.int32), _Out(2)
    einfo = _Out(12) if einfo is None else einfo
    _settle()
    if entry == "solve":
        rc = lib.mvf_solve(Gd.data_ptr(), Kd.data_ptr(), float(ls2), float(jitter), Rd.data_ptr(), m, nrhs, C.ptr, info.ptr,
                           piv.ptr if want_pivots else None, ws.ptr, nbytes, _stream())
    elif entry == "minnorm":
        rc = lib.mvf_solve_minnorm(Gd.data_ptr(), Kd.data_ptr(), float(ls2), float(shift), float(rcond), Rd.data_ptr(), m, nrhs,
                                   C.ptr, info.ptr, einfo.ptr, int(max_sweeps), int(reuse), basis.ptr if basis is not None else None,
                                   int(warm), ws.ptr, nbytes, _stream())
    elif entry in ("lr", "lrd"):
        fn = lib.mvf_solve_minnorm_lr if entry == "lr" else lib.mvf_solve_minnorm_lrd
        rc = fn(Gd.data_ptr(), Kd.data_ptr(), float(ls2), float(tolf), float(rcond), Rd.data_ptr(), m, nrhs, C.ptr, info.ptr,
                einfo.ptr, int(max_sweeps), int(reuse), int(rank_hint), ws.ptr, nbytes, _stream())
    else:
        rc = lib.mvf_solve_minnorm_lrd_async(Gd.data_ptr(), Kd.data_ptr(), float(ls2), float(tolf), float(rcond), Rd.data_ptr(), m,
                                             nrhs, C.ptr, info.ptr, einfo.ptr, int(form_hint), ws.ptr, nbytes, _stream())
    _called(synchronising=entry in ("minnorm", "lr", "lrd"))   # (include/mvf.h: these three read ranks and pivots back)
    torch.cuda.synchronize()
    for o in (C, info, piv, einfo) + ((basis,) if basis is not None else ()):
        assert o.guards_intact(), f"{entry}: an output guard was written"
    assert ws.guards_intact(), f"{entry}: a workspace guard was written"
    out = _Result()
    out.rc, out.ws, out.C_untouched, out.piv_untouched = rc, ws, C.untouched(), piv.untouched()
    out.C, out.info, out.piv, out.einfo = C.host(), int(info.host()[0]), piv.host(), einfo.host()
    return out


def _cstar(c, R):
    key = (c["id"], R.shape, np.ascontiguousarray(R).tobytes())
    if key not in _REFS:
        _REFS[key] = sc.c_star(c, R)
    return _REFS[key]


def _chol_ref(c, jitter):
    key = ("chol", c["id"], jitter)
    if key not in _REFS:
        _REFS[key] = sc.cholesky_solve_ld(c["A"], c["R"], jitter)
    return _REFS[key]


def _within(entry, c, C, Cs, what=""):
    r = sc.ratio(C, Cs, c)
    print(f"{entry} {c['id']} nrhs {C.shape[1]} {what}: |dC| / bound = {r:.3g}")
    _note(entry, c["family"], r)
    assert r <= 1.0, (entry, c["id"], what, r)
    return r


# ================================================================================================== calling conventions
CONVENTION_COVERS = {"mvf_solve": MODES, "mvf_solve_minnorm": MODES, "mvf_solve_minnorm_lr": MODES, "mvf_solve_minnorm_lrd": MODES,
                     "mvf_solve_minnorm_lrd_async": MODES, "mvf_lr_pivot_order": MODES, "mvf_pinv_diag": MODES}


def _conv_solve(path):
    c = sc.solve_cases([65])[0]
    with _option("solve_small_off", 1 if path == "blocked" else 0):
        a = _call("solve", _dev(c["G"]), _dev(c["K"]), c["ls2"], c["R"][:, :3])
    assert a.rc == 0 and a.info == 0, _last_error()
    return a.C, a.piv


def _conv_pinv(a, lc, dtype, lowrank):
    pc, n = lc["pc"], 257
    x4, c4, out = _x4(lc["X"][:n], lc["X"].dtype), _x4(lc["ctrl"], lc["ctrl"].dtype), _Out(n)
    rc = _lib().mvf_pinv_diag(x4.data_ptr(), n, c4.data_ptr(), len(lc["ctrl"]), pc["beta"], pc["rcond"], lowrank, out.ptr, a.ws.ptr,
                              a.ws.nbytes, _k(dtype).cdtype, _stream())
    _called(synchronising=bool(lowrank))   # (include/mvf.h: "Synchronises `stream` once on the lowrank path")
    torch.cuda.synchronize()
    assert rc == 0 and out.guards_intact() and a.ws.guards_intact(), _last_error()
    return out.host()


def _conv_minnorm(dtype):
    """mvf_solve_minnorm, then mvf_pinv_diag on the decomposition it left."""
    lc = _leverage_case(129, dtype)
    a = _call("minnorm", _dev(lc["A"]), _dev(np.zeros((129, 129))), 0.0, np.ones((129, 3)), rcond=lc["pc"]["rcond"])
    assert a.rc == 0 and a.info == 0, _last_error()
    return a.C, a.einfo[:10], _conv_pinv(a, lc, dtype, 0)


def _conv_lr(dtype):
    """mvf_solve_minnorm_lr, then mvf_lr_pivot_order and mvf_pinv_diag on the factorisation it left."""
    lc = _leverage_case(129, dtype)
    a = _call("lr", _dev(lc["A"]), _dev(np.zeros((129, 129))), 0.0, np.ones((129, 3)), rcond=lc["pc"]["rcond"])
    assert a.rc == 0 and a.info == 0, _last_error()
    rc, order, vals, tol = _pivot_order(a.ws, 129)
    _called(synchronising=True)   # (include/mvf.h: "Synchronises `stream`")
    assert rc == 0
    return a.C, a.einfo[:10], order, vals, np.array([tol]), _conv_pinv(a, lc, dtype, 1)


def _conv_lrd(form):
    """mvf_solve_minnorm_lrd on its Jacobi path, or in its factor form, then mvf_solve_minnorm_lrd_async and the synchronous
    direct form on the state each call leaves to the next."""
    m = 128
    c = sc.make_case("well", m)
    Gd, Kd, R = _dev(c["G"]), _dev(c["K"]), c["R"][:, :5]
    if form == "jacobi":
        with _option("lr_no_deflate", 1):
            j = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"])
        assert j.rc == 0 and int(j.einfo[8]) == 0
        return j.C, j.einfo[:10]
    ws = _Ws(_lib().mvf_solve_minnorm_lrd_workspace_bytes(m, 5), fill=0)
    s0 = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"], ws=ws)
    assert s0.rc == 0 and int(s0.einfo[8]) == 1
    a1 = _call("lrd_async", Gd, Kd, c["ls2"], R, rcond=c["rcond"], form_hint=int(s0.einfo[8]), ws=ws)
    assert a1.rc == 0 and a1.info == 0 and int(a1.einfo[8]) == 2, a1.einfo
    s2 = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"], rank_hint=m, ws=ws)
    assert s2.rc == 0 and int(s2.einfo[8]) == 2
    return s0.C, s0.einfo[:10], a1.C, a1.einfo[:10], s2.C, s2.einfo[:10]


CONVENTION_CASES = {"mvf_solve:small": (_conv_solve, "small"), "mvf_solve:blocked": (_conv_solve, "blocked"),
                    "mvf_solve_minnorm+pinv_diag:float64": (_conv_minnorm, "float64"),
                    "mvf_solve_minnorm+pinv_diag:float32": (_conv_minnorm, "float32"),
                    "mvf_solve_minnorm_lr+pivot_order+pinv_diag:float64": (_conv_lr, "float64"),
                    "mvf_solve_minnorm_lr+pivot_order+pinv_diag:float32": (_conv_lr, "float32"),
                    "mvf_solve_minnorm_lrd:jacobi": (_conv_lrd, "jacobi"), "mvf_solve_minnorm_lrd:factor+async+direct": (_conv_lrd, "factor")}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", list(CONVENTION_CASES))
def test_calling_conventions(entry, mode):
    """The plain calls' bits on a side stream behind poisoned inputs, at displaced pointers, and with the inputs unchanged.
    The minimum-norm solves, mvf_lr_pivot_order and the low-rank mvf_pinv_diag synchronise their stream (include/mvf.h): the
    side stream protects their launches up to that point; mvf_solve and mvf_solve_minnorm_lrd_async must return while the
    inputs are still in flight."""
    fn, arg = CONVENTION_CASES[entry]
    plain, got = _under(mode, lambda: fn(arg))
    assert len(plain) == len(got) and all(_same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(plain, got))


# ================================================================================================== mvf_solve
def _solve_case(c, path, nrhs_list, jitter=0.0):
    """mvf_solve on one case and path: C against the longdouble Cholesky solve, pivots, info, the call repeated on the used
    workspace bit-identical to the one on the pattern-filled workspace."""
    Gd, Kd = _operands(c)
    Cr, pr = _chol_ref(c, jitter)
    out = {}
    with _option("solve_small_off", 1 if path == "blocked" else 0):
        for nrhs in nrhs_list:
            R = c["R"][:, :nrhs]
            a = _call("solve", Gd, Kd, c["ls2"], R, jitter=jitter)
            assert a.rc == 0 and a.info == 0, (a.rc, a.info, _last_error())
            _within(f"mvf_solve[{path}]", c, a.C, Cr[:, :nrhs], f"jitter {jitter:g}")
            np.testing.assert_allclose(a.piv, np.asarray(pr, dtype=np.float64), rtol=1e-12 * c["kappa"])
            b = _call("solve", Gd, Kd, c["ls2"], R, jitter=jitter, ws=a.ws)
            assert b.rc == 0 and _same_bits(a.C, b.C) and _same_bits(a.piv, b.piv)
            out[nrhs] = a.C
        R = c["R"][:, :nrhs_list[0]]
        a = _call("solve", Gd, Kd, c["ls2"], R, jitter=jitter, want_pivots=False)  # pivots may be NULL
        assert a.rc == 0 and a.piv_untouched and _same_bits(a.C, out[nrhs_list[0]])
    return out


@pytest.mark.parametrize("m", sc.SOLVE_M_BLOCKED)
def test_solve_blocked_path(m):
    for c in sc.solve_cases([m]):
        _solve_case(c, "blocked", sc.solve_nrhs(m))


@pytest.mark.parametrize("m", sc.SOLVE_M_SMALL)
def test_solve_small_path_and_the_two_paths_agree(m):
    for c in sc.solve_cases([m]):
        small = _solve_case(c, "small", sc.solve_nrhs(m))
        blocked = _solve_case(c, "blocked", [8])
        r = sc.col_dev(small[8], blocked[8]) / sc.bound(c)
        _note("mvf_solve[small vs blocked]", c["family"], r)
        assert r <= 1.0, (c["id"], r)


@pytest.mark.parametrize("m,path", [(100, "small"), (100, "blocked"), (193, "blocked")])
@pytest.mark.parametrize("jitter", [0.0, 1e-6, 1e-2])
def test_solve_jitter_is_scaled_by_the_mean_of_the_diagonal(m, path, jitter):
    for c in sc.solve_cases([m]):
        _solve_case(c, path, [3], jitter=jitter)


@pytest.mark.parametrize("m,path,bad", [(193, "blocked", 0), (193, "blocked", 70), (193, "blocked", 130), (100, "small", 0),
                                        (100, "small", 70), (100, "blocked", 70)])
def test_solve_reports_the_first_non_positive_pivot(m, path, bad):
    G, K, ls2, _ = sc.indefinite_for_solve(m, bad)
    R = sc.make_case("well", m)["R"][:, :3]
    with _option("solve_small_off", 1 if path == "blocked" else 0):
        a = _call("solve", _dev(G), _dev(K), ls2, R)
        b = _call("solve", _dev(G), _dev(K), ls2, R, ws=a.ws)
    assert a.rc == 0 and a.info == 1 + bad and b.info == 1 + bad


def test_solve_refusals():
    lib = _lib()
    c = sc.make_case("well", 65)
    Gd, Kd = _operands(c)
    R9 = _dev(np.zeros((65, 9)))
    for nrhs in (0, 9):
        C, info, ws = _Out(65, 9), _Out(1, dtype=torch.int32), _Ws(lib.mvf_solve_workspace_bytes(65, 8))
        rc = lib.mvf_solve(Gd.data_ptr(), Kd.data_ptr(), c["ls2"], 0.0, R9.data_ptr(), 65, nrhs, C.ptr, info.ptr, None, ws.ptr,
                           ws.nbytes, _stream())
        torch.cuda.synchronize()
        assert rc != 0 and "nrhs" in _last_error() and C.untouched() and info.untouched()
    need = lib.mvf_solve_workspace_bytes(65, 3)
    for kw in (dict(jitter=-1e-9), dict(ws=_Ws(need - 1))):  # negative jitter; a workspace one byte short
        a = _call("solve", Gd, Kd, c["ls2"], c["R"][:, :3], **kw)
        assert a.rc != 0 and a.C_untouched and a.info == ISENTINEL and a.piv_untouched, (kw, _last_error())
    # m = 0: nothing to solve, info = 0
    info = _Out(1, dtype=torch.int32)
    rc = lib.mvf_solve(None, None, 0.0, 0.0, None, 0, 3, None, info.ptr, None, None, 0, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and int(info.host()[0]) == 0 and info.guards_intact() and lib.mvf_solve_workspace_bytes(0, 3) == 0


# ================================================================================================== mvf_solve_minnorm
def _designed(c):
    lam = np.asarray(c["lam"], dtype=np.float64)
    return float(np.abs(lam).max()), float(np.abs(lam[c["keep"]]).min()), float(lam.min())


def _check_minnorm_einfo(entry, c, e, shift=None):
    lmax, lmin_kept, lmin = _designed(c)
    eb = sc.eig_bound(c)
    assert int(e[1]) == c["rank"] and e[1] == np.floor(e[1]), (entry, c["id"], e[1], c["rank"])
    assert e[0] == np.floor(e[0]) and 0 <= e[0] < 60, (entry, c["id"], e[0])  # an integer: x.5 would be the sweep cap
    for i, want in ((2, lmax), (3, lmin_kept)) + (((5, lmin),) if shift is not None else ()):
        r = abs(e[i] - want) / eb
        _note(f"{entry} einfo[{i}]", c["family"], r)
        assert r <= 1.0, (entry, c["id"], i, e[i], want)
    if shift is not None:
        d = np.asarray(np.diag(c["G"]), dtype=LD) + LD(c["ls2"]) * np.asarray(np.diag(c["K"]), dtype=LD)
        want = float(LD(shift) * d.sum() / c["m"])
        assert abs(e[4] - want) <= 1e-14 * want, (c["id"], e[4], want)
    else:
        assert e[4] == 0.0


@pytest.mark.parametrize("m", sc.MINNORM_M)
def test_minnorm_against_the_designed_spectrum(m):
    for c in sc.minnorm_cases([m]):
        Gd, Kd = _operands(c)
        shift = sc.minnorm_shift(c)
        first = None
        for nrhs in (1, 5, 8):
            R = c["R"][:, :nrhs]
            a = _call("minnorm", Gd, Kd, c["ls2"], R, shift=shift, rcond=c["rcond"])
            assert a.rc == 0 and a.info == 0, (c["id"], a.rc, a.info, _last_error())
            _within("mvf_solve_minnorm", c, a.C, _cstar(c, R))
            _check_minnorm_einfo("mvf_solve_minnorm", c, a.einfo, shift)
            assert np.all(a.einfo[6:] == SENTINEL)
            if first is None:
                first = a
                b = _call("minnorm", Gd, Kd, c["ls2"], R, shift=shift, rcond=c["rcond"], ws=a.ws)  # on the used workspace
                assert b.rc == 0 and _same_bits(a.C, b.C) and _same_bits(a.einfo, b.einfo)
            else:
                assert _same_bits(a.einfo[1:6], first.einfo[1:6])  # the decomposition does not depend on the right-hand side
        # reuse: another R, another nrhs, on the workspace of the nrhs = 8 call
        R2 = np.ascontiguousarray(c["R"][:, ::-1][:, :5]) * 1.5
        e2 = _Out(12)
        r = _call("minnorm", Gd, Kd, c["ls2"], R2, shift=shift, rcond=c["rcond"], reuse=1, ws=a.ws, einfo=e2)
        assert r.rc == 0 and r.info == 0
        _within("mvf_solve_minnorm reuse", c, r.C, _cstar(c, R2))
        assert np.all(r.einfo[:7] == SENTINEL) and _same_bits(r.einfo[7:12], a.einfo[1:6])  # [7..11] this call's, the rest untouched


@pytest.mark.parametrize("m", [65, 129])
def test_minnorm_basis_and_warm_start(m):
    """basis_extract_kernel's promise: row i = Y_i / sigma_i for the rows the Jacobi iteration left non-zero, the unit vector
    e_i for a zero row - which keeps Wt orthogonal in the padded space only if the zero rows are exactly the padding rows
    m .. mp-1 and the live rows are zero on the padded columns."""
    mp = sc.pad(m)
    for c in sc.minnorm_cases([m]):
        Gd, Kd = _operands(c)
        shift, R = sc.minnorm_shift(c), c["R"][:, :5]
        basis = _Out(mp, mp)
        assert _lib().mvf_solve_minnorm_basis_bytes(m) == mp * mp * 8
        cold = _call("minnorm", Gd, Kd, c["ls2"], R, shift=shift, rcond=c["rcond"], basis=basis)
        assert cold.rc == 0 and cold.info == 0
        plain = _call("minnorm", Gd, Kd, c["ls2"], R, shift=shift, rcond=c["rcond"])
        assert _same_bits(cold.C, plain.C) and _same_bits(cold.einfo[:6], plain.einfo[:6])  # asking for the basis changes nothing
        Wt = basis.host()
        tol = sc.C_BOUND * m * sc.EPS
        assert np.all(Wt[:m, m:] == 0.0), c["id"]                          # padded columns of the live rows: exactly 0
        assert np.array_equal(Wt[m:], np.eye(mp)[m:]), c["id"]             # padded rows: exactly the unit vectors
        Q = Wt[:m, :m].astype(LD)
        orth = float(np.abs(Q @ Q.T - np.eye(m)).max())
        _note("mvf_solve_minnorm basis orthonormality / (c m eps)", c["family"], orth / tol)
        assert orth <= tol, (c["id"], orth)
        A = c["A"].astype(LD)
        AQ = Q @ A                                                          # row i = (A q_i)^T
        lam = np.einsum("ij,ij->i", AQ, Q)
        res = float(np.abs(AQ - lam[:, None] * Q).max())
        _note("mvf_solve_minnorm basis residual / eigenvalue bound", c["family"], res / sc.eig_bound(c))
        assert res <= sc.eig_bound(c), (c["id"], res)
        dl = float(np.abs(np.sort(lam) - np.sort(np.asarray(c["lam"], dtype=LD))).max())
        assert dl <= sc.eig_bound(c), (c["id"], dl)
        # warm start on the same matrix, then on a nearby one (its cold call for the sweep count)
        warm = _call("minnorm", Gd, Kd, c["ls2"], R, shift=shift, rcond=c["rcond"], basis=basis, warm=1, ws=cold.ws)
        assert warm.rc == 0 and warm.info == 0 and int(warm.einfo[1]) == c["rank"]
        _within("mvf_solve_minnorm warm", c, warm.C, _cstar(c, R), "same matrix")
        assert warm.einfo[0] <= cold.einfo[0], (c["id"], warm.einfo[0], cold.einfo[0])
        n = sc.nearby_case(c)
        Gn, Kn = _dev(n["G"]), _dev(n["K"])
        ncold = _call("minnorm", Gn, Kn, n["ls2"], R, shift=shift, rcond=n["rcond"])
        nwarm = _call("minnorm", Gn, Kn, n["ls2"], R, shift=shift, rcond=n["rcond"], basis=basis, warm=1, ws=cold.ws)
        assert nwarm.rc == 0 and nwarm.info == 0 and int(nwarm.einfo[1]) == n["rank"] == int(ncold.einfo[1])
        _within("mvf_solve_minnorm warm", n, nwarm.C, sc.c_star(n, R), "nearby matrix")
        _within("mvf_solve_minnorm", n, ncold.C, sc.c_star(n, R), "nearby matrix, cold")
        print(f"    sweeps {c['id']}: cold {cold.einfo[0]:g}, warm {warm.einfo[0]:g}; nearby cold {ncold.einfo[0]:g}, warm "
              f"{nwarm.einfo[0]:g}")


def _warm_sweep_params():
    out = []
    for m in (65, 129):
        for c in sc.minnorm_cases([m]):
            marks = ()
            if c["family"] == "rank1":
                marks = pytest.mark.xfail(strict=True, raises=AssertionError, reason=(
                    "rank 1 on a moved matrix: the warm call takes MORE sweeps than the cold call (measured 10 against 8 at "
                    "m = 65, 10 against 9 at m = 129; profiles/solve_kernel_edges.md).  The one well-determined direction is the "
                    "one that moved; the other m - 1 eigenvalues sit degenerate at the shift, their eigenvectors are arbitrary "
                    "and are re-resolved against the factorisation's rounding noise (mvf.h), so the previous basis carries "
                    "nothing into them and the turned direction couples into them at 1e-2 lambda_max against a diagonal of "
                    "delta.  Not fixed here: C and the kept rank of these calls are within the bound "
                    "(test_minnorm_basis_and_warm_start)"))
            out.append(pytest.param(c, id=c["id"], marks=marks))
    return out


@pytest.mark.parametrize("c", _warm_sweep_params())
def test_minnorm_warm_start_on_a_nearby_matrix_takes_no_more_sweeps_than_the_cold_call(c):
    """warm = 1 with the basis of c on the nearby matrix (lambda moved by 1 %, Q turned by a small rotation) against the cold
    call on that matrix: the sweep count is no larger.  One case per (m, family), so that the one family that misses - rank 1,
    by one or two sweeps - is pinned as an expected failure and not exempted: a change of its count in either direction shows."""
    m, mp = c["m"], sc.pad(c["m"])
    Gd, Kd = _operands(c)
    shift, R = sc.minnorm_shift(c), c["R"][:, :5]
    basis = _Out(mp, mp)
    cold = _call("minnorm", Gd, Kd, c["ls2"], R, shift=shift, rcond=c["rcond"], basis=basis)
    n = sc.nearby_case(c)
    Gn, Kn = _dev(n["G"]), _dev(n["K"])
    ncold = _call("minnorm", Gn, Kn, n["ls2"], R, shift=shift, rcond=n["rcond"])
    nwarm = _call("minnorm", Gn, Kn, n["ls2"], R, shift=shift, rcond=n["rcond"], basis=basis, warm=1, ws=cold.ws)
    assert cold.rc == 0 and ncold.rc == 0 and nwarm.rc == 0 and nwarm.info == 0
    print(f"    nearby {c['id']}: cold {ncold.einfo[0]:g} sweeps, warm {nwarm.einfo[0]:g}")
    assert nwarm.einfo[0] == np.floor(nwarm.einfo[0]) and ncold.einfo[0] == np.floor(ncold.einfo[0])
    assert nwarm.einfo[0] <= ncold.einfo[0], (c["id"], nwarm.einfo[0], ncold.einfo[0])


def test_minnorm_sweep_cap_shift_too_small_and_refusals():
    c = sc.make_case("graded", 129)
    Gd, Kd = _operands(c)
    R = c["R"][:, :3]
    a = _call("minnorm", Gd, Kd, c["ls2"], R, rcond=c["rcond"], max_sweeps=1)
    assert a.rc == 0 and a.info == 0 and a.einfo[0] == 1.5  # the sweep cap was hit before convergence
    # a shift too small for the indefinite matrix: info != 0 and C is not written
    ci = sc.make_case("indef", 129)
    Gi, Ki = _operands(ci)
    a = _call("minnorm", Gi, Ki, ci["ls2"], R, shift=2.0 ** -52, rcond=ci["rcond"])
    assert a.rc == 0 and a.info != 0 and a.C_untouched
    # refusals on the host: nothing is written
    need = _lib().mvf_solve_minnorm_workspace_bytes(129, 3)
    for kw in (dict(warm=1), dict(shift=0.0), dict(shift=1.0), dict(shift=-0.5), dict(ws=_Ws(need - 1))):
        a = _call("minnorm", Gd, Kd, c["ls2"], R, rcond=c["rcond"], **kw)
        assert a.rc != 0 and a.C_untouched and a.info == ISENTINEL and np.all(a.einfo == SENTINEL), (kw, _last_error())


# ================================================================================================== mvf_solve_minnorm_lr
def _pivot_order(ws, m):
    order = (ctypes.c_int * m)()
    vals = (ctypes.c_double * m)()
    tol, r = ctypes.c_double(0.0), ctypes.c_int64(-1)
    rc = _lib().mvf_lr_pivot_order(ws.ptr, ws.nbytes, m, order, vals, ctypes.byref(tol), ctypes.byref(r), _stream())
    if rc != 0:
        return rc, None, None, None
    n = int(r.value)
    return rc, np.frombuffer(order, dtype=np.int32, count=n).copy(), np.frombuffer(vals, dtype=np.float64, count=n).copy(), tol.value


def _check_factor_rank(entry, c, e, tolf):
    """einfo[6], the columns of the rank-revealing factor."""
    r6 = int(e[6])
    if c["family"] == "well":
        assert r6 == c["m"], (entry, c["id"], r6)
    elif c["family"] in ("rank1", "rankhalf", "rankm1"):
        assert r6 == c["rank"], (entry, c["id"], r6, c["rank"])
    else:  # graded spectra: the longdouble greedy rank at the tolerance the device reports, and at most two more
        tol = tolf * sc.EPS * e[2]
        r_ld = len(sc.greedy_pivoted_cholesky_ld(c["A"], tol)[0])
        assert r_ld <= r6 <= r_ld + 2, (entry, c["id"], r6, r_ld)


@pytest.mark.parametrize("m", sc.LR_M)
def test_lr_against_the_designed_spectrum(m):
    for c in sc.lr_cases([m]):
        Gd, Kd = _operands(c)
        first = None
        for nrhs in (1, 5, 8) if m < 511 else (5,):
            R = c["R"][:, :nrhs]
            a = _call("lr", Gd, Kd, c["ls2"], R, rcond=c["rcond"])
            assert a.rc == 0 and a.info == 0, (c["id"], a.rc, a.info, _last_error())
            _within("mvf_solve_minnorm_lr", c, a.C, _cstar(c, R))
            _check_minnorm_einfo("mvf_solve_minnorm_lr", c, a.einfo)
            _check_factor_rank("mvf_solve_minnorm_lr", c, a.einfo, 0.25)
            if int(a.einfo[6]) == c["m"]:  # every column kept: the factor's smallest eigenvalue is the matrix's
                assert abs(a.einfo[5] - _designed(c)[2]) <= sc.eig_bound(c), (c["id"], a.einfo[5])
            assert np.all(a.einfo[7:] == SENTINEL)
            if first is None:
                first = a
                b = _call("lr", Gd, Kd, c["ls2"], R, rcond=c["rcond"], ws=a.ws)  # on the used workspace, no hint
                assert b.rc == 0 and _same_bits(a.C, b.C) and _same_bits(a.einfo[:7], b.einfo[:7])
        # reuse with another R and nrhs: [7..11] this call's, [0..6] untouched
        R2 = np.ascontiguousarray(c["R"][:, ::-1][:, :3]) * 1.5
        e2 = _Out(12)
        r = _call("lr", Gd, Kd, c["ls2"], R2, rcond=c["rcond"], reuse=1, ws=a.ws, einfo=e2)
        assert r.rc == 0 and r.info == 0
        _within("mvf_solve_minnorm_lr reuse", c, r.C, _cstar(c, R2))
        assert np.all(r.einfo[:7] == SENTINEL) and _same_bits(r.einfo[7:12], a.einfo[1:6])


@pytest.mark.parametrize("m", sc.PIVOT_M)
def test_lr_pivot_order_is_the_greedy_order(m):
    c = sc.pivot_case(m)
    Gd, Kd = _dev(c["G"]), _dev(c["K"])
    R = c["R"][:, :3]
    a = _call("lr", Gd, Kd, c["ls2"], R, rcond=c["rcond"])
    assert a.rc == 0 and a.info == 0 and int(a.einfo[6]) == m
    _within("mvf_solve_minnorm_lr", c, a.C, sc.c_star(c, R), "pivot case")
    rc, order, vals, tol = _pivot_order(a.ws, m)
    assert rc == 0 and len(order) == m
    np.testing.assert_allclose(tol, 0.25 * sc.EPS * a.einfo[2], rtol=1e-6)
    ref_order, ref_vals, margins = sc.greedy_pivoted_cholesky_ld(c["A"], tol)
    assert margins.min() >= sc.MARGIN_MIN
    np.testing.assert_array_equal(order, ref_order)  # identical over the full length
    dv = float(np.abs(vals.astype(LD) - ref_vals).max() / ref_vals[0])
    _note("mvf_lr_pivot_order values / (1e-9 first pivot)", "graded", dv / 1e-9)
    assert dv <= 1e-9, dv
    r = _call("lr", Gd, Kd, c["ls2"], c["R"][:, 3:8], rcond=c["rcond"], reuse=1, ws=a.ws)
    assert r.rc == 0
    _within("mvf_solve_minnorm_lr reuse", c, r.C, sc.c_star(c, c["R"][:, 3:8]), "pivot case")
    rc, order2, vals2, tol2 = _pivot_order(a.ws, m)
    assert rc == 0 and np.array_equal(order2, order) and _same_bits(vals2, vals) and tol2 == tol  # untouched by reuse


@pytest.mark.parametrize("m", [65, 129, 513])
def test_lr_rank_hint(m):
    for fam in ("well", "rankhalf") + (("graded", "cluster") if m < 511 else ()):
        c = sc.make_case(fam, m)
        Gd, Kd = _operands(c)
        R = c["R"][:, :5]
        cold = _call("lr", Gd, Kd, c["ls2"], R, rcond=c["rcond"])
        rc0, o0, v0, _ = _pivot_order(cold.ws, m)
        hinted = _call("lr", Gd, Kd, c["ls2"], R, rcond=c["rcond"], rank_hint=int(cold.einfo[6]), ws=cold.ws)
        assert hinted.rc == 0 and hinted.info == 0 and int(hinted.einfo[1]) == int(cold.einfo[1]) == c["rank"]
        _within("mvf_solve_minnorm_lr hinted", c, hinted.C, _cstar(c, R))
        # a hint on a workspace that holds no finished order (pattern-filled) is ignored: the result of the call without one.
        # Not its bits: with rank_hint > 0 the driver runs 5 power steps for lambda_max instead of 8 (the warm start vector
        # it hoped for is refused on the device, the step count was chosen on the host), so the stopping tolerance differs
        # in its last digits and with it nothing but the point where the factorisation stops - same factor rank here, the
        # same pivots in the same order with the same values, C within the bound of C* and of the cold call.
        stale = _call("lr", Gd, Kd, c["ls2"], R, rcond=c["rcond"], rank_hint=int(cold.einfo[6]))
        assert stale.rc == 0 and stale.info == 0
        assert int(stale.einfo[1]) == int(cold.einfo[1]) and int(stale.einfo[6]) == int(cold.einfo[6])
        _within("mvf_solve_minnorm_lr stale hint", c, stale.C, _cstar(c, R))
        rc1, o1, v1, _ = _pivot_order(stale.ws, m)
        assert rc0 == 0 and rc1 == 0 and np.array_equal(o0, o1) and _same_bits(v0, v1)
        assert sc.col_dev(stale.C, cold.C) <= sc.bound(c)


@pytest.mark.parametrize("entry", ["lr", "lrd"])
@pytest.mark.parametrize("fill", [0, WS_FILL])
def test_lr_reuse_is_refused_without_a_finished_decomposition(entry, fill):
    """reuse != 0 on a workspace that holds no finished call (zero-filled: what a fresh allocation of the host wrapper looks
    like; pattern-filled: a foreign one) is refused on the host before anything is launched: non-zero return, the message, and
    neither C, info nor einfo written.  (Before the check the zeroed workspace silently returned C = 0 and the foreign one
    sized launches from whatever number sat in the state record.)"""
    c = sc.make_case("well", 129)
    Gd, Kd = _operands(c)
    need = (_lib().mvf_solve_minnorm_lr_workspace_bytes if entry == "lr" else _lib().mvf_solve_minnorm_lrd_workspace_bytes)(129, 3)
    ws = _Ws(need, fill=fill)
    before = ws.big.clone()
    a = _call(entry, Gd, Kd, c["ls2"], c["R"][:, :3], rcond=c["rcond"], reuse=1, ws=ws)
    assert a.rc != 0, "reuse on a workspace without a finished decomposition was accepted"
    assert "no finished decomposition" in _last_error()
    assert a.C_untouched and a.info == ISENTINEL and np.all(a.einfo == SENTINEL)
    assert torch.equal(ws.big, before)  # nothing reached the device
    rc, _, _, _ = _pivot_order(ws, 129)
    assert rc != 0
    # the same workspace is fine for a fresh call, and reuse behind it works
    a = _call(entry, Gd, Kd, c["ls2"], c["R"][:, :3], rcond=c["rcond"], ws=ws)
    r = _call(entry, Gd, Kd, c["ls2"], c["R"][:, 3:5], rcond=c["rcond"], reuse=1, ws=ws)
    assert a.rc == 0 and r.rc == 0
    _within(f"mvf_solve_minnorm_{entry} reuse", c, r.C, _cstar(c, c["R"][:, 3:5]))


# ================================================================================================== mvf_solve_minnorm_lrd
def _expected_form(r6, forced=0):
    """(einfo[7], einfo[8]) of a cold mvf_solve_minnorm_lrd call from the factor's columns (mvf.h)."""
    if r6 < 128:
        return 0, 0
    if forced:
        return (forced, 1) if r6 >= 2 * forced else (_expected_form(r6)[0], 1)
    return (64, 1) if r6 < 512 else (256, 1)


def _check_lrd_einfo(c, e, form):
    lmax, lmin_kept, _ = _designed(c)
    assert int(e[1]) == c["rank"] and e[4] == 0.0 and e[9] == 0.0, (c["id"], e)
    if form == 0:
        assert abs(e[2] - lmax) <= sc.eig_bound(c) and abs(e[3] - lmin_kept) <= sc.eig_bound(c), (c["id"], e)
    else:
        # lambda_max is the power iteration's estimate (mvf.h).  einfo[3] / [5] are Ritz values of the block (the smallest one
        # above the cut / the smallest one): what holds for ANY block is checked here - never below the eigenvalue they
        # approximate, and by interlacing never above the block-size-th smallest eigenvalue of the factor; the eigenvalue
        # bound itself, from both sides, is test_lrd_smallest_kept_eigenvalue's
        np.testing.assert_allclose(e[2], lmax, rtol=1e-6)
        b = int(e[7])
        kept = np.sort(np.abs(np.asarray(c["lam"], dtype=np.float64)[c["keep"]]))
        top = kept[min(b, len(kept)) - 1]
        for i in (3, 5):
            assert lmin_kept - sc.eig_bound(c) <= e[i] <= top + sc.eig_bound(c), (c["id"], i, e[i], lmin_kept, top)


@pytest.mark.parametrize("m", sc.LRD_M)
def test_lrd_forms_against_the_designed_spectrum_and_the_jacobi_path(m):
    for c in sc.lrd_cases([m]):
        Gd, Kd = _operands(c)
        R = c["R"][:, :5]
        a = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"])
        assert a.rc == 0 and a.info == 0, (c["id"], a.rc, a.info, _last_error())
        _check_factor_rank("mvf_solve_minnorm_lrd", c, a.einfo, 0.25)
        block, form = _expected_form(int(a.einfo[6]))
        print(f"lrd {c['id']}: factor columns {int(a.einfo[6])}, block {int(a.einfo[7])}, form {int(a.einfo[8])}, sweeps {a.einfo[0]:g}")
        assert (int(a.einfo[7]), int(a.einfo[8])) == (block, form), (c["id"], a.einfo)
        _check_lrd_einfo(c, a.einfo, form)
        _within(f"mvf_solve_minnorm_lrd[form {form}, block {block}]", c, a.C, _cstar(c, R))
        b = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"], ws=a.ws)  # on the used workspace, no hint
        assert b.rc == 0 and _same_bits(a.C, b.C) and _same_bits(a.einfo[:10], b.einfo[:10])
        with _option("lr_no_deflate", 1):
            j = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"])
        assert j.rc == 0 and int(j.einfo[7]) == 0 and int(j.einfo[8]) == 0 and int(j.einfo[1]) == c["rank"]
        r = sc.col_dev(a.C, j.C) / sc.bound(c)
        _note("mvf_solve_minnorm_lrd vs its Jacobi path", c["family"], r)
        assert r <= 1.0, (c["id"], r)
        # reuse on this form
        R2 = np.ascontiguousarray(c["R"][:, ::-1][:, :3]) * 1.5
        u = _call("lrd", Gd, Kd, c["ls2"], R2, rcond=c["rcond"], reuse=1, ws=a.ws)
        assert u.rc == 0 and u.info == 0
        _within(f"mvf_solve_minnorm_lrd[form {form}] reuse", c, u.C, _cstar(c, R2))


@pytest.mark.parametrize("m,form", [(128, 2), (640, 2), (641, 1)])
def test_lrd_hinted_second_call_takes_the_direct_form_up_to_640(m, form):
    c = sc.make_case("well", m)
    Gd, Kd = _operands(c)
    R = c["R"][:, :5]
    a = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"])
    assert a.rc == 0 and int(a.einfo[6]) == m and int(a.einfo[8]) == 1
    h = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"], rank_hint=m, ws=a.ws)
    assert h.rc == 0 and h.info == 0 and int(h.einfo[8]) == form and int(h.einfo[6]) == m and h.einfo[9] == 0.0, h.einfo
    assert int(h.einfo[7]) == (64 if form == 2 else _expected_form(m)[0])
    _check_lrd_einfo(c, h.einfo, form)
    _within(f"mvf_solve_minnorm_lrd[hinted, form {form}]", c, h.C, _cstar(c, R))
    R2 = np.ascontiguousarray(c["R"][:, ::-1][:, :3]) * 1.5
    u = _call("lrd", Gd, Kd, c["ls2"], R2, rcond=c["rcond"], reuse=1, ws=a.ws)
    assert u.rc == 0
    _within(f"mvf_solve_minnorm_lrd[hinted, form {form}] reuse", c, u.C, _cstar(c, R2))
    rc, order, _, _ = _pivot_order(a.ws, m)
    assert rc == 0 and sorted(order) == list(range(m))  # the pivot order survives the direct form


@pytest.mark.parametrize("block", [64, 128, 256])
def test_lrd_forced_block_at_641(block):
    c = sc.make_case("well", 641)
    Gd, Kd = _operands(c)
    R = c["R"][:, :5]
    with _option("defl_block", block):
        a = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"])
    assert a.rc == 0 and a.info == 0 and int(a.einfo[6]) == 641
    assert (int(a.einfo[7]), int(a.einfo[8])) == (block, 1), a.einfo
    _check_lrd_einfo(c, a.einfo, 1)
    _within(f"mvf_solve_minnorm_lrd[forced block {block}]", c, a.C, _cstar(c, R))


def _lrd_einfo3_params():
    out = [(c, "cold", 0) for m in sc.LRD_M for c in sc.lrd_cases([m])]
    out += [(sc.make_case("well", m), "hinted", 0) for m in (128, 640, 641)]
    out += [(sc.make_case("well", 641), "forced", b) for b in (64, 128, 256)]
    params = []
    for c, call, b in out:
        marks = ()
        if c["rank"] >= 128:  # a factor of >= 128 columns: a deflated form answers (factor form or direct form)
            marks = pytest.mark.xfail(strict=True, raises=AssertionError, reason=(
                "the deflated forms report einfo[3] / [5] as the smallest Ritz value of their block after three applications "
                "of the inverse (mvf.h says so): it lies ABOVE the eigenvalue by 5e-7 ... 4e-4 relative on all 24 such cases "
                "(51 ... 2.3e5 eigenvalue bounds; per case in profiles/solve_kernel_edges.md), where the Jacobi path of the same "
                "entry point is within 3e-5 of the bound.  The kept rank and C, which is all the solve takes from the block, "
                "are exact / within the bound.  Not fixed here: it takes more applications in the hot path"))
        params.append(pytest.param(c, call, b, id=f"{c['id']}-{call}{b or ''}", marks=marks))
    return params


@pytest.mark.parametrize("c,call,block", _lrd_einfo3_params())
def test_lrd_smallest_kept_eigenvalue(c, call, block):
    """einfo[3] (min kept lambda) and einfo[5] (min lambda of the factor; the same number on these cases, whose factor has
    exactly the kept columns) of mvf_solve_minnorm_lrd within the eigenvalue bound C_BOUND m eps lambda_max of the designed
    value, from BOTH sides, on every form: the Jacobi path, the factor form with a 64- and a 256-vector block (cold, hinted,
    forced) and the direct form.  The Jacobi path meets it; every deflated form misses it from above and is an expected
    failure (strict: a block that converges further, or a wrong number, shows) - test_lrd_forms... sandwiches the same two
    outputs between the eigenvalue and the interlacing limit of the block on every case."""
    Gd, Kd = _operands(c)
    R = c["R"][:, :5]
    with _option("defl_block", block):
        a = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"])
        if call == "hinted":
            a = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"], rank_hint=int(a.einfo[6]), ws=a.ws)
    assert a.rc == 0 and a.info == 0 and int(a.einfo[6]) == c["rank"] == int(a.einfo[1])
    lmin = _designed(c)[1]
    r3, r5 = (a.einfo[3] - lmin) / sc.eig_bound(c), (a.einfo[5] - lmin) / sc.eig_bound(c)
    print(f"lrd {c['id']} {call} form {int(a.einfo[8])} block {int(a.einfo[7])}: (einfo[3] - lambda_min) / bound = {r3:.3g}, einfo[5]: "
          f"{r5:.3g}; relative {(a.einfo[3] - lmin) / lmin:.3g}")
    _note(f"mvf_solve_minnorm_lrd einfo[3] [form {int(a.einfo[8])}, block {int(a.einfo[7])}]", c["family"], abs(r3))
    assert abs(r3) <= 1.0 and abs(r5) <= 1.0, (c["id"], call, a.einfo[3], a.einfo[5], lmin)


# ================================================================================================== mvf_solve_minnorm_lrd_async
@pytest.mark.parametrize("m", [128, 640])
def test_lrd_async_is_the_synchronous_direct_form_bit_for_bit(m):
    """Behind an accepted synchronous call (factor form, all m columns kept) on a zeroed workspace, as the host allocates it."""
    c = sc.make_case("well", m)
    Gd, Kd = _operands(c)
    R = c["R"][:, :5]
    need = _lib().mvf_solve_minnorm_lrd_workspace_bytes(m, 5)
    ws_s, ws_a = _Ws(need, fill=0), _Ws(need, fill=0)
    s0 = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"], ws=ws_s)
    s1 = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"], rank_hint=m, ws=ws_s)
    assert int(s0.einfo[6]) == m and int(s0.einfo[8]) == 1 and int(s1.einfo[8]) == 2
    a0 = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"], ws=ws_a)
    assert _same_bits(a0.C, s0.C)
    a1 = _call("lrd_async", Gd, Kd, c["ls2"], R, rcond=c["rcond"], form_hint=int(a0.einfo[8]), ws=ws_a)
    assert a1.rc == 0 and a1.info == 0 and a1.einfo[9] == 0.0 and int(a1.einfo[8]) == 2, a1.einfo
    assert _same_bits(a1.C, s1.C) and _same_bits(a1.einfo[:10], s1.einfo[:10])
    _within("mvf_solve_minnorm_lrd_async", c, a1.C, _cstar(c, R))
    # the state it leaves is the synchronous direct form's: the next synchronous call continues from either, bit for bit
    s2 = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"], rank_hint=m, ws=ws_s)
    a2 = _call("lrd", Gd, Kd, c["ls2"], R, rcond=c["rcond"], rank_hint=m, ws=ws_a)
    assert int(s2.einfo[8]) == 2 and _same_bits(a2.C, s2.C) and _same_bits(a2.einfo[:10], s2.einfo[:10])


@pytest.mark.parametrize("m", [127, 641])
def test_lrd_async_is_refused_outside_128_to_640(m):
    c = sc.make_case("well", m)
    Gd, Kd = _operands(c)
    a = _call("lrd_async", Gd, Kd, c["ls2"], c["R"][:, :3], rcond=c["rcond"], form_hint=1,
              ws=_Ws(_lib().mvf_solve_minnorm_lrd_workspace_bytes(m, 3), fill=0))
    assert a.rc != 0 and "128 <= m <= 640" in _last_error() and a.C_untouched and np.all(a.einfo == SENTINEL)


# ================================================================================================== mvf_pinv_diag
PINV_N = [0, 1, 7, 8, 9, 257]


def _leverage_case(m, dtype):
    """The system and the longdouble reference of one (m, cell dtype): A = U^T U of 257 cells (float64 coordinates, one
    float64 eigh), leverage = sum over the kept eigenpairs of (U q)^2 / lambda with U taken at the coordinates rounded to the
    cell dtype - what the device is handed."""
    key = ("pinv", m, dtype)
    if key not in _REFS:
        pc = sc.pinv_case(257, m)
        _REFS[key] = sc.leverage_reference(pc, np.float32 if dtype == "float32" else np.float64)
    return _REFS[key]


def _pinv_bound(lc, m, dtype):
    b64 = sc.C_BOUND * m * sc.EPS * lc["kappa"]
    return b64 if dtype == "float64" else 4 * sc.FLOAT32_PINV_FLOOR[m]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("lowrank", [0, 1])
@pytest.mark.parametrize("m", [1, 127, 128, 129, 257])
def test_pinv_diag_is_the_leverage(m, lowrank, dtype):
    lib, k = _lib(), _k(dtype)
    lc = _leverage_case(m, dtype)
    pc = lc["pc"]
    Gd, Kd = _dev(lc["A"]), _dev(np.zeros((m, m)))
    a = _call("lr" if lowrank else "minnorm", Gd, Kd, 0.0, np.ones((m, 3)), rcond=pc["rcond"])
    assert a.rc == 0 and a.info == 0
    print(f"pinv_diag m {m} {dtype} lowrank {lowrank}: kept {int(a.einfo[1])} (eigh {lc['rank']}), kappa_kept {lc['kappa']:.3g}")
    assert int(a.einfo[1]) == lc["rank"]
    bound = _pinv_bound(lc, m, dtype)
    c4 = _x4(lc["ctrl"], lc["ctrl"].dtype)
    for n in PINV_N:
        x4 = _x4(lc["X"][:n], lc["X"].dtype)
        out = _Out(max(n, 1))
        torch.cuda.synchronize()
        rc = lib.mvf_pinv_diag(x4.data_ptr() if n else None, n, c4.data_ptr(), m, pc["beta"], pc["rcond"], lowrank, out.ptr, a.ws.ptr,
                               a.ws.nbytes, k.cdtype, _stream())
        torch.cuda.synchronize()
        assert rc == 0 and out.guards_intact() and a.ws.guards_intact(), (n, _last_error())
        if n == 0:
            assert out.untouched()
            continue
        d = out.host()[:n]
        assert bool((out.t[n:] == out.sent).all())
        dev = float(np.abs(d.astype(LD) - lc["ref"][:n]).max() / lc["ref"].max())
        _note(f"mvf_pinv_diag[{dtype}, lowrank {lowrank}]", f"m {m}", dev / bound)
        print(f"    n {n}: |d - ref| / max ref = {dev:.3g} (bound {bound:.3g})")
        assert dev <= bound, (n, dev, bound)
        if n == 257:  # the cells that built A: leverage scores, in [0, 1], summing to the kept rank
            assert d.min() >= -bound and d.max() <= 1 + bound
            assert abs(d.sum() - a.einfo[1]) <= 257 * bound


def test_pinv_diag_refusals():
    lib, k = _lib(), _k("float64")
    m = 129
    lc = _leverage_case(m, "float64")
    x4, c4 = _x4(lc["X"][:9], np.float64), _x4(lc["ctrl"], np.float64)
    out = _Out(9)
    # a pattern-filled workspace holds no decomposition
    ws = _Ws(lib.mvf_solve_minnorm_lr_workspace_bytes(m, 3))
    rc = lib.mvf_pinv_diag(x4.data_ptr(), 9, c4.data_ptr(), m, 0.004, 1e-10, 1, out.ptr, ws.ptr, ws.nbytes, k.cdtype, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and "no finished decomposition" in _last_error() and out.untouched()
    # a deflated decomposition does not hold every eigenpair
    c = sc.make_case("well", m)
    Gd, Kd = _operands(c)
    a = _call("lrd", Gd, Kd, c["ls2"], c["R"][:, :3], rcond=c["rcond"])
    assert a.rc == 0 and int(a.einfo[8]) == 1
    rc = lib.mvf_pinv_diag(x4.data_ptr(), 9, c4.data_ptr(), m, 0.004, 1e-10, 1, out.ptr, a.ws.ptr, a.ws.nbytes, k.cdtype, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and "deflated" in _last_error() and out.untouched() and out.guards_intact()
