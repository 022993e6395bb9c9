"""Kernel-level tests of the wide rhs / apply MFMA kernels (csrc/mvf_wide.hip: mvf_rhs_cached, mvf_apply_cached), called
through HipKernels or straight through the C ABI, against the same operation in float64 ON THE SAME BITS: the kernel-value
cache, P, Yd and Cd are read back from the device and cast to float64, so that no kernel-value error enters and kernel and
reference differ only by the order of float64 additions (plus the stated roundings to the cell dtype).

Tolerances are derived, none is fitted to an observed error.  With u64 = 2^-53, uT = 2^-24 (float32 cells) / 2^-53:
  rhs       |R - R_ref|   <= (n + 2) u64 (|U|^T |P| |Y|)                  elementwise (a sum of n products in any order;
                                                                          + 2: the rounding of U * P in float64 mode)
  apply V   |V - U C|     <= (m_pad + 1) u64 (|U| |C|) + uT |U C|         elementwise (last term: the store in the cell dtype)
  apply r   |r - r_ref|   <= ((dy + 2) u64 + nchunks uT) r_ref            r_ref from V AS READ BACK; nchunks = ceil(dy / 128)
  stats     |s - (s0 + P . r)| <= (n + 2) u64 sum(|P| r)                  r as read back; s0 = stats[0] before the call
R_ref and U C come from the float64 BLAS; r_ref and the stats reference (n dy terms: cheap) are formed in extended precision.
Every case prints its largest error / bound ratios; everything else in this file is equality of bits."""
import numpy as np
import pytest
import torch

from _kernel_scaffold import (DTYPES, bits_equal as _same_bits, called as _called, fresh_kernels as _k, under as _under,
                              watch as _watch)

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53
UT = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
NPT = {"float32": np.float32, "float64": np.float64}
SENT = -7.25  # sentinel of the "nothing is written outside the live region" tests
RATIOS = {}   # (quantity, dtype) -> largest error / bound over the cases run so far (printed with every case)


def _cdiv(a, b):
    return -(-a // b)


def _pad16(dy):
    return _cdiv(dy, 16) * 16


class Case:
    """One (cells, control points, P, Y, C) problem on the device, its cache built; buffers and leading dimensions are the
    test's own."""

    def __init__(self, dtype, n, m, dy, D=3, ldy=None, ldc=None):
        self.k = k = _k(dtype)
        self.dtype, self.n, self.m, self.dy, self.D = dtype, n, m, dy, D
        rng = np.random.default_rng([n, m, dy, D])
        # cells uniform in a box, control points drawn from the cells (no column of U is all zero); beta such that the kernel
        # values span some twenty orders of magnitude without underflowing in float32
        if D == 3:
            X = rng.uniform(-1, 1, (n, 3)) * 50.0
            self.beta = 0.002          # opposite corners: exp(-0.002 * 3e4) = 1e-26
        else:
            X = rng.uniform(-1, 1, (n, D)) * 20.0
            self.beta = 0.005          # exp(-0.005 * D * 1600) = 4e-18 at D = 5
        ctrl = X[rng.choice(n, m, replace=n < m)].copy()
        if n < m:  # more control points than cells: repeated cells, nudged apart
            ctrl += rng.uniform(-1, 1, ctrl.shape)
        c = ctrl.mean(0)
        if D == 3:
            self.x, self.c = k.to_x4(X, c), k.to_x4(ctrl, c)
            k.build_ublk(self.x, self.c, self.beta)
        else:
            self.x, self.c = k.to_xd(X, c), k.to_xd(ctrl, c)
            k.build_ublk_d(self.x, self.c, self.beta)
        self.n_pad, self.m_pad = k.wide_pads(n, m)
        self.ldy = ldy or _pad16(dy)
        self.ldc = ldc or _pad16(dy)
        npt = NPT[dtype]
        # P uniform in (0, 1) with a tenth of the cells at the floor minP = 1e-5: what the E-step produces
        P = np.maximum(rng.uniform(0.0, 1.0, n), 1e-5)
        P[rng.random(n) < 0.1] = 1e-5
        # Y and C standard normal, some columns scaled by 1e3 and 1e-3: an error in a small column cannot hide behind a large
        # one (the bounds are elementwise for this reason)
        scale = np.ones(dy)
        scale[rng.random(dy) < 0.15] = 1e3
        scale[rng.random(dy) < 0.15] = 1e-3
        if dy >= 3:
            scale[0], scale[dy // 2], scale[dy - 1] = 1e-3, 1e-3, 1e3
        Y = rng.standard_normal((n, dy)) * scale
        Cm = rng.standard_normal((m, dy)) * scale
        self.P = k.h2d(P.astype(npt))
        self.Yd = torch.zeros(self.n_pad, self.ldy, dtype=k.tdtype, device=k.device)
        self.Yd[:n, :dy] = k.h2d(Y.astype(npt))
        self.Cd = torch.zeros(self.m_pad, self.ldc, dtype=torch.float64, device=k.device)
        self.Cd[:m, :dy] = k.h2d(Cm)
        self.ws_bytes = int(k.lib.mvf_wide_workspace_bytes(n, m))
        self.ws = torch.empty(self.ws_bytes + 4096, dtype=torch.uint8, device=k.device)  # (+ a guard tail)
        torch.cuda.synchronize()

    def cache(self):
        """The cache un-blocked: Ublk[m_pad / 16][n_pad][16] -> (n_pad, m_pad)."""
        return self.k._ublk.view(self.m_pad // 16, self.n_pad, 16).permute(1, 0, 2).reshape(self.n_pad, self.m_pad)

    def check_cache(self):
        """cache == con_K bit for bit on the live part and zero in the padding: closes the chain cache -> product."""
        k, U = self.k, self.cache()
        if self.D == 3:  # mvf_con_k at d = 3 performs kernel_value's operations in kernel_value's order (mvf_conk.hip)
            K = k.con_k(self.x[:, :3].contiguous(), self.c[:, :3].contiguous(), self.beta)
        else:
            K = k.con_k(self.x, self.c, self.beta)
        torch.cuda.synchronize()
        assert _same_bits(U[: self.n, : self.m].contiguous(), K)
        assert not U[self.n:].any() and not U[:, self.m:].any()
        assert bool((K.max(0).values > 0).all())  # no column of U is all zero
        return U

    # ---- the two entry points through the C ABI: every argument under the test's control
    def rhs(self, R, *, Yd=None, dy=None, ws_bytes=None):
        from spateo_amd._kernels import _ptr

        k = self.k
        Yd = self.Yd if Yd is None else Yd
        with torch.cuda.device(k.device):
            return k.lib.mvf_rhs_cached(_ptr(k._ublk), _ptr(self.P), _ptr(Yd), self.n, self.m, self.dy if dy is None else dy,
                                        Yd.shape[1], _ptr(R), R.shape[1], _ptr(self.ws),
                                        self.ws_bytes if ws_bytes is None else ws_bytes, k.cdtype, k._stream())

    def apply(self, Vd, r, stats, *, Yd=None, Cd=None, P="own", dy=None, ws_bytes=None):
        from spateo_amd._kernels import _ptr

        k = self.k
        Yd = self.Yd if Yd is None else Yd
        Cd = self.Cd if Cd is None else Cd
        P = self.P if isinstance(P, str) else P
        assert Vd.shape[1] == Yd.shape[1]  # Vd shares Yd's leading dimension (mvf.h)
        with torch.cuda.device(k.device):
            return k.lib.mvf_apply_cached(_ptr(k._ublk), self.n, self.m, _ptr(Cd), Cd.shape[1], self.dy if dy is None else dy,
                                          _ptr(Yd), Yd.shape[1], _ptr(P), _ptr(Vd), _ptr(r), _ptr(stats), _ptr(self.ws),
                                          self.ws_bytes if ws_bytes is None else ws_bytes, k.cdtype, k._stream())

    def buffers(self, ldr=None, guard=0, ldy=None):
        """(R, Vd, r, stats), the first three filled with the sentinel: R m (+ guard) rows x ldr, Vd n (+ guard) x ldy, r n (+ guard)."""
        k = self.k
        R = torch.full((self.m + guard, ldr or self.dy), SENT, dtype=torch.float64, device=k.device)
        Vd = torch.full((self.n + guard, ldy or self.ldy), SENT, dtype=k.tdtype, device=k.device)
        r = torch.full((self.n + guard,), SENT, dtype=k.tdtype, device=k.device)
        stats = torch.zeros(1, dtype=torch.float64, device=k.device)
        return R, Vd, r, stats

    def run(self, s0=0.0, **kw):
        """Both entry points once on fresh sentinel buffers -> (R, Vd, r, stats) device tensors."""
        R, Vd, r, stats = self.buffers(**kw)
        stats.fill_(s0)
        assert self.rhs(R) == 0, self.k.lib.mvf_last_error()
        assert self.apply(Vd, r, stats) == 0, self.k.lib.mvf_last_error()
        _called()
        torch.cuda.synchronize()
        return R, Vd, r, stats


# The operands of a Case are HipKernels allocations, made and synchronised when the case is built: no displaced pointers here,
# and on the side stream the outputs, not the inputs, are in flight (a launch on another stream is overwritten by their fill).
CONVENTION_COVERS = {"mvf_rhs_cached": ("side_stream", "inputs"), "mvf_apply_cached": ("side_stream", "inputs")}


@pytest.mark.parametrize("mode", ["side_stream", "inputs"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dy", [5, 65])   # one column tile; more than one panel
def test_calling_conventions(dtype, dy, mode):
    case = Case(dtype, 300, 129, dy)

    def call():
        _watch(case.k._ublk, case.P, case.Yd, case.Cd)
        return case.run(s0=0.5)

    plain, got = _under(mode, call)
    for x, y in zip(plain, got):
        assert _same_bits(x, y)


def _ratio(name, dtype, err, bound):
    """Largest err / bound of this array (0 / 0 counts as 0); keeps the running maximum per (quantity, dtype)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    q = float(np.max(q))
    RATIOS[(name, dtype)] = max(RATIOS.get((name, dtype), 0.0), q)
    return q


def check_against_float64(case):
    """The four derived bounds of the module docstring for one case."""
    n, m, dy, dtype = case.n, case.m, case.dy, case.dtype
    uT, ld = UT[dtype], np.longdouble
    U = case.check_cache().cpu().numpy().astype(np.float64)[:n]   # n x m_pad (the padded control points: zeros)
    P = case.P.cpu().numpy().astype(np.float64)
    Y = case.Yd.cpu().numpy().astype(np.float64)[:n, :dy]
    C = case.Cd.cpu().numpy()[:, :dy]                             # m_pad x dy (rows >= m: zeros here)
    # V = U C first; then U is scaled by P in place (the large case keeps ONE float64 copy of the cache on the host)
    V_ref = U @ C
    V_abs = U @ np.abs(C)
    s0 = 0.25 * float(P @ np.sum((Y - V_ref) ** 2, 1))            # a non-zero stats[0] of the size of the sum it is added to
    R, Vd, r, stats = case.run(s0=s0)
    U *= P[:, None]
    R_ref = U.T[:m] @ Y
    R_abs = U.T[:m] @ np.abs(Y)
    del U
    out = {}
    # ---- rhs
    Rg = R.cpu().numpy()
    assert Rg.shape == (m, dy) and np.isfinite(Rg).all()
    err, bound = np.abs(Rg - R_ref), (n + 2) * U64 * R_abs
    out["rhs"] = _ratio("rhs", dtype, err, bound)
    # ---- apply: V
    Vg = Vd.cpu().numpy().astype(np.float64)[:, :dy]
    assert np.isfinite(Vg).all()
    errv, boundv = np.abs(Vg - V_ref), (case.m_pad + 1) * U64 * V_abs + uT * np.abs(V_ref)
    out["V"] = _ratio("V", dtype, errv, boundv)
    # ---- apply: r against the field as read back
    rg = r.cpu().numpy().astype(np.float64)
    r_ref = np.sum((Y.astype(ld) - Vg.astype(ld)) ** 2, 1)
    errr, boundr = np.abs(rg.astype(ld) - r_ref), ((dy + 2) * U64 + _cdiv(dy, 128) * uT) * r_ref
    out["r"] = _ratio("r", dtype, errr, boundr)
    # ---- apply: stats[0] += sum P r, with r as read back
    sg = float(stats.cpu()[0])
    pr = P.astype(ld) * rg.astype(ld)
    errs, bounds = abs(ld(sg) - (ld(s0) + pr.sum())), (n + 2) * U64 * pr.sum()
    out["stats"] = _ratio("stats", dtype, [errs], [bounds])
    print(f"wide n={n} m={m} dy={dy} D={case.D} {dtype}: error / bound  " + "  ".join(f"{q} {v:.2e}" for q, v in out.items())
          + "   | maxima so far  " + "  ".join(f"{q}/{d} {v:.2e}" for (q, d), v in sorted(RATIOS.items())))
    assert (err <= bound).all(), f"rhs: {int((err > bound).sum())} of {err.size} entries outside the bound, worst ratio {out['rhs']:.3g}"
    assert (errv <= boundv).all(), f"V: {int((errv > boundv).sum())} of {errv.size} entries outside the bound, worst ratio {out['V']:.3g}"
    assert (errr <= boundr).all(), f"r: {int((errr > boundr).sum())} of {errr.size} cells outside the bound, worst ratio {out['r']:.3g}"
    assert sg != s0 and errs <= bounds, f"stats: {sg!r} vs {float(ld(s0) + pr.sum())!r}, error / bound {out['stats']:.3g}"
    case.k.drop_ublk()


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 5000])
def test_cell_count_edges(n, dtype):
    """n below one apply workgroup, on / next to the 128-cell workgroup, the 256-cell cache padding and the 2048-cell slice:
    one slice, two slices with a single live cell in the second, three slices."""
    check_against_float64(Case(dtype, n, 150, 20))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 15, 16, 17, 127, 128, 129, 300, 1030])
def test_control_point_count_edges(m, dtype):
    """M on / next to the 16-point cache block and the 128-point row tile; three row tiles; nine (M > 1024)."""
    check_against_float64(Case(dtype, 3001, m, 20))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dy", [1, 2, 3, 4, 15, 16, 17, 32, 48, 49, 64, 65, 80, 96, 112, 113, 128, 129, 144, 150, 200, 256, 257, 300])
def test_column_count_edges(dy, dtype):
    """Each of the eight NB template instances as the only launch (Dy = 16, 32, ..., 128 and their neighbours), one, two and
    three column chunks, and several NB values in the last chunk after a full one (129, 150, 200, 300)."""
    check_against_float64(Case(dtype, 1500, 130, dy))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dy", [1, 3, 12])
def test_cache_of_the_d_dimensional_builder(dy, dtype):
    """The same kernels on the cache mvf_ublk_build_d writes (D = 5): the producer of every 4- to 8-dimensional fit."""
    check_against_float64(Case(dtype, 1500, 130, dy, D=5))


def _wide_plan(n, m, cus):
    """wide_plan of csrc/mvf_wide.hip restated: (slice_len, nslices, n_pad, workspace bytes)."""
    n_pad, m_pad = _cdiv(n, 256) * 256, _cdiv(m, 128) * 128
    want = max(1, _cdiv(4 * cus, m_pad // 128))
    sl = max(_cdiv(_cdiv(n, want), 256) * 256, 2048)
    nslices = max(1, _cdiv(n_pad, sl))
    return sl, nslices, n_pad, nslices * m_pad * 128 * 8 + _cdiv(_cdiv(n, 128) * 8, 256) * 256


def test_many_row_tiles_and_slices_longer_than_the_minimum():
    """n = 100 003, M = 3000, float32 cells: 24 row tiles, and enough cells for wide_plan to grow the slice length past its
    2048 minimum with a partial last slice (256 compute units: 40 slices of 2560 cells, the last one 256 cells long); every
    smaller case runs at exactly 2048.  The plan is recomputed from the device's compute-unit count and asserted, so that the
    case cannot silently stop covering this on a part with another count."""
    assert _wide_plan(100_003, 3000, 256)[:3] == (2560, 40, 100_096) and _wide_plan(5000, 150, 256)[:3] == (2048, 3, 5120)
    n, m = 100_003, 3000
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sl, nslices, n_pad, ws_bytes = _wide_plan(n, m, cus)
    print(f"wide_plan({n}, {m}) on {cus} compute units: slice_len {sl}, {nslices} slices, the last one {n_pad - (nslices - 1) * sl} cells")
    assert sl > 2048 and nslices >= 2 and n_pad % sl != 0
    case = Case("float32", n, m, 20)
    assert case.ws_bytes == ws_bytes  # the library planned what this test restated
    check_against_float64(case)


# ------------------------------------------------------------------------------------------------ the contract of mvf.h
CONTRACT = [(1111, 139, 21), (1111, 139, 150)]  # n, M, Dy all off their paddings; one and two column chunks


def _garbage(t, rows_from, cols_from, big):
    """t with large finite values of alternating sign in rows >= rows_from and in columns >= cols_from."""
    g = torch.full_like(t, big)
    g.view(-1)[1::2] *= -1
    if g.shape[1] % 2 == 0:
        g[1::2] *= -1  # (with an even row length every column would otherwise carry one sign)
    out = t.clone()
    out[rows_from:] = g[rows_from:]
    out[:, cols_from:] = g[:, cols_from:]
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,dy", CONTRACT)
def test_padding_values_are_inert(n, m, dy, dtype):
    """mvf.h: Yd 'zero (or any finite value) beyond row n and column dy'; C 'the padding's values only have to be finite'."""
    case = Case(dtype, n, m, dy, ldy=_pad16(dy) + 16, ldc=_pad16(dy) + 32)
    zero = case.run(s0=3.5)
    big = 1e30
    Yg, Cg = _garbage(case.Yd, n, dy, big), _garbage(case.Cd, m, dy, big)
    assert torch.equal(Yg[:n, :dy], case.Yd[:n, :dy]) and torch.equal(Cg[:m, :dy], case.Cd[:m, :dy])
    assert bool((Yg[n:].abs() > 9e29).all()) and bool((Yg[:, dy:].abs() > 9e29).all()) and bool((Yg[n:] < 0).any())
    assert bool((Cg[m:].abs() > 9e29).all()) and bool((Cg[:, dy:].abs() > 9e29).all()) and bool((Cg[:, dy:] > 0).any())
    R, Vd, r, stats = case.buffers()
    stats.fill_(3.5)
    assert case.rhs(R, Yd=Yg) == 0 and case.apply(Vd, r, stats, Yd=Yg, Cd=Cg) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(r).all()) and bool(torch.isfinite(Vd).all())
    assert _same_bits(R, zero[0])
    assert _same_bits(Vd, zero[1])  # (columns >= dy: the sentinel, both times)
    assert _same_bits(r, zero[2]) and _same_bits(stats, zero[3])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,dy", CONTRACT)
def test_nothing_is_written_outside_the_live_region(n, m, dy, dtype):
    case = Case(dtype, n, m, dy, ldy=_pad16(dy) + 16)
    case.ws.fill_(0xA5)
    before = (case.Yd.clone(), case.Cd.clone(), case.P.clone(), case.k._ublk.clone())
    R, Vd, r, stats = case.run(s0=1.0, ldr=dy + 5, guard=37)
    assert bool((R[:m, :dy] != SENT).all()) and bool((R[:, dy:] == SENT).all()) and bool((R[m:] == SENT).all())
    assert bool((Vd[:n, :dy] != SENT).all()) and bool((Vd[:, dy:] == SENT).all()) and bool((Vd[n:] == SENT).all())
    assert bool((r[:n] != SENT).all()) and bool((r[n:] == SENT).all())
    assert bool((case.ws[case.ws_bytes:] == 0xA5).all())  # the workspace is used within mvf_wide_workspace_bytes
    for a, b in zip(before, (case.Yd, case.Cd, case.P, case.k._ublk)):  # the inputs are inputs
        assert _same_bits(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,dy", CONTRACT)
def test_leading_dimensions_larger_than_needed(n, m, dy, dtype):
    """ldy = 64 at Dy = 21 (and ldc, ldr above their minima): the same bits as the tight layout."""
    tight = Case(dtype, n, m, dy)
    loose = Case(dtype, n, m, dy, ldy=_pad16(dy) + 32, ldc=_pad16(dy) + 48)
    assert loose.ldy == (64 if dy == 21 else 192) and tight.ldy == _pad16(dy)
    assert torch.equal(tight.Yd[:, :dy], loose.Yd[:, :dy]) and torch.equal(tight.Cd[:, :dy], loose.Cd[:, :dy])
    a = tight.run(s0=2.0)
    b = loose.run(s0=2.0, ldr=dy + 11)
    assert _same_bits(a[0], b[0][:, :dy].contiguous())
    assert _same_bits(a[1][:, :dy].contiguous(), b[1][:, :dy].contiguous())
    assert _same_bits(a[2], b[2]) and _same_bits(a[3], b[3])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,dy", CONTRACT)
def test_apply_without_p_and_stats_accumulates(n, m, dy, dtype):
    """P = NULL: V and r as with P, stats untouched (stats may then be NULL too).  With P: stats[0] +=, so two calls add twice."""
    case = Case(dtype, n, m, dy)
    _, V0, r0, s0 = case.run(s0=0.0)
    _, Vd, r, stats = case.buffers()
    stats.fill_(SENT)
    assert case.apply(Vd, r, stats, P=None) == 0
    torch.cuda.synchronize()
    assert _same_bits(Vd, V0) and _same_bits(r, r0) and float(stats[0]) == SENT
    _, Vd, r, _ = case.buffers()
    assert case.apply(Vd, r, None, P=None) == 0
    torch.cuda.synchronize()
    assert _same_bits(Vd, V0) and _same_bits(r, r0)
    acc = torch.zeros(1, dtype=torch.float64, device=case.k.device)
    assert case.apply(Vd, r, acc) == 0 and case.apply(Vd, r, acc) == 0
    torch.cuda.synchronize()
    t = float(s0[0])
    assert t > 0 and float(acc[0]) == t + t


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,dy", CONTRACT)
def test_two_calls_give_the_same_bits(n, m, dy, dtype):
    case = Case(dtype, n, m, dy)
    a, b = case.run(s0=0.5), case.run(s0=0.5)
    for x, y in zip(a, b):
        assert _same_bits(x, y)
    # ... and so do the HipKernels wrappers the engine calls (their own workspace)
    k = case.k
    R, Vd, r, stats = case.buffers()
    stats.fill_(0.5)
    k.rhs_wide(case.P, case.Yd, dy, m, R)
    k.apply_wide(case.Cd, dy, m, case.Yd, case.P, Vd, r, stats)
    torch.cuda.synchronize()
    for x, y in zip(a, (R, Vd, r, stats)):
        assert _same_bits(x, y)


@pytest.mark.parametrize("dtype", DTYPES)
def test_columns_do_not_depend_on_their_neighbours(dtype):
    """R[:, d] and V[:, d] of the Dy = 150 call carry the bits of column 0 of a Dy = 1 call that is given column d alone: each
    MFMA output element sees the same additions in the same order whatever NB is and whichever column chunk it sits in.  This
    pins the second chunk (col0 = 128) and the NB instances against each other."""
    n, m, dy = 1500, 130, 150
    case = Case(dtype, n, m, dy)
    R, Vd, r, stats = case.run()
    Y1 = torch.zeros(case.n_pad, 16, dtype=case.k.tdtype, device=case.k.device)
    C1 = torch.zeros(case.m_pad, 16, dtype=torch.float64, device=case.k.device)
    for d in (0, 1, 15, 16, 17, 100, 127, 128, 129, 143, 144, 149):
        Y1[:n, 0] = case.Yd[:n, d]
        C1[:m, 0] = case.Cd[:m, d]
        R1, V1, r1, st1 = case.buffers(ldr=1, ldy=16)
        assert case.rhs(R1, Yd=Y1, dy=1) == 0 and case.apply(V1, r1, st1, Yd=Y1, Cd=C1, dy=1) == 0
        torch.cuda.synchronize()
        assert _same_bits(R1[:, 0].contiguous(), R[:, d].contiguous()), f"rhs column {d}"
        assert _same_bits(V1[:, 0].contiguous(), Vd[:, d].contiguous()), f"apply column {d}"


# ------------------------------------------------------------------------------------------------ refusals, on real buffers
@pytest.mark.parametrize("dtype", DTYPES)
def test_refused_calls_launch_nothing(dtype):
    """The refusals of tests/test_abi.py with REAL device buffers behind the pointers: status != 0, the message names the
    entry point, and no output byte changes; the accepted call still works afterwards."""
    n, m, dy = 700, 139, 21
    case = Case(dtype, n, m, dy)
    k, lib = case.k, case.k.lib
    R, Vd, r, stats = case.buffers()
    stats.fill_(SENT)

    def untouched():
        torch.cuda.synchronize()
        return bool((R == SENT).all()) and bool((Vd == SENT).all()) and bool((r == SENT).all()) and float(stats[0]) == SENT

    narrow = torch.zeros(case.n_pad, 16, dtype=k.tdtype, device=k.device)  # ldy = 16 < 32 = dy padded to 16
    Vn = torch.full((n, 16), SENT, dtype=k.tdtype, device=k.device)
    assert case.rhs(R, Yd=narrow) != 0 and b"mvf_rhs_cached" in lib.mvf_last_error()
    assert case.apply(Vn, r, stats, Yd=narrow) != 0 and b"mvf_apply_cached" in lib.mvf_last_error()
    assert untouched() and bool((Vn == SENT).all())
    Rn = torch.full((m, dy - 1), SENT, dtype=torch.float64, device=k.device)  # ldr < dy
    assert case.rhs(Rn) != 0 and b"mvf_rhs_cached" in lib.mvf_last_error()
    Cn = torch.zeros(case.m_pad, 16, dtype=torch.float64, device=k.device)  # ldc < dy padded to 16
    assert case.apply(Vd, r, stats, Cd=Cn) != 0 and b"mvf_apply_cached" in lib.mvf_last_error()
    assert case.rhs(R, ws_bytes=case.ws_bytes - 1) != 0 and b"mvf_rhs_cached: workspace too small" in lib.mvf_last_error()
    assert case.apply(Vd, r, stats, ws_bytes=case.ws_bytes - 1) != 0
    assert b"mvf_apply_cached: workspace too small" in lib.mvf_last_error()
    assert case.rhs(R, dy=0) != 0 and b"mvf_rhs_cached" in lib.mvf_last_error()
    assert case.apply(Vd, r, stats, dy=0) != 0 and b"mvf_apply_cached" in lib.mvf_last_error()
    assert case.apply(Vd, r, None) != 0 and b"mvf_apply_cached: P given but stats is null" in lib.mvf_last_error()
    for nn, mm in ((0, m), (n, 0)):
        case.n, case.m = nn, mm
        assert case.rhs(R) != 0 and b"mvf_rhs_cached" in lib.mvf_last_error()
        assert case.apply(Vd, r, stats) != 0 and b"mvf_apply_cached" in lib.mvf_last_error()
    case.n, case.m = n, m
    cd, k.cdtype = k.cdtype, 7
    assert case.rhs(R) != 0 and b"mvf_rhs_cached: bad dtype" in lib.mvf_last_error()
    assert case.apply(Vd, r, stats) != 0 and b"mvf_apply_cached: bad dtype" in lib.mvf_last_error()
    k.cdtype = cd
    assert untouched() and bool((Rn == SENT).all())
    assert case.rhs(R) == 0 and case.apply(Vd, r, stats) == 0
    torch.cuda.synchronize()
    assert bool((R != SENT).all()) and bool((r != SENT).all())
