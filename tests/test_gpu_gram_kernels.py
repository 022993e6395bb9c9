"""Kernel-level edge tests of csrc/mvf_gram.hip: the tile kernels (gram_f64acc_kernel, gram_cached_kernel,
gram_cached_kernel_shared_cols), ublk_build_kernel, widen_p_kernel, rhs_kernel and the two deterministic reductions, with the
launch plan's slices and phases - on ``cuda:0`` in both cell dtypes and on every path (recompute, cached, in float32 also the
register-operand kernel behind the developer option "gram_reg_cols").

The references are np.longdouble sums over the kernel values THE DEVICE PRODUCED (the cache, asserted equal to mvf_con_k bit
for bit and zero in every padded row and column), so the per-element bound is the summation bound (n + 2) 2^-53 of
tests/_gram_cases.py in BOTH cell dtypes, relative to each element's own sum of absolute terms - not a data-type tolerance
relative to the largest entry.  tests/test_gram_kernel_refs.py proves without a GPU that a correct summation order stays
within that bound and that each targeted defect leaves it by >= 100 x.

Everything else is exact: all paths bit-equal to each other, G == G^T, repeated calls, a NaN-filled workspace between calls
(the reductions read no word the tile kernels skip), stage masks, the raw ABI inside sentinel buffers, refusals.  Run with
``-s`` for the largest |deviation| / bound per case family (profiles/gram_kernel_edges.md records them)."""
import numpy as np
import pytest
import torch

import _gram_cases as gc
from _kernel_scaffold import (DEV, DTYPES, MODES, SENTINEL as _SENTINEL, WS_FILL, bits_equal as _bits_equal, called as _called,
                              dev as _dev, deviation_table, guarded as _guarded, intact as _intact, kernel_cache,
                              option as _option, Out as _Out, same_bits as _same_bits, settle as _settle, take as _take,
                              under as _under, Ws as _Ws, x4 as _sx4)

pytestmark = pytest.mark.gpu

SENTINEL = _SENTINEL[torch.float64]  # what an untouched G or R holds
TILES, RHS, REDUCE, REDUCE_RHS = 1, 2, 4, 8
ALL = 15
_COUNT = [0]
_k = kernel_cache()


def _drop_caches():
    for k in _k.cache.values():
        k.drop_ublk()
        k._gram_ws = None


_note, _deviation_table = deviation_table(
    "| case family | dtype | quantity | largest |deviation| / bound |", columns=4, on_done=_drop_caches,
    footer=lambda seconds, notes: f"test_gpu_gram_kernels: {seconds:.1f} s, {_COUNT[0]} reference comparisons")


def _x4(k, a, center):
    a = np.asarray(a, dtype=np.float64)
    return k.to_x4(a, center) if len(a) else torch.zeros(0, 4, dtype=k.tdtype, device=DEV)


def _device_case(k, c):
    inp = gc.inputs(c["n"], c["m"], c["p_kind"])
    P = torch.from_numpy(inp["P"]).to(k.tdtype).to(DEV)
    return _x4(k, inp["X"], inp["center"]), _x4(k, inp["ctrl"], inp["center"]), _x4(k, inp["Y"], None), P


def _gr(m):
    return _Out(m, m).t, _Out(m, 3).t


def _paths(dtype):
    return ["recompute", "cached"] + (["reg_cols"] if dtype == "float32" else [])


def _gram(k, path, x4, P, y4, c4, beta, **kw):
    """G, R of one path.  The cached paths need k.build_ublk(x4, c4, beta) first; "recompute" leaves the cache alone by handing
    the call a key that does not match (the cache stays for the next cached call)."""
    m = c4.shape[0]
    G, R = _gr(m)
    if path == "recompute":
        ublk, key = k._ublk, k._ublk_key
        k._ublk, k._ublk_key = None, None
        try:
            k.gram(x4, P, y4, c4, beta, G, R, **kw)
        finally:
            k._ublk, k._ublk_key = ublk, key
    else:
        with _option("gram_reg_cols", 1 if path == "reg_cols" else 0):
            k.gram(x4, P, y4, c4, beta, G, R, cache_only=True, **kw)
    return G, R


def _all_paths(k, dtype, x4, P, y4, c4, beta):
    """Every path twice: all bit-equal, G exactly symmetric.  Returns G, R."""
    k.build_ublk(x4, c4, beta)
    G0 = R0 = None
    for path in _paths(dtype):
        for _ in range(2):
            G, R = _gram(k, path, x4, P, y4, c4, beta)
            if G0 is None:
                G0, R0 = G, R
            assert _bits_equal(G, G0) and _bits_equal(R, R0), path
    assert _bits_equal(G0, G0.T.contiguous())
    return G0, R0


def _decoded_cache(k, dtype, x4, c4, beta):
    """The device's kernel values U (n x m, cell dtype) from the cache Ublk[m_pad / 16][n_pad][16] of build_ublk, after the
    exact checks: mvf_con_k's bits, every padded row and column 0, and a raw build into a buffer of exactly mvf_ublk_bytes
    writes the same bits and nothing behind them."""
    n, m = x4.shape[0], c4.shape[0]
    n_pad, m_pad = gc.pads(n, m)
    item = 4 if dtype == "float32" else 8
    need = k.ublk_bytes(n, m)
    assert need == n_pad * m_pad * item and k._ublk.numel() == n_pad * m_pad
    U = k._ublk.view(m_pad // gc.UB, n_pad, gc.UB).permute(1, 0, 2).reshape(n_pad, m_pad)
    assert not U[n:].any() and not U[:, m:].any()
    K = k.con_k(x4[:, :3].contiguous(), c4[:, :3].contiguous(), beta)
    live = U[:n, :m].contiguous()
    assert _bits_equal(live, K)
    buf = _guarded(n_pad * m_pad, k.tdtype)
    torch.cuda.synchronize()
    rc = k.lib.mvf_ublk_build(x4.data_ptr(), n, c4.data_ptr(), m, float(beta), buf.data_ptr(), need, k.cdtype, k._stream())
    torch.cuda.synchronize()
    assert rc == 0 and _intact(buf, n_pad * m_pad) and _bits_equal(buf[:n_pad * m_pad], k._ublk)
    return live


def _compare_full(c, dtype, U, P, y4, G, R):
    """G and R against the longdouble references within the bound, per element."""
    n = c["n"]
    Uh, Ph, yh = U.cpu().numpy(), P.cpu().numpy(), y4.cpu().numpy()[:, :3]
    W = gc.rhs_weights(yh, Ph)
    G_ref = gc.gram_reference(Uh, Ph)
    R_ref, S = gc.rhs_reference(Uh, W)
    rg = gc.ratio(G.cpu().numpy(), G_ref, gc.bound(G_ref, n))
    rr = gc.ratio(R.cpu().numpy(), R_ref, gc.bound(S, n))
    _COUNT[0] += 1
    print(f"gram {gc.case_id(c)} {dtype}: |dG| / bound = {rg:.3g}, |dR| / bound = {rr:.3g}")
    _note(c["family"], dtype, "G", rg)
    _note(c["family"], dtype, "R", rr)
    assert rg <= 1.0 and rr <= 1.0, (rg, rr)
    return G_ref, R_ref


def _check_case(c, dtype):
    k = _k(dtype)
    n, m = c["n"], c["m"]
    x4, c4, y4, P = _device_case(k, c)
    with _option("slice_len", c["slice_len"]):
        if c["slice_len"]:
            p = gc.forced_plan(n, m, dtype, c["slice_len"])
            assert p["nphases"] == 1 and p["nslices"] == gc.cdiv(n, c["slice_len"])
            assert k.lib.mvf_gram_workspace_bytes(n, m, k.cdtype) == \
                gc.align_up(p["gram_bytes"]) + gc.align_up(p["rhs_bytes"]) + p["widened_p_bytes"]
        G, R = _all_paths(k, dtype, x4, P, y4, c4, c["beta"])
    U = _decoded_cache(k, dtype, x4, c4, c["beta"])
    G_ref, R_ref = _compare_full(c, dtype, U, P, y4, G, R)
    k.drop_ublk()
    return G, R, U


# ------------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", gc.M_CASES, ids=gc.case_id)
def test_control_point_edges(c, dtype):
    """m across one cached block and its padding, the 64-column edge threshold, one / two / three / four tiles with the
    edge2 pairings, the second rhs column block and the second ublk_build workgroup column."""
    _check_case(c, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", gc.N_CASES, ids=gc.case_id)
def test_cell_edges(c, dtype):
    """n across the k-step of 4 cells, the superblock of both dtypes (ng_main and the clamped remainder loop), the LDS stage
    and the padded last slice."""
    _check_case(c, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", gc.SLICE_CASES, ids=gc.case_id)
def test_gram_slices_on_the_eight_way_interleave(c, dtype):
    """7, 8, 9, 16, 17 slices of 256 cells, the last with one live cell: gram_reduce_kernel's unrolled rounds and its tail."""
    _check_case(c, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", gc.RHS_SLICE_CASES, ids=gc.case_id)
def test_rhs_slices_on_the_sixteen_lanes(c, dtype):
    """15, 16, 17 and 33 rhs slices on the 16 slice lanes of rhs_reduce_kernel; 17 control points: a second workgroup with one."""
    assert gc.rhs_plan(c["n"], c["m"])[0] == gc.GCHUNK
    _check_case(c, dtype)


# ------------------------------------------------------------------------------------------------------ P
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", gc.P_CASES, ids=gc.case_id)
def test_p_all_zero_all_one_with_holes_and_at_the_floor(c, dtype):
    G, R, _ = _check_case(c, dtype)
    if c["p_kind"] == "zero":
        assert not G.any() and not R.any()
    else:
        assert bool((G.diagonal() > 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_values_that_underflow(dtype):
    """beta = 0.05: the exact float32 kernel values reach the denormal range and 0 (census of IEEE arithmetic in
    tests/test_gram_kernel_refs.py); in float64 mode products of two kernel values underflow.  G finite, diagonal > 0, within
    the bound (with its absolute term).  The census of the DEVICE's own float32 values is printed and its normal and zero
    counts asserted: kernel_value's exp2 (v_exp_f32) returns 0 below the normal range - 0 denormal values measured where IEEE
    arithmetic has thousands - in every kernel alike (the cache holds mvf_con_k's bits), so the operands this case feeds the
    tile kernels are normal values down to 2^-126 and exact zeros."""
    G, R, U = _check_case(gc.UNDERFLOW, dtype)
    assert bool(torch.isfinite(G).all()) and bool(torch.isfinite(R).all()) and float(G.diagonal().min()) > 0
    if dtype == "float32":
        normal, denormal, zero = gc.census(U.cpu().numpy())
        print(f"float32 kernel values on the device: {normal} normal, {denormal} denormal, {zero} zero")
        assert normal > 1000 and zero > 1000


# ------------------------------------------------------------------------------------------------------ three phases
@pytest.mark.parametrize("dtype", DTYPES)
def test_three_phases_against_the_sampled_reference(dtype):
    """299 slices of 256 cells x 153 tile pairs against a buffer of 149 slices: phases of 100, 100 and 99 slices, the last slice
    with one live cell.  The in-stage fold with accumulate = 1, in float32 the widened-P pointer biased by - c0 in a middle
    phase, edge2 with nt = 17."""
    c = gc.PHASE
    k = _k(dtype)
    n, m = c["n"], c["m"]
    x4, c4, y4, P = _device_case(k, c)
    with _option("slice_len", c["slice_len"]):
        p = gc.forced_plan(n, m, dtype, c["slice_len"])
        assert (p["nslices"], p["npairs"], p["fit"], p["nphases"], p["phase_slices"]) == (299, 153, 149, 3, 100)
        ws = k.lib.mvf_gram_workspace_bytes(n, m, k.cdtype)
        assert ws - gc.align_up(p["rhs_bytes"]) - p["widened_p_bytes"] == 100 * 153 * 128 * 128 * 8
        G, R = _all_paths(k, dtype, x4, P, y4, c4, c["beta"])
    U = _decoded_cache(k, dtype, x4, c4, c["beta"])
    Uh, Ph, yh = U.cpu().numpy(), P.cpu().numpy(), y4.cpu().numpy()[:, :3]
    k.drop_ublk()
    Gh, Rh = G.cpu().numpy(), R.cpu().numpy()
    U64 = Uh.astype(np.float64, copy=False)  # (exact)
    rows = gc.sample_rows(m)
    ref = gc.gram_rows_blas(U64, Ph, rows)
    rg = gc.ratio(Gh[rows], ref, gc.bound(ref, n))  # in units of the bound; asserted at 2 (reference + kernel)
    el = gc.sample_elements(m)
    exact = np.array([gc.gram_element_exact(U64[:, i], U64[:, j], Ph) for i, j in el])
    re = gc.ratio(np.array([Gh[i, j] for i, j in el]), exact, gc.bound(exact, n))
    W64 = gc.rhs_weights(yh, Ph).astype(np.float64)
    R_ref, S = U64.T @ W64, U64.T @ np.abs(W64)
    rr = gc.ratio(Rh, R_ref, gc.bound(S, n))
    _COUNT[0] += 1
    print(f"gram {gc.case_id(c)} {dtype}: 40 rows |dG| / bound = {rg:.3g} (of 2), 64 exact elements {re:.3g}, "
          f"|dR| / bound = {rr:.3g} (of 2)")
    _note(c["family"] + " (40 rows, BLAS; asserted at 2)", dtype, "G", rg)
    _note(c["family"] + " (64 elements, fsum)", dtype, "G", re)
    _note(c["family"] + " (BLAS; asserted at 2)", dtype, "R", rr)
    assert rg <= 2.0 and re <= 1.0 and rr <= 2.0, (rg, re, rr)


# ------------------------------------------------------------------------------------------------------ dead work
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", gc.DEAD_MS)
def test_the_reductions_read_no_word_the_tile_kernels_skip(dtype, m):
    """NaN in every byte of the workspace between two calls: the blocks below the diagonal, the dead half of narrow
    last-column tiles and the padded columns are not written by the cached kernels - and must not be read."""
    c = gc.case("dead work", gc.DEAD_N, m)
    k = _k(dtype)
    x4, c4, y4, P = _device_case(k, c)
    k.build_ublk(x4, c4, c["beta"])
    for path in _paths(dtype):
        G1, R1 = _gram(k, path, x4, P, y4, c4, c["beta"])
        torch.cuda.synchronize()
        k._gram_ws.fill_(255)
        assert bool(torch.isnan(k._gram_ws[: k._gram_ws.numel() // 8 * 8].view(torch.float64)).all())
        G2, R2 = _gram(k, path, x4, P, y4, c4, c["beta"])
        assert _bits_equal(G1, G2) and _bits_equal(R1, R2), path
        assert bool(torch.isfinite(G2).all()) and bool(torch.isfinite(R2).all())
    k.drop_ublk()


# ------------------------------------------------------------------------------------------------------ stages, raw ABI
def _raw(k, stages, x4, P, y4, c4, beta, G, R, ws, ws_bytes, ublk=None, n=None, m=None, cached=None, sync=True):
    """mvf_gram_stages, or mvf_gram_cached when a cache is given, through the raw ABI (pointers as integers or None)."""
    n = x4.shape[0] if n is None else n
    m = c4.shape[0] if m is None else m
    args = (x4.data_ptr(), P.data_ptr(), y4.data_ptr() if y4 is not None else None, n, c4.data_ptr(), m, float(beta), G, R, ws,
            ws_bytes, k.cdtype, k._stream())
    _settle()
    if cached if cached is not None else ublk is not None:
        rc = k.lib.mvf_gram_cached(stages, ublk, *args)
    else:
        rc = k.lib.mvf_gram_stages(stages, *args)
    _called()
    if sync:
        torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------------ calling conventions
CONVENTION_COVERS = {"mvf_gram": MODES, "mvf_gram_stages": MODES, "mvf_ublk_build": MODES, "mvf_gram_cached": MODES}
# float32: the sharing kernel as the dispatcher launches it, with persistent workgroups, and the kernel without sharing
GRAM_VARIANTS = [("float32", 0), ("float32", 3), ("float32", 1), ("float64", 0)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype,reg_cols", GRAM_VARIANTS)
def test_calling_conventions(dtype, reg_cols, mode):
    """mvf_ublk_build, then G and R from mvf_gram, mvf_gram_stages and mvf_gram_cached on inputs, outputs, a cache and
    workspaces of the scaffold's own: the plain calls' bits on a side stream behind poisoned inputs, at displaced pointers
    (coordinates one row, P one element, the cache 16 bytes - what include/mvf.h asks of it at mvf_ublk_pack -, workspaces 256
    bytes), and with the inputs unchanged."""
    n, m = 300, 129
    c, k = gc.case("raw", n, m), _k(dtype)
    inp = gc.inputs(n, m, c["p_kind"])
    centre = np.asarray(inp["center"], dtype=np.float64)[None, :3]
    item = 4 if dtype == "float32" else 8
    need, nb = int(k.lib.mvf_gram_workspace_bytes(n, m, k.cdtype)), int(k.lib.mvf_ublk_bytes(n, m, k.cdtype))

    def call():
        x4, c4, y4 = _sx4(inp["X"] - centre, dtype), _sx4(inp["ctrl"] - centre, dtype), _sx4(inp["Y"], dtype)
        P = _dev(inp["P"], k.tdtype)
        ublk = _guarded(nb // item, k.tdtype, unit=16 // item)
        rc = k.lib.mvf_ublk_build(x4.data_ptr(), n, c4.data_ptr(), m, float(c["beta"]), ublk.data_ptr(), nb, k.cdtype, k._stream())
        _called()
        assert rc == 0, k.lib.mvf_last_error()
        bufs = [(_Out(m, m), _Out(m, 3), _Ws(need)) for _ in range(3)]
        for entry, (G, R, ws) in zip(("gram", "stages", "cached"), bufs):   # (no synchronisation between the four calls)
            if entry == "gram":
                rc = k.lib.mvf_gram(x4.data_ptr(), P.data_ptr(), y4.data_ptr(), n, c4.data_ptr(), m, float(c["beta"]), G.ptr, R.ptr,
                                    ws.ptr, need, k.cdtype, k._stream())
                _called()
            else:
                rc = _raw(k, ALL, x4, P, y4, c4, c["beta"], G.ptr, R.ptr, ws.ptr, need, ublk.data_ptr() if entry == "cached" else None,
                          sync=False)
            assert rc == 0, (entry, k.lib.mvf_last_error())
        torch.cuda.synchronize()
        outs = []
        for G, R, ws in bufs:
            assert G.guards_intact() and R.guards_intact() and ws.guards_intact()
            outs += [G.host(), R.host()]
        assert _same_bits(outs[0], outs[2]) and _same_bits(outs[2], outs[4]) and _same_bits(outs[1], outs[5])
        return outs + [_take(ublk, nb // item)]

    with _option("gram_reg_cols", reg_cols):
        plain, got = _under(mode, call)
    assert all(_same_bits(a, b) for a, b in zip(plain, got))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", [(300, 129), (513, 193)])
def test_stage_masks(dtype, n, m):
    """TILES, later REDUCE, later RHS | REDUCE_RHS as three calls give the bits of one call; tiles_only leaves R alone and
    rhs_only leaves G alone."""
    c = gc.case("stages", n, m)
    k = _k(dtype)
    x4, c4, y4, P = _device_case(k, c)
    k.build_ublk(x4, c4, c["beta"])
    for path in ("recompute", "cached"):
        G1, R1 = _gram(k, path, x4, P, y4, c4, c["beta"])
        ublk = k._ublk.data_ptr() if path == "cached" else None
        ws, nb = k._gram_ws.data_ptr(), k._gram_ws.numel()
        G2, R2 = _gr(m)
        for stages in (TILES, REDUCE, RHS | REDUCE_RHS):
            assert _raw(k, stages, x4, P, y4, c4, c["beta"], G2.data_ptr(), R2.data_ptr(), ws, nb, ublk) == 0
            if stages == TILES:
                assert bool((G2 == SENTINEL).all()) and bool((R2 == SENTINEL).all())
            if stages == REDUCE:
                assert _bits_equal(G1, G2) and bool((R2 == SENTINEL).all())
        assert _bits_equal(G1, G2) and _bits_equal(R1, R2), path
        Gt, Rt = _gram(k, path, x4, P, y4, c4, c["beta"], tiles_only=True)
        assert _bits_equal(Gt, G1) and bool((Rt == SENTINEL).all()), path
        Gr, Rr = _gram(k, path, x4, P, y4, c4, c["beta"], rhs_only=True)
        assert _bits_equal(Rr, R1) and bool((Gr == SENTINEL).all()), path
    k.drop_ublk()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", [(300, 129), (257, 193), (513, 440)])
def test_raw_abi_writes_nothing_outside_its_buffers(dtype, n, m):
    """G, R and the workspace at exactly m x m, m x 3 and mvf_gram_workspace_bytes inside larger sentinel buffers."""
    c = gc.case("raw", n, m)
    k = _k(dtype)
    x4, c4, y4, P = _device_case(k, c)
    k.build_ublk(x4, c4, c["beta"])
    need = int(k.lib.mvf_gram_workspace_bytes(n, m, k.cdtype))
    for path in ("recompute", "cached"):
        G1, R1 = _gram(k, path, x4, P, y4, c4, c["beta"])
        Gb, Rb = _Out(m * m), _Out(m * 3)
        wsb = _Ws(need)
        assert wsb.ptr % 256 == 0
        rc = _raw(k, ALL, x4, P, y4, c4, c["beta"], Gb.ptr, Rb.ptr, wsb.ptr, need,
                  k._ublk.data_ptr() if path == "cached" else None)
        assert rc == 0, path
        assert Gb.guards_intact() and Rb.guards_intact(), path
        assert wsb.guards_intact(), path
        assert _bits_equal(Gb.t.view(m, m), G1) and _bits_equal(Rb.t.view(m, 3), R1), path
    k.drop_ublk()


@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_shapes(dtype):
    """n = 0 writes exact zeros into G and R (and nothing around them); m = 0 returns 0 and writes nothing."""
    n, m = 300, 129
    c = gc.case("degenerate", n, m)
    k = _k(dtype)
    x4, c4, y4, P = _device_case(k, c)
    ws = _Ws(k.lib.mvf_gram_workspace_bytes(n, m, k.cdtype))
    Gb, Rb = _Out(m * m), _Out(m * 3)
    rc = _raw(k, ALL, x4, P, y4, c4, c["beta"], Gb.ptr, Rb.ptr, ws.ptr, ws.nbytes, n=0)
    assert rc == 0 and Gb.guards_intact() and Rb.guards_intact()
    assert not Gb.t.any() and not Rb.t.any()
    assert bool((ws.big == WS_FILL).all())
    Gb, Rb = _Out(m * m), _Out(m * 3)
    rc = _raw(k, ALL, x4, P, y4, c4, c["beta"], Gb.ptr, Rb.ptr, ws.ptr, ws.nbytes, m=0)
    assert rc == 0 and bool((Gb.big == SENTINEL).all()) and bool((Rb.big == SENTINEL).all()) and bool((ws.big == WS_FILL).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_the_outputs_untouched(dtype):
    n, m = 300, 129
    c = gc.case("refusals", n, m)
    k = _k(dtype)
    x4, c4, y4, P = _device_case(k, c)
    beta = c["beta"]
    k.build_ublk(x4, c4, beta)
    ublk = k._ublk.data_ptr()
    need = int(k.lib.mvf_gram_workspace_bytes(n, m, k.cdtype))
    # what the recompute path itself needs: the widened P behind the partials belongs to the float32 cached tile stage
    need_stages = need - (gc.align_up(8 * gc.pads(n, m)[0]) if dtype == "float32" else 0)
    ws = _Ws(need)
    G, R = _gr(m)
    g, r, w = G.data_ptr(), R.data_ptr(), ws.ptr
    calls = {
        "beta < 0": dict(beta=-beta), "beta = inf": dict(beta=float("inf")),
        "beta < 0, cached": dict(beta=-beta, ublk=ublk), "beta = inf, cached": dict(beta=float("inf"), ublk=ublk),
        "stage mask 0": dict(stages=0), "stage mask 16": dict(stages=16),
        "stage mask 0, cached": dict(stages=0, ublk=ublk), "stage mask 16, cached": dict(stages=16, ublk=ublk),
        "workspace one byte short": dict(ws_bytes=need_stages - 1),
        "workspace one byte short, cached": dict(ws_bytes=need - 1, ublk=ublk),
        "REDUCE with a null G": dict(G=None), "REDUCE with a null G, cached": dict(G=None, ublk=ublk),
        "mvf_gram_cached with n = 0": dict(n=0, ublk=ublk),
    }
    for name, kw in calls.items():
        rc = _raw(k, kw.get("stages", ALL), x4, P, y4, c4, kw.get("beta", beta), kw.get("G", g), r, w, kw.get("ws_bytes", need),
                  kw.get("ublk"), n=kw.get("n"))
        assert rc != 0, name
        assert bool((G == SENTINEL).all()) and bool((R == SENTINEL).all()), name
    # (the same buffers pass where nothing is wrong: the recompute path with exactly what it needs, the cached one likewise)
    assert _raw(k, ALL, x4, P, y4, c4, beta, g, r, w, need_stages) == 0
    G1, R1 = G.clone(), R.clone()
    assert bool((G1 != SENTINEL).all()) and bool((R1 != SENTINEL).all())
    assert _raw(k, ALL, x4, P, y4, c4, beta, g, r, w, need, ublk) == 0
    assert _bits_equal(G, G1) and _bits_equal(R, R1)
    k.drop_ublk()
    # mvf_ublk_build
    n_pad, m_pad = gc.pads(n, m)
    bytes_ = k.ublk_bytes(n, m)
    builds = {"n = 0": dict(n=0), "m = 0": dict(m=0), "beta < 0": dict(beta=-beta), "beta = inf": dict(beta=float("inf")),
              "cache buffer one byte short": dict(short=1)}
    for name, kw in builds.items():
        buf = _guarded(n_pad * m_pad, k.tdtype)
        torch.cuda.synchronize()
        rc = k.lib.mvf_ublk_build(x4.data_ptr(), kw.get("n", n), c4.data_ptr(), kw.get("m", m), float(kw.get("beta", beta)),
                                  buf.data_ptr(), bytes_ - kw.get("short", 0), k.cdtype, k._stream())
        torch.cuda.synchronize()
        assert rc != 0, name
        assert _intact(buf, 0), name
