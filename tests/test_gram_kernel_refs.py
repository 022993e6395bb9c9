"""No GPU: the references, the bound and the case tables of tests/test_gpu_gram_kernels.py (tests/_gram_cases.py builds them
for both modules), on kernel values made on the host by the kernels' recipe in the cell dtype.

  * a float64 emulation of the kernels' summation order (k-steps of 4 cells chained per slice, slices folded eight-way
    interleaved then pairwise, rhs slices on 16 lanes) stays within the derived bound (n + 2) 2^-53 of the np.longdouble
    reference, for every small case in both cell dtypes - the bound is reachable by a correct kernel;
  * mutation sensitivity: a dropped last cell, a dropped k-step, a dropped slice, a transposed off-diagonal tile, a padded
    control point that is not masked, the last live column taken from its neighbour, P rounded to float32 in float64 mode,
    rhs weights not rounded to float32 in float32 mode, a reduction that skips slice 8 - each moves a compared element by
    >= 100 x the bound in every case it applies to, and each applies where the tables say it does;
  * the sampled reference of the three-phase case: its rows and elements lie where they have to, math.fsum on Dekker pieces
    is the longdouble sum, float64 BLAS rows are within their 2 x;
  * the float32 underflow case holds > 1000 normal, > 1000 denormal and > 1000 zero kernel values;
  * coverage: from the mirrored constants of mvf_gram.hip, the tables hit every boundary they claim."""
import numpy as np
import pytest

import _gram_cases as gc

DTYPES = ["float64", "float32"]
L = np.longdouble


def _host_case(c, dtype):
    inp = gc.inputs(c["n"], c["m"], c["p_kind"])
    x3, c3, y3, P = gc.host_cell_inputs(inp, dtype)
    return x3, c3, y3, P, gc.host_kernel_values(x3, c3, c["beta"])


def _expected_mutations(c, dtype):
    n, m, sl = c["n"], c["m"], gc.emulated_slice_len(c)
    if c["p_kind"] == "zero":
        return set()
    want = {"drop_last_cell"}
    if n > gc.KSTEP:
        want.add("drop_k_step")
    if gc.cdiv(n, sl) >= 2:
        want.add("drop_slice")
    if gc.cdiv(n, sl) > gc.REDUCE_WAYS:
        want.add("reduce_skips_slice_8")
    if gc.rhs_plan(n, m)[1] > gc.REDUCE_WAYS:
        want.add("rhs_reduce_skips_slice_8")
    if m > gc.GT:
        want.add("transpose_off_diagonal_tile")
    if m >= 2:
        want.add("last_column_from_its_neighbour")
    if c["p_kind"] != "one":
        want.add("p_rounded_to_float32" if dtype == "float64" else "rhs_weights_not_rounded")
    return want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", gc.SMALL_CASES, ids=gc.case_id)
def test_emulated_kernel_order_is_within_the_bound_and_mutations_are_not(c, dtype):
    n, m = c["n"], c["m"]
    x3, c3, y3, P, U = _host_case(c, dtype)
    assert U.shape == (n, m) and U.dtype == gc.np_dtype(dtype) and P.dtype == U.dtype
    W = gc.rhs_weights(y3, P)
    assert W.dtype == U.dtype
    G_ref = gc.gram_reference(U, P)
    R_ref, S = gc.rhs_reference(U, W)
    bG, bR = gc.bound(G_ref, n), gc.bound(S, n)
    sl, rsl = gc.emulated_slice_len(c), gc.rhs_plan(n, m)[0]
    rg = gc.ratio(gc.emulate_gram(U, P, sl), G_ref, bG)
    rr = gc.ratio(gc.emulate_rhs(U, W, rsl), R_ref, bR)
    assert rg <= 1.0 and rr <= 1.0, (rg, rr)
    assert (G_ref >= 0).all() and (G_ref == G_ref.T).all()
    if c["p_kind"] == "zero":
        assert not G_ref.any() and not R_ref.any()
    else:
        assert G_ref.max() > 0
    muts = gc.mutations(U, P, y3, sl, rsl, dtype, c["p_kind"])
    assert set(muts) == _expected_mutations(c, dtype)
    for name, (G, R) in muts.items():
        moved = max(gc.ratio(G, G_ref, bG) if G is not None else 0.0, gc.ratio(R, R_ref, bR) if R is not None else 0.0)
        assert moved >= gc.MUTATION_FACTOR, (name, moved)
    # a padded control point that is not masked: ublk_build_kernel stages it at the centre of the frame, where cells are -
    # the cache's padded columns, asserted exactly 0 on the device, would hold values >= 100 x the bound's relative size
    if m % gc.GT:
        assert gc.padded_point_value(x3, c["beta"]) >= gc.MUTATION_FACTOR * (n + 2) * gc.U_ROUND


@pytest.mark.parametrize("dtype", DTYPES)
def test_sampled_reference_of_the_three_phase_case(dtype):
    n, m = gc.PHASE_CASE
    rows = gc.sample_rows(m)
    nt = gc.cdiv(m, gc.GT)
    assert len(rows) == 40 and len(set(rows.tolist())) == 40 and rows.min() == 0 and rows.max() == m - 1
    for t in range(nt):  # every tile's first and last live row: with G == G^T every tile pair's first and last row and column
        assert t * gc.GT in rows and min(m, (t + 1) * gc.GT) - 1 in rows
    assert {15, 16, 63, 64, 111, 112} <= set(rows.tolist())  # 16-block edges of the first tile
    el = gc.sample_elements(m)
    assert len(el) == 64 and all(0 <= i <= j < m for i, j in el) and (0, m - 1) in el and (m - 1, m - 1) in el
    # the two sampled references against the longdouble one, on a shape it can do in full (same code paths)
    c = gc.case("sample", 513, 257)
    _, _, _, P, U = _host_case(c, dtype)
    G_ref = gc.gram_reference(U, P)
    b = gc.bound(G_ref, 513)
    r = gc.sample_rows(257)
    assert gc.ratio(gc.gram_rows_blas(U, P, r), G_ref[r], b[r]) <= 1.0  # (the GPU module allows reference + kernel: 2 x)
    for i, j in gc.sample_elements(257, 16):
        exact = gc.gram_element_exact(U[:, i], U[:, j], P)
        assert abs(L(exact) - G_ref[i, j]) <= L(2.0 ** -52) * G_ref[i, j]  # fsum rounds once; the reference carries n eps_80


def test_underflow_case_has_normals_denormals_and_zeros():
    c = gc.UNDERFLOW
    _, _, _, _, U = _host_case(c, "float32")
    normal, denormal, zero = gc.census(U)
    assert normal > 1000 and denormal > 1000 and zero > 1000, (normal, denormal, zero)
    # float64 mode at the same beta: values far below float32's range, products of two of them underflow in float64
    _, _, _, _, U64 = _host_case(c, "float64")
    assert ((U64 > 0) & (U64 < 2.0 ** -512)).sum() > 300
    two = np.sort(U64, axis=1)[:, :2]
    assert (two[:, 0] * two[:, 1] < 2.0 ** -1022).sum() > 100  # cells whose two smallest values multiply below the normal range


def test_three_phase_plan():
    n, m = gc.PHASE_CASE
    for dtype in DTYPES:
        p = gc.forced_plan(n, m, dtype, gc.SLICE_LEN)
        assert (p["nt"], p["npairs"], p["nslices"], p["fit"], p["nphases"], p["phase_slices"]) == (17, 153, 299, 149, 3, 100)
        assert p["gram_bytes"] == 100 * 153 * 128 * 128 * 8
        assert n - 298 * 256 == 1  # the last slice holds one live cell
        assert p["edge2"] == (dtype == "float64")  # one live column in the last tile column: edge2 with nt = 17
    assert gc.MIN_TILES == 22888


def test_cases_sit_on_every_boundary():
    ms, ns = set(gc.M_TABLE), set(gc.N_TABLE)

    def around(v, s):
        return {v - 1, v, v + 1} <= s

    # UB = 16 (one cached block, one MFMA block): a block with 1, 15, 16 live points and the first point of the second
    assert {1, gc.UB - 1, gc.UB, gc.UB + 1} <= ms
    # 4 * UB = 64 live columns (`live_cols <= 4 * UB`: the 2 x 4 edge shape; GT / 2 in make_plan's edge2): either side of it
    # in one tile, and 64 / 65 live columns in a LAST tile column behind a full one
    assert around(gc.EDGE_COLS, ms) and {gc.GT + gc.EDGE_COLS, gc.GT + gc.EDGE_COLS + 1} <= ms
    # GT = 128: one tile, then two; nt = 3 (odd: edge2 leaves the diagonal tile over) and nt = 4 (even: (2,3) pairs with (3,3))
    assert around(gc.GT, ms)
    nts = {m: gc.cdiv(m, gc.GT) for m in ms}
    edge2 = {m: nts[m] >= 2 and m - (nts[m] - 1) * gc.GT <= gc.GT // 2 for m in ms}
    assert {nts[m] for m in ms if edge2[m]} >= {2, 3, 4, 5} and {nts[m] for m in ms if not edge2[m]} >= {1, 2, 4}
    assert edge2[129] and edge2[257] and edge2[385] and edge2[440] and not edge2[193]
    # RHS_COLS = 512 control points per rhs workgroup, cb_per_block * UB = 512 per ublk_build workgroup column
    assert around(gc.RHS_COLS, ms) and gc.RHS_COLS == gc.UBLK_COLS
    # k-step of 4 cells (v_mfma_f64_16x16x4_f64)
    assert {1, gc.KSTEP - 1, gc.KSTEP, gc.KSTEP + 1} <= ns
    # superblock = 4096 bytes of one operand stream: 4096 / (UB * sizeof(T)) = 64 cells in float32, 32 in float64
    # (SUPER * UGT * 4; ng_main and the clamped remainder loop)
    assert gc.SUPER_CELLS == {"float32": 4096 // (gc.UB * 4), "float64": 4096 // (gc.UB * 8)}
    for cells in gc.SUPER_CELLS.values():
        assert around(cells, ns)
    # GCHUNK = 256 cells: the LDS stage, n_pad and the padded last slice
    assert around(gc.GCHUNK, ns) and {2 * gc.GCHUNK - 1, 2 * gc.GCHUNK + 1} <= ns
    assert set(gc.M_TABLE_NS) == {257, 65} and set(gc.N_TABLE_MS) == {17, 193}
    # gram_reduce_kernel: eight interleaved sums - 7 (tail only), 8 (one full round), 9, 16, 17 slices, one live cell in the last
    ks = [gc.cdiv(c["n"], gc.SLICE_LEN) for c in gc.SLICE_CASES]
    assert ks == gc.SLICE_KS and {gc.REDUCE_WAYS - 1, gc.REDUCE_WAYS, gc.REDUCE_WAYS + 1, 2 * gc.REDUCE_WAYS,
                                  2 * gc.REDUCE_WAYS + 1} <= set(ks)
    assert all(c["n"] % gc.SLICE_LEN == 1 and c["m"] == 130 for c in gc.SLICE_CASES)
    # rhs_reduce_kernel: 16 slice lanes (15, 16, 17 and 33 rhs slices of 256 cells) and 16 control points per workgroup
    rs = [gc.rhs_plan(c["n"], c["m"]) for c in gc.RHS_SLICE_CASES]
    assert [r[1] for r in rs] == [15, 16, 17, 33] and all(r[0] == gc.GCHUNK for r in rs)
    assert gc.RHS_SLICE_M == gc.RHS_LANES + 1
    # the 3e9-byte minimum of the partial-tile buffer (22 888 tiles): three phases, a middle one
    p = gc.forced_plan(*gc.PHASE_CASE, "float32", gc.SLICE_LEN)
    assert p["nphases"] == 3 and p["fit"] == gc.MIN_TILES // p["npairs"] and 2 * p["fit"] < p["nslices"] <= 3 * p["fit"]
    # P variants empty whole k-steps and a whole slice
    P = gc.inputs(*gc.P_CASE, "holes")["P"]
    assert not P[gc.KSTEP:2 * gc.KSTEP].any() and not P[gc.GCHUNK:2 * gc.GCHUNK].any() and P[:gc.KSTEP].all() and P[2 * gc.GCHUNK:2 * gc.GCHUNK + 4].all()
    Pf = gc.inputs(*gc.P_CASE, "floor")["P"]
    assert (Pf == 0).sum() > 250 and (Pf == 1e-5).sum() > 100 and (Pf > 0.5).sum() > 100
    # every case the longdouble reference is asked for in full is affordable; the three-phase case is not
    assert all(gc.full_reference_affordable(c["n"], c["m"]) for c in gc.SMALL_CASES)
    assert not gc.full_reference_affordable(*gc.PHASE_CASE)
    assert set(gc.DEAD_MS) == {129, 193, 257, 385}
