"""CPU proofs behind tests/test_gpu_prep_kernels.py and tests/test_gpu_conk_kernels.py: the references and restatements of
tests/_prep_cases.py agree with independent NumPy / SciPy computations, the case tables reach the branches they name, and every
comparison function the GPU modules use catches a seeded mistake (an unstable sort, a skipped radix byte, a dropped facet, k off
by one, rank 0 kept, a shifted con_K column)."""
import numpy as np
import pytest

import _prep_cases as pc

SENT_UID, SENT_ROW = -1234567890123, -1.2345e300   # the scaffold's sentinels of int64 / float64 buffers


# =========================================================================================================== unique_rows
@pytest.mark.parametrize("name", pc.UNIQUE_NAMES)
def test_unique_restatement_is_numpy_unique(name):
    X, ref = pc.unique_case(name), pc.unique_reference(name)
    count, uid, rows = pc.unique_restated(X, SENT_UID, SENT_ROW)
    assert pc.compare_unique(X, ref, count, uid, rows, SENT_UID, SENT_ROW) == []
    assert np.isfinite(X).all()


def test_unique_compare_catches_an_unstable_sort_and_a_write_behind_count():
    for name in ("n4097_d2_dup4_first_last", "n5000_d16_tied", "n65537_d1", "key_order_d1"):
        X, ref = pc.unique_case(name), pc.unique_reference(name)
        count, uid, rows = pc.unique_restated(X, SENT_UID, SENT_ROW, last_occurrence=True)
        bad = pc.compare_unique(X, ref, count, uid, rows, SENT_UID, SENT_ROW)
        assert bad and "uid" in bad[0], (name, bad)
    X, ref = pc.unique_case("n257_d3"), pc.unique_reference("n257_d3")
    count, uid, rows = pc.unique_restated(X, SENT_UID, SENT_ROW)
    uid2 = uid.copy()
    uid2[count] = 0
    assert pc.compare_unique(X, ref, count, uid2, rows, SENT_UID, SENT_ROW) == ["uid written behind count"]
    rows2 = rows.copy()
    rows2[-1, -1] = 0.0
    assert pc.compare_unique(X, ref, count, uid, rows2, SENT_UID, SENT_ROW) == ["rows written behind count"]
    assert pc.compare_unique(X, ref, count - 1, uid, rows, SENT_UID, SENT_ROW) != []


def test_unique_rows_are_compared_by_bits():
    """-0.0 and 0.0 are one key: the row returned is the FIRST of them, sign included."""
    for name, first in (("key_order_d1", -0.0), ("key_order_d1_negated", 0.0)):
        X, ref = pc.unique_case(name), pc.unique_reference(name)
        zero = X[ref][X[ref][:, 0] == 0.0]
        assert zero.shape == (1, 1) and np.signbit(zero[0, 0]) == np.signbit(first)
        count, uid, rows = pc.unique_restated(X, SENT_UID, SENT_ROW)
        rows = rows.copy()
        j = int(np.flatnonzero(rows[:count, 0] == 0.0)[0])
        rows[j, 0] = -rows[j, 0]
        assert pc.compare_unique(X, ref, count, uid, rows, SENT_UID, SENT_ROW) == ["rows[:count] differ from X[uid] by bits"]


@pytest.mark.parametrize("byte", range(8))
def test_unique_compare_catches_a_skipped_radix_byte(byte):
    """The keys of case ``byte`` differ in that byte alone: without its pass the order is the input order, and the comparison
    says so; every other pass can be left out on this case without a trace - the pass is decisive on its own."""
    name = f"n4097_d1_byte{byte}"
    X, ref = pc.unique_case(name), pc.unique_reference(name)
    raw = np.ascontiguousarray(X[:, 0]).view(np.uint64)
    differ = np.bitwise_or.reduce(raw ^ raw[0])
    assert differ != 0 and (differ & ~(np.uint64(0xFF) << np.uint64(8 * byte))) == 0
    for skip in range(8):
        count, uid, rows = pc.unique_restated(X, SENT_UID, SENT_ROW, skip_byte=skip)
        bad = pc.compare_unique(X, ref, count, uid, rows, SENT_UID, SENT_ROW)
        assert bool(bad) == (skip == byte), (skip, bad)


def test_analytic_reference_of_the_large_case_is_numpy_unique_at_a_cheap_size():
    n = 3 * 4096 + 1
    X = pc.large_case(n)
    uid = pc.large_reference(n)
    assert np.array_equal(uid, np.unique(X, axis=0, return_index=True)[1])
    count, u, rows = pc.unique_restated(X, SENT_UID, SENT_ROW)
    assert pc.compare_unique(X, uid, count, u, rows, SENT_UID, SENT_ROW) == []


def test_large_case_reaches_the_two_branches_it_is_there_for():
    n = pc.LARGE_N
    chunks = pc.cdiv(n, pc.RS_CHUNK)
    hist_segments = pc.cdiv(chunks * pc.RS_BINS, pc.SCAN_SEG)
    assert pc.cdiv(hist_segments, 256) == 2                      # per = 2 in scan_segoff_kernel
    assert pc.cdiv(chunks, pc.SCAN_SEG) == 2                     # two segments in the compaction scan
    assert pc.cdiv(pc.cdiv(65537, pc.RS_CHUNK) * pc.RS_BINS, pc.SCAN_SEG) == 2   # n = 65 537: two segments of the histogram table
    X, uid = pc.large_case(), pc.large_reference()
    assert len(uid) == pc.cdiv(n, 3) and np.array_equal(X[uid, 0], np.arange(len(uid)))
    assert uid.min() == 0 and uid.max() < n and len(np.unique(uid)) == len(uid)
    # first occurrence: no row before uid[v] holds v (checked on a sample; the formula is proved whole at the cheap size)
    for v in (0, 1, 4096, len(uid) - 1):
        assert int(np.flatnonzero(X[:, 0] == float(v))[0]) == uid[v]


# ============================================================================================================ knn_rowsum
@pytest.fixture(scope="module")
def brute():
    """{name: {k: sorted-cdist row sums}}, float64 throughout: an independent statement of the same quantity."""
    from scipy.spatial.distance import cdist

    out = {}
    for name in pc.KNN_NAMES:
        X, ks = pc.knn_case(name), pc.KNN_CASES[name]["ks"]
        sums = {k: np.empty(len(X)) for k in ks}
        for lo in range(0, len(X), 1024):
            D = cdist(X[lo:lo + 1024], X)
            D.sort(axis=1)
            for k in ks:
                sums[k][lo:lo + 1024] = D[:, 1:k].sum(axis=1)
        out[name] = sums
    return out


@pytest.mark.parametrize("name", pc.KNN_NAMES)
def test_knn_references_agree_with_sorted_cdist_within_the_bound(name, brute):
    X, d = pc.knn_case(name), pc.knn_case(name).shape[1]
    for k, (ref, res) in pc.knn_tables(name).items():
        assert ref.shape == (len(X),) and (ref >= 0).all()
        share_brute = pc.compare_knn(brute[name][k], ref, k, d)
        share_res = pc.compare_knn(res, ref[:len(res)], k, d)
        print(f"knn {name} k={k}: sorted cdist uses {share_brute:.3f} of the bound, the order-following restatement {share_res:.3f}")
        assert share_brute <= 1.0 and share_res <= 1.0
    if name == "m257_d3_copies":   # the copies see k - 1 zero distances: the reference is exactly 0 there
        ref5 = pc.knn_tables(name)[5][0]
        assert (ref5[[3, 20, 77, 130, 200, 256]] == 0.0).all() and (np.delete(ref5, [3, 20, 77, 130, 200, 256]) > 0).all()


def test_exact_row_sums_is_fsum():
    import math

    rng = np.random.default_rng(0)
    a = np.abs(rng.standard_normal((64, 1000))) * 10.0 ** rng.integers(-12, 6, (64, 1))    # limbs and the fsum route
    a[5, :7] = 0.0
    a[6] = 0.0
    a[7, 3] = 5e-324
    a[8] = 2.0 ** 19 + 0.5
    lattice = np.sqrt(np.arange(2048.0))[None, :].repeat(3, axis=0)
    for arr in (a, lattice, np.zeros((2, 0)), np.sqrt(((pc.knn_case("m1023_d6")[:40, None] - pc.knn_case("m1023_d6")[None]) ** 2).sum(-1))):
        got = pc.exact_row_sums(arr)
        assert got.tolist() == [math.fsum(r) for r in arr.tolist()]


def test_knn_kdtree_agrees_with_the_reference():
    from scipy.spatial import cKDTree

    for name in ("m255_d3", "m1025_d8", "m1024_d2_lattice"):
        X = pc.knn_case(name)
        for k, (ref, _) in pc.knn_tables(name).items():
            if k <= 258:
                dist, _ = cKDTree(X).query(X, k=k)
                assert pc.compare_knn(dist[:, 1:].sum(axis=1), ref, k, X.shape[1]) <= 1.0


@pytest.mark.parametrize("name", ("m3_d2", "m255_d3", "m257_d3_copies", "m1024_d2_lattice", "m1025_d8"))
def test_knn_compare_catches_k_off_by_one_and_rank_0_kept(name):
    X = pc.knn_case(name)
    m, d = X.shape
    for k, (ref, _) in pc.knn_tables(name).items():
        wrong_k = [kk for kk in (k - 1, k + 1) if 2 <= kk <= m]
        for kk in wrong_k:
            got = pc.knn_restated_block(X, 0, m, (kk,))[kk]
            assert pc.compare_knn(got, ref, k, d) > 1.0, (k, kk)
        got = pc.knn_restated_block(X, 0, m, (k,), skip_rank0=False)[k]
        assert pc.compare_knn(got, ref, k, d) > 1.0, k
    assert pc.compare_knn(np.full(m, np.nan), ref, k, d) > 1.0


# ============================================================================================================= hull_mask
@pytest.mark.parametrize("name", pc.HULL_EXACT_NAMES)
def test_exact_hull_cases_are_exact_and_mixed(name):
    case = pc.hull_exact_case(name)
    P, E, tol = case["points"], case["eq"], case["tol"]
    assert pc.check_fma_exact(P, E)
    assert (E == np.rint(E)).all() and (4 * P == np.rint(4 * P)).all() and tol in (0.0, 0.25, 2.0)
    ref = pc.hull_exact_reference(P, E, tol)
    M, dp, de = pc.hull_exact_margins(P, E)
    worst = np.array([max(row) for row in M], dtype=object)
    on_tol = np.array([w == int(tol * dp * de) for w in worst])
    assert on_tol.any() and ref[on_tol].all()          # margin exactly tol counts as inside
    if len(P) > 1:
        assert ref.any() and not ref.all()
    # float64 evaluation of the same margins is exact on these cases, whatever the order
    plain = (P @ E[:, :3].T + E[:, 3]).max(axis=1) <= tol
    assert np.array_equal(plain, ref)


def test_one_violated_facet_cases_and_the_dropped_facet():
    for pos in pc.POSITIONS:
        name = f"poly_f611_one_violated_at_{'last' if pos < 0 else pos}"
        case = pc.hull_exact_case(name)
        P, E, tol = case["points"], case["eq"], case["tol"]
        at = len(E) - 1 if pos < 0 else pos
        assert len(E) == pc.POLY_FACETS and tuple(E[at]) == (1.0, 0.0, 0.0, -1000.0)
        M, _, _ = pc.hull_exact_margins(P[:1], E)
        assert [j for j, v in enumerate(M[0]) if v > 0] == [at]
        ref = pc.hull_exact_reference(P, E, tol)
        assert not ref[0]
        wrong = pc.hull_exact_reference(P, E, tol, drop=at)
        assert wrong[0] and pc.compare_mask(wrong.astype(np.uint8), ref) != []
        other = pc.hull_exact_reference(P, E, tol, drop=(at + 1) % len(E))
        assert not other[0]
    assert pc.cdiv(pc.POLY_FACETS, pc.HULL_CHUNK) == 3 and pc.POLY_FACETS % pc.HULL_CHUNK not in (0, 1)
    case = pc.hull_exact_case("poly_f611_one_violated_at_256")
    ref = pc.hull_exact_reference(case["points"], case["eq"], case["tol"])
    assert pc.compare_mask(ref.astype(np.uint8), ref) == []
    two = ref.astype(np.uint8)
    two[5] = 2
    assert pc.compare_mask(two, ref)[0] == "a byte that is neither 0 nor 1"


@pytest.mark.parametrize("name", ("cube_n255", "octahedron_n513", "poly_f611_n513"))
def test_exact_hull_reference_is_find_simplex_away_from_the_facets(name):
    from scipy.spatial import Delaunay, HalfspaceIntersection

    case = pc.hull_exact_case(name)
    P, E, tol = case["points"], case["eq"], case["tol"]
    vertices = HalfspaceIntersection(E, np.zeros(3)).intersections
    want = Delaunay(vertices).find_simplex(P) >= 0
    margin = (P @ E[:, :3].T + E[:, 3]).max(axis=1)
    away = (margin < -1.0) | (margin > tol + 1.0)
    assert away.sum() > len(P) // 2
    assert np.array_equal(pc.hull_exact_reference(P, E, tol)[away], want[away])


def test_float_hull_reference_decides_every_point_and_is_find_simplex_away_from_the_facets():
    from scipy.spatial import Delaunay

    case = pc.hull_float_case()
    P, E, tol, s = case["points"], case["eq"], case["tol"], case["s"]
    assert len(P) == 4099 and len(E) >= 600
    inside, und = pc.hull_float_reference(P, E, tol)
    print(f"float hull: {len(E)} facets, {int(inside.sum())} of {len(P)} inside, {int(und.sum())} undecided for the reference alone")
    assert und.mean() <= pc.UNDECIDED_CAP
    assert np.array_equal(inside[~und], (s <= 1.0)[~und])     # pushed out by less than tol: inside; by more: outside
    # the same reference against the formulation the API replaces, on points the tolerance does not reach
    rng = np.random.default_rng(3)
    Q = rng.uniform(-1.0, 1.0, (4000, 3)) * np.array([300.0, 200.0, 150.0])
    ins, _ = pc.hull_float_reference(Q, E, tol)
    margin = (Q @ E[:, :3].T + E[:, 3]).max(axis=1)
    away = np.abs(margin) > 1e-9 * 600.0
    want = Delaunay(case["vertices"]).find_simplex(Q) >= 0
    assert away.all() and 0.2 < want.mean() < 0.8
    assert np.array_equal(ins, want)


def test_compare_mask_ignores_only_the_undecided_points():
    ref = np.array([1, 0, 1, 1], dtype=bool)
    got = np.array([1, 1, 1, 0], dtype=np.uint8)
    assert pc.compare_mask(got, ref) == ["2 points differ, first at 1"]
    assert pc.compare_mask(got, ref, undecided=np.array([0, 1, 0, 0], dtype=bool)) == ["1 points differ, first at 3"]
    assert pc.compare_mask(got, ref, undecided=np.array([0, 1, 0, 1], dtype=bool)) == []


# ================================================================================================================= con_K
@pytest.mark.parametrize("dtype", ("float64", "float32"))
def test_conk_reference_is_exp_of_cdist_and_a_shifted_column_is_caught(dtype):
    from scipy.spatial.distance import cdist

    for n, m, d in ((5, 68, 3), (33, 9, 8), (7, 1025, 1)):
        x, y = pc.conk_points(n, m, d, dtype)
        assert x.dtype == pc.NP_DTYPE[dtype] and y.shape == (m, d)
        ref = pc.conk_reference(x, y, pc.CONK_BETA)
        plain = np.exp(-pc.CONK_BETA * cdist(x.astype(np.float64), y.astype(np.float64), "sqeuclidean"))
        assert pc.compare_conk(plain, ref) < 1e-14
        assert 0.2 < float(ref.max()) <= 1.0 and float(ref.min()) < 0.5
        good = pc.conk_restated(x, y, pc.CONK_BETA)
        assert good.dtype == x.dtype and pc.compare_conk(good, ref) <= pc.CONK_TOL[dtype]
        for j in (0, m // 2, m - 2):
            assert pc.compare_conk(pc.conk_restated(x, y, pc.CONK_BETA, shift_column=j), ref) > pc.CONK_TOL[dtype], (n, m, d, j)
    bad = good.copy()
    bad[0, 0] = np.nan
    assert pc.compare_conk(bad, ref) > pc.CONK_TOL[dtype]


def test_conk_difference_reference_is_one_subtraction_per_element():
    for dtype in ("float64", "float32"):
        x, y = pc.conk_points(3, 257, 5, dtype)
        D = pc.conk_diff_reference(x, y)
        assert D.shape == (3, 5, 257) and D.dtype == x.dtype and D.flags.c_contiguous
        assert D[2, 4, 256] == x[2, 4] - y[256, 4] and D[0, 0, 1] == x[0, 0] - y[1, 0]


def test_case_tables_name_every_branch_they_are_there_for():
    rows = pc.CONK_ROW_CASES.values()
    for dtype in ("float32", "float64"):
        mine = [c for c in rows if c["dtype"] == dtype]
        assert {c["rs"] for c in mine if c["fits"]} == {1, 2, 4}
        assert {1, 8} <= {c["np"] for c in mine if c["fits"]}
        assert {c["rs"] for c in mine if not c["fits"]} == {1, 2, 4}        # the first m past the row form, per RS
        assert 64 in {c["m"] for c in mine}
        for c in mine:                                                       # a partial last span and a lone row
            assert 1 in c["ns"] and c["rs"] + 1 in c["ns"] and 35 in c["ns"] and (c["rs"] == 1 or c["rs"] - 1 in c["ns"])
        flat = [c for c in pc.CONK_FLAT_CASES.values() if c["dtype"] == dtype]
        lds = [3 * c["m"] * pc.NP_DTYPE[dtype]().itemsize for c in flat]
        assert any(v <= 65536 for v in lds) and any(65536 < v <= pc.CONK_FLAT_LDS_MAX for v in lds) and any(v > pc.CONK_FLAT_LDS_MAX for v in lds)
        v = pc.VEC[dtype]
        assert set(pc.conk_2d_ms(dtype)) == {1, v - 1, v + 1, 256 * v - 1, 256 * v + 1}
    assert pc.conk_row_plan(8192, "float32") == (1, True, 8) and pc.conk_row_plan(8208, "float32")[1] is False
    assert not pc.conk_flat_fits(8208, "float32") and pc.conk_flat_fits(6824, "float32") and not pc.conk_flat_fits(6828, "float32")
    for table in (pc.UNIQUE_BRANCH, {k: v["branch"] for k, v in pc.KNN_CASES.items()}, {k: v["branch"] for k, v in pc.HULL_EXACT.items()},
                  {k: v["branch"] for k, v in {**pc.CONK_ROW_CASES, **pc.CONK_FLAT_CASES}.items()}):
        assert all(isinstance(b, str) and b for b in table.values())
    assert set(pc.UNIQUE_BRANCH) == set(pc.UNIQUE_NAMES) | {"large_n16781313_d1"}
    assert {pc.knn_case(n).shape[1] for n in pc.KNN_NAMES} == set(range(1, 9))
    assert {len(pc.knn_case(n)) for n in pc.KNN_NAMES} >= {2, 3, 255, 256, 257, 1023, 1024, 1025, 8192}
