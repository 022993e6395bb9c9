"""Kernel-level tests of ``csrc/mvf_prep.hip`` through the raw C ABI on ``cuda:0``: ``mvf_unique_rows`` (+ its workspace
query), ``mvf_knn_rowsum`` and ``mvf_hull_mask``.  Cases, references, bounds and comparison functions come from
tests/_prep_cases.py (proved on the CPU by tests/test_prep_kernel_refs.py).  Every output sits between guards, every workspace
is exactly the bytes the library asks for between guards of its own, every case runs twice and the two results are compared bit
for bit.  unique_rows and the exact hull cases are compared without a tolerance; knn against the derived bound (k + d + 4) 2^-53
ref; the float hull at every point the np.longdouble margins decide."""
import ctypes

import numpy as np
import pytest
import torch

import _prep_cases as pc
from _kernel_scaffold import (MODES, SENTINEL, Out, Ws, called as _called, deviation_table, dev as _dev, same_bits as _same_bits,
                              stream as _stream, under as _under)

pytestmark = pytest.mark.gpu

SENT_UID, SENT_ROW = SENTINEL[torch.int64], SENTINEL[torch.float64]
_bit_equal_rows = {}     # knn case -> (rows equal to the order-following restatement bit for bit, rows compared)
_float_hull = {}


def _on_done():
    eq, total = sum(a for a, _ in _bit_equal_rows.values()), sum(b for _, b in _bit_equal_rows.values())
    print(f"\nknn_rowsum: {eq} of {total} (case, k, row) results equal the order-following restatement bit for bit (reported, not "
          "asserted: it rests on a correctly rounded device sqrt)")
    for name, (a, b) in sorted(_bit_equal_rows.items()):
        print(f"  {name}: {a} of {b}")
    if _float_hull:
        print("hull_mask, float hull: {facets} facets, {n} points, {inside} inside, {undecided} undecided, {differ} decided points differ"
              .format(**_float_hull))


_note, _deviation_table = deviation_table("| case | quantity | largest |", on_done=_on_done,
                                          footer=lambda seconds, notes: f"test_gpu_prep_kernels: {seconds:.1f} s")


@pytest.fixture(scope="module")
def lib():
    from spateo_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def _err(lib):
    return lib.mvf_last_error() or b""


# =========================================================================================================== unique_rows
class _Unique:
    """One raw ``mvf_unique_rows`` call on device rows ``xd`` (n, d): guarded outputs, a workspace of exactly the bytes asked
    for, all sized by the true shape.  ``claim`` overrides what the call is told (n, d, ws_bytes) and which pointers it gets."""

    def __init__(self, lib, xd, true_n, true_d, **claim):
        n, d = true_n, true_d
        self.n, self.d = n, d
        self.uid, self.rows, self.count = Out(max(n, 1), dtype=torch.int64), Out(max(n * d, 1)), Out(1, dtype=torch.int64)
        self.need = int(lib.mvf_unique_rows_workspace_bytes(n, d))
        self.ws = Ws(max(self.need, 256))
        a = dict(X=None if xd is None else xd.data_ptr(), n=n, d=d, uid=self.uid.ptr, rows=self.rows.ptr, count=self.count.ptr,
                 ws=self.ws.ptr, ws_bytes=self.need)
        a.update(claim)
        self.rc = lib.mvf_unique_rows(a["X"], a["n"], a["d"], a["uid"], a["rows"], a["count"], a["ws"], a["ws_bytes"], _stream())
        _called()
        torch.cuda.synchronize()
        assert self.guards_intact(), "wrote outside an output or the workspace"

    def guards_intact(self):
        return self.uid.guards_intact() and self.rows.guards_intact() and self.count.guards_intact() and self.ws.guards_intact()

    def untouched(self):
        return self.uid.untouched() and self.rows.untouched() and self.count.untouched()

    def host(self):
        return int(self.count.host()[0]), self.uid.host()[:self.n], self.rows.host()[:self.n * self.d].reshape(self.n, self.d)


def _check_unique(lib, X, ref_uid):
    n, d = X.shape
    xd = _dev(X)
    first = _Unique(lib, xd, n, d)
    assert first.rc == 0, _err(lib)
    assert first.need == int(lib.mvf_unique_rows_workspace_bytes(n, d)) > 0
    count, uid, rows = first.host()
    assert pc.compare_unique(X, ref_uid, count, uid, rows, SENT_UID, SENT_ROW) == []
    again = _Unique(lib, xd, n, d)
    assert again.rc == 0, _err(lib)
    count2, uid2, rows2 = again.host()
    assert count2 == count and np.array_equal(uid2, uid) and _same_bits(rows2, rows)
    return count


@pytest.mark.parametrize("name", pc.UNIQUE_NAMES)
def test_unique_rows_is_numpy_unique_bit_for_bit(lib, name):
    X = pc.unique_case(name)
    count = _check_unique(lib, X, pc.unique_reference(name))
    print(f"unique_rows {name}: n = {len(X)}, d = {X.shape[1]}, {count} distinct [{pc.UNIQUE_BRANCH[name]}]")


def test_unique_rows_large_case_two_scan_levels(lib):
    """n = 4097 x 4096 + 1 rows: 4098 chunks, so the segment-offset scan gives two segments to a lane (``per`` = 2, 257 segments of
    the histogram table) and the compaction's table has two segments.  The reference is analytic (tests/_prep_cases.py)."""
    import time

    X, ref = pc.large_case(), pc.large_reference()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    count = _check_unique(lib, X, ref)
    print(f"unique_rows large: n = {len(X)}, {count} distinct, {time.perf_counter() - t0:.1f} s for two calls and their comparisons "
          f"[{pc.UNIQUE_BRANCH['large_n16781313_d1']}]")


def test_unique_rows_of_nothing_sets_count_and_touches_nothing_else(lib):
    call = _Unique(lib, None, 0, 3, uid=None, rows=None, ws=None, ws_bytes=0)
    assert call.rc == 0, _err(lib)
    assert int(call.count.host()[0]) == 0 and call.uid.untouched() and call.rows.untouched()
    xd = _dev(pc.unique_case("n257_d3"))
    call = _Unique(lib, xd, 0, 3)
    assert call.rc == 0 and int(call.count.host()[0]) == 0 and call.uid.untouched() and call.rows.untouched()
    assert bool((call.ws.big == 0xA5).all())


def test_unique_rows_refusals_leave_the_outputs_alone(lib):
    X = pc.unique_case("n257_d3")
    xd = _dev(X)
    need = int(lib.mvf_unique_rows_workspace_bytes(257, 3))
    for claim, msg in ((dict(d=0), b"bad shape"), (dict(d=17), b"bad shape"), (dict(n=-1), b"bad shape"), (dict(count=None), b"null count"),
                       (dict(ws=None), b"workspace too small"), (dict(ws_bytes=need - 1), b"workspace too small"),
                       (dict(X=None), b"null pointer"), (dict(uid=None), b"null pointer"), (dict(rows=None), b"null pointer")):
        call = _Unique(lib, xd, 257, 3, **claim)
        assert call.rc != 0 and b"mvf_unique_rows" in _err(lib) and msg in _err(lib), (claim, _err(lib))
        assert call.untouched() and bool((call.ws.big == 0xA5).all()), claim
    assert _Unique(lib, xd, 257, 3).rc == 0


def test_unique_rows_workspace_bytes(lib):
    f = lib.mvf_unique_rows_workspace_bytes
    for n, d in ((0, 3), (-1, 3), (-2**40, 1), (5, 0), (5, -1), (0, 0)):
        assert f(n, d) == 0, (n, d)
    sizes = sorted(set(pc.UNIQUE_SIZES) | {5000, pc.LARGE_N})
    for d in (1, 3, 16):
        got = [int(f(n, d)) for n in sizes]
        assert got[0] > 0 and got == sorted(got), (d, got)
        # two key and two index buffers of n x 8 bytes and n flags are the least any plan of this algorithm holds
        assert all(b >= 33 * n for b, n in zip(got, sizes))


# ============================================================================================================ knn_rowsum
def _knn_raw(lib, xd, m, d, k, X=True, out=True):
    o = Out(max(m, 1))
    rc = lib.mvf_knn_rowsum(xd.data_ptr() if X else None, m, d, k, o.ptr if out else None, _stream())
    _called()
    torch.cuda.synchronize()
    assert o.guards_intact(), "wrote outside rowsum"
    return rc, o


@pytest.mark.parametrize("name", pc.KNN_NAMES)
def test_knn_rowsum_within_the_derived_bound(lib, name):
    X = pc.knn_case(name)
    m, d = X.shape
    xd = _dev(X)
    equal = rows = 0
    for k, (ref, restated) in pc.knn_tables(name).items():
        rc, o = _knn_raw(lib, xd, m, d, k)
        assert rc == 0, _err(lib)
        got = o.host()[:m]
        share = pc.compare_knn(got, ref, k, d)
        same = int((got[:len(restated)].view(np.int64) == restated.view(np.int64)).sum())
        equal, rows = equal + same, rows + len(restated)
        print(f"knn_rowsum {name} k = {k}: {share:.3f} of the bound (k + d + 4) 2^-53 ref, {same} of {len(restated)} rows equal the "
              f"order-following restatement bit for bit [{pc.KNN_CASES[name]['branch']}]")
        _note(f"knn_rowsum {name}", "share of the bound (k + d + 4) 2^-53 ref", share)
        assert share <= 1.0, (k, share)
        rc, o2 = _knn_raw(lib, xd, m, d, k)
        assert rc == 0 and _same_bits(o2.host(), o.host())
    _bit_equal_rows[name] = (equal, rows)


def test_knn_rowsum_refusals(lib):
    X = pc.knn_case("m257_d5")
    xd = _dev(np.concatenate([X, np.zeros((8193 - 257, 5))]))   # (large enough for every shape the calls claim)
    for m, d, k, kw, msg in ((0, 5, 2, {}, b"need 1 <= m"), (8193, 5, 2, {}, b"need 1 <= m"), (257, 0, 2, {}, b"need 1 <= m"),
                             (257, 9, 2, {}, b"need 1 <= m"), (257, 5, 1, {}, b"need 2 <= k"), (257, 5, 258, {}, b"need 2 <= k"),
                             (1, 5, 2, {}, b"need 2 <= k"), (257, 5, 2, dict(X=False), b"null pointer"),
                             (257, 5, 2, dict(out=False), b"null pointer")):
        rc, o = _knn_raw(lib, xd, m, d, k, **kw)
        assert rc != 0 and b"mvf_knn_rowsum" in _err(lib) and msg in _err(lib), (m, d, k, kw, _err(lib))
        assert o.untouched()


# ============================================================================================================= hull_mask
def _hull_raw(lib, P, E, tol, n=None, nf=None, points=True, eq=True, out=True):
    pd_, ed = _dev(P), _dev(E)
    n = len(P) if n is None else n
    nf = len(E) if nf is None else nf
    o = Out(max(len(P), 1), dtype=torch.uint8)
    rc = lib.mvf_hull_mask(pd_.data_ptr() if points else None, n, ed.data_ptr() if eq else None, nf, ctypes.c_double(tol),
                           o.ptr if out else None, _stream())
    _called()
    torch.cuda.synchronize()
    assert o.guards_intact(), "wrote outside the mask"
    return rc, o


# ==================================================================================================== calling conventions
CONVENTION_COVERS = {"mvf_unique_rows": MODES, "mvf_knn_rowsum": MODES, "mvf_hull_mask": MODES}


def _unique_call(lib, name):
    X = pc.unique_case(name)
    u = _Unique(lib, _dev(X), *X.shape)
    assert u.rc == 0, _err(lib)
    count, uid, rows = u.host()
    return np.array([count]), uid, rows


def _knn_call(lib, name, k):
    X = pc.knn_case(name)
    rc, o = _knn_raw(lib, _dev(X), *X.shape, k)
    assert rc == 0, _err(lib)
    return (o.host(),)


def _hull_call(lib, name):
    case = pc.hull_exact_case(name)
    rc, o = _hull_raw(lib, case["points"], case["eq"], case["tol"])
    assert rc == 0, _err(lib)
    return (o.host(),)


# unique_rows: one chunk of one column; two chunks of three columns.  knn_rowsum: k below and above a wave's 256 candidates.
# hull_mask: one chunk of facets; three.
CONVENTION_CASES = {"mvf_unique_rows:n257_d1": (_unique_call, "n257_d1"), "mvf_unique_rows:n4097_d3": (_unique_call, "n4097_d3"),
                    "mvf_knn_rowsum:k51": (_knn_call, "m257_d5", 51), "mvf_knn_rowsum:k257": (_knn_call, "m257_d5", 257),
                    "mvf_hull_mask:f4": (_hull_call, "poly_f4_n255"), "mvf_hull_mask:f611": (_hull_call, "poly_f611_n513")}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", list(CONVENTION_CASES))
def test_calling_conventions(lib, entry, mode):
    """The plain call's bits on a side stream behind poisoned inputs, at displaced pointers, and with the inputs unchanged."""
    fn, *args = CONVENTION_CASES[entry]
    plain, got = _under(mode, lambda: fn(lib, *args))
    assert len(plain) == len(got) and all(_same_bits(a, b) for a, b in zip(plain, got))


@pytest.mark.parametrize("name", pc.HULL_EXACT_NAMES)
def test_hull_mask_equals_exact_integer_arithmetic(lib, name):
    case = pc.hull_exact_case(name)
    P, E, tol = case["points"], case["eq"], case["tol"]
    ref = pc.hull_exact_reference(P, E, tol)
    rc, o = _hull_raw(lib, P, E, tol)
    assert rc == 0, _err(lib)
    assert pc.compare_mask(o.host()[:len(P)], ref) == []
    rc, o2 = _hull_raw(lib, P, E, tol)
    assert rc == 0 and np.array_equal(o2.host(), o.host())
    print(f"hull_mask {name}: {len(P)} points x {len(E)} facets, tol = {tol}, {int(ref.sum())} inside [{pc.HULL_EXACT[name]['branch']}]")


def test_hull_mask_margin_exactly_tol_is_inside_and_the_next_float_is_outside(lib):
    E = pc.corner_box()
    for tol in (2.0, 0.25, 0.0):
        nxt = float(np.nextafter(tol, np.inf))
        P = np.array([[tol, 0.0, 0.0], [nxt, 0.0, 0.0], [tol, 100.0, -100.0], [nxt, 100.0, -100.0], [-200.0, 0.0, 0.0],
                      [float(np.nextafter(-200.0, -np.inf)), 0.0, 0.0], [-1.0, 3.0, 5.0]])
        ref = pc.hull_exact_reference(P, E, tol)
        assert list(ref) == [True, False, True, False, True, tol > 0.0, True]
        rc, o = _hull_raw(lib, P, E, tol)
        assert rc == 0, _err(lib)
        assert pc.compare_mask(o.host()[:len(P)], ref) == [], tol


def test_hull_mask_float_hull_agrees_wherever_the_margins_decide(lib):
    case = pc.hull_float_case()
    P, E, tol = case["points"], case["eq"], case["tol"]
    inside, und = pc.hull_float_reference(P, E, tol)
    rc, o = _hull_raw(lib, P, E, tol)
    assert rc == 0, _err(lib)
    got = o.host()[:len(P)]
    differ = int(((got != 0) != inside)[~und].sum())
    _float_hull.update(facets=len(E), n=len(P), inside=int(inside.sum()), undecided=int(und.sum()), differ=differ)
    print(f"hull_mask float hull: {len(E)} facets in {pc.cdiv(len(E), pc.HULL_CHUNK)} chunks, {len(P)} points, {int(und.sum())} undecided, "
          f"{differ} decided points differ")
    assert und.mean() <= pc.UNDECIDED_CAP
    assert pc.compare_mask(got, inside, und) == []
    rc, o2 = _hull_raw(lib, P, E, tol)
    assert rc == 0 and np.array_equal(o2.host(), o.host())


def test_hull_mask_non_finite_points_are_outside(lib):
    case = pc.hull_exact_case("poly_f611_n513")
    P = np.zeros((3 * 3 + 1, 3))
    for c in range(3):
        for j, v in enumerate((np.nan, np.inf, -np.inf)):
            P[3 * c + j, c] = v
    rc, o = _hull_raw(lib, P, case["eq"], case["tol"])
    assert rc == 0, _err(lib)
    assert list(o.host()[:10]) == [0] * 9 + [1]


def test_hull_mask_a_nan_facet_is_as_if_not_in_the_list(lib):
    """The documented limit of include/mvf.h: the equations must be finite; a row of NaN constrains nothing, wherever it sits."""
    case = pc.hull_exact_case("poly_f257_n513")
    P, E, tol = case["points"], case["eq"], case["tol"]
    ref = pc.hull_exact_reference(P, E, tol)
    for at in (0, 255, 256, len(E)):
        rc, o = _hull_raw(lib, P, np.insert(E, at, np.nan, axis=0), tol)
        assert rc == 0, _err(lib)
        assert pc.compare_mask(o.host()[:len(P)], ref) == [], at


def test_hull_mask_of_no_points_and_refusals(lib):
    case = pc.hull_exact_case("cube_n255")
    P, E = case["points"], case["eq"]
    rc, o = _hull_raw(lib, P, E, 0.0, n=0, points=False, eq=False, out=False)
    assert rc == 0, _err(lib)
    rc, o = _hull_raw(lib, P, E, 0.0, n=0)
    assert rc == 0 and o.untouched()
    for kw, msg in ((dict(nf=0), b"at least one facet"), (dict(n=-1), b"need n >= 0"), (dict(tol=float("nan")), b"bad tolerance"),
                    (dict(tol=float("inf")), b"bad tolerance"), (dict(tol=float("-inf")), b"bad tolerance"),
                    (dict(points=False), b"null pointer"), (dict(eq=False), b"null pointer"), (dict(out=False), b"null pointer")):
        a = dict(tol=0.0)
        a.update(kw)
        rc, o = _hull_raw(lib, P, E, a.pop("tol"), **a)
        assert rc != 0 and b"mvf_hull_mask" in _err(lib) and msg in _err(lib), (kw, _err(lib))
        assert o.untouched()
