"""Cases, references and comparison functions for the kernel-level tests of ``csrc/mvf_prep.hip`` (``mvf_unique_rows``,
``mvf_knn_rowsum``, ``mvf_hull_mask``) and ``csrc/mvf_conk.hip`` (``mvf_con_k``, ``mvf_con_k_d``).  Pure NumPy, importable
without a GPU; tests/test_prep_kernel_refs.py proves the references on the CPU and shows that every comparison function bites,
tests/test_gpu_prep_kernels.py and tests/test_gpu_conk_kernels.py use them on the device.

Every case table maps a name to its shape and to the branch of the code it is there for (``branch``).  Geometry restated from
the sources: the radix sort and the compaction work on chunks of RS_CHUNK = 4096 rows in sub-tiles of 256, the table scan on
segments of SCAN_SEG = 4096 entries (a histogram table has 256 entries per chunk: two segments from 17 chunks on; the segment
sums are scanned by one workgroup of 256 lanes, ``per`` = ceil(segments / 256) each: ``per`` = 2 needs more than 256 segments =
more than 4096 chunks, which is also the size from which the compaction's own table has two segments); the hull kernel stages
HULL_CHUNK = 256 facets at a time; the kNN kernel sorts the next power of two >= m (>= 2) distances in LDS and lane t of 256
sums ranks 1 + t, 1 + t + 256, ...; con_K takes the row form when RS in {1, 2, 4} rows are a multiple of 64 bytes and RS m <=
256 VEC 8 elements (VEC = 4 float32 / 2 float64; NP = ceil(RS m / (256 VEC)) passes), else the flat form in float32 (3 m
elements of LDS <= 80 KB, raised limit above 64 KB) or the 2-D form.

Bounds.  unique_rows, hull_mask on the exact cases and con_k_d's differences are exact: no tolerance.  knn: the bound of
``knn_bound`` is derived (see there).  con_K: the project's own 1e-11 (float64) / 2e-5 (float32) absolute, the figures
tests/test_gpu_kernels.py and tests/test_gpu_highd_kernels.py assert.  hull_mask on the float hull: every point that is not
*undecided* (``hull_float_reference``) must agree with the np.longdouble margins."""
import functools
import math
from fractions import Fraction

import numpy as np

RS_CHUNK, SCAN_SEG, RS_BINS, HULL_CHUNK = 4096, 4096, 256, 256
U2 = 2.0 ** -53
VEC = {"float32": 4, "float64": 2}
CONK_TOL = {"float64": 1e-11, "float32": 2e-5}
CONK_FLAT_LDS_MAX = 80 * 1024


def cdiv(a, b):
    return -(-a // b)


# =========================================================================================================== unique_rows
UNIQUE_SIZES = (1, 2, 255, 256, 257, 4095, 4096, 4097, 8193, 65537)
LARGE_N, LARGE_A = 4097 * 4096 + 1, 1_000_003


def _ints(n, d, seed):
    """(n, d) small integers as float64: about n / 2 distinct rows, ties in every leading column."""
    rng = np.random.default_rng(seed)
    v = max(2, int(round((n / 2) ** (1.0 / d))) + 1)
    return rng.integers(0, v, size=(n, d)).astype(np.float64)


def _tied_columns(d, seed, n=5000):
    """n rows of d columns with two or three distinct values per column, drawn from 1500 base rows (so most rows have exact
    copies) and a tenth of them changed in the LAST column only: ties run through every column before it."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 2 + d % 2, size=(1500, d)).astype(np.float64)
    X = base[rng.integers(0, len(base), n)].copy()
    flip = rng.integers(0, n, n // 10)
    X[flip, d - 1] = 7.0 - X[flip, d - 1]
    return X


def _key_order():
    big, tiny = np.finfo(np.float64).max, 5e-324
    sub = float(np.nextafter(np.finfo(np.float64).tiny, 0.0))  # the largest subnormal
    vals = [-big, big, -1.5, 2.5, -0.0, 0.0, -0.0, 0.0, tiny, -tiny, sub, -sub, 1.0, float(np.nextafter(1.0, 2.0)),
            float(np.nextafter(1.0, 0.0)), -1.0, float(np.nextafter(-1.0, -2.0)), float(np.nextafter(-1.0, 0.0)), 1e300,
            float(np.nextafter(1e300, np.inf)), 3.0, -3.0, np.finfo(np.float64).tiny, -np.finfo(np.float64).tiny]
    rng = np.random.default_rng(11)
    return np.array(vals + [vals[i] for i in rng.permutation(len(vals))], dtype=np.float64).reshape(-1, 1)


def _one_byte(b, n=4097):
    """n keys that differ in byte b of the float64 only (finite, never zero): the radix pass of that byte decides alone."""
    rng = np.random.default_rng(100 + b)
    digit = rng.integers(0, 256, n).astype(np.uint64)
    if b == 7:  # sign and seven exponent bits: the rest keeps the exponent off all-ones and the value off zero
        bits = (digit << np.uint64(56)) | np.uint64(0x0010000000000001)
    else:
        bits = np.uint64(0x40 << 56) | (digit << np.uint64(8 * b))
    X = bits.view(np.float64).reshape(-1, 1).copy()
    assert np.isfinite(X).all() and (X != 0).all()
    return X


def _dup_first_last(n=4097, k=4):
    """Every row k times, in DESCENDING order of value along the memory: the first occurrence of the smallest row is among the
    largest indices, and a sort that is not stable (or a compaction that keeps the last of a run) returns another index."""
    v = (n - 1 - np.arange(n)) // k
    return np.stack([v, v % 7], axis=1).astype(np.float64)


def _build_unique_cases():
    cases = {}
    for n in UNIQUE_SIZES:
        for d in (1, 3):
            branch = {255: "last sub-tile partial", 256: "one full sub-tile", 257: "second sub-tile of one lane",
                      4095: "last lane of the chunk idle", 4096: "one full chunk", 4097: "second chunk of one row",
                      8193: "three chunks", 65537: "17 chunks: histogram table of two scan segments"}.get(n, "smallest sizes")
            cases[f"n{n}_d{d}"] = (functools.partial(_ints, n, d, 1000 * d + n % 997), branch)
    for d in (2, 5, 8, 16):
        cases[f"n5000_d{d}_tied"] = (functools.partial(_tied_columns, d, d), f"LSD over {d} columns, ties up to the last column")
    n = 4097
    cases["n4097_d2_all_equal"] = (lambda: np.full((n, 2), 3.25), "one run: count = 1, uid = 0")
    cases["n4097_d2_increasing"] = (lambda: np.stack([np.arange(n) // 64, np.arange(n) % 64], 1).astype(np.float64),
                                    "already sorted, all distinct")
    cases["n4097_d2_decreasing"] = (lambda: np.stack([np.arange(n) // 64, np.arange(n) % 64], 1).astype(np.float64)[::-1].copy(),
                                    "reversed, all distinct")
    cases["n4097_d2_dup4_first_last"] = (_dup_first_last, "first-occurrence contract (stability of every pass)")
    cases["key_order_d1"] = (_key_order, "order-preserving key: signs, zeros, subnormals, DBL_MAX, last-bit pairs (first zero -0.0)")
    cases["key_order_d1_negated"] = (lambda: -_key_order(), "the same, every sign flipped (first zero +0.0)")
    for b in range(8):
        cases[f"n4097_d1_byte{b}"] = (functools.partial(_one_byte, b), f"radix pass {b} decisive on its own")
    return cases


_UNIQUE = _build_unique_cases()
UNIQUE_NAMES = tuple(_UNIQUE)
UNIQUE_BRANCH = {name: branch for name, (_, branch) in _UNIQUE.items()}
UNIQUE_BRANCH["large_n16781313_d1"] = ("4098 chunks: per = 2 in scan_segoff_kernel (257 histogram segments), two segments in the "
                                       "compaction scan; analytic reference")


@functools.lru_cache(maxsize=None)
def unique_case(name):
    return np.ascontiguousarray(_UNIQUE[name][0](), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def unique_reference(name):
    """uid of np.unique(X, axis=0, return_index=True): first occurrence of every distinct row, in lexicographic row order."""
    _, uid = np.unique(unique_case(name), axis=0, return_index=True)
    return uid.astype(np.int64)


def large_case(n=LARGE_N, a=LARGE_A):
    """X[i] = float(((i a) mod n) // 3), one column: every value three times (the last one fewer), scattered over the array."""
    assert math.gcd(a, n) == 1
    i = np.arange(n, dtype=np.int64)
    return ((i * a) % n // 3).astype(np.float64).reshape(-1, 1)


def large_reference(n=LARGE_N, a=LARGE_A):
    """The uid of ``large_case`` without a sort: value v sits at the rows i with (i a) mod n in {3v, 3v + 1, 3v + 2}, that is
    i = (3v + r) a^-1 mod n, and np.unique returns the smallest of them; the values 0 .. ceil(n / 3) - 1 are already in order."""
    ainv = pow(a, -1, n)
    v = np.arange(cdiv(n, 3), dtype=np.int64)
    uid = np.full(len(v), n, dtype=np.int64)
    for r in range(3):
        t = 3 * v + r
        i = (t % n) * ainv % n   # < n^2 < 2^49
        uid = np.where(t < n, np.minimum(uid, i), uid)
    return uid


def ordered_key(x):
    """The kernel's order-preserving 64-bit image of a float64 column (-0.0 takes the key of +0.0)."""
    x = np.where(x == 0.0, 0.0, np.asarray(x, dtype=np.float64))
    u = np.ascontiguousarray(x).view(np.uint64)
    return np.where((u >> np.uint64(63)) != 0, ~u, u | np.uint64(1 << 63))


def unique_restated(X, sent_uid, sent_row, last_occurrence=False, skip_byte=None):
    """The kernel's algorithm: LSD over the columns (last first), eight stable 8-bit passes per column on the ordered key,
    run-start flags by VALUE comparison, compaction, gather.  Returns (count, uid, rows) the way the device leaves them: n
    entries each, the sentinel behind ``count``.  Seeded mistakes: ``last_occurrence`` keeps the last row of a run (what an
    unstable sort amounts to), ``skip_byte`` leaves one radix pass out."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    idx = np.arange(n, dtype=np.int64)
    for c in range(d - 1, -1, -1):
        key = ordered_key(X[idx, c])
        for b in range(8):
            if b == skip_byte:
                continue
            o = np.argsort((key >> np.uint64(8 * b)) & np.uint64(255), kind="stable")
            idx, key = idx[o], key[o]
    S = X[idx]
    start = np.ones(n, dtype=bool)
    start[1:] = (S[1:] != S[:-1]).any(axis=1)
    if last_occurrence:
        start = np.append(start[1:], True)
    u = idx[start]
    uid = np.full(n, sent_uid, dtype=np.int64)
    rows = np.full((n, d), sent_row, dtype=np.float64)
    uid[:len(u)] = u
    rows[:len(u)] = X[u]
    return len(u), uid, rows


def compare_unique(X, ref_uid, count, uid, rows, sent_uid, sent_row):
    """Failures (empty: none) of an ``mvf_unique_rows`` result: ``count`` an int, ``uid`` (n,) and ``rows`` (n, d) as the device
    left them in sentinel-filled buffers.  Exact: no tolerance anywhere."""
    X = np.asarray(X)
    n, d = X.shape
    uid, rows = np.asarray(uid).reshape(n), np.asarray(rows).reshape(n, d)
    bad = []
    if int(count) != len(ref_uid):
        return [f"count {int(count)} != {len(ref_uid)}"]
    c = len(ref_uid)
    if not np.array_equal(uid[:c], ref_uid):
        j = int(np.flatnonzero(uid[:c] != ref_uid)[0])
        bad.append(f"uid[{j}] = {uid[j]} != {ref_uid[j]} ({int((uid[:c] != ref_uid).sum())} differ)")
    want = np.ascontiguousarray(X[ref_uid])
    if not np.array_equal(np.ascontiguousarray(rows[:c]).view(np.int64), want.view(np.int64)):
        bad.append("rows[:count] differ from X[uid] by bits")
    if not (uid[c:] == sent_uid).all():
        bad.append("uid written behind count")
    if not (rows[c:] == sent_row).all():
        bad.append("rows written behind count")
    return bad


# ============================================================================================================ knn_rowsum
_SCALES = np.array([300.0, 200.0, 150.0, 100.0, 50.0, 20.0, 10.0, 5.0])


def _ks(m, *more):
    return tuple(sorted({k for k in (2, 257, 258, m, max(2, int(0.2 * m))) + more if 2 <= k <= m}))


def _cloud(m, d, seed):
    return np.random.default_rng(seed).standard_normal((m, d)) * _SCALES[:d]


def _copies():
    X = _cloud(257, 3, 5)
    X[[20, 77, 130, 200, 256]] = X[3]   # five exact copies of point 3: zero distances among the neighbours
    return X


def _lattice():
    g = np.arange(32.0)
    return np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)   # 1024 points: ties at every rank boundary


KNN_CASES = {
    "m2_d1": dict(X=lambda: _cloud(2, 1, 1), ks=_ks(2), branch="np2 = 2: one compare-exchange, 255 idle lanes"),
    "m3_d2": dict(X=lambda: _cloud(3, 2, 2), ks=_ks(3), branch="np2 = 4 with one +inf pad"),
    "m255_d3": dict(X=lambda: _cloud(255, 3, 3), ks=_ks(255), branch="np2 = 256, one pad; k - 1 < 256: some lanes sum nothing"),
    "m256_d4": dict(X=lambda: _cloud(256, 4, 4), ks=_ks(256), branch="np2 = m = 256: no pad, half the lanes per stage"),
    "m257_d5": dict(X=lambda: _cloud(257, 5, 5), ks=_ks(257), branch="np2 = 512: 255 pads; k = 257: every lane one term"),
    "m1023_d6": dict(X=lambda: _cloud(1023, 6, 6), ks=_ks(1023), branch="k = 257 / 258: lane 0 takes its second term at 258"),
    "m1024_d7": dict(X=lambda: _cloud(1024, 7, 7), ks=_ks(1024), branch="np2 = m = 1024"),
    "m1025_d8": dict(X=lambda: _cloud(1025, 8, 8), ks=_ks(1025), branch="np2 = 2048, d = 8: every coordinate slot"),
    "m8192_d2": dict(X=lambda: _cloud(8192, 2, 9), ks=_ks(8192), branch="largest m: 64 KB of LDS, 32 terms per lane at k = m"),
    "m257_d3_copies": dict(X=_copies, ks=_ks(257, 5, 6, 7), branch="five exact copies of one point: several zero distances kept"),
    "m1024_d2_lattice": dict(X=_lattice, ks=_ks(1024, 5, 6, 9, 10), branch="lattice: massive ties at the rank boundary"),
}
KNN_NAMES = tuple(KNN_CASES)


@functools.lru_cache(maxsize=None)
def knn_case(name):
    return np.ascontiguousarray(KNN_CASES[name]["X"](), dtype=np.float64)


def knn_bound(ref, k, d):
    """|rowsum - ref| <= (k + d + 4) 2^-53 ref, derived, not measured: a computed term sqrt(fl(sum of d squares)) carries at
    most (d + 2) / 2 + 1 rounding units (each square two roundings of a relative size the root halves, the d - 1 additions of
    non-negative squares one each, halved too, the root one), and any summation order of k - 1 non-negative terms adds at most
    k - 2 units: k + d / 2 in all, and the reference's own rounded roots and the second-order terms fit in the rest of k + d +
    4.  Where ref = 0 (k - 1 copies of the point) the sum is exactly 0; one subnormal of absolute floor keeps the comparison
    defined."""
    return (k + d + 4) * U2 * np.asarray(ref, dtype=np.float64) + 5e-324


def compare_knn(got, ref, k, d):
    """Largest |got - ref| / bound over the rows: <= 1 passes."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    if not np.isfinite(got).all():
        return math.inf
    diff = np.abs(got.astype(np.longdouble) - ref.astype(np.longdouble))
    return float((diff / knn_bound(ref, k, d).astype(np.longdouble)).max())


def _wave_tree(acc):
    """block_sum<256> of (rows, 256) lane values: wave_sum's shuffle tree (lane l += lane l + o, o = 32 .. 1) in each of the four
    waves, then 0.0 + wave 0 + wave 1 + wave 2 + wave 3."""
    total = np.zeros(acc.shape[0])
    for w in range(4):
        v = acc[:, 64 * w:64 * w + 64].copy()
        o = 32
        while o:
            v = v[:, :o] + v[:, o:2 * o]
            o >>= 1
        total = total + v[:, 0]
    return total


def knn_restated_block(X, lo, hi, ks, skip_rank0=True):
    """{k: rowsum[lo:hi]} the kernel's way: float64 squares added coordinate by coordinate without fma, ascending sort, square
    roots of ranks 1 .. k - 1, lane t summing ranks 1 + t, 1 + t + 256, ... in order, then the wave tree.  ``skip_rank0=False``
    is the seeded mistake "rank 0 not skipped": ranks 0 .. k - 2."""
    m, d = X.shape
    s2 = np.zeros((hi - lo, m))
    for c in range(d):
        df = X[lo:hi, c, None] - X[None, :, c]
        s2 = s2 + df * df
    s2.sort(axis=1)
    rt = np.sqrt(s2)
    first = 1 if skip_rank0 else 0
    out = {}
    for k in ks:
        terms = rt[:, first:first + k - 1]
        pad = (-terms.shape[1]) % 256
        terms = np.concatenate([terms, np.zeros((hi - lo, pad))], axis=1).reshape(hi - lo, -1, 256)
        acc = np.zeros((hi - lo, 256))
        for r in range(terms.shape[1]):
            acc = acc + terms[:, r]
        out[k] = _wave_tree(acc)
    return out


def exact_row_sums(a):
    """math.fsum of every row of a non-negative float64 array, that is the exact sum rounded once.  A row whose entries are all
    multiples of 2^-72 below 2^20 is summed as three integer limbs (20 + 26 + 26 binary places, each limb's sum exact in
    int64) and divided once as Python integers, which rounds correctly; any other row goes through math.fsum itself."""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(len(a))
    for i0 in range(0, len(a), 8):          # (a few rows at a time: the temporaries stay in the cache)
        b = a[i0:i0 + 8]
        s = b * 2.0 ** 20                   # a power of two: exact
        hi = np.floor(s)
        r = (s - hi) * 2.0 ** 26            # the fraction, < 1: exact, and so is the shift
        mid = np.floor(r)
        lo = (r - mid) * 2.0 ** 26
        ok = (lo == np.floor(lo)).all(axis=1) & (hi < 2.0 ** 40).all(axis=1) & (b.shape[1] <= 2 ** 22)
        A, B, C = hi.astype(np.int64).sum(axis=1), mid.astype(np.int64).sum(axis=1), lo.astype(np.int64).sum(axis=1)
        for i in range(len(b)):
            out[i0 + i] = ((int(A[i]) << 52) + (int(B[i]) << 26) + int(C[i])) / (1 << 72) if ok[i] else math.fsum(b[i].tolist())
    return out


def knn_reference_block(X, lo, hi, ks):
    """{k: ref[lo:hi]}: squared distances in np.longdouble from the float64 inputs, the k - 1 smallest after the smallest of the
    row (rank 0, the point itself) is dropped, each square root rounded to float64, summed as math.fsum sums (``exact_row_sums``).  (Rounding is
    monotone, so the k - 1 smallest rounded roots are the rounded roots of the k - 1 smallest; fsum does not depend on order.)"""
    m, d = X.shape
    Xl = X.astype(np.longdouble)
    rt = np.empty((hi - lo, m))
    for a in range(lo, hi, 16):   # (16 rows at a time: the longdouble temporaries stay in the cache)
        b = min(hi, a + 16)
        d2 = np.zeros((b - a, m), dtype=np.longdouble)
        for c in range(d):
            df = Xl[a:b, c, None] - Xl[None, :, c]
            df *= df
            d2 += df
        rt[a - lo:b - lo] = np.sqrt(d2)
    partial = [k for k in ks if k < m]
    out = {}
    if partial:
        kk = max(partial)
        head = np.sort(np.partition(rt, kk - 1, axis=1)[:, :kk], axis=1)
        for k in partial:
            out[k] = exact_row_sums(head[:, 1:k])
    if m in ks:   # everything but the smallest of the row: a zero in its place leaves the exact sum alone
        rt[np.arange(hi - lo), rt.argmin(axis=1)] = 0.0
        out[m] = exact_row_sums(rt)
    return out


RESTATED_ROWS = 1024   # the order-following restatement (reporting only) covers the first rows of a larger case


@functools.lru_cache(maxsize=None)
def knn_tables(name):
    """{k: (reference (m,), order-following restatement of the first min(m, RESTATED_ROWS) rows)} of a case, float64."""
    X, ks = knn_case(name), KNN_CASES[name]["ks"]
    m = len(X)
    mr = min(m, RESTATED_ROWS)
    ref = {k: np.empty(m) for k in ks}
    res = {k: np.empty(mr) for k in ks}
    step = 512
    for lo in range(0, m, step):
        hi = min(m, lo + step)
        a = knn_reference_block(X, lo, hi, ks)
        b = knn_restated_block(X, lo, hi, ks) if lo < mr else None
        for k in ks:
            ref[k][lo:hi] = a[k]
            if b is not None:
                res[k][lo:hi] = b[k]
    return {k: (ref[k], res[k]) for k in ks}


# ============================================================================================================= hull_mask
POSITIONS = (0, 255, 256, 511, 512, -1)   # where the one violated facet sits in the list (-1: the last one)


def _primitive_normals(limit=5):
    r = range(-limit, limit + 1)
    v = [(a, b, c) for a in r for b in r for c in r if math.gcd(math.gcd(abs(a), abs(b)), abs(c)) == 1]
    v.sort(key=lambda n: (n[0] ** 2 + n[1] ** 2 + n[2] ** 2, n))
    return v


POLY_FACETS = 611   # three staging chunks, the last one of 99 facets
_POLY = _primitive_normals()[:POLY_FACETS]
_CUBE = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
_OCTA = [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]


def _bezout(nrm):
    """A small integer u with n . u = 1 (n primitive)."""
    r = range(-5, 6)
    best = min(((a, b, c) for a in r for b in r for c in r if nrm[0] * a + nrm[1] * b + nrm[2] * c == 1),
               key=lambda u: u[0] ** 2 + u[1] ** 2 + u[2] ** 2)
    return np.array(best, dtype=np.int64)


def exact_hull_case(normals, radius, q, tol_units, n, seed, n_boundary=40):
    """Integer facet equations n . x - h <= 0 with h = ceil(radius |n|) and n points on the grid of 1 / q (q = 1 or 4), tol =
    tol_units / q: points with margin exactly tol on some facet (next to the facet's centre, so that many of them are inside), the
    same one grid step further out along that facet, and uniform ones in 1.4 x the radius.  Every product and partial sum of the
    kernel's three fma steps is a multiple of 1 / q below 2^20: exact."""
    rng = np.random.default_rng(seed)
    N = np.array(normals, dtype=np.int64)
    h = np.array([math.isqrt(radius * radius * int(v @ v) - 1) + 1 for v in N], dtype=np.int64)   # ceil(radius |n|)
    pts = []
    for f in rng.permutation(len(N))[:n_boundary]:
        u = _bezout(N[f])
        p0 = np.rint(q * h[f] / float(N[f] @ N[f]) * N[f]).astype(np.int64)
        p = p0 + (q * h[f] + tol_units - int(N[f] @ p0)) * u
        assert int(N[f] @ p) - q * h[f] == tol_units
        pts += [p, p + u]
    box = int(1.4 * radius * q)
    pool = np.array(pts, dtype=np.int64).reshape(-1, 3)
    P = np.concatenate([pool, rng.integers(-box, box + 1, size=(max(0, n - len(pool)), 3))])[:n]
    eq = np.concatenate([N, -h[:, None]], axis=1).astype(np.float64)
    return dict(points=np.ascontiguousarray(P / float(q)), eq=np.ascontiguousarray(eq), tol=tol_units / float(q))


def _one_facet_case(pos):
    """The 611-facet polytope with facet (1, 0, 0) moved to position ``pos`` of the list and 257 points of which the first,
    (1001, 0, 0), violates that facet and no other."""
    normals = [v for v in _POLY if v != (1, 0, 0)]
    pos = len(normals) if pos < 0 else pos
    normals.insert(pos, (1, 0, 0))
    case = exact_hull_case(normals, 1000, 1, 0, 257, 50 + pos)
    case["points"][0] = (1001.0, 0.0, 0.0)
    return case


def corner_box():
    """A box with one facet through the origin, (1, 0, 0 | 0): the margin of (x, 0, 0) on it is x itself, so a point sits at
    margin exactly tol and at nextafter(tol, inf) for tol = 2, 1 / 4 and 0 (where the next value is the smallest subnormal)."""
    return np.array([[1, 0, 0, 0], [-1, 0, 0, -200], [0, 1, 0, -100], [0, -1, 0, -100], [0, 0, 1, -100], [0, 0, -1, -100]], dtype=np.float64)


HULL_EXACT = {
    "cube_n255": dict(make=lambda: exact_hull_case(_CUBE, 100, 1, 2, 255, 1, 6), branch="6 facets, tol = 2 (integer)"),
    "octahedron_n513": dict(make=lambda: exact_hull_case(_OCTA, 150, 4, 1, 513, 2, 8), branch="8 facets, tol = 1 / 4, three workgroups"),
    "poly_f1_n1": dict(make=lambda: exact_hull_case(_POLY[:1], 1000, 1, 2, 1, 3, 1), branch="one facet, one point at margin = tol"),
    "poly_f4_n255": dict(make=lambda: exact_hull_case(_POLY[:4], 1000, 1, 0, 255, 4, 4), branch="4 facets, tol = 0"),
    "poly_f255_n256": dict(make=lambda: exact_hull_case(_POLY[:255], 1000, 1, 2, 256, 5), branch="one partial staging chunk"),
    "poly_f256_n257": dict(make=lambda: exact_hull_case(_POLY[:256], 1000, 4, 1, 257, 6), branch="one full staging chunk, tol = 1 / 4"),
    "poly_f257_n513": dict(make=lambda: exact_hull_case(_POLY[:257], 1000, 1, 2, 513, 7), branch="second chunk of one facet"),
    "poly_f611_n513": dict(make=lambda: exact_hull_case(_POLY, 1000, 1, 2, 513, 8), branch="three facet chunks, the last of 99"),
}
for _pos in POSITIONS:
    HULL_EXACT[f"poly_f611_one_violated_at_{'last' if _pos < 0 else _pos}"] = dict(
        make=functools.partial(_one_facet_case, _pos), branch=f"only the facet at position {'nfacets - 1' if _pos < 0 else _pos} decides")
HULL_EXACT_NAMES = tuple(HULL_EXACT)


@functools.lru_cache(maxsize=None)
def hull_exact_case(name):
    return HULL_EXACT[name]["make"]()


def _as_ints(*arrays):
    """The float arrays as Python integers over one common power-of-two denominator (exact)."""
    fr = [[Fraction(float(v)) for v in np.asarray(a, dtype=np.float64).ravel()] for a in arrays]
    den = max(f.denominator for part in fr for f in part)
    return [np.array([f.numerator * (den // f.denominator) for f in part], dtype=object).reshape(np.shape(a))
            for part, a in zip(fr, arrays)] + [den]


def hull_exact_margins(points, eq):
    """(n, nfacets) margins n_f . p + d_f as Python integers in units of 1 / (dp de) and the two denominators: exact."""
    P, dp = _as_ints(points)
    E, de = _as_ints(eq)
    return P.dot(E[:, :3].T) + E[:, 3][None, :] * dp, dp, de


def hull_exact_reference(points, eq, tol, drop=None):
    """inside[i] = (max over facets of the exact margin <= tol), in Python integer arithmetic.  ``drop``: the seeded mistake
    of a facet left out."""
    M, dp, de = hull_exact_margins(points, eq)
    if drop is not None:
        M = np.delete(M, drop, axis=1)
    t = Fraction(float(tol)) * dp * de
    return np.array([max(row) <= t for row in M], dtype=bool)


def check_fma_exact(points, eq):
    """Every value the three fma steps of the kernel form on this case is a float64: the partial sums d + n_z p_z, + n_y p_y,
    + n_x p_x, as exact rationals, survive a round trip through float (on an even sample of 4096 (point, facet) pairs per step;
    the builder bounds them all: multiples of 1 / q below 2^20)."""
    P, dp = _as_ints(points)
    E, de = _as_ints(eq)
    acc = np.repeat((E[:, 3] * dp)[None, :], len(P), axis=0)
    for c in (2, 1, 0):
        acc = acc + np.outer(P[:, c], E[:, c])
        if not all(Fraction(float(Fraction(int(v), dp * de))) == Fraction(int(v), dp * de) for v in acc.ravel()[:: max(1, acc.size // 4096)]):
            return False
    return True


@functools.lru_cache(maxsize=None)
def hull_float_case(n_vertices=400, n_points=4099, seed=7):
    """A ConvexHull of points on the ellipsoid 300 / 200 / 150 (every point a vertex) and query points that are random convex
    combinations of a facet's vertices pushed along the facet's normal by s tol, s in {-3, -1.5, 0.5, 0.9, 1.1, 1.5, 3}; tol is
    the API's 100 eps x extent."""
    from scipy.spatial import ConvexHull

    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n_vertices, 3))
    V = v / np.linalg.norm(v, axis=1, keepdims=True) * np.array([300.0, 200.0, 150.0])
    hull = ConvexHull(V)
    assert len(hull.vertices) == n_vertices
    eq = np.ascontiguousarray(hull.equations)
    tol = 100.0 * np.finfo(np.float64).eps * float(np.max(hull.max_bound - hull.min_bound))
    f = rng.integers(0, len(eq), n_points)
    w = rng.dirichlet(np.ones(3), n_points)
    s = rng.choice(np.array([-3.0, -1.5, 0.5, 0.9, 1.1, 1.5, 3.0]), n_points)
    P = (w[:, :, None] * V[hull.simplices[f]]).sum(axis=1) + (s * tol)[:, None] * eq[f, :3]
    return dict(points=np.ascontiguousarray(P), eq=eq, tol=tol, s=s, vertices=V)


def hull_float_reference(points, eq, tol):
    """(inside, undecided) from np.longdouble margins.  A point is undecided when for some facet |margin - tol| <= 2^-51 (|n_x p_x|
    + |n_y p_y| + |n_z p_z| + |d_f|): three roundings of the kernel's fma chain (<= 3 x 2^-53 of that sum) with room to spare."""
    P, E = np.asarray(points, dtype=np.longdouble), np.asarray(eq, dtype=np.longdouble)
    inside = np.ones(len(P), dtype=bool)
    und = np.zeros(len(P), dtype=bool)
    for lo in range(0, len(P), 512):
        p = P[lo:lo + 512]
        prod = p[:, None, :] * E[None, :, :3]
        margin = prod.sum(axis=2) + E[None, :, 3]
        scale = np.abs(prod).sum(axis=2) + np.abs(E[None, :, 3])
        inside[lo:lo + 512] = (margin <= tol).all(axis=1)
        und[lo:lo + 512] = (np.abs(margin - tol) <= np.longdouble(2.0 ** -51) * scale).any(axis=1)
    return inside, und


UNDECIDED_CAP = 0.01


def compare_mask(got, ref, undecided=None):
    """Failures (empty: none) of a mask: every byte 0 or 1, equal to the reference at every decided point."""
    got = np.asarray(got)
    bad = []
    if not np.isin(got, (0, 1)).all():
        bad.append("a byte that is neither 0 nor 1")
    diff = got.astype(bool) != np.asarray(ref, dtype=bool)
    if undecided is not None:
        diff &= ~np.asarray(undecided, dtype=bool)
    if diff.any():
        bad.append(f"{int(diff.sum())} points differ, first at {int(np.flatnonzero(diff)[0])}")
    return bad


# ================================================================================================================= con_K
NP_DTYPE = {"float32": np.float32, "float64": np.float64}
CONK_BETA = 0.3


def conk_points(n, m, d, dtype, seed=0):
    """(x, y) in the cell dtype: standard normal, so that exp(-0.3 r^2) spreads over (0, 1]."""
    rng = np.random.default_rng(1000 * d + 7 * n + m + seed)
    return rng.standard_normal((n, d)).astype(NP_DTYPE[dtype]), rng.standard_normal((m, d)).astype(NP_DTYPE[dtype])


def conk_reference(x, y, beta):
    """exp(-beta ||x - y||^2) in np.longdouble on the inputs as given (already rounded to the cell dtype), (n, m) longdouble."""
    xl, yl = np.asarray(x).astype(np.longdouble), np.asarray(y).astype(np.longdouble)
    r2 = np.zeros((len(xl), len(yl)), dtype=np.longdouble)
    for c in range(xl.shape[1]):
        df = xl[:, c, None] - yl[None, :, c]
        r2 += df * df
    return np.exp(-np.longdouble(beta) * r2)


def conk_restated(x, y, beta, shift_column=None):
    """The reference rounded to the cell dtype; ``shift_column = j``: the seeded mistake of column j holding column j + 1."""
    K = conk_reference(x, y, beta).astype(np.asarray(x).dtype)
    if shift_column is not None:
        K[:, shift_column] = K[:, shift_column + 1]
    return K


def compare_conk(got, ref):
    """Largest absolute deviation of a (n, m) result from the longdouble reference (inf for a non-finite entry)."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return math.inf
    return float(np.abs(got.astype(np.longdouble) - ref).max()) if got.size else 0.0


def conk_diff_reference(x, y):
    """D[i, :, j] = x_i - y_j in the cell dtype: one IEEE subtraction per element, exact to the bit."""
    return np.ascontiguousarray(x[:, :, None] - y.T[None])


def conk_row_plan(m, dtype):
    """(RS, fits, NP) of launch_conk's own arithmetic at d = 3."""
    size, vec = NP_DTYPE[dtype]().itemsize, VEC[dtype]
    rs = 1
    while rs < 4 and (rs * m * size) % 64 != 0:
        rs *= 2
    fits = m % vec == 0 and m >= 64 and (rs * m * size) % 64 == 0 and rs * m <= 256 * vec * 8
    return rs, fits, cdiv(rs * m, 256 * vec)


def conk_flat_fits(m, dtype):
    return m % VEC[dtype] == 0 and m >= 64 and 3 * m * NP_DTYPE[dtype]().itemsize <= CONK_FLAT_LDS_MAX


def _row_ns(rs):
    return tuple(sorted({1, 35, rs + 1} | ({rs - 1} if rs > 1 else set())))


def _build_conk_cases():
    rows, flat = {}, {}
    table = {("float32", 1): ((64, 1024, 1040, 8192), 8208), ("float32", 2): ((72, 4088), 4104), ("float32", 4): ((68, 2044), 2052),
             ("float64", 1): ((64, 4096), 4104), ("float64", 2): ((68, 2044), 2052), ("float64", 4): ((66, 1022), 1026)}
    for (dtype, rs), (ms, over) in table.items():
        for m in ms + (over,):
            prs, fits, npass = conk_row_plan(m, dtype)
            assert prs == rs and fits == (m != over), (dtype, rs, m, prs, fits)
            if fits:
                branch = f"row form RS = {rs}, NP = {npass}"
            elif conk_flat_fits(m, dtype) and dtype == "float32":
                branch = f"first m past the row form at RS = {rs}: flat form by default"
            else:
                branch = f"first m past the row form at RS = {rs}: 2-D form by default" + (
                    " and under conk_form = 2 (past the flat form's LDS limit too)" if not conk_flat_fits(m, dtype) else "")
            rows[f"{dtype}_rs{rs}_m{m}"] = dict(dtype=dtype, m=m, ns=_row_ns(rs), rs=rs, fits=fits, np=npass, branch=branch)
    for dtype, ms in (("float32", (64, 5464, 6824, 6828)), ("float64", (64, 2732, 3412, 3414))):
        size = NP_DTYPE[dtype]().itemsize
        for m in ms:
            lds = 3 * m * size
            if not conk_flat_fits(m, dtype):
                branch = f"3 m elements = {lds} B > 80 KB: conk_form = 2 takes the 2-D form"
            else:
                branch = f"flat form, {lds} B of LDS " + ("(above 64 KB: raised limit)" if lds > 65536 else "(below 64 KB)")
            flat[f"{dtype}_flat_m{m}"] = dict(dtype=dtype, m=m, ns=(1, 7), branch=branch)
    return rows, flat


CONK_ROW_CASES, CONK_FLAT_CASES = _build_conk_cases()


def conk_2d_ms(dtype):
    v = VEC[dtype]
    return tuple(dict.fromkeys((1, v - 1, v + 1, 256 * v - 1, 256 * v + 1)))   # scalar tail, one block +- one column


CONK_2D_NS = (31, 32, 33)
CONK_D_MS, CONK_D_NS = (1, 255, 256, 257), (1, 3)
