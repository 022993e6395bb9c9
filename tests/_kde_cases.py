"""Cases, float64 NumPy restatement and bounds for ``csrc/mvf_kde.hip`` (``tdr.kernel_density`` / ``pc_KDE``).

The restatement is sklearn's own arithmetic spelled out: explicit coordinate differences, ``dist = sqrt(dx dx + dy dy + dz dz)``,
the six ``log K(dist, h)`` of ``sklearn.neighbors.KernelDensity`` with its strict support ``dist < h``, ``log w + log K``,
a log-sum-exp per (target, group) and the constants ``log_norm(h, d, kernel) - log(sum of the group's weights)``.
tests/test_kde_kernel_refs.py proves it against sklearn and against tests/golden/ref_kde.npz on the CPU; the GPU suites use the
restatement and the golden only (sklearn need not be there).

Geometry of the kernel, as ``mvf_kde.hip`` states it: a workgroup owns TILE = 256 targets and reads the sources in tiles of 256;
the sources are split over workgroups, at least MIN_CHUNK = 4096 per split and about TARGET_WGS = 1024 workgroups per column, the
split a function of (n, N) alone; one call takes at most MAX_COLUMNS = 64 columns.

Bound of a case (tests/test_sample_kernel_refs.py's margin for float64 restatements): per entry
``max(ALLOW x max(dev_order, dev_sklearn), FLOOR_ULP ulp) x max(1, |ref|)`` with dev_order the deviation between the restatement
summed in source order and in reversed order, dev_sklearn the deviation between the restatement and sklearn (recorded in the
golden by make_golden_kde.py, where sklearn is), both as max |a - b| / max(1, |ref|) over the finite entries.  -inf must match
exactly.  float32 mode: the reference is evaluated on the float32-rounded centred coordinates, so the same bound holds."""
import functools
import math
import os

import numpy as np

TILE, MIN_CHUNK, TARGET_WGS, MAX_COLUMNS = 256, 4096, 1024, 64
ALLOW, FLOOR_ULP = 64.0, 16.0
EPS = float(np.finfo(np.float64).eps)
KERNELS = ("gaussian", "exponential", "tophat", "epanechnikov", "linear", "cosine")
CODES = {k: i for i, k in enumerate(KERNELS)}
COMPACT = ("tophat", "epanechnikov", "linear", "cosine")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_kde.npz")
MARGIN = 1e-9   # no pair distance of a compact case lies within this (relative) of h


def splits(n, N):
    """The number of source splits mvf_kde takes (its kde_chunk, restated)."""
    cd = lambda a, b: -(-a // b)  # noqa: E731
    s = max(1, min(cd(N, MIN_CHUNK), cd(TARGET_WGS, cd(n, TILE))))
    chunk = cd(cd(N, s), TILE) * TILE
    return cd(N, chunk)


# ------------------------------------------------------------------------------------------------------------ the constants
def log_vn(n):
    return 0.5 * n * math.log(math.pi) - math.lgamma(0.5 * n + 1)


def log_sn(n):
    return math.log(2 * math.pi) + log_vn(n - 1)


def log_norm(h, d, kernel):
    """log of 1 / (h^d x the integral of K over R^d)."""
    if kernel == "gaussian":
        f = 0.5 * d * math.log(2 * math.pi)
    elif kernel == "tophat":
        f = log_vn(d)
    elif kernel == "epanechnikov":
        f = log_vn(d) + math.log(2.0 / (d + 2.0))
    elif kernel == "exponential":
        f = log_sn(d - 1) + math.lgamma(d)
    elif kernel == "linear":
        f = log_vn(d) - math.log(d + 1.0)
    else:
        # int_0^1 cos(pi r / 2) r^(d-1) dr = 2/pi (d = 1) and 2/pi - 16/pi^3 (d = 3).  For d = 2 the integral is 2/pi - 4/pi^2,
        # but sklearn's series (_log_kernel_norm: steps of two in k, exact for odd d only) stops at 2/pi - and the columns must
        # equal sklearn's, so its value stands here
        integral = {1: 2 / math.pi, 2: 2 / math.pi, 3: 2 / math.pi - 16 / math.pi**3}[d]
        f = math.log(integral) + log_sn(d - 1)
    return -f - d * math.log(h)


# ---------------------------------------------------------------------------------------------------------- the restatement
def _log_k(dist, h, kernel):
    with np.errstate(divide="ignore", invalid="ignore"):
        if kernel == "gaussian":
            return -0.5 * (dist * dist) / (h * h)
        if kernel == "exponential":
            return -dist / h
        inside = dist < h
        if kernel == "tophat":
            v = np.zeros_like(dist)
        elif kernel == "epanechnikov":
            v = np.log(1.0 - (dist * dist) / (h * h))
        elif kernel == "linear":
            v = np.log(1.0 - dist / h)
        else:
            v = np.log(np.cos(0.5 * np.pi * dist / h))
        return np.where(inside, v, -np.inf)


def pair_dist(T, X):
    T3, X3 = np.zeros((len(T), 3), dtype=T.dtype), np.zeros((len(X), 3), dtype=X.dtype)
    T3[:, : T.shape[1]], X3[:, : X.shape[1]] = T, X
    dx, dy, dz = (T3[:, None, k] - X3[None, :, k] for k in range(3))
    return np.sqrt(dx * dx + dy * dy + dz * dz)


def raw_log_sums(T, X, kernel, h, w=None, g=None, C=1, reverse=False, rows=512):
    """(n, C): log sum_{j in group c} w_j K(|t_i - x_j| / h), unnormalised; -inf where nothing with w > 0 is in reach."""
    n, N = len(T), len(X)
    out = np.full((n, C), -np.inf, dtype=T.dtype)
    g = np.zeros(N, dtype=np.int64) if g is None else np.asarray(g)
    with np.errstate(divide="ignore"):
        lw = np.zeros(N, dtype=T.dtype) if w is None else np.log(np.asarray(w, dtype=T.dtype))
    for c in range(C):
        idx = np.flatnonzero(g == c)
        if reverse:
            idx = idx[::-1]
        if len(idx) == 0:
            continue
        for lo in range(0, n, rows):
            a = _log_k(pair_dist(T[lo : lo + rows], X[idx]), h, kernel) + lw[idx][None, :]
            m = a.max(axis=1)
            ok = np.isfinite(m)
            s = np.exp(a[ok] - m[ok, None]).sum(axis=1)
            out[lo : lo + rows, c][ok] = m[ok] + np.log(s)
    return out


def totals(N, w, g, C):
    if g is None:
        return np.array([float(N) if w is None else float(np.sum(w))])
    return np.bincount(np.asarray(g), weights=w, minlength=C).astype(np.float64)


def normalise(raw, N, d, kernel, h, w=None, g=None, C=1):
    """Unnormalised (n, C) log sums -> log densities: + log_norm - log(sum of the group's weights); an empty group stays -inf."""
    tot = totals(N, w, g, C)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = raw + (log_norm(h, d, kernel) - np.log(tot))[None, :]
    out[:, tot == 0] = -np.inf
    return out


def rounded(a, dtype):
    return a if dtype == "float64" else a.astype(np.float32).astype(np.float64)


def log_density(case, dtype="float64", reverse=False, extended=False):
    """The restatement on the case's centred coordinates as the device stores them (float32 mode: rounded to float32).
    extended: the same arithmetic in np.longdouble (64 significant bits on x86), rounded to float64 at the end - what
    make_golden_kde.py measures the restatement's own rounding against."""
    T, X = rounded(case["T"], dtype), rounded(case["X"], dtype)
    if extended:
        T, X = T.astype(np.longdouble), X.astype(np.longdouble)
    h = np.longdouble(case["h"]) if extended else case["h"]
    raw = raw_log_sums(T, X, case["kernel"], h, case["w"], case["g"], case["C"], reverse=reverse)
    return normalise(raw, len(X), case["d"], case["kernel"], case["h"], case["w"], case["g"], case["C"]).astype(np.float64)


def deviation(a, b, ref):
    """max |a - b| / max(1, |ref|) over the entries finite in ref (the masks of a and b must equal ref's)."""
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(a), fin) and np.array_equal(np.isfinite(b), fin)
    if not fin.any():
        return 0.0
    return float((np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max())


def bound(ref, dev_order, dev_sklearn):
    """Per-entry bound on |got - ref| (inf where ref is -inf: those entries are compared by their masks)."""
    rel = max(ALLOW * max(dev_order, dev_sklearn), FLOOR_ULP * EPS)
    return rel * np.maximum(1.0, np.abs(np.where(np.isfinite(ref), ref, 1.0)))


def assert_decidable(case):
    """No pair distance within MARGIN (relative) of h, in float64 and on the float32-rounded coordinates: the support test
    dist < h has one answer whatever the rounding of the distance."""
    if case["kernel"] not in COMPACT:
        return
    for dtype in ("float64", "float32"):
        T, X = rounded(case["T"], dtype), rounded(case["X"], dtype)
        for lo in range(0, len(T), 512):
            gap = np.abs(pair_dist(T[lo : lo + 512], X) - case["h"])
            assert gap.min() > MARGIN * case["h"], (case["name"], dtype, float(gap.min()))


# ------------------------------------------------------------------------------------------------------------------ the cases
def _cloud(rng, N, d, scale=1.0):
    return rng.random((N, d)) * scale


def _make(name, n, N, d, kernel, h=0.3, C=1, same=False, far=0, weights=None, groups=None, dup=False, seed=0, shift=None):
    """One case.  Sources uniform in the unit cube (x `scale` 1); targets the sources themselves (same; then n == N) or an
    independent draw; `far` extra targets 40 h (exponential: 1000 h) beyond the cloud; `dup`: every fourth source repeats the one
    before it and every fifth target sits exactly on a source."""
    rng = np.random.default_rng(seed + 7919 * len(name))
    X = _cloud(rng, N, d)
    if dup and N >= 4:
        X[3::4] = X[2::4][: len(X[3::4])]
    if groups == "two_clusters":   # group 1 lives 60 h away: its shift at a target near group 0 must be its own
        g = (np.arange(N) % 2).astype(np.int64)
        X[g == 1, 0] += 60.0 * h
    elif groups is not None:
        g = np.asarray(groups(rng, N), dtype=np.int64)
    else:
        g = None
    if same:
        T = X.copy()
    else:
        T = _cloud(rng, n, d)
        if dup and n >= 5:
            T[::5] = X[rng.integers(0, N, len(T[::5]))]
    if far:
        reach = (1000.0 if kernel == "exponential" else 40.0) * h
        F = np.zeros((far, d))
        F[:, 0] = X[:, 0].max() + reach * (1.0 + np.arange(far))
        T = np.vstack([T, F])
    w = None if weights is None else np.asarray(weights(rng, N, g), dtype=np.float64)
    centre = X.mean(axis=0)
    return dict(name=name, T=T - centre, X=X - centre, d=d, kernel=kernel, h=float(h), w=w, g=g,
                C=C if g is None else max(C, int(g.max()) + 1), far=far)


def _g_mod(C, skip=()):
    """Group ids 0 .. C - 1 round robin, without the ids in `skip` (a group id with no source; never the last id)."""
    ids = np.array([c for c in range(C) if c not in skip], dtype=np.int64)
    return lambda rng, N: ids[np.arange(N) % len(ids)]


def _w_mixed(dead_group=None, wide=False):
    """Weights in [0.5, 1.5) with every seventh zero; `dead_group`: all of that group's weights zero; `wide`: 1e-300 .. 1e300."""
    def make(rng, N, g):
        w = 10.0 ** rng.uniform(-300, 300, N) if wide else 0.5 + rng.random(N)
        w[::7] = 0.0
        if dead_group is not None and g is not None:
            w[g == dead_group] = 0.0
        return w
    return make


def _build():
    cases = []
    add = lambda *a, **kw: cases.append(_make(*a, **kw))  # noqa: E731
    # n and N at 1, tile - 1, tile, tile + 1, the split threshold and its neighbour, an N of four splits
    add("n1_N1", 1, 1, 3, "gaussian", same=True)
    add("n257_N255", 257, 255, 3, "gaussian", dup=True)
    add("n255_N256", 255, 256, 3, "gaussian")
    add("n256_N257", 256, 257, 3, "epanechnikov")
    add("n1_N257", 1, 257, 2, "gaussian")
    add("n40_N4096", 40, 4096, 3, "gaussian", h=0.05)            # the last size of one split
    add("n40_N4097", 40, 4097, 3, "gaussian", h=0.05)            # two splits
    add("n300_N12290_gauss", 300, 12290, 3, "gaussian", h=0.05)  # four splits' partials, two target tiles
    add("n300_N12290_epan", 300, 12290, 3, "epanechnikov", h=0.08, weights=_w_mixed())
    # all six kernels in d = 1, 2, 3: targets on and off the sources, duplicates, five targets far beyond the cloud
    for d in (1, 2, 3):
        for k in KERNELS:
            add(f"{k}_d{d}", 300, 300, d, k, h={1: 0.02, 2: 0.09, 3: 0.2}[d], same=True, far=5, dup=True, seed=d)
    for k in KERNELS:
        add(f"{k}_disjoint", 130, 600, 3, k, h=0.15, far=5, seed=11)
    # columns: C = 2, 17 (more than one block of 16) and 65 (more than one call of 64), an id without a source, a group whose
    # weights are all zero, zero weights inside live groups
    add("C2_shift_gauss", 200, 400, 3, "gaussian", h=0.1, groups="two_clusters")
    add("C2_shift_expo", 200, 400, 3, "exponential", h=0.1, groups="two_clusters", weights=_w_mixed())
    add("C17_gauss", 150, 700, 3, "gaussian", h=0.2, groups=_g_mod(17, skip=(3,)), weights=_w_mixed(dead_group=5))
    add("C17_linear", 150, 700, 2, "linear", h=0.2, groups=_g_mod(17, skip=(0, 9)), weights=_w_mixed(dead_group=16))
    add("C65_gauss", 100, 1000, 3, "gaussian", h=0.3, groups=_g_mod(65, skip=(63,)), weights=_w_mixed(dead_group=64))
    add("C65_cosine", 100, 1000, 3, "cosine", h=0.4, groups=_g_mod(65, skip=(1,)))
    add("C65_N4097", 30, 4097, 3, "epanechnikov", h=0.3, groups=_g_mod(65))
    # weights over 600 orders of magnitude
    add("wide_gauss", 200, 500, 3, "gaussian", h=0.1, weights=_w_mixed(wide=True), far=5)
    add("wide_expo", 200, 500, 2, "exponential", h=0.1, weights=_w_mixed(wide=True))
    add("wide_epan", 200, 500, 3, "epanechnikov", h=0.3, weights=_w_mixed(wide=True), groups=_g_mod(2))
    add("wide_tophat", 200, 500, 3, "tophat", h=0.3, weights=_w_mixed(wide=True))
    return {c["name"]: c for c in cases}


CASES = _build()
NAMES = tuple(CASES)
GOLDEN_FULL = ("n257_N255", "n256_N257") + tuple(f"{k}_d3" for k in KERNELS) + ("C17_gauss", "wide_gauss", "wide_epan")
# Cases on which sklearn itself is far off (its log-space bound arithmetic loses a group 60 h away to 3e-7, weights over 600
# orders of magnitude to several units: the deviations printed by make_golden_kde.py), so that the bound built on dev_sklearn says little.
# They are held to a second, tighter bound as well: dev_sklearn replaced by dev_extended, the deviation between the restatement
# and the same arithmetic in np.longdouble (the restatement's own rounding; recorded in the golden, x86 extended precision).
TIGHT = ("C2_shift_gauss", "wide_gauss", "wide_expo", "wide_epan", "wide_tophat")


@functools.lru_cache(maxsize=None)
def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def reference(name, dtype="float64"):
    """(ref, per-entry bound, per-entry tight bound or None, dev_order, dev_sklearn) of a case; computed once, shared by the
    tests, read-only."""
    case = CASES[name]
    assert_decidable(case)
    ref = log_density(case, dtype)
    dev_order = deviation(ref, log_density(case, dtype, reverse=True), ref)
    dev_sk = float(load()[f"skdev_{name}"])
    b = bound(ref, dev_order, dev_sk)
    tight = bound(ref, dev_order, float(load()[f"xdev_{name}"])) if name in TIGHT else None
    for a in (ref, b, tight):
        if a is not None:
            a.setflags(write=False)
    return ref, b, tight, dev_order, dev_sk


def compare(got, ref, b):
    """(largest share of the bound used over the finite entries); the -inf masks must be equal."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), "finite / -inf pattern differs"
    assert np.array_equal(got[~fin], ref[~fin]), "a non-finite entry is not -inf"
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / b[fin]).max())
