"""Cases, NumPy restatement and bounds of the shape-similarity tests (csrc/mvf_shape.hip, tdr/morphometrics/shape_similarity.py).

Clouds are generated here from seeds; tests/golden/ref_shape_similarity.npz (written by make_golden_shape_similarity.py, where
the reference is) holds only what the reference computes on them: per kept subspace ``[cosine, dist]``, the count, the voxel id,
``lstsq``'s rank and singular values, the same ``dist`` under ``lapack_driver="gelss"``, and eigenvector, weight vector and
scores under both drivers.

The restatement follows the reference's arithmetic with the loop over voxels replaced by table comparisons: binning by the
interval tables ``lo <= x`` and ``x < hi``, the fit by QR of the raw monomials and an SVD of the triangle cut at ``eps
sigma_max`` (minimum norm), the surface on the voxel's own 20 x 20 grid, the mean distance and the cosine.

Bounds.  The fit is ill-conditioned by construction (raw monomials), and the reference itself moves when LAPACK's driver is
swapped: ``swap_<case>`` is the relative deviation of ``dist`` per subspace between gelsd and gelss, recorded in the golden.  A
subspace is MARGINAL if any ``sigma_i / sigma_max`` of the reference lies in ``[eps / 16, 16 eps]``: there the rank is a coin
toss.  ``ALLOW`` = 64 is the project's margin for float64 restatements (tests/_kde_cases.py), ``FLOOR_ULP`` = 16 the floor."""
import functools
import math
import os

import numpy as np

EPS = float(np.finfo(np.float64).eps)
ALLOW, FLOOR_ULP = 64.0, 16.0
GRID = 20
ROW_BLOCK, WG_ROWS = 64, 256          # rows a wave / a workgroup of the fit kernel folds at a time
ORDERS = {"linear": 1, "quadratic": 2, "cubic": 3}
P = {"linear": 3, "quadratic": 6, "cubic": 10}
MAX_NSUB = 128
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_shape_similarity.npz")
EDGE_MARGIN = 1e-6                     # no descriptor of an end-to-end cloud lies within this (relative) of a bin edge of stage 4
MARGINAL_SHARE = 0.05
M, S = 10, 5                           # the defaults of stage 4


# ------------------------------------------------------------------------------------------------------------------- clouds
def ellipsoid(seed, n, axes, offset):
    """n points uniform in a solid ellipsoid (a cell cloud fills its organ): random directions, radius U^(1/3), scaled by the
    axes.  The sub-bins of stage 4 compare ABSOLUTE distances with fractions of their ptp, so a shell - every distance far above
    the ptp - would leave the eigenvector empty and the score 0 / 0."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = rng.random(n) ** (1.0 / 3.0)
    return u * np.asarray(axes, dtype=np.float64) * r[:, None] + np.asarray(offset, dtype=np.float64)


def _unique_rows_in_order(a):
    _, first = np.unique(a, axis=0, return_index=True)
    return a[np.sort(first)]


def _one_voxel(seed, k):
    """k points at small real coordinates that one voxel (n_subspace = 1) holds whole, and one more on the cuboid's upper faces
    (ptp is the integer 3 x 2, so no interval holds it): the global centroid then differs from the voxel's, whose cosine would
    otherwise be 0 / 0.  z is a smooth function of (x, y) and noise."""
    rng = np.random.default_rng(seed)
    x, y = 3.0 * rng.random(k + 1), 2.0 * rng.random(k + 1)
    x[0], y[0], x[k], y[k] = 0.0, 0.0, 3.0, 2.0
    z = 1.0 + 0.3 * x - 0.2 * y + 0.1 * x * y + 0.05 * np.sin(2.0 * x) + 0.02 * rng.standard_normal(k + 1)
    return np.c_[x, y, z]


def _x_constant(seed):
    """n_subspace = 3: every point of voxel 0 has the same x (columns of its A are multiples of one another: rank <= 4, and its
    smallest singular values are rounding - the one marginal subspace of some 27, within MARGINAL_SHARE)."""
    rng = np.random.default_rng(seed)
    pts = 3.0 * rng.random((1000, 3))
    pts[:, 2] = 0.5 * pts[:, 2] + 0.3 * pts[:, 0] + 0.2 * pts[:, 1] ** 2
    pts[0] = 0.0, 2.5, 2.5                                   # (the minimum of x lies outside voxel 0: the tables stay)
    pts[bin_points(pts, 3)[0] == 0, 0] = 0.5
    return pts


def _exact_cubic(seed):
    """z an exact cubic of (x, y) on dyadic coordinates: the residual is 0 to rounding, the coefficients show through Z only.
    300 points in the voxel and one on its upper faces, as in _one_voxel."""
    rng = np.random.default_rng(seed)
    x, y = rng.integers(0, 256, 301) / 128.0, rng.integers(0, 256, 301) / 128.0
    x[0], y[0], x[300], y[300] = 0.0, 0.0, 2.0, 2.0
    z = 0.5 + x - 0.25 * y + 0.125 * x * x - 0.5 * x * y + 0.25 * y * y + 0.0625 * x ** 3 - 0.125 * x * x * y + 0.03125 * x * y * y + 0.0625 * y ** 3
    return np.c_[x, y, z]


def _build():
    c = {}
    c["A"] = dict(pcs=_unique_rows_in_order(np.round(ellipsoid(11, 3000, (30, 20, 15), (40, 30, 20)))), n=4)
    c["B"] = dict(pcs=ellipsoid(12, 6000, (30, 20, 15), (0, 0, 0)), n=5)
    c["B4"] = dict(pcs=c["B"]["pcs"], n=4)   # the partner of A in the pairwise score (one n_subspace per call)
    c["C"] = dict(pcs=_unique_rows_in_order(np.round(ellipsoid(13, 4000, (3, 2, 1.5), (4, 3, 2)) * 10.0) / 10.0), n=4)
    c["D"] = dict(pcs=ellipsoid(19, 20000, (300, 200, 150), (1000, 800, 600)), n=8)
    c["D2"] = dict(pcs=ellipsoid(16, 20000, (260, 230, 120), (1000, 800, 600)), n=8)
    for k in (ROW_BLOCK - 1, ROW_BLOCK, ROW_BLOCK + 1, WG_ROWS - 1, WG_ROWS, WG_ROWS + 1, 5000):
        c[f"E_k{k}"] = dict(pcs=_one_voxel(100 + k, k), n=1)
    c["E_k2"] = dict(pcs=np.array([[0.0, 0.0, 1.0], [1.5, 1.25, 1.5], [2.0, 2.0, 1.75]]), n=1)   # (the third lies in no interval)
    c["E_xconst"] = dict(pcs=_x_constant(21), n=3)
    c["E_cubic"] = dict(pcs=_exact_cubic(22), n=1)
    for name, case in c.items():
        case["pcs"] = np.ascontiguousarray(case["pcs"], dtype=np.float64)
        case["orders"] = ("cubic", "quadratic", "linear") if name == "B" else ("cubic",)
    return c


@functools.lru_cache(maxsize=None)
def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# -------------------------------------------------------------------------------------------------------------- restatement
def tables(pcs, n):
    """lo, hi (3, n): `min + j * size` and `(min + j * size) + size` with `size = ceil(ptp) / n` (rough_subspace's own operations)."""
    start, ptp = np.min(pcs, axis=0), np.ptp(pcs, axis=0)
    lo, hi = np.empty((3, n)), np.empty((3, n))
    for a in range(3):
        size = math.ceil(ptp[a]) / n
        for j in range(n):
            lo[a, j] = start[a] + j * size
            hi[a, j] = lo[a, j] + size
    return lo, hi


def bin_points(pcs, n):
    """(point_voxel, n_overlap): the voxel of every point by the table comparisons, -1 for a point no interval holds; a point two
    intervals of an axis hold goes to the lower one and is counted."""
    lo, hi = tables(pcs, n)
    ids, over = [], np.zeros(len(pcs), dtype=bool)
    for a in range(3):
        x = pcs[:, a][:, None]
        inside = (lo[a][None, :] <= x) & (x < hi[a][None, :])
        hits = inside.sum(axis=1)
        ids.append(np.where(hits > 0, inside.argmax(axis=1), -1))
        over |= hits > 1
    bad = (ids[0] < 0) | (ids[1] < 0) | (ids[2] < 0)
    return np.where(bad, -1, (ids[2] * n + ids[1]) * n + ids[0]).astype(np.int32), int(over.sum())


def groups(point_voxel):
    """(kept voxel ids, counts, list of row indices in original order) of the voxels with two points or more."""
    order = np.argsort(point_voxel, kind="stable")
    v = point_voxel[order]
    order, v = order[v >= 0], v[v >= 0]
    ids, first, counts = np.unique(v, return_index=True, return_counts=True)
    keep = counts >= 2
    return ids[keep].astype(np.int32), counts[keep].astype(np.int64), [order[f : f + c] for f, c in zip(first[keep], counts[keep])]


def design(x, y, order):
    one = np.ones_like(x)
    if order == "linear":
        return np.c_[x, y, one]
    if order == "quadratic":
        return np.c_[one, x, y, x * y, x * x, y * y]
    return np.c_[one, x, y, x * x, x * y, y * y, x * x * x, x * x * y, x * (y * y), y * y * y]


def fit(sub, order):
    """(coefficients, rank, singular values): the minimum-norm least-squares solution by QR and an SVD of the triangle, singular
    values at or below eps sigma_max dropped."""
    A, z = design(sub[:, 0], sub[:, 1], order), sub[:, 2]
    if len(sub) >= A.shape[1]:
        Q, R = np.linalg.qr(A)
        d = Q.T @ z
    else:
        R, d = A, z
    U, s, Vt = np.linalg.svd(R, full_matrices=False)
    keep = s > EPS * s[0]
    return Vt[keep].T @ ((U[:, keep].T @ d) / s[keep]), int(keep.sum()), s


def surface_dist(sub, coef, order, g, reverse=False):
    mn, mx = sub.min(axis=0), sub.max(axis=0)
    X, Y = np.meshgrid(np.linspace(mn[0], mx[0], GRID), np.linspace(mn[1], mx[1], GRID))
    XX, YY = X.ravel(), Y.ravel()
    Z = coef[0] * XX + coef[1] * YY + coef[2] if order == "linear" else design(XX, YY, order) @ coef
    dd = np.sqrt((XX - g[0]) ** 2 + (YY - g[1]) ** 2 + (Z - g[2]) ** 2)
    return float(np.sum(dd[::-1] if reverse else dd) / dd.size)


def cosine_of(sub, g, reverse=False):
    rows = sub[::-1] if reverse else sub
    c = np.add.reduce(rows, axis=0) / len(rows) - g
    return float(abs(c[2] / np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])))


@functools.lru_cache(maxsize=None)
def restated(name, order="cubic"):
    """``describe`` on a case (computed once, shared by the tests)."""
    return describe(CASES[name]["pcs"], CASES[name]["n"], order)


def describe(pcs, n, order="cubic"):
    """The restatement on a cloud: a dict like ``subspace_descriptors`` returns, plus ``cosine_rev`` / ``dist_rev`` (the same with
    the sums taken in reversed order: the restatement's own summation-order deviation) and ``sv`` (list of arrays)."""
    pv, n_overlap = bin_points(pcs, n)
    ids, counts, rows = groups(pv)
    g = np.mean(pcs, axis=0)
    out = dict(point_voxel=pv, n_overlap=n_overlap, n_dropped=int((pv < 0).sum()), voxel=ids, count=counts, centroid=g)
    cos, cos_rev, dist, dist_rev, rank, sv = [], [], [], [], [], []
    for r in rows:
        sub = pcs[r]
        coef, rk, s = fit(sub, order)
        cos.append(cosine_of(sub, g)), cos_rev.append(cosine_of(sub, g, True))
        dist.append(surface_dist(sub, coef, order, g)), dist_rev.append(surface_dist(sub, coef, order, g, True))
        rank.append(rk), sv.append(s)
    out.update(cosine=np.array(cos), cosine_rev=np.array(cos_rev), dist=np.array(dist), dist_rev=np.array(dist_rev),
               rank=np.array(rank, dtype=np.int32), sv=sv)
    return out


# ------------------------------------------------------------------------------------------------ eigenvector, score (stage 4, 5)
def calculate_eigenvector(vs, m=M, s=S):
    """Stage 4 restated independently of the product: masks per (i, j) bin, entry mean(dist) / max(dist), weight the count."""
    vs = np.asarray(vs)
    e, w = np.zeros(m * s), np.zeros(m * s)
    for i in range(m):
        rows = vs[(vs[:, 0] >= i / m) & (vs[:, 0] < (i + 1) / m)]
        if not len(rows):
            continue
        dmax, dptp = np.max(rows[:, 1]), np.ptp(rows[:, 1])
        for j in range(s):
            sel = rows[(rows[:, 1] >= dptp * j / s) & (rows[:, 1] < dptp * (j + 1) / s)]
            if len(sel):
                e[i * s + j], w[i * s + j] = np.mean(sel[:, 1]) / dmax, len(sel)
    return e, w / np.sum(w)


def score(e1, w1, e2, w2):
    w = np.max(np.c_[w1, w2], axis=1)
    return round(float(np.sum(w * e1 * e2) / (np.linalg.norm(np.sqrt(w) * e1) * np.linalg.norm(np.sqrt(w) * e2))), 4)


def edge_margin(vs, m=M, s=S):
    """The smallest relative distance of a descriptor to a bin edge of stage 4 that could move it into another bin: cosines
    against i / m, distances against ptp j / s of their cosine bin (the edges at which membership changes)."""
    vs = np.asarray(vs)
    worst = np.inf
    for i in range(m + 1):
        worst = min(worst, float(np.min(np.abs(vs[:, 0] - i / m))))
    for i in range(m):
        rows = vs[(vs[:, 0] >= i / m) & (vs[:, 0] < (i + 1) / m)]
        if len(rows) < 2:
            continue
        dptp = np.ptp(rows[:, 1])
        for j in range(1, s + 1):
            edge = dptp * j / s
            worst = min(worst, float(np.min(np.abs(rows[:, 1] - edge) / np.maximum(np.abs(edge), 1e-300))))
    return worst


# -------------------------------------------------------------------------------------------------------------------- bounds
def marginal(sv_ref):
    """Per subspace: does any sigma_i / sigma_max of the reference lie in [eps / 16, 16 eps]?  sv_ref: (subspaces, p), NaN padded."""
    with np.errstate(invalid="ignore"):
        ratio = sv_ref / sv_ref[:, :1]
        return np.any((ratio >= EPS / 16.0) & (ratio <= 16.0 * EPS), axis=1)


def swap_deviation(G, name, order="cubic"):
    """Per subspace |dist_gelss - dist_gelsd| / |dist_gelsd| of the reference."""
    key = f"{name}_{order}"
    return np.abs(G[f"{key}_dist_gelss"] - G[f"{key}_vs"][:, 1]) / np.abs(G[f"{key}_vs"][:, 1])


def dist_bounds(G, name, order="cubic"):
    """(bound on the maximum, bound on the median or None, mask of the subspaces compared) of the relative deviation of `dist`."""
    swap = swap_deviation(G, name, order)
    floor = FLOOR_ULP * EPS
    if name in ALL_SUBSPACES:
        return max(ALLOW * float(swap.max()), floor), max(ALLOW * float(np.median(swap)), floor), np.ones(len(swap), dtype=bool)
    keep = ~marginal(G[f"{name}_{order}_sv"])
    assert (~keep).mean() <= MARGINAL_SHARE, (name, order, float((~keep).mean()))
    return max(ALLOW * float(swap.max()), floor), None, keep


def cosine_bound(name, order="cubic"):
    r = restated(name, order)
    dev = float(np.max(np.abs(r["cosine"] - r["cosine_rev"]) / np.abs(r["cosine"])))
    return max(ALLOW * dev, FLOOR_ULP * EPS)


# -------------------------------------------------------------------------------------------------------------------- cases
CASES = _build()
NAMES = tuple(CASES)
END_TO_END = ("A", "B", "B4", "D", "D2")              # the clouds the eigenvector and the score are tested on
PAIRS = (("A", "B4"), ("D", "D2"))
ALL_SUBSPACES = ("D", "D2")                         # no subspace is left out of the dist comparison: maximum and median are bounded
