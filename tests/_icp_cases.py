"""Float64 restatements of what ``csrc/mvf_icp.hip`` computes - the batched 2-D ICP, the mesh transform, the cut and the loss -
in the DEVICE's order of operations, the cases the suites share, and the bound of every coordinate comparison, DERIVED here (no
tolerance is hard-coded):

  * every sum over points: a lane of the 256 adds its points ``lane, lane + 256`` in that order, the 64 lanes of a wave fold by
    halving, the four waves add in wave order (``block_sum``);
  * nearest data point: candidates in rising index and a strict ``<`` (``argmin`` takes the first minimum);
  * ``R = V U^T`` of the 2 x 2 covariance as the closed-form orthogonal polar factor of its transpose (``polar2``);
  * coordinates: the deviation the restatement itself shows when every input is perturbed by up to +-4 ulp (8 draws), relative
    to the coordinate scale; the GPU assertion is ``ALLOW`` = 64 times that, the rule of tests/_sample_cases.py.  One ulp is what
    a device ``sin`` / ``cos`` may differ from NumPy's by.  Counts, flags, round numbers and ``gamma`` compare equal.

tests/test_icp_kernel_refs.py proves the restatement against the real reference (tests/golden/ref_mesh_correction.npz)."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ALLOW = 64.0
LANES, WAVE = 256, 64
ICP_DEFAULTS = dict(max_iter=20, error_threshold=1e-6, inlier_threshold=0.1, gamma_threshold=0.05, subsample=500, allow_rotation=False)


def load():
    with np.load(os.path.join(HERE, "golden", "ref_mesh_correction.npz")) as z:
        return {k: z[k] for k in z.files}


def thin_rows(n, subsample):
    """The rows a contour of n points keeps: ``floor(j n / subsample)``."""
    if subsample > 0 and n > subsample:
        return (np.arange(subsample, dtype=np.int64) * n) // subsample
    return np.arange(n, dtype=np.int64)


def block_sum(v):
    """The workgroup's sum of per-point values (at most 512, zero where a lane adds nothing)."""
    v = np.asarray(v, dtype=np.float64)
    assert v.ndim == 1 and len(v) <= 2 * LANES
    p = np.zeros(2 * LANES)
    p[: len(v)] = v
    w = (p[:LANES] + p[LANES:]).reshape(LANES // WAVE, WAVE)
    o = WAVE // 2
    while o:
        w = w[:, :o] + w[:, o: 2 * o]
        o //= 2
    return float(((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])


def polar2(h):
    """``V U^T`` of ``H = U S V^T`` (h = H row-major): the orthogonal polar factor of ``H^T``, a reflection when det < 0."""
    pa, pb, pc, pd = h[0], h[2], h[1], h[3]
    det = pa * pd - pb * pc
    if det >= 0.0:
        p, q = pa + pd, pc - pb
        n = math.sqrt(p * p + q * q)
        return np.array([[p / n, -(q / n)], [q / n, p / n]]) if n > 0.0 else np.eye(2)
    p, q = pa - pd, pb + pc
    n = math.sqrt(p * p + q * q)
    return np.array([[p / n, q / n], [q / n, -(p / n)]])


def icp(contour_1, contour_2, max_iter=20, error_threshold=1e-6, inlier_threshold=0.1, gamma_threshold=0.05, subsample=500,
        allow_rotation=False):
    """What one workgroup of ``icp_batch_kernel`` computes: dict(gamma, iters, inliers, T, translation, dets) - ``dets`` the sign of every
    round's covariance determinant."""
    c1 = np.asarray(contour_1, dtype=np.float64)
    c2 = np.asarray(contour_2, dtype=np.float64)
    c1, c2 = c1[thin_rows(len(c1), subsample)], c2[thin_rows(len(c2), subsample)]
    N, M = len(c1), len(c2)
    m1, m2 = (c1.max(0) + c1.min(0)) / 2, (c2.max(0) + c2.min(0)) / 2
    A, B = c1 - m1, c2 - m2
    ss0 = block_sum(A[:, 0] * A[:, 0] + A[:, 1] * A[:, 1])
    ss1 = block_sum(B[:, 0] * B[:, 0] + B[:, 1] * B[:, 1])
    with np.errstate(all="ignore"):
        scale = (math.sqrt(ss0 / N) + math.sqrt(ss1 / M)) / 2
        A, B = A / scale, B / scale
    prev, iters, ninl, dets = math.inf, 0, 0, []
    ltx = lty = 0.0
    dist = np.full(M, np.inf)
    for it in range(max_iter):
        iters = it + 1
        dx, dy = B[:, 0:1] - A[None, :, 0], B[:, 1:2] - A[None, :, 1]
        d2 = dx * dx + dy * dy
        bi = d2.argmin(1)
        dist = np.sqrt(d2[np.arange(M), bi])
        inl = dist < inlier_threshold
        near = A[bi]
        s = [block_sum(np.where(inl, x, 0.0)) for x in (np.ones(M), B[:, 0], B[:, 1], near[:, 0], near[:, 1], dist)]
        ninl = int(s[0])
        if ninl < 3:
            ltx = lty = 0.0
            break
        cnt = s[0]
        bmx, bmy, amx, amy = s[1] / cnt, s[2] / cnt, s[3] / cnt, s[4] / cnt
        R = np.eye(2)
        if allow_rotation:
            ux, uy, vx, vy = B[:, 0] - bmx, B[:, 1] - bmy, near[:, 0] - amx, near[:, 1] - amy
            h = [block_sum(np.where(inl, x, 0.0)) for x in (ux * vx, ux * vy, uy * vx, uy * vy)]
            dets.append(h[0] * h[3] - h[2] * h[1])
            R = polar2(h)
            tx, ty = amx - (R[0, 0] * bmx + R[0, 1] * bmy), amy - (R[1, 0] * bmx + R[1, 1] * bmy)
        else:
            tx, ty = amx - bmx, amy - bmy
        x, y = B[:, 0].copy(), B[:, 1].copy()
        B = np.stack([(R[0, 0] * x + R[0, 1] * y) + tx, (R[1, 0] * x + R[1, 1] * y) + ty], axis=1)
        ltx, lty = tx, ty
        err = s[5] / cnt
        if abs(prev - err) < error_threshold:
            break
        prev = err
    gamma = block_sum(np.where(dist < gamma_threshold, 1.0, 0.0)) / M
    T = np.stack([scale * B[:, 0] + m1[0], scale * B[:, 1] + m1[1]], axis=1)
    shift = np.array([(scale * ltx + m1[0]) - m2[0], (scale * lty + m1[1]) - m2[1]])
    return dict(gamma=gamma, iters=iters, inliers=ninl, T=T, dets=dets, translation=shift)


def jitter(rng, a, ulp=4):
    """``a`` with every element scaled by ``1 + j 2^-52``, j uniform in -ulp .. ulp."""
    a = np.asarray(a, dtype=np.float64)
    return a * (1.0 + rng.integers(-ulp, ulp + 1, size=a.shape) * 2.0 ** -52)


def deviation(fn, arrays, scale, draws=8, seed=0):
    """max |fn(jittered arrays) - fn(arrays)| / scale over ``draws`` +-4 ulp perturbations; fn returns one array."""
    rng = np.random.default_rng(seed)
    base = np.asarray(fn(*arrays))
    dev = 0.0
    for _ in range(draws):
        got = np.asarray(fn(*[jitter(rng, a) for a in arrays]))
        dev = max(dev, float(np.abs(got - base).max()) / scale)
    return dev


def icp_bound(c1, c2, **kw):
    """(bound on |T - T_restated| in coordinate units, the restatement's result): ALLOW x the 4-ulp deviation, at least
    ALLOW x 2^-52 of the coordinate magnitude (a case may be insensitive to the 8 draws)."""
    c1, c2 = np.asarray(c1, dtype=np.float64), np.asarray(c2, dtype=np.float64)
    mag = float(max(np.abs(c1).max(), np.abs(c2).max()))
    dev = deviation(lambda a, b: icp(a, b, **kw)["T"], (c1, c2), mag)
    return ALLOW * max(dev, 2.0 ** -52) * mag, icp(c1, c2, **kw)


# ---- the mesh ----
def unique_edges(triangles):
    """The unique edges (a < b) of the triangles, sorted by (a, b): int32 (E, 2)."""
    t = np.asarray(triangles, dtype=np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    return np.unique(np.sort(e, axis=1), axis=0).astype(np.int32)


def _mat3_mul(a, b):
    c = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            c[i, j] = (a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]
    return c


def transform(verts, mean, param):
    """``_transform_points`` with the translation on z of every vertex; param = (rx, ry, rz in degrees, tz, scale)."""
    k = 3.14159265358979323846 / 180.0
    ex, ey, ez = float(param[0]) * k, float(param[1]) * k, float(param[2]) * k
    cx, sx, cy, sy, cz, sz = np.cos(ex), np.sin(ex), np.cos(ey), np.sin(ey), np.cos(ez), np.sin(ez)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    R = _mat3_mul(Rz, _mat3_mul(Ry, Rx))
    c = np.asarray(verts, dtype=np.float64) - np.asarray(mean, dtype=np.float64)
    out = np.empty_like(c)
    for j in range(3):
        out[:, j] = float(param[4]) * ((c[:, 0] * R[j, 0] + c[:, 1] * R[j, 1]) + c[:, 2] * R[j, 2]) + mean[j]
    out[:, 2] = out[:, 2] + float(param[3])
    return out


def cut(P, edges, h):
    """The contour of the transformed vertices P at height h: one point per edge whose ends classify differently under
    ``z >= h``, in edge order; (n, 2)."""
    a, b = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    za, zb = P[a, 2], P[b, 2]
    f = (za >= h) != (zb >= h)
    a, b, za, zb = a[f], b[f], za[f], zb[f]
    t = (h - za) / (zb - za)
    return np.stack([P[a, 0] + t * (P[b, 0] - P[a, 0]), P[a, 1] + t * (P[b, 1] - P[a, 1])], axis=1)


def mesh_contours(verts, edges, mean, param, heights):
    P = transform(verts, mean, param)
    return [cut(P, edges, float(h)) for h in heights]


def mesh_loss(verts, edges, mean, params, heights, contours, max_iter=20, error_threshold=1e-6, inlier_threshold=0.1,
              gamma_threshold=0.05, subsample=500):
    """``mvf_mesh_loss``: (loss (n_T,), gamma (n_T, n_S), count (n_T, n_S))."""
    params = np.atleast_2d(np.asarray(params, dtype=np.float64))
    nT, nS = len(params), len(heights)
    loss, gamma, count = np.zeros(nT), np.zeros((nT, nS)), np.zeros((nT, nS), dtype=np.int32)
    for t in range(nT):
        cost = 0.0
        for s, m_c in enumerate(mesh_contours(verts, edges, mean, params[t], heights)):
            count[t, s] = len(m_c)
            if len(m_c):
                gamma[t, s] = icp(contours[s], m_c, max_iter, error_threshold, inlier_threshold, gamma_threshold, subsample, True)["gamma"]
            cost = cost + (1.0 - gamma[t, s])
        loss[t] = (cost if count[t].all() else 1e6) / nS
    return loss, gamma, count


# ---- shared cases ----
def closed_curve(n, seed, noise=0.01, radius=40.0, centre=(120.0, -35.0)):
    """A noisy closed curve in general position: n points, never a lattice."""
    rng = np.random.default_rng(seed)
    th = np.sort(rng.random(n)) * 2 * np.pi
    r = radius * (1 + 0.25 * np.cos(3 * th + 0.4) + 0.1 * np.sin(5 * th))
    return np.stack([centre[0] + r * np.cos(th), centre[1] + 0.8 * r * np.sin(th)], axis=1) + rng.standard_normal((n, 2)) * noise * radius


def moved(c, angle_deg, shift, seed, noise=0.004, n=None, reflect=False):
    """The curve c rotated, shifted, resampled (n of its points, None = all) and with fresh noise: a model for c as data."""
    rng = np.random.default_rng(seed)
    a = np.deg2rad(angle_deg)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    if reflect:
        R = R @ np.diag([1.0, -1.0])
    ctr = c.mean(0)
    pick = np.arange(len(c)) if n is None else np.sort(rng.choice(len(c), n, replace=n > len(c)))
    ext = float(np.ptp(c, axis=0).max())
    return (c[pick] - ctr) @ R.T + ctr + np.asarray(shift) + rng.standard_normal((len(pick), 2)) * noise * ext


def icp_pair(n1, n2, seed, angle=3.0, shift=(1.5, -1.0), reflect=False):
    """(contour_1, contour_2): sizes n1, n2, the model a moved, resampled copy of a dense curve the data is drawn from too."""
    dense = closed_curve(max(n1, n2, 8) * 2, seed)
    rng = np.random.default_rng(seed + 1)
    c1 = dense[np.sort(rng.choice(len(dense), n1, replace=False))]
    c2 = moved(dense, angle, shift, seed + 2, n=n2, reflect=reflect)
    return c1, c2


def zigzag_pair(n, seed, amplitude=0.3):
    """(contour_1, contour_2) whose covariance has a NEGATIVE determinant: two zig-zags along x, the model's teeth pointing
    against the data's, every model point nearest to the data point of its own tooth - the best orthogonal map is a reflection."""
    rng = np.random.default_rng(seed)
    x = np.arange(n, dtype=np.float64)
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    c1 = np.stack([x + rng.uniform(-0.05, 0.05, n), amplitude * sign * rng.uniform(0.9, 1.1, n)], axis=1) + np.array([55.0, -20.0])
    c2 = np.stack([x + rng.uniform(-0.05, 0.05, n), -0.6 * amplitude * sign * rng.uniform(0.9, 1.1, n)], axis=1) + np.array([55.4, -19.8])
    return c1, c2


def ellipsoid(n_lat=9, n_lon=14, radii=(30.0, 22.0, 16.0), centre=(100.0, 60.0, 40.0), seed=5):
    """A closed triangulated surface (points (V, 3), triangles (F, 3)): a UV ellipsoid with jittered vertices, 2 n_lon (n_lat - 1)
    triangles - 224 at the defaults."""
    rng = np.random.default_rng(seed)
    pts = [[0.0, 0.0, 1.0]]
    for i in range(1, n_lat):
        ph = np.pi * i / n_lat
        for j in range(n_lon):
            th = 2 * np.pi * (j + 0.37 * i) / n_lon
            pts.append([np.sin(ph) * np.cos(th), np.sin(ph) * np.sin(th), np.cos(ph)])
    pts.append([0.0, 0.0, -1.0])
    pts = np.array(pts) * (1 + rng.uniform(-0.03, 0.03, (len(pts), 1)))
    tri = []
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon  # noqa: E731
    for j in range(n_lon):
        tri.append([0, ring(1, j), ring(1, j + 1)])
        tri.append([len(pts) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)])
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            tri.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
            tri.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
    return pts * np.array(radii) + np.array(centre), np.array(tri, dtype=np.int64)


def slices_of(verts, tri, param, heights, seed=9, noise=0.0, per=None):
    """Slice contours of the mesh under ``param``: the cut points (optionally ``per`` of them, with noise) - what a stack of
    aligned slices of that organ would show."""
    rng = np.random.default_rng(seed)
    out = []
    for c in mesh_contours(verts, unique_edges(tri), verts.mean(0), param, heights):
        if per is not None and len(c) > per:
            c = c[np.sort(rng.choice(len(c), per, replace=False))]
        out.append(c + rng.standard_normal(c.shape) * noise)
    return out
