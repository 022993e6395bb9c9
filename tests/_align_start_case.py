"""Shared by the CPU and GPU suites of the alignment's start state (``spateo_amd.align.init_sigma2``,
``init_probability_parameters``, ``coarse_rigid_alignment``, ``morpho_start`` and the kernel under them,
``mvf_assign_layer_stats``): the cases of tests/golden/ref_align_start.npz, a float64 NumPy restatement of the four host
functions on DENSE distance matrices (test infrastructure, written from DESIGN.md section 4, "The start state") and of the
kernel's outputs, and the comparison helpers.

The kernel, for one layer's distance matrix d (na, nb):

    cmin_j  = min_i d_ij
    rows_j  = the k_eff = min(k, na) rows with the smallest d_ij in the total order (value ascending, row ascending), vals_j theirs
    sums    = (sum_ij d_ij, sum_ij d_ij^2)

The host functions:

    sigma2   = scale * sum_ij (d_ij)^2 / (D nA nA)       d the SQUARED spatial distance, clamped at 0: squared twice, over nA nA
    param_l  = max(sort_i(min_j d_ij)[int(0.05 nA)] / 5, 0.01)
    coarse   = voxel means -> d (voxels A x voxels B) -> the top_K nearest either way -> pairs -> inlier_from_NN (weighted
               rigid fit with an outlier component, 100 iterations) [-> the mirrored fit] -> pairs above the threshold
"""
import os

import numpy as np

import _assign_case as ac

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_align_start.npz")
QUANTITIES = ("sigma2", "parameters", "init_R", "init_t", "inlier_A", "inlier_B", "inlier_P", "coordsA")
INLIER_RANK = 20


def load():
    return np.load(GOLDEN)


def case_tags(g):
    return [str(t) for t in g["cases"]]


def case_inputs(g, tag):
    """The inputs of one golden case as a dict."""
    n_layers = len(g[f"{tag}_dissimilarity"])
    return dict(coordsA=g[f"{tag}_coordsA_in"], coordsB=g[f"{tag}_coordsB"],
                layers_A=[g[f"{tag}_layerA{l}"] for l in range(n_layers)], layers_B=[g[f"{tag}_layerB{l}"] for l in range(n_layers)],
                dissimilarity=[str(m) for m in g[f"{tag}_dissimilarity"]], probability_type=[str(p) for p in g[f"{tag}_probability_type"]],
                probability_parameters=[None if np.isnan(p) else float(p) for p in g[f"{tag}_probability_parameters_in"]],
                subsample_A=g[f"{tag}_subsample_A"], subsample_B=g[f"{tag}_subsample_B"], init_metric=str(g[f"{tag}_init_metric"]),
                top_K=int(g[f"{tag}_top_K"]), allow_flip=bool(g[f"{tag}_allow_flip"]), R0=g[f"{tag}_R0"])


# ------------------------------------------------------------------------------------------------------ the kernel's outputs
def stored_distance(Xp, Yp, a, b, metric):
    """One product layer's distance on PREPARED operands (as stored): d = a_i + b_j - s <X'_i, Y'_j>, clamped / rooted."""
    s = {"euc": 2.0, "square_euc": 2.0, "kl": 1.0, "sym_kl": 0.5, "cos": 0.5}[metric]
    d = (np.asarray(a)[:, None] + np.asarray(b)[None, :]) - s * np.asarray(Xp, dtype=np.float64).dot(np.asarray(Yp, dtype=np.float64).T)
    if metric in ("euc", "square_euc"):
        d = np.maximum(d, 0.0)
    return np.sqrt(d) if metric == "square_euc" else d


def label_distance(table, labels_A, labels_B):
    return np.asarray(table, dtype=np.float64)[np.asarray(labels_A)][:, np.asarray(labels_B)]


def layer_stats(d, k):
    """{cmin (nb,), sums (2,), rows (nb, k_eff) int32, vals (nb, k_eff)} of a dense distance matrix d (na, nb)."""
    d = np.asarray(d, dtype=np.float64)
    out = {"cmin": d.min(0), "sums": np.array([d.sum(), (d * d).sum()])}
    ke = min(k, d.shape[0])
    if ke:
        order = np.argsort(d, axis=0, kind="stable")[:ke].T       # a stable sort: the smaller row first among equal values
        out["rows"], out["vals"] = order.astype(np.int32), np.take_along_axis(d, order.T, axis=0).T
    return out


def list_gap(d, k):
    """The smallest difference between neighbouring entries of the columns' sorted first min(k, na) + 1 values, relative
    to max |d|: above it the reference alone decides every list's order."""
    d = np.asarray(d, dtype=np.float64)
    ke = min(k + 1, d.shape[0])
    if ke < 2:
        return np.inf
    head = np.sort(d, axis=0)[:ke]
    return float(np.diff(head, axis=0).min() / max(np.abs(d).max(), 1e-300))


# ------------------------------------------------------------------------------------------------------ the host functions
def init_sigma2(coordsA, coordsB, iA, iB, scale=1.0, wrong=None):
    """`wrong`: "single_square" (the distance squared once) or "nanb" (divided by D nA nB): what the reference does NOT do."""
    XA, XB = np.asarray(coordsA, dtype=np.float64)[iA], np.asarray(coordsB, dtype=np.float64)[iB]
    d = ac.layer_distance(XA, XB, "euc")
    total = d.sum() if wrong == "single_square" else (d * d).sum()
    return scale * (total / (XA.shape[1] * len(iA) * (len(iB) if wrong == "nanb" else len(iA))))


def init_probability_parameters(layers_A, layers_B, dissimilarity, probability_type, probability_parameters, iA, iB):
    out = list(probability_parameters)
    for l, (A, B, met, kind, par) in enumerate(zip(layers_A, layers_B, dissimilarity, probability_type, probability_parameters)):
        if par is None and kind.lower() == "gauss":
            row_min = np.sort(ac.layer_distance(np.asarray(A, dtype=np.float64)[iA], np.asarray(B, dtype=np.float64)[iB], met).min(1))
            out[l] = max(row_min[int(len(iA) * 0.05)] / 5, 0.01)
    return out


def voxel_data(coords, gene_exp, voxel_num):
    """Grid nodes from the bounding box's minimum in steps of extent / int(sqrt(voxel_num)); a node's value is the mean over
    the points closer than voxel_size / 2 = sqrt(volume) / (sqrt(N) / 5) / 2; nodes without a point are dropped."""
    coords, gene_exp = np.asarray(coords, dtype=np.float64), np.asarray(gene_exp, dtype=np.float64)
    N, D = coords.shape
    lo, hi = coords.min(0), coords.max(0)
    size = np.sqrt(np.prod(hi - lo)) / (np.sqrt(N) / 5)
    step = (hi - lo) / int(np.sqrt(voxel_num))
    nodes = np.stack(np.meshgrid(*[np.arange(a, b, s) for a, b, s in zip(lo, hi, step)]), axis=-1).reshape(-1, D)
    near = np.sqrt(((coords[None, :, :] - nodes[:, None, :]) ** 2).sum(-1)) < size / 2        # (nodes, points)
    used = near.any(1)
    means = np.array([gene_exp[m].mean(0) for m in near[used]])
    return nodes[used], means


def inlier_from_NN(x, y, distance):
    N, D = x.shape
    w0 = np.maximum(0, distance)
    w0 = w0 / (w0.max() / (np.log(10) * 2))
    alpha, gamma = 1.0, 0.5
    weight = np.exp(-w0 * alpha)
    P = np.ones((N, 1)) * weight
    y_hat = x
    sigma2 = ((y_hat - y) ** 2).sum() / (D * N)
    decrease = np.power(0.1 / alpha, 1 / 80)
    area = max(np.prod(x.max(0) - x.min(0)), np.prod(y.max(0) - y.min(0)))
    Sp = P.sum()

    def responsibilities(s2, gm):
        term = np.exp(-((y - y_hat) ** 2).sum(1, keepdims=True) / (2 * s2)) * weight
        return term / (term + weight.max() * (1 - gm) * np.power(2 * np.pi * s2, D / 2) / (gm * area))

    for it in range(100):
        mu_x, mu_y = (x * P).sum(0) / Sp, (y * P).sum(0) / Sp
        U, _, V = np.linalg.svd((y - mu_y).T.dot((x - mu_x) * P))
        C = np.eye(D)
        C[-1, -1] = np.linalg.det(U.dot(V))
        R = U.dot(C).dot(V)
        t = mu_y - mu_x.dot(R.T)
        y_hat = x.dot(R.T) + t
        P = responsibilities(sigma2, gamma)
        Sp = P.sum()
        gamma = min(max(Sp / N, 0.01), 0.99)
        P = np.maximum(P, 1e-6)
        sigma2 = ((y_hat - y) ** 2 * P).sum() / (D * Sp)
        if it > 20:
            alpha = alpha * decrease
            weight = np.exp(-w0 * alpha)
            weight = weight / weight.max()
    P = responsibilities(1e-2, 0.1)
    return P, R, t, min(max(P.sum() / N, 0.01), 0.99)


def coarse_rigid_alignment(coordsA, coordsB, init_A, init_B, iA, iB, metric, top_K, allow_flip=False):
    XA, XB = np.asarray(coordsA, dtype=np.float64), np.asarray(coordsB, dtype=np.float64)
    D = XA.shape[1]
    vA, gA = voxel_data(XA[iA], np.asarray(init_A)[iA], max(min(int(len(iA) / 20), 1000), 100))
    vB, gB = voxel_data(XB[iB], np.asarray(init_B)[iB], max(min(int(len(iB) / 20), 1000), 100))
    d = ac.layer_distance(gA, gB, metric)
    N, M = d.shape
    top_K = min(top_K, N - 1, M - 1)
    cols, rows = layer_stats(d, top_K), layer_stats(d.T, top_K)
    NN = np.vstack((np.stack([np.repeat(np.arange(M), top_K), cols["rows"].reshape(-1)], 1),
                    np.stack([rows["rows"].reshape(-1), np.repeat(np.arange(N), top_K)], 1))).astype(np.int64)
    dist = np.r_[cols["vals"].reshape(-1), rows["vals"].reshape(-1)][:, None]
    x, y = vA[NN[:, 1]], vB[NN[:, 0]]
    P, R, t, gamma = inlier_from_NN(x, y, dist)
    flipped = False
    if allow_flip:
        F = np.eye(D)
        F[-1, -1] = -1
        P2, R2, t2, gamma2 = inlier_from_NN(x.dot(F), y, dist)
        if gamma2 > gamma:
            P, R, t, flipped = P2, R2.dot(F), t2, True
    threshold = min(np.sort(P[:, 0])[::-1][INLIER_RANK], 0.5)
    keep = np.where(P[:, 0] > threshold)[0]
    return dict(inlier_A=x[keep].dot(R.T) + t, inlier_B=y[keep], inlier_P=P[keep], inlier_pairs=NN[keep], init_R=R, init_t=t,
                coordsA=XA.dot(R.T) + t, flipped=flipped, voxels=(vA, gA, vB, gB))


def canonical(pairs, *arrays):
    """The inlier pairs in one order (B voxel, then A voxel; a pair found from both sides is there twice, with equal
    values): np.argpartition leaves a voxel's neighbours unordered, the device orders them by distance."""
    pairs = np.asarray(pairs, dtype=np.int64)
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    return (pairs[order],) + tuple(np.asarray(a)[order] for a in arrays)


def restate_case(c, wrong=None):
    """Every compared quantity of one golden case from the restatement."""
    out = coarse_rigid_alignment(c["coordsA"], c["coordsB"], c["layers_A"][0], c["layers_B"][0], c["subsample_A"], c["subsample_B"],
                                 c["init_metric"], c["top_K"], c["allow_flip"])
    out["sigma2"] = init_sigma2(out["coordsA"], c["coordsB"], c["subsample_A"], c["subsample_B"], wrong=wrong)
    out["parameters"] = np.array(init_probability_parameters(c["layers_A"], c["layers_B"], c["dissimilarity"], c["probability_type"],
                                                             c["probability_parameters"], c["subsample_A"], c["subsample_B"]),
                                 dtype=np.float64)
    return out


def deviations(got, g, tag):
    """{quantity: max |got - ref| / max |ref|} against the golden case; the inlier pair sets must be equal."""
    ref_pairs, rA, rB, rP = canonical(g[f"{tag}_inlier_pairs"], g[f"{tag}_inlier_A"], g[f"{tag}_inlier_B"], g[f"{tag}_inlier_P"])
    got_pairs, gA, gB, gP = canonical(got["inlier_pairs"], got["inlier_A"], got["inlier_B"], got["inlier_P"])
    assert np.array_equal(ref_pairs, got_pairs), (tag, len(ref_pairs), len(got_pairs))
    vals = dict(got, inlier_A=gA, inlier_B=gB, inlier_P=gP)
    ref = {q: g[f"{tag}_{q}"] for q in QUANTITIES}
    ref.update(inlier_A=rA, inlier_B=rB, inlier_P=rP)
    dev = {}
    for q in QUANTITIES:
        a, b = np.asarray(vals[q], dtype=np.float64).reshape(-1), np.asarray(ref[q], dtype=np.float64).reshape(-1)
        assert a.shape == b.shape and np.isfinite(a).all(), (tag, q, a.shape, b.shape)
        dev[q] = float(np.abs(a - b).max() / np.abs(b).max())
    return dev


def tolerances(g, tag, dtype):
    """float64: max(F64_TOL, 1.25 g F64_TOL) with g the stored amplification; float32: 1.25 x the stored float32 twin's deviation."""
    if dtype == "float64":
        return {q: max(ac.F64_TOL, ac.ALLOW * float(g[f"{tag}_g_{q}"]) * ac.F64_TOL) for q in QUANTITIES}
    return {q: ac.ALLOW * float(g[f"{tag}_f32_{q}"]) for q in QUANTITIES}


def check(got, g, tag, tols, what=""):
    """Print every figure, then assert."""
    dev = deviations(got, g, tag)
    print(f"  {what} case {tag}: " + ", ".join(f"{q} {dev[q]:.2e} (<= {tols[q]:.2e})" for q in QUANTITIES))
    for q in QUANTITIES:
        assert dev[q] <= tols[q], (what, tag, q, dev[q], tols[q])
    return dev
