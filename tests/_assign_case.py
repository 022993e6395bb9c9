"""Shared by the CPU and GPU suites of the alignment's assignment step: the cases of tests/golden/ref_assign.npz, a float64
NumPy restatement of the step (test infrastructure, written from the formulas of DESIGN.md, not from the reference's
text) and the comparison helper.

The step, for A cells i (coordinates x_i, NA of them) and B cells j (y_j, NB), with d_ij = max(|x_i|^2 + |y_j|^2 -
2 x_i.y_j, 0):

    m_i   = alpha_i exp(-SigmaDiag_i / sigma2)                                     (model_mul)
    o     = (2 pi sigma2)^(D/2) (1 - gamma) / (gamma samples_s NA)                 (spatial_outlier)
    e1_ij = exp(-d_ij / (2 sigma2 / sigma2_variance)),   e2_ij = exp(-d_ij / (2 sigma2))
    S0_j  = sum_i e1_ij,  S1_j = sum_i e1_ij m_i,  S2_j = sum_i e2_ij m_i,  S3_j = sum_i e2_ij m_i q_ij
    q_ij  = prod over the layers of their probability of the layer distance
    in_j  = 1 - o / (o + S0_j)                                                      (spatial_inlier)
    P1_ij = e1_ij m_i / (o + S1_j)                         -> K_NA_spatial = row sums
    P2_ij = in_j e2_ij m_i / (S2_j + 1e-8)                 -> K_NA_sigma2 = row sums, sigma2_related = sum P2 d
    P_ij  = in_j e2_ij m_i q_ij / (S3_j + 1e-8)            -> K_NA, K_NB, Sp, PXB = P @ coordsB
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_assign.npz")
QUANTITIES = ("K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2", "Sp", "Sp_spatial", "Sp_sigma2", "sigma2_related", "PXB")
EPS = 1e-8


def load():
    return np.load(GOLDEN)


def case_tags(g):
    return [str(t) for t in g["cases"]]


def case_inputs(g, tag):
    """(positional arguments, keyword arguments) of update_assignment / restatement for one golden case."""
    n_layers = len(g[f"{tag}_dissimilarity"])
    pp = [None if np.isnan(p) else float(p) for p in g[f"{tag}_probability_parameters"]]
    args = (g[f"{tag}_XAHat"], g[f"{tag}_coordsB"], [g[f"{tag}_layerA{l}"] for l in range(n_layers)],
            [g[f"{tag}_layerB{l}"] for l in range(n_layers)])
    kw = dict(dissimilarity=[str(m) for m in g[f"{tag}_dissimilarity"]],
              probability_type=[str(p) for p in g[f"{tag}_probability_type"]], probability_parameters=pp,
              sigma2=float(g[f"{tag}_sigma2"]), alpha=g[f"{tag}_alpha"], SigmaDiag=g[f"{tag}_SigmaDiag"],
              gamma=float(g[f"{tag}_gamma"]), samples_s=float(g[f"{tag}_samples_s"]),
              sigma2_variance=float(g[f"{tag}_sigma2_variance"]))
    return args, kw


def _sq_dist(X, Y):
    return np.maximum((X**2).sum(1)[:, None] + (Y**2).sum(1)[None, :] - 2 * X.dot(Y.T), 0.0)


def _kl(X, Y):
    X, Y = X + 0.01, Y + 0.01
    X, Y = X / X.sum(1, keepdims=True), Y / Y.sum(1, keepdims=True)
    return (X * np.log(X + EPS)).sum(1, keepdims=True) - X.dot(np.log(Y + EPS).T)


def layer_distance(X, Y, metric):
    if metric in ("euc", "euclidean"):        # the reference's naming quirk: "euc" is the SQUARED distance
        return _sq_dist(X, Y)
    if metric in ("square_euc", "square_euclidean"):
        return np.sqrt(_sq_dist(X, Y))
    if metric == "kl":
        return _kl(X, Y)
    if metric == "sym_kl":
        return (_kl(X, Y) + _kl(Y, X).T) / 2
    if metric in ("cos", "cosine"):
        Xn = X / np.maximum(np.sqrt((X**2).sum(1, keepdims=True)), EPS)
        Yn = Y / np.maximum(np.sqrt((Y**2).sum(1, keepdims=True)), EPS)
        return -Xn.dot(Yn.T) * 0.5 + 0.5
    raise ValueError(metric)


def layer_probability(d, kind, param):
    kind = kind.lower()
    if kind in ("gauss", "gaussian"):
        return np.exp(-d / (2 * param))
    if kind in ("cos", "cosine"):
        return 1 - d
    if kind == "prob":
        return d
    raise ValueError(kind)


def restatement(XAHat, coordsB, layers_A, layers_B, *, dissimilarity, probability_type, probability_parameters, sigma2,
                alpha, SigmaDiag, gamma, samples_s, sigma2_variance=1.0, return_P=False, chunk=None):
    """The assignment step in float64 NumPy.  `chunk`: B columns per piece (every sum over i is per column, so the
    pieces are independent; only the row sums are accumulated over the pieces)."""
    XA, XB = np.asarray(XAHat, dtype=np.float64), np.asarray(coordsB, dtype=np.float64)
    NA, D = XA.shape
    NB = len(XB)
    if probability_parameters is None:
        probability_parameters = [None] * len(layers_A)
    m = (np.asarray(alpha, dtype=np.float64) * np.exp(-np.asarray(SigmaDiag, dtype=np.float64) / sigma2))[:, None]
    o = np.power(2 * np.pi * sigma2, D / 2) * (1 - gamma) / (gamma * (samples_s * NA))
    out = {q: np.zeros(NA) for q in ("K_NA", "K_NA_spatial", "K_NA_sigma2")}
    out["K_NB"], out["PXB"], s2r = np.zeros(NB), np.zeros((NA, D)), 0.0
    P_all = np.zeros((NA, NB)) if return_P else None
    step = NB if chunk is None else int(chunk)
    for lo in range(0, NB, step):
        sl = slice(lo, min(lo + step, NB))
        d = _sq_dist(XA, XB[sl])
        e1 = np.exp(-d / (2 * (sigma2 / sigma2_variance)))
        inl = 1 - o / (o + e1.sum(0, keepdims=True))
        e1 = e1 * m
        out["K_NA_spatial"] += (e1 / (o + e1.sum(0, keepdims=True))).sum(1)
        e2 = np.exp(-d / (2 * sigma2)) * m
        P2 = inl * e2 / (e2.sum(0, keepdims=True) + EPS)
        out["K_NA_sigma2"] += P2.sum(1)
        s2r += (P2 * d).sum()
        for A, B, met, kind, par in zip(layers_A, layers_B, dissimilarity, probability_type, probability_parameters):
            e2 = e2 * layer_probability(layer_distance(np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)[sl],
                                                       met), kind, par)
        P = inl * e2 / (e2.sum(0, keepdims=True) + EPS)
        out["K_NA"] += P.sum(1)
        out["K_NB"][sl] = P.sum(0)
        out["PXB"] += P.dot(XB[sl])
        if return_P:
            P_all[:, sl] = P
    out["Sp"], out["Sp_spatial"], out["Sp_sigma2"] = out["K_NB"].sum(), out["K_NA_spatial"].sum(), out["K_NA_sigma2"].sum()
    out["sigma2_related"] = s2r / (D * out["Sp_sigma2"])
    if return_P:
        out["P"] = P_all
    return out


def deviations(got, ref):
    """{quantity: max |got - ref| / max |ref|}; shapes and dtypes are asserted on the way."""
    dev = {}
    for q in QUANTITIES:
        a, b = np.asarray(got[q]), np.asarray(ref[q])
        assert a.shape == b.shape and a.dtype == np.float64, (q, a.shape, b.shape, a.dtype)
        assert np.isfinite(a).all(), q
        dev[q] = float(np.abs(a - b).max() / np.abs(b).max())
    return dev


def golden_ref(g, tag):
    return {q: g[f"{tag}_{q}"] for q in QUANTITIES}


F64_TOL = 1e-10   # exponent arguments up to ~700 carry a few ulps: <= ~1e-12 per positive term (SigmaInv's bound in _align_case)
F32_BASE = 1e-5   # _align_case's float32 bound
ALLOW = 1.25      # tests/_floors.py: a GPU result may sit at most this factor above the reference's own float32 floor


def tolerances(g, tag, dtype):
    """{quantity: bound}: float64 1e-10; float32 max(1.25 x the reference's own float32 floor of that quantity, 1e-5)."""
    if dtype == "float64":
        return {q: F64_TOL for q in QUANTITIES}
    floor = dict(zip([str(q) for q in g["quantities"]], g[f"{tag}_floor_f32"]))
    return {q: max(ALLOW * float(floor[q]), F32_BASE) for q in QUANTITIES}


def check(got, ref, tols, what=""):
    """Print every figure, then assert; returns the worst deviation / bound ratio."""
    dev = deviations(got, ref)
    print(f"  {what}: " + ", ".join(f"{q} {dev[q]:.2e}" for q in QUANTITIES))
    worst = max(dev[q] / tols[q] for q in QUANTITIES)
    for q in QUANTITIES:
        assert dev[q] <= tols[q], (what, q, dev[q], tols[q])
    return worst
