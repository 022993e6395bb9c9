"""Shared by the CPU and GPU suites of the ``"label"`` layer of the alignment: the cases of
tests/golden/ref_assign_label.npz (tests/golden/make_golden_assign_label.py), a float64 NumPy restatement of the assignment
step with label layers (test infrastructure, written from the formulas of tests/_assign_case.py) and small synthetic cases
for the kernel-edge tests.

A label layer l contributes, with integer labels la_i (A) and lb_j (B) and the K x L table T,

    d_ij = T[la_i, lb_j]          q_ij <- q_ij p(d_ij),   p = d ("prob") | 1 - d ("cos") | exp(-d / (2 param)) ("gauss")

to the product of the layer probabilities q of tests/_assign_case.py; nothing else of the step changes.  A B label whose
column of T is zero for every A label present has S3_j = 0 and, by the 1e-8 in the denominator, P_ij = 0 exactly."""
import os

import numpy as np

import _assign_case as ac

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_assign_label.npz")
QUANTITIES = ac.QUANTITIES
_CACHE = {}


def load():
    if "g" not in _CACHE:
        _CACHE["g"] = np.load(GOLDEN)
    return _CACHE["g"]


class View:
    """The arrays of one loop of the file (prefix ``loop.`` / ``svi.``) under the keys of ref_align_loop.npz /
    ref_align_svi.npz, for the deviations / bounds of tests/_align_loop_case.py and tests/_align_svi_case.py."""

    def __init__(self, g, prefix):
        self.g, self.prefix = g, prefix
        self.files = [f[len(prefix):] for f in g.files if f.startswith(prefix)]

    def __getitem__(self, key):
        return self.g[self.prefix + key]


def case_tags(g=None):
    return [str(t) for t in (g or load())["cases"]]


def case_inputs(g, tag):
    """(positional arguments, keyword arguments) of update_assignment / restatement for one step case."""
    src = str(g[f"{tag}_inputs_of"])
    idx = [int(i) for i in g[f"{tag}_layer_index"]]
    pp = [None if np.isnan(p) else float(p) for p in g[f"{tag}_probability_parameters"]]
    args = (g[f"{src}_XAHat"], g[f"{src}_coordsB"], [g[f"{src}_layerA{l}"] for l in idx], [g[f"{src}_layerB{l}"] for l in idx])
    kw = dict(dissimilarity=[str(m) for m in g[f"{tag}_dissimilarity"]],
              probability_type=[str(p) for p in g[f"{tag}_probability_type"]], probability_parameters=pp,
              sigma2=float(g[f"{src}_sigma2"]), alpha=g[f"{src}_alpha"], SigmaDiag=g[f"{src}_SigmaDiag"],
              gamma=float(g[f"{src}_gamma"]), samples_s=float(g[f"{src}_samples_s"]),
              sigma2_variance=float(g[f"{src}_sigma2_variance"]), label_transfer=g[f"{src}_label_transfer"])
    return args, kw


def far_columns(g, tag):
    return g[f"{str(g[f'{tag}_inputs_of'])}_far"]


def golden_ref(g, tag, k=None):
    key = tag if k is None else f"{tag}_k{k}"
    return {q: g[f"{key}_{q}"] for q in QUANTITIES}


def tolerances(g, tag, dtype, k=None):
    """_assign_case.tolerances on this file's floors: float64 1e-10; float32 max(1.25 x the reference's own float32 floor of
    the quantity, 1e-5)."""
    if dtype == "float64":
        return {q: ac.F64_TOL for q in QUANTITIES}
    key = tag if k is None else f"{tag}_k{k}"
    floor = dict(zip([str(q) for q in g["quantities"]], g[f"{key}_floor_f32"]))
    return {q: max(ac.ALLOW * float(floor[q]), ac.F32_BASE) for q in QUANTITIES}


def loop_inputs(g):
    """(args, kw) of morpho_iterate for the dense loop case ``loop.L`` (the SVI case ``svi.S`` runs on the same inputs)."""
    v, t = View(g, "loop."), "L"
    pp = [None if np.isnan(p) else float(p) for p in v[f"{t}_probability_parameters"]]
    args = (v[f"{t}_coordsA"], v[f"{t}_coordsB"], [v[f"{t}_layerA0"], v[f"{t}_layerA1"]], [v[f"{t}_layerB0"], v[f"{t}_layerB1"]])
    kw = dict(dissimilarity=[str(m) for m in v[f"{t}_dissimilarity"]], probability_type=[str(p) for p in v[f"{t}_probability_type"]],
              probability_parameters=pp, label_transfer=v[f"{t}_label_transfer"], inducing_variables=v[f"{t}_inducing_variables"],
              beta=float(v[f"{t}_beta"]), lambdaVF=float(v[f"{t}_lambdaVF"]), sigma2=float(v[f"{t}_sigma2_init"]),
              max_iter=int(v["iters"]), nonrigid_start_iter=int(v[f"{t}_nonrigid_start_iter"]), kappa=float(v[f"{t}_kappa"]),
              gamma_a=float(v[f"{t}_gamma_a"]), gamma_b=float(v[f"{t}_gamma_b"]),
              partial_robust_level=float(v[f"{t}_partial_robust_level"]), samples_s=float(v[f"{t}_samples_s"]),
              nn_init_weight=float(v[f"{t}_nn_init_weight"]))
    return args, kw


def svi_inputs(g):
    v = View(g, "svi.")
    args, kw = loop_inputs(g)
    kw.update(max_iter=int(v["iters"]), nonrigid_start_iter=int(v["S_nonrigid_start_iter"]), batch_size=int(v["batch_size"]),
              batch_perm=v["S_batch_perm"].astype(np.int64))
    return args, kw


# ---- the restatement ----------------------------------------------------------------------------------------------------
def layer_probability(A, B, metric, kind, param, label_transfer):
    """The NA x NB probability matrix of one layer; a label layer reads the table."""
    if metric == "label":
        A, B = np.asarray(A), np.asarray(B)
        assert A.ndim == 1 and B.ndim == 1 and A.dtype.kind in "iu" and B.dtype.kind in "iu"
        d = np.asarray(label_transfer, dtype=np.float64)[A.astype(np.int64)[:, None], B.astype(np.int64)[None, :]]
    else:
        d = ac.layer_distance(np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64), metric)
    return ac.layer_probability(d, kind, param)


def restatement(XAHat, coordsB, layers_A, layers_B, *, dissimilarity, probability_type, probability_parameters, sigma2, alpha,
                SigmaDiag, gamma, samples_s, sigma2_variance=1.0, label_transfer=None, return_P=False, model_mul=None,
                outlier=None):
    """The assignment step in float64 NumPy with label layers.  `model_mul` / `outlier`: given directly (the raw C ABI's
    arguments) instead of through alpha, SigmaDiag, gamma and samples_s."""
    XA, XB = np.asarray(XAHat, dtype=np.float64), np.asarray(coordsB, dtype=np.float64)
    NA, D = XA.shape
    if probability_parameters is None:
        probability_parameters = [None] * len(layers_A)
    m = np.asarray(alpha, dtype=np.float64) * np.exp(-np.asarray(SigmaDiag, dtype=np.float64) / sigma2) if model_mul is None else model_mul
    m = np.asarray(m, dtype=np.float64)[:, None]
    o = np.power(2 * np.pi * sigma2, D / 2) * (1 - gamma) / (gamma * (samples_s * NA)) if outlier is None else outlier
    d = ac._sq_dist(XA, XB)
    e1 = np.exp(-d / (2 * (sigma2 / sigma2_variance)))
    inl = 1 - o / (o + e1.sum(0, keepdims=True))
    e1 = e1 * m
    out = {"K_NA_spatial": (e1 / (o + e1.sum(0, keepdims=True))).sum(1)}
    e2 = np.exp(-d / (2 * sigma2)) * m
    P2 = inl * e2 / (e2.sum(0, keepdims=True) + ac.EPS)
    out["K_NA_sigma2"] = P2.sum(1)
    s2r = (P2 * d).sum()
    for A, B, met, kind, par in zip(layers_A, layers_B, dissimilarity, probability_type, probability_parameters):
        e2 = e2 * layer_probability(A, B, met, kind, par, label_transfer)
    P = inl * e2 / (e2.sum(0, keepdims=True) + ac.EPS)
    out["K_NA"], out["K_NB"], out["PXB"] = P.sum(1), P.sum(0), P.dot(XB)
    out["Sp"], out["Sp_spatial"], out["Sp_sigma2"] = out["K_NB"].sum(), out["K_NA_spatial"].sum(), out["K_NA_sigma2"].sum()
    out["sigma2_related"] = s2r / (D * out["Sp_sigma2"])
    if return_P:
        out["P"] = P
    return out


# ---- small synthetic cases for the kernel edges ---------------------------------------------------------------------------
def edge_table(rng, K, L):
    """Multiples of 1/64 in (0, 1], all different where K L <= 63: a transposed or shifted look-up shows."""
    return (rng.permutation(63)[: K * L].reshape(K, L) + 1.0) / 64.0 if K * L <= 63 else rng.integers(1, 64, (K, L)) / 64.0


def edge_case(NA, NB, K, L, seed=0, D=3, expression=True):
    """NA x NB cells within reach of each other, one label layer (every label of both sides drawn, the last row and the last
    column of the table among them where the sizes allow) and, with `expression`, one small euc layer before it."""
    rng = np.random.default_rng(1000 * NA + NB + 7 * K + L + seed)
    XA = rng.standard_normal((NA, D))
    XB = XA[rng.choice(NA, NB)] + 0.2 * rng.standard_normal((NB, D))
    labA, labB = rng.integers(0, K, NA), rng.integers(0, L, NB)
    labA[-1], labB[-1] = K - 1, L - 1
    layers_A, layers_B, met, kinds, pars = [labA], [labB], ["label"], ["prob"], [None]
    if expression:
        cent = rng.standard_normal((max(K, L), 5))
        layers_A.insert(0, np.round((cent[labA] + 0.5 * rng.standard_normal((NA, 5))) * 32) / 32)
        layers_B.insert(0, np.round((cent[labB] + 0.5 * rng.standard_normal((NB, 5))) * 32) / 32)
        met, kinds, pars = ["euc", "label"], ["gauss", "prob"], [4.0, None]
    sigma2 = 0.3
    return dict(XA=XA, XB=XB, layers_A=layers_A, layers_B=layers_B, dissimilarity=met, probability_type=kinds,
                probability_parameters=pars, label_transfer=edge_table(rng, K, L), sigma2=sigma2,
                alpha=rng.uniform(0.5, 1.0, NA), SigmaDiag=sigma2 * rng.uniform(0.0, 0.3, NA), gamma=0.5,
                samples_s=float(np.prod(XA.max(0) - XA.min(0))) if NA > 1 else 1.0, sigma2_variance=1.5)


EDGE_SHAPES = [(1, 1, 1, 1), (63, 65, 5, 4), (64, 64, 1, 3), (65, 129, 4, 1), (65, 129, 7, 9)]   # (NA, NB, K, L)
