"""Shared by the CPU and GPU suites of the alignment loop (``spateo_amd.align.morpho_iterate``): the cases of
tests/golden/ref_align_loop.npz, a float64 NumPy restatement of the loop (test infrastructure, written from the formulas
below, built on tests/_assign_case.py's restatement of the assignment) and NumPy references of the three kernels of
csrc/mvf_align.hip.

One iteration k, from XAHat, RnA, VnA, alpha, SigmaDiag, sigma2, gamma, sigma2_variance, R, t (initially XAHat = RnA =
coordsA, VnA = 0, alpha = 1, SigmaDiag = 0, gamma = 0.5, sigma2_variance = 1, R = I):

    assignment   (_assign_case.restatement)  ->  K_NA, K_NB, K_NA_spatial, K_NA_sigma2, PXB = P coordsB, the three Sp, sigma2_related
    gamma      = clamp(exp(psi(gamma_a + Sp_spatial) - psi(gamma_a + gamma_b + NB)), 0.01, 0.99)
    alpha_i    = exp(psi(kappa_i + K_NA_spatial_i) - psi(kappa_i NA + Sp_spatial))
    non-rigid  (k > nonrigid_start_iter):  SigmaInv = sigma2 lambdaVF Gamma + U^T diag(K_NA) U,  Coff = pinv(SigmaInv) U^T
                 (PXB - RnA K_NA),  VnA = U Coff,  SigmaDiag = sigma2 diag(U pinv(SigmaInv) U^T)
    rigid        w = sigma2 nn_init_weight Sp / sum(inlier_P) (0 without inliers);  S_B = K_NB.coordsB + w inlier_P^T inlier_B,
                 S_A likewise, deno = Sp + w sum(inlier_P);  mu_XB = S_B / deno, mu_XA = S_A / deno, mu_Vn = K_NA.VnA / Sp
                 A = -(XA_hat^T diag(K_NA) VnA_hat - XA_hat^T (PXB - K_NA mu_XB^T))^T - w ((inlier_A - mu_XA) inlier_P)^T
                 (-(inlier_B - mu_XB)))^T;   U S V = svd(A), R = U diag(1, .., det(U V)) V
                 t = (S_B - K_NA.VnA - S_A R^T + w inlier_P^T (inlier_B - inlier_A R^T)) / deno     (the reference's in-place
                 ``mu_XB += ...`` makes its translation read the AUGMENTED sums S_B, S_A: reproduced, not repaired)
                 RnA = coordsA R^T + t;  XAHat = VnA + RnA
    sigma2     = max(sigma2_related + K_NA_sigma2.SigmaDiag / Sp_sigma2, 1e-3), and max(., 1e-2) while k < 100
    sigma2_variance = min(sigma2_variance (partial_robust_level)^(1/100), partial_robust_level)
after the loop:  mu_A = K_NA.coordsA / Sp, mu_B = K_NB.coordsB / Sp, A = ((PXB - K_NA mu_B^T)^T (coordsA - mu_A)),
                 optimal_R from its SVD as above, optimal_t = mu_B - mu_A optimal_R^T.

``origin`` (case 4): the assignment and PXB_term are taken on coordinates relative to it (translation invariant
quantities); everything else sees the coordinates as given.  ``wrong=`` selects one targeted wrong answer."""
import math
import os

import numpy as np

import _assign_case as ac

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_align_loop.npz")
SCALARS = ("sigma2", "gamma", "R", "t", "Sp")
ARRAYS = ("alpha", "XAHat", "VnA", "K_NA", "Coff")
FINALS = ("optimal_R", "optimal_t")
HOST_TOL = 1e-12   # the project's figure for its reference proofs
F64_TOL = ac.F64_TOL
F32_BASE = ac.F32_BASE
ALLOW = ac.ALLOW
_CACHE = {}


def load():
    if "g" not in _CACHE:
        _CACHE["g"] = np.load(GOLDEN)
    return _CACHE["g"]


def case_tags(g=None):
    return [str(t) for t in (g or load())["cases"]]


def case_inputs(g, tag):
    """(positional arguments, keyword arguments) of morpho_iterate / restatement for one golden case."""
    src = str(g[f"{tag}_layers_of"]) if f"{tag}_layers_of" in g.files else tag
    n_layers = len(g[f"{tag}_dissimilarity"])
    pp = [None if np.isnan(p) else float(p) for p in g[f"{tag}_probability_parameters"]]
    args = (g[f"{tag}_coordsA"], g[f"{tag}_coordsB"], [g[f"{src}_layerA{l}"] for l in range(n_layers)],
            [g[f"{src}_layerB{l}"] for l in range(n_layers)])
    kw = dict(dissimilarity=[str(m) for m in g[f"{tag}_dissimilarity"]],
              probability_type=[str(p) for p in g[f"{tag}_probability_type"]], probability_parameters=pp,
              inducing_variables=g[f"{tag}_inducing_variables"], beta=float(g[f"{tag}_beta"]),
              lambdaVF=float(g[f"{tag}_lambdaVF"]), sigma2=float(g[f"{tag}_sigma2_init"]), max_iter=int(g["iters"]),
              nonrigid_start_iter=int(g[f"{tag}_nonrigid_start_iter"]), kappa=float(g[f"{tag}_kappa"]),
              gamma_a=float(g[f"{tag}_gamma_a"]), gamma_b=float(g[f"{tag}_gamma_b"]),
              partial_robust_level=float(g[f"{tag}_partial_robust_level"]), samples_s=float(g[f"{tag}_samples_s"]),
              nn_init_weight=float(g[f"{tag}_nn_init_weight"]))
    if f"{tag}_inlier_A" in g.files:
        kw["inliers"] = (g[f"{tag}_inlier_A"], g[f"{tag}_inlier_B"], g[f"{tag}_inlier_P"])
    if np.any(g[f"{tag}_origin"] != 0):
        kw["origin"] = g[f"{tag}_origin"]
    return args, kw


def golden_ref(g, tag):
    return {q: g[f"{tag}_{q}"] for q in SCALARS + ARRAYS + FINALS}


# ---- digamma --------------------------------------------------------------------------------------------------------
def digamma(x):
    """psi(x), x > 0 (array): recurrence up to 10, then the asymptotic series through x^-14 - the formula of the device
    function and of spateo_amd.align._digamma, vectorised."""
    x = np.array(x, dtype=np.float64)
    s = np.zeros_like(x)
    for _ in range(10):
        low = x < 10.0
        s = np.where(low, s + 1.0 / x, s)
        x = np.where(low, x + 1.0, x)
    r = 1.0 / x
    r2 = r * r
    p = np.full_like(x, 1.0 / 12.0)
    for c in (-691.0 / 32760.0, 1.0 / 132.0, -1.0 / 240.0, 1.0 / 252.0, -1.0 / 120.0, 1.0 / 12.0):
        p = p * r2 + c
    return ((np.log(x) - 0.5 * r) - p * r2) - s


# ---- the loop -------------------------------------------------------------------------------------------------------
def _kernel(X, Y, beta):
    return np.exp(-beta * ac._sq_dist(X, Y))


def _rotation(A):
    U, _, V = np.linalg.svd(A)
    C = np.eye(len(A))
    C[-1, -1] = np.linalg.det(U @ V)
    return U @ C @ V


def restatement(coordsA, coordsB, layers_A, layers_B, *, dissimilarity, probability_type, probability_parameters,
                inducing_variables, beta, lambdaVF, sigma2, max_iter, nonrigid_start_iter=0, kappa=1.0, gamma_a=1.0, gamma_b=1.0,
                partial_robust_level=10, samples_s=None, inliers=None, nn_init_weight=1.0, origin=None, wrong=None, psi=None):
    """The loop in float64 NumPy; returns per-iteration lists of every compared quantity and the finals.
    wrong: None | "raw_moments" | "no_zero_rule" | "kappa_sum" | "late_floor".  psi: the digamma function, by default
    scipy.special.psi (the restatement is about the loop; the project's own digamma formula - `digamma` above - is proven
    against scipy.special.psi on its own in tests/test_align_loop_host.py.  The loop amplifies: cond(SigmaInv) is 3.6e5 in
    case 1, and the last place of one psi value moves Coff by 1e-11 eight iterations later)."""
    from scipy.linalg import pinv
    from scipy.special import psi as scipy_psi

    psi = scipy_psi if psi is None else psi

    XA, XB = np.asarray(coordsA, dtype=np.float64), np.asarray(coordsB, dtype=np.float64)
    NA, D = XA.shape
    NB = len(XB)
    o = np.zeros(D) if origin is None else np.asarray(origin, dtype=np.float64)
    ctrl = np.asarray(inducing_variables, dtype=np.float64)
    U, Gamma = _kernel(XA - o, ctrl - o, beta), _kernel(ctrl - o, ctrl - o, beta)
    kap = np.broadcast_to(np.asarray(kappa, dtype=np.float64), (NA,)).copy()
    alpha, SigmaDiag, VnA = np.ones(NA), np.zeros(NA), np.zeros((NA, D))
    XAHat, RnA = XA.copy(), XA.copy()
    Coff = np.zeros((len(ctrl), D))
    gamma, s2v, R = 0.5, 1.0, np.eye(D)
    step = np.power(partial_robust_level / 1.0, 1.0 / 100)
    nonrigid = False
    hist = {q: [] for q in SCALARS + ARRAYS}
    for it in range(max_iter):
        a = ac.restatement(XAHat - o, XB - o, layers_A, layers_B, dissimilarity=dissimilarity, probability_type=probability_type,
                           probability_parameters=probability_parameters, sigma2=sigma2, alpha=alpha, SigmaDiag=SigmaDiag,
                           gamma=gamma, samples_s=samples_s, sigma2_variance=s2v, return_P=True)
        P, K_NA, K_NB = a["P"], a["K_NA"], a["K_NB"]
        Sp = P.sum()
        gamma = float(np.clip(np.exp(psi(gamma_a + a["Sp_spatial"]) - psi(gamma_a + gamma_b + NB)), 0.01, 0.99))
        kNA = kap.sum() if wrong == "kappa_sum" else kap * NA
        alpha = np.exp(psi(kap + a["K_NA_spatial"]) - psi(kNA + a["Sp_spatial"]))
        if it > nonrigid_start_iter or nonrigid:
            nonrigid = True
            PXB_term = P.dot(XB - o) - (RnA - o) * K_NA[:, None]
            SigmaInv = sigma2 * lambdaVF * Gamma + U.T.dot(U * K_NA[:, None])
            if wrong == "no_zero_rule":   # the right-hand side through Y = PXB_term / K_NA without the K_NA == 0 rule: 0 / 0
                with np.errstate(divide="ignore", invalid="ignore"):
                    rhs = U.T.dot((PXB_term / K_NA[:, None]) * K_NA[:, None])
                if not np.isfinite(rhs).all():
                    return None
            else:
                rhs = U.T.dot(PXB_term)
            Sigma = pinv(SigmaInv)
            Coff = Sigma.dot(rhs)
            VnA = U.dot(Coff)
            # diag(U Sigma U^T)_i = sum_j U_ij (Sigma U^T)_ji: the products first, then each row's sum in index order
            SigmaDiag = sigma2 * np.einsum("ij->i", np.einsum("ij,ji->ij", U, Sigma.dot(U.T)))
        # ---- rigid ----
        S_A, S_V, S_B = K_NA.dot(XA), K_NA.dot(VnA), K_NB.dot(XB)
        deno, w = Sp, 0.0
        if inliers is not None:
            iA, iB, iP = (np.asarray(v, dtype=np.float64) for v in inliers)
            iP = iP.reshape(-1, 1)
            w = sigma2 * nn_init_weight * Sp / iP.sum()
            S_B, S_A = S_B + w * iP.T.dot(iB)[0], S_A + w * iP.T.dot(iA)[0]
            deno = Sp + w * iP.sum()
        mu_XB, mu_XA, mu_Vn = S_B / deno, S_A / deno, S_V / Sp
        if wrong == "raw_moments":   # raw second moments, the means taken out afterwards
            M1 = XA.T.dot(VnA * K_NA[:, None]) - np.outer(mu_XA, S_V) - np.outer(K_NA.dot(XA), mu_Vn) + Sp * np.outer(mu_XA, mu_Vn)
            M2 = XA.T.dot(P).dot(XB) - np.outer(mu_XA, K_NB.dot(XB)) - np.outer(K_NA.dot(XA), mu_XB) + Sp * np.outer(mu_XA, mu_XB)
        else:
            XA_hat, Vn_hat, XB_hat = XA - mu_XA, VnA - mu_Vn, XB - mu_XB
            M1 = XA_hat.T.dot(Vn_hat * K_NA[:, None])
            M2 = XA_hat.T.dot(P).dot(XB_hat)
        A = -(M1 - M2).T
        if inliers is not None:
            A = A - w * ((iA - mu_XA) * iP).T.dot(-(iB - mu_XB)).T
        R = _rotation(A)
        t_num = S_B - S_V - S_A.dot(R.T)
        if inliers is not None:
            t_num = t_num + w * iP.T.dot(iB - iA.dot(R.T))[0]
        t = t_num / deno
        RnA = XA.dot(R.T) + t
        XAHat = VnA + RnA
        # ---- sigma2 ----
        sigma2 = max(a["sigma2_related"] + K_NA_s2_dot(a["K_NA_sigma2"], SigmaDiag) / a["Sp_sigma2"], 1e-3)
        s2v = min(s2v * step, partial_robust_level)
        if (it >= 100) if wrong == "late_floor" else (it < 100):
            sigma2 = max(sigma2, 1e-2)
        for q, v in (("sigma2", sigma2), ("gamma", gamma), ("R", R), ("t", t), ("Sp", Sp), ("alpha", alpha), ("XAHat", XAHat),
                     ("VnA", VnA), ("K_NA", K_NA), ("Coff", Coff)):
            hist[q].append(np.array(v, dtype=np.float64))
    mu_A, mu_B = K_NA.dot(XA) / Sp, K_NB.dot(XB) / Sp
    if wrong == "raw_moments":
        A = (XA.T.dot(P).dot(XB) - np.outer(mu_A, K_NB.dot(XB)) - np.outer(K_NA.dot(XA), mu_B) + Sp * np.outer(mu_A, mu_B)).T
    else:
        A = P.dot(XB - mu_B).T.dot(XA - mu_A)
    out = {q: np.array(v) for q, v in hist.items()}
    out["optimal_R"] = _rotation(A)
    out["optimal_t"] = mu_B - mu_A.dot(out["optimal_R"].T)
    out["sigma2_variance"] = s2v
    return out


def K_NA_s2_dot(K_NA_sigma2, SigmaDiag):
    return float(np.einsum("i,i", K_NA_sigma2, SigmaDiag))


# ---- comparison -----------------------------------------------------------------------------------------------------
def rel(a, b):
    """max |a - b| / max |b| per leading index; the absolute deviation where b is all zero (VnA, Coff before the non-rigid
    update has run)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all()
    n = len(b)
    d = np.abs(a - b).reshape(n, -1).max(1)
    m = np.abs(b).reshape(n, -1).max(1)
    return np.where(m > 0, d / np.where(m > 0, m, 1.0), d)


def deviations(got, g, tag):
    """{quantity: per stored iteration deviation from the fixture}.  `got` holds every iteration of the scalars and either
    every iteration or the stored ones of the arrays."""
    arr = [int(i) for i in g["arr_iters"]]
    dev = {}
    for q in SCALARS:
        dev[q] = rel(got[q], g[f"{tag}_{q}"])
    for q in ARRAYS:
        v = np.asarray(got[q])
        dev[q] = rel(v[arr] if len(v) == int(g["iters"]) else v, g[f"{tag}_{q}"])
    for q in FINALS:
        dev[q] = rel(np.asarray(got[q])[None], g[f"{tag}_{q}"][None])
    return dev


def bounds(g, tag, base, f32=False, skip=()):
    """{quantity: per stored iteration bound}: base max(1, 1.25 g_k); float32: max(1.25 x the reference's own float32
    floor, that)."""
    out = {}
    for q in SCALARS + ARRAYS + FINALS:
        if q in skip:
            continue
        b = base * np.maximum(1.0, ALLOW * g[f"{tag}_g_{q}"])
        if f32:
            b = np.maximum(ALLOW * g[f"{tag}_f32_{q}"], b)
        out[q] = b
    return out


def check(dev, tol, what=""):
    """Print the worst ratio per quantity, then assert; returns {quantity: worst deviation / bound}."""
    ratio = {q: float((dev[q] / tol[q]).max()) for q in tol}
    print(f"  {what}: " + ", ".join(f"{q} {dev[q].max():.2e} ({ratio[q]:.2g}x)" for q in tol))
    for q in tol:
        assert np.all(dev[q] <= tol[q]), (what, q, dev[q], tol[q])
    return ratio


# ---- NumPy references of the three kernels ---------------------------------------------------------------------------
def alpha_reference(kappa, K_NA_spatial, SigmaDiag, Sp_spatial, sigma2):
    from scipy.special import psi

    n = len(kappa)
    alpha = np.exp(psi(kappa + K_NA_spatial) - psi(kappa * n + Sp_spatial))
    return alpha, alpha * np.exp(-SigmaDiag / sigma2)


def transform_reference(A, V, PXB, K, R, t, origin, npdt):
    """mvf_align_transform in the operation order its header states (A, V, PXB n x 3 float64; V already widened).  Returns
    RnA, XAHat, xa4, PXB_term, Y4, Pw with the cell-dtype outputs rounded by NumPy."""
    R, t, o = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64), np.asarray(origin, dtype=np.float64)
    n = len(A)
    RnA = np.empty((n, 3))
    for d in range(3):
        RnA[:, d] = ((A[:, 0] * R[d, 0] + A[:, 1] * R[d, 1]) + A[:, 2] * R[d, 2]) + t[d]
    XAHat = V + RnA
    xa4 = np.zeros((n, 4), dtype=npdt)
    xa4[:, :3] = (XAHat - o).astype(npdt)
    PXB_term = PXB - (RnA - o) * K[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        Y = np.where(K[:, None] != 0, PXB_term / K[:, None], 0.0)
    Y4 = np.zeros((n, 4), dtype=npdt)
    Y4[:, :3] = Y.astype(npdt)
    return RnA, XAHat, xa4, PXB_term, Y4, K.astype(npdt)


def moments_reference(A, V, K, Ks, K2, sd, PXB, B, KB, origin, mu=None):
    """mvf_align_moments' block with math.fsum: (values (50,), sum |terms| (50,)).  The second-order sums are taken on rows
    centred by `mu` (9 values: what the device formed) or, when None, by the means of the fsum'd first-order sums."""
    f = math.fsum
    val, mag = np.zeros(50), np.zeros(50)

    def put(i, terms):
        terms = np.asarray(terms, dtype=np.float64)
        val[i], mag[i] = f(terms), f(np.abs(terms))

    for d in range(3):
        put(d, K * A[:, d]), put(3 + d, K * V[:, d]), put(6 + d, KB * B[:, d])
    put(9, KB), put(10, K), put(11, Ks), put(12, K2), put(13, K2 * sd)
    Sp = val[9]
    if mu is None:
        mu = val[:9] / Sp if Sp != 0 else np.zeros(9)
    mu = np.asarray(mu, dtype=np.float64)
    val[14:23], mag[14:23] = mu, np.abs(mu)
    xc, vc = A - mu[0:3], V - mu[3:6]
    pc = PXB - K[:, None] * (mu[6:9] - np.asarray(origin, dtype=np.float64))
    for a in range(3):
        for b in range(3):
            put(23 + 3 * a + b, (K * xc[:, a]) * vc[:, b])
            put(32 + 3 * a + b, xc[:, a] * pc[:, b])
        put(41 + a, K * xc[:, a]), put(44 + a, K * vc[:, a]), put(47 + a, pc[:, a])
    return val, mag
