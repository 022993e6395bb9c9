"""The NumPy restatement of ``spateo_amd.align.pca`` and the cases its tests share (no test in here).

Restatement: centre -> ``np.linalg.svd`` -> the sign rule (``restate``); a second route through ``np.linalg.eigh`` of
``Xc^T Xc`` (``restate_eigh``) gives the reference's own noise floor.  Inputs have a planted spectrum (``planted``) so that
every component is individually defined.  ``bounds`` turns the two routes into the tolerances of the parity tests:

    floor_i = || v_svd_i - v_eigh_i ||_2          (the disagreement of the two CPU routes, per component)
    gap_i   = the oracle's distance from lambda_i to its nearest other eigenvalue (all G of them)
    tol_i   = max(1.25 floor_i, G eps lambda_1 / gap_i)      component i:  || v_dev - v_or ||_2 <= tol_i
    score column i:  max_n |delta| <= tol_i max_n || xc_n ||_2    (+ 2^-24 max |score| where the device stores float32 scores)
    variances:       |delta| <= max(1.25 floor_var, G eps) lambda_1,   floor_var = max_i |var_svd_i - var_eigh_i| / lambda_1

1.25 is this project's margin over a reference floor; G eps lambda_1 / gap_i is the first-order perturbation bound of an
eigenvector under a relative perturbation eps of the matrix, with its dimension factor.  eps is float64's in both modes: the
float32 mode's oracle runs on the centred operand rounded to float32, which is what the device stores, and the Gram matrix of
those values is accumulated in float64 (a product of two float32 values is exact in float64).

``ublk_layout`` is the NumPy statement of the cache layout the kernel-level tests compare bit for bit."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)


def sign_rule(V):
    """Every column scaled by +-1 so that its entry of largest magnitude is positive (lowest index on ties)."""
    V = np.array(V, dtype=np.float64)
    for i in range(V.shape[1]):
        j = int(np.argmax(np.abs(V[:, i])))
        if V[j, i] < 0:
            V[:, i] = -V[:, i]
    return V


def planted(n, g, k, seed, offset=True):
    """Z diag(s) Q^T + offset: Z (n, g) standard normal, Q orthogonal, s geometric with ratio 0.8 over the first k + 3
    directions and 1e-3 after."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, g))
    Q, _ = np.linalg.qr(rng.standard_normal((g, g)))
    s = np.full(g, 1e-3)
    lead = min(g, k + 3)
    s[:lead] = 0.8 ** np.arange(lead)
    X = (Z * s) @ Q.T
    if offset:
        X = X + rng.uniform(-2.0, 2.0, g)
    return X


def clip_k(n_comps, N, G):
    return min(int(n_comps), min(N, G) - 1)


def _finish(Xc, V, lam_all, k, dof):
    V = sign_rule(V[:, :k])
    lam = lam_all[:k]
    return {"PCs": V, "scores": Xc @ V, "variance": lam / dof, "variance_ratio": lam / lam_all.sum(), "lam_all": lam_all / dof}


def centred(X, zero_center=True):
    """(Xc float64, mean, the divisor of the variances)."""
    X = np.asarray(X, dtype=np.float64)
    if not zero_center:
        return X, np.zeros(X.shape[1]), X.shape[0]
    mean = X.mean(axis=0)
    return X - mean, mean, X.shape[0] - 1


def restate(Xc, k, dof):
    """PCA of an operand that is already centred (or deliberately not), through the SVD."""
    Xc = np.asarray(Xc, dtype=np.float64)
    _, s, Vt = np.linalg.svd(Xc, full_matrices=False)
    lam_all = np.zeros(Xc.shape[1])
    lam_all[: len(s)] = s * s
    V = np.zeros((Xc.shape[1], max(k, 1)))
    V[:, : min(k, Vt.shape[0])] = Vt[:k].T
    return _finish(Xc, V, lam_all, k, dof)


def restate_eigh(Xc, k, dof):
    """The same through the symmetric eigenproblem of Xc^T Xc."""
    Xc = np.asarray(Xc, dtype=np.float64)
    w, Q = np.linalg.eigh(Xc.T @ Xc)
    return _finish(Xc, Q[:, ::-1], np.maximum(w[::-1], 0.0), k, dof)


def bounds(Xc, k, dof):
    """(oracle, tol (k,), score_scale, var_tol) as the module docstring states them."""
    a, b = restate(Xc, k, dof), restate_eigh(Xc, k, dof)
    floor = np.linalg.norm(a["PCs"] - b["PCs"], axis=0)
    lam = a["lam_all"]
    G = Xc.shape[1]
    gap = np.array([np.abs(np.delete(lam, i) - lam[i]).min() for i in range(k)])
    tol = np.maximum(1.25 * floor, G * EPS * lam[0] / gap)
    floor_var = np.abs(a["variance"] - b["variance"]).max() / lam[0]
    var_tol = max(1.25 * floor_var, G * EPS) * lam[0]
    return a, tol, float(np.linalg.norm(Xc, axis=1).max()), float(var_tol)


def check_against(res_pcs, res_scores, res_var, Xc, k, dof, score_extra=0.0, label=""):
    """The parity assertions; returns the measured maxima relative to their bounds (printed by the caller)."""
    orc, tol, scale, var_tol = bounds(Xc, k, dof)
    dv = np.linalg.norm(res_pcs - orc["PCs"], axis=0)
    ds = np.abs(res_scores - orc["scores"]).max(axis=0)
    dl = np.abs(res_var - orc["variance"])
    s_tol = tol * scale + score_extra * np.abs(orc["scores"]).max()
    print(f"pca parity {label}: max |dv| {dv.max():.3e} (worst dv/tol {np.max(dv / tol):.3g}), max |dscore| {ds.max():.3e} "
          f"(worst/tol {np.max(ds / s_tol):.3g}), max |dvar| {dl.max():.3e} (tol {var_tol:.3e}), min tol {tol.min():.3e}")
    assert (dv <= tol).all(), (dv, tol)
    assert (ds <= s_tol).all(), (ds, s_tol)
    assert (dl <= var_tol).all(), (dl, var_tol)
    return float(dv.max()), float(ds.max()), float(dl.max())


def pads(n, g):
    return -(-n // 256) * 256, -(-g // 128) * 128


def ublk_layout(Xc):
    """An (n, g) array of the cell dtype as the flat cache Ublk[g_pad / 16][n_pad][16], zero padded."""
    n, g = Xc.shape
    n_pad, g_pad = pads(n, g)
    full = np.zeros((n_pad, g_pad), dtype=Xc.dtype)
    full[:n, :g] = Xc
    return np.ascontiguousarray(full.reshape(n_pad, g_pad // 16, 16).transpose(1, 0, 2)).reshape(-1)


def from_ublk(flat, n, g):
    """The inverse: the (n_pad, g_pad) matrix a flat cache holds."""
    n_pad, g_pad = pads(n, g)
    return np.ascontiguousarray(flat.reshape(g_pad // 16, n_pad, 16).transpose(1, 0, 2)).reshape(n_pad, g_pad)
