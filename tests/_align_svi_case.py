"""Shared by the CPU and GPU suites of the SVI mode of the alignment loop (``spateo_amd.align.morpho_iterate_svi``): the cases
of tests/golden/ref_align_svi.npz (their inputs are cases 1 - 3 of ref_align_loop.npz), a float64 NumPy restatement of the
SVI loop (test infrastructure, written from the formulas below on top of tests/_assign_case.py's restatement of the
assignment) and NumPy references of the three kernels the mode adds to csrc/mvf_align.hip.

Iteration k differs from the dense loop of tests/_align_loop_case.py in this (step = min(1, 10 / (k + 1)), bs = batch_size,
batch = perm[(j - k bs) mod NB], j < bs; the running Sp, Sp_spatial, Sp_sigma2, SigmaInv, PXB_term start at 0):

    assignment   on NA x coordsB[batch] / layers_B[batch];  Sp* <- step Sp*_now + (1 - step) Sp*;  sigma2_related = raw /
                 (D Sp_sigma2)
    gamma        with bs in place of NB and the blended Sp_spatial
    alpha      <- step exp(psi(kappa + K_NA_spatial) - psi(kappa NA + Sp_spatial)) + (1 - step) alpha
    non-rigid    SigmaInv <- step (sigma2 lambdaVF Gamma + U^T diag(K_NA) U) + (1 - step) SigmaInv, PXB_term <- step (P
                 coordsB[batch] - RnA K_NA) + (1 - step) PXB_term, Coff = pinv(SigmaInv) U^T PXB_term
    rigid        the sums K_NA.coordsA, K_NA.VnA, K_NB.coordsB[batch], XA_hat^T P XB_hat from the batch; every denominator and
                 the inlier weight from the blended Sp;  R <- step R + (1 - step) R_old BEFORE the translation reads it and
                 t <- step t + (1 - step) t_old, both only when step < 1
    sigma2     = max(sigma2_related + K_NA_sigma2.SigmaDiag / Sp_sigma2 (blended), floors)
after the loop:  optimal_R / optimal_t from the last batch with means over the blended Sp; or (return_mapping) one full
                 non-SVI assignment on the final state, its unblended Sp and the whole B slice."""
import os

import numpy as np

import _align_loop_case as lc
import _assign_case as ac

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_align_svi.npz")
SCALARS, ARRAYS = lc.SCALARS, lc.ARRAYS
FINALS = ("optimal_R", "optimal_t")
FINALS_MAP = ("optimal_R_map", "optimal_t_map", "Sp_map")
HOST_TOL, F64_TOL, F32_BASE, ALLOW = lc.HOST_TOL, lc.F64_TOL, lc.F32_BASE, lc.ALLOW
_CACHE = {}


def load():
    if "g" not in _CACHE:
        _CACHE["g"] = np.load(GOLDEN)
    return _CACHE["g"]


def case_tags(g=None):
    return [str(t) for t in (g or load())["cases"]]


def case_inputs(g, tag):
    """(positional arguments, keyword arguments) of morpho_iterate_svi / restatement for one golden case."""
    args, kw = lc.case_inputs(lc.load(), str(g[f"{tag}_inputs_of"]))
    kw.update(max_iter=int(g["iters"]), nonrigid_start_iter=int(g[f"{tag}_nonrigid_start_iter"]),
              batch_size=int(g["batch_size"]), batch_perm=g[f"{tag}_batch_perm"].astype(np.int64))
    return args, kw


def schedule(perm, bs, it):
    """batch_idx of iteration `it`: the head of the permutation after `it` rolls by bs (np.roll semantics)."""
    perm = np.asarray(perm)
    return perm[(np.arange(bs) - it * bs) % len(perm)]


def default_batch_size(NB):
    return min(max(int(NB / 10), 1000), NB)


def restatement(coordsA, coordsB, layers_A, layers_B, *, dissimilarity, probability_type, probability_parameters,
                inducing_variables, beta, lambdaVF, sigma2, max_iter, batch_size, batch_perm, nonrigid_start_iter=0, kappa=1.0,
                gamma_a=1.0, gamma_b=1.0, partial_robust_level=10, samples_s=None, inliers=None, nn_init_weight=1.0,
                return_mapping=False, psi=None):
    """The SVI loop in float64 NumPy; returns per-iteration lists of every compared quantity and the finals (both the
    last-batch and, with return_mapping, the full-assignment ones under the *_map names)."""
    from scipy.linalg import pinv
    from scipy.special import psi as scipy_psi

    psi = scipy_psi if psi is None else psi
    XA, XB = np.asarray(coordsA, dtype=np.float64), np.asarray(coordsB, dtype=np.float64)
    LB = [np.asarray(b, dtype=np.float64) for b in layers_B]
    NA, D = XA.shape
    NB = len(XB)
    bs = min(int(batch_size), NB)
    ctrl = np.asarray(inducing_variables, dtype=np.float64)
    U, Gamma = lc._kernel(XA, ctrl, beta), lc._kernel(ctrl, ctrl, beta)
    kap = np.broadcast_to(np.asarray(kappa, dtype=np.float64), (NA,)).copy()
    alpha, SigmaDiag, VnA = np.ones(NA), np.zeros(NA), np.zeros((NA, D))
    XAHat, RnA = XA.copy(), XA.copy()
    Coff = np.zeros((len(ctrl), D))
    gamma, s2v, R, t = 0.5, 1.0, np.eye(D), None
    anneal = np.power(partial_robust_level / 1.0, 1.0 / 100)
    Sp = Sp_spatial = Sp_sigma2 = 0.0
    SigmaInv, PXB_term = np.zeros((len(ctrl), len(ctrl))), np.zeros((NA, D))
    nonrigid = False
    akw = dict(dissimilarity=dissimilarity, probability_type=probability_type, probability_parameters=probability_parameters)
    hist = {q: [] for q in SCALARS + ARRAYS + ("batch_idx", "step_size")}
    for it in range(max_iter):
        step = min(1.0, 10.0 / (it + 1.0))
        idx = schedule(batch_perm, bs, it)
        XBb = XB[idx]
        a = ac.restatement(XAHat, XBb, layers_A, [b[idx] for b in LB], sigma2=sigma2, alpha=alpha, SigmaDiag=SigmaDiag,
                           gamma=gamma, samples_s=samples_s, sigma2_variance=s2v, return_P=True, **akw)
        P, K_NA, K_NB = a["P"], a["K_NA"], a["K_NB"]
        Sp_spatial = step * a["Sp_spatial"] + (1 - step) * Sp_spatial
        Sp = step * P.sum() + (1 - step) * Sp
        raw = a["sigma2_related"] * (D * a["Sp_sigma2"])
        Sp_sigma2 = step * a["Sp_sigma2"] + (1 - step) * Sp_sigma2
        sigma2_related = raw / (D * Sp_sigma2)
        gamma = float(np.clip(np.exp(psi(gamma_a + Sp_spatial) - psi(gamma_a + gamma_b + bs)), 0.01, 0.99))
        alpha = step * np.exp(psi(kap + a["K_NA_spatial"]) - psi(kap * NA + Sp_spatial)) + (1 - step) * alpha
        if it > nonrigid_start_iter or nonrigid:
            nonrigid = True
            new = sigma2 * lambdaVF * Gamma + U.T.dot(U * K_NA[:, None])
            SigmaInv = step * new + (1 - step) * SigmaInv
            PXB_term = step * (P.dot(XBb) - RnA * K_NA[:, None]) + (1 - step) * PXB_term
            Sigma = pinv(SigmaInv)
            Coff = Sigma.dot(U.T.dot(PXB_term))
            VnA = U.dot(Coff)
            SigmaDiag = sigma2 * np.einsum("ij->i", np.einsum("ij,ji->ij", U, Sigma.dot(U.T)))
        # ---- rigid ----
        S_A, S_V, S_B = K_NA.dot(XA), K_NA.dot(VnA), K_NB.dot(XBb)
        deno, w = Sp, 0.0
        if inliers is not None:
            iA, iB, iP = (np.asarray(v, dtype=np.float64) for v in inliers)
            iP = iP.reshape(-1, 1)
            w = sigma2 * nn_init_weight * Sp / iP.sum()
            S_B, S_A = S_B + w * iP.T.dot(iB)[0], S_A + w * iP.T.dot(iA)[0]
            deno = Sp + w * iP.sum()
        mu_XB, mu_XA, mu_Vn = S_B / deno, S_A / deno, S_V / Sp
        XA_hat, Vn_hat, XB_hat = XA - mu_XA, VnA - mu_Vn, XBb - mu_XB
        A = -(XA_hat.T.dot(Vn_hat * K_NA[:, None]) - XA_hat.T.dot(P).dot(XB_hat)).T
        if inliers is not None:
            A = A - w * ((iA - mu_XA) * iP).T.dot(-(iB - mu_XB)).T
        R_new = lc._rotation(A)
        R = step * R_new + (1 - step) * R if step < 1 else R_new
        t_num = S_B - S_V - S_A.dot(R.T)
        if inliers is not None:
            t_num = t_num + w * iP.T.dot(iB - iA.dot(R.T))[0]
        t_new = t_num / deno
        t = step * t_new + (1 - step) * t if step < 1 else t_new
        RnA = XA.dot(R.T) + t
        XAHat = VnA + RnA
        # ---- sigma2 ----
        sigma2 = max(sigma2_related + lc.K_NA_s2_dot(a["K_NA_sigma2"], SigmaDiag) / Sp_sigma2, 1e-3)
        s2v = min(s2v * anneal, partial_robust_level)
        if it < 100:
            sigma2 = max(sigma2, 1e-2)
        for q, v in (("sigma2", sigma2), ("gamma", gamma), ("R", R), ("t", t), ("Sp", Sp), ("alpha", alpha), ("XAHat", XAHat),
                     ("VnA", VnA), ("K_NA", K_NA), ("Coff", Coff), ("batch_idx", idx), ("step_size", step)):
            hist[q].append(np.array(v, dtype=np.float64))
    out = {q: np.array(v) for q, v in hist.items()}

    def optimal(P, K_NA, K_NB, XBs, Sp):
        mu_A, mu_B = K_NA.dot(XA) / Sp, K_NB.dot(XBs) / Sp
        Ropt = lc._rotation(P.dot(XBs - mu_B).T.dot(XA - mu_A))
        return Ropt, mu_B - mu_A.dot(Ropt.T)

    out["optimal_R"], out["optimal_t"] = optimal(P, K_NA, K_NB, XBb, Sp)
    if return_mapping:
        a = ac.restatement(XAHat, XB, layers_A, LB, sigma2=sigma2, alpha=alpha, SigmaDiag=SigmaDiag, gamma=gamma,
                           samples_s=samples_s, sigma2_variance=s2v, return_P=True, **akw)
        out["Sp_map"] = a["P"].sum()
        out["optimal_R_map"], out["optimal_t_map"] = optimal(a["P"], a["K_NA"], a["K_NB"], XB, out["Sp_map"])
    return out


# ---- comparison -----------------------------------------------------------------------------------------------------
def deviations(got, g, tag, finals=FINALS):
    """{quantity: per stored iteration deviation from the fixture}; `got` holds every iteration of the scalars and either
    every iteration or the stored ones of the arrays."""
    arr = [int(i) for i in g["arr_iters"]]
    dev = {q: lc.rel(got[q], g[f"{tag}_{q}"]) for q in SCALARS}
    for q in ARRAYS:
        v = np.asarray(got[q])
        dev[q] = lc.rel(v[arr] if len(v) == int(g["iters"]) else v, g[f"{tag}_{q}"])
    for q in finals:
        dev[q] = lc.rel(np.asarray(got[q], dtype=np.float64)[None], g[f"{tag}_{q}"][None])
    return dev


def bounds(g, tag, base, f32=False, skip=(), finals=FINALS):
    """{quantity: per stored iteration bound}: base max(1, 1.25 g_k); float32: max(1.25 x the reference's own float32
    floor, that) - the dense loop's rule (tests/_align_loop_case.py)."""
    out = {}
    for q in SCALARS + ARRAYS + tuple(finals):
        if q in skip:
            continue
        b = base * np.maximum(1.0, ALLOW * g[f"{tag}_g_{q}"])
        if f32:
            b = np.maximum(ALLOW * g[f"{tag}_f32_{q}"], b)
        out[q] = b
    return out


check = lc.check


# ---- NumPy references of the three kernels ---------------------------------------------------------------------------
def alpha_svi_reference(kappa, K_NA_spatial, SigmaDiag, Sp_spatial, sigma2, step, alpha):
    from scipy.special import psi

    n = len(kappa)
    a = np.exp(psi(kappa + K_NA_spatial) - psi(kappa * n + Sp_spatial))
    a = step * a + (1 - step) * alpha if step < 1 else a
    return a, a * np.exp(-SigmaDiag / sigma2)


def transform_svi_reference(RnA, PXB, K, origin, step, PXB_term, npdt):
    """mvf_align_transform_svi in the operation order include/mvf.h states.  Returns PXB_term, Y4, Pw."""
    o = np.asarray(origin, dtype=np.float64)
    now = PXB - (RnA - o) * K[:, None]
    out = (step * now) + ((1.0 - step) * PXB_term)
    Y4 = np.zeros((len(K), 4), dtype=npdt)
    Y4[:, :3] = out.astype(npdt)
    return out, Y4, K.astype(npdt)


# ---- the loops on NumPy stand-ins for the kernels ---------------------------------------------------------------------
import torch  # noqa: E402

import _cpu_kernels as ck  # noqa: E402
from spateo_amd._kernels import Layer  # noqa: E402


class CpuLoopKernels(ck.CpuKernels):
    """NumPy stand-ins for the kernels the alignment loops call (the seam spateo_amd._runtime._make_kernels), built from the
    references of this package: the host half of `morpho_iterate` / `morpho_iterate_svi` - schedule, blends, the rigid update
    from the block, the order of the stages - can then be held against the fixtures without a device.  `D` is the spatial
    dimension of the case (the stand-in assignment works on the D columns)."""
    D = 3

    def h2d_padded(self, a, width, tdtype, minus=None):
        a = np.asarray(a, dtype=np.float64)
        if minus is not None:
            a = a - minus
        buf = np.zeros((len(a), width))
        buf[:, :a.shape[1]] = a
        return torch.from_numpy(buf)

    def to_host(self, tensors, own_pinned=True):
        return [t.numpy().copy() for t in tensors]

    def assign_prepare(self, layer, metric, side):
        L = torch.from_numpy(np.ascontiguousarray(layer, dtype=np.float64))
        return L, torch.zeros(len(L), dtype=torch.float64), L.shape[1]

    def restated(self, xa4, xb4, layers, model_mul, sigma2, s2v, outlier, restatement=ac.restatement, **extra):
        """`restatement` (the assignment's, or a variant with `extra` keywords) on the arguments of an assignment kernel:
        (its result, XA, XB).  The layers are `Layer` records or plain 8-sequences."""
        inv = {0: "euc", 1: "square_euc", 2: "kl", 3: "sym_kl", 4: "cos"}
        invp = {0: "gauss", 1: "cos", 2: "prob"}
        layers = [Layer(*L) for L in layers]
        D = self.D
        XA, XB = ck._np(xa4)[:, :D], ck._np(xb4)[:, :D]
        NA = len(XA)
        # the assignment's restatement takes alpha, SigmaDiag, gamma, samples_s: model_mul goes in as alpha with SigmaDiag = 0,
        # and the outlier term o = (2 pi sigma2)^(D/2) (1 - g) / (g samples_s NA) is met with samples_s = 1 and g solved from it
        c = np.power(2 * np.pi * sigma2, D / 2) / NA
        a = restatement(XA, XB, [ck._np(L.Xp) for L in layers], [ck._np(L.Yp) for L in layers],
                        dissimilarity=[inv[L.metric] for L in layers], probability_type=[invp[L.prob] for L in layers],
                        probability_parameters=[L.param for L in layers], sigma2=sigma2, alpha=ck._np(model_mul),
                        SigmaDiag=np.zeros(NA), gamma=c / (outlier + c), samples_s=1.0, sigma2_variance=s2v, **extra)
        return a, XA, XB

    def assign_result(self, a, more=()):
        """A restatement's result as the dict of tensors HipKernels.assign returns, plus the keys `more`."""
        D = self.D
        pxb = np.zeros((len(a["K_NA"]), 3))
        pxb[:, :D] = a["PXB"]
        raw = a["sigma2_related"] * D * a["Sp_sigma2"]
        out = {q: torch.from_numpy(np.ascontiguousarray(a[q])) for q in ("K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2") + tuple(more)}
        out.update(PXB=torch.from_numpy(pxb), scalars=torch.tensor([raw], dtype=torch.float64))
        return out

    def assign(self, xa4, xb4, layers, model_mul, sigma2, s2v, outlier, dense=False):
        return self.assign_result(self.restated(xa4, xb4, layers, model_mul, sigma2, s2v, outlier)[0])

    def align_alpha(self, kappa, Ks, sd, Sp_spatial, sigma2, alpha, model_mul):
        a, m = lc.alpha_reference(ck._np(kappa), ck._np(Ks), ck._np(sd), Sp_spatial, sigma2)
        alpha.copy_(torch.from_numpy(a))
        model_mul.copy_(torch.from_numpy(m))

    def align_alpha_svi(self, kappa, Ks, sd, Sp_spatial, sigma2, step, alpha, model_mul):
        a, m = alpha_svi_reference(ck._np(kappa), ck._np(Ks), ck._np(sd), Sp_spatial, sigma2, step, ck._np(alpha).copy())
        alpha.copy_(torch.from_numpy(a))
        model_mul.copy_(torch.from_numpy(m))

    def align_moments(self, A, V4, K, Ks, K2, sd, PXB, B, KB, out, origin=None, extra=None):
        o = np.zeros(3) if origin is None else np.asarray(origin)
        val, _ = lc.moments_reference(ck._np(A), ck._np(V4)[:, :3], ck._np(K), ck._np(Ks), ck._np(K2), ck._np(sd), ck._np(PXB), ck._np(B), ck._np(KB), o)
        blk = np.zeros(64)
        blk[:50] = val
        if extra is not None:
            blk[50] = float(extra[0])
        out.copy_(torch.from_numpy(blk))

    def align_transform(self, A, V4, PXB, K_NA, R, t, origin=None, RnA=None, XAHat=None, xa4=None, PXB_term=None, Y4=None, Pw=None):
        n = len(A)
        o = np.zeros(3) if origin is None else np.asarray(origin)
        V = np.zeros((n, 3)) if V4 is None else ck._np(V4)[:, :3]
        P = np.zeros((n, 3)) if PXB is None else ck._np(PXB)
        Kv = np.ones(n) if K_NA is None else ck._np(K_NA)
        r = lc.transform_reference(ck._np(A), V, P, Kv, R, t, o, np.float64)
        for buf, v in zip((RnA, XAHat, xa4, PXB_term, Y4, Pw), r):
            if buf is not None:
                buf.copy_(torch.from_numpy(np.ascontiguousarray(v)))

    def align_transform_svi(self, RnA, PXB, K_NA, step, PXB_term, Y4, Pw, origin=None):
        o = np.zeros(3) if origin is None else np.asarray(origin)
        r = transform_svi_reference(ck._np(RnA), ck._np(PXB), ck._np(K_NA), o, step, ck._np(PXB_term).copy(), np.float64)
        for buf, v in zip((PXB_term, Y4, Pw), r):
            buf.copy_(torch.from_numpy(np.ascontiguousarray(v)))

    def align_gather(self, perm, start, bs, xb4, B, layers, xb4_out, B_out, Yp_out, b_out):
        nb = len(xb4)
        idx = perm.long()[(start + torch.arange(bs)) % nb]
        xb4_out.copy_(xb4[idx])
        B_out.copy_(B[idx])
        for L, yo, bo in zip(layers, Yp_out, b_out):
            yo.copy_(Layer(*L).Yp[idx])
            bo.copy_(Layer(*L).b[idx])


def cpu_loop_kernels(monkeypatch, D):
    """Route spateo_amd.align through CpuLoopKernels (spatial dimension D) for the rest of the test."""
    from spateo_amd import _runtime as rt
    from spateo_amd import align

    def make(device, dtype):
        k = CpuLoopKernels(device, dtype)
        k.D = D
        return k

    def gamma_matrix(k, ctrl, center, beta):
        c = torch.from_numpy(np.ascontiguousarray(ctrl - center))
        return k.con_k(c, c, beta)

    monkeypatch.setattr(rt, "_make_kernels", make)
    monkeypatch.setattr(align, "_consistent_K", gamma_matrix)
