#!/usr/bin/env python
"""Golden vectors that pin the ITERATION LOOP of Spateo's pairwise alignment to real reference code.

    spateo/alignment/methods/morpho_class.py:280-294     the loop of Morpho_pairwise.run
    :1071-1200 _update_assignment_P   :1202-1224 _update_gamma   :1226-1252 _update_alpha   :1254-1298 _update_nonrigid
    :1300-1408 _update_rigid          :1410-1435 _update_sigma2  :1437-1469 _get_optimal_R

This script EXECUTES those methods (unbound, on a ``SimpleNamespace`` self, NumPy backend, dense path, no SVI) from the
state ``_initialize_variational_variables`` sets (:700-747) for ``ITERS`` iterations and stores inputs and outputs in
``tests/golden/ref_align_loop.npz``; ``spateo_amd.align.morpho_iterate`` and the NumPy restatement of
``tests/_align_loop_case.py`` are checked against them.  Stored per case: the inputs; per iteration ``sigma2``, ``gamma``,
``R``, ``t``, ``Sp``; at the iterations ``ARR_ITERS`` (every iteration would put the file above the 1 MB a committed file may
have: the loop is a recurrence, so an error in an iteration that is not stored shows in the next one that is, and in the
scalars of every iteration) the cell-sized ``alpha``, ``XAHat``, ``VnA``, ``K_NA`` and ``Coff``; and the final ``optimal_R``,
``optimal_t``.

Three twins of the reference itself per case, relative to each quantity's maximum:

* ``chunk``: ``use_chunk=True`` with ``split_size=128`` - what the reference's own reorderings cost;
* ``f32``: the float32 NumPy backend - what the data type costs;
* a float64 run with ``coordsB`` perturbed at 1e-10 relative: ``g_k(q)`` = deviation of quantity q at iteration k divided by
  1e-10, as a running maximum over the iterations <= k - how much the loop amplifies an input error.

Cases (about 600 x 450 cells, A a rotated, shifted, smoothly bent copy of B):

1. 3-D, one ``kl`` layer of 40 count features, 40 inducing variables, ``nonrigid_start_iter = 2``;
2. 7 % far B cells (whole columns underflow, gamma leaves its clamp) and two layers (``kl`` + ``cos``);
3. 2-D with ``euc``, ``inliers`` given and ``partial_robust_level = 3``;
4. case 1 translated by 1e4 in every axis.  The reference forms every distance as |x|^2 + |y|^2 - 2 x.y, which at 1e4 keeps
   7 digits of a distance of order 1: its own assignment and kernel matrix would be noise at the 1e-7 level and no
   comparison at 1e-10 would mean anything.  So only the moments see the translation: ``_update_assignment_P`` is handed
   ``XAHat - origin`` and ``coordsB - origin`` (sigma2 and the exponents are those of case 1) and ``U`` / ``GammaSparse`` are
   built from the untranslated points, and so is ``_update_nonrigid``'s ``PXB_term = P coordsB - RnA K_NA`` (translation
   invariant; at 1e4 the reference's own chunk twin moved ``VnA`` by 1.4e-10); ``_update_rigid``, ``_update_sigma2`` and
   ``_get_optimal_R`` run on the translated coordinates.  ``morpho_iterate`` gets ``origin=``.

The maker asserts what keeps the comparison meaningful and fails instead of writing a weak file: max g_k <= 100 for every
compared quantity, 0.01 < gamma < 0.99 in at least half the iterations of case 2, the non-rigid update in at least 8 of the
12 iterations, the final R within 0.05 (Frobenius) of the rotation put in, every stored value finite.

The layers are kept on coarse grids (counts; multiples of 1/32) so that the file stays small once compressed.

    python tests/golden/make_golden_align_loop.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_assign as mga  # noqa: E402
import make_golden_em as mge  # noqa: E402

ITERS = 12
ARR_ITERS = (0, 3, 7, 11)
SCALARS = ("sigma2", "gamma", "R", "t", "Sp")
ARRAYS = ("alpha", "XAHat", "VnA", "K_NA", "Coff")
FINALS = ("optimal_R", "optimal_t")
PERTURB = 1e-10


def rotation(D, angle):
    c, s = np.cos(angle), np.sin(angle)
    R = np.eye(D)
    R[0, 0], R[0, 1], R[1, 0], R[1, 1] = c, -s, s, c
    if D == 3:  # tilt the axis a little, so that no coordinate is left alone
        c2, s2 = np.cos(0.4 * angle), np.sin(0.4 * angle)
        R = R @ np.array([[1, 0, 0], [0, c2, -s2], [0, s2, c2]])
    return R


def make_case(rng, NA, NB, D, layers, sigma2, far_fraction=0.0, inliers=0, **kw):
    """coordsB = a noisy subset of points Z; coordsA = the rigid pre-image of Z, smoothly bent: coordsA R0^T + t0 ~ Z."""
    Z = rng.standard_normal((NA, D))
    src = rng.choice(NA, NB)
    XB = Z[src] + 0.05 * rng.standard_normal((NB, D))
    R0, t0 = rotation(D, 0.35), 0.3 + 0.2 * rng.random(D)
    bend = 0.04 * np.sin(1.3 * Z[:, ::-1] + 0.5)
    XA = (Z + bend - t0) @ R0                       # (Z + bend - t0) R0: then XA R0^T + t0 = Z + bend
    far = np.zeros(0, dtype=np.int64)
    if far_fraction:
        far = np.sort(rng.choice(NB, int(np.ceil(far_fraction * NB)), replace=False))
        reach = np.sqrt(2 * sigma2 * 800.0) + 4 * np.abs(XA).max() * np.sqrt(D)
        XB[far] = Z[src[far]] + reach * (1.0 + rng.random((len(far), 1))) * np.eye(D)[0]
    labA = rng.integers(0, 5, NA)
    labB = labA[src]
    LA, LB = [], []
    for (_, _, _, maker, g) in layers:
        st = rng.bit_generator.state
        LA.append(maker(rng, NA, g, labA))
        rng.bit_generator.state = st  # the same cell-type profiles / centres for both slices
        LB.append(maker(rng, NB, g, labB))
    case = dict(coordsA=XA, coordsB=XB, exp_layers_A=LA, exp_layers_B=LB, sigma2=float(sigma2), R0=R0, t0=t0, far=far,
                dissimilarity=[l[0] for l in layers], probability_type=[l[1] for l in layers],
                probability_parameters=[l[2] for l in layers], origin=np.zeros(D), beta=0.5, lambdaVF=100.0, n_ctrl=40,
                nonrigid_start_iter=2, partial_robust_level=10.0, nn_init_weight=1.0, kappa=1.0, gamma_a=1.0, gamma_b=1.0)
    if inliers:
        idx = rng.choice(NA, inliers, replace=False)
        case["inlier_A"] = XA[idx]
        case["inlier_B"] = Z[idx] + 0.03 * rng.standard_normal((inliers, D))
        case["inlier_P"] = rng.uniform(0.5, 1.0, (inliers, 1))
    case.update(kw)
    return case


def run_loop(mc, backend, utils, case, dtype=np.float64, use_chunk=False, coordsB=None, kernel=None):
    """The real methods for ITERS iterations from the initial state of :700-747.  Returns (history, namespace)."""
    c = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    nx = backend.NumpyBackend()
    type_as = np.zeros(1, dtype=dtype)
    XA, XB = case["coordsA"], case["coordsB"] if coordsB is None else coordsB
    NA, D = XA.shape
    origin = case["origin"]
    s = types.SimpleNamespace(
        nx=nx, type_as=type_as, Dim=dtype(D), D=D, NA=NA, NB=len(XB), coordsA=c(XA), coordsB=c(XB),
        exp_layers_A=[c(a) for a in case["exp_layers_A"]], exp_layers_B=[c(a) for a in case["exp_layers_B"]],
        dissimilarity=case["dissimilarity"], probability_type=case["probability_type"],
        probability_parameters=[None if p is None else dtype(p) for p in case["probability_parameters"]],
        sparse_calculation_mode=False, sparse_top_k=-1, use_chunk=use_chunk, split_size=128, SVI_mode=False,
        pre_compute_dist=False, label_transfer=None, batch_idx=None, guidance=False, guidance_effect=False, X_AI=None,
        graph=None, kernel_type="euc", kernel_bandwidth=case["beta"], lambdaVF=dtype(case["lambdaVF"]),
        nn_init="inlier_A" in case, nn_init_weight=dtype(case["nn_init_weight"]), update_R=True,
        sigma2=dtype(case["sigma2"]), kappa=c(np.full(NA, case["kappa"])),
    )
    if s.nn_init:
        s.inlier_A, s.inlier_B, s.inlier_P = c(case["inlier_A"]), c(case["inlier_B"]), c(case["inlier_P"])
    # ---- _initialize_variational_variables (:700-747), without its sigma2 guess and its SVI part ----
    s.sigma2_variance = dtype(1)
    s.sigma2_variance_end = dtype(case["partial_robust_level"])
    s.sigma2_variance_decress = utils._get_anneling_factor(start=s.sigma2_variance, end=s.sigma2_variance_end, iter=100, nx=nx,
                                                           type_as=type_as)
    s.alpha = np.ones(NA, dtype=dtype)
    s.gamma, s.gamma_a, s.gamma_b = dtype(0.5), dtype(case["gamma_a"]), dtype(case["gamma_b"])
    s.VnA = np.zeros((NA, D), dtype=dtype)
    s.XAHat, s.RnA = s.coordsA.copy(), s.coordsA.copy()
    s.SigmaDiag = np.zeros(NA, dtype=dtype)
    s.R = np.identity(D, dtype=dtype)
    s.nonrigid_flag = False
    s.samples_s = dtype(case["samples_s"])
    s._gamma_001, s._gamma_099 = dtype(0.01), dtype(0.99)
    s.C = np.identity(D, dtype=dtype)
    # ---- _construct_kernel (:825-875) on the points the assignment sees (the untranslated ones) ----
    if kernel is None:
        s.coordsA = c(XA - origin)
        np.random.seed(17)  # _construct_kernel draws the inducing variables from NumPy's global RNG
        mc.Morpho_pairwise._construct_kernel(s, case["n_ctrl"], None)
        kernel = (s.inducing_variables + c(origin), s.GammaSparse, s.U)
        s.coordsA = c(XA)
    s.inducing_variables, s.GammaSparse, s.U = kernel[0], c(kernel[1]), c(kernel[2])
    s.K = len(s.inducing_variables)
    s.Coff = np.zeros((s.K, D), dtype=dtype)
    M = mc.Morpho_pairwise
    hist = {q: [] for q in SCALARS + ARRAYS}
    nonrigid_runs, far_zero = 0, True
    for it in range(ITERS):
        s.XAHat, s.coordsB = s.XAHat - c(origin), s.coordsB - c(origin)   # (case 4; a subtraction of zeros otherwise)
        M._update_assignment_P(s)
        s.XAHat, s.coordsB = s.XAHat + c(origin), c(XB)
        far_zero = far_zero and bool(np.all(s.P[:, case["far"]] == 0.0))
        M._update_gamma(s)
        M._update_alpha(s)
        if it > case["nonrigid_start_iter"] or s.nonrigid_flag:
            s.nonrigid_flag = True
            s.RnA, s.coordsB = s.RnA - c(origin), s.coordsB - c(origin)   # PXB_term = P coordsB - RnA K_NA is translation invariant
            M._update_nonrigid(s)
            s.RnA, s.coordsB = s.RnA + c(origin), c(XB)
            nonrigid_runs += 1
        M._update_rigid(s)
        s.XAHat = s.VnA + s.RnA
        M._update_sigma2(s, iter=it)
        for q in SCALARS:
            v = np.array(getattr(s, q), dtype=np.float64)
            hist[q].append(v.reshape(-1) if q == "t" else v)   # (the reference's t is 1 x D)
        if it in ARR_ITERS:
            for q in ARRAYS:
                hist[q].append(np.array(getattr(s, q), dtype=np.float64))
    M._get_optimal_R(s)
    out = {q: np.array(v) for q, v in hist.items()}
    out["optimal_R"] = np.array(s.optimal_R, dtype=np.float64)
    out["optimal_t"] = np.array(s.optimal_t, dtype=np.float64).reshape(-1)
    out["sigma2_variance"] = np.float64(s.sigma2_variance)
    return out, s, kernel, dict(nonrigid_runs=nonrigid_runs, far_zero=far_zero)


def rel(a, b):
    """max |a - b| / max |b| per iteration (leading axis); the absolute deviation where b is all zero."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = len(b)
    d = np.abs(a - b).reshape(n, -1).max(1)
    m = np.abs(b).reshape(n, -1).max(1)
    return np.where(m > 0, d / np.where(m > 0, m, 1.0), d)


def twin_deviation(ref, other):
    """{quantity: per stored iteration deviation}; the finals as one-element arrays."""
    dev = {q: rel(other[q], ref[q]) for q in SCALARS + ARRAYS}
    for q in FINALS:
        dev[q] = rel(other[q][None], ref[q][None])
    return dev


def main():
    mc, backend, utils = mge.load_morpho_class()
    rng = np.random.default_rng(20261018)
    kl = ("kl", "gauss", 0.1, mga.counts_layer, 40)
    cases = {
        "1": make_case(rng, 607, 451, 3, [kl], 0.45),
        "2": make_case(rng, 593, 447, 3, [("kl", "gauss", 0.1, mga.counts_layer, 31), ("cos", "cos", None, mga.pca_layer, 24)], 0.5,
                       far_fraction=0.07),
        "3": make_case(rng, 611, 443, 2, [("euc", "gauss", 20.0, mga.pca_layer, 30)], 0.4, inliers=60, partial_robust_level=3.0,
                       n_ctrl=16, beta=1.0),   # (40 points at beta = 0.5 in the plane: pinv's cut-off flips under 1e-10)
    }
    for case in cases.values():
        XA, XB = case["coordsA"], case["coordsB"]
        case["samples_s"] = float(max(np.prod(XA.max(0) - XA.min(0)), np.prod(XB.max(0) - XB.min(0))))   # :738-741
    shift = np.full(3, 1e4)
    c4 = dict(cases["1"])
    c4.update(coordsA=cases["1"]["coordsA"] + shift, coordsB=cases["1"]["coordsB"] + shift, origin=shift,
              t0=cases["1"]["t0"] + shift - shift @ cases["1"]["R0"].T)
    cases["4"] = c4
    out = {"cases": np.array(sorted(cases)), "iters": np.int64(ITERS), "arr_iters": np.array(ARR_ITERS),
           "scalars": np.array(SCALARS), "arrays": np.array(ARRAYS), "finals": np.array(FINALS)}
    for tag, case in cases.items():
        ref, s, kernel, info = run_loop(mc, backend, utils, case)
        chunk, _, _, _ = run_loop(mc, backend, utils, case, use_chunk=True, kernel=kernel)
        f32, _, _, _ = run_loop(mc, backend, utils, case, dtype=np.float32, kernel=kernel)
        prng = np.random.default_rng(int(tag))
        XBp = case["origin"] + (case["coordsB"] - case["origin"]) * (1.0 + PERTURB * prng.standard_normal(case["coordsB"].shape))
        pert, _, _, _ = run_loop(mc, backend, utils, case, coordsB=XBp, kernel=kernel)
        g = {q: np.maximum.accumulate(v / PERTURB) for q, v in twin_deviation(ref, pert).items()}
        # arrays are stored at ARR_ITERS only: their running maximum is over the stored iterations
        fl_chunk, fl_f32 = twin_deviation(ref, chunk), twin_deviation(ref, f32)
        # ---- the conditions that keep the comparison meaningful ----
        assert all(np.isfinite(v).all() for v in ref.values()), tag
        gmax = max(float(v.max()) for v in g.values())
        assert gmax <= 100.0, (tag, {q: float(v.max()) for q, v in g.items()})
        assert info["nonrigid_runs"] >= 8, (tag, info)
        assert info["far_zero"], tag
        assert np.linalg.norm(ref["R"][-1] - case["R0"]) <= 0.05, (tag, ref["R"][-1], case["R0"])
        inside = int(np.sum((ref["gamma"] > 0.01) & (ref["gamma"] < 0.99)))
        if tag == "2":
            assert inside >= ITERS // 2 and len(case["far"]) >= 0.05 * len(case["coordsB"]), (inside, ref["gamma"])
        # ---- store ----
        out[f"{tag}_sigma2_init"] = np.float64(case["sigma2"])
        for k in ("coordsA", "coordsB", "samples_s", "origin", "beta", "lambdaVF", "nonrigid_start_iter",
                  "partial_robust_level", "nn_init_weight", "kappa", "gamma_a", "gamma_b", "R0", "t0", "far"):
            out[f"{tag}_{k}"] = np.asarray(case[k])
        out[f"{tag}_inducing_variables"] = np.asarray(kernel[0])
        if tag == "4":  # the inputs of case 1, translated: only the translated coordinates are stored again
            out["4_layers_of"] = np.array("1")
        else:
            for l, (a, b) in enumerate(zip(case["exp_layers_A"], case["exp_layers_B"])):
                out[f"{tag}_layerA{l}"], out[f"{tag}_layerB{l}"] = a, b
        out[f"{tag}_dissimilarity"] = np.array(case["dissimilarity"])
        out[f"{tag}_probability_type"] = np.array(case["probability_type"])
        out[f"{tag}_probability_parameters"] = np.array([np.nan if p is None else p for p in case["probability_parameters"]])
        for k in ("inlier_A", "inlier_B", "inlier_P"):
            if k in case:
                out[f"{tag}_{k}"] = case[k]
        for q in SCALARS + ARRAYS + FINALS:
            out[f"{tag}_{q}"] = ref[q]
            out[f"{tag}_g_{q}"], out[f"{tag}_chunk_{q}"], out[f"{tag}_f32_{q}"] = g[q], fl_chunk[q], fl_f32[q]
        out[f"{tag}_sigma2_variance"] = ref["sigma2_variance"]
        out[f"{tag}_nonrigid_runs"] = np.int64(info["nonrigid_runs"])
        print(f"case {tag}: sigma2 {ref['sigma2'][0]:.4g} -> {ref['sigma2'][-1]:.4g}, gamma inside the clamp in {inside}/{ITERS}, "
              f"|R - R0| {np.linalg.norm(ref['R'][-1] - case['R0']):.3g}, non-rigid in {info['nonrigid_runs']}, max g {gmax:.3g}\n"
              "    chunk floor " + ", ".join(f"{q} {fl_chunk[q].max():.1e}" for q in SCALARS + ARRAYS + FINALS) + "\n"
              "    f32 floor   " + ", ".join(f"{q} {fl_f32[q].max():.1e}" for q in SCALARS + ARRAYS + FINALS) + "\n"
              "    g           " + ", ".join(f"{q} {g[q].max():.2g}" for q in SCALARS + ARRAYS + FINALS))
    path = os.path.join(HERE, "ref_align_loop.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
