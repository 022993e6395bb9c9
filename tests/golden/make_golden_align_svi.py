#!/usr/bin/env python
"""Golden vectors that pin the SVI MODE of the iteration loop of Spateo's pairwise alignment to real reference code.

    spateo/alignment/methods/morpho_class.py:280-304     the loop of Morpho_pairwise.run and what follows it
    :749-760 the SVI state   :894-896 _update_batch   and the SVI branches of _update_assignment_P (:1149-1181), _update_gamma
    (:1214-1218), _update_alpha (:1238-1247), _update_nonrigid (:1269-1274), _update_rigid (:1312-1400), _get_optimal_R

This script EXECUTES those methods (unbound, on a ``SimpleNamespace`` self, NumPy backend, ``SVI_mode=True``), the way
``make_golden_align_loop.py`` does for the dense loop, for ``ITERS`` iterations with ``batch_size = 150`` (no multiple of 64,
no divisor of NB: the roll wraps) from an explicit ``batch_perm``, so ``step_size`` runs from 1 down to 1/3.  The inputs are
cases 1 - 3 of ``ref_align_loop.npz``: rebuilt here from the same seed, asserted equal to what that file holds and NOT stored
again.  Case ``3n`` is case 3 with ``nonrigid_start_iter = 11``: its first non-rigid update comes at iteration 12 with
``step_size < 1`` and is blended against the zeros the running ``SigmaInv`` / ``PXB_term`` start from.

Stored per case in ``tests/golden/ref_align_svi.npz``: ``batch_perm`` and every iteration's ``batch_idx``; per iteration
``sigma2``, ``gamma``, ``R``, ``t``, ``Sp`` (the blended one); at ``ARR_ITERS`` the cell-sized ``alpha``, ``XAHat``, ``VnA``,
``K_NA``, ``Coff``; ``optimal_R`` / ``optimal_t`` as ``_get_optimal_R`` gives them on the last batch, and ``optimal_R_map`` /
``optimal_t_map`` / ``Sp_map`` after the full non-SVI assignment of ``return_mapping=True`` (:300-302).  And the three twins
of the dense maker, relative to each quantity's maximum: ``chunk`` (``use_chunk=True``, ``split_size=128``), ``f32`` (the
float32 backend) and ``g`` (a float64 run with ``coordsB`` perturbed at 1e-10 relative, as a running maximum, divided by
1e-10).

The maker asserts: every value finite, the non-rigid update in at least 8 iterations, max g <= 100, the final R within 0.05
(Frobenius) of the rotation put in, the file below 1 MiB.

    python tests/golden/make_golden_align_svi.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_align_loop as mgl  # noqa: E402
import make_golden_assign as mga  # noqa: E402
import make_golden_em as mge  # noqa: E402

ITERS = 30
ARR_ITERS = (0, 9, 19, 29)
BATCH = 150
SCALARS, ARRAYS = mgl.SCALARS, mgl.ARRAYS
FINALS = ("optimal_R", "optimal_t", "optimal_R_map", "optimal_t_map", "Sp_map")
PERTURB = mgl.PERTURB


def run_loop(mc, backend, utils, case, batch_perm, dtype=np.float64, use_chunk=False, coordsB=None, kernel=None):
    """The real methods for ITERS iterations from the initial state of :700-760."""
    c = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    nx = backend.NumpyBackend()
    type_as = np.zeros(1, dtype=dtype)
    XA, XB = case["coordsA"], case["coordsB"] if coordsB is None else coordsB
    NA, D = XA.shape
    s = types.SimpleNamespace(
        nx=nx, type_as=type_as, Dim=dtype(D), D=D, NA=NA, NB=len(XB), coordsA=c(XA), coordsB=c(XB),
        exp_layers_A=[c(a) for a in case["exp_layers_A"]], exp_layers_B=[c(a) for a in case["exp_layers_B"]],
        dissimilarity=case["dissimilarity"], probability_type=case["probability_type"],
        probability_parameters=[None if p is None else dtype(p) for p in case["probability_parameters"]],
        sparse_calculation_mode=False, sparse_top_k=-1, use_chunk=use_chunk, split_size=128, SVI_mode=True,
        pre_compute_dist=False, label_transfer=None, batch_idx=None, guidance=False, guidance_effect=False, X_AI=None,
        graph=None, kernel_type="euc", kernel_bandwidth=case["beta"], lambdaVF=dtype(case["lambdaVF"]),
        nn_init="inlier_A" in case, nn_init_weight=dtype(case["nn_init_weight"]), update_R=True,
        sigma2=dtype(case["sigma2"]), kappa=c(np.full(NA, case["kappa"])),
    )
    if s.nn_init:
        s.inlier_A, s.inlier_B, s.inlier_P = c(case["inlier_A"]), c(case["inlier_B"]), c(case["inlier_P"])
    # ---- _initialize_variational_variables (:700-747), without its sigma2 guess ----
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
    if kernel is None:
        np.random.seed(17)  # _construct_kernel draws the inducing variables from NumPy's global RNG (as the dense maker)
        mc.Morpho_pairwise._construct_kernel(s, case["n_ctrl"], None)
        kernel = (s.inducing_variables, s.GammaSparse, s.U)
    s.inducing_variables, s.GammaSparse, s.U = kernel[0], c(kernel[1]), c(kernel[2])
    s.K = len(s.inducing_variables)
    s.Coff = np.zeros((s.K, D), dtype=dtype)
    # ---- the SVI state (:749-760) with an explicit batch_perm ----
    s.SVI_deacy = dtype(10.0)
    s.batch_size = min(BATCH, s.NB)
    s.batch_perm = np.array(batch_perm)
    s.Sp, s.Sp_spatial, s.Sp_sigma2 = 0, 0, 0
    s.SigmaInv = np.zeros((s.K, s.K), dtype=dtype)
    s.PXB_term = np.zeros((NA, D), dtype=dtype)
    M = mc.Morpho_pairwise
    hist = {q: [] for q in SCALARS + ARRAYS + ("batch_idx", "step_size")}
    nonrigid_runs = 0
    for it in range(ITERS):
        M._update_batch(s, iter=it)
        M._update_assignment_P(s)
        M._update_gamma(s)
        M._update_alpha(s)
        if it > case["nonrigid_start_iter"] or s.nonrigid_flag:
            s.nonrigid_flag = True
            M._update_nonrigid(s)
            nonrigid_runs += 1
        M._update_rigid(s)
        s.XAHat = s.VnA + s.RnA
        M._update_sigma2(s, iter=it)
        for q in SCALARS:
            v = np.array(getattr(s, q), dtype=np.float64)
            hist[q].append(v.reshape(-1) if q == "t" else v)   # (the reference's t is 1 x D)
        hist["batch_idx"].append(np.array(s.batch_idx))
        hist["step_size"].append(float(s.step_size))
        if it in ARR_ITERS:
            for q in ARRAYS:
                hist[q].append(np.array(getattr(s, q), dtype=np.float64))
    out = {q: np.array(v) for q, v in hist.items()}
    M._get_optimal_R(s)                                        # return_mapping=False: the last batch (:1451-1461)
    out["optimal_R"] = np.array(s.optimal_R, dtype=np.float64)
    out["optimal_t"] = np.array(s.optimal_t, dtype=np.float64).reshape(-1)
    s.SVI_mode = False                                         # return_mapping=True (:300-304)
    M._update_assignment_P(s)
    M._get_optimal_R(s)
    out["optimal_R_map"] = np.array(s.optimal_R, dtype=np.float64)
    out["optimal_t_map"] = np.array(s.optimal_t, dtype=np.float64).reshape(-1)
    out["Sp_map"] = np.array(s.Sp, dtype=np.float64)
    assert len(s.K_NB) == s.NB
    return out, kernel, nonrigid_runs


def twin_deviation(ref, other):
    dev = {q: mgl.rel(other[q], ref[q]) for q in SCALARS + ARRAYS}
    for q in FINALS:
        dev[q] = mgl.rel(other[q][None], ref[q][None])
    return dev


def main():
    mc, backend, utils = mge.load_morpho_class()
    dense = np.load(os.path.join(HERE, "ref_align_loop.npz"))
    rng = np.random.default_rng(20261018)   # the dense maker's seed and its order of cases
    kl = ("kl", "gauss", 0.1, mga.counts_layer, 40)
    cases = {
        "1": mgl.make_case(rng, 607, 451, 3, [kl], 0.45),
        "2": mgl.make_case(rng, 593, 447, 3, [("kl", "gauss", 0.1, mga.counts_layer, 31), ("cos", "cos", None, mga.pca_layer, 24)],
                           0.5, far_fraction=0.07),
        "3": mgl.make_case(rng, 611, 443, 2, [("euc", "gauss", 20.0, mga.pca_layer, 30)], 0.4, inliers=60,
                           partial_robust_level=3.0, n_ctrl=16, beta=1.0),
    }
    for tag, case in cases.items():
        XA, XB = case["coordsA"], case["coordsB"]
        case["samples_s"] = float(max(np.prod(XA.max(0) - XA.min(0)), np.prod(XB.max(0) - XB.min(0))))
        # the inputs are the dense fixture's: not stored again
        assert np.array_equal(dense[f"{tag}_coordsA"], XA) and np.array_equal(dense[f"{tag}_coordsB"], XB), tag
        assert float(dense[f"{tag}_samples_s"]) == case["samples_s"] and float(dense[f"{tag}_sigma2_init"]) == case["sigma2"]
        for l, (a, b) in enumerate(zip(case["exp_layers_A"], case["exp_layers_B"])):
            assert np.array_equal(dense[f"{tag}_layerA{l}"], a) and np.array_equal(dense[f"{tag}_layerB{l}"], b), (tag, l)
        for q in ("inlier_A", "inlier_B", "inlier_P"):
            assert (q in case) == (f"{tag}_{q}" in dense.files) and (q not in case or np.array_equal(dense[f"{tag}_{q}"], case[q]))
    cases["3n"] = dict(cases["3"], nonrigid_start_iter=11)
    out = {"cases": np.array(list(cases)), "iters": np.int64(ITERS), "arr_iters": np.array(ARR_ITERS), "batch_size": np.int64(BATCH),
           "scalars": np.array(SCALARS), "arrays": np.array(ARRAYS), "finals": np.array(FINALS)}
    for tag, case in cases.items():
        src = tag.rstrip("n")
        perm = np.random.default_rng(100 + int(src)).permutation(len(case["coordsB"]))
        ref, kernel, runs = run_loop(mc, backend, utils, case, perm)
        assert np.array_equal(kernel[0], dense[f"{src}_inducing_variables"]), tag
        chunk, _, _ = run_loop(mc, backend, utils, case, perm, use_chunk=True, kernel=kernel)
        f32, _, _ = run_loop(mc, backend, utils, case, perm, dtype=np.float32, kernel=kernel)
        prng = np.random.default_rng(int(src))
        XBp = case["coordsB"] * (1.0 + PERTURB * prng.standard_normal(case["coordsB"].shape))
        pert, _, _ = run_loop(mc, backend, utils, case, perm, coordsB=XBp, kernel=kernel)
        g = {q: np.maximum.accumulate(v / PERTURB) for q, v in twin_deviation(ref, pert).items()}
        fl_chunk, fl_f32 = twin_deviation(ref, chunk), twin_deviation(ref, f32)
        # ---- the conditions that keep the comparison meaningful ----
        assert all(np.isfinite(v).all() for v in ref.values()), tag
        gmax = max(float(v.max()) for v in g.values())
        assert gmax <= 100.0, (tag, {q: float(v.max()) for q, v in g.items()})
        assert runs >= 8, (tag, runs)
        assert np.linalg.norm(ref["R"][-1] - case["R0"]) <= 0.05, (tag, ref["R"][-1], case["R0"])
        assert np.array_equal(ref["step_size"], np.minimum(1.0, 10.0 / (np.arange(ITERS) + 1.0)))
        # ---- store ----
        out[f"{tag}_inputs_of"] = np.array(src)
        out[f"{tag}_nonrigid_start_iter"] = np.int64(case["nonrigid_start_iter"])
        out[f"{tag}_batch_perm"] = perm.astype(np.int16)
        out[f"{tag}_batch_idx"] = ref["batch_idx"].astype(np.int16)
        out[f"{tag}_step_size"] = ref["step_size"]
        out[f"{tag}_nonrigid_runs"] = np.int64(runs)
        for q in SCALARS + ARRAYS + FINALS:
            out[f"{tag}_{q}"] = ref[q]
            out[f"{tag}_g_{q}"], out[f"{tag}_chunk_{q}"], out[f"{tag}_f32_{q}"] = g[q], fl_chunk[q], fl_f32[q]
        print(f"case {tag}: sigma2 {ref['sigma2'][0]:.4g} -> {ref['sigma2'][-1]:.4g}, |R - R0| "
              f"{np.linalg.norm(ref['R'][-1] - case['R0']):.3g}, non-rigid in {runs}, max g {gmax:.3g}\n"
              "    chunk floor " + ", ".join(f"{q} {fl_chunk[q].max():.1e}" for q in SCALARS + ARRAYS + FINALS) + "\n"
              "    f32 floor   " + ", ".join(f"{q} {fl_f32[q].max():.1e}" for q in SCALARS + ARRAYS + FINALS) + "\n"
              "    g           " + ", ".join(f"{q} {g[q].max():.2g}" for q in SCALARS + ARRAYS + FINALS))
    path = os.path.join(HERE, "ref_align_svi.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
