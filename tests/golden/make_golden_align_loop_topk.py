#!/usr/bin/env python
"""Golden vectors that pin the ITERATION LOOP of Spateo's pairwise alignment in ``sparse_calculation_mode`` to real
reference code: the four cases of ``make_golden_align_loop.py`` (same generator, same seed - the inputs are those of
``tests/golden/ref_align_loop.npz`` and are not stored again; the maker asserts that they are equal) run with
``sparse_calculation_mode=True, sparse_top_k=16``:

    spateo/alignment/methods/morpho_class.py:280-294     the loop of Morpho_pairwise.run
    :1071-1200 _update_assignment_P (sparse branch :1187-1198)   utils.py:1085-1094, 1369-1404  the top-k sparsification

Stored in ``tests/golden/ref_align_loop_topk.npz`` per case: what ``ref_align_loop.npz`` stores of the outputs (per iteration
``sigma2``, ``gamma``, ``R``, ``t``, ``Sp``; at ``ARR_ITERS`` ``alpha``, ``XAHat``, ``VnA``, ``K_NA``, ``Coff``; the final ``optimal_R``,
``optimal_t``), the same three twins of the reference itself (``chunk``, ``f32``, and ``g``, the amplification of a 1e-10
perturbation of ``coordsB``), the last assignment's sparse ``P`` (``row``, ``data``; ``col = repeat(arange(NB), 16)``) and

* ``gap``: the smallest relative gap (v_k - v_{k+1}) / v_k between the 16th and the 17th largest value of a column of the
  dense ``P``, over the columns whose 17th value is positive and over all iterations;
* ``near``: the largest share, over the iterations, of such columns whose gap is at most 1e-2.

The maker asserts gap >= 1e-7, the chunk floors <= 1e-9 and the conditions of ``make_golden_align_loop.py``.

    python tests/golden/make_golden_align_loop_topk.py
"""
from __future__ import annotations

import copy
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_align_loop as mgl  # noqa: E402
import make_golden_assign as mga  # noqa: E402
import make_golden_assign_topk as mgt  # noqa: E402
import make_golden_em as mge  # noqa: E402

TOP_K = 16
ITERS, ARR_ITERS, SCALARS, ARRAYS, FINALS, PERTURB = mgl.ITERS, mgl.ARR_ITERS, mgl.SCALARS, mgl.ARRAYS, mgl.FINALS, mgl.PERTURB


def run_loop(mc, backend, utils, case, dtype=np.float64, use_chunk=False, coordsB=None, kernel=None, gaps=False):
    """make_golden_align_loop.run_loop with the sparse mode switched on.  gaps=True: every iteration's assignment is also
    run on the dense path (on a copy of the state) for the gaps of its columns."""
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
        sparse_calculation_mode=True, sparse_top_k=TOP_K, use_chunk=use_chunk, split_size=128, SVI_mode=False,
        pre_compute_dist=False, label_transfer=None, batch_idx=None, guidance=False, guidance_effect=False, X_AI=None,
        graph=None, kernel_type="euc", kernel_bandwidth=case["beta"], lambdaVF=dtype(case["lambdaVF"]),
        nn_init="inlier_A" in case, nn_init_weight=dtype(case["nn_init_weight"]), update_R=True,
        sigma2=dtype(case["sigma2"]), kappa=c(np.full(NA, case["kappa"])),
    )
    if s.nn_init:
        s.inlier_A, s.inlier_B, s.inlier_P = c(case["inlier_A"]), c(case["inlier_B"]), c(case["inlier_P"])
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
    nonrigid_runs, far_zero, gap, near = 0, True, 1.0, 0.0
    for it in range(ITERS):
        s.XAHat, s.coordsB = s.XAHat - c(origin), s.coordsB - c(origin)   # (case 4; a subtraction of zeros otherwise)
        if gaps:
            d = copy.copy(s)
            d.sparse_calculation_mode = False
            M._update_assignment_P(d)
            g_it, n_it = mgt.column_gaps(np.asarray(d.P, dtype=np.float64), min(TOP_K, NA))
            gap, near = min(gap, g_it), max(near, n_it)
        M._update_assignment_P(s)
        s.XAHat, s.coordsB = s.XAHat + c(origin), c(XB)
        far_zero = far_zero and not np.asarray(s.P.tocsc()[:, case["far"]].todense()).any()
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
    return out, s, kernel, dict(nonrigid_runs=nonrigid_runs, far_zero=far_zero, gap=gap, near=near)


def main():
    mc, backend, utils = mge.load_morpho_class()
    rng = np.random.default_rng(20261018)   # make_golden_align_loop.main's: the same four cases
    kl = ("kl", "gauss", 0.1, mga.counts_layer, 40)
    cases = {
        "1": mgl.make_case(rng, 607, 451, 3, [kl], 0.45),
        "2": mgl.make_case(rng, 593, 447, 3, [("kl", "gauss", 0.1, mga.counts_layer, 31), ("cos", "cos", None, mga.pca_layer, 24)],
                           0.5, far_fraction=0.07),
        "3": mgl.make_case(rng, 611, 443, 2, [("euc", "gauss", 20.0, mga.pca_layer, 30)], 0.4, inliers=60, partial_robust_level=3.0,
                           n_ctrl=16, beta=1.0),
    }
    for case in cases.values():
        XA, XB = case["coordsA"], case["coordsB"]
        case["samples_s"] = float(max(np.prod(XA.max(0) - XA.min(0)), np.prod(XB.max(0) - XB.min(0))))   # :738-741
    shift = np.full(3, 1e4)
    c4 = dict(cases["1"])
    c4.update(coordsA=cases["1"]["coordsA"] + shift, coordsB=cases["1"]["coordsB"] + shift, origin=shift,
              t0=cases["1"]["t0"] + shift - shift @ cases["1"]["R0"].T)
    cases["4"] = c4
    dense = np.load(os.path.join(HERE, "ref_align_loop.npz"))
    out = {"cases": np.array(sorted(cases)), "iters": np.int64(ITERS), "arr_iters": np.array(ARR_ITERS), "top_k": np.int64(TOP_K),
           "scalars": np.array(SCALARS), "arrays": np.array(ARRAYS), "finals": np.array(FINALS)}
    for tag, case in cases.items():
        ref, s, kernel, info = run_loop(mc, backend, utils, case, gaps=True)
        chunk, _, _, _ = run_loop(mc, backend, utils, case, use_chunk=True, kernel=kernel)
        f32, _, _, _ = run_loop(mc, backend, utils, case, dtype=np.float32, kernel=kernel)
        prng = np.random.default_rng(int(tag))
        XBp = case["origin"] + (case["coordsB"] - case["origin"]) * (1.0 + PERTURB * prng.standard_normal(case["coordsB"].shape))
        pert, _, _, _ = run_loop(mc, backend, utils, case, coordsB=XBp, kernel=kernel)
        g = {q: np.maximum.accumulate(v / PERTURB) for q, v in mgl.twin_deviation(ref, pert).items()}
        fl_chunk, fl_f32 = mgl.twin_deviation(ref, chunk), mgl.twin_deviation(ref, f32)
        # ---- the inputs are ref_align_loop.npz's ----
        for k in ("coordsA", "coordsB", "samples_s", "origin"):
            assert np.array_equal(dense[f"{tag}_{k}"], np.asarray(case[k])), (tag, k)
        assert np.array_equal(dense[f"{tag}_inducing_variables"], np.asarray(kernel[0])), tag
        src = "1" if tag == "4" else tag
        for l, (a, b) in enumerate(zip(case["exp_layers_A"], case["exp_layers_B"])):
            assert np.array_equal(dense[f"{src}_layerA{l}"], a) and np.array_equal(dense[f"{src}_layerB{l}"], b), (tag, l)
        # ---- the conditions that keep the comparison meaningful ----
        assert all(np.isfinite(v).all() for v in ref.values()), tag
        gmax = max(float(v.max()) for v in g.values())
        assert gmax <= 100.0, (tag, {q: float(v.max()) for q, v in g.items()})
        assert info["nonrigid_runs"] >= 8 and info["far_zero"], (tag, info)
        assert np.linalg.norm(ref["R"][-1] - case["R0"]) <= 0.05, (tag, ref["R"][-1], case["R0"])
        assert info["gap"] >= mgt.MIN_GAP, (tag, info)
        cmax = max(float(v.max()) for v in fl_chunk.values())
        assert cmax <= 1e-9, (tag, cmax)
        P = s.P.tocoo()
        ke = min(TOP_K, len(case["coordsA"]))
        assert np.array_equal(P.col, np.repeat(np.arange(len(case["coordsB"])), ke))
        for q in SCALARS + ARRAYS + FINALS:
            out[f"{tag}_{q}"] = ref[q]
            out[f"{tag}_g_{q}"], out[f"{tag}_chunk_{q}"], out[f"{tag}_f32_{q}"] = g[q], fl_chunk[q], fl_f32[q]
        out[f"{tag}_sigma2_variance"] = ref["sigma2_variance"]
        out[f"{tag}_P_row"], out[f"{tag}_P_data"] = np.asarray(P.row, dtype=np.int32), np.asarray(P.data, dtype=np.float64)
        out[f"{tag}_gap"], out[f"{tag}_near"] = np.float64(info["gap"]), np.float64(info["near"])
        print(f"case {tag}: sigma2 {ref['sigma2'][0]:.4g} -> {ref['sigma2'][-1]:.4g}, Sp {ref['Sp'][-1]:.5g} (dense "
              f"{dense[f'{tag}_Sp'][-1]:.5g}), gap {info['gap']:.2e}, near {info['near']:.3f}, max g {gmax:.3g}, chunk floor {cmax:.1e}\n"
              "    f32 floor   " + ", ".join(f"{q} {fl_f32[q].max():.1e}" for q in SCALARS + ARRAYS + FINALS))
    path = os.path.join(HERE, "ref_align_loop_topk.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
