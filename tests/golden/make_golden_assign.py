#!/usr/bin/env python
"""Golden vectors that pin the ASSIGNMENT STEP of Spateo's alignment to real reference code.

    spateo/alignment/methods/morpho_class.py:1071-1200  Morpho_pairwise._update_assignment_P
    spateo/alignment/methods/utils.py:647-788,866-985   calc_distance / calc_probability and their back ends
    spateo/alignment/methods/utils.py:993-1096          get_P_core

This script EXECUTES ``_update_assignment_P`` (unbound, on a ``SimpleNamespace`` self, NumPy backend, dense path, no SVI)
from the real file on synthetic alignment states and stores inputs and outputs in ``tests/golden/ref_assign.npz``;
``spateo_amd.align.update_assignment`` and the NumPy restatement of ``tests/_assign_case.py`` are checked against them.

Per case and per quantity it also stores two floors measured on the reference itself, relative to the quantity's
maximum: ``chunk`` - the ``use_chunk=True`` run (B in column chunks of 128) against the dense run, what the reference's
own reorderings cost - and ``f32`` - the float32 NumPy-backend run against the float64 one, what the data type costs.

Case ``e`` also runs the real ``_construct_kernel`` + ``_update_nonrigid`` (:825-875, :1254-1298) on the assignment it
has just computed and stores ``Coff`` / ``VnA`` / ``SigmaDiag``: the composition ``update_assignment`` ->
``update_nonrigid``.  Case ``p`` is small and stores the dense ``P`` (``return_P=True``).

The layers are kept on coarse grids (counts; multiples of 1/32) so that the file stays small once compressed.

    python tests/golden/make_golden_assign.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_em as mge  # noqa: E402

QUANTITIES = ("K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2", "Sp", "Sp_spatial", "Sp_sigma2", "sigma2_related", "PXB")
FAR_FRACTION = 0.07  # of the B cells: moved so far away that every term of their column underflows


def counts_layer(rng, n, g, labels, k=5):
    """Count-like expression (non-negative integers) with `k` cell types: what the kl / sym_kl metrics are used on."""
    prof = rng.gamma(0.6, 4.0, (k, g))
    return rng.poisson(prof[labels]).astype(np.float64)


def pca_layer(rng, n, g, labels, k=5):
    """PCA-like representation on a 1/32 grid."""
    cent = rng.standard_normal((k, g)) * 1.5
    return np.round((cent[labels] + 0.7 * rng.standard_normal((n, g))) * 32) / 32


def make_state(backend, rng, NA, NB, D, layers, sigma2, gamma, sigma2_variance, dtype=np.float64):
    """layers: list of (metric, probability type, probability parameter, maker, G)."""
    XA = rng.standard_normal((NA, D))
    src = rng.choice(NA, NB)
    XB = XA[src] + 0.15 * rng.standard_normal((NB, D))
    far = rng.choice(NB, max(1, int(np.ceil(FAR_FRACTION * NB))), replace=False)
    # every far cell sits > reach away from every A cell: exp(-d sigma2_variance / (2 sigma2)) and exp(-d / (2 sigma2))
    # underflow to exactly 0 in float64 (and in float32) for the whole column
    reach = np.sqrt(2 * sigma2 * 800.0 / min(1.0, sigma2_variance)) + 2 * np.abs(XA).max() * np.sqrt(D)
    XB[far] = XA[src[far]] + reach * (1.0 + rng.random((len(far), 1))) * np.eye(D)[0]
    labA = rng.integers(0, 5, NA)
    labB = labA[src]
    LA, LB = [], []
    for (_, _, _, maker, g) in layers:
        st = rng.bit_generator.state
        LA.append(maker(rng, NA, g, labA))
        rng.bit_generator.state = st  # the same cell-type profiles / centres for both slices
        LB.append(maker(rng, NB, g, labB))
    alpha = rng.uniform(0.5, 1.0, NA)
    SigmaDiag = sigma2 * rng.uniform(0.0, 0.3, NA)
    return dict(XAHat=XA, coordsB=XB, exp_layers_A=LA, exp_layers_B=LB, alpha=alpha, SigmaDiag=SigmaDiag,
                sigma2=float(sigma2), gamma=float(gamma), samples_s=float(np.prod(XA.max(0) - XA.min(0))),
                sigma2_variance=float(sigma2_variance), far=np.sort(far),
                dissimilarity=[l[0] for l in layers], probability_type=[l[1] for l in layers],
                probability_parameters=[l[2] for l in layers])


def run_reference(mc, backend, st, dtype=np.float64, use_chunk=False):
    """The real _update_assignment_P on the state `st`, in `dtype` arithmetic."""
    c = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    NA, D = st["XAHat"].shape
    s = types.SimpleNamespace(
        nx=backend.NumpyBackend(), type_as=np.zeros(1, dtype=dtype), Dim=dtype(D), NA=NA, NB=len(st["coordsB"]),
        XAHat=c(st["XAHat"]), coordsB=c(st["coordsB"]), exp_layers_A=[c(a) for a in st["exp_layers_A"]],
        exp_layers_B=[c(a) for a in st["exp_layers_B"]], alpha=c(st["alpha"]), SigmaDiag=c(st["SigmaDiag"]),
        sigma2=dtype(st["sigma2"]), gamma=dtype(st["gamma"]), samples_s=dtype(st["samples_s"]),
        sigma2_variance=dtype(st["sigma2_variance"]), dissimilarity=st["dissimilarity"],
        probability_type=st["probability_type"],
        probability_parameters=[None if p is None else dtype(p) for p in st["probability_parameters"]],
        sparse_calculation_mode=False, sparse_top_k=-1, use_chunk=use_chunk, split_size=128, SVI_mode=False,
        pre_compute_dist=False, label_transfer=None, batch_idx=None,
    )
    mc.Morpho_pairwise._update_assignment_P(s)
    out = {q: np.asarray(getattr(s, q), dtype=np.float64) for q in QUANTITIES if q != "PXB"}
    out["PXB"] = np.asarray(s.P @ s.coordsB, dtype=np.float64)
    return out, s


def floors(ref, other):
    return np.array([np.abs(other[q] - ref[q]).max() / np.abs(ref[q]).max() for q in QUANTITIES])


def main():
    mc, backend, _ = mge.load_morpho_class()
    rng = np.random.default_rng(20261017)
    kl = lambda g, p=0.05: ("kl", "gauss", p, counts_layer, g)  # noqa: E731
    cases = {
        "a": dict(NA=613, NB=457, D=3, sigma2=0.08, gamma=0.6, sigma2_variance=1.0, layers=[kl(37)]),
        "b": dict(NA=587, NB=441, D=3, sigma2=0.05, gamma=0.5, sigma2_variance=1.0,
                  layers=[kl(29), ("cos", "cos", None, pca_layer, 24)]),
        "c": dict(NA=601, NB=463, D=2, sigma2=0.1, gamma=0.7, sigma2_variance=1.0,
                  layers=[("euc", "gauss", 20.0, pca_layer, 30)]),
        "d": dict(NA=595, NB=449, D=3, sigma2=0.06, gamma=0.5, sigma2_variance=1.0,
                  layers=[("sym_kl", "gauss", 0.08, counts_layer, 26)]),
        "e": dict(NA=607, NB=451, D=3, sigma2=0.5, gamma=0.5, sigma2_variance=2.5, layers=[kl(40, 0.1)]),
        "p": dict(NA=149, NB=117, D=3, sigma2=0.07, gamma=0.5, sigma2_variance=0.5,
                  layers=[("square_euc", "gauss", 3.0, pca_layer, 25), ("cos", "cos", None, pca_layer, 24)]),
    }
    out = {"cases": np.array(sorted(cases)), "quantities": np.array(QUANTITIES)}
    for tag, kw in cases.items():
        st = make_state(backend, rng, **kw)
        ref, s = run_reference(mc, backend, st)
        chunk, _ = run_reference(mc, backend, st, use_chunk=True)
        f32, _ = run_reference(mc, backend, st, dtype=np.float32)
        assert all(np.isfinite(v).all() for v in ref.values())
        assert np.all(s.P[:, st["far"]] == 0.0) and len(st["far"]) >= 0.05 * kw["NB"]
        for k in ("XAHat", "coordsB", "alpha", "SigmaDiag", "sigma2", "gamma", "samples_s", "sigma2_variance", "far"):
            out[f"{tag}_{k}"] = np.asarray(st[k])
        out[f"{tag}_dissimilarity"] = np.array(st["dissimilarity"])
        out[f"{tag}_probability_type"] = np.array(st["probability_type"])
        out[f"{tag}_probability_parameters"] = np.array([np.nan if p is None else p for p in st["probability_parameters"]])
        for l, (a, b) in enumerate(zip(st["exp_layers_A"], st["exp_layers_B"])):
            out[f"{tag}_layerA{l}"], out[f"{tag}_layerB{l}"] = a, b
        for q in QUANTITIES:
            out[f"{tag}_{q}"] = ref[q]
        out[f"{tag}_floor_chunk"], out[f"{tag}_floor_f32"] = floors(ref, chunk), floors(ref, f32)
        print(f"case {tag}: NA {kw['NA']} NB {kw['NB']} D {kw['D']} {st['dissimilarity']}: Sp {ref['Sp']:.4g} "
              f"Sp_spatial {ref['Sp_spatial']:.4g} sigma2_related {ref['sigma2_related']:.4g}, {len(st['far'])} far columns\n"
              f"    chunk floor max {out[f'{tag}_floor_chunk'].max():.2e}; f32 floor "
              + ", ".join(f"{q} {v:.1e}" for q, v in zip(QUANTITIES, out[f"{tag}_floor_f32"])))
        if tag == "p":
            out["p_P"] = np.asarray(s.P)
        if tag == "e":  # the composition: the real non-rigid update on this assignment (well conditioned, as ref_em's case a)
            s.coordsA = st["XAHat"]
            s.RnA = st["XAHat"] + 0.02 * rng.standard_normal(st["XAHat"].shape)
            s.kernel_type, s.kernel_bandwidth, s.lambdaVF = "euc", 0.5, 100.0
            s.guidance_effect, s.guidance, s.X_AI, s.graph = False, False, None, None
            np.random.seed(17)  # _construct_kernel draws the inducing variables from NumPy's global RNG
            mc.Morpho_pairwise._construct_kernel(s, 40, None)
            mc.Morpho_pairwise._update_nonrigid(s)
            for k in ("RnA", "inducing_variables", "Coff", "VnA", "SigmaDiag", "SigmaInv", "PXB_term"):
                out[f"e_nr_{k}"] = np.asarray(getattr(s, k))
            out["e_nr_beta"], out["e_nr_lambdaVF"] = np.float64(0.5), np.float64(100.0)
    path = os.path.join(HERE, "ref_assign.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
