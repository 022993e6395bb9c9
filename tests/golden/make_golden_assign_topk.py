#!/usr/bin/env python
"""Golden vectors that pin the ASSIGNMENT STEP in ``sparse_calculation_mode`` to real reference code.

    spateo/alignment/methods/morpho_class.py:1071-1200  Morpho_pairwise._update_assignment_P (sparse branch :1187-1198)
    spateo/alignment/methods/utils.py:993-1096          get_P_core, :1085-1094 its top-k sparsification
    spateo/alignment/methods/utils.py:1369-1404         _dense_to_sparse(axis=0, descending=True)

This script EXECUTES ``_update_assignment_P`` with ``sparse_calculation_mode=True`` (unbound, on a ``SimpleNamespace`` self,
NumPy backend, no SVI) on the synthetic states of ``make_golden_assign.py`` and stores inputs and outputs in
``tests/golden/ref_assign_topk.npz``: per case the inputs, per (case, k) the quantities of ``ref_assign.npz`` formed from
the sparse ``P``, the reference's ``scipy.sparse.coo_matrix`` (``row``, ``col``, ``data`` in its order) and

* ``floor_chunk`` / ``floor_f32``: the ``use_chunk=True`` run (column chunks of 128) and the float32 NumPy-backend run against
  the float64 dense-path run, per quantity, relative to the quantity's maximum;
* ``gap``: the smallest relative gap (v_k - v_{k+1}) / v_k between the k-th and the (k + 1)-th largest value of a column,
  over the columns whose (k + 1)-th value is positive (1.0 when no column has one) - how close the selection comes to a tie;
* ``near``: the share of such columns whose gap is at most 1e-2 (1000 x the float32 base bound): the columns a float32
  comparison of the selected SETS has to leave out.

The maker asserts gap >= 1e-7 (1000 x the float64 bound of tests/_assign_case.py) and near <= 5 % and fails instead of
writing a weak file.  ``spateo_amd.align.update_assignment(sparse_calculation_mode=True)`` and the masked restatement of
``tests/_assign_topk_case.py`` are checked against the file.

    python tests/golden/make_golden_assign_topk.py
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

QUANTITIES = mga.QUANTITIES
MIN_GAP, NEAR_GAP, MAX_NEAR = 1e-7, 1e-2, 0.05


def run_reference(mc, backend, st, k, dtype=np.float64, use_chunk=False):
    """The real _update_assignment_P in sparse_calculation_mode with sparse_top_k = k.  Returns (quantities, coo P)."""
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
        sparse_calculation_mode=True, sparse_top_k=int(k), use_chunk=use_chunk, split_size=128, SVI_mode=False,
        pre_compute_dist=False, label_transfer=None, batch_idx=None,
    )
    mc.Morpho_pairwise._update_assignment_P(s)
    P = s.P.tocoo() if hasattr(s.P, "tocoo") else s.P
    out = {q: np.asarray(getattr(s, q), dtype=np.float64) for q in QUANTITIES if q != "PXB"}
    out["PXB"] = np.asarray(P @ np.asarray(s.coordsB, dtype=np.float64), dtype=np.float64)
    return out, P


def column_gaps(P_dense, k):
    """(smallest relative gap v_k / v_{k+1} over the columns with v_{k+1} > 0, share of those at most NEAR_GAP)."""
    if k >= P_dense.shape[0]:
        return 1.0, 0.0
    v = -np.sort(-P_dense, axis=0)
    vk, vn = v[k - 1], v[k]
    sel = vn > 0
    if not sel.any():
        return 1.0, 0.0
    gap = (vk[sel] - vn[sel]) / vk[sel]
    return float(gap.min()), float((gap <= NEAR_GAP).mean())


def main():
    mc, backend, _ = mge.load_morpho_class()
    rng = np.random.default_rng(20261019)
    kl = lambda g, p=0.05: ("kl", "gauss", p, mga.counts_layer, g)  # noqa: E731
    cases = {
        "a": (dict(NA=613, NB=457, D=3, sigma2=0.04, gamma=0.6, sigma2_variance=1.0, layers=[kl(37)]), (1, 8, 64)),
        "b": (dict(NA=587, NB=441, D=2, sigma2=0.05, gamma=0.5, sigma2_variance=2.5,
                   layers=[("euc", "gauss", 20.0, mga.pca_layer, 30), ("cos", "cos", None, mga.pca_layer, 24)]), (8,)),
        "s": (dict(NA=149, NB=117, D=3, sigma2=0.07, gamma=0.5, sigma2_variance=0.5,
                   layers=[("sym_kl", "gauss", 0.08, mga.counts_layer, 26)]), (8, 200)),
    }
    out = {"cases": np.array(sorted(cases)), "quantities": np.array(QUANTITIES)}
    for tag, (kw, ks) in cases.items():
        st = mga.make_state(backend, rng, **kw)
        dense, sd = mga.run_reference(mc, backend, st)
        P_dense = np.asarray(sd.P, dtype=np.float64)
        for k in ("XAHat", "coordsB", "alpha", "SigmaDiag", "sigma2", "gamma", "samples_s", "sigma2_variance", "far"):
            out[f"{tag}_{k}"] = np.asarray(st[k])
        out[f"{tag}_dissimilarity"] = np.array(st["dissimilarity"])
        out[f"{tag}_probability_type"] = np.array(st["probability_type"])
        out[f"{tag}_probability_parameters"] = np.array([np.nan if p is None else p for p in st["probability_parameters"]])
        for l, (a, b) in enumerate(zip(st["exp_layers_A"], st["exp_layers_B"])):
            out[f"{tag}_layerA{l}"], out[f"{tag}_layerB{l}"] = a, b
        out[f"{tag}_ks"] = np.array(ks)
        for k in ks:
            ref, P = run_reference(mc, backend, st, k)
            chunk, _ = run_reference(mc, backend, st, k, use_chunk=True)
            f32, _ = run_reference(mc, backend, st, k, dtype=np.float32)
            ke = min(k, kw["NA"])
            assert P.shape == (kw["NA"], kw["NB"]) and len(P.data) == ke * kw["NB"]
            assert np.array_equal(P.col, np.repeat(np.arange(kw["NB"]), ke))   # the reference's entry order
            assert all(np.isfinite(v).all() for v in ref.values())
            # what the issue states of the mode: the kept entries are the column-wise top k of the dense P, the two spatial
            # quantities stay the dense ones
            mask = np.zeros_like(P_dense, dtype=bool)
            mask[np.asarray(P.row), np.asarray(P.col)] = True
            masked = np.where(mask, P_dense, 0.0)
            assert np.abs(masked.sum(1) - ref["K_NA"]).max() <= 1e-14 * ref["K_NA"].max()
            assert np.abs(masked.sum(0) - ref["K_NB"]).max() <= 1e-14 * ref["K_NB"].max()
            for q in ("K_NA_spatial", "K_NA_sigma2", "sigma2_related"):
                assert np.array_equal(ref[q], dense[q]), q
            gap, near = column_gaps(P_dense, ke)
            assert gap >= MIN_GAP, (tag, k, gap)
            assert near <= MAX_NEAR, (tag, k, near)
            key = f"{tag}_k{k}"
            for q in QUANTITIES:
                out[f"{key}_{q}"] = ref[q]
            out[f"{key}_row"], out[f"{key}_col"] = np.asarray(P.row, dtype=np.int32), np.asarray(P.col, dtype=np.int32)
            out[f"{key}_data"] = np.asarray(P.data, dtype=np.float64)
            out[f"{key}_floor_chunk"], out[f"{key}_floor_f32"] = mga.floors(ref, chunk), mga.floors(ref, f32)
            out[f"{key}_gap"], out[f"{key}_near"] = np.float64(gap), np.float64(near)
            print(f"case {tag} k {k} (k_eff {ke}): Sp {ref['Sp']:.4g} (dense {dense['Sp']:.4g}), gap {gap:.2e}, near {near:.3f}\n"
                  f"    chunk floor max {out[f'{key}_floor_chunk'].max():.2e}; f32 floor "
                  + ", ".join(f"{q} {v:.1e}" for q, v in zip(QUANTITIES, out[f"{key}_floor_f32"])))
    path = os.path.join(HERE, "ref_assign_topk.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
