#!/usr/bin/env python
"""Golden vectors for the assignment APPLIED to cell features: ``P @ F_B`` and ``P.T @ F_A`` with ``P`` from real reference code.

    spateo/alignment/methods/morpho_class.py:1071-1200  Morpho_pairwise._update_assignment_P   (self.P)

This script EXECUTES ``_update_assignment_P`` exactly as ``make_golden_assign.py`` does (its ``run_reference``, on the inputs
that ``tests/golden/ref_assign.npz`` already stores - they are not stored again) and multiplies the dense ``P`` it leaves in
``self.P`` with synthetic cell features in float64: what a user of the reference forms from ``Morpho_pairwise.run()``'s
result.  ``spateo_amd.align.apply_assignment`` and the NumPy restatement of ``tests/_assign_transfer_case.py`` are checked
against ``tests/golden/ref_assign_transfer.npz``.

Features, per case and width C: the first C // 2 columns one-hot (a label vector with C // 2 classes), the rest standard
normal.  Cases ``a`` (one layer), ``b`` (two layers), ``c`` (2-D) at C = 5; case ``p`` (two layers, small) at C = 5 and 70 - two
64-column chunks - which keeps the file below 1 MB.  Per case: ``K_NA`` / ``K_NB`` (the row / column sums of ``P``) and, per
width, the four quantities

    to_A_raw = P @ F_B    to_A_norm = rows of it over K_NA    to_B_raw = P.T @ F_A    to_B_norm = rows of it over K_NB

(a cell whose sum is 0 keeps a zero row), the scale each deviation is taken relative to - ``max (P @ |F|)`` for the raw
products, ``max |F|`` for the normalised ones - and two floors measured on the reference itself on those scales: ``chunk``
(the ``use_chunk=True`` run's ``P``) and ``f32`` (the float32 NumPy-backend run's ``P``, multiplied and normalised in float32).

    python tests/golden/make_golden_assign_transfer.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _assign_case as ac  # noqa: E402
import make_golden_assign as mga  # noqa: E402
import make_golden_em as mge  # noqa: E402

QUANTITIES = ("to_A_raw", "to_A_norm", "to_B_raw", "to_B_norm")
WIDTHS = {"a": (5,), "b": (5,), "c": (5,), "p": (5, 70)}


def features(rng, n, c):
    """(n, c): c // 2 one-hot columns of a random label vector, then standard normal columns."""
    F = rng.standard_normal((n, c))
    k = c // 2
    F[:, :k] = 0.0
    F[np.arange(n), rng.integers(0, k, n)] = 1.0
    return F


def normalized(M, K):
    out = np.zeros_like(M)
    live = K != 0
    out[live] = M[live] / K[live, None]
    return out


def products(P, F_A, F_B, dtype=np.float64):
    """The four quantities from a dense P, formed in `dtype` arithmetic and returned as float64."""
    P, F_A, F_B = P.astype(dtype), F_A.astype(dtype), F_B.astype(dtype)
    to_A, to_B = P @ F_B, P.T @ F_A
    out = {"to_A_raw": to_A, "to_A_norm": normalized(to_A, P.sum(1)), "to_B_raw": to_B, "to_B_norm": normalized(to_B, P.sum(0))}
    return {q: np.asarray(v, dtype=np.float64) for q, v in out.items()}


def scales(P, F_A, F_B):
    return np.array([(P @ np.abs(F_B)).max(), np.abs(F_B).max(), (P.T @ np.abs(F_A)).max(), np.abs(F_A).max()])


def floors(ref, other, scale, K_NA, K_NB):
    """max |other - ref| / scale per quantity; the normalised ones over every cell with a non-zero sum, none left out."""
    out = []
    for q, s in zip(QUANTITIES, scale):
        live = slice(None) if q.endswith("raw") else ((K_NA if q.startswith("to_A") else K_NB) != 0)
        out.append(np.abs(other[q][live] - ref[q][live]).max() / s)
    return np.array(out)


def state_of(g, tag):
    args, kw = ac.case_inputs(g, tag)
    return dict(XAHat=args[0], coordsB=args[1], exp_layers_A=args[2], exp_layers_B=args[3], alpha=kw["alpha"],
                SigmaDiag=kw["SigmaDiag"], sigma2=kw["sigma2"], gamma=kw["gamma"], samples_s=kw["samples_s"],
                sigma2_variance=kw["sigma2_variance"], dissimilarity=kw["dissimilarity"], probability_type=kw["probability_type"],
                probability_parameters=kw["probability_parameters"])


def main():
    mc, backend, _ = mge.load_morpho_class()
    g = ac.load()
    rng = np.random.default_rng(20261019)
    out = {"cases": np.array(sorted(WIDTHS)), "quantities": np.array(QUANTITIES)}
    for tag, widths in WIDTHS.items():
        st = state_of(g, tag)
        ref, s = mga.run_reference(mc, backend, st)
        assert np.array_equal(ref["K_NA"], g[f"{tag}_K_NA"]) and np.array_equal(ref["K_NB"], g[f"{tag}_K_NB"])   # ref_assign.npz's run
        P = np.asarray(s.P, dtype=np.float64)
        _, sc = mga.run_reference(mc, backend, st, use_chunk=True)
        _, s32 = mga.run_reference(mc, backend, st, dtype=np.float32)
        P_chunk, P32 = np.asarray(sc.P, dtype=np.float64), np.asarray(s32.P)
        assert P32.dtype == np.float32
        K_NA, K_NB = P.sum(1), P.sum(0)
        far = g[f"{tag}_far"]
        assert not K_NB[far].any() and 9 <= int((K_NB == 0).sum()) <= 33
        out[f"{tag}_widths"], out[f"{tag}_K_NA"], out[f"{tag}_K_NB"] = np.array(widths), K_NA, K_NB
        for c in widths:
            F_A, F_B = features(rng, len(K_NA), c), features(rng, len(K_NB), c)
            want = products(P, F_A, F_B)
            scale = scales(P, F_A, F_B)
            pre = f"{tag}_c{c}_"
            out[pre + "F_A"], out[pre + "F_B"], out[pre + "scale"] = F_A, F_B, scale
            for q in QUANTITIES:
                out[pre + q] = want[q]
            out[pre + "floor_chunk"] = floors(want, products(P_chunk, F_A, F_B), scale, K_NA, K_NB)
            out[pre + "floor_f32"] = floors(want, products(P32, F_A, F_B, np.float32), scale, K_NA, K_NB)
            print(f"case {tag} C {c}: {P.shape[0]} x {P.shape[1]}, zero rows {(K_NA == 0).sum()}, zero columns {(K_NB == 0).sum()}, "
                  f"smallest non-zero sum {min(K_NA[K_NA > 0].min(), K_NB[K_NB > 0].min()):.1e}\n    scales "
                  + ", ".join(f"{q} {v:.3g}" for q, v in zip(QUANTITIES, scale)) + "\n    chunk floor "
                  + ", ".join(f"{v:.1e}" for v in out[pre + "floor_chunk"]) + "; f32 floor "
                  + ", ".join(f"{v:.1e}" for v in out[pre + "floor_f32"]))
    path = os.path.join(HERE, "ref_assign_transfer.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
