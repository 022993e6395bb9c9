"""Writes tests/golden/ref_kde.npz: what ``sklearn.neighbors.KernelDensity`` - the one call of the reference's ``pc_KDE``
(spateo/tdr/morphometrics/morphology.py:109) - gives on the cases of tests/_kde_cases.py.

For every case: ``skdev_<name>``, the deviation max |restatement - sklearn| / max(1, |sklearn|) over the finite entries (one of
the two terms of the GPU bound; the -inf patterns are asserted equal here), and ``xdev_<name>``, the same deviation between the
restatement and its own arithmetic in ``np.longdouble`` (the tighter bound of the cases on which sklearn itself is far off).  For the cases of ``GOLDEN_FULL``: the centred inputs
and sklearn's ``score_samples`` themselves (``<name>_T``, ``_X``, ``_w``, ``_g``, ``_score``), per group where the case has
groups; a group without a source or whose weights are all zero is a column of -inf (sklearn has nothing to fit).

Run from the repository root where sklearn is installed:  python tests/golden/make_golden_kde.py"""
import os
import sys

import numpy as np
import sklearn
from sklearn.neighbors import KernelDensity

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _kde_cases as kc  # noqa: E402


def sklearn_scores(case):
    T, X, w, g, C = case["T"], case["X"], case["w"], case["g"], case["C"]
    out = np.full((len(T), C), -np.inf)
    for c in range(C):
        sel = np.ones(len(X), dtype=bool) if g is None else g == c
        wc = None if w is None else w[sel]
        if not sel.any() or (wc is not None and not (wc > 0).any()):
            continue
        with np.errstate(divide="ignore"):
            out[:, c] = KernelDensity(kernel=case["kernel"], bandwidth=case["h"]).fit(X[sel], sample_weight=wc).score_samples(T)
    return out


def main():
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name, case in kc.CASES.items():
        kc.assert_decidable(case)
        score = sklearn_scores(case)
        ref = kc.log_density(case)
        # Where the exact sum is empty (a compact kernel with every source beyond h: decidable by assert_decidable) sklearn's
        # tree returns -inf or the rounding residue of its bound arithmetic (log-densities some 30 below the column's largest);
        # such entries are stored as the -inf they stand for.  The converse - sklearn empty where the sum is not - must not occur.
        empty = ~np.isfinite(ref)
        residue = empty & np.isfinite(score)
        if residue.any():
            top = np.where(np.isfinite(score) & ~empty, score, -np.inf).max(axis=0)
            assert (score[residue] < np.broadcast_to(top, score.shape)[residue] - 27.0).all(), name   # below 2e-12 of the largest
            print(f"  {name}: {int(residue.sum())} sklearn residues in empty entries, largest {score[residue].max():.2f}")
            score[residue] = -np.inf
        assert np.array_equal(np.isfinite(score), np.isfinite(ref)), name
        dev = kc.deviation(ref, score, score)
        xdev = kc.deviation(ref, kc.log_density(case, extended=True), ref)
        out[f"skdev_{name}"], out[f"xdev_{name}"] = np.float64(dev), np.float64(xdev)
        print(f"{name}: n={len(case['T'])} N={len(case['X'])} d={case['d']} C={case['C']} {case['kernel']}: "
              f"|restatement - sklearn| / max(1, |ref|) = {dev:.3e}, |restatement - extended| = {xdev:.3e}, "
              f"-inf entries {int((~np.isfinite(score)).sum())}")
        if name in kc.GOLDEN_FULL:
            out[f"{name}_T"], out[f"{name}_X"], out[f"{name}_score"] = case["T"], case["X"], score
            if case["w"] is not None:
                out[f"{name}_w"] = case["w"]
            if case["g"] is not None:
                out[f"{name}_g"] = case["g"]
    path = os.path.join(HERE, "ref_kde.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
