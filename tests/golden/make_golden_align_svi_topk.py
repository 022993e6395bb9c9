#!/usr/bin/env python
"""Golden vectors that pin the SVI MODE of the alignment loop in ``sparse_calculation_mode`` to real reference code: cases 2
and 3 of ``make_golden_align_svi.py`` (its ``run_loop``, its batch permutations, its 30 iterations of 150 cells) with
``sparse_calculation_mode=True, sparse_top_k=16`` - every batch's assignment and the closing full one of
``return_mapping=True`` keep the 16 largest entries of each column of ``P`` (``get_P_core`` -> ``_dense_to_sparse``,
``spateo/alignment/methods/utils.py:1085-1094, 1369-1404``; ``morpho_class.py:299-302``).

``make_golden_align_svi.run_loop`` builds its own state with the mode off; here ``Morpho_pairwise._update_assignment_P`` is
wrapped for the duration of a run so that it switches the mode on first (and, for the gaps, runs the dense path on a copy
of the state before).  Stored in ``tests/golden/ref_align_svi_topk.npz``: what ``ref_align_svi.npz`` stores per case (the
inputs are ``ref_align_loop.npz``'s), plus ``gap`` - the smallest relative gap between the 16th and the 17th largest value of
a column of the dense ``P`` over the columns whose 17th value is positive, over every assignment of the run - and the closing
assignment's sparse ``P`` (``P_row``, ``P_data``; ``col = repeat(arange(NB), 16)``).  The maker asserts gap >= 1e-7, the chunk
floors <= 1e-9 and the dense maker's conditions.

    python tests/golden/make_golden_align_svi_topk.py
"""
from __future__ import annotations

import contextlib
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_align_loop as mgl  # noqa: E402
import make_golden_align_svi as mgs  # noqa: E402
import make_golden_assign as mga  # noqa: E402
import make_golden_assign_topk as mgt  # noqa: E402
import make_golden_em as mge  # noqa: E402

TOP_K = 16
CASES = ("2", "3")
SCALARS, ARRAYS, FINALS, ITERS, PERTURB = mgs.SCALARS, mgs.ARRAYS, mgs.FINALS, mgs.ITERS, mgs.PERTURB


@contextlib.contextmanager
def sparse_mode(mc, record):
    """Within the block the real _update_assignment_P runs with sparse_calculation_mode=True, sparse_top_k=TOP_K; record:
    {"gap": ..., "P": the last sparse P} (gap only when record["gaps"])."""
    orig = mc.Morpho_pairwise._update_assignment_P

    def wrapped(s):
        if record.get("gaps"):
            d = copy.copy(s)
            d.sparse_calculation_mode = False
            orig(d)
            g, _ = mgt.column_gaps(np.asarray(d.P, dtype=np.float64), min(TOP_K, s.NA))
            record["gap"] = min(record.get("gap", 1.0), g)
        s.sparse_calculation_mode, s.sparse_top_k = True, TOP_K
        orig(s)
        record["P"] = s.P

    mc.Morpho_pairwise._update_assignment_P = wrapped
    try:
        yield
    finally:
        mc.Morpho_pairwise._update_assignment_P = orig


def main():
    mc, backend, utils = mge.load_morpho_class()
    dense = np.load(os.path.join(HERE, "ref_align_loop.npz"))
    svi = np.load(os.path.join(HERE, "ref_align_svi.npz"))
    rng = np.random.default_rng(20261018)   # the dense maker's seed and its order of cases
    kl = ("kl", "gauss", 0.1, mga.counts_layer, 40)
    cases = {
        "1": mgl.make_case(rng, 607, 451, 3, [kl], 0.45),
        "2": mgl.make_case(rng, 593, 447, 3, [("kl", "gauss", 0.1, mga.counts_layer, 31), ("cos", "cos", None, mga.pca_layer, 24)],
                           0.5, far_fraction=0.07),
        "3": mgl.make_case(rng, 611, 443, 2, [("euc", "gauss", 20.0, mga.pca_layer, 30)], 0.4, inliers=60,
                           partial_robust_level=3.0, n_ctrl=16, beta=1.0),
    }
    out = {"cases": np.array(CASES), "iters": np.int64(ITERS), "arr_iters": np.array(mgs.ARR_ITERS), "batch_size": np.int64(mgs.BATCH),
           "top_k": np.int64(TOP_K), "scalars": np.array(SCALARS), "arrays": np.array(ARRAYS), "finals": np.array(FINALS)}
    for tag in CASES:
        case = cases[tag]
        XA, XB = case["coordsA"], case["coordsB"]
        case["samples_s"] = float(max(np.prod(XA.max(0) - XA.min(0)), np.prod(XB.max(0) - XB.min(0))))
        assert np.array_equal(dense[f"{tag}_coordsA"], XA) and np.array_equal(dense[f"{tag}_coordsB"], XB), tag
        perm = np.random.default_rng(100 + int(tag)).permutation(len(XB))
        assert np.array_equal(svi[f"{tag}_batch_perm"], perm)            # the dense SVI fixture's schedule
        rec = {"gaps": True}
        with sparse_mode(mc, rec):
            ref, kernel, runs = mgs.run_loop(mc, backend, utils, case, perm)
        assert np.array_equal(kernel[0], dense[f"{tag}_inducing_variables"]), tag
        P = rec["P"].tocoo()
        with sparse_mode(mc, {}):
            chunk, _, _ = mgs.run_loop(mc, backend, utils, case, perm, use_chunk=True, kernel=kernel)
            f32, _, _ = mgs.run_loop(mc, backend, utils, case, perm, dtype=np.float32, kernel=kernel)
            prng = np.random.default_rng(int(tag))
            XBp = XB * (1.0 + PERTURB * prng.standard_normal(XB.shape))
            pert, _, _ = mgs.run_loop(mc, backend, utils, case, perm, coordsB=XBp, kernel=kernel)
        g = {q: np.maximum.accumulate(v / PERTURB) for q, v in mgs.twin_deviation(ref, pert).items()}
        fl_chunk, fl_f32 = mgs.twin_deviation(ref, chunk), mgs.twin_deviation(ref, f32)
        assert all(np.isfinite(v).all() for v in ref.values()), tag
        gmax = max(float(v.max()) for v in g.values())
        cmax = max(float(v.max()) for v in fl_chunk.values())
        assert gmax <= 100.0, (tag, {q: float(v.max()) for q, v in g.items()})
        assert runs >= 8 and np.linalg.norm(ref["R"][-1] - case["R0"]) <= 0.05, (tag, runs)
        assert rec["gap"] >= mgt.MIN_GAP, (tag, rec["gap"])
        assert cmax <= 1e-9, (tag, cmax)
        assert P.shape == (len(XA), len(XB)) and np.array_equal(P.col, np.repeat(np.arange(len(XB)), TOP_K))
        out[f"{tag}_inputs_of"] = np.array(tag)
        out[f"{tag}_nonrigid_start_iter"] = np.int64(case["nonrigid_start_iter"])
        out[f"{tag}_batch_perm"] = perm.astype(np.int16)
        out[f"{tag}_step_size"] = ref["step_size"]
        for q in SCALARS + ARRAYS + FINALS:
            out[f"{tag}_{q}"] = ref[q]
            out[f"{tag}_g_{q}"], out[f"{tag}_chunk_{q}"], out[f"{tag}_f32_{q}"] = g[q], fl_chunk[q], fl_f32[q]
        out[f"{tag}_gap"] = np.float64(rec["gap"])
        out[f"{tag}_P_row"], out[f"{tag}_P_data"] = np.asarray(P.row, dtype=np.int32), np.asarray(P.data, dtype=np.float64)
        print(f"case {tag}: sigma2 {ref['sigma2'][0]:.4g} -> {ref['sigma2'][-1]:.4g}, Sp_map {float(ref['Sp_map']):.5g} (dense "
              f"{float(svi[f'{tag}_Sp_map']):.5g}), gap {rec['gap']:.2e}, non-rigid in {runs}, max g {gmax:.3g}, chunk floor {cmax:.1e}\n"
              "    f32 floor   " + ", ".join(f"{q} {fl_f32[q].max():.1e}" for q in SCALARS + ARRAYS + FINALS))
    path = os.path.join(HERE, "ref_align_svi_topk.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
