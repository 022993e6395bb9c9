#!/usr/bin/env python
"""Golden vectors that pin the CELL MAPPING after an alignment to real reference code.

    spateo/alignment/utils.py:157-193   get_optimal_mapping_relationship
    spateo/alignment/utils.py:196-255   mapping_aligned_coords
    spateo/alignment/methods/morpho_class.py:1071-1200  Morpho_pairwise._update_assignment_P (the P that is mapped)

This script EXECUTES ``_update_assignment_P`` (through ``make_golden_assign.run_reference`` / ``make_golden_assign_label.
run_reference``) on synthetic alignment states and then the real ``mapping_aligned_coords(XAHat, coordsB, P, keep_all)`` for
both ``keep_all`` - and ``get_optimal_mapping_relationship``, whose ``keep_all=False`` pairs must be the same set - and stores
inputs and outputs in ``tests/golden/ref_assign_best.npz``.  ``spateo_amd.align.optimal_mapping`` and the restatement of
``tests/_assign_best_case.py`` are checked against the file.

The states are those of ``make_golden_assign.py`` (cases a, b, c and the small p; c is 2-D) and one of
``make_golden_assign_label.py`` (l: a "kl" layer and a label layer), each with what makes the tie rules matter:

* the far B cells they already have (all-zero columns of P) and a few far A cells (all-zero rows): the reference maps such
  a cell to the NEAREST cell of the other slice (``keep_all=False``) or to index 0 (``keep_all=True``);
* a few duplicated B cells and duplicated A cells - identical coordinates, layer rows, alpha and SigmaDiag -, which give exact
  ties of the maximum at equal distance: the smaller index.

Per case it also stores ``floor_f32`` - the float32 NumPy-backend run's ``P`` against the float64 run's, relative to max P -
``gap_rows`` / ``gap_cols`` - per row / column of the reference's P the relative gap between its maximum and the largest value
below it (duplicated cells tie exactly in most rows; where the reference's matrix product leaves them an ulp apart the gap says
so and a comparison of indices leaves the row out) - and ``near_rows`` / ``near_cols``: the share of rows / columns whose two largest distinct values lie within ``GAP_FACTOR`` x the
float32 bound of tests/_assign_best_case.py, which an index comparison in float32 has to leave out.  The maker asserts that
share to be at most ``MAX_LEFT_OUT`` = 5 %, and that no far cell's two nearest candidates lie within 1e-6 (relative) of each
other in distance, and fails instead of writing a weak file.  Layers stay on coarse grids so that the file stays small.

    python tests/golden/make_golden_assign_best.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_assign as mga  # noqa: E402
import make_golden_assign_label as mgal  # noqa: E402
import make_golden_em as mge  # noqa: E402

import _assign_best_case as bc  # noqa: E402
import _assign_case as ac  # noqa: E402

N_FAR_A = 5
MIN_DISTANCE_GAP = 1e-6


def plant(rng, st, D):
    """Far A cells and duplicated cells on a state (in place).  The far A cells leave along the second axis (the far B
    cells left along the first): out of reach of every B cell."""
    XA, XB = st["XAHat"], st["coordsB"]
    LA = st["exp_layers_A"] if "exp_layers_A" in st else st["layers_A"]
    LB = st["exp_layers_B"] if "exp_layers_B" in st else st["layers_B"]
    NA, NB = len(XA), len(XB)
    # (a duplicate whose entries the reference's BLAS leaves an ulp apart counts as a near tie for every row it heads: in a
    # small case fewer pairs, so that the share of such rows stays below the cap)
    N_DUP = 4 if NA >= 300 else 2
    near_B = np.setdiff1d(np.arange(NB), st["far"])
    # duplicated B cells: copy j1 -> j2, the pair far apart in index (other lanes, tiles and splits of the device)
    j1 = rng.choice(near_B[near_B < NB // 3], N_DUP, replace=False)
    j2 = rng.choice(near_B[near_B > 2 * NB // 3], N_DUP, replace=False)
    XB[j2] = XB[j1]
    for B in LB:
        B[j2] = B[j1]
    # duplicated A cells
    i1 = rng.choice(np.arange(NA // 3), N_DUP, replace=False)
    i2 = rng.choice(np.arange(2 * NA // 3, NA), N_DUP, replace=False)
    XA[i2] = XA[i1]
    for A in LA:
        A[i2] = A[i1]
    st["alpha"][i2], st["SigmaDiag"][i2] = st["alpha"][i1], st["SigmaDiag"][i1]
    # far A cells (none of the duplicated ones)
    free = np.setdiff1d(np.arange(NA), np.concatenate([i1, i2]))
    far_A = np.sort(rng.choice(free, N_FAR_A, replace=False))
    reach = np.sqrt(2 * st["sigma2"] * 800.0 / min(1.0, st["sigma2_variance"])) + 2 * np.abs(XA).max() * np.sqrt(D)
    XA[far_A] = XA[far_A] + reach * (1.0 + rng.random((N_FAR_A, 1))) * np.eye(D)[1]
    st["far_A"], st["dup_A"], st["dup_B"] = far_A, np.stack([i1, i2], 1), np.stack([j1, j2], 1)


def distance_gap(x, Y):
    """Relative gap between the two smallest DISTINCT distances from x to the rows of Y."""
    d = np.unique(np.sqrt(((Y - x) ** 2).sum(1)))
    return (d[1] - d[0]) / d[0] if len(d) > 1 else 1.0


def near_share(P, bound):
    gap, _ = bc.reference_gaps(P)
    return float((gap <= bc.GAP_FACTOR * bound).mean())


def main():
    mc, backend, _ = mge.load_morpho_class()
    au = mg._load("spateo.alignment.utils", "spateo/alignment/utils.py")
    rng = np.random.default_rng(20261022)
    kl = lambda g, p=0.05: ("kl", "gauss", p, mga.counts_layer, g)  # noqa: E731
    cases = {
        "a": dict(NA=613, NB=457, D=3, sigma2=0.08, gamma=0.6, sigma2_variance=1.0, layers=[kl(37)]),
        "b": dict(NA=587, NB=441, D=3, sigma2=0.05, gamma=0.5, sigma2_variance=1.0,
                  layers=[kl(29), ("cos", "cos", None, mga.pca_layer, 24)]),
        "c": dict(NA=601, NB=463, D=2, sigma2=0.1, gamma=0.7, sigma2_variance=1.0,
                  layers=[("euc", "gauss", 20.0, mga.pca_layer, 30)]),
        "p": dict(NA=149, NB=117, D=3, sigma2=0.07, gamma=0.5, sigma2_variance=0.5,
                  layers=[("square_euc", "gauss", 3.0, mga.pca_layer, 25), ("cos", "cos", None, mga.pca_layer, 24)]),
        "l": dict(NA=211, NB=157, D=3, sigma2=0.06, gamma=0.5, sigma2_variance=1.0, label=True),
    }
    out = {"cases": np.array(sorted(cases))}
    for tag, kw in cases.items():
        D = kw["D"]
        if kw.get("label"):
            st = mgal.make_state(rng, kw["NA"], kw["NB"], D, kw["sigma2"], kw["gamma"], kw["sigma2_variance"],
                                 [("kl", "gauss", 0.08, mga.counts_layer, 26)], 5, 4)
            T = mgal.table(rng, 5, 4)
            spec = [(0, "kl", "gauss", 0.08), (1, "label", "prob", None)]
            plant(rng, st, D)
            P = np.asarray(mgal.run_reference(mc, backend, st, spec, T)[1], dtype=np.float64)
            P32 = np.asarray(mgal.run_reference(mc, backend, st, spec, T, dtype=np.float32)[1], dtype=np.float64)
            LA, LB = st["layers_A"], st["layers_B"]
            meta = ([m for _, m, _, _ in spec], [p for _, _, p, _ in spec], [p for _, _, _, p in spec])
            out[f"{tag}_label_transfer"] = T
        else:
            st = mga.make_state(backend, rng, **kw)
            plant(rng, st, D)
            P = np.asarray(mga.run_reference(mc, backend, st)[1].P, dtype=np.float64)
            P32 = np.asarray(mga.run_reference(mc, backend, st, dtype=np.float32)[1].P, dtype=np.float64)
            LA, LB = st["exp_layers_A"], st["exp_layers_B"]
            meta = (st["dissimilarity"], st["probability_type"], st["probability_parameters"])
        X, Y = st["XAHat"], st["coordsB"]
        assert np.isfinite(P).all() and P.min() >= 0.0
        # ---- what the planted cells are there for
        assert not P[:, st["far"]].any() and not P[st["far_A"]].any()
        for i in st["far_A"]:
            assert distance_gap(X[i], Y) > MIN_DISTANCE_GAP, (tag, "far A cell", i)
        for j in st["far"]:
            assert distance_gap(Y[j], X) > MIN_DISTANCE_GAP, (tag, "far B cell", j)
        # (a duplicate's entries are equal up to what the reference's BLAS makes of the position in the matrix: equal bits in
        # most cases, an ulp apart in some - then the reference itself sees no tie, and the checker leaves the row out)
        for (j1, j2) in st["dup_B"]:
            assert np.allclose(P[:, j1], P[:, j2], rtol=1e-12, atol=0.0)
        for (i1, i2) in st["dup_A"]:
            assert np.allclose(P[i1], P[i2], rtol=1e-12, atol=0.0)
        _, tied_rows = bc.reference_gaps(P)
        _, tied_cols = bc.reference_gaps(P.T)
        live_r, live_c = tied_rows & (P.max(1) > 0), tied_cols & (P.max(0) > 0)
        # (the ulp above: a case may lose its exact ties in one direction; every case keeps some, the large ones both kinds)
        assert live_r.sum() + live_c.sum() >= 1, (tag, "no exact tie of a positive maximum")
        assert len(X) < 300 or (live_r.sum() >= 1 and live_c.sum() >= 1), (tag, live_r.sum(), live_c.sum())
        # ---- the float32 floor of P and the share of near ties under the float32 bound
        floor = float(np.abs(P32 - P).max() / P.max())
        bound = max(ac.ALLOW * floor, ac.F32_BASE)
        near_r, near_c = near_share(P, bound), near_share(P.T, bound)
        assert near_r <= bc.MAX_LEFT_OUT and near_c <= bc.MAX_LEFT_OUT, (tag, near_r, near_c)
        # ---- the real mapping
        ours = bc.best_of(P, X, Y)
        for keep_all, name, col in ((False, "nearest", 0), (True, "all", 1)):
            by_A, by_B = au.mapping_aligned_coords(X, Y, P, keep_all=keep_all)
            for side, m, n, own in (("A", by_A, len(X), 0), ("B", by_B, len(Y), 1)):
                idx, val = np.asarray(m["pi_index"]), np.asarray(m["pi_value"], dtype=np.float64)
                assert idx.shape == (n, 2) and np.array_equal(idx[:, own], np.arange(n))       # sorted, one per cell
                assert np.array_equal(m["mapping_X"], X[idx[:, 0]]) and np.array_equal(m["mapping_Y"], Y[idx[:, 1]])
                assert np.array_equal(val, P[idx[:, 0], idx[:, 1]])
                out[f"{tag}_{name}_{side}_index"], out[f"{tag}_{name}_{side}_value"] = idx.astype(np.int16), val
                # the restatement of tests/_assign_best_case.py says the same
                mine = ours["rows" if side == "A" else "cols"][:, col]
                assert np.array_equal(mine, idx[:, 1 - own]), (tag, name, side, np.flatnonzero(mine != idx[:, 1 - own])[:8])
        Xi, _, Yi, _ = au.get_optimal_mapping_relationship(X=X, Y=Y, pi=P, keep_all=False)
        assert {tuple(r) for r in Xi.tolist()} == {tuple(r) for r in out[f"{tag}_nearest_A_index"].tolist()}
        assert {tuple(r) for r in Yi.tolist()} == {tuple(r) for r in out[f"{tag}_nearest_B_index"].tolist()}
        # the zero rows: the two rules differ (the nearest B cell of a far A cell is not cell 0)
        assert (ours["rows"][st["far_A"], 0] != 0).any() and not ours["rows"][st["far_A"], 1].any()
        # ---- the inputs
        for k in ("XAHat", "coordsB", "alpha", "SigmaDiag", "sigma2", "gamma", "samples_s", "sigma2_variance", "far", "far_A",
                  "dup_A", "dup_B"):
            out[f"{tag}_{k}"] = np.asarray(st[k])
        out[f"{tag}_dissimilarity"], out[f"{tag}_probability_type"] = np.array(meta[0]), np.array(meta[1])
        out[f"{tag}_probability_parameters"] = np.array([np.nan if p is None else p for p in meta[2]])
        for l, (a, b) in enumerate(zip(LA, LB)):
            integer = np.issubdtype(np.asarray(a).dtype, np.integer)
            out[f"{tag}_layerA{l}"], out[f"{tag}_layerB{l}"] = (a.astype(np.int16), b.astype(np.int16)) if integer else (a, b)
        # the reference P's own gaps (tests/_assign_best_case.reference_gaps): where IT decides the mapping it stored
        out[f"{tag}_gap_rows"] = bc.reference_gaps(P)[0].astype(np.float32)
        out[f"{tag}_gap_cols"] = bc.reference_gaps(P.T)[0].astype(np.float32)
        out[f"{tag}_floor_f32"], out[f"{tag}_near_rows"], out[f"{tag}_near_cols"] = np.float64(floor), np.float64(near_r), np.float64(near_c)
        if tag == "p":
            out["p_P"] = P
        print(f"case {tag}: {P.shape} D {D} {list(meta[0])}: f32 floor of P {floor:.2e} (bound {bound:.2e}), near ties rows "
              f"{near_r:.3f} columns {near_c:.3f}, exact ties of a positive maximum rows {int(live_r.sum())} columns "
              f"{int(live_c.sum())}, zero rows {int((P.max(1) == 0).sum())} zero columns {int((P.max(0) == 0).sum())}")
    path = os.path.join(HERE, "ref_assign_best.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
