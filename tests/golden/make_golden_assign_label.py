#!/usr/bin/env python
"""Golden vectors that pin the ``"label"`` LAYER of Spateo's alignment to real reference code.

    spateo/alignment/methods/utils.py:791-832, 908-910   _label_distance_backend: D = label_transfer[labelA, :][:, labelB]
    spateo/alignment/methods/utils.py:264-312, 376-436   check_label_transfer / generate_label_transfer_dict
    spateo/alignment/methods/morpho_class.py:1071-1200   Morpho_pairwise._update_assignment_P, and the loop of ``run``

This script EXECUTES ``_update_assignment_P`` (unbound, on a ``SimpleNamespace`` self with ``label_transfer`` set, NumPy
backend) the way ``make_golden_assign.py`` / ``make_golden_assign_topk.py`` do, and the real loop the way
``make_golden_align_loop.py`` / ``make_golden_align_svi.py`` do, and stores inputs and outputs in
``tests/golden/ref_assign_label.npz``.  A label layer's entries in ``exp_layers_A / B`` are integer vectors; every table is
made of multiples of 1/64, so that the float32 and the float64 reference runs read the same table.

Step cases (``QUANTITIES`` of make_golden_assign.py, the floors ``chunk`` / ``f32`` per quantity, 7 % far B cells each):

    a   the label layer alone (``prob``), NA = 149, NB = 117, K = 5, L = 4; the dense ``P`` is stored
    b   one ``kl`` / ``gauss`` layer + the label layer (``prob``), 587 x 441, D = 3
    c   b with the label layer first          d   b with ``gauss`` on the label layer          e   b with ``cos`` on it
    f   D = 2 (``euc`` / ``gauss`` + label)
    z   211 x 157, K = 6, L = 5, a table with zeros: no A label transfers to B label 3 (those columns: S3 = 0, K_NB = 0 and
        P = 0 exactly, asserted here on the reference), only the rare A label 5 transfers to the rare B label 4 (those columns
        have fewer positive entries than k = 64); in ``sparse_calculation_mode`` with k = 1, 8, 64 as well: the reference's
        coo matrix and ``colgap``, per column (v_k - v_{k+1}) / v_k of the dense P (1 where v_{k+1} = 0 < v_k, 0 where v_k = 0)

Loops (one ``kl`` layer + one label layer, the labels five bands along the first axis): ``loop.*`` - 12 iterations of the
dense loop, the keys of ``ref_align_loop.npz``; ``svi.*`` - 30 iterations with 150-cell batches from a stored
``batch_perm``, the keys of ``ref_align_svi.npz``; both with the three twins (chunk, float32, perturbed) of those makers and
their assertions.  The two loop makers' ``run_loop`` are used as they are: they build the namespace with float layers and
no table, so ``_update_assignment_P`` is entered through a wrapper that first puts the integer labels and the table (in
the run's dtype) on the namespace.

``label_transfer_matrix`` cases: what the real ``check_label_transfer`` returns for two category lists, without and with a
dictionary (on an object with the two ``.obs[key].cat.categories`` the function reads).

    python tests/golden/make_golden_assign_label.py
"""
from __future__ import annotations

import contextlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_align_loop as mgl  # noqa: E402
import make_golden_align_svi as mgs  # noqa: E402
import make_golden_assign as mga  # noqa: E402
import make_golden_em as mge  # noqa: E402

QUANTITIES = mga.QUANTITIES
KS = (1, 8, 64)


def table(rng, K, L, diag=48):
    """K x L multiples of 1/64 in (0, 1): large where row and column agree (mod L), small elsewhere."""
    T = rng.integers(1, 12, (K, L)).astype(np.float64)
    for j in range(K):
        T[j, j % L] = diag + rng.integers(0, 12)
    return T / 64.0


def make_state(rng, NA, NB, D, sigma2, gamma, sigma2_variance, feature_layers, K, L, rare=False):
    """make_golden_assign.make_state plus one label vector per slice: the cell type (A: 0 .. 4, B: the source cell's, folded
    into 0 .. 3); `rare`: 5 % of the A cells carry the extra label K - 1 and two near B cells the extra label L - 1."""
    XA = rng.standard_normal((NA, D))
    src = rng.choice(NA, NB)
    XB = XA[src] + 0.15 * rng.standard_normal((NB, D))
    far = rng.choice(NB, max(1, int(np.ceil(mga.FAR_FRACTION * NB))), replace=False)
    reach = np.sqrt(2 * sigma2 * 800.0 / min(1.0, sigma2_variance)) + 2 * np.abs(XA).max() * np.sqrt(D)
    XB[far] = XA[src[far]] + reach * (1.0 + rng.random((len(far), 1))) * np.eye(D)[0]
    typA = rng.integers(0, 5, NA)
    typB = typA[src]
    LA, LB = [], []
    for (_, _, _, maker, g) in feature_layers:
        st = rng.bit_generator.state
        LA.append(maker(rng, NA, g, typA))
        rng.bit_generator.state = st
        LB.append(maker(rng, NB, g, typB))
    labA, labB = typA % (K - rare), typB % (L - rare)
    if rare:
        labA[rng.choice(NA, int(np.ceil(0.05 * NA)), replace=False)] = K - 1
        labB[rng.choice(np.setdiff1d(np.arange(NB), far), 2, replace=False)] = L - 1
    assert labA.max() == K - 1 and labB.max() == L - 1   # the last row and the last column of the table are read
    LA.append(labA.astype(np.int64)), LB.append(labB.astype(np.int64))
    return dict(XAHat=XA, coordsB=XB, layers_A=LA, layers_B=LB, alpha=rng.uniform(0.5, 1.0, NA),
                SigmaDiag=sigma2 * rng.uniform(0.0, 0.3, NA), sigma2=float(sigma2), gamma=float(gamma),
                samples_s=float(np.prod(XA.max(0) - XA.min(0))), sigma2_variance=float(sigma2_variance), far=np.sort(far))


def run_reference(mc, backend, st, spec, T, dtype=np.float64, use_chunk=False, k=None):
    """The real _update_assignment_P on the state `st` with the layers `spec` = [(stored layer, metric, prob, param)]."""
    c = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    lay = lambda a: np.asarray(a) if np.issubdtype(np.asarray(a).dtype, np.integer) else c(a)  # noqa: E731
    NA, D = st["XAHat"].shape
    s = types.SimpleNamespace(
        nx=backend.NumpyBackend(), type_as=np.zeros(1, dtype=dtype), Dim=dtype(D), NA=NA, NB=len(st["coordsB"]),
        XAHat=c(st["XAHat"]), coordsB=c(st["coordsB"]), exp_layers_A=[lay(st["layers_A"][i]) for i, *_ in spec],
        exp_layers_B=[lay(st["layers_B"][i]) for i, *_ in spec], alpha=c(st["alpha"]), SigmaDiag=c(st["SigmaDiag"]),
        sigma2=dtype(st["sigma2"]), gamma=dtype(st["gamma"]), samples_s=dtype(st["samples_s"]),
        sigma2_variance=dtype(st["sigma2_variance"]), dissimilarity=[m for _, m, _, _ in spec],
        probability_type=[p for _, _, p, _ in spec],
        probability_parameters=[None if p is None else dtype(p) for _, _, _, p in spec],
        sparse_calculation_mode=k is not None, sparse_top_k=-1 if k is None else int(k), use_chunk=use_chunk, split_size=128,
        SVI_mode=False, pre_compute_dist=False, label_transfer=c(T), batch_idx=None,
    )
    assert np.array_equal(s.label_transfer, T)   # representable in the run's dtype
    mc.Morpho_pairwise._update_assignment_P(s)
    P = s.P.tocoo() if hasattr(s.P, "tocoo") else np.asarray(s.P)
    out = {q: np.asarray(getattr(s, q), dtype=np.float64) for q in QUANTITIES if q != "PXB"}
    out["PXB"] = np.asarray(P @ np.asarray(s.coordsB, dtype=np.float64), dtype=np.float64)
    return out, P


def column_gaps(P, k):
    """Per column (v_k - v_{k+1}) / v_k of the dense P: 1 where v_{k+1} = 0 < v_k or every row is kept, 0 where v_k = 0."""
    if k >= P.shape[0]:
        return np.ones(P.shape[1])
    v = -np.sort(-P, axis=0)
    vk, vn = v[k - 1], v[k]
    return np.where(vk > 0, (vk - vn) / np.where(vk > 0, vk, 1.0), 0.0)


@contextlib.contextmanager
def label_layers(mc, labels_A, labels_B, T):
    """Inside: Morpho_pairwise._update_assignment_P sees the LAST layer as the label layer (integer vectors) and the table."""
    real = mc.Morpho_pairwise._update_assignment_P

    def entered(s, *a, **kw):
        s.exp_layers_A[-1], s.exp_layers_B[-1] = labels_A, labels_B
        s.label_transfer = np.asarray(T, dtype=s.type_as.dtype)
        return real(s, *a, **kw)

    mc.Morpho_pairwise._update_assignment_P = entered
    try:
        yield
    finally:
        mc.Morpho_pairwise._update_assignment_P = real


def loop_case(rng, K=5, L=4):
    """Case 1 of make_golden_align_loop.py's kind plus a label layer: five bands along the first axis of the common frame."""
    case = mgl.make_case(rng, 607, 451, 3, [("kl", "gauss", 0.1, mga.counts_layer, 40)], 0.45)
    XA, XB = case["coordsA"], case["coordsB"]
    case["samples_s"] = float(max(np.prod(XA.max(0) - XA.min(0)), np.prod(XB.max(0) - XB.min(0))))
    ZA = XA @ case["R0"].T + case["t0"]
    edges = np.quantile(ZA[:, 0], np.arange(1, K) / K)
    labA, labB = np.searchsorted(edges, ZA[:, 0]), np.minimum(np.searchsorted(edges, XB[:, 0]), L - 1)
    case["exp_layers_A"].append(labA.astype(np.float64)), case["exp_layers_B"].append(labB.astype(np.float64))
    case["dissimilarity"].append("label"), case["probability_type"].append("prob"), case["probability_parameters"].append(None)
    return case, labA.astype(np.int64), labB.astype(np.int64), table(rng, K, L)


def store_loop(out, pre, tag, case, labA, labB, T, ref, g, fl_chunk, fl_f32, kernel, finals):
    out[f"{pre}{tag}_sigma2_init"] = np.float64(case["sigma2"])
    for k in ("coordsA", "coordsB", "samples_s", "beta", "lambdaVF", "nonrigid_start_iter", "partial_robust_level",
              "nn_init_weight", "kappa", "gamma_a", "gamma_b"):
        out[f"{pre}{tag}_{k}"] = np.asarray(case[k])
    out[f"{pre}{tag}_inducing_variables"] = np.asarray(kernel[0])
    out[f"{pre}{tag}_layerA0"], out[f"{pre}{tag}_layerB0"] = case["exp_layers_A"][0], case["exp_layers_B"][0]
    out[f"{pre}{tag}_layerA1"], out[f"{pre}{tag}_layerB1"] = labA.astype(np.int16), labB.astype(np.int16)
    out[f"{pre}{tag}_label_transfer"] = T
    out[f"{pre}{tag}_dissimilarity"] = np.array(case["dissimilarity"])
    out[f"{pre}{tag}_probability_type"] = np.array(case["probability_type"])
    out[f"{pre}{tag}_probability_parameters"] = np.array([np.nan if p is None else p for p in case["probability_parameters"]])
    for q in mgl.SCALARS + mgl.ARRAYS + tuple(finals):
        out[f"{pre}{tag}_{q}"] = ref[q]
        out[f"{pre}{tag}_g_{q}"], out[f"{pre}{tag}_chunk_{q}"], out[f"{pre}{tag}_f32_{q}"] = g[q], fl_chunk[q], fl_f32[q]
    names = mgl.SCALARS + mgl.ARRAYS + tuple(finals)
    print(f"{pre}{tag}: sigma2 {ref['sigma2'][0]:.4g} -> {ref['sigma2'][-1]:.4g}, |R - R0| "
          f"{np.linalg.norm(ref['R'][-1] - case['R0']):.3g}, max g {max(float(v.max()) for v in g.values()):.3g}\n"
          "    chunk floor " + ", ".join(f"{q} {fl_chunk[q].max():.1e}" for q in names) + "\n"
          "    f32 floor   " + ", ".join(f"{q} {fl_f32[q].max():.1e}" for q in names))


def loops(mc, backend, utils, out):
    rng = np.random.default_rng(20261021)
    case, labA, labB, T = loop_case(rng)
    with label_layers(mc, labA, labB, T):
        # ---- the dense loop ----
        ref, s, kernel, info = mgl.run_loop(mc, backend, utils, case)
        chunk, _, _, _ = mgl.run_loop(mc, backend, utils, case, use_chunk=True, kernel=kernel)
        f32, _, _, _ = mgl.run_loop(mc, backend, utils, case, dtype=np.float32, kernel=kernel)
        XBp = case["coordsB"] * (1.0 + mgl.PERTURB * np.random.default_rng(1).standard_normal(case["coordsB"].shape))
        pert, _, _, _ = mgl.run_loop(mc, backend, utils, case, coordsB=XBp, kernel=kernel)
        g = {q: np.maximum.accumulate(v / mgl.PERTURB) for q, v in mgl.twin_deviation(ref, pert).items()}
        assert all(np.isfinite(v).all() for v in ref.values())
        assert max(float(v.max()) for v in g.values()) <= 100.0, {q: float(v.max()) for q, v in g.items()}
        assert info["nonrigid_runs"] >= 8 and np.linalg.norm(ref["R"][-1] - case["R0"]) <= 0.05
        assert np.issubdtype(s.exp_layers_A[-1].dtype, np.integer) and s.label_transfer is not None
        out["loop.cases"], out["loop.iters"], out["loop.arr_iters"] = np.array(["L"]), np.int64(mgl.ITERS), np.array(mgl.ARR_ITERS)
        store_loop(out, "loop.", "L", case, labA, labB, T, ref, g, mgl.twin_deviation(ref, chunk), mgl.twin_deviation(ref, f32),
                   kernel, mgl.FINALS)
        out["loop.L_sigma2_variance"] = ref["sigma2_variance"]
        # ---- the SVI loop on the same inputs ----
        perm = np.random.default_rng(107).permutation(len(case["coordsB"]))
        ref, kernel2, runs = mgs.run_loop(mc, backend, utils, case, perm)
        assert np.array_equal(kernel2[0], kernel[0])
        chunk, _, _ = mgs.run_loop(mc, backend, utils, case, perm, use_chunk=True, kernel=kernel2)
        f32, _, _ = mgs.run_loop(mc, backend, utils, case, perm, dtype=np.float32, kernel=kernel2)
        pert, _, _ = mgs.run_loop(mc, backend, utils, case, perm, coordsB=XBp, kernel=kernel2)
        g = {q: np.maximum.accumulate(v / mgs.PERTURB) for q, v in mgs.twin_deviation(ref, pert).items()}
        assert all(np.isfinite(v).all() for v in ref.values())
        assert max(float(v.max()) for v in g.values()) <= 100.0, {q: float(v.max()) for q, v in g.items()}
        assert runs >= 8 and np.linalg.norm(ref["R"][-1] - case["R0"]) <= 0.05
        assert np.array_equal(ref["step_size"], np.minimum(1.0, 10.0 / (np.arange(mgs.ITERS) + 1.0)))
        out["svi.cases"], out["svi.iters"], out["svi.arr_iters"] = np.array(["S"]), np.int64(mgs.ITERS), np.array(mgs.ARR_ITERS)
        out["svi.batch_size"] = np.int64(mgs.BATCH)
        out["svi.S_batch_perm"], out["svi.S_step_size"] = perm.astype(np.int16), ref["step_size"]
        out["svi.S_inputs_of"] = np.array("L")
        for q in mgs.SCALARS + mgs.ARRAYS + mgs.FINALS:
            out[f"svi.S_{q}"] = ref[q]
        fl_chunk, fl_f32 = mgs.twin_deviation(ref, chunk), mgs.twin_deviation(ref, f32)
        for q in mgs.SCALARS + mgs.ARRAYS + mgs.FINALS:
            out[f"svi.S_g_{q}"], out[f"svi.S_chunk_{q}"], out[f"svi.S_f32_{q}"] = g[q], fl_chunk[q], fl_f32[q]
        out["svi.S_nonrigid_start_iter"] = np.int64(case["nonrigid_start_iter"])
        print(f"svi.S: sigma2 {ref['sigma2'][0]:.4g} -> {ref['sigma2'][-1]:.4g}, non-rigid in {runs}, max g "
              f"{max(float(v.max()) for v in g.values()):.3g}\n    f32 floor   "
              + ", ".join(f"{q} {fl_f32[q].max():.1e}" for q in mgs.SCALARS + mgs.ARRAYS + mgs.FINALS))


def transfer_tables(utils, backend, out):
    """check_label_transfer on two category lists: the default dictionary, and a given one."""
    import pandas as pd

    def sample(cats):
        return types.SimpleNamespace(obs={"ct": pd.Series(pd.Categorical(cats, categories=cats))})

    catA, catB = ["B cell", "T cell", "mono", "neuron", "stroma"], ["T cell", "astro", "mono", "stroma"]
    nx, type_as = backend.NumpyBackend(), np.zeros(1, dtype=np.float64)
    out["lt_catA"], out["lt_catB"] = np.array(catA), np.array(catB)
    out["lt_default"] = np.asarray(utils.check_label_transfer(nx, type_as, sample(catA), sample(catB), "ct", None), dtype=np.float64)
    given = {ca: {cb: 0.1 * (i + 1) + 0.01 * j for j, cb in enumerate(catB)} for i, ca in enumerate(catA)}
    out["lt_given_values"] = np.array([[given[ca][cb] for cb in catB] for ca in catA])
    out["lt_given"] = np.asarray(utils.check_label_transfer(nx, type_as, sample(catA), sample(catB), "ct", given), dtype=np.float64)
    assert out["lt_default"].shape == (5, 4) and np.array_equal(out["lt_default"], out["lt_default"].astype(np.float32))


def main():
    mc, backend, utils = mge.load_morpho_class()
    rng = np.random.default_rng(20261020)
    kl = ("kl", "gauss", 0.05, mga.counts_layer, 29)
    states = {
        "a": (make_state(rng, 149, 117, 3, 0.07, 0.5, 0.5, [], 5, 4), table(rng, 5, 4)),
        "b": (make_state(rng, 587, 441, 3, 0.05, 0.5, 1.0, [kl], 5, 4), table(rng, 5, 4)),
        "f": (make_state(rng, 601, 463, 2, 0.1, 0.7, 1.0, [("euc", "gauss", 20.0, mga.pca_layer, 30)], 5, 4), table(rng, 5, 4)),
        "z": (make_state(rng, 211, 157, 3, 0.06, 0.5, 1.0, [("kl", "gauss", 0.08, mga.counts_layer, 26)], 6, 5, rare=True),
              table(rng, 6, 5)),
    }
    Tz = states["z"][1]
    Tz[:, 3] = 0.0                    # B label 3: no transfer from any A label
    Tz[:, 4], Tz[5, 4] = 0.0, 0.5     # B label 4 (rare): from the rare A label 5 only
    Tz[5, :3] = [0.0, 0.125, 0.0]     # and a few more exact zeros
    # spec: [(stored layer, metric, probability type, parameter)]
    cases = {
        "a": ("a", [(0, "label", "prob", None)]),
        "b": ("b", [(0, "kl", "gauss", 0.05), (1, "label", "prob", None)]),
        "c": ("b", [(1, "label", "prob", None), (0, "kl", "gauss", 0.05)]),
        "d": ("b", [(0, "kl", "gauss", 0.05), (1, "label", "gauss", 0.25)]),
        "e": ("b", [(0, "kl", "gauss", 0.05), (1, "label", "cos", None)]),
        "f": ("f", [(0, "euc", "gauss", 20.0), (1, "label", "prob", None)]),
        "z": ("z", [(0, "kl", "gauss", 0.08), (1, "label", "prob", None)]),
    }
    out = {"cases": np.array(sorted(cases)), "quantities": np.array(QUANTITIES), "z_ks": np.array(KS)}
    for tag, (st, T) in states.items():
        for k in ("XAHat", "coordsB", "alpha", "SigmaDiag", "sigma2", "gamma", "samples_s", "sigma2_variance", "far"):
            out[f"{tag}_{k}"] = np.asarray(st[k])
        for l, (a, b) in enumerate(zip(st["layers_A"], st["layers_B"])):
            integer = np.issubdtype(a.dtype, np.integer)
            out[f"{tag}_layerA{l}"], out[f"{tag}_layerB{l}"] = (a.astype(np.int16), b.astype(np.int16)) if integer else (a, b)
        out[f"{tag}_label_transfer"] = T
        assert np.array_equal(T, T.astype(np.float32)) and np.array_equal(T * 64, np.round(T * 64))
    for tag, (src, spec) in cases.items():
        st, T = states[src]
        ref, P = run_reference(mc, backend, st, spec, T)
        chunk, _ = run_reference(mc, backend, st, spec, T, use_chunk=True)
        f32, _ = run_reference(mc, backend, st, spec, T, dtype=np.float32)
        assert all(np.isfinite(v).all() for v in ref.values())
        assert np.all(P[:, st["far"]] == 0.0) and len(st["far"]) >= 0.05 * P.shape[1]
        out[f"{tag}_inputs_of"] = np.array(src)
        out[f"{tag}_layer_index"] = np.array([i for i, *_ in spec])
        out[f"{tag}_dissimilarity"] = np.array([m for _, m, _, _ in spec])
        out[f"{tag}_probability_type"] = np.array([p for _, _, p, _ in spec])
        out[f"{tag}_probability_parameters"] = np.array([np.nan if p is None else p for _, _, _, p in spec])
        for q in QUANTITIES:
            out[f"{tag}_{q}"] = ref[q]
        out[f"{tag}_floor_chunk"], out[f"{tag}_floor_f32"] = mga.floors(ref, chunk), mga.floors(ref, f32)
        print(f"case {tag}: {P.shape} {[m for _, m, _, _ in spec]}: Sp {ref['Sp']:.4g}, sigma2_related {ref['sigma2_related']:.4g}\n"
              f"    chunk floor max {out[f'{tag}_floor_chunk'].max():.2e}; f32 floor "
              + ", ".join(f"{q} {v:.1e}" for q, v in zip(QUANTITIES, out[f"{tag}_floor_f32"])))
        if tag == "a":
            out["a_P"] = P
        if tag == "c":   # the order of the layers changes the order of the products only
            assert np.abs(ref["K_NA"] - out["b_K_NA"]).max() <= 1e-13 * ref["K_NA"].max()
        if tag == "z":
            labB = st["layers_B"][1]
            dead, rare = np.nonzero(labB == 3)[0], np.setdiff1d(np.nonzero(labB == 4)[0], st["far"])
            # what the issue states of such columns: S3 = 0, so P = in_j 0 / (0 + 1e-8) = 0 exactly and K_NB = 0
            assert len(dead) and np.all(P[:, dead] == 0.0) and np.all(ref["K_NB"][dead] == 0.0)
            positives = (P[:, rare] > 0).sum(0)
            assert len(rare) and positives.max() < 64 and positives.min() >= 1, positives
            out["z_dead_columns"], out["z_rare_columns"] = dead, rare
            for k in KS:
                rk, Pk = run_reference(mc, backend, st, spec, T, k=k)
                ck, _ = run_reference(mc, backend, st, spec, T, k=k, use_chunk=True)
                fk, _ = run_reference(mc, backend, st, spec, T, k=k, dtype=np.float32)
                NA, NB = P.shape
                assert len(Pk.data) == k * NB and np.array_equal(Pk.col, np.repeat(np.arange(NB), k))
                mask = np.zeros_like(P, dtype=bool)
                mask[np.asarray(Pk.row), np.asarray(Pk.col)] = True
                masked = np.where(mask, P, 0.0)
                assert np.abs(masked.sum(1) - rk["K_NA"]).max() <= 1e-14 * rk["K_NA"].max()
                gap = column_gaps(P, k)
                live = gap[gap > 0]
                assert live.min() >= 1e-7, (k, live.min())   # (make_golden_assign_topk.MIN_GAP)
                # the columns a float32 comparison of the selected SETS leaves out (tests/_assign_topk_case.check: at most 5 %)
                left_out = float(((gap <= 1e-2) & P.any(0)).mean())
                assert left_out < 0.05, (k, left_out)
                key = f"z_k{k}"
                for q in QUANTITIES:
                    out[f"{key}_{q}"] = rk[q]
                out[f"{key}_row"], out[f"{key}_data"] = np.asarray(Pk.row, dtype=np.int16), np.asarray(Pk.data, dtype=np.float64)
                out[f"{key}_floor_chunk"], out[f"{key}_floor_f32"] = mga.floors(rk, ck), mga.floors(rk, fk)
                out[f"{key}_colgap"] = gap
                print(f"    k {k}: Sp {rk['Sp']:.4g}, columns with a zero gap {int((gap == 0).sum())} of {NB}, smallest other gap "
                      f"{live.min():.2e}, left out at 1e-2 {left_out:.3f}; f32 floor max {out[f'{key}_floor_f32'].max():.1e}")
    transfer_tables(utils, backend, out)
    loops(mc, backend, utils, out)
    path = os.path.join(HERE, "ref_assign_label.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
