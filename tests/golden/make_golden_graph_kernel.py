#!/usr/bin/env python
"""Golden vectors that pin the GEODESIC KERNEL of Spateo's pairwise alignment to real reference code.

    spateo/alignment/methods/utils.py:1161-1188   construct_knn_graph      :1191-1217   con_K_graph
    spateo/alignment/methods/morpho_class.py:865-871   the kernel_type="geodist" branch of _construct_kernel

This script EXECUTES those functions (through ``make_golden_em.load_morpho_class()``) and stores inputs and outputs in
``tests/golden/ref_graph_kernel.npz`` (data only).

Graph cases (``graph_cases``): ``g2`` / ``g3`` (about 300 random points in the plane / in space), ``blobs`` (two well-separated
blobs: two components, so ``D`` keeps 1e5 across them) and ``dups`` (a cloud with 5 duplicated points: a neighbour at distance 0
takes a slot of the list and adds no edge).  Per case: the points, ``knn``; sklearn's neighbour lists (``kneighbors_graph``, the
columns of every row in ascending order, with their distances); the edges of the reference's graph (i < j, weight), sorted; 8
inducing indices, ``beta``, the reference's ``K`` and the ``D`` under it - ``con_K_graph`` returns ``K`` only, so ``D`` is formed here
by the statements of its loop (``networkx.single_source_dijkstra`` per inducing variable, 1e5 where a node has no entry) and
``exp(-beta * D**2)`` is asserted equal to the reference's ``K`` bit for bit.  n > 2 knn + 1 (sklearn's KD-tree, not its brute-force
branch) and random coordinates (no ties at the k-th distance) throughout.

Loop cases (``cases``): ``L3`` (3-D, 607 / 451 cells, 40 inducing variables, beta = 0.5, graph_knn = 10) and ``L2`` (2-D, 16 inducing
variables, beta = 1.0), the real loop methods driven by ``make_golden_align_loop.run_loop(..., kernel=(inducing, Gamma, U))`` with
the triple from the real ``_construct_kernel`` (``kernel_type="geodist"``), stored the way ``ref_align_loop.npz`` stores its cases
(per iteration scalars, the cell-sized arrays at ``arr_iters``, the ``chunk`` / ``f32`` floors and the amplification ``g`` of a 1e-10
perturbation of ``coordsB``), plus ``inducing_idx``, ``graph_knn``, every 16th row of the reference's ``U`` and, for ``L3``, the
inputs and results of the loop's first ``_update_nonrigid`` call (``first_*``).  The SVI twin through
``make_golden_align_svi.run_loop(..., kernel=...)`` under the prefix ``svi_`` (its own ``iters``, ``arr_iters``, ``batch_size``) is
of ``L2``: on ``L3`` the reference's own SVI run amplifies the 1e-10 perturbation by 1.3e4 (two batch permutations tried: 1.3e4 and
1.9e5; ``pinv``'s cut-off moves), and a comparison at 1e-10 would mean nothing there; ``L2``'s gain is 5.

The maker asserts what keeps the file meaningful and fails instead of writing a weak one: every gain <= 100, at least 8
non-rigid updates, the final R within 0.15 (Frobenius) of the rotation put in, max |U_geodist - U_euc| >= 0.1, the loop graph
connected, every node of every graph with an edge, every value finite, the file below 1 MB.

    python tests/golden/make_golden_graph_kernel.py
"""
from __future__ import annotations

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

M_GRAPH = 8
SEED_KERNEL = 17
SVI_TWIN = "L2"


def graph_case(utils, X, knn, idx, beta):
    import networkx
    from sklearn.neighbors import kneighbors_graph

    n = len(X)
    assert n > 2 * knn + 1
    A = kneighbors_graph(X, knn, mode="distance", include_self=False)
    assert A.nnz == n * knn
    cols, vals = A.indices.reshape(n, knn), A.data.reshape(n, knn)
    order = np.argsort(cols, axis=1)
    graph = utils.construct_knn_graph(X, knn)
    assert graph.number_of_nodes() == n and sorted(graph.nodes) == list(range(n))
    edges = np.array(sorted((min(i, j), max(i, j), w) for i, j, w in graph.edges(data="weight")))
    K = np.asarray(utils.con_K_graph(graph, np.asarray(idx), beta=beta), dtype=np.float64)
    D = 1e5 * np.ones((n, len(idx)))
    for i in range(len(idx)):
        distance, _ = networkx.single_source_dijkstra(graph, source=int(idx[i]), weight="weight")
        for j in range(n):
            if j in distance:
                D[j, i] = distance[j]
    assert np.array_equal(np.exp(-beta * D**2), K)
    return dict(points=X, knn=np.int64(knn), nbr_idx=np.take_along_axis(cols, order, 1).astype(np.int32),
                nbr_dist=np.take_along_axis(vals, order, 1), edges_ij=edges[:, :2].astype(np.int32), edges_w=edges[:, 2].copy(),
                inducing_idx=np.asarray(idx, dtype=np.int64), beta=np.float64(beta), K=K, D=D,
                components=np.int64(networkx.number_connected_components(graph)))


def geodesic_kernel(mc, backend, case, graph_knn):
    """(inducing_idx, (inducing_variables, GammaSparse, U)) from the real _construct_kernel with kernel_type="geodist", and the
    Euclidean U of the same inducing variables."""
    import networkx

    XA = case["coordsA"]
    s = types.SimpleNamespace(nx=backend.NumpyBackend(), coordsA=XA, kernel_type="geodist", kernel_bandwidth=case["beta"],
                              guidance_effect=False, X_AI=None, graph=None, graph_knn=graph_knn)
    np.random.seed(SEED_KERNEL)   # _construct_kernel draws the inducing variables from NumPy's global RNG
    mc.Morpho_pairwise._construct_kernel(s, case["n_ctrl"], None)
    np.random.seed(SEED_KERNEL)   # the same draw again, for the indices it does not keep
    uniq, first = np.unique(XA, return_index=True, axis=0)
    idx = first[np.random.choice(len(uniq), case["n_ctrl"], replace=False)]
    assert np.array_equal(XA[idx], s.inducing_variables) and np.array_equal(s.GammaSparse, s.U[idx])
    assert s.graph.number_of_nodes() == len(XA) and networkx.is_connected(s.graph)
    e = types.SimpleNamespace(nx=s.nx, coordsA=XA, kernel_type="euc", kernel_bandwidth=case["beta"], guidance_effect=False,
                              X_AI=None, graph=None)
    np.random.seed(SEED_KERNEL)
    mc.Morpho_pairwise._construct_kernel(e, case["n_ctrl"], None)
    assert np.array_equal(e.inducing_variables, s.inducing_variables)
    return idx, (s.inducing_variables, s.GammaSparse, s.U), float(np.abs(s.U - e.U).max())


def main():
    mc, backend, utils = mge.load_morpho_class()
    rng = np.random.default_rng(20261021)
    out = {}
    # ---- graph cases ----
    blobs = np.concatenate([rng.standard_normal((170, 2)), [40.0, 0.0] + rng.standard_normal((140, 2))])
    base = rng.random((300, 3)) * [2.0, 1.0, 1.0]
    drng = np.random.default_rng(5)   # (a stream of its own: the cases behind this one keep their draws)
    for attempt in range(4096):
        # 5 duplicated points (one of them three times over).  A point and its copy are equally far from everything else: the draw
        # is repeated until no row has that tie across its knn-th slot, where sklearn's choice is unspecified (ours: the smaller index)
        dups = base.copy()
        a, b, c = drng.choice(300, 3, replace=False)
        copies = drng.choice(np.setdiff1d(np.arange(300), [a, b, c]), 5, replace=False)
        dups[copies] = dups[[a, a, b, b, c]]
        d = np.sort(np.sqrt(((dups[:, None, :] - dups[None, :, :]) ** 2).sum(-1)), axis=1)   # (column 0: the point itself)
        if (d[:, 8] < d[:, 9]).all():
            break
    else:
        raise AssertionError("no tie-free draw of the duplicates")
    dup_sources = (int(a), int(copies[0]))
    graphs = {"g2": (rng.random((307, 2)), 10, 0.5), "g3": (rng.standard_normal((293, 3)), 10, 0.3), "blobs": (blobs, 6, 0.05),
              "dups": (dups, 8, 2.0)}
    out["graph_cases"] = np.array(list(graphs))
    for tag, (X, knn, beta) in graphs.items():
        idx = rng.choice(len(X), M_GRAPH, replace=False)
        if tag == "dups":
            idx = np.concatenate([dup_sources, np.setdiff1d(idx, dup_sources)[: M_GRAPH - 2]])   # a duplicated point and its copy as sources
        c = graph_case(utils, X, knn, idx, beta)
        assert all(np.isfinite(v).all() for v in c.values())
        if tag == "blobs":
            assert c["components"] == 2 and (c["D"] == 1e5).any() and (c["K"] == 0).any()
        if tag == "dups":
            assert (c["nbr_dist"] == 0).sum() >= 5
        for k, v in c.items():
            out[f"{tag}_{k}"] = v
        print(f"graph case {tag}: n {len(X)}, knn {knn}, edges {len(c['edges_w'])}, components {int(c['components'])}, "
              f"zero-distance neighbours {int((c['nbr_dist'] == 0).sum())}, unreachable entries {int((c['D'] == 1e5).sum())}")
    # ---- loop cases ----
    kl = ("kl", "gauss", 0.1, mga.counts_layer, 40)
    cases = {"L3": mgl.make_case(rng, 607, 451, 3, [kl], 0.45),
             "L2": mgl.make_case(rng, 607, 451, 2, [("euc", "gauss", 20.0, mga.pca_layer, 30)], 0.4, n_ctrl=16, beta=1.0)}
    out.update({"cases": np.array(list(cases)), "iters": np.int64(mgl.ITERS), "arr_iters": np.array(mgl.ARR_ITERS),
                "scalars": np.array(mgl.SCALARS), "arrays": np.array(mgl.ARRAYS), "finals": np.array(mgl.FINALS),
                "svi_cases": np.array([SVI_TWIN]), "svi_iters": np.int64(mgs.ITERS), "svi_arr_iters": np.array(mgs.ARR_ITERS),
                "svi_batch_size": np.int64(mgs.BATCH), "svi_finals": np.array(mgs.FINALS)})
    graph_knn = 10
    for tag, case in cases.items():
        XA, XB = case["coordsA"], case["coordsB"]
        case["samples_s"] = float(max(np.prod(XA.max(0) - XA.min(0)), np.prod(XB.max(0) - XB.min(0))))   # :738-741
        idx, kernel, u_gap = geodesic_kernel(mc, backend, case, graph_knn)
        assert u_gap >= 0.1, (tag, u_gap)
        first = {}
        real_update = mc.Morpho_pairwise._update_nonrigid

        def spy(self_):   # the first non-rigid step of the loop, for update_nonrigid(graph_kernel=): its inputs and its results
            if first:
                return real_update(self_)
            first["sigma2"] = np.float64(self_.sigma2)
            real_update(self_)
            first.update(K_NA=np.array(self_.K_NA), PXB_term=np.array(self_.PXB_term), Coff=np.array(self_.Coff),
                         VnA=np.array(self_.VnA), SigmaDiag=np.array(self_.SigmaDiag))

        mc.Morpho_pairwise._update_nonrigid = spy
        try:
            ref, s, _, info = mgl.run_loop(mc, backend, utils, case, kernel=kernel)
        finally:
            mc.Morpho_pairwise._update_nonrigid = real_update
        if tag == "L3":
            for k, v in first.items():
                out[f"{tag}_first_{k}"] = v
        chunk, _, _, _ = mgl.run_loop(mc, backend, utils, case, use_chunk=True, kernel=kernel)
        f32, _, _, _ = mgl.run_loop(mc, backend, utils, case, dtype=np.float32, kernel=kernel)
        prng = np.random.default_rng(len(tag) + int(tag[1]))
        XBp = XB * (1.0 + mgl.PERTURB * prng.standard_normal(XB.shape))
        pert, _, _, _ = mgl.run_loop(mc, backend, utils, case, coordsB=XBp, kernel=kernel)
        g = {q: np.maximum.accumulate(v / mgl.PERTURB) for q, v in mgl.twin_deviation(ref, pert).items()}
        fl_chunk, fl_f32 = mgl.twin_deviation(ref, chunk), mgl.twin_deviation(ref, f32)
        assert all(np.isfinite(v).all() for v in ref.values()), tag
        gmax = max(float(v.max()) for v in g.values())
        r_off = float(np.linalg.norm(ref["R"][-1] - case["R0"]))
        assert gmax <= 100.0, (tag, {q: float(v.max()) for q, v in g.items()})
        assert info["nonrigid_runs"] >= 8, (tag, info)
        assert r_off <= 0.15, (tag, r_off)
        out[f"{tag}_sigma2_init"] = np.float64(case["sigma2"])
        for k in ("coordsA", "coordsB", "samples_s", "origin", "beta", "lambdaVF", "nonrigid_start_iter", "partial_robust_level",
                  "nn_init_weight", "kappa", "gamma_a", "gamma_b", "R0", "t0"):
            out[f"{tag}_{k}"] = np.asarray(case[k])
        out[f"{tag}_inducing_variables"], out[f"{tag}_inducing_idx"] = np.asarray(kernel[0]), idx.astype(np.int64)
        out[f"{tag}_graph_knn"], out[f"{tag}_U_gap"] = np.int64(graph_knn), np.float64(u_gap)
        out[f"{tag}_U_sample"] = np.asarray(kernel[2])[::16].copy()   # every 16th row of the reference's U
        for l, (a, b) in enumerate(zip(case["exp_layers_A"], case["exp_layers_B"])):
            out[f"{tag}_layerA{l}"], out[f"{tag}_layerB{l}"] = a, b
        out[f"{tag}_dissimilarity"] = np.array(case["dissimilarity"])
        out[f"{tag}_probability_type"] = np.array(case["probability_type"])
        out[f"{tag}_probability_parameters"] = np.array([np.nan if p is None else p for p in case["probability_parameters"]])
        for q in mgl.SCALARS + mgl.ARRAYS + mgl.FINALS:
            out[f"{tag}_{q}"] = ref[q]
            out[f"{tag}_g_{q}"], out[f"{tag}_chunk_{q}"], out[f"{tag}_f32_{q}"] = g[q], fl_chunk[q], fl_f32[q]
        out[f"{tag}_sigma2_variance"] = ref["sigma2_variance"]
        out[f"{tag}_nonrigid_runs"] = np.int64(info["nonrigid_runs"])
        print(f"loop case {tag}: |U_geodist - U_euc| {u_gap:.3g}, |R - R0| {r_off:.3g}, non-rigid in {info['nonrigid_runs']}, max g {gmax:.3g}\n"
              "    f32 floor   " + ", ".join(f"{q} {fl_f32[q].max():.1e}" for q in mgl.SCALARS + mgl.ARRAYS + mgl.FINALS) + "\n"
              "    g           " + ", ".join(f"{q} {g[q].max():.2g}" for q in mgl.SCALARS + mgl.ARRAYS + mgl.FINALS))
        if tag != SVI_TWIN:
            continue
        # ---- the SVI twin ----
        perm = np.random.default_rng(103).permutation(len(XB))
        sref, _, runs = mgs.run_loop(mc, backend, utils, case, perm, kernel=kernel)
        schunk, _, _ = mgs.run_loop(mc, backend, utils, case, perm, use_chunk=True, kernel=kernel)
        sf32, _, _ = mgs.run_loop(mc, backend, utils, case, perm, dtype=np.float32, kernel=kernel)
        spert, _, _ = mgs.run_loop(mc, backend, utils, case, perm, coordsB=XBp, kernel=kernel)
        sg = {q: np.maximum.accumulate(v / mgs.PERTURB) for q, v in mgs.twin_deviation(sref, spert).items()}
        sfl_chunk, sfl_f32 = mgs.twin_deviation(sref, schunk), mgs.twin_deviation(sref, sf32)
        sgmax = max(float(v.max()) for v in sg.values())
        s_off = float(np.linalg.norm(sref["R"][-1] - case["R0"]))
        assert all(np.isfinite(v).all() for v in sref.values())
        assert sgmax <= 100.0, {q: float(v.max()) for q, v in sg.items()}
        assert runs >= 8 and s_off <= 0.15, (runs, s_off)
        out[f"svi_{tag}_batch_perm"] = perm.astype(np.int16)
        out[f"svi_{tag}_step_size"] = sref["step_size"]
        out[f"svi_{tag}_nonrigid_runs"] = np.int64(runs)
        for q in mgs.SCALARS + mgs.ARRAYS + mgs.FINALS:
            out[f"svi_{tag}_{q}"] = sref[q]
            out[f"svi_{tag}_g_{q}"], out[f"svi_{tag}_chunk_{q}"], out[f"svi_{tag}_f32_{q}"] = sg[q], sfl_chunk[q], sfl_f32[q]
        print(f"SVI twin of {tag}: |R - R0| {s_off:.3g}, non-rigid in {runs}, max g {sgmax:.3g}")
    path = os.path.join(HERE, "ref_graph_kernel.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
