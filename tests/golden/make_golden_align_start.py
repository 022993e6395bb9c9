#!/usr/bin/env python
"""Golden vectors that pin the START STATE of Spateo's pairwise alignment - what ``Morpho_pairwise`` computes in front of its
loop - to real reference code.

    spateo/alignment/methods/utils.py:1339-1354          _init_guess_sigma2
    spateo/alignment/methods/morpho_class.py:771-820     Morpho_pairwise._init_probability_parameters
    spateo/alignment/methods/morpho_class.py:898-1041    Morpho_pairwise._coarse_rigid_alignment
    spateo/alignment/methods/utils.py:1220-1280, 1283-1336   inlier_from_NN, voxel_data (called by it)

This script EXECUTES those functions (the methods unbound, on a ``SimpleNamespace`` self, NumPy backend) in the reference's
order - coarse alignment, then sigma2 and the parameters on the transformed coordinates - and stores inputs and outputs in
``tests/golden/ref_align_start.npz``; ``spateo_amd.align.init_sigma2`` / ``init_probability_parameters`` /
``coarse_rigid_alignment`` / ``morpho_start`` and the NumPy restatement of ``tests/_align_start_case.py`` are checked against
them.  ``get_rep`` is replaced by a function that returns the arrays (AnnData is not installed here).  ``subsample`` /
``n_sampling`` are small, so that the branch that draws runs; the drawn indices are recorded by seeding ``np.random`` and
repeating the draws.  ``voxel_data`` and ``inlier_from_NN`` are wrapped to record the voxels and the matched pairs.

Cases (about 600 x 450 cells, expression a smooth function of position, A a rotated and shifted copy of B's positions):

1. 3-D, one ``kl`` layer, subsample smaller than both sides;
2. 2-D, ``euc`` (``None``; the coarse alignment's layer) + ``cos`` (parameter given) layers, NA != NB, no subsampling: the ``nA nA`` denominator shows;
3. 3-D with ``allow_flip=True`` and a mirrored A;
4. 2-D, two ``kl`` layers, the second of nearly equal profiles: its estimate lands on the 0.01 floor.

Two twins of the reference itself per case, relative to each quantity's maximum: ``f32`` - the float32 NumPy backend (every input
float32) - and a float64 run with the inputs perturbed
at 1e-10 relative, whose deviation divided by 1e-10 is the amplification ``g`` of the quantity.

The maker fails instead of writing a weak file: every estimated parameter except case 4's above the floor; in every
top-K list the K-th and (K+1)-th distance more than 1e-8 (relative) apart; no point within 1e-9 (relative) of a voxel's
mask boundary; no ``P[:, 0]`` within 1e-6 of the inlier threshold; g <= 100 for every stored quantity; the twins keep the
inlier pairs; case 3 takes the flip branch; the fitted R within 0.05 (Frobenius) of the rotation put in.

The layers are kept on coarse grids (counts; multiples of 1/32) so that the file stays small once compressed.

    python tests/golden/make_golden_align_start.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_align_loop as mgl  # noqa: E402
import make_golden_em as mge  # noqa: E402

QUANTITIES = ("sigma2", "parameters", "init_R", "init_t", "inlier_A", "inlier_B", "inlier_P", "coordsA")
PERTURB = 1e-10


def counts(rng, Z, centres, level=12.0):
    """Count-like expression whose profile is a smooth function of the position: feature g peaks at centres[g]."""
    d2 = ((Z[:, None, :] - centres[None, :, :]) ** 2).sum(-1)
    return rng.poisson(level * np.exp(-d2 / 3.0) + 0.3).astype(np.float64)


def smooth(rng, Z, centres, noise=0.1):
    """PCA-like representation on the 1/32 grid, smooth in the position."""
    d2 = ((Z[:, None, :] - centres[None, :, :]) ** 2).sum(-1)
    return np.round((2.0 * np.exp(-d2 / 4.0) - 0.5 + noise * rng.standard_normal(d2.shape)) * 32) / 32


def lattice(rng, n, D, side=3.4):
    """n points of a jittered regular lattice in a cube: an even density up to the faces, so that neighbouring voxels do not
    hold the same points (equal voxel means would tie in the nearest-neighbour lists)."""
    m = int(np.ceil(n ** (1.0 / D)))
    nodes = np.stack(np.meshgrid(*[np.arange(m)] * D, indexing="ij"), axis=-1).reshape(-1, D).astype(np.float64)
    nodes = nodes[rng.permutation(len(nodes))[:n]]
    return ((nodes + 0.5 + 0.3 * rng.uniform(-1, 1, nodes.shape)) / m - 0.5) * side


def make_case(rng, NA, NB, D, layers, subsample, top_K=10, allow_flip=False, mirror=False):
    """layers: [(metric, probability type, parameter or None, maker, G)]; the first layer is the coarse alignment's."""
    Z = lattice(rng, NA, D)
    src = rng.choice(NA, NB, replace=NB > NA)
    ZB = Z[src] + 0.03 * rng.standard_normal((NB, D))
    R0, t0 = mgl.rotation(D, 0.35), 0.3 + 0.2 * rng.random(D)
    XA = (Z - t0) @ R0                                  # XA R0^T + t0 = Z
    if mirror:
        F = np.eye(D)
        F[-1, -1] = -1
        XA, R0 = XA @ F, R0 @ F                         # (XA F) (R0 F)^T + t0 = Z: the fit must mirror
    LA, LB = [], []
    for (_, _, _, maker, G) in layers:
        centres = rng.standard_normal((G, D)) * 1.5
        LA.append(maker(rng, Z, centres))
        LB.append(maker(rng, ZB, centres))
    return dict(coordsA=XA, coordsB=ZB, exp_layers_A=LA, exp_layers_B=LB, R0=R0, t0=t0, dissimilarity=[l[0] for l in layers],
                probability_type=[l[1] for l in layers], probability_parameters=[l[2] for l in layers], subsample=subsample,
                top_K=top_K, allow_flip=allow_flip, init_metric="kl" if layers[0][0] == "kl" else "euc")


def draws(seed, NA, NB, n):
    """The indices the reference draws after np.random.seed(seed): A first, then B (utils.py:1346-1347, morpho_class.py:806-811,
    922-927)."""
    np.random.seed(seed)
    iA = np.random.choice(NA, n, replace=False) if NA > n else np.arange(NA)
    iB = np.random.choice(NB, n, replace=False) if NB > n else np.arange(NB)
    return iA, iB


def run_reference(mc, backend, utils, case, seed, f32=False, perturb=None):
    """The reference's start state for one case.  f32: the float32 NumPy backend (every input float32); perturb: a Generator
    whose 1e-10 relative noise multiplies every input."""
    nx = backend.NumpyBackend()
    XA, XB = case["coordsA"].copy(), case["coordsB"].copy()
    LA, LB = [a.copy() for a in case["exp_layers_A"]], [b.copy() for b in case["exp_layers_B"]]
    if perturb is not None:
        p = lambda a: a * (1.0 + PERTURB * perturb.standard_normal(a.shape))  # noqa: E731
        XA, XB, LA, LB = p(XA), p(XB), [p(a) for a in LA], [p(b) for b in LB]
    dtype = np.float32 if f32 else np.float64
    XA, XB, LA, LB = XA.astype(dtype), XB.astype(dtype), [a.astype(dtype) for a in LA], [b.astype(dtype) for b in LB]
    NA, NB, n = len(XA), len(XB), case["subsample"]
    rec = {}
    real_dist, real_voxel, real_inlier = utils.calc_distance, utils.voxel_data, utils.inlier_from_NN

    def calc_distance(X, Y, metric="euc", **kw):
        return real_dist(X=X, Y=Y, metric=metric, **kw)

    def voxel_data(**kw):
        out = real_voxel(**kw)
        rec.setdefault("voxels", []).append((out, kw["coords"].copy(), kw["voxel_num"]))
        return out

    def inlier_from_NN(x, y, d):
        out = real_inlier(x, y, d)
        rec.setdefault("fits", []).append((x.copy(), y.copy(), d.copy(), out))
        return out

    def matrix_spy(X, Y, metric="euc", **kw):
        out = calc_distance(X, Y, metric, **kw)
        rec["exp_dist"] = out[0]
        return out

    s = types.SimpleNamespace(nx=nx, type_as=np.zeros(1, dtype=dtype), verbose=False, NA=NA, NB=NB, coordsA=XA, coordsB=XB, sampleA=LA[0],
                              sampleB=LB[0], init_layer="X", init_field="layer" if case["init_metric"] == "kl" else "X_pca",
                              genes=None, nn_init_top_K=case["top_K"], allow_flip=case["allow_flip"], init_transform=True,
                              exp_layers_A=LA, exp_layers_B=LB, dissimilarity=case["dissimilarity"],
                              probability_type=case["probability_type"], probability_parameters=list(case["probability_parameters"]))
    saved = (mc.get_rep, mc.calc_distance, mc.voxel_data, mc.inlier_from_NN, utils.calc_distance)
    mc.get_rep = lambda nx, type_as, sample, rep, rep_field, genes: sample
    mc.calc_distance, mc.voxel_data, mc.inlier_from_NN = matrix_spy, voxel_data, inlier_from_NN
    utils.calc_distance = calc_distance
    try:
        np.random.seed(seed)
        mc.Morpho_pairwise._coarse_rigid_alignment(s, n_sampling=n)
        mc.calc_distance = calc_distance
        np.random.seed(seed)
        sigma2 = utils._init_guess_sigma2(s.coordsA, s.coordsB, subsample=n)
        np.random.seed(seed)
        mc.Morpho_pairwise._init_probability_parameters(s, subsample=n)
    finally:
        mc.get_rep, mc.calc_distance, mc.voxel_data, mc.inlier_from_NN, utils.calc_distance = saved
    (vA, gA), cA, _ = rec["voxels"][0]
    (vB, gB), cB, _ = rec["voxels"][1]
    x, y, dist, fit = rec["fits"][0]
    flipped = False
    if case["allow_flip"]:
        flipped = bool(rec["fits"][1][3][5] > fit[5])
        if flipped:
            fit = rec["fits"][1][3]
    P = fit[0]
    # the pairs as voxel indices: every row of train_x / train_y is a row of the voxel arrays
    look = lambda v, rows: np.array([int(np.flatnonzero((v == r).all(1))[0]) for r in rows])  # noqa: E731
    NN = np.stack([look(vB, y), look(vA, x)], axis=1)
    threshold = min(P[np.argsort(-P[:, 0])[20], 0], 0.5)
    keep = np.where(P[:, 0] > threshold)[0]
    assert f32 or np.array_equal(np.asarray(s.inlier_B), y[keep]) and np.array_equal(np.asarray(s.inlier_P), P[keep])
    out = dict(sigma2=np.float64(sigma2), parameters=np.array([np.nan if p is None else p for p in s.probability_parameters],
                                                              dtype=np.float64),
               init_R=np.asarray(s.init_R, dtype=np.float64), init_t=np.asarray(s.init_t, dtype=np.float64).reshape(-1),
               inlier_A=np.asarray(s.inlier_A, dtype=np.float64), inlier_B=np.asarray(s.inlier_B, dtype=np.float64),
               inlier_P=np.asarray(s.inlier_P, dtype=np.float64), coordsA=np.asarray(s.coordsA, dtype=np.float64),
               inlier_pairs=NN[keep])
    info = dict(flipped=flipped, exp_dist=rec["exp_dist"], P=P, threshold=threshold, voxels=rec["voxels"], n_pairs=len(x),
                n_voxels=(len(vA), len(vB)))
    return out, info


def ordered(out):
    order = np.lexsort((out["inlier_pairs"][:, 1], out["inlier_pairs"][:, 0]))
    return dict(out, inlier_pairs=out["inlier_pairs"][order], inlier_A=out["inlier_A"][order], inlier_B=out["inlier_B"][order],
                inlier_P=out["inlier_P"][order])


def deviation(ref, other):
    a, b = ordered(ref), ordered(other)
    assert np.array_equal(a["inlier_pairs"], b["inlier_pairs"]), "a twin changed the inlier pairs"
    return {q: float(np.abs(np.nan_to_num(b[q]) - np.nan_to_num(a[q])).max() / np.abs(np.nan_to_num(a[q])).max()) for q in QUANTITIES}


def main():
    mc, backend, utils = mge.load_morpho_class()
    rng = np.random.default_rng(20261018)
    cases = {
        "1": make_case(rng, 607, 451, 3, [("kl", "gauss", None, counts, 24)], subsample=400),
        "2": make_case(rng, 593, 447, 2, [("euc", "gauss", None, smooth, 12), ("cos", "cos", 0.3, smooth, 10)], subsample=20000),
        "3": make_case(rng, 611, 443, 3, [("kl", "gauss", None, counts, 24)], subsample=420, allow_flip=True, mirror=True),
        "4": make_case(rng, 450, 380, 2, [("kl", "gauss", None, counts, 16)], subsample=20000),
    }
    # case 4: a second layer of nearly equal profiles, whose estimate lands on the floor
    c4 = cases["4"]
    c4["exp_layers_A"].append(np.full((450, 8), 40.0) + rng.poisson(1.0, (450, 8)))
    c4["exp_layers_B"].append(np.full((380, 8), 40.0) + rng.poisson(1.0, (380, 8)))
    c4["dissimilarity"].append("kl"), c4["probability_type"].append("gauss"), c4["probability_parameters"].append(None)
    out = {"cases": np.array(sorted(cases)), "quantities": np.array(QUANTITIES)}
    for tag, case in cases.items():
        seed = 100 + int(tag)
        ref, info = run_reference(mc, backend, utils, case, seed)
        f32, _ = run_reference(mc, backend, utils, case, seed, f32=True)
        pert, _ = run_reference(mc, backend, utils, case, seed, perturb=np.random.default_rng(int(tag)))
        fl_f32 = deviation(ref, f32)
        g = {q: v / PERTURB for q, v in deviation(ref, pert).items()}
        iA, iB = draws(seed, len(case["coordsA"]), len(case["coordsB"]), case["subsample"])
        # ---- the conditions that keep the comparison meaningful ----
        est = [l for l, p in enumerate(case["probability_parameters"]) if p is None]
        for l in est:
            on_floor = ref["parameters"][l] == 0.01
            assert on_floor == (tag == "4" and l == 1), (tag, l, ref["parameters"])
        d = info["exp_dist"]
        K = case["top_K"]
        assert K < min(d.shape) - 1
        for m in (d, d.T):
            srt = np.sort(m, axis=0)
            assert np.all(srt[K] - srt[K - 1] > 1e-8 * np.abs(d).max()), (tag, "a K-th and (K+1)-th distance too close")
        for (_, coords, voxel_num) in info["voxels"]:
            lo, hi = coords.min(0), coords.max(0)
            size = np.sqrt(np.prod(hi - lo)) / (np.sqrt(len(coords)) / 5)
            nodes = np.stack(np.meshgrid(*[np.arange(a, b, st) for a, b, st in zip(lo, hi, (hi - lo) / int(np.sqrt(voxel_num)))]),
                             axis=-1).reshape(-1, coords.shape[1])
            dist = np.sqrt(((coords[None] - nodes[:, None]) ** 2).sum(-1))
            assert np.abs(dist - size / 2).min() > 1e-9 * size, (tag, "a point on a voxel's mask boundary")
        assert np.abs(info["P"][:, 0] - info["threshold"])[info["P"][:, 0] != info["threshold"]].min() > 1e-6, tag
        assert info["threshold"] == 0.5 or np.sum(info["P"][:, 0] == info["threshold"]) == 1, tag
        assert max(g.values()) <= 100.0, (tag, g)
        assert info["flipped"] == (tag == "3"), (tag, info["flipped"])
        assert np.linalg.norm(ref["init_R"] - case["R0"]) <= 0.05, (tag, ref["init_R"], case["R0"])
        assert info["n_pairs"] >= 22 and all(np.isfinite(np.nan_to_num(v)).all() for v in ref.values())
        # ---- store ----
        for l, (a, b) in enumerate(zip(case["exp_layers_A"], case["exp_layers_B"])):
            out[f"{tag}_layerA{l}"], out[f"{tag}_layerB{l}"] = a, b
        out[f"{tag}_coordsA_in"], out[f"{tag}_coordsB"] = case["coordsA"], case["coordsB"]
        out[f"{tag}_R0"], out[f"{tag}_t0"] = case["R0"], case["t0"]
        out[f"{tag}_dissimilarity"] = np.array(case["dissimilarity"])
        out[f"{tag}_probability_type"] = np.array(case["probability_type"])
        out[f"{tag}_probability_parameters_in"] = np.array([np.nan if p is None else p for p in case["probability_parameters"]])
        out[f"{tag}_subsample_A"], out[f"{tag}_subsample_B"] = iA, iB
        out[f"{tag}_init_metric"], out[f"{tag}_top_K"] = np.array(case["init_metric"]), np.int64(K)
        out[f"{tag}_allow_flip"], out[f"{tag}_flipped"] = np.bool_(case["allow_flip"]), np.bool_(info["flipped"])
        out[f"{tag}_inlier_pairs"] = ref["inlier_pairs"]
        for q in QUANTITIES:
            out[f"{tag}_{q}"], out[f"{tag}_g_{q}"], out[f"{tag}_f32_{q}"] = ref[q], np.float64(g[q]), np.float64(fl_f32[q])
        print(f"case {tag}: voxels {info['n_voxels']}, pairs {info['n_pairs']}, inliers {len(ref['inlier_pairs'])}, sigma2 "
              f"{float(ref['sigma2']):.4g}, parameters {ref['parameters']}, |R - R0| {np.linalg.norm(ref['init_R'] - case['R0']):.3g}, "
              f"flipped {info['flipped']}\n    f32 floor " + ", ".join(f"{q} {fl_f32[q]:.1e}" for q in QUANTITIES) + "\n    g         "
              + ", ".join(f"{q} {g[q]:.2g}" for q in QUANTITIES))
    path = os.path.join(HERE, "ref_align_start.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
