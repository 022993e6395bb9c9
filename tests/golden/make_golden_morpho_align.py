#!/usr/bin/env python
"""Golden vectors that pin ``spateo_amd.align.Morpho_pairwise`` / ``morpho_align`` to the real reference CLASS, AnnData in and
AnnData out.

    spateo/alignment/methods/morpho_class.py:110-313      Morpho_pairwise.__init__ and run()
    :316-441 _check   :443-558 _align_preprocess   :589-680 _normalize_coords / _normalize_exps   :1471-1528 _wrap_output
    spateo/alignment/morpho_alignment.py:22-111           morpho_align (its loop, restated here around the real class: the
                                                          module itself imports more of the package than the stubs carry)

This script EXECUTES the real constructor and ``run()`` (NumPy backend) on small stand-in samples of its own - ``.X`` (CSR
counts), ``.var`` / ``.obs`` (pandas, with a categorical column), ``.obsm``, ``.layers``, ``.uns``, ``sample[:, genes]``,
``sample[rows]``, ``.copy()`` - and stores inputs and outputs in ``tests/golden/ref_morpho_align.npz``.  What the reference
draws from ``np.random`` (inducing variables, ``batch_perm``) is recorded by wrapping ``np.random.choice`` /
``np.random.permutation``; its ``genes`` order (a ``set``'s) is recorded too.  The tests hand both back through the pinning
arguments and ``genes=``.

Cases (about 600 x 450 cells, A a rotated, shifted, smoothly bent copy of B as in make_golden_align_loop.make_case, in raw
units: scaled and moved away from the origin, on a 1/4096 grid; in the cases without a coarse alignment 8 % of the B cells have no
partner and lie far outside the slice, so that gamma leaves its clamp - in the others, on an even lattice, ``gamma_b=60`` does
that: far cells stretch the box, the coarse alignment's voxels then overlap and hold the same cells, and their ties are
broken by ``np.argpartition`` in a way nothing else can reproduce; every gene's expression peaks at a place of its own, the five cell types live in spatial
domains):

1. 2-D data stored as three columns with constant z; CSR ``.X`` counts, the slices hold different, differently ordered gene
   sets with 40 common genes and a ``highly_variable`` column; ``kl``, ``SVI_mode=False``, ``nn_init=True``, ``K=40``,
   ``max_iter=12``, ``nonrigid_start_iter=2`` (and ``beta=8``, ``gamma_b=60``);
2. 3-D, the SVI default with ``batch_size=150`` and 30 iterations; ``X`` with ``kl`` and a CSR ``.layers`` entry with ``euc``;
   ``normalize_g=True`` (so ``_normalize_exps`` acts on the second layer only), ``separate_scale=True``, ``nn_init=False``
   (its far cells carry next to no counts: voxels of equal expression would tie in the coarse alignment's neighbour lists);
3. ``rep_layer=["X", "celltype"]``, ``rep_field=["layer", "obs"]`` and a ``label_transfer_dict``; ``sparse_calculation_mode``
   with ``sparse_top_k=8``, ``return_mapping=True``, ``nn_init=False``, ``separate_mean=False``;
4. ``morpho_align`` over three slices of equal size, once per mode; the second pair starts from the first pair's
   ``align_spatial``.  ``np.random`` is seeded alike in front of every pair, so that one ``inducing_idx`` pins both.

Twins per case, as in the loop maker: ``dtype="float32"``, and a float64 run with the raw coordinates of B perturbed at 1e-10
relative, which gives the amplification ``g`` per quantity.

The maker asserts what keeps the comparison meaningful and fails instead of writing a weak file: the non-rigid update in
most iterations, no two voxels tied at the edge of the coarse alignment's neighbour lists (which one ``np.argpartition``
keeps is not determined), gamma strictly inside its clamp in at least half of them, sigma2 not at its floor throughout, the final
``optimal_R`` within 0.05 (Frobenius) of the rotation put in, every ``g <= 100``, every value finite.

The dense ``P`` is far above what a committed file may hold: it is stored at every ``P_STRIDE``-th row and column, with its
row and column sums.

    python tests/golden/make_golden_morpho_align.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pandas as pd
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_align_loop as mgl  # noqa: E402
import make_golden_align_start as mgs  # noqa: E402
import make_golden_em as mge  # noqa: E402

PERTURB = 1e-10
P_STRIDE = 9
QUANTITIES = ("XAHat", "RnA", "optimal_RnA", "optimal_R", "optimal_t", "R", "t", "sigma2", "gamma", "Coff")
SEED = 17
CASE_SEEDS = {"1": 2, "2": 2, "3": 1, "4": 1}


class Sample:
    """The stand-in for an AnnData the real class is run on."""

    def __init__(self, X, var, obs, obsm, layers=None, uns=None):
        self.X, self.var, self.obs = X, var, obs
        self.obsm, self.layers, self.uns = dict(obsm), dict(layers or {}), dict(uns or {})

    @property
    def var_names(self):
        return self.var.index

    def __getitem__(self, key):
        rows, cols = key if isinstance(key, tuple) else (key, slice(None))
        if isinstance(rows, (int, np.integer)):
            rows = [int(rows)]
        r = np.arange(self.X.shape[0])[rows]
        if isinstance(cols, slice):
            c = np.arange(self.X.shape[1])[cols]
        else:
            where = {g: i for i, g in enumerate(self.var.index)}
            c = np.array([where[g] for g in cols], dtype=np.int64)
        take = lambda m: m[r][:, c]  # noqa: E731
        return Sample(take(self.X), self.var.iloc[c], self.obs.iloc[r], {k: np.asarray(v)[r] for k, v in self.obsm.items()},
                      {k: take(v) for k, v in self.layers.items()}, self.uns)

    def copy(self):
        return Sample(self.X.copy(), self.var.copy(), self.obs.copy(), {k: np.array(v) for k, v in self.obsm.items()},
                      {k: v.copy() for k, v in self.layers.items()}, dict(self.uns))


class Recorder:
    """np.random.choice / np.random.permutation, recorded."""

    def __enter__(self):
        self.choice, self.permutation = [], []
        self._c, self._p = np.random.choice, np.random.permutation

        def choice(*a, **kw):
            out = self._c(*a, **kw)
            self.choice.append(np.array(out))
            return out

        def permutation(*a, **kw):
            out = self._p(*a, **kw)
            self.permutation.append(np.array(out))
            return out

        np.random.choice, np.random.permutation = choice, permutation
        return self

    def __exit__(self, *exc):
        np.random.choice, np.random.permutation = self._c, self._p


def grid(a, step=4096.0):
    return np.round(np.asarray(a) * step) / step


FAR_FRACTION = 0.08   # of the B cells: moved far outside the slice (a unit normal cloud), so that gamma leaves its clamp at 0.99
FAR_REACH = 12.0


def geometry(rng, NA, NB, D, scale=37.0, offset=(22.0, -14.0, 6.5), bend=0.04, far_silent=False, lattice=False):
    """make_golden_align_loop.make_case's geometry, in raw units: B = a noisy subset of a cloud Z (some of its cells without a
    partner), A = the rigid pre-image of Z, smoothly bent.  Returns (rawA, rawB, R0, Z, ZB): the raw
    coordinates, the rotation put in and the positions both slices' expression is a function of."""
    # lattice (the cases with a coarse alignment): an even density, so that neighbouring voxels seldom hold the same cells -
    # equal voxel means tie in the neighbour lists, and which of them np.argpartition keeps is not determined (run_pair counts
    # the ties that are left and the maker refuses a draw that has one)
    Z = mgs.lattice(rng, NA, D, side=5.0) if lattice else rng.standard_normal((NA, D))
    src = rng.choice(NA, NB)
    ZB = Z[src] + 0.05 * rng.standard_normal((NB, D))
    # the far cells express what some random place of the cloud does: far from every gene's centre their rows would be all
    # zero (far_silent: they are)
    where = ZB.copy()
    # (none in the lattice cases: they stretch the box, the voxels overlap and tie; gamma leaves its clamp through gamma_b there)
    far = rng.choice(NB, 0 if lattice else int(np.ceil(FAR_FRACTION * NB)), replace=False)
    ZB[far] = Z[src[far]] + FAR_REACH * (1.0 + rng.random((len(far), 1))) * np.eye(D)[0]
    where[far] = ZB[far] if far_silent else rng.standard_normal((len(far), D))
    R0, t0 = mgl.rotation(D, 0.35), 0.3 + 0.2 * rng.random(D)
    bend = bend * np.sin(1.3 * Z[:, ::-1] + 0.5)
    XA = (Z + bend - t0) @ R0
    off = np.asarray(offset)[:D]
    return grid(XA * scale + off), grid(ZB * scale + off), R0, Z, where


def counts(rng, Z, centres, level=12.0):
    """CSR counts whose profile is a smooth function of the position: gene g peaks at centres[g]
    (make_golden_align_start.counts)."""
    d2 = ((Z[:, None, :] - centres[None, :, :]) ** 2).sum(-1)
    return rng.poisson(level * np.exp(-d2 / 1.5) + 0.05).astype(np.float64)


def gene_sets(rng, n_common, n_onlyA, n_onlyB):
    """Gene names for the two slices: `n_common` shared ones, in different orders, among genes only one slice has.  Returns
    (namesA, namesB, posA, posB): the permutations that put the genes [common, own] into each slice's order."""
    common = [f"g{i:03d}" for i in range(n_common)]
    namesA = common + [f"a{i:03d}" for i in range(n_onlyA)]
    namesB = common + [f"b{i:03d}" for i in range(n_onlyB)]
    pA, pB = rng.permutation(len(namesA)), rng.permutation(len(namesB))
    return [namesA[i] for i in pA], [namesB[i] for i in pB], pA, pB


def build_pair(rng, NA, NB, D, n_common=40, extra=(9, 13), pad_z=False, second_layer=False, hv=False, bend=0.04, far_silent=False, lattice=False):
    """Two stand-in samples and the rotation put in."""
    rawA, rawB, R0, Z, ZB = geometry(rng, NA, NB, D, bend=bend, far_silent=far_silent, lattice=lattice)
    centres = 1.5 * rng.standard_normal((n_common + extra[0] + extra[1], D))
    cA = np.r_[np.arange(n_common), n_common + np.arange(extra[0])]
    cB = np.r_[np.arange(n_common), n_common + extra[0] + np.arange(extra[1])]
    namesA, namesB, pA, pB = gene_sets(rng, n_common, *extra)
    XA = sp.csr_matrix(counts(rng, Z, centres[cA])[:, pA])
    XB = sp.csr_matrix(counts(rng, ZB, centres[cB])[:, pB])
    domains = 1.2 * rng.standard_normal((5, D))                     # five cell types in spatial domains
    cats = ["T0", "T1", "T2", "T3", "T4"]
    samples = []
    for raw, pos, X, names in ((rawA, Z, XA, namesA), (rawB, ZB, XB, namesB)):
        lab = np.argmin(((pos[:, None, :] - domains[None]) ** 2).sum(-1), axis=1)
        var = pd.DataFrame(index=pd.Index(names))
        if hv:   # most genes are marked; a few common ones are not, in one slice or the other
            var["highly_variable"] = rng.random(len(names)) < 0.9
        obs = pd.DataFrame({"celltype": pd.Categorical([cats[i] for i in lab], categories=cats)})
        coords = np.column_stack([raw, np.full(len(raw), 3.5)]) if pad_z else raw
        layers = {}
        if second_layer:   # a smooth representation on a 1/32 grid, mostly zero: CSR
            where = {g: i for i, g in enumerate(names)}
            d2 = ((pos[:, None, :] - centres[None, :, :]) ** 2).sum(-1)
            own = cA if names is namesA else cB
            dense = np.round((2.0 * np.exp(-d2[:, own] / 2.0) - 0.6 + 0.1 * rng.standard_normal((len(pos), len(own)))) * 32) / 32
            dense = np.maximum(dense, 0.0)[:, pA if names is namesA else pB]
            layers["smooth"] = sp.csr_matrix(dense)
            del where
        samples.append(Sample(X, var, obs, {"spatial": coords}, layers))
    return samples[0], samples[1], R0


def perturbed(sample, key, prng):
    out = sample.copy()
    c = out.obsm[key]
    moving = np.array([len(np.unique(c[:, i])) > 1 for i in range(c.shape[1])])
    c = c.copy()
    c[:, moving] = c[:, moving] * (1.0 + PERTURB * prng.standard_normal((len(c), int(moving.sum()))))
    out.obsm[key] = c
    return out


def run_pair(mc, sampleA, sampleB, kwargs, dtype="float64"):
    """The real constructor and run().  Returns (model, P, draws, info)."""
    np.random.seed(SEED)
    with Recorder() as rec:
        model = mc.Morpho_pairwise(sampleA=sampleA.copy(), sampleB=sampleB.copy(), dtype=dtype, device="cpu", verbose=False,
                                   vecfld_key_added="VecFld_morpho", **kwargs)
        after_init = (len(rec.choice), len(rec.permutation))
        # what the loop does per iteration, for the maker's conditions
        info = dict(nonrigid=0, gamma=[], sigma2=[], coarse_ties=0)
        M = mc.Morpho_pairwise
        upd_nonrigid, upd_sigma2, calc_distance = M._update_nonrigid, M._update_sigma2, mc.calc_distance

        def spy_distance(*a, **kw):
            out = calc_distance(*a, **kw)
            if model.nn_init and "coarse" not in info:   # the first distance matrix of run() is the coarse alignment's (:966)
                info["coarse"] = True
                d, K = np.asarray(out[0], dtype=np.float64), int(model.nn_init_top_K)
                for m_ in (d, d.T):                      # the K nearest of every column, then of every row
                    s_ = np.sort(m_, axis=0)
                    info["coarse_ties"] += int(np.sum(s_[K - 1] == s_[K]))
            return out

        mc.calc_distance = spy_distance

        def spy_nonrigid(self, *a, **kw):
            info["nonrigid"] += 1
            return upd_nonrigid(self, *a, **kw)

        def spy_sigma2(self, *a, **kw):
            out = upd_sigma2(self, *a, **kw)
            info["gamma"].append(float(self.gamma)), info["sigma2"].append(float(self.sigma2))
            return out

        M._update_nonrigid, M._update_sigma2 = spy_nonrigid, spy_sigma2
        try:
            P = model.run()
        finally:
            M._update_nonrigid, M._update_sigma2, mc.calc_distance = upd_nonrigid, upd_sigma2, calc_distance
    draws = dict(choice=rec.choice, permutation=rec.permutation, after_init=after_init)
    return model, P, draws, info


EXTRA = ("probability_parameters", "P")   # measured on the twins like QUANTITIES; P: the whole matrix (its stored entries)


def outputs(model):
    out = {q: np.array(getattr(model, q), dtype=np.float64) for q in QUANTITIES}
    out["t"], out["optimal_t"] = out["t"].reshape(-1), out["optimal_t"].reshape(-1)
    out["probability_parameters"] = np.array([0.0 if p is None else float(p) for p in model.probability_parameters])
    P = model.P
    # (a sparse P is compared as the matrix it stands for: which of several equal entries - the zeros of a far cell's column
    # among them - the top-k keeps is not determined)
    out["P"] = np.array(P.toarray() if sp.issparse(P) else P, dtype=np.float64)
    return out


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = np.abs(b).max()
    d = np.abs(a - b).max()
    return float(d / m) if m > 0 else float(d)


def check_conditions(tag, model, info, R0, gs, max_iter):
    assert info["coarse_ties"] == 0, (tag, "voxels tie at the edge of the coarse alignment's neighbour lists", info["coarse_ties"])
    assert info["nonrigid"] >= (2 * max_iter) // 3, (tag, info["nonrigid"])
    gam = np.array(info["gamma"])
    inside = int(np.sum((gam > 0.01) & (gam < 0.99)))
    assert inside >= max_iter // 2, (tag, inside, gam)
    assert not np.all(np.array(info["sigma2"]) <= 1e-2), (tag, info["sigma2"])
    total_R = np.asarray(model.optimal_R, dtype=np.float64)
    if model.nn_init:   # the loop's rotation acts on coordsA after the coarse transform
        total_R = total_R @ np.asarray(model.init_R, dtype=np.float64)
    assert np.linalg.norm(total_R - R0) <= 0.05, (tag, total_R, R0)
    assert max(gs.values()) <= 100.0, (tag, gs)
    return inside


def store_sample(out, prefix, s, layers=()):
    X = s.X.tocsr()
    out[f"{prefix}_X_indptr"], out[f"{prefix}_X_indices"] = X.indptr.astype(np.int32), X.indices.astype(np.int16)
    out[f"{prefix}_X_data"] = X.data.astype(np.int16)
    assert np.array_equal(X.data, out[f"{prefix}_X_data"])
    out[f"{prefix}_X_shape"] = np.array(X.shape)
    out[f"{prefix}_var_names"] = np.array(list(s.var.index))
    if "highly_variable" in s.var.columns:
        out[f"{prefix}_highly_variable"] = s.var["highly_variable"].to_numpy()
    out[f"{prefix}_celltype"] = s.obs["celltype"].cat.codes.to_numpy().astype(np.int8)
    out[f"{prefix}_categories"] = np.array(list(s.obs["celltype"].cat.categories))
    out[f"{prefix}_spatial"] = s.obsm["spatial"]
    for name in layers:
        L = s.layers[name].tocsr()
        out[f"{prefix}_{name}_indptr"], out[f"{prefix}_{name}_indices"] = L.indptr.astype(np.int32), L.indices.astype(np.int16)
        out[f"{prefix}_{name}_data"] = L.data


def pairwise_case(mc, out, tag, sampleA, sampleB, R0, kwargs, iter_stored, layers=()):
    kw = dict(kwargs, iter_key_added="iter_spatial")
    model, P, draws, info = run_pair(mc, sampleA, sampleB, kw)
    ref = outputs(model)
    f32 = outputs(run_pair(mc, sampleA, sampleB, kw, dtype="float32")[0])
    pert = outputs(run_pair(mc, sampleA, perturbed(sampleB, "spatial", np.random.default_rng(int(tag))), kw)[0])
    gs = {q: rel(pert[q], ref[q]) / PERTURB for q in QUANTITIES + EXTRA}
    fl = {q: rel(f32[q], ref[q]) for q in QUANTITIES + EXTRA}
    assert all(np.isfinite(v).all() for v in ref.values()), tag
    inside = check_conditions(tag, model, info, R0, gs, kw["max_iter"])
    # ---- inputs ----
    store_sample(out, f"{tag}_A", sampleA, layers)
    store_sample(out, f"{tag}_B", sampleB, layers)
    out[f"{tag}_R0"] = R0
    # ---- what the reference drew and chose ----
    n_choice, _ = draws["after_init"]
    assert n_choice <= 1 and len(draws["choice"]) == n_choice, (tag, "only the inducing variables may be drawn with choice")
    if n_choice:
        out[f"{tag}_inducing_idx"] = draws["choice"][0]
    if draws["permutation"]:
        assert len(draws["permutation"]) == 1
        out[f"{tag}_batch_perm"] = draws["permutation"][0]
    out[f"{tag}_genes"] = np.array(list(model.genes))
    for q in ("rep_layer", "rep_field", "dissimilarity", "probability_type"):
        out[f"{tag}_{q}"] = np.array(list(getattr(model, q)))
    # ---- outputs ----
    for q in QUANTITIES:
        out[f"{tag}_{q}"] = ref[q]
    for q in QUANTITIES + EXTRA:
        out[f"{tag}_g_{q}"], out[f"{tag}_f32_{q}"] = np.float64(gs[q]), np.float64(fl[q])
    out[f"{tag}_normalize_scales"] = np.array(model.normalize_scales, dtype=np.float64)
    out[f"{tag}_normalize_means"] = np.array(model.normalize_means, dtype=np.float64)
    out[f"{tag}_probability_parameters"] = np.array([np.nan if p is None else float(p) for p in model.probability_parameters])
    out[f"{tag}_inducing_variables"] = np.array(model.inducing_variables, dtype=np.float64)
    out[f"{tag}_vecfld_keys"] = np.array(sorted(model.vecfld))
    out[f"{tag}_norm_dict_keys"] = np.array(sorted(model.vecfld["norm_dict"]))
    for it in iter_stored:
        out[f"{tag}_iter_{it}"] = np.array(model.iter_added[model.key_added][it], dtype=np.float64)
    out[f"{tag}_iter_stored"] = np.array(iter_stored)
    out[f"{tag}_iter_sigma2"] = np.array([float(model.iter_added["sigma2"][it]) for it in range(kw["max_iter"])])
    if sp.issparse(P):
        P = P.tocoo()
        out[f"{tag}_P_row"], out[f"{tag}_P_col"], out[f"{tag}_P_data"] = P.row.astype(np.int32), P.col.astype(np.int32), P.data
        out[f"{tag}_P_shape"] = np.array(P.shape)
    else:
        P = np.asarray(P, dtype=np.float64)
        out[f"{tag}_P_shape"], out[f"{tag}_P_sub"] = np.array(P.shape), P[::P_STRIDE, ::P_STRIDE]
        out[f"{tag}_P_rowsum"], out[f"{tag}_P_colsum"] = P.sum(1), P.sum(0)
    out[f"{tag}_P_max"] = np.float64(P.max())
    print(f"case {tag}: {model.NA} x {model.NB}, D {model.D}, {len(model.genes)} genes, sigma2 {info['sigma2'][0]:.4g} -> "
          f"{info['sigma2'][-1]:.4g}, gamma inside the clamp in {inside}/{kw['max_iter']}, non-rigid in {info['nonrigid']}, "
          f"|optimal_R - R0| {np.linalg.norm(ref['optimal_R'] @ (np.asarray(model.init_R) if model.nn_init else np.eye(model.D)) - R0):.3g}\n"
          "    g         " + ", ".join(f"{q} {gs[q]:.2g}" for q in QUANTITIES + EXTRA) + "\n"
          "    f32 floor " + ", ".join(f"{q} {fl[q]:.1e}" for q in QUANTITIES + EXTRA))
    return model


def reference_morpho_align(mc, models, mode, dtype="float64", key_added="align_spatial", **kwargs):
    """The loop of morpho_alignment.py:67-111 around the real class (np.random seeded alike in front of every pair)."""
    align_models = [m.copy() for m in models]
    for m in align_models:
        m.obsm[key_added] = m.obsm["spatial"].copy()
        m.obsm[f"{key_added}_rigid"] = m.obsm["spatial"].copy()
        m.obsm[f"{key_added}_nonrigid"] = m.obsm["spatial"].copy()
    pis, draws = [], []
    for i in range(len(align_models) - 1):
        modelA, modelB = align_models[i], align_models[i + 1]
        np.random.seed(SEED)
        with Recorder() as rec:
            morpho_model = mc.Morpho_pairwise(sampleA=modelB, sampleB=modelA, spatial_key=key_added, key_added=key_added,
                                              iter_key_added="iter_spatial", vecfld_key_added="VecFld_morpho", dtype=dtype,
                                              device="cpu", verbose=False, **kwargs)
            P = morpho_model.run()
        draws.append(rec.choice)
        modelB.obsm[f"{key_added}_rigid"] = morpho_model.optimal_RnA.copy()
        modelB.obsm[f"{key_added}_nonrigid"] = morpho_model.XAHat.copy()
        modelB.obsm[key_added] = modelB.obsm[f"{key_added}_rigid" if mode == "SN-S" else f"{key_added}_nonrigid"]
        modelB.uns["iter_spatial"], modelB.uns["VecFld_morpho"] = morpho_model.iter_added, morpho_model.vecfld
        pis.append(P.T)
    return align_models, pis, draws, morpho_model


def morpho_align_case(mc, out, tag, rng, kwargs):
    N, D = 503, 2
    # three slices of N cells: slice 1 is a rotated, shifted, bent copy of slice 0's cloud (a pair as in the other cases),
    # slice 2 is slice 1 moved once more, its cells in another order
    s1, s0, _ = build_pair(rng, N, N, D, lattice=True)            # (sampleA, the one that moves, is the LATER slice)
    c1 = s1.obsm["spatial"]
    s2 = s1.copy()
    s2.obsm["spatial"] = grid((c1 - c1.mean(0)) @ mgl.rotation(D, -0.25).T + c1.mean(0) + np.array([11.0, -7.0])
                              + 0.4 * np.sin(c1[:, ::-1] / 29.0))
    s2 = s2[rng.permutation(N)]
    models = [s0, s1, s2]
    genes = sorted(set(s0.var.index) & set(s1.var.index))
    kwargs = dict(kwargs, genes=genes)
    out[f"{tag}_genes"] = np.array(genes)
    for i, s in enumerate(models):
        store_sample(out, f"{tag}_slice{i}", s)
    for mode in ("SN-S", "SN-N"):
        ref, pis, draws, _ = reference_morpho_align(mc, models, mode, **kwargs)
        f32, _, _, _ = reference_morpho_align(mc, models, mode, dtype="float32", **kwargs)
        pmodels = [perturbed(models[0], "spatial", np.random.default_rng(4)), models[1], models[2]]
        pert, _, _, _ = reference_morpho_align(mc, pmodels, mode, **kwargs)
        assert all(len(d) == 1 for d in draws) and np.array_equal(draws[0][0], draws[1][0]), "one inducing_idx must pin both pairs"
        out[f"{tag}_inducing_idx"] = draws[0][0]
        m = mode.replace("-", "")
        for i in (1, 2):
            for key in ("align_spatial_rigid", "align_spatial_nonrigid"):
                a = np.array(ref[i].obsm[key], dtype=np.float64)
                g = rel(pert[i].obsm[key], a) / PERTURB
                assert np.isfinite(a).all() and g <= 100.0, (tag, mode, i, key, g)
                out[f"{tag}_{m}_slice{i}_{key}"] = a
                out[f"{tag}_{m}_slice{i}_g_{key}"] = np.float64(g)
                out[f"{tag}_{m}_slice{i}_f32_{key}"] = np.float64(rel(f32[i].obsm[key], a))
            chosen = "align_spatial_rigid" if mode == "SN-S" else "align_spatial_nonrigid"
            assert np.array_equal(ref[i].obsm["align_spatial"], ref[i].obsm[chosen])
            out[f"{tag}_{m}_slice{i}_sigma2"] = np.float64(ref[i].uns["VecFld_morpho"]["sigma2"])
        out[f"{tag}_{m}_pis_shapes"] = np.array([p.shape for p in pis])
        out[f"{tag}_{m}_pi1_rowsum"] = np.asarray(pis[1], dtype=np.float64).sum(1)
        print(f"case {tag} {mode}: g " + ", ".join(f"{float(out[f'{tag}_{m}_slice{i}_g_{key}']):.2g}" for i in (1, 2)
                                                    for key in ("align_spatial_rigid", "align_spatial_nonrigid")))


def main():
    mc, _, _ = mge.load_morpho_class()
    # one draw per case, chosen among the first few seeds as one on which the reference meets every condition above (without a
    # coarse alignment the rotation found lies 0.02 to 0.07 from the one put in, depending on the cloud; t is small after a
    # coarse alignment, and its g, relative to its own size, moves around 100)
    rngs = {tag: np.random.default_rng(seed) for tag, seed in CASE_SEEDS.items()}
    out = {"cases": np.array(["1", "2", "3", "4"]), "quantities": np.array(QUANTITIES), "p_stride": np.int64(P_STRIDE),
           "perturb": np.float64(PERTURB)}
    common = dict(lambdaVF=100.0)
    # ---- case 1 ----
    A, B, R0 = build_pair(rngs["1"], 607, 451, 2, pad_z=True, hv=True, lattice=True)
    kw1 = dict(common, dissimilarity="kl", SVI_mode=False, nn_init=True, K=40, beta=8.0, max_iter=12, nonrigid_start_iter=2,
               gamma_b=60.0)
    pairwise_case(mc, out, "1", A, B, R0, kw1, iter_stored=(0, 6))
    # ---- case 2 ----
    A, B, R0 = build_pair(rngs["2"], 593, 447, 3, second_layer=True, far_silent=True)
    stiff = dict(lambdaVF=1000.0)   # (at 100 the 150-cell batches leave the rotation 0.08 from the one put in after 30 iterations)
    kw2 = dict(stiff, rep_layer=["X", "smooth"], rep_field=["layer", "layer"], dissimilarity=["kl", "euc"], batch_size=150,
               max_iter=30, nonrigid_start_iter=2, K=40, beta=6.0, normalize_g=True, separate_scale=True, nn_init=False)
    m2 = pairwise_case(mc, out, "2", A, B, R0, kw2, iter_stored=(0, 15), layers=("smooth",))
    raw = A[:, list(m2.genes)].layers["smooth"].toarray()
    i = np.unravel_index(np.argmax(raw), raw.shape)
    out["2_exp_scale"] = np.float64(raw[i] / np.asarray(m2.exp_layers_A[1], dtype=np.float64)[i])
    # ---- case 3 ----
    A, B, R0 = build_pair(rngs["3"], 611, 443, 3)
    cats = list(A.obs["celltype"].cat.categories)
    ltd = {ca: {cb: (0.05 if ca == cb else 1.0 + 0.125 * abs(i - j)) for j, cb in enumerate(cats)} for i, ca in enumerate(cats)}
    kw3 = dict(stiff, rep_layer=["X", "celltype"], rep_field=["layer", "obs"], label_transfer_dict=ltd,
               sparse_calculation_mode=True, sparse_top_k=8, return_mapping=True, nn_init=False, separate_mean=False,
               batch_size=150, max_iter=30, nonrigid_start_iter=2, K=40, beta=6.0)
    pairwise_case(mc, out, "3", A, B, R0, kw3, iter_stored=(0, 15))
    out["3_label_transfer_values"] = np.array([[ltd[ca][cb] for cb in cats] for ca in cats])
    # ---- case 4 ----
    kw4 = dict(kw1)
    morpho_align_case(mc, out, "4", rngs["4"], kw4)
    path = os.path.join(HERE, "ref_morpho_align.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, f"({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
