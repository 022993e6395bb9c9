"""The cases of tests/golden/ref_morpho_align.npz (tests/golden/make_golden_morpho_align.py) as ``AnnDataLite`` samples and
``Morpho_pairwise`` / ``morpho_align`` arguments, and the bounds of the comparison - those of tests/_align_loop_case.py: the
constants are imported, not copied."""
import os

import numpy as np
import scipy.sparse as sp

import _align_loop_case as lc

HERE = os.path.dirname(os.path.abspath(__file__))
F64_TOL, F32_BASE, ALLOW = lc.F64_TOL, lc.F32_BASE, lc.ALLOW
HOST_TOL = 1e-12     # plain float64 sums on the host: normalisation parameters, expression scale
QUANTITIES = ("XAHat", "RnA", "optimal_RnA", "optimal_R", "optimal_t", "R", "t", "sigma2", "gamma", "Coff")
# the constructor arguments of the maker's cases (the settings; the data and what the reference drew come from the file)
CASE_KW = {
    "1": dict(lambdaVF=100.0, dissimilarity="kl", SVI_mode=False, nn_init=True, K=40, beta=8.0, max_iter=12, nonrigid_start_iter=2,
              gamma_b=60.0),
    "2": dict(lambdaVF=1000.0, rep_layer=["X", "smooth"], rep_field=["layer", "layer"], dissimilarity=["kl", "euc"], batch_size=150,
              max_iter=30, nonrigid_start_iter=2, K=40, beta=6.0, normalize_g=True, separate_scale=True, nn_init=False),
    "3": dict(lambdaVF=1000.0, rep_layer=["X", "celltype"], rep_field=["layer", "obs"], sparse_calculation_mode=True, sparse_top_k=8,
              return_mapping=True, nn_init=False, separate_mean=False, batch_size=150, max_iter=30, nonrigid_start_iter=2, K=40,
              beta=6.0),
    "4": dict(lambdaVF=100.0, dissimilarity="kl", SVI_mode=False, nn_init=True, K=40, beta=8.0, max_iter=12, nonrigid_start_iter=2,
              gamma_b=60.0),
}
CASE_LAYERS = {"1": (), "2": ("smooth",), "3": (), "4": ()}


def load():
    with np.load(os.path.join(HERE, "golden", "ref_morpho_align.npz")) as z:
        return {k: z[k] for k in z.files}


def _csr(G, prefix, name, shape, dtype=np.float64):
    return sp.csr_matrix((G[f"{prefix}_{name}_data"].astype(dtype), G[f"{prefix}_{name}_indices"].astype(np.int32),
                          G[f"{prefix}_{name}_indptr"].astype(np.int64)), shape=shape)


def sample(G, prefix, layers=(), dense=False, counts_dtype=np.float64):
    """One stored slice as an AnnDataLite: CSR ``.X`` counts (``dense``: the same matrices as arrays), the ``celltype`` column
    as a pandas categorical, ``highly_variable`` where the case has it."""
    import pandas as pd

    from spateo_amd import AnnDataLite

    shape = tuple(int(v) for v in G[f"{prefix}_X_shape"])
    X = _csr(G, prefix, "X", shape, counts_dtype)
    L = {name: _csr(G, prefix, name, shape) for name in layers}
    if dense:
        X, L = X.toarray(), {k: v.toarray() for k, v in L.items()}
    cats = [str(c) for c in G[f"{prefix}_categories"]]
    obs = {"celltype": pd.Series(pd.Categorical.from_codes(G[f"{prefix}_celltype"].astype(np.int64), categories=cats))}
    var = {"highly_variable": G[f"{prefix}_highly_variable"]} if f"{prefix}_highly_variable" in G else None
    return AnnDataLite(X=X, var_names=[str(g) for g in G[f"{prefix}_var_names"]], layers=L, obs=obs, var=var,
                       obsm={"spatial": np.array(G[f"{prefix}_spatial"])})


def pinning(G, tag):
    """What the reference drew and chose, handed back: ``genes=`` in its order, ``inducing_idx=``, ``batch_perm=``."""
    kw = dict(genes=[str(g) for g in G[f"{tag}_genes"]])
    if f"{tag}_inducing_idx" in G:
        kw["inducing_idx"] = G[f"{tag}_inducing_idx"].astype(np.int64)
    if f"{tag}_batch_perm" in G:
        kw["batch_perm"] = G[f"{tag}_batch_perm"].astype(np.int64)
    return kw


def label_transfer_dict(G, tag):
    cats = [str(c) for c in G[f"{tag}_A_categories"]]
    T = G[f"{tag}_label_transfer_values"]
    return {ca: {cb: float(T[i, j]) for j, cb in enumerate(cats)} for i, ca in enumerate(cats)}


def pair_kwargs(G, tag, **over):
    kw = dict(CASE_KW[tag], **pinning(G, tag))
    if tag == "3":
        kw["label_transfer_dict"] = label_transfer_dict(G, tag)
    kw.update(over)
    return kw


def pair_samples(G, tag, dense=False):
    return sample(G, f"{tag}_A", CASE_LAYERS[tag], dense), sample(G, f"{tag}_B", CASE_LAYERS[tag], dense)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = np.abs(b).max()
    d = np.abs(a - b).max()
    return float(d / m) if m > 0 else float(d)


def bound(g, f32_floor, f32):
    """tests/_align_loop_case.bounds for one quantity: float64 ``1e-10 max(1, 1.25 g)``; float32 ``max(1.25 x the reference's
    own float32 twin, 1e-5 max(1, 1.25 g))``."""
    b = (F32_BASE if f32 else F64_TOL) * max(1.0, ALLOW * float(g))
    return max(ALLOW * float(f32_floor), b) if f32 else b
