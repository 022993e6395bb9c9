"""``align.pca`` / ``align.group_pca`` on the device against the NumPy restatement (``tests/_pca_case.py``: centre ->
``np.linalg.svd`` -> the sign rule), with the bounds derived there - not fitted: per component ``max(1.25 x the
disagreement of the restatement's SVD and eigh routes, G eps lambda_1 / gap_i)``, the scores scaled by the largest row
norm, the variances by ``lambda_1``.  Inputs have a planted spectrum (geometric, ratio 0.8, over the first k + 3 directions),
so every component is individually defined.  The float32 mode's oracle runs on the centred operand rounded to float32 -
what the device stores - and its scores get ``2^-24 max |score|`` more: they leave the device in the cell dtype.

Then the end to end: ``group_pca`` on three ``AnnDataLite`` slices (one CSR) and ``Morpho_pairwise`` on ``obsm["X_pca"]``."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _pca_case as pc
from _kernel_scaffold import bits as _bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def align():
    import spateo_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return spateo_amd.align


_DATA = {}


def _case(name):
    """(list of slices, stacked float64 matrix, k), made once."""
    if name not in _DATA:
        if name == "1000x96":
            X = pc.planted(1000, 96, 10, seed=11)
            _DATA[name] = ([X], X, 10)
        elif name == "257x17":
            X = pc.planted(257, 17, 5, seed=12)
            _DATA[name] = ([X], X, 5)
        else:
            X = pc.planted(1000, 96, 10, seed=13)
            _DATA[name] = ([X[:400], sp.csr_matrix(X[400:750]), X[750:]], X, 10)
    return _DATA[name]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", ["1000x96", "257x17", "3 slices"])
def test_parity_with_the_restatement(align, name, dtype):
    mats, X, k = _case(name)
    N, G = X.shape
    res = align.pca(mats, n_comps=k, dtype=dtype, device=DEV)
    assert [s.shape for s in res["X_pca"]] == [(m.shape[0], k) for m in mats] and res["PCs"].shape == (G, k)
    exact = np.array([math.fsum(X[:, j].tolist()) for j in range(G)]) / N
    assert np.abs(res["mean"] - exact).max() <= N * pc.EPS * np.abs(X).max()
    Xc = X - res["mean"]
    if dtype == "float32":
        Xc = Xc.astype(np.float32).astype(np.float64)   # the operand as the device stores it
    pc.check_against(res["PCs"], np.vstack(res["X_pca"]), res["variance"], Xc, k, N - 1,
                     score_extra=2.0 ** -24 if dtype == "float32" else 0.0, label=f"{name} {dtype}")
    # a ratio's numerator and the trace each carry at most the variances' relative bound, and lambda_i <= trace
    orc, _, _, var_tol = pc.bounds(Xc, k, N - 1)
    assert np.abs(res["variance_ratio"] - orc["variance_ratio"]).max() <= 2 * var_tol / orc["lam_all"][0]
    top = np.argmax(np.abs(res["PCs"]), axis=0)
    assert (res["PCs"][top, np.arange(k)] > 0).all()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_without_centring_it_is_the_svd_of_the_raw_matrix(align, dtype):
    mats, X, k = _case("257x17")
    res = align.pca(mats, n_comps=k, zero_center=False, dtype=dtype, device=DEV)
    assert not res["mean"].any()
    Xr = X.astype(np.float32).astype(np.float64) if dtype == "float32" else X
    pc.check_against(res["PCs"], res["X_pca"][0], res["variance"], Xr, k, len(X), score_extra=2.0 ** -24 if dtype == "float32" else 0.0,
                     label=f"raw 257x17 {dtype}")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_list_of_slices_gives_the_bits_of_the_stacked_matrix(align, dtype):
    mats, X, k = _case("3 slices")
    a = align.pca(mats, n_comps=k, dtype=dtype, device=DEV)
    b = align.pca([X], n_comps=k, dtype=dtype, device=DEV)
    c = align.pca(mats, n_comps=k, dtype=dtype, device=DEV)
    for q in ("PCs", "variance", "variance_ratio", "mean"):
        assert np.array_equal(_bits(a[q]), _bits(b[q])), q
        assert np.array_equal(_bits(a[q]), _bits(c[q])), ("two calls", q)
    assert np.array_equal(_bits(np.vstack(a["X_pca"])), _bits(b["X_pca"][0]))
    assert np.array_equal(_bits(np.vstack(a["X_pca"])), _bits(np.vstack(c["X_pca"])))


def _series(seed=21):
    """Three slices of one tissue: smooth expression programmes over 2-D positions, Poisson counts, the middle slice CSR."""
    from spateo_amd import AnnDataLite

    rng = np.random.default_rng(seed)
    G = 96
    W = rng.standard_normal((4, G)) * 0.6
    out = []
    for i, n in enumerate((400, 350, 250)):
        xy = rng.uniform(0.0, 10.0, (n, 2))
        F = np.stack([np.sin(xy[:, 0] * 0.6), np.cos(xy[:, 1] * 0.5), xy[:, 0] / 10.0, xy[:, 1] / 10.0], axis=1)
        X = rng.poisson(np.exp(1.0 + F @ W)).astype(np.float64)
        th = 0.2 * i
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        out.append(AnnDataLite(X=sp.csr_matrix(X) if i == 1 else X, var_names=[f"g{j}" for j in range(G)],
                               obsm={"spatial": xy @ R.T + 0.5 * i}))
    return out


def test_group_pca_then_morpho_pairwise_end_to_end(align):
    ads = _series()
    align.group_pca(ads, use_hvg=False, n_comps=20, dtype="float32", device=DEV)
    assert [a.obsm["X_pca"].shape for a in ads] == [(400, 20), (350, 20), (250, 20)]
    assert all(np.isfinite(a.obsm["X_pca"]).all() and a.obsm["X_pca"].dtype == np.float64 for a in ads)
    first = [a.obsm["X_pca"].copy() for a in ads]
    align.group_pca(ads, use_hvg=False, n_comps=20, dtype="float32", device=DEV)
    assert all(np.array_equal(_bits(p), _bits(a.obsm["X_pca"])) for p, a in zip(first, ads)), "a second call must give equal bits"
    m = align.Morpho_pairwise(ads[0], ads[1], rep_layer="X_pca", rep_field="obsm", dissimilarity="cos", dtype="float32", device=DEV,
                              verbose=False, SVI_mode=False, nn_init=False, K=20, max_iter=6, nonrigid_start_iter=2)
    m.run()
    assert m.XAHat.shape == (400, 2) and np.isfinite(m.XAHat).all()
    assert np.isfinite(m.optimal_RnA).all() and np.isfinite(m.sigma2) and np.isfinite(np.asarray(m.R)).all()
