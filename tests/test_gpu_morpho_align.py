"""``spateo_amd.align.Morpho_pairwise`` / ``morpho_align`` and the sparse layers on ``cuda:0``.

* CSR layers against the same call with ``.toarray()`` layers: equal bits - ``update_assignment`` (dense and top-k) and a whole
  ``Morpho_pairwise`` run (case 1 at ``max_iter=3``); two ``run()``s of equal objects: equal bits.
* Cases 1 - 4 of tests/golden/ref_morpho_align.npz, the real reference class run on stand-in samples
  (tests/golden/make_golden_morpho_align.py), in both cell dtypes, relative to each quantity's maximum, with the bounds of
  tests/test_gpu_align_loop.py (constants imported through tests/_morpho_align_case.py):
  float64 ``1e-10 max(1, 1.25 g)`` with the fixture's amplification ``g``; float32 ``max(1.25 x the reference's own float32
  twin, 1e-5 max(1, 1.25 g))``; ``Coff`` in float64 only, as there.  The normalisation parameters are plain float64 host sums
  (1e-12).  A sparse ``P`` is compared as the matrix it stands for (which of several equal entries - the zeros of a far cell's
  column among them - the top-k keeps is not determined) and by its column layout.
* ``BA_transform(model.vecfld, raw coordsA)`` reproduces ``XAHat`` and ``optimal_RnA`` to 1e-10 (float64) in cases 1 and 3.  Not
  in case 2, for a reason that lies in the reference: with ``separate_scale=True`` its ``BA_transform`` de-normalises with the
  moving slice's scale (``norm_dict["scale_transformed"]``, ``transform.py:104-107``) where ``_wrap_output`` uses the fixed
  slice's (``normalize_scales[1]``, ``morpho_class.py:1484-1486``); the test asserts the relation that does hold.

Run with ``-s`` for the worst deviation / bound per case and dtype."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import _morpho_align_case as mc
from _kernel_scaffold import fresh_kernels as _k, same_bits as _same_bits

pytestmark = pytest.mark.gpu

DEV = "0"        # the reference's way of naming a GPU: -> cuda:0
G = mc.load()
_RUNS, _WORST = {}, {}


def _run(tag, dtype):
    if (tag, dtype) not in _RUNS:
        from spateo_amd import align

        A, B = mc.pair_samples(G, tag)
        m = align.Morpho_pairwise(A, B, dtype=dtype, device=DEV, verbose=False, iter_key_added="iter_spatial",
                                  **mc.pair_kwargs(G, tag))
        m.returned = m.run()
        _RUNS[(tag, dtype)] = m
    return _RUNS[(tag, dtype)]


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    yield
    print("\n| case | dtype | worst deviation / bound | quantity |\n|---|---|---|---|")
    for (tag, dtype), (v, q) in sorted(_WORST.items()):
        print(f"| {tag} | {dtype} | {v:.3g} | {q} |")


def _ratio(tag, dtype, q, dev, tol):
    r = dev / tol
    if r > _WORST.get((tag, dtype), (0.0, ""))[0]:
        _WORST[(tag, dtype)] = (r, q)
    return r


# ---- sparse layers: the same bits as dense ones ----
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_update_assignment_csr_layers_equal_dense_layers(dtype):
    from spateo_amd import align

    rng = np.random.default_rng(3)
    NA, NB, g = 131, 97, 70
    XA, XB = rng.standard_normal((NA, 3)), rng.standard_normal((NB, 3))
    counts_A, counts_B = rng.poisson(0.4, (NA, g)).astype(np.float64), rng.poisson(0.4, (NB, g)).astype(np.float64)
    counts_A[5] = 0.0                                                       # an empty row
    smooth_A, smooth_B = np.maximum(rng.standard_normal((NA, 33)), 0.0), np.maximum(rng.standard_normal((NB, 33)), 0.0)
    kw = dict(dissimilarity=["kl", "euc", "cos"], probability_type=["gauss", "gauss", "cos"], probability_parameters=[0.1, 5.0, None],
              sigma2=0.3, alpha=rng.uniform(0.5, 1.0, NA), SigmaDiag=0.05 * rng.random(NA), gamma=0.6, samples_s=30.0, dtype=dtype,
              device="cuda:0")
    dense = [[counts_A, smooth_A, smooth_A], [counts_B, smooth_B, smooth_B]]
    # CSR with integer counts, CSC float32-representable values, COO: every format goes through tocsr()
    sparse = [[sp.csr_matrix(counts_A.astype(np.int64)), sp.csc_matrix(smooth_A), sp.coo_matrix(smooth_A)],
              [sp.csr_matrix(counts_B.astype(np.int64)), sp.csc_matrix(smooth_B), sp.coo_matrix(smooth_B)]]
    for extra in (dict(), dict(return_P=True), dict(sparse_calculation_mode=True, sparse_top_k=8)):
        want = align.update_assignment(XA, XB, dense[0], dense[1], **kw, **extra)
        got = align.update_assignment(XA, XB, sparse[0], sparse[1], **kw, **extra)
        assert want.keys() == got.keys()
        for q in want:
            a, b = (v.toarray() if sp.issparse(v) else np.asarray(v) for v in (want[q], got[q]))
            assert _same_bits(a, b), (extra, q)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_assign_prepare_from_csr_equals_the_dense_path(dtype):
    """HipKernels.assign_prepare itself, at several sizes and fillings (three uploads per call: each must keep its own
    device memory until the launch), all-zero and float32 layers among them."""
    import torch

    from spateo_amd import _lib

    k = _k(dtype)
    rng = np.random.default_rng(11)
    for n, g, density in ((607, 33, 0.5), (451, 33, 0.5), (64, 64, 1.0), (300, 7, 0.1), (1000, 130, 0.05), (9, 40, 0.0)):
        dense = rng.poisson(3.0, (n, g)).astype(np.float64) * (rng.random((n, g)) < density)
        for layer in (sp.csr_matrix(dense), sp.csr_matrix(dense.astype(np.float32)), sp.coo_matrix(dense.astype(np.int32))):
            for metric in ("kl", "euc", "cos"):
                for side in (0, 1):
                    want = k.assign_prepare(dense, _lib.ASSIGN_METRICS[metric], side)
                    got = k.assign_prepare(layer, _lib.ASSIGN_METRICS[metric], side)
                    assert want[2] == got[2] and torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]), (n, g, density, metric, side)


def _outputs(m):
    out = {q: np.asarray(getattr(m, q), dtype=np.float64) for q in mc.QUANTITIES}
    out.update(P=np.asarray(m.P), probability_parameters=np.array(m.probability_parameters, dtype=np.float64),
               inducing_variables=m.inducing_variables, normalize_scales=m.normalize_scales, normalize_means=m.normalize_means,
               vecfld_Coff=m.vecfld["Coff"], K_NA=m.K_NA, alpha=m.alpha)
    return out


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_csr_X_equals_dense_X_and_two_runs_agree(dtype):
    from spateo_amd import align

    kw = mc.pair_kwargs(G, "1", max_iter=3)
    runs = []
    for dense in (False, False, True):
        A, B = mc.pair_samples(G, "1", dense=dense)
        m = align.Morpho_pairwise(A, B, dtype=dtype, device=DEV, verbose=False, **kw)
        m.run()
        runs.append(_outputs(m))
    assert sp.issparse(mc.pair_samples(G, "1")[0].X)
    for q in runs[0]:
        assert _same_bits(runs[0][q], runs[1][q]), ("two runs", q)
        assert _same_bits(runs[0][q], runs[2][q]), ("CSR against dense", q)


# ---- the reference's cases ----
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tag", ["1", "2", "3"])
def test_pairwise_cases_against_the_reference(tag, dtype):
    m = _run(tag, dtype)
    f32 = dtype == "float32"
    bad = []

    def check(q, got, ref, g_name=None, scale=None):
        g_name = g_name or q
        tol = mc.bound(G[f"{tag}_g_{g_name}"], G[f"{tag}_f32_{g_name}"], f32)
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (q, got.shape, ref.shape)
        dev = float(np.abs(got - ref).max() / (scale if scale is not None else np.abs(ref).max()))
        r = _ratio(tag, dtype, q, dev, tol)
        print(f"  case {tag} {dtype} {q}: {dev:.2e} / {tol:.2e} ({r:.2g}x)")
        if not dev <= tol:
            bad.append((q, dev, tol))

    for q in mc.QUANTITIES:
        if q == "Coff" and f32:      # the reference's own float32 Coff is off by 0.7 - 1.0: pinv leaves it poorly determined
            continue
        check(q, np.asarray(getattr(m, q), dtype=np.float64).reshape(G[f"{tag}_{q}"].shape), G[f"{tag}_{q}"])
    # what the reference drew, handed back through the pinning arguments
    ctrl = G[f"{tag}_inducing_variables"]
    assert np.abs(m.inducing_variables - ctrl).max() <= mc.HOST_TOL * np.abs(ctrl).max()
    for q in ("normalize_scales", "normalize_means"):
        assert np.abs(getattr(m, q) - G[f"{tag}_{q}"]).max() <= mc.HOST_TOL * np.abs(G[f"{tag}_{q}"]).max(), q
    ref_pp = np.nan_to_num(G[f"{tag}_probability_parameters"], nan=0.0)
    check("probability_parameters", [0.0 if p is None else p for p in m.probability_parameters], ref_pp)
    # the per-iteration record
    stored = [int(i) for i in G[f"{tag}_iter_stored"]]
    assert sorted(m.iter_added["align_spatial"]) == list(range(m.max_iter)) == sorted(m.iter_added["sigma2"])
    for it in stored:
        check(f"iter_added[{it}]", m.iter_added["align_spatial"][it], G[f"{tag}_iter_{it}"], "XAHat")
    check("iter_added[sigma2]", [float(m.iter_added["sigma2"][i]) for i in range(m.max_iter)], G[f"{tag}_iter_sigma2"], "sigma2")
    # P
    P, shape, pmax = m.returned, tuple(int(v) for v in G[f"{tag}_P_shape"]), float(G[f"{tag}_P_max"])
    assert P is m.P and P.shape == shape
    if tag == "3":
        assert sp.issparse(P) and P.format == "coo" and P.nnz == len(G["3_P_data"])
        k = P.nnz // shape[1]
        assert np.array_equal(P.col, np.repeat(np.arange(shape[1]), k)) and np.array_equal(P.col, G["3_P_col"])   # the layout
        ref = sp.coo_matrix((G["3_P_data"], (G["3_P_row"], G["3_P_col"])), shape=shape).toarray()
        check("P", P.toarray(), ref, "P", scale=pmax)
    else:
        assert isinstance(P, np.ndarray) and (tag != "2" or shape[1] == 150)      # case 2: NA x batch_size
        s = int(G["p_stride"])
        check("P[::s, ::s]", P[::s, ::s], G[f"{tag}_P_sub"], "P", scale=pmax)
        check("P row sums", P.sum(1), G[f"{tag}_P_rowsum"], "P")
        check("P column sums", P.sum(0), G[f"{tag}_P_colsum"], "P")
    assert not bad, bad
    assert sorted(m.vecfld) == [str(v) for v in G[f"{tag}_vecfld_keys"]]
    assert m.genes == [str(v) for v in G[f"{tag}_genes"]]


@pytest.mark.parametrize("tag", ["1", "2", "3"])
def test_BA_transform_reproduces_the_aligned_coordinates(tag):
    from spateo_amd import align

    m = _run(tag, "float64")
    hat, _, opt = align.BA_transform(m.vecfld, m.raw_coordsA, dtype="float64", device="cuda:0")
    if tag == "2":   # separate_scale=True: the reference's BA_transform scales back with the MOVING slice's scale (see above)
        s0, s1, mean = m.normalize_scales[0], m.normalize_scales[1], m.normalize_means[1]
        hat, opt = (hat - mean) / s0 * s1 + mean, (opt - mean) / s0 * s1 + mean
    for q, got in (("XAHat", hat), ("optimal_RnA", opt)):
        want = getattr(m, q)
        dev = float(np.abs(got - want).max() / np.abs(want).max())
        print(f"  case {tag} BA_transform {q}: {dev:.2e}")
        assert dev <= mc.F64_TOL, (q, dev)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("mode", ["SN-S", "SN-N"])
def test_morpho_align_over_three_slices(mode, dtype):
    from spateo_amd import align

    models = [mc.sample(G, f"4_slice{i}") for i in range(3)]
    assert all(sp.issparse(s.X) for s in models)
    kw = dict(mc.CASE_KW["4"], **mc.pinning(G, "4"))
    aligned, pis = align.morpho_align(models, mode=mode, dtype=dtype, device=DEV, verbose=False, **kw)
    f32, tag, m_ = dtype == "float32", f"4 {mode}", mode.replace("-", "")
    assert len(aligned) == 3 and len(pis) == 2
    assert [tuple(p.shape) for p in pis] == [tuple(int(v) for v in s) for s in G[f"4_{m_}_pis_shapes"]]
    assert np.array_equal(aligned[0].obsm["align_spatial"], models[0].obsm["spatial"])       # the first slice stays
    assert "align_spatial" not in models[1].obsm                                             # the models were copied
    bad = []
    for i in (1, 2):
        chosen = "align_spatial_rigid" if mode == "SN-S" else "align_spatial_nonrigid"
        assert np.array_equal(aligned[i].obsm["align_spatial"], aligned[i].obsm[chosen])
        assert sorted(aligned[i].uns["iter_spatial"]["sigma2"]) == list(range(kw["max_iter"]))
        assert aligned[i].uns["VecFld_morpho"]["method"] == "Spateo"
        for key in ("align_spatial_rigid", "align_spatial_nonrigid"):
            ref = G[f"4_{m_}_slice{i}_{key}"]
            tol = mc.bound(G[f"4_{m_}_slice{i}_g_{key}"], G[f"4_{m_}_slice{i}_f32_{key}"], f32)
            dev = float(np.abs(aligned[i].obsm[key] - ref).max() / np.abs(ref).max())
            r = _ratio(tag, dtype, f"slice {i} {key}", dev, tol)
            print(f"  case {tag} {dtype} slice {i} {key}: {dev:.2e} / {tol:.2e} ({r:.2g}x)")
            if not dev <= tol:
                bad.append((i, key, dev, tol))
    assert not bad, bad


def test_P_above_the_cap_is_not_returned(monkeypatch):
    from spateo_amd import align

    A, B = mc.pair_samples(G, "1")
    m = align.Morpho_pairwise(A, B, dtype="float64", device=DEV, verbose=False, **mc.pair_kwargs(G, "1", max_iter=2))
    monkeypatch.setattr(align, "RETURN_P_MAX_ENTRIES", m.NA * m.NB - 1)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        P = m.run()
    assert P is None and m.P is None
    assert len([w for w in caught if "sparse_calculation_mode" in str(w.message)]) == 1
    assert np.isfinite(m.XAHat).all()
