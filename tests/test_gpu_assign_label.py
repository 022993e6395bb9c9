"""The ``"label"`` layer of the alignment on ``cuda:0`` through the public functions - ``update_assignment`` (dense, ``return_P``,
``sparse_calculation_mode``), ``morpho_iterate`` and ``morpho_iterate_svi`` with ``label_transfer=`` - in both cell dtypes against
goldens of the real reference code run with a label layer (tests/golden/make_golden_assign_label.py).

Bounds, relative to each quantity's maximum - those of tests/test_gpu_assign.py, test_gpu_assign_topk.py, test_gpu_align_loop.py
and test_gpu_align_svi.py: the step in float64 1e-10, in float32 max(1.25 x the reference's own float32 floor of that quantity,
1e-5); the loops 1e-10 max(1, 1.25 g_k) and max(1.25 x the reference's own float32 floor, 1e-5 max(1, 1.25 g_k)), ``Coff`` in
float64 only.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import _align_loop_case as lc
import _align_svi_case as sc
import _assign_case as ac
import _assign_label_case as lab
import _assign_topk_case as tk

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = ["float64", "float32"]
G = lab.load()
_REST = {}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def _run(tag, dtype, **extra):
    from spateo_amd import align

    args, kw = lab.case_inputs(G, tag)
    return align.update_assignment(*args, dtype=dtype, device=DEV, **kw, **extra)


def _dense_restatement(tag):
    if tag not in _REST:
        args, kw = lab.case_inputs(G, tag)
        _REST[tag] = lab.restatement(*args, return_P=True, **kw)
    return _REST[tag]


# ---- the step ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag", lab.case_tags(G))
def test_every_golden_case_every_quantity(tag, dtype):
    """a: the label layer alone; b / c: kl + label in both orders; d / e: gauss / cos on the label layer; f: D = 2; z: a table
    with zeros.  Every case has its far columns."""
    got = _run(tag, dtype)
    ac.check(got, lab.golden_ref(G, tag), lab.tolerances(G, tag, dtype), f"case {tag} {dtype}")
    far = lab.far_columns(G, tag)
    assert len(far) >= 0.05 * len(got["K_NB"]) and np.all(got["K_NB"][far] == 0.0)
    for q, v in got.items():
        assert np.isfinite(v).all(), (tag, q)


@pytest.mark.parametrize("dtype", DTYPES)
def test_label_layer_alone_dense_P(dtype):
    """NA = 149, NB = 117, K = 5, L = 4: the dense P against the reference's; a transposed table cannot pass."""
    got = _run("a", dtype, return_P=True)
    P = G["a_P"]
    assert got["P"].shape == P.shape == (149, 117) and got["P"].dtype == np.float64
    err = float(np.abs(got["P"] - P).max() / P.max())
    tol = ac.F64_TOL if dtype == "float64" else max(ac.ALLOW * float(G["a_floor_f32"].max()), ac.F32_BASE)
    print(f"  dense P {dtype}: {err:.2e} (bound {tol:.2e})")
    assert err <= tol
    assert np.all(got["P"][:, lab.far_columns(G, "a")] == 0.0)
    assert np.abs(got["P"].sum(1) - got["K_NA"]).max() <= 1e-12 * got["K_NA"].max()
    assert np.abs(got["P"].sum(0) - got["K_NB"]).max() <= 1e-12 * got["K_NB"].max()
    plain = _run("a", dtype)
    for q in ac.QUANTITIES:
        assert np.array_equal(plain[q], got[q]), q


@pytest.mark.parametrize("dtype", DTYPES)
def test_columns_without_any_transfer_are_exactly_zero(dtype):
    got = _run("z", dtype, return_P=True)
    dead, rare = G["z_dead_columns"], G["z_rare_columns"]
    assert len(dead) and np.all(got["P"][:, dead] == 0.0) and np.all(got["K_NB"][dead] == 0.0)
    assert np.all(got["K_NB"][rare] > 0.0) and np.isfinite(got["P"]).all()
    ref = _dense_restatement("z")["P"]
    assert np.array_equal(got["P"] > 0, ref > 0)        # the zeros of the table are the zeros of P, entry by entry


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_are_bit_identical(dtype):
    for tag in ("c", "z"):
        r1, r2 = _run(tag, dtype), _run(tag, dtype)
        for q in ac.QUANTITIES:
            assert np.array_equal(r1[q], r2[q]), (tag, q)


# ---- sparse_calculation_mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [int(k) for k in G["z_ks"]])
def test_top_k_with_a_label_layer(dtype, k):
    """Case z, k = 1, 8, 64: values and sums as tests/test_gpu_assign_topk.py compares them; the row indices against the
    reference's only where the kept value is positive and the column's tie gap is not zero (the zeros of the table tie
    exactly at 0, and the reference's sort breaks such ties as it likes).  The rare columns have fewer than 64 positive
    entries."""
    args, kw = lab.case_inputs(G, "z")
    NA, NB = len(args[0]), len(args[1])
    got = _run("z", dtype, sparse_calculation_mode=True, sparse_top_k=k)
    tols = lab.tolerances(G, "z", dtype, k)
    ac.check(got, lab.golden_ref(G, "z", k), tols, f"update_assignment z k {k} {dtype}")
    rows, vals = tk.coo_lists(got["P"], NB)
    assert got["P"].shape == (NA, NB) and np.array_equal(rows, got["topk_rows"]) and np.array_equal(vals, got["topk_values"])
    tol = ac.F64_TOL if dtype == "float64" else tols["K_NB"]
    stored = np.asarray(args[1], dtype=np.float64).astype(dtype).astype(np.float64)
    tk.check(dict(rows=rows, vals=vals, K_NA=got["K_NA"], K_NB=got["K_NB"], PXB=got["PXB"]), _dense_restatement("z")["P"], stored,
             k, tol, sum_tols={q: tols[q] for q in tk.SUMS}, what=f"update_assignment z k {k} {dtype}", XB_ref=args[1])
    grow, gval = G[f"z_k{k}_row"].reshape(NB, k).astype(np.int32), G[f"z_k{k}_data"].reshape(NB, k)
    gap = G[f"z_k{k}_colgap"]        # (its smallest non-zero value is 1.6e-3: no float32 rounding of a coordinate moves a row)
    decided = (gval > 0) & (gap > 0)[:, None]
    print(f"  rows compared in {int(decided.any(1).sum())} of {NB} columns")
    assert decided.any() and np.array_equal(rows[decided], grow[decided])
    assert np.abs(vals - gval).max() <= tol * gval.max()
    if k == 64:
        few = (gval[G["z_rare_columns"]] > 0).sum(1)
        assert few.max() < k and np.array_equal((vals[G["z_rare_columns"]] > 0).sum(1), few)
    far = lab.far_columns(G, "z")
    assert not got["K_NB"][far].any() and not got["topk_values"][far].any()
    again = _run("z", dtype, sparse_calculation_mode=True, sparse_top_k=k)
    for q in ac.QUANTITIES + ("topk_rows", "topk_values"):
        assert np.asarray(got[q]).tobytes() == np.asarray(again[q]).tobytes(), q


# ---- the loops -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_morpho_iterate_with_a_label_layer(dtype):
    from spateo_amd import align

    V = lab.View(G, "loop.")
    args, kw = lab.loop_inputs(G)
    out = align.morpho_iterate(*args, dtype=dtype, device=DEV, record="arrays", **kw)
    got = dict(out["history"], optimal_R=out["optimal_R"], optimal_t=out["optimal_t"])
    f32 = dtype == "float32"
    tol = lc.bounds(V, "L", lc.F32_BASE if f32 else lc.F64_TOL, f32=f32, skip=("Coff",) if f32 else ())
    ratio = lc.check(lc.deviations(got, V, "L"), tol, f"label loop {dtype}")
    assert max(ratio.values()) <= 1.0 and len(out["history"]["Sp"]) == 12
    assert abs(out["sigma2_variance"] - float(V["L_sigma2_variance"])) <= 1e-12 * out["sigma2_variance"]
    assert out["vecfld"]["dissimilarity"] == ["kl", "label"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_morpho_iterate_svi_with_a_label_layer(dtype):
    """30 iterations of 150-cell batches from the stored batch_perm: the batches carry the B labels."""
    from spateo_amd import align

    V = lab.View(G, "svi.")
    args, kw = lab.svi_inputs(G)
    assert kw["max_iter"] == 30 and kw["batch_size"] == 150
    out = align.morpho_iterate_svi(*args, dtype=dtype, device=DEV, record="arrays", **kw)
    got = dict(out["history"], optimal_R=out["optimal_R"], optimal_t=out["optimal_t"])
    f32 = dtype == "float32"
    tol = sc.bounds(V, "S", sc.F32_BASE if f32 else sc.F64_TOL, f32=f32, skip=("Coff",) if f32 else ())
    ratio = sc.check(sc.deviations(got, V, "S"), tol, f"label SVI loop {dtype}")
    assert max(ratio.values()) <= 1.0
    np.testing.assert_array_equal(out["history"]["step_size"], V["S_step_size"])
    assert len(out["K_NB"]) == 150
    # return_mapping: the closing full assignment reads the label layer of the whole slice
    full = align.morpho_iterate_svi(*args, dtype=dtype, device=DEV, record=False, return_mapping=True, **kw)
    got = dict(optimal_R_map=full["optimal_R"], optimal_t_map=full["optimal_t"], Sp_map=full["Sp"])
    tol = sc.bounds(V, "S", sc.F32_BASE if f32 else sc.F64_TOL, f32=f32, finals=sc.FINALS_MAP)
    tol = {q: tol[q] for q in sc.FINALS_MAP}
    dev = {q: lc.rel(np.asarray(got[q], dtype=np.float64)[None], V[f"S_{q}"][None]) for q in sc.FINALS_MAP}
    sc.check(dev, tol, f"label SVI loop {dtype} return_mapping")
    assert len(full["K_NB"]) == len(args[1]) and np.array_equal(full["XAHat"], out["XAHat"])
