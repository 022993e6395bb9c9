"""``sparse_calculation_mode`` of the alignment on ``cuda:0`` through the public functions - ``update_assignment``,
``morpho_iterate``, ``morpho_iterate_svi`` with ``sparse_calculation_mode=True`` - against goldens of the real reference code in
that mode (tests/golden/ref_assign_topk.npz, ref_align_loop_topk.npz, ref_align_svi_topk.npz) in both cell dtypes: float64 at
1e-10 (the loops: 1e-10 max(1, 1.25 g_k)), float32 at max(1.25 x the reference's own float32 floor, 1e-5 (the loops: 1e-5 max(1,
1.25 g_k))) - the bounds of tests/test_gpu_assign.py, test_gpu_align_loop.py and test_gpu_align_svi.py.  The selection
itself goes through ``_assign_topk_case.check`` against the formula restatement's dense P.  Two calls give equal bits."""
import numpy as np
import pytest
import torch

import _align_loop_case as lc
import _align_svi_case as sc
import _assign_case as ac
import _assign_topk_case as tk

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = ["float64", "float32"]
G = tk.load()
API_KEYS = [(t, k) for t, k in tk.case_keys(G) if k <= 64]   # (a k above the cap is refused: tests/test_assign_topk_host.py)


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag,k", API_KEYS)
def test_update_assignment_against_the_reference_goldens(dtype, tag, k):
    from spateo_amd import align

    args, kw = ac.case_inputs(G, tag)
    NA, NB = len(args[0]), len(args[1])
    got = align.update_assignment(*args, dtype=dtype, device=DEV, sparse_calculation_mode=True, sparse_top_k=k, **kw)
    tols = tk.tolerances(G, tag, k, dtype)
    ac.check(got, tk.golden_ref(G, tag, k), tols, f"update_assignment {tag} k {k} {dtype}")
    rows, vals = tk.coo_lists(got["P"], NB)
    assert got["P"].shape == (NA, NB) and np.array_equal(rows, got["topk_rows"]) and np.array_equal(vals, got["topk_values"])
    dense = ac.restatement(*args, return_P=True, **kw)
    tol = ac.F64_TOL if dtype == "float64" else tols["K_NB"]
    stored = np.asarray(args[1], dtype=np.float64).astype(dtype).astype(np.float64)   # coordsB as the device holds it
    tk.check(dict(rows=rows, vals=vals, K_NA=got["K_NA"], K_NB=got["K_NB"], PXB=got["PXB"]), dense["P"], stored, k, tol,
             sum_tols={q: tols[q] for q in tk.SUMS}, what=f"update_assignment {tag} k {k} {dtype}", XB_ref=args[1])
    far = G[f"{tag}_far"]
    assert not got["K_NB"][far].any() and not got["topk_values"][far].any()
    again = align.update_assignment(*args, dtype=dtype, device=DEV, sparse_calculation_mode=True, sparse_top_k=k, **kw)
    for q in ac.QUANTITIES + ("topk_rows", "topk_values"):
        assert np.asarray(got[q]).tobytes() == np.asarray(again[q]).tobytes(), q


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag", lc.case_tags())
def test_morpho_iterate_against_the_reference_loop(dtype, tag):
    from spateo_amd import align

    L = tk.load_loop()
    args, kw = lc.case_inputs(lc.load(), tag)
    NA, NB = len(args[0]), len(args[1])
    out = align.morpho_iterate(*args, dtype=dtype, device=DEV, record="arrays", sparse_calculation_mode=True,
                               sparse_top_k=int(L["top_k"]), **kw)
    got = dict(out["history"], optimal_R=out["optimal_R"], optimal_t=out["optimal_t"])
    f32 = dtype == "float32"
    tol = lc.bounds(L, tag, lc.F32_BASE if f32 else lc.F64_TOL, f32=f32)
    lc.check(lc.deviations(got, L, tag), tol, f"case {tag} top-k loop {dtype}")
    rows, vals = tk.coo_lists(out["P"], NB)
    assert out["P"].shape == (NA, NB) and rows.shape == (NB, 16)
    assert np.abs(np.asarray(out["P"].sum(1)).ravel() - out["K_NA"]).max() <= tk.REF_TOL * out["K_NA"].max()
    assert np.abs(vals.sum(1) - out["K_NB"]).max() <= tk.REF_TOL * out["K_NB"].max()
    if dtype == "float64":   # (gap >= 1e-7 in every iteration: the selection is the reference's)
        grow, gval = L[f"{tag}_P_row"].reshape(NB, 16), L[f"{tag}_P_data"].reshape(NB, 16)
        assert np.array_equal(rows[gval > 0], grow[gval > 0])
        assert np.abs(vals - gval).max() <= float(tol["K_NA"][-1]) * gval.max()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag", sc.case_tags(tk.load_svi()))
def test_morpho_iterate_svi_against_the_reference_loop(dtype, tag):
    from spateo_amd import align

    S = tk.load_svi()
    args, kw = sc.case_inputs(S, tag)
    NA, NB = len(args[0]), len(args[1])
    out = align.morpho_iterate_svi(*args, dtype=dtype, device=DEV, record="arrays", return_mapping=True,
                                   sparse_calculation_mode=True, sparse_top_k=int(S["top_k"]), **kw)
    got = dict(out["history"], optimal_R_map=out["optimal_R"], optimal_t_map=out["optimal_t"], Sp_map=out["Sp"])
    f32 = dtype == "float32"
    tol = sc.bounds(S, tag, sc.F32_BASE if f32 else sc.F64_TOL, f32=f32, finals=sc.FINALS_MAP)
    sc.check(sc.deviations(got, S, tag, sc.FINALS_MAP), tol, f"case {tag} top-k SVI loop {dtype}")
    rows, vals = tk.coo_lists(out["P"], NB)
    assert out["P"].shape == (NA, NB) and rows.shape == (NB, 16) and len(out["K_NB"]) == NB
    assert np.abs(vals.sum(1) - out["K_NB"]).max() <= tk.REF_TOL * out["K_NB"].max()
    if dtype == "float64":
        grow, gval = S[f"{tag}_P_row"].reshape(NB, 16), S[f"{tag}_P_data"].reshape(NB, 16)
        assert np.array_equal(rows[gval > 0], grow[gval > 0])
