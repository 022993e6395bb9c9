"""Shared by the CPU and GPU suites of the assignment step in ``sparse_calculation_mode`` (``mvf_assign_topk``,
``update_assignment(sparse_calculation_mode=True)`` and both loops): the cases of tests/golden/ref_assign_topk.npz,
ref_align_loop_topk.npz and ref_align_svi_topk.npz, a masked restatement, a NumPy stand-in of ``HipKernels.assign_topk``
and ONE checker.

The mode keeps, in every column j of ``P`` (tests/_assign_case.py), the k_eff = min(k, NA) largest entries - on equal values
the smaller row: the total order (value descending, row ascending).  ``K_NA``, ``K_NB``, ``Sp`` and ``PXB`` are formed from the
kept entries; ``K_NA_spatial``, ``K_NA_sigma2`` and ``sigma2_related`` stay the dense ones.

Within a column every entry carries a RELATIVE error (the exponent arguments reach ~700: _assign_case.F64_TOL), so whether two
candidates can be told apart is a matter of their relative gap (v_k - v_{k+1}) / v_k.  The checker compares the selected SETS
in the columns whose reference gap exceeds 1000 x the bound (the project's mutation factor) and holds every other column to
optimality within the bound; the sums are compared with the reference ``P`` masked by the selection UNDER TEST, so that a
near-tie that flips an entry cannot fail a sum it did not corrupt."""
import os

import numpy as np

import _align_svi_case as sc
import _assign_case as ac

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_assign_topk.npz")
GOLDEN_LOOP = os.path.join(HERE, "golden", "ref_align_loop_topk.npz")
GOLDEN_SVI = os.path.join(HERE, "golden", "ref_align_svi_topk.npz")
REF_TOL = 1e-12           # _assign_edge_cases.REF_TOL: the identities between the outputs
GAP_FACTOR = 1000.0       # _cell_cases.MUTATION_FACTOR
MAX_LEFT_OUT = 0.05       # of the columns: near ties the set comparison may leave out
SUMS = ("K_NA", "K_NB", "PXB")
_CACHE = {}


def load():
    if "g" not in _CACHE:
        _CACHE["g"] = np.load(GOLDEN)
    return _CACHE["g"]


def load_loop():
    if "l" not in _CACHE:
        _CACHE["l"] = np.load(GOLDEN_LOOP)
    return _CACHE["l"]


def load_svi():
    """The SVI loop in the mode (make_golden_align_svi_topk.py): the keys of ref_align_svi.npz, for _align_svi_case's
    case_inputs / deviations / bounds."""
    if "s" not in _CACHE:
        _CACHE["s"] = np.load(GOLDEN_SVI)
    return _CACHE["s"]


def case_keys(g=None):
    """[(case tag, k)] of the step goldens."""
    g = load() if g is None else g
    return [(str(t), int(k)) for t in g["cases"] for k in g[f"{t}_ks"]]


def golden_ref(g, tag, k):
    return {q: g[f"{tag}_k{k}_{q}"] for q in ac.QUANTITIES}


def golden_lists(g, tag, k):
    """(rows (NB, k_eff), vals (NB, k_eff)) of the reference's coo matrix, whose entries run column by column."""
    NB = len(g[f"{tag}_coordsB"])
    return g[f"{tag}_k{k}_row"].reshape(NB, -1), g[f"{tag}_k{k}_data"].reshape(NB, -1)


def tolerances(g, tag, k, dtype):
    """{quantity: bound}: float64 1e-10; float32 max(1.25 x the reference's own float32 floor of that quantity, 1e-5)."""
    if dtype == "float64":
        return {q: ac.F64_TOL for q in ac.QUANTITIES}
    floor = dict(zip([str(q) for q in g["quantities"]], g[f"{tag}_k{k}_floor_f32"]))
    return {q: max(ac.ALLOW * float(floor[q]), ac.F32_BASE) for q in ac.QUANTITIES}


# ---- the selection ------------------------------------------------------------------------------------------------------
def top_lists(P, k):
    """(rows (NB, k_eff) int32, vals (NB, k_eff)): per column the k_eff largest entries, value descending, row ascending."""
    P = np.asarray(P, dtype=np.float64)
    ke = min(int(k), P.shape[0])
    order = np.argsort(-P, axis=0, kind="stable")[:ke]        # stable: equal values keep their row order
    return order.T.astype(np.int32), np.take_along_axis(P, order, axis=0).T.copy()


def mask_of(rows, shape):
    m = np.zeros(shape, dtype=bool)
    m[np.asarray(rows, dtype=np.int64), np.arange(shape[1])[:, None]] = True
    return m


def masked_sums(P, rows, XB):
    """K_NA, K_NB, PXB of P restricted to the entries `rows` (NB, k_eff) selects."""
    Pm = np.where(mask_of(rows, P.shape), P, 0.0)
    return {"K_NA": Pm.sum(1), "K_NB": Pm.sum(0), "PXB": Pm.dot(XB)}


def restatement(*args, k, **kw):
    """The masked restatement: _assign_case.restatement(return_P=True), then the column-wise top-k mask.  Returns the
    QUANTITIES of _assign_case plus rows, vals and the dense P."""
    d = ac.restatement(*args, return_P=True, **kw)
    XB = np.asarray(args[1], dtype=np.float64)
    rows, vals = top_lists(d["P"], k)
    out = dict(d)
    out.update(masked_sums(d["P"], rows, XB))
    out["Sp"] = out["K_NB"].sum()
    out["rows"], out["vals"] = rows, vals
    return out


class CpuTopkKernels(sc.CpuLoopKernels):
    """CpuLoopKernels plus a NumPy `assign_topk`: the dense stand-in's P, masked."""

    def assign_topk(self, xa4, xb4, layers, model_mul, sigma2, s2v, outlier, k):
        a, _, _ = self.restated(xa4, xb4, layers, model_mul, sigma2, s2v, outlier, restatement=restatement, k=k)
        return self.assign_result(a, more=("rows", "vals"))


def cpu_topk_kernels(monkeypatch, D):
    """Route spateo_amd.align through CpuTopkKernels (spatial dimension D) for the rest of the test."""
    from spateo_amd import _runtime as rt

    sc.cpu_loop_kernels(monkeypatch, D)

    def make(device, dtype):
        k = CpuTopkKernels(device, dtype)
        k.D = D
        return k

    monkeypatch.setattr(rt, "_make_kernels", make)


# ---- the checker --------------------------------------------------------------------------------------------------------
def reference_gaps(P, k):
    """Per column of the reference P: (gap, all_zero).  gap = (v_k - v_{k+1}) / v_k, which the caller holds against its bound:
    1 where v_{k+1} = 0 < v_k or every row is kept, 0 where v_k = 0 (a tie among zeros, decided by the row alone)."""
    v = -np.sort(-P, axis=0)
    ke = min(k, P.shape[0])
    all_zero = ~P.any(0)
    if ke >= P.shape[0]:
        return np.ones(P.shape[1]), all_zero
    vk, vn = v[ke - 1], v[ke]
    gap = np.where(vn > 0, (vk - vn) / np.where(vk > 0, vk, 1.0), np.where(vk > 0, 1.0, 0.0))
    return gap, all_zero


def check(got, P_ref, XB, k, tol, sum_tols=None, what="", XB_ref=None):
    """The checker of a top-k result, every figure printed before the assertions.

    got: rows (NB, k_eff), vals (NB, k_eff), K_NA (NA,), K_NB (NB,), PXB (NA, D).  P_ref: the reference's dense P (NA, NB).
    XB: the coordinates PXB was formed with (NB, D) - in float32 mode the float32-stored ones; XB_ref: the reference's
    coordinates where they differ from XB (the unrounded ones), for the comparison with the masked reference.  tol: the bound of the entries (relative to max P) and of the selection;
    sum_tols: {K_NA, K_NB, PXB: bound against the reference P masked by got's selection} (default: tol).

    1  shapes, dtypes, rows in range and distinct per column, the order (value descending, row ascending on equal values);
    2  vals against P_ref at the returned positions;
    3  optimality: no kept entry's reference value lies below the largest non-kept one by more than tol x the column maximum;
    4  set equality with the reference in every column whose reference gap exceeds 1000 tol (an all-zero column: rows
       0 .. k_eff - 1); the share of columns left out is at most 5 %;
    5  consistency at REF_TOL: K_NA = the row sums of the returned entries, K_NB = their column sums in stored order, PXB =
       their product with XB; and the three against P_ref masked by got's own selection at sum_tols.
    Returns the figures."""
    P_ref, XB = np.asarray(P_ref, dtype=np.float64), np.asarray(XB, dtype=np.float64)
    NA, NB = P_ref.shape
    ke = min(int(k), NA)
    rows, vals = np.asarray(got["rows"]), np.asarray(got["vals"])
    sum_tols = {q: tol for q in SUMS} if sum_tols is None else sum_tols
    fig = {}
    # ---- 1
    assert rows.shape == (NB, ke) and vals.shape == (NB, ke), (what, rows.shape, vals.shape, (NB, ke))
    assert rows.dtype == np.int32 and vals.dtype == np.float64, (what, rows.dtype, vals.dtype)
    assert np.isfinite(vals).all(), what
    in_range = bool((rows >= 0).all() and (rows < NA).all())
    srt = np.sort(rows, axis=1)
    distinct = bool((np.diff(srt, axis=1) > 0).all())
    dv, dr = np.diff(vals, axis=1), np.diff(rows, axis=1)
    ordered = bool(((dv < 0) | ((dv == 0) & (dr > 0))).all())
    print(f"  {what}: rows in range {in_range}, distinct {distinct}, ordered {ordered}")
    assert in_range, (what, "a row index outside [0, NA)")
    assert distinct, (what, "a row twice in one column")
    assert ordered, (what, "a list that is not (value descending, row ascending)")
    # ---- 2
    cols = np.arange(NB)[:, None]
    top = float(P_ref.max())
    at = P_ref[rows.astype(np.int64), cols]
    fig["vals"] = float(np.abs(vals - at).max() / top) if top > 0 else float(np.abs(vals).max())
    # ---- 3
    kept = mask_of(rows, P_ref.shape)
    colmax = P_ref.max(0)
    if ke < NA:
        worst_kept = np.where(kept, P_ref, np.inf).min(0)
        best_left = np.where(kept, -np.inf, P_ref).max(0)
        short = (best_left - worst_kept) / np.where(colmax > 0, colmax, 1.0)
        fig["optimality"] = float(max(short.max(), 0.0))
    else:
        fig["optimality"] = 0.0
    # ---- 4
    gap, all_zero = reference_gaps(P_ref, ke)
    decidable = (gap > GAP_FACTOR * tol) | all_zero
    ref_rows, _ = top_lists(P_ref, ke)
    same_set = (srt == np.sort(ref_rows, axis=1)).all(1)
    fig["left_out"] = float(1.0 - decidable.mean())
    fig["sets_differ"] = int((decidable & ~same_set).sum())
    # ---- 5
    K_NA = np.zeros(NA)
    np.add.at(K_NA, rows.reshape(-1).astype(np.int64), vals.reshape(-1))
    PXB = np.zeros((NA, XB.shape[1]))
    np.add.at(PXB, rows.reshape(-1).astype(np.int64), vals.reshape(-1, 1) * np.repeat(XB, ke, axis=0))
    K_NB = np.zeros(NB)
    for p in range(ke):                                   # the stored order
        K_NB = K_NB + vals[:, p]
    own = {"K_NA": K_NA, "K_NB": K_NB, "PXB": PXB}
    ref = masked_sums(P_ref, rows, XB if XB_ref is None else np.asarray(XB_ref, dtype=np.float64))
    for q in SUMS:
        a = np.asarray(got[q], dtype=np.float64)
        assert a.shape == own[q].shape, (what, q, a.shape, own[q].shape)
        assert np.isfinite(a).all(), (what, q)
        for name, b in (("own", own[q]), ("ref", ref[q])):
            m = float(np.abs(b).max())
            fig[f"{q}_{name}"] = float(np.abs(a - b).max() / m) if m > 0 else float(np.abs(a).max())
    print(f"  {what}: " + ", ".join(f"{q} {v:.2e}" if isinstance(v, float) else f"{q} {v}" for q, v in fig.items()))
    assert fig["vals"] <= tol, (what, "vals", fig["vals"], tol)
    assert fig["optimality"] <= tol, (what, "a kept entry below a left-out one", fig["optimality"], tol)
    assert fig["left_out"] <= MAX_LEFT_OUT, (what, "too many near ties for the set comparison", fig["left_out"])
    assert fig["sets_differ"] == 0, (what, "the selected set differs from the reference's", np.nonzero(decidable & ~same_set)[0][:8])
    for q in SUMS:
        assert fig[f"{q}_own"] <= REF_TOL, (what, q, "against the returned entries", fig[f"{q}_own"])
        assert fig[f"{q}_ref"] <= sum_tols[q], (what, q, "against the masked reference", fig[f"{q}_ref"], sum_tols[q])
    return fig


def coo_lists(P, NB):
    """(rows, vals) (NB, k_eff) of a scipy.sparse.coo_matrix in the reference's layout; the layout itself is asserted."""
    ke = len(P.data) // NB
    assert len(P.data) == ke * NB and np.array_equal(P.col, np.repeat(np.arange(NB), ke))
    return np.asarray(P.row).reshape(NB, ke).astype(np.int32), np.asarray(P.data, dtype=np.float64).reshape(NB, ke)
