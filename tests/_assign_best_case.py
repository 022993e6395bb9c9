"""Shared by the CPU and GPU suites of the cell mapping from the fused assignment (``mvf_assign_best``,
``st.align.optimal_mapping``, ``optimal_mapping=True`` of both loops and of ``Morpho_pairwise``): the cases of
tests/golden/ref_assign_best.npz, a NumPy restatement of the two tie rules, a NumPy stand-in of ``HipKernels.assign_best`` and
ONE checker.

Per row i of ``P`` (and, with the sides exchanged, per column) the result is the maximum and two indices:

    nearest  the j first in (P_ij descending, |x_i - y_j|^2 ascending, j ascending)    mapping_aligned_coords(keep_all=False)
    first    the j first in (P_ij descending, j ascending)                             mapping_aligned_coords(keep_all=True)

Every entry of ``P`` carries a RELATIVE error (tests/_assign_topk_case.py), so whether the largest entry of a row can be told
from the runner-up is a matter of the relative gap (v_1 - v') / v_1, v' the largest value BELOW the maximum.  Where that gap
exceeds ``GAP_FACTOR`` x the bound the checker demands the reference's indices exactly - the rows whose maximum is attained
several times (exact ties: duplicated cells) and the all-zero rows (far cells) among them, where the rule alone decides; every
other row is held to optimality within the bound.  The constants are the project's: nothing is introduced here."""
import os

import numpy as np
import torch

import _assign_case as ac
import _assign_topk_case as tk
import _cpu_kernels as ck
from spateo_amd._kernels import Layer

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_assign_best.npz")
GAP_FACTOR = tk.GAP_FACTOR        # _cell_cases.MUTATION_FACTOR
MAX_LEFT_OUT = tk.MAX_LEFT_OUT    # of the rows / columns: near ties the index comparison may leave out
KEYS = ("rows", "row_values", "cols", "col_values")
_CACHE = {}


def load():
    if "g" not in _CACHE:
        with np.load(GOLDEN) as z:
            _CACHE["g"] = {k: z[k] for k in z.files}
    return _CACHE["g"]


def case_tags(g=None):
    g = load() if g is None else g
    return [str(t) for t in g["cases"]]


def case_inputs(g, tag):
    """(positional arguments, keyword arguments) of optimal_mapping (without keep_all) for one golden case; a label layer's
    arrays come back as int64 and the table as ``label_transfer``."""
    args, kw = ac.case_inputs(g, tag)
    LA, LB = list(args[2]), list(args[3])
    for l, met in enumerate(kw["dissimilarity"]):
        if met == "label":
            LA[l], LB[l] = LA[l].astype(np.int64), LB[l].astype(np.int64)
    if f"{tag}_label_transfer" in g:
        kw["label_transfer"] = g[f"{tag}_label_transfer"]
    return (args[0], args[1], LA, LB), kw


def tolerance(g, tag, dtype):
    """The bound of the entries, relative to max P: float64 1e-10; float32 max(1.25 x the reference's own float32 floor of
    P, 1e-5) - the rules of tests/_assign_case.py."""
    if dtype == "float64":
        return ac.F64_TOL
    return max(ac.ALLOW * float(g[f"{tag}_floor_f32"]), ac.F32_BASE)


def golden_mapping(g, tag, keep_all):
    """((pi_index, pi_value) by A, (pi_index, pi_value) by B) of the real mapping_aligned_coords."""
    k = "all" if keep_all else "nearest"
    return tuple((g[f"{tag}_{k}_{side}_index"].astype(np.int32), g[f"{tag}_{k}_{side}_value"]) for side in ("A", "B"))


# ---- the planted ties of the kernel-level tests -------------------------------------------------------------------------
TIE_SHAPE = (200, 300)    # 4 row tiles x 5 column tiles, every tile a split of its own in both directions


def tie_case():
    """_assign_edge_cases.make_case with zero_A / zero_B / dup, then the ties planted, for tests/test_gpu_assign_best_kernels.py
    (tests/test_assign_best_host.py proves on the CPU what the case holds).  dup: the first 6 near B cells are exact copies of
    their A cell, so each heads its A cell's row and is headed by it.  Three of them are copied on to the next lane, to
    another tile and to another split (columns), and their A cells likewise (rows) - with alpha and SigmaDiag, so that the
    entries tie.  Four far A cells, one per row tile, sit above B cells of the later column tiles: all-zero rows of P whose
    nearest partner is not column 0; the far B cells make_case moves away are the all-zero columns."""
    import _assign_edge_cases as ec

    na, nb = TIE_SHAPE
    c = ec.make_case("best-ties", na, nb, [("kl", "gauss", None, 20)], zero_A=(na - 1,), zero_B=(nb - 1,), dup=6, far="some",
                     sigma2=0.1)
    rng = np.random.default_rng(11)
    XA, XB, LA, LB = c["XA"], c["XB"], c["layers_A"][0], c["layers_B"][0]
    far = set(c["far"].tolist())
    groups_B, groups_A, taken_A, taken_B = [], [], set(), set()
    for n, j1 in enumerate(c["dup"][::2]):
        j1 = int(j1)
        i1 = int(np.flatnonzero((XA == XB[j1]).all(1))[0])       # the A cell column j1 copies
        copies_B = [j1 + 1, j1 + ec.TILE + 3 + n, j1 + 3 * ec.TILE + 17 + n]
        copies_A = [i1 + 1, (i1 + ec.TILE + 5 + n) % na, (i1 + 2 * ec.TILE + 9 + n) % na]
        if far & set(copies_B) or taken_B & set(copies_B + [j1]) or taken_A & set(copies_A + [i1]) or max(copies_B) >= nb \
                or i1 + 1 >= na or set(c["dup"].tolist()) & set(copies_B[1:]):
            continue
        XB[copies_B], LB[copies_B] = XB[j1], LB[j1]
        XA[copies_A], LA[copies_A] = XA[i1], LA[i1]
        c["alpha"][copies_A], c["SigmaDiag"][copies_A] = c["alpha"][i1], c["SigmaDiag"][i1]
        taken_B.update(copies_B + [j1]), taken_A.update(copies_A + [i1])
        groups_B.append(sorted([j1] + copies_B)), groups_A.append(sorted([i1] + copies_A))
    reach = np.sqrt(2 * c["sigma2"] * 800.0) + 2 * np.abs(XA).max() * np.sqrt(3)
    zero_rows = np.array([min(i for i in range(t * ec.TILE + 5, na) if i not in taken_A) for t in range(4)])
    near_late = np.array([j for j in range(2 * ec.TILE, nb) if j not in far and j not in taken_B])
    XA[zero_rows] = XB[near_late[:: len(near_late) // 4][:4]] + reach * (1.5 + rng.random((4, 1))) * np.eye(3)[1]
    c["zero_rows"], c["copies_B"], c["copies_A"] = zero_rows, groups_B, groups_A
    return c


# ---- the restatement ------------------------------------------------------------------------------------------------------
def _side(P, X, Y):
    """Per row of P (n, m): ((n, 2) int32 = nearest, first; (n,) maxima).  X (n, D) the rows' coordinates, Y (m, D)."""
    P = np.asarray(P, dtype=np.float64)
    top = P.max(1)
    cand = P == top[:, None]
    first = cand.argmax(1)
    nearest = first.copy()
    for i in np.flatnonzero(cand.sum(1) > 1):
        js = np.flatnonzero(cand[i])
        nearest[i] = js[np.argmin(((Y[js] - X[i]) ** 2).sum(1))]     # argmin: the smallest index among equal distances
    return np.stack([nearest, first], axis=1).astype(np.int32), top


def best_of(P, X, Y):
    """The two orders restated on a dense P (NA, NB) with the coordinates X (NA, D) and Y (NB, D): HipKernels.assign_best's
    dict as host arrays."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    rows, rv = _side(P, X, Y)
    cols, cv = _side(np.asarray(P).T, Y, X)
    return {"rows": rows, "row_values": rv, "cols": cols, "col_values": cv}


class CpuBestKernels(tk.CpuTopkKernels):
    """CpuTopkKernels plus a NumPy `assign_best`: best_of on the dense stand-in's P.  CALLS logs, in order, every assignment
    made through any instance - ("assign" | "assign_topk" | "assign_best", the operands and the state as host copies; for
    assign_best the dense P as well) - so that a test can see which assignment the mapping followed."""
    CALLS = []

    @staticmethod
    def _state(xa4, xb4, layers, model_mul, sigma2, s2v, outlier):
        return dict(xa4=ck._np(xa4).copy(), xb4=ck._np(xb4).copy(), b=[ck._np(Layer(*L).b).copy() for L in layers],
                    model_mul=ck._np(model_mul).copy(), sigma2=float(sigma2), s2v=float(s2v), outlier=float(outlier))

    def assign(self, xa4, xb4, layers, model_mul, sigma2, s2v, outlier, dense=False):
        self.CALLS.append(("assign", self._state(xa4, xb4, layers, model_mul, sigma2, s2v, outlier)))
        return super().assign(xa4, xb4, layers, model_mul, sigma2, s2v, outlier, dense=dense)

    def assign_topk(self, xa4, xb4, layers, model_mul, sigma2, s2v, outlier, k):
        self.CALLS.append(("assign_topk", self._state(xa4, xb4, layers, model_mul, sigma2, s2v, outlier)))
        return super().assign_topk(xa4, xb4, layers, model_mul, sigma2, s2v, outlier, k)

    def assign_best(self, xa4, xb4, layers, model_mul, sigma2, s2v, outlier, rows=True, cols=True):
        a, XA, XB = self.restated(xa4, xb4, layers, model_mul, sigma2, s2v, outlier, return_P=True)
        b = best_of(a["P"], XA, XB)
        self.CALLS.append(("assign_best", dict(self._state(xa4, xb4, layers, model_mul, sigma2, s2v, outlier), P=a["P"])))
        keep = (("rows", "row_values") if rows else ()) + (("cols", "col_values") if cols else ())
        return {q: torch.from_numpy(np.ascontiguousarray(b[q])) for q in keep}


def cpu_best_kernels(monkeypatch, D):
    """Route spateo_amd.align through CpuBestKernels (spatial dimension D) for the rest of the test."""
    from spateo_amd import _runtime as rt

    tk.cpu_topk_kernels(monkeypatch, D)
    del CpuBestKernels.CALLS[:]

    def make(device, dtype):
        k = CpuBestKernels(device, dtype)
        k.D = D
        return k

    monkeypatch.setattr(rt, "_make_kernels", make)


# ---- the checker ----------------------------------------------------------------------------------------------------------
def reference_gaps(P):
    """Per row of the reference P: (gap, tied).  gap = (v_1 - v') / v_1 with v' the largest value below the maximum v_1: 1
    where there is none (every entry equals the maximum - an all-zero row among them) or v' = 0; tied: the maximum is attained
    more than once."""
    P = np.asarray(P, dtype=np.float64)
    top = P.max(1)
    at_top = P == top[:, None]
    below = np.where(at_top, -np.inf, P).max(1) if P.shape[1] else np.full(len(P), -np.inf)
    safe = np.where(top > 0, top, 1.0)
    gap = np.where(np.isfinite(below) & (top > 0), (top - np.maximum(below, 0.0)) / safe, 1.0)
    return gap, at_top.sum(1) > 1


def check_side(idx, val, P, X, Y, tol, what=""):
    """One direction of a result against a reference P (n, m) whose ROWS are the cells of that direction (the caller hands
    P.T, and Y, X, for the columns), every figure printed before the assertions.

    1  shapes and dtypes; indices in [0, m);
    2  val against P at both returned indices, within tol x max P;
    3  optimality: no entry of the row exceeds the returned ones by more than tol x max P;
    4  both indices equal the restatement's in every row whose gap (reference_gaps) exceeds GAP_FACTOR x tol: the rule alone
       decides among the entries that equal the maximum (exact ties, all-zero rows);
    5  the share of rows left out by 4 is at most MAX_LEFT_OUT.
    Returns the figures."""
    P = np.asarray(P, dtype=np.float64)
    n, m = P.shape
    idx, val = np.asarray(idx), np.asarray(val)
    assert idx.shape == (n, 2) and val.shape == (n,), (what, idx.shape, val.shape, (n, m))
    assert idx.dtype == np.int32 and val.dtype == np.float64, (what, idx.dtype, val.dtype)
    assert np.isfinite(val).all(), what
    in_range = bool((idx >= 0).all() and (idx < m).all())
    print(f"  {what}: indices in range {in_range}")
    assert in_range, (what, "an index outside [0, m)")
    top = float(P.max())
    scale = top if top > 0 else 1.0
    rowmax = P.max(1)
    fig = {}
    at = np.stack([P[np.arange(n), idx[:, c].astype(np.int64)] for c in (0, 1)], axis=1)
    fig["value"] = float(np.abs(val[:, None] - at).max() / scale)
    fig["optimality"] = float((rowmax[:, None] - at).max() / scale)
    ref_idx, _ = _side(P, X, Y)
    gap, tied = reference_gaps(P)
    decidable = gap > GAP_FACTOR * tol
    differ = decidable & (idx != ref_idx).any(1)
    fig["left_out"] = float(1.0 - decidable.mean())
    fig["tied"], fig["zero"] = int((tied & decidable).sum()), int((rowmax == 0).sum())
    fig["differ"] = int(differ.sum())
    print(f"  {what}: " + ", ".join(f"{q} {v:.2e}" if isinstance(v, float) else f"{q} {v}" for q, v in fig.items()))
    assert fig["value"] <= tol, (what, "the value against P at the index", fig["value"], tol)
    assert fig["optimality"] <= tol, (what, "an entry above the returned one", fig["optimality"], tol)
    assert fig["differ"] == 0, (what, "indices differ from the reference's", np.flatnonzero(differ)[:8], idx[differ][:8],
                                ref_idx[differ][:8])
    assert fig["left_out"] <= MAX_LEFT_OUT, (what, "too many near ties for the index comparison", fig["left_out"])
    return fig


def check(best, P, X, Y, tol, what=""):
    """Both directions of HipKernels.assign_best's result (host arrays) against a reference P (NA, NB)."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    return {"rows": check_side(best["rows"], best["row_values"], P, X, Y, tol, what + " rows"),
            "cols": check_side(best["cols"], best["col_values"], np.asarray(P).T, Y, X, tol, what + " columns")}


def golden_best(g, tag):
    """The stored mappings of the real function (both keep_all) as a `best` dict."""
    (nA, vA), (nB, vB) = golden_mapping(g, tag, False)
    (fA, _), (fB, _) = golden_mapping(g, tag, True)
    return {"rows": np.stack([nA[:, 1], fA[:, 1]], axis=1).astype(np.int32), "row_values": vA,
            "cols": np.stack([nB[:, 0], fB[:, 0]], axis=1).astype(np.int32), "col_values": vB}


def check_golden_indices(best, P, g, tag, tol, what=""):
    """The real function's stored indices against a result, wherever both the reference's own P (its stored gaps) and P decide
    them at GAP_FACTOR x tol; at most MAX_LEFT_OUT of the rows / columns are left out."""
    gold = golden_best(g, tag)
    for side, Q in (("rows", np.asarray(P)), ("cols", np.asarray(P).T)):
        gap, _ = reference_gaps(Q)
        decided = (gap > GAP_FACTOR * tol) & (g[f"{tag}_gap_{side}"].astype(np.float64) > GAP_FACTOR * tol)
        print(f"  {what} {side}: {int(decided.sum())} of {len(decided)} decided, {int((best[side][decided] != gold[side][decided]).any(1).sum())} differ")
        assert decided.mean() >= 1.0 - MAX_LEFT_OUT, (what, side, decided.mean())
        assert np.array_equal(best[side][decided], gold[side][decided]), (what, side)
    return gold


def best_from_mappings(by_nearest, by_first):
    """The raw `best` dict from two results of optimal_mapping (keep_all False, True): what the checker reads."""
    (nA, nB), (fA, fB) = by_nearest, by_first
    assert np.array_equal(nA["pi_value"], fA["pi_value"]) and np.array_equal(nB["pi_value"], fB["pi_value"])
    return {"rows": np.stack([nA["pi_index"][:, 1], fA["pi_index"][:, 1]], axis=1).astype(np.int32), "row_values": nA["pi_value"],
            "cols": np.stack([nB["pi_index"][:, 0], fB["pi_index"][:, 0]], axis=1).astype(np.int32), "col_values": nB["pi_value"]}
