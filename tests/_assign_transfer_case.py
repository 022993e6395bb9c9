"""Shared by the CPU and GPU suites of the assignment applied to cell features (``mvf_assign_apply``,
``align.apply_assignment``): the cases of tests/golden/ref_assign_transfer.npz (inputs: tests/golden/ref_assign.npz), a NumPy
restatement of the four quantities, the comparison helper and two stated wrong kernels.  No GPU and no torch.

With P the dense assignment (tests/_assign_case.py), K_NA / K_NB its row / column sums, F_B (NB, C) and F_A (NA, C):

    to_A_raw = P @ F_B      to_A_norm[i] = to_A_raw[i] / K_NA[i]      (a cell whose sum is 0 keeps a zero row)
    to_B_raw = P.T @ F_A    to_B_norm[j] = to_B_raw[j] / K_NB[j]

Deviations: the raw products relative to max (P @ |F|), the normalised ones relative to max |F| over EVERY cell with a non-zero
sum.  Bounds (the project's): float64 F64_TOL = 1e-10; float32 at the API max(1.25 x the reference's own float32 floor, 1e-5).
"""
import os

import numpy as np

import _assign_case as ac
import _assign_edge_cases as ec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_assign_transfer.npz")
QUANTITIES = ("to_A_raw", "to_A_norm", "to_B_raw", "to_B_norm")
F64_TOL, F32_BASE, ALLOW = ac.F64_TOL, ac.F32_BASE, ac.ALLOW
CHUNK, BLOCK = 64, 16          # feature columns per sweep, per MFMA column block


def load():
    return np.load(GOLDEN)


def cases(g):
    """[(tag, C)] of the golden file."""
    return [(str(t), int(c)) for t in g["cases"] for c in g[f"{t}_widths"]]


def features(g, tag, c):
    return g[f"{tag}_c{c}_F_A"], g[f"{tag}_c{c}_F_B"]


def golden_ref(g, tag, c):
    out = {q: g[f"{tag}_c{c}_{q}"] for q in QUANTITIES}
    out.update(K_NA=g[f"{tag}_K_NA"], K_NB=g[f"{tag}_K_NB"], scale=dict(zip(QUANTITIES, g[f"{tag}_c{c}_scale"])))
    return out


def normalized(M, K):
    out = np.zeros_like(M)
    live = np.asarray(K) != 0
    out[live] = M[live] / np.asarray(K)[live, None]
    return out


def products(P, F_A=None, F_B=None):
    """The reference of a dense P: the quantities of the directions whose features are given, K_NA, K_NB and the scales."""
    P = np.asarray(P, dtype=np.float64)
    out = {"K_NA": P.sum(1), "K_NB": P.sum(0), "scale": {}}
    if F_B is not None:
        out["to_A_raw"] = P @ F_B
        out["to_A_norm"] = normalized(out["to_A_raw"], out["K_NA"])
        out["scale"].update(to_A_raw=float((P @ np.abs(F_B)).max()), to_A_norm=float(np.abs(F_B).max()))
    if F_A is not None:
        out["to_B_raw"] = P.T @ F_A
        out["to_B_norm"] = normalized(out["to_B_raw"], out["K_NB"])
        out["scale"].update(to_B_raw=float((P.T @ np.abs(F_A)).max()), to_B_norm=float(np.abs(F_A).max()))
    return out


def quantities_of(raw, norm=None):
    """apply_assignment's results (normalize=False, and optionally normalize=True) under the names of QUANTITIES."""
    out = {f"{q}_raw": raw[q] for q in ("to_A", "to_B") if q in raw}
    if norm is not None:
        out.update({f"{q}_norm": norm[q] for q in ("to_A", "to_B") if q in norm})
    return out


def deviations(got, ref):
    """{quantity: max |got - ref| / scale} over the quantities in `got`; shapes, dtype and finiteness asserted on the way."""
    dev = {}
    for q in QUANTITIES:
        if q not in got:
            continue
        a, b = np.asarray(got[q]), np.asarray(ref[q])
        assert a.shape == b.shape and a.dtype == np.float64, (q, a.shape, b.shape, a.dtype)
        assert np.isfinite(a).all(), q
        K = ref["K_NA"] if q.startswith("to_A") else ref["K_NB"]
        if q.endswith("norm"):
            assert not a[K == 0].any(), f"{q}: a cell without partners must keep a zero row"
            a, b = a[K != 0], b[K != 0]          # every cell with a non-zero sum, none left out
        dev[q] = float(np.abs(a - b).max() / ref["scale"][q]) if a.size else 0.0
    return dev


def tolerances(g, tag, c, dtype):
    if dtype == "float64":
        return {q: F64_TOL for q in QUANTITIES}
    floor = dict(zip(QUANTITIES, g[f"{tag}_c{c}_floor_f32"]))
    return {q: max(ALLOW * float(floor[q]), F32_BASE) for q in QUANTITIES}


def check(got, ref, tols, what=""):
    """Print every figure, then assert; returns the deviations."""
    dev = deviations(got, ref)
    print(f"  {what}: " + ", ".join(f"{q} {v:.2e}" for q, v in dev.items()))
    for q, v in dev.items():
        assert v <= tols[q], (what, q, v, tols[q])
    return dev


def mutations(P, F_A, F_B):
    """[(name, quantities)]: two stated wrong kernels - the rows of F permuted inside one 16-row block (an operand fed to the
    matrix unit in the wrong lane order), and the last 64-column chunk dropped."""
    def rows_permuted(F):
        F = F.copy()
        lo = BLOCK if len(F) >= 2 * BLOCK else 0
        hi = min(lo + BLOCK, len(F))
        F[lo:hi] = F[lo:hi][::-1]
        return F

    out = [("rows of F permuted inside one 16-row block", products(P, rows_permuted(F_A), rows_permuted(F_B)))]
    if F_A.shape[1] > CHUNK:
        dropped = products(P, F_A, F_B)
        for q in QUANTITIES:
            dropped[q] = dropped[q].copy()
            dropped[q][:, (F_A.shape[1] - 1) // CHUNK * CHUNK:] = 0.0
        out.append(("the last 64-column chunk dropped", dropped))
    return out


def apply_width(c):
    return BLOCK * min(CHUNK // BLOCK, ec.cdiv(c, BLOCK))


def workspace_bytes(na, nb, cb, ca):
    """mvf_assign_apply's workspace: pass 1's partials and the factors (mvf_assign's first two blocks), K_NB, the sweeps'
    partial products (the larger direction's: splits x padded cells x padded chunk width) and the partial K_NA; float64, each
    block rounded up to 256 bytes."""
    rt, ct, rs, cs = ec.plan(na, nb)
    up = lambda n: ec.cdiv(8 * n, 256) * 256  # noqa: E731
    part = max(cs * rt * ec.TILE * apply_width(cb), rs * ct * ec.TILE * apply_width(ca))
    return up(rs * 4 * ct * ec.TILE) + up(4 * ct * ec.TILE) + up(ct * ec.TILE) + up(part) + up(cs * rt * ec.TILE)
