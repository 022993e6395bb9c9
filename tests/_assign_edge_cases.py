"""Shared by tests/test_assign_kernel_refs.py (CPU) and tests/test_gpu_assign_kernels.py (GPU): inputs, case lists and
plain NumPy references for the kernels of ``csrc/mvf_assign.hip`` at the edges of their tiling.  No GPU and no torch.

Two references, both test infrastructure written from DESIGN.md section 4 (not from the kernel's text):

* ``prepare_reference`` states ``mvf_assign_prepare``: the operand X' / Y' as the cell dtype stores it, zero-padded to ld, and
  a / b in float64, rounded where the kernel rounds.
* ``pair_reference`` states the pairwise stage in product form on PREPARED operands, d = a_i + b_j - s <X'_i, Y'_j>.  Fed
  with the operands a device wrote it has the device's inputs exactly, so float32 mode (float64 arithmetic on
  float32-stored operands) can be held to the float64 bound.

Tiling constants of the kernel: tile 64, wave block 32, MFMA block 16, k-step 16, prepare lane stride 64, at most 64 splits,
1024 workgroups aimed at.  The case lists below are data; tests/test_assign_kernel_refs.py proves what they cover.
"""
import functools
import zlib

import numpy as np

TILE, WAVE_BLOCK, MFMA_BLOCK, KSTEP, LANES = 64, 32, 16, 16, 64
MAX_SPLITS, TARGET_WGS, MAX_LAYERS = 64, 1024, 4
EPS = 1e-8
METRICS = {"euc": 0, "square_euc": 1, "kl": 2, "sym_kl": 3, "cos": 4}   # include/mvf.h
PROBS = {"gauss": 0, "cos": 1, "prob": 2}
RAW = ("K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2", "PXB", "scalar")  # what mvf_assign writes; "P": mvf_assign_dense

REF_TOL = 1e-12          # product form against the formula restatement and against long double; the identities
PREP_F64_TOL = 1e-13     # prepared float64 operands: a <= 2000-term positive sum in another order + 1 - 2 ulp log / sqrt: ~5e-15
PREP_F32_FRACTION = 1e-3  # float32 operands: one float32 ulp in at most this fraction of the elements
DENSE_MAX_ENTRIES = 1 << 20   # pair_reference returns the dense P up to this many entries
MUTATION_SHIFT = 1e-7    # _cell_cases.MUTATION_FACTOR (1000) x _assign_case.F64_TOL (1e-10)


def cdiv(a, b):
    return -(-a // b)


def padded_features(g, metric):
    return cdiv(2 * g if metric == "sym_kl" else g, KSTEP) * KSTEP


def plan(na, nb):
    """(row tiles, column tiles, row splits, column splits) of a call: pass 1 splits the rows of a column panel, pass 2 the
    columns of a row panel, over at most 64 workgroups each, aiming at 1024 workgroups per pass."""
    rt, ct = cdiv(na, TILE), cdiv(nb, TILE)
    return rt, ct, max(1, min(rt, MAX_SPLITS, cdiv(TARGET_WGS, ct))), max(1, min(ct, MAX_SPLITS, cdiv(TARGET_WGS, rt)))


def workspace_bytes(na, nb):
    """Pass-1 partials (splits x 4 x padded columns), factors (4 per padded column), pass-2 partials (splits x padded rows x
    8), one value per padded row; float64, each block rounded up to 256 bytes."""
    rt, ct, rs, cs = plan(na, nb)
    up = lambda n: cdiv(8 * n, 256) * 256  # noqa: E731
    return up(rs * 4 * ct * TILE) + up(4 * ct * TILE) + up(cs * rt * TILE * 8) + up(rt * TILE)


def split_tiles(tiles, splits, y):
    """The tiles split y of `splits` takes: [tiles y / splits, tiles (y + 1) / splits)."""
    return tiles * y // splits, tiles * (y + 1) // splits


# ------------------------------------------------------------------------------------------------------ references
def _lane_sum(v):
    """Row sums as one wave forms them: 64 interleaved partials (lane l takes k = l, l + 64, ...), then a pairwise tree."""
    n, g = v.shape
    part = np.zeros((n, LANES))
    for k0 in range(0, g, LANES):
        w = min(LANES, g - k0)
        part[:, :w] += v[:, k0:k0 + w]
    while part.shape[1] > 1:
        h = part.shape[1] // 2
        part = part[:, :h] + part[:, h:]
    return part[:, 0]


def prepare_reference(layer, metric, side, dtype, lane_order=False):
    """mvf_assign_prepare in NumPy: (X' (side 0) or Y' (side 1) in `dtype`, (n, ld), pad features zero; a or b, float64).
    `lane_order`: the row totals summed as 64 interleaved partials and a tree instead of NumPy's order."""
    x = np.asarray(layer, dtype=np.float64)
    n, g = x.shape
    T = np.dtype(dtype).type
    rowsum = _lane_sum if lane_order else (lambda v: v.sum(1))
    out = np.zeros((n, padded_features(g, metric)), dtype=T)
    if metric in ("euc", "square_euc"):     # cast first; |x|^2 of the cast values, on both sides
        out[:, :g] = x.astype(T)
        w = out[:, :g].astype(np.float64)
        ab = rowsum(w * w)
    elif metric == "cos":                   # divided in float64, then cast; the norm floored at 1e-8
        nrm = np.maximum(np.sqrt(rowsum(x * x)), EPS)
        out[:, :g] = (x / nrm[:, None]).astype(T)
        ab = np.full(n, 0.5 if side == 0 else 0.0)
    elif metric in ("kl", "sym_kl"):        # p cast, log(p + 1e-8) of the cast p, a / b from cast p x float64 log
        tot = rowsum(x + 0.01)
        p = ((x + 0.01) / tot[:, None]).astype(T)
        lp = np.log(p.astype(np.float64) + EPS)
        e = rowsum(p.astype(np.float64) * lp)
        first, second = (p, lp.astype(T)) if side == 0 else (lp.astype(T), p)   # A: [p, log p]; B: [log q, q]
        out[:, :g] = first
        if metric == "sym_kl":
            out[:, g:2 * g] = second
            ab = 0.5 * e
        else:
            ab = e if side == 0 else np.zeros(n)
    else:
        raise ValueError(metric)
    return out, np.asarray(ab, dtype=np.float64)


def prepare_layers(case, dtype):
    """[(X', Y', a, b, metric, prob, param)] of a case from prepare_reference."""
    out = []
    for A, B, met, kind, par in zip(case["layers_A"], case["layers_B"], case["dissimilarity"], case["probability_type"],
                                    case["probability_parameters"]):
        Xp, a = prepare_reference(A, met, 0, dtype)
        Yp, b = prepare_reference(B, met, 1, dtype)
        out.append((Xp, Yp, a, b, met, kind, par))
    return out


def stored_coords(X, dtype):
    """(n, 3) float64: the coordinates as the cell dtype holds them, zero-padded to 3-D."""
    X = np.asarray(X, dtype=np.float64)
    out = np.zeros((len(X), 3))
    out[:, :X.shape[1]] = X.astype(dtype).astype(np.float64)
    return out


def raw_scalars(case):
    """(model_mul, spatial_outlier) as update_assignment forms them (_assign_case: m_i and o)."""
    NA, D = case["XA"].shape
    s2, gamma = case["sigma2"], case["gamma"]
    return (case["alpha"] * np.exp(-case["SigmaDiag"] / s2),
            float(np.power(2 * np.pi * s2, D / 2) * (1 - gamma) / (gamma * (case["samples_s"] * NA))))


def pair_reference(xa_stored, xb_stored, layers, model_mul, sigma2, sigma2_variance, outlier, xp=np.float64, tweak=None,
                   chunk_entries=1 << 21):
    """The pairwise stage on prepared operands, in `xp` arithmetic (np.float64 or np.longdouble).

    xa_stored (NA, >= 3), xb_stored (NB, >= 3): stored coordinates; layers: [(X', Y', a, b, metric, prob, param)].
    Returns K_NA, K_NB, K_NA_spatial, K_NA_sigma2 (vectors), PXB (NA, 3), scalar (= scalars[0], sum_ij m_i e2 c2 d), the
    dense P (up to DENSE_MAX_ENTRIES entries), the column sums S (4, NB) and the per-column minimum of q.  Every sum over i
    is per column, so the columns are worked in independent chunks.

    `tweak` (mutations() only) states a wrong kernel: {"pass1_rows": rows the column sums run over, "pass2_cols": columns
    the row sums run over, "s0_extra_rows": rows added once more to S0, "s1_for_s0", "swap_c2_c3"}."""
    tw = tweak or {}
    f = lambda v: np.asarray(v, dtype=xp)  # noqa: E731
    xa, xb, m = f(xa_stored)[:, :3], f(xb_stored)[:, :3], f(model_mul)
    NA, NB = len(xa), len(xb)
    o, eps = xp(outlier), xp(EPS)
    h1 = xp(-1) / (xp(2) * (xp(sigma2) / xp(sigma2_variance)))
    h2 = xp(-1) / (xp(2) * xp(sigma2))
    n2a, n2b = (xa * xa).sum(1), (xb * xb).sum(1)
    rows1 = np.arange(NA) if tw.get("pass1_rows") is None else np.asarray(tw["pass1_rows"])
    keep2 = np.ones(NB, dtype=bool)
    if tw.get("pass2_cols") is not None:
        keep2[:] = False
        keep2[np.asarray(tw["pass2_cols"])] = True
    lay = [(f(X), f(Y), f(a), f(b), met, kind, par) for X, Y, a, b, met, kind, par in layers]
    out = {q: np.zeros(NA, dtype=xp) for q in ("K_NA", "K_NA_spatial", "K_NA_sigma2")}
    out.update(K_NB=np.zeros(NB, dtype=xp), PXB=np.zeros((NA, 3), dtype=xp), S=np.zeros((4, NB), dtype=xp),
               q_min=np.zeros(NB, dtype=xp))
    if NA * NB <= DENSE_MAX_ENTRIES:
        out["P"] = np.zeros((NA, NB), dtype=xp)
    scalar = xp(0)
    step = max(1, chunk_entries // NA)
    for lo in range(0, NB, step):
        sl = slice(lo, min(lo + step, NB))
        d = np.maximum((n2a[:, None] + n2b[None, sl]) - 2 * xa.dot(xb[sl].T), 0)   # |x|^2 + |y|^2 - 2 x.y, clamped
        e2 = np.exp(d * h2)
        e1 = e2 if h1 == h2 else np.exp(d * h1)   # sigma2_variance = 1: the same numbers
        q = np.ones_like(d)
        for X, Y, a, b, met, kind, par in lay:
            s = {"euc": 2, "square_euc": 2, "kl": 1, "sym_kl": xp(0.5), "cos": xp(0.5)}[met]
            dl = (a[:, None] + b[None, sl]) - s * X.dot(Y[sl].T)
            if met in ("euc", "square_euc"):
                dl = np.maximum(dl, 0)
            if met == "square_euc":
                dl = np.sqrt(dl)
            q = q * {"gauss": lambda v: np.exp(v * (xp(-1) / (xp(2) * xp(par)))), "cos": lambda v: 1 - v,
                     "prob": lambda v: v}[kind](dl)
        e2m = e2 * m[:, None]
        S0 = e1[rows1].sum(0) + sum(e1[r] for r in tw.get("s0_extra_rows", ()))
        S1, S2, S3 = (e1 * m[:, None])[rows1].sum(0), e2m[rows1].sum(0), (e2m * q)[rows1].sum(0)
        inl = 1 - o / (o + (S1 if tw.get("s1_for_s0") else S0))
        c1, c2, c3 = 1 / (o + S1), inl / (S2 + eps), inl / (S3 + eps)
        out["K_NB"][sl] = c3 * S3
        if tw.get("swap_c2_c3"):
            c2, c3 = c3, c2
        k2 = keep2[sl].astype(xp)
        P2, P = e2m * (c2 * k2), e2m * q * (c3 * k2)
        out["K_NA_spatial"] += m * (e1 * (c1 * k2)).sum(1)
        out["K_NA_sigma2"] += P2.sum(1)
        out["K_NA"] += P.sum(1)
        out["PXB"] += P.dot(xb[sl])
        scalar = scalar + (P2 * d).sum()
        if "P" in out:
            out["P"][:, sl] = P
        out["S"][:, sl] = (S0, S1, S2, S3)
        out["q_min"][sl] = q.min(0)
    out["scalar"] = np.asarray(scalar, dtype=xp)
    return out


def quantities(raw, D):
    """The QUANTITIES of _assign_case from the raw outputs, as update_assignment derives them."""
    out = {q: np.asarray(raw[q], dtype=np.float64) for q in ("K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2")}
    out["Sp"], out["Sp_spatial"], out["Sp_sigma2"] = (np.float64(out[q].sum()) for q in ("K_NB", "K_NA_spatial", "K_NA_sigma2"))
    out["sigma2_related"] = np.float64(float(raw["scalar"]) / (D * float(out["Sp_sigma2"])))
    out["PXB"] = np.asarray(raw["PXB"], dtype=np.float64)[:, :D]
    return out


def raw_deviations(got, ref, with_P=False):
    """{output: max |got - ref| / max |ref|} over the raw outputs (exact agreement where the reference is all zero)."""
    dev = {}
    for q in RAW + (("P",) if with_P and "P" in ref else ()):
        a, b = np.asarray(got[q]), np.asarray(ref[q])
        assert a.shape == b.shape, (q, a.shape, b.shape)
        assert np.isfinite(np.asarray(a, dtype=np.float64)).all(), q
        top = np.abs(b).max()
        dev[q] = float(np.abs(a - b).max() / top) if top > 0 else (0.0 if not np.any(a) else np.inf)
    return dev


def reference_for(case, dtype, xp=np.float64, tweak=None, layers=None):
    """pair_reference on the case's prepare_reference operands and stored coordinates."""
    mm, o = raw_scalars(case)
    lay = prepare_layers(case, dtype) if layers is None else layers
    return pair_reference(stored_coords(case["XA"], dtype), stored_coords(case["XB"], dtype), lay, mm, case["sigma2"],
                          case["sigma2_variance"], o, xp=xp, tweak=tweak)


# ------------------------------------------------------------------------------------------------------ case makers
SIGMA2S = (0.05, 0.08, 0.1, 0.2, 0.5)
FAR_FRACTION = 0.07
DEFAULT_PARAM = {"kl": lambda g: 0.2, "sym_kl": lambda g: 0.2, "cos": lambda g: 0.1, "euc": lambda g: float(g),
                 "square_euc": lambda g: float(np.sqrt(g))}   # gauss widths of the order of the typical layer distance


def counts_layer(rng, g, labels, prof_seed, k=5):
    """Count-like expression with k cell types (kl / sym_kl); the cell-type profiles come from `prof_seed`."""
    prof = np.random.default_rng(prof_seed).gamma(0.6, 4.0, (k, g))
    return rng.poisson(prof[labels]).astype(np.float64)


def grid_layer(rng, g, labels, prof_seed, k=5):
    """PCA-like representation on the 1/32 grid (euc / square_euc / cos): sums of squares and dot products of such rows are
    exact in float64 in any order, so coincident rows give a layer distance of exactly 0 on the device and on the host."""
    cent = np.random.default_rng(prof_seed).standard_normal((k, g)) * 1.5
    return np.round((cent[labels] + 0.7 * rng.standard_normal((len(labels), g))) * 32) / 32


def make_case(name, NA, NB, layers, D=3, sigma2=None, gamma=0.05, sigma2_variance=1.0, zero_A=(), zero_B=(), dup=0,
              far="some"):
    """One input of the step, as the goldens are made: A cells normal, B cells jittered copies of A cells, a fraction of the B
    columns out of reach of every A cell (`far`: "some" - 7 % when NB >= 16 -, "all", "none").  layers: [(metric,
    probability type, parameter or None for the default, features)].  zero_A / zero_B: rows whose layers are all zero
    ("all": every row); dup: the first `dup` near B cells are exact copies (coordinates and layers) of their A cell."""
    seed = zlib.crc32(name.encode())
    rng = np.random.default_rng(seed)
    sigma2 = SIGMA2S[seed % len(SIGMA2S)] if sigma2 is None else sigma2
    XA = rng.standard_normal((NA, D))
    src = rng.choice(NA, NB)
    XB = XA[src] + 0.15 * rng.standard_normal((NB, D))
    n_far = {"some": int(np.ceil(FAR_FRACTION * NB)) if NB >= 16 else 0, "all": NB, "none": 0}[far]
    far_idx = np.sort(rng.choice(NB, n_far, replace=False))
    # beyond `reach` both spatial exponentials are exactly 0 in float64 for the whole column (argument below -800)
    reach = np.sqrt(2 * sigma2 * 800.0 / min(1.0, sigma2_variance)) + 2 * np.abs(XA).max() * np.sqrt(D)
    XB[far_idx] = XA[src[far_idx]] + reach * (1.0 + rng.random((n_far, 1))) * np.eye(D)[0]
    labA = rng.integers(0, 5, NA)
    LA, LB = [], []
    for l, (met, _, _, g) in enumerate(layers):
        maker = counts_layer if met in ("kl", "sym_kl") else grid_layer
        LA.append(maker(rng, g, labA, (seed, l)))   # the same cell-type profiles / centres for both slices, own noise
        LB.append(maker(rng, g, labA[src], (seed, l)))
    near = np.setdiff1d(np.arange(NB), far_idx)[:dup]
    XB[near] = XA[src[near]]
    for A, B in zip(LA, LB):
        B[near] = A[src[near]]
        A[np.arange(NA) if zero_A == "all" else list(zero_A)] = 0.0
        B[np.arange(NB) if zero_B == "all" else list(zero_B)] = 0.0
    extent = np.maximum(XA.max(0) - XA.min(0), 1.0)
    return dict(name=name, XA=XA, XB=XB, layers_A=LA, layers_B=LB, dissimilarity=[l[0] for l in layers],
                probability_type=[l[1] for l in layers],
                probability_parameters=[(DEFAULT_PARAM[l[0]](l[3]) if l[2] is None else l[2]) if l[1] == "gauss" else None
                                        for l in layers],
                sigma2=float(sigma2), alpha=rng.uniform(0.5, 1.0, NA), SigmaDiag=sigma2 * rng.uniform(0.0, 0.3, NA),
                gamma=float(gamma), samples_s=float(np.prod(extent)), sigma2_variance=float(sigma2_variance), far=far_idx,
                dup=near, features=[l[3] for l in layers])


def call_arguments(case):
    """(positional, keyword) arguments of update_assignment / _assign_case.restatement."""
    kw = {k: case[k] for k in ("dissimilarity", "probability_type", "probability_parameters", "sigma2", "alpha", "SigmaDiag",
                               "gamma", "samples_s", "sigma2_variance")}
    return (case["XA"], case["XB"], case["layers_A"], case["layers_B"]), kw


# ------------------------------------------------------------------------------------------------------ the lists
CELL_NAS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
CELL_NBS = (1, 65, 200)
FEATURE_GS = (1, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129)
SYM_GS = (1, 7, 8, 9, 24, 32, 33)        # 2 g -> ld: edges at 8 / 9 and 32 / 33
BIG_GS = (1000, 2000)
FEATURE_SHAPE, BIG_SHAPE = (130, 97), (300, 200)
PREPARE_NS = (1, 3, 4, 5, 257)           # four waves, i.e. four cells, per workgroup
PREPARE_GS = tuple(sorted(set(FEATURE_GS + SYM_GS + BIG_GS)))
METRIC_PROB = (("cos", "gauss"), ("cos", "cos"), ("cos", "prob"), ("euc", "gauss"), ("square_euc", "gauss"), ("kl", "gauss"),
               ("sym_kl", "gauss"), ("kl", "prob"))   # every pair whose probability stays >= 0 (asserted on the reference)
LAYER_SET = (("kl", "gauss", None, 7), ("cos", "cos", None, 17), ("sym_kl", "gauss", None, 25), ("euc", "gauss", None, 200))
SPLIT_PLANS = {(4417, 50): (70, 1, 64, 1), (50, 4417): (1, 70, 1, 64), (2500, 2500): (40, 40, 26, 26),
               (150, 38400): (3, 600, 2, 64), (65600, 130): (1025, 3, 64, 1), (130, 65600): (3, 1025, 1, 64),
               (4096, 4096): (64, 64, 16, 16)}
DENSE_SHAPES = ((1, 1), (65, 63), (64, 64), (129, 257), (1, 300), (300, 1))


def _specs():
    s = {}
    kl = lambda g: [("kl", "gauss", None, g)]  # noqa: E731
    for na in CELL_NAS:
        for nb in CELL_NBS:
            for a, b in ((na, nb), (nb, na)):
                s.setdefault(f"cells-{a}x{b}", ("cells", dict(NA=a, NB=b, layers=kl(20))))
    for met in ("euc", "cos", "kl"):
        for g in FEATURE_GS:
            s[f"feat-{met}-g{g}"] = ("features", dict(NA=FEATURE_SHAPE[0], NB=FEATURE_SHAPE[1], layers=[(met, "gauss", None, g)]))
    for g in SYM_GS:
        s[f"feat-sym_kl-g{g}"] = ("features", dict(NA=FEATURE_SHAPE[0], NB=FEATURE_SHAPE[1], layers=[("sym_kl", "gauss", None, g)]))
    for met in ("kl", "euc"):
        for g in BIG_GS:
            s[f"feat-{met}-g{g}"] = ("features 1000+", dict(NA=BIG_SHAPE[0], NB=BIG_SHAPE[1], layers=[(met, "gauss", None, g)]))
    for met, kind in METRIC_PROB:
        s[f"mp-{met}-{kind}"] = ("metric x probability", dict(NA=150, NB=110, layers=[(met, kind, None, 24)]))
    for n in (1, 2, 3, 4):
        s[f"layers-{n}"] = ("layers", dict(NA=140, NB=101, layers=list(LAYER_SET[:n])))
    s["layers-4-reversed"] = ("layers", dict(NA=140, NB=101, layers=list(LAYER_SET[::-1])))
    for na, nb in SPLIT_PLANS:
        s[f"split-{na}x{nb}"] = ("splits", dict(NA=na, NB=nb, layers=kl(24)))
    s["deg-1x1"] = ("degenerate", dict(NA=1, NB=1, layers=kl(5)))
    for met in ("cos", "kl"):
        one = [(met, "gauss", None, 24)]
        s[f"deg-zero-row-each-side-{met}"] = ("degenerate", dict(NA=70, NB=66, layers=one, zero_A=(3, 69), zero_B=(0, 65)))
        s[f"deg-all-zero-A-{met}"] = ("degenerate", dict(NA=70, NB=66, layers=one, zero_A="all"))
        s[f"deg-all-zero-B-{met}"] = ("degenerate", dict(NA=70, NB=66, layers=one, zero_B="all"))
    for met in METRICS:
        s[f"deg-duplicates-{met}"] = ("degenerate", dict(NA=70, NB=66, layers=[(met, "gauss", None, 24)], dup=20))
    s["deg-all-far"] = ("degenerate", dict(NA=70, NB=66, layers=kl(24), far="all"))
    s["deg-none-far"] = ("degenerate", dict(NA=70, NB=66, layers=kl(24), far="none"))
    s["deg-2d-variance"] = ("degenerate", dict(NA=70, NB=66, D=2, sigma2_variance=2.5, layers=[("euc", "gauss", None, 24)]))
    for na, nb in DENSE_SHAPES:
        s[f"dense-{na}x{nb}"] = ("dense", dict(NA=na, NB=nb, layers=[("kl", "gauss", None, 20), ("cos", "cos", None, 17)]))
    return s


SPECS = _specs()
PAIR_CASES = tuple(n for n, (fam, _) in SPECS.items() if fam != "dense")   # stage B; the dense shapes run in stage C
DENSE_CASES = tuple(n for n, (fam, _) in SPECS.items() if fam == "dense")
SPLIT_CASES = tuple(n for n, (fam, _) in SPECS.items() if fam == "splits")
CELL_CASES = tuple(n for n, (fam, _) in SPECS.items() if fam == "cells")
WRAPPER_CASES = {"feat-kl-g2000": "a", "layers-4": "b", "split-4417x50": "a", "deg-2d-variance": "c",
                 "deg-zero-row-each-side-kl": "a", "deg-zero-row-each-side-cos": "b"}   # case -> nearest golden (float32 floor)


def family(name):
    return SPECS[name][0]


def shape(name):
    """(NA, NB) of a case, without building it."""
    return SPECS[name][1]["NA"], SPECS[name][1]["NB"]


@functools.lru_cache(maxsize=8)
def case(name):
    return make_case(name, **SPECS[name][1])


# ------------------------------------------------------------------------------------------------------ mutations
MUTATION_CASES = ("feat-kl-g17", "feat-euc-g33", "cells-65x65", "layers-2", "split-4417x50", "split-50x4417")


def mutations(c, dtype=np.float64):
    """[(name, raw outputs)]: targeted wrong answers, each the reference run on altered inputs or with one stated slip
    (pair_reference's `tweak`): what an off-by-one in the k-loop, the tile masks, the factors or the split bookkeeping
    would return."""
    lay = prepare_layers(c, dtype)
    NA, NB = len(c["XA"]), len(c["XB"])
    rt, ct, rs, cs = plan(NA, NB)
    g0 = (2 if c["dissimilarity"][0] == "sym_kl" else 1) * c["features"][0]

    def without_feature(k):
        X = lay[0][0].copy()
        X[:, k] = 0
        return [(X,) + lay[0][1:]] + lay[1:]

    ref = lambda **kw: reference_for(c, dtype, **kw)  # noqa: E731
    out = [("the last feature dropped", ref(layers=without_feature(g0 - 1))),
           ("the last real feature of the first k-step dropped", ref(layers=without_feature(min(g0, KSTEP) - 1))),
           ("S1 used for S0", ref(tweak={"s1_for_s0": True})),
           ("c2 and c3 swapped", ref(tweak={"swap_c2_c3": True})),
           ("a clamped pad row counted once more in S0", ref(tweak={"s0_extra_rows": [NA - 1]}))]
    if NA > 1:
        out.append(("the last A row left out of the column sums", ref(tweak={"pass1_rows": np.arange(NA - 1)})))
    if NB > 1:
        out.append(("the last B column left out of the row sums", ref(tweak={"pass2_cols": np.arange(NB - 1)})))
    if rs > 1:
        lo, hi = split_tiles(rt, rs, rs // 2)
        rows = np.concatenate([np.arange(0, lo * TILE), np.arange(min(hi * TILE, NA), NA)])
        out.append(("one row split's partials left out", ref(tweak={"pass1_rows": rows})))
    if cs > 1:
        lo, hi = split_tiles(ct, cs, cs // 2)
        cols = np.concatenate([np.arange(0, lo * TILE), np.arange(min(hi * TILE, NB), NB)])
        out.append(("one column split's partials left out", ref(tweak={"pass2_cols": cols})))
    if len(lay) == 2:   # layer 2's operands under layer 1's metric and probability
        out.append(("layer 2's operands taken for layer 1", ref(layers=[lay[1][:4] + lay[0][4:], lay[1]])))
    return out
