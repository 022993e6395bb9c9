#!/usr/bin/env python
"""One iteration of the pairwise alignment, two ways, on the same inputs in the same process, alternating:

* ``loop``      - ``spateo_amd.align.morpho_iterate`` (device resident; per iteration the host reads 64 float64);
* ``composed``  - the same iteration from the public stages ``update_assignment`` + NumPy + ``update_nonrigid`` (host arrays
                  in and out of every stage: what a hand-written loop had to do before ``morpho_iterate``).

The loop's time per iteration is the slope between a call of ``--short`` and one of ``--long`` iterations (its one-time
upload and preparation drop out); the composed form is timed per iteration directly, from the second iteration on.  Both
run the non-rigid update in every timed iteration (``nonrigid_start_iter=0``).  The split of the loop (assignment /
non-rigid / glue) comes from a separate, synchronising call under ``_runtime.PROFILE_FITS``; the bytes crossing the link per
iteration are computed from the shapes.  One JSON line per (shape, dtype) on stdout.

    python tools/align_loop_bench.py --cells 10000 100000 --repeats 3 [--out profiles/align_loop.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spateo-release_amd"))


def make_inputs(n, g, m, seed=0):
    """Slice B = a noisy copy of points Z, slice A = their rotated, shifted, smoothly bent pre-image; one count layer."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, 3))
    src = rng.permutation(n)
    XB = Z[src] + 0.05 * rng.standard_normal((n, 3))
    c, s = np.cos(0.35), np.sin(0.35)
    R0 = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    XA = (Z + 0.04 * np.sin(1.3 * Z[:, ::-1] + 0.5) - 0.4) @ R0
    lab = rng.integers(0, 5, n)
    prof = rng.gamma(0.6, 4.0, (5, g))
    LA, LB = rng.poisson(prof[lab]).astype(np.float64), rng.poisson(prof[lab[src]]).astype(np.float64)
    ctrl = XA[rng.choice(n, m, replace=False)]
    return XA, XB, LA, LB, ctrl


def digamma(x):
    x = np.array(x, dtype=np.float64)
    s = np.zeros_like(x)
    for _ in range(10):
        low = x < 10.0
        s = np.where(low, s + 1.0 / x, s)
        x = np.where(low, x + 1.0, x)
    r2 = 1.0 / (x * x)
    p = np.full_like(x, 1.0 / 12.0)
    for c in (-691.0 / 32760.0, 1.0 / 132.0, -1.0 / 240.0, 1.0 / 252.0, -1.0 / 120.0, 1.0 / 12.0):
        p = p * r2 + c
    return ((np.log(x) - 0.5 / x) - p * r2) - s


def composed(align, XA, XB, LA, LB, ctrl, common, iters, dtype, device):
    """`iters` iterations from the public stages; returns (per-iteration seconds, {stage: seconds per iteration}, sigma2)."""
    NA, D = XA.shape
    NB = len(XB)
    sigma2, gamma, s2v = common["sigma2"], 0.5, 1.0
    alpha, SigmaDiag, VnA = np.ones(NA), np.zeros(NA), np.zeros((NA, D))
    XAHat, RnA = XA.copy(), XA.copy()
    samples_s = float(max(np.prod(XA.max(0) - XA.min(0)), np.prod(XB.max(0) - XB.min(0))))
    step = 10.0 ** (1.0 / 100)
    times, stages = [], {"assign": 0.0, "nonrigid": 0.0, "glue": 0.0}
    for it in range(iters):
        t0 = time.perf_counter()
        a = align.update_assignment(XAHat, XB, [LA], [LB], dissimilarity=["kl"], probability_type=["gauss"],
                                    probability_parameters=[0.1], sigma2=sigma2, alpha=alpha, SigmaDiag=SigmaDiag, gamma=gamma,
                                    samples_s=samples_s, sigma2_variance=s2v, dtype=dtype, device=device)
        t1 = time.perf_counter()
        K_NA, K_NB, PXB = a["K_NA"], a["K_NB"], a["PXB"]
        gamma = float(np.clip(np.exp(digamma(1.0 + a["Sp_spatial"]) - digamma(2.0 + NB)), 0.01, 0.99))
        alpha = np.exp(digamma(1.0 + a["K_NA_spatial"]) - digamma(1.0 * NA + a["Sp_spatial"]))
        PXB_term = PXB - RnA * K_NA[:, None]
        t2 = time.perf_counter()
        if it > 0:   # as the loop with nonrigid_start_iter = 0 (morpho_class.py:289): not in the first iteration
            nr = align.update_nonrigid(XA, ctrl, common["beta"], K_NA, PXB_term, sigma2, common["lambdaVF"], dtype=dtype,
                                       device=device)
            VnA, SigmaDiag = nr["VnA"], nr["SigmaDiag"]
        t3 = time.perf_counter()
        Sp = a["Sp"]
        mu_A, mu_V, mu_B = K_NA @ XA / Sp, K_NA @ VnA / Sp, K_NB @ XB / Sp
        XA_hat = XA - mu_A
        A = -(XA_hat.T @ ((VnA - mu_V) * K_NA[:, None]) - XA_hat.T @ (PXB - K_NA[:, None] * mu_B)).T
        U, _, V = np.linalg.svd(A)
        C = np.eye(D)
        C[-1, -1] = np.linalg.det(U @ V)
        R = U @ C @ V
        t = mu_B - mu_V - mu_A @ R.T
        RnA = XA @ R.T + t
        XAHat = VnA + RnA
        sigma2 = max(a["sigma2_related"] + float(a["K_NA_sigma2"] @ SigmaDiag) / a["Sp_sigma2"], 1e-3)
        s2v = min(s2v * step, 10.0)
        sigma2 = max(sigma2, 1e-2)
        t4 = time.perf_counter()
        if it >= 1:
            times.append(t4 - t0)
            stages["assign"] += t1 - t0
            stages["nonrigid"] += t3 - t2
            stages["glue"] += (t2 - t1) + (t4 - t3)
    n = max(1, len(times))
    return times, {q: v / n for q, v in stages.items()}, sigma2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--features", type=int, default=50)
    ap.add_argument("--inducing", type=int, default=500)
    ap.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--short", type=int, default=2)
    ap.add_argument("--long", type=int, default=6)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from spateo_amd import _runtime as rt
    from spateo_amd import align

    assert torch.cuda.is_available(), "this benchmark needs a GPU: there is nothing to fall back to"
    lines = []
    for n in args.cells:
        XA, XB, LA, LB, ctrl = make_inputs(n, args.features, args.inducing)
        common = dict(beta=0.5, lambdaVF=100.0, sigma2=0.45)
        kw = dict(dissimilarity=["kl"], probability_type=["gauss"], probability_parameters=[0.1], inducing_variables=ctrl,
                  nonrigid_start_iter=0, record=False, device=args.device, **common)
        for dtype in args.dtypes:
            def loop(iters):
                t0 = time.perf_counter()
                out = align.morpho_iterate(XA, XB, [LA], [LB], max_iter=iters, dtype=dtype, **kw)
                return time.perf_counter() - t0, out

            loop(args.short), composed(align, XA, XB, LA, LB, ctrl, common, 2, dtype, args.device)   # warm-up of both forms
            per_loop, per_comp, st_comp = [], [], []
            for _ in range(args.repeats):                                                          # alternating
                ts, _ = loop(args.short)
                tl, out = loop(args.long)
                per_loop.append((tl - ts) / (args.long - args.short))
                times, stages, s2c = composed(align, XA, XB, LA, LB, ctrl, common, args.long, dtype, args.device)
                per_comp.append(float(np.mean(times)))
                st_comp.append(stages)
            rt.PROFILE_FITS = True
            try:
                loop(args.long)
                prof = dict(rt.last_fit_profile())
            finally:
                rt.PROFILE_FITS = False
            its = args.long
            g, m = args.features, args.inducing
            line = dict(
                cells=n, features=g, inducing=m, dtype=dtype, repeats=args.repeats,
                loop_ms=1e3 * float(np.median(per_loop)), loop_ms_min=1e3 * min(per_loop), loop_ms_max=1e3 * max(per_loop),
                composed_ms=1e3 * float(np.median(per_comp)), composed_ms_min=1e3 * min(per_comp), composed_ms_max=1e3 * max(per_comp),
                # synchronising profile of one `long` call: the first iteration has no non-rigid update
                loop_split_ms=dict(assign=1e3 * prof["assign"] / its, nonrigid=1e3 * prof["nonrigid"] / (its - 1),
                                   glue=1e3 * prof["glue"] / its, setup_once=1e3 * prof["setup"], result_once=1e3 * prof["result"]),
                composed_split_ms={q: 1e3 * float(np.mean([s[q] for s in st_comp])) for q in st_comp[0]},
                # bytes over the link per iteration: the loop reads its block and the solve's status words; the composed form
                # uploads XAHat, coordsB, both layers, alpha-derived model_mul, then coordsA, the control points, K_NA and Y, and
                # downloads four NA-vectors, K_NB, PXB, the scalar, then SigmaInv (float64 m x m, twice: G and Gamma), Coff, VnA
                # and SigmaDiag
                loop_link_bytes=64 * 8 + 4 + 8,
                composed_link_bytes=8 * (2 * 3 * n + 2 * n * g + n) + 8 * (3 * n + 3 * m + n + 3 * n)
                + 8 * (4 * n + n + 3 * n + 1) + 8 * (2 * m * m + 3 * m + 3 * n + n),
                sigma2_loop=float(out["sigma2"]), sigma2_composed=float(s2c),
            )
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
