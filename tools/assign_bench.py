#!/usr/bin/env python
"""Time per call of the fused assignment step (``mvf_assign``; spateo_amd.align.update_assignment's device part) and, for
scale, of the same step written with plain torch ops in column chunks on the same GPU - the shape in which the
reference's torch backend runs ``_update_assignment_P`` with ``use_chunk=True``
(spateo/alignment/methods/morpho_class.py:1103-1144).  One JSON line per measurement.

    python tools/assign_bench.py --n 100000 --features 50 2000 --dtypes float64 float32 --baseline
    rocprofv3 --kernel-trace --stats -d out -- python tools/assign_bench.py --n 100000 --features 50 --reps 1

One kl layer with a gauss probability; 3-D coordinates; B = A's cells displaced, so every column has neighbours.  The
times are device times between two stream events around the launches (operands already on the device; the O(N G)
preparation is timed separately).  `mfma_fraction` = 2 passes x 2 NA NB G' flop / time / 78.6 Tflop/s (the float64
matrix peak of DESIGN.md), G' = the padded feature count.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spateo-release_amd"))

F64_MATRIX_PEAK = 78.6e12


def make_inputs(n, g, seed=0):
    rng = np.random.default_rng(seed)
    XA = rng.standard_normal((n, 3))
    XB = XA[rng.permutation(n)] + 0.05 * rng.standard_normal((n, 3))
    prof = rng.gamma(0.6, 4.0, (8, g))
    LA = rng.poisson(prof[rng.integers(0, 8, n)]).astype(np.float64)
    LB = rng.poisson(prof[rng.integers(0, 8, n)]).astype(np.float64)
    return XA, XB, LA, LB, rng.uniform(0.5, 1.0, n)


def fused(k, XA, XB, LA, LB, mm, sigma2, outlier, param, reps):
    from spateo_amd import _lib

    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    t0 = time.perf_counter()
    Xp, a, ld = k.assign_prepare(LA, _lib.ASSIGN_METRICS["kl"], 0)
    Yp, b, _ = k.assign_prepare(LB, _lib.ASSIGN_METRICS["kl"], 1)
    torch.cuda.synchronize()
    t_prep = time.perf_counter() - t0
    xa4, xb4, mmd = k.to_x4(XA), k.to_x4(XB), k.h2d(mm)
    layers = [(Xp, Yp, a, b, ld, _lib.ASSIGN_METRICS["kl"], 0, param)]
    times, out = [], None
    for _ in range(reps + 1):  # the first call is a warm-up (code-object load)
        s, e = ev(), ev()
        s.record()
        out = k.assign(xa4, xb4, layers, mmd, sigma2, 1.0, outlier)
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) / 1e3)
    return min(times[1:]), t_prep, ld, float(out["K_NB"].sum())


def torch_chunked(XA, XB, LA, LB, mm, sigma2, outlier, param, dtype, chunk, device):
    """The step with torch ops, B in column chunks (every intermediate NA x chunk)."""
    td = torch.float64 if dtype == "float64" else torch.float32
    dev = lambda a: torch.as_tensor(a, dtype=td, device=device)  # noqa: E731
    XA, XB, LA, LB, mm = dev(XA), dev(XB), dev(LA), dev(LB), dev(mm)[:, None]
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    X = LA + 0.01
    X = X / X.sum(1, keepdim=True)
    XlogX = (X * torch.log(X + 1e-8)).sum(1, keepdim=True)
    na2 = (XA**2).sum(1)[:, None]
    K_NA = torch.zeros(len(XA), dtype=td, device=device)
    K_NA_spatial, K_NA_sigma2 = torch.zeros_like(K_NA), torch.zeros_like(K_NA)
    PXB = torch.zeros(len(XA), 3, dtype=td, device=device)
    K_NB, s2r = [], 0.0
    for lo in range(0, len(XB), chunk):
        yb, lb = XB[lo:lo + chunk], LB[lo:lo + chunk] + 0.01
        d = torch.clamp(na2 + (yb**2).sum(1)[None, :] - 2 * XA @ yb.T, min=0.0)
        e2 = torch.exp(-d / (2 * sigma2))
        inl = 1 - outlier / (outlier + e2.sum(0, keepdim=True))
        e2 = e2 * mm
        K_NA_spatial += (e2 / (outlier + e2.sum(0, keepdim=True))).sum(1)
        P2 = inl * e2 / (e2.sum(0, keepdim=True) + 1e-8)
        K_NA_sigma2 += P2.sum(1)
        s2r = s2r + (P2 * d).sum()
        del P2
        lb = lb / lb.sum(1, keepdim=True)
        e2 = e2 * torch.exp(-(XlogX - X @ torch.log(lb + 1e-8).T) / (2 * param))
        P = inl * e2 / (e2.sum(0, keepdim=True) + 1e-8)
        K_NA += P.sum(1)
        K_NB.append(P.sum(0))
        PXB += P @ yb
        del P, e2, d
    Sp = torch.cat(K_NB).sum()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / 1e3, float(Sp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--features", type=int, nargs="+", default=[50, 2000])
    ap.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--chunk", type=int, default=4096)
    args = ap.parse_args()
    from spateo_amd._kernels import HipKernels

    sigma2, gamma, param = 0.01, 0.5, 0.05
    for g in args.features:
        XA, XB, LA, LB, mm = make_inputs(args.n, g)
        outlier = float((2 * np.pi * sigma2) ** 1.5 * (1 - gamma) / (gamma * np.prod(XA.max(0) - XA.min(0)) * args.n))
        for dtype in args.dtypes:
            k = HipKernels("cuda:0", dtype)
            t, t_prep, ld, sp = fused(k, XA, XB, LA, LB, mm, sigma2, outlier, param, args.reps)
            rec = dict(kind="fused", n=args.n, features=g, padded=ld, dtype=dtype, seconds=round(t, 5),
                       prepare_seconds_incl_h2d=round(t_prep, 4), Sp=sp,
                       mfma_fraction=round(2 * 2 * args.n * args.n * ld / t / F64_MATRIX_PEAK, 4))
            print(json.dumps(rec), flush=True)
            del k
            torch.cuda.empty_cache()
            if args.baseline:
                tb, spb = torch_chunked(XA, XB, LA, LB, mm, sigma2, outlier, param, dtype, args.chunk, "cuda:0")  # warm-up
                tb, spb = torch_chunked(XA, XB, LA, LB, mm, sigma2, outlier, param, dtype, args.chunk, "cuda:0")
                print(json.dumps(dict(kind="torch_chunked", n=args.n, features=g, dtype=dtype, chunk=args.chunk,
                                      seconds=round(tb, 5), Sp=spb, fused_speedup=round(tb / t, 2))), flush=True)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
