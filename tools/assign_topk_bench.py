#!/usr/bin/env python
"""Time per call of the top-k sparse assignment step (``mvf_assign_topk``: the reference's ``sparse_calculation_mode``) next to
the dense fused step (``mvf_assign``) on the same inputs and in the same process.  One JSON line per measurement.

    python tools/assign_topk_bench.py --n 100000 --features 50 --ks 1 16 64 --dtypes float64 float32
    rocprofv3 --kernel-trace --stats -d out -- python tools/assign_topk_bench.py --n 20000 --ks 16 --reps 1

The inputs are tools/assign_bench.py's (one kl layer with a gauss probability, 3-D coordinates, B = A's cells displaced).  The
times are device times between two stream events around the launches, the minimum over ``--reps`` calls after one warm-up;
``ratio`` = top-k time / dense time.  ``insertions_per_column`` is the COMPUTED expectation k (1 + ln(NA / k)) of list
insertions for rows in random order (the k-th largest of the first n rows changes with probability k / n at row n) - what the
selection adds to pass 1 - not a measurement.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spateo-release_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from assign_bench import make_inputs  # noqa: E402


def timed(fn, reps):
    times, out = [], None
    for _ in range(reps + 1):  # the first call is a warm-up (code-object load)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) / 1e3)
    return min(times[1:]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100000])
    ap.add_argument("--features", type=int, default=50)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    from spateo_amd import _lib
    from spateo_amd._kernels import HipKernels

    sigma2, gamma, param = 0.01, 0.5, 0.05
    for n in args.n:
        XA, XB, LA, LB, mm = make_inputs(n, args.features)
        outlier = float((2 * np.pi * sigma2) ** 1.5 * (1 - gamma) / (gamma * np.prod(XA.max(0) - XA.min(0)) * n))
        for dtype in args.dtypes:
            k = HipKernels("cuda:0", dtype)
            Xp, a, ld = k.assign_prepare(LA, _lib.ASSIGN_METRICS["kl"], 0)
            Yp, b, _ = k.assign_prepare(LB, _lib.ASSIGN_METRICS["kl"], 1)
            xa4, xb4, mmd = k.to_x4(XA), k.to_x4(XB), k.h2d(mm)
            layers = [(Xp, Yp, a, b, ld, _lib.ASSIGN_METRICS["kl"], 0, param)]
            t_dense, dense = timed(lambda: k.assign(xa4, xb4, layers, mmd, sigma2, 1.0, outlier), args.reps)
            sp_dense = float(dense["K_NB"].sum())
            print(json.dumps(dict(kind="dense", n=n, features=args.features, dtype=dtype, seconds=round(t_dense, 5), Sp=sp_dense)),
                  flush=True)
            del dense
            for top_k in args.ks:
                t, out = timed(lambda: k.assign_topk(xa4, xb4, layers, mmd, sigma2, 1.0, outlier, top_k), args.reps)
                ke = min(top_k, n)
                print(json.dumps(dict(kind="topk", n=n, features=args.features, dtype=dtype, k=top_k, seconds=round(t, 5),
                                      ratio=round(t / t_dense, 3), Sp=float(out["K_NB"].sum()), Sp_dense=sp_dense,
                                      insertions_per_column=round(ke * (1 + np.log(n / ke)), 1))), flush=True)
                del out
                torch.cuda.empty_cache()
            del k
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
