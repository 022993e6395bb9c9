#!/usr/bin/env python
"""Time per call of the cell mapping from the fused assignment (``mvf_assign_best``: the best partner of every row and column
of P, without P) next to the dense fused step (``mvf_assign``) on the same inputs and in the same process.  One JSON line per
measurement.

    python tools/assign_best_bench.py --n 20000 100000 --features 50 --dtypes float64 float32
    rocprofv3 --kernel-trace --stats -d out -- python tools/assign_best_bench.py --n 20000 --reps 1

The inputs are tools/assign_bench.py's (one kl layer with a gauss probability, 3-D coordinates, B = A's cells displaced).  The
times are device times between two stream events around the launches, the minimum over ``--reps`` calls after one warm-up;
``ratio`` = mapping time / assignment time.  ``expected_ratio`` is the COMPUTED expectation, not a measurement: pass 1 and two
tile sweeps against ``mvf_assign``'s two sweeps, 1.5.  ``rows_only`` / ``cols_only`` time the call with the other pair NULL
(pass 1 and one sweep: expected 1.0).
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

EXPECTED_RATIO = 1.5


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
    ap.add_argument("--n", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--features", type=int, default=50)
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
            print(json.dumps(dict(kind="assign", n=n, features=args.features, dtype=dtype, seconds=round(t_dense, 5),
                                  Sp=float(dense["K_NB"].sum()))), flush=True)
            del dense
            t, out = timed(lambda: k.assign_best(xa4, xb4, layers, mmd, sigma2, 1.0, outlier), args.reps)
            t_rows, _ = timed(lambda: k.assign_best(xa4, xb4, layers, mmd, sigma2, 1.0, outlier, cols=False), args.reps)
            t_cols, _ = timed(lambda: k.assign_best(xa4, xb4, layers, mmd, sigma2, 1.0, outlier, rows=False), args.reps)
            rows, cols = out["rows"].cpu().numpy(), out["cols"].cpu().numpy()
            in_range = bool(rows.min() >= 0 and rows.max() < n and cols.min() >= 0 and cols.max() < n)
            print(json.dumps(dict(kind="best", n=n, features=args.features, dtype=dtype, seconds=round(t, 5),
                                  ratio=round(t / t_dense, 3), expected_ratio=EXPECTED_RATIO, rows_only=round(t_rows, 5),
                                  cols_only=round(t_cols, 5), in_range=in_range,
                                  workspace_MB=round(int(k.lib.mvf_assign_best_workspace_bytes(n, n)) / 1e6, 1))), flush=True)
            del out, k
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
