#!/usr/bin/env python
"""Time per call of the wide evaluator (``mvf_eval_wide``: values and Jacobian of a field with Dy output columns at d = 3) next
to the composition the package allowed before it: ``con_k`` materialising the n x m kernel matrix, then torch float64 matmuls
with ``C`` - one for the values and d more on coordinate-scaled copies for the gradient.  One JSON line per measurement.

    python tools/eval_wide_bench.py --shapes grid48 genes2000 --reps 5
    python tools/eval_wide_bench.py --shapes grid48 --arms new --reps 1        # under rocprofv3 --kernel-trace --stats

Both arms run in ONE process on the same inputs, alternating (yardstick, yardstick again, new) per repetition after one warm-up
round; device times between two stream events around the launches.  ``aa_spread`` = the largest relative difference between the
two yardstick samples of a repetition: the run-to-run spread a difference between the arms has to exceed.  ``flop`` is COMPUTED
from the shape, 2 n m dy (1 + d) (values alone: 2 n m dy), and ``f64_matrix_fraction`` = flop / time / F64_MATRIX_PEAK (the
float64 matrix peak tools/assign_bench.py uses).  The yardstick's outputs are left in its natural (n, dy) layouts (no transposition
into (dy, d, n)): it is not charged for the layout.  ``deviation`` = largest difference between the arms relative to the largest
entry, per output.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spateo-release_amd"))

F64_MATRIX_PEAK = 78.6e12
SHAPES = {  # name -> (n, m, dy)
    "grid48": (64 ** 3, 500, 48),          # a 64^3 grid, the README's 48 genes
    "genes2000": (100_000, 2000, 2000),    # 100 k points, 2000 genes
    "tiny": (4096, 128, 48),
}
BETA, D = 0.004, 3


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["grid48", "genes2000"], choices=sorted(SHAPES))
    ap.add_argument("--dtype", default="float32", choices=["float32", "float64"])
    ap.add_argument("--arms", nargs="+", default=["yardstick", "new"], choices=["yardstick", "new"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    from spateo_amd import _lib
    from spateo_amd._kernels import HipKernels

    k = HipKernels("cuda:0", args.dtype)
    for name in args.shapes:
        n, m, dy = SHAPES[name]
        rng = np.random.default_rng(0)
        ctrl = rng.uniform(-30, 30, (m, D))
        X = rng.uniform(-30, 30, (n, D))
        center = ctrl.mean(0)
        x4, c4 = k.to_x4(X, center), k.to_x4(ctrl, center)
        Cd = k.h2d(rng.uniform(0.5, 1.5, (m, dy)) * 0.02)
        xs, cs = x4[:, :D].contiguous(), c4[:, :D].contiguous()
        x64, c64 = xs.double(), cs.double()

        def yardstick(flags):
            K = k.con_k(xs, cs, BETA).double()
            v = K @ Cd
            if not flags & _lib.EVAL_JAC:
                return v, None
            J = [(-2.0 * BETA) * (x64[:, i : i + 1] * v - (K * c64[:, i][None, :]) @ Cd) for i in range(D)]
            return v, J

        def new(flags):
            o = k.eval_wide(x4, c4, D, BETA, Cd, flags)
            return o.get(_lib.EVAL_V), o.get(_lib.EVAL_JAC)

        for label, flags in (("V|JAC", _lib.EVAL_V | _lib.EVAL_JAC), ("V", _lib.EVAL_V)):
            flop = 2.0 * n * m * dy * (1 + (D if flags & _lib.EVAL_JAC else 0))
            samples = {"yardstick": [], "yardstick_again": [], "new": []}
            dev = {}
            for rep in range(args.warmup + args.reps):
                got = {}
                for arm in ("yardstick", "yardstick_again", "new"):
                    base = arm.split("_")[0]
                    if base not in args.arms:
                        continue
                    t, out = timed(lambda: (yardstick if base == "yardstick" else new)(flags))
                    if rep >= args.warmup:
                        samples[arm].append(t)
                    if rep == 0:
                        got[base] = out
                    else:
                        del out
                if rep == 0 and len(got) == 2:
                    (v0, J0), (v1, J1) = got["yardstick"], got["new"]
                    dev["v"] = float((v0 - v1).abs().max() / v0.abs().max())
                    if J0 is not None:
                        scale = max(float(j.abs().max()) for j in J0)
                        dev["jac"] = max(float((J0[i].T - J1[:, i, :]).abs().max()) for i in range(D)) / scale
                del got
                torch.cuda.empty_cache()
            rec = dict(kind="eval_wide", shape=name, n=n, m=m, dy=dy, d=D, dtype=args.dtype, flags=label, flop=flop, deviation=dev)
            for arm, ts in samples.items():
                if ts:
                    rec[arm] = dict(samples_s=[round(t, 6) for t in ts], median_s=round(float(np.median(ts)), 6),
                                    min_s=round(min(ts), 6),
                                    f64_matrix_fraction=round(flop / float(np.median(ts)) / F64_MATRIX_PEAK, 4))
            if samples["yardstick"] and samples["yardstick_again"]:
                rec["aa_spread"] = round(max(abs(a - b) / min(a, b) for a, b in zip(samples["yardstick"], samples["yardstick_again"])), 4)
            if samples["yardstick"] and samples["new"]:
                both = samples["yardstick"] + samples["yardstick_again"]
                rec["speedup_median"] = round(float(np.median(both)) / float(np.median(samples["new"])), 3)
            print(json.dumps(rec), flush=True)
        del x4, c4, Cd, xs, cs, x64, c64
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
