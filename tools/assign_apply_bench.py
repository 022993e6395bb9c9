#!/usr/bin/env python
"""Time per call of the assignment applied to cell features without P (``mvf_assign_apply``: ``P @ FB`` and ``P^T @ FA``) next to
the fused step (``mvf_assign``) on the same inputs and in the same process.  One JSON line per measurement.

    python tools/assign_apply_bench.py --n 100000 --features 50 --widths 32 64 --dtypes float64 float32
    python tools/assign_apply_bench.py --n 10000 --widths 64 --dtypes float64 --against-dense
    rocprofv3 --kernel-trace --stats -d out -- python tools/assign_apply_bench.py --n 100000 --widths 64 --reps 1 --dtypes float32

The inputs are tools/assign_bench.py's (one kl layer with a gauss probability, 3-D coordinates, B = A's cells displaced); the
features are standard normal.  Device times between two stream events around the launches, the minimum over ``--reps`` calls
after one warm-up.  Per direction and width C: ``call`` = pass 1 + the factors + cdiv(C, 64) sweeps; ``sweep`` = the call at
C + 64 columns minus the call at C columns - ONE more sweep and its reduction behind the same pass 1, a difference of two
measurements; ``steps`` = sweep / the time of one ``mvf_assign`` step.  ``mfma_floor_ms`` is COMPUTED, not measured: 2 NA NB C
flop of the product over the float64 matrix peak of DESIGN.md.

``--against-dense`` (API level, host wall clock around calls that end with the results on the host): ``apply_assignment``
against ``update_assignment(return_P=True)`` followed by the two host products.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from assign_bench import F64_MATRIX_PEAK, make_inputs  # noqa: E402

CHUNK = 64


def timed(fn, reps):
    times = []
    for _ in range(reps + 1):  # the first call is a warm-up (code-object load)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) / 1e3)
        del out
    return min(times[1:])


def device_level(args):
    from spateo_amd import _lib
    from spateo_amd._kernels import HipKernels

    sigma2, gamma, param = 0.01, 0.5, 0.05
    for n in args.n:
        XA, XB, LA, LB, mm = make_inputs(n, args.features)
        outlier = float((2 * np.pi * sigma2) ** 1.5 * (1 - gamma) / (gamma * np.prod(XA.max(0) - XA.min(0)) * n))
        F = np.random.default_rng(1).standard_normal((n, max(args.widths) + CHUNK))
        for dtype in args.dtypes:
            k = HipKernels("cuda:0", dtype)
            Xp, a, ld = k.assign_prepare(LA, _lib.ASSIGN_METRICS["kl"], 0)
            Yp, b, _ = k.assign_prepare(LB, _lib.ASSIGN_METRICS["kl"], 1)
            xa4, xb4, mmd, Fd = k.to_x4(XA), k.to_x4(XB), k.h2d(mm), k.h2d(F)
            layers = [(Xp, Yp, a, b, ld, _lib.ASSIGN_METRICS["kl"], 0, param)]
            head = (xa4, xb4, layers, mmd, sigma2, 1.0, outlier)
            t_step = timed(lambda: k.assign(*head), args.reps)
            print(json.dumps(dict(kind="assign", n=n, features=args.features, dtype=dtype, seconds=round(t_step, 5))), flush=True)
            for c in args.widths:
                rec = dict(kind="apply", n=n, features=args.features, dtype=dtype, C=c,
                           mfma_floor_ms=round(2.0 * n * n * c / F64_MATRIX_PEAK * 1e3, 2),
                           workspace_MB=round(int(k.lib.mvf_assign_apply_workspace_bytes(n, n, c, c)) / 1e6, 1))
                for name, key in (("to_A", "features_B"), ("to_B", "features_A")):
                    # (column slices of one wider tensor: rows of max + 64 doubles, ld > c)
                    t_c = timed(lambda: k.assign_apply(*head, **{key: Fd[:, :c]}), args.reps)
                    t_more = timed(lambda: k.assign_apply(*head, **{key: Fd[:, : c + CHUNK]}), args.reps)
                    rec[f"{name}_call"], rec[f"{name}_sweep"] = round(t_c, 5), round(t_more - t_c, 5)
                    rec[f"{name}_steps"] = round((t_more - t_c) / t_step, 3)
                t_both = timed(lambda: k.assign_apply(*head, features_B=Fd[:, :c], features_A=Fd[:, :c]), args.reps)
                rec["both_call"] = round(t_both, 5)
                print(json.dumps(rec), flush=True)
            del k, Xp, Yp, xa4, xb4, Fd
            torch.cuda.empty_cache()


def api_level(args):
    from spateo_amd import align

    sigma2, gamma, param = 0.01, 0.5, 0.05
    for n in args.n:
        XA, XB, LA, LB, mm = make_inputs(n, args.features)
        kw = dict(dissimilarity="kl", probability_type="gauss", probability_parameters=[param], sigma2=sigma2, alpha=mm,
                  SigmaDiag=np.zeros(n), gamma=gamma, samples_s=float(np.prod(XA.max(0) - XA.min(0))), device="cuda:0")
        for dtype in args.dtypes:
            for c in args.widths:
                F_A, F_B = (np.random.default_rng(s).standard_normal((n, c)) for s in (2, 3))
                best = {}
                for rep in range(args.reps + 1):
                    t0 = time.perf_counter()
                    got = align.apply_assignment(XA, XB, [LA], [LB], features_A=F_A, features_B=F_B, normalize=False, dtype=dtype, **kw)
                    t1 = time.perf_counter()
                    P = align.update_assignment(XA, XB, [LA], [LB], return_P=True, dtype=dtype, **kw)["P"]
                    t2 = time.perf_counter()
                    to_A, to_B = P @ F_B, P.T @ F_A
                    t3 = time.perf_counter()
                    if rep:
                        for q, v in (("apply", t1 - t0), ("dense_P", t2 - t1), ("host_products", t3 - t2)):
                            best[q] = min(best.get(q, np.inf), v)
                dev = max(np.abs(got["to_A"] - to_A).max() / np.abs(P @ np.abs(F_B)).max(),
                          np.abs(got["to_B"] - to_B).max() / np.abs(P.T @ np.abs(F_A)).max())
                print(json.dumps(dict(kind="api", n=n, features=args.features, dtype=dtype, C=c,
                                      apply_assignment=round(best["apply"], 4), update_assignment_return_P=round(best["dense_P"], 4),
                                      host_products=round(best["host_products"], 4), P_MB=round(n * n * 8 / 1e6, 1),
                                      deviation=float(dev))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100000])
    ap.add_argument("--features", type=int, default=50)
    ap.add_argument("--widths", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--against-dense", action="store_true")
    args = ap.parse_args()
    (api_level if args.against_dense else device_level)(args)


if __name__ == "__main__":
    main()
