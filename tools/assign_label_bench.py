#!/usr/bin/env python
"""What a ``"label"`` layer costs in the fused assignment step (``mvf_assign``): time per call of ``tools/assign_bench.py``'s
configuration (one ``kl`` layer with a ``gauss`` probability, 3-D coordinates, NA = NB = n) alone, with an added label layer
(a K x L table look-up per pair) and, for scale, with an added ``euc`` layer of 16 features (one k-step of f64 MFMA per
pair) in place of it.  One JSON line per (dtype, round, configuration).

    python tools/assign_label_bench.py --n 100000 --features 50 --reps 3 --rounds 3

The operands are prepared once per dtype; the configurations are then timed in turn, ``--rounds`` times over, so that a
drift of the machine shows as a difference between rounds and not between configurations.  Times are device times between
two stream events around the launches; ``seconds`` is the best of ``--reps`` calls after a warm-up call, ``times`` all of
them.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spateo-release_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from assign_bench import make_inputs  # noqa: E402


def timed(k, xa4, xb4, layers, mm, sigma2, outlier, reps):
    times, out = [], None
    for _ in range(reps + 1):  # the first call is a warm-up
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = k.assign(xa4, xb4, layers, mm, sigma2, 1.0, outlier)
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) / 1e3)
    return times[1:], float(out["K_NB"].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--features", type=int, default=50)
    ap.add_argument("--classes", type=int, nargs=2, default=[12, 10], help="K L of the label-transfer table")
    ap.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from spateo_amd import _lib
    from spateo_amd._kernels import HipKernels

    sigma2, gamma, param = 0.01, 0.5, 0.05
    n, (K, L) = args.n, args.classes
    XA, XB, LA, LB, mm = make_inputs(n, args.features)
    rng = np.random.default_rng(1)
    labA, labB = rng.integers(0, K, n), rng.integers(0, L, n)
    T = rng.uniform(0.05, 1.0, (K, L))
    T = (T / T.sum(1, keepdims=True)).astype(np.float32).astype(np.float64)
    EA, EB = rng.standard_normal((n, 16)), rng.standard_normal((n, 16))
    outlier = float((2 * np.pi * sigma2) ** 1.5 * (1 - gamma) / (gamma * np.prod(XA.max(0) - XA.min(0)) * n))
    for dtype in args.dtypes:
        k = HipKernels("cuda:0", dtype)
        kl, euc = _lib.ASSIGN_METRICS["kl"], _lib.ASSIGN_METRICS["euc"]
        Xp, a, ld = k.assign_prepare(LA, kl, 0)
        Yp, b, _ = k.assign_prepare(LB, kl, 1)
        Ep, ea, eld = k.assign_prepare(EA, euc, 0)
        Fp, eb, _ = k.assign_prepare(EB, euc, 1)
        base = (Xp, Yp, a, b, ld, kl, 0, param)
        label = (k.h2d(T), None, k.assign_label_prepare(labA, K), k.assign_label_prepare(labB, L), L, _lib.ASSIGN_LABEL, 2, 0.0)
        configs = {"kl": [base], "kl+label": [base, label], "kl+euc16": [base, (Ep, Fp, ea, eb, eld, euc, 0, 40.0)],
                   "label": [label]}
        xa4, xb4, mmd = k.to_x4(XA), k.to_x4(XB), k.h2d(mm)
        for rnd in range(args.rounds):
            for name, layers in configs.items():
                times, sp = timed(k, xa4, xb4, layers, mmd, sigma2, outlier, args.reps)
                print(json.dumps(dict(kind="fused", config=name, n=n, features=args.features, table=[K, L], dtype=dtype, round=rnd,
                                      seconds=round(min(times), 5), times=[round(t, 5) for t in times], Sp=sp)), flush=True)
        del k
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
