#!/usr/bin/env python
"""One SVI iteration of the pairwise alignment, two ways, on the same inputs in the same process, alternating:

* ``loop``      - ``spateo_amd.align.morpho_iterate_svi`` (device resident; per iteration the host reads 64 float64);
* ``composed``  - the same iteration from the public stages: ``update_assignment`` on the batch's rows of ``coordsB`` and of
                  the B layer + NumPy blends + ``update_nonrigid(svi=)`` (host arrays in and out of every stage: the only way
                  to run the reference's default mode before ``morpho_iterate_svi``).

As in ``tools/align_loop_bench.py`` (whose inputs these are): the loop's time per iteration is the slope between a call of
``--short`` and one of ``--long`` iterations; the composed form is timed per iteration directly, from the second iteration
on; both run the non-rigid update in every timed iteration; the loop's split comes from a separate, synchronising call under
``_runtime.PROFILE_FITS``; the bytes crossing the link per iteration are computed from the shapes.  Also per (shape, dtype):
the dense loop's iteration (``morpho_iterate``, the same slope) for the SVI / dense ratio, and ``mvf_align_gather`` next to
the batch's ``mvf_assign`` (HIP events around repeated launches on prepared operands).  One JSON line per (shape, dtype).

    python tools/align_svi_bench.py --cells 10000 100000 --repeats 3 [--out profiles/align_svi.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from align_loop_bench import digamma, make_inputs  # noqa: E402


def composed(align, XA, XB, LA, LB, ctrl, common, iters, bs, perm, dtype, device):
    """`iters` SVI iterations from the public stages; returns (per-iteration seconds, {stage: seconds per iteration}, sigma2)."""
    NA, D = XA.shape
    NB, m = len(XB), len(ctrl)
    sigma2, gamma, s2v = common["sigma2"], 0.5, 1.0
    alpha, SigmaDiag, VnA = np.ones(NA), np.zeros(NA), np.zeros((NA, D))
    XAHat, RnA = XA.copy(), XA.copy()
    samples_s = float(max(np.prod(XA.max(0) - XA.min(0)), np.prod(XB.max(0) - XB.min(0))))
    anneal = 10.0 ** (1.0 / 100)
    Sp = Sp_spatial = Sp_sigma2 = 0.0
    SigmaInv, PXB_run = np.zeros((m, m)), np.zeros((NA, D))
    R, t = np.eye(D), np.zeros(D)
    times, stages = [], {"assign": 0.0, "nonrigid": 0.0, "glue": 0.0}
    for it in range(iters):
        t0 = time.perf_counter()
        step = min(1.0, 10.0 / (it + 1.0))
        idx = perm[(np.arange(bs) - it * bs) % NB]
        XBb, LBb = XB[idx], LB[idx]
        tg = time.perf_counter()
        a = align.update_assignment(XAHat, XBb, [LA], [LBb], dissimilarity=["kl"], probability_type=["gauss"],
                                    probability_parameters=[0.1], sigma2=sigma2, alpha=alpha, SigmaDiag=SigmaDiag, gamma=gamma,
                                    samples_s=samples_s, sigma2_variance=s2v, dtype=dtype, device=device)
        t1 = time.perf_counter()
        K_NA, K_NB, PXB = a["K_NA"], a["K_NB"], a["PXB"]
        raw = a["sigma2_related"] * (D * a["Sp_sigma2"])
        Sp = step * a["Sp"] + (1 - step) * Sp
        Sp_spatial = step * a["Sp_spatial"] + (1 - step) * Sp_spatial
        Sp_sigma2 = step * a["Sp_sigma2"] + (1 - step) * Sp_sigma2
        gamma = float(np.clip(np.exp(digamma(1.0 + Sp_spatial) - digamma(2.0 + bs)), 0.01, 0.99))
        alpha = step * np.exp(digamma(1.0 + a["K_NA_spatial"]) - digamma(1.0 * NA + Sp_spatial)) + (1 - step) * alpha
        PXB_term = PXB - RnA * K_NA[:, None]
        t2 = time.perf_counter()
        if it > 0:   # as the loop with nonrigid_start_iter = 0 (morpho_class.py:289): not in the first iteration
            nr = align.update_nonrigid(XA, ctrl, common["beta"], K_NA, PXB_term, sigma2, common["lambdaVF"], dtype=dtype,
                                       device=device, svi=dict(step_size=step, SigmaInv_prev=SigmaInv, PXB_prev=PXB_run))
            VnA, SigmaDiag, SigmaInv, PXB_run = nr["VnA"], nr["SigmaDiag"], nr["SigmaInv"], nr["PXB_term"]
        t3 = time.perf_counter()
        mu_A, mu_V, mu_B = K_NA @ XA / Sp, K_NA @ VnA / Sp, K_NB @ XBb / Sp
        XA_hat = XA - mu_A
        A = -(XA_hat.T @ ((VnA - mu_V) * K_NA[:, None]) - XA_hat.T @ (PXB - K_NA[:, None] * mu_B)).T
        U, _, V = np.linalg.svd(A)
        C = np.eye(D)
        C[-1, -1] = np.linalg.det(U @ V)
        Rn = U @ C @ V
        R = step * Rn + (1 - step) * R if step < 1 else Rn
        tn = (K_NB @ XBb - K_NA @ VnA - (K_NA @ XA) @ R.T) / Sp
        t = step * tn + (1 - step) * t if step < 1 else tn
        RnA = XA @ R.T + t
        XAHat = VnA + RnA
        sigma2 = max(raw / (D * Sp_sigma2) + float(a["K_NA_sigma2"] @ SigmaDiag) / Sp_sigma2, 1e-3)
        s2v = min(s2v * anneal, 10.0)
        sigma2 = max(sigma2, 1e-2)
        t4 = time.perf_counter()
        if it >= 1:
            times.append(t4 - t0)
            stages["assign"] += t1 - tg
            stages["nonrigid"] += t3 - t2
            stages["glue"] += (tg - t0) + (t2 - t1) + (t4 - t3)
    n = max(1, len(times))
    return times, {q: v / n for q, v in stages.items()}, sigma2


def gather_vs_assign(align, XA, XB, LA, LB, bs, perm, dtype, device, reps=20):
    """(mvf_align_gather ms, the batch's mvf_assign ms) per launch on prepared operands: HIP events around `reps` launches."""
    import torch

    from spateo_amd import _runtime as rt

    k = rt._make_kernels(device, dtype)
    layers = align._prepare_layers(k, [LA], [LB], [(2, 0, 0.1)])
    xa4, xb4, B64 = k.to_x4(XA), k.to_x4(XB), k.h2d_padded(XB, 3, torch.float64)
    dperm = k.h2d(perm.astype(np.int32))
    xb4_b, B64_b = k.empty(bs, 4), k.empty(bs, 3, dtype=torch.float64)
    Yp_b, b_b = [k.empty(bs, layers[0][4])], [k.empty(bs, dtype=torch.float64)]
    layers_b = [(layers[0][0], Yp_b[0], layers[0][2], b_b[0]) + tuple(layers[0][4:])]
    mm = torch.ones(len(XA), dtype=torch.float64, device=k.device)
    outlier = align._spatial_outlier(0.45, 0.5, 100.0, len(XA), 3)

    def timed(fn, n):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    g_ms = timed(lambda i=0: k.align_gather(dperm, (-i * bs) % len(XB), bs, xb4, B64, layers, xb4_b, B64_b, Yp_b, b_b), reps)
    a_ms = timed(lambda i=0: k.assign(xa4, xb4_b, layers_b, mm, 0.45, 1.0, outlier), max(3, reps // 5))
    return g_ms, a_ms


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
        bs = max(1, n // 10)
        perm = np.random.default_rng(1).permutation(n)
        common = dict(beta=0.5, lambdaVF=100.0, sigma2=0.45)
        kw = dict(dissimilarity=["kl"], probability_type=["gauss"], probability_parameters=[0.1], inducing_variables=ctrl,
                  nonrigid_start_iter=0, record=False, device=args.device, **common)
        for dtype in args.dtypes:
            def loop(iters, dense=False):
                t0 = time.perf_counter()
                if dense:
                    out = align.morpho_iterate(XA, XB, [LA], [LB], max_iter=iters, dtype=dtype, **kw)
                else:
                    out = align.morpho_iterate_svi(XA, XB, [LA], [LB], max_iter=iters, dtype=dtype, batch_size=bs, batch_perm=perm,
                                                   **kw)
                return time.perf_counter() - t0, out

            def comp(iters):
                return composed(align, XA, XB, LA, LB, ctrl, common, iters, bs, perm, dtype, args.device)

            loop(args.short), comp(2), loop(args.short, dense=True)                                  # warm-up of every form
            per_loop, per_comp, per_dense, st_comp = [], [], [], []
            for _ in range(args.repeats):                                                          # alternating
                ts, _ = loop(args.short)
                tl, out = loop(args.long)
                per_loop.append((tl - ts) / (args.long - args.short))
                times, stages, s2c = comp(args.long)
                per_comp.append(float(np.mean(times)))
                st_comp.append(stages)
                ts, _ = loop(args.short, dense=True)
                tl, _ = loop(args.long, dense=True)
                per_dense.append((tl - ts) / (args.long - args.short))
            rt.PROFILE_FITS = True
            try:
                loop(args.long)
                prof = dict(rt.last_fit_profile())
            finally:
                rt.PROFILE_FITS = False
            g_ms, a_ms = gather_vs_assign(align, XA, XB, LA, LB, bs, perm, dtype, args.device)
            its = args.long
            g, m = args.features, args.inducing
            line = dict(
                cells=n, batch=bs, features=g, inducing=m, dtype=dtype, repeats=args.repeats,
                loop_ms=1e3 * float(np.median(per_loop)), loop_ms_min=1e3 * min(per_loop), loop_ms_max=1e3 * max(per_loop),
                composed_ms=1e3 * float(np.median(per_comp)), composed_ms_min=1e3 * min(per_comp), composed_ms_max=1e3 * max(per_comp),
                dense_ms=1e3 * float(np.median(per_dense)), dense_ms_min=1e3 * min(per_dense), dense_ms_max=1e3 * max(per_dense),
                loop_split_ms=dict(assign=1e3 * prof["assign"] / its, nonrigid=1e3 * prof["nonrigid"] / (its - 1),
                                   glue=1e3 * prof["glue"] / its, setup_once=1e3 * prof["setup"], result_once=1e3 * prof["result"]),
                composed_split_ms={q: 1e3 * float(np.mean([s[q] for s in st_comp])) for q in st_comp[0]},
                gather_ms=g_ms, batch_assign_ms=a_ms,
                # bytes over the link per iteration: the loop reads its block and the solve's status words; the composed form
                # uploads XAHat, the batch's coordinates, the A layer and the batch's rows of the B layer, model_mul, then coordsA,
                # the control points, K_NA, two right-hand sides and SigmaInv_prev, and downloads four NA-vectors, K_NB, PXB, the
                # scalar, then SigmaInv (G and Gamma), Coff, VnA and SigmaDiag
                loop_link_bytes=64 * 8 + 4 + 8,
                composed_link_bytes=8 * (3 * n + 3 * bs + n * g + bs * g + n) + 8 * (3 * n + 3 * m + n + 2 * 3 * n + m * m)
                + 8 * (4 * n + bs + 3 * n + 1) + 8 * (2 * m * m + 3 * m + 3 * n + n),
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
