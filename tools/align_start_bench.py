#!/usr/bin/env python
"""The alignment's start state on one MI355X (``profiles/align_start.md``).

* ``--kernel``: ``mvf_assign_layer_stats`` at ``--n`` x ``--n`` (default 20 000, the reference's subsample) for ``kl`` at 2000
  features and ``cos`` at 50, with k = 0 and k = 10: device time between two stream events around the call (operands on the
  device; the median of ``--repeats`` after a warm-up call), and its fraction of the float64 matrix peak,
  2 n n G' flop / time / 78.6 Tflop/s (G' = the padded feature count).  ``--numpy`` adds the dense NumPy form on the host's
  CPUs: the n x n float64 distance matrix of the same metric, its row minima and ``np.argpartition`` over both axes, with the
  bytes it allocates.
* ``--start``: the whole ``morpho_start`` call at ``--cells`` x ``--cells`` (default 100 000) cells, 50 count features, 500
  inducing variables, host clock around the call (it ends in device-to-host copies); the host voxelisation alone next to it.

One JSON line per measurement on stdout.

    python tools/align_start_bench.py --kernel --numpy --start [--out profiles/align_start.json]
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
F64_MATRIX_PEAK = 78.6e12


def layers(rng, n, g, metric):
    if metric == "kl":
        prof = rng.gamma(0.6, 4.0, (5, g))
        return rng.poisson(prof[rng.integers(0, 5, n)]).astype(np.float64), rng.poisson(prof[rng.integers(0, 5, n)]).astype(np.float64)
    return rng.standard_normal((n, g)), rng.standard_normal((n, g))


def numpy_form(A, B, metric, k):
    """The dense form: (seconds, bytes of the matrices it allocates).  The distance as the reference's back ends state it."""
    t0 = time.perf_counter()
    if metric == "kl":
        X, Y = A + 0.01, B + 0.01
        X, Y = X / X.sum(1, keepdims=True), Y / Y.sum(1, keepdims=True)
        d = (X * np.log(X + 1e-8)).sum(1, keepdims=True) - X @ np.log(Y + 1e-8).T
    else:
        X = A / np.maximum(np.linalg.norm(A, axis=1, keepdims=True), 1e-8)
        Y = B / np.maximum(np.linalg.norm(B, axis=1, keepdims=True), 1e-8)
        d = 0.5 - 0.5 * (X @ Y.T)
    nbytes = d.nbytes
    d.min(1)
    if k:
        i0 = np.argpartition(d, k, axis=0)[:k]
        i1 = np.argpartition(d, k, axis=1)[:, :k]
        nbytes += 2 * d.shape[0] * d.shape[1] * 8        # argpartition returns a full index matrix per axis
        del i0, i1
    return time.perf_counter() - t0, nbytes


def bench_kernel(args, emit):
    import torch

    from spateo_amd import _lib
    from spateo_amd._kernels import HipKernels

    n = args.n
    for metric, g in (("kl", 2000), ("cos", 50)):
        rng = np.random.default_rng(0)
        A, B = layers(rng, n, g, metric)
        for dtype in ("float64", "float32"):
            kk = HipKernels("cuda:0", dtype)
            code = _lib.ASSIGN_METRICS[metric]
            Xp, a, ld = kk.assign_prepare(A, code, 0)
            Yp, b, _ = kk.assign_prepare(B, code, 1)
            layer = (Xp, Yp, a, b, ld, code, 2, 0.0)
            for k in (0, 10):
                kk.assign_layer_stats(layer, n, n, k)
                torch.cuda.synchronize()
                times = []
                for _ in range(args.repeats):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = kk.assign_layer_stats(layer, n, n, k)
                    e1.record()
                    torch.cuda.synchronize()
                    times.append(e0.elapsed_time(e1) * 1e-3)
                t = float(np.median(times))
                emit(dict(what="mvf_assign_layer_stats", n=n, metric=metric, features=g, padded=int(ld), dtype=dtype, k=k, seconds=t,
                          min=min(times), max=max(times), fraction_of_f64_matrix_peak=2.0 * n * n * ld / t / F64_MATRIX_PEAK,
                          workspace_bytes=int(kk.lib.mvf_assign_layer_stats_workspace_bytes(n, n, k)),
                          sum_d=float(out["sums"][0].cpu())))
        if args.numpy:
            for k in (0, 10):
                sec, nbytes = numpy_form(A, B, metric, k)
                emit(dict(what="numpy dense form", n=n, metric=metric, features=g, k=k, seconds=sec, matrix_bytes=nbytes,
                          omp_num_threads=os.environ.get("OMP_NUM_THREADS")))


def bench_start(args, emit):
    import torch

    from spateo_amd import align

    n = args.cells
    rng = np.random.default_rng(1)
    Z = rng.uniform(-1.5, 1.5, (n, 3))
    src = rng.permutation(n)
    XB = Z[src] + 0.02 * rng.standard_normal((n, 3))
    c, s = np.cos(0.35), np.sin(0.35)
    XA = (Z - 0.4) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    centres = rng.standard_normal((50, 3)) * 1.5
    rate = lambda P: 12.0 * np.exp(-((P[:, None, :] - centres[None]) ** 2).sum(-1) / 3.0) + 0.3  # noqa: E731
    LA, LB = rng.poisson(rate(Z)).astype(np.float64), rng.poisson(rate(Z[src])).astype(np.float64)
    # the two host stages timed inside the call: the voxelisation (twice per call) and inlier_from_NN
    host = {"voxel_data": 0.0, "inlier_from_NN": 0.0}
    voxels = []

    def timed(name, fn):
        def run(*a, **k):
            t0 = time.perf_counter()
            out = fn(*a, **k)
            host[name] += time.perf_counter() - t0
            if name == "voxel_data":
                voxels.append(len(out[0]))
            return out
        return run

    align._voxel_data, align._pair_inlier_fit = timed("voxel_data", align._voxel_data), timed("inlier_from_NN", align._pair_inlier_fit)
    for dtype in ("float64", "float32"):
        kw = dict(dissimilarity="kl", probability_type="gauss", inducing_variables_num=500, dtype=dtype, device="cuda:0")
        align.morpho_start(XA, XB, LA, LB, **kw)
        times = []
        host.update(voxel_data=0.0, inlier_from_NN=0.0)
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = align.morpho_start(XA, XB, LA, LB, **kw)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        emit(dict(what="morpho_start", cells=n, features=50, dtype=dtype, seconds=float(np.median(times)), min=min(times),
                  max=max(times), voxel_data_seconds_per_call=host["voxel_data"] / args.repeats,
                  inlier_from_NN_seconds_per_call=host["inlier_from_NN"] / args.repeats, voxels=voxels[-2:], sigma2=st["sigma2"],
                  parameters=st["probability_parameters"], inliers=len(st["inliers"][2]),
                  rotation_error=float(np.linalg.norm(st.init_R - np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--start", action="store_true")
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    if args.kernel:
        bench_kernel(args, emit)
    if args.start:
        bench_start(args, emit)
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
