#!/usr/bin/env python
"""Sparse layers and the whole ``Morpho_pairwise`` call on one MI355X (``profiles/morpho_align.md``).

* ``--prepare``: ``HipKernels.assign_prepare`` from CSR against the dense path (the parent's behaviour: an n x g float64 host
  array, uploaded, then ``mvf_assign_prepare``) on the same matrix, ``--n`` x ``--g`` (default 100 000 x 2 000) with
  ``--density`` (default 5 %) of the entries set, ``kl``, both cell dtypes.  The two paths alternate, ``--repeats`` times each
  after a warm-up call; host clock around the call with a device synchronisation at both ends (the call starts from host
  arrays, the uploads are part of it); min - max.  Host bytes allocated are the peak of ``tracemalloc`` over one call, bytes
  over the link those of the arrays uploaded.  The outputs are compared bit for bit.
* ``--run``: a whole ``Morpho_pairwise(...).run()`` at ``--cells`` x ``--cells`` (default 10 000) cells with 50 ``kl`` count
  features as CSR ``.X``, the constructor's defaults but ``max_iter=--iters``: preprocessing (the constructor), start state,
  loop and output, split by wrapping ``align.morpho_start`` and the loop; host clock, synchronised.

One JSON line per measurement on stdout.

    python tools/morpho_align_bench.py --prepare --run [--out profiles/morpho_align.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import tracemalloc

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spateo-release_amd"))


def bench_prepare(args, emit):
    import torch

    from spateo_amd import _lib
    from spateo_amd._kernels import HipKernels, csr_arrays

    n, g = args.n, args.g
    rng = np.random.default_rng(0)
    M = sp.random(n, g, density=args.density, format="csr", random_state=rng, dtype=np.float64,
                  data_rvs=lambda k: rng.integers(1, 30, k).astype(np.float64))
    code = _lib.ASSIGN_METRICS["kl"]
    link_csr = sum(a.nbytes for a in csr_arrays(M)[:3])
    for dtype in ("float64", "float32"):
        k = HipKernels("cuda:0", dtype)

        def dense():
            return k.assign_prepare(M.toarray(), code, 0)

        def csr():
            return k.assign_prepare(M, code, 0)

        outs = {}
        for name, fn in (("dense", dense), ("csr", csr)):   # warm-up, and what each path allocates on the host
            tracemalloc.start()
            outs[name] = fn()
            torch.cuda.synchronize()
            outs[name + "_host_peak"] = tracemalloc.get_traced_memory()[1]
            tracemalloc.stop()
        same = all(bool(torch.equal(a, b)) for a, b in zip(outs["dense"][:2], outs["csr"][:2]))
        times = {"dense": [], "csr": []}
        for _ in range(args.repeats):
            for name, fn in (("dense", dense), ("csr", csr)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        for name in ("dense", "csr"):
            emit(dict(what=f"assign_prepare from {name}", n=n, g=g, nnz=int(M.nnz), dtype=dtype, seconds_min=min(times[name]),
                      seconds_max=max(times[name]), host_peak_bytes=int(outs[name + "_host_peak"]),
                      link_bytes=int(n * g * 8 if name == "dense" else link_csr), equal_bits=same))


def bench_run(args, emit):
    import torch

    import spateo_amd as st
    from spateo_amd import align

    n = args.cells
    rng = np.random.default_rng(1)
    Z = rng.uniform(-1.5, 1.5, (n, 3))
    src = rng.permutation(n)
    c, s = np.cos(0.35), np.sin(0.35)
    XA, XB = (Z - 0.4) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) * 40.0, (Z[src] + 0.02 * rng.standard_normal((n, 3))) * 40.0
    centres = rng.standard_normal((50, 3)) * 1.5
    rate = lambda P: 12.0 * np.exp(-((P[:, None, :] - centres[None]) ** 2).sum(-1) / 1.5) + 0.05  # noqa: E731
    A = st.AnnDataLite(X=sp.csr_matrix(rng.poisson(rate(Z)).astype(np.float64)), obsm={"spatial": XA})
    B = st.AnnDataLite(X=sp.csr_matrix(rng.poisson(rate(Z[src])).astype(np.float64)), obsm={"spatial": XB})
    phases = {}

    def timed(name, fn):
        def run(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            phases[name] = phases.get(name, 0.0) + time.perf_counter() - t0
            return out
        return run

    start, loop = align.morpho_start, align.morpho_iterate_svi
    align.morpho_start, align.morpho_iterate_svi = timed("start", start), timed("loop", loop)
    try:
        for dtype in ("float64", "float32"):
            rows = []
            for rep in range(args.repeats + 1):   # the first is the warm-up
                phases.clear()
                t0 = time.perf_counter()
                m = align.Morpho_pairwise(A, B, dtype=dtype, device="0", verbose=False, max_iter=args.iters, K=50, beta=1.0)
                phases["preprocessing"] = time.perf_counter() - t0
                m.run()
                total = time.perf_counter() - t0
                phases["output"] = total - sum(phases.values())
                rows.append(dict(phases, total=total))
            rows = rows[1:]
            emit(dict(what="Morpho_pairwise.run", cells=n, features=50, density=float(A.X.nnz) / (n * 50), dtype=dtype, iters=args.iters,
                      **{q: [min(r[q] for r in rows), max(r[q] for r in rows)] for q in rows[0]}, sigma2=float(m.sigma2),
                      rotation_error=float(np.linalg.norm(m.optimal_R @ m.init_R - np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])))))
    finally:
        align.morpho_start, align.morpho_iterate_svi = start, loop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prepare", action="store_true")
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--g", type=int, default=2000)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--cells", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    if args.prepare:
        bench_prepare(args, emit)
    if args.run:
        bench_run(args, emit)
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
