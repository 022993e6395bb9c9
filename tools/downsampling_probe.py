#!/usr/bin/env python
"""Measurements behind profiles/downsampling.md (records, not gates), on cuda:0:

  trn      microseconds per TRN step at n = 2000 nodes, N = 100 000 cells, d = 3: one slice and 32 slices in one launch
           (host clock around ``HipKernels.trn``, which ends in a device synchronise; T = tmax n steps with a short tmax - the
           cost of a step does not depend on t), beside the vectorised NumPy restatement of tests/_sample_cases.py
  kmeans   ``st.align.sample_by_kmeans`` at N = 1 000 000, n = 2000, d = 3 against ``scipy.cluster.vq.kmeans2`` from the same start
  ref      ``st.align.morpho_align_ref`` end to end on a synthetic series of slices with TRN reference slices, split into
           sampling / alignment / transformation

    python tools/downsampling_probe.py OUT.json [trn] [kmeans] [ref] [--cells 1000000] [--slices 4]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "spateo-release_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def _sync():
    import torch

    torch.cuda.synchronize()


def probe_trn(out):
    import _sample_cases as sc
    from spateo_amd import _runtime as rt
    from spateo_amd._downsampling import trn_schedule

    N, d, n, tmax = 100_000, 3, 2000, 10
    X = sc.uniform_cloud(N, d, seed=1)
    T, l, ep, kc = trn_schedule(n, tmax=tmax)
    k = rt._shared_kernels("cuda:0", "float64")

    def problems(count, steps):
        ps = []
        for s in range(count):
            rs = np.random.RandomState(100 + s)
            ps.append(dict(X=X, w_idx=rs.randint(0, N, n), p_idx=rs.randint(0, N, steps), l=l[:steps], ep=ep[:steps], kc=None))
        return ps

    res = {"N": N, "d": d, "n": n, "steps": T}
    for count in (1, 32):
        k.trn(problems(count, 64))                       # warm-up: code object, staging buffers
        _sync()
        t0 = time.perf_counter(); k.trn(problems(count, 0)); _sync(); base = time.perf_counter() - t0   # uploads, no steps
        times = []
        for _ in range(3):
            ps = problems(count, T)
            t0 = time.perf_counter(); k.trn(ps); _sync(); times.append(time.perf_counter() - t0)
        res[f"slices_{count}"] = {"call_s": times, "call_without_steps_s": base,
                                  "us_per_step": 1e6 * (float(np.median(times)) - base) / T,
                                  "us_per_step_per_slice": 1e6 * (float(np.median(times)) - base) / T / count}
    steps = 2000
    t0 = time.perf_counter(); sc.trn_restate(X, n, tmax=steps / n); host = time.perf_counter() - t0
    res["numpy_restatement_us_per_step"] = 1e6 * host / steps
    out["trn"] = res


def probe_kmeans(out):
    from scipy.cluster.vq import kmeans2

    import _sample_cases as sc
    from spateo_amd import align

    N, n, d = 1_000_000, 2000, 3
    X = sc.uniform_cloud(N, d, seed=2)
    C0 = X[np.random.default_rng(0).choice(N, n, replace=False)]
    align.sample_by_kmeans(X[:10000], 50, init=C0[:50], device="cuda:0")          # warm-up
    times = []
    for _ in range(3):
        t0 = time.perf_counter(); idx = align.sample_by_kmeans(X, n, return_index=True, init=C0, iter=10, device="cuda:0")
        times.append(time.perf_counter() - t0)
    t0 = time.perf_counter(); C2, lab2 = kmeans2(X, C0.copy(), iter=2, minit="matrix"); host2 = time.perf_counter() - t0
    from spateo_amd import _runtime as rt

    C_dev, lab_dev, _ = rt._shared_kernels("cuda:0", "float64").kmeans(X, C0, 2)
    out["kmeans"] = {"N": N, "n": n, "d": d, "sample_by_kmeans_iter10_s": times, "kmeans2_iter2_s": host2,
                     "kmeans2_s_per_iteration": host2 / 2, "labels_equal_after_2_iterations": bool(np.array_equal(lab_dev, lab2)),
                     "centroid_deviation_over_extent": float(np.abs(C_dev - C2).max() / np.abs(X).max()),
                     "distinct_cells": int(len(np.unique(idx)))}


def synthetic_series(cells, slices, genes=16, seed=0):
    from spateo_amd import AnnDataLite
    from spateo_amd._synthetic import embryo_cloud

    rng = np.random.default_rng(seed)
    freq = rng.uniform(0.5, 2.5, (genes, 3)) / np.array([2000.0, 1200.0, 900.0])
    models = []
    for s in range(slices):
        P = embryo_cloud(rng, cells)
        lam = 2.0 * np.exp(np.sin(2 * np.pi * (P @ freq.T) + np.arange(genes)))                  # smooth expression patterns
        counts = rng.poisson(lam).astype(np.float32)
        counts[:, 0] += 1.0                                                                          # no all-zero cell
        a = 0.15 * s
        R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        moved = (P + 15.0 * np.sin(P[:, [1, 2, 0]] / 400.0)) @ R.T + np.array([120.0, -80.0, 40.0]) * s
        models.append(AnnDataLite(X=counts, obsm={"spatial": moved}))
    return models


def probe_ref(out, cells, slices):
    from spateo_amd import align

    models = synthetic_series(cells, slices)
    kw = dict(dtype="float32", device="cuda:0", verbose=False, iter_key_added=None)
    align.morpho_align_ref(synthetic_series(3000, 2, seed=1), n_sampling=200, sampling_method="trn", max_iter=5, **kw)   # warm-up
    _sync()
    t0 = time.perf_counter(); refs = align.downsampling(models, n_sampling=2000, sampling_method="trn"); _sync()
    t_sampling = time.perf_counter() - t0
    t0 = time.perf_counter(); align.morpho_align(refs, **kw); _sync(); t_align = time.perf_counter() - t0
    t0 = time.perf_counter(); res = align.morpho_align_ref(models, models_ref=refs, **kw); _sync(); t_rest = time.perf_counter() - t0
    moved = [float(np.abs(m.obsm["align_spatial"] - m.obsm["spatial"]).max()) for m in res[0]]
    out["morpho_align_ref"] = {"cells_per_slice": cells, "slices": slices, "reference_cells": [r.n_obs for r in refs],
                               "sampling_s": t_sampling, "alignment_of_reference_slices_s": t_align,
                               "align_ref_given_reference_slices_s": t_rest, "transformation_and_copies_s": t_rest - t_align,
                               "end_to_end_s": t_sampling + t_rest, "max_displacement_per_slice": moved}


def main():
    args = sys.argv[1:]
    path = args[0]
    which = [a for a in args[1:] if a in ("trn", "kmeans", "ref")] or ["trn", "kmeans", "ref"]
    cells = int(args[args.index("--cells") + 1]) if "--cells" in args else 1_000_000
    slices = int(args[args.index("--slices") + 1]) if "--slices" in args else 4
    out = {}
    for name in which:
        t0 = time.perf_counter()
        {"trn": probe_trn, "kmeans": probe_kmeans, "ref": lambda o: probe_ref(o, cells, slices)}[name](out)
        print(name, "done in %.1f s" % (time.perf_counter() - t0), json.dumps(out.get({"ref": "morpho_align_ref"}.get(name, name))), flush=True)
        with open(path, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
