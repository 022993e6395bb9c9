"""Measurements of the kernel along the tissue (``csrc/mvf_graph.hip``, ``spateo_amd/_graph.py``) for profiles/geodist.md: every
stage of ``st.align.graph_kernel`` on a side stream between device events - the neighbour search (``mvf_knn``), the union of the
lists into CSR (torch), the shortest paths (``mvf_graph_sssp`` in batches of 32 sweeps, with the sweeps queued), the kernel
values - and one iteration of ``morpho_iterate`` with and without ``graph_kernel=`` (host clock around a call of three
iterations minus a call of two: the difference is an iteration with the non-rigid update).  One JSON line per measurement on
stdout and in ``--out``.

  python tools/graph_kernel_bench.py --out graph_kernel_bench.jsonl [--sizes 20000 100000 1000000] [--dims 2 3] [--m 40 200]
                                     [--ckdtree] [--loop-max 100000]
  python tools/graph_kernel_bench.py --cpu-only --ckdtree [--reference 2000]

``--ckdtree`` adds SciPy's ``cKDTree`` query of the same cloud on this host's CPU.  ``--cpu-only`` skips everything that needs a
GPU.  ``--reference N`` times the real ``construct_knn_graph`` + ``con_K_graph`` (40 inducing variables) on N points where the
reference checkout that the golden makers read is there (tests/golden/make_golden_em.py loads it).  Every shape is warmed up once; the median of
the repeats is reported with their spread.  The clouds are uniform in a box; a folded sheet would change the sweep count (the
graph's diameter), not the cost of a sweep."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "spateo-release_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from spateo_amd import _graph, align  # noqa: E402
from spateo_amd import _runtime as rt  # noqa: E402

DEV = "cuda:0"
KNN = 10
BETA = 0.01


def emit(fh, **rec):
    line = json.dumps(rec)
    print(line, flush=True)
    fh.write(line + "\n")
    fh.flush()


def median_spread(ts):
    ts = sorted(ts)
    return dict(median_ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1])


def timed(stream, fn, repeats):
    """fn() on the side stream between two events: (the last result, [ms])."""
    out, ts = fn(), []   # warm-up
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = fn()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return out, ts


def cloud(n, d):
    return np.random.default_rng(n + d).random((n, d)) * (1000.0 if d == 2 else 100.0)


def host_ckdtree(fh, X):
    from scipy.spatial import cKDTree

    t0 = time.perf_counter()
    cKDTree(X).query(X, KNN + 1)
    emit(fh, stage="cKDTree build + query (host CPU)", n=len(X), d=X.shape[1], k=KNN, seconds=time.perf_counter() - t0)


def host_reference(fh, n, d):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_em as mge

    _, _, utils = mge.load_morpho_class()
    X = cloud(n, d)
    idx = np.random.default_rng(40).choice(n, 40, replace=False)
    t0 = time.perf_counter()
    graph = utils.construct_knn_graph(X, KNN)
    t1 = time.perf_counter()
    utils.con_K_graph(graph, idx, beta=BETA)
    emit(fh, stage="reference (host CPU)", n=n, d=d, m=40, construct_knn_graph_s=t1 - t0, con_K_graph_s=time.perf_counter() - t1)


def stages(fh, n, d, ms, repeats, ckdtree):
    X = cloud(n, d)
    k = rt._shared_kernels(DEV, "float64")
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        Xd = k.h2d(X)
        (idx, dist), t = timed(side, lambda: k.knn(Xd, KNN), repeats)
        emit(fh, stage="knn", n=n, d=d, k=KNN, **median_spread(t))
        csr, t = timed(side, lambda: _graph._union(k, idx, dist, n), repeats)
        emit(fh, stage="union", n=n, d=d, edges=int(csr[1].shape[0]) // 2, **median_spread(t))
        graph = _graph.KnnGraph(n, dev=csr)
        for m in ms:
            src = k.h2d(np.random.default_rng(m).choice(n, m, replace=False).astype(np.int32))
            (D, sweeps), t = timed(side, lambda: k.graph_sssp(*csr, n, src), max(1, repeats // 2))
            emit(fh, stage="sssp", n=n, d=d, m=m, sweeps_queued=sweeps, unreachable=int(torch.isinf(D).sum()), **median_spread(t))
            _, t = timed(side, lambda: _graph._kernel_values(D, BETA), repeats)
            emit(fh, stage="kernel_values", n=n, d=d, m=m, **median_spread(t))
            del D
    if ckdtree:
        host_ckdtree(fh, X)
    return X, graph


def loop_iteration(fh, X, graph, m, repeats):
    """One morpho_iterate iteration with the non-rigid update, Euclidean and geodesic: a call of 3 iterations minus one of 2."""
    n, d = X.shape
    rng = np.random.default_rng(1)
    XB = X[rng.choice(n, n, replace=False)] + 0.01 * rng.standard_normal((n, d))
    LA = rng.random((n, 16))
    LB = LA[rng.choice(n, n)]
    idx = rng.choice(n, m, replace=False)
    gk = align.graph_kernel(X, idx, BETA, graph=graph, device=DEV)
    common = dict(dissimilarity="kl", probability_type="gauss", probability_parameters=[0.1], inducing_variables=X[idx], beta=BETA,
                  lambdaVF=100.0, sigma2=float(np.ptp(X, 0).mean() ** 2) * 1e-3, nonrigid_start_iter=0, device=DEV, record=False,
                  dtype="float32")
    for name, extra in (("euc", {}), ("geodist", dict(kernel_type="geodist", graph_kernel=gk))):
        ts = {}
        for iters in (2, 3):
            align.morpho_iterate(X, XB, [LA], [LB], max_iter=iters, **common, **extra)   # warm-up
            runs = []
            for _ in range(repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                align.morpho_iterate(X, XB, [LA], [LB], max_iter=iters, **common, **extra)
                runs.append(1e3 * (time.perf_counter() - t0))
            ts[iters] = sorted(runs)[len(runs) // 2]
        emit(fh, stage="morpho_iterate iteration", kernel=name, n=n, d=d, m=m, ms=ts[3] - ts[2], call_of_2_ms=ts[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="graph_kernel_bench.jsonl")
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 100000, 1000000])
    ap.add_argument("--dims", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--m", type=int, nargs="+", default=[40, 200])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ckdtree", action="store_true")
    ap.add_argument("--loop-max", type=int, default=100000, help="largest n at which the morpho_iterate iteration is timed")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--reference", type=int, default=0, help="points of the real reference's run (0: none)")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        if a.reference:
            for d in a.dims:
                host_reference(fh, a.reference, d)
        if a.cpu_only:
            for n in a.sizes if a.ckdtree else []:
                for d in a.dims:
                    host_ckdtree(fh, cloud(n, d))
            return
        assert torch.cuda.is_available(), "the measurements need a GPU"
        for n in a.sizes:
            for d in a.dims:
                X, graph = stages(fh, n, d, a.m, a.repeats, a.ckdtree)
                if n <= a.loop_max:
                    try:
                        loop_iteration(fh, X, graph, a.m[0], 3)
                    except Exception as e:   # (a measurement that cannot be taken is recorded, the others go on)
                        emit(fh, stage="morpho_iterate iteration", n=n, d=d, error=f"{type(e).__name__}: {e}"[:300])


if __name__ == "__main__":
    main()
