"""Developer probe (GPU): the 4- to 8-dimensional path against the 3-D one, float32 cells unless stated.
  - kernel-value cache build at 2 M cells x 2000 control points: D = 3 (`mvf_ublk_build`, x4 rows) against D = 4, 8
    (`mvf_ublk_build_d`), float32 and float64 cells, ms per build and the HBM write rate (n_pad m_pad sizeof(dtype) bytes),
  - one EM iteration at D = 5 against D = 3 (same N, M, Dy = 5: the cached wide rhs / apply path in both),
  - the evaluator (`mvf_eval_d`) on 64^3 query points, M = 500, D = 4 and 8: every quantity, and v alone; the 3-D
    `mvf_eval` on the same count beside it.
Times are HIP events around the launches after a warm-up.  Prints one JSON line and writes it to `--out`
(default profiles/highd_probe.json).  Run under `rocprofv3 --kernel-trace` for the per-kernel rows (tools/rocpd_summary.py
turns its database into the table of profiles/highd_kernel_stats.md)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spateo-release_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "highd_probe.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch

    from spateo_amd import _lib
    from spateo_amd._kernels import HipKernels
    from spateo_amd.engine import SparseVFCEngine

    dev = "cuda:0"
    rng = np.random.default_rng(0)

    def timed(fn, reps=a.reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def cloud(n, d):
        return rng.standard_normal((n, d)) * np.linspace(300.0, 120.0, d)

    out = {"dtype": "float32"}
    # ---- cache build, 2 M x 2000
    n, m, beta = 2_000_000, 2000, 1e-4
    for dtype, dims in (("float32", (3, 4, 8)), ("float64", (3, 4, 8))):
        k = HipKernels(dev, dtype)
        n_pad, m_pad = k.wide_pads(n, m)
        nbytes = n_pad * m_pad * (4 if dtype == "float32" else 8)
        build = {}
        for d in dims:
            X = cloud(n, d)
            ctrl = X[:m]
            c = ctrl.mean(0)
            if d == 3:
                x, cc = k.to_x4(X, c), k.to_x4(ctrl, c)
                ms = timed(lambda: k.build_ublk(x, cc, beta))
            else:
                x, cc = k.to_xd(X, c), k.to_xd(ctrl, c)
                ms = timed(lambda: k.build_ublk_d(x, cc, beta))
            build[f"D{d}"] = {"ms": ms, "TB_s": nbytes / ms / 1e9}
            k.drop_ublk()
            del x, cc
            torch.cuda.empty_cache()
        out["cache_build_2Mx2000" + ("" if dtype == "float32" else "_float64")] = {"bytes": nbytes, **build}
        del k
        torch.cuda.empty_cache()
    # ---- one EM iteration, D = 5 against D = 3, Dy = 5
    n, m = 1_000_000, 1000
    em = {}
    for d in (3, 5):
        X = cloud(n, d)
        Y = rng.standard_normal((n, 5))
        ctrl = X[rng.choice(n, m, replace=False)]
        eng = SparseVFCEngine(X, Y, ctrl, 1e-4, dtype="float32", device=dev)
        eng.init_state()
        for _ in range(2):
            eng.em_step(lambda_=0.02)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        steps = 3
        for _ in range(steps):
            eng.em_step(lambda_=0.02)
        e1.record()
        torch.cuda.synchronize()
        em[f"D{d}"] = {"ms_per_em_step": e0.elapsed_time(e1) / steps, "wide": bool(eng.wide)}
        del eng
        torch.cuda.empty_cache()
    out["em_step_1Mx1000_dy5"] = em
    # ---- evaluator, 64^3 queries, M = 500
    nq, m = 64**3, 500
    k = HipKernels(dev, "float32")
    ev = {}
    for d in (3, 4, 8):
        Q = cloud(nq, d)
        ctrl = cloud(m, d)
        C = torch.from_numpy(rng.standard_normal((m, d))).to(dev)
        c = ctrl.mean(0)
        if d == 3:
            q4, c4 = k.to_x4(Q, c), k.to_x4(ctrl, c)
            every = _lib.EVAL_V | _lib.EVAL_JAC | _lib.EVAL_DIV | _lib.EVAL_ACC | _lib.EVAL_CURV
            ev["D3"] = {"all_ms": timed(lambda: k.eval(q4, c4, 5e-5, C, every)),
                        "v_ms": timed(lambda: k.eval(q4, c4, 5e-5, C, _lib.EVAL_V))}
        else:
            qd, cd = k.to_xd(Q, c), k.to_xd(ctrl, c)
            every = _lib.EVAL_V | _lib.EVAL_JAC | _lib.EVAL_DIV | _lib.EVAL_ACC | _lib.EVAL_CURV
            ev[f"D{d}"] = {"all_ms": timed(lambda: k.eval_d(qd, cd, 5e-5, C, every)),
                           "v_ms": timed(lambda: k.eval_d(qd, cd, 5e-5, C, _lib.EVAL_V))}
    out["eval_64cube_M500"] = ev
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
