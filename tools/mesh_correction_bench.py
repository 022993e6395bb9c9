#!/usr/bin/env python
"""Timings of the mesh correction on the device, and of the reference on the CPU (profiles/mesh_correction.md).

    python tools/mesh_correction_bench.py gpu [--out FILE]     one optimisation step at the default 15 labels (2250 candidate
        transformations x 20 slices, a mesh of 10 000 triangles, contours of about 500 points), the split between cutting and
        ICP, a whole default run, and icp_batch at 45 000 problems
    python tools/mesh_correction_bench.py cpu                  the reference's own ICP and _calculate_loss (loaded from the
        reference checkout by tests/golden/make_golden_mesh_correction.py, with that script's stand-in cut) on a subset, scaled

Kernel time is taken with events on the launch stream around the C-ABI call, everything already on the device; the median of the
repeats after one warm-up call."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "spateo-release_amd"), ROOT):
    sys.path.insert(0, p)
import _icp_cases as ic  # noqa: E402

N_SLICES, LABELS = 20, 15
TRUTH = np.array([3.0, -2.0, 6.0, 0.8, 1.04])


def workload():
    """(verts, tri, heights, contours): 10 000 triangles, 20 heights, slice contours of 500 points cut from the moved mesh."""
    verts, tri = ic.ellipsoid(n_lat=21, n_lon=250, radii=(300.0, 220.0, 160.0), centre=(1000.0, 600.0, 400.0))
    heights = np.linspace(290.0, 510.0, N_SLICES)
    contours = []
    rng = np.random.default_rng(3)
    for c in ic.mesh_contours(verts, ic.unique_edges(tri), verts.mean(0), TRUTH, heights):
        pick = np.sort(rng.choice(len(c), min(500, len(c)), replace=False))
        contours.append(c[pick] + rng.standard_normal((len(pick), 2)) * 0.5)
    return verts, tri, heights, contours


def step_parameters(mc):
    """The 10 L^2 parameter sets of the first optimisation step at the default ranges, duplicates included."""
    rot = mc._generate_labeling(180, LABELS)
    labels = np.array([rot, rot, rot, mc._generate_labeling(0.5 * 220.0, LABELS), mc._generate_labeling(1.5, LABELS, "log")]).T
    return np.concatenate([mc._get_parameters_from_pair(p, labels).reshape(-1, 5) for p in mc._make_pairs()])


def gpu(out):
    import torch

    import spateo_amd as st
    from spateo_amd import _lib, _mesh_correction as mc, _runtime as rt

    lib = _lib.load()
    dev = "cuda:0"
    verts, tri, heights, contours = workload()
    edges = ic.unique_edges(tri)
    params = step_parameters(mc)
    res = dict(triangles=len(tri), edges=len(edges), slices=N_SLICES, transformations=len(params),
               contour_points=[int(np.mean([len(c) for c in contours]))], device=torch.cuda.get_device_name(0))
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    dv, de, dp, dh = t(verts), t(edges, np.int32), t(params), t(heights)
    flat = np.concatenate(contours)
    off = np.concatenate([[0], np.cumsum([len(c) for c in contours])]).astype(np.int64)
    dc, do = t(flat), t(off)
    nT, nS = len(params), N_SLICES
    loss, gamma = torch.empty(nT, dtype=torch.float64, device=dev), torch.empty(nT, nS, dtype=torch.float64, device=dev)
    count = torch.empty(nT, nS, dtype=torch.int32, device=dev)
    need = int(lib.mvf_mesh_loss_workspace_bytes(nT, nS))
    ws = torch.empty(need // 8 + 2, dtype=torch.float64, device=dev)
    m3 = (ctypes.c_double * 3)(*verts.mean(0))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn, repeats=5):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), [round(m, 3) for m in ms]

    def loss_call(max_iter):
        rc = lib.mvf_mesh_loss(dv.data_ptr(), len(verts), de.data_ptr(), len(edges), m3, dp.data_ptr(), nT, dh.data_ptr(), dc.data_ptr(),
                               do.data_ptr(), len(flat), nS, max_iter, 1e-6, 0.1, 0.05, 500, loss.data_ptr(), gamma.data_ptr(),
                               count.data_ptr(), ws.data_ptr(), need, stream)
        assert rc == 0, lib.mvf_last_error()

    res["step_kernel_ms"], res["step_kernel_ms_all"] = timed(lambda: loss_call(20))
    res["step_kernel_ms_max_iter_1"], _ = timed(lambda: loss_call(1))
    res["step_kernel_ms_max_iter_2"], _ = timed(lambda: loss_call(2))
    loss_call(20)
    torch.cuda.synchronize()
    cnt = count.cpu().numpy()
    res["cut_points_mean"] = float(cnt[cnt > 0].mean()) if (cnt > 0).any() else 0.0
    res["transformations_cut_everywhere"] = int((cnt > 0).all(axis=1).sum())
    # the cut alone: mvf_mesh_contours for as many (transformation, slice) cuts, one pass each (the loss kernel makes two)
    pts = torch.empty(nS, 2048, 2, dtype=torch.float64, device=dev)
    c32 = torch.empty(nS, dtype=torch.int32, device=dev)
    p5s = [(ctypes.c_double * 5)(*p) for p in params[:: len(params) // 50][:50]]

    def cuts():
        for p5 in p5s:
            lib.mvf_mesh_contours(dv.data_ptr(), len(verts), de.data_ptr(), len(edges), m3, p5, dh.data_ptr(), nS, 2048, pts.data_ptr(),
                                  c32.data_ptr(), stream)

    res["cut_50_transformations_ms"], _ = timed(cuts)
    # through the API: upload, call, read back
    k = rt._shared_kernels(dev, "float64")
    k.mesh_loss(k.mesh_upload(verts, edges), verts.mean(0), params[:50], heights, contours, 20, 1e-6, 0.1, 0.05, 500)
    t0 = time.perf_counter()
    st.align.mesh_correction_loss(contours, (verts, tri), params, heights)
    res["step_api_wall_s"] = time.perf_counter() - t0
    # a whole default run
    slices = [type("S", (), {"obsm": {"spatial": c}})() for c in contours]
    model = st.align.Mesh_correction(slices, heights, (verts, tri), contours=contours)
    t0 = time.perf_counter()
    model.run_discrete_optimization()
    res["default_run_wall_s"] = time.perf_counter() - t0
    res["default_run_losses"] = [float(v) for v in model.losses[1:]]
    res["default_run_best"] = {k2: np.asarray(v).tolist() for k2, v in model.best_transformation.items()}
    t0 = time.perf_counter()
    model.perform_correction()
    res["perform_correction_wall_s"] = time.perf_counter() - t0
    # icp_batch at 45 000 problems of 500 x 500 points (20 distinct pairs, repeated)
    kinds = [ic.icp_pair(500, 500, 40 + i, angle=2.0, shift=(0.5, 0.3)) for i in range(20)]
    c1 = [kinds[i % 20][0] for i in range(45000)]
    c2 = [kinds[i % 20][1] for i in range(45000)]
    k.icp_batch(c1[:100], c2[:100], 20, 1e-6, 0.1, 0.05, 500, True, want_T=False)
    t0 = time.perf_counter()
    g, stt, _, _ = k.icp_batch(c1, c2, 20, 1e-6, 0.1, 0.05, 500, True, want_T=False)
    res["icp_batch_45000_wall_s"] = time.perf_counter() - t0
    res["icp_batch_rounds_mean"] = float(stt[:, 0].mean())
    d1, d2 = t(np.concatenate(c1[:20])), t(np.concatenate(c2[:20]))
    gam, sta = torch.empty(45000, dtype=torch.float64, device=dev), torch.empty(45000, 2, dtype=torch.int32, device=dev)
    recs = np.zeros(45000, dtype=np.dtype([(f, np.int64) for f, _ in _lib.IcpProblem._fields_]))
    i = np.arange(45000)
    recs["contour_1"], recs["n1"] = d1.data_ptr() + (i % 20) * 8000, 500
    recs["contour_2"], recs["n2"] = d2.data_ptr() + (i % 20) * 8000, 500
    recs["gamma"], recs["stats"] = gam.data_ptr() + i * 8, sta.data_ptr() + i * 8
    wsb = int(lib.mvf_icp_batch_workspace_bytes(45000))
    w2 = torch.empty(wsb // 8, dtype=torch.float64, device=dev)
    rp = recs.ctypes.data_as(ctypes.POINTER(_lib.IcpProblem))
    res["icp_batch_45000_kernel_ms"], res["icp_batch_45000_kernel_ms_all"] = timed(
        lambda: lib.mvf_icp_batch(rp, 45000, 20, 1e-6, 0.1, 0.05, 500, 1, w2.data_ptr(), wsb, stream), repeats=3)
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as fh:
            fh.write(line + "\n")


def cpu():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_mesh_correction as mg

    mu = mg.load_utils()
    res = {}
    for n in (40, 120, 500):
        c1, c2 = ic.icp_pair(n, n, 40 + n, angle=2.0, shift=(0.5, 0.3))
        mu.ICP(c1, c2, allow_rotation=True)
        t0 = time.perf_counter()
        for _ in range(20):
            mu.ICP(c1, c2, allow_rotation=True)
        res[f"reference_icp_ms_{n}"] = (time.perf_counter() - t0) / 20 * 1e3
    verts, tri, heights, contours = workload()
    mu._transform_points = lambda pts, rot, tr, sc: ic.transform(pts, np.mean(pts, axis=0), [rot[0], rot[1], rot[2], tr, sc])
    mesh = mg.CutMesh(verts, ic.unique_edges(tri))
    from spateo_amd import _mesh_correction as mc

    params = step_parameters(mc)
    subset = params[:: len(params) // 8][:8]
    t0 = time.perf_counter()
    vals = [mu._calculate_loss(contours, mesh, p, heights, "ICP") for p in subset]
    per = (time.perf_counter() - t0) / len(subset)
    res.update(reference_loss_s_per_transformation=per, subset=len(subset), cut_everywhere=int(sum(v < 1e3 for v in vals)),
               reference_step_s_scaled=per * len(params), cpus=os.cpu_count())
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("gpu", "cpu"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gpu(a.out) if a.what == "gpu" else cpu()
