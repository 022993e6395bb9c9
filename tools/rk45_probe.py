"""Developer probe (GPU): the RK45 integrator (`mvf_integrate_rk45`) at BASELINE config 2's shape - 50 k trajectories,
M = 500 control points, interpolation_num = 250, arc-length sampling - against the RK4 arc-length path it is an
alternative to, in the same process, both dtypes.  Times
  - the RK45 launch alone (HIP events on its stream; two passes over the steps, sampling in the kernel),
  - the whole `integrate_field(..., integrator="rk45")` call (uploads, launch, one copy back),
  - the RK4 arc-length path: the fused RK4 launch (1001 dense samples x 2 substeps), `mvf_eval` on the dense samples and
    the host resampling, i.e. the whole `integrate_field(..., integrator="rk4")` call, plus its launch alone,
  - SciPy `solve_ivp` RK45 per cell (dynamo `fate`'s procedure, the oracle's restatement) on 200 cells, extrapolated.
Prints one JSON line; `--out PATH` also writes it to PATH.  Run under `rocprofv3 --kernel-trace --stats` for the kernel
rows."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spateo-release_amd"))
import numpy as np
import torch

import spateo_amd as st
from spateo_amd import _lib
from spateo_amd._kernels import HipKernels
from spateo_amd._synthetic import make_config
from spateo_amd.vectorfield import integrate_field

X, V, M = make_config("C2")
vf = st.SparseVFC(X, V, None, M=M, lambda_=0.02, lstsq_method="scipy", dtype="float32", device="cuda:0", MaxIter=30)
vf["method"] = "sparsevfc"
n, n_t, t_end = len(X), 250, 50.0
out = {"trajectories": n, "ctrl": M, "interpolation_num": n_t, "t_end": t_end, "sampling": "arc_length"}


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


for dtype in ("float32", "float64"):
    k = HipKernels("cuda:0", dtype)
    c = vf["X_ctrl"].mean(0)
    x4, c4 = k.to_x4(X, c), k.to_x4(vf["X_ctrl"], c)
    Cd = torch.from_numpy(np.ascontiguousarray(vf["C"])).cuda()
    res = {}
    # RK45 launch alone (device outputs allocated once; HIP events bracket the launches)
    buf_t = torch.empty(n, n_t, dtype=torch.float64, device="cuda:0")
    buf_x = torch.empty(n, n_t, 3, dtype=torch.float64, device="cuda:0")
    buf_s = torch.empty(n, 4, dtype=torch.int32, device="cuda:0")
    aff = None

    def launch():
        import ctypes

        w = (ctypes.c_double * 6)(1.0, 1.0, 1.0, *[float(v) for v in c])
        _lib.check(k.lib.mvf_integrate_rk45(x4.data_ptr(), n, c4.data_ptr(), c4.shape[0], float(vf["beta"]),
                                            Cd.data_ptr(), aff, 3, w, t_end, 1e-3, 1e-6, t_end / n_t, 100_000,
                                            _lib.RK45_ARC_LENGTH, n_t, buf_t.data_ptr(), buf_x.data_ptr(),
                                            buf_s.data_ptr(), k.cdtype, k._stream()), "mvf_integrate_rk45")

    launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        launch()
    e1.record()
    torch.cuda.synchronize()
    res["rk45_launch_ms"] = e0.elapsed_time(e1) / 3
    s = buf_s.cpu().numpy()
    res["rk45_accepted_mean"], res["rk45_accepted_max"] = float(s[:, 0].mean()), int(s[:, 0].max())
    res["rk45_rejected_mean"] = float(s[:, 1].mean())
    res["rk45_field_evals_mean_per_pass"] = float(s[:, 2].mean())
    res["rk45_status_counts"] = {str(v): int((s[:, 3] == v).sum()) for v in np.unique(s[:, 3])}
    # RK4 launch alone at the arc-length plan (1001 dense samples, 2 substeps each)
    dt = t_end / (4 * n_t)
    e0.record()
    for _ in range(3):
        tr = k.integrate(x4, c4, vf["beta"], Cd, dt, 2, 4 * n_t + 1)
        del tr
    e1.record()
    torch.cuda.synchronize()
    res["rk4_launch_ms"] = e0.elapsed_time(e1) / 3
    # whole calls
    res["rk45_integrate_field_ms"] = timed(lambda: integrate_field(vf, X, t_end=t_end, interpolation_num=n_t,
                                                                   integrator="rk45", dtype=dtype, device="cuda:0"))
    res["rk4_integrate_field_ms"] = timed(lambda: integrate_field(vf, X, t_end=t_end, interpolation_num=n_t,
                                                                  integrator="rk4", dtype=dtype, device="cuda:0"), reps=1)
    res["rk45_over_rk4_whole_call"] = res["rk45_integrate_field_ms"] / res["rk4_integrate_field_ms"]
    out[dtype] = res
    print(dtype, json.dumps(res), flush=True)

# SciPy per cell (the reference's procedure), 200 cells, extrapolated to all
from oracle import sparsevfc_oracle as svo  # noqa: E402
from oracle import trajectory_oracle as tro  # noqa: E402

vf64 = dict(X_ctrl=vf["X_ctrl"], C=vf["C"], beta=vf["beta"])
t0 = time.perf_counter()
tro.fate_arclength(lambda x: svo.vector_field_function(x, vf64), X[:200], t_end, n_t, "forward")
sec = time.perf_counter() - t0
out["scipy_200_cells_s"] = sec
out["scipy_extrapolated_s"] = sec / 200 * n
print(json.dumps(out))
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
