"""Measurements of ``st.tdr.kernel_density`` (``csrc/mvf_kde.hip``) for profiles/kde.md: the device against sklearn on the same
host, pairs/s at 100 k and 1 M points with 1 and 20 groups, and the same sums as a chunked ``torch.cdist`` + ``logsumexp`` on
the same GPU.  Needs a GPU; one JSON line per measurement on stdout and in ``--out``.

  python tools/kde_bench.py --out kde_bench.jsonl [--sizes 20000 100000 1000000] [--no-sklearn] [--no-torch]

Cloud: standard normal points in 3-D, h = 0.3.  Times: the API call is a host clock around a call that ends in the
device-to-host copy of the result; the kernel time is a pair of device events around ``mvf_kde`` alone, inputs already on the
device.  Every shape is warmed up once; the median of the repeats is reported with their spread."""
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

import spateo_amd as st  # noqa: E402
from spateo_amd import _lib  # noqa: E402
from spateo_amd import _runtime as rt  # noqa: E402

DEV = "cuda:0"
H = 0.3


def emit(fh, **rec):
    line = json.dumps(rec)
    print(line, flush=True)
    fh.write(line + "\n")
    fh.flush()


def cloud(N, seed=0):
    return np.random.default_rng(seed).standard_normal((N, 3))


def median_spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def time_api(X, kernel, dtype, groups, repeats):
    kw = dict(kernel=kernel, bandwidth=H, dtype=dtype, device=DEV, groups=groups)
    out = st.tdr.kernel_density(X, **kw)   # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = st.tdr.kernel_density(X, **kw)
        ts.append(time.perf_counter() - t0)
    return out, ts


def time_kernel(X, kernel, dtype, groups, C, repeats):
    """Device events around mvf_kde alone (one chunk of at most 64 columns)."""
    k = rt._shared_kernels(DEV, dtype)
    Xc = X - X.mean(axis=0)
    x4 = k.to_x4(Xc)
    g = None if groups is None else k.h2d(np.ascontiguousarray(groups, dtype=np.int32))
    n = len(X)
    need = int(k.lib.mvf_kde_workspace_bytes(n, n, C))
    ws = k.empty(max(need // 8, 1), dtype=torch.float64)
    out = k.empty(n, C, dtype=torch.float64)
    stream = torch.cuda.current_stream(DEV)

    def call():
        _lib.check(k.lib.mvf_kde(x4.data_ptr(), n, x4.data_ptr(), n, 3, _lib.KDE_KERNELS[kernel], H, None, None if g is None else g.data_ptr(),
                                 C, out.data_ptr(), ws.data_ptr(), ws.numel() * 8, k.cdtype, stream.cuda_stream), "mvf_kde")

    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return ts


def torch_chunked(X, kernel, tdtype, rows=4096, cols=65536):
    """The same log-density as a user writes it today: cdist in chunks, logsumexp (gaussian) or a clamped sum (epanechnikov)."""
    x = torch.from_numpy(X - X.mean(axis=0)).to(DEV, dtype=tdtype)
    n = x.shape[0]
    out = torch.empty(n, dtype=tdtype, device=DEV)
    for lo in range(0, n, rows):
        t = x[lo : lo + rows]
        acc = None
        for c0 in range(0, n, cols):
            # (the default mode, a matrix product for |x|^2 + |y|^2 - 2 x.y: what a user gets; the exact-difference mode launches one
            # workgroup per pair, and HIP refuses that grid from 2^24 pairs per call on)
            d = torch.cdist(t, x[c0 : c0 + cols])
            if kernel == "gaussian":
                part = torch.logsumexp(d.square_().mul_(-0.5 / (H * H)), dim=1)
                acc = part if acc is None else torch.logaddexp(acc, part)
            else:
                part = d.square_().mul_(-1.0 / (H * H)).add_(1.0).clamp_(min=0.0).sum(dim=1)
                acc = part if acc is None else acc + part
        out[lo : lo + rows] = acc if kernel == "gaussian" else acc.log()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="kde_bench.jsonl")
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 100000, 1000000])
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--torch-max", type=int, default=100000, help="largest size of the chunked torch baseline")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kde_bench.py needs a GPU"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    from spateo_amd.tdr.morphometrics.morphology import kde_log_norm

    with open(a.out, "w") as fh:
        emit(fh, what="device", name=torch.cuda.get_device_name(0), cus=torch.cuda.get_device_properties(0).multi_processor_count)
        for N in a.sizes:
            X = cloud(N)
            groups = np.random.default_rng(1).integers(0, 20, N)
            repeats = 5 if N <= 100000 else 2
            for kernel in ("gaussian", "epanechnikov"):
                results = {}
                for dtype in ("float64", "float32"):
                    for C, g in ((1, None), (20, groups)):
                        if C == 20 and N == 20000:
                            continue
                        out, ts = time_api(X, kernel, dtype, g, repeats)
                        med, lo, hi = median_spread(ts)
                        kt = median_spread(time_kernel(X, kernel, dtype, g, C, repeats))
                        results[(dtype, C)] = out
                        emit(fh, what="device", N=N, kernel=kernel, dtype=dtype, C=C, api_s=med, api_min_s=lo, api_max_s=hi,
                             kernel_s=kt[0], kernel_min_s=kt[1], kernel_max_s=kt[2], pairs_per_s_api=N * N / med,
                             pairs_per_s_kernel=N * N / kt[0], repeats=repeats)
                ref = results[("float64", 1)]
                if not a.no_torch and N <= a.torch_max:
                    for tdtype in (torch.float64, torch.float32):
                        torch_chunked(X[: min(N, 8192)], kernel, tdtype)   # warm-up of every op on a small shape
                        torch.cuda.synchronize()
                        ts = []
                        for _ in range(3 if N <= 100000 else 1):
                            t0 = time.perf_counter()
                            got = torch_chunked(X, kernel, tdtype)
                            torch.cuda.synchronize()
                            ts.append(time.perf_counter() - t0)
                        med, lo, hi = median_spread(ts)
                        got = got.double().cpu().numpy() + kde_log_norm(H, 3, kernel) - np.log(N)
                        fin = np.isfinite(ref) & np.isfinite(got)
                        emit(fh, what="torch_chunked", N=N, kernel=kernel, dtype=str(tdtype), s=med, min_s=lo, max_s=hi, pairs_per_s=N * N / med,
                             max_abs_diff_vs_device=float(np.abs(got[fin] - ref[fin]).max()),
                             mask_equal=bool(np.array_equal(np.isfinite(ref), np.isfinite(got))))
                if not a.no_sklearn and N <= 20000:
                    from sklearn.neighbors import KernelDensity

                    t0 = time.perf_counter()
                    sk = KernelDensity(kernel=kernel, bandwidth=H).fit(X).score_samples(X)
                    s = time.perf_counter() - t0
                    fin = np.isfinite(ref)
                    emit(fh, what="sklearn", N=N, kernel=kernel, s=s, pairs_per_s=N * N / s,
                         max_abs_diff_vs_device=float(np.abs(sk[fin] - ref[fin]).max()))


if __name__ == "__main__":
    main()
