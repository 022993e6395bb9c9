"""TEST DOUBLE (never imported by the product): the sampler methods of ``HipKernels`` - ``trn``, ``nearest_rows``, ``kmeans`` - on
the float64 NumPy restatements of tests/_sample_cases.py, so that the host logic of ``st.align.trn`` / ``sample_by_kmeans`` /
``downsampling`` / ``morpho_align_ref`` runs behind the kernel seam without a GPU.  It is the checker standing in for the device,
not a fallback: the product binds only ``HipKernels``."""
import numpy as np

import _sample_cases as sc


class SampleCpuKernels:
    def __init__(self, device=None, dtype="float64"):
        self.device, self.dtype_name = device, dtype
        self.calls = {"trn": 0, "trn_problems": 0, "nearest_rows": 0, "kmeans": 0}

    def trn(self, problems):
        """The steps of ``mvf_trn`` from the host-made draws and schedules, as include/mvf.h states them."""
        self.calls["trn"] += 1
        self.calls["trn_problems"] += len(problems)
        out = []
        for pr in problems:
            X = np.asarray(pr["X"], dtype=np.float64)
            W = X[pr["w_idx"]].copy()
            n = len(W)
            K = np.empty(n, dtype=np.int64)
            for t, p in enumerate(pr["p_idx"]):
                D = X[p] - W
                sD = D[:, 0] * D[:, 0]
                for j in range(1, X.shape[1]):
                    sD = sD + D[:, j] * D[:, j]
                K[np.argsort(sD, kind="stable")] = np.arange(n)
                f = pr["ep"][t] * np.exp(-K[:, None] / pr["l"][t])
                move = np.ones(n, dtype=bool) if pr.get("kc") is None else K < pr["kc"][t]
                W[move] += f[move] * D[move]
            out.append(W)
        return out

    def nearest_rows(self, X, Q):
        self.calls["nearest_rows"] += 1
        return sc.nearest_restate(X, Q)

    def kmeans(self, X, C0, iters):
        self.calls["kmeans"] += 1
        C, labels, counts = sc.kmeans_restate(X, C0, iters)
        return C, labels, counts
