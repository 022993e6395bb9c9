"""NumPy stand-in for the ``pca_*`` methods of ``HipKernels`` (``spateo_amd._kernels``): what the host tests put behind the
kernel seam (``spateo_amd._runtime._make_kernels``) to run ``align.pca`` / ``align.group_pca`` without a GPU.  It restates
what the kernels compute - the means in float64, ``x - mean`` formed in float64 and rounded to the cell dtype, a float64 Gram
matrix of the stored values, scores accumulated in float64 and stored in the cell dtype - not how they do it."""
import numpy as np


class PcaCpuKernels:
    free_bytes = 1 << 40  # what mem_free() reports; a test lowers it to meet the refusal

    def __init__(self, device=None, dtype="float32"):
        self.dtype_name = dtype
        self.cell = np.float32 if dtype == "float32" else np.float64
        self.calls = []
        self._x = self._mu = None

    def mem_free(self):
        return int(self.free_bytes)

    def ublk_bytes(self, n, m):
        return np.dtype(self.cell).itemsize * (-(-int(n) // 256) * 256) * (-(-int(m) // 128) * 128)

    @staticmethod
    def _dense(sl):
        if sl[0] == "dense":
            return np.asarray(sl[1], dtype=np.float64)
        _, indptr, indices, data, n, g = sl
        out = np.zeros((n, g))
        for i in range(n):
            cols = indices[indptr[i] : indptr[i + 1]]
            keep = (cols >= 0) & (cols < g)
            out[i, cols[keep]] = data[indptr[i] : indptr[i + 1]][keep]
        return out

    def pca_open(self, n_total, g):
        self.calls.append("open")
        self._n, self._g = int(n_total), int(g)
        self._x = self._mu = None

    def pca_close(self):
        self.calls.append("close")
        self._x = self._mu = None

    def pca_means(self, slices):
        self.calls.append("means")
        X = np.vstack([self._dense(sl) for sl in slices])
        assert X.shape == (self._n, self._g)
        self._mu = X.sum(axis=0) / self._n
        return self._mu.copy()

    def pca_pack(self, slices, centred):
        self.calls.append("pack")
        X = np.vstack([self._dense(sl) for sl in slices])
        assert X.shape == (self._n, self._g)
        self._x = (X - self._mu if centred else X).astype(self.cell)

    def pca_gram(self):
        self.calls.append("gram")
        x = self._x.astype(np.float64)
        return x.T @ x

    def pca_scores(self, V):
        self.calls.append("scores")
        return (self._x.astype(np.float64) @ np.asarray(V, dtype=np.float64)).astype(self.cell).astype(np.float64)
