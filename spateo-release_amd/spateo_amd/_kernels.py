"""Thin Python layer over the libmvf C ABI: torch supplies device memory and the HIP stream, nothing else.

Every method launches hand-written HIP kernels asynchronously on torch's current stream of ``device`` and returns
device tensors.  Nothing here computes on the host and nothing falls back to torch/NumPy arithmetic.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib

_DT = {"float32": (torch.float32, _lib.MVF_F32), "float64": (torch.float64, _lib.MVF_F64)}
_NP = {torch.float64: np.float64, torch.float32: np.float32, torch.int32: np.int32, torch.int64: np.int64}


def _ptr(t):
    return None if t is None else t.data_ptr()


class Layer(NamedTuple):
    """One prepared layer of the assignment step, the record every HipKernels method that takes layers reads (a plain
    8-sequence in this order is accepted too).  A product layer: Xp (na, ld) / Yp (nb, ld) in the cell dtype and a (na,) /
    b (nb,) float64 from assign_prepare.  A label layer (metric == _lib.ASSIGN_LABEL): Xp the (K, L) float64 table, Yp
    None, a / b the labels of the A / B cells from assign_label_prepare, ld = L.  prob and param: the probability type
    and its parameter (include/mvf.h)."""
    Xp: object
    Yp: object
    a: object
    b: object
    ld: int
    metric: int
    prob: int
    param: float

    @property
    def is_label(self):
        return self.metric == _lib.ASSIGN_LABEL

    def exchanged(self):
        """The layer whose column statistics are this one's row statistics: Xp <-> Yp, a <-> b (na <-> nb is the caller's)."""
        return self._replace(Xp=self.Yp, Yp=self.Xp, a=self.b, b=self.a)

    def with_columns(self, Yp, b):
        """The same layer over another set of B rows (an SVI batch)."""
        return self._replace(Yp=Yp, b=b)


def layer_array(layers):
    """The layers as the C ABI takes them, (_lib.AssignLayer * max(len(layers), 1)), every field set; a missing Yp is NULL."""
    arr = (_lib.AssignLayer * max(len(layers), 1))()
    for s, t in zip(arr, layers):
        L = Layer(*t)
        s.Xp, s.Yp, s.a, s.b, s.ld = _ptr(L.Xp), _ptr(L.Yp), _ptr(L.a), _ptr(L.b), int(L.ld)
        s.metric, s.prob, s.param = int(L.metric), int(L.prob), float(L.param)
    return arr


def is_sparse(layer):
    """A scipy.sparse matrix / array (SciPy is imported only where one may have been handed in)."""
    if isinstance(layer, (np.ndarray, list, tuple)) or torch.is_tensor(layer):
        return False
    import scipy.sparse as sp

    return sp.issparse(layer)


CSR_STAGING_MAX_BYTES = 64 << 20  # staging rows of mvf_assign_prepare_csr (g float64 each): at most this much, and
CSR_STAGING_MAX_ROWS = 16384      # no more rows than the library launches blocks of four for


def csr_arrays(layer):
    """A scipy.sparse layer -> (indptr int64, indices int32, data float32 | float64, n, g), the host arrays
    mvf_assign_prepare_csr reads, in O(nnz): canonical CSR (duplicates summed on a copy), integer counts cast to
    float64.  indptr is checked here (non-decreasing from >= 0, ending inside `data`), before anything is launched."""
    m = layer.tocsr()
    n, g = m.shape
    if g > np.iinfo(np.int32).max:
        raise ValueError(f"a sparse layer may have at most 2^31 - 1 columns (int32 column indices), got {g}")
    indptr = np.asarray(m.indptr)
    if indptr.shape != (n + 1,) or indptr[0] < 0 or (np.diff(indptr) < 0).any() or indptr[-1] > len(m.data) or len(m.indices) != len(m.data):
        raise ValueError("malformed CSR layer: indptr must have n + 1 non-decreasing entries from >= 0 that end inside data")
    if not m.has_canonical_format:
        m = m.copy()
        m.sum_duplicates()
        indptr = np.asarray(m.indptr)
    data = np.asarray(m.data)
    if data.dtype not in (np.float32, np.float64):
        data = data.astype(np.float64)
    return (np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(m.indices, dtype=np.int32),
            np.ascontiguousarray(data), int(n), int(g))


def pca_slices(mats):
    """The per-slice matrices of `align.pca` as the kernels' pca_* methods take them, validated on the host: a dense slice
    -> ("dense", C-contiguous (n, g) float32 | float64 array; other dtypes become float64), a scipy.sparse slice -> ("csr",
    indptr, indices, data, n, g) from `csr_arrays`.  Equal column counts and finite values, or ValueError - checked chunk by
    chunk, without a boolean copy of a whole slice."""
    out, g = [], None
    for i, m in enumerate(mats):
        if is_sparse(m):
            sl = ("csr",) + csr_arrays(m)
            shape, values = (sl[4], sl[5]), sl[3][None, :]
        else:
            a = np.asarray(m)
            if a.ndim != 2:
                raise ValueError(f"slice {i}: expected an (n, g) matrix, got shape {a.shape}")
            a = np.ascontiguousarray(a, dtype=a.dtype if a.dtype in (np.float32, np.float64) else np.float64)
            sl, shape, values = ("dense", a), a.shape, a
        if g is None:
            g = shape[1]
        if shape[1] != g:
            raise ValueError(f"slice {i} has {shape[1]} columns, slice 0 has {g}")
        step = max(1, (1 << 22) // max(1, values.shape[1]))
        for lo in range(0, values.shape[0], step):
            if not np.isfinite(values[lo : lo + step]).all():
                raise ValueError(f"slice {i} holds non-finite values")
        out.append(sl)
    return out, (0 if g is None else int(g))


def _on_device(fn):
    """Run a kernel method with the instance's GPU as the thread's current HIP device: libmvf launches on the stream it
    is handed, but hipFuncSetAttribute / hipMemsetAsync / occupancy queries inside it act on the CURRENT device, which
    need not be `self.device` (SparseVFC(device="cuda:1") without set_device, SparseVFC_many threads)."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *a, **kw):
        if torch.cuda.current_device() == self._dev_index:  # the usual case: no context switch (microseconds per launch,
            return fn(self, *a, **kw)                        # exposed at the head of a sub-millisecond EM iteration)
        with torch.cuda.device(self.device):
            return fn(self, *a, **kw)

    return wrapped


class HipKernels:
    """libmvf kernels bound to one GPU and one cell dtype ("float32" | "float64")."""

    def __init__(self, device=None, dtype="float32"):
        if not torch.cuda.is_available():
            raise RuntimeError(
                "spateo_amd needs an AMD GPU (HIP device) - torch.cuda.is_available() is False and there is no "
                "CPU fallback for the SparseVFC path."
            )
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._gram_need = {}
        if dtype not in _DT:
            raise ValueError(f"dtype must be 'float32' or 'float64', got {dtype!r}")
        self.dtype_name = dtype
        self.tdtype, self.cdtype = _DT[dtype]
        self._gram_ws = None
        self._solve_ws = None
        self._mn_ws = None
        self._lr_ws = None
        self._mins = torch.empty(_lib.MVF_ESTEP_MIN_DOUBLES, dtype=torch.float64, device=self.device)
        self._scratch = None  # per-workgroup partials of the deterministic reductions (apply / estep_p / quadform)
        # optional per-launch timing of the dominant (Gram MFMA) kernel: list of (start, end) torch events recorded
        # on the launch stream; bench.py sets this to [] to enable it
        self.gram_events = None
        self._ublk = None       # cached float32 kernel values (layout Ublk[m/16][n][16]) for the Gram kernel
        self._ublk_key = None
    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    @_on_device
    def to_x4(self, arr, center=None):
        """Host (n, d<=3) float64 array -> device (n, 4) tensor of the cell dtype (zero padded), optionally centred."""
        a = np.asarray(arr, dtype=np.float64)
        if a.ndim != 2 or not (1 <= a.shape[1] <= 3):
            raise ValueError(f"expected an (n, d) array with d <= 3, got shape {a.shape}")
        c = None if center is None else np.asarray(center, dtype=np.float64)[None, : a.shape[1]]
        return self.h2d_padded(a, 4, self.tdtype, minus=c)

    @_on_device
    def to_xd(self, arr, center=None):
        """Host (n, d) float64 array, 4 <= d <= 8 -> device (n, d) tensor of the cell dtype (plain rows: what
        mvf_ublk_build_d / mvf_eval_d read), optionally centred - the same float64 subtraction and rounding as to_x4."""
        a = np.asarray(arr, dtype=np.float64)
        if a.ndim != 2 or not (4 <= a.shape[1] <= 8):
            raise ValueError(f"expected an (n, d) array with 4 <= d <= 8, got shape {a.shape}")
        c = None if center is None else np.asarray(center, dtype=np.float64)[None, : a.shape[1]]
        return self.h2d_padded(a, a.shape[1], self.tdtype, minus=c)

    # pinned staging: host arrays up to this size travel through page-locked tensors of torch's caching host allocator
    # (one DMA, no driver-side bounce copies); larger ones keep the pageable path so that a fit of 8 M cells does not
    # leave hundreds of MB of the host page-locked for the life of the process
    PINNED_MAX_BYTES = 128 << 20
    DEVICE_PAD_MIN_ROWS = 4096   # from here on h2d_padded ships the raw rows and pads / centres / casts on the device

    def h2d(self, a, tdtype=None):
        """Host array -> device tensor (optionally cast) THROUGH page-locked staging.  Never `torch.from_numpy(a).to(device)`:
        a copy from a pageable range the runtime has not seen before costs 18 - 28 ms on this stack whatever its size (a
        500 x 3 array: 28 ms; measured with the caller keeping its results, i.e. every array of the next call at a fresh
        address - a second `SparseVFC` call cost 60 ms instead of 26).  Arrays above PINNED_MAX_BYTES keep the pageable path:
        at their size the fixed cost does not matter."""
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a)
        dt = tdtype or t.dtype
        if 0 < t.numel() * t.element_size() <= self.PINNED_MAX_BYTES:
            host = torch.empty(t.shape, dtype=dt, pin_memory=True)
            # (NumPy's single-threaded copy / cast, not torch's: a torch CPU op fans out over every core it sees - 128 threads on
            # the test boxes, whose containers hold a 16-CPU quota - and the spinning pool gets the whole process throttled for
            # the rest of the scheduler period: 50 - 90 ms stalls every few calls, `nr_throttled` in /sys/fs/cgroup/cpu.stat)
            np.copyto(host.numpy(), a, casting="unsafe")
            return host.to(self.device, non_blocking=True)
        if t.numel() == 0:
            return t.to(self.device).to(dt)
        # larger arrays: the same, streamed through two page-locked 32 MB staging buffers (the cast, if any, on the device)
        flat = a.reshape(-1)
        out = torch.empty(flat.shape, dtype=t.dtype, device=self.device)
        per = max(1, (32 << 20) // a.itemsize)
        stage = [torch.empty(per, dtype=t.dtype, pin_memory=True) for _ in range(2)]
        free = [None, None]
        stream = torch.cuda.current_stream(self.device)
        for i, lo in enumerate(range(0, flat.shape[0], per)):
            hi, b = min(lo + per, flat.shape[0]), i & 1
            if free[b] is not None:
                free[b].synchronize()
            np.copyto(stage[b].numpy()[: hi - lo], flat[lo:hi])
            out[lo:hi].copy_(stage[b][: hi - lo], non_blocking=True)
            free[b] = torch.cuda.Event()
            free[b].record(stream)
        out = out.reshape(t.shape)
        return out if dt == t.dtype else out.to(dt)

    def h2d_padded(self, a, width, tdtype, minus=None):
        """Host (n, d <= width) float64 array -> device (n, width) tensor of `tdtype`, zero padded.  minus (1 x d float64, may
        be None): subtracted in float64 on the way - the difference is rounded to `tdtype` as it is written into the staging
        buffer, ONE pass over the data (the evaluator API used to make a centred float64 temporary first)."""
        n, d = a.shape
        nbytes = n * width * (4 if tdtype == torch.float32 else 8)

        def fill(hv):
            if minus is None:
                hv[:, :d] = a
            else:
                np.subtract(a, minus, out=hv[:, :d], casting="same_kind")
            hv[:, d:] = 0

        if n >= self.DEVICE_PAD_MIN_ROWS and a.dtype == np.float64 and 0 < n * d * 8 <= self.PINNED_MAX_BYTES:
            # many rows: the RAW float64 rows travel (one contiguous copy into page-locked staging, one DMA) and the device
            # centres, casts and pads - the same float64 subtraction and the same rounding, i.e. the same bits.  NumPy's strided
            # subtract-and-cast into the padded staging buffer ran at 5 GB/s: 1.2 ms of the 2.5 ms the Jacobian + curl calls on
            # the 64^3 grid cost at the API, 1.1 ms per array of a 250 k-cell fit.
            host = torch.empty((n, d), dtype=torch.float64, pin_memory=True)
            np.copyto(host.numpy(), a)
            xd = host.to(self.device, non_blocking=True)
            if minus is not None:
                xd -= torch.tensor(np.asarray(minus, dtype=np.float64).reshape(-1)[:d].tolist(), dtype=torch.float64,
                                   device=self.device)
            out = torch.zeros((n, width), dtype=tdtype, device=self.device)
            out[:, :d] = xd
            return out
        if 0 < nbytes <= self.PINNED_MAX_BYTES and not (a.dtype == np.float64 and n >= self.DEVICE_PAD_MIN_ROWS):
            host = torch.empty((n, width), dtype=tdtype, pin_memory=True)
            fill(host.numpy())
            return host.to(self.device, non_blocking=True)
        if a.dtype == np.float64 and n >= self.DEVICE_PAD_MIN_ROWS:
            # millions of rows (8 M cells: 192 MB raw): the same device-side centring / cast / padding, the raw rows streamed
            # through two page-locked 32 MB staging buffers (NumPy's strided cast into a pageable (n, 4) buffer + a pageable
            # upload cost 70 ms per array at 8 M rows and left the runtime a fresh pageable range to digest)
            out = torch.zeros((n, width), dtype=tdtype, device=self.device)
            sub = None if minus is None else torch.tensor(np.asarray(minus, dtype=np.float64).reshape(-1)[:d].tolist(),
                                                          dtype=torch.float64, device=self.device)
            rows = max(1, (32 << 20) // (d * 8))
            stage = [torch.empty((rows, d), dtype=torch.float64, pin_memory=True) for _ in range(2)]
            free = [None, None]  # event after which a staging buffer may be refilled
            stream = torch.cuda.current_stream(self.device)
            for i, lo in enumerate(range(0, n, rows)):
                hi, b = min(lo + rows, n), i & 1
                if free[b] is not None:
                    free[b].synchronize()
                np.copyto(stage[b].numpy()[: hi - lo], a[lo:hi])
                xd = stage[b][: hi - lo].to(self.device, non_blocking=True)
                free[b] = torch.cuda.Event()
                free[b].record(stream)
                out[lo:hi, :d] = xd if sub is None else xd - sub
            return out
        buf = np.empty((n, width), dtype=np.float32 if tdtype == torch.float32 else np.float64)
        fill(buf)
        return torch.from_numpy(buf).to(self.device)

    def d2h(self, t):
        """Device tensor -> ordinary (pageable) host NumPy array, THROUGH page-locked staging: the runtime never sees the
        destination.  A `.cpu()` into a pageable range it has not seen before stalls for 50 - 100 ms every few calls on this
        stack (and so does the unmapping of such a range when the caller drops the array): 6 MB of unique rows cost 1.4 ms
        or 90 (tools/kept_results_probe.py)."""
        if not t.is_cuda:
            return t.numpy()
        return self.to_host([t], own_pinned=False)[0]

    @_on_device
    def to_host(self, tensors, own_pinned=True):
        """Device tensors -> host NumPy arrays with ONE stream synchronisation: page-locked destinations while the total
        stays under PINNED_MAX_BYTES (own_pinned: the arrays returned own their pinned block until they are garbage
        collected; else they are pageable copies of it and the block goes back to torch's host cache), otherwise pageable
        arrays filled through two page-locked 32 MB staging buffers."""
        tensors = [t.contiguous() for t in tensors]
        total = sum(t.numel() * t.element_size() for t in tensors)
        stream = torch.cuda.current_stream(self.device)
        if total <= self.PINNED_MAX_BYTES:
            hosts = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in tensors]
            for h, t in zip(hosts, tensors):
                h.copy_(t, non_blocking=True)
            stream.synchronize()
            return [h.numpy() if own_pinned else h.numpy().copy() for h in hosts]
        outs = []
        chunk = 32 << 20
        stage = [torch.empty(chunk, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        events = [torch.cuda.Event(), torch.cuda.Event()]
        for t in tensors:
            out = np.empty(tuple(t.shape), dtype=torch.empty(0, dtype=t.dtype).numpy().dtype)
            flat_d = t.view(-1).view(torch.uint8)
            flat_h = out.reshape(-1).view(np.uint8)
            nb = flat_d.numel()
            pending = []  # (buffer index, lo, hi) in flight
            for i, lo in enumerate(range(0, nb, chunk)):
                b = i & 1
                if len(pending) == 2:
                    pb, plo, phi = pending.pop(0)
                    events[pb].synchronize()
                    flat_h[plo:phi] = stage[pb][: phi - plo].numpy()
                hi = min(lo + chunk, nb)
                stage[b][: hi - lo].copy_(flat_d[lo:hi], non_blocking=True)
                events[b].record(stream)
                pending.append((b, lo, hi))
            for pb, plo, phi in pending:
                events[pb].synchronize()
                flat_h[plo:phi] = stage[pb][: phi - plo].numpy()
            outs.append(out)
        return outs

    def _red(self, n, at_least=0):
        """Scratch of the deterministic reductions: mvf_reduce_scratch_doubles(n) float64, and never fewer than
        `at_least` (mvf_quadform writes one partial per control point: m float64, mvf.h)."""
        need = max(int(self.lib.mvf_reduce_scratch_doubles(int(n))), int(at_least))
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.float64, device=self.device)
        return self._scratch.data_ptr()

    def empty(self, *shape, dtype=None):
        return torch.empty(*shape, dtype=dtype or self.tdtype, device=self.device)

    def zeros(self, *shape, dtype=None):
        return torch.zeros(*shape, dtype=dtype or self.tdtype, device=self.device)

    # ------------------------------------------------------------------ kernels
    @_on_device
    def unique_rows(self, X):
        """np.unique(X, axis=0, return_index=True) for a finite host float64 (n, d) array, on the device:
        returns host (unique rows sorted lexicographically, index of the first occurrence of each)."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        n, d = X.shape
        xd = self.h2d(X)
        uid = torch.empty(n, dtype=torch.int64, device=self.device)
        rows = torch.empty(n, d, dtype=torch.float64, device=self.device)
        cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
        need = int(self.lib.mvf_unique_rows_workspace_bytes(n, d))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.mvf_unique_rows(_ptr(xd), n, d, _ptr(uid), _ptr(rows), _ptr(cnt), _ptr(ws), ws.numel(),
                                            self._stream()), "mvf_unique_rows")
        k = int(cnt.cpu()[0])
        # (page-locked arrays, no second copy: the callers gather from them and drop them - preprocess.unique_rows' result never
        # reaches the user as is)
        S, idx = self.to_host([rows[:k], uid[:k]])
        return S, idx

    @_on_device
    def knn_mean_distance(self, X, k):
        """Mean distance from each point to its k - 1 nearest other points (host float64 (m, d) in, float out): the
        neighbour search of dynamo's bandwidth_selector on the device (m <= 8192, d <= 8)."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        m, d = X.shape
        xd = self.h2d(X)
        rows = torch.empty(m, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.mvf_knn_rowsum(_ptr(xd), m, d, int(k), _ptr(rows), self._stream()), "mvf_knn_rowsum")
        return float(np.sum(self.d2h(rows)) / (m * (k - 1)))

    @_on_device
    def con_k(self, x, y, beta, return_d=False, dtype=None):
        """x: (n, d), y: (m, d) device tensors (cell dtype, or `dtype`) -> K (n, m) [and D (n, d, m)]."""
        tdtype, cdtype = _DT[dtype] if dtype is not None else (self.tdtype, self.cdtype)
        if x.dtype != tdtype or y.dtype != tdtype:
            raise TypeError(f"con_k: expected {tdtype} tensors, got {x.dtype} / {y.dtype}")
        n, d = x.shape
        m = y.shape[0]
        x, y = x.contiguous(), y.contiguous()
        K = self.empty(n, m, dtype=tdtype)
        if return_d:
            D = self.empty(n, d, m, dtype=tdtype)
            for lo in range(0, n, 65535):  # mvf_con_k_d takes at most 65535 rows per call: chunk (rows are contiguous)
                nn = min(65535, n - lo)
                _lib.check(self.lib.mvf_con_k_d(_ptr(x[lo:]), nn, _ptr(y), m, d, float(beta), _ptr(K[lo:]), _ptr(D[lo:]),
                                                cdtype, self._stream()), "mvf_con_k_d")
            return K, D
        _lib.check(self.lib.mvf_con_k(_ptr(x), n, _ptr(y), m, d, float(beta), _ptr(K), cdtype, self._stream()),
                   "mvf_con_k")
        return K

    @_on_device
    def apply(self, x4, ctrl4, beta, C, y4=None, P=None, stats=None):
        """V4 = con_K(x, ctrl) @ C; with y4 also r = ||y - V||^2 and stats[0] += sum P r.  Returns (V4, r)."""
        n, m = x4.shape[0], ctrl4.shape[0]
        V4 = self.empty(n, 4)
        r = self.empty(n) if y4 is not None else None
        _lib.check(self.lib.mvf_apply(_ptr(x4), n, _ptr(ctrl4), m, float(beta), _ptr(C), _ptr(V4), _ptr(y4), _ptr(P),
                                      _ptr(r), _ptr(stats), self._red(n), self.cdtype, self._stream()), "mvf_apply")
        return V4, r

    @_on_device
    def estep_min(self, r, sigma2):
        """Returns a device float64 view (2,): [min non-zero t1, #zeros]."""
        _lib.check(self.lib.mvf_estep_min(_ptr(r), r.shape[0], float(sigma2), _ptr(self._mins), self.cdtype,
                                          self._stream()), "mvf_estep_min")
        return self._mins[:2]

    @_on_device
    def estep_p(self, r, sigma2, gamma, a, dy, minP, theta, zero_fill, P_out, stats):
        """zero_fill: a host float, or a device float64 tensor whose first element is the fill (estep_min's result,
        possibly MIN-all-reduced): then the two E-step phases chain on the stream without a host round trip."""
        fill_dev = zero_fill if torch.is_tensor(zero_fill) else None
        _lib.check(self.lib.mvf_estep_p(_ptr(r), r.shape[0], float(sigma2), float(gamma), float(a), int(dy),
                                        float(minP), float(theta), 0.0 if fill_dev is not None else float(zero_fill),
                                        _ptr(fill_dev), _ptr(P_out), _ptr(stats),
                                        self._red(r.shape[0]), self.cdtype, self._stream()), "mvf_estep_p")

    def read_host(self, t):
        """A contiguous device tensor as a host NumPy array, through ONE blocking copy on the current stream."""
        out = np.empty(t.shape, dtype=_NP[t.dtype])
        _lib.check(self.lib.mvf_read_back(out.ctypes.data, _ptr(t), out.nbytes, self._stream()), "mvf_read_back")
        return out

    @_on_device
    def estep(self, r, sigma2, gamma, a, dy, minP, theta, P_out, stats):
        """Both phases of the E-step in one call (one process: no MIN all-reduce between them); `stats` is overwritten."""
        _lib.check(self.lib.mvf_estep(_ptr(r), r.shape[0], float(sigma2), float(gamma), float(a), int(dy), float(minP),
                                      float(theta), _ptr(self._mins), _ptr(P_out), _ptr(stats), self._red(r.shape[0]),
                                      self.cdtype, self._stream()), "mvf_estep")

    def ublk_bytes(self, n, m):
        return int(self.lib.mvf_ublk_bytes(n, m, self.cdtype))

    @_on_device
    def build_ublk(self, x4, ctrl4, beta):
        """Materialise the float32 kernel values once per fit (U is constant across EM iterations); later `gram`
        calls with the same (x4, ctrl4, beta) stream them instead of regenerating them."""
        n, m = x4.shape[0], ctrl4.shape[0]
        need = self.ublk_bytes(n, m)
        self._ublk = None
        self._ublk = torch.empty(need // self._ublk_itemsize(), dtype=self.tdtype, device=self.device)
        _lib.check(self.lib.mvf_ublk_build(_ptr(x4), n, _ptr(ctrl4), m, float(beta), _ptr(self._ublk), need,
                                           self.cdtype, self._stream()), "mvf_ublk_build")
        self._ublk_key = (x4.data_ptr(), ctrl4.data_ptr(), n, m, float(beta))

    @_on_device
    def build_ublk_d(self, xd, ctrld, beta):
        """build_ublk for 4 <= d <= 8: xd (n, d), ctrld (m, d) from to_xd (mvf_ublk_build_d, same cache layout).  A `gram`
        call with the same (xd, ctrld, beta) then runs its tile and reduce stages on the cache (neither reads the points)."""
        n, m, d = xd.shape[0], ctrld.shape[0], xd.shape[1]
        if ctrld.shape[1] != d:
            raise ValueError(f"cells have {d} columns, control points {ctrld.shape[1]}")
        need = self.ublk_bytes(n, m)
        self._ublk = None
        self._ublk = torch.empty(need // self._ublk_itemsize(), dtype=self.tdtype, device=self.device)
        _lib.check(self.lib.mvf_ublk_build_d(_ptr(xd), n, _ptr(ctrld), m, d, float(beta), _ptr(self._ublk), need,
                                             self.cdtype, self._stream()), "mvf_ublk_build_d")
        self._ublk_key = (xd.data_ptr(), ctrld.data_ptr(), n, m, float(beta))

    def _ublk_itemsize(self):
        return 4 if self.tdtype == torch.float32 else 8

    # ---- wide right-hand sides (Dy > 3): one pass over the cached kernel values for all columns (mvf_wide.hip) ----
    @staticmethod
    def wide_pads(n, m):
        """(cells, control points, columns -> padded extents) of the buffers mvf_rhs_cached / mvf_apply_cached read."""
        return -(-int(n) // 256) * 256, -(-int(m) // 128) * 128

    def _wide_ws(self, n, m):
        need = int(self.lib.mvf_wide_workspace_bytes(int(n), int(m)))
        if getattr(self, "_wide_buf", None) is None or self._wide_buf.numel() < need:
            self._wide_buf = None
            self._wide_buf = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        return self._wide_buf

    @_on_device
    def rhs_wide(self, P, Yd, dy, m, R):
        """R (m x dy float64) = U^T diag(P) Yd[:, :dy] from the cache of build_ublk (Yd: padded rows x padded columns)."""
        if self._ublk is None:
            raise RuntimeError("rhs_wide needs the kernel-value cache (build_ublk)")
        n = P.shape[0]
        ws = self._wide_ws(n, m)
        _lib.check(self.lib.mvf_rhs_cached(_ptr(self._ublk), _ptr(P), _ptr(Yd), n, int(m), int(dy), Yd.shape[1], _ptr(R),
                                           R.shape[1], _ptr(ws), ws.numel(), self.cdtype, self._stream()), "mvf_rhs_cached")

    @_on_device
    def apply_wide(self, Cd, dy, m, Yd, P, Vd, r, stats):
        """Vd[:, :dy] = U Cd[:, :dy]; r = sum_d (Yd - Vd)^2; stats[0] += sum P r (Cd: padded rows x padded columns, float64)."""
        if self._ublk is None:
            raise RuntimeError("apply_wide needs the kernel-value cache (build_ublk)")
        n = Vd.shape[0]
        ws = self._wide_ws(n, m)
        _lib.check(self.lib.mvf_apply_cached(_ptr(self._ublk), n, int(m), _ptr(Cd), Cd.shape[1], int(dy), _ptr(Yd), Yd.shape[1],
                                             _ptr(P), _ptr(Vd), _ptr(r), _ptr(stats), _ptr(ws), ws.numel(), self.cdtype,
                                             self._stream()), "mvf_apply_cached")

    def drop_ublk(self):
        self._ublk = None
        self._cache_bufs = None
        self._ublk_key = None

    @_on_device
    def gram(self, x4, P, y4, ctrl4, beta, G, R, rhs_only=False, tiles_only=False, cache_only=False):
        """G = U^T P U (m x m), R = U^T P Y (m x 3).  rhs_only: only R for this y4 (G unchanged) - for Y wider than 3,
        and the second half of a multi-rank step; tiles_only: only G (tile stage + its reduction) - the first half of a
        multi-rank step, whose all-reduce of G then overlaps the rhs kernels.  cache_only: raise unless the cache of
        build_ublk / build_ublk_d for these (x4, ctrl4, beta) is there (4 <= D <= 8: x4 then holds plain (n, D) rows, which
        the regenerating kernels would misread as x4 vectors)."""
        n, m = x4.shape[0], ctrl4.shape[0]
        key = (n, m, _lib.OPTION_EPOCH[0])
        need = self._gram_need.get(key)
        if need is None:  # (the call runs the launch plan's search: once per shape, not once per EM iteration)
            need = self._gram_need[key] = self.lib.mvf_gram_workspace_bytes(n, m, self.cdtype)
        if self._gram_ws is None or self._gram_ws.numel() < need:
            self._gram_ws = None
            self._gram_ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        args = (_ptr(x4), _ptr(P), _ptr(y4), n, _ptr(ctrl4), m, float(beta), _ptr(G), _ptr(R), _ptr(self._gram_ws),
                self._gram_ws.numel())
        cached = self._ublk is not None and self._ublk_key == (x4.data_ptr(), ctrl4.data_ptr(), n, m, float(beta))
        if cache_only and not cached:
            raise _lib.MVFError("gram: the kernel-value cache of these points is not built (no regenerating Gram kernel "
                                "reads plain (n, D) rows)")
        if cached:
            def run(stages):
                _lib.check(self.lib.mvf_gram_cached(stages, _ptr(self._ublk), *args, self.cdtype, self._stream()),
                           "mvf_gram_cached")
        else:
            def run(stages):
                _lib.check(self.lib.mvf_gram_stages(stages, *args, self.cdtype, self._stream()), "mvf_gram_stages")
        if rhs_only:
            run(_lib.GRAM_RHS | _lib.GRAM_REDUCE_RHS)
            return
        rest = _lib.GRAM_REDUCE if tiles_only else _lib.GRAM_RHS | _lib.GRAM_REDUCE | _lib.GRAM_REDUCE_RHS
        if self.gram_events is None:
            run(_lib.GRAM_TILES | rest)
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(_lib.GRAM_TILES)
        e1.record()
        self.gram_events.append((e0, e1))
        run(rest)

    @_on_device
    def solve(self, G, K, lambda_sigma2, jitter, R, C_out, info, pivots=None):
        """Cholesky solve of (G + ls2 K + jitter mean(diag) I) C = R.  info[0] != 0: non-positive pivot.
        pivots (float64[2], optional): [min L_jj^2, max L_jj^2] - the host's numerical-rank certificate."""
        m, nrhs = R.shape
        need = self.lib.mvf_solve_workspace_bytes(m, nrhs)
        if self._solve_ws is None or self._solve_ws.numel() < need:
            self._solve_ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.mvf_solve(_ptr(G), _ptr(K), float(lambda_sigma2), float(jitter), _ptr(R), m, nrhs,
                                      _ptr(C_out), _ptr(info), _ptr(pivots), _ptr(self._solve_ws),
                                      self._solve_ws.numel(), self._stream()), "mvf_solve")

    @_on_device
    def solve_minnorm(self, G, K, lambda_sigma2, shift, R, C_out, info, einfo, rcond=None, reuse=False, max_sweeps=60,
                      basis=None, warm=False):
        """Minimum-norm solve with the gelsd cut-off (eigenvalues below rcond * max|lambda| dropped; rcond = float64
        eps = scipy.linalg.lstsq's default).  reuse=True applies the decomposition left in the workspace by the
        previous call (same matrix) to another right-hand side.  ``basis`` (float64 tensor from ``minnorm_basis``)
        receives the eigenvectors; ``warm=True`` starts from the ones it holds (the previous EM iteration's).
        Synchronises the stream (once per Jacobi sweep)."""
        m, nrhs = R.shape
        need = self.lib.mvf_solve_minnorm_workspace_bytes(m, nrhs)
        if self._mn_ws is None or self._mn_ws.numel() < need:
            if reuse:
                raise RuntimeError("solve_minnorm(reuse=True) without a previous decomposition")
            self._mn_ws = None
            self._mn_ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        rc = float(np.finfo(np.float64).eps) if rcond is None else float(rcond)
        _lib.check(self.lib.mvf_solve_minnorm(_ptr(G), _ptr(K), float(lambda_sigma2), float(shift), rc, _ptr(R), m,
                                              nrhs, _ptr(C_out), _ptr(info), _ptr(einfo), int(max_sweeps),
                                              1 if reuse else 0, _ptr(basis), 1 if warm else 0, _ptr(self._mn_ws),
                                              self._mn_ws.numel(), self._stream()), "mvf_solve_minnorm")

    @_on_device
    def pinv_diag(self, x4, ctrl4, beta, rcond=None, lowrank=False):
        """diag(U pinv(A) U^T) (float64, n) from the decomposition the last solve_minnorm_lr (lowrank=True) / solve_minnorm
        call of this object left in its workspace; U = con_K(x, ctrl, beta) is regenerated, never materialised."""
        ws = self._lr_ws if lowrank else self._mn_ws
        if ws is None:
            raise RuntimeError("pinv_diag without a previous decomposition")
        n, m = x4.shape[0], ctrl4.shape[0]
        out = torch.empty(n, dtype=torch.float64, device=self.device)
        rc = float(np.finfo(np.float64).eps) if rcond is None else float(rcond)
        _lib.check(self.lib.mvf_pinv_diag(_ptr(x4), n, _ptr(ctrl4), m, float(beta), rc, 1 if lowrank else 0, _ptr(out),
                                          _ptr(ws), ws.numel(), self.cdtype, self._stream()), "mvf_pinv_diag")
        return out

    @_on_device
    def solve_minnorm_lr(self, G, K, lambda_sigma2, R, C_out, info, einfo, rcond=None, reuse=False, max_sweeps=60,
                         rank_hint=0, tolf=0.25, deflate=False):
        """The same truncated minimum-norm solve through the rank-revealing factor (pivoted Cholesky stopped at
        tolf * eps * lambda_max, Jacobi on the r kept columns only).  einfo[_lib.EINFO_FACTOR_RANK] = r; pass it back as
        ``rank_hint`` for the next, nearby matrix.  deflate=True (mvf_solve_minnorm_lrd): only the invariant subspace below the cut-off
        is computed and projected out - same truncation, no full eigendecomposition (no pinv_diag afterwards).
        Synchronises the stream."""
        m, nrhs = R.shape
        fn = self.lib.mvf_solve_minnorm_lrd if deflate else self.lib.mvf_solve_minnorm_lr
        need = (self.lib.mvf_solve_minnorm_lrd_workspace_bytes if deflate else self.lib.mvf_solve_minnorm_lr_workspace_bytes)(m, nrhs)
        if self._lr_ws is None or self._lr_ws.numel() < need:
            if reuse:
                raise RuntimeError("solve_minnorm_lr(reuse=True) without a previous decomposition")
            self._lr_ws = None
            # (zeroed: the 64-byte state record in it must not be read as a finished factorisation - ADVICE r5; once per allocation)
            self._lr_ws = torch.zeros(max(need, 1), dtype=torch.uint8, device=self.device)
        rc = float(np.finfo(np.float64).eps) if rcond is None else float(rcond)
        _lib.check(fn(_ptr(G), _ptr(K), float(lambda_sigma2), float(tolf), rc, _ptr(R), m, nrhs, _ptr(C_out), _ptr(info),
                      _ptr(einfo), int(max_sweeps), 1 if reuse else 0, int(rank_hint), _ptr(self._lr_ws),
                      self._lr_ws.numel(), self._stream()), "mvf_solve_minnorm_lrd" if deflate else "mvf_solve_minnorm_lr")

    @_on_device
    def solve_minnorm_lrd_async(self, G, K, lambda_sigma2, R, C_out, info, einfo, form_hint, rcond=None, tolf=0.25):
        """The direct form of the deflated solve without any host synchronisation (mvf_solve_minnorm_lrd_async): form_hint =
        the previous call's einfo[_lib.EINFO_FORM] on this workspace (LRD_FORM_FACTOR / LRD_FORM_DIRECT, with EINFO_FACTOR_RANK
        == m; + LRD_HINT_MOVED: the matrix moved).  einfo[_lib.EINFO_REJECTED] == 1 afterwards means NOT accepted: repeat through
        solve_minnorm_lr(deflate=True).  Needs the workspace of a previous call."""
        m, nrhs = R.shape
        if self._lr_ws is None or self._lr_ws.numel() < self.lib.mvf_solve_minnorm_lrd_workspace_bytes(m, nrhs):
            raise RuntimeError("solve_minnorm_lrd_async without the workspace of a previous deflated solve")
        rc = float(np.finfo(np.float64).eps) if rcond is None else float(rcond)
        _lib.check(self.lib.mvf_solve_minnorm_lrd_async(_ptr(G), _ptr(K), float(lambda_sigma2), float(tolf), rc, _ptr(R), m, nrhs,
                                                        _ptr(C_out), _ptr(info), _ptr(einfo), int(form_hint), _ptr(self._lr_ws),
                                                        self._lr_ws.numel(), self._stream()), "mvf_solve_minnorm_lrd_async")

    @_on_device
    def lr_pivot_order(self, m, with_values=False):
        """Host int array: the pivots (control-point indices, in the order taken) of the last solve_minnorm_lr call; with
        with_values also (the diagonal value of each pivot when it was taken, the stopping tolerance)."""
        import ctypes

        if self._lr_ws is None:
            raise RuntimeError("lr_pivot_order without a previous solve_minnorm_lr")
        order = (ctypes.c_int * int(m))()
        vals = (ctypes.c_double * int(m))()
        tol = ctypes.c_double(0.0)
        r = ctypes.c_int64(0)
        _lib.check(self.lib.mvf_lr_pivot_order(_ptr(self._lr_ws), self._lr_ws.numel(), int(m), order, vals, ctypes.byref(tol),
                                               ctypes.byref(r), self._stream()), "mvf_lr_pivot_order")
        idx = np.frombuffer(order, dtype=np.int32, count=int(r.value)).astype(np.int64)
        if with_values:
            return idx, np.frombuffer(vals, dtype=np.float64, count=int(r.value)).copy(), float(tol.value)
        return idx

    @_on_device
    def minnorm_basis(self, m):
        """Uninitialised eigenvector-basis buffer for solve_minnorm's warm start (m x m padded to multiples of 64)."""
        return torch.empty(int(self.lib.mvf_solve_minnorm_basis_bytes(m)) // 8, dtype=torch.float64, device=self.device)

    @_on_device
    def lincomb3(self, out, a, A, b=0.0, B=None, c=0.0, C=None):
        """out = a A + b B + c C (float64 device tensors of one shape; B, C optional; out may alias an input)."""
        _lib.check(self.lib.mvf_lincomb3(_ptr(out), float(a), _ptr(A), float(b), _ptr(B), float(c), _ptr(C),
                                         out.numel(), self._stream()), "mvf_lincomb3")
        return out

    @_on_device
    def hull_mask(self, points, equations, tol):
        """Host (n, 3) points and SciPy ConvexHull.equations (nf, 4) -> host bool (n,): inside the hull."""
        P = self.h2d(np.ascontiguousarray(points, dtype=np.float64))
        E = self.h2d(np.ascontiguousarray(equations, dtype=np.float64))
        out = torch.empty(P.shape[0], dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.mvf_hull_mask(_ptr(P), P.shape[0], _ptr(E), E.shape[0], float(tol), _ptr(out),
                                          self._stream()), "mvf_hull_mask")
        return self.d2h(out).astype(bool)

    @_on_device
    def quadform(self, K, C, out):
        _lib.check(self.lib.mvf_quadform(_ptr(K), _ptr(C), K.shape[0], C.shape[1], _ptr(out),
                                         self._red(K.shape[0], at_least=K.shape[0]), self._stream()), "mvf_quadform")

    @_on_device
    def sym_pack(self, G, tri):
        """Packed upper triangle of the symmetric G (what the multi-GPU host all-reduces)."""
        _lib.check(self.lib.mvf_sym_pack(_ptr(G), G.shape[0], _ptr(tri), self._stream()), "mvf_sym_pack")

    @_on_device
    def sym_unpack(self, tri, G):
        _lib.check(self.lib.mvf_sym_unpack(_ptr(tri), G.shape[0], _ptr(G), self._stream()), "mvf_sym_unpack")

    @_on_device
    def assign_prepare(self, layer, metric, side):
        """One side (0 = A cells, 1 = B cells) of one layer of the assignment step: host (n, g) float64 -> device
        (X' or Y' (n, ld) in the cell dtype, a or b (n,) float64, ld)  (mvf_assign_prepare).  A scipy.sparse layer goes up
        as its CSR arrays and is expanded row by row on the device (mvf_assign_prepare_csr): the same bits, and no (n, g)
        float64 array on either side of the link."""
        if is_sparse(layer):
            return self._assign_prepare_csr(layer, metric, side)
        L = np.ascontiguousarray(layer, dtype=np.float64)
        n, g = L.shape
        ld = int(self.lib.mvf_assign_padded_features(g, int(metric)))
        Lp = self.empty(n, ld)
        ab = self.empty(n, dtype=torch.float64)
        _lib.check(self.lib.mvf_assign_prepare(_ptr(self.h2d(L)), n, g, int(metric), int(side), _ptr(Lp), ld, _ptr(ab),
                                               self.cdtype, self._stream()), "mvf_assign_prepare")
        return Lp, ab, ld

    def _assign_prepare_csr(self, layer, metric, side):
        indptr, indices, data, n, g = csr_arrays(layer)
        ld = int(self.lib.mvf_assign_padded_features(g, int(metric)))
        Lp = self.empty(n, ld)
        ab = self.empty(n, dtype=torch.float64)
        if n == 0:
            return Lp, ab, ld
        if len(data) == 0:  # an all-zero layer: the arrays still need an address
            indices, data = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=data.dtype)
        need = int(self.lib.mvf_assign_prepare_csr_min_workspace_bytes(g))
        rows = min(-(-n // 4) * 4, CSR_STAGING_MAX_ROWS, max(4, CSR_STAGING_MAX_BYTES // (8 * g) // 4 * 4))
        ws = self.empty(max(need, rows * g * 8) // 8, dtype=torch.float64)
        # (the three uploads stay referenced until the launch is queued: a tensor dropped right after its address is taken
        # hands its block back to the allocator, and the next upload may be given the same address)
        d_indptr, d_indices, d_data = self.h2d(indptr), self.h2d(indices), self.h2d(data)
        _lib.check(self.lib.mvf_assign_prepare_csr(_ptr(d_indptr), _ptr(d_indices), _ptr(d_data),
                                                   int(data.dtype == np.float32), n, g, int(metric), int(side), _ptr(Lp), ld,
                                                   _ptr(ab), _ptr(ws), ws.numel() * 8, self.cdtype, self._stream()),
                   "mvf_assign_prepare_csr")
        return Lp, ab, ld

    @_on_device
    def assign_label_prepare(self, labels, classes):
        """One side of a label layer: host integer labels (n,), validated by the caller to lie in 0 .. classes - 1 -> device
        float64 (n,), the labels as mvf_assign_layer's a / b hold them  (mvf_assign_label_prepare)."""
        lab = self.h2d(np.ascontiguousarray(labels, dtype=np.int32))
        ab = self.empty(lab.shape[0], dtype=torch.float64)
        _lib.check(self.lib.mvf_assign_label_prepare(_ptr(lab), lab.shape[0], int(classes), _ptr(ab), self._stream()),
                   "mvf_assign_label_prepare")
        return ab

    def _assign_call(self, name, workspace_bytes, size_args, common, middle):
        """One call of an assignment entry point: the head its kind shares, built from `common` = (xa4, xb4, layers,
        model_mul, sigma2, sigma2_variance, spatial_outlier) (None: mvf_assign_layer_stats, which has none), the entry
        point's own `middle` arguments, and the tail: a fresh workspace of `workspace_bytes(*size_args)`, dtype, stream."""
        head = ()
        if common is not None:
            xa4, xb4, layers, model_mul, sigma2, sigma2_variance, spatial_outlier = common
            head = (_ptr(xa4), xa4.shape[0], _ptr(xb4), xb4.shape[0], layer_array(layers), len(layers), _ptr(model_mul),
                    float(sigma2), float(sigma2_variance), float(spatial_outlier))
        need = int(workspace_bytes(*size_args))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        _lib.check(getattr(self.lib, name)(*head, *middle, _ptr(ws), need, self.cdtype, self._stream()), name)

    def _assign_outputs(self, na, nb):
        """The outputs mvf_assign, _dense and _topk share, in the order the C ABI takes them."""
        shapes = {"K_NA": (na,), "K_NB": (nb,), "K_NA_spatial": (na,), "K_NA_sigma2": (na,), "PXB": (na, 3), "scalars": (1,)}
        return {q: self.empty(*s, dtype=torch.float64) for q, s in shapes.items()}

    @_on_device
    def assign(self, xa4, xb4, layers, model_mul, sigma2, sigma2_variance, spatial_outlier, dense=False):
        """The fused assignment step (mvf_assign / mvf_assign_dense).  layers: a list of `Layer` records (or plain
        8-sequences in their order) of device tensors from assign_prepare / assign_label_prepare.  Returns device float64
        tensors {K_NA, K_NB, K_NA_spatial, K_NA_sigma2, PXB (na, 3), scalars (1,) = sum P_sigma2 d [, P (na, nb)]}."""
        na, nb = xa4.shape[0], xb4.shape[0]
        out = self._assign_outputs(na, nb)
        if dense:
            out["P"] = self.empty(na, nb, dtype=torch.float64)
        self._assign_call("mvf_assign_dense" if dense else "mvf_assign", self.lib.mvf_assign_workspace_bytes, (na, nb),
                          (xa4, xb4, layers, model_mul, sigma2, sigma2_variance, spatial_outlier),
                          [_ptr(t) for t in out.values()])   # (P comes last in the ABI too)
        return out

    @_on_device
    def assign_topk(self, xa4, xb4, layers, model_mul, sigma2, sigma2_variance, spatial_outlier, k):
        """The assignment step of the reference's sparse_calculation_mode (mvf_assign_topk): the k_eff = min(k, na) largest
        entries of every column of P are kept.  Returns assign's dict - K_NA, K_NB, PXB of the kept entries, K_NA_spatial,
        K_NA_sigma2, scalars the dense ones - plus rows (nb, k_eff) int32 and vals (nb, k_eff) float64: column j's entries,
        value descending, row ascending."""
        na, nb = xa4.shape[0], xb4.shape[0]
        k = int(k)
        ke = min(k, na)
        out = self._assign_outputs(na, nb)
        out["rows"], out["vals"] = self.empty(nb, ke, dtype=torch.int32), self.empty(nb, ke, dtype=torch.float64)
        self._assign_call("mvf_assign_topk", self.lib.mvf_assign_topk_workspace_bytes, (na, nb, k),
                          (xa4, xb4, layers, model_mul, sigma2, sigma2_variance, spatial_outlier),
                          [k] + [_ptr(t) for t in out.values()])
        return out

    @_on_device
    def assign_best(self, xa4, xb4, layers, model_mul, sigma2, sigma2_variance, spatial_outlier, rows=True, cols=True):
        """The best partner per cell from the fused assignment (mvf_assign_best): arguments as assign takes them.  Returns
        device tensors {rows (na, 2) int32 = per A cell the B index under the "nearest" rule (value descending, distance
        ascending, index ascending) and under the "first" rule (value descending, index ascending), row_values (na,) float64
        = max_j P_ij, cols (nb, 2) int32 / col_values (nb,) float64: the same per B cell over the A cells}.  ``rows=False``
        / ``cols=False`` skips that direction (its two entries are absent); one of them must stay."""
        na, nb = xa4.shape[0], xb4.shape[0]
        f64 = torch.float64
        out = {}
        if rows:
            out["rows"], out["row_values"] = self.empty(na, 2, dtype=torch.int32), self.empty(na, dtype=f64)
        if cols:
            out["cols"], out["col_values"] = self.empty(nb, 2, dtype=torch.int32), self.empty(nb, dtype=f64)
        self._assign_call("mvf_assign_best", self.lib.mvf_assign_best_workspace_bytes, (na, nb),
                          (xa4, xb4, layers, model_mul, sigma2, sigma2_variance, spatial_outlier),
                          [_ptr(out.get(q)) for q in ("rows", "row_values", "cols", "col_values")])
        return out

    @_on_device
    def assign_apply(self, xa4, xb4, layers, model_mul, sigma2, sigma2_variance, spatial_outlier, features_B=None,
                     features_A=None, sums=True):
        """The assignment applied to cell features without P (mvf_assign_apply): arguments as assign takes them, plus
        features_B (nb, cb) and / or features_A (na, ca), device float64 (rows may be strided: a column slice of a wider
        row-major tensor).  Returns device float64 tensors {to_A (na, cb) = P @ features_B, to_B (nb, ca) = P^T @ features_A,
        K_NB (nb,) and - with features_B, which its sweep carries - K_NA (na,)}; a direction without features is absent, one
        must be given.  ``sums=False`` leaves K_NA / K_NB out."""
        na, nb = xa4.shape[0], xb4.shape[0]
        f64 = torch.float64
        if features_A is None and features_B is None:
            raise ValueError("assign_apply: features_A or features_B must be given")
        for F, n, name in ((features_B, nb, "features_B"), (features_A, na, "features_A")):
            if F is None:
                continue
            if F.dtype != f64 or F.dim() != 2 or F.shape[0] != n or F.shape[1] < 1 or (n > 0 and F.stride(1) != 1) \
                    or (n > 1 and F.stride(0) < F.shape[1]):
                raise ValueError(f"assign_apply: {name} must be a float64 ({n}, c >= 1) tensor with contiguous rows")
        out = {}
        cb = ca = ldb = lda = 0
        if features_B is not None:
            cb = int(features_B.shape[1])
            ldb = int(features_B.stride(0)) if nb > 1 else cb
            out["to_A"] = self.empty(na, cb, dtype=f64)
            if sums:
                out["K_NA"] = self.empty(na, dtype=f64)
        if features_A is not None:
            ca = int(features_A.shape[1])
            lda = int(features_A.stride(0)) if na > 1 else ca
            out["to_B"] = self.empty(nb, ca, dtype=f64)
        if sums:
            out["K_NB"] = self.empty(nb, dtype=f64)
        self._assign_call("mvf_assign_apply", self.lib.mvf_assign_apply_workspace_bytes, (na, nb, cb, ca),
                          (xa4, xb4, layers, model_mul, sigma2, sigma2_variance, spatial_outlier),
                          (_ptr(features_B), cb, ldb, _ptr(out.get("to_A")), _ptr(features_A), ca, lda, _ptr(out.get("to_B")),
                           _ptr(out.get("K_NA")), _ptr(out.get("K_NB"))))
        return out

    @_on_device
    def assign_layer_stats(self, layer, na, nb, k=0):
        """Column statistics of one layer's (na, nb) distance matrix (mvf_assign_layer_stats).  layer: one `Layer` as assign
        takes them (prob and param are not read).  Returns device tensors {cmin (nb,) float64, sums (2,) float64 = sum d,
        sum d^2} and, for k > 0, rows (nb, k_eff) int32 / vals (nb, k_eff) float64, k_eff = min(k, na): column j's smallest
        entries, value ascending, row ascending.  The statistics of the rows: the same call on `layer.exchanged()` with na
        and nb exchanged."""
        na, nb, k = int(na), int(nb), int(k)
        ke = min(k, na)
        f64 = torch.float64
        out = {"cmin": self.empty(nb, dtype=f64), "sums": self.empty(2, dtype=f64)}
        if k > 0:
            out["rows"], out["vals"] = self.empty(nb, ke, dtype=torch.int32), self.empty(nb, ke, dtype=f64)
        self._assign_call("mvf_assign_layer_stats", self.lib.mvf_assign_layer_stats_workspace_bytes, (na, nb, k), None,
                          (layer_array([layer]), na, nb, k, _ptr(out["cmin"]), _ptr(out.get("rows")), _ptr(out.get("vals")),
                           _ptr(out["sums"])))
        return out

    # ---- the O(N) glue of the alignment loop (mvf_align.hip): device tensors in, device tensors out ----
    @_on_device
    def align_alpha(self, kappa, K_NA_spatial, SigmaDiag, Sp_spatial, sigma2, alpha, model_mul):
        """alpha and the next assignment's model_mul (float64 (na,) device tensors, overwritten) - mvf_align_alpha."""
        _lib.check(self.lib.mvf_align_alpha(_ptr(kappa), _ptr(K_NA_spatial), _ptr(SigmaDiag), kappa.shape[0], float(Sp_spatial),
                                            float(sigma2), _ptr(alpha), _ptr(model_mul), self._stream()), "mvf_align_alpha")

    @staticmethod
    def _host3(v, n):
        import ctypes

        return None if v is None else (ctypes.c_double * n)(*[float(x) for x in np.asarray(v, dtype=np.float64).reshape(n)])

    @_on_device
    def align_moments(self, A, V4, K_NA, K_NA_spatial, K_NA_sigma2, SigmaDiag, PXB, B, K_NB, out, origin=None, extra=None):
        """The iteration's one block of reductions (mvf_align_moments) into `out` (float64, ALIGN_MOMENT_DOUBLES)."""
        na, nb = A.shape[0], B.shape[0]
        need = int(self.lib.mvf_align_workspace_bytes(na, nb))
        if getattr(self, "_align_ws", None) is None or self._align_ws.numel() < need:
            self._align_ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.mvf_align_moments(_ptr(A), _ptr(V4), _ptr(K_NA), _ptr(K_NA_spatial), _ptr(K_NA_sigma2), _ptr(SigmaDiag),
                                              _ptr(PXB), na, _ptr(B), _ptr(K_NB), nb, self._host3(origin, 3), _ptr(extra), _ptr(out),
                                              _ptr(self._align_ws), self._align_ws.numel(), self.cdtype, self._stream()),
                   "mvf_align_moments")

    @_on_device
    def align_transform(self, A, V4, PXB, K_NA, R, t, origin=None, RnA=None, XAHat=None, xa4=None, PXB_term=None, Y4=None,
                        Pw=None):
        """mvf_align_transform: R (3 x 3), t (3) host; every output is an optional preallocated device tensor."""
        Rt = self._host3(np.concatenate([np.asarray(R, dtype=np.float64).reshape(9), np.asarray(t, dtype=np.float64).reshape(3)]), 12)
        _lib.check(self.lib.mvf_align_transform(_ptr(A), _ptr(V4), _ptr(PXB), _ptr(K_NA), A.shape[0], Rt, self._host3(origin, 3),
                                                _ptr(RnA), _ptr(XAHat), _ptr(xa4), _ptr(PXB_term), _ptr(Y4), _ptr(Pw), self.cdtype,
                                                self._stream()), "mvf_align_transform")

    # ---- the SVI mode of the loop ----
    @_on_device
    def align_gather(self, perm, start, bs, xb4, B, layers, xb4_out, B_out, Yp_out, b_out):
        """mvf_align_gather: the rows perm[(start + j) mod nb], j < bs, of xb4, B (nb x 3 float64) and every layer's Yp / b
        into the preallocated batch buffers.  perm: device int32, a permutation of range(nb) (the caller's guarantee)."""
        nb = xb4.shape[0]
        if perm.dtype != torch.int32 or perm.shape != (nb,) or B.shape != (nb, 3):
            raise ValueError("align_gather: perm must be int32 (nb,) and B (nb, 3)")
        if xb4_out.shape[0] < bs or B_out.shape[0] < bs or len(Yp_out) != len(layers) or len(b_out) != len(layers):
            raise ValueError("align_gather: the batch buffers do not fit the batch")
        for (_, Yp, _, b, ld, metric, *_), Yo, bo in zip(layers, Yp_out, b_out):
            if metric == _lib.ASSIGN_LABEL:     # only the B labels (b) are gathered: the table has no rows per cell
                if b.shape != (nb,) or bo.shape[0] < bs:
                    raise ValueError("align_gather: a layer's buffers do not fit")
            elif Yp.shape != (nb, ld) or b.shape != (nb,) or Yo.shape[0] < bs or Yo.shape[1] != ld or bo.shape[0] < bs:
                raise ValueError("align_gather: a layer's buffers do not fit")
        import ctypes

        vp = ctypes.c_void_p * max(len(layers), 1)
        _lib.check(self.lib.mvf_align_gather(_ptr(perm), nb, int(start), int(bs), _ptr(xb4), _ptr(xb4_out), _ptr(B), _ptr(B_out),
                                             layer_array(layers), len(layers), vp(*[_ptr(t) for t in Yp_out]),
                                             vp(*[_ptr(t) for t in b_out]), self.cdtype, self._stream()), "mvf_align_gather")

    @_on_device
    def align_alpha_svi(self, kappa, K_NA_spatial, SigmaDiag, Sp_spatial, sigma2, step, alpha, model_mul):
        """mvf_align_alpha_svi: alpha <- step exp(...) + (1 - step) alpha (in place) and the next model_mul."""
        _lib.check(self.lib.mvf_align_alpha_svi(_ptr(kappa), _ptr(K_NA_spatial), _ptr(SigmaDiag), kappa.shape[0], float(Sp_spatial),
                                                float(sigma2), float(step), _ptr(alpha), _ptr(model_mul), self._stream()),
                   "mvf_align_alpha_svi")

    @_on_device
    def align_transform_svi(self, RnA, PXB, K_NA, step, PXB_term, Y4, Pw, origin=None):
        """mvf_align_transform_svi: PXB_term <- step (PXB - (RnA - origin) K_NA) + (1 - step) PXB_term in place, Y4 / Pw."""
        _lib.check(self.lib.mvf_align_transform_svi(_ptr(RnA), _ptr(PXB), _ptr(K_NA), RnA.shape[0], self._host3(origin, 3),
                                                    float(step), _ptr(PXB_term), _ptr(Y4), _ptr(Pw), self.cdtype, self._stream()),
                   "mvf_align_transform_svi")

    # ---- down-sampling (mvf_sample.hip): float64 whatever the cell dtype, host arrays in, host arrays out ----
    def _f64_rows(self, X):
        return self.h2d(np.ascontiguousarray(X, dtype=np.float64))

    @_on_device
    def trn(self, problems):
        """mvf_trn for a list of problems in one call: each a dict with X (N, d), w_idx (n,), p_idx (T,) int64 and the
        schedules l, ep (T,), kc (T,) or None.  Returns the list of node matrices W (n, d), host float64."""
        recs = (_lib.TrnProblem * max(len(problems), 1))()
        keep, outs = [], []
        for rec, pr in zip(recs, problems):
            X = self._f64_rows(pr["X"])
            n, T = len(pr["w_idx"]), len(pr["p_idx"])
            dev = [self.h2d(np.ascontiguousarray(pr[k], dtype=np.int64)) for k in ("w_idx", "p_idx")]
            dev += [self.h2d(np.ascontiguousarray(pr[k], dtype=np.float64)) for k in ("l", "ep")]
            kc = None if pr.get("kc") is None else self.h2d(np.ascontiguousarray(pr["kc"], dtype=np.float64))
            W = self.empty(n, X.shape[1], dtype=torch.float64)
            rec.X, rec.N, rec.d, rec.n, rec.T = _ptr(X), X.shape[0], X.shape[1], n, T
            rec.w_idx, rec.p_idx, rec.l, rec.ep, rec.kc, rec.W = _ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), _ptr(dev[3]), _ptr(kc), _ptr(W)
            keep.append((X, dev, kc))
            outs.append(W)
        _lib.check(self.lib.mvf_trn(recs, len(problems), self._stream()), "mvf_trn")
        return [np.array(w) for w in self.to_host(outs, own_pinned=False)] if outs else []

    @_on_device
    def nearest_rows(self, X, Q):
        """mvf_nearest_rows: for every row of Q (n, d) the index of the nearest row of X (N, d), the smallest among equal
        distances; host int64 (n,)."""
        Xd, Qd = self._f64_rows(X), self._f64_rows(Q)
        N, n = Xd.shape[0], Qd.shape[0]
        need = int(self.lib.mvf_nearest_rows_workspace_bytes(N, n))
        ws = self.empty(max(need // 8, 1), dtype=torch.float64)
        idx = self.empty(n, dtype=torch.int64)
        _lib.check(self.lib.mvf_nearest_rows(_ptr(Xd), N, Xd.shape[1], _ptr(Qd), n, _ptr(idx), _ptr(ws), ws.numel() * 8,
                                             self._stream()), "mvf_nearest_rows")
        return np.array(self.d2h(idx))

    @_on_device
    def kmeans(self, X, C0, iters):
        """mvf_kmeans: `iters` Lloyd steps from the start matrix C0 (n, d) on X (N, d), all queued at once.  Returns host
        (centroids (n, d) float64, labels (N,) int32, counts (n,) int64)."""
        Xd, Cd = self._f64_rows(X), self._f64_rows(np.array(C0, dtype=np.float64))
        N, n = Xd.shape[0], Cd.shape[0]
        need = int(self.lib.mvf_kmeans_workspace_bytes(N, n))
        ws = self.empty(max(need // 8, 1), dtype=torch.float64)
        labels, counts = self.empty(N, dtype=torch.int32), self.empty(n, dtype=torch.int64)
        _lib.check(self.lib.mvf_kmeans(_ptr(Xd), N, Xd.shape[1], _ptr(Cd), n, int(iters), _ptr(labels), _ptr(counts), _ptr(ws),
                                       ws.numel() * 8, self._stream()), "mvf_kmeans")
        C, lab, cnt = self.to_host([Cd, labels, counts], own_pinned=False)
        return np.array(C), np.array(lab), np.array(cnt)

    # ---- mesh correction (mvf_icp.hip): float64 whatever the cell dtype, host arrays in, host arrays out ----
    @staticmethod
    def _pack_rows(arrays, width):
        """(the arrays stacked into one (total, width) float64 matrix, offsets (len + 1,) int64 of their first rows)."""
        offsets = np.zeros(len(arrays) + 1, dtype=np.int64)
        np.cumsum([len(a) for a in arrays], out=offsets[1:])
        flat = np.concatenate(arrays, axis=0) if arrays else np.zeros((0, width))
        return np.ascontiguousarray(flat, dtype=np.float64).reshape(-1, width), offsets

    @_on_device
    def icp_batch(self, contours_1, contours_2, max_iter, error_threshold, inlier_threshold, gamma_threshold, subsample,
                  allow_rotation, want_T=True):
        """mvf_icp_batch for lists of (n, 2) float64 contours, one launch per 4096 pairs.  Returns host arrays gamma (P,), stats
        (P, 2) int32 (rounds, inliers of the last query), translation (P, 2) and the list of T_contour_2 (None without want_T)."""
        P = len(contours_1)
        if P == 0:
            return np.zeros(0), np.zeros((0, 2), dtype=np.int32), np.zeros((0, 2)), ([] if want_T else None)
        c1, o1 = self._pack_rows(contours_1, 2)
        c2, o2 = self._pack_rows(contours_2, 2)
        n1, n2 = np.diff(o1), np.diff(o2)
        m2 = np.where((subsample > 0) & (n2 > subsample), subsample, n2)  # rows of every T_contour_2
        oT = np.zeros(P + 1, dtype=np.int64)
        np.cumsum(m2, out=oT[1:])
        d1, d2 = self.h2d(c1), self.h2d(c2)
        gamma, stats = self.empty(P, dtype=torch.float64), self.empty(P, 2, dtype=torch.int32)
        shift = self.empty(P, 2, dtype=torch.float64)
        T = self.empty(max(int(oT[-1]), 1), 2, dtype=torch.float64) if want_T else None
        recs = np.zeros(P, dtype=np.dtype([(f, np.int64) for f, _ in _lib.IcpProblem._fields_]))
        assert recs.dtype.itemsize == C.sizeof(_lib.IcpProblem)
        recs["contour_1"], recs["n1"] = _ptr(d1) + o1[:-1] * 16, n1
        recs["contour_2"], recs["n2"] = _ptr(d2) + o2[:-1] * 16, n2
        recs["gamma"] = _ptr(gamma) + np.arange(P, dtype=np.int64) * 8
        recs["stats"] = _ptr(stats) + np.arange(P, dtype=np.int64) * 8
        recs["translation"] = _ptr(shift) + np.arange(P, dtype=np.int64) * 16
        recs["T_contour_2"] = (_ptr(T) + oT[:-1] * 16) if want_T else 0
        need = int(self.lib.mvf_icp_batch_workspace_bytes(P))
        ws = self.empty(max(need // 8, 1), dtype=torch.float64)
        _lib.check(self.lib.mvf_icp_batch(recs.ctypes.data_as(C.POINTER(_lib.IcpProblem)), P, int(max_iter), float(error_threshold),
                                          float(inlier_threshold), float(gamma_threshold), int(subsample), int(bool(allow_rotation)),
                                          _ptr(ws), ws.numel() * 8, self._stream()), "mvf_icp_batch")
        outs = self.to_host([gamma, stats, shift] + ([T] if want_T else []), own_pinned=False)  # (synchronises: recs may go)
        g, st, sh = (np.array(o) for o in outs[:3])
        Ts = None
        if want_T:
            Th = np.array(outs[3])
            Ts = [Th[oT[i]:oT[i + 1]] for i in range(P)]
        return g, st, sh, Ts

    def mesh_upload(self, points, edges):
        """The device copies (verts (V, 3) float64, edges (E, 2) int32) of a mesh, for the two calls below."""
        return self.h2d(np.ascontiguousarray(points, dtype=np.float64)), self.h2d(np.ascontiguousarray(edges, dtype=np.int32))

    @_on_device
    def mesh_loss(self, dev_mesh, mean, params, heights, contours, max_iter, error_threshold, inlier_threshold, gamma_threshold,
                  subsample):
        """mvf_mesh_loss: params (n_T, 5), heights (n_S,), contours: list of n_S (n, 2) arrays.  Returns host (loss (n_T,), gamma
        (n_T, n_S), count (n_T, n_S) int32)."""
        verts, edges = dev_mesh
        params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 5)
        nT, nS = len(params), len(heights)
        if nT == 0:
            return np.zeros(0), np.zeros((0, nS)), np.zeros((0, nS), dtype=np.int32)
        flat, off = self._pack_rows(list(contours), 2)
        dp, dh, dc, do = self.h2d(params), self.h2d(np.ascontiguousarray(heights, dtype=np.float64)), self.h2d(flat), self.h2d(off)
        loss, gamma = self.empty(nT, dtype=torch.float64), self.empty(nT, nS, dtype=torch.float64)
        count = self.empty(nT, nS, dtype=torch.int32)
        need = int(self.lib.mvf_mesh_loss_workspace_bytes(nT, nS))
        ws = self.empty(max(need // 8, 2), dtype=torch.float64)
        m3 = (C.c_double * 3)(*[float(v) for v in mean])
        _lib.check(self.lib.mvf_mesh_loss(_ptr(verts), verts.shape[0], _ptr(edges), edges.shape[0], m3, _ptr(dp), nT, _ptr(dh), _ptr(dc),
                                          _ptr(do), flat.shape[0], nS, int(max_iter), float(error_threshold), float(inlier_threshold),
                                          float(gamma_threshold), int(subsample), _ptr(loss), _ptr(gamma), _ptr(count), _ptr(ws),
                                          ws.numel() * 8, self._stream()), "mvf_mesh_loss")
        return tuple(np.array(o) for o in self.to_host([loss, gamma, count], own_pinned=False))

    @_on_device
    def mesh_contours(self, dev_mesh, mean, param, heights):
        """mvf_mesh_contours: the list of n_S (n, 2) contours of the mesh under one transformation (5 numbers), whole.  Two
        calls: with capacity 0 for the counts, then with the largest count as the capacity."""
        verts, edges = dev_mesh
        nS = len(heights)
        dh = self.h2d(np.ascontiguousarray(heights, dtype=np.float64))
        counts = self.empty(nS, dtype=torch.int32)
        m3 = (C.c_double * 3)(*[float(v) for v in mean])
        p5 = (C.c_double * 5)(*[float(v) for v in param])

        def call(cap, pts):
            _lib.check(self.lib.mvf_mesh_contours(_ptr(verts), verts.shape[0], _ptr(edges), edges.shape[0], m3, p5, _ptr(dh), nS, cap,
                                                  _ptr(pts), _ptr(counts), self._stream()), "mvf_mesh_contours")

        call(0, None)
        cnt = np.array(self.d2h(counts))
        cap = int(cnt.max())
        if cap == 0:
            return [np.zeros((0, 2)) for _ in range(nS)]
        pts = self.empty(nS, cap, 2, dtype=torch.float64)
        call(cap, pts)
        host = np.array(self.d2h(pts))
        return [host[s, : cnt[s]].copy() for s in range(nS)]

    # ---- density of the cloud (mvf_kde.hip): centred host arrays in, a host (n, C) float64 array out ----
    @_on_device
    def kde(self, targets, sources, kernel, bandwidth, weight=None, group=None, C=1):
        """mvf_kde: out[i, c] = log sum over the sources j of column c (group[j] == c; one column without `group`) of
        w_j K(|t_i - s_j| / bandwidth), unnormalised, -inf where nothing is in reach.  targets (n, d), sources (N, d): host
        float64, d <= 3, centred by the caller (they are rounded to the cell dtype here; every distance is float64); weight (N,)
        float64 or None; group (N,) integers in [0, C) or None.  The columns run in chunks of KDE_MAX_COLUMNS."""
        t4, s4 = self.to_x4(targets), self.to_x4(sources)
        n, N, d, C = int(t4.shape[0]), int(s4.shape[0]), int(np.shape(sources)[1]), int(C)
        w = None if weight is None else self.h2d(np.ascontiguousarray(weight, dtype=np.float64))
        g = None if group is None else self.h2d(np.ascontiguousarray(group, dtype=np.int32))
        out = self.empty(n, C, dtype=torch.float64)
        ws = None
        for c0 in range(0, C, _lib.KDE_MAX_COLUMNS):
            cc = min(_lib.KDE_MAX_COLUMNS, C - c0)
            need = int(self.lib.mvf_kde_workspace_bytes(n, N, cc))
            if ws is None or ws.numel() * 8 < need:
                ws = self.empty(max(need // 8, 1), dtype=torch.float64)
            part = out if cc == C else self.empty(n, cc, dtype=torch.float64)
            gc = g if (g is None or c0 == 0) else g - c0   # a source of another chunk falls outside [0, cc): in no column
            _lib.check(self.lib.mvf_kde(_ptr(t4), n, _ptr(s4), N, d, _lib.KDE_KERNELS[kernel], float(bandwidth), _ptr(w), _ptr(gc), cc,
                                        _ptr(part), _ptr(ws), ws.numel() * 8, self.cdtype, self._stream()), "mvf_kde")
            if part is not out:
                out[:, c0 : c0 + cc] = part
        return np.array(self.d2h(out))

    # ---- shape of the cloud (mvf_shape.hip): float64 whatever the cell dtype ----
    @_on_device
    def shape_queue(self, pts, lo, hi, order, centroid):
        """mvf_shape_descriptors queued on the current stream, nothing read back: pts (n, 3) host float64, lo / hi the (3, nsub)
        interval tables, order 1 | 2 | 3, centroid the mean of the points.  Returns what ``shape_read`` takes; each queued call
        owns its buffers, so any number of them may wait for one read."""
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        n, nsub = int(pts.shape[0]), int(np.shape(lo)[1])
        cap = max(min(nsub ** 3, n // 2), 1)
        dp = self.h2d(pts)
        dlo, dhi = self.h2d(np.ascontiguousarray(lo, dtype=np.float64)), self.h2d(np.ascontiguousarray(hi, dtype=np.float64))
        i32, i64, f64 = torch.int32, torch.int64, torch.float64
        outs = [self.empty(n, dtype=i32), self.empty(cap, dtype=i32), self.empty(cap, dtype=i64), self.empty(cap, dtype=f64),
                self.empty(cap, dtype=f64), self.empty(cap, dtype=i32), self.empty(cap, 2, dtype=f64), self.empty(3, dtype=i64)]
        need = int(self.lib.mvf_shape_descriptors_workspace_bytes(n, nsub))
        ws = self.empty(max(need // 8, 1), dtype=f64)
        g = (C.c_double * 3)(*[float(v) for v in centroid])
        _lib.check(self.lib.mvf_shape_descriptors(_ptr(dp), n, _ptr(dlo), _ptr(dhi), nsub, int(order), g, *[_ptr(t) for t in outs],
                                                  _ptr(ws), ws.numel() * 8, self._stream()), "mvf_shape_descriptors")
        return outs, (dp, dlo, dhi, ws)  # (the inputs and the workspace live until the read)

    @_on_device
    def shape_read(self, queued):
        """The results of ``shape_queue`` calls with one synchronisation: a list of dicts of host arrays, the per-subspace ones
        cut to the number of kept subspaces."""
        host = self.to_host([t for outs, _ in queued for t in outs], own_pinned=False)
        res = []
        for q in range(len(queued)):
            pv, voxel, count, cosine, dist, rank, sv, counts = host[8 * q : 8 * q + 8]
            m = int(counts[0])
            res.append(dict(voxel=voxel[:m].copy(), count=count[:m].copy(), cosine=cosine[:m].copy(), dist=dist[:m].copy(),
                            rank=rank[:m].copy(), sigma_max=sv[:m, 0].copy(), sigma_min_ratio=sv[:m, 1].copy(), point_voxel=pv,
                            n_dropped=int(counts[1]), n_overlap=int(counts[2])))
        return res

    # ---- digitization (mvf_heat.hip): the heat-equation loops, float64 whatever the cell dtype ----
    def _heat_ws(self, need):
        """A 256-byte aligned workspace of at least `need` bytes (torch's allocator aligns to 512)."""
        ws = self.empty(max(-(-need // 8), 1), dtype=torch.float64)
        assert ws.data_ptr() % 256 == 0
        return ws

    @_on_device
    def heat_grid(self, init, border, mask, max_err, max_itr, block_steps=0):
        """mvf_heat_grid: the whole loop of ``domain_heat_eqn_solver``.  init, border, mask: host (H, W) float64 (the field with
        its boundary lines written, ``field_border``, ``field_mask``).  Returns (field * mask as a host (H, W) float64 array,
        sweeps, last err, hit_max_itr).  block_steps: 0 (the library's choice) or the sweeps per launch, 1 .. HEAT_MAX_STEPS."""
        init = np.ascontiguousarray(init, dtype=np.float64)
        H, W = (int(v) for v in init.shape)
        di, db, dm = (self.h2d(np.ascontiguousarray(a, dtype=np.float64)) for a in (init, border, mask))
        out = self.empty(H, W, dtype=torch.float64)
        need = int(self.lib.mvf_heat_grid_workspace_bytes(H, W))
        ws = self._heat_ws(need)
        sweeps, err, hit = C.c_int64(0), C.c_double(0.0), C.c_int(0)
        _lib.check(self.lib.mvf_heat_grid(_ptr(di), _ptr(db), _ptr(dm), H, W, float(max_err), float(max_itr), int(block_steps), _ptr(out),
                                          C.byref(sweeps), C.byref(err), C.byref(hit), _ptr(ws), ws.numel() * 8, self._stream()),
                   "mvf_heat_grid")
        return np.array(self.d2h(out)), int(sweeps.value), float(err.value), bool(hit.value)

    @_on_device
    def heat_graph(self, indptr, indices, data, fixed_value, max_err, max_itr):
        """mvf_heat_graph: the whole loop of ``digitize_general`` on the CSC arrays of the adjacency (host: indptr (n + 1,) int64,
        indices int32 in ascending row order per column, data float64) and fixed_value (n,) float64, the reference's
        ``mask_field``.  Returns (field as a host (n,) float64 array, sweeps, last err, hit_max_itr)."""
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=np.float64)
        fixed_value = np.ascontiguousarray(fixed_value, dtype=np.float64)
        n = int(fixed_value.shape[0])
        if indptr.shape != (n + 1,) or len(indices) != len(data) or (n and int(indptr[-1]) != len(data)):
            raise ValueError("malformed CSC adjacency: indptr must have n + 1 entries that end at len(data) == len(indices)")
        out = self.empty(n, dtype=torch.float64)
        need = int(self.lib.mvf_heat_graph_workspace_bytes(n, len(data)))
        ws = self._heat_ws(need)
        sweeps, err, hit = C.c_int64(0), C.c_double(0.0), C.c_int(0)
        hp = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        _lib.check(self.lib.mvf_heat_graph(hp(indptr), hp(indices), hp(data), hp(fixed_value), n, float(max_err), float(max_itr),
                                           _ptr(out), C.byref(sweeps), C.byref(err), C.byref(hit), _ptr(ws), ws.numel() * 8,
                                           self._stream()), "mvf_heat_graph")
        return np.array(self.d2h(out)), int(sweeps.value), float(err.value), bool(hit.value)

    # ---- a kernel along the tissue (mvf_graph.hip): float64 whatever the cell dtype ----
    SSSP_BATCH = 32  # Bellman-Ford sweeps queued between two reads of the status block

    @_on_device
    def knn(self, points, k):
        """mvf_knn: points a device (n, d) float64 tensor, d in {2, 3}.  Returns device (idx (n, k) int32, dist (n, k) float64),
        every row ascending by (distance, index), the point itself left out by index.  Queued on the current stream."""
        n, d = (int(v) for v in points.shape)
        points = points.contiguous()
        idx, dist = self.empty(n, int(k), dtype=torch.int32), self.empty(n, int(k), dtype=torch.float64)
        need = int(self.lib.mvf_knn_workspace_bytes(n, d, int(k)))
        ws = self._heat_ws(need)
        _lib.check(self.lib.mvf_knn(_ptr(points), n, d, int(k), _ptr(idx), _ptr(dist), _ptr(ws), ws.numel() * 8, self._stream()),
                   "mvf_knn")
        return idx, dist

    @_on_device
    def graph_sssp(self, indptr, indices, weights, n, sources):
        """Shortest-path distances from `sources` (device int32 (m,)) through the CSR graph (device indptr int64 (n + 1,), indices
        int32, weights float64): mvf_graph_sssp queued SSSP_BATCH sweeps at a time, the status block read between the batches
        (mvf_read_back), until a whole batch lowered nothing.  A path has at most n - 1 edges: after n sweeps in all without that
        the graph's arrays are at fault, and this raises.  Returns (device (n, m) float64 with +inf where there is no path, sweeps
        queued)."""
        n, m, nnz = int(n), int(sources.shape[0]), int(indices.shape[0])
        dist = self.empty(n, m, dtype=torch.float64)
        status = self.zeros(_lib.SSSP_STATUS, dtype=torch.int64)
        queued, init = 0, 1
        while True:
            _lib.check(self.lib.mvf_graph_sssp(_ptr(indptr), _ptr(indices) if nnz else None, _ptr(weights) if nnz else None, n, nnz,
                                               _ptr(sources), m, _ptr(dist), m, init, self.SSSP_BATCH, _ptr(status), self._stream()),
                       "mvf_graph_sssp")
            queued, init = queued + self.SSSP_BATCH, 0
            if int(self.read_host(status)[0]) == 0:
                return dist, queued
            if queued >= n + self.SSSP_BATCH:
                raise _lib.MVFError(f"graph_sssp: no fixed point after {queued} sweeps over {n} nodes (a negative weight?)")

    @_on_device
    def pack_ublk(self, U):
        """The rows of a device (n, m) float64 matrix as the Gram kernel's operand cache, in the cell dtype, uncentred
        (mvf_ublk_pack, the way pca_pack fills it): what gram_on_cache, rhs_on_cache, apply_on_cache and pinv_diag_cached read."""
        n, m = (int(v) for v in U.shape)
        U = U.contiguous()
        need = self.ublk_bytes(n, m)
        self._ublk = None
        self._ublk = torch.empty(need // self._ublk_itemsize(), dtype=self.tdtype, device=self.device)
        self._ublk_key = None  # (no (x4, ctrl4, beta) builds this cache: `gram` must not mistake it for a fit's)
        self._ublk_shape = (n, m)
        self._cache_bufs = None
        _lib.check(self.lib.mvf_ublk_pack(_ptr(U), 0, n, m, None, n, 0, _ptr(self._ublk), need, self.cdtype, self._stream()),
                   "mvf_ublk_pack")

    @_on_device
    def gram_on_cache(self, P, G):
        """G = U^T diag(P) U from the packed cache: the tile and reduce stages of mvf_gram_cached (neither reads x4 / ctrl4,
        which must only be non-NULL: P stands in, as in pca_gram)."""
        n, m = self._ublk_shape
        need = int(self.lib.mvf_gram_workspace_bytes(n, m, self.cdtype))
        if self._gram_ws is None or self._gram_ws.numel() < need:
            self._gram_ws = None
            self._gram_ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.mvf_gram_cached(_lib.GRAM_TILES | _lib.GRAM_REDUCE, _ptr(self._ublk), _ptr(P), _ptr(P), None, n, _ptr(P), m,
                                            0.0, _ptr(G), None, _ptr(self._gram_ws), self._gram_ws.numel(), self.cdtype,
                                            self._stream()), "mvf_gram_cached")

    def _cache_operands(self):
        """The padded operands of the wide kernels on the packed cache, allocated once per pack_ublk: Yd (n rounded up to 256, 16)
        and a zero twin, Vd (n, 16), r (n,), Cd (m rounded up to 128, 16 float64).  Only the live columns are ever written."""
        if getattr(self, "_cache_bufs", None) is None:
            n, m = self._ublk_shape
            n_pad, m_pad = self.wide_pads(n, m)
            self._cache_bufs = dict(Yd=self.zeros(n_pad, 16), zero=self.zeros(n_pad, 16), Vd=self.empty(n, 16), r=self.empty(n),
                                    Cd=self.zeros(m_pad, 16, dtype=torch.float64))
        return self._cache_bufs

    def _cache_rows(self, Y4):
        """Y4 (n, 4) as the padded (n rounded up to 256, 16) operand of the wide kernels (the other columns zero)."""
        Yd = self._cache_operands()["Yd"]
        Yd[: Y4.shape[0], :4] = Y4
        return Yd

    @_on_device
    def rhs_on_cache(self, P, Y4, R):
        """R (m, 3 float64) = U^T diag(P) Y4[:, :3] from the packed cache (mvf_rhs_cached)."""
        self.rhs_wide(P, self._cache_rows(Y4), 3, self._ublk_shape[1], R)

    @_on_device
    def apply_on_cache(self, C):
        """V4 (n, 4, cell dtype) = U C for C (m, 3 float64) from the packed cache (mvf_apply_cached against Yd = 0)."""
        n, m = self._ublk_shape
        b = self._cache_operands()
        b["Cd"][:m, :3] = C
        self.apply_wide(b["Cd"], 3, m, b["zero"], None, b["Vd"], b["r"], None)
        return b["Vd"][:, :4].contiguous()

    @_on_device
    def pinv_diag_cached(self, rcond=None, lowrank=False):
        """pinv_diag with the rows of U read from the packed cache (mvf_pinv_diag_cached)."""
        ws = self._lr_ws if lowrank else self._mn_ws
        if ws is None or self._ublk is None:
            raise RuntimeError("pinv_diag_cached needs a previous decomposition and the packed cache")
        n, m = self._ublk_shape
        out = torch.empty(n, dtype=torch.float64, device=self.device)
        rc = float(np.finfo(np.float64).eps) if rcond is None else float(rcond)
        _lib.check(self.lib.mvf_pinv_diag_cached(_ptr(self._ublk), self._ublk.numel() * self._ublk_itemsize(), n, m, rc,
                                                 1 if lowrank else 0, _ptr(out), _ptr(ws), ws.numel(), self.cdtype, self._stream()),
                   "mvf_pinv_diag_cached")
        return out

    # ---- PCA across slices on the kernel-value cache (mvf_pca.hip + the cached Gram / apply kernels, unchanged) ----
    PCA_UPLOAD_BYTES = 256 << 20  # rows of a dense slice travel in chunks of at most this much (each chunk is a slice of its own)

    def mem_free(self):
        """Bytes of device memory free right now."""
        return int(torch.cuda.mem_get_info(self.device)[0])

    @_on_device
    def pca_open(self, n_total, g):
        """The cache (mvf_ublk_bytes(n_total, g) of the cell dtype) and the partial column sums of one PCA."""
        self.pca_close()
        self._pca_n, self._pca_g = int(n_total), int(g)
        need = self.ublk_bytes(self._pca_n, self._pca_g)
        self._ublk = torch.empty(need // self._ublk_itemsize(), dtype=self.tdtype, device=self.device)
        self._ublk_key = None  # (no (x4, ctrl4, beta) builds this cache: `gram` must not mistake it for a fit's)
        self._pca_mu = None
        self._pca_dev = {}  # slice index -> the device copies of a CSR slice's three arrays (uploaded once, used by both passes)

    def pca_close(self):
        self.drop_ublk()
        self._pca_mu = self._pca_dev = None

    def _pca_chunks(self, sl):
        """A dense slice as (first row, device rows) chunks of at most PCA_UPLOAD_BYTES."""
        a = sl[1]
        rows = max(1, self.PCA_UPLOAD_BYTES // max(1, a.shape[1] * a.itemsize))
        for lo in range(0, a.shape[0], rows):
            yield lo, self.h2d(a[lo : lo + rows])

    def _pca_csr(self, i, sl):
        """Device (indptr, indices, data) of CSR slice i and the staging area of expanded rows (bounded like assign_prepare's)."""
        _, indptr, indices, data, n, g = sl
        if i not in self._pca_dev:
            if len(data) == 0:  # an all-zero slice: the arrays still need an address
                indices, data = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=data.dtype)
            self._pca_dev[i] = (self.h2d(indptr), self.h2d(indices), self.h2d(data))
        rows = min(n, CSR_STAGING_MAX_ROWS, max(1, CSR_STAGING_MAX_BYTES // (data.itemsize * g)))
        stage = self.empty(-(-rows * g * data.itemsize // 8), dtype=torch.float64)
        return self._pca_dev[i], stage

    @_on_device
    def pca_means(self, slices):
        """Column means of the stacked slices (mvf_colmeans / mvf_colmeans_csr): host float64 (g,); kept on the device for
        pca_pack.  slices: what `pca_slices` made of the caller's matrices."""
        n_total, g = self._pca_n, self._pca_g
        need = int(self.lib.mvf_colmeans_workspace_bytes(n_total, g))
        ws = self.empty(need // 8, dtype=torch.float64)
        self._pca_mu = self.empty(g, dtype=torch.float64)
        row0 = 0
        for i, sl in enumerate(slices):
            if sl[0] == "csr":
                (d_indptr, d_indices, d_data), stage = self._pca_csr(i, sl)
                _lib.check(self.lib.mvf_colmeans_csr(_ptr(d_indptr), _ptr(d_indices), _ptr(d_data), int(sl[3].dtype == np.float32),
                                                     sl[4], g, n_total, row0, _ptr(self._pca_mu), _ptr(ws), need, _ptr(stage),
                                                     stage.numel() * 8, self._stream()), "mvf_colmeans_csr")
                row0 += sl[4]
                continue
            for lo, xd in self._pca_chunks(sl):
                _lib.check(self.lib.mvf_colmeans(_ptr(xd), int(xd.dtype == torch.float32), xd.shape[0], g, n_total, row0 + lo,
                                                 _ptr(self._pca_mu), _ptr(ws), need, self._stream()), "mvf_colmeans")
            row0 += sl[1].shape[0]
        return self.d2h(self._pca_mu)

    @_on_device
    def pca_pack(self, slices, centred):
        """The slices, one behind the other, minus pca_means' means (centred) or as they are, into the cache."""
        n_total, g = self._pca_n, self._pca_g
        mu = self._pca_mu if centred else None
        if centred and mu is None:
            raise RuntimeError("pca_pack(centred=True) needs pca_means first")
        nbytes = self._ublk.numel() * self._ublk_itemsize()
        row0 = 0
        for i, sl in enumerate(slices):
            if sl[0] == "csr":
                (d_indptr, d_indices, d_data), stage = self._pca_csr(i, sl)
                _lib.check(self.lib.mvf_ublk_pack_csr(_ptr(d_indptr), _ptr(d_indices), _ptr(d_data), int(sl[3].dtype == np.float32),
                                                      sl[4], g, _ptr(mu), n_total, row0, _ptr(self._ublk), nbytes, _ptr(stage),
                                                      stage.numel() * 8, self.cdtype, self._stream()), "mvf_ublk_pack_csr")
                row0 += sl[4]
                continue
            for lo, xd in self._pca_chunks(sl):
                _lib.check(self.lib.mvf_ublk_pack(_ptr(xd), int(xd.dtype == torch.float32), xd.shape[0], g, _ptr(mu), n_total,
                                                  row0 + lo, _ptr(self._ublk), nbytes, self.cdtype, self._stream()), "mvf_ublk_pack")
            row0 += sl[1].shape[0]
        self._pca_dev = {}

    @_on_device
    def pca_gram(self):
        """G = Xc^T Xc (g x g float64, host) from the packed cache: mvf_gram_cached's tile and reduce stages with P = 1.
        Neither stage reads x4 / ctrl4 (they must only be non-NULL: P stands in), y4 and R belong to stages not asked for."""
        n, g = self._pca_n, self._pca_g
        need = int(self.lib.mvf_gram_workspace_bytes(n, g, self.cdtype))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        P = torch.ones(n, dtype=self.tdtype, device=self.device)
        G = self.empty(g, g, dtype=torch.float64)
        _lib.check(self.lib.mvf_gram_cached(_lib.GRAM_TILES | _lib.GRAM_REDUCE, _ptr(self._ublk), _ptr(P), _ptr(P), None, n, _ptr(P),
                                            g, 0.0, _ptr(G), None, _ptr(ws), ws.numel(), self.cdtype, self._stream()),
                   "mvf_gram_cached")
        return self.d2h(G)

    @_on_device
    def pca_scores(self, V):
        """Xc V for host V (g, k <= 128 float64): mvf_apply_cached with C = V against Yd = 0; the scores come back in the
        cell dtype, as the kernel stores them, widened to float64 on the host: (n_total, k)."""
        n, g = self._pca_n, self._pca_g
        V = np.asarray(V, dtype=np.float64)
        k = V.shape[1]
        n_pad, m_pad = self.wide_pads(n, g)
        ld = -(-k // 16) * 16
        Ch = np.zeros((m_pad, ld))
        Ch[:g, :k] = V
        Cd = self.h2d(Ch)
        Yd = self.zeros(n_pad, ld)
        Vd = self.empty(n, ld)
        r = self.empty(n)
        ws = self._wide_ws(n, g)
        _lib.check(self.lib.mvf_apply_cached(_ptr(self._ublk), n, g, _ptr(Cd), ld, k, _ptr(Yd), ld, None, _ptr(Vd), _ptr(r), None,
                                             _ptr(ws), ws.numel(), self.cdtype, self._stream()), "mvf_apply_cached")
        return self.d2h(Vd[:, :k]).astype(np.float64)

    @staticmethod
    def _affine_buf(affine):
        if affine is None:
            return None
        import ctypes

        alpha, jmul, A, b = affine
        al = np.broadcast_to(np.asarray(alpha, dtype=np.float64).reshape(-1), (3,))  # a scalar or one value per component
        vals = [float(x) for x in al] + [float(jmul)] + [float(x) for x in np.asarray(A, dtype=np.float64).reshape(9)] + \
               [float(x) for x in np.asarray(b, dtype=np.float64).reshape(3)]
        return (ctypes.c_double * 16)(*vals)

    @_on_device
    def integrate(self, x4, ctrl4, beta, C, dt, substeps, n_out, affine=None):
        """RK4 trajectories of dx/dt = v(x): returns a float64 device tensor (n, n_out, 3)."""
        n, m = x4.shape[0], ctrl4.shape[0]
        traj = torch.empty(n, n_out, 3, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.mvf_integrate(_ptr(x4), n, _ptr(ctrl4), m, float(beta), _ptr(C), self._affine_buf(affine),
                                          float(dt), int(substeps), int(n_out), _ptr(traj), self.cdtype,
                                          self._stream()), "mvf_integrate")
        return traj

    @_on_device
    def integrate_rk45(self, x4, ctrl4, beta, C, d, world, t_bound, rtol, atol, max_step, max_steps, sampling, n_out,
                       affine=None):
        """SciPy-RK45 trajectories of dx/dt = v(x) (mvf.h: mvf_integrate_rk45).  `world` = (scale (3,), offset (3,)) maps
        the x4 coordinates to the caller's (y = q * scale + offset), `sampling` = _lib.RK45_UNIFORM_TIME | RK45_ARC_LENGTH.
        Returns host arrays (t (n, n_out), traj (n, n_out, 3) in world coordinates, stats (n, 4) int32 = accepted,
        rejected, field evaluations, status), copied back in one transfer."""
        import ctypes

        n, m = x4.shape[0], ctrl4.shape[0]
        # one device buffer: t | traj | stats (n x 4 int32 = n x 2 float64), so that one copy brings everything back
        buf = torch.empty(n * (4 * n_out + 2), dtype=torch.float64, device=self.device)
        t = buf[: n * n_out].view(n, n_out)
        traj = buf[n * n_out : 4 * n * n_out].view(n, n_out, 3)
        stats = buf[4 * n * n_out :].view(torch.int32).view(n, 4)
        scale, offset = world
        w = (ctypes.c_double * 6)(*[float(v) for v in np.asarray(scale, dtype=np.float64).reshape(3)],
                                  *[float(v) for v in np.asarray(offset, dtype=np.float64).reshape(3)])
        _lib.check(self.lib.mvf_integrate_rk45(_ptr(x4), n, _ptr(ctrl4), m, float(beta), _ptr(C), self._affine_buf(affine),
                                               int(d), w, float(t_bound), float(rtol), float(atol), float(max_step),
                                               int(max_steps), int(sampling), int(n_out), _ptr(t), _ptr(traj),
                                               _ptr(stats), self.cdtype, self._stream()), "mvf_integrate_rk45")
        (host,) = self.to_host([buf], own_pinned=False)
        return (host[: n * n_out].reshape(n, n_out), host[n * n_out : 4 * n * n_out].reshape(n, n_out, 3),
                host[4 * n * n_out :].view(np.int32).reshape(n, 4))

    @_on_device
    def eval(self, x4, ctrl4, beta, C, flags, affine=None):
        """Fused evaluator.  Returns a dict of float64 device tensors for the requested MVF_EVAL_* flags.
        `affine` = (alpha, jmul, A (3x3), b (3)) applies v = alpha K@C + A q + b, J = jmul J (GP variant)."""
        n, m = x4.shape[0], ctrl4.shape[0]
        f64 = torch.float64
        out = {}

        def buf(flag, *shape):
            if flags & flag:
                t = torch.empty(*shape, dtype=f64, device=self.device)
                out[flag] = t
                return t
            return None

        v = buf(_lib.EVAL_V, n, 3)
        jac = buf(_lib.EVAL_JAC, 3, 3, n)
        div = buf(_lib.EVAL_DIV, n)
        curl = buf(_lib.EVAL_CURL, n, 3)
        acc = buf(_lib.EVAL_ACC, n, 3)
        curv = buf(_lib.EVAL_CURV, n, 3)
        tors = buf(_lib.EVAL_TORS, n, 3)
        jdet = buf(_lib.EVAL_JDET, n)
        aff = self._affine_buf(affine)
        _lib.check(self.lib.mvf_eval_affine(_ptr(x4), n, _ptr(ctrl4), m, float(beta), _ptr(C), aff, int(flags), _ptr(v),
                                            _ptr(jac), _ptr(div), _ptr(curl), _ptr(acc), _ptr(curv), _ptr(tors),
                                            _ptr(jdet), self.cdtype, self._stream()), "mvf_eval_affine")
        return out

    @_on_device
    def eval_wide(self, x4, ctrl4, d, beta, C, flags):
        """Values and spatial gradients of a field with any number of output columns at d <= 3 (mvf_eval_wide): x4 (n, 4) and
        ctrl4 (m, 4) from to_x4, C (m, dy) float64 device tensor with unit column stride - a column slice of a wider matrix
        is passed as it is, its row stride is the kernel's ldc.  flags: EVAL_V | EVAL_JAC.  Returns {flag: float64 device
        tensor}: v (n, dy), jac (dy, d, n)."""
        n, m = x4.shape[0], ctrl4.shape[0]
        if C.dim() != 2 or C.shape[0] != m or C.dtype != torch.float64 or (C.shape[1] > 1 and C.stride(1) != 1):
            raise ValueError(f"eval_wide: expected float64 coefficients ({m}, dy) with unit column stride, got "
                             f"{tuple(C.shape)} {C.dtype} strides {tuple(C.stride())}")
        if x4.dtype != self.tdtype or ctrl4.dtype != self.tdtype:
            raise TypeError(f"eval_wide: expected {self.tdtype} points, got {x4.dtype} / {ctrl4.dtype}")
        dy = C.shape[1]
        ldc = max(int(C.stride(0)), dy) if m > 1 else dy
        shapes = {_lib.EVAL_V: (n, dy), _lib.EVAL_JAC: (dy, int(d), n)}
        out = {f: torch.empty(*s, dtype=torch.float64, device=self.device) for f, s in shapes.items() if flags & f}
        _lib.check(self.lib.mvf_eval_wide(_ptr(x4), n, _ptr(ctrl4), m, int(d), float(beta), _ptr(C), ldc, dy, int(flags),
                                          _ptr(out.get(_lib.EVAL_V)), dy, _ptr(out.get(_lib.EVAL_JAC)), self.cdtype,
                                          self._stream()), "mvf_eval_wide")
        return out

    @_on_device
    def eval_d(self, xd, ctrld, beta, C, flags):
        """Fused evaluator for 4 <= d <= 8 (mvf_eval_d): xd (n, d), ctrld (m, d) from to_xd, C (m, dy) float64 device
        tensor, dy <= 8.  Returns {flag: float64 device tensor}: v (n, dy), jac (dy, d, n), and for dy == d div (n,),
        acc (n, d), curv (n, d)."""
        n, d = xd.shape
        m, dy = C.shape
        if ctrld.dim() != 2 or ctrld.shape[1] != d or ctrld.shape[0] != m:
            raise ValueError(f"eval_d: points (n, {d}), control points {tuple(ctrld.shape)} and coefficients {tuple(C.shape)} "
                             f"disagree")
        if xd.dtype != self.tdtype or ctrld.dtype != self.tdtype or C.dtype != torch.float64:
            raise TypeError(f"eval_d: expected {self.tdtype} points and float64 coefficients, got {xd.dtype} / {ctrld.dtype} / "
                            f"{C.dtype}")
        C = C.contiguous()
        f64 = torch.float64
        shapes = {_lib.EVAL_V: (n, dy), _lib.EVAL_JAC: (dy, d, n), _lib.EVAL_DIV: (n,), _lib.EVAL_ACC: (n, d),
                  _lib.EVAL_CURV: (n, d)}
        out = {f: torch.empty(*s, dtype=f64, device=self.device) for f, s in shapes.items() if flags & f}
        _lib.check(self.lib.mvf_eval_d(_ptr(xd), n, _ptr(ctrld), m, d, float(beta), _ptr(C), dy, int(flags),
                                       *(_ptr(out.get(f)) for f in shapes), self.cdtype, self._stream()), "mvf_eval_d")
        return out
