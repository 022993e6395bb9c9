"""Kernel-level tests of the PCA entry points through the raw C ABI: ``mvf_colmeans`` / ``mvf_ublk_pack``, their CSR twins,
and ``mvf_gram_cached`` on a packed cache.  Shapes are the smallest that cross an edge: 1 / 255 / 256 / 257 / 700 rows (the
cache pads rows to 256) against 1 / 15 / 16 / 17 / 127 / 128 / 129 / 200 columns (cache blocks of 16, tiles of 128, mean
workgroups of 256 columns), and 2500 rows in slices that cut the 1024-row blocks of the column sums.  Every output and the
workspace sit in front of a guard; every call is checked for equal bits on a second run where the issue is determinism.

Bounds: means against ``math.fsum`` with the plain summation bound n eps max|x| (float64 eps: the sums are float64); the
cache bit for bit against ``(X - mu_device)`` rounded to the cell dtype in the NumPy statement of the layout
(``_pca_case.ublk_layout``); the Gram matrix against ``Xc^T Xc`` of the operands read back, with the bounds of
``test_gpu_kernels.test_gram_vs_oracle`` (1e-11 / 3e-6 relative to the largest entry)."""
import math

import numpy as np
import pytest
import torch

import _pca_case as pc
from _kernel_scaffold import (DEV, MODES, bits as _bits, called as _called, dev as _dev, guarded as _guarded, intact as _guard_ok,
                              same_bits as _same_bits, stream as _stream, under as _under)

pytestmark = pytest.mark.gpu

TD = {"float32": torch.float32, "float64": torch.float64}
SHAPES = [(1, 1), (1, 129), (255, 15), (255, 128), (256, 16), (256, 200), (257, 17), (257, 127), (700, 1), (700, 129), (700, 200),
          (256, 128)]


@pytest.fixture(scope="module")
def lib():
    from spateo_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def _cd(cell):
    from spateo_amd import _lib

    return _lib.MVF_F32 if cell == "float32" else _lib.MVF_F64


def _check(lib, rc, what):
    assert rc == 0, (what, lib.mvf_last_error())


def _matrix(n, g, xdtype, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, g)) * rng.uniform(0.5, 20.0, g) + rng.uniform(-30.0, 30.0, g)
    return np.ascontiguousarray(X.astype(xdtype))


class Run:
    """One matrix of n_total x g: guarded means, workspace and cache, filled through slices."""

    def __init__(self, lib, n_total, g, cell):
        self.lib, self.n, self.g, self.cell = lib, n_total, g, cell
        self.ws_bytes = int(lib.mvf_colmeans_workspace_bytes(n_total, g))
        self.ub_bytes = int(lib.mvf_ublk_bytes(n_total, g, _cd(cell)))
        n_pad, g_pad = pc.pads(n_total, g)
        assert self.ub_bytes == n_pad * g_pad * (4 if cell == "float32" else 8) and self.ws_bytes == -(-n_total // 1024) * g * 8
        self.ws = _guarded(self.ws_bytes // 8)
        self.ws[: self.ws_bytes // 8] = float("nan")  # a partial sum read before it was written would show
        self.mean = _guarded(g)
        item = 4 if cell == "float32" else 8
        self.ublk = _guarded(self.ub_bytes // item, TD[cell], unit=16 // item)   # (the cache must be 16-byte aligned)
        self.keep = []

    def means(self, X, row0=0):
        xd = _dev(X, None)
        self.keep.append(xd)
        _check(self.lib, self.lib.mvf_colmeans(xd.data_ptr(), int(X.dtype == np.float32), X.shape[0], self.g, self.n, row0,
                                               self.mean.data_ptr(), self.ws.data_ptr(), self.ws_bytes, _stream()), "mvf_colmeans")
        _called()

    def pack(self, X, row0=0, centred=True):
        xd = _dev(X, None)
        self.keep.append(xd)
        _check(self.lib, self.lib.mvf_ublk_pack(xd.data_ptr(), int(X.dtype == np.float32), X.shape[0], self.g,
                                                self.mean.data_ptr() if centred else None, self.n, row0, self.ublk.data_ptr(),
                                                self.ub_bytes, _cd(self.cell), _stream()), "mvf_ublk_pack")
        _called()

    def _csr(self, csr, stage_bytes):
        indptr, indices, data = csr
        if len(data) == 0:  # no entry at all: the arrays still need an address (indptr keeps them unread)
            indices, data = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=data.dtype)
        dev = [_dev(a, None) for a in (indptr, indices, data)]
        stage = _guarded(-(-stage_bytes // 8))
        self.keep += dev + [stage]
        return dev, stage

    def means_csr(self, csr, stage_bytes, row0=0):
        (ip, ix, da), stage = self._csr(csr, stage_bytes)
        _check(self.lib, self.lib.mvf_colmeans_csr(ip.data_ptr(), ix.data_ptr(), da.data_ptr(), int(csr[2].dtype == np.float32),
                                                   len(csr[0]) - 1, self.g, self.n, row0, self.mean.data_ptr(), self.ws.data_ptr(),
                                                   self.ws_bytes, stage.data_ptr(), stage_bytes, _stream()), "mvf_colmeans_csr")
        _called()
        torch.cuda.synchronize()
        assert _guard_ok(stage, -(-stage_bytes // 8)), "written behind the staging area"

    def pack_csr(self, csr, stage_bytes, row0=0, centred=True):
        (ip, ix, da), stage = self._csr(csr, stage_bytes)
        _check(self.lib, self.lib.mvf_ublk_pack_csr(ip.data_ptr(), ix.data_ptr(), da.data_ptr(), int(csr[2].dtype == np.float32),
                                                    len(csr[0]) - 1, self.g, self.mean.data_ptr() if centred else None, self.n, row0,
                                                    self.ublk.data_ptr(), self.ub_bytes, stage.data_ptr(), stage_bytes, _cd(self.cell),
                                                    _stream()), "mvf_ublk_pack_csr")
        _called()
        torch.cuda.synchronize()
        assert _guard_ok(stage, -(-stage_bytes // 8)), "written behind the staging area"

    def host(self):
        """(means, flat cache) on the host, the guards checked."""
        torch.cuda.synchronize()
        nel = self.ub_bytes // (4 if self.cell == "float32" else 8)
        assert _guard_ok(self.mean, self.g), "written behind the means"
        assert _guard_ok(self.ws, self.ws_bytes // 8), "written behind the workspace"
        assert _guard_ok(self.ublk, nel), "written behind the cache"
        return self.mean[: self.g].cpu().numpy().copy(), self.ublk[:nel].cpu().numpy().copy()


CONVENTION_COVERS = {"mvf_colmeans": MODES, "mvf_ublk_pack": MODES, "mvf_colmeans_csr": MODES, "mvf_ublk_pack_csr": MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cell", ["float32", "float64"])
@pytest.mark.parametrize("form", ["dense", "csr"])
def test_calling_conventions(lib, form, cell, mode):
    """Means, then the cache from them (mvf_colmeans + mvf_ublk_pack, or their CSR twins at a staging area of 37 rows): the
    plain calls' bits on a side stream behind poisoned inputs, at displaced pointers, and with the inputs unchanged."""
    n, g = 257, 17
    csr, dense = _csr_case(n, g, "float32", seed=n + g)

    def call():
        run = Run(lib, n, g, cell)
        if form == "dense":
            run.means(dense)
            run.pack(dense)
        else:
            run.means_csr(csr, 37 * g * 4 + 5)
            run.pack_csr(csr, 37 * g * 4 + 5)
        return run.host()

    plain, got = _under(mode, call)
    assert _same_bits(plain[0], got[0]) and _same_bits(plain[1], got[1])


def _expected_cache(X, mu, cell):
    Xc = np.asarray(X, dtype=np.float64) - mu if mu is not None else np.asarray(X, dtype=np.float64)
    return pc.ublk_layout(Xc.astype(np.float32 if cell == "float32" else np.float64))


@pytest.mark.parametrize("xdtype", ["float32", "float64"])
@pytest.mark.parametrize("cell", ["float32", "float64"])
@pytest.mark.parametrize("n,g", SHAPES)
def test_means_and_pack(lib, n, g, cell, xdtype):
    X = _matrix(n, g, xdtype, seed=1000 * n + g)
    run = Run(lib, n, g, cell)
    run.means(X)
    run.pack(X)
    mu, flat = run.host()
    exact = np.array([math.fsum(X[:, j].astype(np.float64).tolist()) for j in range(g)]) / n
    err, bound = np.abs(mu - exact).max(), n * pc.EPS * float(np.abs(X).max())
    print(f"means {n} x {g} {xdtype}: max |delta| {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert np.array_equal(_bits(flat), _bits(_expected_cache(X, mu, cell))), "cache differs from (X - mu) in the layout"
    full = pc.from_ublk(flat, n, g)
    assert not full[n:].any() and not full[:, g:].any(), "padding must be exactly zero"
    # a second run on fresh buffers: the same bits
    again = Run(lib, n, g, cell)
    again.means(X)
    again.pack(X)
    mu2, flat2 = again.host()
    assert np.array_equal(_bits(mu), _bits(mu2)) and np.array_equal(_bits(flat), _bits(flat2))


@pytest.mark.parametrize("cell", ["float32", "float64"])
@pytest.mark.parametrize("n,g", [(257, 17), (700, 129)])
def test_pack_without_centring(lib, n, g, cell):
    X = _matrix(n, g, "float64", seed=7)
    run = Run(lib, n, g, cell)
    run.pack(X, centred=False)
    _, flat = run.host()
    assert np.array_equal(_bits(flat), _bits(_expected_cache(X, None, cell)))


def _csr_case(n, g, dtype, seed):
    """(indptr, indices, data), dense equivalent: empty rows, one full row, unsorted indices, out-of-range indices (skipped)."""
    rng = np.random.default_rng(seed)
    dense = np.zeros((n, g), dtype=dtype)
    indptr, indices, data = [0], [], []
    for i in range(n):
        if i % 5 == 0 and i != 10:
            cols = np.array([], dtype=np.int64)                      # an empty row
        elif i == 10 % n:
            cols = rng.permutation(g)                                # a full row, unsorted
        else:
            cols = rng.permutation(g)[: rng.integers(0, max(2, g // 3) + 1)]   # unsorted, distinct
        vals = (rng.standard_normal(len(cols)) * 5 + 1).astype(dtype)
        dense[i, cols] = vals
        cols, vals = cols.tolist(), vals.tolist()
        if i % 7 == 3:                                               # entries outside [0, g): skipped, never an address
            cols += [g, -1, g + 12345, np.iinfo(np.int32).min]
            vals += [99.0, 98.0, 97.0, 96.0]
        indices += cols
        data += vals
        indptr.append(len(indices))
    return (np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int32), np.array(data, dtype=dtype)), dense


@pytest.mark.parametrize("xdtype", ["float32", "float64"])
@pytest.mark.parametrize("cell", ["float32", "float64"])
@pytest.mark.parametrize("n,g", [(257, 17), (700, 129), (1, 1), (2500, 40)])
def test_csr_equals_dense_at_two_staging_sizes(lib, n, g, cell, xdtype):
    csr, dense = _csr_case(n, g, xdtype, seed=n + g)
    ref = Run(lib, n, g, cell)
    ref.means(dense)
    ref.pack(dense)
    mu, flat = ref.host()
    item = 4 if xdtype == "float32" else 8
    for stage_bytes in (g * item, 37 * g * item + 5):   # one row per chunk; 37 rows and a few bytes no row fits
        run = Run(lib, n, g, cell)
        run.means_csr(csr, stage_bytes)
        run.pack_csr(csr, stage_bytes)
        mu_c, flat_c = run.host()
        assert np.array_equal(_bits(mu), _bits(mu_c)), f"means differ at a staging area of {stage_bytes} bytes"
        assert np.array_equal(_bits(flat), _bits(flat_c)), f"cache differs at a staging area of {stage_bytes} bytes"


@pytest.mark.parametrize("cell", ["float32", "float64"])
def test_slices_equal_the_stacked_matrix(lib, cell):
    """2500 rows cut at 700 and 1800: both cuts fall inside a 1024-row block of the column sums and inside a 256-row group
    of the cache; the middle slice is CSR and float32, the outer ones dense float64."""
    n, g = 2500, 17
    csr, mid = _csr_case(1100, g, "float32", seed=3)
    top, bottom = _matrix(700, g, "float64", seed=4), _matrix(700, g, "float64", seed=5)
    X = np.vstack([top, mid.astype(np.float64), bottom])
    one = Run(lib, n, g, cell)
    one.means(X)
    one.pack(X)
    mu, flat = one.host()
    cut = Run(lib, n, g, cell)
    cut.means(top, 0)
    cut.means_csr(csr, 100 * g * 4, 700)
    cut.means(bottom, 1800)
    cut.pack(top, 0)
    cut.pack_csr(csr, 100 * g * 4, 700)
    cut.pack(bottom, 1800)
    mu_c, flat_c = cut.host()
    assert np.array_equal(_bits(mu), _bits(mu_c)) and np.array_equal(_bits(flat), _bits(flat_c))
    exact = np.array([math.fsum(X[:, j].tolist()) for j in range(g)]) / n
    assert np.abs(mu - exact).max() <= n * pc.EPS * np.abs(X).max()
    assert np.array_equal(_bits(flat), _bits(_expected_cache(X, mu, cell)))


@pytest.mark.parametrize("cell,tol", [("float64", 1e-11), ("float32", 3e-6)])
@pytest.mark.parametrize("n,g", [(1, 1), (257, 17), (256, 128), (700, 129), (700, 200), (2500, 40)])
def test_gram_on_a_packed_cache(lib, n, g, cell, tol):
    from spateo_amd import _lib

    X = _matrix(n, g, "float64", seed=n * 31 + g)
    run = Run(lib, n, g, cell)
    run.means(X)
    run.pack(X)
    _, flat = run.host()
    Xc = pc.from_ublk(flat, n, g)[:n, :g].astype(np.float64)   # the operands as the device holds them
    ws_bytes = int(lib.mvf_gram_workspace_bytes(n, g, _cd(cell)))
    ws = _guarded(ws_bytes, torch.uint8)
    P = torch.ones(n, dtype=TD[cell], device=DEV)
    got = []
    for _ in range(2):
        G = _guarded(g * g)
        _check(lib, lib.mvf_gram_cached(_lib.GRAM_TILES | _lib.GRAM_REDUCE, run.ublk.data_ptr(), P.data_ptr(), P.data_ptr(), None, n,
                                        P.data_ptr(), g, 0.0, G.data_ptr(), None, ws.data_ptr(), ws_bytes, _cd(cell), _stream()),
               "mvf_gram_cached")
        torch.cuda.synchronize()
        assert _guard_ok(G, g * g) and _guard_ok(ws, ws_bytes)
        got.append(G[: g * g].cpu().numpy().reshape(g, g))
    ref = Xc.T @ Xc
    rel = float(np.abs(got[0] - ref).max() / max(np.abs(ref).max(), 1e-300))
    print(f"gram on a packed cache {n} x {g} {cell}: relmax {rel:.3e} (tol {tol:.0e})")
    assert np.array_equal(got[0], got[0].T) and np.array_equal(_bits(got[0]), _bits(got[1]))
    assert rel < tol
