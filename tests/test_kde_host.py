"""Host-side tests of ``spateo_amd.tdr.morphometrics.morphology`` and the ``mvf_kde`` C ABI, without a device: validation and
every named refusal (before the kernels are bound), the exports, the kernel codes against the header, the no-launch paths of
the entry point, and ``pc_KDE`` / ``cell_density`` over a NumPy stand-in for the kernels (the restatement of tests/_kde_cases.py
behind ``HipKernels.kde``'s signature), which checks what the host adds: centring, constants, columns and written keys."""
import ctypes
import os
import re

import numpy as np
import pytest

import _kde_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mvf.h")


class KdeCpuKernels:
    """``HipKernels.kde`` on the CPU: centred host arrays in, unnormalised (n, C) log sums out."""

    def __init__(self, device=None, dtype="float64"):
        self.device, self.dtype_name, self.calls = device, dtype, []

    def kde(self, targets, sources, kernel, bandwidth, weight=None, group=None, C=1):
        self.calls.append(dict(targets=np.array(targets), sources=np.array(sources), kernel=kernel, C=C))
        T, X = kc.rounded(np.asarray(targets, dtype=np.float64), self.dtype_name), kc.rounded(np.asarray(sources, dtype=np.float64), self.dtype_name)
        return kc.raw_log_sums(T, X, kernel, float(bandwidth), weight, group, C)


@pytest.fixture
def seam(monkeypatch):
    from spateo_amd import _runtime as rt

    made = []
    monkeypatch.setattr(rt, "_make_kernels", lambda device, dtype: made.append(KdeCpuKernels(device, dtype)) or made[-1])
    monkeypatch.setattr(rt, "_shared_kernels", lambda device, dtype: rt._make_kernels(device, dtype))
    return made


@pytest.fixture
def no_kernels(monkeypatch):
    from spateo_amd import _runtime as rt

    def refuse(device, dtype):
        raise AssertionError("the kernels were bound before the arguments were refused")

    monkeypatch.setattr(rt, "_make_kernels", refuse)
    monkeypatch.setattr(rt, "_shared_kernels", refuse)


class Cloud:
    """What pc_KDE touches of a pyvista PolyData."""

    def __init__(self, points):
        self.points, self.point_data = np.array(points, dtype=np.float64), {}

    def copy(self):
        new = Cloud(self.points)
        new.point_data = dict(self.point_data)
        return new


# ---------------------------------------------------------------------------------------------------------- exports, codes
def test_exports():
    import spateo_amd as st
    from spateo_amd.tdr import morphometrics
    from spateo_amd.tdr.morphometrics import morphology

    assert set(morphology.__all__) == {"kernel_density", "pc_KDE", "cell_density"}
    for name in morphology.__all__:
        assert getattr(st.tdr, name) is getattr(morphology, name) is getattr(morphometrics, name)


def test_kernel_codes_match_the_header():
    from spateo_amd import _lib

    text = open(HEADER).read()
    assert list(_lib.KDE_KERNELS) == list(kc.KERNELS)
    for name, code in _lib.KDE_KERNELS.items():
        assert int(re.search(rf"MVF_KDE_{name.upper()} = (\d+)", text).group(1)) == code == kc.CODES[name]
    assert int(re.search(r"#define MVF_KDE_MAX_COLUMNS (\d+)", text).group(1)) == _lib.KDE_MAX_COLUMNS == kc.MAX_COLUMNS
    assert text.count("morphology.py:109") >= 2 and {"mvf_kde", "mvf_kde_workspace_bytes"} <= set(_lib.SIGNATURES)


# ------------------------------------------------------------------------------------------------- C ABI without a launch
def test_entry_point_refuses_and_returns_without_launching():
    from spateo_amd import _lib

    lib = _lib.load()
    assert lib.mvf_version() == 7
    p = ctypes.c_void_p(8)     # never dereferenced: every call below returns before a launch

    def call(t4=p, n=100, s4=p, N=50, d=3, kernel=0, h=0.5, C=1, out=p, ws=p, ws_bytes=1 << 30, dtype=_lib.MVF_F64):
        return lib.mvf_kde(t4, n, s4, N, d, kernel, h, None, None, C, out, ws, ws_bytes, dtype, None)

    assert call(n=0) == 0 and call(C=0) == 0 and call(n=0, t4=None, out=None) == 0
    for kw, msg in ((dict(d=0), b"bad shape"), (dict(d=4), b"bad shape"), (dict(n=-1), b"bad shape"), (dict(N=-1), b"bad shape"),
                    (dict(C=-1), b"bad shape"), (dict(C=65), b"bad shape"), (dict(h=0.0), b"bad shape"), (dict(h=-1.0), b"bad shape"),
                    (dict(h=float("inf")), b"bad shape"), (dict(kernel=6), b"bad kernel"), (dict(kernel=-1), b"bad kernel"),
                    (dict(dtype=2), b"bad dtype"), (dict(t4=None), b"null pointer"), (dict(s4=None), b"null pointer"),
                    (dict(out=None), b"null pointer"), (dict(ws=None), b"null pointer"), (dict(ws_bytes=8), b"workspace too small")):
        assert call(**kw) != 0, kw
        assert b"mvf_kde" in lib.mvf_last_error() and msg in lib.mvf_last_error(), (kw, lib.mvf_last_error())
    with pytest.raises(_lib.MVFError, match="bad kernel"):
        _lib.check(call(kernel=9), "mvf_kde")


def test_workspace_bytes():
    from spateo_amd import _lib

    lib = _lib.load()
    for n, N, C in ((1, 1, 1), (300, 4096, 1), (300, 4097, 1), (300, 12290, 64), (100_000, 100_000, 20), (1_000_000, 1_000_000, 1)):
        assert lib.mvf_kde_workspace_bytes(n, N, C) == (kc.splits(n, N) + 1) * n * C * 8
    assert kc.splits(1_000_000, 1_000_000) == 1 and kc.splits(300, 1_000_000) == 245
    for n, N, C in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, 65), (-1, 5, 1)):
        assert lib.mvf_kde_workspace_bytes(n, N, C) == 0


# ------------------------------------------------------------------------------------------------------------- validation
def test_refusals_come_before_the_kernels(no_kernels):
    import scipy.sparse as sp

    from spateo_amd.tdr import kernel_density

    X = np.random.default_rng(0).random((20, 3))
    with pytest.raises(NotImplementedError, match="1 <= d <= 3"):
        kernel_density(np.zeros((5, 4)))
    with pytest.raises(NotImplementedError, match="1 <= d <= 3"):
        kernel_density(X, targets=np.zeros((5, 4)))
    with pytest.raises(NotImplementedError, match="sparse"):
        kernel_density(sp.csr_matrix(X))
    with pytest.raises(NotImplementedError, match="scott"):
        kernel_density(X, bandwidth="scott")
    with pytest.raises(ValueError, match="gaussian.*exponential.*tophat.*epanechnikov.*linear.*cosine"):
        kernel_density(X, kernel="triangle")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bandwidth"):
            kernel_density(X, bandwidth=bad)
    for w in (-np.ones(20), np.full(20, np.nan), np.full(20, np.inf), np.ones(19), np.ones((20, 1)), np.full(20, 1e-310)):
        with pytest.raises(ValueError, match="sample_weight"):
            kernel_density(X, sample_weight=w)
    with pytest.raises(ValueError, match="sum of the weights"):
        kernel_density(X, sample_weight=np.full(20, 1e308))
    for g in (-np.ones(20, dtype=int), np.full(20, 0.5), np.zeros(19, dtype=int), np.zeros((20, 1), dtype=int), np.array(["a"] * 20),
              np.zeros(20, dtype=bool)):
        with pytest.raises(ValueError, match="groups"):
            kernel_density(X, groups=g)
    with pytest.raises(ValueError, match="targets"):
        kernel_density(X, targets=np.zeros((5, 2)))
    with pytest.raises(ValueError, match="non-finite"):
        kernel_density(np.full((3, 3), np.nan))
    with pytest.raises(ValueError, match="empty"):
        kernel_density(np.zeros((0, 3)))
    with pytest.raises(ValueError, match="dtype"):
        kernel_density(X, dtype="float16")
    assert kernel_density(X, targets=np.zeros((0, 3))).shape == (0,)
    assert kernel_density(X, targets=np.zeros((0, 3)), groups=np.arange(20) % 3).shape == (0, 3)


# ------------------------------------------------------------------------------------------------------- what the host adds
@pytest.mark.parametrize("name", ("gaussian_d3", "cosine_d2", "C17_gauss", "wide_epan"))
def test_kernel_density_adds_sklearns_constants(seam, name):
    from spateo_amd.tdr import kernel_density

    G, case = kc.load(), kc.CASES[name]
    offset = np.array([1000.0, -50.0, 3.0])[: case["d"]]      # the host centres: an offset of the cloud changes nothing visible
    got = kernel_density(case["X"] + offset, case["T"] + offset, kernel=case["kernel"], bandwidth=case["h"], sample_weight=case["w"],
                         groups=case["g"])
    score = G[f"{name}_score"] if name in kc.GOLDEN_FULL else kc.log_density(case)
    assert got.shape == ((len(case["T"]),) if case["g"] is None else (len(case["T"]), case["C"]))
    got = got.reshape(score.shape)
    assert np.array_equal(np.isfinite(got), np.isfinite(score))
    fin = np.isfinite(score)
    if name not in kc.TIGHT:                          # (on the wide weights sklearn itself is units off: _kde_cases.TIGHT)
        assert np.abs(got[fin] - score[fin]).max() < 1e-9
    ref = kc.log_density(case)
    assert np.abs(got[fin] - ref[fin]).max() < 1e-9
    call = seam[-1].calls[-1]
    assert np.abs(call["sources"].mean(axis=0)).max() < 1e-5 and call["C"] == case["C"]      # centred by (nearly) the source mean


def test_centre_is_exact_on_grid_coordinates():
    from spateo_amd.tdr.morphometrics.morphology import _centre

    rng = np.random.default_rng(3)
    X = rng.integers(0, 1 << 14, (500, 3)) / 1024.0 + 4096.0          # coordinates on a 2^-10 grid
    for sub in (X, X[:37], X[::5]):
        c = _centre(sub)
        assert np.abs(c - sub.mean(axis=0)).max() <= np.ptp(sub, axis=0).max() * 2.0 ** -20
        assert np.array_equal((X - c) - (X[:1] - c), X - X[:1])      # differences survive the centring bit for bit
    assert np.array_equal(_centre(np.ones((4, 3))), np.ones(3))


def test_pc_kde_on_a_stand_in_object(seam):
    from spateo_amd.tdr import pc_KDE

    case = kc.CASES["gaussian_d3"]
    pc = Cloud(case["X"] + 7.0)
    out, cmap = pc_KDE(pc, key_added="dens", kernel="gaussian", bandwidth=case["h"], colormap="viridis")
    assert out is not pc and cmap == "viridis" and "dens" not in pc.point_data
    want = kc.log_density(dict(case, T=case["X"]))[:, 0]
    assert out.point_data["dens"].shape == (300,) and np.abs(out.point_data["dens"] - want).max() < 1e-9
    none, cmap = pc_KDE(pc, bandwidth=case["h"], inplace=True)
    assert none is None and cmap == "hot_r" and np.array_equal(pc.point_data["kde"], out.point_data["dens"])
    import sys

    assert "pyvista" not in sys.modules


def test_cell_density_written_keys(seam):
    import pandas as pd

    from spateo_amd import AnnDataLite
    from spateo_amd.tdr import cell_density

    case = kc.CASES["C17_gauss"]
    labels = pd.Categorical.from_codes(case["g"] % 3, categories=["a", "b", "c", "unused"])
    adata = AnnDataLite(obsm={"spatial": case["X"]}, obs={"type": pd.Series(labels)})
    assert cell_density(adata, bandwidth=0.2) is None
    assert adata.obs["kde"].shape == (700,) and "kde" not in adata.obsm
    assert cell_density(adata, group_key="type", key_added="dens", bandwidth=0.2, kernel="epanechnikov") is None
    assert adata.obsm["dens"].shape == (700, 4) and np.isneginf(adata.obsm["dens"][:, 3]).all()
    assert adata.uns["dens"] == {"categories": ["a", "b", "c", "unused"], "group_key": "type"}
    want = kc.log_density(dict(case, T=case["X"], g=case["g"] % 3, C=3, w=None, kernel="epanechnikov", h=0.2))
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(adata.obsm["dens"][:, :3]), fin) and np.abs(adata.obsm["dens"][:, :3][fin] - want[fin]).max() < 1e-9
    with pytest.raises(ValueError, match="categorical"):
        cell_density(adata, group_key="kde")
    with pytest.raises(KeyError):
        cell_density(adata, spatial_key="nope")
    with pytest.raises(TypeError):
        cell_density(adata, groups=np.zeros(700, dtype=int))
