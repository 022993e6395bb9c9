#!/usr/bin/env python
"""Golden vectors for the reference-model route of the alignment (``st.align.trn`` / ``downsampling`` / ``morpho_align_ref`` and
friends), from the REAL reference code executed as it lies in the reference checkout - nothing of it is copied, the file holds
arrays only:

  * ``TRNET`` / ``trn(..., return_index=False)`` of ``spateo/alignment/methods/sampling.py`` (loaded by
    ``make_golden_sampling.load_reference_sampling``; only the progress logger is stubbed): the nodes ``W`` of ten cases and
    the three numbers NumPy's global generator gives next.  ``{tag}_repeat`` says whether the start draw holds a cell twice
    (then two nodes start identical and the reference's unstable ``argsort`` decides which is which).
  * ``solve_RT_by_correspondence`` of ``spateo/alignment/utils.py`` and the composition of
    ``morpho_align_apply_transformation`` of ``spateo/alignment/morpho_alignment.py`` on three tiny slices (loaded with the
    stubs ``make_golden.py`` installs; ``anndata`` is the ``AnnDataLite`` stand-in).
  * the ``tmax = 20`` series ``s{n}_*`` of tests/test_gpu_sample_kernels.py (n up to 4096, far beyond what the reference's
    nested loop finishes in): the float64 restatement of tests/_sample_cases.py - proved bit-equal to the real ``TRNET`` on the
    cases above by tests/test_sample_kernel_refs.py - and its deviation under a +-4 ulp perturbation of every exponential.

    python tests/golden/make_golden_downsampling.py      -> tests/golden/ref_downsampling.npz
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_sampling as mgs  # noqa: E402


def trn_cases():
    """tag -> (N, d, n, seed or None, kwargs)"""
    return {
        "a": (1500, 3, 48, 7, {}),
        "b": (3000, 2, 33, 3, {}),
        "c": (1500, 2, 48, None, {}),
        "d": (400, 3, 64, None, {}),
        "e": (200, 2, 40, None, {}),
        "f": (1200, 3, 40, 7, {"c": 0.001}),
        "g": (900, 2, 50, 11, {"tmax": 20}),
        "h": (300, 3, 1, None, {}),
        "i": (40, 2, 40, None, {}),
        "j": (800, 1, 24, 12345, {}),
    }


def coordinates(N, d):
    rng = np.random.default_rng(1000 * N + d)
    return rng.random((N, d)) * np.array([2000.0, 1200.0, 900.0][:d])   # uniform random: no lattice, no ties by construction


def load_alignment():
    """The real utils.py and morpho_alignment.py of the reference's alignment package."""
    mg.install_stubs()
    sys.modules["spateo.logging"].logger_manager.progress_logger = lambda it, **kw: it
    meth = sys.modules["spateo.alignment.methods"]
    meth.Morpho_pairwise, meth.empty_cache = None, None
    tr = types.ModuleType("spateo.alignment.transform")
    tr.BA_transform = None
    sys.modules["spateo.alignment.transform"] = tr
    ut = mg._load("spateo.alignment.utils", "spateo/alignment/utils.py")
    ma = mg._load("spateo.alignment.morpho_alignment", "spateo/alignment/morpho_alignment.py")
    return ut, ma


def main():
    import _sample_cases as sc

    sm = mgs.load_reference_sampling()
    sm.LoggerManager.progress_logger = staticmethod(lambda it, progress_name=None: it)
    out = {}
    for tag, (N, d, n, seed, kw) in trn_cases().items():
        X = coordinates(N, d)
        np.random.seed(4242)
        W = sm.trn(X, n, return_index=False, **kw) if seed is None else sm.trn(X, n, return_index=False, seed=seed, **kw)
        nxt = np.random.random(3)
        draw = np.random.RandomState(19491001 if seed is None else seed).randint(0, N, n)
        out[f"{tag}_X"], out[f"{tag}_n"], out[f"{tag}_seed"] = X, np.int64(n), np.int64(-1 if seed is None else seed)
        out[f"{tag}_tmax"], out[f"{tag}_c"] = np.float64(kw.get("tmax", 200)), np.float64(kw.get("c", 0))
        out[f"{tag}_W"], out[f"{tag}_next"] = np.asarray(W), nxt
        out[f"{tag}_repeat"] = np.bool_(len(np.unique(draw)) < n)
        print(tag, (N, d, n), "repeat in the start draw:", bool(out[f"{tag}_repeat"]))

    # solve_RT_by_correspondence and the composition, from the real alignment package
    sys.modules.pop("spateo.alignment.methods.utils", None)
    ut, ma = load_alignment()
    rng = np.random.default_rng(20261020)
    for tag, D, flip in (("rt2", 2, False), ("rt3", 3, False), ("rtf", 2, True)):
        Y = rng.standard_normal((60, D)) * 40
        Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
        if (np.linalg.det(Q) < 0) != flip:
            Q[:, 0] *= -1
        X = 1.3 * Y @ Q.T + rng.standard_normal(D) * 10 + 0.05 * rng.standard_normal((60, D))
        R, t, s = ut.solve_RT_by_correspondence(X, Y, return_scale=True)
        R2, t2 = ut.solve_RT_by_correspondence(X, Y)
        assert np.array_equal(R, R2) and np.array_equal(t, t2)
        out[f"{tag}_X"], out[f"{tag}_Y"], out[f"{tag}_R"], out[f"{tag}_t"], out[f"{tag}_s"] = X, Y, R, t, np.float64(s)
    slices = [mg.AnnDataLite(obsm={"spatial": rng.random((n, 2)) * 100}) for n in (7, 5, 9)]
    trans = []
    for i in range(2):
        a = rng.uniform(-1, 1)
        trans.append({"Rotation": np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]), "Translation": rng.standard_normal(2) * 20})
    for i, m in enumerate(slices):
        out[f"ap_spatial{i}"] = m.obsm["spatial"].copy()
    done = ma.morpho_align_apply_transformation(slices, transformation=trans)
    for i, m in enumerate(done):
        out[f"ap_aligned{i}"] = np.asarray(m.obsm["align_spatial"])
    for i, tr in enumerate(trans):
        out[f"ap_R{i}"], out[f"ap_t{i}"] = tr["Rotation"], tr["Translation"]

    # the tmax = 20 series of the kernel tests, from the restatement
    for n, (N, d) in sc.SERIES.items():
        X = sc.series_coordinates(n)
        W = sc.trn_restate(X, n, tmax=20)
        W4 = sc.trn_restate(X, n, tmax=20, jitter_ulp=4)
        out[f"s{n}_W"] = W
        out[f"s{n}_dev"] = np.float64(np.abs(W4 - W).max() / np.abs(X).max())
        print("series", n, (N, d), "4-ulp deviation / extent", out[f"s{n}_dev"])
    path = os.path.join(HERE, "ref_downsampling.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
