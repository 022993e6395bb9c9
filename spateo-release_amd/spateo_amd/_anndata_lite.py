"""Minimal AnnData stand-in.

The reference wrappers only touch ``.obsm``, ``.obs``, ``.uns``, ``.n_obs`` and ``.copy()`` of the AnnData object
(``sparsevfc.py:313-316``, ``differential_geometry.py:62-70,334-339``).  ``anndata`` is not installable in the build
image, so the wrappers duck-type their argument; a real ``anndata.AnnData`` works unchanged, and this class lets the
path run (and be tested) where ``anndata`` is absent.

The alignment (``spateo_amd.align.Morpho_pairwise``) also reads ``.X`` / ``.layers`` (dense or ``scipy.sparse``, kept as
handed in), ``.var_names``, the columns of ``.var`` (a dict of per-gene columns here) and categorical ``.obs`` columns
(anything with a pandas-style ``.cat`` accessor is kept as it is).
"""
from __future__ import annotations

import copy

import numpy as np


class _ObsFrame(dict):
    """dict of per-cell columns; assignment coerces to a 1-D NumPy array like ``DataFrame.__setitem__`` would."""

    def __setitem__(self, key, value):
        super().__setitem__(key, value if hasattr(value, "cat") else np.asarray(value))  # (a categorical keeps its categories)


def _is_sparse(m):
    return hasattr(m, "tocsr") and hasattr(m, "nnz")


def _matrix(m):
    """An expression matrix as stored: a scipy.sparse matrix stays sparse (np.asarray would wrap it in an object array)."""
    return m if _is_sparse(m) else np.asarray(m)


class AnnDataLite:
    def __init__(self, obsm=None, obs=None, uns=None, n_obs=None, X=None, var_names=None, layers=None, var=None):
        self.X = None if X is None else _matrix(X)
        self.var_names = list(var_names) if var_names is not None else (
            [str(i) for i in range(self.X.shape[1])] if self.X is not None else [])
        self.layers = {k: _matrix(v) for k, v in (layers or {}).items()}
        self.var = {k: np.asarray(v) for k, v in (var or {}).items()}     # per-gene columns, e.g. "highly_variable"
        self.obsm = dict(obsm or {})
        self.obs = _ObsFrame()
        for k, v in (obs or {}).items():
            self.obs[k] = v
        self.uns = dict(uns or {})
        if n_obs is None:
            n_obs = self.X.shape[0] if self.X is not None else (len(next(iter(self.obsm.values()))) if self.obsm else 0)
        self.n_obs = int(n_obs)

    def copy(self):
        return copy.deepcopy(self)

    def var_index(self, names):
        """Column positions of the genes ``names`` (in their order); ``KeyError`` names a gene that is not there."""
        where = {g: i for i, g in enumerate(self.var_names)}
        missing = [g for g in names if g not in where]
        if missing:
            raise KeyError(f"genes not in var_names: {missing[:5]}")
        return np.array([where[g] for g in names], dtype=np.int64)

    def select_vars(self, names):
        """A copy restricted to the genes ``names`` (``adata[:, names]``): ``X`` and every layer column-selected - a sparse
        matrix as CSR, in O(nnz) -, ``var`` and ``var_names`` with them; the per-cell fields are shared, not copied."""
        idx = self.var_index(names)
        take = lambda m: m.tocsr()[:, idx] if _is_sparse(m) else m[:, idx]  # noqa: E731
        new = AnnDataLite(obsm=self.obsm, uns=self.uns, n_obs=self.n_obs, X=None if self.X is None else take(self.X),
                          var_names=list(names), layers={k: take(v) for k, v in self.layers.items()},
                          var={k: v[idx] for k, v in self.var.items()})
        for k, v in self.obs.items():
            new.obs[k] = v
        return new

    def select_obs(self, idx):
        """A copy restricted to the cells ``idx`` (integer positions, in their order, repeats allowed: ``adata[idx, :]``):
        ``obs``, ``obsm``, ``X`` and every layer row-selected - a sparse matrix as CSR -, ``var``, ``var_names`` and ``uns``
        carried over (``uns`` copied, so the subset's results do not land in the parent)."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if len(idx) and (idx.min() < -self.n_obs or idx.max() >= self.n_obs):
            raise IndexError(f"cell positions must lie inside 0 .. {self.n_obs}")
        take = lambda m: m.tocsr()[idx] if _is_sparse(m) else m[idx]  # noqa: E731
        new = AnnDataLite(obsm={k: np.asarray(v)[idx] for k, v in self.obsm.items()}, uns=copy.deepcopy(self.uns), n_obs=len(idx),
                          X=None if self.X is None else take(self.X), var_names=list(self.var_names),
                          layers={k: take(v) for k, v in self.layers.items()}, var=dict(self.var))
        for k, v in self.obs.items():
            new.obs[k] = v.iloc[idx].reset_index(drop=True) if hasattr(v, "iloc") else v[idx]
        return new
