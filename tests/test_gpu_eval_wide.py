"""``st.tdr.kernel_interpolation(return_model=True)`` / ``kernel_interpolation_predict`` / ``vector_field_function`` on a field of
21 output columns (20 genes + 1 obs key) in 3-D and in 2-D, on the real kernels (mvf_eval_wide), both cell dtypes: predict at the
fit's own targets gives the fit's output, predict and its gradient at new points match the oracle evaluated on the returned
model, and the public evaluator functions no longer refuse such a field.  Tolerance: _cell_cases.TOL of each quantity's maximum."""
import numpy as np
import pytest

import spateo_amd as st
from oracle import dg_oracle as dgo
from oracle import sparsevfc_oracle as svo

from _cell_cases import TOL, relmax

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
_FITS = {}


def _fit(d, dtype):
    """One fit per (d, dtype), shared by the tests below (nothing modifies it)."""
    if (d, dtype) not in _FITS:
        rng = np.random.default_rng(11 + d)
        n, ng = 3000, 20
        S = rng.uniform(-1, 1, (n, d)) * 50
        z = S[:, d - 1]
        genes = np.column_stack([np.sin(S[:, 0] / (14 + g)) * np.cos(z / (11 + 2 * g)) + 0.1 * g for g in range(ng)])
        genes += 0.01 * rng.standard_normal(genes.shape)
        names = [f"g{g}" for g in range(ng)]
        ad = st.AnnDataLite(X=genes, var_names=names, obs={"score": np.cos(z / 25)}, obsm={"spatial": S})
        tgt = rng.uniform(-1, 1, (300, d)) * 45
        new = rng.uniform(-1, 1, (257, d)) * 45
        out, model = st.tdr.kernel_interpolation(ad, target_points=tgt, keys=["score"] + names, lambda_=3.0, M=50, MaxIter=10,
                                                 seed=0, dtype=dtype, return_model=True)
        _FITS[(d, dtype)] = (out, model, tgt, new, names)
    return _FITS[(d, dtype)]


def _table(ad):
    return np.column_stack([np.asarray(ad.obs["score"], dtype=float), np.asarray(ad.X)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [3, 2])
def test_predict_at_the_fits_targets_gives_the_fits_output(d, dtype):
    out, model, tgt, _, names = _fit(d, dtype)
    assert model["C"].shape == (50, 21) and model["obs_keys"] == ["score"] and model["var_keys"] == names
    again = st.tdr.kernel_interpolation_predict(model, tgt, dtype=dtype)
    assert list(again.var_names) == names and np.array_equal(np.asarray(again.obsm["spatial"]), tgt)
    e = relmax(_table(again), _table(out))
    print(f"predict vs fit d={d} {dtype}: {e:.2e}")
    assert e <= TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [3, 2])
def test_predict_and_gradient_at_new_points_match_the_oracle(d, dtype):
    _, model, _, new, names = _fit(d, dtype)
    got = st.tdr.kernel_interpolation_predict(model, new, gradient=True, dtype=dtype)
    v = svo.vector_field_function(new, model)
    J = dgo.Jacobian_rkhs_gaussian(new, model, vectorize=True)  # (21, d, 257)
    assert _table(got).shape == (257, 21) and J.shape == (21, d, 257)
    ev = relmax(_table(got), v)
    grad = np.stack([np.column_stack([np.asarray(got.obs[f"score_grad_{i}"], dtype=float), got.layers[f"grad_{i}"]]).T
                     for i in range(d)], axis=1)  # (21, d, 257)
    ej = relmax(grad, J)
    print(f"predict vs oracle d={d} {dtype}: v={ev:.2e} grad={ej:.2e}")
    assert ev <= TOL[dtype] and ej <= TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_public_evaluators_take_the_wide_field(dtype):
    _, model, _, new, _ = _fit(3, dtype)
    v = st.vector_field_function(new, model, dtype=dtype)  # NotImplementedError before mvf_eval_wide
    assert v.shape == (257, 21) and relmax(v, svo.vector_field_function(new, model)) <= TOL[dtype]
    ad = st.AnnDataLite(obsm={"X": new}, uns={"VecFld": model})
    f = st.SvcVectorField(dtype=dtype).from_adata(ad)
    J = f.get_Jacobian()(new)
    assert J.shape == (21, 3, 257) and relmax(J, dgo.Jacobian_rkhs_gaussian(new, model, vectorize=True)) <= TOL[dtype]
    assert f.get_Jacobian()(new[0]).shape == (21, 3)
    with pytest.raises(ValueError, match="as many output columns as dimensions"):
        f.compute_divergence(new)
