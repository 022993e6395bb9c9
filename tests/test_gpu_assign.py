"""GPU tests of the alignment's assignment step, through ``spateo_amd.align.update_assignment`` -> the C ABI
(``mvf_assign_prepare`` / ``mvf_assign`` / ``mvf_assign_dense``), both cell dtypes, against goldens of the real
``Morpho_pairwise._update_assignment_P`` (tests/golden/make_golden_assign.py).

Bounds, relative to each quantity's maximum (tests/_assign_case.py): float64 1e-10 (exponent arguments up to ~700 carry a
few ulps, i.e. <= ~1e-12 per positive term; the bound _align_case holds SigmaInv to); float32 max(1.25 x the reference's
own float32-vs-float64 floor of that quantity, 1e-5).  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import _assign_case as ac

pytestmark = pytest.mark.gpu

DTYPES = ("float64", "float32")


@pytest.fixture(scope="module")
def g():
    return ac.load()


@pytest.fixture(scope="module")
def st():
    import spateo_amd

    return spateo_amd


def _run(st, g, tag, dtype, **extra):
    args, kw = ac.case_inputs(g, tag)
    return st.align.update_assignment(*args, dtype=dtype, device="cuda:0", **kw, **extra)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_golden_case_every_quantity(st, g, dtype):
    worst = 0.0
    for tag in ac.case_tags(g):
        got = _run(st, g, tag, dtype)
        tols = ac.tolerances(g, tag, dtype)
        worst = max(worst, ac.check(got, ac.golden_ref(g, tag), tols, f"case {tag} {dtype}"))
        if dtype == "float32":
            floor = dict(zip(ac.QUANTITIES, g[f"{tag}_floor_f32"]))
            dev = ac.deviations(got, ac.golden_ref(g, tag))
            print(f"    worst ratio to the reference's float32 floor: {max(dev[q] / floor[q] for q in ac.QUANTITIES):.2f}")
    print(f"  {dtype}: worst deviation / bound over all cases {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_underflowing_columns_give_exact_zeros_and_no_nan(st, g, dtype):
    for tag in ("a", "p"):
        got = _run(st, g, tag, dtype, return_P=True)
        far = g[f"{tag}_far"]
        assert len(far) >= 0.05 * len(got["K_NB"])
        assert np.all(got["K_NB"][far] == 0.0) and np.all(got["P"][:, far] == 0.0)
        for q, v in got.items():
            assert np.isfinite(v).all(), (tag, q)
        live = np.setdiff1d(np.arange(len(got["K_NB"])), far)
        assert np.all(got["K_NB"][live] > 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_P_against_the_golden(st, g, dtype):
    got = _run(st, g, "p", dtype, return_P=True)
    P = g["p_P"]
    assert got["P"].shape == P.shape and got["P"].dtype == np.float64
    err = float(np.abs(got["P"] - P).max() / P.max())
    tol = ac.F64_TOL if dtype == "float64" else max(ac.ALLOW * float(g["p_floor_f32"].max()), ac.F32_BASE)
    print(f"  dense P {dtype}: {err:.2e} (bound {tol:.2e})")
    assert err <= tol
    # ... and it is the P the fused outputs belong to
    assert np.abs(got["P"].sum(1) - got["K_NA"]).max() <= 1e-12 * got["K_NA"].max()
    assert np.abs(got["P"].sum(0) - got["K_NB"]).max() <= 1e-12 * got["K_NB"].max()
    stored = g["p_coordsB"].astype(dtype).astype(np.float64)  # the coordinates as the cell dtype holds them
    assert np.abs(got["P"] @ stored - got["PXB"]).max() <= 1e-12 * np.abs(got["PXB"]).max()
    # the dense variant returns the same bits as the fused one
    plain = _run(st, g, "p", dtype)
    for q in ac.QUANTITIES:
        assert np.array_equal(plain[q], got[q]), q


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_are_bit_identical(st, g, dtype):
    for tag in ("b", "c"):
        r1, r2 = _run(st, g, tag, dtype), _run(st, g, tag, dtype)
        for q in ac.QUANTITIES:
            assert np.array_equal(r1[q], r2[q]), (tag, q)


def _large_case():
    """NA = 20 011, NB = 15 013, two layers (kl on 40 count-like features + cos on 24): 313 x 235 tiles, i.e. several
    workgroups per row / column panel and the split reduction; 6 % of the B cells out of reach of every A cell."""
    rng = np.random.default_rng(20261018)
    NA, NB, D = 20011, 15013, 3
    XA = rng.standard_normal((NA, D))
    src = rng.choice(NA, NB)
    XB = XA[src] + 0.15 * rng.standard_normal((NB, D))
    sigma2 = 0.05  # as the golden case the float32 floor is taken from
    far = np.sort(rng.choice(NB, 900, replace=False))
    XB[far, 0] += np.sqrt(2 * sigma2 * 800.0) + 2 * np.abs(XA).max() * np.sqrt(D)
    lab = rng.integers(0, 6, NA)
    prof, cent = rng.gamma(0.6, 4.0, (6, 40)), rng.standard_normal((6, 24)) * 1.5
    layers_A = [rng.poisson(prof[lab]).astype(np.float64), cent[lab] + 0.7 * rng.standard_normal((NA, 24))]
    layers_B = [rng.poisson(prof[lab[src]]).astype(np.float64), cent[lab[src]] + 0.7 * rng.standard_normal((NB, 24))]
    kw = dict(dissimilarity=["kl", "cos"], probability_type=["gauss", "cos"], probability_parameters=[0.05, None],
              sigma2=sigma2, alpha=rng.uniform(0.5, 1.0, NA), SigmaDiag=sigma2 * rng.uniform(0.0, 0.3, NA), gamma=0.5,
              samples_s=float(np.prod(XA.max(0) - XA.min(0))), sigma2_variance=1.0)
    return (XA, XB, layers_A, layers_B), kw, far


@pytest.fixture(scope="module")
def large():
    args, kw, far = _large_case()
    return args, kw, far, ac.restatement(*args, chunk=512, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_size_no_golden_holds_against_the_chunked_restatement(st, g, large, dtype):
    args, kw, far, ref = large
    got = st.align.update_assignment(*args, dtype=dtype, device="cuda:0", **kw)
    tols = ac.tolerances(g, "b", dtype)  # the float32 floor of the nearest golden case (kl + cos)
    ac.check(got, ref, tols, f"20011 x 15013 {dtype}")
    assert np.all(got["K_NB"][far] == 0.0)
    again = st.align.update_assignment(*args, dtype=dtype, device="cuda:0", **kw)
    for q in ac.QUANTITIES:
        assert np.array_equal(got[q], again[q]), q


@pytest.mark.parametrize("dtype", DTYPES)
def test_composition_with_update_nonrigid(st, g, dtype):
    """update_assignment -> PXB - RnA K_NA -> update_nonrigid against the real _update_assignment_P + _update_nonrigid, at
    the bounds _align_case.check_update_nonrigid holds its well-conditioned case to."""
    got = _run(st, g, "e", dtype)
    PXB_term = got["PXB"] - g["e_nr_RnA"] * got["K_NA"][:, None]
    r = st.align.update_nonrigid(g["e_XAHat"], g["e_nr_inducing_variables"], float(g["e_nr_beta"]), got["K_NA"], PXB_term,
                                 float(g["e_sigma2"]), float(g["e_nr_lambdaVF"]), dtype=dtype, device="cuda:0")
    tol = {"float64": (1e-8, 1e-8, 1e-8), "float32": (2e-3, 1e-3, 2e-3)}[dtype]
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())  # noqa: E731
    errs = [rel(r[q], g[f"e_nr_{q}"]) for q in ("Coff", "VnA", "SigmaDiag")]
    print(f"  composition {dtype}: Coff {errs[0]:.2e}, VnA {errs[1]:.2e}, SigmaDiag {errs[2]:.2e}; "
          f"PXB_term {rel(PXB_term, g['e_nr_PXB_term']):.2e}")
    for e, t, q in zip(errs, tol, ("Coff", "VnA", "SigmaDiag")):
        assert e < t, (q, e, t)
