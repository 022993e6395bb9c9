"""``spateo_amd.align.init_sigma2`` / ``init_probability_parameters`` / ``coarse_rigid_alignment`` / ``morpho_start`` on
``cuda:0`` against tests/golden/ref_align_start.npz: the real reference functions run on four cases
(tests/golden/make_golden_align_start.py), with the indices the reference drew, in both cell dtypes, per quantity relative
to the quantity's maximum.

* float64: ``max(1e-10, 1.25 g 1e-10)`` - 1e-10 is the assignment step's own bound (``_assign_case.F64_TOL``), g the
  amplification the maker measured on the reference with its perturbed twin;
* float32: 1.25 x the deviation of the reference's own float32-backend twin.

Both numbers are read from the npz.  The inlier pair sets must be equal.  One end-to-end case: the loops started from
``morpho_start`` on case 1 recover the rotation put in within the maker's 0.05 (Frobenius), ``morpho_iterate`` and
``morpho_iterate_svi`` alike."""
import numpy as np
import pytest

import _align_start_case as sc
import test_align_start_host as host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = sc.load()
TAGS = sc.case_tags(G)
_STARTS = {}


def _start(tag, dtype):
    if (tag, dtype) not in _STARTS:
        from spateo_amd import align

        _STARTS[(tag, dtype)] = host.start_of_case(align, sc.case_inputs(G, tag), dtype, device=DEV)
    return _STARTS[(tag, dtype)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tag", TAGS)
def test_start_state_against_the_reference(tag, dtype):
    st, got = _start(tag, dtype)
    sc.check(got, G, tag, sc.tolerances(G, tag, dtype), f"cuda {dtype}")
    assert (np.linalg.det(st.init_R) < 0) == bool(G[f"{tag}_flipped"])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("tag", ["2", "3"])
def test_the_stand_alone_functions_give_morpho_starts_numbers(tag, dtype):
    from spateo_amd import align

    c = sc.case_inputs(G, tag)
    st, _ = _start(tag, dtype)
    kw = dict(subsample_A=c["subsample_A"], subsample_B=c["subsample_B"], dtype=dtype, device=DEV)
    assert align.init_sigma2(st.coordsA, c["coordsB"], **kw) == st["sigma2"]                          # two calls: equal bits
    assert align.init_probability_parameters(c["layers_A"], c["layers_B"], dissimilarity=c["dissimilarity"],
                                             probability_type=c["probability_type"],
                                             probability_parameters=c["probability_parameters"], **kw) == st["probability_parameters"]
    # a draw of our own runs and is reproducible
    own = dict(subsample=150, seed=5, dtype=dtype, device=DEV)
    assert align.init_sigma2(st.coordsA, c["coordsB"], **own) == align.init_sigma2(st.coordsA, c["coordsB"], **own) > 0


@pytest.mark.parametrize("loop", ["morpho_iterate", "morpho_iterate_svi"])
def test_the_loops_start_from_morpho_start(loop):
    from spateo_amd import align

    c = sc.case_inputs(G, "1")
    st, _ = _start("1", "float64")
    extra = dict(batch_size=200, seed=0) if loop.endswith("svi") else {}
    out = getattr(align, loop)(st.coordsA, c["coordsB"], c["layers_A"], c["layers_B"], dissimilarity=c["dissimilarity"],
                               probability_type=c["probability_type"], beta=0.5, lambdaVF=100.0, max_iter=6, record=False,
                               dtype="float64", device=DEV, **extra, **st)
    err = np.linalg.norm(out["R"] @ st.init_R - c["R0"])
    print(f"  {loop} from morpho_start: |R init_R - R0| {err:.3g} (the coarse fit alone: {np.linalg.norm(st.init_R - c['R0']):.3g}), "
          f"sigma2 {st['sigma2']:.4g} -> {out['sigma2']:.4g}")
    assert err <= 0.05 and np.isfinite(out["XAHat"]).all()
