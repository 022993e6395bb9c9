"""No GPU: the references and the input designs of tests/test_gpu_cell_kernels.py, on exactly the inputs that module runs
(tests/_cell_cases.py builds them for both).

  * the float64 restatements of tests/_cpu_kernels.py (CpuKernels.eval / .integrate / .estep_* / .quadform / .sym_* /
    .lincomb3) against 80-bit np.longdouble evaluations: <= 1e-12 of each quantity's maximum, two digits below the tightest
    tolerance the GPU module asserts against them (1e-10);
  * conditioning: |v| and |a| bounded away from 0 relative to their maxima and no query whose curvature / torsion towers over
    the rest, so that a max-norm relative error over ALL queries is meaningful and nothing has to be masked;
  * mutation sensitivity: a reference built with the off-by-one a case exists to catch (last control point dropped, last
    point of the first staging chunk dropped, last query repeating its neighbour, t2 with dy = 3, the zero-fill left at 0)
    differs from the true one by >= 1000 x the tolerance the GPU module asserts - in float32 mode, the wider of the two.  For
    the evaluator the eight outputs are compared in one test, so the condition is on the output that moves most (v and J;
    torsion's tolerance of 2e-3 x 1000 exceeds any possible relative deviation);
  * the derived bound of the E-step sums: a float64 sum in the kernel's blocked order lies within 1e-12 of math.fsum."""
import math

import numpy as np
import pytest
import torch

import _cell_cases as cc
from _cpu_kernels import CpuKernels

L = np.longdouble
REF_TOL = 1e-12


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _cpu_eval(case, flags=cc.EVAL_ALL):
    k = CpuKernels()
    out = k.eval(k.to_x4(case["X"]), k.to_x4(case["ctrl"]), case["beta"], _t(case["C"]), flags, affine=case["affine"])
    return {f: o.numpy() for f, o in out.items()}


@pytest.mark.parametrize("family,n,m", cc.EVAL_CASES)
def test_evaluator_restatement_conditioning_and_mutations(family, n, m):
    case = cc.eval_case(n, m, family)
    ref = _cpu_eval(case)
    assert set(ref) == set(cc.EVAL_FLAGS)
    hp = cc.eval_reference(L, case["X"], case["ctrl"], case["C"], case["beta"], case["affine"])
    for f, e in cc.eval_errors(ref, hp).items():
        assert e <= REF_TOL, (cc.EVAL_NAMES[f], e)
    # the module's own pair-by-pair float64 form (what the mutated references below are built with) is the restatement
    own = cc.eval_reference(np.float64, case["X"], case["ctrl"], case["C"], case["beta"], case["affine"])
    for f, e in cc.eval_errors(own, ref).items():
        assert e <= REF_TOL, (cc.EVAL_NAMES[f], e)
    vn, an = np.linalg.norm(ref[cc.EVAL_V], axis=1), np.linalg.norm(ref[cc.EVAL_ACC], axis=1)
    assert vn.min() / vn.max() >= 0.03
    assert an.min() / an.max() >= 5e-3
    for f in (cc.EVAL_CURV, cc.EVAL_TORS):
        qn = np.linalg.norm(ref[f], axis=1)
        assert np.isfinite(qn).all() and qn.max() <= 20 * np.median(qn), cc.EVAL_NAMES[f]
    muts = {name: cc.eval_reference(np.float64, mc["X"], mc["ctrl"], mc["C"], mc["beta"], mc["affine"])
            for name, mc in cc.eval_mutations(case).items()}
    if n >= 2:
        muts["dup_last_query"] = cc.dup_last_query(ref)
    assert ("drop_last_ctrl" in muts) and (("drop_chunk_end" in muts) == (m > 256))
    for name, mut in muts.items():
        moved = max(e / cc.eval_tol("float32", f) for f, e in cc.eval_errors(mut, ref).items())
        assert moved >= cc.MUTATION_FACTOR, (name, moved)


def test_evaluator_sweep_covers_what_it_claims():
    assert {n for n, _ in cc.EVAL_SWEEP} == set(cc.EVAL_NS) and {m for _, m in cc.EVAL_SWEEP} == set(cc.EVAL_MS)
    for n in cc.EVAL_NS:
        assert sum(1 for a, _ in cc.EVAL_SWEEP if a == n) >= 2
    for m in cc.EVAL_MS:
        assert sum(1 for _, b in cc.EVAL_SWEEP if b == m) >= 2
    assert any(m % 4 and m > 256 for _, m in cc.EVAL_SWEEP)


def test_evaluator_restatement_without_control_points():
    case = cc.eval_case_empty(17, "affine")
    flags = cc.EVAL_V | cc.EVAL_JAC | cc.EVAL_DIV | cc.EVAL_CURL | cc.EVAL_JDET
    out = _cpu_eval(case, flags)
    _, _, A, b = case["affine"]
    np.testing.assert_array_equal(out[cc.EVAL_V], case["X"] @ A.T + b)  # exact: dyadic inputs
    assert np.array_equal(case["X"], case["X"].astype(np.float32)) and not _cpu_eval(cc.eval_case_empty(5), flags)[cc.EVAL_V].any()
    assert not out[cc.EVAL_JAC].any() and not out[cc.EVAL_JDET].any() and out[cc.EVAL_JAC].shape == (3, 3, 17)
    k = CpuKernels()
    tr = k.integrate(k.to_x4(case["X"]), k.to_x4(case["ctrl"]), cc.BETA, _t(case["C"]), 0.5, 2, 3,
                     affine=(1.0, 1.0, np.zeros((3, 3)), b)).numpy()
    np.testing.assert_allclose(tr[:, 2], case["X"] + b, rtol=1e-14)  # a constant field: straight lines


# ------------------------------------------------------------------------------------------------------ RK4
def _sub(n):
    """The start points the expensive checks run on: the first and the last 32 (trajectories are independent of each other)."""
    return np.unique(np.r_[np.arange(min(n, 32)), np.arange(max(0, n - 32), n)])


@pytest.mark.parametrize("n,m,affine", [(n, m, False) for n, m in cc.RK4_SHAPES] + [cc.RK4_AFFINE_SHAPE + (True,)])
def test_rk4_restatement_and_mutations(n, m, affine):
    case = cc.rk4_case(n, m, affine)
    assert np.array_equal(case["X"], case["X"].astype(np.float32)) and np.array_equal(case["ctrl"], case["ctrl"].astype(np.float32))
    X = case["X"][_sub(n)]
    k = CpuKernels()
    args = (case["beta"], cc.RK4_DT, cc.RK4_SUBSTEPS, cc.RK4_NOUT)
    ref = k.integrate(k.to_x4(X), k.to_x4(case["ctrl"]), case["beta"], _t(case["C"]), *args[1:], affine=case["affine"]).numpy()
    hp = cc.rk4_reference(L, X, case["ctrl"], case["C"], *args, affine=case["affine"])
    ext = cc.extent(ref)
    assert 1.0 < ext < 15.0  # short trajectories: a few units inside a +-30 cloud
    assert np.abs(ref - hp).max() / ext <= REF_TOL
    muts = {name: cc.rk4_reference(np.float64, X, mc["ctrl"], mc["C"], *args, affine=mc["affine"])
            for name, mc in cc.rk4_mutations(case).items()}
    if n >= 2:
        dup = ref.copy()
        dup[-1] = dup[-2]
        muts["dup_last_start"] = dup
    for dtype, cap in cc.RK4_CAP.items():
        assert (f"drop_chunk_end_{dtype}" in muts) == (m > cap) == (cc.rk4_chunks(m, dtype) > 1)
    for name, mut in muts.items():
        moved = np.abs(mut - ref).max() / ext / cc.TOL["float32"]
        assert moved >= cc.MUTATION_FACTOR, (name, moved)


def test_rk4_shapes_cover_what_they_claim():
    assert cc.RK4_CAP == {"float32": 3072, "float64": 2304}
    assert {m for _, m in cc.RK4_SHAPES} == set(cc.RK4_MS) and {n for n, _ in cc.RK4_SHAPES} == set(cc.RK4_NS)
    assert max(cc.rk4_chunks(m, "float64") for m in cc.RK4_MS) == 3 and max(cc.rk4_chunks(m, "float32") for m in cc.RK4_MS) == 3
    for dtype, cap in cc.RK4_CAP.items():
        assert {cap - 1, cap, cap + 1} <= set(cc.RK4_MS)


# ------------------------------------------------------------------------------------------------------ E-step
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,kind,dy,gamma", [c for c in cc.ESTEP_CASES if c[0] <= 5000])
def test_estep_reference_is_the_restatement_and_the_design_is_sensitive(n, kind, dy, gamma, dtype):
    r = cc.estep_residuals(n, kind, dtype)
    s2, a, minP = cc.ESTEP_SIGMA2, cc.ESTEP_A, cc.ESTEP_MINP
    ref = cc.estep_reference(r, s2, gamma, a, dy, minP, dtype)
    theta, dist = cc.pick_theta(ref["stored"])
    assert dist >= 1e-6 and abs(ref["pf"] - theta).min() >= 1e-6
    # families are what they say
    x = r / (2 * s2)
    assert not ((x > 700) & (x < 800)).any()
    if kind == "all":
        assert (x > 800).all() and ref["mins"] == (np.inf, float(n))
    if kind == "one":
        assert ref["nzero"] == n - 1 and ref["mins"][0] == math.exp(-r[n // 2] / (2 * s2))
    if kind == "none":
        assert ref["nzero"] == 0
    if kind == "mixed" and n >= 255:
        assert 0 < ref["nzero"] < n
    # CpuKernels.estep_min / estep_p state the same thing
    k = CpuKernels()
    mins = k.estep_min(_t(r), s2).numpy()
    assert mins[0] == ref["mins"][0] and mins[1] == ref["mins"][1]
    P, st = torch.empty(n, dtype=torch.float64), torch.zeros(5, dtype=torch.float64)
    k.estep_p(_t(r), s2, gamma, a, dy, minP, theta, torch.tensor([mins[0]]), P, st)
    np.testing.assert_array_equal(P.numpy(), ref["pf"])
    np.testing.assert_allclose(st.numpy()[:2], ref["sums"][:2], rtol=1e-13)
    np.testing.assert_allclose(st.numpy()[2], math.fsum(ref["pf"]), rtol=1e-13)
    assert st[3] == (ref["pf"] > theta).sum() == (ref["stored"] > theta).sum() and st[4] == ref["nzero"]
    # mutations: >= 1000 x the asserted tolerance (P: 1 float32 ulp ~ 1.2e-7 relative, sums: 1e-12)
    ulp = float(np.finfo(np.float32).eps)

    def moved(mut):
        with np.errstate(invalid="ignore", divide="ignore"):
            dp = np.nanmax(np.abs(mut["stored"] - ref["stored"]) / ref["stored"]) / ulp
            ds = max(abs(x - y) / abs(y) for x, y in zip(mut["sums"], ref["sums"]) if y) / cc.ESTEP_SUM_RTOL
        return max(dp, ds)

    if dy != 3:
        assert moved(cc.estep_reference(r, s2, gamma, a, 3, minP, dtype)) >= cc.MUTATION_FACTOR
    if ref["nzero"] and np.isfinite(ref["mins"][0]):
        assert moved(cc.estep_reference(r, s2, gamma, a, dy, minP, dtype, zero_fill=0.0)) >= cc.MUTATION_FACTOR


def test_estep_cases_cover_what_they_claim():
    assert {c[0] for c in cc.ESTEP_CASES} == set(cc.ESTEP_NS)
    assert {(c[2], c[3]) for c in cc.ESTEP_CASES} >= {(dy, g) for dy in cc.ESTEP_DYS for g in cc.ESTEP_GAMMAS}
    assert {c[1] for c in cc.ESTEP_CASES} == {"mixed", "all", "none", "one"}
    big = cc.ESTEP_NS[-1]
    assert big > 2048 * 1024 and cc.estep_blocks(big) == 2048 and -(-big // (2048 * 256)) == 5  # lanes take 4 or 5 cells
    assert (big, "all", 5, 0.5) in cc.ESTEP_CASES


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_estep_blocked_sum_is_within_the_derived_bound(dtype):
    """>= 0 summands, at most ceil(n / (nb 256)) sequential additions per lane, log2(256) + log2(2048) tree levels and 8 more
    sequential additions: every partial sum carries a relative error below ~30 x 2^-53 = 3.3e-15; 1e-12 leaves two digits."""
    n = cc.ESTEP_NS[-1]
    r = cc.estep_residuals(n, "mixed", dtype)
    ref = cc.estep_reference(r, cc.ESTEP_SIGMA2, 0.5, cc.ESTEP_A, 3, cc.ESTEP_MINP, dtype)
    theta, dist = cc.pick_theta(ref["stored"])
    assert dist >= 1e-6
    for terms, exact in zip((ref["p"] * r, ref["p"], ref["stored"]), ref["sums"]):
        got = cc.blocked_sum(terms)
        assert abs(got - exact) <= 30 * 2.0 ** -53 * exact < cc.ESTEP_SUM_RTOL * exact
    assert cc.blocked_sum(np.ones(n)) == n


# ------------------------------------------------------------------------------------------------------ small kernels
@pytest.mark.parametrize("m,nrhs", [s for s in cc.QUADFORM_SHAPES if s[0] <= 1000])
def test_quadform_restatement(m, nrhs):
    K, C = cc.quadform_case(m, nrhs)
    assert (K > 0).all() and (C > 0).all()
    out = torch.zeros(1, dtype=torch.float64)
    CpuKernels().quadform(_t(K), _t(C), out)
    np.testing.assert_allclose(float(out[0]), cc.quadform_reference(K, C), rtol=1e-13)
    np.testing.assert_allclose(cc.quadform_reference(K, C), float(np.trace(C.T.astype(L) @ K.astype(L) @ C.astype(L))), rtol=1e-15)


@pytest.mark.parametrize("n", cc.LINCOMB_NS)
def test_lincomb3_restatement_and_one_binade_design(n):
    (a, A), (b, B), (c, C) = cc.lincomb3_case(n)
    k = CpuKernels()
    for kw in ({}, {"b": b, "B": B}, {"c": c, "C": C}, {"b": b, "B": B, "c": c, "C": C}):
        ref = cc.lincomb3_reference(a, A, **kw)
        lo = 2.0 ** math.floor(math.log2(ref.min()))
        assert ref.max() < 2 * lo  # one binade: the ulp is the same for every element and every intermediate
        out = torch.empty(n, dtype=torch.float64)
        k.lincomb3(out, a, _t(A), **{key: (_t(v) if key in "BC" else v) for key, v in kw.items()})
        assert (np.abs(out.numpy() - ref) <= np.spacing(ref)).all()


@pytest.mark.parametrize("m", [m for m in cc.SYM_MS if m <= 257])
def test_sym_pack_restatement(m):
    G = cc.sym_case(m)
    k = CpuKernels()
    tri = torch.empty(m * (m + 1) // 2, dtype=torch.float64)
    k.sym_pack(_t(G), tri)
    np.testing.assert_array_equal(tri.numpy(), G[np.triu_indices(m)])
    assert np.abs(tri.numpy()).max() < 1e300  # nothing of the lower triangle
    F = torch.empty(m, m, dtype=torch.float64)
    k.sym_unpack(tri, F)
    np.testing.assert_array_equal(F.numpy(), cc.sym_completion(tri.numpy(), m))
    np.testing.assert_array_equal(F.numpy(), F.numpy().T)
