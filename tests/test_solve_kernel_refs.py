"""No GPU: the references, the bound and the case lists of tests/test_gpu_solve_kernels.py (tests/_solve_cases.py builds
them for both modules).

  * the np.longdouble references (C* from the designed spectrum, the longdouble Cholesky solve) agree with the float64
    LAPACK route on the same rounded matrices - np.linalg.eigh truncated solve, scipy.linalg.cho_solve - within the bound
    divided by 16 on every case: C_BOUND is 16 x the measured worst ratio, rounded up to a power of two (run with ``-s``
    for the ratios; profiles/solve_kernel_edges.md records them);
  * the restatements of the device algorithms in tests/_cpu_kernels.py (CpuKernels.solve / .solve_minnorm /
    .solve_minnorm_lr / .pinv_diag) stay within the bound on every case;
  * targeted defects, each applied to a NumPy restatement of the device's steps (padding to a multiple of 64, shifted
    factorisation, eigenpairs, cut-off, back-substitution per right-hand-side column, reuse, warm basis), leave the bound by
    >= 100 x on at least one case, and every spectrum family is told apart by the defect it exists for (FAMILY_DEFECT);
  * the pivot-order cases: the longdouble greedy margin is >= 2^-20 at every step, and every pivot is far above the
    stopping tolerance - the condition under which the GPU test may demand the identical order over the full length."""
import numpy as np
import pytest
import torch

import _solve_cases as sc
from _cpu_kernels import CpuKernels

LD = np.longdouble
_RATIOS = {}


def _note(route, c, r):
    key = (route, c["family"])
    if r > _RATIOS.get(key, (0.0, ""))[0]:
        _RATIOS[key] = (float(r), c["id"])


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    yield
    print("\n| route | family | largest deviation / (m eps kappa_kept) | case |\n|---|---|---|---|")
    for (route, fam), (r, cid) in sorted(_RATIOS.items()):
        print(f"| {route} | {fam} | {r:.3g} | {cid} |")
    lap = [r for (route, _), (r, _) in _RATIOS.items() if route.startswith("lapack")]
    if lap:
        print(f"largest LAPACK-route ratio {max(lap):.3g} -> 16 x = {16 * max(lap):.3g} -> C_BOUND = {sc.C_BOUND:g}")


def _unit_ratio(C, Cs, c):
    """deviation / (m eps kappa_kept): the ratio C_BOUND is measured in."""
    return sc.col_dev(C, Cs) / (c["m"] * sc.EPS * c["kappa"])


# ------------------------------------------------------------------------------------------ references vs LAPACK
def test_case_lists_cover_the_paddings_and_switches():
    assert sc.C_BOUND == 2.0 ** round(np.log2(sc.C_BOUND))
    for edge in (64, 128):  # padding / Jacobi tile / hinted panel; small kernel vs blocked, lower limit of the deflated forms
        assert {edge - 1, edge, edge + 1} <= set(sc.SOLVE_M_BLOCKED)
    assert {511, 512, 513} <= set(sc.LR_M) and {511, 512, 513, 640, 641, 127, 128, 129} <= set(sc.LRD_M)
    assert sc.solve_nrhs(65) == list(range(1, 9)) == sc.solve_nrhs(129)
    fams = {c["family"] for c in sc.minnorm_cases()}
    assert fams == set(sc.FAMILIES)
    assert {c["family"] for c in sc.lr_cases()} == set(sc.LR_FAMILIES)
    for c in sc.all_cases():
        assert c["A"].dtype == np.float64 and np.array_equal(c["A"], c["A"].T) and np.array_equal(c["G"], c["G"].T)
        # a non-trivial split: both operands matter (1e-3 of lambda_max on the exact-rank families, see make_case)
        assert np.abs(c["ls2"] * c["K"]).max() > (1e-4 if c["family"].startswith("rank") else 0.05) * c["lmax"]
    c = sc.make_case("ortho", 129)
    q0 = sc.q_times(c["refl"], np.eye(129, dtype=LD)[:, :1])[:, 0]
    assert abs(float(q0.sum())) < 1e-17 * 129  # the dominant eigenvector is orthogonal to the cold power iteration's start


@pytest.mark.parametrize("c", sc.all_cases(), ids=lambda c: c["id"])
def test_longdouble_references_agree_with_lapack(c):
    m = c["m"]
    Cs = sc.c_star(c, c["R"])
    C, w, keep = sc.lapack_minnorm(c)
    assert int(keep.sum()) == c["rank"]  # the kept set is unambiguous after rounding
    r = _unit_ratio(C, Cs, c)
    _note("lapack eigh vs C*", c, r)
    assert 16 * r <= sc.C_BOUND, r
    lam = np.asarray(c["lam"], dtype=np.float64)
    assert abs(np.abs(w).max() - np.abs(lam).max()) <= sc.eig_bound(c) / 16
    assert abs(np.abs(w[keep]).min() - np.abs(lam[c["keep"]]).min()) <= sc.eig_bound(c) / 16
    assert abs(w.min() - lam.min()) <= sc.eig_bound(c) / 16
    if c["family"] in sc.SOLVE_FAMILIES and m <= max(sc.SOLVE_M_BLOCKED):
        for jitter in (0.0, 1e-6, 1e-2):
            Cr, piv = sc.cholesky_solve_ld(c["A"], c["R"], jitter)
            r = _unit_ratio(sc.lapack_solve(c, jitter), Cr, c)
            _note("lapack cho_solve vs longdouble Cholesky", c, r)
            assert 16 * r <= sc.C_BOUND, (jitter, r)
            if jitter == 0.0:  # the Cholesky reference solves the designed system
                r = _unit_ratio(Cr, Cs, c)
                _note("longdouble Cholesky vs C*", c, r)
                assert 16 * r <= sc.C_BOUND, r
                d = np.diag(np.linalg.cholesky(c["A"])) ** 2
                np.testing.assert_allclose([d.min(), d.max()], np.asarray(piv, dtype=np.float64), rtol=1e-12 * c["kappa"])


# ------------------------------------------------------------------------------------------ tests/_cpu_kernels.py
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("c", sc.all_cases(), ids=lambda c: c["id"])
def test_cpu_restatements_stay_within_the_bound(c):
    m, k = c["m"], CpuKernels()
    G, K, R = _t(c["G"]), _t(c["K"]), _t(c["R"])
    Cs = sc.c_star(c, c["R"])
    C, info, einfo = torch.zeros(m, 8, dtype=torch.float64), torch.ones(1, dtype=torch.int32), torch.zeros(12, dtype=torch.float64)
    k.solve_minnorm(G, K, c["ls2"], sc.minnorm_shift(c), R, C, info, einfo, rcond=c["rcond"])
    r = sc.ratio(C.numpy(), Cs, c)
    _note("CpuKernels.solve_minnorm", c, r * sc.C_BOUND)
    assert int(info[0]) == 0 and r <= 1.0 and int(einfo[1]) == c["rank"]
    R2 = c["R"][:, ::-1][:, :5].copy()
    C2 = torch.zeros(m, 5, dtype=torch.float64)
    k.solve_minnorm(G, K, c["ls2"], sc.minnorm_shift(c), _t(R2), C2, info, einfo, rcond=c["rcond"], reuse=True)
    assert sc.ratio(C2.numpy(), sc.c_star(c, R2), c) <= 1.0
    if c["family"] in sc.LR_FAMILIES:
        for deflate in (False, True):
            C.zero_()
            k.solve_minnorm_lr(G, K, c["ls2"], R, C, info, einfo, rcond=c["rcond"], deflate=deflate)
            r = sc.ratio(C.numpy(), Cs, c)
            _note("CpuKernels.solve_minnorm_lr", c, r * sc.C_BOUND)
            assert int(info[0]) == 0 and r <= 1.0 and int(einfo[1]) == c["rank"], (deflate, r)
            assert c["rank"] <= int(einfo[6]) <= m
    if c["family"] in sc.SOLVE_FAMILIES and m <= max(sc.SOLVE_M_BLOCKED):
        piv = torch.zeros(2, dtype=torch.float64)
        for jitter in (0.0, 1e-2):
            Cr, pr = sc.cholesky_solve_ld(c["A"], c["R"], jitter)
            k.solve(G, K, c["ls2"], jitter, R, C, info, piv)
            r = sc.ratio(C.numpy(), Cr, c)
            _note("CpuKernels.solve", c, r * sc.C_BOUND)
            assert int(info[0]) == 0 and r <= 1.0
            np.testing.assert_allclose(piv.numpy(), np.asarray(pr, dtype=np.float64), rtol=1e-12 * c["kappa"])


@pytest.mark.parametrize("m", [1, 127, 128, 129, 257])
def test_cpu_pinv_diag_and_the_float32_floor(m):
    """CpuKernels.pinv_diag within the solve bound of the longdouble leverage sum; and the float32 floor: the same reference
    (same A, same eigenpairs) with U from float32-rounded coordinates against float64 ones - the constants of
    _solve_cases.FLOAT32_PINV_FLOOR (profiles/solve_kernel_edges.md records them)."""
    pc = sc.pinv_case(257, m)
    lc = sc.leverage_reference(pc, np.float64)
    ref, kappa, rank = lc["ref"], lc["kappa"], lc["rank"]
    k = CpuKernels()
    b64 = sc.C_BOUND * m * sc.EPS * kappa
    C, info, einfo = torch.zeros(m, 3, dtype=torch.float64), torch.ones(1, dtype=torch.int32), torch.zeros(12, dtype=torch.float64)
    for lowrank in (False, True):
        if lowrank:
            k.solve_minnorm_lr(_t(lc["A"]), _t(np.zeros((m, m))), 0.0, _t(np.ones((m, 3))), C, info, einfo, rcond=pc["rcond"])
        else:
            k.solve_minnorm(_t(lc["A"]), _t(np.zeros((m, m))), 0.0, sc.SHIFT, _t(np.ones((m, 3))), C, info, einfo, rcond=pc["rcond"])
        d = k.pinv_diag(k.to_x4(pc["X"], pc["center"]), k.to_x4(pc["ctrl"], pc["center"]), pc["beta"], rcond=pc["rcond"],
                        lowrank=lowrank).numpy()
        assert int(einfo[1]) == rank
        dev = float(np.abs(d - ref).max() / ref.max())
        assert dev <= b64, (lowrank, dev)
        assert d.min() >= -b64 and d.max() <= 1 + b64 and abs(d.sum() - rank) <= 257 * b64
    ref32 = sc.leverage_reference(pc, np.float32)["ref"]
    floor = float(np.abs(ref32 - ref).max() / ref.max())
    print(f"pinv_diag m = {m}: kappa_kept {kappa:.3g}, rank {rank}, float64 bound {b64:.3g}, float32 floor {floor:.4g}")
    assert floor <= sc.FLOAT32_PINV_FLOOR[m] <= 1.1 * floor  # the recorded constant is the measured one


# ------------------------------------------------------------------------------------------ targeted defects
DEFECTS = ["pad_not_zeroed", "shift_not_subtracted", "cut_relative_to_min", "last_rhs_column_dropped",
           "jitter_scaled_by_max_diag", "reuse_keeps_previous_scaling", "warm_basis_transposed", "lambda_max_underestimated",
           "cut_on_signed_lambda"]
# The defect each family exists for: the one that shows only (or chiefly) because of what is special about that spectrum.
# The generic defects (padding, reuse, the dropped column) leave the bound on every family and prove nothing about a family.
FAMILY_DEFECT = {
    "well": "jitter_scaled_by_max_diag",      # kappa = 1e2: what a wrongly scaled jitter does is not drowned by the bound
    "graded": "shift_not_subtracted",          # eigenvalues down to 1e-8 lambda_max: delta is a visible fraction of them
    "rank1": "cut_relative_to_min",            # exact zeros: a cut that follows the smallest |lambda| keeps the null space
    "rankhalf": "shift_not_subtracted",        # exact zeros: unshifted they sit at delta, above the cut, and are kept
    "rankm1": "cut_relative_to_min",
    "cluster": "cut_relative_to_min",          # dropped eigenvalues 1e3 below the kept ones, both far from zero
    "ortho": "lambda_max_underestimated",      # dominant eigenvector orthogonal to the cold power iteration's start
    "indef": "cut_on_signed_lambda",           # negative eigenvalues: the cut and the kept rank are on |lambda|
}


def _restated_minnorm(c, R, defect=None, prev_R=None, warm_from=None):
    """The device's steps in NumPy float64: pad to a multiple of 64, factor A + delta I, eigenpairs of the factor,
    lambda = sigma^2 - delta, cut at rcond max|lambda|, C = sum q (q^T R) / lambda column by column."""
    m, A = c["m"], c["A"]
    delta = sc.minnorm_shift(c) * np.trace(A) / m
    # a correct kernel leaves the padding decoupled (zero rows / columns, unit diagonal for the factorisation, rows dropped
    # again): the m x m problem.  The defect: rows / columns m .. mp-1 keep what the workspace held
    mp = sc.pad(m) if defect == "pad_not_zeroed" else m
    Ap = np.zeros((mp, mp))
    Ap[:m, :m] = A
    if mp > m:
        stale = np.random.default_rng(1).uniform(-1, 1, (mp, mp)) * c["lmax"]
        stale = (stale + stale.T) / 2
        Ap[m:, :] = stale[m:, :]
        Ap[:, m:] = stale[:, m:]
    Wt = None
    if warm_from is not None:  # rows = eigenvectors of the nearby matrix
        Wt = np.linalg.eigh(warm_from["A"])[1].T
        Ap = Wt @ Ap @ Wt.T
    sig2, q = np.linalg.eigh(Ap + delta * np.eye(mp))
    if Wt is not None:
        q = (Wt if defect == "warm_basis_transposed" else Wt.T) @ q
    lam = sig2 - (0.0 if defect == "shift_not_subtracted" else delta)
    absl = np.abs(lam)
    lmax = absl.max() * (1e-3 if defect == "lambda_max_underestimated" else 1.0)
    cut = c["rcond"] * (absl[absl > 0].min() if defect == "cut_relative_to_min" else lmax)
    keep = (lam > cut) if defect == "cut_on_signed_lambda" else (absl > cut)
    Rs = prev_R if defect == "reuse_keeps_previous_scaling" else R
    Rp = np.zeros((mp, R.shape[1]))
    Rp[:m] = Rs[:, : R.shape[1]]
    C = ((q[:, keep] / lam[keep]) @ (q[:, keep].T @ Rp))[:m]
    if defect == "last_rhs_column_dropped" and R.shape[1] == 8:
        C[:, 7] = 0.0
    return C, int(keep.sum())


def _restated_solve(c, R, jitter, defect=None):
    A = c["A"]
    d = np.diag(A)
    A = A + jitter * (d.max() if defect == "jitter_scaled_by_max_diag" else d.mean()) * np.eye(c["m"])
    return np.linalg.solve(A, R)


def _defect_cases():
    return [c for c in sc.minnorm_cases() if c["m"] >= 2]


def test_restatement_without_a_defect_is_within_the_bound():
    for c in _defect_cases():
        Cs = sc.c_star(c, c["R"])
        C, rank = _restated_minnorm(c, c["R"])
        assert rank == c["rank"] and sc.ratio(C, Cs, c) <= 1.0, c["id"]
        C, rank = _restated_minnorm(c, c["R"], warm_from=sc.nearby_case(c))
        assert rank == c["rank"] and sc.ratio(C, Cs, c) <= 1.0, c["id"]
        if c["family"] in sc.SOLVE_FAMILIES:
            assert sc.ratio(_restated_solve(c, c["R"], 1e-2), sc.cholesky_solve_ld(c["A"], c["R"], 1e-2)[0], c) <= 1.0


def test_each_defect_leaves_the_bound_by_100x_and_every_family_is_told_apart():
    worst = {}
    for c in _defect_cases():
        Cs = sc.c_star(c, c["R"])
        R2 = c["R"][:, ::-1].copy()
        for defect in DEFECTS:
            if defect == "jitter_scaled_by_max_diag":
                if c["family"] not in sc.SOLVE_FAMILIES:
                    continue
                r = sc.ratio(_restated_solve(c, c["R"], 1e-2, defect), sc.cholesky_solve_ld(c["A"], c["R"], 1e-2)[0], c)
            elif defect == "lambda_max_underestimated":
                if c["family"] != "ortho":
                    continue
                r = sc.ratio(_restated_minnorm(c, c["R"], defect)[0], Cs, c)
            elif defect == "reuse_keeps_previous_scaling":
                r = sc.ratio(_restated_minnorm(c, R2, defect, prev_R=c["R"])[0], sc.c_star(c, R2), c)
            elif defect == "warm_basis_transposed":
                r = sc.ratio(_restated_minnorm(c, c["R"], defect, warm_from=sc.nearby_case(c))[0], Cs, c)
            else:
                r = sc.ratio(_restated_minnorm(c, c["R"], defect)[0], Cs, c)
            key = (defect, c["family"])
            if r > worst.get(key, (0.0, ""))[0]:
                worst[key] = (r, c["id"])
    print("\n| defect | family | largest deviation / bound | case |\n|---|---|---|---|")
    for (defect, fam), (r, cid) in sorted(worst.items()):
        print(f"| {defect} | {fam} | {r:.3g} | {cid} |")
    for defect in DEFECTS:
        best = max(r for (d, _), (r, _) in worst.items() if d == defect)
        assert best >= 100.0, (defect, best)
    # a family that its own defect does not distinguish would be dead weight
    assert set(FAMILY_DEFECT) == set(sc.FAMILIES)
    for fam, defect in FAMILY_DEFECT.items():
        assert worst[(defect, fam)][0] >= 100.0, (fam, defect, worst[(defect, fam)])
    # ... and the defects that need a special spectrum do nothing on the plain ones (the families are not interchangeable)
    assert worst[("cut_on_signed_lambda", "well")][0] <= 1.0 and worst[("cut_relative_to_min", "well")][0] <= 1.0


# ------------------------------------------------------------------------------------------ pivot-order cases
@pytest.mark.parametrize("m", sc.PIVOT_M)
def test_pivot_cases_have_a_clear_greedy_order(m):
    c = sc.pivot_case(m)
    tol = 0.25 * sc.EPS * c["lmax"]
    order, piv, margins = sc.greedy_pivoted_cholesky_ld(c["A"], tol)
    print(f"pivot case m = {m}: smallest margin {margins.min():.3g} (2^{np.log2(margins.min()):.1f}), smallest pivot / tol "
          f"{float(piv.min() / tol):.3g}")
    assert len(order) == m and sorted(order) == list(range(m))
    assert margins.min() >= sc.MARGIN_MIN
    assert float(piv.min()) >= 1e3 * tol  # no pivot anywhere near the stopping tolerance
    assert np.all(np.diff(np.asarray(piv, dtype=np.float64)) <= 0)  # falling, as mvf.h says
    # the stopping tolerance mvf_lr_pivot_order reports is tolf eps x the 8-step power estimate of lambda_max: settled to 1e-7
    # on these matrices, so that the GPU test may compare it with the Jacobi iteration's lambda_max (einfo[2]) to 1e-6
    assert abs(sc.power_estimate(c["A"]) - c["lmax"]) <= 1e-7 * c["lmax"]


@pytest.mark.parametrize("c", sc.exact_rank_cases(), ids=lambda c: c["id"])
def test_exact_rank_cases_leave_nothing_near_the_stopping_tolerance(c):
    """The condition under which the GPU test may demand einfo[6] == the designed rank: in longdouble, on the float64 matrix
    the device assembles, the greedy factorisation's remaining diagonal after that many pivots (the rounding of the matrix)
    is below an eighth of the stopping tolerance 0.25 eps lambda_max, and the last kept pivot is far above it."""
    tol = 0.25 * sc.EPS * c["lmax"]
    r = c["rank"]
    for dtype in (LD, np.float64):  # (float64: the rounding a float64 factorisation adds on its own)
        _, piv, _ = sc.greedy_pivoted_cholesky_ld(c["A"], 0.0, max_steps=r + 1, dtype=dtype)
        assert len(piv) >= r and float(piv[r - 1]) >= 1e6 * tol
        assert len(piv) == r or float(piv[r]) <= sc.EXACT_RANK_RESIDUAL_MAX * tol, (dtype, float(piv[r] / tol))
