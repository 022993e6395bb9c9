"""GPU tests of the coefficient-solve POLICY of the EM engine (engine.py::_solve_all_local): which solver form answers each
iteration of small whole fits that between them take every form - jitter Cholesky, certified Cholesky, full-width Jacobi, the
rank-revealing solve, the deflated solve in its factor and direct forms (synchronous and asynchronous) and the `reuse` batches.

Per case the per-iteration sequence of (`_solver_signature[0]`, block) and the `cholesky` / `minnorm` / `async` counts are
compared with a literal table.  The table was recorded on the commit BEFORE the policy was split into one method per form
(profiles/solve_policy_refactor.md), never from the code under test: it pins which path the engine takes, the numbers of the
paths are the business of test_gpu_em.py / test_gpu_scale.py / test_gpu_solve_kernels.py.

Sizes: 20 000 C2 cells with 500 control points reach the direct form from the second rank-deficient iteration on (no need for
C2's own 50 000); 200 control points and the 4-D cloud stay certified at that size, so the full-width Jacobi cases ask for it by
name ("full") at 500.  The rejected async call is pinned on the host
(tests/test_host_logic.py::test_direct_form_async_branch_rejected), not here.

signature[0]: 1 = lstsq_method "cholesky", 2 = certified Cholesky, 3 = rank-revealing / deflated, 4 = full-width Jacobi.
block: einfo[7] of the deflated solve (64 direct / small factor, 128 / 256 factor form, 0 = its Jacobi form answered);
None where the iteration appended none (Cholesky, full-width Jacobi, "lowrank")."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _c2(n, dy=3):
    """C2 cells; dy > 3 appends smooth functions of the points as further columns (kernel_interpolation's use)."""
    from spateo_amd._synthetic import make_config

    X, V, _ = make_config("C2", N=n)
    if dy > 3:
        extra = [np.sin(X[:, 0] / 80 + j) + 0.3 * np.cos(X[:, 1] / 60 * (j + 1)) for j in range(dy - 3)]
        V = np.column_stack([V] + extra)
    return X, V


def _lifted4(n):
    """C2's ellipsoid and a rotating / sheared field in four dimensions, unit rms, noise 0.05."""
    rng = np.random.default_rng(0)
    g = rng.standard_normal((n, 4))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    X = g * (rng.random(n) ** 0.25)[:, None] * np.linspace(300.0, 120.0, 4)
    A = 0.02 * np.eye(4)
    A[0, 1], A[1, 0], A[2, 3], A[3, 2] = -0.01, 0.01, -0.015, 0.015
    V = X @ A.T + 2.0 * np.sin(2 * np.pi * np.roll(X, 1, axis=1) / float(np.abs(X).max()))
    V /= np.sqrt(np.mean(V**2))
    return X, V + 0.05 * rng.standard_normal(V.shape)


# name -> (data, M, lambda_, EM steps, engine options)
CASES = {
    "certified_cholesky": (lambda: _c2(6000), 100, 3.0, 6, {}),
    "full_jacobi_m200": (lambda: _c2(20_000), 200, 0.02, 12, {}),
    "full_jacobi_warm": (lambda: _c2(20_000), 500, 0.02, 8, {"minnorm_method": "full"}),
    "direct_form": (lambda: _c2(20_000), 500, 0.02, 12, {}),
    "direct_form_sync_only": (lambda: _c2(20_000), 500, 0.02, 6, {"async_direct": False}),
    "factor_form": (lambda: _c2(20_000), 1100, 3.0, 6, {}),
    "lowrank": (lambda: _c2(10_000), 800, 0.02, 5, {"minnorm_method": "lowrank"}),
    "dy5_one_batch": (lambda: _c2(20_000, 5), 500, 0.02, 8, {}),
    "dy7_reuse_batches": (lambda: _c2(20_000, 7), 500, 0.02, 8, {}),
    "dy7_reuse_full": (lambda: _c2(20_000, 7), 500, 0.02, 6, {"minnorm_method": "full"}),
    "cholesky_mode": (lambda: _c2(6000), 200, 0.02, 5, {"lstsq_method": "cholesky"}),
    "four_dimensions": (lambda: _lifted4(20_000), 500, 0.02, 8, {}),
}


def run_case(name, dtype, on_step=None):
    """The fit of CASES[name] in `dtype`; returns (engine, [(signature[0], block) per iteration]).  on_step(engine) is
    called after every EM iteration."""
    from spateo_amd.vectorfield import SparseVFCEngine, sparsevfc_preprocess

    data, M, lambda_, steps, opt = CASES[name]
    X, Y = data()
    valid, Xv, Yv, idx, ctrl, beta = sparsevfc_preprocess(X, Y, M=M, seed=0)
    SparseVFCEngine.minnorm_method = opt.get("minnorm_method")
    try:
        eng = SparseVFCEngine(Xv, Yv, ctrl, beta, dtype=dtype, device="cuda:0")
    finally:
        SparseVFCEngine.minnorm_method = None
    eng.async_direct = opt.get("async_direct", True)
    eng.lstsq_method = opt.get("lstsq_method", "scipy")
    eng.init_state(0.9)
    seq = []
    for _ in range(steps):
        nblock = len(eng.solver_stats.get("block", []))
        eng.em_step(a=5.0, lambda_=lambda_, minP=1e-5, theta=0.75)
        blocks = eng.solver_stats.get("block", [])
        seq.append((int(eng._solver_signature[0]), blocks[-1] if len(blocks) > nblock else None))
        if on_step is not None:
            on_step(eng)
    return eng, seq


def _counts(eng):
    st_ = eng.solver_stats
    return st_["cholesky"], st_["minnorm"], st_.get("async", 0)


# (case, dtype) -> ([(signature[0], block) per iteration], (cholesky, minnorm, async)): the parent commit's run
EXPECTED = {
    ("certified_cholesky", "float64"): ([(2, None)] * 6, (6, 0, 0)),
    ("certified_cholesky", "float32"): ([(2, None)] * 6, (6, 0, 0)),
    ("full_jacobi_m200", "float64"): ([(2, None)] * 12, (12, 0, 0)),   # (200 control points stay certified at this size)
    ("full_jacobi_m200", "float32"): ([(2, None)] * 12, (12, 0, 0)),
    ("full_jacobi_warm", "float64"): ([(2, None)] + [(4, None)] * 7, (1, 7, 0)),
    ("full_jacobi_warm", "float32"): ([(4, None)] * 8, (0, 8, 0)),
    ("direct_form", "float64"): ([(2, None)] + [(3, 64)] * 11, (1, 11, 9)),   # two synchronous calls, then async
    ("direct_form", "float32"): ([(3, 64)] * 12, (0, 12, 9)),                 # (the first factor keeps 498 of 500: three)
    ("direct_form_sync_only", "float64"): ([(2, None)] + [(3, 64)] * 5, (1, 5, 0)),
    ("direct_form_sync_only", "float32"): ([(3, 64)] * 6, (0, 6, 0)),
    ("factor_form", "float64"): ([(3, 256)] + [(3, 128)] + [(3, 256)] * 4, (0, 6, 0)),
    ("factor_form", "float32"): ([(3, 256)] * 6, (0, 6, 0)),
    ("lowrank", "float64"): ([(3, None)] * 5, (0, 5, 0)),
    ("lowrank", "float32"): ([(3, None)] * 5, (0, 5, 0)),
    ("dy5_one_batch", "float64"): ([(2, None)] + [(3, 64)] * 7, (1, 7, 5)),   # six right-hand sides in ONE batch: async
    ("dy5_one_batch", "float32"): ([(3, 64)] * 8, (0, 8, 5)),
    ("dy7_reuse_batches", "float64"): ([(2, None)] + [(3, 64)] * 7, (1, 7, 0)),   # two batches: never async
    ("dy7_reuse_batches", "float32"): ([(3, 64)] * 8, (0, 8, 0)),
    ("dy7_reuse_full", "float64"): ([(2, None)] + [(4, None)] * 5, (1, 5, 0)),
    ("dy7_reuse_full", "float32"): ([(4, None)] * 6, (0, 6, 0)),
    ("cholesky_mode", "float64"): ([(1, None)] * 5, (5, 0, 0)),
    ("cholesky_mode", "float32"): ([(1, None)] * 5, (5, 0, 0)),
    ("four_dimensions", "float64"): ([(2, None)] * 8, (8, 0, 0)),
    ("four_dimensions", "float32"): ([(2, None)] * 8, (8, 0, 0)),
}


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", list(CASES))
def test_solver_form_per_iteration(name, dtype):
    assert torch.cuda.is_available()
    eng, seq = run_case(name, dtype)
    want_seq, want_counts = EXPECTED[(name, dtype)]
    print(name, dtype, seq, _counts(eng))
    assert seq == want_seq
    assert _counts(eng) == want_counts
    if name == "direct_form":
        assert eng.solver_stats.get("async", 0) >= 1  # the host-sync-free branch was taken, whatever the table says
    if hasattr(eng.k, "drop_ublk"):
        eng.k.drop_ublk()
