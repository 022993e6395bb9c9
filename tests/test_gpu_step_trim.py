"""The EM step after its non-MFMA work was trimmed (P widened once per tile-stage phase instead of in every wave, the rhs
weights staged in LDS already widened, packed float32 distance arithmetic in the rhs / apply kernels) computes the SAME
BITS as before:

  * G and R of the cached path equal those of the recompute path (which widens nothing ahead of time) - across cell counts
    that are not multiples of the 256-cell chunk, in one and in several phases, on a reused workspace;
  * one whole EM iteration reproduces what the parent commit's build computed (tests/golden/step_trim_parent_bits.npz,
    written by tests/golden/make_golden_step_trim.py): this is what pins rhs_kernel and apply_kernel, which both Gram paths
    share;
  * two engines on two streams at once equal the sequential run.

Every comparison is bit for bit (torch.equal / np.array_equal): nothing here changes a summation order or a rounding."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_step_trim as gen  # noqa: E402
from _kernel_scaffold import fresh_kernels as _k, option as _option  # noqa: E402


def _inputs(k, seed, n, m):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (n, 3)) * 30.0
    ctrl = rng.uniform(-1, 1, (m, 3)) * 30.0  # (points of their own: m may exceed n)
    Y = rng.standard_normal((n, 3))
    P = torch.from_numpy(rng.uniform(1e-5, 1.0, n).astype(np.float32)).to("cuda:0")
    center = ctrl.mean(0)
    return k.to_x4(X, center), k.to_x4(ctrl, center), k.to_x4(Y), P


def _gr(m):
    return (torch.empty(m, m, dtype=torch.float64, device="cuda:0"), torch.empty(m, 3, dtype=torch.float64, device="cuda:0"))


def _recompute_and_cached(kk, x4, P, y4, c4, beta, m):
    """(G, R) of the recompute kernels (cache dropped), then of the cached path, on the same HipKernels."""
    kk.drop_ublk()
    G, R = _gr(m)
    kk.gram(x4, P, y4, c4, beta, G, R)
    kk.build_ublk(x4, c4, beta)
    Gc, Rc = _gr(m)
    kk.gram(x4, P, y4, c4, beta, Gc, Rc)
    return G, R, Gc, Rc


@pytest.mark.parametrize("m", [40, 130, 300, 1080])
@pytest.mark.parametrize("n", [255, 256, 4097, 70_001])
def test_cached_equals_recompute_float32(n, m):
    """The tail of the widened P (n not a multiple of 256, the last slice padded) and the rhs next to it."""
    kk = _k("float32")
    x4, c4, y4, P = _inputs(kk, 1000 + n + m, n, m)
    G, R, Gc, Rc = _recompute_and_cached(kk, x4, P, y4, c4, 0.003, m)
    assert torch.equal(G, Gc) and torch.equal(R, Rc)
    assert torch.equal(Gc, Gc.T)
    kk.drop_ublk()


@pytest.mark.parametrize("n_first,n", [(400_000, 300_001), (1_600_000, 1_200_001)])
def test_phases_and_workspace_reuse_float32(n_first, n):
    """256-cell slices (the plan test_gram_partial_tiles_in_phases forces) at m = 300, n after a LONGER call on the same
    HipKernels: what the earlier call left in the workspace (its widened P among it) must not leak, and a second call gives the
    same bits.  At 300 001 cells the 1172 slices x 6 tile pairs still fit the minimum partial-tile buffer (one phase); 1 200 001
    cells need two phases, each widening its own cells of P."""
    m, beta = 300, 0.003
    with _option("slice_len", 256):
        kk = _k("float32")
        x4, c4, y4, P = _inputs(kk, 5, n_first, m)
        kk.build_ublk(x4, c4, beta)
        kk.gram(x4, P, y4, c4, beta, *_gr(m))  # the longer call: fills the workspace
        x4, c4, y4, P = _inputs(kk, 6, n, m)
        G, R, Gc, Rc = _recompute_and_cached(kk, x4, P, y4, c4, beta, m)
        assert torch.equal(G, Gc) and torch.equal(R, Rc)
        G2, R2 = _gr(m)
        kk.gram(x4, P, y4, c4, beta, G2, R2)
        assert torch.equal(G2, Gc) and torch.equal(R2, Rc)
        if n > 1_000_000:  # really more than one phase: the buffer is smaller than all partial tiles
            assert kk.lib.mvf_gram_workspace_bytes(n, m, kk.cdtype) < (n // 256) * 6 * 128 * 128 * 8
        # the timed path (tile stage and the rest as two calls) gives the same bits
        kk.gram_events = []
        G3, R3 = _gr(m)
        kk.gram(x4, P, y4, c4, beta, G3, R3)
        assert len(kk.gram_events) == 1 and torch.equal(G3, Gc) and torch.equal(R3, Rc)
        kk.drop_ublk()


@pytest.mark.parametrize("m,dtype", gen.CASES)
def test_em_step_reproduces_parent_bits(m, dtype):
    """One EM iteration (E-step, Gram + rhs, solve, apply, statistics, sigma^2) against the bits the parent commit's build
    produced for the same seeded inputs."""
    with np.load(gen.OUT) as z:
        want = {name: z[f"m{m}_{dtype}_{name}"] for name in ("R", "C", "stats", "sigma2", "V_sha256", "r_sha256", "V_rows", "r_rows")}
    got = gen.case(m, dtype)
    for name in ("R", "V_rows", "r_rows", "V_sha256", "r_sha256", "stats", "C", "sigma2"):
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.dtype == b.dtype and a.shape == b.shape, name
        if not np.array_equal(a, b) and a.dtype != np.uint8:
            print(f"{name}: {int((a != b).sum())} of {a.size} values differ, max |diff| {np.abs(a.astype(np.float64) - b).max():.3e}")
        assert np.array_equal(a, b), name


def test_two_engines_on_two_streams_equal_the_sequential_run():
    """Two fits at once, each from its own host thread on its own stream (the pattern of the many-organs run): whatever a step
    keeps per call must not be shared between them."""
    from spateo_amd._synthetic import make_config
    from spateo_amd.engine import SparseVFCEngine
    from spateo_amd.vectorfield import bandwidth_selector

    jobs = []
    for seed, n, m in ((11, 70_001, 300), (12, 50_003, 260)):
        X, V, _ = make_config("C3", N=n, seed=seed)
        ctrl = X[np.random.default_rng(seed).choice(n, m, replace=False)]
        jobs.append((X, V, ctrl, 1 / bandwidth_selector(ctrl) ** 2))

    def fit(job, out, i, stream=None):
        def run():
            eng = SparseVFCEngine(*job, dtype="float32", device="cuda:0")
            eng.init_state(gamma=0.9)
            for _ in range(3):
                eng.em_step(a=5, lambda_=3.0)
            Vh, Ph, Ch = eng.results()
            out[i] = (Vh, Ph, Ch, eng.sigma2, eng.R[0].cpu().numpy(), eng.G.cpu().numpy())
            eng.k.drop_ublk()

        try:
            if stream is None:
                run()
            else:
                with torch.cuda.stream(stream):
                    run()
                stream.synchronize()
        except BaseException as exc:  # noqa: BLE001 - reported by the main thread
            out[i] = exc

    seq, par = [None, None], [None, None]
    for i, job in enumerate(jobs):
        fit(job, seq, i)
    threads = [threading.Thread(target=fit, args=(job, par, i, torch.cuda.Stream(device="cuda:0"))) for i, job in enumerate(jobs)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for a, b in zip(seq, par):
        assert not isinstance(a, BaseException) and not isinstance(b, BaseException), (a, b)
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.parametrize("m", [130, 600])
@pytest.mark.parametrize("n,cpt", [(1_100_001, 4), (600_001, 2)])
def test_apply_packed_lanes_equal_one_cell_per_lane(n, cpt, m):
    """apply_kernel<float, 4> and <float, 2> (packed float32 arithmetic over a lane's cells) against apply_kernel<float, 1> (the
    scalar kernel_value) on the SAME cells.  mvf_apply halves the cells per lane from 4 while that leaves fewer than 1024
    workgroups: n > 1 047 552 runs 4 per lane, 523 776 < n <= 1 047 552 runs 2, chunks of 100 000 cells run 1.  A cell's V and r
    depend on nothing but the cell, the control points and C (one sum over the control points in index order), so the two ways
    must agree bit for bit.  (The parent-bits fixture's 70 001 cells run one cell per lane: it pins the rhs kernel and the rest
    of the step, this test pins the packed apply.)  m = 130: one LDS stage, padded to a multiple of 4; m = 600: two stages."""
    assert (-(-n // (256 * cpt)) >= 1024) and (cpt == 4 or -(-n // (256 * 2 * cpt)) < 1024)  # the launch really takes `cpt`
    kk = _k("float32")
    x4, c4, y4, P = _inputs(kk, 2000 + n + m, n, m)
    C = torch.from_numpy(np.random.default_rng(3).standard_normal((m, 3))).to("cuda:0")
    beta = 0.003
    stats = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    V, r = kk.apply(x4, c4, beta, C, y4, P, stats)
    chunk = 100_000
    assert -(-chunk // 256) < 1024  # one cell per lane
    s1 = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        Vc, rc = kk.apply(x4[lo:hi], c4, beta, C, y4[lo:hi], P[lo:hi], s1)
        assert torch.equal(Vc, V[lo:hi]) and torch.equal(rc, r[lo:hi]), (lo, hi)
    # sum P r: the same terms in another partition of the block sums
    assert abs(float(stats[0]) - float(s1[0])) <= 1e-12 * abs(float(s1[0]))
    # without residuals (the evaluator's use of the kernel): the same field
    V2, _ = kk.apply(x4, c4, beta, C)
    assert torch.equal(V2, V)
