"""The persistent launch of the float32 shared-column Gram tile kernel (gram_cached_kernel_shared_cols_persistent: at most
one workgroup per resident slot, each taking job numbers from a counter until they run out) computes the SAME BITS as the
launch of one workgroup per job and as the register-operand kernel: a job's partial tile is addressed by (slice, pair) and
the reduction sums the partial tiles in index order, so neither the order of the jobs nor the workgroup that runs one shows.

The developer option "gram_reg_cols" selects the path: 0 = the plan's choice (persistent when a launch holds more than two
rounds of jobs), 1 = register-operand kernel, 2 = shared-column kernel per job, 3 = shared-column kernel persistent.  Every
comparison is torch.equal.

Shapes are the smallest at which the new code can go wrong.  The slice length is forced to 256 cells, so jobs are short and
many.  m = 130: two tile columns, the second a narrow edge (diagonal and 2 x 4 edge shapes only); m = 200: a wide edge (the
full 2 x 8 shape off the diagonal); m = 1080: nine tile columns as in the golden EM step, all three shapes, so a workgroup
changes shape from job to job.  m = 100 is one tile pair, so the number of jobs is the
number of slices and can be set exactly around the number of resident slots, which is read from the device.  A persistent
workgroup's first job is its own index, so none is ever without a job: "exactly one" (jobs <= slots), "one or two"
(slots + 1) and "many" all occur."""
import threading

import numpy as np
import pytest
import torch

from _kernel_scaffold import DEV, fresh_kernels as _k, option as _option

pytestmark = pytest.mark.gpu

BETA = 0.003
REG_COLS, PER_JOB, PERSISTENT = 1, 2, 3
SLICE = 256
MIN_BUFFER_TILES = int(3e9 // (128 * 128 * 8))  # make_plan: the partial-tile buffer holds at least 3 GB


def _slots():
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count  # gram_slots() of csrc/mvf_gram.hip


def _npairs(m):
    nt = -(-m // 128)
    return nt * (nt + 1) // 2


def _jobs_per_phase(n, m):
    """(jobs of the largest launch, phases) of make_plan with 256-cell slices."""
    nslices = -(-n // SLICE)
    fit = max(1, max(_npairs(m), MIN_BUFFER_TILES) // _npairs(m))
    nphases = -(-nslices // fit)
    return -(-nslices // nphases) * _npairs(m), nphases


def _inputs(k, seed, n, m):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (n, 3)) * 30.0
    ctrl = rng.uniform(-1, 1, (m, 3)) * 30.0
    Y = rng.standard_normal((n, 3))
    center = ctrl.mean(0)
    return k.to_x4(X, center), k.to_x4(ctrl, center), k.to_x4(Y), _weights(seed, n)


def _weights(seed, n):
    return torch.from_numpy(np.random.default_rng(10_000 + seed).uniform(1e-5, 1.0, n).astype(np.float32)).to(DEV)


def _gram(kk, path, x4, P, y4, c4, m, poison=False):
    """G, R of the cached path `path` (a value of "gram_reg_cols"); poison: every byte of the workspace set first (a
    counter that is not zeroed again then hands out no job at all, and the partial tiles read back as NaN)."""
    G = torch.empty(m, m, dtype=torch.float64, device=DEV)
    R = torch.empty(m, 3, dtype=torch.float64, device=DEV)
    if poison and kk._gram_ws is not None:
        kk._gram_ws.fill_(0xFF)
    with _option("gram_reg_cols", path):
        kk.gram(x4, P, y4, c4, BETA, G, R, cache_only=True)
    return G, R


def _check_paths(kk, x4, P, y4, c4, m, auto=True):
    Gj, Rj = _gram(kk, PER_JOB, x4, P, y4, c4, m)
    Gp, Rp = _gram(kk, PERSISTENT, x4, P, y4, c4, m, poison=True)
    Gr, Rr = _gram(kk, REG_COLS, x4, P, y4, c4, m)
    assert torch.isfinite(Gj).all()
    assert torch.equal(Gp, Gj) and torch.equal(Rp, Rj)
    assert torch.equal(Gp, Gr) and torch.equal(Rp, Rr)
    assert torch.equal(Gp, Gp.T)
    if auto:
        Ga, Ra = _gram(kk, 0, x4, P, y4, c4, m, poison=True)
        assert torch.equal(Ga, Gj) and torch.equal(Ra, Rj)
    return Gj, Rj


@pytest.mark.parametrize("m", [130, 200, 1080])
@pytest.mark.parametrize("n", [70_001, SLICE * 37 + 5])
def test_persistent_equals_per_job_and_register_operands(n, m):
    """Tile shapes by m, cell counts that leave a padded last slice: 274 and 38 slices of 256 cells."""
    with _option("slice_len", SLICE):
        kk = _k("float32")
        x4, c4, y4, P = _inputs(kk, n + m, n, m)
        kk.build_ublk(x4, c4, BETA)
        _check_paths(kk, x4, P, y4, c4, m)
        kk.drop_ublk()


@pytest.mark.parametrize("edge", ["below", "equal", "one above", "two rounds", "just past two rounds", "far above"])
def test_job_counts_around_the_resident_slots(edge):
    """m = 100: one (diagonal) tile pair, jobs = slices.  Below and at the slot count every workgroup runs exactly one job and
    leaves on the first number it takes; one above, one workgroup runs two; at 2 x slots the plan still launches per job and one
    job further it turns persistent; far above every workgroup runs many."""
    slots, m = _slots(), 100
    nslices = {"below": slots - 1, "equal": slots, "one above": slots + 1, "two rounds": 2 * slots,
               "just past two rounds": 2 * slots + 1, "far above": 4 * slots + 3}[edge]
    n = SLICE * (nslices - 1) + 17
    assert _jobs_per_phase(n, m) == (nslices, 1)
    with _option("slice_len", SLICE):
        kk = _k("float32")
        x4, c4, y4, P = _inputs(kk, nslices, n, m)
        kk.build_ublk(x4, c4, BETA)
        _check_paths(kk, x4, P, y4, c4, m)
        kk.drop_ublk()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_job_counts_around_the_resident_slots_three_pairs(delta):
    """m = 130: three tile pairs of two shapes per slice, the slice count next to slots / 3."""
    slots, m = _slots(), 130
    nslices = slots // 3 + delta
    n = SLICE * nslices
    with _option("slice_len", SLICE):
        kk = _k("float32")
        x4, c4, y4, P = _inputs(kk, 50 + delta, n, m)
        kk.build_ublk(x4, c4, BETA)
        _check_paths(kk, x4, P, y4, c4, m)
        kk.drop_ublk()


@pytest.mark.parametrize("nslices,nphases", [(600, 2), (1017, 3)])
def test_phases_on_one_workspace_with_the_counter_zeroed_every_phase(nslices, nphases):
    """m = 1080: 45 tile pairs, so the 3 GB partial-tile buffer holds 508 slices and 600 / 1017 slices take two / three
    launches, each with its own count of jobs.  Then a second call on the same workspace with other weights: the counter of
    the first call's last launch (and, poisoned, every byte of the workspace) must not leak into it."""
    m = 1080
    n = SLICE * (nslices - 1) + 5
    jobs, ph = _jobs_per_phase(n, m)
    assert ph == nphases and jobs > 2 * _slots()  # the plan's own choice is the persistent launch
    with _option("slice_len", SLICE):
        kk = _k("float32")
        x4, c4, y4, P = _inputs(kk, nslices, n, m)
        kk.build_ublk(x4, c4, BETA)
        G1, R1 = _check_paths(kk, x4, P, y4, c4, m)
        P2 = _weights(7, n)
        Gp, Rp = _gram(kk, PERSISTENT, x4, P2, y4, c4, m)                # straight behind another persistent call
        Gq, Rq = _gram(kk, PERSISTENT, x4, P2, y4, c4, m, poison=True)   # and on a poisoned workspace
        Gj, Rj = _gram(kk, PER_JOB, x4, P2, y4, c4, m)
        assert torch.equal(Gp, Gj) and torch.equal(Rp, Rj) and torch.equal(Gq, Gj) and torch.equal(Rq, Rj)
        assert not torch.equal(Gj, G1)
        kk.drop_ublk()


def test_two_engines_on_two_streams_equal_the_sequential_run():
    """Two HipKernels at once, each from its own host thread on its own stream, every tile stage persistent: the counter lives in
    each one's own workspace, so the two must not see each other."""
    shapes = ((21, 70_001, 300), (22, 50_003, 260))

    def run(seed, n, m, out, i, stream=None):
        def work():
            kk = _k("float32")
            x4, c4, y4, P = _inputs(kk, seed, n, m)
            kk.build_ublk(x4, c4, BETA)
            res = []
            for rep in range(3):
                G = torch.empty(m, m, dtype=torch.float64, device=DEV)
                R = torch.empty(m, 3, dtype=torch.float64, device=DEV)
                kk.gram(x4, _weights(seed + rep, n), y4, c4, BETA, G, R, cache_only=True)
                res.append((G.cpu(), R.cpu()))
            kk.drop_ublk()
            out[i] = res

        try:
            if stream is None:
                work()
            else:
                with torch.cuda.stream(stream):
                    work()
                stream.synchronize()
        except BaseException as exc:  # noqa: BLE001 - reported by the main thread
            out[i] = exc

    for _, n, m in shapes:
        assert _jobs_per_phase(n, m)[1] == 1
    with _option("slice_len", SLICE), _option("gram_reg_cols", PER_JOB):
        want = [None, None]
        for i, (seed, n, m) in enumerate(shapes):
            run(seed, n, m, want, i)
    with _option("slice_len", SLICE), _option("gram_reg_cols", PERSISTENT):
        seq, par = [None, None], [None, None]
        for i, (seed, n, m) in enumerate(shapes):
            run(seed, n, m, seq, i)
        threads = [threading.Thread(target=run, args=(seed, n, m, par, i, torch.cuda.Stream(device=DEV)))
                   for i, (seed, n, m) in enumerate(shapes)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    for w, a, b in zip(want, seq, par):
        assert not any(isinstance(x, BaseException) for x in (w, a, b)), (w, a, b)
        for (Gw, Rw), (Ga, Ra), (Gb, Rb) in zip(w, a, b):
            assert torch.equal(Ga, Gw) and torch.equal(Ra, Rw)
            assert torch.equal(Gb, Gw) and torch.equal(Rb, Rw)
