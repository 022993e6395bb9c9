"""The calling-convention modes of tests/_kernel_scaffold.py on ``cuda:0``: two controls which show that the side-stream mode
bites - a torch operation and a library launch, both issued on the null stream while the inputs are in flight on the side
stream, do NOT see the data -, the calibration of its delay, and the convention tests of the four small entry points no kernel
module calls raw (``mvf_sym_pack``, ``mvf_sym_unpack``, ``mvf_lincomb3``, ``mvf_quadform``) with their plain references.

The controls use float data only and no index input: whatever a launch on the wrong stream reads, it addresses nothing out of
range."""
import numpy as np
import pytest
import torch

import _kernel_scaffold as ks

pytestmark = pytest.mark.gpu
M = 97   # 97 rows: one partial block of 256 lanes per row


@pytest.fixture(scope="module")
def lib():
    from spateo_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    mine = [e for e in ks.convention.log if "test_gpu_abi_conventions" in e["test"]]
    if not mine:
        return
    print(f"\nside stream: candidate {ks._side['attempt']} runs beside the null stream; {ks.cycles_per_ms():.4g} _sleep cycles per ms; "
          f"{len(mine)} blocks, longest plain call {max(e['plain_ms'] for e in mine):.1f} ms, longest delay "
          f"{max(e['delay_ms'] for e in mine):.0f} ms, blocks that saw the delay over: {sum(any(e['completed']) for e in mine)}")


def _sym(seed=5):
    a = np.random.default_rng(seed).standard_normal((M, M))
    return a + a.T


def _pack(lib, G, null_stream=False):
    Gd, tri = ks.dev(G), ks.guarded(M * (M + 1) // 2)
    rc = lib.mvf_sym_pack(ks.ptr(Gd), M, ks.ptr(tri), None if null_stream else ks.stream())
    assert rc == 0, lib.mvf_last_error()
    ks.called()
    torch.cuda.synchronize()
    assert ks.intact(tri, M * (M + 1) // 2)
    return tri[: M * (M + 1) // 2].cpu().numpy()


def _unpack(lib, tri):
    td, G = ks.dev(tri), ks.Out(M, M)
    rc = lib.mvf_sym_unpack(ks.ptr(td), M, G.ptr, ks.stream())
    assert rc == 0, lib.mvf_last_error()
    ks.called()
    torch.cuda.synchronize()
    assert G.guards_intact()
    return G.host()


def _lincomb3(lib, a, A, b, B, c, C):
    out = ks.Out(len(A))
    Ad, Bd, Cd = ks.dev(A), None if B is None else ks.dev(B), None if C is None else ks.dev(C)
    rc = lib.mvf_lincomb3(out.ptr, a, ks.ptr(Ad), b, ks.ptr(Bd), c, ks.ptr(Cd), len(A), ks.stream())
    assert rc == 0, lib.mvf_last_error()
    ks.called()
    torch.cuda.synchronize()
    assert out.guards_intact()
    return out.host()


def _quadform(lib, K, C):
    m, nrhs = C.shape
    Kd, Cd, out, scratch = ks.dev(K), ks.dev(C), ks.Out(1), ks.Out(m)
    rc = lib.mvf_quadform(ks.ptr(Kd), ks.ptr(Cd), m, nrhs, out.ptr, scratch.ptr, ks.stream())
    assert rc == 0, lib.mvf_last_error()
    ks.called()
    torch.cuda.synchronize()
    assert out.guards_intact() and scratch.guards_intact()
    return out.host()


def _cases(lib):
    rng = np.random.default_rng(11)
    G = _sym()
    iu = np.triu_indices(M)
    A, B, C = rng.standard_normal((3, 1001))
    K, Cm = _sym(7), rng.standard_normal((M, 3))
    lin = 0.25 * A + -3.0 * B + 1.5 * C
    return {
        "mvf_sym_pack": (lambda: _pack(lib, G), lambda got: ks.same_bits(got, G[iu])),
        "mvf_sym_unpack": (lambda: _unpack(lib, G[iu]), lambda got: ks.same_bits(got, G)),
        # (at most 3 roundings on the device, fused or not, and 5 in NumPy's, each half an ulp of a number below S = sum |terms|)
        "mvf_lincomb3": (lambda: _lincomb3(lib, 0.25, A, -3.0, B, 1.5, C),
                         lambda got: (np.abs(got - lin) <= 8 * 2.0 ** -53 * (0.25 * np.abs(A) + 3.0 * np.abs(B) + 1.5 * np.abs(C))).all()),
        "mvf_lincomb3:A-only": (lambda: _lincomb3(lib, 0.25, A, 0.0, None, 0.0, None), lambda got: ks.same_bits(got, 0.25 * A)),
        # (M * 3 M products of numbers below 16 each, summed in some order: n eps sum |terms|)
        "mvf_quadform": (lambda: _quadform(lib, K, Cm),
                         lambda got: abs(got[0] - np.einsum("ik,ij,jk", Cm, K, Cm))
                         <= 3 * M * M * 2.0 ** -52 * np.einsum("ik,ij,jk", np.abs(Cm), np.abs(K), np.abs(Cm))),
    }


CONVENTION_COVERS = {"mvf_sym_pack": ks.MODES, "mvf_sym_unpack": ks.MODES, "mvf_lincomb3": ks.MODES, "mvf_quadform": ks.MODES}


@pytest.mark.parametrize("mode", ks.MODES)
@pytest.mark.parametrize("entry", ["mvf_sym_pack", "mvf_sym_unpack", "mvf_lincomb3", "mvf_lincomb3:A-only", "mvf_quadform"])
def test_calling_conventions(lib, entry, mode):
    call, right = _cases(lib)[entry]
    plain, got = ks.under(mode, call)
    assert right(plain)
    assert ks.same_bits(plain, got)


def test_the_delay_is_calibrated_and_outlasts_its_floor():
    """One _sleep of the floor's length, timed with events: within a factor 2 of the floor (the calibration holds), and the
    event behind it is not complete right after the enqueue."""
    cycles = int(ks.DELAY_FLOOR_MS * ks.cycles_per_ms())
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    early = b.query()
    b.synchronize()
    ms = a.elapsed_time(b)
    print(f"_sleep: {ks.cycles_per_ms():.4g} cycles per ms; a delay of {ks.DELAY_FLOOR_MS} ms took {ms:.2f} ms")
    assert not early and 0.5 * ks.DELAY_FLOOR_MS <= ms <= 2.0 * ks.DELAY_FLOOR_MS


def test_control_a_torch_operation_on_the_default_stream_sees_no_data():
    """The side stream does not order against the null stream, and the delay outlasts the enqueue: ``live * 1`` on the default
    stream, complete on the host while the copy into ``live`` still waits behind the delay, is not the data - and ``live`` is,
    once the block is over."""
    data = np.random.default_rng(2).standard_normal(4099)

    def op():
        live = ks.dev(data)
        with torch.cuda.stream(torch.cuda.default_stream(ks.DEV)):
            seen = live * 1
            done = torch.cuda.Event()
            done.record()
        done.synchronize()
        ks.called()
        return live, seen

    (_, plain), seconds = ks.timed(op)   # (first, as everywhere: the first use of a kernel loads it and waits for the device)
    assert ks.same_bits(plain.cpu().numpy(), data)
    with ks.convention("side_stream", seconds) as mode:
        live, seen = op()
    assert mode.completed == [False]
    assert not np.array_equal(seen.cpu().numpy(), data)
    assert ks.same_bits(live.cpu().numpy(), data)


def test_control_a_library_launch_on_the_null_stream_is_detected(lib):
    """``mvf_sym_pack(G, m, tri, NULL)`` while G is in flight on the side stream: the launch runs at once on the null stream,
    and the sentinel fill of ``tri``, behind the delay, overwrites what it wrote.  The same helper on the side stream gives
    the plain call's bits."""
    G = _sym(13)
    plain, seconds = ks.timed(lambda: _pack(lib, G))
    with ks.convention("side_stream", seconds) as mode:
        wrong = _pack(lib, G, null_stream=True)
    assert mode.completed == [False]
    assert not ks.same_bits(wrong, plain)
    with ks.convention("side_stream", seconds):
        assert ks.same_bits(_pack(lib, G), plain)
