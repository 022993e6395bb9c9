"""The shared scaffold of the kernel-level tests (tests/_kernel_scaffold.py) on ``device="cpu"``: the guards bite at their first
and last element and not one element earlier, on either side where there are two; the bit comparisons tell apart what ``==``
does not; ``written`` sees one element left over; the deviation table keeps maxima and prints header, sorted rows and footer."""
import numpy as np
import pytest
import torch

import _kernel_scaffold as ks

SIZES = [1, 7, 4097]
TDTYPES = list(ks.SENTINEL)


def _other(tdtype):
    """A value that is not the sentinel of ``tdtype``."""
    return 1.5 if tdtype.is_floating_point else 3


def test_the_constants_every_module_relies_on():
    assert ks.GUARD == 4096 and ks.GUARD_BYTES == 4096 and ks.WS_FILL == 0xA5
    assert set(TDTYPES) == {torch.float64, torch.float32, torch.uint8, torch.int32, torch.int64}
    for tdtype, s in ks.SENTINEL.items():  # a tensor filled with the sentinel compares equal to it, and the sentinel is no NaN
        assert bool((torch.full((3,), s, dtype=tdtype) == s).all())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tdtype", TDTYPES, ids=str)
def test_one_sided_guard(tdtype, n):
    buf = ks.guarded(n, tdtype, device="cpu")
    assert buf.numel() == n + ks.GUARD and buf.dtype == tdtype
    assert ks.intact(buf, n) and not ks.written(buf, n)
    for at in (n, n + ks.GUARD - 1):  # the first and the last element of the guard
        buf = ks.guarded(n, tdtype, device="cpu")
        buf[at] = _other(tdtype)
        assert not ks.intact(buf, n)
        with pytest.raises(AssertionError):
            ks.take(buf, n)
    buf = ks.guarded(n, tdtype, device="cpu")
    buf[n - 1] = _other(tdtype)  # the last live element
    assert ks.intact(buf, n)
    got = ks.take(buf, n)
    assert got.shape == (n,) and got[n - 1] == _other(tdtype)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tdtype", TDTYPES, ids=str)
def test_written_sees_one_element_left_over(tdtype, n):
    buf = ks.guarded(n, tdtype, fill=_other(tdtype), device="cpu")
    assert ks.written(buf, n) and ks.intact(buf, n)
    for at in {0, n // 2, n - 1}:
        buf = ks.guarded(n, tdtype, fill=_other(tdtype), device="cpu")
        buf[at] = ks.SENTINEL[tdtype]
        assert not ks.written(buf, n)


def test_nan_workspace():
    ws = ks.nan_workspace(56, device="cpu")
    assert ws.numel() == 7 + ks.GUARD and bool(torch.isnan(ws[:7]).all()) and ks.intact(ws, 7)
    with pytest.raises(AssertionError):
        ks.nan_workspace(57, device="cpu")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tdtype", TDTYPES, ids=str)
def test_two_sided_output(tdtype, n):
    out = ks.Out(n, dtype=tdtype, device="cpu")
    assert out.t.shape == (n,) and out.guards_intact() and out.untouched()
    assert out.ptr == out.big.data_ptr() + ks.GUARD * out.big.element_size()  # the payload sits GUARD elements in
    for at in (ks.GUARD - 1, ks.GUARD + n, 0, 2 * ks.GUARD + n - 1):  # one element before, one behind, both far ends
        out = ks.Out(n, dtype=tdtype, device="cpu")
        out.big[at] = _other(tdtype)
        assert not out.guards_intact() and out.untouched()
    for at in (0, n - 1):
        out = ks.Out(n, dtype=tdtype, device="cpu")
        out.t[at] = _other(tdtype)
        assert out.guards_intact() and not out.untouched() and out.host()[at] == _other(tdtype)


def test_two_sided_output_shapes_and_fill():
    out = ks.Out(7, 3, device="cpu")
    assert out.t.shape == (7, 3) and out.n == 21 and out.host().shape == (7, 3)
    out.t[6, 2] = 0.0
    assert out.guards_intact() and not out.untouched()
    out = ks.Out(7, fill=0.0, device="cpu")  # a fill of the caller's: payload and guards hold it
    assert not out.big.any() and out.guards_intact() and out.untouched()
    out.big[ks.GUARD + 7] = ks.SENTINEL[torch.float64]
    assert not out.guards_intact()


@pytest.mark.parametrize("n", SIZES)
def test_two_sided_workspace(n):
    ws = ks.Ws(n, device="cpu")
    assert ws.nbytes == n and ws.ptr == ws.big.data_ptr() + ks.GUARD_BYTES and ws.guards_intact()
    for at in (ks.GUARD_BYTES - 1, ks.GUARD_BYTES + n, 0, 2 * ks.GUARD_BYTES + n - 1):
        ws = ks.Ws(n, device="cpu")
        ws.big[at] = 0
        assert not ws.guards_intact()
    for at in (0, n - 1):
        ws = ks.Ws(n, device="cpu")
        ws.big[ks.GUARD_BYTES + at] = 0
        assert ws.guards_intact()
    ws = ks.Ws(n, fill=0, device="cpu")
    assert ws.guards_intact() and not ws.big[ks.GUARD_BYTES:ks.GUARD_BYTES + n].any()
    assert bool((ws.big[:ks.GUARD_BYTES] == ks.WS_FILL).all()) and bool((ws.big[ks.GUARD_BYTES + n:] == ks.WS_FILL).all())


def _nan(payload, np_dtype):
    if np_dtype == np.float64:
        return np.array([0x7FF8000000000000 | payload], dtype=np.uint64).view(np.float64)
    return np.array([0x7FC00000 | payload], dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("np_dtype", [np.float64, np.float32])
def test_bit_comparisons(np_dtype):
    def both(a, b):
        r = ks.same_bits(a, b)
        assert ks.bits_equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b))) == r
        return r

    x = np.array([1.0, 0.0, -2.5], dtype=np_dtype)
    assert both(x, x.copy())
    z = x.copy()
    z[1] = -0.0
    assert np.array_equal(x, z) and not both(x, z)  # the sign of zero counts
    n1, n2 = _nan(1, np_dtype), _nan(2, np_dtype)
    assert np.isnan(n1).all() and np.isnan(n2).all()
    assert both(n1, n1.copy()) and not both(n1, n2)  # the same NaN twice; two payloads
    other = np.float32 if np_dtype == np.float64 else np.float64
    assert np.array_equal(x, x.astype(other)) and not both(x, x.astype(other))  # equal values, another dtype
    assert not both(x, x.reshape(3, 1)) and not both(x, x[:2])  # another shape
    assert both(x.reshape(3, 1)[::-1], x[::-1].reshape(3, 1))  # strides do not count
    assert ks.bits(x).dtype.itemsize == x.dtype.itemsize and ks.bits(x).dtype.kind in "iu"


def test_bit_comparisons_of_integers():
    for np_dtype in (np.int32, np.int64, np.uint8):
        a = np.array([1, 2, 3], dtype=np_dtype)
        assert ks.same_bits(a, a.copy()) and ks.bits_equal(torch.from_numpy(a), torch.from_numpy(a.copy()))
        b = a.copy()
        b[2] = 4
        assert not ks.same_bits(a, b) and not ks.bits_equal(torch.from_numpy(a), torch.from_numpy(b))


def test_small_helpers():
    t = ks.dev(np.arange(6, dtype=np.int64).reshape(2, 3)[:, ::2], device="cpu")
    assert t.dtype == torch.float64 and t.is_contiguous() and t.tolist() == [[0.0, 2.0], [3.0, 5.0]]
    assert ks.dev(np.arange(3, dtype=np.int16), None, device="cpu").dtype == torch.int16
    assert ks.dev(np.arange(3), torch.int32, device="cpu").dtype == torch.int32
    assert ks.ptr(None) is None and ks.ptr(t) == t.data_ptr()
    for dtype, tdtype in ((np.float32, torch.float32), ("float64", torch.float64)):
        for a in (np.arange(6.0).reshape(2, 3), np.arange(4.0).reshape(2, 2), np.zeros((0, 3))):
            x = ks.x4(a, dtype, device="cpu")
            d = a.shape[1]
            assert x.shape == (len(a), 4) and x.dtype == tdtype
            assert np.array_equal(x.numpy()[:, :d], a) and not x[:, d:].any()


def test_deviation_table(capsys):
    done = []
    note, fixture = ks.deviation_table("| a | b | worst |", footer=lambda s, n: f"took {s >= 0}, {n} notes",
                                       on_done=lambda: done.append(1))
    note("y", "float64", 1.0)
    note("x", "float32", 0.25)
    note("y", "float64", 3.0)
    note("y", "float64", 2.0)
    note("x", "float64", 1e-9)
    with pytest.raises(AssertionError):
        note("x", 1.0)  # one key part short of the header
    gen = note.report()
    next(gen)
    assert not done
    with pytest.raises(StopIteration):
        next(gen)
    assert done == [1]
    assert capsys.readouterr().out == ("\n| a | b | worst |\n|---|---|---|\n| x | float32 | 0.25 |\n| x | float64 | 1e-09 |\n"
                                       "| y | float64 | 3 |\ntook True, 5 notes\n")


def test_deviation_table_with_another_arity(capsys):
    note, fixture = ks.deviation_table("| a | b | c | worst |x| |", columns=4)
    note("p", "q", "r", 0.5)
    note("p", "q", "a", 2)
    gen = note.report()
    next(gen)
    with pytest.raises(StopIteration):
        next(gen)
    assert capsys.readouterr().out == "\n| a | b | c | worst |x| |\n|---|---|---|---|\n| p | q | a | 2 |\n| p | q | r | 0.5 |\n"


# ---- calling conventions (the side stream needs a device: tests/test_gpu_kernels.py holds its controls) ----
def _start(t):
    """Address of the first byte of the allocation a tensor lives in."""
    return t.untyped_storage().data_ptr()


def test_outside_any_mode_pointers_sit_at_the_allocation_start():
    assert ks.convention.active is None and ks.MODES == ("side_stream", "displaced", "inputs")
    t = ks.dev(np.arange(6.0).reshape(2, 3), device="cpu")
    x = ks.x4(np.arange(6.0).reshape(2, 3), np.float32, device="cpu")
    g = ks.guarded(7, torch.int32, device="cpu")
    assert t.data_ptr() == _start(t) and t.shape == (2, 3) and t.dtype == torch.float64 and t._base is None
    assert x.data_ptr() == _start(x) and x.shape == (2, 4) and x.dtype == torch.float32
    assert g.data_ptr() == _start(g) and g.shape == (7 + ks.GUARD,) and g.dtype == torch.int32
    out, ws = ks.Out(7, 3, device="cpu"), ks.Ws(24, device="cpu")
    assert out.ptr == _start(out.big) + ks.GUARD * 8 and out.big.numel() == 21 + 2 * ks.GUARD
    assert ws.ptr == _start(ws.big) + ks.GUARD_BYTES and ws.big.numel() == 24 + 2 * ks.GUARD_BYTES
    ks.called()  # a no-op


@pytest.mark.parametrize("tdtype", TDTYPES, ids=str)
def test_displaced_pointers_start_one_unit_in_and_the_guards_still_bite(tdtype):
    n, size = 7, torch.empty(0, dtype=tdtype).element_size()
    with ks.convention("displaced"):
        t = ks.dev(np.arange(6).reshape(2, 3), tdtype, device="cpu")
        wide = ks.dev(np.arange(6), tdtype, device="cpu", unit=4)   # a pointer with a stated alignment of 4 elements
        assert t.data_ptr() == _start(t) + size and t.shape == (2, 3) and t.flatten().tolist() == list(range(6))
        assert wide.data_ptr() == _start(wide) + 4 * size
        buf = ks.guarded(n, tdtype, device="cpu")
        assert buf.data_ptr() == _start(buf) + size and buf.numel() == n + ks.GUARD and ks.intact(buf, n)
        for at in (-1, n, n + ks.GUARD - 1):    # the element in front, the first and the last one behind
            buf = ks.guarded(n, tdtype, device="cpu")
            buf._base[1 + at] = _other(tdtype)
            assert not ks.intact(buf, n)
            with pytest.raises(AssertionError):
                ks.take(buf, n)
        buf = ks.guarded(n, tdtype, fill=_other(tdtype), device="cpu")
        assert ks.written(buf, n) and ks.intact(buf, n) and ks.take(buf, n).tolist() == [_other(tdtype)] * n
        out = ks.Out(n, dtype=tdtype, device="cpu")
        assert out.ptr == _start(out.big) + (ks.GUARD + 1) * size and out.guards_intact() and out.untouched()
        for at in (ks.GUARD, ks.GUARD + 1 + n, 0, 2 * ks.GUARD + n):
            out = ks.Out(n, dtype=tdtype, device="cpu")
            out.big[at] = _other(tdtype)
            assert not out.guards_intact() and out.untouched()
        for at in (0, n - 1):
            out = ks.Out(n, dtype=tdtype, device="cpu")
            out.t[at] = _other(tdtype)
            assert out.guards_intact() and not out.untouched()
    assert ks.convention.active is None and ks.guarded(n, tdtype, device="cpu").storage_offset() == 0


def test_displaced_rows_and_workspaces_keep_their_alignment():
    with ks.convention("displaced"):
        for dtype, row in ((np.float32, 16), (np.float64, 32)):
            x = ks.x4(np.arange(6.0).reshape(2, 3), dtype, device="cpu")
            assert x.data_ptr() == _start(x) + row and x.shape == (2, 4) and x[1].tolist() == [3.0, 4.0, 5.0, 0.0]
        ws = ks.Ws(24, device="cpu")
        assert ws.ptr == _start(ws.big) + ks.GUARD_BYTES + ks.WS_ALIGN and ws.guards_intact()
        for at in (ks.GUARD_BYTES + ks.WS_ALIGN - 1, ks.GUARD_BYTES + ks.WS_ALIGN + 24, 0, 2 * ks.GUARD_BYTES + ks.WS_ALIGN + 23):
            ws = ks.Ws(24, device="cpu")
            ws.big[at] = 0
            assert not ws.guards_intact()
        for at in (0, 23):
            ws = ks.Ws(24, device="cpu")
            ws.big[ks.GUARD_BYTES + ks.WS_ALIGN + at] = 0
            assert ws.guards_intact()
        buf = ks.guarded(24, device="cpu", unit=32)   # a workspace of doubles held in a one-sided buffer
        assert buf.data_ptr() == _start(buf) + 256 and ks.intact(buf, 24)
        buf._base[31] = 0.0
        assert not ks.intact(buf, 24)


@pytest.mark.parametrize("mode", ["inputs", "displaced"])
def test_a_changed_input_is_caught_to_the_bit(mode):
    with ks.convention(mode):
        a = ks.dev(np.array([1.0, 0.0, -2.5]), device="cpu")
        x = ks.x4(np.ones((2, 3)), np.float32, device="cpu")
        io = ks.dev(np.arange(3), torch.int32, device="cpu", inout=True)
        io[1] = 7     # not const in the header: the call may write it
    for flip in ("sign of zero", "one mantissa bit", "padding of a row"):
        with pytest.raises(ks.ConventionError, match="changed its input number"):
            with ks.convention(mode):
                a = ks.dev(np.array([1.0, 0.0, -2.5]), device="cpu")
                x = ks.x4(np.ones((2, 3)), np.float32, device="cpu")
                if flip == "sign of zero":
                    a[1] = -0.0
                elif flip == "one mantissa bit":
                    a.view(torch.int64)[2] ^= 1
                else:
                    x.view(torch.int32)[1, 3] ^= 1
    with pytest.raises(ZeroDivisionError):   # an exception of the block passes through, and the mode ends
        with ks.convention(mode):
            1 / 0
    assert ks.convention.active is None


def test_under_runs_plain_first_then_the_mode():
    seen = []

    def fn():
        seen.append(None if ks.convention.active is None else ks.convention.active.mode)
        return ks.dev(np.arange(3.0), device="cpu").data_ptr() % 8

    assert ks.under("displaced", fn) == (0, 0) and seen == [None, "displaced"]
    with pytest.raises(AssertionError):
        ks.convention("sideways")


def test_watched_tensors_must_keep_their_bits():
    t = torch.arange(5, dtype=torch.float64)
    ks.watch(t)                      # outside a block: nothing is kept
    t[0] = 7.0
    with ks.convention("inputs"):
        ks.watch(t, None)
        ks.called()                  # outside the side stream: no-ops, whatever the entry point is
        ks.called(synchronising=True)
    with pytest.raises(ks.ConventionError, match="changed its input number 0"):
        with ks.convention("inputs"):
            ks.watch(t)
            t[4] = -t[4]
