"""Scaffolding of every kernel-level GPU test module (tests/test_gpu_*_kernels.py and the host-level modules that need a piece of
it): the cached ``HipKernels`` per cell dtype, guarded buffers and their checks, the bit comparisons, the developer-option block
and the table of largest deviations.

What belongs here: anything two kernel test modules need that knows nothing about an entry point of the library.  What does not:
raw calls of one entry point, reference restatements and case builders stay in that entry point's module or case file, and what
only the alignment path shares lives in tests/_align_kernel_scaffold.py.  No test module imports another one.

Nothing here registers a fixture globally, and every function that allocates takes ``device`` (default: DEV), so that
tests/test_kernel_scaffold.py proves on the CPU that the guards and the bit comparisons bite."""
import time

import numpy as np
import pytest
import torch

DEV = "cuda:0"
DTYPES = ["float64", "float32"]
GUARD = 4096        # sentinel elements behind every one-sided buffer, and either side of an Out
GUARD_BYTES = 4096  # sentinel bytes either side of a Ws (keeps the 256-byte alignment of the workspace)
WS_FILL = 0xA5
SENTINEL = {torch.float64: -1.2345e300, torch.float32: -1.2345e30, torch.uint8: 0xA5, torch.int32: -12345,
            torch.int64: -1234567890123}


def fresh_kernels(dtype):
    """A new ``HipKernels`` of the cell dtype: no kernel-value cache, no workspace, no earlier decomposition."""
    from spateo_amd._kernels import HipKernels

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels(DEV, dtype)


def kernel_cache():
    """``k(dtype="float64")`` of one test module: its own cached ``HipKernels`` per cell dtype (``k.cache``).  The cache is per
    module because an instance owns state the tests read: the kernel-value cache, the Gram workspace and the solver workspaces."""
    cache = {}

    def k(dtype="float64"):
        if dtype not in cache:
            cache[dtype] = fresh_kernels(dtype)
        return cache[dtype]

    k.cache = cache
    return k


def dev(a, tdtype=torch.float64, device=DEV):
    """A host array on the device as ``tdtype`` (None: its own dtype)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if tdtype is None else t.to(tdtype)).to(device)


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def x4(a, dtype, device=DEV):
    """(n, d <= 4) host coordinates as (n, 4) rows of the NumPy ``dtype``, the other components zero, without ``to_x4``."""
    a = np.asarray(a)
    buf = np.zeros((len(a), 4), dtype=dtype)
    buf[:, :a.shape[1]] = a
    return torch.from_numpy(buf).to(device)


# ------------------------------------------------------------------------------------------------------ one-sided buffers
def guarded(n, tdtype=torch.float64, fill=None, device=DEV):
    """n live elements and GUARD more, all holding the sentinel (``fill``: the live ones hold it instead)."""
    buf = torch.full((n + GUARD,), SENTINEL[tdtype], dtype=tdtype, device=device)
    if fill is not None:
        buf[:n] = fill
    return buf


def intact(buf, n):
    return bool((buf[n:] == SENTINEL[buf.dtype]).all())


def written(buf, n):
    return bool((buf[:n] != SENTINEL[buf.dtype]).all())


def take(buf, n):
    """The n live elements of a guarded output on the host; the guard must be untouched."""
    assert intact(buf, n), "wrote past the end of an output"
    return buf[:n].cpu().numpy()


def nan_workspace(nbytes, device=DEV):
    """A guarded workspace whose live bytes are NaN bit patterns: a kernel that reads workspace it did not write returns NaN."""
    assert nbytes % 8 == 0
    return guarded(nbytes // 8, fill=float("nan"), device=device)


# ------------------------------------------------------------------------------------------------------ two-sided objects
class Out:
    """An output buffer inside a larger tensor: GUARD sentinel elements either side, the payload sentinel-filled too."""

    def __init__(self, *shape, dtype=torch.float64, fill=None, device=DEV):
        self.sent = SENTINEL[dtype] if fill is None else fill
        n = int(np.prod(shape)) if shape else 1
        self.big = torch.full((n + 2 * GUARD,), self.sent, dtype=dtype, device=device)
        self.t = self.big[GUARD:GUARD + n].view(*shape)
        self.n = n

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.big[:GUARD] == self.sent).all()) and bool((self.big[GUARD + self.n:] == self.sent).all())

    def untouched(self):
        return bool((self.t == self.sent).all())

    def host(self):
        return self.t.cpu().numpy().copy()


class Ws:
    """A workspace of exactly `nbytes` inside GUARD_BYTES either side, everything filled with WS_FILL (`fill` for the payload)."""

    def __init__(self, nbytes, fill=WS_FILL, device=DEV):
        self.nbytes = int(nbytes)
        self.big = torch.full((self.nbytes + 2 * GUARD_BYTES,), WS_FILL, dtype=torch.uint8, device=device)
        if fill != WS_FILL:
            self.big[GUARD_BYTES:GUARD_BYTES + self.nbytes] = fill
        assert torch.device(device).type == "cpu" or self.big.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return self.big.data_ptr() + GUARD_BYTES

    def guards_intact(self):
        return bool((self.big[:GUARD_BYTES] == WS_FILL).all()) and bool((self.big[GUARD_BYTES + self.nbytes:] == WS_FILL).all())


# ------------------------------------------------------------------------------------------------------ bit comparisons
_INT = {8: np.int64, 4: np.int32, 2: np.int16, 1: np.uint8}
_TINT = {8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(_INT[a.dtype.itemsize])


def same_bits(a, b):
    """NumPy arrays of the same dtype, shape and bytes (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def bits_equal(a, b):
    """Torch tensors of the same dtype, shape and bytes (NaN payloads and the sign of zero included)."""
    it = _TINT[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ------------------------------------------------------------------------------------------------------ options, tables
class option:
    """A developer option of the library for the length of a block; restored on the way out."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        from spateo_amd import _lib

        self.old = _lib.debug_option(self.name, self.value)

    def __exit__(self, *exc):
        from spateo_amd import _lib

        _lib.debug_option(self.name, self.old)


def deviation_table(header, columns=3, footer=None, on_done=None):
    """(note, fixture) of one test module.  ``note(*key, value)`` keeps the largest value per key, which has one part per column
    of the table but the last.  The module-scoped autouse fixture - to be bound to a name of the module - runs ``on_done()`` when
    the module is done and prints the rows in sorted order under ``header``, then ``footer(seconds, notes)`` if there is one: the
    module's time on the clock, with the device idle, and the number of ``note`` calls."""
    worst, calls = {}, [0]

    def note(*args):
        *key, value = args
        assert len(key) == columns - 1, (header, args)
        worst[tuple(key)] = max(worst.get(tuple(key), 0.0), float(value))
        calls[0] += 1

    def report():
        t0 = time.perf_counter()
        yield
        if footer is not None and torch.cuda.is_available():
            torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        if on_done is not None:
            on_done()
        print(f"\n{header}\n" + "|---" * columns + "|")
        for key, v in sorted(worst.items()):
            print("| " + " | ".join(str(part) for part in key) + f" | {v:.3g} |")
        if footer is not None:
            print(footer(seconds, calls[0]))

    note.report = report  # the fixture's body, undecorated (tests/test_kernel_scaffold.py runs it by hand)
    return note, pytest.fixture(scope="module", autouse=True)(report)
