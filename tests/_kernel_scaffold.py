"""Scaffolding of every kernel-level GPU test module (tests/test_gpu_*_kernels.py and the host-level modules that need a piece of
it): the cached ``HipKernels`` per cell dtype, guarded buffers and their checks, the bit comparisons, the developer-option block,
the table of largest deviations, and the calling-convention modes (``convention``: the same raw helper on a side stream behind
in-flight inputs, at displaced pointers, and with its inputs checked for change; tests/test_abi_conventions_ledger.py keeps the
list of entry points that run under them).

What belongs here: anything two kernel test modules need that knows nothing about an entry point of the library.  What does not:
raw calls of one entry point, reference restatements and case builders stay in that entry point's module or case file, and what
only the alignment path shares lives in tests/_align_kernel_scaffold.py.  No test module imports another one.

Nothing here registers a fixture globally, and every function that allocates takes ``device`` (default: DEV), so that
tests/test_kernel_scaffold.py proves on the CPU that the guards and the bit comparisons bite."""
import os
import time

import numpy as np
import pytest
import torch

DEV = "cuda:0"
DTYPES = ["float64", "float32"]
GUARD = 4096        # sentinel elements behind every one-sided buffer, and either side of an Out
GUARD_BYTES = 4096  # sentinel bytes either side of a Ws (keeps the 256-byte alignment of the workspace)
WS_FILL = 0xA5
WS_ALIGN = 256      # the largest alignment a MVF_REQUIRE asks of a workspace
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


def dev(a, tdtype=torch.float64, device=DEV, inout=False, unit=1):
    """A host array on the device as ``tdtype`` (None: its own dtype).  ``inout``: the header does not declare it ``const``
    (``convention`` then leaves it out of the input check); ``unit``: elements by which ``convention("displaced")`` moves it -
    1 unless the header or a ``MVF_REQUIRE`` states an alignment for this pointer."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    t = t if tdtype is None else t.to(tdtype)
    return t.to(device) if convention.active is None else convention.active.input(t, device, inout, unit)


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def x4(a, dtype, device=DEV):
    """(n, d <= 4) host coordinates as (n, 4) rows of the NumPy ``dtype``, the other components zero, without ``to_x4``."""
    a = np.asarray(a)
    buf = np.zeros((len(a), 4), dtype=dtype)
    buf[:, :a.shape[1]] = a
    t = torch.from_numpy(buf)
    return t.to(device) if convention.active is None else convention.active.input(t, device, False, 4)


# ------------------------------------------------------------------------------------------------------ one-sided buffers
def guarded(n, tdtype=torch.float64, fill=None, device=DEV, unit=1):
    """n live elements and GUARD more, all holding the sentinel (``fill``: the live ones hold it instead).  Under
    ``convention("displaced")`` the buffer starts ``unit`` sentinel elements into its allocation (``unit`` as for ``dev``), and
    ``intact`` looks at those as well."""
    front = _displacement(unit)
    buf = torch.full((front + n + GUARD,), SENTINEL[tdtype], dtype=tdtype, device=device)[front:]
    if fill is not None:
        buf[:n] = fill
    return buf


def intact(buf, n):
    if not bool((buf[n:] == SENTINEL[buf.dtype]).all()):
        return False
    if buf._base is None or not buf.storage_offset():
        return True
    return bool((buf._base[:buf.storage_offset()] == SENTINEL[buf.dtype]).all())  # (displaced: the unit in front)


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

    def __init__(self, *shape, dtype=torch.float64, fill=None, device=DEV, unit=1):
        self.sent = SENTINEL[dtype] if fill is None else fill
        n = int(np.prod(shape)) if shape else 1
        self.at = GUARD + _displacement(unit)  # (displaced: one unit off the alignment that GUARD elements keep)
        self.big = torch.full((n + self.at + GUARD,), self.sent, dtype=dtype, device=device)
        self.t = self.big[self.at:self.at + n].view(*shape)
        self.n = n

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.big[:self.at] == self.sent).all()) and bool((self.big[self.at + self.n:] == self.sent).all())

    def untouched(self):
        return bool((self.t == self.sent).all())

    def host(self):
        return self.t.cpu().numpy().copy()


class Ws:
    """A workspace of exactly `nbytes` inside GUARD_BYTES either side, everything filled with WS_FILL (`fill` for the payload).
    ``convention("displaced")`` moves it by WS_ALIGN bytes, the largest alignment the library asks of a workspace."""

    def __init__(self, nbytes, fill=WS_FILL, device=DEV):
        self.nbytes = int(nbytes)
        self.at = GUARD_BYTES + _displacement(WS_ALIGN)
        self.big = torch.full((self.nbytes + self.at + GUARD_BYTES,), WS_FILL, dtype=torch.uint8, device=device)
        if fill != WS_FILL:
            self.big[self.at:self.at + self.nbytes] = fill
        assert torch.device(device).type == "cpu" or self.big.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return self.big.data_ptr() + self.at

    def guards_intact(self):
        return bool((self.big[:self.at] == WS_FILL).all()) and bool((self.big[self.at + self.nbytes:] == WS_FILL).all())


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


# ------------------------------------------------------------------------------------------------------ calling conventions
MODES = ("side_stream", "displaced", "inputs")
DELAY_FLOOR_MS = 30.0   # shortest delay in front of the inputs of a side-stream call
DELAY_FACTOR = 4.0      # x the host time of the same helper's plain call: its staging copies happen twice, and timer noise
_side = {}              # the side stream and the calibration of the delay kernel, once per process


class ConventionError(AssertionError):
    """A calling-convention mode found the call at fault, or could not protect it (the message says which)."""


def _displacement(unit):
    c = convention.active
    return int(unit) if c is not None and c.mode == "displaced" else 0


def cycles_per_ms():
    """Cycles of ``torch.cuda._sleep`` per millisecond on DEV, timed once per process with events around one sleep."""
    if "cycles_per_ms" not in _side:
        torch.cuda._sleep(1000)  # the first launch loads the kernel
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cycles = 20_000_000
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        _side["cycles_per_ms"] = cycles / a.elapsed_time(b)
    return _side["cycles_per_ms"]


def side_stream():
    """The side stream of the process: a ``torch.cuda.Stream`` that is shown not to order against the null stream.  Streams
    share the hardware queues of the process, and work on a stream that shares the null stream's queue runs in the order of its
    enqueue with work on the null stream - behind such a stream's delay a launch on the null stream would see the data after
    all.  So each candidate is probed: a 5 ms delay on it, a small operation on the null stream behind; the candidate is taken
    when that operation completes while the delay still runs."""
    if "stream" not in _side:
        default, cycles = torch.cuda.default_stream(DEV), int(5 * cycles_per_ms())
        with torch.cuda.stream(default):
            x = torch.zeros(64, device=DEV)
            for tdtype in SENTINEL:  # the first use of a torch kernel loads it, which waits for the device: not behind a delay
                torch.full((64,), 0, dtype=tdtype, device=DEV).copy_(torch.full((64,), 1, dtype=tdtype, device=DEV))
            for attempt in range(1, 33):
                S = torch.cuda.Stream(DEV)
                torch.cuda.synchronize()
                with torch.cuda.stream(S):
                    torch.cuda._sleep(cycles)
                    E = torch.cuda.Event()
                    E.record(S)
                x += 1
                D = torch.cuda.Event()
                D.record(default)
                while True:
                    d, e = D.query(), E.query()
                    if d or e:
                        break
                S.synchronize()
                if d and not e:
                    _side["stream"], _side["attempt"] = S, attempt
                    break
            else:
                raise ConventionError("none of 32 streams runs beside the null stream: the side-stream mode cannot bite here")
    return _side["stream"]


def timed(fn):
    """(fn(), its host wall time in seconds): the plain call in front of a ``convention("side_stream", seconds)`` one."""
    t0 = time.perf_counter()
    got = fn()
    return got, time.perf_counter() - t0


def called(synchronising=None):
    """A raw helper calls this between the library call and its own synchronisation.  Outside ``convention("side_stream")`` it
    does nothing; inside, it notes whether the delay in front of the inputs was over when the library call returned.
    ``synchronising``: whether include/mvf.h documents this entry point as synchronising its stream (None: as the block says)."""
    c = convention.active
    if c is not None and c.mode == "side_stream":
        done = bool(c.E.query())
        c.completed.append(done)
        if done and not (c.synchronising if synchronising is None else synchronising):
            c.too_short = True


def watch(*tensors):
    """Device tensors the caller made itself (``HipKernels`` allocations, say) and hands to the library as ``const``: under
    any ``convention`` they must come out of the block with the bits they have now."""
    c = convention.active
    if c is not None:
        c.inputs += [(t, t.clone()) for t in tensors if t is not None]


def settle():
    """``torch.cuda.synchronize()`` in front of a library call - but not under ``convention("side_stream")``, where waiting for
    the device would wait for the inputs, which is what that mode must not do."""
    c = convention.active
    if c is None or c.mode != "side_stream":
        torch.cuda.synchronize()


class convention:
    """``with convention(mode): got = _raw(...)``: the allocations of this scaffold and ``stream()`` follow one calling mode, so
    that an unchanged raw helper makes its library call under it; outside the block everything is as without it.

    "inputs"      ``dev`` and ``x4`` keep a copy of what they return, and on the way out every tensor must hold the copy's bits
                  (but those made with ``inout=True``: arguments the header does not declare ``const``).  The other two modes
                  check this as well.
    "displaced"   every pointer of ``dev``, ``x4``, ``guarded`` and ``Out`` starts one unit into (``Out``: off the alignment
                  of) its allocation - one row for ``x4``, one element otherwise, ``unit`` elements where the caller says that
                  the header states an alignment, WS_ALIGN bytes for a ``Ws`` -, the guards adjacent on both sides.
    "side_stream" a stream S that does not order against the null stream is current, with a delay kernel and an event E
                  behind it.  ``dev`` and ``x4`` stage their data on the default stream, wait for it on the host, and on S fill
                  the tensor they return with poison (NaN; integers 0, a valid index) and copy the data over it; outputs and
                  workspaces are filled on S as well, and ``stream()`` is S.  A launch that reads on another stream reads
                  poison or what the memory held before, never the data; one that writes there is overwritten by the fill.  S is synchronised on the way out.
                  ``called()`` notes ``E.query()``: False proves that every launch was enqueued while the inputs were poison.
                  True on an entry point the header calls asynchronous is an error of the test (the delay was too short), not
                  a pass; for one documented as synchronising (``synchronising=True``) the mode protects the launches up to
                  the first synchronisation only, and ``completed`` says so.  The delay is max(DELAY_FLOOR_MS, DELAY_FACTOR x
                  ``plain_seconds``); whenever an input is staged after E has completed, a new delay and a new E go in front."""
    active = None
    log = []  # one dict per side-stream block of the process (test, plain seconds, delay in ms, what called() saw), for reports

    def __init__(self, mode, plain_seconds=0.0, synchronising=False):
        assert mode in MODES, mode
        self.mode, self.synchronising, self.plain_seconds = mode, synchronising, plain_seconds
        self.delay_ms = max(DELAY_FLOOR_MS, DELAY_FACTOR * 1e3 * plain_seconds)
        self.inputs, self.completed, self.stages, self.too_short = [], [], [], False

    def __enter__(self):
        assert convention.active is None, "convention blocks do not nest"
        if self.mode == "side_stream":
            self.cycles = int(self.delay_ms * cycles_per_ms())
            self.S = side_stream()
            self.default = torch.cuda.default_stream(DEV)
            self.current = torch.cuda.stream(self.S)
            self.current.__enter__()
            self.arm()
        convention.active = self
        return self

    def arm(self):
        torch.cuda._sleep(self.cycles)
        self.E = torch.cuda.Event()
        self.E.record(self.S)

    def input(self, t, device, inout, unit):
        """The host tensor ``t`` on ``device`` under the mode."""
        front = int(unit) if self.mode == "displaced" else 0
        if self.mode == "side_stream":
            with torch.cuda.stream(self.default):
                stage = t.to(device)
                self.default.synchronize()
            if self.E.query():  # (a helper that synchronised and stages more: the next call is protected again)
                self.arm()
            live = torch.full((t.numel(),), float("nan") if t.is_floating_point() else 0, dtype=t.dtype, device=device)
            live = live.view(t.shape)
            live.copy_(stage, non_blocking=True)
            self.stages.append(stage)
            keep = stage
        else:
            big = torch.empty((front + t.numel(),), dtype=t.dtype, device=device)
            live = big[front:].view(t.shape)
            live.copy_(t)
            keep = live.clone()
        if not inout:
            self.inputs.append((live, keep))
        return live

    def __exit__(self, etype, evalue, tb):
        convention.active = None
        if self.mode == "side_stream":
            self.S.synchronize()
            self.current.__exit__(etype, evalue, tb)
            convention.log.append(dict(test=os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], plain_ms=1e3 * self.plain_seconds,
                                       delay_ms=self.delay_ms, completed=list(self.completed), too_short=self.too_short))
        if etype is not None:
            return False
        for i, (live, keep) in enumerate(self.inputs):
            if not bits_equal(live, keep):
                raise ConventionError(f"the call changed its input number {i}, {tuple(live.shape)} {live.dtype}")
        if self.mode == "side_stream":
            if not self.completed:
                raise ConventionError("the raw helper never called called(): nothing shows that the call was protected")
            if self.too_short:
                raise ConventionError(f"the delay of {self.delay_ms:.1f} ms was over when the library call returned: too short "
                                      "to protect an asynchronous entry point (an error of the test, not a result)")
        return False


def under(mode, fn, synchronising=False):
    """(plain, got): ``fn()`` plainly, timed, then under ``convention(mode)``."""
    plain, seconds = timed(fn)
    with convention(mode, seconds, synchronising):
        got = fn()
    return plain, got
