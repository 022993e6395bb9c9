"""Every launch and copy of ``csrc/`` goes to the stream of its entry point: a source check, on the CPU, of what include/mvf.h
promises in one line ("`stream` is a hipStream_t ... every call is asynchronous on it").  It reaches the launches no GPU test
can tell apart from correct ones: those behind a synchronisation point of a documented-blocking entry point, and those of
developer paths.

The scanner blanks comments and string literals, then takes every call of a watched name with a balanced-parenthesis parse of
its arguments (the launches span lines, and their arguments hold calls and casts of their own).  It asserts that

  - argument 5 of every ``hipLaunchKernelGGL`` is ``st`` or ``(hipStream_t)stream``,
  - so is the last argument of every ``hipMemcpyAsync``, ``hipMemsetAsync``, ``hipEventRecord``, ``hipMemcpyWithStream`` and
    ``hipStreamSynchronize``, and none of them leaves its last argument to the default (the null stream),
  - every ``st`` is a parameter or ``hipStream_t st = (hipStream_t)stream;`` and is assigned nowhere else,
  - there is no ``<<<`` launch,
  - every call that blocks the host is in ``BLOCKING`` below, by file, enclosing function and call, as often as stated there.

The last part of the module doctors a source string of its own and expects each fault with its line."""
import pathlib
import re

import pytest

CSRC = pathlib.Path(__file__).resolve().parents[1] / "spateo-release_amd" / "csrc"
STREAMS = ("st", "(hipStream_t)stream")
# name -> (position of the stream argument, number of arguments)
ON_STREAM = {"hipLaunchKernelGGL": (4, None), "hipMemcpyAsync": (4, 5), "hipMemsetAsync": (3, 4), "hipEventRecord": (1, 2),
             "hipMemcpyWithStream": (4, 5), "hipStreamSynchronize": (0, 1)}
BLOCKS = ("hipMemcpy", "hipMemset", "hipDeviceSynchronize", "hipEventSynchronize", "hipStreamSynchronize", "hipMemcpyWithStream",
          "hipStreamWaitEvent", "hipMemcpyDtoH", "hipMemcpyHtoD", "hipMemcpyDtoD", "hipMemcpy2D", "hipMemcpyPeer")
# (file, enclosing function, call) -> (how often, why it may block)
BLOCKING = {
    ("mvf_lib.hip", "mvf_read_back", "hipMemcpyWithStream"):
        (1, "mvf.h: 'blocking device -> host copy of a small status block on `stream`'"),
    ("mvf_heat.hip", "heat_read_status", "hipStreamSynchronize"):
        (1, "mvf.h: both heat entries 'read the device's status block every few batches and return when it has stopped: they block'"),
    ("mvf_heat.hip", "mvf_heat_grid", "hipStreamSynchronize"):
        (1, "mvf.h: 'they block' - out is complete when the host outputs sweeps, err and hit_max_itr are returned"),
    ("mvf_heat.hip", "mvf_heat_graph", "hipStreamSynchronize"):
        (1, "mvf.h: 'they block' - out is complete when the host outputs sweeps, err and hit_max_itr are returned"),
    ("mvf_minnorm.hip", "rb_sync", "hipStreamSynchronize"):
        (1, "mvf.h: the minimum-norm solves, mvf_lr_pivot_order and the low-rank mvf_pinv_diag read ranks and pivots back"),
    ("mvf_minnorm.hip", "lr_solve", "hipEventSynchronize"):
        (3, "developer option lr_timing: phase times on stderr"),
    ("mvf_minnorm.hip", "lr_solve", "hipMemcpy"):
        (2, "developer option lr_timing: sweep and section counters for the lines on stderr"),
}


def blank(src):
    """``src`` with comments and the insides of string and character literals replaced by spaces; newlines stay."""
    out, i, n = [], 0, len(src)
    while i < n:
        two = src[i:i + 2]
        if two == "//":
            j = src.find("\n", i)
            j = n if j < 0 else j
            out.append(" " * (j - i))
            i = j
        elif two == "/*":
            j = src.find("*/", i + 2)
            j = n if j < 0 else j + 2
            out.append(re.sub(r"[^\n]", " ", src[i:j]))
            i = j
        elif src[i] in "\"'":
            q, j = src[i], i + 1
            while j < n and src[j] != q and src[j] != "\n":
                j += 2 if src[j] == "\\" else 1
            out.append(q + " " * (j - i - 1) + q)
            i = j + 1
        else:
            out.append(src[i])
            i += 1
    return "".join(out)


def arguments(text, at):
    """Top-level arguments of the call whose ``(`` is ``text[at]``, white space squeezed out, or None if it never closes."""
    depth, args, start = 0, [], at + 1
    for i in range(at, len(text)):
        c = text[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                last = text[start:i]
                if args or last.strip():
                    args.append(last)
                return ["".join(a.split()) for a in args]
        elif c == "," and depth == 1:
            args.append(text[start:i])
            start = i + 1
    return None


_HEADER = re.compile(r"^[A-Za-z_].*?\b(?!__launch_bounds__|__attribute__|alignas)([A-Za-z_]\w*)\s*\(", re.M)


def enclosing(text, at):
    """Name of the function around ``text[at]``: the last line in front that starts in column 0 and opens a parameter list."""
    name = "?"
    for m in _HEADER.finditer(text, 0, at):
        name = m.group(1)
    return name


def scan(file, src):
    """(findings, blocking): findings are (file, line, function, what); blocking counts (file, function, call)."""
    text = blank(src)
    findings, blocking = [], {}

    def line(at):
        return text.count("\n", 0, at) + 1

    for m in re.finditer(r"<<<", text):
        findings.append((file, line(m.start()), enclosing(text, m.start()), "a <<< launch"))
    for m in re.finditer(r"\b(hip[A-Z]\w*)\s*\(", text):
        name, at = m.group(1), m.end() - 1
        if name not in ON_STREAM and name not in BLOCKS:
            continue
        fn, args = enclosing(text, at), arguments(text, at)
        if args is None:
            findings.append((file, line(at), fn, f"{name}: unbalanced call"))
            continue
        if name in ON_STREAM:
            pos, count = ON_STREAM[name]
            if len(args) <= pos or (count is not None and len(args) != count):
                findings.append((file, line(at), fn, f"{name} with {len(args)} arguments: its stream is left to the default"))
            elif args[pos] not in STREAMS:
                findings.append((file, line(at), fn, f"{name} on '{args[pos]}', not on the stream of the call"))
        if name in BLOCKS:
            key = (file, fn, name)
            blocking.setdefault(key, []).append(line(at))
    for m in re.finditer(r"\bhipStream_t\s+st\b\s*([^\s])([^;\n]*)", text):
        if m.group(1) in ",)":
            continue  # a parameter
        if m.group(1) + m.group(2).rstrip() != "= (hipStream_t)stream":
            findings.append((file, line(m.start()), enclosing(text, m.start()), "st defined as something else than the stream"))
    for m in re.finditer(r"(?<![\w.>])st\s*=(?!=)", text):
        before = text[max(0, m.start() - 40):m.start()]
        if not re.search(r"\b(hipStream_t|int|unsigned)\s+$", before):  # (a loop counter of a kernel may be called st)
            findings.append((file, line(m.start()), enclosing(text, m.start()), "st assigned"))
    return findings, blocking


def sources():
    files = sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("*.h")))
    assert len(files) >= 20, files
    return files


def scan_all():
    findings, blocking, launches = [], {}, 0
    for f in sources():
        src = f.read_text()
        found, blocks = scan(f.name, src)
        findings += found
        blocking.update(blocks)
        launches += len(re.findall(r"\bhipLaunchKernelGGL\s*\(", blank(src)))
    return findings, blocking, launches


def test_every_launch_copy_and_event_is_on_the_stream_of_its_call():
    findings, _, launches = scan_all()
    assert launches >= 231   # the scanner sees the launches at all
    assert not findings, "\n".join(f"{f}:{ln} in {fn}: {what}" for f, ln, fn, what in findings)


def test_every_blocking_call_is_listed_with_its_reason():
    _, blocking, _ = scan_all()
    unlisted = {k: v for k, v in blocking.items() if k not in BLOCKING}
    assert not unlisted, f"blocking calls outside the list (file, function, call -> lines): {unlisted}"
    for key, (count, reason) in BLOCKING.items():
        assert reason and len(blocking.get(key, [])) == count, (key, blocking.get(key), "listed as", count)


def test_the_timing_blocks_are_behind_the_developer_option():
    """The two blocking copies and the event waits of mvf_minnorm.hip run under `timing` alone."""
    text = blank((CSRC / "mvf_minnorm.hip").read_text())
    lines = text.split("\n")
    _, blocking = scan("mvf_minnorm.hip", text)
    for (_, fn, name), at in blocking.items():
        if name == "hipStreamSynchronize":
            continue
        for ln in at:
            indent = len(lines[ln - 1]) - len(lines[ln - 1].lstrip())
            guard = next(l for l in reversed(lines[:ln - 1])
                         if l.strip() and not l.startswith("#") and len(l) - len(l.lstrip()) < indent)
            assert "timing" in guard, (fn, name, ln, guard)


# ---- the scanner bites ----
GOOD = '''#include "mvf_common.h"
// hipMemcpy(a, b, n) in a comment, and <<<1, 2>>> too
static void helper(hipStream_t st, double* p, int64_t n) {
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, p,
                       f(n, 3),
                       n);
    const char* msg = "hipMemset(p, 0, n) in a string";
}
extern "C" int mvf_thing(double* p, double* q, int64_t n, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    MVF_CHECK_HIP(hipMemsetAsync(p, 0, (size_t)n * sizeof(double), st));
    hipLaunchKernelGGL((pair_kernel<double, 4>), dim3(g(n), 1), dim3(256), lds_bytes(n), (hipStream_t)stream, p, q, n);
    MVF_CHECK_HIP(hipMemcpyAsync(q, p, (size_t)n * sizeof(double),
                                 hipMemcpyDeviceToDevice, st));
    MVF_CHECK_HIP(hipEventRecord(ev[0], st));
    helper(st, p, n);
    return 0;
}
'''


def test_the_clean_sample_is_clean():
    assert scan("sample.hip", GOOD) == ([], {})
    assert arguments("f(a, g(b, c), (T)d)", 1) == ["a", "g(b,c)", "(T)d"] and arguments("f()", 1) == [] and arguments("f(a", 1) is None


@pytest.mark.parametrize("old, new, line, fn, what", [
    ("dim3(256), 0, st, p,", "dim3(256), 0, 0, p,", 4, "helper", "hipLaunchKernelGGL on '0'"),
    ("lds_bytes(n), (hipStream_t)stream, p", "lds_bytes(n), 0, p", 12, "mvf_thing", "hipLaunchKernelGGL on '0'"),
    ("hipMemcpyDeviceToDevice, st));", "hipMemcpyDeviceToDevice));", 13, "mvf_thing", "hipMemcpyAsync with 4 arguments"),
    ("sizeof(double), st));", "sizeof(double)));", 11, "mvf_thing", "hipMemsetAsync with 3 arguments"),
    ("hipEventRecord(ev[0], st)", "hipEventRecord(ev[0])", 15, "mvf_thing", "hipEventRecord with 1 arguments"),
    ("hipEventRecord(ev[0], st)", "hipEventRecord(ev[0], nullptr)", 15, "mvf_thing", "hipEventRecord on 'nullptr'"),
    ("st = (hipStream_t)stream;", "st = 0;", 10, "mvf_thing", "st defined as something else"),
    ("    helper(st, p, n);", "    st = other;\n    helper(st, p, n);", 16, "mvf_thing", "st assigned"),
    ("    helper(st, p, n);", "    fill_kernel<<<1, 256, 0, st>>>(p, n);", 16, "mvf_thing", "a <<< launch"),
], ids=["launch-0", "cast-launch-0", "copy-dropped", "memset-dropped", "event-dropped", "event-null", "st-zero", "st-assigned",
        "chevrons"])
def test_a_doctored_stream_is_reported_with_its_line(old, new, line, fn, what):
    assert GOOD.count(old) == 1
    findings, blocking = scan("sample.hip", GOOD.replace(old, new))
    assert len(findings) == 1 and not blocking, findings
    assert findings[0][:3] == ("sample.hip", line, fn) and findings[0][3].startswith(what), findings


@pytest.mark.parametrize("call", ["hipMemcpy(q, p, 8, hipMemcpyDeviceToDevice)", "hipDeviceSynchronize()", "hipMemset(p, 0, 8)",
                                  "hipEventSynchronize(ev[0])", "hipStreamSynchronize(st)"])
def test_an_added_blocking_call_is_reported_with_its_line(call):
    name = call[:call.index("(")]
    findings, blocking = scan("sample.hip", GOOD.replace("    helper(st, p, n);", f"    (void){call};"))
    assert not findings and blocking == {("sample.hip", "mvf_thing", name): [16]}
    assert ("sample.hip", "mvf_thing", name) not in BLOCKING
    findings, _ = scan("sample.hip", GOOD.replace("    helper(st, p, n);", "    hipStreamSynchronize(0);"))
    assert [f[1:] for f in findings] == [(16, "mvf_thing", "hipStreamSynchronize on '0', not on the stream of the call")]
