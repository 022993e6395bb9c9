"""Kernel-level edge tests of the fused assignment step (``csrc/mvf_assign.hip``) through the raw C ABI - ``mvf_assign_prepare``,
``mvf_assign``, ``mvf_assign_dense`` - on ``cuda:0`` in both cell dtypes, at the tile / wave / MFMA-block / k-step / split edges
where such kernels go wrong.  tests/_assign_edge_cases.py holds the inputs, the case lists and the NumPy references;
tests/test_assign_kernel_refs.py proves without a GPU that the references are right to 1e-12, that every case is well
conditioned and that each targeted off-by-one would move a compared quantity by >= 1e-7.

A  ``mvf_assign_prepare`` alone against ``prepare_reference``: euc operands bit for bit, pad features exactly 0, float64
   operands within 1e-13 max(1, |v|), float32 operands within one float32 ulp in at most 1e-3 of the elements, a / b within
   1e-12 of the value recomputed from the read-back operands.
B  The pair stage on the device's OWN operands: the prepared operands and coordinates are read back and fed to
   ``pair_reference``; every output within 1e-10 (``_assign_case.F64_TOL``) of the quantity's maximum in BOTH dtype modes (with
   the stored operands as input, float32 mode does the same float64 arithmetic).  Every call has a guard behind every
   output and behind the workspace, runs on a workspace filled with NaN bit patterns, and is made twice (same bits).
C  The dense variant at shapes whose tile edges cut P.
D  Workspace: NaN-filled against zero-filled, stale partials of a larger call, a larger workspace than needed; a non-default
   stream.
E  One representative per family through ``spateo_amd.align.update_assignment`` against the formula restatement, at the bounds
   of tests/test_gpu_assign.py.

No bound is fitted to what the device returned.  Run with ``-s`` for the largest deviation of every family
(profiles/assign_kernel_edges.md records them)."""
import numpy as np
import pytest
import torch

import _assign_case as ac
import _assign_edge_cases as ec
from _align_kernel_scaffold import assign as _assign, device_case, kernels as _k, prepare as _prepare, watch_case as _watch_case
from _kernel_scaffold import (DEV, DTYPES, deviation_table, guarded as _guarded, nan_workspace as _nan_workspace,
                              same_bits as _same_bits, under as _under)

pytestmark = pytest.mark.gpu

_note, _deviation_table = deviation_table("| case family | dtype | largest deviation |")


def _device_case(name, dtype):
    return device_case(name, lambda: ec.case(name), dtype)


CONVENTION_COVERS = {"mvf_assign": ("side_stream", "inputs"), "mvf_assign_dense": ("side_stream", "inputs")}


@pytest.mark.parametrize("mode", ["side_stream", "inputs"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dense", [False, True], ids=["mvf_assign", "mvf_assign_dense"])
@pytest.mark.parametrize("case", ["cells-65x65", "layers-2", "split-50x4417"])   # one tile pair; two layers; the split plan
def test_calling_conventions(case, dense, dtype, mode):
    """The plain call's bits with the call on a side stream - the case's operands are made when the case is built, so the
    outputs and the workspace, not the inputs, are in flight there: a launch on another stream is overwritten by their fill -,
    and with every operand unchanged by the call."""
    dc = _device_case(case, dtype)

    def call():
        _watch_case(dc)
        return _assign(dc, dense=dense)

    plain, got = _under(mode, call)
    assert sorted(plain) == sorted(got) and all(_same_bits(plain[q], got[q]) for q in plain)


# ------------------------------------------------------------------------------------------------------ A: prepare
def _ulps32(got, ref):
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", sorted(ec.METRICS))
def test_prepare_feature_sweep_both_sides(dtype, metric):
    k = _k(dtype)
    T = np.dtype(dtype).type
    rng = np.random.default_rng(11)
    worst, off, total, worst_ab = 0.0, 0, 0, 0.0
    for g in ec.PREPARE_GS:
        gp = 2 * g if metric == "sym_kl" else g
        for n in ec.PREPARE_NS:
            labels = rng.integers(0, 5, n)
            layer = (ec.counts_layer if metric in ("kl", "sym_kl") else ec.grid_layer)(rng, g, labels, 11)
            zero = 1 if n >= 3 else None   # one all-zero row among live ones
            if zero is not None:
                layer[zero] = 0.0
            for side in (0, 1):
                Lp, ab, ld = _prepare(k, layer, metric, side)
                got, gab = Lp.cpu().numpy(), ab.cpu().numpy()
                ref, rab = ec.prepare_reference(layer, metric, side, T)
                assert got.shape == ref.shape == (n, ld) and got.dtype == ref.dtype
                assert not got[:, gp:].any(), (g, n, side, "pad features")
                if metric in ("euc", "square_euc"):
                    assert np.array_equal(got, ref), (g, n, side)
                elif dtype == "float64":
                    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
                    worst = max(worst, float(err.max()))
                    assert err.max() <= ec.PREP_F64_TOL, (g, n, side, float(err.max()))
                else:
                    ulps = _ulps32(got[:, :gp], ref[:, :gp])
                    assert ulps.max() <= 1.0, (g, n, side, float(ulps.max()))
                    off, total = off + int((ulps > 0).sum()), total + ulps.size
                # a / b from the operands the device stored
                w = got.astype(np.float64)
                if metric in ("euc", "square_euc"):
                    want = (w * w).sum(1)
                elif metric == "cos":
                    want = np.full(n, 0.5 if side == 0 else 0.0)
                    assert np.array_equal(gab, want)
                else:
                    p = w[:, :g] if (side == 0) else (w[:, g:2 * g] if metric == "sym_kl" else None)
                    e = np.zeros(n) if p is None else (p * np.log(p + ec.EPS)).sum(1)
                    want = 0.5 * e if metric == "sym_kl" else e
                top = max(float(np.abs(want).max()), float(np.abs(rab).max()))
                if top > 0:
                    worst_ab = max(worst_ab, float(np.abs(gab - want).max() / top), float(np.abs(gab - rab).max() / top))
                    assert np.abs(gab - want).max() <= ec.REF_TOL * top and np.abs(gab - rab).max() <= ec.REF_TOL * top, (g, n, side)
                else:
                    assert not gab.any()
                if zero is not None:   # all-zero rows: cos a zero operand row and a = 1/2, kl / sym_kl the uniform profile
                    if metric == "cos":
                        assert not got[zero].any() and gab[zero] == (0.5 if side == 0 else 0.0)
                    elif metric in ("kl", "sym_kl"):
                        for part in ([got[zero, :g]] + ([got[zero, g:2 * g]] if metric == "sym_kl" else [])):
                            assert (part == part[0]).all(), (g, n, side)
                        p0 = got[zero, 0] if side == 0 else (got[zero, g] if metric == "sym_kl" else None)
                        if p0 is not None and dtype == "float64":
                            assert abs(p0 - 1.0 / g) <= ec.PREP_F64_TOL
                        elif p0 is not None:
                            assert _ulps32(np.array([p0]), np.array([T(1.0 / g)]))[0] <= 1.0
    print(f"prepare {metric} {dtype}: operands {worst:.2e} (float64, rel), {off} of {total} float32 elements one ulp off; "
          f"a / b {worst_ab:.2e}")
    if dtype == "float64":
        _note(f"prepare {metric}: operands", dtype, worst)
    else:
        _note(f"prepare {metric}: fraction of elements one ulp off", dtype, off / max(total, 1))
        assert off <= ec.PREP_F32_FRACTION * total, (off, total)
    _note(f"prepare {metric}: a / b", dtype, worst_ab)


# ------------------------------------------------------------------------------------------------------ B: pair stage
def _check_against_reference(dc, got, dense=False):
    ref = dc.reference()
    dev = ec.raw_deviations(got, ref, with_P=dense)
    print(f"  {dc.name} {dc.dtype} plan {ec.plan(dc.na, dc.nb)}: " + ", ".join(f"{q} {v:.1e}" for q, v in dev.items()))
    for q, v in dev.items():
        _note(f"{ec.family(dc.name)}: {q}", dc.dtype, v)
    for q, v in dev.items():
        assert v <= ac.F64_TOL, (dc.name, dc.dtype, q, v)
    far = dc.case["far"]
    assert not got["K_NB"][far].any() and (not dense or not got["P"][:, far].any())   # out of reach: exact zeros
    near = np.setdiff1d(np.arange(dc.nb), far)
    assert np.all(got["K_NB"][near] > 0.0)
    return dev


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ec.PAIR_CASES)
def test_pair_stage_on_the_devices_own_operands(dtype, name):
    dc = _device_case(name, dtype)
    got = _assign(dc)
    _check_against_reference(dc, got)
    again = _assign(dc)
    for q in ec.RAW:
        assert _same_bits(got[q], again[q]), (name, q)   # two calls, same bits: every case, every split plan
    if ec.SPECS[name][1].get("far") == "all":
        assert all(not got[q].any() for q in ec.RAW)


# ------------------------------------------------------------------------------------------------------ C: dense
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ec.DENSE_CASES)
def test_dense_variant_where_tile_edges_cut_P(dtype, name):
    dc = _device_case(name, dtype)
    got = _assign(dc, dense=True)   # (the guard behind P[na nb] is checked in _assign)
    _check_against_reference(dc, got, dense=True)
    plain = _assign(dc)
    for q in ec.RAW:
        assert _same_bits(plain[q], got[q]), (name, q)
    P = got["P"]
    for a, b, q in ((P.sum(1), got["K_NA"], "K_NA"), (P.sum(0), got["K_NB"], "K_NB"), (P @ dc.xb[:, :3], got["PXB"], "PXB")):
        err = float(np.abs(a - b).max() / np.abs(b).max())
        _note(f"dense: P against {q}", dtype, err)
        assert err <= ec.REF_TOL, (name, q, err)


# ------------------------------------------------------------------------------------------------------ D: workspace, stream
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("small,large", [("cells-65x33", "feat-kl-g17"), ("feat-kl-g17", "split-2500x2500"),
                                         ("split-50x4417", "split-4417x50")])
def test_workspace_contents_and_size_do_not_matter(dtype, small, large):
    """A workspace larger than needed, (1) zero-filled, (2) NaN-filled, (3) holding the partials of a larger call: same bits,
    nothing written behind it."""
    ds, dl = _device_case(small, dtype), _device_case(large, dtype)
    need_s, need_l = ec.workspace_bytes(ds.na, ds.nb), ec.workspace_bytes(dl.na, dl.nb)
    size = max(need_s, need_l) + 4096
    assert need_s < size
    ws = _guarded(size // 8)
    ws[: size // 8] = 0.0
    zero = _assign(ds, ws=ws, ws_bytes=size)
    ws[: size // 8] = float("nan")
    nan = _assign(ds, ws=ws, ws_bytes=size)
    big = _assign(dl, ws=ws, ws_bytes=size)
    stale = _assign(ds, ws=ws, ws_bytes=size)
    ws2 = _nan_workspace(size)
    ws2[: need_s // 8] = 0.0   # NaN everywhere behind what the call needs
    tight = _assign(ds, ws=ws2, ws_bytes=size)
    _check_against_reference(dl, big)
    for q in ec.RAW:
        assert _same_bits(zero[q], nan[q]) and _same_bits(zero[q], stale[q]) and _same_bits(zero[q], tight[q]), (small, q)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["feat-kl-g17", "split-4417x50", "layers-4"])
def test_a_call_on_another_stream_gives_the_same_bits(dtype, name):
    dc = _device_case(name, dtype)
    first = _assign(dc)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        assert dc.k._stream() == stream.cuda_stream != torch.cuda.default_stream(DEV).cuda_stream
        other = _assign(dc, dense=False)
    torch.cuda.synchronize()
    for q in ec.RAW:
        assert _same_bits(first[q], other[q]), (name, q)


# ------------------------------------------------------------------------------------------------------ E: the wrapper
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(ec.WRAPPER_CASES))
def test_update_assignment_on_one_representative_per_family(dtype, name):
    """Padding to x4, model_mul, the outlier constant, the PXB[:, :D] slice and the scalars on the new shapes, against the
    formula restatement on the UNROUNDED inputs: float64 1e-10, float32 max(1.25 x the float32 floor of the nearest golden,
    1e-5) - the bounds of test_a_size_no_golden_holds_against_the_chunked_restatement."""
    import spateo_amd

    c = ec.case(name)
    args, kw = ec.call_arguments(c)
    got = spateo_amd.align.update_assignment(*args, dtype=dtype, device=DEV, **kw)
    ref = ac.restatement(*args, chunk=512, **kw)
    tols = ac.tolerances(ac.load(), ec.WRAPPER_CASES[name], dtype)
    assert all(t >= ac.F32_BASE for t in tols.values()) or dtype == "float64"
    ac.check(got, ref, tols, f"update_assignment {name} {dtype}")
    dev = ac.deviations(got, ref)
    _note("update_assignment: all quantities", dtype, max(dev.values()))
    assert got["PXB"].shape == c["XA"].shape and not got["K_NB"][c["far"]].any()
