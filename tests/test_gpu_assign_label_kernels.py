"""Kernel-level edge tests of the label branch of the fused assignment step (``csrc/mvf_assign.hip``) through the raw C ABI -
``mvf_assign_label_prepare``, ``mvf_assign``, ``mvf_assign_dense``, ``mvf_assign_topk``, ``mvf_align_gather`` - on ``cuda:0`` in
both cell dtypes, against the NumPy restatement of tests/_assign_label_case.py fed with the coordinates as the cell dtype
stores them (the look-up and every sum are float64 in both modes, so both are held to 1e-10, ``_assign_case.F64_TOL``).

Shapes (NA x NB; K x L): 1 x 1 (1 x 1), 63 x 65 (5 x 4), 64 x 64 (K = 1), 65 x 129 (L = 1) and 65 x 129 (7 x 9) - the tile
edges, tables of one row and of one column, and in the last two the smallest sizes at which both passes split their work
(``_assign_edge_cases.plan``).  Every case draws the last row and the last column of its table.  Every output sits in front of
a guard, the workspace is filled with NaN bit patterns, and every call is made twice: the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import _assign_case as ac
import _assign_edge_cases as ec
import _assign_label_case as lab
import _assign_topk_case as tk

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = ["float64", "float32"]
SENTINEL = -1.2345e300
GUARD = 4096
LABEL, PROBS = 5, {"gauss": 0, "cos": 1, "prob": 2}
_KERNELS = {}


def _k(dtype):
    if dtype not in _KERNELS:
        from spateo_amd._kernels import HipKernels

        assert torch.cuda.is_available(), "GPU tests need a HIP device"
        _KERNELS[dtype] = HipKernels(DEV, dtype)
    return _KERNELS[dtype]


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _guarded(n, tdtype=torch.float64):
    return torch.full((n + GUARD,), SENTINEL if tdtype == torch.float64 else -12345, dtype=tdtype, device=DEV)


def _intact(buf, n):
    return bool((buf[n:] == (SENTINEL if buf.dtype == torch.float64 else -12345)).all())


def _label_prepare(k, labels, classes):
    """mvf_assign_label_prepare into a guarded buffer."""
    from spateo_amd import _lib

    lab32 = _dev(np.asarray(labels), torch.int32)
    out = _guarded(len(labels))
    _lib.check(k.lib.mvf_assign_label_prepare(lab32.data_ptr(), len(labels), int(classes), out.data_ptr(), k._stream()),
               "mvf_assign_label_prepare")
    torch.cuda.synchronize()
    assert _intact(out, len(labels))
    return out[: len(labels)]


class _Case:
    """An edge case on the device: the label layer prepared through the raw entry point, an expression layer (if any)
    through HipKernels.assign_prepare, and the restatement on the coordinates as stored."""

    def __init__(self, shape, dtype, expression=True):
        NA, NB, K, L = shape
        c, k = lab.edge_case(NA, NB, K, L, expression=expression), _k(dtype)
        self.c, self.k, self.na, self.nb = c, k, NA, NB
        self.xa4, self.xb4 = k.to_x4(c["XA"]), k.to_x4(c["XB"])
        self.mm_host, self.outlier = ec.raw_scalars(c)
        self.mm = _dev(self.mm_host)
        self.T = _dev(c["label_transfer"])
        self.layers, host_A, host_B = [], [], []
        for A, B, met, kind, par in zip(c["layers_A"], c["layers_B"], c["dissimilarity"], c["probability_type"],
                                        c["probability_parameters"]):
            if met == "label":
                a, b = _label_prepare(k, A, K), _label_prepare(k, B, L)
                assert np.array_equal(a.cpu().numpy(), A.astype(np.float64)) and np.array_equal(b.cpu().numpy(), B.astype(np.float64))
                self.layers.append((self.T, None, a, b, L, LABEL, PROBS[kind], 0.0))
                host_A.append(A), host_B.append(B)
            else:
                Xp, a, ld = k.assign_prepare(A, ec.METRICS[met], 0)
                Yp, b, _ = k.assign_prepare(B, ec.METRICS[met], 1)
                self.layers.append((Xp, Yp, a, b, ld, ec.METRICS[met], PROBS[kind], float(par)))
                g = A.shape[1]      # the operands as stored ("euc": the features themselves)
                host_A.append(Xp.double().cpu().numpy()[:, :g]), host_B.append(Yp.double().cpu().numpy()[:, :g])
        D = c["XA"].shape[1]
        self.XA, self.XB = self.xa4.double().cpu().numpy()[:, :D], self.xb4.double().cpu().numpy()[:, :D]
        self.ref = lab.restatement(self.XA, self.XB, host_A, host_B, dissimilarity=c["dissimilarity"],
                                   probability_type=c["probability_type"], probability_parameters=c["probability_parameters"],
                                   sigma2=c["sigma2"], alpha=None, SigmaDiag=None, gamma=None, samples_s=None,
                                   sigma2_variance=c["sigma2_variance"], label_transfer=c["label_transfer"], return_P=True,
                                   model_mul=self.mm_host, outlier=self.outlier)

    def struct(self, layers=None):
        from spateo_amd import _lib

        layers = self.layers if layers is None else layers
        arr = (_lib.AssignLayer * len(layers))()
        for s, (Xp, Yp, a, b, ld, metric, prob, param) in zip(arr, layers):
            s.Xp, s.Yp, s.a, s.b = (None if t is None else t.data_ptr() for t in (Xp, Yp, a, b))
            s.ld = int(ld)
            s.metric, s.prob, s.param = int(metric), int(prob), float(param)
        return arr

    def call(self, mode="plain", k=0, layers=None, check=True):
        """mvf_assign ("plain"), mvf_assign_dense ("dense") or mvf_assign_topk ("topk") on guarded buffers and a NaN-filled,
        guarded workspace of exactly the size the library asks for.  Returns (status, host arrays)."""
        lib, na, nb, c = self.k.lib, self.na, self.nb, self.c
        ke = min(k, na)
        sizes = {"K_NA": na, "K_NB": nb, "K_NA_spatial": na, "K_NA_sigma2": na, "PXB": 3 * na, "scalar": 1}
        if mode == "dense":
            sizes["P"] = na * nb
        if mode == "topk":
            sizes["vals"] = nb * ke
        bufs = {q: _guarded(n) for q, n in sizes.items()}
        rows = _guarded(nb * ke, torch.int32) if mode == "topk" else None
        need = int(lib.mvf_assign_topk_workspace_bytes(na, nb, k) if mode == "topk" else lib.mvf_assign_workspace_bytes(na, nb))
        ws = _guarded(need // 8)
        ws[: need // 8] = float("nan")
        head = (self.xa4.data_ptr(), na, self.xb4.data_ptr(), nb, self.struct(layers), len(self.layers if layers is None else layers),
                self.mm.data_ptr(), float(c["sigma2"]), float(c["sigma2_variance"]), float(self.outlier))
        outs = tuple(bufs[q].data_ptr() for q in ("K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2", "PXB", "scalar"))
        tail = (ws.data_ptr(), need, self.k.cdtype, self.k._stream())
        if mode == "dense":
            status = lib.mvf_assign_dense(*head, *outs, bufs["P"].data_ptr(), *tail)
        elif mode == "topk":
            status = lib.mvf_assign_topk(*head, k, *outs, rows.data_ptr(), bufs["vals"].data_ptr(), *tail)
        else:
            status = lib.mvf_assign(*head, *outs, *tail)
        torch.cuda.synchronize()
        if status != 0 or not check:
            return status, None
        for q, n in sizes.items():
            assert _intact(bufs[q], n), f"wrote behind {q}[{n}]"
        assert _intact(ws, need // 8), "wrote behind the workspace"
        out = {q: bufs[q][:n].cpu().numpy() for q, n in sizes.items()}
        out["PXB"] = out["PXB"].reshape(na, 3)
        if mode == "dense":
            out["P"] = out["P"].reshape(na, nb)
        if mode == "topk":
            assert _intact(rows, nb * ke)
            out["rows"], out["vals"] = rows[: nb * ke].cpu().numpy().reshape(nb, ke), out["vals"].reshape(nb, ke)
        for q, v in out.items():
            assert np.isfinite(v).all(), f"{q} is not finite"
        return status, out


def _compare(case, out, what):
    ref, D = case.ref, case.XA.shape[1]
    dev = {}
    for q in ("K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2"):
        dev[q] = float(np.abs(out[q] - ref[q]).max() / np.abs(ref[q]).max())
    dev["PXB"] = float(np.abs(out["PXB"][:, :D] - ref["PXB"]).max() / np.abs(ref["PXB"]).max())
    raw = ref["sigma2_related"] * D * ref["Sp_sigma2"]
    dev["scalar"] = float(abs(out["scalar"][0] - raw) / abs(raw))
    print(f"  {what}: " + ", ".join(f"{q} {v:.2e}" for q, v in dev.items()))
    for q, v in dev.items():
        assert v <= ac.F64_TOL, (what, q, v)
    assert not out["PXB"][:, D:].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", lab.EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_label_branch_at_the_tile_and_table_edges(shape, dtype):
    NA, NB, K, L = shape
    if (NA, NB) == (65, 129):
        rt, ct, rs, cs = ec.plan(NA, NB)
        assert rs > 1 and cs > 1 and ec.plan(64, 129)[2] == 1 and ec.plan(65, 64)[3] == 1   # the smallest sizes that split both passes
    for expression in (True, False):
        case = _Case(shape, dtype, expression)
        c = case.c
        assert c["layers_A"][-1].max() == K - 1 and c["layers_B"][-1].max() == L - 1
        what = f"{NA} x {NB}, table {K} x {L}, {'euc + label' if expression else 'label alone'}, {dtype}"
        _, plain = case.call()
        _compare(case, plain, what)
        _, dense = case.call("dense")
        _compare(case, dense, what + " (dense)")
        assert np.abs(dense["P"] - case.ref["P"]).max() <= ac.F64_TOL * case.ref["P"].max()
        _, again = case.call()
        for q in plain:
            assert plain[q].tobytes() == again[q].tobytes() == dense[q].tobytes(), q


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,par", [("gauss", 0.25), ("cos", None)])
def test_probability_types_on_a_label_layer(kind, par, dtype):
    """gauss and cos on the look-up, with the label layer FIRST."""
    case = _Case((63, 65, 5, 4), dtype)
    c = case.c
    order = [1, 0]
    for key in ("layers_A", "layers_B", "dissimilarity", "probability_type", "probability_parameters"):
        c[key] = [c[key][i] for i in order]
    c["probability_type"][0], c["probability_parameters"][0] = kind, par
    T, _, a, b, L, _, _, _ = case.layers[1]
    layers = [(T, None, a, b, L, LABEL, PROBS[kind], 0.0 if par is None else par), case.layers[0]]
    Xp, Yp = case.layers[0][0], case.layers[0][1]
    g = c["layers_A"][1].shape[1]
    case.ref = lab.restatement(case.XA, case.XB, [c["layers_A"][0], Xp.double().cpu().numpy()[:, :g]],
                               [c["layers_B"][0], Yp.double().cpu().numpy()[:, :g]], dissimilarity=c["dissimilarity"],
                               probability_type=c["probability_type"], probability_parameters=c["probability_parameters"],
                               sigma2=c["sigma2"], alpha=None, SigmaDiag=None, gamma=None, samples_s=None,
                               sigma2_variance=c["sigma2_variance"], label_transfer=c["label_transfer"], return_P=True,
                               model_mul=case.mm_host, outlier=case.outlier)
    _, out = case.call(layers=layers)
    _compare(case, out, f"label ({kind}) + euc, {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 8, 64])
def test_top_k_through_the_raw_abi(k, dtype):
    case = _Case((65, 129, 7, 9), dtype)
    _, out = case.call("topk", k)
    tk.check(out, case.ref["P"], case.XB, k, ac.F64_TOL, what=f"65 x 129 k {k} {dtype}")
    _, again = case.call("topk", k)
    for q in out:
        assert out[q].tobytes() == again[q].tobytes(), q


def test_malformed_label_layers_are_rejected():
    """Null pointers and ld < 1 in the four entry points that take the layer, classes < 1 in the preparation: the error code
    and message style of the neighbouring checks, nothing launched."""
    case = _Case((63, 65, 5, 4), "float64", expression=False)
    k, lib = case.k, case.k.lib
    T, _, a, b, L, metric, prob, param = case.layers[0]
    bad = {"a null table": (None, None, a, b, L), "null A labels": (T, None, None, b, L), "null B labels": (T, None, a, None, L),
           "L = 0": (T, None, a, b, 0), "L < 0": (T, None, a, b, -4), "Yp set: a product layer with the label code": (T, T, a, b, L)}
    for mode, kk in (("plain", 0), ("dense", 0), ("topk", 8)):
        for what, (t_, y_, a_, b_, l_) in bad.items():
            status, _ = case.call(mode, kk, layers=[(t_, y_, a_, b_, l_, metric, prob, param)])
            msg = lib.mvf_last_error().decode()
            assert status != 0 and ("null pointer in layer 0" in msg or "ld" in msg or "bad metric 5" in msg), (mode, what, status, msg)
        status, _ = case.call(mode, kk, layers=[(T, None, a, b, L, 6, prob, param)])
        assert status != 0 and "bad metric" in lib.mvf_last_error().decode()
        status, _ = case.call(mode, kk, layers=[(T, None, a, b, L, metric, 0, 0.0)])   # gauss on a label layer needs its parameter
        assert status != 0 and "gauss" in lib.mvf_last_error().decode()
    # mvf_align_gather: b and b_out are needed, Yp / Yp_out are not read
    nb, bs = case.nb, 16
    perm = _dev(np.random.default_rng(0).permutation(nb), torch.int32)
    xb4_out, B, B_out, b_out = k.empty(bs, 4), k.zeros(nb, 3, dtype=torch.float64), k.empty(bs, 3, dtype=torch.float64), _guarded(bs)
    vp = ctypes.c_void_p * 1

    def gather(layer, bo):
        return lib.mvf_align_gather(perm.data_ptr(), nb, 3, bs, case.xb4.data_ptr(), xb4_out.data_ptr(), B.data_ptr(),
                                    B_out.data_ptr(), case.struct([layer]), 1, vp(None), vp(bo), k.cdtype, k._stream())

    assert gather(case.layers[0], b_out.data_ptr()) == 0
    torch.cuda.synchronize()
    idx = perm.cpu().numpy()[(3 + np.arange(bs)) % nb]
    assert np.array_equal(b_out[:bs].cpu().numpy(), c_labels(case)[idx]) and _intact(b_out, bs)
    assert gather((T, None, a, None, L, metric, prob, param), b_out.data_ptr()) != 0 and b"null pointer" in lib.mvf_last_error()
    assert gather(case.layers[0], None) != 0 and b"null pointer" in lib.mvf_last_error()
    assert gather((T, None, a, b, 0, metric, prob, param), b_out.data_ptr()) != 0 and b"ld" in lib.mvf_last_error()
    # the preparation
    lab32 = _dev(np.zeros(8), torch.int32)
    out = _guarded(8)
    assert lib.mvf_assign_label_prepare(lab32.data_ptr(), 8, 0, out.data_ptr(), None) != 0 and b"classes" in lib.mvf_last_error()
    assert lib.mvf_assign_label_prepare(None, 8, 3, out.data_ptr(), None) != 0 and b"null pointer" in lib.mvf_last_error()
    assert lib.mvf_assign_label_prepare(lab32.data_ptr(), 8, 3, None, None) != 0
    assert lib.mvf_assign_label_prepare(None, 0, 3, None, None) == 0                     # n == 0 launches nothing
    assert lib.mvf_assign_padded_features(7, LABEL) == 0                                  # a label layer has no prepared rows
    # labels outside the table are clamped into it: the look-up cannot leave the table
    wild = _label_prepare(k, np.array([-3, 0, 2, 3, 99]), 3)
    assert np.array_equal(wild.cpu().numpy(), [0.0, 0.0, 2.0, 2.0, 2.0])


def c_labels(case):
    return np.asarray(case.c["layers_B"][-1], dtype=np.float64)
