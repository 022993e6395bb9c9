"""Scaffolding of the kernel-level GPU tests of the alignment path (tests/test_gpu_assign*_kernels.py,
test_gpu_align*_kernels.py, test_gpu_prepare_csr_kernels.py): the ``HipKernels`` per cell dtype that those nine modules share,
and the device cases and raw-ABI calls that several of them need.  What knows nothing about the alignment path - guarded
buffers, bit comparisons, the table of largest deviations - lives in tests/_kernel_scaffold.py and is imported from there.
No test module imports another one: what two of them need lives here."""
import numpy as np
import torch

import _assign_edge_cases as ec
import _assign_label_case as lab
from _kernel_scaffold import called, dev, guarded, intact, kernel_cache, nan_workspace, watch, written

LABEL, PROBS = 5, {"gauss": 0, "cos": 1, "prob": 2}  # MVF_ASSIGN_LABEL and the probability types of include/mvf.h
kernels = kernel_cache()  # one cache for the nine alignment modules
_CASES = {}


# ------------------------------------------------------------------------------------------------------ raw calls
def prepare(k, layer, metric, side):
    """mvf_assign_prepare into guarded buffers: (X' / Y' (n, ld) device view, a / b (n,) device view, ld)."""
    from spateo_amd import _lib

    L = dev(np.asarray(layer, dtype=np.float64))
    n, g = L.shape
    ld = int(k.lib.mvf_assign_padded_features(g, ec.METRICS[metric]))
    assert ld == ec.padded_features(g, metric)
    Lp, ab = guarded(n * ld, k.tdtype), guarded(n)
    _lib.check(k.lib.mvf_assign_prepare(L.data_ptr(), n, g, ec.METRICS[metric], side, Lp.data_ptr(), ld, ab.data_ptr(), k.cdtype,
                                        k._stream()), "mvf_assign_prepare")
    called()
    torch.cuda.synchronize()
    assert intact(Lp, n * ld) and intact(ab, n), "mvf_assign_prepare wrote behind a buffer"
    assert written(Lp, n * ld) and written(ab, n), "mvf_assign_prepare left an element unwritten"
    return Lp[: n * ld].view(n, ld), ab[:n], ld


class DeviceCase:
    """A case of _assign_edge_cases on the device: coordinates and model_mul uploaded, every layer prepared BY THE DEVICE,
    and all of it read back."""

    def __init__(self, name, c, dtype):
        k = kernels(dtype)
        self.name, self.dtype, self.case, self.k = name, dtype, c, k
        self.na, self.nb = len(c["XA"]), len(c["XB"])
        self.xa4, self.xb4 = k.to_x4(c["XA"]), k.to_x4(c["XB"])
        self.mm_host, self.outlier = ec.raw_scalars(c)
        self.mm = dev(self.mm_host)
        self.layers, self.host_layers = [], []
        for A, B, met, kind, par in zip(c["layers_A"], c["layers_B"], c["dissimilarity"], c["probability_type"],
                                        c["probability_parameters"]):
            Xp, a, ld = prepare(k, A, met, 0)
            Yp, b, _ = prepare(k, B, met, 1)
            self.layers.append((Xp, Yp, a, b, ld, ec.METRICS[met], ec.PROBS[kind], 0.0 if par is None else float(par)))
            self.host_layers.append((Xp.double().cpu().numpy(), Yp.double().cpu().numpy(), a.cpu().numpy(), b.cpu().numpy(),
                                     met, kind, par))
        self.xa, self.xb = self.xa4.double().cpu().numpy(), self.xb4.double().cpu().numpy()
        assert not self.xa[:, 3].any() and not self.xb[:, 3].any() and not self.xa[:, c["XA"].shape[1]:].any()
        self._ref = None

    def reference(self):
        """pair_reference on exactly what the device holds."""
        if self._ref is None:
            c = self.case
            self._ref = ec.pair_reference(self.xa, self.xb, self.host_layers, self.mm_host, c["sigma2"], c["sigma2_variance"],
                                          self.outlier)
        return self._ref


def device_case(key, make, dtype):
    """The DeviceCase of ``make()`` under ``key``; the last four stay on the device."""
    if (key, dtype) not in _CASES:
        if len(_CASES) >= 4:
            _CASES.pop(next(iter(_CASES)))
        _CASES[(key, dtype)] = DeviceCase(str(key), make(), dtype)
    return _CASES[(key, dtype)]


def watch_case(dc):
    """Under a ``convention`` of tests/_kernel_scaffold.py: the operands of a DeviceCase or LabelCase, which the library takes
    as ``const``, must leave the block unchanged."""
    watch(dc.xa4, dc.xb4, dc.mm, *[t for layer in dc.layers for t in layer[:4] if torch.is_tensor(t)])


def layer_struct(dc):
    from spateo_amd._kernels import layer_array

    return layer_array(dc.layers)


def assign(dc, dense=False, ws=None, ws_bytes=None):
    """mvf_assign / mvf_assign_dense through the raw ABI on the current stream.  Every output sits in front of a guard; the
    workspace (default: exactly mvf_assign_workspace_bytes, NaN-filled, guarded) likewise.  Returns host arrays."""
    from spateo_amd import _lib

    k, na, nb = dc.k, dc.na, dc.nb
    sizes = {"K_NA": na, "K_NB": nb, "K_NA_spatial": na, "K_NA_sigma2": na, "PXB": 3 * na, "scalar": 1}
    if dense:
        sizes["P"] = na * nb
    bufs = {q: guarded(n) for q, n in sizes.items()}
    need = int(k.lib.mvf_assign_workspace_bytes(na, nb))
    assert need == ec.workspace_bytes(na, nb)
    if ws is None:
        ws, ws_bytes = nan_workspace(need), need
    c = dc.case
    head = (dc.xa4.data_ptr(), na, dc.xb4.data_ptr(), nb, layer_struct(dc), len(dc.layers), dc.mm.data_ptr(), float(c["sigma2"]),
            float(c["sigma2_variance"]), float(dc.outlier)) + tuple(bufs[q].data_ptr() for q in
                                                                   ("K_NA", "K_NB", "K_NA_spatial", "K_NA_sigma2", "PXB", "scalar"))
    tail = (ws.data_ptr(), int(ws_bytes), k.cdtype, k._stream())
    if dense:
        _lib.check(k.lib.mvf_assign_dense(*head, bufs["P"].data_ptr(), *tail), "mvf_assign_dense")
    else:
        _lib.check(k.lib.mvf_assign(*head, *tail), "mvf_assign")
    called()
    torch.cuda.synchronize()
    for q, n in sizes.items():
        assert intact(bufs[q], n), f"{dc.name}: wrote behind {q}[{n}]"
        assert written(bufs[q], n), f"{dc.name}: left an element of {q} unwritten"
    assert intact(ws, ws_bytes // 8), f"{dc.name}: wrote behind the workspace"
    out = {q: bufs[q][:n].cpu().numpy() for q, n in sizes.items()}
    out["PXB"] = out["PXB"].reshape(na, 3)
    out["scalar"] = out["scalar"].reshape(())
    if dense:
        out["P"] = out["P"].reshape(na, nb)
    for q, v in out.items():
        assert np.isfinite(v).all(), f"{dc.name}: {q} is not finite"
    return out


# ------------------------------------------------------------------------------------------------------ label layers
def label_prepare(k, labels, classes):
    """mvf_assign_label_prepare into a guarded buffer."""
    from spateo_amd import _lib

    lab32 = dev(np.asarray(labels), torch.int32)
    out = guarded(len(labels))
    _lib.check(k.lib.mvf_assign_label_prepare(lab32.data_ptr(), len(labels), int(classes), out.data_ptr(), k._stream()),
               "mvf_assign_label_prepare")
    called()
    torch.cuda.synchronize()
    assert intact(out, len(labels))
    return out[: len(labels)]


class LabelCase:
    """An edge case of _assign_label_case on the device: the label layer prepared through the raw entry point, an expression
    layer (if any) through HipKernels.assign_prepare, and the restatement on the coordinates as stored."""

    def __init__(self, shape, dtype, expression=True):
        NA, NB, K, L = shape
        c, k = lab.edge_case(NA, NB, K, L, expression=expression), kernels(dtype)
        self.c, self.k, self.na, self.nb = c, k, NA, NB
        self.xa4, self.xb4 = k.to_x4(c["XA"]), k.to_x4(c["XB"])
        self.mm_host, self.outlier = ec.raw_scalars(c)
        self.mm = dev(self.mm_host)
        self.T = dev(c["label_transfer"])
        self.layers, host_A, host_B = [], [], []
        for A, B, met, kind, par in zip(c["layers_A"], c["layers_B"], c["dissimilarity"], c["probability_type"],
                                        c["probability_parameters"]):
            if met == "label":
                a, b = label_prepare(k, A, K), label_prepare(k, B, L)
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
        from spateo_amd._kernels import layer_array

        return layer_array(self.layers if layers is None else layers)

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
        bufs = {q: guarded(n) for q, n in sizes.items()}
        rows = guarded(nb * ke, torch.int32) if mode == "topk" else None
        need = int(lib.mvf_assign_topk_workspace_bytes(na, nb, k) if mode == "topk" else lib.mvf_assign_workspace_bytes(na, nb))
        ws = nan_workspace(need)
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
        called()
        torch.cuda.synchronize()
        if status != 0 or not check:
            return status, None
        for q, n in sizes.items():
            assert intact(bufs[q], n), f"wrote behind {q}[{n}]"
        assert intact(ws, need // 8), "wrote behind the workspace"
        out = {q: bufs[q][:n].cpu().numpy() for q, n in sizes.items()}
        out["PXB"] = out["PXB"].reshape(na, 3)
        if mode == "dense":
            out["P"] = out["P"].reshape(na, nb)
        if mode == "topk":
            assert intact(rows, nb * ke)
            out["rows"], out["vals"] = rows[: nb * ke].cpu().numpy().reshape(nb, ke), out["vals"].reshape(nb, ke)
        for q, v in out.items():
            assert np.isfinite(v).all(), f"{q} is not finite"
        return status, out
