"""The float32 cached Gram tile kernel that shares its widened column panels through LDS (gram_cached_kernel_shared_cols)
computes the SAME BITS as the recompute path and as the register-operand kernel gram_cached_kernel<float> (developer
option "gram_reg_cols"): same operand values, same MFMA order per output element, so every comparison is torch.equal.

Shapes are the smallest at which the kernel can go wrong: one block (m = 16); either side of the 64-column limit of the
2 x 4 edge shape in a single tile (64, 65), a two-column edge tile (130), 64 and 65 live columns in the last tile column
(192, 193), the headline's remainder 3 * 128 + 56 (440); cell counts that leave empty and partial groups, a ring shorter
than its depth and the remainder loop (1, 255, 256, 257, 511, 4097)."""
import numpy as np
import pytest
import torch

from _kernel_scaffold import fresh_kernels as _k, option as _option

pytestmark = pytest.mark.gpu

BETA = 0.003


def _inputs(k, seed, n, m, spread=30.0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (n, 3)) * spread
    ctrl = rng.uniform(-1, 1, (m, 3)) * spread  # (points of their own: m may exceed n)
    Y = rng.standard_normal((n, 3))
    P = torch.from_numpy(rng.uniform(1e-5, 1.0, n).astype(np.float32)).to("cuda:0")
    center = ctrl.mean(0)
    return k.to_x4(X, center), k.to_x4(ctrl, center), k.to_x4(Y), P


def _gr(m):
    return (torch.empty(m, m, dtype=torch.float64, device="cuda:0"), torch.empty(m, 3, dtype=torch.float64, device="cuda:0"))


def _cached(kk, x4, P, y4, c4, beta, m, reg_cols):
    from spateo_amd import _lib

    with _option("gram_reg_cols", 1 if reg_cols else 0):
        if reg_cols:
            assert _lib.debug_options().get("gram_reg_cols") == 1  # what the bench reports as developer_options
        G, R = _gr(m)
        kk.gram(x4, P, y4, c4, beta, G, R, cache_only=True)
    return G, R


def _check(kk, x4, P, y4, c4, beta, m):
    """G, R of the recompute path, of the shared-column kernel (the default) and of the register-operand kernel."""
    kk.drop_ublk()
    G, R = _gr(m)
    kk.gram(x4, P, y4, c4, beta, G, R)
    kk.build_ublk(x4, c4, beta)
    Gs, Rs = _cached(kk, x4, P, y4, c4, beta, m, reg_cols=False)
    Gr, Rr = _cached(kk, x4, P, y4, c4, beta, m, reg_cols=True)
    assert torch.equal(Gs, G) and torch.equal(Rs, R)
    assert torch.equal(Gs, Gr) and torch.equal(Rs, Rr)
    assert torch.equal(Gs, Gs.T)
    return Gs, Rs


@pytest.mark.parametrize("m", [16, 64, 65, 130, 192, 193, 440])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 511, 4097])
def test_shared_cols_equal_recompute_and_register_operands(n, m):
    kk = _k("float32")
    x4, c4, y4, P = _inputs(kk, 3000 + n + m, n, m)
    _check(kk, x4, P, y4, c4, BETA, m)
    kk.drop_ublk()


def test_two_phases_of_256_cell_slices_twice_on_one_workspace():
    """slice_len forced to 256 at m = 300: 1 200 001 cells need two phases (the partial-tile buffer is smaller than all
    partial tiles); a second call on the same HipKernels gives the same bits."""
    n, m = 1_200_001, 300
    with _option("slice_len", 256):
        kk = _k("float32")
        x4, c4, y4, P = _inputs(kk, 6, n, m)
        assert kk.lib.mvf_gram_workspace_bytes(n, m, kk.cdtype) < (n // 256) * 6 * 128 * 128 * 8  # more than one phase
        Gs, Rs = _check(kk, x4, P, y4, c4, BETA, m)
        G2, R2 = _cached(kk, x4, P, y4, c4, BETA, m, reg_cols=False)
        assert torch.equal(G2, Gs) and torch.equal(R2, Rs)
        kk.drop_ublk()


def test_p_with_exact_zeros_and_the_floor():
    """P holds exact zeros and 1e-5 next to ordinary weights (a zero P K product in a row operand)."""
    n, m = 4097, 193
    kk = _k("float32")
    x4, c4, y4, P = _inputs(kk, 77, n, m)
    Ph = P.cpu().numpy().copy()
    Ph[::3] = 0.0
    Ph[1::7] = np.float32(1e-5)
    assert (Ph == 0).sum() > 1000 and (Ph == np.float32(1e-5)).sum() > 300 and (Ph > 0.5).sum() > 300
    P = torch.from_numpy(Ph).to("cuda:0")
    _check(kk, x4, P, y4, c4, BETA, m)
    kk.drop_ublk()


def test_kernel_values_that_underflow_to_denormals_and_to_zero():
    """A large beta on the same geometry: many float32 kernel values exp2(-e) fall into the denormal range (126 < e <= 149)
    and many below it.  Checked on the CPU first, in float32 arithmetic on the scaled coordinates the kernels use."""
    n, m, beta = 4097, 193, 0.05
    kk = _k("float32")
    x4, c4, y4, P = _inputs(kk, 78, n, m)
    s = np.float32(np.sqrt(beta * np.log2(np.e)))
    xs, cs = x4.cpu().numpy()[:, :3] * s, c4.cpu().numpy()[:, :3] * s
    d = xs[:, None, :] - cs[None, :, :]
    e = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).astype(np.float32)
    with np.errstate(under="ignore"):
        kv = np.exp2(-e).astype(np.float32)
    tiny = np.finfo(np.float32).tiny
    n_denormal, n_zero, n_normal = int(((kv > 0) & (kv < tiny)).sum()), int((kv == 0).sum()), int((kv >= tiny).sum())
    print(f"float32 kernel values on the CPU: {n_normal} normal, {n_denormal} denormal, {n_zero} zero")
    assert n_denormal > 1000 and n_zero > 1000 and n_normal > 1000
    G, _ = _check(kk, x4, P, y4, c4, beta, m)
    assert torch.isfinite(G).all() and float(G.diagonal().min()) > 0
    kk.drop_ublk()
