"""``st.tdr.kernel_density`` / ``pc_KDE`` / ``cell_density`` on ``cuda:0`` against sklearn's recorded scores (tests/golden/ref_kde.npz)
and the restatement of tests/_kde_cases.py: the public API end to end - centring, upload, the column chunks, ``mvf_kde``, the
constants.  The bounds are the cases' own (tests/_kde_cases.py)."""
import numpy as np
import pytest
import torch

import _kde_cases as kc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"


class Cloud:
    def __init__(self, points):
        self.points, self.point_data = np.array(points, dtype=np.float64), {}

    def copy(self):
        new = Cloud(self.points)
        new.point_data = dict(self.point_data)
        return new


def _api(case, dtype="float64", **kw):
    import spateo_amd as st

    return st.tdr.kernel_density(case["X"], case["T"], kernel=case["kernel"], bandwidth=case["h"], sample_weight=case["w"],
                                 groups=case["g"], dtype=dtype, device=DEV, **kw)


@pytest.mark.parametrize("dtype", ("float64", "float32"))
@pytest.mark.parametrize("name", kc.GOLDEN_FULL)
def test_kernel_density_against_the_golden(name, dtype):
    """The case's coordinates are centred already and the host's centre is 0 up to 2^-20 of the extent, so in float32 mode the
    device stores the case's own rounded coordinates and the float32 reference applies."""
    case, G = kc.CASES[name], kc.load()
    ref, bound, tight, dev_order, dev_sk = kc.reference(name, dtype)
    got = _api(case, dtype).reshape(ref.shape)
    share = kc.compare(got, ref, bound)
    print(f"kernel_density {name} [{dtype}]: share of the bound {share:.4f}")
    assert share <= 1.0 and (tight is None or kc.compare(got, ref, tight) <= 1.0)
    if dtype == "float64" and name not in kc.TIGHT:      # sklearn's recorded scores themselves, within the same bound
        score = G[f"{name}_score"]
        assert kc.compare(got, score, kc.bound(score, dev_order, dev_sk)) <= 1.0


@pytest.mark.parametrize("name", ("C65_gauss", "C65_cosine", "C65_N4097"))
def test_more_columns_than_one_call_takes(name):
    """65 groups: the host runs two chunks of columns (64 + 1) with the group ids shifted."""
    case = kc.CASES[name]
    ref, bound, _, _, _ = kc.reference(name)
    got = _api(case)
    assert got.shape == (len(case["T"]), 65)
    assert kc.compare(got, ref, bound) <= 1.0


def test_pc_kde_against_the_golden():
    import spateo_amd as st

    case, G = kc.CASES["gaussian_d3"], kc.load()
    pc = Cloud(case["X"] + np.array([500.0, -20.0, 3.0]))
    out, cmap = st.tdr.pc_KDE(pc, bandwidth=case["h"], device=DEV)
    ref, bound, _, _, _ = kc.reference("gaussian_d3")
    assert cmap == "hot_r" and "kde" not in pc.point_data
    # (the offset cloud is re-centred by the host: differences change by rounding of the offset coordinates, 1e-13 of the extent)
    assert np.abs(out.point_data["kde"] - G["gaussian_d3_score"][:300, 0]).max() < 1e-9
    pc0 = Cloud(case["X"])
    assert st.tdr.pc_KDE(pc0, bandwidth=case["h"], inplace=True, device=DEV) == (None, "hot_r")
    assert kc.compare(pc0.point_data["kde"], ref[:300], bound[:300]) <= 1.0


def test_groups_equal_per_group_calls_bit_for_bit():
    """The shift is per (target, group) and a column's summation order does not depend on the other columns: with coordinates on
    a 2^-10 grid (exact under any centre the host picks) column c of a grouped call has the bits of a call on that group's
    points alone, and of a call whose weights keep that group only - the latter over two splits as well."""
    import spateo_amd as st

    rng = np.random.default_rng(12)
    X = rng.integers(0, 1 << 13, (900, 3)) / 1024.0 + 256.0
    T = rng.integers(0, 1 << 13, (130, 3)) / 1024.0 + 256.0
    g = rng.integers(0, 5, 900)
    g[g == 3] = 4                                                   # group 3 has no source
    w = 0.25 + rng.integers(0, 8, 900) / 4.0
    for kernel, h in (("gaussian", 0.5), ("exponential", 0.7), ("epanechnikov", 1.1)):
        full = st.tdr.kernel_density(X, T, kernel=kernel, bandwidth=h, sample_weight=w, groups=g, device=DEV)
        assert full.shape == (130, 5) and np.isneginf(full[:, 3]).all() and np.isfinite(full[:, [0, 1, 2, 4]]).any()
        for c in (0, 1, 2, 4):
            sub = st.tdr.kernel_density(X[g == c], T, kernel=kernel, bandwidth=h, sample_weight=w[g == c], device=DEV)
            assert np.array_equal(sub.view(np.uint64), full[:, c].view(np.uint64)), (kernel, c)
    X2 = np.vstack([X] * 5)[:4200]                                   # two splits of the sources
    g2, w2 = np.tile(g, 5)[:4200], np.tile(w, 5)[:4200]
    assert kc.splits(130, 4200) == 2
    full = st.tdr.kernel_density(X2, T, bandwidth=0.5, sample_weight=w2, groups=g2, device=DEV)
    for c in (0, 4):
        one = st.tdr.kernel_density(X2, T, bandwidth=0.5, sample_weight=np.where(g2 == c, w2, 0.0), device=DEV)
        assert np.array_equal(one.view(np.uint64), full[:, c].view(np.uint64)), c


def test_targets_on_a_small_grid():
    import spateo_amd as st

    case = kc.CASES["epanechnikov_disjoint"]
    ax = np.linspace(-0.6, 0.6, 7)
    grid = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3) + 0.0137   # 343 voxels, two target tiles
    probe = dict(case, T=grid, far=0)
    kc.assert_decidable(probe)
    want = kc.log_density(probe)
    dev_order = kc.deviation(want, kc.log_density(probe, reverse=True), want)
    got = st.tdr.kernel_density(case["X"], grid, kernel="epanechnikov", bandwidth=case["h"], device=DEV)
    assert got.shape == (343,) and np.isneginf(want).any() and np.isfinite(want).any()
    # sklearn's deviation is not recorded for this probe; the forward / reversed deviation and the floor alone bound it
    assert kc.compare(got, want, kc.bound(want, dev_order, 0.0)) <= 1.0


def test_cell_density():
    import pandas as pd

    import spateo_amd as st

    case = kc.CASES["C17_gauss"]
    codes = case["g"] % 4
    adata = st.AnnDataLite(obsm={"spatial": case["X"]}, obs={"type": pd.Series(pd.Categorical.from_codes(codes, categories=list("abcd")))})
    st.tdr.cell_density(adata, bandwidth=case["h"], device=DEV)
    st.tdr.cell_density(adata, group_key="type", key_added="by_type", bandwidth=case["h"], device=DEV)
    assert adata.uns["by_type"]["categories"] == list("abcd") and adata.obsm["by_type"].shape == (700, 4)
    for probe, got in ((dict(case, T=case["X"], g=None, C=1, w=None), adata.obs["kde"][:, None]),
                       (dict(case, T=case["X"], g=codes, C=4, w=None), adata.obsm["by_type"])):
        want = kc.log_density(probe)
        dev_order = kc.deviation(want, kc.log_density(probe, reverse=True), want)
        assert kc.compare(got, want, kc.bound(want, dev_order, 0.0)) <= 1.0
