"""CPU proofs behind tests/test_gpu_assign_kernels.py (no GPU): the references of tests/_assign_edge_cases.py are right, the
cases are well conditioned, the targeted wrong answers would be seen, and the case lists cover what they claim.

Bounds: 1e-12 of each quantity's maximum for the product-form reference against the formula restatement of
tests/_assign_case.py and against its own long-double run (the bound test_cell_kernel_refs.py and test_assign_host.py use);
every mutation must move a compared quantity by >= 1e-7 = _cell_cases.MUTATION_FACTOR x _assign_case.F64_TOL."""
import numpy as np
import pytest

import _assign_case as ac
import _assign_edge_cases as ec
import _cell_cases as cc


@pytest.fixture(scope="module")
def g():
    return ac.load()


_REFS = {}


def _reference(name, dtype):
    """reference_for in float64 arithmetic; the costly cases (splits, 1000+ features) are computed once per module."""
    key = (name, np.dtype(dtype).name)
    if key in _REFS:
        return _REFS[key]
    ref = ec.reference_for(ec.case(name), dtype)
    if ec.family(name) in ("splits", "features 1000+"):
        _REFS[key] = ref
    return ref


def _all_far(name):
    return ec.SPECS[name][1].get("far") == "all"


# ------------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("name", ec.PAIR_CASES + ec.DENSE_CASES)
def test_product_form_agrees_with_the_formula_restatement(name):
    c = ec.case(name)
    args, kw = ec.call_arguments(c)
    raw = _reference(name, np.float64)
    if _all_far(name):   # nothing in reach: every output exactly 0 (the restatement's sigma2_related is 0 / 0)
        assert all(not np.any(raw[q]) for q in ec.RAW + ("P",)) and all(np.isfinite(raw[q]).all() for q in ec.RAW)
        return
    want = ac.restatement(*args, chunk=512, return_P="P" in raw, **kw)
    dev = ac.deviations(ec.quantities(raw, c["XA"].shape[1]), want)
    if "P" in want:
        dev["P"] = float(np.abs(raw["P"] - want["P"]).max() / want["P"].max())
    print(f"  {name}: " + ", ".join(f"{q} {v:.1e}" for q, v in dev.items()))
    assert max(dev.values()) <= ec.REF_TOL, dev


def test_product_form_reproduces_the_goldens(g):
    for tag in ac.case_tags(g):
        (XA, XB, LA, LB), kw = ac.case_inputs(g, tag)
        c = dict(XA=XA, XB=XB, layers_A=LA, layers_B=LB, **kw)
        c["dissimilarity"] = [{"euclidean": "euc", "square_euclidean": "square_euc", "cosine": "cos"}.get(m, m)
                              for m in kw["dissimilarity"]]
        c["probability_type"] = [{"gaussian": "gauss", "cosine": "cos"}.get(p.lower(), p.lower()) for p in kw["probability_type"]]
        raw = ec.reference_for(c, np.float64)
        dev = ac.deviations(ec.quantities(raw, XA.shape[1]), ac.golden_ref(g, tag))
        assert max(dev.values()) <= ec.REF_TOL, (tag, dev)
        if tag == "p":
            assert np.abs(raw["P"] - g["p_P"]).max() <= ec.REF_TOL * g["p_P"].max()


@pytest.mark.parametrize("name", ec.PAIR_CASES + ec.DENSE_CASES)
def test_every_case_is_well_conditioned(name):
    """float64 against long double on the same prepared operands: a case that fails this is ill-conditioned and is
    changed, the bound is not."""
    assert np.finfo(np.longdouble).eps < 1e-18
    c = ec.case(name)
    for dtype in (np.float64, np.float32):
        lay = ec.prepare_layers(c, dtype)
        if _all_far(name):   # exactly 0 in float64 BY underflow: the long-double values are below float64's range
            exact, wide = ec.reference_for(c, dtype, layers=lay), ec.reference_for(c, dtype, xp=np.longdouble, layers=lay)
            for q in ec.RAW + ("P",):
                assert not np.any(exact[q]) and np.abs(wide[q]).max() < np.finfo(np.float64).tiny, q
            continue
        dev = ec.raw_deviations(_reference(name, dtype), ec.reference_for(c, dtype, xp=np.longdouble, layers=lay), with_P=True)
        print(f"  {name} {np.dtype(dtype).name}: " + ", ".join(f"{q} {v:.1e}" for q, v in dev.items()))
        assert max(dev.values()) <= ec.REF_TOL, (np.dtype(dtype).name, dev)
        if ec.family(name) in ("splits", "features 1000+"):   # the cost is in these; the float32 operands add nothing new
            break


@pytest.mark.parametrize("name", ec.PAIR_CASES + ec.DENSE_CASES)
def test_probabilities_are_non_negative_and_far_columns_exactly_zero(name):
    c = ec.case(name)
    for dtype in (np.float64, np.float32):
        raw = _reference(name, dtype)
        assert raw["q_min"].min() >= 0.0, (name, float(raw["q_min"].min()))
        far = c["far"]
        for q in ("K_NB", "S"):
            assert not np.any(raw[q][..., far]), q
        assert "P" not in raw or not np.any(raw["P"][:, far])
        near = np.setdiff1d(np.arange(len(c["XB"])), far)
        assert np.all(raw["K_NB"][near] > 0.0)
        assert all(np.isfinite(raw[q]).all() for q in ec.RAW)
    if len(c["XB"]) >= 16 and not ec.SPECS[name][1].get("far") == "none":
        assert 0.05 * len(c["XB"]) <= len(far)
        assert len(far) <= 0.08 * len(c["XB"]) + 1 or _all_far(name)


# ------------------------------------------------------------------------------------------------------ sensitivity
PAD_ROW = "a clamped pad row counted once more in S0"


def test_every_mutation_moves_a_compared_quantity():
    """Every targeted wrong answer is >= 1e-7 away on every mutation case it applies to.  The pad row counted in S0 acts
    through in_j = 1 - o / (o + S0) alone: it is held to that on the cases of at most 130 A cells (o is ~ 1 / NA)."""
    assert np.isclose(ec.MUTATION_SHIFT, cc.MUTATION_FACTOR * ac.F64_TOL, rtol=1e-12, atol=0)
    names = set()
    for name in ec.MUTATION_CASES:
        assert name in ec.PAIR_CASES
        c = ec.case(name)
        good = _reference(name, np.float64)
        for what, bad in ec.mutations(c):
            dev = ec.raw_deviations(bad, good)   # the fused outputs alone: what every GPU case compares
            moved = max(dev.values())
            print(f"  {name}: {what}: {moved:.1e} ({max(dev, key=dev.get)})")
            if what != PAD_ROW or len(c["XA"]) <= 130:
                assert moved >= ec.MUTATION_SHIFT, (name, what, dev)
                names.add(what)
    assert len(names) == 10 and PAD_ROW in names, sorted(names)


def test_the_mutation_cases_reach_every_regime():
    seen = set()
    for name in ec.MUTATION_CASES:
        c = ec.case(name)
        NA, NB = len(c["XA"]), len(c["XB"])
        rs, cs = ec.plan(NA, NB)[2:]
        seen |= {"row split" if rs > 1 else "", "column split" if cs > 1 else "", "two layers" if len(c["features"]) == 2 else "",
                 "g = 1 mod 16" if c["features"][0] % 16 == 1 and c["features"][0] > 16 else "",
                 "64 splits over 70 tiles" if 64 in (rs, cs) else ""}
    assert {"row split", "column split", "two layers", "g = 1 mod 16", "64 splits over 70 tiles"} <= seen


# ------------------------------------------------------------------------------------------------------ coverage
def test_plan_restatement_matches_the_library_and_the_named_regimes():
    from spateo_amd import _lib

    lib = _lib.load()
    for (na, nb), want in ec.SPLIT_PLANS.items():
        assert ec.plan(na, nb) == want, (na, nb, ec.plan(na, nb))
        assert f"split-{na}x{nb}" in ec.SPLIT_CASES
    shapes = list(ec.SPLIT_PLANS) + [ec.shape(n) for n in ec.CELL_CASES] + \
        [ec.FEATURE_SHAPE, ec.BIG_SHAPE, (600, 450), (100_000, 100_000), (20011, 15013)] + list(ec.DENSE_SHAPES)
    for na, nb in shapes:
        assert lib.mvf_assign_workspace_bytes(na, nb) == ec.workspace_bytes(na, nb), (na, nb)
    assert ec.plan(600, 450) == (10, 8, 10, 8) and ec.plan(20011, 15013) == (313, 235, 5, 4)   # what test_gpu_assign.py runs
    plans = set(ec.SPLIT_PLANS.values())
    assert any(p[2] == ec.MAX_SPLITS and p[0] % p[2] for p in plans) and any(p[3] == ec.MAX_SPLITS and p[1] % p[3] for p in plans)
    assert any(p[0] >= 1024 and p[3] == 1 for p in plans) and any(p[1] >= 1024 and p[2] == 1 for p in plans)
    sizes = {ec.split_tiles(70, 64, y)[1] - ec.split_tiles(70, 64, y)[0] for y in range(64)}
    assert sizes == {1, 2}   # the uneven partition at the cap
    for name in ec.SPLIT_CASES:
        assert ec.case(name)["features"] == [24]


def test_feature_sweep_covers_the_k_loop_and_the_prepare_stride():
    lds = set()
    for name in ec.PAIR_CASES:
        if ec.family(name).startswith("features"):
            c = ec.case(name)
            lds.add(ec.padded_features(c["features"][0], c["dissimilarity"][0]))
    assert {16, 32, 48, 64, 80, 128, 144} <= lds and {1008, 2000} <= lds
    gs = set(ec.FEATURE_GS)
    for edge in (ec.KSTEP, 2 * ec.KSTEP, 3 * ec.KSTEP, ec.LANES, 2 * ec.LANES):
        assert {edge - 1, edge, edge + 1} <= gs
    assert {ec.padded_features(g_, "sym_kl") for g_ in ec.SYM_GS} >= {16, 32, 48, 64, 80}
    assert ec.padded_features(8, "sym_kl") == 16 and ec.padded_features(9, "sym_kl") == 32
    assert set(ec.PREPARE_GS) >= gs | set(ec.SYM_GS) | set(ec.BIG_GS) and 4 in ec.PREPARE_NS and 5 in ec.PREPARE_NS
    from spateo_amd import _lib

    lib = _lib.load()
    for met, code in ec.METRICS.items():
        for g_ in ec.PREPARE_GS:
            assert lib.mvf_assign_padded_features(g_, code) == ec.padded_features(g_, met)
    assert ec.METRICS == {m: _lib.ASSIGN_METRICS[m] for m in ec.METRICS} and ec.PROBS == {p: _lib.ASSIGN_PROBS[p] for p in ec.PROBS}


def test_cell_sweep_and_the_other_lists_cover_what_they_claim():
    shapes = {ec.shape(n) for n in ec.CELL_CASES}
    for side in (0, 1):
        ns = {s[side] for s in shapes}
        for k in (1, 2):
            assert {ec.TILE * k - 1, ec.TILE * k, ec.TILE * k + 1} <= ns
        assert {1, 15, 16, 17, 31, 32, 33, 4 * ec.TILE + 1} <= ns
    assert all((b, a) in shapes for a, b in shapes)
    assert {(ec.case(n)["dissimilarity"][0], ec.case(n)["probability_type"][0]) for n in ec.PAIR_CASES
            if ec.family(n) == "metric x probability"} == set(ec.METRIC_PROB)
    assert {m for m, _ in ec.METRIC_PROB} == set(ec.METRICS) and {p for _, p in ec.METRIC_PROB} == set(ec.PROBS)
    assert {(m, p) for m, p in ec.METRIC_PROB if m == "cos"} == {("cos", p) for p in ec.PROBS}
    four, rev = ec.case("layers-4"), ec.case("layers-4-reversed")
    lds = [ec.padded_features(g_, m) for g_, m in zip(four["features"], four["dissimilarity"])]
    assert len(set(lds)) == ec.MAX_LAYERS == 4 and rev["dissimilarity"] == four["dissimilarity"][::-1]
    assert [len(ec.case(f"layers-{n}")["features"]) for n in (1, 2, 3, 4)] == [1, 2, 3, 4]
    deg = ec.case("deg-zero-row-each-side-kl")
    assert not deg["layers_A"][0][69].any() and not deg["layers_B"][0][0].any() and deg["layers_A"][0][1].any()
    assert ec.case("deg-2d-variance")["XA"].shape[1] == 2 and ec.case("deg-2d-variance")["sigma2_variance"] == 2.5
    assert len(ec.case("deg-all-far")["far"]) == 66 and len(ec.case("deg-none-far")["far"]) == 0
    assert len(ec.case("deg-1x1")["XA"]) == len(ec.case("deg-1x1")["XB"]) == 1
    for name in ec.PAIR_CASES:   # the inputs follow the goldens
        c = ec.case(name)
        assert 0.05 <= c["sigma2"] <= 0.5 and np.abs(c["XA"]).max() < 10
    assert set(ec.WRAPPER_CASES) <= set(ec.PAIR_CASES)


@pytest.mark.parametrize("met", ["euc", "square_euc", "cos"])
def test_coincident_rows_give_a_layer_distance_of_exactly_zero(met):
    """On the 1/32 grid |x|^2, |y|^2 and x.y are exact in float64 in every order, so a + b - 2 x.y of coincident rows is 0."""
    c = ec.case(f"deg-duplicates-{met}")
    assert len(c["dup"]) == 20
    for dtype in (np.float64, np.float32):
        (X, Y, a, b, *_), = ec.prepare_layers(c, dtype)
        if met == "cos":
            continue   # unit rows are not on the grid: their distance is a rounding error of 1/2 - 1/2 <x, x>
        assert np.array_equal(X.astype(np.float64), np.pad(c["layers_A"][0], ((0, 0), (0, X.shape[1] - 24))))
        for j in c["dup"]:
            i = int(np.flatnonzero((c["XA"] == c["XB"][j]).all(1))[0])
            assert a[i] + b[j] - 2 * float(X[i].astype(np.float64) @ Y[j].astype(np.float64)) == 0.0
            assert a[i] + b[j] - 2 * float(X[i, ::-1].astype(np.float64) @ Y[j, ::-1].astype(np.float64)) == 0.0


# ------------------------------------------------------------------------------------------------------ float32 operands
@pytest.mark.parametrize("met", sorted(ec.METRICS))
def test_summation_order_moves_few_float32_operands_by_one_ulp(met):
    """The row total of the prepare kernel is summed as 64 interleaved partials and a tree, NumPy's is pairwise: the
    float32-stored operands differ in at most 1e-3 of the elements, by one ulp - what the GPU test holds the device to."""
    rng = np.random.default_rng(7)
    for g_ in (1, 17, 65, 129, 2000):
        labels = rng.integers(0, 5, 257)
        layer = (ec.counts_layer if met in ("kl", "sym_kl") else ec.grid_layer)(rng, g_, labels, 7)
        for side in (0, 1):
            A, a = ec.prepare_reference(layer, met, side, np.float32)
            B, b = ec.prepare_reference(layer, met, side, np.float32, lane_order=True)
            ulps = np.abs(A.astype(np.float64) - B.astype(np.float64)) / np.spacing(np.abs(A)).astype(np.float64)
            assert ulps.max() <= 1.0 and (ulps > 0).mean() <= ec.PREP_F32_FRACTION, (g_, side, ulps.max(), (ulps > 0).mean())
            assert np.abs(a - b).max() <= ec.REF_TOL * max(np.abs(a).max(), 1.0)
            A64, _ = ec.prepare_reference(layer, met, side, np.float64)
            B64, _ = ec.prepare_reference(layer, met, side, np.float64, lane_order=True)
            assert np.abs(A64 - B64).max() <= ec.PREP_F64_TOL * max(1.0, np.abs(A64).max())
