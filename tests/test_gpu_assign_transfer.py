"""GPU tests of ``st.align.apply_assignment`` and of ``apply=`` in the loops and ``Morpho_pairwise``: the assignment applied to cell
features without the dense ``P``.

Against tests/golden/ref_assign_transfer.npz (``P`` of the real ``_update_assignment_P`` times the features, in float64), raw and
normalised, in both cell dtypes: float64 at ``F64_TOL = 1e-10``, float32 at ``max(1.25 x the reference's own float32 floor,
1e-5)``; the raw products relative to ``max (P @ |F|)``, the normalised ones relative to ``max |F|`` over every cell with a
non-zero sum (``_assign_transfer_case``).  In the loops ``applied`` is held to the dense ``P`` of the same last assignment
(``return_P=True``) and, where the run ends on a full assignment of the returned state (SVI), to ``apply_assignment`` on that
state; every other output keeps the bits of the run without the keyword."""
import numpy as np
import pytest

import _align_loop_case as lc
import _align_svi_case as sc
import _assign_case as ac
import _assign_transfer_case as tc
import _morpho_align_case as mc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = ["float64", "float32"]
G = tc.load()
GA = ac.load()
ITERS = 4


def _both(args, kw, dtype, **features):
    from spateo_amd import align

    raw = align.apply_assignment(*args, normalize=False, dtype=dtype, device=DEV, **features, **kw)
    norm = align.apply_assignment(*args, dtype=dtype, device=DEV, **features, **kw)       # normalize=True is the default
    return raw, norm


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag,c", tc.cases(G))
def test_apply_assignment_against_the_golden(tag, c, dtype):
    args, kw = ac.case_inputs(GA, tag)
    F_A, F_B = tc.features(G, tag, c)
    raw, norm = _both(args, kw, dtype, features_A=F_A, features_B=F_B)
    assert sorted(raw) == sorted(norm) == ["K_NA", "K_NB", "to_A", "to_B"]
    ref = tc.golden_ref(G, tag, c)
    tc.check(tc.quantities_of(raw, norm), ref, tc.tolerances(G, tag, c, dtype), what=f"case {tag} C {c} {dtype}")
    sums = ac.tolerances(GA, tag, dtype)
    for q in ("K_NA", "K_NB"):
        assert np.array_equal(raw[q], norm[q])
        assert np.abs(raw[q] - ref[q]).max() <= sums[q] * np.abs(ref[q]).max(), q
    far = GA[f"{tag}_far"]                                   # the far B cells: no partner, a zero row either way
    assert not raw["to_B"][far].any() and not norm["to_B"][far].any()
    live = ref["K_NB"] != 0
    hot = c // 2                                             # the one-hot half: a class distribution per B cell
    assert np.abs(norm["to_B"][live, :hot].sum(1) - 1).max() < 1e-9 and norm["to_B"][:, :hot].min() >= 0
    again, _ = _both(args, kw, dtype, features_A=F_A, features_B=F_B)
    for q in raw:
        assert raw[q].tobytes() == again[q].tobytes(), q     # two calls, the same bits


@pytest.mark.parametrize("dtype", DTYPES)
def test_label_vectors_and_single_directions(dtype):
    from spateo_amd import align

    args, kw = ac.case_inputs(GA, "p")
    NA, NB = len(args[0]), len(args[1])
    rng = np.random.default_rng(3)
    labA, labB = rng.integers(0, 6, NA), rng.integers(0, 3, NB).astype(np.int32)
    labA[0] = 5
    hotA, hotB = np.eye(6)[labA], np.eye(3)[labB]
    call = lambda **f: align.apply_assignment(*args, dtype=dtype, device=DEV, **f, **kw)  # noqa: E731
    by_label, by_matrix = call(features_A=labA, features_B=labB), call(features_A=hotA, features_B=hotB)
    assert by_label["to_B"].shape == (NB, 6) and by_label["to_A"].shape == (NA, 3)
    for q in by_matrix:
        assert by_label[q].tobytes() == by_matrix[q].tobytes(), q
    # every live cell's class distribution sums to 1; the most likely class of a B cell is a class of slice A
    live = by_label["K_NB"] != 0
    assert np.abs(by_label["to_B"][live].sum(1) - 1).max() < 1e-9 and not by_label["to_B"][~live].any()
    # one direction only: the other's entries are absent, the bits are the same
    only_B, only_A = call(features_A=labA), call(features_B=labB)
    assert sorted(only_B) == ["K_NB", "to_B"] and sorted(only_A) == ["K_NA", "K_NB", "to_A"]
    for part in (only_A, only_B):
        for q in part:
            assert part[q].tobytes() == by_label[q].tobytes(), q
    # against the device's own dense P, the float64 bound in both modes (the same stored operands)
    P = align.update_assignment(*args, return_P=True, dtype=dtype, device=DEV, **kw)["P"]
    raw = call(features_A=hotA, features_B=hotB, normalize=False)
    tc.check(tc.quantities_of(raw, by_matrix), tc.products(P, hotA, hotB), {q: ac.F64_TOL for q in tc.QUANTITIES},
             what=f"case p {dtype} against the device's P")


def _equal(a, b, path=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), (path, sorted(a), sorted(b))
        for key in a:
            _equal(a[key], b[key], f"{path}/{key}")
    elif isinstance(a, np.ndarray) and a.dtype.kind == "f":
        assert a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)), path
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    elif hasattr(a, "toarray"):
        assert np.array_equal(a.toarray(), b.toarray()), path
    else:
        assert a == b or (a is None and b is None), path


def _loop_features(NA, NB):
    rng = np.random.default_rng(11)
    return rng.integers(0, 4, NA), rng.standard_normal((NB, 70))      # a label vector; two chunks of columns


def _against_P(applied, P, labA, F_B, what, normalize):
    want = tc.products(P, np.eye(4)[labA], F_B)
    kind = "norm" if normalize else "raw"
    got = {f"to_A_{kind}": applied["to_A"], f"to_B_{kind}": applied["to_B"]}
    tc.check(got, want, {q: ac.F64_TOL for q in tc.QUANTITIES}, what=what)
    for q in ("K_NA", "K_NB"):
        assert np.abs(applied[q] - want[q]).max() <= ac.F64_TOL * np.abs(want[q]).max(), q


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("normalize", [False, True])
def test_morpho_iterate_with_the_keyword(dtype, normalize):
    from spateo_amd import align

    args, kw = lc.case_inputs(lc.load(), "3")
    kw = dict(kw, max_iter=ITERS, dtype=dtype, device=DEV)
    labA, F_B = _loop_features(len(args[0]), len(args[1]))
    plain = align.morpho_iterate(*args, return_P=True, **kw)
    out = align.morpho_iterate(*args, return_P=True, apply=dict(features_A=labA, features_B=F_B, normalize=normalize), **kw)
    applied = out.pop("applied")
    _equal(out, plain)
    assert sorted(applied) == ["K_NA", "K_NB", "to_A", "to_B"] and applied["to_B"].shape == (len(args[1]), 4)
    _against_P(applied, plain["P"], labA, F_B, f"morpho_iterate {dtype}", normalize)
    assert np.array_equal(applied["K_NB"], out["K_NB"])               # the factor kernel's, as the last assignment's


def test_morpho_iterate_with_the_keyword_in_the_sparse_mode():
    """`applied` comes from the kept entries: the returned coo_matrix times F, on the host."""
    from spateo_amd import align

    args, kw = lc.case_inputs(lc.load(), "3")
    kw = dict(kw, max_iter=ITERS, dtype="float64", device=DEV, sparse_calculation_mode=True, sparse_top_k=8)
    labA, F_B = _loop_features(len(args[0]), len(args[1]))
    plain = align.morpho_iterate(*args, **kw)
    out = align.morpho_iterate(*args, apply=dict(features_A=labA, features_B=F_B, normalize=False), **kw)
    applied = out.pop("applied")
    _equal(out, plain)
    P = out["P"].tocsr()
    assert np.array_equal(applied["to_A"], P @ F_B) and np.array_equal(applied["to_B"], P.T @ np.eye(4)[labA])
    assert np.array_equal(applied["K_NA"], out["K_NA"]) and np.array_equal(applied["K_NB"], out["K_NB"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_morpho_iterate_svi_with_the_keyword(dtype):
    from spateo_amd import align

    args, kw = sc.case_inputs(sc.load(), "3")
    kw = dict(kw, max_iter=ITERS, dtype=dtype, device=DEV)
    labA, F_B = _loop_features(len(args[0]), len(args[1]))
    mapped = align.morpho_iterate_svi(*args, return_mapping=True, return_P=True, **kw)
    out = align.morpho_iterate_svi(*args, return_P=True, apply=dict(features_A=labA, features_B=F_B), **kw)   # the closing one comes with it
    applied = out.pop("applied")
    _equal(out, mapped)
    assert mapped["P"].shape == (len(args[0]), len(args[1])) and applied["to_B"].shape == (len(args[1]), 4)
    _against_P(applied, mapped["P"], labA, F_B, f"morpho_iterate_svi {dtype}", True)
    if dtype == "float64":      # the closing assignment reads the returned state: apply_assignment on it is the same thing
        state = dict(dissimilarity=kw["dissimilarity"], probability_type=kw["probability_type"],
                     probability_parameters=kw["probability_parameters"], sigma2=out["sigma2"], alpha=out["alpha"],
                     SigmaDiag=out["SigmaDiag"], gamma=out["gamma"], samples_s=kw["samples_s"], sigma2_variance=out["sigma2_variance"])
        direct = align.apply_assignment(out["XAHat"], args[1], args[2], args[3], features_A=labA, features_B=F_B, dtype=dtype,
                                        device=DEV, **state)
        want = tc.products(mapped["P"], np.eye(4)[labA], F_B)
        for q in ("to_A", "to_B"):
            dev = np.abs(applied[q] - direct[q]).max() / want["scale"][f"{q}_norm"]
            print(f"  svi float64: applied against apply_assignment on the returned state, {q}: {dev:.2e}")
            assert dev <= ac.F64_TOL, (q, dev)


def test_morpho_iterate_svi_with_the_keyword_in_the_sparse_mode():
    from spateo_amd import align

    args, kw = sc.case_inputs(sc.load(), "3")
    kw = dict(kw, max_iter=ITERS, dtype="float64", device=DEV, sparse_calculation_mode=True, sparse_top_k=8)
    labA, F_B = _loop_features(len(args[0]), len(args[1]))
    mapped = align.morpho_iterate_svi(*args, return_mapping=True, **kw)
    out = align.morpho_iterate_svi(*args, apply=dict(features_A=labA, features_B=F_B, normalize=False), **kw)
    applied = out.pop("applied")
    _equal(out, mapped)
    P = out["P"].tocsr()
    assert P.shape == (len(args[0]), len(args[1]))
    assert np.array_equal(applied["to_A"], P @ F_B) and np.array_equal(applied["to_B"], P.T @ np.eye(4)[labA])


@pytest.mark.parametrize("dtype", DTYPES)
def test_morpho_pairwise_apply(dtype):
    from spateo_amd import align

    M = mc.load()
    A, B = mc.pair_samples(M, "1")
    kw = mc.pair_kwargs(M, "1")
    m = align.Morpho_pairwise(A, B, dtype=dtype, device="0", verbose=False, apply=dict(features_A="celltype", features_B="spatial"), **kw)
    P = m.run()
    assert P is not None and P.shape == (m.NA, m.NB)
    cats = list(A.obs["celltype"].cat.categories)
    assert m.applied["categories_A"] == cats and "categories_B" not in m.applied
    hot = np.eye(len(cats))[np.asarray(A.obs["celltype"].cat.codes)]
    F_B = np.asarray(B.obsm["spatial"], dtype=np.float64)
    assert m.applied["to_B"].shape == (m.NB, len(cats)) and m.applied["to_A"].shape == (m.NA, F_B.shape[1])
    want = tc.products(P, hot, F_B)
    tc.check({"to_A_norm": m.applied["to_A"], "to_B_norm": m.applied["to_B"]}, want, {q: ac.F64_TOL for q in tc.QUANTITIES},
             what=f"Morpho_pairwise {dtype}")
    # the same model without the keyword (its last assignment the full one all the same): the same alignment, nothing applied
    off = align.Morpho_pairwise(A, B, dtype=dtype, device="0", verbose=False, **dict(kw, return_mapping=True))
    off.run()
    assert off.applied is None
    assert np.array_equal(off.XAHat, m.XAHat) and np.array_equal(off.P, m.P) and off.sigma2 == m.sigma2
    with pytest.raises(KeyError, match="neither an obs column nor an obsm key"):
        align.Morpho_pairwise(A, B, dtype=dtype, device="0", verbose=False, apply=dict(features_A="nope"), **kw)
