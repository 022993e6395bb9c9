"""No GPU: the reference, the filter and the input designs of tests/test_gpu_rk45_kernels.py, on exactly the inputs that module
runs (tests/_rk45_cases.py builds them for both).

  * the stability filter keeps >= 90 % of every case's starts (with the committed seeds: all of them);
  * the identities of solve_ivp's counters the GPU module turns into expected stats: every step attempt costs 6 evaluations on
    top of 2 initial ones, so rejected = (nfev - 2) / 6 - accepted; the cases hold rejections, fired and unfired paths;
  * the event field behaves as designed: three kinds of starts (leaving rest, entering rest, never moving), each at least twice;
  * the hand-stepped scipy.integrate.RK45 behind status -2 reproduces solve_ivp where the cap is not reached, and the capped
    case has rows on both sides of the cap;
  * mutation sensitivity: a reference built with the mistake a case exists to catch (a planted control point dropped - the last
    one, the last of a chunk, the first of the next; the error norm or the at-rest test over 3 components for d < 3; the event
    threshold at 1.1e-5) moves the compared samples by >= 1000 x the float64 tolerance on every such case;
  * the float32 yardstick D32 (printed; profiles/rk45_kernel_edges.md records it);
  * the arc-length rule of _rk45_cases.resample is oracle.trajectory_oracle.fate_arclength's.
Run with ``-s`` to see the filter counts and D32."""
import numpy as np
import pytest

import _rk45_cases as rc

N_CHECK = 101


def _samples(sols, case, sampling="uniform_time", n_out=N_CHECK):
    return [rc.resample_sol(s, case["t_bound"], n_out, sampling)[1][:, : case["d"]] for s in sols]


def _moved(case, mutated):
    """Largest deviation of the compared samples (uniform_time, 101 samples) in float64 tolerances."""
    ref = _samples(rc.reference(case), case)
    return max(float(np.abs(a - b).max()) for a, b in zip(ref, _samples(mutated, case))) / (rc.TOL_X64 * rc.data_extent(case))


def _solve_all(case, f, **kw):
    return [rc.solve(f, y0, case["t_bound"], case["max_step"], **kw) for y0 in rc.world_starts(case)]


ALL_CASES = {c["name"]: c for dt in rc.DTYPES for c in rc.sweep_cases(dt)}


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_filter_and_counter_identities(name):
    case = ALL_CASES[name]
    assert len(case["starts"]) <= 24
    sols, kept = rc.reference(case), rc.kept(case)
    print(f"filter {name}: kept {int(kept.sum())} of {len(kept)}; steps {min(len(s.t) for s in sols) - 1}.."
          f"{max(len(s.t) for s in sols) - 1}, rejected {sum(rc.rejected(s) for s in sols)}, fired {sum(s.status == 1 for s in sols)}")
    assert kept.sum() >= rc.KEEP_MIN * len(kept)
    assert kept.all()   # the committed seeds
    for s in sols:
        assert s.status in (0, 1) and (s.nfev - 2) % 6 == 0 and rc.rejected(s) >= 0
        assert len(s.t) - 1 <= 70   # cost: about 40 to 60 steps


def test_cases_hold_rejections_and_both_statuses():
    for dt in rc.DTYPES:
        for case in (rc.lane_case(dt), rc.free_case(dt), rc.count_case(dt, rc.CAP[dt] + 1)):
            rej = [rc.rejected(s) for s in rc.reference(case)]
            assert sum(r > 0 for r in rej) >= 3 and 0 in rej, (case["name"], rej)
    assert rc.CAP == {"float32": 3072, "float64": 2304}
    for dt in rc.DTYPES:
        cap = rc.CAP[dt]
        assert rc.planted(cap - 1, cap) == [cap - 2] and rc.planted(cap, cap) == [cap - 1]
        assert rc.planted(cap + 1, cap) == [cap - 1, cap]
        assert rc.planted(2 * cap + 1, cap) == [cap - 1, cap, 2 * cap - 1, 2 * cap]
        assert {m % 4 for m in rc.count_ms(dt) if 0 < m < 16} == {0, 1, 3}


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_event_field_has_the_three_kinds_of_starts(d, sign):
    case = rc.event_case(d, sign)
    f = rc.field64(case)
    leaves = enters = still = 0
    for y0, sol in zip(rc.world_starts(case), rc.reference(case)):
        rest0 = bool(np.all(np.abs(f(y0)) < 1e-5))
        if sol.status == 1 and rest0:
            leaves += 1
            assert len(sol.t) - 1 < 25 and 2e4 < abs(sol.t[-1]) < 4e4      # (-20.9, 0.3, -0.2) forward: 18 steps, t = 29858
        elif sol.status == 1:
            enters += 1
            assert 4e4 < abs(sol.t[-1]) < 6e4                               # (-20.0, ...) backward: t = -49433
        else:
            assert rest0 and rc.motion(sol.y.T) == 0.0 and sol.t[-1] == case["t_bound"]   # a path of length exactly 0
            still += 1
    assert min(leaves, enters, still) >= 2, (leaves, enters, still)


def test_hand_stepped_rk45_is_solve_ivp_and_the_capped_case_straddles_the_cap():
    case = rc.free_case("float64")
    f = rc.field64(case)
    for y0, sol in zip(rc.world_starts(case)[:3], rc.reference(case)):   # no cap reached, no event: the same steps
        c = rc.capped_reference(f, y0, case["t_bound"], case["max_step"], 100_000)
        assert sol.status == 0 and c["status"] == 0 and c["accepted"] == len(sol.t) - 1 and c["rejected"] == rc.rejected(sol)
        np.testing.assert_array_equal(c["t"], sol.t)
        np.testing.assert_array_equal(c["x"], sol.y.T)
        tq = np.linspace(0, case["t_bound"], 50)
        np.testing.assert_array_equal(c["dense"](tq), sol.sol(tq))
    case = rc.capped_case()
    f = rc.field64(case)
    refs, kept = rc.capped_references(case)
    assert kept.all()
    status = [r["status"] for r in refs]
    assert status.count(0) >= 2 and status.count(-2) >= 3, status
    at_rest_done = 0
    for y0, r in zip(rc.world_starts(case), refs):
        assert r["accepted"] + r["rejected"] == rc.CAPPED_STEPS if r["status"] == -2 else r["accepted"] + r["rejected"] <= rc.CAPPED_STEPS
        rest = {bool(np.all(np.abs(f(x)) < 1e-5)) for x in r["x"]}
        assert len(rest) == 1, "no event inside the capped steps"
        if r["status"] == 0:
            assert r["t"][-1] == case["t_bound"]
        at_rest_done += rest == {True} and r["status"] == 0
    assert at_rest_done >= 2   # rows at rest that finish within the cap, with their normal status
    assert any(r["status"] == -2 and r["accepted"] == 5 and rc.motion(r["x"]) == 0.0 for r in refs)   # capped on a path of length 0
    assert any(r["status"] == -2 and r["accepted"] >= 2 for r in refs)
    assert case["max_step"] >= abs(case["t_bound"])


def _planted_cases():
    out = []
    for dt in rc.DTYPES:
        cap = rc.CAP[dt]
        for case in [rc.lane_case(dt)] + [rc.count_case(dt, m) for m in rc.count_ms(dt) if m]:
            m = len(case["ctrl"])
            for j in (range(m) if m < 16 else rc.planted(m, cap)):   # a short list: every index, the whole unroll-by-4 remainder
                what = "last" if j == m - 1 else ("chunk end" if (j + 1) % cap == 0 else ("chunk start" if j % cap == 0 and j else "remainder"))
                out.append(pytest.param(case, j, id=f"{dt} m={m} drop {j} ({what})"))
    return out


@pytest.mark.parametrize("case,j", _planted_cases())
def test_dropping_a_planted_control_point_is_a_gross_error(case, j):
    moved = _moved(case, _solve_all(case, rc.field64(case, drop=[j])))
    print(f"{case['name']}: without control point {j} the samples move by {moved:.3g} tolerances")
    assert moved >= rc.MUTATION_FACTOR


def test_planted_points_cover_the_chunk_boundaries():
    ids = {p.id for p in _planted_cases()}
    for dt in rc.DTYPES:
        cap = rc.CAP[dt]
        for m, j in [(cap + 1, cap - 1), (cap + 1, cap), (2 * cap + 1, 2 * cap - 1), (2 * cap + 1, 2 * cap), (2 * cap, cap),
                     (cap, cap - 1), (5, 4), (1, 0), (3, 0), (3, 1), (3, 2), (4, 0), (5, 0)]:
            assert any(i.startswith(f"{dt} m={m} drop {j} ") for i in ids), (dt, m, j)


def _pad3(f, d):
    def g(y):
        v = np.zeros(3)
        v[:d] = f(y[:d])
        return v
    return g


@pytest.mark.parametrize("d", [1, 2])
def test_a_norm_over_three_components_is_a_gross_error(d):
    """SciPy on a 3-vector state whose tail is zero: the RMS norms divide by sqrt(3)."""
    cases = [rc.dim_case(dt, d) for dt in rc.DTYPES] + ([rc.world_cases(dt)[1] for dt in rc.DTYPES] if d == 2 else [])
    for case in {c["name"]: c for c in cases}.values():
        f3 = _pad3(rc.field64(case), d)
        sols = [rc.solve(f3, np.concatenate([y0, np.zeros(3 - d)]), case["t_bound"], case["max_step"]) for y0 in rc.world_starts(case)]
        moved = _moved(case, sols)
        print(f"{case['name']}: the norm over 3 components moves the samples by {moved:.3g} tolerances")
        assert moved >= rc.MUTATION_FACTOR


@pytest.mark.parametrize("d", [1, 2, 3])
def test_event_threshold_and_at_rest_over_three_components_are_gross_errors(d):
    for sign in (1.0, -1.0) if d == 3 else (1.0,):
        case = rc.event_case(d, sign)
        moved = _moved(case, _solve_all(case, rc.field64(case), threshold=1.1e-5))
        print(f"{case['name']}: a threshold of 1.1e-5 moves the samples by {moved:.3g} tolerances")
        assert moved >= rc.MUTATION_FACTOR
    if d < 3:   # the unused columns of C hold garbage: a kernel that looked at them would never see the field at rest
        case = rc.event_case(d, 1.0)
        g = rc.with_garbage(case)
        np.testing.assert_array_equal(rc.field64(g)(rc.world_starts(case)[0]), rc.field64(case)(rc.world_starts(case)[0]))
        moved = _moved(case, _solve_all(case, rc.field64(case), rest_field=rc.field64(g, components=3)))
        print(f"{case['name']}: the at-rest test over 3 components moves the samples by {moved:.3g} tolerances")
        assert moved >= rc.MUTATION_FACTOR


def test_float32_yardstick():
    for sampling in rc.SAMPLINGS:
        rows = [(c["name"], rc.float32_deviation(c, sampling)) for c in rc.float32_cases()]
        for name, dev in rows:
            print(f"D32 {sampling} {name}: {dev:.3g}")
        d32 = rc.d32(sampling)
        print(f"D32({sampling}) = {d32:.4g}; float32 state tolerance = {rc.D32_FACTOR} x D32 = {rc.D32_FACTOR * d32:.4g} of the extent of"
              f" motion ({'above' if rc.D32_FACTOR * d32 > 2e-3 else 'below'} the 2e-3 of the float32 morphopath test)")
        assert d32 == max(d for _, d in rows) and 0 < d32 < 2e-2
        capped = rc.d32_capped(sampling)
        print(f"D32 of the status -2 case ({sampling}) = {capped:.4g}; tolerance {rc.D32_FACTOR * capped:.4g}")
        assert 0 < capped < 2e-2
    agree = [(a.status == b.status) for c in rc.float32_cases() for a, b in zip(rc.reference(c), rc.reference32(c))]
    print(f"status agrees between the two CPU routes on {sum(agree)} of {len(agree)} starts")
    assert sum(agree) >= 0.9 * len(agree)


def test_float32_restatement_is_the_field_to_float32_accuracy():
    for case in (rc.count_case("float32", 5), rc.count_case("float32", rc.CAP["float32"] + 1), rc.event_case(1, 1.0), rc.event_case(2, 1.0),
                 rc.event_case(3, 1.0), rc.event_case(3, -1.0), rc.world_cases("float32")[0]):
        f64, f32 = rc.field64(case), rc.field32(case)
        vs = np.array([[f64(y), f32(y)] for y in rc.world_starts(case)])
        assert np.abs(vs[:, 0] - vs[:, 1]).max() <= rc.FIELD32_RTOL * np.abs(vs[:, 0]).max()
        assert np.abs(vs[:, 0] - vs[:, 1]).max() > 0


@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_arc_length_rule_is_fate_arclength(direction):
    from oracle import trajectory_oracle as tro

    n = 40
    case = rc.lane_case("float64", 1.0 if direction == "forward" else -1.0)
    assert case["max_step"] == rc.T_MOVING / n
    T, Y = tro.fate_arclength(rc.field64(case), rc.world_starts(case)[:4], rc.T_MOVING, n, direction)
    for sol, t, y in zip(rc.reference(case), T, Y):
        tq, x = rc.resample_sol(sol, case["t_bound"], n, "arc_length")
        np.testing.assert_array_equal(tq, t)
        np.testing.assert_array_equal(x, y)
