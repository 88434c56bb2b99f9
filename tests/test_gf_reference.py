"""The restatement tests/gf_ref.py of the global fusion, checked on the CPU: its float64 and long-double runs take the same decisions
on every named chain (tests/gf_inputs.py) with every deciding quantity well away from its threshold, the substructured algebra of
the device equals the dense normal equations at several S, and the closed-form Jacobians the device writes equal both the explicit
6 x 4 . 4 x 3 product and central differences through Plus."""
import numpy as np
import pytest

import gf_inputs
import gf_ref

K_BAR = 32
NAMES = list(gf_inputs.CASES)
INTS = ("status", "termination", "iterations", "successful_steps", "unsuccessful_steps")


def bar_of(x64, x80):
    return max(K_BAR * float(np.abs(x64 - x80).max()), 1e-12 * float(np.abs(x64).max()))


@pytest.mark.parametrize("name", NAMES)
def test_both_precisions_decide_alike_and_far_from_every_threshold(name):
    r64, r80 = gf_inputs.ref_case(name, "f64"), gf_inputs.ref_case(name, "f80")
    for k in INTS:
        assert r64[k] == r80[k], (name, k)
    assert r64["verdicts"] == r80["verdicts"], name
    assert len(r64["decisions"]) == len(r80["decisions"])
    for r in (r64, r80):
        for value, threshold in r["decisions"]:
            big = max(abs(value), abs(threshold))
            assert big == 0 or abs(value - threshold) >= 1e-6 * big, (name, value, threshold)
    for a, b in zip(r64["decisions"], r80["decisions"]):
        assert (a[0] > a[1]) == (b[0] > b[1]), name


def test_the_named_cases_are_what_their_names_say():
    r = {n: gf_inputs.ref_case(n, "f64") for n in NAMES}
    sizes = {n: len(gf_inputs.case(n)["local"]) for n in NAMES}
    assert {1, 2, 3, 4, 5, 8, 9, 41, 2 * gf_ref.DEFAULT_SEGMENT + 3} <= set(sizes.values())
    assert all(gf_inputs.case(n)["opt"]["segment"] == 4 for n in NAMES if n != "default_segment")
    assert gf_inputs.case("default_segment")["opt"]["segment"] == 0
    assert gf_ref.plan(4, 4) == ([3], [(0, 3), (4, 4)]) and gf_ref.plan(3, 4) == ([], [(0, 3)])
    assert gf_ref.plan(41, 4)[1][-1] == (40, 41)                                     # a ragged last segment
    assert list(gf_inputs.case("fix_places")["gps_node"]) == [0, 2, 3, 4, 13]          # beside, on, behind separator 3; both ends
    assert r["n1"]["iterations"] == 0 and r["n1_fix"]["iterations"] >= 1
    assert r["no_fix"]["iterations"] == 0 and r["no_fix"]["termination"] == gf_ref.CONVERGENCE and float(r["no_fix"]["initial_cost"]) < 1e-20
    v_ = r["reject"]["verdicts"]
    assert "reject" in v_ and "accept" in v_[v_.index("reject"):], v_                # a rejection followed by an acceptance
    assert r["no_convergence"]["termination"] == gf_ref.NO_CONVERGENCE and r["no_convergence"]["iterations"] == 5
    assert r["ftol"]["verdicts"][-1] == "function_tolerance" and r["ptol"]["verdicts"][-1] == "parameter_tolerance"

    def huber_sides(name):   # of the fixes at the start: the first len(fixes) Huber decisions
        m = len(gf_inputs.case(name)["gps_node"])
        return [bool(s > b) for s, b in r[name]["decisions"][:m]]
    assert not any(huber_sides("all_inside")) and all(huber_sides("all_outside"))
    m = len(gf_inputs.case("outlier")["gps_node"])
    assert [bool(s > 1000 * b) for s, b in r["outlier"]["decisions"][:m]] == [i == 4 for i in range(m)]   # one fix, tens of metres off
    # Huber tames the gross outlier: the poses stay near the run without that fix
    g = gf_inputs.case("outlier")
    keep = [i for i in range(len(g["gps_node"])) if i != 4]
    clean = gf_ref.optimize(g["local"], g["glob"], g["gps_node"][keep], g["gps_xyz"][keep], g["gps_accuracy"][keep], g["opt"])
    assert np.abs(clean["pose"][:, :3] - r["outlier"]["pose"][:, :3]).max() < 1.0
    # the yawed frame comes most of the way back in its five iterations (two of them rejected): from 50 m off to within 10 m
    g = gf_inputs.case("yawed_frame")
    assert np.abs(g["glob"][g["gps_node"], :3] - g["gps_xyz"]).max() > 40
    assert np.abs(r["yawed_frame"]["pose"][g["gps_node"], :3] - g["gps_xyz"]).max() < 10.0
    assert "reject" in r["yawed_frame"]["verdicts"]
    a = np.unwrap(np.arctan2(gf_inputs.case("turning")["local"][:, 1], gf_inputs.case("turning")["local"][:, 0]))
    assert abs(a[-1] - a[0]) > 2 * np.pi


@pytest.mark.parametrize("name", NAMES)
def test_chain_algebra_equals_the_dense_normal_equations(name):
    r64, r80, d80 = gf_inputs.ref_case(name, "f64"), gf_inputs.ref_case(name, "f80"), gf_inputs.ref_case(name, "f80", "dense")
    x64, x80, xd = gf_ref.solution(r64), gf_ref.solution(r80), gf_ref.solution(d80)
    bar = bar_of(x64, x80)
    n = len(gf_inputs.case(name)["local"])
    for S in (None, 2, 3, 7, n + 1):
        c80 = r80 if S is None else gf_inputs.ref_case(name, "f80", "chain", S)
        for k in INTS:
            assert c80[k] == d80[k], (name, S, k)
        assert c80["verdicts"] == d80["verdicts"]
        err = float(np.abs(gf_ref.solution(c80) - xd).max())
        print(name, "S", S, "chain - dense %.3g, bar %.3g" % (err, bar))
        assert err <= bar, (name, S)


def _random_edge(rng, ld):
    def pose():
        q = rng.normal(0, 1, 4)
        q = q / np.linalg.norm(q) * rng.uniform(0.9, 1.1)    # not quite unit: the functor normalises where it rotates
        return np.array([*rng.normal(0, 3, 3), *q], dtype=ld)
    m = rng.normal(0, 1, 4)
    return pose(), pose(), np.array([*rng.normal(0, 1, 3), *(m / np.linalg.norm(m))], dtype=ld)


def test_closed_form_jacobians_match_the_product_and_central_differences():
    ld = np.longdouble
    rng = np.random.default_rng(5)
    tv, qv = ld(0.1), ld(0.01)
    for trial in range(6):
        xi, xj, meas = _random_edge(rng, ld)
        Ji, Jj = gf_ref.edge_jac_closed(xi, xj, meas, tv, qv)
        Pi, Pj = gf_ref.edge_jac_product(xi, xj, meas, tv, qv)
        size = max(float(np.abs(Pi).max()), float(np.abs(Pj).max()))
        assert np.abs(Ji - Pi).max() <= 1e-16 * size and np.abs(Jj - Pj).max() <= 1e-16 * size, trial
        h = ld(1e-7)
        for which, J in ((0, Ji), (1, Jj)):
            for c in range(6):
                d = np.zeros(6, dtype=ld)
                d[c] = h
                z = np.zeros(6, dtype=ld)
                lo = gf_ref.edge_residual(gf_ref.plus(xi, -d if which == 0 else z), gf_ref.plus(xj, -d if which == 1 else z), meas, tv, qv)
                hi = gf_ref.edge_residual(gf_ref.plus(xi, d if which == 0 else z), gf_ref.plus(xj, d if which == 1 else z), meas, tv, qv)
                assert np.abs((hi - lo) / (2 * h) - J[:, c]).max() < 1e-9 * size, (trial, which, c)
    # Plus: the identity at zero, |delta| and not half of it, and its Jacobian at zero
    x = _random_edge(rng, ld)[0]
    assert np.array_equal(gf_ref.plus(x, np.zeros(6, dtype=ld)), x)
    d = np.array([0.3, 0, 0, 0, 0, 0], dtype=ld)
    unit = np.array([0, 0, 0, 1, 0, 0, 0], dtype=ld)
    assert np.abs(gf_ref.plus(unit, d)[3:] - np.array([np.cos(ld(0.3)), np.sin(ld(0.3)), 0, 0], dtype=ld)).max() < 1e-18
    for c in range(3):
        d = np.zeros(6, dtype=ld)
        d[c] = ld(1e-7)
        num = (gf_ref.plus(x, d)[3:] - gf_ref.plus(x, -d)[3:]) / ld(2e-7)
        assert np.abs(num - gf_ref.plus_jacobian(x[3:])[:, c]).max() < 1e-12
