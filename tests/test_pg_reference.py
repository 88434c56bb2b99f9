"""The restatement tests/pg_ref.py of the pose-graph optimisation, checked on the CPU: its float64 and long-double runs take the
same decisions on every named case (tests/pg_inputs.py) with every deciding quantity well away from its threshold, the banded
algebra of the device equals the dense normal equations, the analytic Jacobians equal central differences, and a graph that is a
pure yaw-and-shift of a consistent trajectory gets exactly that drift."""
import ctypes as C

import numpy as np
import pytest

import vplines_slam_amd as v

import pg_inputs
import pg_ref

K_BAR = 32
NAMES = list(pg_inputs.CASES)
INTS = ("status", "termination", "iterations", "successful_steps", "unsuccessful_steps")


def bar_of(x64, x80):
    return max(K_BAR * float(np.abs(x64 - x80).max()), 1e-12 * float(np.abs(x64).max()))


@pytest.mark.parametrize("name", NAMES)
def test_both_precisions_decide_alike_and_far_from_every_threshold(name):
    r64, r80 = pg_inputs.ref_case(name, "f64"), pg_inputs.ref_case(name, "f80")
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


def test_the_named_cases_end_the_way_their_names_say():
    r = {n: pg_inputs.ref_case(n, "f64") for n in NAMES}
    v_ = r["reject"]["verdicts"]
    assert "reject" in v_ and "accept" in v_[v_.index("reject"):], v_          # a rejection followed by an acceptance
    assert r["reject"]["unsuccessful_steps"] >= 1
    assert r["ftol"]["verdicts"] == ["accept", "function_tolerance"]
    assert r["ptol"]["verdicts"][-1] == "parameter_tolerance"
    assert r["five"]["iterations"] == 5 and r["no_convergence"]["termination"] == pg_ref.NO_CONVERGENCE
    assert r["n1"]["iterations"] == 0 and r["n1"]["successful_steps"] == 0
    assert r["no_loops"]["iterations"] == 0                                   # the gradient tolerance holds at the start
    assert pg_inputs.ref_case("mixed_sequence", "f64")["status"] == pg_ref.UNSUPPORTED
    # Huber tames the gross outlier: the poses stay within centimetres of the run without that edge
    g = pg_inputs.case("outlier")
    ll = g["loop_local"].copy()
    ll[22] = -1
    clean = pg_ref.optimize(g["vio_T"], g["vio_R"], ll, g["loop_info"])
    assert np.abs(clean["T"] - r["outlier"]["T"]).max() < 0.3
    sizes = {n: len(pg_inputs.case(n)["vio_T"]) for n in NAMES}
    assert {1, 2, 5, 6, 18, 24, 40} <= set(sizes.values())
    assert pg_inputs.case("n6_loop_to_0")["loop_local"][5] == 0


@pytest.mark.parametrize("name", NAMES)
def test_banded_algebra_equals_the_dense_normal_equations(name):
    r64, r80, d80 = pg_inputs.ref_case(name, "f64"), pg_inputs.ref_case(name, "f80"), pg_inputs.ref_case(name, "f80", "dense")
    for k in INTS:
        assert r80[k] == d80[k], (name, k)
    assert r80["verdicts"] == d80["verdicts"]
    x64, x80, xd = pg_ref.solution(r64), pg_ref.solution(r80), pg_ref.solution(d80)
    err, bar = float(np.abs(x80 - xd).max()), bar_of(x64, x80)
    print(name, "banded - dense %.3g, bar %.3g" % (err, bar))
    assert err <= bar


@pytest.mark.parametrize("loop", [False, True])
def test_analytic_jacobians_match_central_differences(loop):
    ld = np.longdouble
    rng = np.random.default_rng(5)
    for trial in range(6):
        xa = np.array([rng.uniform(-170, 170), *rng.normal(0, 3, 3)], dtype=ld)
        xb = np.array([rng.uniform(-170, 170), *rng.normal(0, 3, 3)], dtype=ld)
        pra = np.array(rng.uniform(-10, 10, 2), dtype=ld)
        meas = np.array([*rng.normal(0, 1, 3), xb[0] - xa[0] + rng.uniform(-20, 20)], dtype=ld)
        div = ld(10) if loop else ld(1)
        _, Ja, Jb = pg_ref.edge_eval(xa, xb, pra, meas, div)
        h = ld(1e-7)
        for which, J in ((0, Ja), (1, Jb)):
            for c in range(4):
                d = np.zeros(4, dtype=ld)
                d[c] = h
                lo = pg_ref.edge_eval(xa - d * (which == 0), xb - d * (which == 1), pra, meas, div, False)[0]
                hi = pg_ref.edge_eval(xa + d * (which == 0), xb + d * (which == 1), pra, meas, div, False)[0]
                assert np.abs((hi - lo) / (2 * h) - J[:, c]).max() < 1e-9, (trial, which, c)


def test_drift_of_a_pure_yaw_and_shift_is_that_yaw_and_shift():
    """a consistent trajectory: the loop edges agree with the VIO poses, so nothing moves and the drift is zero; then the same
    graph with the optimised window's VIO poses turned and shifted as a whole keeps its relative geometry, so the poses stay put
    and node n-1 -- which the drift is read from -- reports exactly that turn and shift against a VIO pose given without it"""
    g = pg_inputs.make_graph(12, [], 31, yaw_drift=0.0, t_drift=(0, 0, 0))
    n = 12
    Rq = [pg_ref.qmat(pg_ref.mat2q(R)) for R in g["vio_R"]]
    eul = [pg_ref.R2ypr(R) for R in Rq]
    ll, li = g["loop_local"].copy(), g["loop_info"].copy()
    for (i, a) in ((9, 1), (11, 2)):
        ll[i] = a
        li[i, :3] = Rq[a].T.dot(g["vio_T"][i] - g["vio_T"][a])
        li[i, 7] = eul[i][0] - eul[a][0]
    r = pg_ref.optimize(g["vio_T"], g["vio_R"], ll, li)
    assert abs(r["yaw_drift"]) < 1e-9 and np.abs(r["t_drift"]).max() < 1e-9 and np.abs(r["T"] - g["vio_T"]).max() < 1e-9
    # the drift formula itself (pose_graph.cpp:549-557): corrected pose = turn * vio + shift
    yaw, shift = 7.5, np.array([0.4, -1.1, 0.2])
    turn = pg_ref.ypr2R(np.array([yaw, 0.0, 0.0]))
    T2 = g["vio_T"].dot(turn.T) + shift
    R2 = np.array([turn.dot(R) for R in g["vio_R"]])
    r2 = pg_ref.optimize(T2, R2, ll, li)
    assert np.abs(r2["T"] - T2).max() < 1e-9                                   # still consistent: nothing moves
    cur_R, cur_T = r2["R"][n - 1], r2["T"][n - 1]
    yaw_drift = pg_ref.R2ypr(cur_R)[0] - pg_ref.R2ypr(g["vio_R"][n - 1])[0]
    rd = pg_ref.ypr2R(np.array([yaw_drift, 0.0, 0.0]))
    assert abs(pg_ref.norm_angle(np.float64(yaw_drift - yaw))) < 1e-9
    assert np.abs(cur_T - rd.dot(g["vio_T"][n - 1]) - shift).max() < 1e-9
    # and on a graph that does move: the reported drift carries the VIO pose of node n-1 onto its corrected pose
    g, r = pg_inputs.case("n40"), pg_inputs.ref_case("n40", "f64")
    assert abs(r["yaw_drift"]) > 0.01
    assert np.abs(r["r_drift"].dot(g["vio_T"][-1]) + r["t_drift"] - r["T"][-1]).max() < 1e-12
    assert abs(pg_ref.R2ypr(r["r_drift"].dot(g["vio_R"][-1]))[0] - r["x"][-1, 0]) < 1e-9
    assert np.abs(r["tail_T"] - (g["tail_T"].dot(r["r_drift"].T) + r["t_drift"])).max() < 1e-12


def test_default_options_and_struct_layouts():
    o = v.default_pg_options()
    ref = pg_ref.default_options()
    for f, _ in v.capi.PgOptions._fields_:
        assert getattr(o, f) == ref[f], f
    assert C.sizeof(v.capi.PgOptions) == 8 + 11 * 8
    assert C.sizeof(v.capi.CPgInput) == 8 + 7 * 8
    assert C.sizeof(v.capi.CPgResult) == 6 * 4 + 8 * (3 + 9 + 3) + 4 * 8
    assert (v.capi.PG_MAX_NODES, v.capi.PG_MAX_LOOPS) == (4096, 256)
