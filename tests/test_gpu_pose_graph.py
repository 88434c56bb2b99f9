"""vpl_pg_optimize_batch on the device against the sequential restatement tests/pg_ref.py (banded algebra) on the named graphs of
tests/pg_inputs.py.

Integers, termination and status are equal.  The solution vector -- T, R, t_drift, r_drift, yaw_drift, final cost -- is held to the
project's bar: max(32 max |x64 - x80|, 1e-12 |x64|_inf), x64 / x80 the restatement's float64 and np.longdouble runs;
tests/test_pg_reference.py holds the two to the same decisions with every deciding quantity 1e-6 away from its threshold.  A batch
follows its items and repeats bit for bit; vpl_pg_debug_step's g, first step and model cost change are compared with the dense
long-double solve of the same system."""
import numpy as np
import pytest

import vplines_slam_amd as v

import pg_inputs
import pg_ref

pytestmark = pytest.mark.gpu

K_BAR = 32
NAMES = list(pg_inputs.CASES)
INTS = ("status", "termination", "iterations", "successful_steps", "unsuccessful_steps")


def graph_input(name):
    g = pg_inputs.case(name)
    return v.PoseGraphInput(g["vio_T"], g["vio_R"], g["loop_local"], g["loop_info"], g["sequence"], g["tail_T"], g["tail_R"])


def options(name):
    return v.default_pg_options(**pg_inputs.case(name)["opt"])


def opt_key(name):
    return tuple(sorted(pg_inputs.case(name)["opt"].items()))


def got_dict(res):
    return dict(T=res.T, R=res.R, t_drift=np.array(res.t_drift[:]), r_drift=np.array(res.r_drift[:]), yaw_drift=res.yaw_drift,
                final_cost=res.final_cost)


def check(name, res):
    r64, r80 = pg_inputs.ref_case(name, "f64"), pg_inputs.ref_case(name, "f80")
    print(name, {k: getattr(res, k) for k in INTS}, "reference", {k: r64[k] for k in INTS}, r64["verdicts"])
    for k in INTS:
        assert getattr(res, k) == r64[k], (name, k, getattr(res, k), r64[k])
    x64, x80, x = pg_ref.solution(r64), pg_ref.solution(r80), pg_ref.solution(got_dict(res))
    d = float(np.abs(x64 - x80).max())
    bar = max(K_BAR * d, 1e-12 * float(np.abs(x64).max()))
    err = float(np.abs(x - x64).max())
    print("   error %.3g, bar %.3g (|x64 - x80| %.3g)" % (err, bar, d))
    assert err <= bar, (name, err, bar, d)
    ic = float(r64["initial_cost"])
    assert abs(res.initial_cost - ic) <= 1e-12 * max(ic, 1e-300) + 32 * abs(ic - float(r80["initial_cost"]))


@pytest.mark.parametrize("name", NAMES)
def test_pose_graph_matches_the_sequential_restatement(gpu_ctx, name):
    res = gpu_ctx.pose_graph_optimize([graph_input(name)], options(name))
    check(name, res[0])


def test_pose_graph_batch_follows_the_items_and_repeats_bit_for_bit(gpu_ctx):
    plain = [n for n in NAMES if opt_key(n) == ()]
    assert "ftol" in plain and "five" in plain and "n1" in plain      # a graph that ends early beside a five-iteration one
    first = {}
    for order in (plain, ["five", "ftol"] + [n for n in plain[::-1] if n not in ("five", "ftol")], ["ftol", "five"]):
        inputs = [graph_input(n) for n in order]
        res = gpu_ctx.pose_graph_optimize(inputs)
        again = gpu_ctx.pose_graph_optimize(inputs)
        for i, n in enumerate(order):
            check(n, res[i])
            assert res[i].data() == again[i].data(), n
            assert first.setdefault(n, res[i].data()) == res[i].data(), n     # the same bytes in every order and batch
    for group in (["reject"], ["reject", "reject"]):
        res = gpu_ctx.pose_graph_optimize([graph_input(n) for n in group], options("reject"))
        for i, n in enumerate(group):
            check(n, res[i])
            assert first.setdefault(n, res[i].data()) == res[i].data(), n


@pytest.mark.parametrize("name", ["n2", "n6_loop_to_0", "n18", "circle24", "n40", "n120", "same_old", "three_apart", "yaw_crossing", "outlier", "reject"])
def test_first_step_against_the_dense_long_double_solve(gpu_ctx, name):
    got = gpu_ctx.pose_graph_debug_step(graph_input(name), options(name))
    exact = pg_inputs.ref_case(name, "f80", "dense")["first"]
    own = pg_inputs.ref_case(name, "f64", "banded")["first"]
    ld = np.longdouble
    for key, mine in (("g", got["g"]), ("step", got["step"]), ("model", np.array([got["model_cost_change"]]))):
        ex = np.atleast_1d(np.asarray(exact[key], ld))
        ref_err = float(np.abs(np.atleast_1d(np.asarray(own[key], ld)) - ex).max())
        err = float(np.abs(np.asarray(mine, ld) - ex).max())
        bar = max(K_BAR * ref_err, 1e-12 * float(np.abs(ex).max()))
        print("%s %s: error %.3g, the float64 restatement's %.3g, ratio %.3g, bar %.3g" % (name, key, err, ref_err, err / max(ref_err, 1e-300), bar))
        assert err <= bar, (name, key, err, bar)


def test_tail_and_drift(gpu_ctx):
    for name in ("n40", "n6_loop_to_0", "n1"):
        g = pg_inputs.case(name)
        res = gpu_ctx.pose_graph_optimize([graph_input(name)])[0]
        rd, td = np.array(res.r_drift[:]).reshape(3, 3), np.array(res.t_drift[:])
        assert len(res.tail_T) == len(g["tail_T"]) > 0
        assert np.abs(res.tail_T - (g["tail_T"].dot(rd.T) + td)).max() <= 1e-12
        assert np.abs(res.tail_R - np.array([rd.dot(R) for R in g["tail_R"]])).max() <= 1e-12
        assert np.abs(rd.dot(g["vio_T"][-1]) + td - res.T[-1]).max() <= 1e-12
        assert np.abs(rd - pg_ref.ypr2R(np.array([res.yaw_drift, 0.0, 0.0]))).max() <= 1e-12
    assert res.iterations == 0 and np.abs(res.T - g["vio_T"]).max() == 0 and np.abs(res.R[0] - g["vio_R"][0]).max() < 1e-12   # n = 1


def test_pose_graph_refusals(gpu_ctx):
    o = v.default_pg_options()
    ref = pg_ref.default_options()
    for f, _ in v.capi.PgOptions._fields_:
        assert getattr(o, f) == ref[f], f
    q = graph_input("n5")
    assert gpu_ctx.pose_graph_optimize([q], v.default_pg_options(initial_radius=0.0), check=False) == -1
    assert gpu_ctx.pose_graph_optimize([q], v.default_pg_options(max_iterations=-1), check=False) == -1
    assert gpu_ctx.pose_graph_optimize([q], v.default_pg_options(loop_yaw_scale=0.0), check=False) == -1
    ci = q.to_c()
    ci.vio_R = None
    assert gpu_ctx.pose_graph_optimize([ci], check=False) == -1
    g = pg_inputs.case("n5")
    bad = g["loop_local"].copy()
    bad[2] = 2
    assert gpu_ctx.pose_graph_optimize([v.PoseGraphInput(g["vio_T"], g["vio_R"], bad, g["loop_info"])], check=False) == -1
    n = v.capi.PG_MAX_NODES + 1
    eye = np.tile(np.eye(3), (n, 1, 1))
    big = v.PoseGraphInput(np.zeros((n, 3)), eye, -np.ones(n), np.zeros((n, 8)))
    assert gpu_ctx.pose_graph_optimize([big], check=False) == -4
    n = v.capi.PG_MAX_LOOPS + 2
    many = v.PoseGraphInput(np.zeros((n, 3)), eye[:n], np.arange(n) - 1, np.zeros((n, 8)))
    assert gpu_ctx.pose_graph_optimize([many], check=False) == -4
    assert gpu_ctx.pose_graph_optimize([q] * 65, check=False) == -4            # the fixture's context has max_windows = 64
    # a graph of two sequences is not run; its neighbour in the batch is
    res = gpu_ctx.pose_graph_optimize([graph_input("mixed_sequence"), q])
    assert res[0].status == v.capi.PG_UNSUPPORTED and res[0].iterations == 0 and not res[0].T.any()
    check("n5", res[1])
