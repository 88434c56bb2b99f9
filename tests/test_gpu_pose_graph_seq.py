"""vpl_pg_optimize_seq_batch on the device against the sequential restatement tests/pgs_ref.py (banded algebra) on the named graphs
of tests/pgs_inputs.py, the way tests/test_gpu_pose_graph.py holds vpl_pg_optimize_batch.

Integers, termination and status are equal.  The solution vector -- T, R, t_drift, r_drift, yaw_drift, final cost -- is held to the
project's bar: max(32 max |x64 - x80|, 1e-12 |x64|_inf), x64 / x80 the restatement's float64 and np.longdouble runs
(tests/test_pgs_reference.py holds the two to the same decisions).  The first step is compared with the dense long-double solve;
single-sequence graphs give the bytes of vpl_pg_optimize_batch; a mixed batch repeats bit for bit in any order and composition;
constant nodes come back with their incoming T bit for bit."""
import numpy as np
import pytest

import vplines_slam_amd as v

import pg_inputs
import pg_ref
import pgs_inputs

pytestmark = pytest.mark.gpu

K_BAR = 32
NAMES = list(pgs_inputs.CASES)
INTS = ("status", "termination", "iterations", "successful_steps", "unsuccessful_steps")


def graph_input(name):
    g = pgs_inputs.case(name) if name in pgs_inputs.CASES else pg_inputs.case(name)
    return v.PoseGraphInput(g["vio_T"], g["vio_R"], g["loop_local"], g["loop_info"], g["sequence"], g["tail_T"], g["tail_R"])


def options(name):
    g = pgs_inputs.case(name) if name in pgs_inputs.CASES else pg_inputs.case(name)
    return v.default_pg_options(**g["opt"])


def got_dict(res):
    return dict(T=res.T, R=res.R, t_drift=np.array(res.t_drift[:]), r_drift=np.array(res.r_drift[:]), yaw_drift=res.yaw_drift,
                final_cost=res.final_cost)


def check(name, res):
    r64, r80 = pgs_inputs.ref_case(name, "f64"), pgs_inputs.ref_case(name, "f80")
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
    # constant nodes: the incoming T, bit for bit
    g, c = pgs_inputs.case(name), r64["const"]
    assert res.T[c].tobytes() == g["vio_T"][c].tobytes(), name
    if len(g["tail_T"]):
        rd, td = np.array(res.r_drift[:]).reshape(3, 3), np.array(res.t_drift[:])
        assert np.abs(res.tail_T - (g["tail_T"].dot(rd.T) + td)).max() <= 1e-12
        assert np.abs(res.tail_R - np.array([rd.dot(R) for R in g["tail_R"]])).max() <= 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_seq_pose_graph_matches_the_sequential_restatement(gpu_ctx, name):
    res = gpu_ctx.pose_graph_optimize_seq([graph_input(name)], options(name))
    check(name, res[0])


@pytest.mark.parametrize("name", ["two_seq", "base_map", "short_runs"])
def test_first_step_against_the_dense_long_double_solve(gpu_ctx, name):
    got = gpu_ctx.pose_graph_debug_step_seq(graph_input(name), options(name))
    exact = pgs_inputs.ref_case(name, "f80", "dense")["first"]
    own = pgs_inputs.ref_case(name, "f64", "banded")["first"]
    ld = np.longdouble
    for key, mine in (("g", got["g"]), ("step", got["step"]), ("model", np.array([got["model_cost_change"]]))):
        ex = np.atleast_1d(np.asarray(exact[key], ld))
        ref_err = float(np.abs(np.atleast_1d(np.asarray(own[key], ld)) - ex).max())
        err = float(np.abs(np.asarray(mine, ld) - ex).max())
        bar = max(K_BAR * ref_err, 1e-12 * float(np.abs(ex).max()))
        print("%s %s: error %.3g, the float64 restatement's %.3g, bar %.3g" % (name, key, err, ref_err, bar))
        assert err <= bar, (name, key, err, bar)
    const_rows = np.repeat(pgs_inputs.ref_case(name, "f64")["const"][1:], 4)
    assert not got["g"][const_rows].any() and not got["step"][const_rows].any()


def test_single_sequence_graphs_give_the_bytes_of_the_existing_call(gpu_ctx):
    by_opt = {}
    for n in pg_inputs.CASES:
        by_opt.setdefault(tuple(sorted(pg_inputs.case(n)["opt"].items())), []).append(n)
    for key, names in by_opt.items():
        inputs = [graph_input(n) for n in names]
        opt = v.default_pg_options(**dict(key))
        old = gpu_ctx.pose_graph_optimize(inputs, opt)
        new = gpu_ctx.pose_graph_optimize_seq(inputs, opt)
        for n, a, b in zip(names, old, new):
            assert a.data() == b.data(), n
        # an explicit, equal, non-zero sequence: the same again
        for q in inputs:
            q.sequence = np.full(len(q.vio_T), 7, dtype=np.int32)
        for n, a, b in zip(names, old, gpu_ctx.pose_graph_optimize_seq(inputs, opt)):
            assert a.data() == b.data(), n


def test_a_mixed_batch_repeats_bit_for_bit_in_any_order_and_composition(gpu_ctx):
    plain = [n for n in NAMES if not pgs_inputs.case(n)["opt"]] + ["n18", "ftol", "n1"]      # single-sequence graphs among them
    first = {}
    for order in (plain, plain[::-1], ["base_map", "n18", "two_seq"], ["short_runs"]):
        inputs = [graph_input(n) for n in order]
        res = gpu_ctx.pose_graph_optimize_seq(inputs)
        again = gpu_ctx.pose_graph_optimize_seq(inputs)
        for i, n in enumerate(order):
            if n in pgs_inputs.CASES:
                check(n, res[i])
            assert res[i].data() == again[i].data(), n
            assert first.setdefault(n, res[i].data()) == res[i].data(), n
    for group in (["seq_reject"], ["seq_reject", "reject", "seq_reject"]):
        res = gpu_ctx.pose_graph_optimize_seq([graph_input(n) for n in group], options("seq_reject"))
        for i, n in enumerate(group):
            assert first.setdefault(n, res[i].data()) == res[i].data(), n
        check("seq_reject", res[0])


def test_an_edge_between_two_constant_nodes_changes_no_output(gpu_ctx):
    g = pgs_inputs.case("base_map")
    ll, li = g["loop_local"].copy(), g["loop_info"].copy()
    ll[4] = -1
    ll[3], li[3, :3], li[3, 7] = 1, (5.0, -3.0, 2.0), 77.0
    other = v.PoseGraphInput(g["vio_T"], g["vio_R"], ll, li, g["sequence"], g["tail_T"], g["tail_R"])
    res = gpu_ctx.pose_graph_optimize_seq([graph_input("base_map"), other])
    assert res[0].data() == res[1].data()
    # a run of one node without a loop is no unknown
    g = pgs_inputs.make_seq_graph([(1, 5), (2, 1), (3, 5)], [(8, 2)], 48)
    res = gpu_ctx.pose_graph_optimize_seq([v.PoseGraphInput(g["vio_T"], g["vio_R"], g["loop_local"], g["loop_info"], g["sequence"])])[0]
    assert res.iterations >= 1 and res.T[5].tobytes() == g["vio_T"][5].tobytes() and res.T[6].tobytes() != g["vio_T"][6].tobytes()


def test_seq_refusals(gpu_ctx):
    g = pgs_inputs.case("two_seq")
    seq = g["sequence"].copy()
    seq[3] = -1
    bad = v.PoseGraphInput(g["vio_T"], g["vio_R"], g["loop_local"], g["loop_info"], seq)
    assert gpu_ctx.pose_graph_optimize_seq([graph_input("two_seq"), bad], check=False) == -1
    ll = g["loop_local"].copy()
    ll[2] = 2
    assert gpu_ctx.pose_graph_optimize_seq([v.PoseGraphInput(g["vio_T"], g["vio_R"], ll, g["loop_info"], g["sequence"])], check=False) == -1
    assert gpu_ctx.pose_graph_optimize_seq([graph_input("two_seq")], v.default_pg_options(initial_radius=0.0), check=False) == -1
    n = v.capi.PG_MAX_NODES + 1
    big = v.PoseGraphInput(np.zeros((n, 3)), np.tile(np.eye(3), (n, 1, 1)), -np.ones(n), np.zeros((n, 8)), np.ones(n))
    assert gpu_ctx.pose_graph_optimize_seq([big], check=False) == -4
    # the existing call still refuses the graph this one runs
    assert gpu_ctx.pose_graph_optimize([graph_input("two_seq")])[0].status == v.capi.PG_UNSUPPORTED
    assert gpu_ctx.pose_graph_optimize_seq([graph_input("two_seq")])[0].status == v.capi.PG_OK
