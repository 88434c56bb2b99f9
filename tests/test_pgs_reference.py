"""The restatement tests/pgs_ref.py of the pose-graph optimisation over several sequences, checked on the CPU: on every
single-sequence graph of tests/pg_inputs.py it returns exactly what tests/pg_ref.py returns; on the named graphs of
tests/pgs_inputs.py its float64 and long-double runs take the same decisions with every deciding quantity well away from its
threshold, the banded algebra equals the dense normal equations, constant nodes come back exactly and an edge between two
constant nodes changes nothing.  Also: the library exports the new call."""
import numpy as np
import pytest

import vplines_slam_amd as v

import pg_inputs
import pg_ref
import pgs_inputs
import pgs_ref

K_BAR = 32
NAMES = list(pgs_inputs.CASES)
INTS = ("status", "termination", "iterations", "successful_steps", "unsuccessful_steps")


def bar_of(x64, x80):
    """the bound tests/test_pg_reference.py uses"""
    return max(K_BAR * float(np.abs(x64 - x80).max()), 1e-12 * float(np.abs(x64).max()))


def equal_results(a, b):
    assert set(a) - {"const"} == set(b) - {"const"}
    for k in b:
        if k in ("decisions", "rhos"):
            assert len(a[k]) == len(b[k]) and all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(a[k], b[k])), k
        elif k == "first":
            assert (a[k] is None) == (b[k] is None)
            if b[k] is not None:
                for f in ("g", "step", "model"):
                    assert np.array_equal(np.asarray(a[k][f]), np.asarray(b[k][f])), (k, f)
        elif k in ("verdicts", "edges") or k in INTS:
            assert a[k] == b[k], k
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("name", list(pg_inputs.CASES))
def test_single_sequence_graphs_give_exactly_what_pg_ref_gives(name):
    g = pg_inputs.case(name)
    for dtype, dt in (("f64", np.float64), ("f80", np.longdouble)):
        for seq in (None, np.full(len(g["vio_T"]), 3, dtype=np.int32)):
            mine = pgs_ref.optimize(g["vio_T"], g["vio_R"], g["loop_local"], g["loop_info"], seq, g["tail_T"], g["tail_R"], g["opt"], dt)
            equal_results(mine, pg_inputs.ref_case(name, dtype))
    dense = pgs_ref.optimize(g["vio_T"], g["vio_R"], g["loop_local"], g["loop_info"], None, g["tail_T"], g["tail_R"], g["opt"], np.longdouble, "dense")
    equal_results(dense, pg_inputs.ref_case(name, "f80", "dense"))


@pytest.mark.parametrize("name", NAMES)
def test_both_precisions_decide_alike_and_far_from_every_threshold(name):
    r64, r80 = pgs_inputs.ref_case(name, "f64"), pgs_inputs.ref_case(name, "f80")
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


@pytest.mark.parametrize("name", NAMES)
def test_banded_algebra_equals_the_dense_normal_equations(name):
    r64, r80, d80 = pgs_inputs.ref_case(name, "f64"), pgs_inputs.ref_case(name, "f80"), pgs_inputs.ref_case(name, "f80", "dense")
    for k in INTS:
        assert r80[k] == d80[k], (name, k)
    assert r80["verdicts"] == d80["verdicts"]
    x64, x80, xd = pgs_ref.solution(r64), pgs_ref.solution(r80), pgs_ref.solution(d80)
    err, bar = float(np.abs(x80 - xd).max()), bar_of(x64, x80)
    print(name, "banded - dense %.3g, bar %.3g" % (err, bar))
    assert err <= bar


def test_the_named_cases_have_the_shapes_their_names_say():
    r = {n: pgs_inputs.ref_case(n, "f64") for n in NAMES}
    g = {n: pgs_inputs.case(n) for n in NAMES}
    runs = lambda s: [len(list(grp)) for grp in np.split(s, np.flatnonzero(np.diff(s)) + 1)]
    assert runs(g["two_seq"]["sequence"]) == [6, 6] and g["two_seq"]["loop_local"][9] == 2
    assert runs(g["two_seq_two_loops"]["sequence"]) == [8, 10] and (g["two_seq_two_loops"]["loop_local"] >= 0).sum() == 2
    b = g["base_map"]
    assert runs(b["sequence"]) == [5, 8] and not b["sequence"][:5].any() and [b["loop_local"][i] for i in (4, 8, 11)] == [0, 1, 3]
    f = g["floats"]
    assert runs(f["sequence"]) == [5, 5, 6] and (f["loop_local"][5:10] < 0).all() and not ((f["loop_local"] >= 5) & (f["loop_local"] < 10)).any()
    assert runs(g["short_runs"]["sequence"]) == [3, 1, 2, 6]
    assert runs(g["two_seq_130"]["sequence"]) == [65, 65]
    assert "reject" in r["seq_reject"]["verdicts"] and r["seq_reject"]["unsuccessful_steps"] >= 1
    assert r["seq_ftol"]["verdicts"][-1] == "function_tolerance"
    for n in NAMES:
        assert r[n]["iterations"] >= 1, n
    # the edges: none across a break, none between two constants
    for n in NAMES:
        seq, const = g[n]["sequence"], r[n]["const"]
        for a, b_, loop in r[n]["edges"]:
            assert loop or seq[a] == seq[b_]
            assert not (const[a] and const[b_])
    assert int(r["base_map"]["const"].sum()) == 5 and int(r["two_seq"]["const"].sum()) == 1
    assert (4, 0, True) not in r["base_map"]["edges"] and (1, 8, True) in r["base_map"]["edges"]


@pytest.mark.parametrize("dtype", ["f64", "f80"])
def test_constant_nodes_come_back_exactly(dtype):
    dt = np.float64 if dtype == "f64" else np.longdouble
    for name in NAMES:
        g, r = pgs_inputs.case(name), pgs_inputs.ref_case(name, dtype)
        c = r["const"]
        assert c[0] and np.array_equal(r["T"][c], g["vio_T"][c].astype(dt)), name
        for k in np.flatnonzero(c):
            R = g["vio_R"][k].astype(dt)
            assert np.array_equal(r["R"][k], pg_ref.ypr2R(pg_ref.R2ypr(pg_ref.qmat(pg_ref.mat2q(R))))), (name, k)
        assert not np.array_equal(r["T"][~c], g["vio_T"][~c].astype(dt)), name


def test_an_edge_between_two_constant_nodes_changes_no_output():
    g = pgs_inputs.case("base_map")
    base = pgs_inputs.ref_case("base_map", "f64")
    ll, li = g["loop_local"].copy(), g["loop_info"].copy()
    ll[4] = -1                                        # without the loop inside the map
    a = pgs_ref.optimize(g["vio_T"], g["vio_R"], ll, li, g["sequence"], g["tail_T"], g["tail_R"], g["opt"])
    ll[3], li[3, :3], li[3, 7] = 1, (5.0, -3.0, 2.0), 77.0    # with another, grossly wrong one
    b = pgs_ref.optimize(g["vio_T"], g["vio_R"], ll, li, g["sequence"], g["tail_T"], g["tail_R"], g["opt"])
    for r in (a, b):
        equal_results(r, base)
    # the sequential edges inside the map: moving a map node that no live node is tied to changes nothing but that node
    T = g["vio_T"].copy()
    T[2] += (0.3, -0.2, 0.1)
    c = pgs_ref.optimize(T, g["vio_R"], g["loop_local"], g["loop_info"], g["sequence"], g["tail_T"], g["tail_R"], g["opt"])
    keep = np.arange(len(T)) != 2
    assert np.array_equal(c["T"][keep], base["T"][keep]) and np.array_equal(c["T"][2], T[2])
    assert c["final_cost"] == base["final_cost"] and c["initial_cost"] == base["initial_cost"]


def test_an_untouched_free_node_is_not_an_unknown():
    g = pgs_inputs.make_seq_graph([(1, 5), (2, 1), (3, 5)], [(8, 2)], 48)     # node 5: a run of one without a loop
    r = pgs_ref.optimize(g["vio_T"], g["vio_R"], g["loop_local"], g["loop_info"], g["sequence"])
    assert r["const"][5] and np.array_equal(r["T"][5], g["vio_T"][5]) and r["iterations"] >= 1
    assert pgs_ref.optimize(g["vio_T"], g["vio_R"], g["loop_local"], g["loop_info"], -g["sequence"])["status"] == pgs_ref.INVALID


@pytest.mark.parametrize("name", list(pgs_inputs.SCRIPTS))
def test_session_scripts_decide_alike_in_both_precisions(name):
    (a, pa, _), (b, pb, _) = pgs_inputs.ref_script(name, "f64"), pgs_inputs.ref_script(name, "f80")
    turns = 0
    for op, ra, rb in zip(pgs_inputs.script(name), a, b):
        if op[0] == "update_loop":
            assert ra == rb and isinstance(ra, bool)
        elif op[0] == "optimize":
            assert ra["status"] == rb["status"]
            if ra["status"] == pgs_ref.NOTHING:
                continue
            turns += 1
            for k in INTS + ("n_nodes", "first_index", "cur_index"):
                assert ra[k] == rb[k], (name, k)
            assert ra["verdicts"] == rb["verdicts"] and len(ra["decisions"]) == len(rb["decisions"])
            for r in (ra, rb):
                for value, threshold in r["decisions"]:
                    big = max(abs(value), abs(threshold))
                    assert big == 0 or abs(value - threshold) >= 1e-6 * big, (name, value, threshold)
        else:
            assert ra["index"] == rb["index"] and ra["optimize_pending"] == rb["optimize_pending"]
    assert turns >= 1 and float(np.abs(pa[-1]["T"] - pb[-1]["T"].astype(np.float64)).max()) < 1e-12


def test_the_restated_list_handling():
    pg = pgs_ref.PoseGraph(max_keyframes=4)
    eye, info = np.eye(3), np.array([0.5, 0, 0, np.cos(np.radians(5.0)), 0, 0, np.sin(np.radians(5.0)), 10.0])   # t, q of a yaw of 10 degrees, yaw
    assert pg.add(2, np.zeros(3), eye) == -1 and pg.add(0, np.zeros(3), eye) == -1 and pg.add(1, np.zeros(3), eye, 0, info) == -1
    assert pg.add(1, np.zeros(3), eye)["index"] == 0 and pg.optimize()["status"] == pgs_ref.NOTHING
    assert pg.add(1, np.ones(3), eye)["optimize_pending"] is False
    # a second sequence from an origin of its own: its first loop puts it where the loop says, and its stored keyframes with it
    assert pg.add(2, np.array([10.0, 0, 0]), eye)["index"] == 2
    r = pg.add(2, np.array([11.0, 0, 0]), eye, 1, info)
    assert r["optimize_pending"] and pg.sequence_loop == [0, 0, 1] and pg.earliest_loop_index == 1
    yaw = np.radians(10.0)
    want = np.ones(3) + np.array([0.5, 0, 0])
    assert np.abs(r["vio_T"] - want).max() < 1e-12 and abs(pgs_ref.R2ypr(pg.vio_R[3])[0] - 10.0) < 1e-9
    assert np.abs(pg.vio_T[2] - (want - np.array([np.cos(yaw), np.sin(yaw), 0]))).max() < 1e-12
    assert np.array_equal(pg.vio_T[1], np.ones(3)) and pg.add(2, np.zeros(3), eye) == -4 and len(pg) == 4
    assert pg.update_loop(0, info) == -1 and pg.update_loop(3, info) is True
    far = info.copy()
    far[7] = 31.0
    assert pg.update_loop(3, far) is False and pg.loop_info[3][7] == 10.0
    res = pg.optimize()
    assert (res["first_index"], res["cur_index"], res["n_nodes"]) == (1, 3, 3) and pg.queue == [] and pg.optimize()["status"] == pgs_ref.NOTHING


def test_library_exports_the_new_calls_and_struct_sizes():
    import ctypes as C
    lib = v.load_hip_library()
    for name in ("vpl_pg_optimize_seq_batch", "vpl_pg_debug_step_seq", "vpl_pgs_create", "vpl_pgs_add_keyframe", "vpl_pgs_optimize"):
        assert hasattr(lib, name), name
    assert hasattr(v.Context, "pose_graph_optimize_seq")
    assert C.sizeof(v.capi.PgsOptions) == 8 + C.sizeof(v.capi.PgOptions) == 8 + 8 + 11 * 8
    assert C.sizeof(v.capi.CPgsKeyframe) == 8 + 8 * (3 + 9 + 3 + 9 + 8)
    assert C.sizeof(v.capi.CPgsKeyframeOut) == 8 + 8 * (3 + 9 + 3 + 9 + 9 + 3)
    assert C.sizeof(v.capi.CPgsResult) == 8 * 4 + 8 * (2 + 1 + 9 + 3)
    o = v.default_pgs_options()
    assert (o.max_keyframes, o.fast_relocalization, o.pg.max_iterations, o.pg.huber_delta) == (8192, 0, 5, 0.1)
    assert (v.capi.PGS_MAX_KEYFRAMES, v.capi.PGS_OK, v.capi.PGS_NOTHING) == (65536, 0, 2)
