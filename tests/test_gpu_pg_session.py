"""The pose-graph session (vpl_pgs_*) on the device against the restatement pgs_ref.PoseGraph: the scripts of tests/pgs_inputs.py
are replayed on both.  After every add / load the returned record is compared, after every optimize the whole path, the drift and
the result.  Doubles are held to the project's bar, max(32 max |x64 - x80|, 1e-12 |x64|_inf) with x64 / x80 the restatement's
float64 and np.longdouble replays (tests/test_pgs_reference.py holds the two to the same decisions); integers are equal.  Then:
the session's optimisation gives the bytes of vpl_pg_optimize_seq_batch on the same graph, the queue keeps the last index and the
earliest loop, refusals and capacity leave the session as it was, and a script repeats bit for bit."""
import numpy as np
import pytest

import vplines_slam_amd as v

import pgs_inputs

pytestmark = pytest.mark.gpu

K_BAR = 32
INTS = ("status", "termination", "iterations", "successful_steps", "unsuccessful_steps", "n_nodes", "first_index", "cur_index")
ld = np.longdouble


def held(got, r64, r80, what):
    x, x64, x80 = (np.asarray(a, ld).ravel() for a in (got, r64, r80))
    bar = max(K_BAR * float(np.abs(x64 - x80).max()), 1e-12 * float(np.abs(x64).max()))
    err = float(np.abs(x - x64).max())
    assert err <= bar, (what, err, bar)
    return err, bar


def path_bytes(s):
    p = s.path()
    return b"".join(p[k].tobytes() for k in sorted(p)) + b"".join(np.asarray(a).tobytes() for a in s.drift())


def session(gpu_ctx, name=None, **kw):
    kw = dict(pgs_inputs.SCRIPT_OPTIONS.get(name, {}), **kw)
    return v.PoseGraphSession(gpu_ctx, v.default_pgs_options(**kw))


def replay(s, name, compare=True):
    """-> what every optimize returned"""
    ops = pgs_inputs.script(name)
    ref64, ref80 = pgs_inputs.ref_script(name, "f64"), pgs_inputs.ref_script(name, "f80")
    results, worst = [], 0.0
    for i, op in enumerate(ops):
        r64, r80 = ref64[0][i], ref80[0][i]
        if op[0] in ("add", "load"):
            got = s.add(*op[1:]) if op[0] == "add" else s.load(*op[1:])
            if compare:
                assert got["index"] == r64["index"] and got["optimize_pending"] == r64["optimize_pending"], (name, i)
                for k in ("vio_T", "vio_R", "T", "R", "w_r_vio", "w_t_vio"):
                    worst = max(worst, held(got[k], r64[k], r80[k], (name, i, k))[0])
        elif op[0] == "update_loop":
            assert s.update_loop(*op[1:]) == r64, (name, i)
        else:
            res = s.optimize()
            results.append(res)
            if not compare:
                continue
            if r64["status"] == pgs_inputs.pgs_ref.NOTHING:
                assert res.status == v.capi.PGS_NOTHING
                continue
            print(name, "optimize at step", i, {k: getattr(res, k) for k in INTS}, r64["verdicts"])
            for k in INTS:
                assert getattr(res, k) == r64[k], (name, i, k, getattr(res, k), r64[k])
            for k in ("final_cost", "yaw_drift", "r_drift", "t_drift"):
                got = getattr(res, k)
                held(got[:] if k in ("r_drift", "t_drift") else got, r64[k], r80[k], (name, i, k))
        if compare and op[0] != "add":
            # the whole list and the drift, after everything that can move more than the new keyframe
            p, p64, p80 = s.path(), ref64[1][i], ref80[1][i]
            assert np.array_equal(p["sequence"], p64["sequence"]) and np.array_equal(p["loop_index"], p64["loop_index"]), (name, i)
            for k in ("T", "R", "vio_T", "vio_R", "loop_info"):
                err, bar = held(p[k], p64[k], p80[k], (name, i, "path", k))
                worst = max(worst, err)
            yaw, rd, td = s.drift()
            held(np.concatenate([[yaw], rd.ravel(), td]), np.concatenate([[ref64[2][i][0]], ref64[2][i][1].ravel(), ref64[2][i][2]]),
                 np.concatenate([[ref80[2][i][0]], ref80[2][i][1].ravel(), ref80[2][i][2]]), (name, i, "drift"))
    if compare:
        p, p64, p80 = s.path(), ref64[1][-1], ref80[1][-1]
        for k in ("T", "R", "vio_T", "vio_R", "loop_info"):
            held(p[k], p64[k], p80[k], (name, "end", k))
        print(name, "largest error %.3g" % worst)
    return results


@pytest.mark.parametrize("name", list(pgs_inputs.SCRIPTS))
def test_script_matches_the_restatement(gpu_ctx, name):
    with session(gpu_ctx, name) as s:
        replay(s, name)


def test_what_the_scripts_exercise(gpu_ctx):
    # single: the keyframes added behind a queued loop are the tail of the optimisation and take the drift on entry
    with session(gpu_ctx) as s:
        ops = pgs_inputs.script("single")
        at = ops.index(("optimize",))
        for op in ops[:at]:
            s.add(*op[1:], out=False)
        assert len(s) == 23
        before = s.path()
        res = s.optimize()
        after = s.path()
        assert (res.first_index, res.cur_index, res.n_nodes) == (3, 20, 18) and res.iterations >= 1
        assert before["T"][:3].tobytes() == after["T"][:3].tobytes()                       # in front of the earliest loop: untouched
        assert before["vio_T"].tobytes() == after["vio_T"].tobytes() and before["vio_R"].tobytes() == after["vio_R"].tobytes()
        yaw, rd, td = s.drift()
        assert abs(yaw) > 1e-3 and np.abs(after["T"][21:] - (after["vio_T"][21:].dot(rd.T) + td)).max() <= 1e-12   # the tail
        assert np.abs(after["T"][21:] - before["T"][21:]).max() > 1e-4
        got = s.add(*ops[at + 1][1:])                                                       # the next one takes the drift on entry
        assert np.abs(got["T"] - (rd.dot(got["vio_T"]) + td)).max() <= 1e-12 and np.abs(got["T"] - got["vio_T"]).max() > 1e-4
    # second_sequence: the first loop into sequence 1 moves every earlier keyframe of sequence 2 and none of sequence 1; the second
    # loop shifts nothing
    with session(gpu_ctx) as s:
        ops = [op for op in pgs_inputs.script("second_sequence") if op[0] == "add"]
        for op in ops[:17]:
            s.add(*op[1:], out=False)
        before = s.path()
        got = s.add(*ops[17][1:])
        after = s.path()
        assert before["vio_T"][:12].tobytes() == after["vio_T"][:12].tobytes() and before["vio_R"][:12].tobytes() == after["vio_R"][:12].tobytes()
        assert np.linalg.norm(after["vio_T"][12:17] - before["vio_T"][12:17], axis=1).min() > 1e-2
        assert np.abs(after["vio_T"][12:17] - (before["vio_T"][12:17].dot(got["w_r_vio"].T) + got["w_t_vio"])).max() <= 1e-12
        assert np.abs(after["vio_R"][12:17] - np.array([got["w_r_vio"].dot(R) for R in before["vio_R"][12:17]])).max() <= 1e-12
        assert before["T"].tobytes() == after["T"][:17].tobytes()                           # the poses are not shifted (:103-124)
        for op in ops[18:22]:
            s.add(*op[1:], out=False)
        before = s.path()
        again = s.add(*ops[22][1:])
        assert ops[22][4] == 7 and s.path(0, 22)["vio_T"].tobytes() == before["vio_T"].tobytes()
        assert again["w_r_vio"].tobytes() == got["w_r_vio"].tobytes() and again["w_t_vio"].tobytes() == got["w_t_vio"].tobytes()
    # base_map: the loaded keyframes come back with what was loaded -- T bit for bit; R is ypr2R(R2ypr(.)) of it, as optimize4DoF writes it
    with session(gpu_ctx) as s:
        results = replay(s, "base_map", compare=False)
        assert [r.iterations > 0 for r in results] == [False, False, True]
        loaded = [op for op in pgs_inputs.script("base_map") if op[0] == "load"]
        p = s.path(0, 6)
        assert p["T"].tobytes() == np.array([op[3] for op in loaded]).tobytes() and not p["sequence"].any()
        assert np.abs(p["R"] - np.array([op[4] for op in loaded])).max() <= 1e-12


@pytest.mark.parametrize("name", ["single", "second_sequence", "base_map"])
def test_the_session_optimises_as_the_batch_call_does(gpu_ctx, name):
    with session(gpu_ctx, name) as s:
        done = 0
        for op in pgs_inputs.script(name):
            if op[0] != "optimize":
                getattr(s, op[0])(*op[1:], **({"out": False} if op[0] != "update_loop" else {}))
                continue
            p = s.path()
            first = int(p["loop_index"][p["loop_index"] >= 0].min())
            cur = int(np.flatnonzero(p["loop_index"] >= 0).max())
            ll = np.where(p["loop_index"] >= 0, p["loop_index"] - first, -1)[first:cur + 1]
            q = v.PoseGraphInput(p["vio_T"][first:cur + 1], p["vio_R"][first:cur + 1], ll, p["loop_info"][first:cur + 1], p["sequence"][first:cur + 1],
                                 p["vio_T"][cur + 1:], p["vio_R"][cur + 1:])
            want = gpu_ctx.pose_graph_optimize_seq([q])[0]
            res = s.optimize()
            after = s.path()
            assert (res.first_index, res.cur_index) == (first, cur)
            assert after["T"][first:cur + 1].tobytes() == want.T.tobytes() and after["R"][first:cur + 1].tobytes() == want.R.tobytes()
            assert after["T"][cur + 1:].tobytes() == want.tail_T.tobytes() and after["R"][cur + 1:].tobytes() == want.tail_R.tobytes()
            assert after["T"][:first].tobytes() == p["T"][:first].tobytes()
            assert (res.termination, res.iterations, res.initial_cost, res.final_cost, res.yaw_drift) == \
                   (want.termination, want.iterations, want.initial_cost, want.final_cost, want.yaw_drift)
            assert bytes(res.r_drift) == bytes(want.r_drift) and bytes(res.t_drift) == bytes(want.t_drift)
            done += 1
        assert done >= 2


def test_queue(gpu_ctx):
    with session(gpu_ctx) as s:
        res = replay(s, "two_queued")
        assert (res[0].first_index, res[0].cur_index, res[0].status) == (2, 13, v.capi.PGS_OK)
        assert res[1].status == v.capi.PGS_NOTHING and res[1].iterations == 0
        before = path_bytes(s)
        assert s.optimize().status == v.capi.PGS_NOTHING and path_bytes(s) == before


def test_fast_relocalization_moves_the_drift(gpu_ctx):
    ops = pgs_inputs.script("fast_relocalization")
    at = [i for i, op in enumerate(ops) if op[0] == "update_loop"][0]
    drifts = {}
    for fast in (False, True):
        with session(gpu_ctx, fast_relocalization=fast) as s:
            for op in ops[:at]:
                getattr(s, op[0])(*op[1:])
            d0 = s.drift()
            assert s.update_loop(*ops[at][1:]) is True
            drifts[fast] = s.drift()
            assert (np.concatenate([d0[1].ravel(), d0[2]]).tobytes() == np.concatenate([drifts[fast][1].ravel(), drifts[fast][2]]).tobytes()) == (not fast)
            assert np.abs(s.path(12, 1)["loop_info"][0] - ops[at][2]).max() == 0
    r64 = pgs_inputs.ref_script("fast_relocalization", "f64")[2][at]
    r80 = pgs_inputs.ref_script("fast_relocalization", "f80")[2][at]
    yaw, rd, td = drifts[True]
    held(np.concatenate([[yaw], rd.ravel(), td]), np.concatenate([[r64[0]], r64[1].ravel(), r64[2]]), np.concatenate([[r80[0]], r80[1].ravel(), r80[2]]), "drift")


def test_refusals_and_capacity_leave_the_session_as_it_was(gpu_ctx):
    ops = [op for op in pgs_inputs.script("single") if op[0] == "add"]
    with session(gpu_ctx, max_keyframes=8) as s:
        for op in ops[:5]:
            s.add(*op[1:])
        before = path_bytes(s)
        info = ops[20][5]
        assert s.add(3, ops[5][2], ops[5][3], check=False) == -1                 # a sequence jump
        assert s.add(0, ops[5][2], ops[5][3], check=False) == -1
        assert s.add(1, ops[5][2], ops[5][3], 5, info, check=False) == -1        # loop_index >= index
        assert s.add(1, ops[5][2], ops[5][3], -2, info, check=False) == -1
        assert s.load(ops[5][2], ops[5][3], ops[5][2], ops[5][3], 7, info, check=False) == -1
        assert s.update_loop(2, info, check=False) == -1 and s.update_loop(9, info, check=False) == -1
        assert len(s) == 5 and path_bytes(s) == before
        for op in ops[5:8]:
            s.add(*op[1:])
        before = path_bytes(s)
        assert s.add(*ops[8][1:], check=False) == -4 and s.add(*ops[8][1:], out=False, check=False) == -4   # keyframe max_keyframes + 1
        assert len(s) == 8 and path_bytes(s) == before
        assert s.path(5, 4, check=False) == -1
        s.reset()
        assert len(s) == 0 and s.add(*ops[0][1:])["index"] == 0
    lib = gpu_ctx.lib
    import ctypes as C
    h = C.c_void_p()
    assert lib.vpl_pgs_create(gpu_ctx.h, C.byref(v.default_pgs_options(max_keyframes=0)), C.byref(h)) == -1
    assert lib.vpl_pgs_create(gpu_ctx.h, C.byref(v.default_pgs_options(max_keyframes=v.capi.PGS_MAX_KEYFRAMES + 1)), C.byref(h)) == -4
    assert lib.vpl_pgs_create(gpu_ctx.h, C.byref(v.default_pgs_options(initial_radius=0.0)), C.byref(h)) == -1 and not h.value


def test_a_range_of_4097_nodes_is_refused(gpu_ctx):
    n = v.capi.PG_MAX_NODES
    eye, info = np.eye(3), np.array([0.1, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0])
    with session(gpu_ctx, max_keyframes=n + 8) as s:
        for k in range(n):
            s.add(1, (0.1 * k, 0.0, 0.0), eye, out=False)
        got = s.add(1, (0.1 * n, 0.0, 0.0), eye, 0, info)
        assert got["index"] == n and got["optimize_pending"]
        before = path_bytes(s)
        assert s.optimize(check=False) == -4
        assert path_bytes(s) == before
        assert s.optimize(check=False) == -4                                      # the queue is as it was


def test_the_same_script_twice_gives_the_same_bytes(gpu_ctx):
    seen = []
    with session(gpu_ctx) as s, session(gpu_ctx) as other:                        # two sessions on one context
        for sess in (s, other, s):
            if len(sess):
                sess.reset()                                                      # ... and one of them again after a reset
            replay(sess, "second_sequence", compare=False)
            seen.append(path_bytes(sess))
    assert seen[0] == seen[1] == seen[2]
