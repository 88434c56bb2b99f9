"""vpl_odo_select / Session.select: the feature selector fed from the session -- state k from slot 10 of the store, the cloud
gathered on the device from the resident tracks, the id book kept per sequence -- against Context.select_features fed with what
the test builds in NumPy from get_tracks / get_states and with the restatement's book (tests/select_ref.py).

One short session is played once (played()) and the tests read what it recorded.  Per image: the book's split, the selection,
the selected image into the session (keyframe).  Values: the f of every selection against the plain call's, inside the value
bar of tests/select_inputs.py computed from the restatement's float64 and long double runs of the same input (K = 32)."""
import functools
import os

import numpy as np
import pytest

import select_inputs as si
import select_ref as ref
import vplines_slam_amd as v
from test_gpu_sequence import Measurements, _ctx, NF, LINE_MIN_OBS
from test_gpu_odo_session import feed_window, next_frame, MAX_PT, MAX_LT

pytestmark = pytest.mark.gpu

E_INVALID, E_CAPACITY = -1, -4
N_IMAGES = 3           # images selected and fed after the window
SELECT_ALL = 600       # max_features above every image: kappa never binds, every candidate with f > -1 is taken
LAST_KAPPA = 3         # ... but in the last image, where the restatement plays along


def measurements():
    """the session tests' measurements with the point ids renamed in the order of first appearance, from 1: a front end's ids
    grow, and the book splits an image on the largest id it has seen"""
    M = Measurements(NF + N_IMAGES + 1)
    name = {}
    for F in sorted(M.pobs):
        for i in sorted(M.pobs[F]):
            name.setdefault(i, len(name) + 1)
        M.pobs[F] = {name[i]: o for i, o in sorted(M.pobs[F].items())}
    return M


def params(M, max_features):
    par = si.params(max_features=max_features, init_thresh=20)
    par.q_ic, par.t_ic = M.ex[[6, 3, 4, 5]].copy(), M.ex[:3].copy()
    return par


def prob_of(i):
    return 0.1 + 0.9 * ((int(i) * 37) % 101) / 100.0


def select_frame(M, F):
    """the image of global frame F and its IMU-propagated state, as estimator_node hands them to the selector"""
    pose, sb = M.pred[F]
    ids = list(M.pobs[F])
    xy = np.array(list(M.pobs[F].values())).reshape(-1, 3)
    smp = np.asarray(M.imu[max(F, 1)]).reshape(-1, 7)      # (frame 0 ends no interval; nothing reads it there)
    return v.SelectFrame(pose[:3], pose[[6, 3, 4, 5]], sb[:3], np.zeros(3), smp[-1, 1:4], smp[-1, 4:7], len(smp), float(smp[0, 0]), ids, xy[:, 0],
                         xy[:, 1], [prob_of(i) for i in ids])


def qR(q_xyzw):
    return np.array(ref.qmat(np.asarray(q_xyzw)[[3, 0, 1, 2]]))


def numpy_cloud(ses, M, oldest, solved_ids, fr, par):
    """initKDTree from what the session lets a caller read: the tracks with nobs >= 2, start < 8, start <= 7.5 that a solve has
    taken (solved_ids: kept by the test), into camera k + 1.  oldest: the global frame in slot 0 -- a track's first observation
    is the measurement of its id in frame oldest + start"""
    tr = ses.get_tracks(0)
    st = ses.get_states(0)
    pose, ex = np.asarray(st[0]).reshape(NF, 7), np.asarray(st[2]).reshape(7)
    R1, Ric = np.array(ref.qmat(fr.Q1)), np.array(ref.qmat(par.q_ic))
    out = []
    for i, s, n, d in zip(tr["point_id"], tr["point_start"], tr["point_nobs"], tr["inv_depth"]):
        if not (n >= 2 and s < NF - 3 and s <= 0.75 * (NF - 1) and int(i) in solved_ids):
            continue
        depth = 1.0 / d
        w = qR(pose[s, 3:]) @ (qR(ex[3:]) @ (M.pobs[oldest + s][int(i)] * depth) + ex[:3]) + pose[s, :3]
        pc = Ric.T @ (R1.T @ (w - fr.P1) - par.t_ic)
        out.append([pc[0] / pc[2], pc[1] / pc[2], depth])
    return np.array(out).reshape(-1, 3)


def scene_of(ses, fr, new, subset, kappa, cloud):
    st = ses.get_states(0)
    pose, sb = np.asarray(st[0]).reshape(NF, 7), np.asarray(st[1]).reshape(NF, 9)
    at = {int(i): k for k, i in enumerate(fr.id)}
    return si.Scene(P0=pose[NF - 1, :3], Q0=pose[NF - 1, [6, 3, 4, 5]], V0=sb[NF - 1, :3], Ba0=sb[NF - 1, 3:6], P1=fr.P1, Q1=fr.Q1, V1=fr.V1,
                    Ba1=fr.Ba1, acc=fr.acc, gyr=fr.gyr, n_imu=fr.n_imu, delta_imu=fr.delta_imu, new_id=np.array(new, dtype=np.int32),
                    new_x=fr.x[[at[i] for i in new]], new_y=fr.y[[at[i] for i in new]], new_prob=fr.prob[[at[i] for i in new]],
                    used_x=fr.x[[at[i] for i in subset]], used_y=fr.y[[at[i] for i in subset]], cloud=cloud, kappa=kappa)


@functools.lru_cache(maxsize=None)
def played():
    """-> the records of one session: per select call what Session.select gave, what Context.select_features gave on the NumPy
    input, the restatement's book, and at the end the guards and the traffic"""
    opt = v.default_options()
    M = measurements()
    old = os.environ.get("VPL_DEBUG_GUARDS")
    os.environ["VPL_DEBUG_GUARDS"] = "1"      # read when the context is made: a pattern behind every device array, the call's own included
    try:
        ctx = _ctx()
    finally:
        if old is None:
            del os.environ["VPL_DEBUG_GUARDS"]
        else:
            os.environ["VPL_DEBUG_GUARDS"] = old
    ses = v.Session(ctx, n_seq=1, opt=opt, line_min_obs=LINE_MIN_OBS, max_point_tracks=MAX_PT, max_line_tracks=MAX_LT)
    book = ref.Book(SELECT_ALL, 20)
    rec = dict(calls=[])
    # ---- no window yet: the book alone (the first image passes whole)
    fr = select_frame(M, 0)
    image, new, subset, kappa = book.split(fr.id)
    got = ses.select(params(M, SELECT_ALL), [fr])[0]
    rec["first"] = dict(got=got, want_out=book.finish(image, new, subset, False, []), n_image=len(set(fr.id)), stats=ctx.select_stats())
    feed_window(ses, 0, ctx, M, opt)
    solved = set()
    res = None
    for k in range(N_IMAGES + 1):
        F = NF + k
        last = k == N_IMAGES
        fr = select_frame(M, F)
        image, new, subset, kappa = book.split(fr.id)
        par = params(M, len(subset) + LAST_KAPPA if last else SELECT_ALL)
        if last:
            kappa = LAST_KAPPA
        cloud = numpy_cloud(ses, M, k, solved, fr, par)
        s = scene_of(ses, fr, new, subset, kappa, cloud)
        plain = ctx.select_features(par, [s])[0]
        got = ses.select(par, [fr])[0]
        launches = ctx.select_stats()[0]
        out = book.finish(image, new, subset, True, [int(i) for i in got["ids"]])
        call = dict(got=got, plain=plain, want_out=out, n_new=len(new), n_used=len(subset), kappa=kappa, n_cloud=len(cloud), scene=s, par=par,
                    launches=launches, image=set(int(i) for i in fr.id))
        if k == 0:      # the window has not been solved: between solve and advance nothing may be selected either
            call["refused"] = None
        rec["calls"].append(call)
        if last:
            break
        # the solve takes the tracks with nobs >= 2 and start < 8 (those are "solved" from now on), then the selected image enters
        tr = ses.get_tracks(0)
        solved |= {int(i) for i, s_, n in zip(tr["point_id"], tr["point_start"], tr["point_nobs"]) if n >= 2 and s_ < NF - 3}
        res = ses.solve()[0]
        if k == 0:
            before = bytes(np.asarray(ses.get_states(0)[0]))
            call["refused"] = ses.select(par, [select_frame(M, F + 1)], check=False)
            call["states_same"] = before == bytes(np.asarray(ses.get_states(0)[0]))
        f = next_frame(ctx, M, F, res, opt)
        keep = [j for j, i in enumerate(f.point_id) if int(i) in set(out)]
        f = v.Frame(f.point_id[keep], f.point_obs[keep], f.line_id, f.line_obs, pose=f.pose, speed_bias=f.speed_bias,
                    preint=f.preint)
        ses.advance([f])
        call["tracks_after"] = set(int(i) for i in ses.get_tracks(0)["point_id"])
        call["fed"] = set(int(i) for i in f.point_id)
        solved &= call["tracks_after"]         # (an erased track takes its flag along)
    rec["guards"] = ctx.debug_guards()
    ses.close()
    ctx.close()
    return rec


def test_session_select_equals_the_plain_call_on_a_numpy_built_cloud():
    """every image after the window: the ids and their order are the plain call's, every f inside the value bar the restatement's
    two precisions set for that round (the last image, where kappa binds), the counts are the book's and the filter's"""
    rec = played()
    for k, c in enumerate(rec["calls"]):
        got, plain = c["got"], c["plain"]
        assert got["initialized"] and (got["n_new"], got["n_used"], got["kappa"], got["n_cloud"]) == (c["n_new"], c["n_used"], c["kappa"], c["n_cloud"]), k
        assert list(got["ids"]) == list(plain["ids"]), k
        assert (got["n_invisible"], got["n_ineligible"], got["n_candidates"]) == (plain["n_invisible"], plain["n_ineligible"], plain["n_candidates"])
        assert list(got["out"]) == c["want_out"], k
        assert c["launches"] == 4, k
    assert rec["guards"] == 0
    c = rec["calls"][-1]
    assert c["n_cloud"] > 20 and c["n_new"] > LAST_KAPPA and len(c["got"]["ids"]) == LAST_KAPPA
    r64, r80 = (ref.run(dt, c["par"], c["scene"]) for dt in (np.float64, np.longdouble))
    assert len(r80["rounds"]) >= LAST_KAPPA
    for r in range(LAST_KAPPA):
        bar = si.value_bar(r64["rounds"][r][2], r80["rounds"][r][2])
        err = abs(c["got"]["f"][r] - c["plain"]["f"][r])
        print("round %d: |f session - f plain| %.3g, bar %.3g, ratio %.3g" % (r, err, bar, err / bar))
        assert err <= bar, r


def test_before_the_first_solve_the_cloud_is_empty_and_every_depth_is_one():
    """the window is set but not solved: no track has solve_flag, n_cloud = 0, and the result has the bits of the plain call
    without a cloud"""
    c = played()["calls"][0]
    assert c["n_cloud"] == 0 and c["got"]["n_cloud"] == 0 and c["n_new"] > 0
    assert list(c["got"]["ids"]) == list(c["plain"]["ids"]) and len(c["got"]["ids"]) > 0
    assert np.array_equal(c["got"]["f"], c["plain"]["f"])
    assert len(played()["calls"][1]["scene"].cloud) > 0          # ... and after the first solve it is not


def test_without_a_window_only_the_book_runs():
    """the first image passes whole and nothing is launched"""
    r = played()["first"]
    assert not r["got"]["initialized"] and r["got"]["n_new"] == r["n_image"] and len(r["got"]["ids"]) == 0
    assert list(r["got"]["out"]) == r["want_out"] and len(r["want_out"]) == r["n_image"]
    assert r["stats"] == (0, 0, 0)


def test_the_selected_ids_feed_advance_and_the_session_goes_on():
    """what select hands out enters the window: the frame that advance took holds exactly those ids, the tracks of the
    selected new ids exist afterwards, and the next select sees them as tracked"""
    calls = played()["calls"]
    for k, c in enumerate(calls[:-1]):
        assert c["fed"] == set(c["want_out"]), k
        assert set(int(i) for i in c["got"]["ids"]) <= c["tracks_after"], k
    for a, b in zip(calls, calls[1:]):
        again = set(int(i) for i in a["got"]["ids"]) & b["image"]
        assert again and again <= set(b["want_out"]) and b["n_used"] >= len(again)


def test_refused_between_solve_and_advance_and_the_session_is_as_it_was():
    c = played()["calls"][0]
    assert c["refused"] == E_INVALID and c["states_same"]


def test_refusals_move_no_book():
    """delta_imu = 0 and an image above the capacity are refused; the call after them gives what it gives without them"""
    opt = v.default_options()
    M = measurements()
    outs = []
    for bad in (False, True):
        ctx = _ctx()
        ses = v.Session(ctx, n_seq=1, opt=opt, line_min_obs=LINE_MIN_OBS, max_point_tracks=MAX_PT, max_line_tracks=MAX_LT)
        par = params(M, SELECT_ALL)
        ses.select(par, [select_frame(M, 0)])
        feed_window(ses, 0, ctx, M, opt)
        if bad:
            fr = select_frame(M, NF)
            fr.delta_imu = 0.0
            assert ses.select(par, [fr], check=False) == E_INVALID
            fr = select_frame(M, NF)
            fr.n_imu = 0
            assert ses.select(par, [fr], check=False) == E_INVALID
            n = v.capi.SEL_MAX_FEATURES + 1
            big = v.SelectFrame(fr.P1, fr.Q1, fr.V1, fr.Ba1, fr.acc, fr.gyr, 10, 0.005, np.arange(5000, 5000 + n), np.zeros(n), np.zeros(n), np.ones(n))
            assert ses.select(par, [big], check=False) == E_CAPACITY
        got = ses.select(par, [select_frame(M, NF)])[0]
        outs.append((list(got["ids"]), list(got["out"]), got["f"].tobytes(), got["n_new"]))
        assert ctx.debug_guards() == 0
        ses.close()
        ctx.close()
    assert outs[0] == outs[1] and outs[0][3] > 0


def test_a_session_that_never_selects_moves_the_bytes_it_moved():
    """two sessions on the same frames, one calls select before every keyframe (and feeds the whole image all the same): the
    results have the same bits and vpl_odo_stats the same three numbers"""
    opt = v.default_options()
    M = measurements()
    recs = []
    for use in (False, True):
        ctx = _ctx()
        ses = v.Session(ctx, n_seq=1, opt=opt, line_min_obs=LINE_MIN_OBS, max_point_tracks=MAX_PT, max_line_tracks=MAX_LT)
        feed_window(ses, 0, ctx, M, opt)
        mine = []
        for k in range(2):
            if use:
                ses.select(params(M, SELECT_ALL), [select_frame(M, NF + k)])
            res = ses.solve()[0]
            ses.advance([next_frame(ctx, M, NF + k, res, opt)])
            mine.append((bytes(res), ses.stats()))
        recs.append(mine)
        ses.close()
        ctx.close()
    assert recs[0] == recs[1]
