"""Who owns the device arrays a session takes from the context it borrows (csrc/host_common.h: every array of a context is
recorded with its owner; vpl_odo_destroy / vpl_trk_destroy give back exactly the session's): the record before, during and
after a session, counted through Context.debug_allocs / FrontendContext.debug_allocs, under VPL_DEBUG_GUARDS=1.

Shapes: the smallest at which ownership can go wrong -- two sequences, 64 point tracks and 8 line tracks on the small context of
tests/test_gpu_odo_keyframe_rule.py; the windows and the IMU stream are those of tests/test_gpu_odo_imu.py, thinned to the 48
landmarks and 8 segments of lowest id seen in frame 5 so that they fit (THIN_P / THIN_L).

No test here makes an allocation fail on the card: the failure paths of odo_resize_inbox and vpl_odo_enable_imu are checked
by reading them."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import vplines_slam_amd as v
from test_gpu_sequence import NF, LINE_MIN_OBS
from test_gpu_odo_imu import Stream, feed, measurements, obs_of
from test_gpu_odo_keyframe_rule import _small_ctx
from test_gpu_trk_session import K_, bar_frame, golden_frames

pytestmark = pytest.mark.gpu

N_SEQ, MAX_PT, MAX_LT = 2, 64, 8
THIN_P, THIN_L = 48, 8
N_KEYFRAMES = 3
# the constants of csrc/ba_odo.h the sizes below are made of
ODO_PAR_HDR = 3
HEAD_DOUBLES = 16 + C.sizeof(v.capi.Preintegration) // 8     # pose + speed/bias + the caller's pre-integration: what sample rows replace
GROWING_SAMPLES = 70                                          # the smallest max_samples whose rows (7 doubles each) outgrow that head


@functools.lru_cache(maxsize=None)
def thin_measurements():
    """the sequence of seed 77 with the observations of THIN_P landmarks and THIN_L segments only; a copy: the shared one is not
    written to"""
    M = copy.copy(measurements(NF + N_KEYFRAMES, 77))
    keep_p, keep_l = sorted(M.pobs[5])[:THIN_P], sorted(M.lobs[5])[:THIN_L]
    M.pobs = {F: {i: o for i, o in obs.items() if i in keep_p} for F, obs in M.pobs.items()}
    M.lobs = {F: {i: o for i, o in obs.items() if i in keep_l} for F, obs in M.lobs.items()}
    return M


def streams():
    """one per sequence: the same images, the second with 7-sample intervals from frame 11 on (the decisions of the two agree,
    their IMU sides do not)"""
    M = thin_measurements()
    return [Stream(M), Stream(M, {NF + k: 7 for k in range(N_KEYFRAMES)})]


def make_session(ctx):
    return v.Session(ctx, n_seq=N_SEQ, opt=v.default_options(), init_depth=5.0, line_min_obs=LINE_MIN_OBS, max_point_tracks=MAX_PT,
                     max_line_tracks=MAX_LT)


def feed_all(ses, ctx, sts, imu):
    for i, st in enumerate(sts):
        feed(ses, i, ctx, st, v.default_options(), imu=imu)


def imu_frames(sts, F):
    return [v.ImuFrame(st.imu[F], *obs_of(st.M, F)) for st in sts]


def decision_tuple(d):
    return tuple(getattr(d, f) for f, _ in v.capi.OdoDecision._fields_)


def test_head_that_the_sample_rows_replace_is_483_doubles():
    assert HEAD_DOUBLES == 483 and 7 * (GROWING_SAMPLES - 1) <= HEAD_DOUBLES < 7 * GROWING_SAMPLES


def test_both_orders_of_the_enable_calls_give_the_same_record_and_the_same_bits(monkeypatch):
    """enable_imu(70) then enable_keyframe_rule() on one context, the other order on a second: the same (arrays, bytes), and
    three keyframe_imu_auto calls whose results, imu_out and decisions are equal bit for bit"""
    monkeypatch.setenv("VPL_DEBUG_GUARDS", "1")
    sts = streams()
    ctxs = [_small_ctx(N_SEQ), _small_ctx(N_SEQ)]
    sess = [make_session(c) for c in ctxs]
    sess[0].enable_imu(GROWING_SAMPLES)
    sess[0].enable_keyframe_rule()
    sess[1].enable_keyframe_rule()
    sess[1].enable_imu(GROWING_SAMPLES)
    counts = [c.debug_allocs() for c in ctxs]
    print("record with both features, either order:", counts)
    assert counts[0] == counts[1]
    for ses, ctx in zip(sess, ctxs):
        feed_all(ses, ctx, sts, imu=True)
    for k in range(N_KEYFRAMES):
        out = [ses.keyframe_imu_auto(imu_frames(sts, NF + k)) for ses in sess]
        dec = [[decision_tuple(ses.decision(i)) for i in range(N_SEQ)] for ses in sess]
        for i in range(N_SEQ):
            assert bytes(out[0][0][i]) == bytes(out[1][0][i]), (k, i, "result")
            assert bytes(out[0][1][i]) == bytes(out[1][1][i]), (k, i, "imu_out")
        assert dec[0] == dec[1], (k, dec)
        assert out[0][0][0].n_points_solved >= 20, k                       # (not vacuous: the thinned window is solved)
        print("keyframe %d: decisions %s, %d points and %d lines solved" % (k, [d[0] for d in dec[0]], out[0][0][0].n_points_solved,
                                                                             out[0][0][0].n_lines_solved))
    for ses, ctx in zip(sess, ctxs):
        assert ctx.debug_guards() == 0
        ses.close()
        ctx.close()


def test_enable_calls_that_do_not_grow_the_inbox_add_no_inbox(monkeypatch):
    """enable_imu(8): 56 doubles of samples fit where the 483 of the head lie -- six IMU arrays more, of 2 x n_seq x (8 x 7 + 6)
    doubles and 2 x n_seq ints.  enable_keyframe_rule() alone: one inbox in, one out, n_seq x 4 x (ODO_PAR_HDR + max_point_tracks)
    bytes larger"""
    monkeypatch.setenv("VPL_DEBUG_GUARDS", "1")
    ctx = _small_ctx(N_SEQ)
    ses = make_session(ctx)
    n0, b0 = ctx.debug_allocs()
    ses.enable_imu(8)
    n1, b1 = ctx.debug_allocs()
    assert (n1 - n0, b1 - b0) == (6, 2 * N_SEQ * ((8 * 7 + 6) * 8 + 4))
    ses.close()
    ses = make_session(ctx)
    assert ctx.debug_allocs() == (n0, b0)
    ses.enable_keyframe_rule()
    n2, b2 = ctx.debug_allocs()
    assert (n2 - n0, b2 - b0) == (0, N_SEQ * 4 * (ODO_PAR_HDR + MAX_PT))
    assert ctx.debug_guards() == 0
    ses.close()
    ctx.close()


def test_destroy_gives_everything_back_and_a_second_session_runs(monkeypatch):
    """the record before Session(...) and after create, both enable calls, one keyframe and close() is the same; a second
    session on the same context then runs a keyframe with every guard intact"""
    monkeypatch.setenv("VPL_DEBUG_GUARDS", "1")
    sts = streams()
    ctx = _small_ctx(N_SEQ)
    before = ctx.debug_allocs()
    for _ in range(2):
        ses = make_session(ctx)
        ses.enable_imu(GROWING_SAMPLES)
        ses.enable_keyframe_rule()
        assert ctx.debug_allocs()[0] > before[0]
        feed_all(ses, ctx, sts, imu=True)
        res, _ = ses.keyframe_imu_auto(imu_frames(sts, NF))
        assert res[0].n_points_solved >= 20
        assert ctx.debug_guards() == 0
        ses.close()
        assert ctx.debug_allocs() == before
    ctx.close()


def trk_session_bytes(n_seq, max_lines, px):
    """the 15 arrays of a tracker session (csrc/trk_session.h): two stores of kept line records (56 bytes), ids, t_cnt and a
    16-int header; keep, vert, the two debug tables, take; the inbox (frames padded to 16 bytes, seeds) and the outbox (per
    sequence 16 ints, 9 doubles, the ids padded to 8 bytes, 8 doubles per line)"""
    store = n_seq * max_lines * (56 + 4 + 4) + n_seq * 16 * 4
    tables = 4 * n_seq * max_lines * 4 + n_seq * 4
    inbox = ((n_seq * px + 15) & ~15) + n_seq * 4
    outbox = n_seq * (16 * 4 + 9 * 8 + ((max_lines * 4 + 7) & ~7) + max_lines * 64)
    return 2 * store + tables + inbox + outbox


def test_tracker_session_gives_back_its_own_and_leaves_what_the_context_made_meanwhile(monkeypatch):
    """max_lines = 8 on the golden frames' size.  While the session is open the context allocates for itself (the CLAHE tables
    with the first frame, the blurred copy with keep_blurred): close() removes the session's 15 arrays and nothing else, the
    lazily made ones stay in the record, are used by a second session and are guard-checked"""
    monkeypatch.setenv("VPL_DEBUG_GUARDS", "1")
    from test_preproc import euroc_maps
    a, _ = golden_frames()
    H, W = a.shape
    fe = v.frontend.FrontendContext(device=0, max_images=2, width=W, height=H, max_lines=8)
    fe.match_reserve(1, 8192)
    fe.set_maps(*euroc_maps(W, H))
    opt = v.default_tracker_options(**K_)
    before = fe.debug_allocs()
    t = v.TrackerSession(fe, 1, opt)
    r0 = t.frame(bar_frame(a.shape)[None], [7])[0]
    fe.keep_blurred(True)
    r1 = t.frame(bar_frame(a.shape, 1)[None], [9])[0]
    assert 1 <= r0["n_lines"] <= 8 and r1["matched"] == 1
    n_open, b_open = fe.debug_allocs()
    t.close()
    n_closed, b_closed = fe.debug_allocs()
    assert (n_open - n_closed, b_open - b_closed) == (15, trk_session_bytes(1, 8, W * H))
    lazy = (n_closed - before[0], b_closed - before[1])
    print("made by the context while the session was open: %d arrays, %d bytes" % lazy)
    assert lazy[0] >= 2 and lazy[1] >= 2 * W * H                       # at least the blurred copy (max_images frames) and the CLAHE tables
    assert fe.debug_guards() == 0
    t = v.TrackerSession(fe, 1, opt)
    assert fe.debug_allocs() == (n_open, b_open)                       # nothing lazy is made twice
    r2 = t.frame(bar_frame(a.shape)[None], [7])[0]
    assert r2["n_lines"] == r0["n_lines"] and np.array_equal(r2["obs"], r0["obs"])
    assert fe.debug_guards() == 0
    t.close()
    assert fe.debug_allocs() == (n_closed, b_closed)
    fe.close()


def test_a_context_whose_session_was_closed_has_the_record_of_one_that_never_had_one(monkeypatch):
    """the context's own arrays stay, in their order: the same count and bytes as a fresh context of the same capacities, and
    the solve that follows on the bare context runs with every guard intact"""
    monkeypatch.setenv("VPL_DEBUG_GUARDS", "1")
    fresh, used = _small_ctx(N_SEQ), _small_ctx(N_SEQ)
    ses = make_session(used)
    ses.enable_keyframe_rule()
    ses.enable_imu(GROWING_SAMPLES)
    ses.close()
    assert used.debug_allocs() == fresh.debug_allocs()
    opt = v.default_options()
    w = v.workload.generate(v.workload.seed_for(3, 0), v.workload.config(40, 12, True), 0.0)
    out = []
    for ctx in (fresh, used):
        wc = w.copy()
        v.workload.set_preintegrations([wc], ctx.preintegrate(*v.workload.imu_batch_arrays([wc]), opt))
        _, rep = ctx.solve_windows([wc], opt)
        out.append((wc.pose.tobytes(), rep[0].iterations, rep[0].final_cost))
        assert ctx.debug_guards() == 0
    assert out[0] == out[1]
    for ctx in (fresh, used):
        ctx.close()


def test_a_context_closed_before_its_session_takes_the_session_with_it(monkeypatch):
    """vpl_odo_destroy reads the context the session borrows, so the session has to go first whichever of the two the caller
    closes -- or the garbage collector finalises -- first: Context.close() destroys a session that is still open (as
    FrontendContext.close() does with its tracker session), after which the session's own close() has nothing left to do.  A
    context that makes its own session likewise, and a new session on a context whose first one was closed is registered again."""
    monkeypatch.setenv("VPL_DEBUG_GUARDS", "1")
    ctx = _small_ctx(N_SEQ)
    before = ctx.debug_allocs()
    ses = make_session(ctx)
    ses.close()
    assert ctx._odo is None and ctx.debug_allocs() == before
    ses = make_session(ctx)
    ses.enable_keyframe_rule()
    assert ctx._odo is ses and ctx.debug_allocs()[0] > before[0]
    ctx.close()
    assert not ses.h and not ctx.h and ctx._odo is None
    ses.close()
    del ses, ctx
    own = v.Session(None, n_seq=1, opt=v.default_options(), max_point_tracks=MAX_PT, max_line_tracks=MAX_LT, device=0, max_windows=1,
                    max_points=48, max_point_obs=48 * NF, max_lines=12, max_line_obs=12 * NF)      # (_small_ctx's capacities)
    ctx = own.ctx
    ctx.close()                                   # the borrowed side first
    assert not own.h
    own.close()
    assert own.ctx is None
