"""The keyframe decision of a session (vpl_odo_enable_keyframe_rule / _get_decision / the _auto calls; k_odo_parallax) and the
failure mask, on the device.

The reference for every number is the NumPy / Python restatement below of FeatureManager::addFeatureCheckParallax
(feature_manager.cpp:166-188) with compensatedParallax2 (:958-996) and of Estimator::failureDetection (estimator.cpp:909-936), run
on the integer table vpl_odo_get_tracks returns and on the observations the TEST fed: a sequential double sum in the book's order.
Nothing is compared with a second run of the code under test, except where the subject is equality of two ways to call it
(auto against explicit flags) -- and there the flags come from the restatement.

Bar on parallax_sum: all terms are non-negative, so two summation orders of n doubles differ by at most 2 (n - 1) 2^-53 relative;
2 more ulp per term for the contraction of du * du + dv * dv into an fma: relative (n + 4) 2^-52.  Counts and flags are exact, and
every input keeps the restated mean at least 1e-9 (relative) away from the threshold -- asserted on the restatement."""
import functools

import numpy as np
import pytest

import vplines_slam_amd as v
from test_gpu_sequence import NF, LINE_MIN_OBS
from test_gpu_odo_session import feed_window, next_frame, _obs_frame, _preint, _ctxn, MAX_PT, MAX_LT
from test_gpu_odo_imu import measurements, Stream, feed, session, obs_of, prior_tuple
from test_odo_keyframe_rule_api import failure_restated

pytestmark = pytest.mark.gpu

WS = NF - 1
REC = v.capi.ODO_DECISION_RECORD_BYTES
DEFAULT_PARALLAX = 10.0 / 460.0


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def compensated_parallax2(p_i, p_j):
    """feature_manager.cpp:958-996: frame_i = frame_count - 2, frame_j = frame_count - 1; p_i_comp = p_i"""
    ans = 0.0
    u_j, v_j = p_j[0], p_j[1]
    dep_i = p_i[2]
    u_i, v_i = p_i[0] / dep_i, p_i[1] / dep_i
    du, dv = u_i - u_j, v_i - v_j
    du_comp, dv_comp = u_i - u_j, v_i - v_j
    return max(ans, float(np.sqrt(min(du * du + dv * dv, du_comp * du_comp + dv_comp * dv_comp))))


def restate(tracks, obs_at, min_parallax=DEFAULT_PARALLAX, min_track_num=20):
    """tracks: vpl_odo_get_tracks of the window with the new image in slot 10; obs_at(id, slot): the observation the test fed.
    Returns dict(flag, last_track_num, parallax_num, parallax_sum); asserts the distance of the mean from the threshold."""
    s, n, last = 0.0, 0, 0
    for lm, st, nb in zip(tracks["point_id"], tracks["point_start"], tracks["point_nobs"]):
        lm, st, nb = int(lm), int(st), int(nb)
        if st <= WS - 2 and st + nb - 1 >= WS - 1:
            s += compensated_parallax2(obs_at(lm, WS - 2), obs_at(lm, WS - 1))
            n += 1
        if st < WS and st + nb - 1 == WS:      # the new image continued this track (an id continues one track, once)
            last += 1
    if n:
        assert abs(s / n - min_parallax) >= 1e-9 * abs(min_parallax), ("the input sits on the threshold", s / n, min_parallax)
    old = last < min_track_num or n == 0 or s / n >= min_parallax
    return dict(flag=v.MARGIN_OLD if old else v.MARGIN_SECOND_NEW, last_track_num=last, parallax_num=n, parallax_sum=s)


def assert_decision(what, d, want):
    n = want["parallax_num"]
    err = abs(d.parallax_sum - want["parallax_sum"])
    bar = (n + 4) * 2.0 ** -52 * want["parallax_sum"]
    print("%s: flag %d, last_track_num %d, parallax_num %d, sum %.17g (restated %.17g, |diff| %.3g, bar %.3g)"
          % (what, d.flag, d.last_track_num, d.parallax_num, d.parallax_sum, want["parallax_sum"], err, bar))
    assert (d.last_track_num, d.parallax_num) == (want["last_track_num"], n), what
    assert err <= bar, (what, err, bar)
    assert d.flag == want["flag"], what
    assert d.parallax_mean == (d.parallax_sum / n if n else 0.0), what


# ---- windows built by hand (set_window only, no solve) ------------------------------------------------------------------------
class Hand:
    """tracks (id, first frame, last frame) with random observations; frame-8 observations of every third track carry z != 1
    (x and y scaled with it), frame-9 observations of every fifth a z != 1 that the rule ignores"""

    def __init__(self, rng, spans, step):
        self.obs = {}
        for k, (lm, a, b) in enumerate(spans):
            p = rng.uniform(-0.5, 0.5, 2)
            for f in range(a, NF):             # (drawn up to frame 10 whatever b is: equal seeds give equal observations)
                p = p + rng.normal(0, step, 2)
                z = 1.0
                if f == WS - 2 and k % 3 == 0:
                    z = float(rng.uniform(0.5, 2.0))
                if f == WS - 1 and k % 5 == 0:
                    z = float(rng.uniform(0.5, 2.0))
                if f <= b:
                    self.obs[(lm, f)] = np.array([p[0] * z, p[1] * z, z]) if f == WS - 2 else np.array([p[0], p[1], z])
        self.frames = []
        for f in range(NF):
            ids = [lm for lm, a, b in spans if a <= f <= b]
            self.frames.append(v.Frame(ids, np.array([self.obs[(lm, f)] for lm in ids]).reshape(-1, 3), [], []))

    def obs_at(self, lm, slot):
        return self.obs[(lm, slot)]

    def set(self, ses, seq):
        pose = np.zeros((NF, 7))
        pose[:, 6] = 1.0
        ex = np.array([0, 0, 0, 0, 0, 0, 1.0])
        ses.set_window(seq, pose, np.zeros((NF, 9)), ex, (v.capi.Preintegration * NF)(), self.frames)


def _spans_none():
    """25 tracks that start in frame 9 and continue (last_track_num 25, none qualifies), 10 that end in frame 8"""
    return [(100 + i, WS - 1, WS) for i in range(25)] + [(200 + i, i % 8, WS - 2) for i in range(10)]


def _spans_one():
    return [(7, 3, WS)] + [(100 + i, WS - 1, WS) for i in range(24)]


def _spans_257():
    """300 tracks: 257 qualify -- starts 0..8 mixed, 40 of them end in frame 9 -- and 43 do not: 20 end in frame 8, 13 start in
    frame 9, 10 in frame 10"""
    sp = [(1000 + i, i % 9, WS - 1 if i % 6 == 0 and i < 240 else WS) for i in range(257)]
    assert sum(1 for _, _, b in sp if b == WS - 1) == 40
    sp += [(2000 + i, i % 8, WS - 2) for i in range(20)] + [(3000 + i, WS - 1, WS) for i in range(13)] + [(4000 + i, WS, WS) for i in range(10)]
    order = np.random.default_rng(3).permutation(len(sp))
    return [sp[i] for i in order]


def _spans_64(continued):
    """64 qualifying tracks, `continued` of them seen in frame 10"""
    return [(500 + i, i % 9, WS if i < continued else WS - 1) for i in range(64)]


def _small_ctx(n):
    return v.Context(device=0, max_windows=n, max_points=48, max_point_obs=48 * NF, max_lines=12, max_line_obs=12 * NF)


def _hand_session(ctx, n, max_pt):
    return v.Session(ctx, n_seq=n, opt=v.default_options(), init_depth=5.0, line_min_obs=LINE_MIN_OBS, max_point_tracks=max_pt, max_line_tracks=8)


@functools.lru_cache(maxsize=None)
def hand_windows():
    """built once, shared, never written to"""
    rng = np.random.default_rng(20261018)
    return dict(none=Hand(rng, _spans_none(), 0.03), one=Hand(rng, _spans_one(), 0.03), many=Hand(rng, _spans_257(), 0.03),
                **{"small%d" % c: Hand(np.random.default_rng(64), _spans_64(c), 0.002) for c in (64, 19, 20)})


def test_shapes_at_which_the_kernel_can_go_wrong(monkeypatch):
    """four sequences in one session of max_point_tracks = 320: no qualifying track | one | 257 of 300 (one more than a pass of
    the work-group; tracks that end in 8 and in 9) | 64 below the threshold; then last_track_num 19 and 20 on the same 64"""
    monkeypatch.setenv("VPL_DEBUG_GUARDS", "1")
    H = hand_windows()
    ctx = _small_ctx(4)
    ses = _hand_session(ctx, 4, 320)
    seqs = [H["none"], H["one"], H["many"], H["small64"]]
    for i in (0, 1):
        seqs[i].set(ses, i)
    ses.enable_keyframe_rule()             # the windows that are there are decided in this call, ...
    with pytest.raises(RuntimeError):
        ses.decision(2)                    # (no window yet)
    assert ses.last_rc == -1
    for i in (2, 3):
        seqs[i].set(ses, i)                # ... later ones by set_window
    want = [restate(ses.get_tracks(i), h.obs_at) for i, h in enumerate(seqs)]
    assert [w["parallax_num"] for w in want] == [0, 1, 257, 64]
    assert [w["flag"] for w in want] == [v.MARGIN_OLD, v.MARGIN_OLD, v.MARGIN_OLD, v.MARGIN_SECOND_NEW]
    assert all(w["last_track_num"] >= 20 for w in want)
    for i in range(4):
        assert_decision("sequence %d" % i, ses.decision(i), want[i])
        assert ses.decision(i).failure == 0
    d0 = ses.decision(0)
    assert (d0.parallax_sum, d0.parallax_mean) == (0.0, 0.0)
    # last_track_num 19, then 20, min_track_num = 20, the same 64 tracks below the threshold
    for h, flag, last in ((H["small19"], v.MARGIN_OLD, 19), (H["small20"], v.MARGIN_SECOND_NEW, 20)):
        h.set(ses, 3)
        w = restate(ses.get_tracks(3), h.obs_at)
        assert (w["flag"], w["last_track_num"], w["parallax_num"]) == (flag, last, 64)
        assert w["parallax_sum"] == want[3]["parallax_sum"] < 64 * DEFAULT_PARALLAX      # the same data, below the threshold
        assert_decision("last_track_num %d" % last, ses.decision(3), w)
    # a second enable call replaces the thresholds and recomputes: with a threshold below sequence 3's mean it is a keyframe
    mean3 = w["parallax_sum"] / 64
    ses.enable_keyframe_rule(min_parallax=mean3 / 2, min_track_num=5)
    assert_decision("moved threshold", ses.decision(3), restate(ses.get_tracks(3), H["small20"].obs_at, mean3 / 2, 5))
    assert ses.decision(3).flag == v.MARGIN_OLD
    assert_decision("moved threshold, sequence 2", ses.decision(2), restate(ses.get_tracks(2), H["many"].obs_at, mean3 / 2, 5))
    assert ctx.debug_guards() == 0
    ses.close()
    ctx.close()


def test_sum_has_the_same_bits_wherever_the_sequence_sits():
    """the 257-track window alone in a session of max_point_tracks = 1024, and as sequence 2 of 4 with max_point_tracks = 320"""
    H = hand_windows()
    ctx_a, ctx_b = _small_ctx(1), _small_ctx(4)
    sa, sb = _hand_session(ctx_a, 1, 1024), _hand_session(ctx_b, 4, 320)
    sa.enable_keyframe_rule()
    sb.enable_keyframe_rule()
    H["many"].set(sa, 0)
    for i, k in enumerate(("none", "one", "many", "small64")):
        H[k].set(sb, i)
    da, db = sa.decision(0), sb.decision(2)
    want = restate(sa.get_tracks(0), H["many"].obs_at)
    assert_decision("alone", da, want)
    assert_decision("third of four", db, want)
    assert np.float64(da.parallax_sum).tobytes() == np.float64(db.parallax_sum).tobytes(), (da.parallax_sum, db.parallax_sum)
    for s_, c_ in ((sa, ctx_a), (sb, ctx_b)):
        s_.close()
        c_.close()


# ---- after slides: the synthetic sequences of the session tests ---------------------------------------------------------------
class Slots:
    """which global frame sits in which slot of the window (the test's own mirror of the slides)"""

    def __init__(self, M):
        self.M, self.gf = M, list(range(NF))

    def slide(self, flag, F):
        self.gf = self.gf[1:] + [F] if flag == v.MARGIN_OLD else self.gf[:WS - 1] + [self.gf[WS], F]

    def obs_at(self, lm, slot):
        return self.M.pobs[self.gf[slot]][lm]


AFTER_SLIDES_FLAGS = (v.MARGIN_OLD, v.MARGIN_SECOND_NEW, v.MARGIN_OLD, v.MARGIN_OLD, v.MARGIN_SECOND_NEW, v.MARGIN_OLD)


def test_decision_after_every_slide_equals_the_restatement_and_costs_one_record(monkeypatch):
    """one sequence, 6 keyframes with explicit flags (the decision is advice); after set_window and after every advance the
    decision equals the restatement; the read-back of the advance is exactly one record; the failure mask is the restatement's
    -- 0 on these keyframes -- with last_P followed by the test; under VPL_DEBUG_GUARDS=1"""
    monkeypatch.setenv("VPL_DEBUG_GUARDS", "1")
    opt = v.default_options()
    M = measurements(NF + 10, 77)
    ctx = _ctxn(1)
    ses = v.Session(ctx, n_seq=1, opt=opt, init_depth=5.0, line_min_obs=LINE_MIN_OBS, max_point_tracks=MAX_PT, max_line_tracks=MAX_LT)
    ses.enable_keyframe_rule()
    feed_window(ses, 0, ctx, M, opt)
    sl = Slots(M)
    assert_decision("window", ses.decision(0), restate(ses.get_tracks(0), sl.obs_at))
    last_pose = M.pred[NF - 2][0].copy()
    flags_decided = []
    for k, flag in enumerate(AFTER_SLIDES_FLAGS):
        res = ses.solve([flag])
        d2h_solve, tab_solve = ses.stats()[2], ses.stats()[1]
        pose10, sb10 = np.ctypeslib.as_array(res[0].pose)[NF - 1].copy(), np.ctypeslib.as_array(res[0].speed_bias)[NF - 1].copy()
        fail = ses.decision(0).failure
        assert fail == failure_restated(sb10, pose10, last_pose) == 0, (k, fail)
        last_pose = pose10
        ses.advance([next_frame(ctx, M, NF + k, res[0], opt)])
        sl.slide(flag, NF + k)
        h2d, tab, d2h = ses.stats()
        assert d2h == d2h_solve + 1 * REC, (k, d2h, d2h_solve)
        want = restate(ses.get_tracks(0), sl.obs_at)
        d = ses.decision(0)
        assert_decision("keyframe %d" % k, d, want)
        assert d.failure == 0
        flags_decided.append(d.flag)
        assert want["parallax_num"] >= 30 and want["last_track_num"] >= 20, k
    print("decisions:", flags_decided)
    assert ctx.debug_guards() == 0
    ses.close()
    ctx.close()


def consecutive_displacements(M, n_frames):
    """per frame F >= 1: the mean displacement of the landmarks seen in F - 1 and F"""
    out = []
    for F in range(1, n_frames):
        common = [i for i in M.pobs[F] if i in M.pobs[F - 1]]
        out.append(float(np.mean([np.hypot(*(M.pobs[F][i][:2] - M.pobs[F - 1][i][:2])) for i in common])))
    return out


def threshold_from_measurements(M, n_frames):
    """the median of the consecutive-frame displacements, placed midway between its two neighbours in sorted order"""
    d = sorted(consecutive_displacements(M, n_frames))
    m = len(d) // 2
    return 0.5 * (d[m - 1] + d[m + 1])


AUTO_KEYFRAMES = 10


def test_auto_equals_explicit_flags_from_the_restatement():
    """two sessions on two contexts, 10 keyframes: one through keyframe_auto, the other through keyframe with the flags the
    restatement computes from the second session's own book -- results, tracks after every slide and the final prior are
    equal bit for bit; both flags occur at least twice"""
    opt = v.default_options()
    M = measurements(NF + AUTO_KEYFRAMES, 77)
    thr = threshold_from_measurements(M, NF + AUTO_KEYFRAMES)
    ctx_a, ctx_b = _ctxn(1), _ctxn(1)
    mk = lambda c: v.Session(c, n_seq=1, opt=opt, init_depth=5.0, line_min_obs=LINE_MIN_OBS, max_point_tracks=MAX_PT, max_line_tracks=MAX_LT)
    sa, sb = mk(ctx_a), mk(ctx_b)
    sa.enable_keyframe_rule(min_parallax=thr)
    feed_window(sa, 0, ctx_a, M, opt)
    feed_window(sb, 0, ctx_b, M, opt)
    sl = Slots(M)
    bias = np.zeros(6)
    flags = []
    for k in range(AUTO_KEYFRAMES):
        F = NF + k
        want = restate(sb.get_tracks(0), sl.obs_at, thr)
        flags.append(want["flag"])
        assert_decision("keyframe %d" % k, sa.decision(0), want)
        s9 = np.concatenate([M.pred[F][1][:3], bias])
        f = _obs_frame(M, F, pose=M.pred[F][0], speed_bias=s9, preint=_preint(ctx_a, M, F, s9[3:6], s9[6:9], opt))
        ra = sa.keyframe_auto([f])[0]
        rb = sb.keyframe([f], [want["flag"]])[0]
        sl.slide(want["flag"], F)
        assert bytes(ra) == bytes(rb), k
        ta, tb = sa.get_tracks(0), sb.get_tracks(0)
        for name in ta:
            assert np.array_equal(ta[name], tb[name]), (k, name)
        bias = np.ctypeslib.as_array(ra.speed_bias)[NF - 1, 3:].copy()
    print("threshold %.6g, flags %s" % (thr, flags))
    assert flags.count(v.MARGIN_OLD) >= 2 and flags.count(v.MARGIN_SECOND_NEW) >= 2, flags
    assert prior_tuple(sa.get_prior(0)) == prior_tuple(sb.get_prior(0))
    for s_, c_ in ((sa, ctx_a), (sb, ctx_b)):
        s_.close()
        c_.close()


def test_imu_form_auto_equals_explicit_flags_from_the_restatement():
    """keyframe_imu_auto for 3 keyframes against keyframe_imu with the restated flags; the record comes back in the copy of the
    18 doubles: d2h of the advance grows by one record"""
    opt = v.default_options()
    st = Stream(measurements(NF + AUTO_KEYFRAMES, 77))
    thr = threshold_from_measurements(st.M, NF + AUTO_KEYFRAMES)
    ctx_a, ctx_b = _ctxn(1), _ctxn(1)
    sa, sb = session(ctx_a, 1, opt), session(ctx_b, 1, opt)
    sa.enable_keyframe_rule(min_parallax=thr)
    feed(sa, 0, ctx_a, st, opt)
    feed(sb, 0, ctx_b, st, opt)
    sl = Slots(st.M)
    for k in range(3):
        F = NF + k
        want = restate(sb.get_tracks(0), sl.obs_at, thr)
        assert_decision("keyframe %d" % k, sa.decision(0), want)
        frame = v.ImuFrame(st.imu[F], *obs_of(st.M, F))
        ra, ia = sa.keyframe_imu_auto([frame])
        rb, ib = sb.keyframe_imu([frame], [want["flag"]])
        sl.slide(want["flag"], F)
        assert bytes(ra[0]) == bytes(rb[0]) and bytes(ia[0]) == bytes(ib[0]), k
        assert sa.stats()[2] == sb.stats()[2] + REC, (k, sa.stats(), sb.stats())
        ta, tb = sa.get_tracks(0), sb.get_tracks(0)
        for name in ta:
            assert np.array_equal(ta[name], tb[name]), (k, name)
        assert bytes(sa.get_preint(0)) == bytes(sb.get_preint(0)), k
    assert_decision("after the last keyframe", sa.decision(0), restate(sb.get_tracks(0), sl.obs_at, thr))
    assert prior_tuple(sa.get_prior(0)) == prior_tuple(sb.get_prior(0))
    for s_, c_ in ((sa, ctx_a), (sb, ctx_b)):
        s_.close()
        c_.close()


def test_disagreeing_sequences_are_refused_and_explicit_flags_still_work():
    """two sequences, the threshold midway between their restated means: keyframe_auto and solve_auto return VPL_E_INVALID and
    name the count for each flag; the explicit-flag keyframe that follows gives the bits of a plain twin session that never made
    the refused calls"""
    opt = v.default_options()
    Ms = [measurements(NF + AUTO_KEYFRAMES, 77), measurements(NF + 4, 78)]
    ctx_a, ctx_b = _ctxn(2), _ctxn(2)
    mk = lambda c: v.Session(c, n_seq=2, opt=opt, init_depth=5.0, line_min_obs=LINE_MIN_OBS, max_point_tracks=MAX_PT, max_line_tracks=MAX_LT)
    sa, sb = mk(ctx_a), mk(ctx_b)
    for i, M in enumerate(Ms):
        feed_window(sa, i, ctx_a, M, opt)
        feed_window(sb, i, ctx_b, M, opt)
    sls = [Slots(M) for M in Ms]
    free = [restate(sa.get_tracks(i), sls[i].obs_at, 1e300) for i in range(2)]          # (a threshold nothing sits on: the means)
    means = [w["parallax_sum"] / w["parallax_num"] for w in free]
    assert means[0] != means[1]
    thr = 0.5 * (means[0] + means[1])
    sa.enable_keyframe_rule(min_parallax=thr)
    want = [restate(sa.get_tracks(i), sls[i].obs_at, thr) for i in range(2)]
    assert sorted(w["flag"] for w in want) == [v.MARGIN_OLD, v.MARGIN_SECOND_NEW]
    for i in range(2):
        assert_decision("sequence %d" % i, sa.decision(i), want[i])
    s9 = [np.concatenate([M.pred[NF][1][:3], np.zeros(6)]) for M in Ms]
    frames = [_obs_frame(M, NF, pose=M.pred[NF][0], speed_bias=s, preint=_preint(ctx_a, M, NF, s[3:6], s[6:9], opt)) for M, s in zip(Ms, s9)]
    for call in (lambda: sa.keyframe_auto(frames), sa.solve_auto):
        with pytest.raises(RuntimeError) as e:
            call()
        assert sa.last_rc == -1
        assert "1 want VPL_MARGIN_OLD, 1 VPL_MARGIN_SECOND_NEW" in str(e.value), str(e.value)
    for i in range(2):
        assert_decision("sequence %d after the refusal" % i, sa.decision(i), want[i])
    ra, rb = sa.keyframe(frames, [v.MARGIN_OLD] * 2), sb.keyframe(frames, [v.MARGIN_OLD] * 2)
    for i in range(2):
        assert bytes(ra[i]) == bytes(rb[i]), i
        ta, tb = sa.get_tracks(i), sb.get_tracks(i)
        for name in ta:
            assert np.array_equal(ta[name], tb[name]), (i, name)
        assert prior_tuple(sa.get_prior(i)) == prior_tuple(sb.get_prior(i)), i
    for s_, c_ in ((sa, ctx_a), (sb, ctx_b)):
        s_.close()
        c_.close()


def test_rule_off_refuses_the_decision_and_the_auto_calls():
    H = hand_windows()
    ctx = _small_ctx(1)
    ses = _hand_session(ctx, 1, 320)
    H["one"].set(ses, 0)
    f = H["one"].frames[NF - 1]
    frame = v.Frame(f.point_id, f.point_obs, [], [], pose=[0, 0, 0, 0, 0, 0, 1.0], speed_bias=np.zeros(9), preint=v.capi.Preintegration())
    for call in (lambda: ses.decision(0), ses.solve_auto, lambda: ses.keyframe_auto([frame]),
                 lambda: ses.keyframe_imu_auto([v.ImuFrame(np.zeros((1, 7)), f.point_id, f.point_obs)])):
        with pytest.raises(RuntimeError):
            call()
        assert ses.last_rc == -1
    ses.close()
    ctx.close()
