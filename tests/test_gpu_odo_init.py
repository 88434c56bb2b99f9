"""vpl_odo_init: the keyframe session takes its first window from the visual-inertial alignment.  A session of two sequences (F = 11
with every frame a key frame, F = 14 with three non-key frames) against vpl_init_align_batch on the same inputs (bit for bit),
against the oracle's point triangulation on the SfM camera frames scaled by s (the bar of tests/test_line_map.py's parity test,
1e-9 relative), a first solve, a failing sequence, an IMU-enabled session and the refusal of an interval longer than its buffer."""
import ctypes as C

import numpy as np
import pytest

import oracle_api as o
import vplines_slam_amd as v
import init_align_ref as ref
from init_align_inputs import KEY11, KEY14, device_input, measurements
from test_gpu_odo_imu import assert_held_equals, batch, obs_of, sb10
from test_gpu_odo_session import MAX_LT, MAX_PT, _ctxn, _obs_frame
from test_gpu_sequence import LINE_MIN_OBS

pytestmark = pytest.mark.gpu

NF = 11
TRI_BAR = 1e-9      # tests/test_line_map.py::test_gpu_triangulate_points_matches_oracle


def raw(x):
    return C.string_at(C.addressof(x), C.sizeof(x))


def cases():
    """[(input, Measurements, key)]"""
    return [(device_input(11, KEY11), measurements(11, 77), KEY11), (device_input(14, KEY14), measurements(14, 77), KEY14)]


def frames_of(M, key):
    return [_obs_frame(M, F) for F in key]


def session(ctx, n, opt):
    return v.Session(ctx, n_seq=n, opt=opt, init_depth=5.0, line_min_obs=LINE_MIN_OBS, max_point_tracks=MAX_PT, max_line_tracks=MAX_LT)


def oracle_depths(q, M, key, tr, opt):
    """triangulate(Ps, TIC_TMP = 0, RIC) of the selected tracks on the SfM camera frames -> (selected mask, depths)"""
    R = q.R.reshape(-1, 3, 3)
    pose = np.zeros((NF, 7))
    for i, k in enumerate(key):
        qq = ref.mat2q(R[k], np.float64)
        pose[i] = [*q.T[k], qq[1], qq[2], qq[3], qq[0]]
    ex0 = np.array([0, 0, 0, *M.ex[3:]])
    sel = (tr["point_nobs"] >= 2) & (tr["point_start"] < NF - 3)
    start, nobs, ids = tr["point_start"][sel], tr["point_nobs"][sel], tr["point_id"][sel]
    obs = np.concatenate([[M.pobs[key[s + k]][int(i)] for k in range(n)] for s, n, i in zip(start, nobs, ids)])
    w = v.Window(pose, np.zeros((NF, 9)), ex0, start, nobs, obs, -np.ones(len(start)), [], [], np.zeros((0, 8)), np.zeros((0, 6)))
    o.triangulate_points(w, opt, 5.0)
    return sel, 1.0 / w.inv_depth


def test_init_equals_the_alignment_scales_the_triangulation_and_solves():
    opt = v.default_options()
    ctx = _ctxn(2)
    cs = cases()
    want, wpre, _ = ctx.init_align([c[0] for c in cs], opt)
    ses = session(ctx, 2, opt)
    allocs = ctx.debug_allocs()
    res = ses.init([c[0] for c in cs], [c[1].ex for c in cs], [frames_of(c[1], c[2]) for c in cs])
    assert ctx.debug_allocs() == allocs                      # the call gives back every array it takes
    for i, (q, M, key) in enumerate(cs):
        assert res[i].ok == 1 and raw(res[i]) == raw(want[i]), i
        pose, sb, ex = ses.get_states(i)                      # what k_odo_init_finish put into the store
        assert np.array_equal(pose, np.array(want[i].pose)) and np.array_equal(sb, np.array(want[i].speed_bias)), i
        assert np.array_equal(ex, M.ex) and np.abs(M.ex[:3]).max() > 0, i
        held = ses.get_preint(i)
        for f in range(1, NF):
            assert_held_equals((i, f), held[f], wpre[i][f])
            assert held[f].sum_dt == wpre[i][f].sum_dt
        tr = ses.get_tracks(i)
        sel, d = oracle_depths(q, M, key, tr, opt)
        assert sel.sum() > 20 and (~sel).sum() > 0
        want_invd = 1.0 / (res[i].s * d)
        err = np.abs(tr["inv_depth"][sel] / want_invd - 1).max()
        print("sequence %d: %d selected tracks, s %.6f, max relative |invd - 1 / (s d)| %.3g" % (i, sel.sum(), res[i].s, err))
        assert err < TRI_BAR
        assert np.all(tr["inv_depth"][~sel] == -1.0)
        assert len(tr["line_id"]) > 0 and not tr["line_triangulated"].any() and not tr["line_plk"].any()
    r = ses.solve()
    for i, (q, M, key) in enumerate(cs):
        assert r[i].report.termination in (0, 1) and r[i].report.iterations >= 1 and r[i].n_points_solved > 20, i
        assert r[i].report.final_cost < r[i].report.initial_cost
    ses.close()
    ctx.close()


def test_a_failing_sequence_is_left_without_a_window():
    opt = v.default_options()
    ctx = _ctxn(2)
    (q11, M11, _), (q14, M14, _) = cases()
    ses = session(ctx, 2, opt)
    first = ses.init([q11, q14], [M11.ex, M14.ex], [frames_of(M11, KEY11), frames_of(M14, KEY14)])
    assert first[0].ok and first[1].ok
    bad = device_input(11, KEY11, flip_T=True)
    res = ses.init([bad, q14], [M11.ex, M14.ex], [frames_of(M11, KEY11), frames_of(M14, KEY14)])
    assert res[0].ok == 0 and res[0].fail & v.capi.INIT_FAIL_SCALE and res[1].ok == 1
    assert raw(res[1]) == raw(first[1])
    fl = np.zeros(2, np.int32)
    out = (v.capi.OdoResult * 2)()
    assert ses.lib.vpl_odo_solve(ses.h, fl.ctypes.data_as(C.POINTER(C.c_int)), out) == -1       # sequence 0 holds no window
    assert ses.lib.vpl_odo_get_preint(ses.h, 0, (v.capi.Preintegration * NF)()) == -1
    held = ses.get_preint(1)
    _, wpre, _ = ctx.init_align([q14], opt)
    for f in range(1, NF):
        assert_held_equals(f, held[f], wpre[0][f])
    # ... and takes one again
    again = ses.init([q11, q14], [M11.ex, M14.ex], [frames_of(M11, KEY11), frames_of(M14, KEY14)])
    assert raw(again[0]) == raw(first[0]) and ses.solve()[0].report.iterations >= 1
    ses.close()
    ctx.close()


def test_imu_session_runs_keyframe_imu_directly_after_init():
    opt = v.default_options()
    ctx = _ctxn(1)
    M = measurements(12, 77)
    q = device_input(11, KEY11, n_meas=12)
    ses = session(ctx, 1, opt)
    ses.enable_imu(20)
    res = ses.init([q], [M.ex], [frames_of(M, KEY11)])
    assert res[0].ok
    r, imu = ses.keyframe_imu([v.ImuFrame(M.imu[11], *obs_of(M, 11))])
    want = batch(ctx, opt, [(M.imu[11], q.samples[-1, 1:4], q.samples[-1, 4:7], sb10(r[0])[3:])])
    held = ses.get_preint(0)
    assert_held_equals("new interval", held[NF - 1], want[0])
    assert imu[0].sum_dt[1] == held[NF - 1].sum_dt
    # window interval 10 longer than max_samples (two image intervals, 40 samples): refused, everything as it was
    q12 = device_input(12, tuple(range(10)) + (11,))
    before = [raw(p) for p in ses.get_preint(0)]
    tracks = ses.get_tracks(0)
    assert ses.init([q12], [M.ex], [frames_of(M, tuple(range(10)) + (11,))], check=False) == -4
    assert [raw(p) for p in ses.get_preint(0)] == before
    after = ses.get_tracks(0)
    assert all(np.array_equal(tracks[k], after[k]) for k in tracks)
    ses.keyframe_imu([v.ImuFrame(M.imu[11], *obs_of(M, 11))])      # and the session goes on
    ses.close()
    ctx.close()


def test_keyframe_rule_decides_directly_after_init():
    opt = v.default_options()
    ctx = _ctxn(2)
    cs = cases()
    ses = session(ctx, 2, opt)
    ses.enable_keyframe_rule()
    res = ses.init([c[0] for c in cs], [c[1].ex for c in cs], [frames_of(c[1], c[2]) for c in cs])
    for i in range(2):
        d = ses.decision(i)
        assert res[i].ok and d.flag in (v.MARGIN_OLD, v.MARGIN_SECOND_NEW) and d.parallax_num > 0 and d.parallax_sum > 0, i
    ses.close()
    ctx.close()


def test_refusals_leave_the_session_as_it_was():
    opt = v.default_options()
    ctx = _ctxn(1)
    (q11, M11, _), _ = cases()
    ses = session(ctx, 1, opt)
    ses.init([q11], [M11.ex], [frames_of(M11, KEY11)])
    before = [raw(p) for p in ses.get_preint(0)]
    ci = q11.to_c()
    ci.R = None
    assert ses.init([ci], [M11.ex], [frames_of(M11, KEY11)], check=False) == -1
    key = q11.key.copy()
    key[3] = key[2]
    bad = v.capi.InitInput(q11.R, q11.T, q11.n_samples, q11.samples, q11.acc0, q11.gyr0, q11.lin_ba, q11.lin_bg, key, q11.bas, q11.bgs, q11.tic)
    assert ses.init([bad], [M11.ex], [frames_of(M11, KEY11)], check=False) == -1
    assert [raw(p) for p in ses.get_preint(0)] == before
    ses.solve()
    assert ses.init([q11], [M11.ex], [frames_of(M11, KEY11)], check=False) == -1     # between solve and advance
    ses.close()
    ctx.close()
