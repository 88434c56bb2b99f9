"""wall time of the keyframe session (vpl_odo_solve + vpl_odo_advance) per keyframe over the sequence of
tests/test_gpu_sequence.py -- the companion of tools/time_odometry.py, which times the same 32 keyframes through
vpl_ba_solve_odometry + vpl_ba_slide_window with the feature manager on the host.  Medians over keyframes 4..31 of the C calls
alone and of the stages inside them; then --batch N sequences (default 64) in one session for --batch-keyframes keyframes:
keyframes per second.  Every C call ends in a stream synchronise, so the host clock around it is the time of the work.
--mode imu: the same sequence through vpl_odo_keyframe_imu (raw samples in; pre-integration, merge and propagation on the device).
--mode halves: the only faithful alternative without it -- vpl_odo_solve, vpl_preintegrate_batch from the bias it returned, the
propagation on the host (not timed: a C++ caller's costs microseconds), vpl_odo_advance; the three C calls are summed.
--mode rule: what the keyframe rule (vpl_odo_enable_keyframe_rule: one more launch and a 24-byte record per image) costs -- the plain
sequence through a rule-enabled session and through a plain one, alternating, --repeat times (default there: 3), with explicit
MARGIN_OLD flags in both so that the two do the same work; medians over keyframes 4..31 of "slide + new frame" and of the keyframe.
--mode init-align: vpl_init_align_batch (the visual-inertial alignment, once per start of a sequence) for 1 and for --batch
sequences of 14 and of 40 image frames, pre-integrations read back; median, min and max of 7 calls after one warm-up call.
--mode init: vpl_odo_init (the session takes its first window from the alignment: observations up, alignment, triangulation, scale)
for sessions of 1 and of --batch sequences of 14 image frames; the same statistics.
--mode init-structure: vpl_init_structure_batch (GlobalSFM::construct and the PnP of the non-key frames, once per start) on the
inputs of tests/sfm_inputs.py -- one 11-frame sequence, the 40 / 11 / 14-frame batch of the tests, one and eight 40-frame sequences
of 150 tracks; median, min and max of 30 calls after three warm-up calls, then the kernels' device events from a call of its own.
--mode init-relpose: vpl_init_relative_pose_batch (Estimator::relativePose, once per start) on scenes of tests/relpose_inputs.py --
1 and --batch sequences of 100 tracks with 20 % outliers and of 1024 tracks with 30 %; the C call alone, without the optional
arrays: median, min and max of 30 calls after three warm-up calls, then the kernels' device events from a call of its own."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import vplines_slam_amd as v
import test_gpu_sequence as T
import test_gpu_odo_session as S


def run(seeds, n_keyframes, rule=False):
    opt = v.default_options()
    n = len(seeds)
    Ms = [T.Measurements(T.NF + n_keyframes, seed=s) for s in seeds]
    ctx = S._ctxn(n)
    ses = v.Session(ctx, n_seq=n, opt=opt, init_depth=5.0, line_min_obs=T.LINE_MIN_OBS, max_point_tracks=S.MAX_PT, max_line_tracks=S.MAX_LT)
    if rule:
        ses.enable_keyframe_rule()
    for i, M in enumerate(Ms):
        S.feed_window(ses, i, ctx, M, opt)
    acc = {"solve_c_call": [], "advance_c_call": [], "stage_triangulate": [], "stage_only_line_opt": [], "stage_solve": [],
           "stage_slide_new_frame": [], "h2d_payload_B": [], "h2d_table_B": [], "d2h_B": []}
    for k in range(n_keyframes):
        res = ses.solve()
        acc["solve_c_call"].append(ses.last_call_s)
        frames = [S.next_frame(ctx, Ms[i], T.NF + k, res[i], opt) for i in range(n)]
        ses.advance(frames)
        acc["advance_c_call"].append(ses.last_call_s)
        for nm, ms in zip(("stage_triangulate", "stage_only_line_opt", "stage_solve", "stage_slide_new_frame"), ses.stage_ms()):
            acc[nm].append(ms * 1e-3)
        for nm, b in zip(("h2d_payload_B", "h2d_table_B", "d2h_B"), ses.stats()):
            acc[nm].append(b)
    ses.close()
    ctx.close()
    return acc


def run_imu(M, n_keyframes, halves):
    """one sequence on the consistent IMU stream of tests/test_gpu_odo_imu.py; seconds per keyframe of the C calls and of the
    session's fourth stage (slide + new frame)"""
    import ctypes as C
    import time
    import test_gpu_odo_imu as I
    opt = v.default_options()
    st = I.Stream(M)
    ctx = S._ctxn(1)
    ses = I.session(ctx, 1, opt, imu=not halves)
    I.feed(ses, 0, ctx, st, opt, imu=not halves)
    acc = {"keyframe_c_calls": [], "stage_slide_new_frame": [], "preintegrate_c_call": []}
    for k in range(n_keyframes):
        F = T.NF + k
        if not halves:
            ses.keyframe_imu([v.ImuFrame(st.imu[F], *I.obs_of(M, F))])
            acc["keyframe_c_calls"].append(ses.last_call_s)
            acc["preintegrate_c_call"].append(0.0)
        else:
            res = ses.solve()
            t = ses.last_call_s
            sb = np.zeros(9)
            sb[:3], sb[3:] = M.pred[F][1][:3], I.sb10(res[0])[3:]
            args = [np.ascontiguousarray(a) for a in (np.zeros(1, np.int32), np.array([len(st.imu[F])], np.int32), st.imu[F],
                                                      st.acc0(F)[None], st.gyr0(F)[None], sb[None, 3:6], sb[None, 6:9])]
            pre = (v.capi.Preintegration * 1)()
            ptr = [a.ctypes.data_as(C.POINTER(C.c_int if a.dtype == np.int32 else C.c_double)) for a in args]
            t0 = time.perf_counter()
            rc = ctx.lib.vpl_preintegrate_batch(ctx.h, 1, *ptr, C.byref(opt), pre)
            tp = time.perf_counter() - t0
            assert rc == 0
            ses.advance([v.Frame(*I.obs_of(M, F), pose=M.pred[F][0], speed_bias=sb, preint=pre[0])])
            acc["keyframe_c_calls"].append(t + tp + ses.last_call_s)
            acc["preintegrate_c_call"].append(tp)
        acc["stage_slide_new_frame"].append(ses.stage_ms()[3] * 1e-3)
    ses.close()
    ctx.close()
    return acc


def run_init_align(n, F):
    """seconds per vpl_init_align_batch call over n copies of the F-frame input of tests/test_gpu_init_align.py"""
    import time
    import init_align_inputs as A
    opt = v.default_options()
    q = A.device_input(14, A.KEY14) if F == 14 else A.device_input(40, A.KEY40)
    ctx = v.Context(device=0, max_windows=n, max_points=8, max_point_obs=64, max_lines=8, max_line_obs=64)
    ts = []
    for k in range(8):
        t0 = time.perf_counter()
        res, _, _ = ctx.init_align([q] * n, opt)
        ts.append(time.perf_counter() - t0)
        assert all(r.ok for r in res)
    ctx.close()
    return ts[1:]


def run_init_structure(tag, kws, reps=30):
    """one line: wall time per vpl_init_structure_batch call over the sequences sfm_inputs.sequence(**kw) builds, and its kernels"""
    import time
    import sfm_inputs as si
    qs = [v.SfmInput(**si.sequence(**kw)[0]) for kw in kws]
    ctx = v.Context(device=0, max_windows=len(qs), max_points=8, max_point_obs=64, max_lines=8, max_line_obs=64)
    for _ in range(3):
        res = ctx.init_structure(qs)[0]
    assert all(r.ok for r in res)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.init_structure(qs)
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e3
    ctx.enable_kernel_timing(True)
    ctx.init_structure(qs)
    kt = {k: round(x[0], 3) for k, x in ctx.kernel_times().items() if k.startswith("k_sfm")}
    ctx.close()
    print("init_structure %s: tracks %s, observations %s, BA iterations %s: median %.3f ms (min %.3f, max %.3f) per call; kernels ms %s"
          % (tag, [len(q.track_start) for q in qs], [int(q.track_nobs.sum()) for q in qs], [r.iterations for r in res], np.median(ts), ts.min(),
             ts.max(), kt))


def run_init_relpose(name, n, reps=30):
    """one line: wall time per vpl_init_relative_pose_batch call over n copies of a scene (seeds 0 .. n - 1), and its kernels"""
    import ctypes as C
    import time
    import relpose_inputs as ri
    Sc, _ = ri.scene(name)
    qs = [v.RelPoseInput(seed=k, **Sc) for k in range(n)]
    ci = (v.capi.CRelPoseInput * n)()
    for k, q in enumerate(qs):
        q.to_c(ci[k])
    res = (v.capi.RelPoseResult * n)()
    ctx = v.Context(device=0, max_windows=n, max_points=8, max_point_obs=64, max_lines=8, max_line_obs=64)
    call = lambda: ctx.lib.vpl_init_relative_pose_batch(ctx.h, n, ci, res, None, None, None)
    for _ in range(3):
        assert call() == 0
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e3
    ctx.enable_kernel_timing(True)
    assert call() == 0
    kt = {k: round(x[0], 3) for k, x in ctx.kernel_times().items() if k.startswith("k_relpose")}
    its = [res[0].cand[i].iterations for i in range(10)]
    print("init_relative_pose %s, n_seq=%d: ok %d of %d, iterations of sequence 0 %s: median %.3f ms (min %.3f, max %.3f) per call; kernels ms %s"
          % (name, n, sum(r.ok for r in res), n, its, np.median(ts), ts.min(), ts.max(), kt))
    ctx.close()


def run_init(n):
    """seconds per vpl_odo_init call of a session of n sequences, each the 14-frame input with its observations"""
    import init_align_inputs as A
    opt = v.default_options()
    q = A.device_input(14, A.KEY14)
    M = A.measurements(14, 77)
    frames = [S._obs_frame(M, F) for F in A.KEY14]
    ctx = S._ctxn(n)
    ses = v.Session(ctx, n_seq=n, opt=opt, init_depth=5.0, line_min_obs=T.LINE_MIN_OBS, max_point_tracks=S.MAX_PT, max_line_tracks=S.MAX_LT)
    ts = []
    for k in range(8):
        res = ses.init([q] * n, [M.ex] * n, [frames] * n)
        ts.append(ses.last_call_s)
        assert all(r.ok for r in res)
    ses.close()
    ctx.close()
    return ts[1:]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batch-keyframes", type=int, default=12)
    ap.add_argument("--mode", choices=("plain", "imu", "halves", "rule", "init-align", "init", "init-structure", "init-relpose"), default="plain")
    ap.add_argument("--repeat", type=int, default=1, help="imu / halves: run the sequence this many times, the two modes alternating")
    a = ap.parse_args()
    if a.mode == "init":
        for n in (1, a.batch):
            ts = np.array(run_init(n)) * 1e3
            print("odo_init F=14 n_seq=%d: median %.3f ms (min %.3f, max %.3f) per call" % (n, np.median(ts), ts.min(), ts.max()))
        sys.exit(0)
    if a.mode == "init-relpose":
        for name in ("100 tracks, 20 % outliers", "1024 tracks"):
            for n in (1, a.batch):
                run_init_relpose(name, n)
        sys.exit(0)
    if a.mode == "init-structure":
        import sfm_inputs as si
        big = dict(F=40, key=si.KEY40, l=3, noisy=True, n_tracks=150)
        run_init_structure("1 x F=11", [dict(F=11, key=si.KEY11, l=4, noisy=True)])
        run_init_structure("F=40, 11, 14", [dict(F=40, key=si.KEY40, l=3, noisy=True), dict(F=11, key=si.KEY11, l=4, noisy=True), dict(F=14, key=si.KEY14, l=4)])
        run_init_structure("1 x F=40, 150 tracks", [big])
        run_init_structure("8 x F=40, 150 tracks", [dict(big, track_seed=k) for k in range(8)])
        sys.exit(0)
    if a.mode == "init-align":
        for F in (14, 40):
            for n in (1, a.batch):
                ts = np.array(run_init_align(n, F)) * 1e3
                print("init_align F=%d n_seq=%d: median %.3f ms (min %.3f, max %.3f) per call" % (F, n, np.median(ts), ts.min(), ts.max()))
        sys.exit(0)
    if a.mode == "rule":
        for r in range(a.repeat if a.repeat > 1 else 3):
            for name, rule in (("rule", True), ("plain", False)):
                acc = run([77], T.N_KEYFRAMES, rule=rule)
                acc["keyframe_c_calls"] = list(np.array(acc["solve_c_call"]) + np.array(acc["advance_c_call"]))
                print("%s run %d: %s | d2h %d B, tables %d B" % (name, r, " | ".join("%s median %.4f ms (min %.4f, max %.4f)" % (
                    k, np.median(acc[k][4:]) * 1e3, np.min(acc[k][4:]) * 1e3, np.max(acc[k][4:]) * 1e3)
                    for k in ("stage_slide_new_frame", "advance_c_call", "keyframe_c_calls")), np.median(acc["d2h_B"][4:]), np.median(acc["h2d_table_B"][4:])))
        sys.exit(0)
    if a.mode != "plain":
        M = T.Measurements(T.NF + T.N_KEYFRAMES)
        for r in range(a.repeat):
            for mode in (("imu", "halves") if a.repeat > 1 else (a.mode,)):
                acc = run_imu(M, T.N_KEYFRAMES, mode == "halves")
                print("%s run %d: %s" % (mode, r, " | ".join("%s median %.3f ms (min %.3f, max %.3f)" % (
                    k, np.median(x[4:]) * 1e3, np.min(x[4:]) * 1e3, np.max(x[4:]) * 1e3) for k, x in acc.items())))
        sys.exit(0)
    acc = run([77], T.N_KEYFRAMES)
    tot = np.array(acc["solve_c_call"][4:]) + np.array(acc["advance_c_call"][4:])
    print("keyframe_c_calls: median %.2f ms, min %.2f, max %.2f over %d keyframes (solve + advance, one sequence)"
          % (np.median(tot) * 1e3, tot.min() * 1e3, tot.max() * 1e3, len(tot)))
    for k, x in acc.items():
        x = np.array(x[4:], float)
        if k.endswith("_B"):
            print("%s: median %d bytes per keyframe" % (k, np.median(x)))
        else:
            print("%s: median %.2f ms, min %.2f, max %.2f over %d keyframes" % (k, np.median(x) * 1e3, x.min() * 1e3, x.max() * 1e3, len(x)))
    if a.batch > 1:
        acc = run(list(range(77, 77 + a.batch)), a.batch_keyframes)
        tot = np.array(acc["solve_c_call"][4:]) + np.array(acc["advance_c_call"][4:])
        print("batch of %d sequences: median %.2f ms per call pair = %.0f keyframes / s (stages: %s ms)"
              % (a.batch, np.median(tot) * 1e3, a.batch / np.median(tot),
                 " | ".join("%.2f" % (np.median(acc[s][4:]) * 1e3) for s in ("stage_triangulate", "stage_only_line_opt", "stage_solve", "stage_slide_new_frame"))))
