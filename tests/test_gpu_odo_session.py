"""The keyframe session (vpl_odo_*, v.Session): the feature manager and the window resident on the device, one call per keyframe,
against the loop that keeps them on the host -- tests/test_gpu_sequence.py's Run over vpl_ba_solve_odometry /
vpl_ba_slide_window.  Both sides run the same deterministic kernels on the same bytes (the session gathers on the device what
the loop packs on the host), so the bar is EQUALITY of every number either side produces, keyframe after keyframe, free running:
the chaos test_gpu_sequence's docstring describes does not enter, a single differing bit would.

The new interval's pre-integration starts from the bias the solve has just estimated (Run.keyframe: sb[10, 3:] = sb[9, 3:]
after the slide), so the session is driven through the two halves of vpl_odo_keyframe -- solve, then advance with a frame built
from solve's result -- except where a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

import vplines_slam_amd as v
from test_gpu_sequence import Measurements, Run, Backend, _ctx, _solved_diff, NF, N_KEYFRAMES, LINE_MIN_OBS
from test_gpu_solve import POS_TOL, ROT_TOL

pytestmark = pytest.mark.gpu

MAX_PT, MAX_LT = 1024, 512
RESULT_BYTES = C.sizeof(v.capi.OdoResult)
PREINT_BYTES = C.sizeof(v.capi.Preintegration)


def _preint(ctx, M, F, ba, bg, opt):
    return Backend(ctx).preintegrate(M.imu[F], M.acc0[F], M.gyr0[F], np.array(ba, float), np.array(bg, float), opt)


def _obs_frame(M, F, **kw):
    return v.Frame(list(M.pobs[F]), np.array(list(M.pobs[F].values())).reshape(-1, 3),
                   list(M.lobs[F]), np.array(list(M.lobs[F].values())).reshape(-1, 8), **kw)


def feed_window(ses, seq, ctx, M, opt):
    """frames 0..10 as Run.__init__ sets them up"""
    pose = np.stack([M.pred[F][0] for F in range(NF)])
    sb = np.stack([M.pred[F][1] for F in range(NF)])
    pre = (v.capi.Preintegration * NF)()
    for j in range(1, NF):
        p = _preint(ctx, M, j, sb[j, 3:6], sb[j, 6:9], opt)
        C.memmove(C.byref(pre[j]), C.byref(p), C.sizeof(p))
    ses.set_window(seq, pose, sb, M.ex, pre, [_obs_frame(M, F) for F in range(NF)])


def next_frame(ctx, M, F, res, opt):
    """global frame F enters slot 10 the way Run.keyframe puts it there: predicted pose and velocity, the bias of what is
    frame 9 after the slide (frame 10 of the solve's result), the pre-integration from that bias"""
    sb = np.zeros(9)
    sb[:3] = M.pred[F][1][:3]
    sb[3:] = np.ctypeslib.as_array(res.speed_bias)[NF - 1, 3:]
    return _obs_frame(M, F, pose=M.pred[F][0], speed_bias=sb, preint=_preint(ctx, M, F, sb[3:6], sb[6:9], opt))


class Loop:
    """Run of test_gpu_sequence.py for a LIST of sequences on one context, with the marginalisation flag a parameter: the
    existing entry points called with the batch of windows per keyframe"""

    def __init__(self, ctx, Ms, opt):
        self.ctx, self.opt = ctx, opt
        self.runs = [Run(Backend(ctx), M, opt) for M in Ms]

    def keyframe(self, flag=v.MARGIN_OLD):
        opt = v.default_options()
        C.memmove(C.byref(opt), C.byref(self.opt), C.sizeof(opt))
        opt.marginalization_flag = flag
        sel = []
        for r in self.runs:
            pts = [t for t in r.pts.values() if len(t.obs) >= 2 and t.start < NF - 3]
            lns = [t for t in r.lns.values() if len(t.obs) >= LINE_MIN_OBS and t.start < NF - 3]
            sel.append((pts, lns, r._window(pts, lns)))
        pri, lrep, rep = self.ctx.solve_odometry([s[2] for s in sel], opt, 5.0)
        out = []
        for i, (r, (pts, lns, w)) in enumerate(zip(self.runs, sel)):
            r.prior = v.Prior()
            C.memmove(C.byref(r.prior), C.byref(pri[i]), C.sizeof(r.prior))
            r.pose[:], r.sb[:], r.ex[:] = w.pose, w.speed_bias, w.ex_pose
            for k, t in enumerate(pts):
                t.invd = float(w.inv_depth[k])
            for k, t in enumerate(lns):
                t.plk, t.tri = w.line_plk[k].copy(), int(w.line_triangulated[k])
                if w.line_removed[k]:
                    del r.lns[t.lm]
            for t in [t for t in pts if not t.invd > 0]:
                del r.pts[t.lm]
            out.append(dict(pose=r.pose.copy(), sb=r.sb.copy(), ex=r.ex.copy(), lrep=lrep[i], rep=rep[i], n_points=len(pts),
                            n_lines=int(w.line_triangulated[:len(lns)].sum()) if lns else 0))
        sel = [(list(r.pts.values()), list(r.lns.values())) for r in self.runs]
        ws = [r._window(p, l) for r, (p, l) in zip(self.runs, sel)]
        for w in ws:
            w.prior = None
        sts = self.ctx.slide_window(ws, flag, 5.0)
        for r, (pts, lns), w, st in zip(self.runs, sel, ws, sts):
            r.pose[:], r.sb[:] = w.pose, w.speed_bias
            for book, tr, start, nobs, drop in ((r.pts, pts, st.point_start, st.point_nobs, st.point_drop),
                                                (r.lns, lns, st.line_start, st.line_nobs, st.line_drop)):
                for i, t in enumerate(tr):
                    if nobs[i] == 0:
                        del book[t.lm]
                        continue
                    if drop[i] >= 0:
                        del t.obs[drop[i]]
                    t.start = int(start[i])
                    assert len(t.obs) == nobs[i]
            for i, t in enumerate(pts):
                t.invd = float(w.inv_depth[i])
            for i, t in enumerate(lns):
                t.plk = w.line_plk[i].copy()
            if flag == v.MARGIN_OLD:
                for j in range(1, NF - 1):
                    C.memmove(C.byref(r.pre[j]), C.byref(r.pre[j + 1]), C.sizeof(r.pre[j]))
            r.newest += 1
            F = r.newest
            r.pose[NF - 1], r.sb[NF - 1, :3] = r.M.pred[F][0], r.M.pred[F][1][:3]
            r.sb[NF - 1, 3:] = r.sb[NF - 2, 3:]
            r._preint(NF - 1, F)
            r._add_frame(NF - 1, F)
        return out


def _rep_tuple(r):
    return tuple(getattr(r, f) for f, _ in v.capi.SolveReport._fields_)


def assert_same_solve(k, res, want):
    """the session's result of one sequence against the loop's: states, both reports, the tracks that took part"""
    assert np.array_equal(np.ctypeslib.as_array(res.pose), want["pose"]), (k, "pose")
    assert np.array_equal(np.ctypeslib.as_array(res.speed_bias), want["sb"]), (k, "speed_bias")
    assert np.array_equal(np.ctypeslib.as_array(res.ex_pose), want["ex"]), (k, "ex_pose")
    assert _rep_tuple(res.report) == _rep_tuple(want["rep"]), (k, _rep_tuple(res.report), _rep_tuple(want["rep"]))
    assert _rep_tuple(res.line_report) == _rep_tuple(want["lrep"]), (k, _rep_tuple(res.line_report), _rep_tuple(want["lrep"]))
    assert (res.n_points_solved, res.n_lines_solved) == (want["n_points"], want["n_lines"]), k


def assert_same_tracks(k, ses, seq, run):
    """after the slide and the new frame: the feature manager (order included) and the prior"""
    tr = ses.get_tracks(seq)
    pts, lns = list(run.pts.values()), list(run.lns.values())
    assert np.array_equal(tr["point_id"], [t.lm for t in pts]), (k, "point ids")
    assert np.array_equal(tr["point_start"], [t.start for t in pts]) and np.array_equal(tr["point_nobs"], [len(t.obs) for t in pts]), k
    assert np.array_equal(tr["inv_depth"], np.array([t.invd for t in pts])), (k, "inverse depths")
    assert np.array_equal(tr["line_id"], [t.lm for t in lns]), (k, "line ids")
    assert np.array_equal(tr["line_start"], [t.start for t in lns]) and np.array_equal(tr["line_nobs"], [len(t.obs) for t in lns]), k
    assert np.array_equal(tr["line_triangulated"], [t.tri for t in lns]), (k, "triangulated")
    assert np.array_equal(tr["line_plk"], np.array([t.plk for t in lns]).reshape(-1, 6)), (k, "Pluecker lines")
    p, q = ses.get_prior(seq), run.prior
    assert (p.n, p.n_blocks) == (q.n, q.n_blocks), (k, p.n, q.n)
    for name in ("block_kind", "block_frame", "block_idx"):
        assert list(getattr(p, name))[:p.n_blocks] == list(getattr(q, name))[:q.n_blocks], (k, name)
    assert np.array_equal(p.J(), q.J()), (k, "J0")
    assert np.array_equal(np.ctypeslib.as_array(p.r0)[:p.n], np.ctypeslib.as_array(q.r0)[:q.n]), (k, "r0")
    assert np.array_equal(np.ctypeslib.as_array(p.x0)[:p.n_blocks], np.ctypeslib.as_array(q.x0)[:q.n_blocks]), (k, "x0")


def _ctxn(n):
    return v.Context(device=0, max_windows=n, max_points=256, max_point_obs=256 * NF, max_lines=128, max_line_obs=128 * NF)


def run_pair(seeds, n_keyframes, flags=None, check_traffic=False, prior_rule=None):
    """the loop on one context, the session on a second one of the same capacities, the same measurements"""
    opt = v.default_options()
    n = len(seeds)
    Ms = [Measurements(NF + n_keyframes, seed=s) for s in seeds]
    ctx_a, ctx_b = _ctxn(n), _ctxn(n)
    if prior_rule is not None:
        ctx_a.set_prior_rule(prior_rule)
        ctx_b.set_prior_rule(prior_rule)
    loop = Loop(ctx_a, Ms, opt)
    ses = v.Session(ctx_b, n_seq=n, opt=opt, init_depth=5.0, line_min_obs=LINE_MIN_OBS, max_point_tracks=MAX_PT, max_line_tracks=MAX_LT)
    for i, M in enumerate(Ms):
        feed_window(ses, i, ctx_b, M, opt)
    for i in range(n):
        tr = ses.get_tracks(i)
        assert np.array_equal(tr["point_id"], [t.lm for t in loop.runs[i].pts.values()])
    sizes = []
    for k in range(n_keyframes):
        flag = v.MARGIN_OLD if flags is None else flags[k]
        want = loop.keyframe(flag)
        res = ses.solve([flag] * n)
        d2h_solve = ses.stats()[2]
        for i in range(n):
            assert_same_solve((k, i), res[i], want[i])
        frames = [next_frame(ctx_b, Ms[i], NF + k, res[i], opt) for i in range(n)]
        lines_gathered = [sum(1 for s_, nb in zip(*(ses.get_tracks(i)[f] for f in ("line_start", "line_nobs"))) if nb >= LINE_MIN_OBS and s_ < NF - 3)
                          for i in range(n)]
        nblocks = [ses.get_prior(i).n_blocks for i in range(n)]
        ses.advance(frames)
        for i in range(n):
            assert_same_tracks((k, i), ses, i, loop.runs[i])
            assert res[i].n_point_tracks == len(loop.runs[i].pts) and res[i].n_line_tracks == len(loop.runs[i].lns)
        sizes.append((res[0].n_points_solved, res[0].n_lines_solved))
        if check_traffic:
            h2d, tab, d2h = ses.stats()
            want_h2d = sum(8 * (3 * len(f.point_id) + 8 * len(f.line_id) + 7 + 9) + PREINT_BYTES for f in frames)
            assert h2d == want_h2d, (k, h2d, want_h2d)
            bound = sum(RESULT_BYTES + 4 * (2 * lines_gathered[i] + res[i].n_points_solved) + 4 * (2 + 3 * nblocks[i]) for i in range(n))
            bound += v.capi.ODO_D2H_PAD_BYTES
            print("keyframe %d: h2d payload %d B, tables %d B, d2h %d B (bound %d)" % (k, h2d, tab, d2h, bound))
            assert d2h == d2h_solve and d2h <= bound, (k, d2h, bound)
            # no J0 in either direction: a 45 x 45 prior alone is 16 KB
            assert d2h < 8 * 45 * 45
    bad = ctx_b.debug_guards()
    assert bad == 0, bad
    ses.close()
    ctx_a.close()
    ctx_b.close()
    return sizes


def test_session_is_bit_identical_to_the_host_loop_for_32_keyframes_and_moves_only_the_new_frame(monkeypatch):
    """One sequence, free running, 32 keyframes: Run (the existing loop) against the session -- states, both reports, tracks in
    the solve, and after every slide the whole feature manager and the prior; and what travelled (per keyframe: the new frame's
    doubles down, the result + a few integers up; never a J0).  The contexts are made with VPL_DEBUG_GUARDS=1: the pattern behind
    every device array, the session's store and tables included, is intact at the end."""
    monkeypatch.setenv("VPL_DEBUG_GUARDS", "1")
    opt = v.default_options()
    M = Measurements(NF + N_KEYFRAMES)
    ctx_a, ctx_b = _ctx(), _ctx()

    class Rec(Backend):
        def solve_odometry(self, w, o_):
            self.w = w
            pri, lrep, rep = self.ctx.solve_odometry([w], o_, 5.0)
            self.lrep, self.rep = lrep[0], rep[0]
            q = v.Prior()
            C.memmove(C.byref(q), C.byref(pri[0]), C.sizeof(q))
            return q, rep[0].iterations, rep[0].num_successful_steps, lrep[0].n_lines_removed

    be = Rec(ctx_a)
    run = Run(be, M, opt)
    ses = v.Session(ctx_b, n_seq=1, opt=opt, init_depth=5.0, line_min_obs=LINE_MIN_OBS, max_point_tracks=MAX_PT, max_line_tracks=MAX_LT)
    feed_window(ses, 0, ctx_b, M, opt)
    sizes = []
    for k in range(N_KEYFRAMES):
        solved = run.keyframe()
        # (Run has advanced already: what its solve produced is in `solved` and in the backend's record)
        res = ses.solve()
        d2h_solve = ses.stats()[2]
        r = res[0]
        assert np.array_equal(np.ctypeslib.as_array(r.pose), solved[0]), (k, "pose")
        assert np.array_equal(np.ctypeslib.as_array(r.speed_bias), be.w.speed_bias), (k, "speed_bias")
        assert np.array_equal(np.ctypeslib.as_array(r.ex_pose), be.w.ex_pose), (k, "ex_pose")
        assert _rep_tuple(r.report) == _rep_tuple(be.rep), (k, _rep_tuple(r.report), _rep_tuple(be.rep))
        assert _rep_tuple(r.line_report) == _rep_tuple(be.lrep), (k, _rep_tuple(r.line_report), _rep_tuple(be.lrep))
        n_lines_window = len(be.w.line_start)
        assert (r.n_points_solved, solved[2]) == (solved[1], n_lines_window), k
        assert r.n_lines_solved == (int(be.w.line_triangulated[:n_lines_window].sum()) if n_lines_window else 0), k
        nblocks = ses.get_prior(0).n_blocks
        frame = next_frame(ctx_b, M, NF + k, r, opt)
        ses.advance([frame])
        assert_same_tracks(k, ses, 0, run)
        assert (r.n_point_tracks, r.n_line_tracks) == (len(run.pts), len(run.lns)), k
        # what travelled
        h2d, tab, d2h = ses.stats()
        want_h2d = 8 * (3 * len(frame.point_id) + 8 * len(frame.line_id) + 7 + 9) + PREINT_BYTES
        assert h2d == want_h2d, (k, h2d, want_h2d)
        bound = RESULT_BYTES + 4 * (2 * n_lines_window + r.n_points_solved) + 4 * (2 + 3 * nblocks) + v.capi.ODO_D2H_PAD_BYTES
        print("keyframe %2d: %3d points %2d of %2d lines in the solve | h2d payload %5d B, tables %6d B, d2h %4d B (bound %4d)"
              % (k, r.n_points_solved, r.n_lines_solved, n_lines_window, h2d, tab, d2h, bound))
        assert d2h == d2h_solve and d2h <= bound, (k, d2h, bound)
        assert d2h < 8 * 45 * 45 and h2d < 8 * 45 * 45            # a 45 x 45 J0 alone is 16 KB
        sizes.append((r.n_points_solved, n_lines_window))
    assert ctx_b.debug_guards() == 0
    ses.close()
    ctx_a.close()
    ctx_b.close()
    assert min(s[0] for s in sizes) >= 60 and max(s[1] for s in sizes) >= 10


def test_session_first_keyframes_are_within_the_bars_of_the_oracle():
    """free running against the ORACLE for the first two keyframes: the bar test_free_running_sequence_... applies to k < 2"""
    opt = v.default_options()
    M = Measurements(NF + 2)
    ctx = _ctx()
    orc = Run(Backend(None), M, opt)
    ses = v.Session(ctx, n_seq=1, opt=opt, init_depth=5.0, line_min_obs=LINE_MIN_OBS, max_point_tracks=MAX_PT, max_line_tracks=MAX_LT)
    feed_window(ses, 0, ctx, M, opt)
    for k in range(2):
        b = orc.keyframe()
        tr = ses.get_tracks(0)
        n_lines_window = int(((tr["line_nobs"] >= LINE_MIN_OBS) & (tr["line_start"] < NF - 3)).sum())
        r = ses.solve()[0]
        ses.advance([next_frame(ctx, M, NF + k, r, opt)])
        tr = ses.get_tracks(0)
        a = (np.ctypeslib.as_array(r.pose).copy(), r.n_points_solved, n_lines_window, r.report.iterations, r.report.num_successful_steps, r.line_report.n_lines_removed, sorted(int(i) for i in tr["line_id"]),
             int(tr["line_triangulated"].sum()))
        # (the line ids and flags are compared after the slide and the new frame on both sides)
        b = b[:6] + (sorted(orc.lns), sum(t.tri for t in orc.lns.values()))
        dp, dr, same = _solved_diff(a, b)
        print("keyframe %d: session vs oracle %.2g m %.2g rad, same decisions: %s" % (k, dp, dr, same))
        assert same and dp <= POS_TOL and dr <= ROT_TOL, (k, dp, dr, a[1:6], b[1:6])
    ses.close()
    ctx.close()


def test_batch_of_four_sequences_is_bit_identical_to_the_batched_host_loop(monkeypatch):
    """n_seq = 4 (seeds 77..80) in one session against the existing entry points called with the same four windows per keyframe,
    8 keyframes -- batch against batch; under VPL_DEBUG_GUARDS=1"""
    monkeypatch.setenv("VPL_DEBUG_GUARDS", "1")
    sizes = run_pair([77, 78, 79, 80], 8, check_traffic=True)
    assert min(s[0] for s in sizes) >= 30


def test_margin_second_new_on_alternate_keyframes():
    flags = [v.MARGIN_SECOND_NEW if k % 2 else v.MARGIN_OLD for k in range(8)]
    run_pair([77], 8, flags=flags)


def test_eigen_prior_rule_set_on_the_borrowed_context_applies_to_the_session():
    """vpl_ba_set_prior_rule(VPL_PRIOR_EIGEN) on both contexts: the session calls the same solve, the priors stay equal"""
    run_pair([77], 4, prior_rule=v.PRIOR_EIGEN)


def test_keyframe_in_one_call_equals_solve_then_advance():
    """vpl_odo_keyframe with a frame that is complete beforehand (its bias and pre-integration from the PREVIOUS result) gives
    the bits of the two halves called one after the other with the same frames"""
    opt = v.default_options()
    M = Measurements(NF + 4)
    ctx_a, ctx_b = _ctx(), _ctx()
    sa = v.Session(ctx_a, n_seq=1, opt=opt, line_min_obs=LINE_MIN_OBS, max_point_tracks=MAX_PT, max_line_tracks=MAX_LT)
    sb = v.Session(ctx_b, n_seq=1, opt=opt, line_min_obs=LINE_MIN_OBS, max_point_tracks=MAX_PT, max_line_tracks=MAX_LT)
    feed_window(sa, 0, ctx_a, M, opt)
    feed_window(sb, 0, ctx_b, M, opt)
    bias = np.zeros(6)
    for k in range(4):
        s9 = np.concatenate([M.pred[NF + k][1][:3], bias])
        f = _obs_frame(M, NF + k, pose=M.pred[NF + k][0], speed_bias=s9, preint=_preint(ctx_a, M, NF + k, s9[3:6], s9[6:9], opt))
        ra = sa.keyframe([f])[0]
        rb = sb.solve()[0]
        sb.advance([f])
        assert bytes(ra) == bytes(rb), k
        ta, tb = sa.get_tracks(0), sb.get_tracks(0)
        for name in ta:
            assert np.array_equal(ta[name], tb[name]), (k, name)
        bias = np.ctypeslib.as_array(ra.speed_bias)[NF - 1, 3:].copy()
    for s_ in (sa, sb):
        s_.close()
    ctx_a.close()
    ctx_b.close()


def test_refused_frame_leaves_the_session_as_it_was():
    """a frame that overflows max_point_tracks: VPL_E_CAPACITY, and the following valid keyframe gives the bits of a session
    that never saw the refused call; a bad flag and a missing array likewise"""
    opt = v.default_options()
    M = Measurements(NF + 2)
    ctx_a, ctx_b = _ctx(), _ctx()
    n0 = len({i for F in range(NF) for i in M.pobs[F]})
    cap = n0 + len(M.pobs[NF]) + 8
    sa = v.Session(ctx_a, n_seq=1, opt=opt, line_min_obs=LINE_MIN_OBS, max_point_tracks=cap, max_line_tracks=MAX_LT)
    sb = v.Session(ctx_b, n_seq=1, opt=opt, line_min_obs=LINE_MIN_OBS, max_point_tracks=cap, max_line_tracks=MAX_LT)
    feed_window(sa, 0, ctx_a, M, opt)
    feed_window(sb, 0, ctx_b, M, opt)
    s9 = np.concatenate([M.pred[NF][1][:3], np.zeros(6)])
    good = _obs_frame(M, NF, pose=M.pred[NF][0], speed_bias=s9, preint=_preint(ctx_a, M, NF, s9[3:6], s9[6:9], opt))
    big_ids = np.arange(100000, 100000 + cap + 1)
    big = v.Frame(big_ids, np.tile([0.0, 0.0, 1.0], (len(big_ids), 1)), [], [], pose=M.pred[NF][0], speed_bias=s9, preint=good.preint)
    with pytest.raises(RuntimeError):
        sa.keyframe([big])
    assert sa.last_rc == -4
    with pytest.raises(RuntimeError):
        sa.keyframe([good], [7])
    assert sa.last_rc == -1
    ra, rb = sa.keyframe([good])[0], sb.keyframe([good])[0]
    assert bytes(ra) == bytes(rb)
    ta, tb = sa.get_tracks(0), sb.get_tracks(0)
    for name in ta:
        assert np.array_equal(ta[name], tb[name]), name
    pa, pb = sa.get_prior(0), sb.get_prior(0)
    assert pa.n == pb.n and pa.n > 0 and np.array_equal(pa.J(), pb.J())
    for s_ in (sa, sb):
        s_.close()
    ctx_a.close()
    ctx_b.close()
