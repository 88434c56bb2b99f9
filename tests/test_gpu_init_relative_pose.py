"""vpl_init_relative_pose_batch on the device against the NumPy restatement of Estimator::relativePose (tests/relpose_ref.py) over
the same sample stream (vpl_relpose_debug_plan).

Shapes -- the smallest at which each thing can go wrong (tests/relpose_inputs.py): candidates with 15 and 20 correspondences (not
tried), 21 (the smallest count that is), 65 (one past a wave), 1024 (the cap); a candidate with enough tracks and 18 px of
parallax, so that l = 1; l = 9; a sequence in which nothing succeeds; 20 % outliers, where the loop stops inside the first round of
256 iterations, and 50 %, where it crosses rounds; the trajectory run backwards; between them each of recoverPose's four poses wins
the vote.  Short tracks that end before frame 10 lie between the others in every list.

Every integer and both masks are equal: n_corres, status, the loop's end, the winning (iteration, root), the inlier counts,
recoverPose's count and choice, l, ok, fail.  hyp_count is equal outside the leave-out mask -- the hypotheses on which the
restatement's float64 and np.longdouble runs disagree (test_relpose_reference.py: none on these inputs).  F, R and T of every
candidate are held, as in test_gpu_init_structure.py, to K x max |x64 - x80| over the candidate's solution vector (F, R, T), never
below 1e-12 |x|_inf; K = 32.  Every test prints the ratios it meets (DESIGN.md has the table)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import vplines_slam_amd as v
import relpose_inputs as ri

pytestmark = pytest.mark.gpu

NF = 11
K_BAR = 32.0
GUARDS = os.environ.get("VPL_DEBUG_GUARDS") == "1"


def context():
    return v.Context(device=0, max_windows=4, max_points=8, max_point_obs=64, max_lines=8, max_line_obs=64)


def close(ctx):
    if GUARDS:
        assert ctx.debug_guards() == 0
    ctx.close()


def raw(x):
    return C.string_at(C.addressof(x), C.sizeof(x))


@functools.lru_cache(maxsize=None)
def dev_input(name):
    S, _ = ri.scene(name)
    return v.RelPoseInput(seed=ri.seed_of(name), **S)


def compare(tag, name, res, m0, m1, hyp):
    """one sequence's result against the restatement of scene `name`"""
    r64, r80 = ri.restated(name)
    assert (res.ok, res.fail, res.l) == (r64["ok"], r64["fail"], r64["l"]), (tag, res.ok, res.fail, res.l, r64["ok"], r64["fail"], r64["l"])
    leave = r64["hyp"] != r80["hyp"]
    assert np.array_equal(hyp[~leave], r64["hyp"][~leave]), (tag, "hyp_count", np.argwhere((hyp != r64["hyp"]) & ~leave)[:5])
    worst = 0.0
    for i in range(NF - 1):
        c = res.cand[i]
        got = (c.n_corres, c.status, c.iterations, c.best_iteration, c.best_root, c.inliers, c.good, c.pose_choice, c.numeric)
        want = tuple(int(r64[k][i]) for k in ("n_corres", "status", "iterations", "best_iteration", "best_root", "inliers", "good", "choice")) + (0,)
        assert got == want, (tag, i, got, want)
        N = c.n_corres
        assert np.array_equal(m0[i, :N], r64["mask_ransac"][i]) and np.array_equal(m1[i, :N], r64["mask_pose"][i]), (tag, i, "masks")
        assert not m0[i, N:].any() and not m1[i, N:].any()
        p64, p80 = float(r64["average_parallax"][i]), float(r80["average_parallax"][i])
        assert abs(c.average_parallax - p64) <= max(K_BAR * abs(p64 - p80), 1e-12 * abs(p64)), (tag, i, c.average_parallax, p64)
        x = np.concatenate([np.array(c.F), np.array(c.R), np.array(c.T)])
        x64, x80 = (np.concatenate([r["F"][i].reshape(-1), r["R"][i].reshape(-1), r["T"][i].reshape(-1)]) for r in (r64, r80))
        if not x64.any():
            assert not x.any(), (tag, i, "a candidate without a model hands out nothing")
            continue
        d = float(np.abs(x64 - x80).max())
        bar = max(K_BAR * d, 1e-12 * float(np.abs(x64).max()))
        err = float(np.abs(x - x64.astype(np.float64)).max())
        worst = max(worst, err / d if d > 0 else 0.0)
        assert err <= bar, (tag, i, err, bar, d)
    if res.ok:
        assert np.array_equal(np.array(res.relative_R), np.array(res.cand[res.l].R)) and np.array_equal(np.array(res.relative_T), np.array(res.cand[res.l].T))
    else:
        assert not np.array(res.relative_R).any() and not np.array(res.relative_T).any()
    print("%s: ok %d l %d, statuses %s, iterations %s; worst ratio of |dev - x64| to max|x64 - x80| over (F, R, T): %.2f"
          % (tag, res.ok, res.l, [res.cand[i].status for i in range(NF - 1)], [res.cand[i].iterations for i in range(NF - 1)], worst))


def solve_alone(ctx, names):
    for name in names:
        res, m0, m1, hyp = ctx.init_relative_pose([dev_input(name)])
        compare(name + " alone", name, res[0], m0[0], m1[0], hyp[0])


def test_counts_15_20_21_and_65():
    ctx = context()
    solve_alone(ctx, ("counts 15 20 21 65",))
    close(ctx)


def test_outliers_inside_the_first_round_and_across_rounds():
    ctx = context()
    solve_alone(ctx, ("100 tracks, 20 % outliers", "60 tracks, 50 % outliers"))
    close(ctx)


def test_the_cap_of_1024_tracks():
    ctx = context()
    solve_alone(ctx, ("1024 tracks",))
    close(ctx)


def test_noisy_observations_forwards_and_backwards():
    ctx = context()
    solve_alone(ctx, ("333 tracks, noisy", "backwards"))
    close(ctx)


def test_l_is_the_first_frame_that_succeeds():
    """frame 0 with enough tracks and too little parallax: l = 1; nothing pairs with frame 10 before frame 9: l = 9"""
    ctx = context()
    solve_alone(ctx, ("frame 0 without parallax", "l = 9"))
    close(ctx)


def test_three_sequences_in_one_call():
    """each against the restatement, bit-identical to the same sequence alone and to a second run; the sequence in which nothing
    succeeds comes back with ok = 0, l = -1 and a zero pose"""
    ctx = context()
    names = ("60 tracks, 50 % outliers", "nothing succeeds", "counts 15 20 21 65")
    qs = [dev_input(n) for n in names]
    res, m0, m1, hyp = ctx.init_relative_pose(qs)
    for i, name in enumerate(names):
        compare("%s (sequence %d of 3)" % (name, i), name, res[i], m0[i], m1[i], hyp[i])
        one, a0, a1, ah = ctx.init_relative_pose([qs[i]])
        assert raw(one[0]) == raw(res[i]) and np.array_equal(a0[0], m0[i]) and np.array_equal(a1[0], m1[i]) and np.array_equal(ah[0], hyp[i]), name
    again, b0, b1, bh = ctx.init_relative_pose(qs)
    assert raw(again) == raw(res) and np.array_equal(b0, m0) and np.array_equal(b1, m1) and np.array_equal(bh, hyp)
    assert (res[1].ok, res[1].fail, res[1].l) == (0, v.capi.RELPOSE_FAIL_NONE, -1)
    # the same seed in another place of the batch, another seed in the same place
    swapped, _, _, _ = ctx.init_relative_pose(qs[::-1])
    assert raw(swapped[2]) == raw(res[0]) and raw(swapped[0]) == raw(res[2])
    S, _ = ri.scene(names[0])
    other, _, _, oh = ctx.init_relative_pose([v.RelPoseInput(seed=5, **S)])
    assert other[0].ok == 1 and other[0].l == res[0].l and not np.array_equal(oh[0], hyp[0])
    # without the optional arrays
    bare = ctx.init_relative_pose(qs, want_masks=False, want_hyp=False)
    assert raw(bare[0]) == raw(res) and bare[1] is None and bare[3] is None
    close(ctx)


def test_a_nan_observation_fails_its_sequence_and_leaves_the_neighbours():
    ctx = context()
    name = "100 tracks, 20 % outliers"
    S, truth = ri.scene(name)
    good, g0, g1, gh = ctx.init_relative_pose([dev_input(name)])
    obs = S["track_obs"].copy()
    j = int(truth["tracks"][0][0])                    # a track every candidate pairs with frame 10: its observation there
    obs[int(np.sum(S["track_nobs"][:j + 1])) - 1, 1] = np.nan
    bad = v.RelPoseInput(seed=ri.seed_of(name), **dict(S, track_obs=obs))
    two, m0, m1, hyp = ctx.init_relative_pose([bad, dev_input(name)])
    assert two[0].ok == 0 and two[0].fail & v.capi.RELPOSE_FAIL_NUMERIC and two[0].l == -1
    assert not np.array(two[0].relative_R).any() and not np.array(two[0].relative_T).any()
    assert all(two[0].cand[i].numeric == 1 and two[0].cand[i].status != v.capi.RELPOSE_SUCCESS for i in range(NF - 1))
    assert raw(two[1]) == raw(good[0]) and np.array_equal(m0[1], g0[0]) and np.array_equal(m1[1], g1[0]) and np.array_equal(hyp[1], gh[0])
    close(ctx)


def test_refusals_leave_the_next_call_unaffected():
    ctx = context()
    name = "counts 15 20 21 65"
    S, _ = ri.scene(name)
    q = dev_input(name)
    first, f0, _, fh = ctx.init_relative_pose([q])
    allocs = ctx.debug_allocs()

    def variant(**kw):
        return v.RelPoseInput(seed=ri.seed_of(name), **dict(S, **kw))

    cases = []
    for field in ("track_start", "track_nobs", "track_obs"):
        ci = q.to_c()
        setattr(ci, field, None)
        cases.append(("null " + field, [ci], -1))
    nobs = S["track_nobs"].copy()
    j = int(np.argmax(S["track_start"] + nobs == NF))
    nobs[j] += 1
    cases.append(("a track past frame 10", [variant(track_nobs=nobs, track_obs=np.concatenate([S["track_obs"], S["track_obs"][:1]]))], -1))
    nobs = S["track_nobs"].copy()
    nobs[0] = 0
    cases.append(("a track without observations", [variant(track_nobs=nobs)], -1))
    start = S["track_start"].copy()
    start[0] = -1
    cases.append(("a track that starts before the window", [variant(track_start=start)], -1))
    ci = q.to_c()
    ci.n_tracks = -1
    cases.append(("a negative count", [ci], -1))
    n = v.capi.SFM_MAX_TRACKS + 1
    cases.append(("more tracks than the cap", [variant(track_start=np.zeros(n), track_nobs=np.ones(n), track_obs=np.zeros((n, 2)))], -4))
    cases.append(("more sequences than max_windows", [q] * 5, -4))
    cases.append(("a bad sequence behind a good one", [q, variant(track_nobs=nobs)], -1))
    for what, inputs, code in cases:
        assert ctx.init_relative_pose(inputs, check=False) == code, what
        again, a0, _, ah = ctx.init_relative_pose([q])
        assert raw(again) == raw(first) and np.array_equal(a0, f0) and np.array_equal(ah, fh), what
    assert ctx.debug_allocs() == allocs      # the call gives back every array it takes
    # no track at all is not refused: nothing to pair, nothing succeeds
    none, _, _, _ = ctx.init_relative_pose([v.RelPoseInput([], [], np.zeros((0, 2)))])
    assert (none[0].ok, none[0].fail, none[0].l) == (0, v.capi.RELPOSE_FAIL_NONE, -1)
    close(ctx)


def test_init_visual_feeds_the_structure_and_the_alignment():
    """exact observations end to end: Context.init_visual on the F = 14 input of the structure tests (its l / relative_R /
    relative_T thrown away), then Context.init_align with the raw IMU stream.  The metric distance between the camera centres of
    frames l and 10 is s times their SfM distance, to 1e-6 relative of the same quantity from the exact frames of
    init_align_inputs.sfm_frames (the bar of tests/test_gpu_init_structure.py).  vpl_init_visual_batch, the same composition in
    C, gives the same bits."""
    import init_align_inputs as ai
    import sfm_inputs as si
    ctx, opt = context(), v.default_options()
    S, truth = si.case("F14 l4 exact")
    blank = v.SfmInput(**dict(S, l=0, relative_R=np.zeros((3, 3)), relative_T=np.zeros(3)))
    rel, st = ctx.init_visual([blank], seeds=[11])
    assert rel[0].ok == 1 and st[0] is not None and st[0][0].ok == 1
    l = rel[0].l
    res = st[0][0]
    a = res.arrays()
    F, key = 14, si.KEY14
    base = ai.device_input(F, key)
    q = v.capi.InitInput(a["frame_R"][:F], a["frame_T"][:F], base.n_samples, base.samples, base.acc0, base.gyr0, base.lin_ba, base.lin_bg,
                         base.key, base.bas, base.bgs, base.tic)
    out, _, _ = ctx.init_align([q], opt, want_preint=False)
    want, _, _ = ctx.init_align([base], opt, want_preint=False)
    assert out[0].ok == 1 and want[0].ok == 1
    f0, f1 = key[l], key[NF - 1]
    got_d = out[0].s * np.linalg.norm(a["frame_T"][f1] - a["frame_T"][f0])
    want_d = want[0].s * np.linalg.norm(base.T[f1] - base.T[f0])
    print("l = %d; metric distance of the cameras of frames l and 10: %.9f from the relative pose and the structure, %.9f from the exact frames "
          "(relative difference %.3g)" % (l, got_d, want_d, abs(got_d - want_d) / want_d))
    # the C twin: one call, the same bits
    ci = (v.capi.CSfmInput * 1)()
    blank.to_c(ci[0])
    seeds = (C.c_ulonglong * 1)(11)
    crel, cres = (v.capi.RelPoseResult * 1)(), (v.capi.SfmResult * 1)()
    assert ctx.lib.vpl_init_visual_batch(ctx.h, 1, ci, seeds, crel, cres, None, None, None, None) == 0
    assert raw(crel[0]) == raw(rel[0]) and raw(cres[0]) == raw(res)
    assert abs(got_d - want_d) <= 1e-6 * want_d
    close(ctx)


def test_init_visual_skips_the_sequence_whose_relative_pose_fails():
    import sfm_inputs as si
    ctx = context()
    S, _ = si.case("F11 l4 exact")
    T, _ = ri.scene("nothing succeeds")
    n = len(T["track_start"])
    dead = v.SfmInput(**dict(S, track_id=np.arange(n), track_start=T["track_start"], track_nobs=T["track_nobs"], track_obs=T["track_obs"]))
    live = v.SfmInput(**S)
    rel, st = ctx.init_visual([dead, live], seeds=[ri.seed_of("nothing succeeds"), 3])
    assert rel[0].ok == 0 and st[0] is None and rel[1].ok == 1 and st[1][0].ok == 1
    alone_rel, alone = ctx.init_visual([live], seeds=[3])
    assert raw(alone_rel[0]) == raw(rel[1]) and raw(alone[0][0]) == raw(st[1][0])
    ci = (v.capi.CSfmInput * 2)()
    dead.to_c(ci[0])
    live.to_c(ci[1])
    seeds = (C.c_ulonglong * 2)(ri.seed_of("nothing succeeds"), 3)
    crel, cres = (v.capi.RelPoseResult * 2)(), (v.capi.SfmResult * 2)()
    pb = np.ones((2, v.capi.SFM_MAX_TRACKS, 3))
    assert ctx.lib.vpl_init_visual_batch(ctx.h, 2, ci, seeds, crel, cres, None, pb.ctypes.data_as(C.POINTER(C.c_double)), None, None) == 0
    assert raw(crel) == raw(rel) and raw(cres[1]) == raw(st[1][0]) and np.array_equal(pb[1], st[1][2])
    assert (cres[0].ok, cres[0].fail) == (0, v.capi.SFM_FAIL_RELATIVE_POSE) and not pb[0].any()
    close(ctx)


def test_everything_under_debug_guards_in_a_fresh_process():
    """every test above once more with VPL_DEBUG_GUARDS=1 (read when a context is made): the pattern behind every device array the
    call takes is checked inside the call, the context's own when it is closed"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, VPL_DEBUG_GUARDS="1", PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    code = ("import test_gpu_init_relative_pose as t; assert t.GUARDS\n"
            "for name in sorted(dir(t)):\n"
            "    if name.startswith('test_') and 'fresh_process' not in name: getattr(t, name)()\n"
            "print('guards ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=here, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "guards ok" in r.stdout
