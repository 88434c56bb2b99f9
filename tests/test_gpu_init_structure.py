"""vpl_init_structure_batch on the device against the NumPy restatement of GlobalSFM::construct and the frame PnP
(tests/sfm_ref.py), stage by stage: the schedule's integers, what the chain leaves, what the BA leaves, then R / T of every image frame.

Shapes -- the smallest at which each thing can go wrong: F = 11 with every frame a key frame and l = 4 (both halves of the chain; 70
tracks, about 400 observations: more than one wave of lanes); l = 0 (no backward chain) and l = 9 (no forward PnP); F = 14 with KEY14
(the PnP of three non-key frames); F = 40 (the cap: 29 non-key frames); one call with F = 40, 11, 14 in that order; exact observations
and observations with half a pixel of noise; a key frame seen by 9 triangulated points; a non-key frame that lists 5.

Integers and decisions are equal: iterations, successful steps, termination, the iterations of every PnP, the fail mask.  The numbers
are held, as in test_gpu_init_align.py, to a bar measured from the restatement itself: K x max |x64 - x80| over the solution vector of
the stage a number comes from (its float64 against its np.longdouble run on the same input), never below 1e-12 |x|_inf; K = 32 leaves a
decade for the device's summation order and its sin / cos.  Every test prints the ratios it meets (DESIGN.md has the table)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import vplines_slam_amd as v
import sfm_ref as ref
import sfm_inputs as si

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
    S, _ = si.case(name)
    return v.SfmInput(**S)


def stage_vectors(r, F):
    """the solution vector of every stage of a restatement's run"""
    f64 = lambda *a: np.concatenate([np.asarray(x).astype(np.float64).reshape(-1) for x in a])
    return dict(chain=f64(r["chain_q"], r["chain_t"], r["points_chain"]), ba=f64(r["ba_q"], r["ba_t"], r["points_ba"], r["Q"], r["T"]),
                frames=f64(r["R"], r["Tf"]))


def device_vectors(res, pc, pb, n, F):
    a = res.arrays()
    return dict(chain=np.concatenate([a["chain_q"].reshape(-1), a["chain_t"].reshape(-1), pc[:n].reshape(-1)]),
                ba=np.concatenate([a["ba_q"].reshape(-1), a["ba_t"].reshape(-1), pb[:n].reshape(-1), a["Q"].reshape(-1), a["T"].reshape(-1)]),
                frames=np.concatenate([a["frame_R"][:F].reshape(-1), a["frame_T"][:F].reshape(-1)]))


def compare(tag, name, res, pc, pb, tracked):
    """one sequence's result against the restatement of case `name`"""
    S, _ = si.case(name)
    r64, r80 = si.restated(name)
    F, N = S["n_frames"], len(S["track_start"])
    plan = v.sfm_debug_plan(S["l"], S["track_start"], S["track_nobs"])
    for k in ("step", "fa", "fb", "count"):
        assert np.array_equal(plan[k], r64["plan"][k]), (tag, k)
    assert plan["first_fail"] == r64["plan"]["first_fail"]
    assert (res.ok, res.fail) == (r64["ok"], r64["fail"]), (tag, res.ok, res.fail, r64["ok"], r64["fail"])
    assert (res.iterations, res.successful_steps, res.termination) == (r64["iterations"], r64["successful_steps"], r64["termination"]), \
        (tag, res.iterations, res.successful_steps, res.termination, r64["iterations"], r64["successful_steps"], r64["termination"])
    a = res.arrays()
    if not (r64["fail"] & (ref.FAIL_KEY_PNP | ref.FAIL_NUMERIC)):
        assert np.array_equal(a["pnp_iterations"], r64["pnp_iterations"]), (tag, a["pnp_iterations"], r64["pnp_iterations"])
    if r64["ok"]:
        assert np.array_equal(a["frame_iterations"][:F], r64["frame_iterations"]), (tag, a["frame_iterations"][:F], r64["frame_iterations"])
        assert not (a["frame_iterations"][F:] != -1).any()
    got, w64, w80 = device_vectors(res, pc, pb, N, F), stage_vectors(r64, F), stage_vectors(r80, F)
    assert not pc[N:].any() and not pb[N:].any() and not a["frame_R"][F:].any() and not a["frame_T"][F:].any()
    rows = []
    for st in ("chain", "ba", "frames"):
        if not w64[st].any():
            assert not got[st].any(), (tag, st, "nothing behind a failing stage is handed out")
            rows.append("%s zeroed" % st)
            continue
        d = np.abs(w64[st] - w80[st]).max()
        bar = max(K_BAR * d, 1e-12 * np.abs(w64[st]).max())
        err = np.abs(got[st] - w64[st]).max()
        rows.append("%s %.2f (%.2g of %.2g)" % (st, err / d if d > 0 else 0.0, err, bar))
        assert err <= bar, (tag, st, err, bar, d)
    for name_, dev, want in (("initial_cost", res.initial_cost, r64["initial_cost"]), ("final_cost", res.final_cost, r64["final_cost"])):
        d = abs(float(r64[name_]) - float(r80[name_]))
        bar = max(K_BAR * d, 1e-12 * abs(float(want)))
        rows.append("%s %.2f" % (name_, abs(dev - float(want)) / d if d > 0 else 0.0))
        assert abs(dev - float(want)) <= bar, (tag, name_, dev, float(want), bar)
    ids, xyz = tracked
    if r64["Q"].any():                                # the BA passed: sfm_tracked_points
        tri = np.nonzero(plan["step"] >= 0)[0]
        assert res.n_tracked == len(tri) and np.array_equal(ids, S["track_id"][tri]) and np.array_equal(xyz, pb[tri])
    else:
        assert res.n_tracked == 0 and len(ids) == 0
    print("%s: ok %d fail %d, BA %d iterations (%d successful, termination %d); ratio to max|x64 - x80| (error of bar): %s"
          % (tag, res.ok, res.fail, res.iterations, res.successful_steps, res.termination, ", ".join(rows)))


def plan_of(S):
    return v.sfm_debug_plan(S["l"], S["track_start"], S["track_nobs"])


def solve_alone(ctx, names):
    for name in names:
        res, pc, pb, tr = ctx.init_structure([dev_input(name)])
        compare(name + " alone", name, res[0], pc[0], pb[0], tr[0])


def test_11_frames_both_halves_of_the_chain_exact_and_noisy():
    ctx = context()
    solve_alone(ctx, ("F11 l4 exact", "F11 l4 noisy"))
    close(ctx)


def test_l_at_either_end_of_the_window():
    ctx = context()
    solve_alone(ctx, ("F11 l0 noisy", "F11 l9 exact"))
    close(ctx)


def test_14_frames_with_three_non_key_frames():
    ctx = context()
    solve_alone(ctx, ("F14 l4 exact", "F14 l6 noisy"))
    close(ctx)


def test_40_frames():
    ctx = context()
    solve_alone(ctx, ("F40 l5 exact", "F40 l3 noisy"))
    close(ctx)


def test_three_sequences_in_one_call():
    """F = 40, 11, 14 in one launch: each against the restatement, bit-identical to the same sequence alone and to a second run"""
    ctx = context()
    names = ("F40 l3 noisy", "F11 l4 noisy", "F14 l4 exact")
    qs = [dev_input(n) for n in names]
    res, pc, pb, tr = ctx.init_structure(qs)
    for i, name in enumerate(names):
        compare("%s (sequence %d of 3)" % (name, i), name, res[i], pc[i], pb[i], tr[i])
        one, pc1, pb1, tr1 = ctx.init_structure([qs[i]])
        assert raw(one[0]) == raw(res[i]) and np.array_equal(pc1[0], pc[i]) and np.array_equal(pb1[0], pb[i]), name
        assert np.array_equal(tr1[0][0], tr[i][0]) and np.array_equal(tr1[0][1], tr[i][1])
    again, pc2, pb2, _ = ctx.init_structure(qs)
    assert raw(again) == raw(res) and np.array_equal(pc2, pc) and np.array_equal(pb2, pb)
    close(ctx)


def test_starved_frames_fail_their_sequence_and_leave_the_neighbours():
    """a key frame seen by 9 triangulated points (forward and backward chain), a non-key frame that lists 5: the flag, everything
    behind the failing stage zero, the neighbours in the batch bit for bit what they are alone"""
    ctx = context()
    names = ("F11 l4 noisy, frame 5 starved", "F11 l4 noisy", "F14 l4 noisy, image frame 7 starved", "F11 l4 noisy, frame 2 starved")
    qs = [dev_input(n) for n in names]
    res, pc, pb, tr = ctx.init_structure(qs)
    for i, name in enumerate(names):
        compare(name, name, res[i], pc[i], pb[i], tr[i])
    plan = v.sfm_debug_plan(4, qs[0].track_start, qs[0].track_nobs)
    assert plan["count"][5] == 9 and plan["first_fail"] == 5
    plan = v.sfm_debug_plan(4, qs[3].track_start, qs[3].track_nobs)
    assert plan["count"][2] == 9 and plan["first_fail"] == 2
    assert res[0].fail == res[3].fail == v.capi.SFM_FAIL_KEY_PNP and res[0].ok == 0
    assert not pc[0].any() and not pb[0].any() and not res[0].arrays()["Q"].any()
    assert res[2].fail == v.capi.SFM_FAIL_FRAME_PNP and res[2].ok == 0
    a = res[2].arrays()
    assert a["Q"].any() and res[2].n_tracked > 0 and not a["frame_R"].any() and not a["frame_T"].any()
    good, pcg, pbg, _ = ctx.init_structure([qs[1]])
    assert raw(good[0]) == raw(res[1]) and good[0].ok == 1 and np.array_equal(pbg[0], pb[1]) and np.array_equal(pcg[0], pc[1])
    # a non-finite observation is not refused: that sequence fails with the numeric bit, its neighbour is untouched
    S, _ = si.case("F11 l4 noisy")
    obs = S["track_obs"].copy()
    j = int(np.argmax(plan_of(S)["step"] == 1))       # a track frames l and 10 triangulate
    obs[int(np.sum(S["track_nobs"][:j])), 0] = np.nan
    bad = v.SfmInput(**dict(S, track_obs=obs))
    two, _, pb2, _ = ctx.init_structure([bad, qs[1]])
    assert two[0].ok == 0 and two[0].fail & v.capi.SFM_FAIL_NUMERIC
    assert raw(two[1]) == raw(good[0]) and np.array_equal(pb2[1], pbg[0])
    close(ctx)


def test_refusals_leave_the_next_call_unaffected():
    ctx = context()
    name = "F14 l4 exact"
    S, _ = si.case(name)
    q = dev_input(name)
    first, _, pb0, _ = ctx.init_structure([q])
    allocs = ctx.debug_allocs()

    def variant(**kw):
        return v.SfmInput(**dict(S, **kw))

    cases = []
    for field in ("track_id", "track_start", "track_nobs", "track_obs", "frame_npts", "frame_id", "frame_xy"):
        ci = q.to_c()
        setattr(ci, field, None)
        cases.append(("null " + field, [ci], -1))
    cases.append(("l = 10", [variant(l=10)], -1))
    cases.append(("l = -1", [variant(l=-1)], -1))
    key = S["key"].copy()
    key[6] = key[5]
    cases.append(("key repeats", [variant(key=key)], -1))
    cases.append(("key[10] != F - 1", [variant(key=np.arange(11))], -1))
    key = S["key"].copy()
    key[0] = 1
    cases.append(("key[0] != 0", [variant(key=key)], -1))
    cases.append(("F < 11", [variant(n_frames=10, key=np.arange(11), frame_pts={})], -1))
    nobs = S["track_nobs"].copy()
    j = int(np.argmax(S["track_start"] + nobs == NF))
    nobs[j] += 1
    cases.append(("a track past frame 10", [variant(track_nobs=nobs, track_obs=np.concatenate([S["track_obs"], S["track_obs"][:1]]))], -1))
    nobs = S["track_nobs"].copy()
    nobs[0] = 0
    cases.append(("a track without observations", [variant(track_nobs=nobs)], -1))
    cases.append(("F > 40", [variant(n_frames=41, key=np.array(si.KEY40[:10] + (40,)))], -4))
    n = v.capi.SFM_MAX_TRACKS + 1
    cases.append(("more tracks than the cap", [variant(track_id=np.arange(n), track_start=np.zeros(n), track_nobs=np.ones(n), track_obs=np.zeros((n, 2)))], -4))
    m = v.capi.SFM_MAX_FRAME_POINTS + 1
    cases.append(("a frame list longer than the cap", [variant(frame_pts={3: (np.arange(m), np.zeros((m, 2)))})], -4))
    cases.append(("more sequences than max_windows", [q] * 5, -4))
    cases.append(("a bad sequence behind a good one", [q, variant(l=10)], -1))
    for what, inputs, code in cases:
        assert ctx.init_structure(inputs, check=False) == code, what
        again, _, pb1, _ = ctx.init_structure([q])
        assert raw(again) == raw(first) and np.array_equal(pb1, pb0), what
    assert ctx.debug_allocs() == allocs      # the call gives back every array it takes
    close(ctx)


def test_the_result_feeds_the_alignment():
    """exact observations end to end: R / T of the call into Context.init_align with the raw IMU stream of init_align_inputs.  The
    metric distance between the camera centres of frames l and 10 is s times their SfM distance, to 1e-6 relative of the same
    quantity from the exact frames of init_align_inputs.sfm_frames."""
    import init_align_inputs as ai
    ctx, opt = context(), v.default_options()
    name = "F14 l4 exact"
    S, _ = si.case(name)
    res, _, _, _ = ctx.init_structure([dev_input(name)])
    assert res[0].ok == 1
    a = res[0].arrays()
    F, key, l = 14, si.KEY14, S["l"]
    base = ai.device_input(F, key)
    q = v.capi.InitInput(a["frame_R"][:F], a["frame_T"][:F], base.n_samples, base.samples, base.acc0, base.gyr0, base.lin_ba, base.lin_bg,
                         base.key, base.bas, base.bgs, base.tic)
    out, _, _ = ctx.init_align([q], opt, want_preint=False)
    want, _, _ = ctx.init_align([base], opt, want_preint=False)
    assert out[0].ok == 1 and want[0].ok == 1
    f0, f1 = key[l], key[NF - 1]
    got_d = out[0].s * np.linalg.norm(a["frame_T"][f1] - a["frame_T"][f0])
    want_d = want[0].s * np.linalg.norm(base.T[f1] - base.T[f0])
    M = ai.measurements(F, 77)
    _, _, T_exact, _ = ai.sfm_frames(M, F, 5)
    true_d = ai.SCALE * np.linalg.norm(T_exact[f1] - T_exact[f0])
    print("metric distance of the cameras of frames l and 10: %.9f from the structure, %.9f from the exact frames (relative difference %.3g); true %.9f"
          % (got_d, want_d, abs(got_d - want_d) / want_d, true_d))
    assert abs(got_d - want_d) <= 1e-6 * want_d
    close(ctx)


def test_everything_under_debug_guards_in_a_fresh_process():
    """every test above once more with VPL_DEBUG_GUARDS=1 (read when a context is made): the pattern behind every device array the
    call takes is checked inside the call, the context's own when it is closed"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, VPL_DEBUG_GUARDS="1", PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    code = ("import test_gpu_init_structure as t; assert t.GUARDS\n"
            "for name in sorted(dir(t)):\n"
            "    if name.startswith('test_') and 'fresh_process' not in name: getattr(t, name)()\n"
            "print('guards ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=here, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "guards ok" in r.stdout
