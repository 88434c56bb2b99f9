"""The vision-only initial structure without a GPU: the host-built schedule of GlobalSFM::construct (vpl_sfm_debug_plan) against the
NumPy restatement's (tests/sfm_ref.py), the plain-C++ header that builds it under the sanitizers, and the restatement itself held to
ground truth and to its own extended-precision run."""
import ctypes as C
import os
import subprocess

import numpy as np

import vplines_slam_amd as v
import sfm_ref as ref
import sfm_inputs as si

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_debug_plan_equals_the_restatements_schedule():
    """300 random track tables -- sparse ones starve a frame's PnP -- and every l"""
    rng = np.random.default_rng(11)
    starved = 0
    for rep in range(300):
        start, nobs = si.random_tables(rng, int(rng.integers(0, 25)) if rep % 3 == 0 else int(rng.integers(25, 140)))
        for l in range(10):
            got, want = v.sfm_debug_plan(l, start, nobs), ref.schedule(l, start, nobs)
            for name in ("step", "fa", "fb", "count"):
                assert np.array_equal(got[name], want[name]), (rep, l, name)
            assert got["first_fail"] == want["first_fail"], (rep, l)
            starved += want["first_fail"] >= 0
    assert 500 < starved < 2500, starved    # both kinds are well represented
    # the sequences of the GPU tests
    for name in si.CASES:
        S, _ = si.case(name)
        got, want = v.sfm_debug_plan(S["l"], S["track_start"], S["track_nobs"]), ref.schedule(S["l"], S["track_start"], S["track_nobs"])
        assert all(np.array_equal(got[k], want[k]) for k in ("step", "fa", "fb", "count")) and got["first_fail"] == want["first_fail"], name


def test_debug_plan_refusals():
    assert v.sfm_debug_plan(10, [0], [2]) == -1
    assert v.sfm_debug_plan(-1, [0], [2]) == -1
    assert v.sfm_debug_plan(3, [9], [3]) == -1                 # runs past frame 10
    assert v.sfm_debug_plan(3, [9], [0]) == -1
    assert v.sfm_debug_plan(3, [11], [1]) == -1
    assert v.sfm_debug_plan(3, np.zeros(v.capi.SFM_MAX_TRACKS + 1), np.ones(v.capi.SFM_MAX_TRACKS + 1)) == -4
    assert v.sfm_debug_plan(3, np.zeros(v.capi.SFM_MAX_TRACKS), np.ones(v.capi.SFM_MAX_TRACKS))["first_fail"] == 4


def test_struct_layouts():
    # what the header implies (ints, doubles, pointers; natural alignment)
    assert C.sizeof(v.capi.CSfmInput) == 4 * 14 + 8 * 21 + 8 + 8 * 4 + 8 * 3
    assert C.sizeof(v.capi.SfmResult) == 4 * (6 + 11 + 40) + 4 + 8 * (2 + 3 * 11 * 7 + 40 * 12)


def test_plan_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "sfm_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "vplines-slam_amd", "csrc"), os.path.join(ROOT, "tests", "native", "sfm_plan_check.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "sfm plan ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_restatement_recovers_the_truth_from_exact_observations():
    """In the gauge of construct -- frame l's camera the origin, the distance between the cameras of frames l and 10 the unit -- the
    restatement alone finds the true cameras and points to 1e-6 relative (a wrong Jacobian or gauge shows as 1e-2; LM stops on 1e-6 of
    the cost and 1e-8 of the step at quadratic convergence)."""
    for name in ("F11 l4 exact", "F11 l9 exact", "F14 l4 exact", "F40 l5 exact"):
        S, truth = si.case(name)
        r = ref.initial_structure(S, np.float64)
        assert r["ok"] == 1 and r["fail"] == 0, name
        plan = v.sfm_debug_plan(S["l"], S["track_start"], S["track_nobs"])      # the schedule the device works from
        tri = plan["step"] >= 0
        assert np.array_equal(tri, r["plan"]["step"] >= 0)
        qn = r["ba_q"] / np.sqrt((r["ba_q"] ** 2).sum(1))[:, None]
        e_R = np.abs(ref.qmats(qn) - truth["cam_R"]).max()
        e_t = np.abs(r["ba_t"] - truth["cam_t"]).max() / np.abs(truth["cam_t"]).max()
        e_X = np.abs(r["points_ba"][tri] - truth["points"][tri]).max() / np.abs(truth["points"][tri]).max()
        e_fR = np.abs(r["R"] @ S["ric"] - truth["img_R"]).max()
        e_fT = np.abs(r["Tf"] - truth["img_T"]).max() / np.abs(truth["img_T"]).max()
        print("%s: cameras R %.2g t %.2g, points %.2g, image frames R %.2g T %.2g (relative)" % (name, e_R, e_t, e_X, e_fR, e_fT))
        assert max(e_R, e_t, e_X, e_fR, e_fT) < 1e-6, name
        assert np.array_equal(np.sort(S["track_id"][r["tracked"]]), np.sort(S["track_id"][tri]))
        assert not r["points_ba"][~tri].any() and (~tri).sum() >= 5 and (plan["step"] == 5).sum() >= 3


def test_float64_and_extended_runs_take_the_same_decisions():
    """a condition on the inputs of the GPU tests: iterations, accepted steps and termination of every solve, the failure mask"""
    for name in si.CASES:
        r64, r80 = si.restated(name)
        assert r64["solves"] == r80["solves"], name
        assert (r64["ok"], r64["fail"]) == (r80["ok"], r80["fail"]), name
        assert np.array_equal(r64["pnp_iterations"], r80["pnp_iterations"]) and np.array_equal(r64["frame_iterations"], r80["frame_iterations"])
        print("%s: ok %d fail %d, BA %s, %d solves" % (name, r64["ok"], r64["fail"], (r64["iterations"], r64["successful_steps"], r64["termination"]),
                                                   len(r64["solves"])))
    # the restatement's codes are the header's
    assert (ref.FAIL_KEY_PNP, ref.FAIL_FRAME_PNP, ref.FAIL_BA, ref.FAIL_NUMERIC) == (v.capi.SFM_FAIL_KEY_PNP, v.capi.SFM_FAIL_FRAME_PNP,
                                                                                      v.capi.SFM_FAIL_BA, v.capi.SFM_FAIL_NUMERIC)
    assert si.restated("F11 l4 noisy, frame 5 starved")[0]["fail"] == ref.FAIL_KEY_PNP
    assert si.restated("F11 l4 noisy, frame 2 starved")[0]["fail"] == ref.FAIL_KEY_PNP
    assert si.restated("F14 l4 noisy, image frame 7 starved")[0]["fail"] == ref.FAIL_FRAME_PNP
    assert si.restated("F11 l4 noisy")[0]["iterations"] >= 3      # the noise makes the BA work
