"""The loop verification without a GPU: the five-point sample stream and the stopping table (csrc/loop_plan.h) under the
sanitizers and against values computed here, vpl_loop_debug_plan against the same, and the conditions on the inputs of
tests/test_gpu_loop_verify.py: the restatement's float64 and extended-precision runs take the same decisions on every case."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vplines_slam_amd as v
import lc_inputs
import lc_ref
import sfm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("loop_plan") / "loop_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "vplines-slam_amd", "csrc"), os.path.join(ROOT, "tests", "native", "loop_plan_check.cpp"),
                           "-o", exe])
    return exe


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_plan_header_under_the_sanitizers(plan_check):
    assert "loop plan ok" in run(plan_check)


@pytest.mark.parametrize("seed, N", [(0, 5), (101, 26), (2 ** 64 - 1, 60), (123456789012345, 1024)])
def test_plan_header_gives_the_values_computed_here(plan_check, seed, N):
    lines = run(plan_check, seed, N, 0.99, 100).splitlines()
    samples = np.array([[int(x) for x in l.split()[1:]] for l in lines if l.startswith("s ")])
    table = np.array([int(x) for x in [l for l in lines if l.startswith("t")][0].split()[1:]])
    want_s = np.array([lc_ref.sample5(seed, it, N) for it in range(100)])
    want_t = np.array([lc_ref.niters_after(N, g) for g in range(N + 1)])
    assert samples.shape == (100, 5) and np.array_equal(samples, want_s)
    assert np.array_equal(table, want_t)
    # five distinct indices in range; the table monotone, 100 at zero inliers, 0 at N
    srt = np.sort(samples, axis=1)
    assert samples.min() >= 0 and samples.max() < N and (srt[:, 1:] != srt[:, :-1]).all()
    assert table[0] == 100 and table[N] == 0 and (np.diff(table) <= 0).all()
    # the library hands out the same
    p = v.loop_debug_plan(seed, N)
    assert np.array_equal(p["samples"], want_s) and np.array_equal(p["niters_after"], want_t)


def test_debug_plan_refusals_and_the_formula():
    assert v.loop_debug_plan(0, 4) == -1 and v.loop_debug_plan(0, 30, max_iters=0) == -1 and v.loop_debug_plan(0, 30, max_iters=1001) == -1
    assert v.loop_debug_plan(0, v.capi.LOOP_MAX_POINTS + 1) == -4
    # the stop after a model that fits 70 % of 60 points: log(0.01) / log(1 - 0.7^5) = 25.03
    assert lc_ref.niters_after(60, 42) == 25 and lc_ref.niters_after(40, 40) == 0 and lc_ref.niters_after(40, 0) == 100
    assert C.sizeof(v.capi.LoopResult) == 6 * 4 + 8 * 20 and C.sizeof(v.capi.LoopOptions) == 8 + 4 * 8
    assert C.sizeof(v.capi.CLoopInput) == 8 + 2 * 8 + 8 * 24 + 8
    assert (lc_ref.FEW_POINTS, lc_ref.NO_MODEL, lc_ref.NUMERIC, lc_ref.FEW_INLIERS, lc_ref.REJECTED, lc_ref.CLOSED) == (
        v.capi.LOOP_FEW_POINTS, v.capi.LOOP_NO_MODEL, v.capi.LOOP_NUMERIC, v.capi.LOOP_FEW_INLIERS, v.capi.LOOP_REJECTED, v.capi.LOOP_CLOSED)


def test_inputs_keep_their_margins():
    """inliers at most 1e-3 from the true projection (before the rounding to float), outliers at least 0.1"""
    for name in lc_inputs.LOOP_CASES:
        S, _ = lc_inputs.loop_case(name)
        Ro, To = S["old_R"] @ lc_inputs.QIC, S["old_T"] + S["old_R"] @ lc_inputs.TIC
        po = (S["pts3d"].astype(np.float64) - To) @ Ro
        e = np.sqrt(((po[:, :2] / po[:, 2:3] - S["old_norm"]) ** 2).sum(1))
        assert (po[:, 2] > 1).all() and e[~S["outlier"]].max() <= 1e-3 + 1e-6, (name, e[~S["outlier"]].max())
        if S["outlier"].any():
            assert e[S["outlier"]].min() >= 0.1 - 1e-6, (name, e[S["outlier"]].min())


def test_float64_and_extended_runs_take_the_same_decisions():
    sfm_ref.require_extended()
    stages = set()
    for name, c in lc_inputs.LOOP_CASES.items():
        r64, r80 = lc_inputs.ref_loop_case(name)
        S, _ = lc_inputs.loop_case(name)
        for k in ("has_loop", "stage", "ransac_iterations", "best_inliers", "lm_iterations", "lm_termination"):
            assert r64[k] == r80[k], (name, k, r64[k], r80[k])
        assert np.array_equal(r64["status"], r80["status"]), name
        assert r64["stage"] == c["stage"], (name, r64["stage"])
        stages.add(r64["stage"])
        if r64["stage"] >= lc_ref.FEW_INLIERS:      # solved: the true inliers, the old keyframe's pose within the noise
            assert np.array_equal(r64["status"].astype(bool), ~S["outlier"]), name
            assert np.abs(r64["PnP_T_old"] - S["old_T"]).max() < 0.02 and np.abs(r64["PnP_R_old"] - S["old_R"]).max() < 2e-3, name
        else:
            assert not r64["status"].any()
        print(name, "stage", r64["stage"], "iterations", r64["ransac_iterations"], "inliers", r64["best_inliers"],
              "yaw %.3f |t| %.3f" % (float(r64["loop_info"][7]), float(np.sqrt((r64["loop_info"][:3] ** 2).sum()))))
    assert stages == {lc_ref.FEW_POINTS, lc_ref.FEW_INLIERS, lc_ref.REJECTED, lc_ref.CLOSED}
    # the shapes the cases are there for
    r = lc_inputs.ref_loop_case("60 points, 30 % outliers")[0]
    assert r["best_inliers"] == 42 and 1 < r["ransac_iterations"] < 100
    r = lc_inputs.ref_loop_case("40 points, 25 inliers")[0]
    assert r["best_inliers"] == 25 and r["has_loop"] == 0 and r["PnP_R_old"].any()
    r = lc_inputs.ref_loop_case("relative yaw 35 degrees")[0]
    assert abs(abs(float(r["loop_info"][7])) - 35) < 0.1 and r["best_inliers"] == 40
    r = lc_inputs.ref_loop_case("relative translation 25 m")[0]
    assert abs(float(np.sqrt((r["loop_info"][:3] ** 2).sum())) - 25) < 0.1 and abs(float(r["loop_info"][7])) < 30
    assert lc_inputs.ref_loop_case("25 points")[0]["ransac_iterations"] == 0
