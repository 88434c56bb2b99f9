"""The relative pose without a GPU: the sample stream and the stopping table (vpl_relpose_debug_plan) against the NumPy
restatement (tests/relpose_ref.py), the plain-C++ header that makes them under the sanitizers, and the restatement itself held to
ground truth and to its own extended-precision run on every input the GPU tests use (tests/relpose_inputs.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

import vplines_slam_amd as v
import relpose_ref as ref
import relpose_inputs as ri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = [name for name, sc in ri.SCENES.items() if not sc.get("noisy")]


def test_debug_plan_samples_are_seven_distinct_indices_below_n():
    for N in (21, 22, 64, 65, 1024):
        for seed, i in ((0, 0), (1, 0), (1, 9), (2 ** 64 - 1, 4), (123456789012345, 7)):
            s = v.relpose_debug_plan(seed, i, N)["samples"]
            assert s.shape == (1000, 7) and s.min() >= 0 and s.max() < N, (N, seed, i)
            srt = np.sort(s, axis=1)
            assert (srt[:, 1:] != srt[:, :-1]).all(), (N, seed, i)
    # a stream is a function of (seed, candidate, iteration, N) alone: the same again, another with any of them changed
    a = v.relpose_debug_plan(7, 3, 65)["samples"]
    assert np.array_equal(a, v.relpose_debug_plan(7, 3, 65)["samples"])
    for other in (v.relpose_debug_plan(8, 3, 65), v.relpose_debug_plan(7, 4, 65)):
        assert (other["samples"] != a).any(1).mean() > 0.9
    # every index is drawn: 7000 draws over 65
    assert len(np.unique(a)) == 65


def test_debug_plan_table_is_the_opencv_formula():
    """niters_after[good] = RANSACUpdateNumIters(0.99, (N - good) / N, 7, 1000) as the restatement evaluates it, every good"""
    for N in (21, 22, 64, 65, 1024):
        got, want = v.relpose_debug_plan(0, 0, N)["niters_after"], ref.niters_table(N)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (N, [(int(g), int(got[g]), int(want[g])) for g in bad])
        assert got[0] == 1000 and got[N] == 0 and (np.diff(got) <= 0).all()
    # the stop after a hypothesis that fits 80 % / 50 % of the correspondences
    assert ref.niters_after(100, 80) == 20 and ref.niters_after(60, 30) == 587


def test_debug_plan_refusals():
    assert v.relpose_debug_plan(0, -1, 30) == -1
    assert v.relpose_debug_plan(0, 10, 30) == -1
    assert v.relpose_debug_plan(0, 0, 6) == -1
    assert v.relpose_debug_plan(0, 0, v.capi.SFM_MAX_TRACKS + 1) == -4
    assert isinstance(v.relpose_debug_plan(0, 9, 7), dict)


def test_struct_layouts():
    # what the header implies (ints, doubles, pointers; natural alignment)
    assert C.sizeof(v.capi.CRelPoseInput) == 8 + 3 * 8 + 8
    assert C.sizeof(v.capi.RelPoseCandidate) == 4 * 10 + 8 * (1 + 9 + 9 + 3)
    assert C.sizeof(v.capi.RelPoseResult) == 4 * 4 + 8 * 12 + 10 * C.sizeof(v.capi.RelPoseCandidate)
    assert (ref.FEW_CORRES, ref.LOW_PARALLAX, ref.NO_MODEL, ref.FEW_GOOD, ref.SUCCESS) == (
        v.capi.RELPOSE_FEW_CORRES, v.capi.RELPOSE_LOW_PARALLAX, v.capi.RELPOSE_NO_MODEL, v.capi.RELPOSE_FEW_GOOD, v.capi.RELPOSE_SUCCESS)
    assert (ref.FAIL_NONE, ref.FAIL_NUMERIC, ref.MAX_ITERS) == (v.capi.RELPOSE_FAIL_NONE, v.capi.RELPOSE_FAIL_NUMERIC, v.capi.RELPOSE_MAX_ITERS)


def test_plan_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "relpose_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "vplines-slam_amd", "csrc"), os.path.join(ROOT, "tests", "native", "relpose_plan_check.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "relpose plan ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_cubic_branches():
    """three roots, one root, the vanishing leading coefficient down to the linear equation, the repeated root"""
    for dt in (np.float64, np.longdouble):
        c = lambda *a: ref.cubic(*[dt(x) for x in a])
        assert np.allclose(np.array(c(1, -6, 11, -6), dtype=float), [1, 2, 3], atol=1e-13)
        assert np.allclose(np.array(c(2, 0, 2, 0), dtype=float), [0], atol=1e-13)              # x (x^2 + 1)
        assert np.allclose(np.array(c(0, 1, -3, 2), dtype=float), [1, 2], atol=1e-13)
        assert np.allclose(np.array(c(0, 0, 2, -3), dtype=float), [1.5]) and c(0, 0, 0, 1) == [] and c(0, 1, 0, 1) == []
        assert np.allclose(np.array(c(0, 1, -2, 1), dtype=float), [1])
        assert np.allclose(np.array(c(1, -4, 5, -2), dtype=float), [2], atol=1e-12)            # (x - 1)^2 (x - 2): the simple root
        assert np.allclose(np.array(c(1, -3, 3, -1), dtype=float), [1], atol=1e-12)            # (x - 1)^3


def _angles(R, T, Rt, Tt):
    """(rotation angle of R^T Rt, angle between T and Tt) in radians, both from sines: no arccos next to 1"""
    E = (R.T @ Rt).astype(np.longdouble)
    w = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]) / 2
    t = T.astype(np.longdouble) / np.sqrt((T.astype(np.longdouble) ** 2).sum())
    assert (E.trace() - 1) / 2 > 0.9 and t @ Tt > 0.9          # (small angles: the sines stand for them)
    return float(np.sqrt((w * w).sum())), float(np.sqrt((np.cross(t, Tt.astype(np.longdouble)) ** 2).sum()))


def test_restatement_recovers_the_truth_from_exact_observations():
    """The restatement alone against ground truth: l is the first frame that passes both gates and keeps more than 12 points in
    front by construction; the final mask of every candidate that ran is the true inlier set; rotation and translation direction of
    every successful candidate lie within ten times the worst error of the extended-precision run over these inputs (what is left
    on exact data is the rounding of the points to float: 6e-8 relative of a coordinate, divided by the parallax)."""
    worst, rows = [0.0, 0.0], []
    for name in EXACT:
        S, truth = ri.scene(name)
        r64, r80 = ri.restated(name)
        for r in (r64, r80):
            assert r["l"] == truth["l"] and r["ok"] == (truth["l"] >= 0), name
            for i in range(10):
                assert r["n_corres"][i] == len(truth["tracks"][i])
                if r["status"][i] >= ref.FEW_GOOD:
                    assert np.array_equal(r["mask_pose"][i], truth["inlier"][i]), (name, i)
                    assert r["good"][i] == truth["inlier"][i].sum()
        for i in np.nonzero(r80["status"] == ref.SUCCESS)[0]:
            e80 = _angles(r80["R"][i], r80["T"][i], truth["R"][i], truth["T"][i])
            e64 = _angles(r64["R"][i], r64["T"][i], truth["R"][i], truth["T"][i])
            worst = [max(worst[0], e80[0]), max(worst[1], e80[1])]
            rows.append((name, i, e64, e80))
    print("worst of the extended-precision run against the truth: rotation %.3g rad, translation direction %.3g rad" % tuple(worst))
    for name, i, e64, e80 in rows:
        assert e64[0] <= 10 * worst[0] and e64[1] <= 10 * worst[1], (name, i, e64, worst)
    assert worst[0] < 1e-5 and worst[1] < 1e-3        # (float rounding over the smallest parallax met, not a wrong model)
    assert len(rows) >= 30


def test_float64_and_extended_runs_take_the_same_decisions():
    """a condition on the inputs of the GPU tests: l, every status, the loop's end, the winner, both masks; the counts of at least
    99 % of the hypotheses (the others are the leave-out mask of the GPU test); every real-valued gate 1e-6 relative from its
    threshold (the two integer gates compare integers the two runs agree on: n_corres = 20 is a case, not a near miss)"""
    choices = set()
    for name in ri.SCENES:
        r64, r80 = ri.restated(name)
        assert (r64["ok"], r64["fail"], r64["l"]) == (r80["ok"], r80["fail"], r80["l"]), name
        for k in ("n_corres", "status", "iterations", "best_iteration", "best_root", "inliers", "good", "choice"):
            assert np.array_equal(r64[k], r80[k]), (name, k, r64[k], r80[k])
        for i in range(10):
            assert np.array_equal(r64["mask_ransac"][i], r80["mask_ransac"][i]) and np.array_equal(r64["mask_pose"][i], r80["mask_pose"][i]), (name, i)
            if r64["n_corres"][i] > 20:
                p = float(r64["average_parallax"][i]) * 460
                assert abs(p - 30) >= 1e-6 * 30, (name, i, p)
            if r64["status"][i] >= ref.FEW_GOOD:
                choices.add(int(r64["choice"][i]))
        ev = (r64["hyp"] >= 0) | (r80["hyp"] >= 0)
        differ = r64["hyp"] != r80["hyp"]
        print("%s: l %d, statuses %s, %d hypotheses, %d differ" % (name, r64["l"], r64["status"], ev.sum(), differ.sum()))
        assert differ.sum() <= 0.01 * ev.sum(), (name, differ.sum(), ev.sum())
    assert choices == {0, 1, 2, 3}       # each of recoverPose's four poses wins the vote somewhere
    # the shapes the scenes are there for
    r = ri.restated("counts 15 20 21 65")[0]
    assert list(r["n_corres"][:4]) == [15, 20, 21, 65] and list(r["status"][:4]) == [ref.FEW_CORRES, ref.FEW_CORRES, ref.SUCCESS, ref.SUCCESS] and r["l"] == 2
    assert (ri.restated("1024 tracks")[0]["n_corres"] == 1024).all()
    r = ri.restated("frame 0 without parallax")[0]
    assert r["status"][0] == ref.LOW_PARALLAX and r["n_corres"][0] > 20 and r["l"] == 1
    assert ri.restated("l = 9")[0]["l"] == 9
    r = ri.restated("nothing succeeds")[0]
    assert (r["ok"], r["fail"], r["l"]) == (0, ref.FAIL_NONE, -1) and set(r["status"]) == {ref.FEW_CORRES, ref.LOW_PARALLAX, ref.FEW_GOOD}
    r = ri.restated("100 tracks, 20 % outliers")[0]
    assert 0 < r["iterations"].max() < 256
    r = ri.restated("60 tracks, 50 % outliers")[0]
    assert r["iterations"].max() > 256 and (r["hyp"][:, 256:] >= 0).any()      # the loop crosses a round of 256
