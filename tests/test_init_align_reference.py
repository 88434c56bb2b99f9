"""The NumPy restatement of the visual-inertial alignment (tests/init_align_ref.py) held to ground truth, and the host-only pieces
of vpl_init_align_batch: the job list and the struct layouts.  No GPU.

Input: the trajectory of test_gpu_sequence.Measurements(11), rotated by a random Rw and scaled by 1 / 2.7 as an SfM would hand it
over, with exact pre-integration deltas computed from the true states -- so the alignment has an exact answer: scale 2.7, gravity
Rw G, delta_bg 0."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import vplines_slam_amd as v
import init_align_ref as ref
from init_align_inputs import KEY11, KEY14, SCALE, exact_pre, measurements, sfm_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G_NORM = v.default_options().g_norm
ZERO = np.zeros((11, 3))


def align(rw_seed, dt=np.float64, T_noise=0.0, flip_T=False, dv_scale=1.0):
    M = measurements(11, 77)
    Rw, R, T, tic = sfm_frames(M, 11, rw_seed)
    pre = exact_pre(M, 11, G_NORM)
    if T_noise:
        T = T + np.random.default_rng(rw_seed + 1).normal(0, T_noise, T.shape)
    if flip_T:
        T = -T
    for p in pre[1:]:
        p.delta_v = p.delta_v * dv_scale
    return Rw, ref.visual_initial_align(R, T, (pre, pre), KEY11, ZERO, ZERO, tic, G_NORM, dt)


@pytest.mark.parametrize("rw_seed", [77, 5])
def test_noise_free_alignment_recovers_scale_gravity_and_zero_bias(rw_seed):
    Rw, r = align(rw_seed)
    g_lin = np.linalg.norm(r["g_linear"])
    print("seed %d: s %.12f, |g_linear| %.10f, |delta_bg| %.3g" % (rw_seed, r["s"], g_lin, np.linalg.norm(r["delta_bg"])))
    assert r["ok"] and r["fail"] == 0
    assert abs(r["s"] - SCALE) < 1e-8 and abs(r["s_linear"] - SCALE) < 1e-8
    assert abs(g_lin - G_NORM) < 1e-8
    assert abs(np.linalg.norm(r["g_refined"]) - G_NORM) < 1e-8
    assert np.linalg.norm(r["delta_bg"]) < 1e-10
    if rw_seed == 77:
        assert np.abs(r["g_refined"] - Rw @ [0, 0, G_NORM]).max() < 1e-8
    # the state change: gravity along +z, frame 0 at the origin without yaw, the window at metric scale
    assert np.abs(r["g"] - [0, 0, G_NORM]).max() < 1e-7
    assert np.abs(r["pose"][0, :3]).max() == 0
    M = measurements(11, 77)
    d_true = np.linalg.norm(M.pose_true[10][:3] - M.pose_true[0][:3])
    assert abs(np.linalg.norm(r["pose"][10, :3]) - d_true) < 1e-7
    R0 = ref.qmat(np.roll(r["pose"][0, 3:], 1), np.float64)
    assert abs(ref.R2ypr(R0, np.float64)[0]) < 1e-9
    # with every frame a key frame Vs is the frames' own velocity: its norm is the true one
    for f in (0, 5, 10):
        assert abs(np.linalg.norm(r["speed_bias"][f, :3]) - np.linalg.norm(M.sb_true[f][:3])) < 1e-7


def test_extended_precision_run_agrees_with_the_float64_run():
    ref.require_extended()
    _, r64 = align(77)
    _, r80 = align(77, np.longdouble)
    d = np.abs(r64["x"] - r80["x"].astype(np.float64)).max()
    print("max |x64 - x80| = %.3g on |x|_inf = %.3g" % (d, np.abs(r64["x"]).max()))
    assert r80["ok"] and d < 1e-9 * np.abs(r64["x"]).max()


def test_noise_on_T_passes_both_checks_and_refines_the_scale():
    """1e-4 (SfM units) of noise on every camera position: a few parts in a thousand of the frame-to-frame motion"""
    for rw_seed in (77, 5):
        _, r = align(rw_seed, T_noise=1e-4)
        g_lin = np.linalg.norm(r["g_linear"])
        print("seed %d: first solve |g| %.4f s %.4f -> refined s %.4f" % (rw_seed, g_lin, r["s_linear"], r["s"]))
        assert r["ok"]
        assert abs(g_lin - G_NORM) < 0.5 and r["s_linear"] > 1.0      # both of the reference's checks, with room
        # the refinement recovers the scale to about a percent.  RefineGravity zeroes A and b once, before its four rounds, so the
        # first round's system outweighs the later ones by 1000 per round and the scale stays near what round 0 solved; a
        # restatement that zeroed them every round would move on from there (and from these figures)
        assert abs(r["s"] - SCALE) < 0.03
        assert abs(np.linalg.norm(r["g_refined"]) - G_NORM) < 1e-9     # the refinement keeps the norm it is given


def test_negated_T_fails_on_the_scale():
    _, r = align(77, flip_T=True)
    assert not r["ok"] and r["fail"] == ref.FAIL_SCALE
    assert abs(r["s_linear"] + SCALE) < 1e-8 and "s" not in r


def test_scaled_delta_v_fails_on_the_gravity_norm():
    _, r = align(77, dv_scale=1.5)
    off = abs(np.linalg.norm(r["g_linear"]) - G_NORM)
    print("|g| off by %.3f" % off)
    assert off > 2.0
    assert not r["ok"] and r["fail"] & ref.FAIL_GRAVITY


def test_job_list_matches_the_restatement():
    rng = np.random.default_rng(3)
    for F, key in ((11, KEY11), (14, KEY14)):
        ns = rng.integers(1, 21, F).astype(np.int32)
        ns[0] = 0
        got = v.capi.init_debug_jobs(ns, key)
        want = ref.build_jobs(ns, key)
        assert got.shape == (F + 9, 3) and np.array_equal(got, want), (F, got, want)
    # window interval 3 of the 14-frame list spans image intervals 3 and 4 and starts where interval 3 starts
    ns = np.arange(14, dtype=np.int32)
    got = v.capi.init_debug_jobs(ns, KEY14)
    assert tuple(got[13 + 2]) == (1 + 2, 3 + 4, 1 + 2 - 1)
    assert tuple(got[0]) == (0, 1, -1) and tuple(got[13]) == (0, 1, -1)


def test_job_list_refusals():
    ns = np.ones(14, dtype=np.int32)
    bad_key = list(KEY14)
    bad_key[4] = bad_key[3]
    assert v.capi.init_debug_jobs(ns, bad_key) == -1                       # not strictly increasing
    assert v.capi.init_debug_jobs(ns, KEY11) == -1                         # key[10] != F - 1
    assert v.capi.init_debug_jobs(ns, (1,) + KEY14[1:]) == -1              # key[0] != 0
    assert v.capi.init_debug_jobs(np.ones(10, dtype=np.int32), KEY11) == -1   # F < 11
    assert v.capi.init_debug_jobs(np.ones(41, dtype=np.int32), tuple(range(10)) + (40,)) == -4   # F > 40
    z = ns.copy()
    z[7] = 0
    assert v.capi.init_debug_jobs(z, KEY14) == -1                          # an interval without samples
    z = ns.copy()
    z[0] = 0
    assert not isinstance(v.capi.init_debug_jobs(z, KEY14), int)           # entry 0 is not read


def test_struct_layouts_match_the_header():
    # what the header implies (ints, doubles, pointers; natural alignment) ...
    assert C.sizeof(v.capi.CInitInput) == 8 + 4 * 8 + 2 * 24 + 2 * 8 + (44 + 4) + 2 * 264 + 24
    assert C.sizeof(v.capi.InitResult) == 8 + 8 * (3 + 3 + 1 + 1 + 3 + 3 + 40 * 3 + 11 * 7 + 11 * 9)
    assert v.capi.InitResult.g.offset + 8 * (3 + 120 + 77 + 99) == C.sizeof(v.capi.InitResult)   # g .. speed_bias contiguous
    # ... and what a C compiler makes of it
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vplines_ba.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d\\n", '
           'sizeof(vpl_init_input), sizeof(vpl_init_result), offsetof(vpl_init_input, key), offsetof(vpl_init_input, tic), '
           'offsetof(vpl_init_result, pose), VPL_INIT_MAX_FRAMES); return 0; }\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")], check=True)
        out = subprocess.run([os.path.join(d, "s")], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [C.sizeof(v.capi.CInitInput), C.sizeof(v.capi.InitResult), v.capi.CInitInput.key.offset,
                                     v.capi.CInitInput.tic.offset, v.capi.InitResult.pose.offset, v.capi.INIT_MAX_FRAMES]
