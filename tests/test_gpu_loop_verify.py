"""vpl_loop_verify_batch on the device against the sequential restatement tests/lc_ref.py:verify over the same sample stream.

Decisions and integers are equal: status, has_loop, the stage, the RANSAC iterations, the best inlier count, the iterations and
termination of the final solve.  Poses and loop_info are held to the project's bar (initial structure):
max(32 max |x64 - x80|, 1e-12 |x|_inf) over the solution vector (PnP_T_old, PnP_R_old, loop_info), x64 / x80 the restatement's float64
and np.longdouble runs on the same input.  The inputs keep every inlier within 1e-3 of its projection and every outlier at least 0.1
away (threshold 10 / 460), and tests/test_loop_reference.py holds the two runs to the same masks and counts on every case."""
import numpy as np
import pytest

import vplines_slam_amd as v

import lc_inputs
import lc_ref

pytestmark = pytest.mark.gpu

K_BAR = 32
NAMES = list(lc_inputs.LOOP_CASES)


def loop_input(name):
    S, seed = lc_inputs.loop_case(name)
    return v.LoopInput(S["pts3d"], S["old_norm"], S["origin_vio_T"], S["origin_vio_R"], lc_inputs.TIC, lc_inputs.QIC, seed)


def solution(r):
    return np.concatenate([np.asarray(r["PnP_T_old"], np.longdouble).ravel(), np.asarray(r["PnP_R_old"], np.longdouble).ravel(),
                           np.asarray(r["loop_info"], np.longdouble).ravel()])


def check(name, res, status):
    r64, r80 = lc_inputs.ref_loop_case(name)
    got = dict(PnP_T_old=np.array(res.PnP_T_old[:]), PnP_R_old=np.array(res.PnP_R_old[:]), loop_info=np.array(res.loop_info[:]))
    ints = ("has_loop", "stage", "ransac_iterations", "best_inliers", "lm_iterations", "lm_termination")
    print(name, {k: getattr(res, k) for k in ints}, "reference", {k: r64[k] for k in ints})
    for k in ints:
        assert getattr(res, k) == r64[k], (name, k, getattr(res, k), r64[k])
    assert status.dtype == np.uint8 and np.array_equal(status, r64["status"]), name
    assert r64["stage"] == lc_inputs.LOOP_CASES[name]["stage"]
    x64, x80, x = solution(r64), solution(r80), solution(got)
    d = float(np.abs(x64 - x80).max())
    bar = max(K_BAR * d, 1e-12 * float(np.abs(x64).max()))
    err = float(np.abs(x - x64).max())
    print("   error %.3g, bar %.3g (|x64 - x80| %.3g)" % (err, bar, d))
    assert err <= bar, (name, err, bar, d)


@pytest.mark.parametrize("name", NAMES)
def test_loop_verify_matches_the_sequential_restatement(gpu_ctx, name):
    res, status = gpu_ctx.loop_verify([loop_input(name)])
    check(name, res[0], status[0])
    S, _ = lc_inputs.loop_case(name)
    if lc_inputs.LOOP_CASES[name]["stage"] >= lc_ref.FEW_INLIERS:      # solved: the inliers are the true ones and are kept
        assert np.array_equal(status[0].astype(bool), ~S["outlier"])
        assert np.abs(np.array(res[0].PnP_T_old[:]) - S["old_T"]).max() < 0.02
    else:
        assert not status[0].any() and res[0].has_loop == 0


def test_loop_verify_batch_follows_the_items_and_repeats_bit_for_bit(gpu_ctx):
    for order in (NAMES, NAMES[::-1][2:] + NAMES[-2:]):
        inputs = [loop_input(n) for n in order]
        res, status = gpu_ctx.loop_verify(inputs)
        again, status2 = gpu_ctx.loop_verify(inputs)
        for i, n in enumerate(order):
            check(n, res[i], status[i])
            assert bytes(res[i]) == bytes(again[i]) and np.array_equal(status[i], status2[i]), n


def test_loop_verify_refusals(gpu_ctx):
    q = loop_input(NAMES[0])
    o = v.default_loop_options()
    assert (o.min_loop_num, o.max_iters, o.reproj_error, o.confidence, o.max_yaw_deg, o.max_t) == (25, 100, 10.0 / 460.0, 0.99, 30.0, 20.0)
    o.max_iters = 0
    assert gpu_ctx.loop_verify([q], o, check=False) == -1
    big = v.LoopInput(np.zeros((v.capi.LOOP_MAX_POINTS + 1, 3)), np.zeros((v.capi.LOOP_MAX_POINTS + 1, 2)), np.zeros(3), np.eye(3),
                      np.zeros(3), np.eye(3))
    assert gpu_ctx.loop_verify([big], check=False) == -4
    res, status = gpu_ctx.loop_verify([v.LoopInput(np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(3), np.eye(3), np.zeros(3), np.eye(3))])
    assert res[0].stage == lc_ref.FEW_POINTS and res[0].has_loop == 0 and len(status[0]) == 0
