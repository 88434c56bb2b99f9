"""k_chol assembles the dense part of the reduced camera system in the registers of its partner waves while the two
speed/bias chains are eliminated (ba_step.h, phase 1).  The windows of the benchmark shape and of the steady-state shape
(a prior of n = 75 dims, a tenth of the point tracks over all 11 frames) against the oracle: the same iteration pattern, poses
at the parity bar.  A window whose prior is scaled far beyond its data (an ill-conditioned system whose factorisation may fail
and is then retried by k_solve) must still follow the oracle."""
import ctypes as C

import numpy as np
import pytest

import oracle_api as o
import vplines_slam_amd as v
from test_gpu_solve import POS_TOL, ROT_TOL, make_windows, pose_err

pytestmark = pytest.mark.gpu


def _check(wg, wc, rep_g, opt):
    for i in range(len(wc)):
        _, rep_c = o.solve_window(wc[i], opt)
        assert rep_g[i].iterations == rep_c.iterations, i
        assert rep_g[i].num_successful_steps == rep_c.num_successful_steps, i
        dp, dr = pose_err(wg[i], wc[i])
        assert dp <= POS_TOL and dr <= ROT_TOL, (i, dp, dr)


def test_benchmark_shape_matches_the_oracle():
    ws, opt = make_windows(8, 200, 80, True, seed0=900)
    ctx = v.Context(device=0, max_windows=8, max_points=200, max_point_obs=1200, max_lines=80, max_line_obs=480)
    wa = [w.copy() for w in ws]
    pri, _ = ctx.solve_windows(wa, opt)
    # second solve of the same windows with the first one's priors: the prior of frame 0's speed/bias (the fast path)
    wg, wc = [], []
    for i, w in enumerate(ws):
        w = w.copy()
        w.prior = pri[i]
        wg.append(w.copy())
        wc.append(w.copy())
    _, rep_g = ctx.solve_windows(wg, opt)
    ctx.close()
    _check(wg, wc, rep_g, opt)


def _steady_pair(k):
    opt = v.default_options()
    cfg = v.workload.config(200, 80, True)
    t = 0.41 * k
    a = v.workload.graft_long_tracks(v.workload.seed_for(3, 6100 + k), cfg, t, 1)
    b = v.workload.graft_long_tracks(v.workload.seed_for(3, 6200 + k), cfg, t + cfg.kf_dt)   # every 10th track
    o.preintegrate_windows([a, b], opt)
    prior, _ = o.solve_window(a.copy(), opt)
    b.prior = prior
    return b, prior, cfg, opt


def test_steady_state_shape_matches_the_oracle():
    pairs = [_steady_pair(k) for k in range(3)]
    cfg, opt = pairs[0][2], pairs[0][3]
    assert all(p[1].n > 60 for p in pairs), [p[1].n for p in pairs]
    ctx = v.Context(device=0, max_windows=3, max_points=200, max_point_obs=v.workload.steady_point_obs(cfg), max_lines=80,
                    max_line_obs=80 * cfg.track_len)
    wg = [p[0].copy() for p in pairs]
    wc = [p[0].copy() for p in pairs]
    _, rep_g = ctx.solve_windows(wg, opt)
    ctx.close()
    _check(wg, wc, rep_g, opt)


@pytest.mark.parametrize("scale", [1e4, 1e7])
def test_huge_prior_follows_the_oracle(scale):
    b, prior, cfg, opt = _steady_pair(7)
    big = v.Prior()
    C.memmove(C.byref(big), C.byref(prior), C.sizeof(big))
    n = big.n
    np.ctypeslib.as_array(big.J0)[: n * n] *= scale
    np.ctypeslib.as_array(big.r0)[:n] *= scale
    b.prior = big
    wg, wc = [b.copy()], [b.copy()]
    ctx = v.Context(device=0, max_windows=1, max_points=200, max_point_obs=v.workload.steady_point_obs(cfg), max_lines=80,
                    max_line_obs=80 * cfg.track_len)
    _, rep_g = ctx.solve_windows(wg, opt)
    ctx.close()
    _check(wg, wc, rep_g, opt)
