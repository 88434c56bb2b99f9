"""The trust-region step as one launch (k_step, ba_step.h) against the same three bodies as three launches (k_schur, k_chol,
k_back): VPL_BA_STEP_FUSED=1 (the default) / 0, read when the context is created.  The bodies, the order of every sum and the
window -> work-group mapping are the same, so the results have to be identical BIT FOR BIT: for narrow and wide rows, with the
general path (k_solve) inside the batch -- it runs after k_step, and between k_chol and k_back in the three-launch form --, for
a window whose factorisation can fail and is retried, and for the timed solve, which always takes the three-launch form."""
import ctypes as C

import numpy as np
import pytest

import oracle_api as o
import vplines_slam_amd as v
from test_gpu_solve import POS_TOL, ROT_TOL, _relayout_points, make_windows, pose_err

pytestmark = pytest.mark.gpu

STEP_KERNELS = ["k_schur", "k_chol", "k_solve", "k_back"]


def _context(monkeypatch, fused, env=None, **caps):
    """a context created under VPL_BA_STEP_FUSED=fused (and the other switches in env); the environment is restored"""
    env = dict(env or {}, VPL_BA_STEP_FUSED=fused)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    try:
        return v.Context(device=0, **caps)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _copy_prior(p):
    q = v.Prior()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(q))
    return q


def _bits(windows, pri, rep):
    """everything a solve hands back that the step decides"""
    return dict(states=v.shard.pack_states(windows),
                invd=[np.array(w.inv_depth) for w in windows], plk=[np.array(w.line_plk) for w in windows],
                cost=[r.final_cost for r in rep], iters=[r.iterations for r in rep], steps=[r.num_successful_steps for r in rep],
                J=[p.J().copy() for p in pri], r=[p.r().copy() for p in pri])


def _assert_same_bits(a, b):
    assert np.array_equal(a["states"], b["states"])
    assert a["cost"] == b["cost"] and a["iters"] == b["iters"] and a["steps"] == b["steps"]
    for key in ("invd", "plk", "J", "r"):
        assert len(a[key]) == len(b[key])
        for x, y in zip(a[key], b[key]):
            assert np.array_equal(x, y), key


def _solve(ctx, ws, opt, priors=None):
    wa = [w.copy() for w in ws]
    if priors is not None:
        for w, p in zip(wa, priors):
            w.prior = p
    pri, rep = ctx.solve_windows(wa, opt)
    return wa, pri, rep


@pytest.fixture(scope="module")
def small_windows():
    return make_windows(4, 60, 20, True)


def _solve_twice(ctx, ws, opt):
    """the windows, then the same windows with the priors of the first solve: only then do k_chol's chains see a prior"""
    wa, pri, rep = _solve(ctx, ws, opt)
    keep = [_copy_prior(p) for p in pri]
    wb, pri2, rep2 = _solve(ctx, ws, opt, keep)
    return _bits(wa, pri, rep), _bits(wb, pri2, rep2)


def test_narrow_rows_same_bits(monkeypatch, small_windows):
    ws, opt = small_windows
    out = []
    for fused in ("0", "1"):
        ctx = _context(monkeypatch, fused, max_windows=4, max_points=60, max_point_obs=360, max_lines=20, max_line_obs=120)
        out.append(_solve_twice(ctx, ws, opt))
        ctx.close()
    _assert_same_bits(out[0][0], out[1][0])
    _assert_same_bits(out[0][1], out[1][1])
    assert all(p.shape[0] > 0 for p in out[1][1]["J"])


def test_capacity_beyond_the_compact_system_same_bits(monkeypatch, small_windows):
    """The same windows on a context of 60 points and 214 lines: 4 maxP + 28 maxL = 6 232 doubles of landmark constants are
    more than the 5 952 of the compact system that takes their place in k_schur's LDS (ba_step_layout.h: region r1), so every
    region behind it starts where kP | kL end, not where Cacc ends.  The two forms give the same bits, and the result is the
    oracle's within the bars of test_window_solve_parity_no_prior.  (Not compared with the small context: k_lin's tables depend
    on the capacity.)  Lines, not points, carry the capacity over that side: k_lin keeps 14 doubles per point of capacity in
    LDS (lin_smem_base), so vpl_ctx_create refuses 1000 points beside 80 lines, and with 80 lines every capacity it accepts
    (at most 508 points) stays below the compact system; 214 lines leave k_lin room for a prior of 47 dims."""
    ws, opt = small_windows
    caps = dict(max_windows=4, max_points=60, max_point_obs=360, max_lines=214, max_line_obs=120)
    assert 4 * 60 + 28 * 214 > 74 * 80 + 32
    out, solved = [], None
    for fused in ("0", "1"):
        ctx = _context(monkeypatch, fused, **caps)
        out.append(_solve_twice(ctx, ws, opt))
        if fused == "1":
            solved = _solve(ctx, ws, opt)
        ctx.close()
    _assert_same_bits(out[0][0], out[1][0])
    _assert_same_bits(out[0][1], out[1][1])
    wg, _, rep_g = solved
    _assert_same_bits(out[1][0], _bits(*solved))
    for i, w in enumerate(ws):
        wc = w.copy()
        _, rep_c = o.solve_window(wc, opt)
        assert rep_g[i].iterations == rep_c.iterations and rep_g[i].num_successful_steps == rep_c.num_successful_steps, i
        assert abs(rep_g[i].initial_cost - rep_c.initial_cost) <= 1e-9 * rep_c.initial_cost
        assert abs(rep_g[i].final_cost - rep_c.final_cost) <= 5e-5 * max(1.0, rep_c.final_cost)
        dp, dr = pose_err(wg[i], wc)
        assert dp <= POS_TOL and dr <= ROT_TOL, (i, dp, dr)
        assert np.abs(wg[i].speed_bias - wc.speed_bias).max() < 1e-4
        assert np.abs(wg[i].inv_depth - wc.inv_depth).max() < 1e-5


@pytest.fixture(scope="module")
def long_track_windows():
    """three windows of 100 points + 12 lines with tracks of up to 11 frames: the ragged layouts of
    test_skewed_ragged_windows_marginalisation_pass_terminates (rows wider than the 6-frame view, most tracks short)"""
    import test_point_units as tpu
    rng = np.random.default_rng(11)
    layouts = []
    for trial in range(1500):
        start, nobs = tpu._random_window(rng, 100, 0.6)
        lt, st, R, R0 = tpu._tables(start, nobs)
        if R > R0 >= 1 and not tpu._replay(st, R0, 0):
            layouts.append((start, nobs))
        if len(layouts) == 3:
            break
    assert len(layouts) == 3
    opt = v.default_options()
    cfg = v.workload.config(100, 12, True)
    cfg.track_len = 11
    base = [v.workload.generate(v.workload.seed_for(3, 6100 + i), cfg, 0.37 * i) for i in range(3)]
    o.preintegrate_windows(base, opt)
    return [_relayout_points(b, s, n) for b, (s, n) in zip(base, layouts)], opt


@pytest.mark.parametrize("wide", ["", "1"], ids=["mixed", "all_tiles"])
def test_wide_rows_same_bits(monkeypatch, long_track_windows, wide):
    """rows of more than 6 frames: k_step<3, true> (narrow view + wide chunks); VPL_BA_SCHUR_WIDE=1: k_step<5, false>"""
    ws, opt = long_track_windows
    env = {"VPL_BA_SCHUR_WIDE": wide} if wide else None
    out = []
    for fused in ("0", "1"):
        ctx = _context(monkeypatch, fused, env, max_windows=3, max_points=100, max_point_obs=1100, max_lines=12, max_line_obs=132)
        out.append(_solve_twice(ctx, ws, opt))
        ctx.close()
    _assert_same_bits(out[0][0], out[1][0])
    _assert_same_bits(out[0][1], out[1][1])


def _speed_bias_3_prior(w, rng):
    """a prior that ties speed/bias 3: outside k_chol's elimination order, routed to k_solve at upload (the construction of
    test_prior_with_speed_bias_of_a_later_frame_takes_the_general_path)"""
    p = v.Prior()
    kinds, frames = [0, 1, 2], [2, 3, 0]                 # pose 2, speed/bias 3, extrinsic
    n = 6 + 9 + 6
    p.n, p.n_blocks = n, 3
    idx = 0
    for b, (k, f) in enumerate(zip(kinds, frames)):
        p.block_kind[b], p.block_frame[b], p.block_idx[b] = k, f, idx
        x0 = (w.pose[f] if k == 0 else w.speed_bias[f] if k == 1 else w.ex_pose)
        for j in range(len(x0)):
            p.x0[b][j] = float(x0[j])
        idx += 9 if k == 1 else 6
    J = np.triu(rng.normal(size=(n, n))) * 3.0 + 5.0 * np.eye(n)
    r = rng.normal(size=n) * 0.1
    flat = np.zeros(171 * 171)
    flat[: n * n] = J.reshape(-1)
    for j in range(n * n):
        p.J0[j] = float(flat[j])
    for j in range(n):
        p.r0[j] = float(r[j])
    return p


def test_general_path_inside_a_fused_batch(monkeypatch):
    """two ordinary windows and two of the general path in one batch: k_solve runs after k_step and must find what the
    three-launch form gives it between k_chol and k_back"""
    ws, opt = make_windows(4, 60, 20, True, seed0=90)
    rng = np.random.default_rng(3)
    priors = [None, _speed_bias_3_prior(ws[1], rng), None, _speed_bias_3_prior(ws[3], rng)]
    out = []
    for fused in ("0", "1"):
        ctx = _context(monkeypatch, fused, max_windows=4, max_points=60, max_point_obs=360, max_lines=20, max_line_obs=120)
        wa = [w.copy() for w in ws]
        for w, p in zip(wa, priors):
            if p is not None:
                w.prior = p
        pri, rep = ctx.solve_windows(wa, opt)
        out.append(_bits(wa, pri, rep))
        ctx.close()
    _assert_same_bits(out[0], out[1])
    for i, (w, p) in enumerate(zip(ws, priors)):
        c = w.copy()
        if p is not None:
            c.prior = p
        _, rep_c = o.solve_window(c, opt)
        assert out[1]["iters"][i] == rep_c.iterations and out[1]["steps"][i] == rep_c.num_successful_steps, i


@pytest.fixture(scope="module")
def ill_conditioned():
    from test_gpu_chol_assembly import _steady_pair
    return _steady_pair(7)


@pytest.mark.parametrize("scale", [1e4, 1e7])
def test_retry_path_same_bits_and_leaves_no_flag(monkeypatch, ill_conditioned, scale):
    """A prior scaled far beyond its data (test_gpu_chol_assembly.py): the factorisation in k_chol may fail, the window is
    flagged for this iteration and k_solve retries with a larger mu.  The flag comes down in k_solve (fused) or in k_back:
    an ordinary solve on the same context afterwards equals a fresh context's."""
    b, prior, cfg, opt = ill_conditioned
    big = _copy_prior(prior)
    n = big.n
    np.ctypeslib.as_array(big.J0)[: n * n] *= scale
    np.ctypeslib.as_array(big.r0)[:n] *= scale
    caps = dict(max_windows=1, max_points=200, max_point_obs=v.workload.steady_point_obs(cfg), max_lines=80,
                max_line_obs=80 * cfg.track_len)
    hard, after = [], []
    for fused in ("0", "1"):
        ctx = _context(monkeypatch, fused, **caps)
        hard.append(_bits(*_solve(ctx, [b], opt, [big])))
        after.append(_bits(*_solve(ctx, [b], opt, [prior])))
        ctx.close()
    _assert_same_bits(hard[0], hard[1])
    _assert_same_bits(after[0], after[1])
    fresh = _context(monkeypatch, "1", **caps)
    ref = _bits(*_solve(fresh, [b], opt, [prior]))
    fresh.close()
    _assert_same_bits(after[1], ref)


def test_timed_solve_is_the_same_computation_in_three_launches(monkeypatch, small_windows):
    """kernel timing attributes time and active windows per phase: the timed solve issues k_schur, k_chol, k_solve, k_back
    whatever the switch says, and gives the bits of the untimed fused solve"""
    ws, opt = small_windows
    caps = dict(max_windows=4, max_points=60, max_point_obs=360, max_lines=20, max_line_obs=120)
    ctx = _context(monkeypatch, "1", **caps)
    plain = _bits(*_solve(ctx, ws, opt))
    ctx.close()
    ctx = _context(monkeypatch, "1", **caps)
    ctx.enable_kernel_timing(True)
    timed = _bits(*_solve(ctx, ws, opt))
    prof = ctx.launch_profile()
    ctx.enable_kernel_timing(False)
    again = _bits(*_solve(ctx, ws, opt))          # and back to the one launch on the same context
    ctx.close()
    _assert_same_bits(plain, timed)
    _assert_same_bits(plain, again)
    names = [p[0] for p in prof]
    assert "k_step" not in names
    step = [n for n in names if n in STEP_KERNELS]
    assert step == STEP_KERNELS * opt.num_iterations, names
    first = names.index("k_schur")
    assert names[first:first + 4] == STEP_KERNELS
    # the first step: every window computes a new Gauss-Newton step in k_schur, k_chol and k_back, none in k_solve
    acts = [p[2] for p in prof[first:first + 4]]
    assert [a[1] for a in acts] == [len(ws), len(ws), 0, len(ws)], acts
