"""VPL_PRIOR_EIGEN (vpl_ba_set_prior_rule, k_prior_eigen in csrc/ba_prior_eig.h): the kept block of the marginalisation
turned into the next prior by the reference's rule (marginalization_factor.cpp:349-357) -- eigenvalues above 1e-8 kept,
J0 = sqrt(S) V^T, r0 = S^-1/2 V^T b -- instead of the default pivoted Cholesky factor.

Checked here: the factor against numpy's eigh of the device's own kept block (benchmark windows, n = 45, and the steady
state, n = 75); the 32-window chain of tests/test_gpu_chain.py with the device carrying its own eigen-rule prior; the random
shapes of tests/test_gpu_fuzz.py behind their own priors under both rules; determinism (two solves, half a batch alone, graph
replay against kernel-by-kernel launches); switching the rule on one context; a NaN window; the guard pads."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_api as o
import vplines_slam_amd as v
from vplines_slam_amd.capi import Prior
from test_gpu_solve import POS_TOL, ROT_TOL, pose_err

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EPS = np.finfo(np.float64).eps
KMARG_EPS = 1e-8
N_CHAIN = 32


def _copy_prior(p):
    q = Prior()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(q))
    return q


def _bench_ctx(nw, cfg, steady=False):
    pobs = v.workload.steady_point_obs(cfg) if steady else cfg.n_points * cfg.track_len
    ctx = v.Context(device=0, max_windows=nw, max_points=cfg.n_points, max_point_obs=pobs, max_lines=cfg.n_lines,
                    max_line_obs=cfg.n_lines * cfg.track_len)
    ctx.set_prior_rule(v.PRIOR_EIGEN)
    return ctx


def _kept_block(ctx, w):
    lib = ctx.lib
    lib.vpl_ba_debug_marg_Ab.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    A = np.zeros(80 * 80)
    b = np.zeros(80)
    n = lib.vpl_ba_debug_marg_Ab(ctx.h, w, A.ctypes.data_as(C.POINTER(C.c_double)), b.ctypes.data_as(C.POINTER(C.c_double)))
    assert n > 0
    return A[: n * n].reshape(n, n).copy(), b[:n].copy()


def _signed(vec):
    """the sign convention of the factor: the largest component (lowest index on ties) positive"""
    j = int(np.argmax(np.abs(vec)))
    return vec if vec[j] >= 0 else -vec


def _check_factor(A, b, J, r, tag):
    """J, r of one window against eigh of its kept block A (lower triangle); -> (kept rows, eigen count, checked rows)"""
    n = A.shape[0]
    As = np.tril(A) + np.tril(A, -1).T
    S, V = np.linalg.eigh(As)
    smax = np.abs(S).max()
    delta = 64 * EPS * smax
    kept = np.abs(J).max(axis=1) > 0
    nk = int(kept.sum())
    lo, hi = int((S > KMARG_EPS + delta).sum()), int((S > KMARG_EPS - delta).sum())
    assert lo <= nk <= hi, (tag, nk, lo, hi)
    if lo == hi:
        assert nk == lo, tag
    # rows in ascending eigenvalue order: the dropped ones first, then non-decreasing norms
    assert not kept[: n - nk].any() and kept[n - nk:].all(), tag
    sq = (J * J).sum(axis=1)
    assert np.all(np.diff(sq[n - nk:]) >= -1e-12 * sq.max()), tag
    # sign convention on the device's own rows
    for k in np.nonzero(kept)[0]:
        j = int(np.argmax(np.abs(J[k])))
        assert J[k, j] > 0, (tag, k)
    # rows of well-separated kept eigenvalues are sqrt(S_k) v_k^T
    checked = 0
    for k in range(n):
        if not (S[k] > KMARG_EPS + delta):
            continue
        gap = np.abs(np.delete(S, k) - S[k]).min() if n > 1 else np.inf
        if gap <= 1e5 * delta:
            continue
        vk = V[:, k]
        mags = np.sort(np.abs(vk))[::-1]
        want = np.sqrt(S[k]) * _signed(vk)
        err = np.abs(J[k] - want).max()
        if n > 1 and mags[0] - mags[1] <= 1e-6 * mags[0]:   # a near tie decides the sign by rounding
            err = min(err, np.abs(J[k] + want).max())
        assert err <= 1e-5 * np.sqrt(S[k]), (tag, k, S[k], err)
        checked += 1
    # J0^T J0 is the positive part of the spectrum
    Vp = V[:, S > KMARG_EPS]
    Ap = (Vp * S[S > KMARG_EPS]) @ Vp.T
    assert np.abs(J.T @ J - Ap).max() <= 1e-12 * smax, tag
    # r0 through its definition on the device's own rows: J0_k b = S_k r0_k with S_k = |J0_k|^2; dropped rows zero
    nb = np.linalg.norm(b)
    for k in range(n):
        if kept[k]:
            jn = np.linalg.norm(J[k])
            assert abs(J[k] @ b - jn * jn * r[k]) <= 1e-12 * jn * nb + 1e-300, (tag, k)
        else:
            assert r[k] == 0.0, (tag, k)
    return nk, int((S > KMARG_EPS).sum()), checked


def test_factor_is_the_references_on_the_devices_own_kept_blocks():
    opt = v.default_options()
    cfg = v.workload.config(200, 80)
    ids = list(range(64))
    ctx = _bench_ctx(len(ids), cfg)
    B, keep = v.workload.primed_batch(ctx, ids, cfg, opt)      # the A windows (no incoming prior) solved under the eigen rule
    rows = []
    for i in range(len(ids)):
        A, b = _kept_block(ctx, i)
        assert keep[i].n == A.shape[0]
        rows.append(_check_factor(A, b, keep[i].J(), keep[i].r(), ("A", i)))
    pri, rep = ctx.solve_windows(B, opt)                       # the B windows behind their eigen-rule priors
    for i in range(len(ids)):
        A, b = _kept_block(ctx, i)
        assert rep[i].termination in (0, 1) and pri[i].n == A.shape[0]
        rows.append(_check_factor(A, b, pri[i].J(), pri[i].r(), ("B", i)))
    ctx.close()
    # the steady state: n = 75
    ctx = _bench_ctx(32, cfg, steady=True)
    Bs, n_prior = v.workload.steady_batch(ctx, ids[:32], cfg, opt)
    assert n_prior == 75
    ctx.solve()
    ctx.synchronize()
    pri, rep = ctx.download()
    steady = []
    for i in range(32):
        A, b = _kept_block(ctx, i)
        assert A.shape[0] == 75 and pri[i].n == 75
        steady.append(_check_factor(A, b, pri[i].J(), pri[i].r(), ("steady", i)))
    ctx.close()
    kept = np.array([r[0] for r in rows])
    print("eigen rule, n = 45: kept %d..%d directions (first window %d), %d rows checked against eigh; n = 75: kept %d..%d, %d rows"
          % (kept.min(), kept.max(), kept[0], sum(r[2] for r in rows), min(r[0] for r in steady), max(r[0] for r in steady),
             sum(r[2] for r in steady)))
    assert sum(r[2] for r in rows) > 0 and sum(r[2] for r in steady) > 0


def _chain_windows():
    opt = v.default_options()
    cfg = v.workload.config(200, 80, True)
    ws = [v.workload.generate(v.workload.seed_for(3, 7000 + k), cfg, 0.25 + k * cfg.kf_dt) for k in range(N_CHAIN)]
    o.preintegrate_windows(ws, opt)
    return ws, opt


def test_free_running_chain_under_the_eigen_rule():
    """tests/test_gpu_chain.py's 32 windows: the device carries its own eigen-rule prior, the oracle its own (the
    reference's rule); every window inside the bar"""
    ws, opt = _chain_windows()
    ctx = v.Context(device=0, max_windows=1, max_points=200, max_point_obs=200 * 11, max_lines=80, max_line_obs=80 * 11)
    ctx.set_prior_rule(v.PRIOR_EIGEN)
    worst, pd, pc = (0.0, 0.0), None, None
    for k, w in enumerate(ws):
        wd, wc = w.copy(), w.copy()
        wd.prior, wc.prior = pd, pc
        pri, rep = ctx.solve_windows([wd], opt)
        pd = _copy_prior(pri[0])
        p, rc = o.solve_window(wc, opt)
        pc = _copy_prior(p)
        dp, dr = pose_err(wd, wc)
        assert dp <= POS_TOL and dr <= ROT_TOL, (k, dp, dr)
        assert pd.n == pc.n, k
        worst = (max(worst[0], dp), max(worst[1], dr))
    ctx.close()
    print("free-running chain of %d windows under the eigen rule: worst dp %.3g m dr %.3g rad" % (N_CHAIN, worst[0], worst[1]))


def test_random_shapes_behind_their_own_prior_under_both_rules():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_parity
    lines_e, lines_d = [], []
    eig = fuzz_parity.run(14, 8, 11, out=lines_e.append, prior_rule=v.PRIOR_EIGEN)
    dflt = fuzz_parity.run(14, 8, 11, out=lines_d.append)
    pick = lambda lines: "\n".join(l for l in lines if "MISS" in l or "REFUSED" in l or "fuzz_parity" in l)
    tail = "eigen rule:\n" + pick(lines_e) + "\npivoted Cholesky:\n" + pick(lines_d)
    ce, cd = eig["miss"] - eig["miss_first"], dflt["miss"] - dflt["miss_first"]
    print("chained misses, 14 x 8 windows of seed 11: eigen rule %d, pivoted Cholesky %d\n%s" % (ce, cd, tail))
    assert eig["miss_first"] == 0 and dflt["miss_first"] == 0, tail
    # (the chained windows that still leave the bar under the eigen rule are weakly determined ones behind a prior whose
    #  kept block differs from the oracle's by the rounding of its Schur complement: DESIGN.md section 7)
    assert ce <= cd, tail


def _primed(n, cfg, opt):
    helper = v.Context(device=0, max_windows=n, max_points=cfg.n_points, max_point_obs=cfg.n_points * cfg.track_len,
                       max_lines=cfg.n_lines, max_line_obs=cfg.n_lines * cfg.track_len)
    B, keep = v.workload.primed_batch(helper, list(range(100, 100 + n)), cfg, opt)
    helper.close()
    return B, keep


def _solve(ctx, ws, opt):
    ws = [w.copy() for w in ws]
    pri, rep = ctx.solve_windows(ws, opt)
    return ws, [_copy_prior(p) for p in pri]


def _same(a, b):
    (wa, pa), (wb, pb) = a, b
    assert len(wa) == len(wb)
    for i in range(len(wa)):
        assert np.array_equal(wa[i].pose, wb[i].pose) and np.array_equal(wa[i].speed_bias, wb[i].speed_bias), i
        assert np.array_equal(wa[i].ex_pose, wb[i].ex_pose), i
        assert pa[i].n == pb[i].n and np.array_equal(pa[i].J(), pb[i].J()) and np.array_equal(pa[i].r(), pb[i].r()), i


def test_eigen_rule_is_deterministic():
    import torch
    opt = v.default_options()
    cfg = v.workload.config(200, 80)
    B, keep = _primed(16, cfg, opt)
    ctx = _bench_ctx(16, cfg)
    first = _solve(ctx, B, opt)
    _same(first, _solve(ctx, B, opt))
    half = _solve(ctx, B[8:], opt)
    _same(half, (first[0][8:], first[1][8:]))
    # graph replay (a stream of its own) against kernel-by-kernel launches (leg timing on)
    st = torch.cuda.Stream(device=0)
    ctx.set_stream(st.cuda_stream)
    ws = [w.copy() for w in B]
    ctx.upload(ws, opt)
    ctx.solve(); ctx.synchronize()
    pri, _ = ctx.download()
    graph = (ws, [_copy_prior(p) for p in pri])
    ctx.lib.vpl_ctx_enable_leg_timing.argtypes = [C.c_void_p, C.c_int]
    assert ctx.lib.vpl_ctx_enable_leg_timing(ctx.h, 1) == 0
    ws = [w.copy() for w in B]
    ctx.upload(ws, opt)
    ctx.solve(); ctx.synchronize()
    pri, _ = ctx.download()
    _same(graph, (ws, [_copy_prior(p) for p in pri]))
    _same(graph, first)
    ctx.close()


def test_switching_the_rule_on_one_context():
    opt = v.default_options()
    cfg = v.workload.config(120, 40, True)
    mk = lambda base: [v.workload.generate(v.workload.seed_for(3, base + i), cfg, 0.3 * i + (base - 7400) / 100 * cfg.kf_dt)
                       for i in range(4)]
    Wa, Wb, Wc = mk(7400), mk(7500), mk(7600)
    o.preintegrate_windows(Wa + Wb + Wc, opt)

    def fresh(rule):
        c = v.Context(device=0, max_windows=4, max_points=120, max_point_obs=120 * 11, max_lines=40, max_line_obs=40 * 11)
        c.set_prior_rule(rule)
        return c

    def chained(ctx, ws):
        ws = [w.copy() for w in ws]
        ctx.upload(ws, opt, chained=True)
        ctx.solve(); ctx.synchronize()
        pri, _ = ctx.download()
        return ws, [_copy_prior(p) for p in pri]

    def behind(ws, pri):
        ws = [w.copy() for w in ws]
        for i in range(len(ws)):
            ws[i].prior = pri[i]
        return ws

    # references: a fresh context per call, the priors handed over through the host (the bits of the device hand-over)
    f = fresh(v.PRIOR_PIVOTED_CHOLESKY); r1 = _solve(f, Wa, opt); f.close()
    f = fresh(v.PRIOR_EIGEN); r2 = _solve(f, behind(Wb, r1[1]), opt); f.close()
    f = fresh(v.PRIOR_PIVOTED_CHOLESKY); r3 = _solve(f, behind(Wc, r2[1]), opt); f.close()
    f = fresh(v.PRIOR_PIVOTED_CHOLESKY); r2d = _solve(f, behind(Wb, r1[1]), opt); f.close()
    assert any(not np.array_equal(a.J(), b.J()) for a, b in zip(r2[1], r2d[1]))   # the two rules give different priors
    # one context: default -> eigen -> default, with the device hand-over in between
    ctx = fresh(v.PRIOR_PIVOTED_CHOLESKY)
    _same(_solve(ctx, Wa, opt), r1)
    ctx.set_prior_rule(v.PRIOR_EIGEN)
    _same(chained(ctx, Wb), r2)
    ctx.set_prior_rule(v.PRIOR_PIVOTED_CHOLESKY)
    _same(chained(ctx, Wc), r3)
    _same(_solve(ctx, Wa, opt), r1)                     # as a context that never switched
    # an unknown rule is refused and changes nothing
    for bad in (2, -1):
        with pytest.raises(RuntimeError):
            ctx.set_prior_rule(bad)
    _same(_solve(ctx, Wa, opt), r1)
    # the setter collects a pending vpl_ba_marginalize_async first; that call ran under the rule it was enqueued with
    f = fresh(v.PRIOR_EIGEN)
    pe, me, ne = f.marginalize([w.copy() for w in Wb], opt, v.MARGIN_OLD)
    f.close()
    ctx.set_prior_rule(v.PRIOR_EIGEN)
    pa, ma, na = ctx.marginalize([w.copy() for w in Wb], opt, v.MARGIN_OLD, async_=True)
    assert all(pa[i].n == 0 for i in range(4))          # not collected yet
    ctx.lib.vpl_ba_set_prior_rule.argtypes = [C.c_void_p, C.c_int]
    assert ctx.lib.vpl_ba_set_prior_rule(ctx.h, v.PRIOR_PIVOTED_CHOLESKY) == 0
    assert all(pa[i].n > 0 for i in range(4))          # collected by the setter
    ctx.collect()
    for i in range(4):
        assert pa[i].n == pe[i].n and np.array_equal(pa[i].J(), pe[i].J()) and np.array_equal(pa[i].r(), pe[i].r()), i
    assert np.array_equal(ma, me) and np.array_equal(na, ne)
    _same(_solve(ctx, Wa, opt), r1)
    ctx.close()


def test_nan_window_under_the_eigen_rule():
    """the pattern of test_gpu_solve.py's NaN test: the NaN windows fail as ceres fails them, the kernel returns, the clean
    window is solved (states and prior) as it is on its own"""
    opt = v.default_options()
    cfg = v.workload.config(40, 12, True)
    kinds = ("point_obs", "line_obs", "clean", "inv_depth", "imu", "pose")
    ws = []
    for i, what in enumerate(kinds):
        w = v.workload.generate(v.workload.seed_for(3, 7 + i), cfg, 0.1 * i)
        if what == "imu":
            w.extra["imu_samples"][3, 2, 1] = np.nan
        ws.append(w)
    o.preintegrate_windows(ws, opt)
    ws[0].point_obs[5, 0] = np.nan
    ws[1].line_obs[7, 2] = np.nan
    ws[3].inv_depth[3] = np.nan
    ws[5].pose[4, 1] = np.nan
    ctx = v.Context(device=0, max_windows=6, max_points=40, max_point_obs=40 * 11, max_lines=12, max_line_obs=12 * 11)
    ctx.set_prior_rule(v.PRIOR_EIGEN)
    wg = [w.copy() for w in ws]
    pri, rep = ctx.solve_windows(wg, opt)
    alone = _solve(ctx, [ws[2]], opt)
    ctx.close()
    for i, what in enumerate(kinds):
        if what == "clean":
            assert rep[i].termination in (0, 1)
            _same(([wg[i]], [_copy_prior(pri[i])]), alone)
            wc = ws[i].copy()
            o.solve_window(wc, opt)
            dp, dr = pose_err(wg[i], wc)
            assert dp <= POS_TOL and dr <= ROT_TOL
        else:
            assert (rep[i].iterations, rep[i].num_successful_steps, rep[i].termination) == (-1, -1, 2), what


def test_guard_pads_stay_intact_under_the_eigen_rule():
    """kept blocks of 45 and 75 dims and batches of mixed size through k_prior_eigen with 0xA5 behind every device array
    (VPL_DEBUG_GUARDS=1): closing the contexts reports no overrun"""
    script = r"""
import sys
sys.path.insert(0, %r)
import vplines_slam_amd as v
opt = v.default_options()
cfg = v.workload.config(200, 80)
ctx = v.Context(device=0, max_windows=8, max_points=200, max_point_obs=200 * cfg.track_len, max_lines=80, max_line_obs=80 * cfg.track_len)
ctx.set_prior_rule(v.PRIOR_EIGEN)
B, keep = v.workload.primed_batch(ctx, list(range(8)), cfg, opt)
ctx.solve_windows(B[:3], opt)
ctx.solve_windows(B, opt)
ctx.close()
ctx = v.Context(device=0, max_windows=4, max_points=200, max_point_obs=v.workload.steady_point_obs(cfg), max_lines=80, max_line_obs=80 * cfg.track_len)
ctx.set_prior_rule(v.PRIOR_EIGEN)
Bs, n = v.workload.steady_batch(ctx, [0, 1, 2, 3], cfg, opt, chain=3)
ctx.solve(); ctx.synchronize(); ctx.download()
ctx.close()
print("guards ok", n)
""" % ROOT
    env = dict(os.environ, VPL_DEBUG_GUARDS="1")
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "guards ok" in r.stdout
