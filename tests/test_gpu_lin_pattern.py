"""k_lin stores only the entries of the packed camera Hessian that a window's factors can fill (csrc/ba_asm_pattern.h): the
pattern of the fast path for every window, the complement only for windows of the general path.  Everything else holds the zeros
Hcc was allocated with; an upload behind a batch that had a general window fills them again.  No arithmetic depends on any of
this, so every comparison here is exact: the complement read back through vpl_ba_debug_linearization is 0.0, and a context that
has seen general windows gives the bits a fresh one gives."""
import ctypes as C

import numpy as np
import pytest

import vplines_slam_amd as v
from test_gpu_solve import make_windows

pytestmark = pytest.mark.gpu
NC = 171
CAP = dict(max_windows=4, max_points=60, max_point_obs=660, max_lines=20, max_line_obs=220)


def _pattern():
    """[171, 171] bool, symmetric: the visual block, the IMU band (15-dim frame blocks and their sub-diagonal neighbours),
    speed/bias 0 against the visual dims"""
    vis = lambda c: c >= 165 or c % 15 < 6
    m = np.zeros((NC, NC), bool)
    for r in range(NC):
        for c in range(r + 1):
            fr, fc = (r // 15 if r < 165 else -1), (c // 15 if c < 165 else -1)
            band = fr >= 0 and fc >= 0 and fr - fc in (0, 1)
            m[r, c] = m[c, r] = (vis(r) and vis(c)) or band or (6 <= c < 15 and vis(r))
    assert int(np.tril(m).sum()) == 6147
    return m


PAT = _pattern()


def _ctx(**over):
    return v.Context(device=0, **dict(CAP, **over))


def _copy_prior(p):
    q = v.Prior()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(q))
    return q


def _later_speed_bias_prior(w, rng):
    """a prior over pose 2, speed/bias 3 and the extrinsic (test_prior_with_speed_bias_of_a_later_frame_takes_the_general_path):
    outside k_chol's elimination order, routed to k_solve at upload; speed/bias 3 against the extrinsic lies outside the pattern"""
    p = v.Prior()
    n = 6 + 9 + 6
    p.n, p.n_blocks = n, 3
    idx = 0
    for b, (k, f) in enumerate(zip([0, 1, 2], [2, 3, 0])):
        p.block_kind[b], p.block_frame[b], p.block_idx[b] = k, f, idx
        x0 = (w.pose[f] if k == 0 else w.speed_bias[f] if k == 1 else w.ex_pose)
        for j in range(len(x0)):
            p.x0[b][j] = float(x0[j])
        idx += 9 if k == 1 else 6
    J = np.triu(rng.normal(size=(n, n))) * 3.0 + 5.0 * np.eye(n)
    np.ctypeslib.as_array(p.J0)[: n * n] = J.reshape(-1)
    np.ctypeslib.as_array(p.r0)[:n] = rng.normal(size=n) * 0.1
    return p


_cache = {}


def _inputs():
    """four fast-path windows that carry the prior a first solve left them (frame 0's speed/bias: the fast path), four general
    ones (a later frame's speed/bias), and the options; built once"""
    if not _cache:
        ws, opt = make_windows(4, 60, 20, True, seed0=3300)
        ctx = _ctx()
        pri, _ = ctx.solve_windows([w.copy() for w in ws], opt)
        fast = []
        for w, p in zip(ws, pri):
            w = w.copy()
            w.prior = _copy_prior(p)
            assert all(p.block_frame[b] == 0 for b in range(p.n_blocks) if p.block_kind[b] == 1)
            fast.append(w)
        ctx.close()
        gs, _ = make_windows(4, 60, 20, True, seed0=3400)
        rng = np.random.default_rng(3)
        gen = []
        for w in gs:
            w = w.copy()
            w.prior = _later_speed_bias_prior(w, rng)
            gen.append(w)
        _cache.update(fast=fast, gen=gen, opt=opt)
    return _cache["fast"], _cache["gen"], _cache["opt"]


def _options(**kw):
    opt = v.default_options()
    for k, val in kw.items():
        setattr(opt, k, val)
    return opt


def _run(ctx, ws, opt):
    """upload + solve + download; everything the comparison looks at, per window"""
    g = [w.copy() for w in ws]
    pri, rep = ctx.solve_windows(g, opt)
    out = []
    for i, w in enumerate(g):
        lin = ctx.debug_linearization(i)
        out.append(dict(H=lin["H"][:NC, :NC].copy(), g=lin["g"][:NC].copy(), states=v.shard.pack_states([w])[0], invd=w.inv_depth.copy(),
                        plk=w.line_plk.copy(), cost=(rep[i].initial_cost, rep[i].final_cost, rep[i].iterations, rep[i].num_successful_steps),
                        prior_n=pri[i].n, J=pri[i].J(), r=pri[i].r(), path=ctx.debug_step(i)["path"]))
    return out


def _same(a, b, what):
    for k in ("H", "g", "states", "invd", "plk", "J", "r"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["cost"] == b["cost"] and a["prior_n"] == b["prior_n"], what


def _complement_is_zero(H, what):
    assert np.all(H[~PAT] == 0.0), (what, int(np.count_nonzero(H[~PAT])))
    assert np.all(np.diag(H)[:30] > 0.0), what            # (and the pattern was assembled: the IMU factor of frames 0 and 1 is in every pass)


def test_complement_holds_zeros_after_the_solve_and_after_the_marginalisation_pass():
    fast, _, _ = _inputs()
    ctx = _ctx()
    for flag, what in ((v.capi.MARGIN_NONE, "solve pass"), (v.capi.MARGIN_OLD, "marginalisation pass")):
        res = _run(ctx, fast, _options(marginalization_flag=flag))
        for i, r in enumerate(res):
            assert r["path"] == 0
            _complement_is_zero(r["H"], (what, i))
            # the prior's speed/bias 0 against the poses it ties: the part of the pattern only a prior fills
            assert np.count_nonzero(r["H"][30:36, 6:15]) > 0, (what, i)
    ctx.close()


def test_fast_windows_behind_general_ones_find_no_stale_entries():
    fast, gen, opt = _inputs()
    used = _ctx()
    rg = _run(used, gen, opt)
    for i, r in enumerate(rg):
        assert r["path"] == 1
        assert np.count_nonzero(r["H"][165:171, 51:60]) > 0, i      # speed/bias 3 against the extrinsic: outside the pattern
    second = _run(used, fast, opt)
    used.close()
    fresh = _ctx()
    first = _run(fresh, fast, opt)
    fresh.close()
    for i in range(4):
        _complement_is_zero(second[i]["H"], i)
        _same(second[i], first[i], i)


def test_mixed_batch_gives_every_window_what_it_gives_alone():
    fast, gen, opt = _inputs()
    batch = [fast[0], gen[0], fast[1], gen[1]]
    ctx = _ctx()
    together = _run(ctx, batch, opt)
    ctx.close()
    for i, w in enumerate(batch):
        one = _ctx()
        alone = _run(one, [w], opt)[0]
        one.close()
        assert together[i]["path"] == alone["path"] == i % 2
        _same(together[i], alone, i)          # (H whole: for the general windows the complement entries too)
        if i % 2 == 0:
            _complement_is_zero(together[i]["H"], i)
        else:
            assert np.count_nonzero(together[i]["H"][~PAT]) > 0, i


def test_fixed_extrinsic_rows_are_zero():
    """estimate_extrinsic = 0: the solve pass leaves zeros in the extrinsic's rows (the marginalisation pass evaluates every
    block, constant or not: its Hcc has them), and with either pass last the result is a fresh context's"""
    fast, gen, _ = _inputs()
    for flag in (v.capi.MARGIN_NONE, v.capi.MARGIN_OLD):
        opt = _options(estimate_extrinsic=0, marginalization_flag=flag)
        used = _ctx()
        _run(used, gen, opt)
        second = _run(used, fast, opt)
        used.close()
        fresh = _ctx()
        first = _run(fresh, fast, opt)
        fresh.close()
        for i in range(4):
            if flag == v.capi.MARGIN_NONE:
                assert np.all(second[i]["H"][165:, :] == 0.0) and np.all(second[i]["g"][165:] == 0.0), i
            _complement_is_zero(second[i]["H"], (flag, i))
            _same(second[i], first[i], (flag, i))


def test_forced_general_path_assembles_the_same_pattern_entries(monkeypatch):
    """VPL_BA_GENERAL=1 (read when the context is made) sends every window through both passes of the assembly; at the same
    states -- a solve of zero iterations, no marginalisation pass behind it -- Hcc is the default run's on the pattern and zero
    elsewhere, and a batch solved by the default context's successor in the same slots starts from zeros again"""
    fast, _, _ = _inputs()
    opt = _options(num_iterations=0, marginalization_flag=v.capi.MARGIN_NONE)
    ctx = _ctx()
    default = _run(ctx, fast, opt)
    ctx.close()
    monkeypatch.setenv("VPL_BA_GENERAL", "1")
    gen = _ctx()
    monkeypatch.delenv("VPL_BA_GENERAL")
    forced = _run(gen, fast, opt)
    again = _run(gen, fast, opt)              # (behind a batch of general windows: the upload's zero fill, then both passes)
    gen.close()
    for i in range(4):
        assert default[i]["path"] == 0 and forced[i]["path"] == 1
        _complement_is_zero(forced[i]["H"], i)
        assert np.array_equal(forced[i]["H"], default[i]["H"]) and np.array_equal(forced[i]["g"], default[i]["g"]), i
        assert np.array_equal(again[i]["H"], default[i]["H"]), i


def test_prior_larger_than_the_image_in_lds_is_added_behind_the_pattern_pass():
    """A context of 60 points and 214 lines leaves k_lin's LDS room for a prior of 47 dims; the steady-state prior of 75 dims
    (every point track over all 11 frames) is then added to the assembled entries in HBM, behind the pass over the pattern --
    and behind a batch of general windows in the same slots the result is a fresh context's."""
    opt = v.default_options()
    cfg = v.workload.config(60, 20, True)
    import oracle_api as o
    a = [v.workload.graft_long_tracks(v.workload.seed_for(3, 3500 + k), cfg, 0.41 * k, 1) for k in range(2)]
    b = [v.workload.graft_long_tracks(v.workload.seed_for(3, 3600 + k), cfg, 0.41 * k + cfg.kf_dt, 1) for k in range(2)]
    o.preintegrate_windows(a + b, opt)
    cap = dict(max_windows=2, max_points=60, max_point_obs=660, max_lines=214, max_line_obs=214 * 11)
    small = _ctx(max_windows=2)
    pri, _ = small.solve_windows([w.copy() for w in a], opt)
    assert all(p.n > 47 for p in pri), [p.n for p in pri]
    for w, p in zip(b, pri):
        w.prior = _copy_prior(p)
    small.close()
    _, gen, _ = _inputs()
    used = _ctx(**cap)
    _run(used, gen[:2], opt)
    second = _run(used, b, opt)
    used.close()
    fresh = _ctx(**cap)
    first = _run(fresh, b, opt)
    fresh.close()
    for i in range(2):
        assert first[i]["path"] == 0
        _complement_is_zero(second[i]["H"], i)
        assert np.count_nonzero(second[i]["H"][135:141, 6:15]) > 0, i      # the prior's speed/bias 0 against pose 9
        _same(second[i], first[i], i)
