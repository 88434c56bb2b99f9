"""How the kernels consume a GIVEN prior, against the long-double restatement prior_ref.py (checked against the oracle on the CPU
by test_prior_reference.py): k_eval_prior behind vpl_prior_factor, k_prep's H = J0^T J0 and g0 = J0^T r0, lin_prior's
r = r0 + J0 dx and g = g0 + H dx, lin_assemble's three ways of putting the prior into Hcc (prH in LDS, pr_H read again on the
general path, the += pass for n > PRH_N), and the prior's terms in k_cost and k_solve.  Priors, state families and windows:
prior_inputs.py.  The reference is always taken at the states the device reports (vpl_ba_debug_linearization): k_prep passes the
window's quaternions through a rotation matrix and back.

Units: prior_ref's (forward error of the reference's own formula, the rounding of dx propagated).  Bars: 8 x max(yardstick, 1),
the yardstick being what the float64 restatement of the REFERENCE's formulation reaches on the same prior on the CPU
(prior_ref.YARDSTICK); nothing is tuned to the device.  Every entry with a positive unit is compared, every other entry has to
be 0.0.  Contexts: 40 points / 12 lines (lin_prh_n = 76: n = 75 keeps J0^T J0 in LDS, n = 81 takes the += pass) and 478 / 12
(lin_prh_n = 44: n = 48 and n = 75 take the += pass on the fast path); test_prior_reference.py evaluates lin_prh_n for both."""
import numpy as np
import pytest

import prior_inputs as pi
import prior_ref as pr
import step_ref as sr
import vplines_slam_amd as v

pytestmark = pytest.mark.gpu
EPS, LD = pr.EPS64, pr.LD
SMALL, LARGE = (40, 12), (478, 12)

_cache, _failed = {}, {}


def _once(key, make):
    """one device run per key; after a failed run nothing more of this file is sent to the device"""
    if _failed:
        raise _failed["first"]
    if key not in _cache:
        try:
            _cache[key] = make()
        except BaseException as e:
            _failed["first"] = e
            raise
    return _cache[key]


def _context(n_windows, cap=SMALL):
    return v.Context(device=0, max_windows=n_windows, max_points=cap[0], max_point_obs=cap[0] * 11, max_lines=cap[1],
                     max_line_obs=cap[1] * 11)


def _linearise(ctx, windows, opt):
    ctx.upload([w.copy() for w in windows], opt)
    ctx.solve()
    ctx.synchronize()
    return [ctx.debug_linearization(k) for k in range(len(windows))]


def _opt0(**kw):
    return sr._options(num_iterations=0, **kw)


def _pids(batch):
    return [pi.pid_of(n, s) for n in pi.BATCHES[batch] for s in "us"]


def _windows(pids, family):
    return [pi.window(*pi.case(pid, family)) for pid in pids]


def _batch(batch, family):
    """batch A, B or C (both row-scale variants of every size) of a family, linearised in a fresh small-capacity context"""
    def make():
        ctx = _context(len(_pids(batch)))
        try:
            return _linearise(ctx, _windows(_pids(batch), family), _opt0())
        finally:
            ctx.close()
    return _once((batch, family), make)


def _x_dev(lin):
    return dict(pose=lin["pose"], sb=lin["speed_bias"], ex=lin["ex_pose"])


def _amax(a):
    return float(np.abs(a).max())


def _check_share(pid, family, lin, ex_free=True, label=""):
    """H, g, x_cost of a prior-only window against prior_ref at the device's states -> the Ref"""
    prior, x = pi.case(pid, family)
    xd = _x_dev(lin)
    assert (lin["n"], lin["n_points"], lin["n_lines"]) == (pr.NC, 0, 0)
    # the states the kernels linearised at are the uploaded ones up to the rounding of quaternion -> matrix -> quaternion
    assert _amax(xd["pose"][:, :3] - x["pose"][:, :3]) <= 8 * EPS * max(1.0, _amax(x["pose"][:, :3]))
    assert sr_qdiff(xd["pose"][:, 3:], x["pose"][:, 3:]) <= 8 * EPS and sr_qdiff(xd["ex"][3:], x["ex"][3:]) <= 8 * EPS
    assert _amax(xd["sb"] - x["sb"]) <= 8 * EPS * max(1.0, _amax(x["sb"])) and _amax(xd["ex"][:3] - x["ex"][:3]) <= 8 * EPS
    ref = pr.Ref(prior, xd, ex_free)
    H, g = lin["H"], lin["g"]
    assert np.array_equal(H, H.T)
    assert np.all(H[ref.unit_H == 0] == 0.0) and np.all(g[ref.unit_g == 0] == 0.0), "an entry outside the prior's columns is not 0.0"
    got = dict(H=pr.rho(H, ref.H, ref.unit_H), g=pr.rho(g, ref.g, ref.unit_g),
               cost=float(abs(LD(lin["x_cost"]) - ref.cost) / ref.unit_cost))
    print("%s%s %s rho_H %.3g rho_g %.3g rho_cost %.3g (bars %.3g %.3g %.3g)"
          % (label, pid, family, got["H"], got["g"], got["cost"], pr.bar("H", pid), pr.bar("g", pid), pr.bar("cost", pid)))
    for what, val in got.items():
        assert val <= pr.bar(what, pid), (pid, family, what, val)
    return ref


def sr_qdiff(a, b):
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return max(min(np.abs(p - q).max(), np.abs(p + q).max()) for p, q in zip(a, b))


@pytest.fixture(scope="module")
def factor_ctx():
    ctx = _context(1)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("pid", pi.PRIORS)
def test_prior_factor_kernel(factor_ctx, pid):
    """vpl_prior_factor (k_eval_prior): the residuals of every size and family within the r bar, the Jacobian blocks J0's columns
    bit for bit with a zero seventh pose column -- the sharpest check of prior_block_dx, which k_lin, k_cost and k_solve share"""
    for family in pi.FAMILIES:
        prior, x = pi.case(pid, family)
        ref = pr.Ref(prior, x)
        r, jac = _once(("factor", pid, family), lambda: factor_ctx.prior_factor(prior, pr.params(prior, x)))
        rho_r = pr.rho(r, ref.r, ref.unit_r)
        print("k_eval_prior %s %s rho_r %.3g (bar %.3g)" % (pid, family, rho_r, pr.bar("r", pid)))
        assert rho_r <= pr.bar("r", pid)
        if family == "at_x0":
            assert np.array_equal(r, prior.r())
        off = 0
        for Jb in ref.jac_blocks():
            assert np.array_equal(jac[off:off + Jb.size].reshape(Jb.shape), Jb)
            off += Jb.size
        assert off == jac.size


@pytest.mark.parametrize("family", pi.FAMILIES)
@pytest.mark.parametrize("batch", sorted(pi.BATCHES))
def test_prior_only_linearisation(batch, family):
    """k_prep + k_lin on windows whose only residual block is the prior.  A: 21 .. 75 (register pass, tail loop, second row pass,
    partial tiles and K-steps; 21 on the general path); B: 75, 81, 111 (prH in LDS, the += pass, pass B of the general path);
    C: 48, 117, 171 (nstage = 112: one window staged, two on k_prep's unstaged loop)"""
    lins = _batch(batch, family)
    for pid, lin in zip(_pids(batch), lins):
        ref = _check_share(pid, family, lin)
        if family == "at_x0":        # the device's states are the uploaded ones, dx is exactly 0
            prior, x = pi.case(pid, family)
            off = {k: _amax(a - x[k]) for k, a in _x_dev(lin).items()}
            assert all(d == 0.0 for d in off.values()), (pid, off)
            assert np.all(ref.dx == 0)
    if family == "at_x0":
        # ... so g is g0, whatever the states: bit for bit the g of the same J0, r0 at another state with dx = 0
        def make():
            ctx = _context(len(_pids(batch)))
            try:
                return _linearise(ctx, [pi.window(*pi.zero_dx_case(pid)) for pid in _pids(batch)], _opt0())
            finally:
                ctx.close()
        zero = _once((batch, "zero_dx"), make)
        for pid, lin, z in zip(_pids(batch), lins, zero):
            assert np.array_equal(lin["g"], z["g"]) and np.array_equal(lin["H"], z["H"]), pid
            zref = pr.Ref(*pi.zero_dx_case(pid))
            assert np.all(zref.dx == 0) and abs(LD(z["x_cost"]) - zref.cost) <= pr.bar("cost", pid) * zref.unit_cost


def test_prh_n_below_n_on_the_fast_path():
    """A context of 478 points / 12 lines leaves k_lin LDS for priors of up to lin_prh_n = 44 dims (40 / 12: 76), so the
    fast-path priors of 48 and 75 dims go into Hcc by the += pass behind pass A instead of from prH.  Within the bars, and H
    equal to the small-capacity context's to the last bit: both paths only copy pr_H where the prior is the only term"""
    pids = [pi.pid_of(n, s) for n in (48, 75) for s in "us"]
    for family in ("general", "exact"):
        def make(cap):
            ctx = _context(len(pids), cap)
            try:
                return _linearise(ctx, _windows(pids, family), _opt0())
            finally:
                ctx.close()
        large = _once(("prh", family, LARGE), lambda: make(LARGE))
        small = _once(("prh", family, SMALL), lambda: make(SMALL))
        for pid, a, b in zip(pids, large, small):
            _check_share(pid, family, a, label="478/12 ")
            assert np.array_equal(a["H"], b["H"]) and np.array_equal(a["g"], b["g"]) and a["x_cost"] == b["x_cost"], pid


def test_extrinsic_held_constant():
    """estimate_extrinsic = 0 with n = 75 (prH in LDS: lin_asm_store zeroes the rows) and n = 81 (the += pass skips them): rows
    and columns 165..170 of H and the same entries of g exactly zero, the rest within the bars -- r and the cost keep the
    extrinsic's dx"""
    pids = [pi.pid_of(n, s) for n in (75, 81) for s in "us"]
    for family in ("general", "exact"):
        def make():
            ctx = _context(len(pids))
            try:
                return _linearise(ctx, _windows(pids, family), _opt0(estimate_extrinsic=0))
            finally:
                ctx.close()
        for pid, lin in zip(pids, _once(("ex_fixed", family), make)):
            assert np.all(lin["H"][165:171, :] == 0.0) and np.all(lin["H"][:, 165:171] == 0.0) and np.all(lin["g"][165:171] == 0.0)
            ref = _check_share(pid, family, lin, ex_free=False, label="ex fixed ")
            assert np.abs(ref.dx[-6:]).min() > 0


def test_stale_strides_and_batch_position():
    """pr_J0 and pr_H are strided by the batch's largest prior: batch C (171) then batch A (75) on ONE context, then A in reversed
    order -- H, g and cost of every window bit-identical to batch A in a fresh context, whatever was there before and wherever
    in the batch the window sits"""
    fresh = _batch("A", "general")
    pids = _pids("A")

    def make():
        ctx = _context(len(pids))
        try:
            c = _linearise(ctx, _windows(_pids("C"), "general"), _opt0())
            a = _linearise(ctx, _windows(pids, "general"), _opt0())
            rev = _linearise(ctx, _windows(pids[::-1], "general"), _opt0())
            return c, a, rev[::-1]
        finally:
            ctx.close()
    c, a, rev = _once("stale", make)
    for lin, ref in zip(c, _batch("C", "general")):
        assert np.array_equal(lin["H"], ref["H"]) and np.array_equal(lin["g"], ref["g"]) and lin["x_cost"] == ref["x_cost"]
    for pid, f, x, y in zip(pids, fresh, a, rev):
        for name, lin in (("behind batch C", x), ("reversed", y)):
            assert np.array_equal(lin["H"], f["H"]), (pid, name)
            assert np.array_equal(lin["g"], f["g"]) and lin["x_cost"] == f["x_cost"], (pid, name)


def test_prior_behind_landmarks():
    """step_ref's case d (37 points, 11 lines, ragged tracks) behind a general-family prior of 75 dims (prH from LDS, summed with
    the visual and IMU terms in registers) and of 81 (added in HBM behind them): H and g of the camera block in step_ref's units
    and bars, the prior's row of the reference taken from prior_ref (long double from dx on) at the device's states"""
    ws = [pi.landmark_window(n) for n in (75, 81)]

    def make():
        ctx = _context(2)
        try:
            return _linearise(ctx, ws, _opt0())
        finally:
            ctx.close()
    for n, w, lin in zip((75, 81), ws, _once("landmarks", make)):
        prob = sr.Problem(w, _opt0(), prior_rows=pr.prior_rows)
        x0 = prob.initial_state()
        assert (lin["n"], lin["n_points"], lin["n_lines"]) == (prob.n, prob.nP, prob.nL)
        assert _amax(lin["pose"] - x0["pose"]) <= 1e-12 and _amax(lin["ex_pose"] - x0["ex"]) <= 1e-12
        x = dict(pose=lin["pose"], sb=lin["speed_bias"], ex=lin["ex_pose"], invd=w.inv_depth[:prob.nP].copy(), orth=lin["line_orth"])
        ref = prob.linearize(x)
        C = slice(0, sr.NC)
        H, g = lin["H"], lin["g"]
        assert np.all(H[C, C][ref.unit_H[C, C] == 0] == 0.0)
        rho_H, rho_g = sr.rho(H[C, C], ref.H[C, C], ref.unit_H[C, C]), sr.rho(g[C], ref.g[C], ref.unit_g[C])
        print("case d behind n = %d: rho_H %.3g rho_g %.3g (bars %.3g %.3g)" % (n, rho_H, rho_g, sr.bar("H"), sr.bar("g")))
        assert rho_H <= sr.bar("H") and rho_g <= sr.bar("g")
        # the prior's own entries are not lost in the sums: taken out of H, what is left has none of it where the prior alone
        # would sit -- speed/bias 0 against the poses of frames 2.. holds nothing but the prior
        share = pr.Ref(w.prior, _x_dev(lin))
        only = np.zeros((sr.NC, sr.NC), bool)
        only[6:15, 30:165] = only[30:165, 6:15] = True
        only &= np.asarray(share.unit_H > 0)
        assert only.any() and pr.rho(np.where(only, H[C, C], 0), np.where(only, share.H, 0), np.where(only, share.unit_H, 0)) <= pr.bar("H", "n%du" % n)


def _one_iteration(which):
    w, opt = pi.step_window(which)

    def make():
        ctx = _context(1)
        try:
            w1 = w.copy()
            ctx.upload([w1], opt)
            ctx.solve()
            ctx.synchronize()
            lin, stp = ctx.debug_linearization(0), ctx.debug_step(0)
            _, rep = ctx.download()
            lin0 = _linearise(ctx, [w], _opt0(estimate_extrinsic=opt.estimate_extrinsic))[0]
            return lin0, lin, stp, rep[0]
        finally:
            ctx.close()
    return (w, opt) + _once(which, make)


def _candidate_cost(which):
    """the cost the solve reports after ONE accepted iteration -- k_cost's (k_solve's) evaluation at the candidate, copied to x_cost
    on acceptance -- against the long-double cost at the device's own candidate states, as
    test_cost_of_the_accepted_step_at_displaced_biases does for the IMU factors alone"""
    w, opt, lin0, lin, s, rep = _one_iteration(which)
    assert rep.iterations == 1 and rep.num_successful_steps == 1 and s["num_successful"] == 1 and s["status"] == 3
    assert rep.final_cost == lin["x_cost"] and rep.final_cost < rep.initial_cost and rep.initial_cost == lin0["x_cost"]
    assert np.array_equal(lin["H"], lin0["H"]) and np.array_equal(lin["g"], lin0["g"])
    cand = dict(pose=s["pose_c"], sb=s["speed_bias_c"], ex=s["ex_pose_c"])
    cost, unit = pr.cost_at(w, opt, cand)
    rho_c = float(abs(LD(rep.final_cost) - cost)) / unit
    print("%s: cost %.6g -> %.6g, rho_cost at the candidate %.3g (bar %.3g)"
          % (which, rep.initial_cost, rep.final_cost, rho_c, pr.bar("cost", which)))
    xc = pr.candidate(which)[6]       # the yardstick's state is the device's candidate up to the rounding of the step
    assert _amax(s["pose_c"][:, :3] - xc["pose"][:, :3]) <= 1e-6 and _amax(s["speed_bias_c"] - xc["sb"]) <= 1e-6
    assert rho_c <= pr.bar("cost", which)
    return w, opt, lin0, s


def test_k_solve_cost_and_gradient_of_the_largest_prior():
    """n = 171 (MAXPN, MAXPB), prior-only, one iteration on the general path: k_solve's inline copy of the prior evaluation gives
    the candidate's cost, and the scaled gradient vpl_ba_debug_step returns is the reference's scale g / diag.  Unit of the
    gradient: (scale / diag) unit(g) + |grad| (4 eps64 + unit(H_ii) / H_ii) -- scale / diag = 1 / sqrt(H_ii) up to a few roundings,
    so the diagonal's relative error enters with a factor 1 / 2 and is counted whole; bar: that of g"""
    w, opt, lin0, s = _candidate_cost("n171u_step")
    assert s["path"] == 1
    ref = pr.Ref(w.prior, _x_dev(lin0))
    scale, D, grad = sr.scaling(ref.H, ref.g)
    dH = np.diag(ref.H)
    unit = (scale / D) * ref.unit_g + np.abs(grad) * (4 * EPS + np.diag(ref.unit_H) / dH)
    rho_grad = pr.rho(s["grad"], grad, unit)
    print("n171u_step: rho_grad %.3g (bar %.3g)" % (rho_grad, pr.bar("g", "n171u")))
    assert rho_grad <= pr.bar("g", "n171u")


def test_k_cost_of_a_prior_beside_the_imu_factors():
    """n = 75 behind step_ref's case a (IMU factors on, no landmark), fast path: cost_body's inline copy of the prior evaluation,
    its register pass over the first 48 columns and its tail, summed with the ten IMU terms; combined units prior_ref + imu_ref"""
    w, opt, lin0, s = _candidate_cost("n75u_imu_step")
    assert s["path"] == 0
