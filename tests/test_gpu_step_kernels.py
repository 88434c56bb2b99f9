"""The trust-region step kernels one by one against the long-double restatement of the same operations (step_ref.py, checked
against the oracle on the CPU by test_step_reference.py): what k_lin / k_lin2 leave as linearisation, what k_step (k_schur +
k_chol + k_back) or k_solve make of it, and what the solve hands back -- read out with vpl_ba_debug_linearization and
vpl_ba_debug_step.  Every window is solved twice without marginalisation: num_iterations = 0 (linearisation) and 1 (step).

Units and bars (rho = error / unit; nothing is tuned to the device):
  4a  x_cost in units eps64 * cost (eps64 sum |terms|), bar 8 x what one ulp of the states does to the float64 cost of the case;
      H, g entrywise in units eps64 sum_f w_f |J_f|^T |J_f| and eps64 sum_f w_f |J_f|^T |r_f| of the reference (w_f = cond2 of the
      covariance for an IMU factor, 1 otherwise); entries with unit 0 are structural zeros and must be 0.0.  Bar: 8 x the
      worst ratio the float64 restatement reaches on the CPU in a shuffled order at states one ulp away (step_ref.YARDSTICK).
  4b  scale, diag, grad, alpha, a1 are a handful of flops on H_dev, g_dev: rho <= 8 in eps64 |value| (sums: eps64 sum |terms|).
  4c  the solve as linear algebra on the device's OWN linearisation: row-wise backward error of A y = b over all rows, bar 8 x
      what a float64 dense Cholesky reaches; a2, a3, dogleg_step_norm in eps64 sum |terms|; model_cost_change directly as
      -(d^T g + d^T H d / 2) in eps64 (sum |d_i g_i| + sum |d_i H_ij d_j| / 2), not through the device's identities; rho <= 8;
      with a prior (gauge pinned) also forward against the reference's step in eps64 cond2(A).
  4d  the candidate against x [+] delta (1e-14 poses, 1e-13 line parameters: the bars of test_parameterisations_parity; plain
      additions 4 eps64 (|x| + |d|)), the downloaded window against the gauge-fixed candidate at 1e-9 relative (the bar of
      test_line_map.py for the same conversion) -- line_plk and the free ex_pose included.

Cases (step_ref.cases(); table in DESIGN.md 2): a no landmark, b one point with two observations, c 5 points + 1 line, d 37 + 11
ragged 6-frame tracks, e tracks of up to 11 frames starting in frames 0..7 (WS = 72) under the three VPL_BA_SCHUR_WIDE
settings, f d's shape with the oracle's prior, g a prior holding a later speed/bias (k_solve), d again under VPL_BA_GENERAL=1
and VPL_BA_STEP_FUSED=0, with the extrinsic held constant, and with three lines not triangulated.  The windows of a setting
share ONE batch in a context of 40 points / 12 lines: strides, padding slots and the window order are in play."""
import numpy as np
import pytest

import step_ref as sr
import vplines_slam_amd as v

pytestmark = pytest.mark.gpu
EPS = sr.EPS64
LD = sr.LD

SETTINGS = sr.SETTINGS
PAIRS = [("default", c) for c in SETTINGS["default"][1]] + [("ex_fixed", "i_ex"), ("general", "d"), ("unfused", "d")] + \
        [(s, c) for s in ("wide_unset", "wide_1", "wide_-1") for c in ("c", "e")]


class Run:
    """what the device did with one window: linearisation read-out (num_iterations = 0), step read-out and the downloaded
    window (num_iterations = 1), and the reference at the device's line parameters"""


_runs, _failed = {}, {}


def _solve_setting(setting):
    env, ids, _ = SETTINGS[setting]
    opt1 = sr.cases()[ids[0]][1]
    assert all(sr.cases()[i][1].estimate_extrinsic == opt1.estimate_extrinsic for i in ids)
    opt0 = sr._options(estimate_extrinsic=opt1.estimate_extrinsic, num_iterations=0)
    with pytest.MonkeyPatch.context() as mp:
        for k, val in env.items():
            mp.setenv(k, val)
        ctx = v.Context(device=0, max_windows=len(ids), max_points=sr.CAP_POINTS, max_point_obs=sr.CAP_POINTS * 11,
                        max_lines=sr.CAP_LINES, max_line_obs=sr.CAP_LINES * 11)
    try:
        w0 = [sr.cases()[i][0].copy() for i in ids]
        ctx.upload(w0, opt0)
        ctx.solve()
        ctx.synchronize()
        lin0 = [ctx.debug_linearization(k) for k in range(len(ids))]
        w1 = [sr.cases()[i][0].copy() for i in ids]
        ctx.upload(w1, opt1)
        ctx.solve()
        ctx.synchronize()
        lin1 = [ctx.debug_linearization(k) for k in range(len(ids))]
        stp = [ctx.debug_step(k) for k in range(len(ids))]
        _, rep = ctx.download()
        for k, case in enumerate(ids):
            r = Run()
            r.lin, r.lin_after, r.step, r.window = lin0[k], lin1[k], stp[k], w1[k]
            r.iterations, r.successful = rep[k].iterations, rep[k].num_successful_steps
            _runs[(setting, case)] = r
    finally:
        ctx.close()       # (raises under VPL_DEBUG_GUARDS=1 when a kernel wrote behind an array)


@pytest.fixture
def run(request):
    setting, case = request.param
    if _failed:
        raise _failed["first"]         # (after a failed solve nothing more of this file is sent to the device)
    if (setting, case) not in _runs:
        try:
            _solve_setting(setting)
        except BaseException as e:
            _failed["first"] = e
            raise
    r = _runs[(setting, case)]
    if not hasattr(r, "ref"):
        prob, x0, _, _ = sr.reference(case)
        r.prob, r.x0 = prob, x0
        r.x_dev = dict(pose=r.lin["pose"], sb=r.lin["speed_bias"], ex=r.lin["ex_pose"], invd=r.lin["inv_depth"], orth=r.lin["line_orth"])
        # the reference at the uploaded states as the kernels take them: quaternions through a rotation matrix (x0 has that), the
        # inverse depths as uploaded, and the DEVICE's line parameters (checked against plk_to_orth in 4a)
        x = dict(x0, invd=prob.w.inv_depth[:prob.nP].copy())
        if prob.nL and r.lin["line_orth"].shape == x0["orth"].shape:
            x["orth"] = r.lin["line_orth"].copy()
        r.ref = prob.linearize(x)
    return r


def _ids(p):
    return "%s-%s" % p


def _ratio(dev, ref):
    """max |dev - ref| / (eps64 |ref|); where the reference is exactly 0 the device has to be too"""
    dev, ref = np.asarray(dev, LD), np.asarray(ref, LD)
    z = ref == 0
    assert np.all(dev[z] == 0), "non-zero where the reference formula gives exactly 0"
    return float((np.abs(dev - ref)[~z] / (EPS * np.abs(ref[~z]))).max()) if (~z).any() else 0.0


def _amax(a):
    return float(np.abs(a).max()) if np.size(a) else 0.0


def _qdiff(a, b):
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return max(min(np.abs(x - y).max(), np.abs(x + y).max()) for x, y in zip(a, b))


@pytest.mark.parametrize("run", PAIRS, ids=_ids, indirect=True)
def test_4a_linearisation(run):
    prob, lin, ref, x0 = run.prob, run.lin, run.ref, run.x0
    assert (lin["n"], lin["n_points"], lin["n_lines"]) == (prob.n, prob.nP, prob.nL)
    assert list(lin["line_index"]) == list(prob.lines)
    # the states the kernels linearised at: the uploaded ones.  Device and reference alike pass the quaternions through a
    # rotation matrix on the way in and the whole state through the (here: identity) gauge fix on the way out, so "equal" is
    # equal up to the rounding of those maps: 8 eps64 |x|, not bit for bit
    assert _amax(run.x_dev["pose"][:, :3] - x0["pose"][:, :3]) <= 8 * EPS * max(1.0, _amax(x0["pose"][:, :3]))
    assert _qdiff(run.x_dev["pose"][:, 3:], x0["pose"][:, 3:]) <= 8 * EPS
    assert _amax(run.x_dev["sb"] - x0["sb"]) <= 8 * EPS * max(1.0, _amax(x0["sb"]))
    assert _amax(run.x_dev["ex"][:3] - x0["ex"][:3]) <= 8 * EPS and _qdiff(run.x_dev["ex"][3:], x0["ex"][3:]) <= 8 * EPS
    assert np.array_equal(run.x_dev["invd"], prob.w.inv_depth[:prob.nP])
    assert run.x_dev["orth"].shape == x0["orth"].shape and _amax(run.x_dev["orth"] - x0["orth"]) <= 1e-12
    # the step kernels read the linearisation, they do not write it
    assert np.array_equal(run.lin_after["H"], lin["H"]) and np.array_equal(run.lin_after["g"], lin["g"])
    H, g = lin["H"], lin["g"]
    assert np.array_equal(H, H.T)
    assert np.all(H[ref.unit_H == 0] == 0.0) and np.all(g[ref.unit_g == 0] == 0.0), "a structural zero is not 0.0 on the device"
    rho_H, rho_g = sr.rho(H, ref.H, ref.unit_H), sr.rho(g, ref.g, ref.unit_g)
    case = run_key(run)[1]
    rho_c = float(abs(LD(lin["x_cost"]) - ref.cost)) / ref.unit_cost
    print("4a rho_H %.3g rho_g %.3g rho_cost %.3g (bars %.3g %.3g %.3g)" % (rho_H, rho_g, rho_c, sr.bar("H"), sr.bar("g"), sr.bar("cost", case)))
    assert rho_H <= sr.bar("H")
    assert rho_g <= sr.bar("g")
    assert rho_c <= sr.bar("cost", case)


@pytest.mark.parametrize("run", PAIRS, ids=_ids, indirect=True)
def test_4b_scaling_and_cauchy_scalars(run):
    H, g, s = run.lin["H"], run.lin["g"], run.step
    scale, D, grad = sr.scaling(H, g)
    r = [_ratio(s["scale"], scale), _ratio(s["diag"], D), _ratio(s["grad"], grad)]
    u = scale * grad / D
    Hl = np.asarray(H, LD)
    q, q_terms = u @ (Hl @ u), (np.abs(u)[:, None] * np.abs(Hl) * np.abs(u)[None, :]).sum()
    a1 = grad @ grad
    alpha = a1 / q
    r_a1 = float(abs(LD(s["a1"]) - a1) / (EPS * a1))
    r_alpha = float(abs(LD(s["alpha"]) - alpha) / (EPS * alpha * (1 + q_terms / q)))
    print("4b rho scale %.3g diag %.3g grad %.3g a1 %.3g alpha %.3g" % (r[0], r[1], r[2], r_a1, r_alpha))
    assert max(r) <= 8 and r_a1 <= 8 and r_alpha <= 8


@pytest.mark.parametrize("run", PAIRS, ids=_ids, indirect=True)
def test_4c_gauss_newton_step_as_linear_algebra(run):
    setting, case = run_key(run)
    H, g, s = np.asarray(run.lin["H"], LD), np.asarray(run.lin["g"], LD), run.step
    scale, D, grad, gn = (np.asarray(s[k], LD) for k in ("scale", "diag", "grad", "gn"))
    assert s["path"] == (1 if setting == "general" or case == "g" else 0)
    # the step was valid: k_cost evaluated and accepted it (it clears step_valid when it has consumed the candidate, so after a
    # solve the flag itself reads 0); an invalid step is never evaluated and leaves mu multiplied by 10
    assert s["mu"] == 1e-8 and s["iter"] == 1 and s["num_successful"] == 1 and s["status"] == 3 and s["step_valid"] == 0
    assert s["model_cost_change"] > 0.0
    assert run.iterations == 1 and run.successful == 1
    A = scale[:, None] * H * scale[None, :] + np.diag(LD(1e-8) * D * D)
    b = scale * g
    y = -gn / D
    om = sr.omega(A, y, b)
    fin = sr.finish(H, g, scale, D, grad, gn, s["alpha"])
    assert fin["branch"] == "gauss-newton"
    r_a2 = float(abs(LD(s["a2"]) - fin["a2"]) / (EPS * fin["a2"]))
    r_a3 = float(abs(LD(s["a3"]) - fin["a3"]) / (EPS * np.abs(grad * gn).sum()))
    r_dn = float(abs(LD(s["dogleg_step_norm"]) - fin["dogleg_step_norm"]) / (EPS * fin["dogleg_step_norm"]))
    # (the device forms y^T H_s y as -a3 - mu a2, exact only when A y = b; at its backward error that identity costs nothing
    # that shows: the plain unit holds)
    r_mcc = float(abs(LD(s["model_cost_change"]) - fin["model_cost_change"]) / (EPS * fin["mcc_terms"]))
    print("4c omega %.3g (bar %.3g) rho a2 %.3g a3 %.3g dogleg_step_norm %.3g model_cost_change %.3g"
          % (om, sr.bar("omega", case), r_a2, r_a3, r_dn, r_mcc))
    assert om <= sr.bar("omega", case)
    assert r_a2 <= 8 and r_a3 <= 8 and r_dn <= 8
    assert r_mcc <= 8
    if case in ("f", "g"):      # the prior pins the gauge: the step itself is determined to eps64 cond2(A)
        st = sr.step(run.ref.H, run.ref.g, run.ref.J)
        lv = sr.live(run.ref.H)
        gn_ref = np.asarray(st["gn"], LD)
        fw = float(np.sqrt(((gn - gn_ref) ** 2).sum()) / (EPS * sr.cond2(st["A"][np.ix_(lv, lv)]) * np.sqrt((gn_ref ** 2).sum())))
        print("4c forward |gn_dev - gn_ref| / (eps64 cond2 |gn_ref|) = %.3g (bar %.3g)" % (fw, sr.bar("gn", case)))
        assert fw <= sr.bar("gn", case)


@pytest.mark.parametrize("run", PAIRS, ids=_ids, indirect=True)
def test_4d_candidate_and_hand_back(run):
    prob, s, x = run.prob, run.step, run.x_dev
    assert run.iterations == 1 and run.successful == 1
    fin = sr.finish(run.lin["H"], run.lin["g"], s["scale"], s["diag"], s["grad"], s["gn"], s["alpha"])
    d = np.asarray(fin["delta"], np.float64)
    want = prob.plus(x, d)
    assert _amax(s["pose_c"] - want["pose"]) <= 1e-14
    assert _amax(s["ex_pose_c"] - want["ex"]) <= 1e-14
    if not prob.ex_free:
        assert np.array_equal(s["ex_pose_c"], x["ex"])
    dsb = np.stack([d[15 * f + 6:15 * f + 15] for f in range(sr.NF)])
    assert np.all(np.abs(s["speed_bias_c"] - want["sb"]) <= 4 * EPS * (np.abs(x["sb"]) + np.abs(dsb)))
    assert np.all(np.abs(s["inv_depth_c"] - want["invd"]) <= 4 * EPS * (np.abs(x["invd"]) + np.abs(d[sr.NC:sr.NC + prob.nP])))
    assert _amax(s["line_orth_c"] - want["orth"]) <= 1e-13
    # what the solve hands back: the accepted candidate through the gauge fix, lines into their start camera frame
    cand = dict(pose=s["pose_c"], sb=s["speed_bias_c"], ex=s["ex_pose_c"], invd=s["inv_depth_c"], orth=s["line_orth_c"])
    hb, w = prob.hand_back(cand), run.window
    rel = lambda a, ref: _amax(a - ref) <= 1e-9 * _amax(ref)
    assert rel(w.pose[:, :3], hb["pose"][:, :3])
    assert _qdiff(w.pose[:, 3:], hb["pose"][:, 3:]) <= 1e-9
    assert rel(w.speed_bias, hb["sb"])
    assert rel(w.ex_pose[:3], hb["ex"][:3]) and _qdiff(w.ex_pose[3:], hb["ex"][3:]) <= 1e-9
    if prob.nP:
        assert rel(w.inv_depth, hb["invd"])
    for dl, l in enumerate(prob.lines):
        assert rel(w.line_plk[l], hb["plk"][dl]), (dl, l)
    gone = np.setdiff1d(np.arange(len(w.line_start)), prob.lines)
    assert np.array_equal(w.line_plk[gone], prob.w.line_plk[gone])


def run_key(run):
    return next(k for k, r in _runs.items() if r is run)
