"""The IMU factors of a window's linearisation against the long-double IMU factor (imu_ref.py, checked against the oracle and the
device math on the CPU by test_imu_reference.py): what k_prep's whitening (wave_chol16 -> X^T X -> wave_chol16), lin_imu_raw,
lin_imu_whiten, lin_imu_cost and the IMU part of lin_assemble leave in H, g and x_cost, read out with
vpl_ba_debug_linearization after a solve of zero iterations, and k_cost's IMU evaluation after one iteration.

Units and bars (rho = error / unit; nothing is tuned to the device).  J^T P J, J^T P r and r^T P r / 2 of a factor do not depend
on the square root of P = cov^-1 that whitened it, so they are compared with their long-double values in imu_ref's units
(eps64 k_f a a^T, eps64 k_f a b, eps64 k_f b^2 / 2 from the Jacobi-scaled covariance, entrywise never above step_ref's
eps64 cond2(cov) |J_w|^T |J_w|); a window's unit is the sum over its factors.  Bar: 8 x max(yardstick, 1), the yardstick being what
the float64 restatement of the device's path reaches on the CPU in a shuffled order at states one ulp away (imu_ref.YARDSTICK).
Entries with unit 0 are structural zeros and must be 0.0.  A relative error of 1e-9 of one block of the raw Jacobian is beyond these
bars (test_imu_reference.py::test_sharpness_of_the_bars); 4a of test_gpu_step_kernels.py needs ~1e-5.

Cases (imu_ref.cases(); table in DESIGN.md 2): m0 no landmark, nothing displaced; m1 biases 0.02 / 0.005 off the pre-integrations'
linearisation point and stepping from frame to frame; m2 intervals of 0.2, 0.06 and 0.04 s among the 0.1 s ones; m3 = m1 with one
factor skipped (sum_dt > 10); m4 = 5 points + 1 line + VP with m1's biases; m5 = 37 + 11 with the oracle's prior and m1's biases.
All of them share ONE batch (step_ref's case d between them) in a context of 40 points / 12 lines, once per setting of
VPL_BA_LIN_SPLIT: unset, 0 (one work-group per window) and 1 (lin_body<0, 2> does the IMU phases in a second work-group)."""
import numpy as np
import pytest

import imu_ref as ir
import step_ref as sr
import vplines_slam_amd as v

pytestmark = pytest.mark.gpu
EPS = sr.EPS64
LD = sr.LD

SETTINGS = {"unset": {}, "split0": {"VPL_BA_LIN_SPLIT": "0"}, "split1": {"VPL_BA_LIN_SPLIT": "1"}}
BATCH = ["m0", "m1", "d", "m2", "m3", "m4", "m5"]          # upload order; d is step_ref's, between the IMU cases
BASE = {"m4": "c", "m5": "f"}                                # the step_ref case whose visual part a case has
_lin, _solve, _failed = {}, {}, {}


def _window(case):
    return (sr.cases() if case == "d" else ir.cases())[case][0].copy()


def _context(setting):
    with pytest.MonkeyPatch.context() as mp:
        for k, val in SETTINGS[setting].items():
            mp.setenv(k, val)
        return v.Context(device=0, max_windows=len(BATCH), max_points=sr.CAP_POINTS, max_point_obs=sr.CAP_POINTS * 11,
                         max_lines=sr.CAP_LINES, max_line_obs=sr.CAP_LINES * 11)


def _run_setting(setting):
    """one context per setting: the whole batch with num_iterations = 0; in the unset setting also one iteration of [c, m1]"""
    ctx = _context(setting)
    try:
        ctx.upload([_window(c) for c in BATCH], sr._options(num_iterations=0))
        ctx.solve()
        ctx.synchronize()
        for k, c in enumerate(BATCH):
            _lin[(setting, c)] = ctx.debug_linearization(k)
        if setting == "unset":
            ws = [sr.cases()["c"][0].copy(), _window("m1")]
            ctx.upload(ws, sr._options())
            ctx.solve()
            ctx.synchronize()
            _solve["lin"], _solve["step"] = ctx.debug_linearization(1), ctx.debug_step(1)
            _solve["report"] = ctx.download()[1][1]
    finally:
        ctx.close()       # (raises under VPL_DEBUG_GUARDS=1 when a kernel wrote behind an array)


def _get(setting):
    if _failed:
        raise _failed["first"]         # (after a failed solve nothing more of this file is sent to the device)
    if (setting, BATCH[0]) not in _lin:
        try:
            _run_setting(setting)
        except BaseException as e:
            _failed["first"] = e
            raise


@pytest.fixture
def lin(request):
    setting, case = request.param
    _get(setting)
    return setting, case, _lin[(setting, case)]


def _amax(a):
    return float(np.abs(a).max()) if np.size(a) else 0.0


def _qdiff(a, b):
    return max(min(np.abs(x - y).max(), np.abs(x + y).max()) for x, y in zip(np.atleast_2d(a), np.atleast_2d(b)))


def _states_are_the_uploaded_ones(d, pose, sb):
    """as 4a: equal up to the rounding of the quaternion -> matrix -> quaternion map and the identity gauge fix"""
    assert _amax(d["pose"][:, :3] - pose[:, :3]) <= 8 * EPS * max(1.0, _amax(pose[:, :3]))
    assert _qdiff(d["pose"][:, 3:], pose[:, 3:]) <= 8 * EPS
    assert _amax(d["speed_bias"] - sb) <= 8 * EPS * max(1.0, _amax(sb))


PAIRS = [(s, c) for s in SETTINGS for c in ir.cases()]


@pytest.mark.parametrize("lin", [p for p in PAIRS if p[1] in ir.IMU_ONLY], ids=lambda p: "%s-%s" % p, indirect=True)
def test_imu_only_window(lin):
    setting, case, d = lin
    w, opt, pose, sb, ref = ir.reference(case)
    assert (d["n"], d["n_points"], d["n_lines"]) == (171, 0, 0)
    _states_are_the_uploaded_ones(d, pose, sb)
    H, g = d["H"], d["g"]
    assert np.array_equal(H, H.T)
    assert np.all(H[165:, :] == 0.0) and np.all(g[165:] == 0.0)            # nothing touches the extrinsic
    Hc, gc = H[:165, :165], g[:165]
    assert np.all(Hc[ref.unit_H == 0] == 0.0) and np.all(gc[ref.unit_g == 0] == 0.0), "a structural zero is not 0.0 on the device"
    if case == "m3":       # the skipped factor 6 (frames 5 | 6) contributes nothing: no coupling, and the window falls apart there
        assert np.all(Hc[81:90, 96:105] == 0.0) and np.all(Hc[:90, 90:] == 0.0)
        assert np.all(ref.unit_H[:90, 90:] == 0) and float(ir.reference("m1")[4].cost - ref.cost) > 1e3 * ref.unit_cost
    rH, rg, rc = ir.rho3(Hc, gc, d["x_cost"], ref)
    print("%s %s rho_H %.3g rho_g %.3g rho_cost %.3g (bars %.3g %.3g %.3g)"
          % (setting, case, rH, rg, rc, ir.bar("H", case), ir.bar("g", case), ir.bar("cost", case)))
    assert rH <= ir.bar("H", case)
    assert rg <= ir.bar("g", case)
    assert rc <= ir.bar("cost", case)


@pytest.mark.parametrize("lin", [p for p in PAIRS if p[1] in BASE], ids=lambda p: "%s-%s" % p, indirect=True)
def test_window_with_landmarks_or_prior(lin):
    """m4, m5.  Reference and units: imu_ref.Combined -- step_ref's linearisation of the window with its IMU rows (the oracle's
    float64 whitened evaluator) taken out and the long-double IMU share put in; step_ref's unit of the remaining rows + the IMU
    unit.  The speed/bias rows and columns 15 f + 6 .. 15 f + 14 see only IMU factors and the prior: bar 8 x max(IMU yardstick, 1).
    The other entries also carry the visual factors, whose one-ulp-of-the-states uncertainty step_ref.YARDSTICK records: its bar.
    The cost: unit = IMU cost unit + eps64 x the rest of the cost, bar = the larger of the two parts' bars (an error within
    bar_i unit_i of each part is within max(bar_i) of the summed unit)."""
    setting, case, d = lin
    w, opt, pose, sb, share = ir.reference(case)
    ref = ir.Combined(case, orth=d["line_orth"])       # (at the device's line parameters, as test_gpu_step_kernels.py does)
    prob = ref.prob
    assert (d["n"], d["n_points"], d["n_lines"]) == (prob.n, prob.nP, prob.nL)
    _states_are_the_uploaded_ones(d, pose, sb)
    assert d["line_orth"].shape == ref.x0["orth"].shape and _amax(d["line_orth"] - ref.x0["orth"]) <= 1e-12
    H, g = d["H"], d["g"]
    assert np.array_equal(H, H.T)
    assert np.all(H[ref.unit_H == 0] == 0.0) and np.all(g[ref.unit_g == 0] == 0.0), "a structural zero is not 0.0 on the device"
    r_sbH, r_sbg, r_H, r_g, r_c = ref.rhos(H, g, d["x_cost"])
    bar_c = max(ir.bar("cost", case), sr.bar("cost", BASE[case]))
    print("%s %s speed/bias rho_H %.3g rho_g %.3g (bars %.3g %.3g); rest rho_H %.3g rho_g %.3g (bars %.3g %.3g); rho_cost %.3g (bar %.3g)"
          % (setting, case, r_sbH, r_sbg, ir.bar("H", case), ir.bar("g", case), r_H, r_g, sr.bar("H"), sr.bar("g"), r_c, bar_c))
    assert r_sbH <= ir.bar("H", case)
    assert r_sbg <= ir.bar("g", case)
    assert r_H <= sr.bar("H") and r_g <= sr.bar("g")
    assert r_c <= bar_c


def test_the_settings_agree_bit_for_bit():
    """VPL_BA_LIN_SPLIT unset, 0 and 1: one or two work-groups per window leave the same linearisation, d's included"""
    for s in SETTINGS:
        _get(s)
    for c in BATCH:
        a = _lin[("unset", c)]
        for s in ("split0", "split1"):
            b = _lin[(s, c)]
            for k in ("H", "g", "pose", "speed_bias", "ex_pose", "inv_depth", "line_orth"):
                assert np.array_equal(a[k], b[k]), (c, s, k)
            assert a["x_cost"] == b["x_cost"], (c, s)


def test_cost_of_the_accepted_step_at_displaced_biases():
    """One iteration of m1 (second window of a batch behind step_ref's case c).  The step is accepted, so the cost the solve
    reports (report.final_cost = tr.x_cost) is the candidate's cost: k_cost (cost_body, ba_solve.h) evaluated it at the
    candidate states pose_c / sb_c -- raw residuals by imu_residual_raw, whitened with k_prep's sqrt_info -- and copied it to
    x_cost when it accepted.  It is held to the long-double r^T P r / 2 at the candidate as vpl_ba_debug_step reads it out, which
    the acceptance makes the state the solve hands back, in the cost unit of that state.  Bar: 8 x the yardstick AT THE
    CANDIDATE (imu_ref.yardstick_step: the reference's candidate, cost 10 after 6.8e5): there the unit eps k_f b^2 / 2 has shrunk
    with the square of the residuals, the rounding of the raw residuals -- eps x positions of metres -- with their first power,
    and the float64 restatement is at 54 units on the very same inputs, at 90 .. 440 one ulp away.  The only check of k_cost's IMU
    evaluation at dba, dbg != 0."""
    _get("unset")
    d, s, rep = _solve["lin"], _solve["step"], _solve["report"]
    w, opt, pose, sb, ref0 = ir.reference("m1")
    assert rep.iterations == 1 and rep.num_successful_steps == 1 and s["num_successful"] == 1 and s["status"] == 3
    assert rep.final_cost == d["x_cost"] and rep.final_cost < rep.initial_cost
    lin0 = _lin[("unset", "m1")]
    assert np.array_equal(d["H"], lin0["H"]) and np.array_equal(d["g"], lin0["g"]) and rep.initial_cost == lin0["x_cost"]
    assert np.all(s["speed_bias_c"][:, 3:9] != sb[:, 3:9]), "the step does not move a bias"
    ref = ir.Share(w, s["pose_c"], s["speed_bias_c"], opt.g_norm)
    r_c = float(abs(LD(rep.final_cost) - ref.cost)) / ref.unit_cost
    print("k_cost at the candidate of m1: cost %.6g -> %.6g, rho_cost %.3g (bar %.3g)"
          % (rep.initial_cost, rep.final_cost, r_c, ir.bar("cost", "m1_step")))
    cand = ir.candidate("m1")       # the yardstick's state is the device's candidate up to the rounding of the step
    assert _amax(s["pose_c"][:, :3] - cand[2][:, :3]) <= 1e-6 and _amax(s["speed_bias_c"] - cand[3]) <= 1e-6
    assert r_c <= ir.bar("cost", "m1_step")
