"""The point, line and VP factors and the two parameterisations on the device against vis_ref.py's long-double values (checked on
the CPU by test_vis_reference.py): the evaluators behind the C ABI on every case of DESIGN.md 2, k_lin's point and line phases
through the linearisation of the windows c, d, e and c_edge, k_cost's visual evaluation (Huber included) through the cost of
c_edge's first step, and k_line_opt's evaluator in its three lane layouts through the first cost of onlyLineOpt.

Units and bars (rho = error / unit; nothing is tuned to the device or the oracle).  Evaluators: unit of an entry = eps64 |value| +
what rounding each input alone does to it, in long double; bar = 8 x max(what vis_ref's own float64 run reaches on the case, 1)
(vis_ref.YARDSTICK).  Entries with unit 0 are structural zeros and must be 0.0.  Windows: step_ref's units of H, g and the cost;
bar = 8 x max(the float64 assembly of vis_ref's float64 factors in a shuffled order at states one ulp away, 1)
(vis_ref.YARDSTICK_WINDOW).  line_orth_plus is compared as orth_to_plk of its output, normalised, up to the common sign."""
import numpy as np
import pytest

import step_ref as sr
import vis_ref as vr
import vplines_slam_amd as v

pytestmark = pytest.mark.gpu
LD = sr.LD
EPS = sr.EPS64
BLOCK = 64                   # threads per block of the k_eval_* launches (vplines_ba.hip: dim3((n + 63) / 64), dim3(64))
_failed, _win = {}, {}


def _guard(f, *a, **kw):
    """after a failed device call nothing more of this file is sent to the device"""
    if _failed:
        raise _failed["first"]
    try:
        return f(*a, **kw)
    except BaseException as e:
        _failed["first"] = e
        raise


def _device(ctx, kind, X, want_jac=True):
    X = np.ascontiguousarray(X)
    if kind in ("proj", "line", "vp"):
        f, k = {"proj": (ctx.projection_factor, 22), "line": (ctx.line_factor, 18), "vp": (ctx.vp_factor, 18)}[kind]
        r, jac = _guard(f, X[:, :k], X[:, k:], want_jac=want_jac)
        return np.concatenate([r, jac], axis=1) if want_jac else r
    f, k = {"pose_plus": (ctx.pose_plus, 7), "orth_plus": (ctx.line_orth_plus, 4)}[kind]
    return _guard(f, X[:, :k], X[:, k:])


@pytest.mark.parametrize("kind", ["proj", "line", "vp", "pose_plus", "orth_plus"])
def test_evaluator_on_every_case(gpu_ctx, kind):
    """one call with the cases concatenated; then n = 1, and n = one more than a block with an edge case in the tail lane"""
    X, where = vr.by_kind(kind)
    assert len(X) <= 300
    out = _device(gpu_ctx, kind, X)
    assert out.shape[0] == len(X) and np.all(np.isfinite(out))
    late = []
    for name, m0, m in where:
        _, _, ref, unit, _, rho64 = vr.evaluated(name)
        o = out[m0:m0 + m]
        if kind != "orth_plus":
            assert np.all(o[unit == 0] == 0.0), "%s: a structural zero is not 0.0 on the device" % name
        got = vr.split(kind, vr.rho_rows(kind, o, ref, unit))
        y = vr.split(kind, rho64)
        for what, val in got.items():
            print("%s %s rho %.3g (bar %.3g; float64 restatement %.3g)" % (name, what, val, vr.bar(name, what), y[what]))
            if not val <= vr.bar(name, what):
                late.append((name, what, val, vr.bar(name, what)))
        if name in vr.GENERIC and kind == "orth_plus":        # the angles themselves where they are determined
            assert np.abs(o - np.asarray(vr.run(kind, X[m0:m0 + m]), np.float64)).max() <= 1e-13
    assert not late, late
    if kind in ("proj", "line", "vp"):
        assert np.array_equal(_device(gpu_ctx, kind, X, want_jac=False), out[:, :2]), "want_jac = False changes the residual"
    # n = 1; n = BLOCK + 1: a second block of one lane, holding the last edge case
    name, m0, m = where[-1]
    _, _, ref, unit, _, _ = vr.evaluated(name)
    tail = np.concatenate([np.resize(X[:where[0][2]], (BLOCK, X.shape[1])), X[-1:]])
    for Y, row in ((X[-1:], 0), (tail, BLOCK)):
        o = _device(gpu_ctx, kind, Y)
        assert o.shape[0] == len(Y)
        got = vr.split(kind, vr.rho_rows(kind, o[row:row + 1], ref[-1:], unit[-1:]))
        print("%s n = %d, last lane: %s" % (name, len(Y), vr._fmt(got)))
        assert all(val <= vr.bar(name, what) for what, val in got.items()), (name, len(Y), got)
        assert np.array_equal(o[row], out[-1]), "the same factor gives other bits in another lane"
        assert np.array_equal(o[:row], out[np.arange(row) % where[0][2]])


# ---- the visual share of a window's H, g and cost --------------------------------------------------------------------------
BATCH = ["c", "d", "c_edge"]         # e goes alone: its tracks of 11 observations set the width of a batch's rows


def _context(max_windows, max_lines=sr.CAP_LINES):
    return v.Context(device=0, max_windows=max_windows, max_points=sr.CAP_POINTS, max_point_obs=sr.CAP_POINTS * 11,
                     max_lines=max_lines, max_line_obs=max_lines * 11)


def _window(case):
    return vr.window_cases()[case][0].copy()


def _run_windows():
    ctx = _context(len(BATCH))
    try:
        for batch in (BATCH, ["e"]):
            ctx.upload([_window(c) for c in batch], sr._options(num_iterations=0))
            ctx.solve()
            ctx.synchronize()
            for k, c in enumerate(batch):
                _win[c] = ctx.debug_linearization(k)
        ctx.upload([_window("c_edge")], sr._options())
        ctx.solve()
        ctx.synchronize()
        _win["step_lin"], _win["step"] = ctx.debug_linearization(0), ctx.debug_step(0)
        _win["report"] = ctx.download()[1][0]
    finally:
        ctx.close()


def _windows():
    if "report" not in _win:
        _guard(_run_windows)
    return _win


@pytest.mark.parametrize("case", vr.WINDOW_CASES)
def test_linearisation_against_long_double_factors(case):
    """debug_linearization after a solve of zero iterations: k_lin's point and line phases (and the IMU phase the other tests
    hold) against the window linearised with vis_ref's long-double factors at the device's own line parameters"""
    d = _windows()[case]
    w, opt = vr.window_cases()[case]
    prob, x, ref = vr.reference(case, orth=d["line_orth"], invd=w.inv_depth[:len(w.point_start)])
    assert (d["n"], d["n_points"], d["n_lines"]) == (prob.n, prob.nP, prob.nL)
    x0 = prob.initial_state()
    assert d["line_orth"].shape == x0["orth"].shape and np.abs(d["line_orth"] - x0["orth"]).max() <= 1e-12
    assert np.array_equal(d["inv_depth"], x["invd"])
    H, g = d["H"], d["g"]
    assert np.array_equal(H, H.T)
    assert np.all(H[ref.unit_H == 0] == 0.0) and np.all(g[ref.unit_g == 0] == 0.0), "a structural zero is not 0.0 on the device"
    got = dict(H=sr.rho(H, ref.H, ref.unit_H), g=sr.rho(g, ref.g, ref.unit_g), cost=float(abs(LD(d["x_cost"]) - ref.cost)) / ref.unit_cost)
    print("%s k_lin %s bars %s" % (case, vr._fmt(got), vr._fmt({k: vr.bar_window(case, k) for k in got})))
    for k, val in got.items():
        assert val <= vr.bar_window(case, k), (case, k, val)


def test_cost_of_c_edge_after_one_iteration():
    """k_cost's visual evaluation, Huber's two branches included: the cost the solve reports for the accepted step of c_edge is the
    cost at the candidate debug_step reads out; held to the long-double cost there in eps64 x cost, bar 8 x the yardstick at the
    reference's candidate (c_edge_step).  Were the step rejected, that is asserted and the initial cost alone is checked."""
    win = _windows()
    rep, s, lin0 = win["report"], win["step"], win["c_edge"]
    w, opt = vr.window_cases()["c_edge"]
    assert rep.iterations == 1 and rep.initial_cost == lin0["x_cost"]
    if rep.num_successful_steps != 1:
        assert s["num_successful"] == 0 and rep.final_cost == rep.initial_cost
        return
    assert s["num_successful"] == 1 and rep.final_cost == win["step_lin"]["x_cost"] and rep.final_cost < rep.initial_cost
    prob = vr.problem("c_edge")
    xc = dict(pose=s["pose_c"], sb=s["speed_bias_c"], ex=s["ex_pose_c"], invd=s["inv_depth_c"], orth=s["line_orth_c"])
    ref = prob.linearize(xc)
    first = np.concatenate([[0], np.cumsum(np.asarray(w.point_nobs) - 1)]).astype(int)
    assert ref.sq[first[vr.EDGE["huber"]]] > opt.huber_delta ** 2 > ref.sq[first[vr.EDGE["huber"]] + 1], "one branch of Huber is not taken"
    rho = float(abs(LD(rep.final_cost) - ref.cost)) / ref.unit_cost
    print("k_cost at the candidate of c_edge: cost %.6g -> %.6g, rho_cost %.3g (bar %.3g)"
          % (rep.initial_cost, rep.final_cost, rho, vr.bar("c_edge_step", "cost")))
    cand = vr.candidate("c_edge")[1]          # the yardstick's state is the device's candidate up to the rounding of the step
    assert np.abs(s["pose_c"][:, :3] - cand["pose"][:, :3]).max() <= 1e-6 and np.abs(s["inv_depth_c"] - cand["invd"]).max() <= 1e-6
    assert rho <= vr.bar("c_edge_step", "cost")


# max_lines of the context -> lanes per line of the k_line_opt launch (vplines_ba.hip launch_line_opt, LOPT_THREADS = 256):
# 4 * 12 <= 256: G = 4;  4 * 100 > 256 >= 2 * 100: G = 2;  2 * 200 > 256: G = 1
LANES = {12: 4, 100: 2, 200: 1}


@pytest.mark.parametrize("max_lines", list(LANES))
def test_line_opt_first_cost_in_every_lane_layout(max_lines):
    """lopt_eval<G>: case e's 6 triangulated lines with tracks of 5 .. 11 through onlyLineOpt with num_iterations = 0; the initial
    cost against the long-double sum of log(1 + s) / 2 over vis_ref.line at the world orth of the uploaded Pluecker lines"""
    assert LANES[max_lines] == (4 if 4 * max_lines <= 256 else 2 if 2 * max_lines <= 256 else 1)
    w, opt = vr.window_cases()["e"]
    P, O = vr.line_opt_rows(w, opt)
    ref = vr.line_opt_cost(P, O, opt.line_factor)

    def run():
        ctx = _context(1, max_lines)
        try:
            return ctx.only_line_opt([w.copy()], sr._options(num_iterations=0))[0]
        finally:
            ctx.close()
    rep = _guard(run)
    assert rep.iterations == 0
    rho = float(abs(LD(rep.initial_cost) - ref) / (EPS * ref))
    print("k_line_opt<%d>: initial cost %.9g, rho %.3g (bar %.3g)" % (LANES[max_lines], rep.initial_cost, rho, vr.bar("line_opt", "cost")))
    assert rho <= vr.bar("line_opt", "cost")
