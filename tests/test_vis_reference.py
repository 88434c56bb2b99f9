"""vis_ref.py -- the point, line and VP factors, the parameterisations and the losses in long double -- checked on the CPU: against
central differences of its own residuals, against the literal matrix chain of the VP factor, and the oracle's float64 evaluators
held to it in vis_ref's units on every case of DESIGN.md 2.  Bars: vis_ref.bar = 8 x max(the float64 run of vis_ref itself, 1) per
case; nothing is tuned to the oracle or the device."""
import numpy as np
import pytest

import oracle_api as o
import step_ref as sr
import vis_ref as vr

LD = sr.LD
EPS_LD = float(np.finfo(LD).eps)
H_FD = LD(1e-8)


def _oracle(kind, X):
    if kind == "proj":
        return np.concatenate(o.projection_factor(X[:, :22], X[:, 22:]), axis=1)
    if kind == "line":
        return np.concatenate(o.line_factor(X[:, :18], X[:, 18:]), axis=1)
    if kind == "vp":
        return np.concatenate(o.vp_factor(X[:, :18], X[:, 18:]), axis=1)
    if kind == "pose_plus":
        return o.pose_plus(X[:, :7], X[:, 7:])
    if kind == "orth_plus":
        return o.line_orth_plus(X[:, :4], X[:, 4:])
    if kind == "plk_to_orth":
        return np.stack([o.plk_to_orth(x) for x in X])
    return np.stack([o.orth_to_plk(x) for x in X])


def test_every_case_is_finite_in_both_runs():
    assert len(vr.cases()) == len(vr.YARDSTICK) - 1
    for name in vr.cases():
        kind, X, ref, unit, out64, rho = vr.evaluated(name)
        assert np.all(np.isfinite(X)) and np.all(np.isfinite(np.asarray(ref, np.float64))), name
        assert np.all(np.isfinite(out64)) and np.all(np.isfinite(unit)) and np.all(np.isfinite(rho)), name
        assert np.all(np.isfinite(np.asarray(vr.run(kind, X), np.float64))), name
    # structural zeros, and only they, have unit 0 in a generic case
    for name, zeros in (("p_generic", [8, 15, 22, 29, 36, 43]), ("l_generic", [8, 15, 22, 29]),
                        ("v_generic", [2, 3, 4, 8, 9, 10, 11, 15, 16, 17, 18, 22, 23, 24, 25, 29, 31, 35])):
        unit = vr.evaluated(name)[3]
        assert np.array_equal(np.nonzero(np.all(unit == 0, axis=0))[0], zeros) and not np.any(np.delete(unit, zeros, axis=1) == 0), name


def test_q_and_minus_q_give_the_same_bits():
    for name, sl in (("p_neg_qi", slice(3, 7)), ("p_neg_qj", slice(10, 14)), ("p_neg_qic", slice(17, 21))):
        kind, X = vr.cases()[name]
        Y = X.copy()
        Y[:, sl] = -Y[:, sl]
        for dt in (LD, np.float64):
            assert np.array_equal(vr.run(kind, X, dt), vr.run(kind, Y, dt)), name


def _local(kind, jac):
    """[2, nloc] local columns of an evaluator's Jacobian [44] / [36]"""
    cols = [jac[0:14].reshape(2, 7)[:, :6], jac[14:28].reshape(2, 7)[:, :6]]
    cols += [jac[28:42].reshape(2, 7)[:, :6], jac[42:44].reshape(2, 1)] if kind == "proj" else [jac[28:36].reshape(2, 4)]
    return np.concatenate(cols, axis=1)


BLOCKS = {"proj": [(slice(0, 7), "pose"), (slice(7, 14), "pose"), (slice(14, 21), "pose"), (slice(21, 22), "add")],
          "line": [(slice(0, 7), "pose"), (slice(7, 14), "pose"), (slice(14, 18), "orth")]}
# where the analytic Jacobian is not the derivative through the parameterisation, or that map is not smooth at the point
NOT_SMOOTH = {
    "p_q_norm_1+1e-6": "all",       # the reference's Jacobians are derivatives at unit quaternions only (toRotationMatrix of a
                                    # quaternion of norm 1 + 1e-6 is 1 + 2e-6 times a rotation; q * v and inverse() are not)
    "l_orth1_+pi/2": "orth", "l_orth1_-pi/2": "orth",      # line_orth_plus goes through asin(-u1.z) at |u1.z| = 1 - 5e-17
    "l_origin_1e-3": "orth",        # and through asin(W10) at W10 = 1 - 5e-7
}


def _central(f, x, blocks, h):
    """central differences of f with step h through pose_plus / line_orth_plus / + -> [2, nloc] (long double)"""
    cols = []
    for sl, how in blocks:
        nloc = {"pose": 6, "orth": 4, "add": 1}[how]
        for k in range(nloc):
            def at(t):
                d = np.zeros(nloc, LD)
                d[k] = t
                xp = x.copy()
                if how == "pose":
                    xp[sl] = vr._pose_plus1(np.concatenate([x[sl], d]), LD)
                elif how == "orth":
                    xp[sl] = vr._orth_plus1(np.concatenate([x[sl], d]), LD)
                else:
                    xp[sl] = x[sl] + d
                return f(xp)
            cols.append((at(h) - at(-h)) / (2 * h))
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("kind", ["proj", "line"])
def test_jacobians_are_central_differences_of_the_residual(kind):
    """Every true derivative, in long double, step h = 1e-8.  D(h) = f' + h^2 f''' / 6 + O(h^4), so D(2h) - D(h) = h^2 f''' / 2 is
    three times the truncation term of D(h), measured from the residual alone: the bar is |D(2h) - D(h)| entrywise, plus the
    rounding of the difference quotient, 256 eps_ld max(|r|, |J|) / h (3e-9 of the largest entry).  All cases but the blocks
    NOT_SMOOTH names."""
    f1 = {"proj": vr._proj1, "line": vr._line1}[kind]
    si = vr.SQRT_INFO[kind]
    worst = 0.0
    for name, (k, X) in vr.cases().items():
        if k != kind or NOT_SMOOTH.get(name) == "all":
            continue
        blocks = [b for b in BLOCKS[kind] if NOT_SMOOTH.get(name) != b[1]]
        keep = np.concatenate([np.full({"pose": 6, "orth": 4, "add": 1}[b[1]], NOT_SMOOTH.get(name) != b[1]) for b in BLOCKS[kind]])
        for x in X[:8]:
            x = np.asarray(x, LD)
            f = lambda xp: f1(xp, si, LD, want_jac=False)
            out = f1(x, si, LD)
            J = _local(kind, out[2:])[:, keep]
            D1, D2 = _central(f, x, blocks, H_FD), _central(f, x, blocks, 2 * H_FD)
            bar = np.abs(D2 - D1) + 256 * EPS_LD * max(np.abs(out[:2]).max(), np.abs(J).max()) / H_FD
            ratio = float((np.abs(J - D1) / bar).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, ratio)
    print("%s: worst |J - D(h)| / bar %.3g" % (kind, worst))


def test_vp_jacobian_is_the_literal_chain():
    """the VP Jacobian is no derivative (line_projection_factor.cpp:62-64): residual and pose / extrinsic / orth blocks against
    the chain written out block by block, as test_vp_factor_matches_literal_formula does it, in long double"""
    for name, (kind, X) in vr.cases().items():
        if kind != "vp":
            continue
        for x in X:
            x = np.asarray(x, LD)
            out = vr._vp1(x, 10.0, LD)
            twb, Rwb, tbc, Rbc, Lw, Lb, Lc = vr._line_chain(x, LD)
            ob = x[18:21]
            dc = Rbc.T @ (Rwb.T @ Lw[3:])
            expect = 10 * np.array([dc[0] / dc[2] - ob[0] / ob[2], dc[1] / dc[2] - ob[1] / ob[2]])
            tol = lambda a: 64 * EPS_LD * max(1.0, float(np.abs(a).max()))
            assert np.abs(out[:2] - expect).max() <= tol(expect) * max(1.0, float(np.abs(dc / dc[2]).max())), name
            jel = 10 * np.array([[-1 / ob[2], 0, ob[0] / ob[2]], [0, -1 / ob[2], ob[1] / ob[2]]], LD)
            J = _local("vp", out[2:])
            Jp = jel @ (Rbc.T @ vr.skew(Rwb.T @ Lw[3:]))
            Je = jel @ vr.skew(Rbc.T @ (Rwb.T @ Lw[3:]))
            nn, vn = np.sqrt(Lw[:3] @ Lw[:3]), np.sqrt(Lw[3:] @ Lw[3:])
            u1, u2 = Lw[:3] / nn, Lw[3:] / vn
            w0, w1 = nn / np.sqrt(nn * nn + vn * vn), vn / np.sqrt(nn * nn + vn * vn)
            Kb = np.stack([w1 * np.cross(u1, u2), np.zeros(3, LD), -w1 * u1, w0 * u2], axis=1)
            Jo = jel @ ((Rwb @ Rbc).T @ Kb)
            assert np.all(J[:, 0:3] == 0) and np.all(J[:, 6:9] == 0) and np.all(J[:, 13] == 0), name
            for a, b in ((J[:, 3:6], Jp), (J[:, 9:12], Je), (J[:, 12:16], Jo)):
                assert np.abs(a - b).max() <= tol(b), name


def test_losses_against_the_corrector_step_ref_spells():
    delta = LD(1.0)
    for name, s, rho, sc in vr.loss_rows(LD, 1.0):
        s = LD(s)
        if name == "huber":
            want = (2 * delta * np.sqrt(s) - delta * delta, np.sqrt(delta / np.sqrt(s))) if s > delta * delta else (s, LD(1))
        else:
            want = (np.log(1 + s), 1 / np.sqrt(1 + s))
        assert abs(rho - want[0]) <= 4 * EPS_LD * abs(want[0]) and abs(sc - want[1]) <= 4 * EPS_LD * abs(want[1]), (name, s)
    assert vr.huber(1.0 + 1e-12, 1.0)[1] < 1 and vr.huber(1.0 - 1e-12, 1.0)[1] == 1
    y = vr.loss_yardstick()
    assert y["huber"] <= vr.bar("loss", "huber") and y["cauchy"] <= vr.bar("loss", "cauchy")


@pytest.mark.parametrize("name", list(vr.cases()))
def test_the_oracle_is_within_the_bars(name):
    kind, X, ref, unit, out64, rho64 = vr.evaluated(name)
    rho = vr.rho_rows(kind, _oracle(kind, X), ref, unit)
    got = vr.split(kind, rho)
    print("%s oracle %s bars %s" % (name, vr._fmt(got), vr._fmt({k: vr.bar(name, k) for k in got})))
    for what, val in got.items():
        assert val <= vr.bar(name, what), (name, what, val, vr.bar(name, what))
    if name in vr.GENERIC and kind in ("orth_plus", "plk_to_orth"):         # the angles themselves where they are determined
        assert np.abs(_oracle(kind, X) - np.asarray(vr.run(kind, X), np.float64)).max() <= 1e-13


def _detects(name):
    """the smallest relative error of one entry the bar of a case still detects: min over entries of bar * unit / |value|"""
    kind, X, ref, unit, _, _ = vr.evaluated(name)
    out = []
    for what, cols in (("r", slice(0, 2)), ("J", slice(2, None))):
        a, u = np.abs(np.asarray(ref[:, cols], np.float64)), unit[:, cols]
        m = (u > 0) & (a > 0)
        out.append(float((vr.bar(name, what) * u[m] / a[m]).min()))
    return out


def test_sharpness_of_the_bars():
    """One block of the Jacobian of the float64 run scaled by 1 + 1e-9, or its residual by 1 + 1e-12, leaves the bar in EVERY factor
    of the generic cases.  The ill-conditioned cases keep the bars their own float64 run sets; what they still detect, as the
    smallest relative error of one entry of the residual and of the Jacobian: p_j_off_0.001 3e-13, 4e-13; p_j_off_1e-06 9e-10, 2e-9;
    p_j_off_1e-08 3e-8, 6e-8 -- there a tangent basis turned by 1e-7 is found, a wrong last digit is not (the reference's b1 =
    normalize(tmp - a (a . tmp)) itself differs by 7e-14, 3e-10, 1.1e-8 between float64 and long double; asserted: within 16 x
    that); l_image_inf 6e-9, 6e-8 (|nc.xy| = 1e-6 |nc.z|: ten inputs' rounding moves it by 2e-9 of itself, the Jacobian goes with its
    third power, the bar is 43: 3e-7 asserted); l_origin_1e3 1e-12 in the residual (positions of 1e3 m against a line metres away);
    l_obs_on_line nothing relative in the residual, which is 0 in exact arithmetic; every other projection and line case 2e-13 or
    less."""
    for name, blocks in (("p_generic", vr.PROJ_BLOCKS), ("l_generic", vr.LINE_BLOCKS)):
        kind, X, ref, unit, out64, _ = vr.evaluated(name)
        for block, cols in blocks.items():
            out = out64.copy()
            out[:, 2 + np.array(cols)] *= 1.0 + 1e-9
            rho = vr.rho_rows(kind, out, ref, unit)[:, 2:].max(axis=1)
            assert np.all(rho > vr.bar(name, "J")), (name, block, rho.min())
        out = out64.copy()
        out[:, :2] *= 1.0 + 1e-12
        rho = vr.rho_rows(kind, out, ref, unit)[:, :2].max(axis=1)
        assert np.all(rho > vr.bar(name, "r")), (name, "r", rho.min())
    loose = {"p_j_off_0.001": 16 * 7e-14, "p_j_off_1e-06": 16 * 3e-10, "p_j_off_1e-08": 16 * 1.1e-8, "l_image_inf": 3e-7,
             "l_origin_1e3": 2e-12}
    for name, (kind, _) in vr.cases().items():
        if kind not in ("proj", "line"):
            continue
        d = _detects(name)
        print("%s detects a relative error of %.1e (r) %.1e (J) of one entry" % (name, d[0], d[1]))
        assert max(d[name == "l_obs_on_line":]) <= loose.get(name, 2e-13), (name, d)


def _same(now, table):
    assert set(now) == set(table)
    for case, y in now.items():
        for k, val in table[case].items():
            assert abs(y[k] - val) <= 5e-3 * max(abs(val), 1.0), (case, k, y[k], val)


def test_the_yardsticks_in_vis_ref_are_the_ones_measured_now():
    """to three digits (an entry below 1, which bar() floors at 1, to 0.005)"""
    _same(vr.measure(), vr.YARDSTICK)
    _same(vr.measure_window(), vr.YARDSTICK_WINDOW)


# ---- a window's H, g and cost with long-double visual rows --------------------------------------------------------------------
def test_c_edge_has_a_factor_on_each_huber_branch():
    prob, x, lin = vr.reference("c_edge")
    w, opt = vr.window_cases()["c_edge"]
    first = np.concatenate([[0], np.cumsum(np.asarray(w.point_nobs) - 1)]).astype(int)
    d2 = opt.huber_delta ** 2
    assert lin.sq[first[vr.EDGE["huber"]]] > 100 * d2, "the displaced observation is not in Huber's linear branch"
    assert lin.sq[first[vr.EDGE["huber"]] + 1] < d2, "the same point's next observation is not in the quadratic branch"
    assert np.all(w.point_obs[1, 0:2] == 0.0) and np.all(np.isfinite(np.asarray(lin.H, np.float64)))


@pytest.mark.parametrize("case", vr.WINDOW_CASES)
def test_the_oracle_linearisation_is_within_the_bars_of_the_long_double_factors(case):
    prob, x, lin = vr.reference(case)
    w, opt = vr.window_cases()[case]
    lo = sr.Problem(w, opt).linearize(x)
    assert np.array_equal(lin.unit_H == 0, np.asarray(lo.H, np.float64) == 0)
    got = dict(H=sr.rho(lo.H, lin.H, lin.unit_H), g=sr.rho(lo.g, lin.g, lin.unit_g), cost=float(abs(lo.cost - lin.cost)) / lin.unit_cost)
    print("%s oracle rows %s bars %s" % (case, vr._fmt(got), vr._fmt({k: vr.bar_window(case, k) for k in got})))
    for k, val in got.items():
        assert val <= vr.bar_window(case, k), (case, k, val)


def test_the_oracle_line_opt_cost_is_the_long_double_sum():
    w, opt = vr.window_cases()["e"]
    P, O = vr.line_opt_rows(w, opt)
    ref = vr.line_opt_cost(P, O, opt.line_factor)
    o0 = sr._options(num_iterations=0)
    rep = o.only_line_opt(w.copy(), o0)
    rho = float(abs(LD(rep.initial_cost) - ref) / (sr.EPS64 * ref))
    print("only_line_opt e: cost %.6g, oracle rho %.3g (bar %.3g)" % (float(ref), rho, vr.bar("line_opt", "cost")))
    assert len(P) == int(np.sum(w.line_nobs)) and rho <= vr.bar("line_opt", "cost")
