"""linemap_ref.py on the CPU: its cases are what they claim (trace shapes, which erase rule fires, the sides of the thresholds, every
decision margin at least 1e3 x the deviation of the float64 runs), its SVD against LAPACK and mpmath, the oracle within the bars
on every case and iteration count, the yardstick tables those this machine measures, and the bars sharp enough to notice each rule
of the minimiser and of the two triangulations altered on its own."""
import numpy as np
import pytest

import linemap_ref as lr
import oracle_api as o

LD = lr.LD
LO = list(lr.lo_cases())
TL = list(lr.tl_cases())
TP = list(lr.tp_cases())


def _letters(res):
    return "".join("A" if t["accepted"] else "T" if t.get("terminated") else "R" if t["valid"] else "I" for t in res["trace"])


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def test_the_line_opt_cases_are_what_they_claim():
    gen, four = lr.lo_reference("lo_generic"), lr.lo_reference("lo_four")
    for res, n in ((gen, 6), (four, 4)):
        assert res["problem"].nL == n and _letters(res) == "AAAAT" and res["trace"][-1]["terminated"] == "function"
        assert res["report"]["termination"] == 1 and res["report"]["iterations"] == res["report"]["successful"] == 4
    assert sorted(len(ob) for ob in gen["problem"].obs) == sorted(lr.LO_NOBS) and {2, 5, 11} <= set(lr.LO_NOBS)
    assert lr.sweep("lo_generic") == [1, 2, 3, 4, 5]          # lo_cap: k = 1 .. 4 stop on the cap mid-flight, k = 5 on the tolerance
    assert [lr.at(gen, k)[0]["termination"] for k in lr.sweep("lo_generic")] == [0, 0, 0, 0, 1]
    three = lr.lo_reference("lo_three")
    assert not three["ran"] and three["report"] == dict(iterations=0, successful=0, termination=0, initial_cost=0.0, final_cost=0.0)
    # a rejected step followed by an accepted one; the attempt after a rejection solves with the kept diagonal and the radius divided
    # by decrease_factor (2, then 4); after the acceptance the diagonal is new and decrease_factor is back at 2
    rej = lr.lo_reference("lo_reject")
    assert _letters(rej) == "ARRAAAAA"
    t = rej["trace"]
    assert not t[1]["reused"] and t[2]["reused"] and t[3]["reused"] and not t[4]["reused"]
    assert t[2]["radius"] == t[1]["radius"] / 2 and t[3]["radius"] == t[2]["radius"] / 4
    assert np.array_equal(t[2]["diag"], t[1]["diag"]) and np.array_equal(t[3]["diag"], t[1]["diag"])
    assert not np.array_equal(t[4]["diag"], t[1]["diag"])
    assert [r["decrease_factor"] for r in t[1:5]] == [2, 4, 8, 2]
    # the total cost decides: on the rejected step the lines that were not pushed must stay too
    orth = [s[0] for s in rej["states"]]
    assert np.array_equal(orth[2], orth[1]) and np.array_equal(orth[3], orth[1]) and not np.array_equal(orth[4], orth[1])
    assert t[1]["rho"] < lr.MIN_REL_DECREASE < t[3]["rho"]
    # lo_reject2: a rejection after the acceptance that followed a rejection -- where a decrease_factor that is not reset shows
    assert _letters(lr.lo_reference("lo_reject2")) == "ARAARRRR"
    assert [r["decrease_factor"] for r in lr.lo_reference("lo_reject2")["trace"]] == [2, 2, 4, 2, 2, 4, 8, 16]
    for name, n in lr.FULL.items():
        res = lr.lo_reference(name)
        assert res["problem"].nL == n == len(lr.lo_cases()[name][0].line_start) and _letters(res) == "AA"
        assert {len(ob) for ob in res["problem"].obs} == {2, 3}
    assert [4 if 4 * n <= 256 else 2 if 2 * n <= 256 else 1 for n in lr.FULL.values()] == [4, 2, 1, 2]


@pytest.mark.parametrize("name", list(lr.OUT_RULE))
def test_each_erase_rule_decides_for_one_line(name):
    line, rule = lr.OUT_RULE[name]
    res = lr.lo_reference(name)
    K = lr.lo_cases()[name][1]
    rules = [out[1] for out in lr.at(res, K)[3]]
    assert len(rules) == 5 and rules == [rule if l == line else 0 for l in range(5)], rules
    # remove_line_outlier alone on the handed-back line: the same rule, with the margins of the rules it evaluated
    prob = res["problem"]
    plk = prob.hand_back(res["states"][-1][0])
    for l in range(5):
        erased, r, m = lr.remove_line_outlier(plk[l], prob.cams[prob.starts[l]:prob.starts[l] + len(prob.obs[l])], prob.obs[l])
        assert r == rules[l] and erased == (r != 0) and set(m) == set(("behind", "dist", "err")[:r if r else 3])


@pytest.mark.parametrize("name", LO)
def test_every_decision_of_a_line_opt_case_has_its_margin(name):
    """the condition on a case: all float64 runs decide as the long-double run, and the smallest relative margin of any comparison
    the loop or removeLineOutlier made is at least 1e3 x the largest relative deviation the float64 runs show"""
    same, margin, dev = lr.condition(name)
    print("%s: smallest margin %.3g, largest deviation %.3g" % (name, margin, dev))
    assert same, "%s: a float64 run takes another decision than the long-double run" % name
    assert margin >= lr.MARGIN_FACTOR * dev, (name, margin, dev)
    res = lr.lo_reference(name)
    assert not any(not t["valid"] for t in res["trace"]) and res["report"]["termination"] != 2


def test_the_triangulation_cases_are_what_they_claim():
    ref = lr.tl_reference("tl_threshold")
    assert [abs(d["min_cos"] - t) < 1e-9 for (_, _, d), t in zip(ref, lr.TL_TARGETS)] == [True] * 4
    assert [plk is not None for plk, _, _ in ref] == [t < lr.COS_MAX for t in lr.TL_TARGETS] == [True, False, True, False]
    gen = lr.tl_reference("tl_generic")
    assert sorted(lr.tl_cases()["tl_generic"].line_nobs) == [2, 3, 4, 5, 7, 9, 10, 11] and sum(p is not None for p, _, _ in gen) >= 6
    last = [d["chosen"] == n - 1 for (p, _, d), n in zip(gen, lr.tl_cases()["tl_generic"].line_nobs) if p is not None]
    assert not all(last), "argmin is the last observation everywhere"
    one = lr.tl_reference("tl_one_obs")
    assert [d is None for _, _, d in one] == [True, False, True, False]
    assert [d is None for _, _, d in lr.tl_reference("tl_keep")] == [False, True, False, True]
    stride = lr.tl_reference("tl_stride")
    assert len(stride) == 129 and stride[128][0] is not None, "lane 0's second line is not triangulated"
    assert 40 <= sum(p is not None for p, _, _ in stride[:128]) <= 120
    assert [len(lr.tl_reference("tl_batch%d" % i)) for i in range(3)] == [5, 1, 9]
    # points
    th = lr.tp_reference("tp_threshold")
    assert [round(d["svd_depth"], 6) for _, _, d in th] == [0.09, 0.11, 0.09, 0.11]
    assert [d["used_init"] for _, _, d in th] == [True, False, True, False]
    assert all(d["used_init"] and d["svd_depth"] < 0 for _, _, d in lr.tp_reference("tp_behind"))
    assert sorted(lr.tp_cases()["tp_generic"].point_nobs) == [2, 3, 7, 11]
    wk = lr.tp_cases()["tp_keep"]
    assert np.signbit(wk.inv_depth[1]) and wk.inv_depth[1] == 0
    assert [d is None for _, _, d in lr.tp_reference("tp_keep")] == [True, True, False, True]
    sb = lr.tp_reference("tp_short_baseline")
    assert all(u / abs(float(inv)) > 100 * lr.EPS64 for inv, u, _ in sb), "the nearly degenerate tracks do not have a large unit"
    st = lr.tp_reference("tp_stride")
    assert len(st) == 129 and sum(u is not None for _, u, _ in st) == lr.TP_UNIT_SUBSET and not any(d["used_init"] for _, _, d in st)


@pytest.mark.parametrize("name", TL + TP)
def test_every_decision_of_a_triangulation_case_has_its_margin(name):
    """as for onlyLineOpt: the float64 runs one ulp away choose the same observation and fall on the same side of 0.998 and of 0.1
    (tl_rho / tp_rho are infinite otherwise), and the margins are 1e3 x the relative deviation of the result"""
    if name in TL:
        ref = [r for r in lr.tl_reference(name) if r[2] is not None]
        margin = min([min(d["m_cos"], d["m_argmin"]) for _, _, d in ref] + [np.inf])
        y = lr.tl_measure(name)["plk"]
        dev = max([float((u / np.abs(p).max()).max()) for p, u, _ in ref if p is not None] + [0.0]) * max(y, 1.0)
    else:
        ref = [r for r in lr.tp_reference(name) if r[2] is not None]
        margin = min(d["m_depth"] for _, _, d in ref)
        m = lr.tp_measure(name)
        dev = max([u / abs(float(inv)) for inv, u, d in ref if u] + [0.0]) * max(m["invd"], 1.0)
        dev = max(dev, lr.EPS64 * m.get("rest", 0.0))
        y = m["invd"]
    print("%s: smallest margin %.3g, largest deviation %.3g" % (name, margin, dev))
    assert np.isfinite(y) and margin >= lr.MARGIN_FACTOR * dev, (name, margin, dev)


# ---- the SVD -------------------------------------------------------------------------------------------------------------------------
def _dlt_matrices():
    for name in TP:
        w = lr.tp_cases()[name]
        for p, (inv, unit, dec) in enumerate(lr.tp_reference(name)):
            if dec is not None and unit:
                pose, obs = lr.point_track(w, p)
                yield name, inv, unit, lr.dlt_rows(pose, w.ex_pose, obs)


def test_hestenes_against_lapack_in_the_float64_yardstick():
    """the long-double one-sided Jacobi against numpy.linalg.svd of the same matrix rounded to float64: the depth LAPACK's null vector
    gives is within the case's float64 bar of the long-double one, and the singular values agree to float64"""
    n = 0
    for name, inv, unit, A in _dlt_matrices():
        s2, V = lr.hestenes(A)
        assert np.abs(np.asarray(V.T @ V, np.float64) - np.eye(4)).max() < 1e-17
        u, s, vt = np.linalg.svd(np.asarray(A, np.float64))
        assert np.abs(np.sort(np.sqrt(np.asarray(s2, np.float64)))[::-1] - s).max() <= 16 * lr.EPS64 * s[0]
        rho = float(abs(LD(vt[-1, 3] / vt[-1, 2]) - inv) / unit)
        assert rho <= lr.bar(name, "invd"), (name, rho)
        n += 1
    assert n >= 20


def test_hestenes_against_mpmath_at_40_digits():
    """the reference itself: against mpmath.svd_r at 40 digits its inverse depth is at least 2^-8 of a unit fine (long double carries
    11 bits more than float64; three are left to the conditioning of the null vector beyond what the unit already holds)"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    worst = 0.0
    for name, inv, unit, A in _dlt_matrices():
        M = mp.matrix([[mp.mpf(float(a)) + mp.mpf(float(a - LD(float(a)))) for a in row] for row in A])
        S, Vt = mp.svd_r(M, full_matrices=False, compute_uv=True)[1:]
        k = min(range(4), key=lambda j: S[j])
        inv_mp = Vt[k, 3] / Vt[k, 2]
        err = abs(mp.mpf(float(inv)) + mp.mpf(float(inv - LD(float(inv)))) - inv_mp) / mp.mpf(unit)
        worst = max(worst, float(err))
    print("long-double Jacobi against mpmath: %.3g units" % worst)
    assert worst <= 2.0 ** -8


# ---- the oracle within the bars ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LO)
def test_oracle_only_line_opt_within_the_bars(name):
    w = lr.lo_cases()[name][0]
    worst = dict(cost0=0.0, cost=0.0, line=0.0)
    for k in lr.sweep(name):
        w2 = w.copy()
        rep = o.only_line_opt(w2, lr.options(k))
        got = lr.lo_check(name, k, rep, w2)
        for what, val in got.items():
            b = lr.lo_bar(name, what, None if what == "cost0" else k)
            assert val <= b, (name, k, what, val, b)
            worst[what] = max(worst[what], val)
    print("%s oracle %s" % (name, lr._fmt(worst)))


@pytest.mark.parametrize("name", TL)
def test_oracle_triangulate_lines_within_the_bars(name):
    w2 = lr.tl_cases()[name].copy()
    o.triangulate_lines(w2, lr.options())
    got = lr.tl_check(name, w2)
    print("%s oracle %s (bar %.3g)" % (name, lr._fmt(got), lr.bar(name, "plk")))
    assert got["plk"] <= lr.bar(name, "plk")


@pytest.mark.parametrize("name", TP)
def test_oracle_triangulate_points_within_the_bars(name):
    w2 = lr.tp_cases()[name].copy()
    o.triangulate_points(w2, lr.options(), lr.INIT_DEPTH)
    got = lr.tp_check(name, w2)
    print("%s oracle %s" % (name, lr._fmt(got)))
    for what, val in got.items():
        assert val <= lr.bar(name, what), (name, what, val)


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
def test_the_yardsticks_in_linemap_ref_are_the_ones_this_machine_measures():
    """seeded; reproduces up to the libm in use: within a factor 4 where a bar depends on it, entries below 1 (floored at 1 by the
    bar) only have to stay below 4"""
    now = lr.measure()
    assert set(now) == set(lr.YARDSTICK) == set(LO + TL + TP)
    for case, y in now.items():
        for k, val in lr.YARDSTICK[case].items():
            for a, b in zip(np.atleast_1d(y[k]), np.atleast_1d(val)):
                if b < 1.0:
                    assert a < 4.0, (case, k, a, b)
                else:
                    assert 0.25 * b <= a <= 4.0 * b, (case, k, a, b)
            assert np.size(y[k]) == np.size(val)


# ---- sharpness -----------------------------------------------------------------------------------------------------------------------
def _lo_fails(variant):
    """the line-opt cases on which the reference run with one rule altered leaves the trace or a bar"""
    out = []
    for name in ("lo_generic", "lo_reject", "lo_reject2", "lo_four"):
        w, K = lr.lo_cases()[name]
        ref = lr.lo_reference(name)
        bad = lr.only_line_opt(w, lr.options(K), variant=variant, cap=K)
        if lr.decisions(bad) != lr.decisions(ref):
            out.append((name, "trace"))
            continue
        for k in lr.sweep(name):
            c0, c, ln = lr.lo_compare(bad, ref, k)
            if c0 > lr.lo_bar(name, "cost0") or c > lr.lo_bar(name, "cost", k) or ln > lr.lo_bar(name, "line", k):
                out.append((name, "bar at k = %d: %.3g %.3g %.3g" % (k, c0, c, ln)))
                break
    return out


def _tl_fails(variant):
    out = []
    for name in TL:
        w = lr.tl_cases()[name]
        run = lambda l: lr.triangulate_line(lr.line_track(w, l)[0], w.ex_pose, lr.line_track(w, l)[1], variant=variant)[0]
        got = [None if dec is None else run(l) for l, (_, _, dec) in enumerate(lr.tl_reference(name))]
        if lr.tl_rho(name, got) > lr.bar(name, "plk"):
            out.append(name)
    return out


def _tp_fails(variant):
    out = []
    for name in TP:
        w = lr.tp_cases()[name]
        run = lambda p: lr.triangulate_point(lr.point_track(w, p)[0], w.ex_pose, lr.point_track(w, p)[1], lr.INIT_DEPTH, variant=variant)[0]
        got = [None if dec is None else float(1 / run(p)) for p, (_, _, dec) in enumerate(lr.tp_reference(name))]
        if max(lr.tp_rho(name, got)) > lr.bar(name, "invd"):
            out.append(name)
    return out


CAUGHT_BY = dict(stale_diagonal=_lo_fails, no_reset=_lo_fails, no_cube=_lo_fails, no_corrector_J=_lo_fails,
                 drop_sub1=_lo_fails, **{"cos_0.99": _tl_fails, "depth_0": _tp_fails, "last_obs": _tl_fails})


@pytest.mark.parametrize("variant", list(CAUGHT_BY))
def test_sharpness_of_the_bars(variant):
    """the reference with ONE rule altered leaves the trace or a bar of at least one case: the diagonal of the first step kept for
    good; decrease_factor not reset after a success; the radius update without the cube; sqrt(rho') dropped from the Jacobian; the
    second observation of a track of two dropped; cos 0.99; depth 0.0; the last observation for the argmin"""
    fails = CAUGHT_BY[variant](variant)
    print("%s: caught by %s" % (variant, fails))
    assert fails, "no case notices %s" % variant


def test_two_alterations_no_input_can_show():
    """`reuse_diagonal` ignored in the direction of recomputing every time: a rejected step leaves x, so the Jacobian and with it
    clamp(diag(S H S)) are what they were -- the long-double runs agree bit for bit.  (Ignored in the other direction, the first
    diagonal kept for good, it is `stale_diagonal` above.)  No Jacobi scaling: with the damping proportional to the diagonal,
    S (S H S + diag(S H S) / r)^-1 S g = (H + diag(H) / r)^-1 g -- the step does not depend on S unless the clamp at 1e-6 acts, which
    needs a column with H_ii in [1e-6, 1.002e-6]; H_ii at the start is above 1e-3 (asserted), so the runs agree to the rounding of long
    double, far inside the bars"""
    assert set(lr.VARIANTS) == set(CAUGHT_BY) | {"no_reuse", "no_jacobi"}
    for name in ("lo_reject", "lo_reject2"):
        w, K = lr.lo_cases()[name]
        ref, alt = lr.lo_reference(name), lr.only_line_opt(w, lr.options(K), variant="no_reuse", cap=K)
        assert lr.decisions(alt) == lr.decisions(ref)
        assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(alt["states"], ref["states"]))
    assert _lo_fails("no_jacobi") == []
    for name in ("lo_generic", "lo_reject", "lo_reject2", "lo_four"):
        prob = lr.lo_reference(name)["problem"]
        H = prob.evaluate(prob.orth0, True)[1]
        d = np.asarray(H[:, np.arange(4), np.arange(4)], np.float64)
        assert d.min() > 1e-3, (name, d.min())
