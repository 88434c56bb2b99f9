"""The long-double IMU pre-integration (preint_ref.py) on the CPU, before test_gpu_preint.py lets it judge the kernel:

* the float64 run of the restatement, orc_preintegrate and hc_preintegrate (vpl_preint.h::preint_step -- a serial dense form the
  device does NOT run) against the long-double run on every case of preint_inputs.py: below CPU_BAR = 8 units, which is what
  lets the suite's BAR = 32 units stand for the device; structural zeros exact; sum_dt within n eps sum |dt|;
* the committed YARDSTICK is what this machine measures;
* the long-double P is symmetric to its units and its symmetric part has no eigenvalue below -BAR units;
* the empty interval is the identity;
* checks (a) and (b) of preint_ref.py, which a misreading shared by the restatement, the oracle and the kernel cannot pass: the
  bias columns of J and the covariance against central differences of the restatement's own deltas, over one motion sampled at
  dt, dt / 2 and dt / 4;
* what (a) and (b) see and what they cannot (test_what_checks_a_and_b_catch);
* the units are sharp: the reference's dt^3 terms, which (a) and (b) cannot see, are far beyond BAR in them.

Measured here (python tests/preint_ref.py), gaps at dt, dt / 2, dt / 4 and the two ratios:
  (a) p_bg 2.9e-2 1.4e-2 7.1e-3 (2.02 2.01), r_bg 4.5e-2 2.2e-2 1.1e-2 (2.05 2.03), v_bg 3.0e-2 1.5e-2 7.3e-3 (2.04 2.01);
      p_ba, v_ba 3e-11 and r_ba 0 at every dt: J's accelerometer-bias columns are the exact derivative (the deltas are
      linear in ba).
  (b) P-R 3.4e-2 1.9e-2 1.0e-2 (1.78 1.90), P-BG 6.0e-2 2.7e-2 1.3e-2 (2.21 2.07), R-R 5.0e-2 2.6e-2 1.3e-2 (1.93 1.97),
      R-V (1.78 1.91), R-BG (1.93 1.97), V-BG (2.20 2.07), P-P 2.6e-6 1.3e-6 7.3e-7 (2.04 1.72), P-V (1.92 1.83),
      V-V (1.84 1.78); the blocks with BA and BG-BG below 1e-12: exact."""
import numpy as np
import pytest

import preint_inputs as pi
import preint_ref as pr
import step_ref as sr
from test_golden import hostcheck  # noqa: F401  (the module fixture that compiles tests/native/devmath_hostcheck.cpp)

CASES = list(pi.COUNTS)


def test_the_cases_are_what_they_claim():
    c = pi.cases()
    assert list(c) == CASES
    assert {k: len(x["samples"]) for k, x in c.items()} == pi.COUNTS
    assert set(pi.COUNTS.values()) == {0, 1, 2, 3, 19, 20, 37, 64}
    dts = {k: x["samples"][:, 0] for k, x in c.items()}
    assert np.all(dts["n20"] == 0.005) and np.all(dts["n19"] == 0.0025) and np.all(dts["n64"] == 0.0025)
    for k in ("n37_jitter", "n3_fast_jitter"):
        assert np.all((dts[k] >= 0.001) & (dts[k] <= 0.009)) and len(set(dts[k])) == len(dts[k])
    assert dts["n20_dt0"][10] == 0.0 and np.count_nonzero(dts["n20_dt0"]) == 19
    assert dts["n64_long"].sum() > 10.0                                  # past the skip rule of estimator.cpp:1088
    big = lambda x: 0.45 < np.linalg.norm(x["ba"]) < 0.55 and 0.09 < np.linalg.norm(x["bg"]) < 0.11
    zero = lambda x: not x["ba"].any() and not x["bg"].any()
    assert all(big(x) or zero(x) for x in c.values()) and sum(map(big, c.values())) >= 6 and sum(map(zero, c.values())) >= 5
    for k in ("n20_fast", "n64_fast"):
        w = np.linalg.norm(c[k]["samples"][:, 4:7] - c[k]["bg"], axis=1)
        a = np.linalg.norm(c[k]["samples"][:, 1:4] - c[k]["ba"], axis=1)
        assert 8.0 < w.max() < 12.0 and 25.0 < a.max() < 40.0 and np.all(dts[k] == 0.005)
    f = c["n20_fall"]
    assert np.all(f["samples"][:, 1:4] - f["ba"] == 0.0) and np.all(f["acc0"] - f["ba"] == 0.0)
    assert all(x["noise"] == pi.NOISE for k, x in c.items() if k != "default20")
    assert c["default20"]["noise"] == pi.default_noise() != pi.NOISE
    an, gn, aw, gw = pi.NOISE
    assert an / gn > 30 and gn / aw > 5 and aw / gw > 30                    # every swap of two densities is a change of x 30 or more in Q


@pytest.mark.parametrize("case", CASES)
def test_cpu_implementations_against_long_double(case, hostcheck):  # noqa: F811
    c, ref = pi.cases()[case], pr.reference(case)
    for name, out in (("f64", pr.run_f64(c)), ("oracle", pr.run_oracle(c)), ("hostcheck", pr.run_hostcheck(c, hostcheck))):
        e = pr.errors(out, ref)                   # asserts the structural zeros and sum_dt
        print("%-9s %s: dp %.3g dq %.3g dv %.3g J %.3g P %.3g asym %.3g units" % (name, case, e["dp"], e["dq"], e["dv"], e["J"], e["P"], e["asym"]))
        assert pr.worst(e) < pr.CPU_BAR, (name, e)
        assert e["asym"] <= pr.BAR, (name, e)
        assert np.array_equal(out.lba, c["ba"]) and np.array_equal(out.lbg, c["bg"])


def test_the_yardstick_in_preint_ref_is_what_this_machine_measures(hostcheck):  # noqa: F811
    """seeded; reproduces up to the libm and the matrix product in use.  Every entry is below 1.5 units: they only have to stay
    below 4, and below CPU_BAR = 8 the bar stands"""
    now = pr.measure(hostcheck)
    assert set(now) == set(pr.YARDSTICK) == set(CASES)
    for case, y in now.items():
        for k, val in pr.YARDSTICK[case].items():
            assert val < pr.CPU_BAR and y[k] < pr.CPU_BAR
            assert (y[k] == 0.0) if val == 0 else (y[k] < 4.0 * max(val, 1.0)), (case, k, y[k], val)


@pytest.mark.parametrize("case", CASES)
def test_long_double_covariance_is_symmetric_and_positive(case):
    ref = pr.reference(case)
    P = ref.P
    assert pr._ratio(P - P.T, np.zeros((15, 15), sr.LD), ref.unit_P + ref.unit_P.T) <= 1.0
    sym = np.asarray((P + P.T) / 2, np.float64)
    d = np.sqrt(np.where(np.diag(sym) > 0, np.diag(sym), 1.0))             # Jacobi scaling: cond2(P) is almost all scaling
    lam = np.linalg.eigvalsh(sym / np.outer(d, d)).min()
    unit = np.linalg.norm(ref.unit_P / np.outer(d, d), 2)
    assert lam >= -pr.BAR * unit - 15 * sr.EPS64, (lam, unit)             # (+ eigvalsh's own float64 rounding of a matrix of norm <= 15)
    if ref.n > 0:
        assert np.all(np.diag(sym) > 0)


def test_structural_zeros_are_where_the_issue_says():
    ref = pr.reference("n20")
    off = ~np.eye(15, dtype=bool)
    assert np.all(ref.zero_J[9:15][off[9:15]]) and np.all(ref.J[9:15] == np.eye(15)[9:15])        # rows 9..14 of J: the identity
    assert np.all(ref.zero_J[3:6, 9:12]) and np.all(ref.unit_J[3:6, 9:12] == 0)                    # dq_dba
    assert np.all(ref.zero_P[9:12, 12:15]) and np.all(ref.zero_P[12:15, 9:12])                      # bias blocks off the diagonal
    assert np.all(ref.zero_P[9:12, 9:12][off[:3, :3]]) and np.all(ref.zero_P[3:6, 9:12])
    assert not ref.zero_J[:9, :9].all() and not ref.zero_P[:9, :9].any()
    assert np.all(ref.unit_J[~ref.zero_J] > 0) and np.all(ref.unit_P[~ref.zero_P] > 0)


def test_the_empty_interval_is_the_identity(hostcheck):  # noqa: F811
    c, ref = pi.cases()["n0"], pr.reference("n0")
    assert ref.n == 0 and ref.sum_dt == 0 and not ref.unit_J.any() and not ref.unit_P.any() and ref.unit_dq == 0
    for out in (pr.Out.of(ref), pr.run_f64(c), pr.run_oracle(c), pr.run_hostcheck(c, hostcheck)):
        assert out.sum_dt == 0.0 and not out.dp.any() and not out.dv.any() and np.array_equal(out.q, [0, 0, 0, 1])
        assert np.array_equal(out.J, np.eye(15)) and not out.P.any()


# ---- checks (a) and (b) -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gaps_a():
    return [pr.bias_gap(c) for c in pi.halving()]


@pytest.fixture(scope="module")
def cov_b():
    return [pr.noise_cov(c) for c in pi.halving_noise()]


def _verdict_b(cov_b, **kw):
    g = [pr.noise_gap(c, S, **kw) for c, S in zip(pi.halving_noise(), cov_b)]
    return {(i, j): pr.halves([x[i, j] for x in g]) for i in range(5) for j in range(5)}


def test_a_bias_columns_of_J_against_central_differences(gaps_a):
    h = pi.halving()
    assert [len(c["samples"]) for c in h] == [16, 32, 64] and all(abs(c["samples"][:, 0].sum() - 0.16) < 1e-12 for c in h)
    verdict = {k: pr.halves([g[k] for g in gaps_a]) for k in pr.BIAS_BLOCKS}
    print({k: [g[k] for g in gaps_a] for k in pr.BIAS_BLOCKS})
    assert verdict == dict(p_ba="exact", r_ba="exact", v_ba="exact", p_bg="shrinks", r_bg="shrinks", v_bg="shrinks"), verdict


def test_b_covariance_against_the_noise_jacobian(cov_b):
    h = pi.halving_noise()
    assert [len(c["samples"]) for c in h] == [4, 8, 16] and all(c["noise"] == pi.NOISE for c in h)
    verdict = _verdict_b(cov_b)
    exact = {(i, j) for i in range(5) for j in range(5) if 3 in (i, j)} | {(4, 4)}       # every block with BA, and BG-BG: dt I only
    for ij, w in verdict.items():
        assert w == ("exact" if ij in exact else "shrinks"), (ij, w)


def test_what_checks_a_and_b_catch(gaps_a, cov_b):
    """A misreading put into the restatement itself -- what a port shared by oracle and kernel could carry -- against (a) / (b).
    Caught: every swap of two noise densities, a first-order block with the wrong sign or in the wrong block column.
    NOT caught, by construction: the reference's terms beyond first order -- the factor (I - [w]x dt) of F's theta columns, the
    sign of dp_dbg (dt^3) and of V's dt^3 / 8 term, one of the two gyroscope shares of the position noise.  They change a gap
    that is O(dt) by O(dt) (measured: p_bg 2.9e-2 -> 4.8e-2 without the factor, ratios 1.95 1.97; P-R 3.4e-2 -> 0.18 with the
    sign flipped, ratios 6.4 3.5) and vanish in the limit like the gap itself; only the reference's own lines say what they are,
    and the restatement, held to those lines, says it to the oracle, preint_step and the kernel (test_the_units_are_sharp)."""
    an, gn, aw, gw = pi.NOISE
    for noise in ((gn, an, aw, gw), (an, gn, gw, aw), (aw, gn, an, gw), (an, gw, aw, gn)):
        assert "stays" in _verdict_b(cov_b, noise=noise).values(), noise
    for m in ("dtheta_dbg_sign", "dv_dba_block"):
        g = [pr.bias_gap(c, mutate=m) for c in pi.halving()]
        assert "stays" in [pr.halves([x[k] for x in g]) for k in pr.BIAS_BLOCKS], m
        assert "stays" in _verdict_b(cov_b, mutate=m).values(), m
    for m in ("no_ImW", "dp_dbg_sign"):
        g = [pr.bias_gap(c, mutate=m) for c in pi.halving()]
        assert "stays" not in [pr.halves([x[k] for x in g]) for k in pr.BIAS_BLOCKS], m


@pytest.mark.parametrize("mutate", ["no_ImW", "dp_dbg_sign", "b_sign", "one_gn"])
def test_the_units_are_sharp(mutate):
    """a float64 run that misreads one of the reference's higher-order terms is beyond BAR = 32 units on the ordinary cases,
    by orders of magnitude"""
    for case in ("n20", "n37_jitter", "n20_fast", "default20"):
        c, ref = pi.cases()[case], pr.reference(case)
        bad = pr.Out.of(pr.integrate(c["samples"], c["acc0"], c["gyr0"], c["ba"], c["bg"], c["noise"], np.float64, units=False, mutate=mutate))
        e = pr.errors(bad, ref)
        print(mutate, case, e)
        assert pr.worst(e) > 1e3 * pr.BAR, (case, e)
