"""prior_ref.py against the oracle, on the CPU: the long-double restatement of MarginalizationFactor::Evaluate and of the prior's
share of H, g that test_gpu_prior_factor.py holds the kernels to.  Every prior and state family of prior_inputs.py; bars
8 x max(yardstick, 1) from prior_ref.YARDSTICK, whose rows are what the float64 restatement of the reference's own formulation
reaches on the same inputs."""
import os
import subprocess

import numpy as np
import pytest

import oracle_api as o
import prior_inputs as pi
import prior_ref as pr

CASES = [(pid, fam) for pid in pi.PRIORS for fam in pi.FAMILIES]


def _id(c):
    return "%s-%s" % c


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_oracle_prior_factor(case):
    """o.prior_factor: residuals within the r bar, Jacobian blocks J0's columns exactly, a pose's seventh column exactly 0"""
    pid, fam = case
    prior, x = pi.case(pid, fam)
    ref = pr.Ref(prior, x)
    r, jac = o.prior_factor(prior, pr.params(prior, x))
    rho_r = pr.rho(r, ref.r, ref.unit_r)
    print("oracle %s %s rho_r %.3g (bar %.3g)" % (pid, fam, rho_r, pr.bar("r", pid)))
    assert rho_r <= pr.bar("r", pid)
    off = 0
    for Jb in ref.jac_blocks():
        got = jac[off:off + Jb.size].reshape(Jb.shape)
        assert np.array_equal(got, Jb)
        if Jb.shape[1] == 7:
            assert np.all(got[:, 6] == 0.0)
        off += Jb.size
    assert off == jac.size


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_float64_restatements(case):
    """both formulations in float64 -- the reference's J0^T (r0 + J0 dx), whose worst rho per prior IS the yardstick, and the
    device's g0 + H dx -- stay within the bars; the table in the module is the one measure() gives"""
    pid, fam = case
    prior, x = pi.case(pid, fam)
    ref = pr.Ref(prior, x)
    for form in ("ref", "dev"):
        got = pr.rhos(pr.restate64(prior, x, form), ref)
        print("%s %s %s " % (pid, fam, form) + " ".join("%s %.3g" % kv for kv in got.items()))
        for what, val in got.items():
            assert val <= pr.bar(what, pid), (form, what)
            if form == "ref":     # the recorded yardstick covers this case (printed with three digits)
                assert val <= 1.006 * pr.YARDSTICK[pid][what] + 1e-12, (what, val, "YARDSTICK is stale: python tests/prior_ref.py")


@pytest.mark.parametrize("pid", pi.PRIORS)
def test_families_are_what_they_claim(pid):
    prior, x = pi.case(pid, "exact")
    d64, dld = pr.dx_of(prior, x, np.float64)[0], pr.dx_of(prior, x, pr.LD)[0]
    assert np.array_equal(d64.astype(pr.LD), dld), "a dx entry of the exact family is not exact in float64"
    assert np.all(d64 != 0.0)
    ref = pr.Ref(prior, x)
    assert np.all(ref.unit_dx <= 9 * pr.EPS64 * np.abs(dld))
    # ... also at states that went through a rotation matrix and back, as the device's do
    import step_ref as sr
    xc = dict(x, pose=x["pose"].copy(), ex=x["ex"].copy())
    for q in list(xc["pose"][:, 3:]) + [xc["ex"][3:]]:
        q[:] = sr.R_quat(sr.quat_R(q / np.linalg.norm(q)))
    assert np.array_equal(pr.dx_of(prior, xc, np.float64)[0].astype(pr.LD), pr.dx_of(prior, xc, pr.LD)[0])
    prior, x = pi.case(pid, "at_x0")
    ref = pr.Ref(prior, x)
    assert np.all(ref.dx == 0) and np.array_equal(ref.r, prior.r().astype(pr.LD)) and np.array_equal(ref.g, ref.g0)
    half = (prior.r().astype(pr.LD) ** 2).sum() / 2
    assert abs(ref.cost - half) <= 8 * np.finfo(pr.LD).eps * half
    p0, x0 = pi.zero_dx_case(pid)
    assert np.all(pr.Ref(p0, x0).dx == 0) and np.array_equal(p0.J(), prior.J()) and np.array_equal(p0.r(), prior.r())
    prior, x = pi.case(pid, "general")
    ref = pr.Ref(prior, x)
    turn = [float(np.linalg.norm(ref.dx[idx + 3:idx + 6].astype(np.float64))) for kind, fr, idx, col0, ls, gs in pr.blocks(prior) if kind != 1]
    assert max(turn) > 1.5, "no block is rotated far"       # |dx| = 2 sin(angle / 2)
    assert np.abs(ref.dx).min() < 1e-8, "no block is displaced by 1e-9"


# mutation -> (prior, family, quantity, formulation) of the case on which the float64 restatement WITH the mutation has to exceed
# the bar: (a) no sign flip for w < 0, (b) conj(q0) without the division on |q0| = 1 + 1e-6, (c) q (x) q0^-1, (d) columns from 48
# on dropped from J0 dx, (e) rows from 64 on given r0 of row - 64, (f) one off-diagonal tile of H from J0 J0^T, (g) the extrinsic
# block written at 15 * frame, (h) g0 omitted
SHOWS = {
    "a": ("n81u", "general", "dx", "ref"), "b": ("n75u", "general", "dx", "ref"), "c": ("n48s", "general", "dx", "ref"),
    "d": ("n81u", "exact", "r", "ref"), "e": ("n111s", "exact", "r", "ref"), "f": ("n117s", "exact", "H", "dev"),
    "g": ("n117s", "exact", "H", "ref"), "h": ("n48s", "exact", "g", "dev"),
}


@pytest.mark.parametrize("mutation", pr.MUTATIONS)
def test_units_see_each_mutation(mutation):
    pid, fam, what, form = SHOWS[mutation]
    prior, x = pi.case(pid, fam)
    ref = pr.Ref(prior, x)
    clean = pr.rhos(pr.restate64(prior, x, form), ref)[what]
    bad = pr.rhos(pr.restate64(prior, x, form, mutation), ref)[what]
    print("mutation %s on %s %s: rho_%s %.3g -> %.3g (bar %.3g)" % (mutation, pid, fam, what, clean, bad, pr.bar(what, pid)))
    assert clean <= pr.bar(what, pid) < bad


def test_exact_family_sees_the_H_dx_arithmetic():
    """what the exact-dx family is for: ONE entry of H wrong in its 40th bit (2^-40 relative, 4.5e3 eps64) in g0 + H dx shows in g
    on it, and does not on the general family, whose unit is dominated by the propagated rounding of dx"""
    out = {}
    for fam in ("exact", "general"):
        prior, x = pi.case("n75u", fam)
        ref = pr.Ref(prior, x)
        J0, r0 = prior.J(), prior.r()
        H = J0.T @ J0
        H[40, 40] *= 1.0 + 2.0 ** -40
        g = J0.T @ r0 + H @ pr.dx_of(prior, x, np.float64)[0]
        out[fam] = pr.rho(pr.scatter(prior, H, g, dtype=np.float64)[1], ref.g, ref.unit_g)
    print("H[40, 40] (1 + 2^-40): rho_g exact %.3g general %.3g (bar %.3g)" % (out["exact"], out["general"], pr.bar("g", "n75u")))
    assert out["exact"] > pr.bar("g", "n75u")


def test_with_the_extrinsic_held_constant():
    """ex_free = False: the extrinsic's rows and columns of H and entries of g are zero, r keeps the extrinsic's dx"""
    for n in (75, 81):
        prior, x = pi.case(pi.pid_of(n), "general")
        free, fixed = pr.Ref(prior, x), pr.Ref(prior, x, ex_free=False)
        assert np.array_equal(fixed.r, free.r) and fixed.cost == free.cost
        assert np.all(fixed.H[165:] == 0) and np.all(fixed.H[:, 165:] == 0) and np.all(fixed.g[165:] == 0)
        assert np.all(fixed.unit_H[165:] == 0) and np.all(fixed.unit_g[165:] == 0)
        assert np.array_equal(fixed.H[:165, :165], free.H[:165, :165]) and np.array_equal(fixed.g[:165], free.g[:165])
        got = pr.rhos(pr.restate64(prior, x, "dev", ex_free=False), fixed)
        assert all(got[k] <= pr.bar(k, pi.pid_of(n)) for k in got)


def test_step_ref_takes_the_prior_rows():
    """the opt-in hook: step_ref.Problem with prior_rows=prior_ref.prior_rows agrees with the oracle's rows within the r bar and
    carries the prior's share H, g of prior_ref exactly; without the hook nothing changes"""
    import step_ref as sr
    w = pi.landmark_window(75)
    opt = sr._options()
    prob, plain = sr.Problem(w, opt, prior_rows=pr.prior_rows), sr.Problem(w, opt)
    x = prob.initial_state()
    kind, wt, huber, r, blocks = prob.rows(x)[0]
    kind0, _, _, r0, blocks0 = plain.rows(x)[0]
    assert kind == kind0 == "prior" and not huber and wt == 1.0
    ref = pr.Ref(w.prior, x)
    assert r.dtype == pr.LD and np.array_equal(r, ref.r)
    assert pr.rho(r0, ref.r, ref.unit_r) <= pr.bar("r", "n75u")
    for (c, Jb), (c0, Jb0) in zip(blocks, blocks0):
        assert c == c0 and np.array_equal(np.asarray(Jb, np.float64), Jb0)
    assert len(prob.rows(x)) == len(plain.rows(x))


def test_lin_prh_n_of_the_capacities_used(tmp_path):
    """lin_prh_n (csrc/ba_lin.h) evaluated on the host for the two capacities test_gpu_prior_factor.py makes its contexts with:
    40 points / 12 lines keeps priors of up to 76 dims in LDS (n = 75 is the LDS path, n = 81 the += pass), 478 / 12 only up to
    44 (n = 48 and n = 75 take the += pass on the fast path)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "lin_prh_n")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           "-I" + os.path.join(root, "vplines-slam_amd", "csrc"),
                           os.path.join(root, "tests", "native", "lin_prh_n.cpp"), "-o", exe])
    out = subprocess.run([exe, "40", "12", "478", "12"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = [tuple(int(t) for t in line.split()) for line in out.stdout.strip().splitlines()]
    print(got)
    assert [g[:3] for g in got] == [(40, 12, 76), (478, 12, 44)]
    assert all(g[3] == 1 for g in got), "a capacity the context would refuse"
