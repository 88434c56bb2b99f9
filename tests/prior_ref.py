"""The marginalisation prior as a residual block, restated in np.longdouble -- the reference for how a GIVEN prior is consumed:
MarginalizationFactor::Evaluate (marginalization_factor.cpp:502-520, oracle/marginalization.cpp) and the prior's share of the
window's normal equations.  test_prior_reference.py checks it against the oracle on the CPU, test_gpu_prior_factor.py holds
k_eval_prior, k_prep + k_lin (lin_prior, lin_assemble), k_cost and k_solve to it.  How a prior is produced (k_marg) is not here.

What is restated, per kept block of the prior (kind 0 pose, 1 speed/bias, 2 extrinsic; x0 its linearisation point):
  dx     speed/bias: x - x0.  Pose, extrinsic: p - p0 and +-2 vec(q0^-1 (x) q), q0^-1 = conj(q0) / |q0|^2 (Eigen's inverse()), the
         sign + when the product's w >= 0 and - otherwise.
  r      r0 + J0 dx                      cost   r^T r / 2 (no loss function)
  H, g   J0^T J0 and J0^T r, scattered to the 171 camera columns through the block table (pose f -> 15 f, speed/bias f ->
         15 f + 6, extrinsic -> 165).  With the extrinsic held constant its columns of J0 are zero columns (r keeps its dx).

Units (first-order forward error of the reference's OWN formula in float64; rho = |error| / unit):
  dx     eps64 (|x| + |x0|) for a difference, 2 eps64 sum |a_i b_j| over the four products of a quaternion-product entry
  r      eps64 (|r0| + |J0| |dx|) + |J0| unit(dx)
  g      eps64 |J0|^T (|r0| + |J0| |dx|) + |J0|^T |J0| unit(dx): dx is a difference of nearby states, and what its rounding does
         to g is orders of magnitude above the first term on general inputs
  H      eps64 |J0|^T |J0| (no factor n)
  cost   eps64 r^T r / 2 + |r|^T unit(r)
The device does not compute g by that formula: k_prep forms H = J0^T J0 (FP64 matrix cores) and g0 = J0^T r0, lin_prior writes
g = g0 + H dx.  Both formulations are restated in float64 below (restate64); the reference's is the yardstick the bars come from
(bar = 8 x max(yardstick, 1), YARDSTICK below), the device's is measured beside it.  On general inputs the propagated-dx term
of unit(g) would hide an error of the H dx arithmetic itself; the exact-dx family of prior_inputs.py (x0 quaternions identity,
dyadic positions: dx exact in float64) leaves little more than the linear-algebra term of the unit.

`python tests/prior_ref.py` prints the table YARDSTICK below was copied from."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "np.longdouble is not an extended type here: restate the linear algebra below with mpmath"
EPS64 = float(np.finfo(np.float64).eps)
NF, NC = 11, 171
MUTATIONS = "abcdefgh"


# ---- the block table ------------------------------------------------------------------------------------------------------
def blocks(prior):
    """[(kind, frame, first row of dx, first camera column, local size, global size)] in the prior's block order"""
    out = []
    for b in range(prior.n_blocks):
        kind, fr, idx = int(prior.block_kind[b]), int(prior.block_frame[b]), int(prior.block_idx[b])
        out.append((kind, fr, idx, 15 * fr if kind == 0 else 15 * fr + 6 if kind == 1 else 165, 9 if kind == 1 else 6,
                    9 if kind == 1 else 7))
    return out


def cam_map(prior, mutate=None):
    """row of dx -> camera column.  mutate g: an extrinsic block written at 15 * frame instead of 165"""
    m = np.full(prior.n, -1, int)
    for kind, fr, idx, col0, ls, _ in blocks(prior):
        if mutate == "g" and kind == 2:
            col0 = 15 * fr
        m[idx:idx + ls] = col0 + np.arange(ls)
    assert np.all(m >= 0), "the block table does not cover the prior's rows"
    return m


def block_states(prior, x):
    """the parameter blocks of the prior at the window states x = dict(pose [11, 7], sb [11, 9], ex [7])"""
    return [x["pose"][fr] if kind == 0 else x["sb"][fr] if kind == 1 else x["ex"] for kind, fr, *_ in blocks(prior)]


def params(prior, x):
    """what vpl_prior_factor / o.prior_factor take: the blocks one after the other, poses with their seven numbers"""
    return np.concatenate(block_states(prior, x))


def x0_blocks(prior):
    return [np.array(prior.x0[b][:gs], np.float64) for b, (*_, gs) in enumerate(blocks(prior))]


# ---- dx ---------------------------------------------------------------------------------------------------------------------
def _qmul(a, b):
    """(w, x, y, z) product and, entry by entry, the sum of the absolute values of its four terms"""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    t = [[aw * bw, -ax * bx, -ay * by, -az * bz], [aw * bx, ax * bw, ay * bz, -az * by],
         [aw * by, ay * bw, az * bx, -ax * bz], [aw * bz, az * bw, ax * by, -ay * bx]]
    q = [((r[0] + r[1]) + r[2]) + r[3] for r in t]
    s = [((abs(r[0]) + abs(r[1])) + abs(r[2])) + abs(r[3]) for r in t]
    return q, s


def block_dx(kind, x, x0, dt, mutate=None):
    """dx of one kept block in the arithmetic dt, and sum |terms| of every entry (its unit is eps64 times that)"""
    x, x0 = np.asarray(x, np.float64).astype(dt), np.asarray(x0, np.float64).astype(dt)
    if kind == 1:
        return x - x0, np.abs(x) + np.abs(x0)
    d, t = np.zeros(6, dt), np.zeros(6, dt)
    d[:3], t[:3] = x[:3] - x0[:3], np.abs(x[:3]) + np.abs(x0[:3])
    q0, q = (x0[6], x0[3], x0[4], x0[5]), (x[6], x[3], x[4], x[5])
    n2 = ((q0[0] * q0[0] + q0[1] * q0[1]) + q0[2] * q0[2]) + q0[3] * q0[3]
    if mutate == "b":                      # conj(q0) without the division
        n2 = dt(1)
    inv = (q0[0] / n2, -q0[1] / n2, -q0[2] / n2, -q0[3] / n2)
    dq, terms = _qmul(q, inv) if mutate == "c" else _qmul(inv, q)
    sgn = dt(2) if (dq[0] >= 0 or mutate == "a") else dt(-2)
    for k in range(3):
        d[3 + k], t[3 + k] = sgn * dq[1 + k], 2 * terms[1 + k]
    return d, t


def dx_of(prior, x, dt, mutate=None):
    dx, terms = np.zeros(prior.n, dt), np.zeros(prior.n, dt)
    for (kind, fr, idx, col0, ls, gs), xb, x0 in zip(blocks(prior), block_states(prior, x), x0_blocks(prior)):
        dx[idx:idx + ls], terms[idx:idx + ls] = block_dx(kind, xb, x0, dt, mutate)
    return dx, terms


# ---- the reference ------------------------------------------------------------------------------------------------------
def scatter(prior, Hn, gn, ex_free=True, mutate=None, dtype=LD):
    """the prior's n x n, n into the 171 camera columns"""
    m = cam_map(prior, mutate)
    H, g = np.zeros((NC, NC), dtype), np.zeros(NC, dtype)
    np.add.at(H, (m[:, None], m[None, :]), Hn)       # (add: a mutated map may hit a column twice)
    np.add.at(g, m, gn)
    if not ex_free:
        H[165:, :], H[:, 165:], g[165:] = 0, 0, 0
    return H, g


class Ref:
    """dx, r, cost, Hn / gn (the prior's own index), H / g (camera index) in long double, each with its unit"""

    def __init__(self, prior, x, ex_free=True):
        self.prior, self.n, self.ex_free = prior, prior.n, ex_free
        J0, r0 = prior.J().astype(LD), prior.r().astype(LD)
        if not ex_free:                    # a constant block has no Jacobian; its dx still enters r through J0 below
            Jg = J0.copy()
            for kind, fr, idx, col0, ls, gs in blocks(prior):
                if kind == 2:
                    Jg[:, idx:idx + ls] = 0
        else:
            Jg = J0
        self.dx, terms = dx_of(prior, x, LD)
        self.unit_dx = EPS64 * terms
        aJ, aJg = np.abs(J0), np.abs(Jg)
        self.r = r0 + J0 @ self.dx
        lin_terms = np.abs(r0) + aJ @ np.abs(self.dx)
        self.unit_r = EPS64 * lin_terms + aJ @ self.unit_dx
        self.Hn, self.unit_Hn = Jg.T @ Jg, EPS64 * (aJg.T @ aJg)
        self.gn = Jg.T @ self.r
        self.unit_gn = EPS64 * (aJg.T @ lin_terms) + aJg.T @ (aJ @ self.unit_dx)
        self.cost = self.r @ self.r / 2
        self.unit_cost = EPS64 * self.cost + np.abs(self.r) @ self.unit_r
        self.g0n = Jg.T @ r0
        self.H, self.g = scatter(prior, self.Hn, self.gn)
        self.unit_H, self.unit_g = scatter(prior, self.unit_Hn, self.unit_gn)
        self.g0 = scatter(prior, self.Hn, self.g0n)[1]

    def jac_blocks(self):
        """the Jacobian blocks as Evaluate hands them out: J0's columns, a zero seventh column behind a pose's six"""
        J0 = self.prior.J()
        out = []
        for kind, fr, idx, col0, ls, gs in blocks(self.prior):
            Jb = np.zeros((self.n, gs))
            Jb[:, :ls] = J0[:, idx:idx + ls]
            out.append(Jb)
        return out


def rows(prior, x):
    """the prior as a residual block of step_ref.Problem.rows: r and the column blocks of J0 in long double"""
    ref = Ref(prior, x)
    J0 = prior.J().astype(LD)
    return ("prior", 1.0, False, ref.r, [(col0, J0[:, idx:idx + ls]) for kind, fr, idx, col0, ls, gs in blocks(prior)])


def prior_rows(problem, x):
    """the opt-in hook of step_ref.Problem(w, opt, prior_rows=prior_ref.prior_rows)"""
    return rows(problem.w.prior, dict(pose=x["pose"], sb=x["sb"], ex=x["ex"]))


# ---- float64 restatements: the yardsticks --------------------------------------------------------------------------------
def restate64(prior, x, form="ref", mutate=None, ex_free=True):
    """dx, r, Hn, gn, H, g, cost in float64.  form "ref": g = J0^T (r0 + J0 dx), the reference's formulation; "dev": g = g0 + H dx
    with H = J0^T J0 and g0 = J0^T r0, the device's.  r is summed as Evaluate sums it: r0 first, then column after column.
    mutate: one of MUTATIONS (test_prior_reference.py: each has to show on a named case)"""
    J0, r0 = prior.J(), prior.r()
    n = prior.n
    dx, _ = dx_of(prior, x, np.float64, mutate)
    Jr = J0.copy()
    if mutate == "d":                      # the tail loop over the columns from 48 on, forgotten
        Jr[:, 48:] = 0.0
    r = r0.copy()
    if mutate == "e":                      # the second row pass reading r0 of its first-pass row
        r[64:] = r0[:max(n - 64, 0)]
    for c in range(n):
        r = r + Jr[:, c] * dx[c]
    Hn = J0.T @ J0
    if mutate == "f" and n >= 32:          # one off-diagonal 16 x 16 tile taken from J0 J0^T
        Hn[16:32, 0:16] = (J0 @ J0.T)[16:32, 0:16]
    if form == "ref":
        gn = J0.T @ r
    else:
        g0 = np.zeros(n) if mutate == "h" else J0.T @ r0
        gn = g0 + Hn @ dx
    if not ex_free:                        # the constant block's rows and columns go, its dx has gone into r and g
        for kind, fr, idx, col0, ls, gs in blocks(prior):
            if kind == 2:
                Hn[idx:idx + ls, :], Hn[:, idx:idx + ls], gn[idx:idx + ls] = 0.0, 0.0, 0.0
    H, g = scatter(prior, Hn, gn, ex_free, mutate, np.float64)
    return dict(dx=dx, r=r, Hn=Hn, gn=gn, H=H, g=g, cost=0.5 * float(r @ r))


def rho(dev, ref, unit):
    """max |dev - ref| / unit over the entries with a unit (the others are structural zeros)"""
    dev, ref, unit = np.asarray(dev, LD), np.asarray(ref, LD), np.asarray(unit, LD)
    m = unit > 0
    return float((np.abs(dev - ref)[m] / unit[m]).max()) if m.any() else 0.0


QUANTITIES = ("dx", "r", "H", "g", "cost")


def rhos(got, ref):
    """rho of dx, r, H, g (camera index) and cost of a restatement (or anything with those keys) against a Ref"""
    return dict(dx=rho(got["dx"], ref.dx, ref.unit_dx), r=rho(got["r"], ref.r, ref.unit_r), H=rho(got["H"], ref.H, ref.unit_H),
                g=rho(got["g"], ref.g, ref.unit_g), cost=float(abs(LD(got["cost"]) - ref.cost) / ref.unit_cost))


# Yardsticks: the worst rho of restate64(form="ref") over the three state families of every prior of prior_inputs.py
# (`python tests/prior_ref.py` prints this table; "u" rows of unit scale, "s" row scales over 10^[-3, 7]).
YARDSTICK = {
    "n21u": dict(dx=0.738, r=0.355, H=0.848, g=0.186, cost=0.324),   # g0 + H dx: g=0.312
    "n21s": dict(dx=0.842, r=0.384, H=1.31, g=0.584, cost=0.101),   # g0 + H dx: g=0.446
    "n48u": dict(dx=0.524, r=0.579, H=1.46, g=0.264, cost=0.0687),   # g0 + H dx: g=0.143
    "n48s": dict(dx=0.605, r=0.399, H=1.92, g=0.286, cost=0.0155),   # g0 + H dx: g=0.168
    "n51u": dict(dx=0.986, r=0.395, H=1.17, g=0.307, cost=0.0206),   # g0 + H dx: g=0.11
    "n51s": dict(dx=0.715, r=0.302, H=3.19, g=0.384, cost=0.102),   # g0 + H dx: g=0.381
    "n63u": dict(dx=0.765, r=0.467, H=1.04, g=0.325, cost=0.0261),   # g0 + H dx: g=0.118
    "n63s": dict(dx=0.655, r=0.529, H=3.22, g=0.155, cost=0.146),   # g0 + H dx: g=0.172
    "n66u": dict(dx=0.329, r=0.501, H=1.11, g=0.25, cost=0.0165),   # g0 + H dx: g=0.183
    "n66s": dict(dx=0.642, r=0.533, H=3.31, g=0.116, cost=0.0352),   # g0 + H dx: g=0.18
    "n75u": dict(dx=0.933, r=0.295, H=1.75, g=0.198, cost=0.0748),   # g0 + H dx: g=0.151
    "n75s": dict(dx=1.03, r=0.477, H=2.05, g=0.319, cost=0.0445),   # g0 + H dx: g=0.14
    "n81u": dict(dx=0.854, r=0.464, H=1.16, g=0.155, cost=0.0707),   # g0 + H dx: g=0.153
    "n81s": dict(dx=0.736, r=0.349, H=3.43, g=0.197, cost=0.065),   # g0 + H dx: g=0.213
    "n111u": dict(dx=0.766, r=0.539, H=2.63, g=0.293, cost=0.0657),   # g0 + H dx: g=0.159
    "n111s": dict(dx=0.705, r=0.788, H=3.38, g=0.192, cost=0.068),   # g0 + H dx: g=0.133
    "n117u": dict(dx=0.585, r=0.434, H=2.01, g=0.252, cost=0.0322),   # g0 + H dx: g=0.143
    "n117s": dict(dx=0.455, r=0.49, H=4.5, g=0.237, cost=0.0737),   # g0 + H dx: g=0.393
    "n171u": dict(dx=0.694, r=0.321, H=2.68, g=0.107, cost=0.0146),   # g0 + H dx: g=0.0877
    "n171s": dict(dx=0.824, r=0.379, H=5.63, g=0.097, cost=0.0246),   # g0 + H dx: g=0.14
    # the cost at the candidate of the first step (yardstick_step; prior_inputs.step_window)
    "n171u_step": dict(cost=0.0207),   # cost 0.237 at the candidate, 37.7 before
    "n75u_imu_step": dict(cost=3.31),   # cost 5.14e+03 at the candidate, 6.82e+05 before
}
MARGIN = 8.0      # as step_ref.MARGIN: the same order of rounding as the yardstick, not the same bits


def bar(what, pid):
    """what a device ratio may reach on prior `pid`: MARGIN * max(yardstick, 1)"""
    return MARGIN * max(YARDSTICK[pid][what], 1.0)


def measure(form="ref"):
    import prior_inputs as pi
    out = {}
    for pid in pi.PRIORS:
        worst = dict.fromkeys(QUANTITIES, 0.0)
        for fam in pi.FAMILIES:
            prior, x = pi.case(pid, fam)
            got = rhos(restate64(prior, x, form), Ref(prior, x))
            worst = {k: max(worst[k], got[k]) for k in QUANTITIES}
        out[pid] = worst
    return out


# ---- the cost at the candidate of the first step (k_cost, k_solve) ------------------------------------------------------------
def cost_at(w, opt, x):
    """(cost, unit) of a window without landmarks at the states x = dict(pose, sb, ex): the prior's r^T r / 2 and, where the
    window has IMU factors, imu_ref's long-double share, the units added"""
    import imu_ref as ir
    ref = Ref(w.prior, x, bool(opt.estimate_extrinsic))
    cost, unit = ref.cost, float(ref.unit_cost)
    if ir.active(w):
        share = ir.Share(w, x["pose"], x["sb"], opt.g_norm)
        cost, unit = cost + share.cost, unit + share.unit_cost
    return cost, unit


def cost64_at(w, opt, x, order=None):
    import imu_ref as ir
    cost = restate64(w.prior, x)["cost"]
    if ir.active(w):
        cost += ir.share64(w, x["pose"], x["sb"], opt.g_norm, order)[2]
    return cost


def candidate(which):
    """the reference's own first step on a step window of prior_inputs.py: (window, options, Problem, x0, Lin, step, candidate)"""
    import prior_inputs as pi
    import step_ref as sr
    w, opt = pi.step_window(which)
    prob = sr.Problem(w, opt, prior_rows=prior_rows)
    x0 = prob.initial_state()
    lin = prob.linearize(x0)
    st = sr.step(lin.H, lin.g, lin.J)
    return w, opt, prob, x0, lin, st, prob.plus(x0, st["delta"])


def yardstick_step(which, seed):
    """rho_ref of the cost at the candidate: the float64 restatement at states one ulp from the reference's candidate, the IMU
    factors in a shuffled order (as imu_ref.yardstick_step)"""
    import imu_ref as ir
    import step_ref as sr
    w, opt, prob, x0, lin, st, xc = candidate(which)
    rng = np.random.default_rng(seed)
    x = sr.perturbed(dict(pose=xc["pose"], sb=xc["sb"], ex=xc["ex"]), rng)
    cost, unit = cost_at(w, opt, xc)
    c64 = cost64_at(w, opt, x, rng.permutation(len(ir.active(w))) if ir.active(w) else None)
    return dict(cost=float(abs(LD(c64) - cost)) / unit, at=float(cost), before=float(lin.cost))


STEP_WINDOWS = ("n171u_step", "n75u_imu_step")


if __name__ == "__main__":
    dev = measure("dev")
    for pid, y in measure().items():
        print('    "%s": dict(dx=%.3g, r=%.3g, H=%.3g, g=%.3g, cost=%.3g),   # g0 + H dx: g=%.3g'
              % (pid, y["dx"], y["r"], y["H"], y["g"], y["cost"], dev[pid]["g"]))
    for k, which in enumerate(STEP_WINDOWS):
        y = yardstick_step(which, 3000 + k)
        print('    "%s": dict(cost=%.3g),   # cost %.3g at the candidate, %.3g before' % (which, y["cost"], y["at"], y["before"]))
