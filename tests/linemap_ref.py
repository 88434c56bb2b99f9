"""The line-map stage that runs before every main solve -- FeatureManager::triangulateLine, FeatureManager::triangulate and
Estimator::onlyLineOpt with its removeLineOutlier -- in any NumPy dtype, np.longdouble by default: the reference
test_linemap_reference.py checks on the CPU and holds the oracle to, and test_gpu_linemap.py holds k_triangulate,
k_triangulate_points, k_line_opt (4, 2 and 1 lanes per line) and k_gauge's setLineOrth + removeLineOutlier to.  Run with
dt = np.float64, the factors summed in a shuffled order at states, lines and observations one ulp away, it is the yardstick.

Written from feature_manager.cpp (triangulateLine :413-563, triangulate :565-621, setLineOrth :367-388, reprojection_error
:390-411, removeLineOutlier :702-798), line_geometry.cpp (pi_from_ppp, pipi_plk, plk_to_pose, plk_from_pose) and estimator.cpp
(onlyLineOpt :950-1039, vector2double / double2vector); the minimiser is ceres-solver 1.12's TrustRegionMinimizer +
LevenbergMarquardtStrategy + CauchyLoss(1) with the corrector, by the rule list of DESIGN.md 2 (ceres' sources are not in this
tree): Jacobi scaling 1 / (1 + |col|) fixed at iteration 0, (S H S + diag / radius) y = S g per line (every line is its own
e-block of DENSE_SCHUR, the cameras being constant), diag = clamp(diag(S H S), 1e-6, 1e32) kept after a rejected step,
model_cost_change = -m.(r + m / 2) with m = J_s step, the parameter and function tolerances tested on the candidate BEFORE the
iteration is recorded, rho = cost_change / model_cost_change > 1e-3 accepts, radius / max(1/3, 1 - (2 rho - 1)^3) capped at 1e16
on accept with decrease_factor back to 2, radius / decrease_factor and decrease_factor * 2 on reject.  The factor, the
parameterisation, the loss and the conversions are vis_ref's; neither the oracle nor vpl_math.h is called.

Every branch decision is recorded with its margin, relative to the size of what is compared (`margins`): a case is only a case
if all float64 yardstick runs take the long-double run's decisions and the smallest margin is >= MARGIN_FACTOR x the largest
relative deviation those runs show in what is compared (condition()).

Units (rho = error / unit).  A triangulated Pluecker vector and an inverse depth: vis_ref.units' rule, eps64 |f_k| + sum_i
|f_k(x + spacing(x_i) e_i) - f_k(x)| over the non-zero inputs, in long double.  Costs: eps64 x cost.  A line after the loop: the
camera-frame Pluecker vector normalised to |n|^2 + |v|^2 = 1, up to the common sign, eps64 per entry; what the loop amplifies is in
the yardstick, not in the unit.  Bar = step_ref.MARGIN x max(yardstick, 1) per case and quantity; onlyLineOpt's per iteration
count k too.  `python tests/linemap_ref.py` prints the tables YARDSTICK was copied from."""
import functools

import numpy as np

import step_ref as sr
import vis_ref as vr
import vplines_slam_amd as v
from imu_ref import _q, qmat, skew

LD = sr.LD
assert np.finfo(LD).eps < 1e-18, "np.longdouble is not an extended type here: restate the linear algebra below with mpmath"
EPS64 = sr.EPS64
MARGIN = sr.MARGIN
MARGIN_FACTOR = 1e3                  # smallest decision margin >= this x the largest relative deviation of the yardstick runs
COS_MAX, DEPTH_MIN = 0.998, 0.1      # feature_manager.cpp:492, :615
ERASE_DIST, ERASE_ERR = 10.0, 3.0 / 500.0     # :760, :792
RADIUS0, MAX_RADIUS, MIN_RADIUS = 1e4, 1e16, 1e-32
MIN_DIAG, MAX_DIAG = 1e-6, 1e32
MIN_REL_DECREASE, F_TOL, P_TOL, G_TOL = 1e-3, 1e-6, 1e-8, 1e-10
MAX_INVALID = 5
SEEDS = (5000, 5001, 5002)           # of the yardstick runs
VARIANTS = ("no_jacobi", "no_reuse", "stale_diagonal", "no_reset", "no_cube", "no_corrector_J", "drop_sub1", "cos_0.99", "depth_0",
            "last_obs")


def _norm(a):
    return np.sqrt(a @ a)


def cameras(pose, ex, dt=LD):
    """[(Rwc, twc)] per frame: Rs the matrix of the normalised quaternion, Rwc = Rs ric, twc = Ps + Rs tic"""
    pose, ex = np.asarray(pose, dt), np.asarray(ex, dt)
    qe = _q(ex, dt)
    ric, tic = qmat(qe / _norm(qe)), ex[:3]
    out = []
    for p in pose:
        q = _q(p, dt)
        Rs = qmat(q / _norm(q))
        out.append((Rs @ ric, p[:3] + Rs @ tic))
    return out


def vector2double(pose, ex):
    """float64 parameter blocks as vector2double leaves them: the quaternion of the normalised quaternion's matrix"""
    pose, ex = np.array(pose, np.float64), np.array(ex, np.float64)
    for q in list(pose[:, 3:]) + [ex[3:]]:
        q[:] = sr.R_quat(sr.quat_R(q / np.linalg.norm(q)))
    return pose, ex


def _rel(a, b):
    """|a - b| relative to the larger of the two"""
    a, b = float(a), float(b)
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else 0.0


# ---- FeatureManager::triangulateLine ---------------------------------------------------------------------------------------
def pi_from_ppp(x1, x2, x3):
    return np.concatenate([np.cross(x1 - x3, x2 - x3), [-(x3 @ np.cross(x1, x2))]])


def pipi_plk(pi1, pi2):
    dp = np.outer(pi1, pi2) - np.outer(pi2, pi1)
    return np.array([dp[0, 3], dp[1, 3], dp[2, 3], -dp[1, 2], dp[0, 2], -dp[0, 1]], pi1.dtype)


def triangulate_line(pose, ex, obs, dt=LD, variant=None):
    """pose [no, 7]: the frames of the track from its start frame, obs [no, >= 4] -> (plk [6] in the start camera frame or None
    = left untriangulated, decisions: chosen observation, min_cos, m_argmin = runner-up - smallest cosine, m_cos = |min_cos - 0.998|)"""
    cams = cameras(pose, ex, dt)
    ob = np.asarray(obs, dt)
    one = dt(1)
    R0, t0 = cams[0]
    pii = pi_from_ppp(np.array([ob[0, 0], ob[0, 1], one]), np.array([ob[0, 2], ob[0, 3], one]), np.zeros(3, dt))
    ni = pii[:3] / _norm(pii[:3])
    cos, planes = [], []
    for k in range(1, len(ob)):
        R1, t1 = cams[k]
        t = R0.T @ (t1 - t0)
        R = R0.T @ R1
        p3 = R @ np.array([ob[k, 0], ob[k, 1], one]) + t
        p4 = R @ np.array([ob[k, 2], ob[k, 3], one]) + t
        pij = pi_from_ppp(p3, p4, t)
        cos.append(ni @ (pij[:3] / _norm(pij[:3])))
        planes.append(pij)
    dec = dict(chosen=-1, min_cos=1.0, m_argmin=np.inf, m_cos=np.inf)
    below = [k for k, c in enumerate(cos) if c < one]          # min_cos_theta starts at 1.0 and is replaced on `<`
    if not below:
        return None, dec
    k = min(below, key=lambda j: (cos[j], j))
    if variant == "last_obs":
        k = len(cos) - 1
    rest = sorted(float(c) for j, c in enumerate(cos) if j != k)
    cmax = dt(0.99) if variant == "cos_0.99" else dt(COS_MAX)
    dec = dict(chosen=k + 1, min_cos=float(cos[k]), m_argmin=(rest[0] - float(cos[k])) if rest else np.inf,
               m_cos=abs(float(cos[k] - dt(COS_MAX))))
    if cos[k] > cmax:
        return None, dec
    return pipi_plk(pii, planes[k]), dec


# ---- FeatureManager::triangulate ---------------------------------------------------------------------------------------------
def hestenes(A):
    """one-sided Jacobi SVD in A's dtype: (squared singular values [n], V [n, n]) of A [m, n], A V = U diag(sigma)"""
    A = A.copy()
    n = A.shape[1]
    V = np.eye(n, dtype=A.dtype)
    eps = np.finfo(A.dtype).eps
    for _ in range(60):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                al, be, ga = A[:, p] @ A[:, p], A[:, q] @ A[:, q], A[:, p] @ A[:, q]
                if ga == 0 or abs(ga) <= eps * np.sqrt(al * be):
                    continue
                rotated = True
                zeta = (be - al) / (2 * ga)
                t = (1 if zeta >= 0 else -1) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = 1 / np.sqrt(1 + t * t)
                s = c * t
                for M in (A, V):
                    a, b = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = c * a - s * b, s * a + c * b
        if not rotated:
            break
    return np.array([A[:, j] @ A[:, j] for j in range(n)], A.dtype), V


def dlt_rows(pose, ex, obs, dt=LD):
    """svd_A [2 no, 4] of feature_manager.cpp:587-605 in the start camera frame"""
    cams = cameras(pose, ex, dt)
    ob = np.asarray(obs, dt)
    R0, t0 = cams[0]
    rows = []
    for k in range(len(ob)):
        R1, t1 = cams[k]
        t = R0.T @ (t1 - t0)
        R = R0.T @ R1
        P = np.concatenate([R.T, (-(R.T @ t))[:, None]], axis=1)
        f = ob[k, :3] / _norm(ob[k, :3])
        rows += [f[0] * P[2] - f[2] * P[0], f[1] * P[2] - f[2] * P[1]]
    return np.array(rows, dt)


def triangulate_point(pose, ex, obs, init_depth=5.0, dt=LD, variant=None):
    """-> (depth as estimated_depth is left, decisions: svd depth, m_depth = |depth - 0.1| relative)"""
    s2, V = hestenes(dlt_rows(pose, ex, obs, dt))
    vv = V[:, int(np.argmin(s2))]
    depth = vv[2] / vv[3]
    dec = dict(svd_depth=float(depth), used_init=bool(depth < (0.0 if variant == "depth_0" else DEPTH_MIN)), m_depth=_rel(depth, DEPTH_MIN))
    return (dt(init_depth) if dec["used_init"] else depth), dec


# ---- removeLineOutlier (one line) ------------------------------------------------------------------------------------------------
def remove_line_outlier(plk, cams, obs, dt=LD):
    """plk [6] in the start camera frame, cams: (Rwc, twc) of the track's frames, obs [no, >= 4] -> (erased, rule 0 = kept / 1 =
    behind the camera / 2 = end points more than 10 apart / 3 = reprojection error, margins of the rules evaluated)"""
    plk, ob = np.asarray(plk, dt), np.asarray(obs, dt)
    one, zero = dt(1), dt(0)
    nc, vc = plk[:3], plk[3:]
    Lc = np.zeros((4, 4), dt)
    Lc[:3, :3], Lc[:3, 3], Lc[3, :3] = skew(nc), vc, -vc
    p11, p21 = np.array([ob[0, 0], ob[0, 1], one]), np.array([ob[0, 2], ob[0, 3], one])
    ln = np.cross(p11, p21)[:2]
    ln = ln / _norm(ln)
    p12, p22 = np.array([p11[0] + ln[0], p11[1] + ln[1], one]), np.array([p21[0] + ln[0], p21[1] + ln[1], one])
    cam = np.zeros(3, dt)
    e1, e2 = Lc @ pi_from_ppp(cam, p11, p12), Lc @ pi_from_ppp(cam, p21, p22)
    e1, e2 = e1 / e1[3], e2 / e2[3]
    m = dict(behind=float(min(abs(e1[2]), abs(e2[2])) / max(_norm(e1[:3]), _norm(e2[:3]))))
    if e1[2] < zero or e2[2] < zero:
        return True, 1, m
    d = _norm(e1 - e2)
    m["dist"] = _rel(d, ERASE_DIST)
    if d > dt(ERASE_DIST):
        return True, 2, m
    Rwc, twc = cams[0]
    line_w = vr._plk_to_pose(plk, Rwc, twc)
    allerr = zero
    for k in range(len(ob)):
        n = vr._plk_from_pose(line_w, cams[k][0], cams[k][1])[:3]
        n = n / _norm(n[:2])
        err = (abs(n @ np.array([ob[k, 0], ob[k, 1], one])) + abs(n @ np.array([ob[k, 2], ob[k, 3], one]))) / 2
        if allerr < err:
            allerr = err
    m["err"] = _rel(allerr, ERASE_ERR)
    if allerr > dt(3.0) / dt(500.0):
        return True, 3, m
    return False, 0, m


# ---- Estimator::onlyLineOpt ----------------------------------------------------------------------------------------------------
def perturbed_window(w, rng):
    """a copy of w with poses, extrinsic, lines, observations and inverse depths one relative ulp away"""
    w2 = w.copy()
    x = sr.perturbed(dict(pose=w.pose, ex=w.ex_pose, plk=w.line_plk, lobs=w.line_obs, pobs=w.point_obs), rng)
    w2.pose[:], w2.ex_pose[:], w2.line_plk[:], w2.line_obs[:], w2.point_obs[:] = x["pose"], x["ex"], x["plk"], x["lobs"], x["pobs"]
    return w2


class LineProblem:
    """the residual blocks onlyLineOpt adds (vis_ref.line_opt_rows) with their evaluation in dtype dt; `order` shuffles the order in
    which the factors enter the sums"""

    def __init__(self, w, opt, dt=LD, variant=None, rng=None):
        self.dt, self.variant, self.si = dt, variant, opt.line_factor
        self.pose, self.ex = vector2double(w.pose, w.ex_pose)
        P, O = vr.line_opt_rows(w, opt, self.pose, self.ex, w.line_plk)
        self.lines = np.nonzero(np.asarray(w.line_triangulated[:len(w.line_start)]) != 0)[0]
        self.nL = len(self.lines)
        nobs = [int(w.line_nobs[l]) for l in self.lines]
        self.seg = np.concatenate([[0], np.cumsum(nobs)]).astype(int)
        self.P, self.O = np.asarray(P, dt).reshape(-1, 18), np.asarray(O, dt).reshape(-1, 4)
        self.line_of = np.repeat(np.arange(self.nL), nobs)
        keep = np.ones(len(self.line_of), bool)
        if variant == "drop_sub1":               # a track of 2 whose second observation no lane takes
            for l, n in enumerate(nobs):
                if n == 2:
                    keep[self.seg[l] + 1] = False
        self.factors = np.nonzero(keep)[0]
        self.order = self.factors if rng is None else rng.permutation(self.factors)
        self.orth0 = np.array([self.P[self.seg[l], 14:18] for l in range(self.nL)], dt).reshape(self.nL, 4)
        self.starts = [int(w.line_start[l]) for l in self.lines]
        loff = np.concatenate([[0], np.cumsum(w.line_nobs)]).astype(int)
        self.obs = [np.asarray(w.line_obs[loff[l]:loff[l + 1], :4], dt) for l in self.lines]
        self.cams = cameras(self.pose, self.ex, dt)

    def evaluate(self, orth, want_jac):
        """-> cost, H [nL, 4, 4], g [nL, 4], [(line, corrected J [2, 4], corrected r [2])] at orth [nL, 4]"""
        dt = self.dt
        cost, H, g, rows = dt(0), np.zeros((self.nL, 4, 4), dt), np.zeros((self.nL, 4), dt), []
        for f in self.order:
            l = self.line_of[f]
            x = np.concatenate([self.P[f, :14], orth[l], self.O[f]])
            out = vr._line1(x, self.si, dt, want_jac)
            r = out[:2]
            rho, sq = vr.cauchy(r @ r, 1.0, dt)
            cost = cost + rho / 2
            if want_jac:
                J = out[2 + 28:2 + 36].reshape(2, 4)
                Jc, rc = (J if self.variant == "no_corrector_J" else J * sq), r * sq
                H[l] = H[l] + Jc.T @ Jc
                g[l] = g[l] + Jc.T @ rc
                rows.append((l, Jc, rc))
        return cost, H, g, rows

    def plus(self, orth, delta):
        return np.stack([vr._orth_plus1(np.concatenate([a, b]), self.dt) for a, b in zip(orth, delta)])

    def hand_back(self, orth):
        """setLineOrth: the camera-frame Pluecker vectors [nL, 6] of world orth [nL, 4]"""
        return np.stack([vr._plk_from_pose(vr.orth_to_plk(orth[l], self.dt), *self.cams[self.starts[l]]) for l in range(self.nL)])

    def outliers(self, plk):
        """removeLineOutlier on the handed-back lines -> [(erased, rule, margins)]"""
        return [remove_line_outlier(plk[l], self.cams[self.starts[l]:self.starts[l] + len(self.obs[l])], self.obs[l], self.dt)
                for l in range(self.nL)]


def _chol_solve(A, b):
    """(A^-1 b, smallest pivot relative to its diagonal entry) by Cholesky; None when a pivot is not positive"""
    n = len(b)
    L = np.zeros_like(A)
    worst = np.inf
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        worst = min(worst, float(d / A[j, j]) if A[j, j] > 0 else -np.inf)
        if not d > 0:
            return None, worst
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return sr.solve_upper(L.T, sr.solve_lower(L, b, A.dtype), A.dtype), worst


def only_line_opt(w, opt, dt=LD, variant=None, rng=None, cap=None):
    """the whole of onlyLineOpt on Window w (not modified) with at most `cap` iterations (default opt.num_iterations).  Returns a
    dict: report (iterations, successful, termination 0 = iteration cap / 1 = convergence / 2 = failure, initial_cost, final_cost),
    states[k] = (orth [nL, 4], cost, successful steps) after k attempted steps (a run capped at k <= iterations stops there: at()),
    trace (one record per attempted step), margins (every comparison made, relative), problem"""
    cap = opt.num_iterations if cap is None else cap
    prob = LineProblem(w, opt, dt, variant, rng)
    if prob.nL < 4:                       # "if (feature_index < 3) return;": nothing runs, removeLineOutlier included
        return dict(report=dict(iterations=0, successful=0, termination=0, initial_cost=0.0, final_cost=0.0), states=[], trace=[],
                    margins={}, problem=prob, ran=False)
    nL = prob.nL
    x = prob.orth0.copy()
    cost, H, g, rows = prob.evaluate(x, True)
    initial_cost = cost
    idx = np.arange(4)
    scale = np.ones((nL, 4), dt) if variant == "no_jacobi" else 1 / (1 + np.sqrt(H[:, idx, idx]))
    margins, trace = {}, []

    def note(name, val):
        margins[name] = min(margins.get(name, np.inf), float(val))

    def grad_max():
        return max(float(np.abs(x[l] - prob.plus(x[l:l + 1], -g[l:l + 1])[0]).max()) for l in range(nL))

    gmax = grad_max()
    x_norm = np.sqrt((x * x).sum())
    radius, decrease, reuse, diag = dt(RADIUS0), dt(2), False, None
    it = nsucc = ninvalid = 0
    states = [(x.copy(), cost, 0)]
    note("gmax", _rel(gmax, G_TOL))
    term = 1 if gmax <= G_TOL else None
    while term is None:
        if it >= cap:
            term = 0
            break
        it += 1
        # LevenbergMarquardtStrategy::ComputeStep
        Hs = scale[:, :, None] * H * scale[:, None, :]
        gs = scale * g
        if (not reuse or variant == "no_reuse") and not (variant == "stale_diagonal" and diag is not None):
            diag = np.clip(Hs[:, idx, idx], dt(MIN_DIAG), dt(MAX_DIAG))
        step, fail, piv = np.zeros((nL, 4), dt), False, np.inf
        for l in range(nL):
            y, p = _chol_solve(Hs[l] + np.diag(diag[l] / radius), gs[l])
            piv = min(piv, p)
            if y is None or not np.all(np.isfinite(np.asarray(y, np.float64))):
                fail = True
            else:
                step[l] = -y
        note("pivot", piv)
        rec = dict(radius=float(radius), reused=bool(reuse), diag=np.asarray(diag, np.float64).copy(), decrease_factor=float(decrease))
        reuse = True
        mcc = dt(0)
        for l, Jc, rc in rows:
            m = (Jc * scale[l]) @ step[l]
            mcc = mcc - m @ (rc + m / 2)
        rec["model_cost_change"] = float(mcc)
        note("model_cost_change", abs(float(mcc / cost)))
        if fail or not mcc > 0:
            ninvalid += 1
            rec.update(valid=False, accepted=False)
            trace.append(rec)
            if ninvalid >= MAX_INVALID:
                term, it = 2, it - 1
                break
            radius, decrease = radius / decrease, decrease * 2          # StepIsInvalid: treated as a rejected step
            states.append((x.copy(), cost, nsucc))
            continue
        ninvalid = 0
        cand = prob.plus(x, step * scale)
        cand_cost = prob.evaluate(cand, False)[0]
        step_norm = np.sqrt(((x - cand) ** 2).sum())
        change = cost - cand_cost
        rho = change / mcc
        rec.update(valid=True, candidate_cost=float(cand_cost), step_norm=float(step_norm), rho=float(rho))
        note("parameter_tolerance", abs(float(step_norm - P_TOL * (x_norm + P_TOL))) / float(x_norm))
        if step_norm <= P_TOL * (x_norm + P_TOL):
            rec.update(accepted=False, terminated="parameter")
            trace.append(rec)
            term, it = 1, it - 1
            break
        note("function_tolerance", abs(float(abs(change) - F_TOL * cost)) / float(cost))
        if abs(change) <= F_TOL * cost:
            rec.update(accepted=False, terminated="function")
            trace.append(rec)
            term, it = 1, it - 1
            break
        note("rho", abs(float(change - MIN_REL_DECREASE * mcc)) / float(cost))
        if rho > MIN_REL_DECREASE:
            x = cand
            cost, H, g, rows = prob.evaluate(x, True)
            x_norm = np.sqrt((x * x).sum())
            gmax = grad_max()
            nsucc += 1
            shrink = 1 - (2 * rho - 1) if variant == "no_cube" else 1 - (2 * rho - 1) ** 3
            radius = min(dt(MAX_RADIUS), radius / max(dt(1) / 3, shrink))
            if variant != "no_reset":
                decrease = dt(2)
            reuse = False
            rec["accepted"] = True
        else:
            radius, decrease, reuse = radius / decrease, decrease * 2, True
            rec["accepted"] = False
        trace.append(rec)
        states.append((x.copy(), cost, nsucc))
        if rec["accepted"]:
            note("gmax", _rel(gmax, G_TOL))
            if gmax <= G_TOL:
                term = 1
                break
        if radius < MIN_RADIUS:
            term = 1
            break
    return dict(report=dict(iterations=it, successful=nsucc, termination=term, initial_cost=initial_cost, final_cost=cost), states=states,
                trace=trace, margins=margins, problem=prob, ran=True)


def at(res, k):
    """what a run capped at k iterations leaves: (report, orth, plk [nL, 6], [(erased, rule, margins)])"""
    prob, full = res["problem"], res["report"]
    if not res["ran"]:
        return dict(full), None, None, []
    if k > full["iterations"] or (k == full["iterations"] and full["termination"] == 0):
        rep = dict(full)
        orth = res["states"][-1][0]
    else:
        orth, cost, nsucc = res["states"][k]
        rep = dict(iterations=k, successful=nsucc, termination=0, initial_cost=full["initial_cost"], final_cost=cost)
    plk = prob.hand_back(orth)
    return rep, orth, plk, prob.outliers(plk)


def unit_plk(plk, dt=LD):
    plk = np.asarray(plk, dt)
    return plk / np.sqrt((plk * plk).sum(axis=-1, keepdims=True))


def rho_lines(got, ref):
    """worst |u - u_ref| / eps64 over the lines, u the normalised Pluecker vectors up to the common sign"""
    a, b = unit_plk(got), unit_plk(ref)
    err = np.minimum(np.abs(a - b).max(axis=-1), np.abs(a + b).max(axis=-1))
    return float(err.max() / EPS64) if err.size else 0.0


def rho_cost(got, ref):
    return float(abs(LD(got) - LD(ref)) / (EPS64 * LD(ref))) if ref != 0 else (0.0 if got == 0 else np.inf)


def decisions(res):
    """what a run decided, as comparable data: the trace of (valid, accepted, terminated), the report's integers and the erase rules
    after every iteration count"""
    tr = tuple((r["valid"], r["accepted"], r.get("terminated")) for r in res["trace"])
    rep = res["report"]
    rules = tuple(tuple(o[1] for o in at(res, k)[3]) for k in range(1, rep["iterations"] + 2)) if res["ran"] else ()
    return tr, (rep["iterations"], rep["successful"], rep["termination"]), rules


# ---- units of the two triangulations -----------------------------------------------------------------------------------------
def _units(f, x):
    """vis_ref.units' rule for f(x) -> [m] at float64 x"""
    x = np.asarray(x, np.float64)
    f0 = f(x)
    u = EPS64 * np.abs(f0)
    for i in np.nonzero(x)[0]:
        xp = x.copy()
        xp[i] = x[i] + np.spacing(abs(x[i]))
        u = u + np.abs(f(xp) - f0)
    return f0, np.asarray(u, np.float64)


def line_track(w, l):
    """(pose rows of the track, obs [no, 4]) of line l"""
    off = int(np.sum(w.line_nobs[:l]))
    s, no = int(w.line_start[l]), int(w.line_nobs[l])
    return w.pose[s:s + no], w.line_obs[off:off + no, :4]


def point_track(w, p):
    off = int(np.sum(w.point_nobs[:p]))
    s, no = int(w.point_start[p]), int(w.point_nobs[p])
    return w.pose[s:s + no], w.point_obs[off:off + no]


def line_units(w, l):
    """(plk long double [6], unit [6]) of the triangulation of line l of w; None, None when it stays untriangulated"""
    pose, obs = line_track(w, l)
    no = len(obs)
    if triangulate_line(pose, w.ex_pose, obs)[0] is None:
        return None, None
    f = lambda x: triangulate_line(x[:7 * no].reshape(no, 7), x[7 * no:7 * no + 7], x[7 * no + 7:].reshape(no, 4))[0]
    return _units(f, np.concatenate([pose.ravel(), w.ex_pose, obs.ravel()]))


def point_units(w, p, init_depth=5.0):
    """(inverse depth long double, unit) of the triangulation of point track p (0 where init_depth is taken: the exact bits)"""
    pose, obs = point_track(w, p)
    no = len(obs)
    d, dec = triangulate_point(pose, w.ex_pose, obs, init_depth)
    if dec["used_init"]:
        return 1 / d, 0.0
    f = lambda x: np.array([1 / triangulate_point(x[:7 * no].reshape(no, 7), x[7 * no:7 * no + 7], x[7 * no + 7:].reshape(no, 3),
                                                  init_depth)[0]])
    f0, u = _units(f, np.concatenate([pose.ravel(), w.ex_pose, obs.ravel()]))
    return f0[0], float(u[0])


# ---- the cases -----------------------------------------------------------------------------------------------------
def generate(seed, L=0, P=0, sigma_px=0.3, t=0.3, kf=1.0):
    """a window of full-length tracks (11 observations from frame 0), noise-free poses, the true map; kf stretches the time between
    keyframes (the parallax of the tracks)"""
    import oracle_api as o
    cfg = v.workload.config(P, L, True)
    cfg.track_len = 11
    cfg.pose_sigma_p = cfg.pose_sigma_theta_deg = 0.0
    cfg.pix_sigma = sigma_px / 460.0
    cfg.orth_sigma = 0.0
    cfg.depth_rel_sigma = 0.0
    cfg.kf_dt *= kf
    w = v.workload.generate(seed, cfg, t)
    o.preintegrate_windows([w], v.default_options())
    return w


def cut(w, line_nobs=None, point_nobs=None, lines=None, points=None):
    """w with the chosen tracks (default all) cut to their first n observations"""
    lines = np.arange(len(w.line_start)) if lines is None else np.asarray(lines, int)
    points = np.arange(len(w.point_start)) if points is None else np.asarray(points, int)
    ln = np.asarray(w.line_nobs)[lines] if line_nobs is None else np.asarray(line_nobs, np.int32)
    pn = np.asarray(w.point_nobs)[points] if point_nobs is None else np.asarray(point_nobs, np.int32)
    loff = np.concatenate([[0], np.cumsum(w.line_nobs)]).astype(int)
    poff = np.concatenate([[0], np.cumsum(w.point_nobs)]).astype(int)
    lobs = np.concatenate([w.line_obs[loff[l]:loff[l] + n] for l, n in zip(lines, ln)]) if len(lines) else w.line_obs[:0]
    pobs = np.concatenate([w.point_obs[poff[p]:poff[p] + n] for p, n in zip(points, pn)]) if len(points) else w.point_obs[:0]
    return v.capi.Window(w.pose, w.speed_bias, w.ex_pose, np.asarray(w.point_start)[points], pn, pobs, np.asarray(w.inv_depth)[points],
                         np.asarray(w.line_start)[lines], ln, lobs, np.asarray(w.line_plk)[lines], w.preint, None)


def options(num_iterations=8):
    opt = v.default_options()
    opt.num_iterations = num_iterations
    return opt


LANES = {12: 4, 100: 2, 200: 1}           # max_lines of a context -> lanes per line of k_line_opt
LO_NOBS = [2, 5, 11, 3, 7, 4]
LO_SEED = 7108
LO_PUSH = {"lo_reject": (1, 0.3), "lo_reject2": (2, 1.5)}     # case -> (line, angle its Pluecker normal is turned by about its direction)
FULL = {"lo_full_4": 64, "lo_full_2": 128, "lo_full_1": 256, "lo_full_65": 65}     # case -> max_lines = number of lines


def _perturb_map(w, seed, rel=0.02):
    rng = np.random.default_rng(seed)
    w.line_plk += rng.normal(0, rel, w.line_plk.shape) * np.abs(w.line_plk)
    return w


def _lo_base():
    return cut(generate(LO_SEED, L=6), line_nobs=LO_NOBS)


def _rotate_about(a, axis, ang):
    axis = axis / np.linalg.norm(axis)
    return a * np.cos(ang) + np.cross(axis, a) * np.sin(ang) + axis * (axis @ a) * (1 - np.cos(ang))


@functools.lru_cache(maxsize=None)
def lo_cases():
    """name -> (Window, iteration cap K of the sweep k = 1 .. K)"""
    out = {}
    out["lo_generic"] = (_perturb_map(_lo_base(), 1), 8)
    for name, (l, ang) in LO_PUSH.items():
        wr = _perturb_map(_lo_base(), 1)
        wr.line_plk[l, :3] = _rotate_about(wr.line_plk[l, :3], wr.line_plk[l, 3:], ang)
        out[name] = (wr, 8)
    out["lo_four"] = (_perturb_map(cut(_lo_base(), lines=[0, 1, 2, 3]), 2), 8)
    out["lo_three"] = (_perturb_map(cut(_lo_base(), lines=[0, 1, 2]), 3), 8)
    for name, n in FULL.items():
        wf = generate(7200 + n, L=n)
        out[name] = (_perturb_map(cut(wf, line_nobs=2 + np.arange(n) % 2), 4), 2)
    out.update(out_cases())
    return out


OUT_RULE = {"out_behind": (1, 1), "out_far": (2, 2), "out_err": (3, 3), "out_kept": (None, 0)}     # case -> (line, rule)
OUT_NOBS = [6, 4, 9, 5, 11]


def out_cases():
    """four windows of 5 lines; in the first three one rule of removeLineOutlier decides for one line after the loop"""
    out = {}
    base = lambda: _perturb_map(cut(generate(7301, L=5, sigma_px=0.1), line_nobs=OUT_NOBS), 5, 0.005)
    wb = base()
    wb.line_plk[1, :3] *= -1.0              # the mirror image through the camera centre: the same image lines, negative depth
    out["out_behind"] = (wb, 8)
    wf = base()
    p1, p2 = wf.line_obs[np.sum(OUT_NOBS[:2]), 0:2].copy(), wf.line_obs[np.sum(OUT_NOBS[:2]), 2:4].copy()
    wf.line_obs[np.sum(OUT_NOBS[:2]), 2:4] = p1 + OUT_STRETCH * (p2 - p1)     # line 2's first observation: one end moved along the image line
    out["out_far"] = (wf, 8)
    we = base()
    we.line_obs[np.sum(OUT_NOBS[:3]) + 2, [1, 3]] += 0.05        # one corrupted observation of line 3
    out["out_err"] = (we, 8)
    out["out_kept"] = (base(), 8)
    return out


OUT_STRETCH = 40.0


@functools.lru_cache(maxsize=None)
def lo_reference(name):
    """the long-double run of a case, capped at its K"""
    w, K = lo_cases()[name]
    return only_line_opt(w, options(K), cap=K)


@functools.lru_cache(maxsize=None)
def lo_yardstick_runs(name):
    w, K = lo_cases()[name]
    out = []
    for s in SEEDS:
        rng = np.random.default_rng(s)
        out.append(only_line_opt(perturbed_window(w, rng), options(K), dt=np.float64, rng=rng, cap=K))
    return out


def lo_compare(res, ref, k):
    """(rho of the initial cost, of the final cost, of the lines) of a run's state under cap k against the reference's"""
    rep, _, plk, _ = at(res, k)
    rrep, _, rplk, _ = at(ref, k)
    return rho_cost(rep["initial_cost"], rrep["initial_cost"]), rho_cost(rep["final_cost"], rrep["final_cost"]), rho_lines(plk, rplk)


def sweep(name):
    """the iteration caps at which a case is compared: 1 .. K, K the cap at which the reference terminates (or the case's cap)"""
    ref = lo_reference(name)
    K = lo_cases()[name][1]
    if not ref["ran"]:
        return [K]
    return list(range(1, min(K, ref["report"]["iterations"] + 1) + 1))


def lo_measure(name):
    """yardstick of a case: per k of the sweep the worst rho over the seeds (initial cost | final cost | lines), whether all runs took
    the reference's decisions, and the largest relative deviation of what is compared"""
    ref = lo_reference(name)
    runs = lo_yardstick_runs(name)
    same = all(decisions(r) == decisions(ref) for r in runs)
    ks = sweep(name)
    y = dict(cost0=0.0, cost=[0.0] * len(ks), line=[0.0] * len(ks))
    if ref["ran"] and same:
        for r in runs:
            for j, k in enumerate(ks):
                c0, c, ln = lo_compare(r, ref, k)
                y["cost0"], y["cost"][j], y["line"][j] = max(y["cost0"], c0), max(y["cost"][j], c), max(y["line"][j], ln)
    dev = EPS64 * max([y["cost0"]] + y["cost"] + y["line"])
    return y, same, dev


def condition(name):
    """(all yardstick runs took the reference's decisions, smallest relative margin of the case, largest relative deviation of what
    is compared in the yardstick runs): a case needs same and margin >= MARGIN_FACTOR x deviation"""
    _, same, dev = lo_measure(name)
    return same, min_margin(lo_reference(name))[0], dev


def min_margin(res):
    m = dict(res["margins"])
    for k in range(1, res["report"]["iterations"] + 2) if res["ran"] else ():
        for erased, rule, mm in at(res, k)[3]:
            for name, val in mm.items():
                m["erase_" + name] = min(m.get("erase_" + name, np.inf), val)
    return (min(m.values()) if m else np.inf), m


def lo_bar(name, what, k=None):
    y = YARDSTICK[name][what]
    if k is not None:
        y = y[sweep(name).index(k)]
    return MARGIN * max(y, 1.0)


# -- triangulation cases: name -> Window with line_triangulated / inv_depth set as the case needs ---------------------------------
INIT_DEPTH = 5.0


def _untriangulated(w):
    w.line_triangulated[:] = 0
    w.line_plk[:] = 0.0
    return w


TL_KF = 3.0          # keyframes three times as far apart: most tracks of two or three observations pass cos 0.998
TL_TARGETS = (0.9975, 0.9985, 0.9975, 0.9985)      # tl_threshold: the cosine of the two planes of lines 0 .. 3
_TL_ENDS = (([-0.3, 0.2, 1.0], [0.4, -0.1, 1.1]), ([0.2, 0.3, 1.0], [-0.2, -0.25, 0.9]), ([-0.4, -0.1, 1.0], [0.1, 0.35, 1.2]),
            ([0.3, -0.3, 1.0], [-0.1, 0.3, 1.05]))


def _tl_crafted(w):
    """w's lines (two observations each) replaced by the images of 3-D segments placed at the distance from the start camera at
    which the planes of the two observations make the cosines TL_TARGETS (bisection in float64; the farther, the less parallax)"""
    cams = cameras(w.pose, w.ex_pose, np.float64)
    off = np.concatenate([[0], np.cumsum(w.line_nobs)]).astype(int)
    for l, target in enumerate(TL_TARGETS):
        s = int(w.line_start[l])

        def obs_at(z):
            rows = []
            for k in (s, s + 1):
                ends = [cams[k][0].T @ (cams[s][0] @ (z * np.array(e)) + cams[s][1] - cams[k][1]) for e in _TL_ENDS[l]]
                rows.append([ends[0][0] / ends[0][2], ends[0][1] / ends[0][2], ends[1][0] / ends[1][2], ends[1][1] / ends[1][2]])
            return np.array(rows)
        cos_at = lambda z: triangulate_line(w.pose[s:s + 2], w.ex_pose, obs_at(z), np.float64)[1]["min_cos"]
        lo, hi = 0.3, 300.0
        assert cos_at(lo) < target < cos_at(hi)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if cos_at(mid) < target else (lo, mid)
        w.line_obs[off[l]:off[l] + 2, :4] = obs_at(lo)
    return w


@functools.lru_cache(maxsize=None)
def tl_cases():
    out = {}
    out["tl_generic"] = _untriangulated(cut(generate(7402, L=8, kf=TL_KF), line_nobs=[2, 3, 4, 5, 7, 9, 10, 11]))
    out["tl_threshold"] = _tl_crafted(_untriangulated(cut(generate(7410, L=4), line_nobs=[2, 2, 2, 2])))
    w1 = _untriangulated(cut(generate(7403, L=4, kf=TL_KF), line_nobs=[1, 4, 1, 6]))
    w1.line_plk[:] = np.arange(24).reshape(4, 6) + 0.5
    out["tl_one_obs"] = w1
    wk = cut(generate(7404, L=4, kf=TL_KF), line_nobs=[3, 4, 5, 6])
    wk.line_triangulated[:] = [0, 1, 0, 1]
    wk.line_plk[[0, 2]] = 0.0
    wk.line_plk[[1, 3]] *= 1.75
    out["tl_keep"] = wk
    out["tl_stride"] = _untriangulated(cut(generate(7405, L=129, kf=TL_KF), line_nobs=3 - np.arange(129) % 2))
    for i, (n, nobs) in enumerate(((5, [2, 11, 4, 6, 3]), (1, [7]), (9, [3, 3, 5, 11, 2, 8, 4, 6, 10]))):
        out["tl_batch%d" % i] = _untriangulated(cut(generate(7406 + i, L=n, kf=TL_KF), line_nobs=nobs))
    return out


@functools.lru_cache(maxsize=None)
def tl_reference(name):
    """per line of the case: (plk long double or None, unit, decisions)"""
    w = tl_cases()[name]
    out = []
    for l in range(len(w.line_start)):
        if w.line_triangulated[l] or w.line_nobs[l] < 2:
            out.append((None, None, None))
            continue
        pose, obs = line_track(w, l)
        plk, dec = triangulate_line(pose, w.ex_pose, obs)
        out.append((plk,) + ((line_units(w, l)[1],) if plk is not None else (None,)) + (dec,))
    return out


def tl_run64(name, seed):
    """the float64 run at inputs one ulp away -> per line plk or None"""
    w = perturbed_window(tl_cases()[name], np.random.default_rng(seed))
    out = []
    for l, (plk, unit, dec) in enumerate(tl_reference(name)):
        pose, obs = line_track(w, l)
        out.append(None if dec is None else triangulate_line(pose, w.ex_pose, obs, dt=np.float64)[0])
    return out


def tl_rho(name, got):
    """worst rho of per-line vectors `got` (None = untriangulated) against the reference; inf where the flags differ"""
    worst = 0.0
    for g, (plk, unit, dec) in zip(got, tl_reference(name)):
        if dec is None:
            continue
        if (g is None) != (plk is None):
            return np.inf
        if plk is not None:
            worst = max(worst, float((np.abs(np.asarray(g, LD) - plk) / unit).max()))
    return worst


def tl_measure(name):
    return dict(plk=max(tl_rho(name, tl_run64(name, s)) for s in SEEDS))


# points
TP_UNIT_SUBSET = 16


def _project(w, Pc0, start, no):
    """observations (x / z, y / z, 1) of the point Pc0 (start camera frame) in frames start .. start + no - 1"""
    cams = cameras(w.pose, w.ex_pose, np.float64)
    Pw = cams[start][0] @ Pc0 + cams[start][1]
    obs = []
    for k in range(start, start + no):
        pc = cams[k][0].T @ (Pw - cams[k][1])
        assert pc[2] > 0.02, "the crafted point is not in front of frame %d" % k
        obs.append([pc[0] / pc[2], pc[1] / pc[2], 1.0])
    return np.array(obs)


def _crafted(seed, pts, nobs):
    w = generate(seed, P=len(pts))
    w = cut(w, point_nobs=nobs)
    off = np.concatenate([[0], np.cumsum(nobs)]).astype(int)
    for p, Pc in enumerate(pts):
        w.point_obs[off[p]:off[p + 1]] = _project(w, np.asarray(Pc, float), int(w.point_start[p]), nobs[p])
    w.inv_depth[:] = -1.0
    return w


@functools.lru_cache(maxsize=None)
def tp_cases():
    out = {}
    wg = cut(generate(7501, P=4), point_nobs=[2, 3, 7, 11])
    wg.inv_depth[:] = -1.0
    out["tp_generic"] = wg
    out["tp_threshold"] = _crafted(7502, [[0.004, -0.003, 0.09], [-0.005, 0.002, 0.11], [0.002, 0.004, 0.09], [0.003, 0.001, 0.11]],
                                   [2, 2, 3, 3])
    wb = cut(generate(7503, P=4), point_nobs=[2, 4, 6, 11])
    wb.inv_depth[:] = -1.0
    wb.point_obs[:, :2] *= -1.0
    out["tp_behind"] = wb
    wk = cut(generate(7504, P=4), point_nobs=[3, 3, 3, 3])
    wk.inv_depth[:] = [0.37, -0.0, -1.0, 2.5]
    out["tp_keep"] = wk
    out["tp_short_baseline"] = _crafted(7505, [[30.0, -20.0, 400.0], [-50.0, 10.0, 800.0]], [2, 3])
    ws = cut(generate(7506, P=129), point_nobs=2 + np.arange(129) % 3)
    ws.inv_depth[:] = -1.0
    out["tp_stride"] = ws
    return out


@functools.lru_cache(maxsize=None)
def tp_reference(name):
    """per track (inverse depth long double or None = kept, unit or None = not computed, decisions)"""
    w = tp_cases()[name]
    out = []
    for p in range(len(w.point_start)):
        if not w.inv_depth[p] < 0:
            out.append((None, None, None))
            continue
        pose, obs = point_track(w, p)
        d, dec = triangulate_point(pose, w.ex_pose, obs, INIT_DEPTH)
        unit = point_units(w, p, INIT_DEPTH)[1] if (name != "tp_stride" or p < TP_UNIT_SUBSET) else None
        out.append((1 / d, unit, dec))
    return out


def tp_run64(name, seed):
    w = perturbed_window(tp_cases()[name], np.random.default_rng(seed))
    run = lambda p: triangulate_point(point_track(w, p)[0], w.ex_pose, point_track(w, p)[1], INIT_DEPTH, np.float64)[0]
    return [None if dec is None else 1.0 / float(run(p)) for p, (_, _, dec) in enumerate(tp_reference(name))]


def tp_rho(name, got):
    """(worst rho in units over the tracks that have one, worst |error| / (eps64 |value|) over the others); a track that takes
    init_depth must have the exact bits"""
    ru, rv = 0.0, 0.0
    for g, (inv, unit, dec) in zip(got, tp_reference(name)):
        if dec is None:
            continue
        if dec["used_init"]:
            if g != 1.0 / INIT_DEPTH:
                return np.inf, np.inf
        elif unit is not None:
            ru = max(ru, float(abs(LD(g) - inv) / unit))
        else:
            rv = max(rv, float(abs(LD(g) - inv) / (EPS64 * abs(inv))))
    return ru, rv


def tp_measure(name):
    r = [tp_rho(name, tp_run64(name, s)) for s in SEEDS]
    out = dict(invd=max(a for a, _ in r))
    if name == "tp_stride":
        out["rest"] = max(b for _, b in r)
    return out


# ---- what the oracle and the device are held to: the same checks for both ---------------------------------------------------------
def lo_check(name, k, rep, w_out):
    """a run of onlyLineOpt on the case's window under num_iterations = k (rep: its SolveReport, w_out: the window it left) against
    the reference: the report's integers, the erase flags and the untouched entries exactly; -> rho of cost0, cost, line"""
    w_in = lo_cases()[name][0]
    ref = lo_reference(name)
    rrep, _, rplk, outl = at(ref, k)
    got = (rep.iterations, rep.num_successful_steps, rep.termination)
    assert got == (rrep["iterations"], rrep["successful"], rrep["termination"]), (name, k, got, rrep)
    if not ref["ran"]:           # fewer than four lines: nothing is touched, the report is empty
        assert np.array_equal(w_out.line_plk, w_in.line_plk) and rep.n_lines_removed == 0 and not w_out.line_removed.any()
        assert rep.initial_cost == 0.0 and rep.final_cost == 0.0
        return dict(cost0=0.0, cost=0.0, line=0.0)
    lines = ref["problem"].lines
    erased = np.array([o[0] for o in outl], bool)
    flags = np.zeros(len(w_in.line_removed), np.int32)
    flags[lines[erased]] = 1
    assert np.array_equal(w_out.line_removed, flags), (name, k, w_out.line_removed, flags)
    assert rep.n_lines_removed == int(erased.sum())
    same = np.ones(len(w_in.line_plk), bool)
    same[lines[~erased]] = False                 # an erased or untriangulated line keeps the caller's bits
    assert np.array_equal(w_out.line_plk[same], w_in.line_plk[same])
    assert np.all(np.isfinite(w_out.line_plk)) and np.isfinite(rep.initial_cost) and np.isfinite(rep.final_cost)
    return dict(cost0=rho_cost(rep.initial_cost, rrep["initial_cost"]), cost=rho_cost(rep.final_cost, rrep["final_cost"]),
                line=rho_lines(w_out.line_plk[lines[~erased]], rplk[~erased]))


def tl_check(name, w_out):
    """a window triangulateLine left against the reference: flags exact, untouched entries bit-equal -> rho of the vectors"""
    w_in = tl_cases()[name]
    ref = tl_reference(name)
    n = len(ref)
    want = np.array([1 if (dec is None and w_in.line_triangulated[l]) or plk is not None else 0 for l, (plk, _, dec) in enumerate(ref)])
    assert np.array_equal(w_out.line_triangulated[:n], want), (name, w_out.line_triangulated[:n], want)
    new = np.array([plk is not None for plk, _, _ in ref])
    assert np.array_equal(w_out.line_plk[~new], w_in.line_plk[~new]), "%s: a line that is not triangulated here lost its bits" % name
    assert np.all(np.isfinite(w_out.line_plk))
    return dict(plk=tl_rho(name, [w_out.line_plk[l] if new[l] else None for l in range(n)]))


def tp_check(name, w_out):
    w_in = tp_cases()[name]
    ref = tp_reference(name)
    kept = np.array([dec is None for _, _, dec in ref])
    same = np.array_equal(w_out.inv_depth[kept].view(np.int64), w_in.inv_depth[kept].view(np.int64))
    assert same, "%s: a track with a depth lost its bits" % name
    assert np.all(np.isfinite(w_out.inv_depth))
    ru, rv = tp_rho(name, [None if kept[p] else float(w_out.inv_depth[p]) for p in range(len(ref))])
    return dict(invd=ru, rest=rv) if name == "tp_stride" else dict(invd=ru)


def bar(name, what):
    return MARGIN * max(YARDSTICK[name][what], 1.0)


# Yardsticks: this module in float64, factors in a shuffled order, states, lines and observations one ulp away, against its
# long-double run; worst over SEEDS (`python tests/linemap_ref.py` prints them).  onlyLineOpt: cost0 the initial cost, cost and
# line per iteration cap k = 1, 2, ... of the sweep.
YARDSTICK = {
    "lo_generic": dict(cost0=170, cost=[4.68e+03, 1.46e+03, 858, 922, 922], line=[472, 342, 66, 41, 41]),
    "lo_reject": dict(cost0=78.1, cost=[5.27e+03, 5.27e+03, 5.27e+03, 1.48e+04, 6.58e+03, 8.67e+04, 5.18e+04, 8.43e+03],
        line=[1.23e+03, 1.23e+03, 1.23e+03, 847, 1.45e+03, 2.15e+03, 1.13e+03, 453]),
    "lo_reject2": dict(cost0=49.5, cost=[7.96e+04, 7.96e+04, 1.14e+06, 4.53e+04, 4.53e+04, 4.53e+04, 4.53e+04, 4.53e+04],
        line=[2.98e+04, 2.98e+04, 1.72e+06, 2.03e+06, 2.03e+06, 2.03e+06, 2.03e+06, 2.03e+06]),
    "lo_four": dict(cost0=327, cost=[1.82e+03, 2.32e+03, 1.55e+03, 1.83e+03, 1.83e+03], line=[164, 177, 79.3, 71.1, 71.1]),
    "lo_three": dict(cost0=0, cost=[0], line=[0]),
    "lo_full_4": dict(cost0=58.9, cost=[379, 2.4e+03], line=[314, 1.65e+03]),
    "lo_full_2": dict(cost0=22.3, cost=[539, 1.56e+03], line=[358, 1.67e+03]),
    "lo_full_1": dict(cost0=14.6, cost=[238, 877], line=[886, 2.17e+03]),
    "lo_full_65": dict(cost0=8.17, cost=[822, 7e+03], line=[803, 1.18e+03]),
    "out_behind": dict(cost0=91, cost=[6.16e+03, 6.16e+03, 6.16e+03, 7.3e+03, 7.3e+03, 7.3e+03, 1.08e+05, 5.06e+05], line=[646, 646,
        646, 5.91e+03, 5.91e+03, 5.91e+03, 9.93e+03, 1.97e+04]),
    "out_far": dict(cost0=153, cost=[1.01e+04, 1.17e+04, 1.05e+04, 1.05e+04, 1.06e+04, 7.99e+03, 1.42e+04, 1.29e+04], line=[87.6,
        140, 309, 643, 4.15e+03, 3.21e+04, 5.97e+04, 6.12e+04]),
    "out_err": dict(cost0=147, cost=[442, 427, 410, 403, 366, 438, 377, 272], line=[87.6, 140, 309, 643, 4.15e+03, 1.85e+04,
        4.19e+04, 1.51e+04]),
    "out_kept": dict(cost0=161, cost=[1.2e+04, 1.17e+04, 1.07e+04, 1.05e+04, 1.05e+04, 8.92e+03, 1.4e+04, 1.26e+04], line=[87.6,
        140, 309, 643, 4.15e+03, 3.1e+04, 6.73e+04, 4.5e+04]),
    "tl_generic": dict(plk=2.3),
    "tl_threshold": dict(plk=1.36),
    "tl_one_obs": dict(plk=0.951),
    "tl_keep": dict(plk=1.04),
    "tl_stride": dict(plk=1.88),
    "tl_batch0": dict(plk=1.64),
    "tl_batch1": dict(plk=0.834),
    "tl_batch2": dict(plk=1.93),
    "tp_generic": dict(invd=1.22),
    "tp_threshold": dict(invd=1.26),
    "tp_behind": dict(invd=0),
    "tp_keep": dict(invd=0.848),
    "tp_short_baseline": dict(invd=1.39),
    "tp_stride": dict(invd=1.19, rest=515),
}


def measure():
    out = {}
    for name in lo_cases():
        out[name] = lo_measure(name)[0]
    for name in tl_cases():
        out[name] = tl_measure(name)
    for name in tp_cases():
        out[name] = tp_measure(name)
    return out


def _fmt(d):
    f = lambda a: "[%s]" % ", ".join("%.3g" % x for x in a) if isinstance(a, list) else "%.3g" % a
    return "dict(%s)" % ", ".join("%s=%s" % (k, f(a)) for k, a in d.items())


if __name__ == "__main__":
    import textwrap
    for name, y in measure().items():
        print(textwrap.fill('    "%s": %s,' % (name, _fmt(y)), 132, subsequent_indent=" " * 8, break_long_words=False))
