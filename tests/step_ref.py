"""One trust-region iteration of the window problem, restated densely in np.longdouble -- the reference the step kernels
(k_lin / k_lin2, k_step = k_schur + k_chol + k_back, k_solve) are judged against in test_gpu_step_kernels.py, and which
test_step_reference.py checks against the oracle on the CPU first.

What is restated: ceres' TrustRegionMinimizer with jacobi scaling and the TRADITIONAL_DOGLEG strategy as oracle/problem.cpp
(Dogleg, SolveWith) does it, over the residual blocks Estimator::optimizationwithLine adds (oracle/window.cpp solve_window):
the prior, the IMU factors 1..10, every point track's observation 0 against k >= 1, every triangulated line's observations
(line factor, VP factor when its flag is set).  Residuals and Jacobians come from the oracle's factor evaluators in double
and are promoted; everything after that (Huber scaling, J^T J, the scaling, the Cholesky solve, the dogleg step, the model
cost change) is long double.  Columns are local coordinates: the evaluators' zero seventh pose column is dropped.
Problem(w, opt, evaluators=vis_ref.Evaluators) takes the point, line and VP rows from vis_ref.py instead, in true long double
(test_gpu_vis_factors.py); the IMU rows have their long-double form in imu_ref.py; Problem(w, opt, prior_rows=prior_ref.prior_rows)
takes the prior's row from prior_ref.py, in long double from dx on (test_gpu_prior_factor.py) -- the cases below keep the oracle's.

Index of a window with nP points and nL triangulated lines (n = 171 + nP + 4 nL): frame f pose 15 f + 0..5, speed/bias
15 f + 6..14, extrinsic 165..170, inverse depth of point p 171 + p, line l 171 + nP + 4 l + 0..3.

`python tests/step_ref.py` prints the table YARDSTICK below was copied from."""
import functools

import numpy as np

import oracle_api as o
import vplines_slam_amd as v

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "np.longdouble is not an extended type here: restate the linear algebra below with mpmath"
EPS64 = float(np.finfo(np.float64).eps)
NF, NC = 11, 171
MU0, RADIUS0 = 1e-8, 1e4            # DoglegStrategy::mu_, Solver::Options::initial_trust_region_radius
MIN_DIAG, MAX_DIAG = 1e-6, 1e32     # min_lm_diagonal, max_lm_diagonal


# ---- small geometry (double), as oracle/geometry.h and smallmat.h spell it -----------------------------------------------
def quat_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def R_quat(m):
    """Eigen's Quaternion(Matrix3) (x, y, z, w)"""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def yaw_deg(R):
    return np.arctan2(R[1, 0], R[0, 0]) / np.pi * 180.0


def yaw_R(deg):
    y = deg / 180.0 * np.pi
    return np.array([[np.cos(y), -np.sin(y), 0.0], [np.sin(y), np.cos(y), 0.0], [0.0, 0.0, 1.0]])


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def plk_to_pose(plk, Rcw, tcw):
    n, d = plk[:3], plk[3:]
    return np.concatenate([Rcw @ n + skew(tcw) @ (Rcw @ d), Rcw @ d])


def plk_from_pose(plk, Rcw, tcw):
    return plk_to_pose(plk, Rcw.T, -(Rcw.T @ tcw))


# ---- the problem of one window -----------------------------------------------------------------------------------------
class Problem:
    def __init__(self, w, opt, evaluators=o, prior_rows=None):
        """evaluators: what has projection_factor, line_factor and vp_factor(params, observations, sqrt_info) -> r, jac for the
        point, line and VP rows: the oracle's (float64) by default; vis_ref.Evaluators gives long-double rows.
        prior_rows: (problem, x) -> the prior's entry of rows(); None: the oracle's prior_factor (float64)"""
        self.w, self.opt, self.ev, self.prior_rows = w, opt, evaluators, prior_rows
        self.nP = len(w.point_start)
        nl_all = len(w.line_start)
        self.lines = np.nonzero(np.asarray(w.line_triangulated[:nl_all]) != 0)[0]     # solved line -> the window's line
        self.nL = len(self.lines)
        self.n = NC + self.nP + 4 * self.nL
        self.poff = np.concatenate([[0], np.cumsum(w.point_nobs)]).astype(int)
        self.loff = np.concatenate([[0], np.cumsum(w.line_nobs)]).astype(int)
        self.ex_free = bool(opt.estimate_extrinsic)
        assert w.failure is None

    def classes(self):
        """name -> columns of the full index"""
        f = np.arange(NF)
        pos = (15 * f[:, None] + np.arange(3)).ravel()
        rot = (15 * f[:, None] + 3 + np.arange(3)).ravel()
        sb = (15 * f[:, None] + 6 + np.arange(9)).ravel()
        return dict(pos=pos, rot=rot, sb=sb, ex_pos=np.arange(165, 168), ex_rot=np.arange(168, 171),
                    invd=NC + np.arange(self.nP), line=NC + self.nP + np.arange(4 * self.nL))

    def initial_state(self):
        """the window's states as parameter blocks (vector2double, oracle/window.cpp:68-93): world orth of every solved line
        from its Pluecker vector in the start camera frame"""
        w = self.w
        ric, tic = quat_R(w.ex_pose[3:] / np.linalg.norm(w.ex_pose[3:])), w.ex_pose[:3]
        orth = np.zeros((self.nL, 4))
        for dl, l in enumerate(self.lines):
            s = int(w.line_start[l])
            Rs = quat_R(w.pose[s, 3:] / np.linalg.norm(w.pose[s, 3:]))
            orth[dl] = o.plk_to_orth(plk_to_pose(w.line_plk[l], Rs @ ric, w.pose[s, :3] + Rs @ tic))
        # load_window and vector2double: Rs = Quat(...).normalized().toRotationMatrix(), para_Pose = Quaternion(Rs), the
        # inverse depth through the depth -- the oracle and the device (k_prep) linearise at these states, not at the raw ones
        pose, ex = w.pose.copy(), w.ex_pose.copy()
        for q in list(pose[:, 3:]) + [ex[3:]]:
            q[:] = R_quat(quat_R(q / np.linalg.norm(q)))
        return dict(pose=pose, sb=w.speed_bias.copy(), ex=ex, invd=1.0 / (1.0 / w.inv_depth[:self.nP]), orth=orth)

    def rows(self, x):
        """the residual blocks at x, in the oracle's order: (kind, weight of the unit, huber, r [m], [(first column, J [m, k])])"""
        w, opt = self.w, self.opt
        pose, sb, ex, invd, orth = x["pose"], x["sb"], x["ex"], x["invd"], x["orth"]
        out = []
        pr = w.prior
        if pr is not None and pr.n > 0 and self.prior_rows is not None:
            out.append(self.prior_rows(self, x))
        elif pr is not None and pr.n > 0:
            params, meta = [], []
            for b in range(pr.n_blocks):
                kind, fr = pr.block_kind[b], pr.block_frame[b]
                params.append(pose[fr] if kind == 0 else sb[fr] if kind == 1 else ex)
                meta.append((15 * fr if kind == 0 else 15 * fr + 6 if kind == 1 else 165, 9 if kind == 1 else 7, 9 if kind == 1 else 6))
            r, jac = o.prior_factor(pr, np.concatenate(params))
            blocks, off = [], 0
            for col0, size, k in meta:
                blocks.append((col0, jac[off:off + pr.n * size].reshape(pr.n, size)[:, :k]))
                off += pr.n * size
            out.append(("prior", 1.0, False, r, blocks))
        for j in range(1, NF):
            if w.preint[j].sum_dt > 10.0:
                continue
            params = np.concatenate([pose[j - 1], sb[j - 1], pose[j], sb[j]])[None]
            r, jac = o.imu_factor(params, [w.preint[j]], opt.g_norm)
            jac = jac[0]
            cov = np.array(w.preint[j].covariance).reshape(15, 15)
            out.append(("imu", float(np.linalg.cond(cov)), False, r[0],
                        [(15 * (j - 1), jac[0:105].reshape(15, 7)[:, :6]), (15 * (j - 1) + 6, jac[105:240].reshape(15, 9)),
                         (15 * j, jac[240:345].reshape(15, 7)[:, :6]), (15 * j + 6, jac[345:480].reshape(15, 9))]))
        P, pts, where = [], [], []
        for p in range(self.nP):
            s = int(w.point_start[p])
            ob = w.point_obs[self.poff[p]:self.poff[p + 1]]
            for k in range(1, len(ob)):
                P.append(np.concatenate([pose[s], pose[s + k], ex, [invd[p]]]))
                pts.append(np.concatenate([ob[0], ob[k]]))
                where.append((s, s + k, p))
        if P:
            r, jac = self.ev.projection_factor(np.array(P), np.array(pts), opt.focal_length / 1.5)
            for i, (fi, fj, p) in enumerate(where):
                out.append(("proj", 1.0, True, r[i],
                            [(15 * fi, jac[i, 0:14].reshape(2, 7)[:, :6]), (15 * fj, jac[i, 14:28].reshape(2, 7)[:, :6]),
                             (165, jac[i, 28:42].reshape(2, 7)[:, :6]), (NC + p, jac[i, 42:44].reshape(2, 1))]))
        for dl, l in enumerate(self.lines):
            s = int(w.line_start[l])
            ob = w.line_obs[self.loff[l]:self.loff[l + 1]]
            params = np.array([np.concatenate([pose[s + k], ex, orth[dl]]) for k in range(len(ob))])
            rl, jl = self.ev.line_factor(params, ob[:, 0:4], opt.line_factor)
            rv, jv = self.ev.vp_factor(params, ob[:, 4:7], opt.vp_factor)
            col = NC + self.nP + 4 * dl
            for k in range(len(ob)):
                for kind, r, jac in (("line", rl, jl), ("vp", rv, jv)):
                    if kind == "vp" and ob[k, 7] != 1.0:
                        continue
                    out.append((kind, 1.0, True, r[k],
                                [(15 * (s + k), jac[k, 0:14].reshape(2, 7)[:, :6]), (165, jac[k, 14:28].reshape(2, 7)[:, :6]),
                                 (col, jac[k, 28:36].reshape(2, 4))]))
        return out

    def linearize(self, x):
        """-> Lin at x (long double)"""
        rows = self.rows(x)
        M = sum(len(r[3]) for r in rows)
        J, r, wrow = np.zeros((M, self.n), LD), np.zeros(M, LD), np.ones(M)
        delta = LD(self.opt.huber_delta)
        cost, m0, sq, kinds = LD(0), 0, [], []
        for kind, wt, huber, rf, blocks in rows:
            m = len(rf)
            rf = np.asarray(rf, LD)
            s = rf @ rf
            sc, rho = LD(1), s
            if huber:
                sq.append(float(s))
                if s > delta * delta:      # rho' = delta / sqrt(s), rho'' < 0: the corrector scales by sqrt(rho') alone
                    sc = np.sqrt(delta / np.sqrt(s))
                    rho = 2 * delta * np.sqrt(s) - delta * delta
            cost += rho / 2
            r[m0:m0 + m] = sc * rf
            for col0, Jb in blocks:
                J[m0:m0 + m, col0:col0 + Jb.shape[1]] = sc * np.asarray(Jb, LD)
            wrow[m0:m0 + m] = wt
            kinds.append((kind, m0, m))
            m0 += m
        if not self.ex_free:
            J[:, 165:171] = 0
        return Lin(J, r, wrow, cost, np.array(sq), kinds)

    def assemble64(self, x, order=None):
        """H, g, cost of the same problem in float64, one residual block after the other in `order` (a permutation)"""
        rows = self.rows(x)
        H, g, cost = np.zeros((self.n, self.n)), np.zeros(self.n), 0.0
        delta = float(self.opt.huber_delta)
        for i in (range(len(rows)) if order is None else order(len(rows))):
            kind, wt, huber, rf, blocks = rows[i]
            s = float(rf @ rf)
            sc, rho = 1.0, s
            if huber and s > delta * delta:
                sc = np.sqrt(delta / np.sqrt(s))
                rho = 2 * delta * np.sqrt(s) - delta * delta
            cost += 0.5 * rho
            idx = np.concatenate([col0 + np.arange(Jb.shape[1]) for col0, Jb in blocks])
            Jf = sc * np.concatenate([Jb for _, Jb in blocks], axis=1)
            if not self.ex_free:
                Jf[:, (idx >= 165) & (idx < 171)] = 0.0
            H[np.ix_(idx, idx)] += Jf.T @ Jf
            g[idx] += Jf.T @ (sc * rf)
        return H, g, cost

    def plus(self, x, delta):
        """x [+] delta: pose_plus, line_orth_plus and plain addition"""
        d = np.asarray(delta, np.float64)
        dp = np.stack([d[15 * f:15 * f + 6] for f in range(NF)])
        out = dict(pose=o.pose_plus(x["pose"], dp), sb=x["sb"] + np.stack([d[15 * f + 6:15 * f + 15] for f in range(NF)]),
                   ex=o.pose_plus(x["ex"][None], d[None, 165:171])[0] if self.ex_free else x["ex"].copy(),
                   invd=x["invd"] + d[NC:NC + self.nP], orth=x["orth"].copy())
        if self.nL:
            out["orth"] = o.line_orth_plus(x["orth"], d[NC + self.nP:].reshape(self.nL, 4))
        return out

    def hand_back(self, x):
        """double2vector2 (oracle/window.cpp:97-140) and the write-back of solve_window on the parameter blocks x: the yaw of R0
        and P0 of the window as it came restored, the lines carried through that transform and into their start camera frame.
        -> dict(pose, sb, ex, invd, plk [nL, 6])"""
        w = self.w
        P0 = w.pose[0, :3]
        y0 = yaw_deg(quat_R(w.pose[0, 3:] / np.linalg.norm(w.pose[0, 3:])))
        rot = yaw_R(y0 - yaw_deg(quat_R(x["pose"][0, 3:])))
        p0c = x["pose"][0, :3]
        Rs = [rot @ quat_R(x["pose"][i, 3:] / np.linalg.norm(x["pose"][i, 3:])) for i in range(NF)]
        Ps = [rot @ (x["pose"][i, :3] - p0c) + P0 for i in range(NF)]
        pose = np.array([np.concatenate([Ps[i], R_quat(Rs[i])]) for i in range(NF)])
        sb = x["sb"].copy()
        for i in range(NF):
            sb[i, :3] = rot @ x["sb"][i, :3]
        tic, ric = x["ex"][:3], quat_R(x["ex"][3:])
        ex = np.concatenate([tic, R_quat(ric)])
        two = -(rot @ p0c) + P0
        plk = np.zeros((self.nL, 6))
        for dl, l in enumerate(self.lines):
            orth = o.plk_to_orth(plk_to_pose(o.orth_to_plk(x["orth"][dl]), rot, two))
            s = int(w.line_start[l])
            plk[dl] = plk_from_pose(o.orth_to_plk(orth), Rs[s] @ ric, Ps[s] + Rs[s] @ tic)
        return dict(pose=pose, sb=sb, ex=ex, invd=1.0 / (1.0 / x["invd"]), plk=plk)


class Lin:
    """J, r (Huber-scaled, long double), H = J^T J, g = J^T r, cost, and the rounding units of H and g"""

    def __init__(self, J, r, wrow, cost, sq, kinds):
        self.J, self.r, self.cost, self.sq, self.kinds = J, r, cost, sq, kinds
        self.H, self.g = J.T @ J, J.T @ r
        aJ, ar = np.abs(J).astype(np.float64), np.abs(r).astype(np.float64)
        # first-order rounding units: eps64 * sum_f w_f |J_f|^T |J_f| and eps64 * sum_f w_f |J_f|^T |r_f|.  w_f = cond2 of the
        # covariance for an IMU factor: its whitening matrix is a double-precision factor of cov^-1 and no better than that
        self.unit_H = EPS64 * (aJ.T @ (wrow[:, None] * aJ))
        self.unit_g = EPS64 * (aJ.T @ (wrow * ar))
        self.unit_cost = EPS64 * float(cost)       # eps64 * sum |terms|: every term rho / 2 of the cost is positive


# ---- long-double linear algebra ------------------------------------------------------------------------------------------
def cholesky_ld(A):
    A = np.array(A, LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = A[j, j]
        assert d > 0, "matrix is not positive definite at column %d" % j
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = A[j + 1:, j] / L[j, j]
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return L


def solve_lower(L, b, dtype):
    y = np.zeros(len(b), dtype)
    for i in range(len(b)):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    return y


def solve_upper(U, b, dtype):
    n = len(b)
    y = np.zeros(n, dtype)
    for i in range(n - 1, -1, -1):
        y[i] = (b[i] - U[i, i + 1:] @ y[i + 1:]) / U[i, i]
    return y


def solve_ld(A, b):
    L = cholesky_ld(A)
    return solve_upper(L.T, solve_lower(L, np.asarray(b, LD), LD), LD)


def solve64(A, b):
    """the float64 yardstick: np.linalg.cholesky and two triangular solves"""
    L = np.linalg.cholesky(np.asarray(A, np.float64))
    return solve_upper(L.T, solve_lower(L, np.asarray(b, np.float64), np.float64), np.float64)


def omega(A, y, b):
    """row-wise backward error max_i |A y - b|_i / (|A_i|_2 |y|_2 + |b_i|) over all rows, in units of eps64"""
    A, y, b = np.asarray(A, LD), np.asarray(y, LD), np.asarray(b, LD)
    res = np.abs(A @ y - b)
    den = np.sqrt((A * A).sum(axis=1)) * np.sqrt(y @ y) + np.abs(b)
    return float((res / den).max() / EPS64)


def live(H):
    """columns some residual block depends on (ceres drops the others from the program; here they are zero columns)"""
    return np.nonzero(np.asarray(np.diag(H), np.float64) > 0)[0]


def cond2(A):
    a = np.asarray(A, np.float64)
    return float(np.linalg.cond(a))


# ---- the step -------------------------------------------------------------------------------------------------------------
def scaling(H, g):
    """jacobi scale, DoglegStrategy::diagonal_ and gradient_ of (H, g)"""
    H, g = np.asarray(H, LD), np.asarray(g, LD)
    dH = np.diag(H)
    scale = 1 / (1 + np.sqrt(dH))
    D = np.sqrt(np.clip(scale * scale * dH, LD(MIN_DIAG), LD(MAX_DIAG)))
    return scale, D, scale * g / D


def step(H, g, J=None, mu=MU0, radius=RADIUS0):
    """Dogleg::ComputeStep and the model cost change of SolveWith (oracle/problem.cpp:401-493, 601-616) on H = J^T J, g = J^T r"""
    H, g = np.asarray(H, LD), np.asarray(g, LD)
    scale, D, grad = scaling(H, g)
    u = scale * grad / D
    a1 = grad @ grad
    if J is not None:
        Ju = np.asarray(J, LD) @ u
        q = Ju @ Ju
    else:
        q = u @ (H @ u)
    alpha = a1 / q
    A = scale[:, None] * H * scale[None, :] + np.diag(LD(mu) * D * D)
    b = scale * g
    y = solve_ld(A, b)
    gn = -D * y
    s = finish(H, g, scale, D, grad, gn, alpha, radius)
    s.update(A=A, b=b, y=y, q=q, u=u)
    return s


def finish(H, g, scale, D, grad, gn, alpha, radius=RADIUS0):
    """ComputeTraditionalDoglegStep and what follows it, from the vectors of a step (the reference's or the device's)"""
    H, g, scale, D, grad, gn = (np.asarray(a, LD) for a in (H, g, scale, D, grad, gn))
    alpha, radius = LD(alpha), LD(radius)
    a1, a2, a3 = grad @ grad, gn @ gn, grad @ gn
    gnorm, gnn = np.sqrt(a1), np.sqrt(a2)
    if gnn <= radius:
        branch, t, dnorm = "gauss-newton", gn.copy(), gnn
    elif gnorm * alpha >= radius:
        branch, t, dnorm = "cauchy", -(radius / gnorm) * grad, radius
    else:
        b_dot_a = -alpha * a3
        a_sq = (alpha * gnorm) ** 2
        bma = a_sq - 2 * b_dot_a + a2
        c = b_dot_a - a_sq
        d = np.sqrt(c * c + bma * (radius * radius - a_sq))
        beta = (d - c) / bma if c <= 0 else (radius * radius - a_sq) / (d + c)
        branch, t = "dogleg", (-alpha * (1 - beta)) * grad + beta * gn
        dnorm = np.sqrt(t @ t)
    delta = scale * t / D
    Hd = H @ delta
    mcc = -(delta @ g + (delta @ Hd) / 2)
    mcc_terms = np.abs(delta * g).sum() + (np.abs(delta)[:, None] * np.abs(H) * np.abs(delta)[None, :]).sum() / 2
    return dict(scale=scale, diag=D, grad=grad, gn=gn, alpha=alpha, a1=a1, a2=a2, a3=a3, branch=branch, step=t, delta=delta,
                dogleg_step_norm=dnorm, model_cost_change=mcc, mcc_terms=mcc_terms)


# ---- yardsticks: what float64 on the CPU does to the same operations --------------------------------------------------
def perturbed(x, rng):
    """every state entry moved by one relative ulp, random signs"""
    return {k: a * (1.0 + EPS64 * rng.choice([-1.0, 1.0], size=a.shape)) for k, a in x.items()}


def rho(dev, ref, unit):
    """max |dev - ref| / unit over the entries with a unit (the others are structural zeros)"""
    dev, ref, unit = np.asarray(dev, LD), np.asarray(ref, LD), np.asarray(unit, LD)
    m = unit > 0
    return float((np.abs(dev - ref)[m] / unit[m]).max()) if m.any() else 0.0


def yardstick(prob, x, lin, st, seed):
    """rho_ref(H), rho_ref(g): H, g in float64 in a shuffled order of the residual blocks at states one ulp away, against the
    long-double ones; omega_ref, rho_ref(gn): a float64 dense Cholesky solve of the reference's A y = b"""
    rng = np.random.default_rng(seed)
    H64, g64, c64 = prob.assemble64(perturbed(x, rng), order=lambda m: rng.permutation(m))
    y64 = solve64(st["A"], st["b"])
    gn64 = -np.asarray(st["diag"], np.float64) * y64
    lv = live(lin.H)
    cond = cond2(st["A"][np.ix_(lv, lv)])
    gn_ref = np.asarray(st["gn"], np.float64)
    return dict(H=rho(H64, lin.H, lin.unit_H), g=rho(g64, lin.g, lin.unit_g),
                cost=float(abs(LD(c64) - lin.cost)) / lin.unit_cost,
                omega=omega(st["A"], y64, st["b"]),
                gn=float(np.linalg.norm(gn64 - gn_ref) / (EPS64 * cond * np.linalg.norm(gn_ref))), cond=cond)


# ---- the cases of test_step_reference.py and test_gpu_step_kernels.py -----------------------------------------------------
CAP_POINTS, CAP_LINES = 40, 12          # capacity of the contexts the cases are solved in: above most windows' counts


def _options(**kw):
    opt = v.default_options()
    opt.num_iterations = 1
    opt.marginalization_flag = v.capi.MARGIN_NONE
    for k, a in kw.items():
        setattr(opt, k, a)
    return opt


def _generate(P, L, vp, index, track_len=6, t=None):
    cfg = v.workload.config(P, L, vp)
    cfg.track_len = track_len
    w = v.workload.generate(v.workload.seed_for(3, 9000 + index), cfg, 0.29 * index if t is None else t)
    o.preintegrate_windows([w], v.default_options())
    return w, cfg


def _later_speed_bias_prior(w, rng):
    """a prior over pose 2, speed/bias 3 and the extrinsic (the construction of
    test_prior_with_speed_bias_of_a_later_frame_takes_the_general_path): outside k_chol's elimination order"""
    p = v.Prior()
    kinds, frames = [0, 1, 2], [2, 3, 0]
    n = 6 + 9 + 6
    p.n, p.n_blocks = n, 3
    idx = 0
    for b, (k, f) in enumerate(zip(kinds, frames)):
        p.block_kind[b], p.block_frame[b], p.block_idx[b] = k, f, idx
        x0 = (w.pose[f] if k == 0 else w.speed_bias[f] if k == 1 else w.ex_pose)
        for j in range(len(x0)):
            p.x0[b][j] = float(x0[j])
        idx += 9 if k == 1 else 6
    J = np.triu(rng.normal(size=(n, n))) * 3.0 + 5.0 * np.eye(n)
    r = rng.normal(size=n) * 0.1
    for j in range(n * n):
        p.J0[j] = float(J.reshape(-1)[j])
    for j in range(n):
        p.r0[j] = float(r[j])
    return p


# setting -> (environment when the context is made, cases of ONE batch in upload order, longest track of the batch).  The
# longest track sets the width WS = 6 * longest + 6 of the compact W rows and with it the kernel: 6 -> k_step<3, false>,
# 11 -> WS = 72 and the mixed / all-tiles / narrow landmark elimination that VPL_BA_SCHUR_WIDE picks
SETTINGS = {
    "default": ({}, ["a", "b", "c", "d", "f", "g", "i_tri"], 6),
    "ex_fixed": ({}, ["i_ex"], 6),
    "general": ({"VPL_BA_GENERAL": "1"}, ["a", "d"], 6),
    "unfused": ({"VPL_BA_STEP_FUSED": "0"}, ["a", "d"], 6),
    "wide_unset": ({}, ["c", "e"], 11),
    "wide_1": ({"VPL_BA_SCHUR_WIDE": "1"}, ["c", "e"], 11),
    "wide_-1": ({"VPL_BA_SCHUR_WIDE": "-1"}, ["c", "e"], 11),
}


@functools.lru_cache(maxsize=None)
def cases():
    """id -> (Window, options).  One window per shape; the ids are those of the table in DESIGN.md 2."""
    from test_gpu_solve import _ragged, _relayout_points
    out = {}
    out["a"] = (_generate(0, 0, False, 0)[0], _options())
    w11, _ = _generate(1, 0, False, 1, track_len=11)
    out["b"] = (_relayout_points(w11, [0], [2]), _options())
    out["c"] = (_generate(5, 1, True, 2)[0], _options())
    d = _ragged(_generate(37, 11, True, 3)[0], np.random.default_rng(31))
    out["d"] = (d, _options())
    # e: tracks of up to 11 observations, full and cut short, start frames 0..7
    we, _ = _generate(12, 6, True, 4, track_len=11)
    rng = np.random.default_rng(41)
    start = np.arange(12) % 8
    nobs = np.array([11 - s if p % 2 == 0 else rng.integers(2, 11 - s + 1) for p, s in enumerate(start)])
    e = _relayout_points(we, start, nobs)
    ln = np.array([n if l % 2 == 0 else rng.integers(5, n + 1) for l, n in enumerate(e.line_nobs)], np.int32)
    loff = np.concatenate([[0], np.cumsum(e.line_nobs)])
    lobs = np.concatenate([e.line_obs[loff[l]:loff[l] + ln[l]] for l in range(len(ln))])
    e = v.capi.Window(e.pose, e.speed_bias, e.ex_pose, e.point_start, e.point_nobs, e.point_obs, e.inv_depth, e.line_start, ln, lobs,
                      e.line_plk, e.preint, None)
    out["e"] = (e, _options())
    # f: d's shape one keyframe behind a window whose marginalisation (the oracle's) left the prior
    wa, cfg = _generate(37, 11, True, 5, t=1.7)
    prior, _ = o.solve_window(wa.copy(), v.default_options())
    wb = _ragged(_generate(37, 11, True, 6, t=1.7 + cfg.kf_dt)[0], np.random.default_rng(61))
    wb.prior = prior
    out["f"] = (wb, _options())
    wg = _ragged(_generate(37, 11, True, 7)[0], np.random.default_rng(71))
    wg.prior = _later_speed_bias_prior(wg, np.random.default_rng(72))
    out["g"] = (wg, _options())
    out["i_ex"] = (d, _options(estimate_extrinsic=0))
    it = d.copy()
    it.line_triangulated[[1, 4, 10]] = 0
    out["i_tri"] = (it, _options())
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """(Problem, x0, Lin, step) of a case at the window's own initial state"""
    w, opt = cases()[case]
    prob = Problem(w, opt)
    x0 = prob.initial_state()
    lin = prob.linearize(x0)
    return prob, x0, lin, step(lin.H, lin.g, lin.J)


# Yardsticks of the float64 restatement on the CPU (`python tests/step_ref.py` prints this table): rho_ref(H), rho_ref(g),
# rho_ref(cost) in eps64 * cost, omega_ref, rho_ref(gn) per case, seeds 1000 + position of the case.
YARDSTICK = {
    "a": dict(H=3.65e-06, g=1.49e-05, cost=74.4, omega=0.218, gn=0.0735),   # n = 171, cond2(A) = 2.69e+08
    "b": dict(H=1.6e+03, g=504, cost=158, omega=0.257, gn=0.00406),   # n = 172, cond2(A) = 7.22e+09
    "c": dict(H=662, g=495, cost=15.6, omega=0.196, gn=0.0368),   # n = 180, cond2(A) = 6.93e+08
    "d": dict(H=1.86e+03, g=3.14e+03, cost=26.1, omega=0.338, gn=0.0115),   # n = 252, cond2(A) = 5.97e+08
    "e": dict(H=1.09e+04, g=420, cost=81.8, omega=0.393, gn=0.0353),   # n = 207, cond2(A) = 5.95e+08
    "f": dict(H=1.73e+03, g=1.04e+04, cost=35.5, omega=0.463, gn=0.0211),   # n = 252, cond2(A) = 5.74e+08
    "g": dict(H=2.47e+03, g=1.42e+03, cost=183, omega=0.609, gn=0.0173),   # n = 252, cond2(A) = 6.02e+08
    "i_ex": dict(H=1.19e+03, g=3.13e+03, cost=13, omega=0.229, gn=0.0316),   # n = 252, cond2(A) = 3.98e+08
    "i_tri": dict(H=1.65e+03, g=4e+03, cost=5.72, omega=0.315, gn=0.0538),   # n = 240, cond2(A) = 6.25e+08
}
MARGIN = 8.0      # the device evaluates the factors in its own arrangement, contracts to FMA and sums in ticket order: the same
                  # order of rounding as the yardstick, not the same bits; a dropped or misplaced term is >= 1e6 units


def bar(what, case=None):
    """what a device ratio may reach: MARGIN * max(yardstick, 1) -- the worst case's yardstick for H and g (case = None), the
    case's own for the cost (in eps64 * cost: what one ulp of the states does to it) and for the solve (omega, gn)"""
    y = max(c[what] for c in YARDSTICK.values()) if case is None else YARDSTICK[case][what]
    return MARGIN * max(y, 1.0)


def measure():
    out = {}
    for k, case in enumerate(cases()):
        prob, x0, lin, st = reference(case)
        out[case] = yardstick(prob, x0, lin, st, 1000 + k)
    return out


if __name__ == "__main__":
    for case, y in measure().items():
        print('    "%s": dict(H=%.3g, g=%.3g, cost=%.3g, omega=%.3g, gn=%.3g),   # n = %d, cond2(A) = %.3g'
              % (case, y["H"], y["g"], y["cost"], y["omega"], y["gn"], reference(case)[0].n, y["cond"]))
