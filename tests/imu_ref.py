"""The IMU factor and a window's IMU share of H, g and the cost in np.longdouble -- the reference test_imu_reference.py checks
against the oracle and the device math on the CPU, and test_gpu_imu_linearisation.py / test_gpu_factors.py hold the kernels to.

Written from the formulas of IMUFactor::Evaluate (imu_factor.h:64-178) and IntegrationBase::evaluate
(integration_base.h:200-226): Eigen's Quaternion::inverse (conjugate / squaredNorm, nothing normalised), _transformVector,
toRotationMatrix, Utility::deltaQ (first order, w = 1), Qleft, Qright.  Raw residual r [15] and raw Jacobian J [15, 30] over the
local columns [pose_i 6 | speed/bias_i 9 | pose_j 6 | speed/bias_j 9]; rows P 0..2, R 3..5, V 6..8, BA 9..11, BG 12..14.

Information form.  What a window's linearisation holds of a factor is H_f = J^T P J, g_f = J^T P r, c_f = r^T P r / 2 with
P = cov^-1: none of them depends on WHICH square root of P whitened J and r, so they compare with a true long-double value
(P by a long-double Cholesky of cov).  Units: cond2(cov) ~ 8e8 is almost all scaling -- with d = sqrt(diag(cov)) the
Jacobi-scaled C = D^-1 cov D^-1 has cond2 ~ 14 -- and Cholesky / inversion of an SPD matrix are insensitive to diagonal
scaling (van der Sluis; Demmel), so a float64 P carries an entrywise error of order eps k_f / (d_i d_j), k_f = cond2(C) |C^-1|_2:
  unit_H_f = eps k_f a a^T,  unit_g_f = eps k_f a b,  unit_c_f = eps k_f b^2 / 2,   a = |J|^T d^-1 [30],  b = |r|^T d^-1.
The rank-one form is loose where a large and a small column meet (bias against position); there step_ref's unit
eps cond2(cov) |J_w|^T |J_w| (and |J_w|^T |r_w| for g) is the smaller one, and the unit is the entrywise MINIMUM of the two: nothing
is held more loosely than step_ref holds it.  An entry with unit 0 is a structural zero.

`python tests/imu_ref.py` prints the table YARDSTICK below was copied from."""
import ctypes as C
import functools

import numpy as np

import step_ref as sr
import vplines_slam_amd as v

LD = sr.LD
EPS64 = sr.EPS64
NF, NCAM = 11, 165            # frames; pose + speed/bias dims of a window (the IMU factors touch nothing behind them)


# ---- quaternions (w, x, y, z) as Eigen spells them, in the dtype of the operands -----------------------------------------
def _q(pose7, dt):
    p = np.asarray(pose7, dt)
    return np.array([p[6], p[3], p[4], p[5]], dt)


def qmul(a, b):
    aw, av, bw, bv = a[0], a[1:], b[0], b[1:]
    return np.concatenate([[aw * bw - av @ bv], aw * bv + bw * av + np.cross(av, bv)])


def qinv(q):
    """Quaternion::inverse: conjugate / squaredNorm"""
    return np.concatenate([[q[0]], -q[1:]]) / (q @ q)


def qrot(q, x):
    """_transformVector: v + w uv + qv x uv, uv = 2 qv x v (a rotation only for a unit q; q is not normalised here)"""
    uv = np.cross(q[1:], x)
    uv = uv + uv
    return x + q[0] * uv + np.cross(q[1:], uv)


def qmat(q):
    """toRotationMatrix (no normalisation)"""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], q.dtype)


def skew(t):
    z = t.dtype.type(0)
    return np.array([[z, -t[2], t[1]], [t[2], z, -t[0]], [-t[1], t[0], z]], t.dtype)


def _q44(q, sign):
    """Utility::Qleft (sign = +1) / Qright (-1)"""
    m = np.zeros((4, 4), q.dtype)
    m[0, 0], m[0, 1:], m[1:, 0] = q[0], -q[1:], q[1:]
    m[1:, 1:] = q[0] * np.eye(3, dtype=q.dtype) + sign * skew(q[1:])
    return m


class Pre:
    """what the factor reads of a vpl_preintegration, in dtype dt"""

    def __init__(self, p, dt=LD):
        a = lambda f: np.array(getattr(p, f), np.float64).astype(dt)
        self.sum_dt = dt(p.sum_dt)
        self.dp, self.dv, self.lba, self.lbg = a("delta_p"), a("delta_v"), a("linearized_ba"), a("linearized_bg")
        dq = a("delta_q")                                  # stored x, y, z, w
        self.dq = np.array([dq[3], dq[0], dq[1], dq[2]], dt)
        jac = a("jacobian").reshape(15, 15)
        self.dp_dba, self.dp_dbg, self.dq_dbg = jac[0:3, 9:12], jac[0:3, 12:15], jac[3:6, 12:15]
        self.dv_dba, self.dv_dbg = jac[6:9, 9:12], jac[6:9, 12:15]
        self.cov = np.array(p.covariance, np.float64).reshape(15, 15)


def raw(pre, pose_i, sb_i, pose_j, sb_j, g_norm, dt=LD, scale=None):
    """raw residual r [15] and Jacobian J [15, 30] of one factor in dtype dt.  scale: {name of a block of the raw Jacobian:
    factor}, for the sharpness check of the bars (pi_pp pi_pr pi_rr pi_vr si_pv si_pba si_pbg si_rbg si_vv si_vba si_vbg pj_pp
    pj_rr sj_vv)"""
    p = Pre(pre, dt)
    pi, si, pj, sj = (np.asarray(a, dt) for a in (pose_i, sb_i, pose_j, sb_j))
    Pi, Pj, Qi, Qj = pi[:3], pj[:3], _q(pi, dt), _q(pj, dt)
    Vi, Bai, Bgi, Vj, Baj, Bgj = si[0:3], si[3:6], si[6:9], sj[0:3], sj[3:6], sj[6:9]
    G = np.array([0, 0, g_norm], dt)
    t = p.sum_dt
    half = dt(1) / 2
    dba, dbg = Bai - p.lba, Bgi - p.lbg
    th = p.dq_dbg @ dbg
    cq = qmul(p.dq, np.concatenate([[dt(1)], th / 2]))                 # delta_q * deltaQ(dq_dbg dbg)
    cv = p.dv + p.dv_dba @ dba + p.dv_dbg @ dbg
    cp = p.dp + p.dp_dba @ dba + p.dp_dbg @ dbg
    Qii = qinv(Qi)
    ep = qrot(Qii, half * G * t * t + Pj - Pi - Vi * t)
    ev = qrot(Qii, G * t + Vj - Vi)
    r = np.zeros(15, dt)
    r[0:3] = ep - cp
    r[3:6] = 2 * qmul(qinv(cq), qmul(Qii, Qj))[1:]
    r[6:9] = ev - cv
    r[9:12] = Baj - Bai
    r[12:15] = Bgj - Bgi
    RiT = qmat(Qii)
    I3 = np.eye(3, dtype=dt)
    B = dict(pi_pp=((0, 0), -RiT), pi_pr=((0, 3), skew(ep)),
             pi_rr=((3, 3), -(_q44(qmul(qinv(Qj), Qi), 1) @ _q44(cq, -1))[1:, 1:]), pi_vr=((6, 3), skew(ev)),
             si_pv=((0, 6), -RiT * t), si_pba=((0, 9), -p.dp_dba), si_pbg=((0, 12), -p.dp_dbg),
             si_rbg=((3, 12), -_q44(qmul(qmul(qinv(Qj), Qi), cq), 1)[1:, 1:] @ p.dq_dbg),
             si_vv=((6, 6), -RiT), si_vba=((6, 9), -p.dv_dba), si_vbg=((6, 12), -p.dv_dbg),
             si_baba=((9, 9), -I3), si_bgbg=((12, 12), -I3),
             pj_pp=((0, 15), RiT), pj_rr=((3, 18), _q44(qmul(qmul(qinv(cq), Qii), Qj), 1)[1:, 1:]),
             sj_vv=((6, 21), RiT), sj_baba=((9, 24), I3), sj_bgbg=((12, 27), I3))
    J = np.zeros((15, 30), dt)
    for name, ((r0, c0), blk) in B.items():
        J[r0:r0 + 3, c0:c0 + 3] = blk * dt(scale[name]) if scale and name in scale else blk
    return r, J


def information_ld(cov):
    """P = cov^-1 by the long-double Cholesky: cov = L L^T, P = L^-T L^-1; and the lower factor of P (sqrt_info = its transpose)"""
    L = sr.cholesky_ld(cov)
    X = np.stack([sr.solve_lower(L, e, LD) for e in np.eye(15, dtype=LD)], axis=1)        # L^-1
    P = X.T @ X
    return P, sr.cholesky_ld(P)


class Factor:
    """one factor in information form, with its units.  r, J: raw, long double"""

    def __init__(self, r, J, cov):
        self.r, self.J, self.cov = r, J, np.asarray(cov, np.float64)
        P, LP = information_ld(cov)
        self.P = P
        self.H, self.g, self.c = J.T @ P @ J, J.T @ (P @ r), (r @ (P @ r)) / 2
        d = np.sqrt(np.diag(self.cov))
        Cs = self.cov / np.outer(d, d)
        self.cond_cov = float(np.linalg.cond(self.cov))
        self.k = float(np.linalg.cond(Cs) * np.linalg.norm(np.linalg.inv(Cs), 2))
        a = (np.abs(J).astype(np.float64) / d[:, None]).sum(axis=0)
        b = float((np.abs(r).astype(np.float64) / d).sum())
        Jw, rw = np.abs(LP.T @ J).astype(np.float64), np.abs(LP.T @ r).astype(np.float64)
        self.unit_H_old, self.unit_g_old = EPS64 * self.cond_cov * (Jw.T @ Jw), EPS64 * self.cond_cov * (Jw.T @ rw)
        self.unit_H = np.minimum(EPS64 * self.k * np.outer(a, a), self.unit_H_old)
        self.unit_g = np.minimum(EPS64 * self.k * a * b, self.unit_g_old)
        self.unit_c = EPS64 * self.k * b * b / 2


def factor(pre, pose_i, sb_i, pose_j, sb_j, g_norm, scale=None):
    r, J = raw(pre, pose_i, sb_i, pose_j, sb_j, g_norm, LD, scale)
    return Factor(r, J, np.array(pre.covariance, np.float64).reshape(15, 15))


def from_whitened(rw, Jw):
    """H, g, c (long double) of a whitened residual [15] and Jacobian [15, 30]: what an evaluator's output says in information form"""
    rw, Jw = np.asarray(rw, LD), np.asarray(Jw, LD)
    return Jw.T @ Jw, Jw.T @ rw, (rw @ rw) / 2


def jac480_to_30(jac):
    """the evaluators' four row-major blocks [15, 7 | 9 | 7 | 9] -> [15, 30] (the zero seventh pose column dropped)"""
    jac = np.asarray(jac)
    return np.concatenate([jac[0:105].reshape(15, 7)[:, :6], jac[105:240].reshape(15, 9), jac[240:345].reshape(15, 7)[:, :6],
                           jac[345:480].reshape(15, 9)], axis=1)


# ---- the float64 restatement of the device's path (yardstick) ----------------------------------------------------------
def whitened64(pre, pose_i, sb_i, pose_j, sb_j, g_norm):
    """k_prep + lin_imu_raw + lin_imu_whiten in float64: cov = G G^T, X = G^-1, P = X^T X, P = L L^T, sqrt_info = L^T; raw r, J in
    float64, whitened.  -> r_w [15], J_w [15, 30]"""
    cov = np.array(pre.covariance, np.float64).reshape(15, 15)
    G = np.linalg.cholesky(cov)
    X = np.stack([sr.solve_lower(G, e, np.float64) for e in np.eye(15)], axis=1)
    S = np.linalg.cholesky(X.T @ X).T
    r, J = raw(pre, pose_i, sb_i, pose_j, sb_j, g_norm, np.float64)
    return S @ r, S @ J


def _scatter(H, g, j, Hf, gf):
    """factor j (frames j - 1, j): its 30 local columns are the window's 15 (j - 1) .. 15 (j + 1) - 1"""
    s = slice(15 * (j - 1), 15 * (j + 1))
    H[s, s] += Hf
    g[s] += gf


def active(w):
    """the factors a solve evaluates: !(sum_dt > 10) (estimator.cpp:1088)"""
    return [j for j in range(1, NF) if not (w.preint[j].sum_dt > 10.0)]


class Share:
    """the IMU share of a window's H [165, 165], g [165] and cost at the states pose [11, 7], sb [11, 9], long double, with the
    units: the sums of the factors' units"""

    def __init__(self, w, pose, sb, g_norm, scale=None):
        self.H, self.g, self.cost = np.zeros((NCAM, NCAM), LD), np.zeros(NCAM, LD), LD(0)
        self.unit_H, self.unit_g, self.unit_cost = np.zeros((NCAM, NCAM)), np.zeros(NCAM), 0.0
        self.unit_H_old, self.unit_g_old = np.zeros((NCAM, NCAM)), np.zeros(NCAM)
        self.factors = {}
        for j in active(w):
            f = factor(w.preint[j], pose[j - 1], sb[j - 1], pose[j], sb[j], g_norm, scale)
            self.factors[j] = f
            _scatter(self.H, self.g, j, f.H, f.g)
            _scatter(self.unit_H, self.unit_g, j, f.unit_H, f.unit_g)
            _scatter(self.unit_H_old, self.unit_g_old, j, f.unit_H_old, f.unit_g_old)
            self.cost += f.c
            self.unit_cost += f.unit_c


def share64(w, pose, sb, g_norm, order=None):
    """the same share by the float64 restatement, the factors summed in `order`"""
    H, g, cost = np.zeros((NCAM, NCAM)), np.zeros(NCAM), 0.0
    js = active(w)
    for k in (range(len(js)) if order is None else order):
        j = js[k]
        rw, Jw = whitened64(w.preint[j], pose[j - 1], sb[j - 1], pose[j], sb[j], g_norm)
        _scatter(H, g, j, Jw.T @ Jw, Jw.T @ rw)
        cost += 0.5 * float(rw @ rw)
    return H, g, cost


def share_oracle(w, pose, sb, g_norm):
    """the same share from the oracle's whitened evaluator (float64), summed in long double"""
    import oracle_api as o
    H, g, cost = np.zeros((NCAM, NCAM), LD), np.zeros(NCAM, LD), LD(0)
    for j in active(w):
        r, jac = o.imu_factor(np.concatenate([pose[j - 1], sb[j - 1], pose[j], sb[j]])[None], [w.preint[j]], g_norm)
        Hf, gf, cf = from_whitened(r[0], jac480_to_30(jac[0]))
        _scatter(H, g, j, Hf, gf)
        cost += cf
    return H, g, cost


def rho3(H, g, cost, ref):
    """(rho_H, rho_g, rho_cost) of a share against the reference share `ref`"""
    return (sr.rho(H, ref.H, ref.unit_H), sr.rho(g, ref.g, ref.unit_g), float(abs(LD(cost) - ref.cost)) / ref.unit_cost)


# ---- the cases of test_imu_reference.py, test_gpu_imu_linearisation.py and test_gpu_factors.py -----------------------------
def _set_pre(w, j, pre):
    C.memmove(C.byref(w.preint[j]), C.byref(pre), C.sizeof(v.Preintegration))


def _preintegrate(samples, acc0, gyr0, ba, bg, opt):
    """orc_preintegrate over `samples` [n, 7] (dt, acc, gyr) after the first measurement (acc0, gyr0), linearised at (ba, bg)"""
    import oracle_api as o
    out = v.Preintegration()
    p = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    s = np.ascontiguousarray(samples, np.float64)
    o.load().orc_preintegrate(s.shape[0], p(s), p(acc0), p(gyr0), p(ba), p(bg), C.byref(opt), C.byref(out))
    return out


def displace_biases(w):
    """m1's edit: every frame's biases a common 0.02 (accelerometer) / 0.005 (gyroscope) off the linearisation point of the
    pre-integrations, and from frame to frame a random walk of steps of up to 3 sqrt(cov_ii) of the bias rows (~1e-6, ~1e-7):
    whitened bias residuals of O(1..10), correction terms dp_dba dba ... of 1e-4 m"""
    w = w.copy()
    rng = np.random.default_rng(5150)
    w.speed_bias[:, 3:6] += 0.02 * np.array([1.0, -0.7, 0.4])
    w.speed_bias[:, 6:9] += 0.005 * np.array([-0.6, 1.0, 0.8])
    for f in range(1, NF):
        sd = np.sqrt(np.diag(np.array(w.preint[f].covariance).reshape(15, 15)))
        w.speed_bias[f, 3:9] = w.speed_bias[f - 1, 3:9] + rng.uniform(-3, 3, 6) * sd[9:15]
    return w


def unequal_intervals(w0):
    """m2's edit of a window without landmarks, every frame's state staying consistent with its pre-integrations: frame 4
    leaves, so interval 4 is pre-integrated over the concatenated samples of 4 and 5 (sum_dt ~ 0.2, what a MARGIN_SECOND_NEW merge
    leaves), frames 5..9 move up; interval 10 is cut after 60 % of its samples, where a new frame 9 is propagated from frame 8 by
    the first part (and moved a little, so that its residuals are not zero); the rest is the new, short interval 10"""
    w = w0.copy()
    opt = v.default_options()
    imu, acc0, gyr0 = w0.extra["imu_samples"], w0.extra["imu_acc0"], w0.extra["imu_gyr0"]
    ba, bg = w0.speed_bias[0, 3:6], w0.speed_bias[0, 6:9]
    assert np.all(w0.speed_bias[:, 3:9] == w0.speed_bias[0, 3:9]) and len(w0.point_start) == 0 and len(w0.line_start) == 0
    _set_pre(w, 4, _preintegrate(np.concatenate([imu[4], imu[5]]), acc0[4], gyr0[4], ba, bg, opt))
    for k in range(4, 9):
        w.pose[k], w.speed_bias[k] = w0.pose[k + 1], w0.speed_bias[k + 1]
    for k in range(5, 9):
        _set_pre(w, k, w0.preint[k + 1])
    n1 = (6 * len(imu[10])) // 10
    first = _preintegrate(imu[10][:n1], acc0[10], gyr0[10], ba, bg, opt)
    last = _preintegrate(imu[10][n1:], imu[10][n1 - 1, 1:4], imu[10][n1 - 1, 4:7], ba, bg, opt)
    _set_pre(w, 9, first)
    _set_pre(w, 10, last)
    # the frame where the cut is: P = Pi + Vi t - G t^2 / 2 + Ri dp, V = Vi - G t + Ri dv, Q = Qi dq (integration_base.h:220-222)
    Pi, Vi, qi = w0.pose[9, :3], w0.speed_bias[9, :3], w0.pose[9, 3:] / np.linalg.norm(w0.pose[9, 3:])
    Ri, t, G = sr.quat_R(qi), first.sum_dt, np.array([0.0, 0.0, opt.g_norm])
    rng = np.random.default_rng(5151)
    dq = np.array(first.delta_q)
    q = qmul(np.array([qi[3], qi[0], qi[1], qi[2]]), np.array([dq[3], dq[0], dq[1], dq[2]]))
    q = qmul(q, np.concatenate([[1.0], 1e-3 * rng.normal(size=3)]))
    q /= np.linalg.norm(q)
    w.pose[9, :3] = Pi + Vi * t - 0.5 * G * t * t + Ri @ np.array(first.delta_p) + 1e-3 * rng.normal(size=3)
    w.pose[9, 3:] = [q[1], q[2], q[3], q[0]]
    w.speed_bias[9, :3] = Vi - G * t + Ri @ np.array(first.delta_v) + 1e-3 * rng.normal(size=3)
    w.speed_bias[9, 3:9] = w0.speed_bias[9, 3:9]
    w.pose[10], w.speed_bias[10] = w0.pose[10], w0.speed_bias[10]
    return w


@functools.lru_cache(maxsize=None)
def cases():
    """id -> (Window, options): m0 .. m5 of DESIGN.md 2; options as step_ref's (one iteration, no marginalisation)"""
    sc = sr.cases()
    opt = sr._options()
    out = {"m0": (sc["a"][0], opt)}
    out["m1"] = (displace_biases(sc["a"][0]), opt)
    out["m2"] = (unequal_intervals(sc["a"][0]), opt)
    w = displace_biases(sc["a"][0])
    w.preint[6].sum_dt = 10.5                 # m3: factor 6 is skipped; frames 0..5 and 6..10 fall apart
    out["m3"] = (w, sr._options(num_iterations=0))
    out["m4"] = (displace_biases(sc["c"][0]), opt)
    out["m5"] = (displace_biases(sc["f"][0]), opt)
    return out


IMU_ONLY = ("m0", "m1", "m2", "m3")


def states(w):
    """the states the oracle and k_prep linearise at (step_ref.Problem.initial_state): quaternions through a rotation matrix"""
    pose = w.pose.copy()
    for q in pose[:, 3:]:
        q[:] = sr.R_quat(sr.quat_R(q / np.linalg.norm(q)))
    return pose, w.speed_bias.copy()


@functools.lru_cache(maxsize=None)
def reference(case):
    """(Window, options, pose, sb, Share) of a case at the window's own initial state"""
    w, opt = cases()[case]
    pose, sb = states(w)
    return w, opt, pose, sb, Share(w, pose, sb, opt.g_norm)


class Combined:
    """a whole window (m4, m5): step_ref's linearisation with its IMU rows (the oracle's float64 whitened evaluator) taken out and
    the long-double IMU share put in.  Units: step_ref's of the remaining rows (prior, points, lines: w = 1) + the IMU units;
    cost unit: eps64 x the rest of the cost + the IMU cost unit.  sb: the speed/bias dims 15 f + 6 .. 15 f + 14, which only IMU
    factors and the prior touch.  orth: the line parameters to linearise at (the device's own; default the window's)"""

    def __init__(self, case, orth=None):
        w, opt, pose, sb, share = reference(case)
        self.prob = prob = sr.Problem(w, opt)
        self.x0 = x0 = prob.initial_state()
        assert np.array_equal(x0["pose"], pose) and np.array_equal(x0["sb"], sb)
        self.x = dict(x0, invd=w.inv_depth[:prob.nP].copy(), orth=x0["orth"] if orth is None else np.array(orth))
        full = prob.linearize(self.x)
        n = prob.n
        self.sb = np.zeros(n, bool)
        self.sb[(15 * np.arange(NF)[:, None] + 6 + np.arange(9)).ravel()] = True
        vis = np.ones(len(full.r), bool)
        for kind, m0, m in full.kinds:
            if kind == "imu":
                vis[m0:m0 + m] = False
            elif kind != "prior":
                assert np.all(full.J[m0:m0 + m][:, self.sb] == 0), "a visual factor touches a speed/bias column"
        Jv, rv = full.J[vis], full.r[vis]
        aJ, ar = np.abs(Jv).astype(np.float64), np.abs(rv).astype(np.float64)
        self.H, self.g = Jv.T @ Jv, Jv.T @ rv
        self.unit_H, self.unit_g = EPS64 * (aJ.T @ aJ), EPS64 * (aJ.T @ ar)
        self.H[:NCAM, :NCAM] += share.H
        self.g[:NCAM] += share.g
        self.unit_H[:NCAM, :NCAM] += share.unit_H
        self.unit_g[:NCAM] += share.unit_g
        cost_vis = full.cost - (full.r[~vis] @ full.r[~vis]) / 2
        self.cost, self.unit_cost = cost_vis + share.cost, EPS64 * float(cost_vis) + share.unit_cost

    def rhos(self, H, g, cost):
        """-> rho_H, rho_g over the entries with a speed/bias row or column, rho_H, rho_g over the others, rho_cost"""
        sbm = self.sb[:, None] | self.sb[None, :]
        part = lambda a, b, u, m: sr.rho(np.where(m, a, 0), np.where(m, b, 0), np.where(m, u, 0))
        return (part(H, self.H, self.unit_H, sbm), part(g, self.g, self.unit_g, self.sb),
                part(H, self.H, self.unit_H, ~sbm), part(g, self.g, self.unit_g, ~self.sb),
                float(abs(LD(cost) - self.cost)) / self.unit_cost)


def yardstick(case, seed):
    """rho_ref of H, g, cost: the float64 restatement of the device's path, factors in a shuffled order, states one ulp away;
    and the same with the inputs shared exactly (what the single-factor ABI is held to), worst factor"""
    w, opt, pose, sb, ref = reference(case)
    rng = np.random.default_rng(seed)
    x = sr.perturbed(dict(pose=pose, sb=sb), rng)
    H, g, c = share64(w, x["pose"], x["sb"], opt.g_norm, order=rng.permutation(len(active(w))))
    out = dict(zip(("H", "g", "cost"), rho3(H, g, c, ref)))
    fH = fg = fc = 0.0
    for j, f in ref.factors.items():
        rw, Jw = whitened64(w.preint[j], pose[j - 1], sb[j - 1], pose[j], sb[j], opt.g_norm)
        Hf, gf, cf = from_whitened(rw, Jw)
        fH, fg = max(fH, sr.rho(Hf, f.H, f.unit_H)), max(fg, sr.rho(gf, f.g, f.unit_g))
        fc = max(fc, float(abs(cf - f.c)) / f.unit_c)
    out.update(fH=fH, fg=fg, fcost=fc, k=max(f.k for f in ref.factors.values()))
    return out


@functools.lru_cache(maxsize=None)
def candidate(case):
    """(Window, options, pose, sb, Share) at x0 [+] delta_ref, the candidate of the reference's first step (step_ref.step on the
    window's long-double linearisation): where k_cost evaluates the cost, up to the rounding of the step"""
    w, opt, _, _, _ = reference(case)
    prob = sr.Problem(w, opt)
    x0 = prob.initial_state()
    lin = prob.linearize(x0)
    xc = prob.plus(x0, sr.step(lin.H, lin.g, lin.J)["delta"])
    return w, opt, xc["pose"], xc["sb"], Share(w, xc["pose"], xc["sb"], opt.g_norm)


def yardstick_step(case, seed):
    """rho_ref of the cost at the candidate.  Its own entry: the unit eps k_f b^2 / 2 shrinks with the residuals, what the
    rounding of the raw residuals (eps x positions of metres, whitened) does to the cost shrinks with their first power only"""
    w, opt, pose, sb, ref = candidate(case)
    rng = np.random.default_rng(seed)
    x = sr.perturbed(dict(pose=pose, sb=sb), rng)
    _, _, c = share64(w, x["pose"], x["sb"], opt.g_norm, order=rng.permutation(len(active(w))))
    return dict(cost=float(abs(LD(c) - ref.cost)) / ref.unit_cost)


# Yardsticks of the float64 restatement on the CPU (`python tests/imu_ref.py` prints this table): rho_ref of H, g, cost of the
# window's IMU share (shuffled order, states one ulp away, seed 2000 + position of the case) and of the single factors at
# shared inputs (fH, fg, fcost: the worst factor), in the units above; m1_step: the cost at the candidate of m1's first step.
YARDSTICK = {
    "m0": dict(H=0.22, g=8.25, cost=0.636, fH=0.145, fg=1.19, fcost=0.832),   # k_f = 105
    "m1": dict(H=0.206, g=7.23, cost=1.64, fH=0.145, fg=1.23, fcost=0.728),   # k_f = 105
    "m2": dict(H=0.196, g=8.39, cost=0.499, fH=0.145, fg=1.19, fcost=0.832),   # k_f = 107
    "m3": dict(H=0.161, g=6.74, cost=0.802, fH=0.145, fg=1.23, fcost=0.728),   # k_f = 105
    "m4": dict(H=0.207, g=6.3, cost=0.437, fH=0.169, fg=0.904, fcost=0.6),   # k_f = 105
    "m5": dict(H=0.321, g=5.3, cost=0.496, fH=0.233, fg=1.38, fcost=0.564),   # k_f = 105
    "m1_step": dict(cost=367),   # cost 10 at the candidate
}
MARGIN = 8.0


def bar(what, case):
    """what a device ratio may reach: MARGIN * max(the case's yardstick, 1)"""
    return MARGIN * max(YARDSTICK[case][what], 1.0)


def measure():
    out = {case: yardstick(case, 2000 + k) for k, case in enumerate(cases())}
    out["m1_step"] = yardstick_step("m1", 2000 + len(out))
    return out


if __name__ == "__main__":
    for case, y in measure().items():
        if case == "m1_step":
            print('    "m1_step": dict(cost=%.3g),   # cost %.3g at the candidate' % (y["cost"], float(candidate("m1")[4].cost)))
            continue
        print('    "%s": dict(H=%.3g, g=%.3g, cost=%.3g, fH=%.3g, fg=%.3g, fcost=%.3g),   # k_f = %.3g'
              % (case, y["H"], y["g"], y["cost"], y["fH"], y["fg"], y["fcost"], y["k"]))
