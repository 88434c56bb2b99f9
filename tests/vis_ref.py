"""The point, line and vanishing-point factors, the two local parameterisations and the two robust losses in any NumPy dtype,
np.longdouble by default -- the reference test_vis_reference.py checks against its own central differences and holds the oracle to
on the CPU, and test_gpu_vis_factors.py holds the device evaluators, k_lin's point and line phases, k_cost and k_line_opt's first
evaluation to.  Run with dt = np.float64 it is the yardstick: what float64 reaches on the same formulas.

Written from the formulas of ProjectionFactor (projection_factor.cpp:6-19 tangent base, 26-126 Evaluate, UNIT_SPHERE_ERROR as
parameters.h:27 defines it), lineProjectionFactor::Evaluate (line_projection_factor.cpp:251-380), vpProjectionFactor::Evaluate
(line_projection_factor.cpp:11-153; its Jacobian is the literal matrix of lines 62-64, not a derivative), plk_to_orth /
orth_to_plk / plk_to_pose / plk_from_pose / skew_symmetric (line_geometry.cpp:62-126, 155-159, 198-216),
LineOrthParameterization::Plus (line_parameterization.cpp:7-66), PoseLocalParameterization::Plus
(pose_local_parameterization.cpp:3-19) and Utility::deltaQ (utility.h:12-24); ceres' HuberLoss / CauchyLoss::Evaluate and the
corrector's sqrt(rho') scale.  Quaternions as Eigen spells them (imu_ref's qmul, qinv, qrot, qmat): q * v for the residual,
toRotationMatrix for the Jacobians, matrix products left to right, nothing normalised that the reference does not normalise.

Layouts are oracle_api's: projection(params [n, 22], pts [n, 6]) -> r [n, 2], jac [n, 44] (2 x 7 | 2 x 7 | 2 x 7 | 2 x 1 row-major,
the seventh pose columns 0); line / vp(params [n, 18], obs [n, 4] / vp [n, 3]) -> r [n, 2], jac [n, 36] (2 x 7 | 2 x 7 | 2 x 4).

Units (rho = error / unit).  Of output entry k of an evaluator f at float64 inputs x, everything in long double:
    unit_k = eps64 |f_k(x)| + sum_i |f_k(x + spacing(x_i) e_i) - f_k(x)|      over the non-zero inputs (parameters and observations),
what rounding the inputs alone may do to the entry.  An entry with unit 0 is a structural zero.  Bar of a case:
step_ref.MARGIN x max(yardstick, 1), the yardstick being the worst rho of this module's float64 run against its long-double run
on the inputs of the case (YARDSTICK; `python tests/vis_ref.py` prints the tables it was copied from).  line_orth_plus and
plk_to_orth are compared as orth_to_plk(out), normalised to |n|^2 + |v|^2 = 1, up to the common sign: near theta_1 = +-pi/2 the
three Euler angles are not individually determined."""
import functools

import numpy as np

import step_ref as sr
import vplines_slam_amd as v
from imu_ref import _q, qinv, qmat, qmul, qrot, skew

LD = sr.LD
EPS64 = sr.EPS64
MARGIN = sr.MARGIN
TINY = np.finfo(np.float64).tiny
SQRT_INFO = dict(proj=460.0 / 1.5, line=306.666666667, vp=10.0)       # oracle_api's defaults


def _norm(a):
    return np.sqrt(a @ a)


def _normalized(a):
    """MatrixBase::normalized: a / sqrt(squaredNorm) where that is positive"""
    n2 = a @ a
    return a / np.sqrt(n2) if n2 > 0 else a


# ---- line geometry (line_geometry.cpp) -----------------------------------------------------------------------------------
def _orth_R(theta):
    s1, c1, s2, c2, s3, c3 = np.sin(theta[0]), np.cos(theta[0]), np.sin(theta[1]), np.cos(theta[1]), np.sin(theta[2]), np.cos(theta[2])
    return np.array([[c2 * c3, s1 * s2 * c3 - c1 * s3, c1 * s2 * c3 + s1 * s3],
                     [c2 * s3, s1 * s2 * s3 + c1 * c3, c1 * s2 * s3 - s1 * c3],
                     [-s2, s1 * c2, c1 * c2]], theta.dtype)


def orth_to_plk(orth, dt=LD):
    """line_geometry.cpp:86-126: n = cos(phi) u1, v = sin(phi) u2"""
    orth = np.asarray(orth, dt)
    R = _orth_R(orth[:3])
    return np.concatenate([np.cos(orth[3]) * R[:, 0], np.sin(orth[3]) * R[:, 1]])


def plk_to_orth(plk, dt=LD):
    """line_geometry.cpp:62-83"""
    plk = np.asarray(plk, dt)
    n, vv = plk[:3], plk[3:]
    u1, u2 = n / _norm(n), vv / _norm(vv)
    u3 = np.cross(u1, u2)
    w = np.array([_norm(n), _norm(vv)], dt)
    w = w / _norm(w)
    return np.array([np.arctan2(u2[2], u3[2]), np.arcsin(-u1[2]), np.arctan2(u1[1], u1[0]), np.arcsin(w[1])], dt)


def _plk_to_pose(L, Rcw, tcw):
    nw, vw = L[:3], L[3:]
    return np.concatenate([Rcw @ nw + (skew(tcw) @ Rcw) @ vw, Rcw @ vw])


def _plk_from_pose(L, Rcw, tcw):
    Rwc = Rcw.T
    return _plk_to_pose(L, Rwc, -(Rwc @ tcw))


def plk_unit(orth, dt=LD):
    """orth_to_plk(orth) scaled to |n|^2 + |v|^2 = 1: what two sets of angles are compared as"""
    L = orth_to_plk(orth, dt)
    return L / _norm(L)


# ---- the parameterisations ---------------------------------------------------------------------------------------------
def _pose_plus1(x, dt):
    x = np.asarray(x, dt)
    q = qmul(_q(x[0:7], dt), np.concatenate([[dt(1)], x[10:13] / dt(2)]))          # _q * deltaQ(delta + 3)
    q = q / _norm(q)
    return np.concatenate([x[0:3] + x[7:10], q[1:], q[:1]])


def _orth_plus1(x, dt):
    x = np.asarray(x, dt)
    th, phi, d = x[0:3], x[3], x[4:8]
    one, zero = dt(1), dt(0)
    R = _orth_R(th)
    w1, w2 = np.cos(phi), np.sin(phi)
    Rz = np.array([[np.cos(d[2]), -np.sin(d[2]), zero], [np.sin(d[2]), np.cos(d[2]), zero], [zero, zero, one]], dt)
    Ry = np.array([[np.cos(d[1]), zero, np.sin(d[1])], [zero, one, zero], [-np.sin(d[1]), zero, np.cos(d[1])]], dt)
    Rx = np.array([[one, zero, zero], [zero, np.cos(d[0]), -np.sin(d[0])], [zero, np.sin(d[0]), np.cos(d[0])]], dt)
    R = ((R @ Rx) @ Ry) @ Rz
    W = np.array([[w1, -w2], [w2, w1]], dt) @ np.array([[np.cos(d[3]), -np.sin(d[3])], [np.sin(d[3]), np.cos(d[3])]], dt)
    return np.array([np.arctan2(R[2, 1], R[2, 2]), np.arcsin(-R[2, 0]), np.arctan2(R[1, 0], R[0, 0]), np.arcsin(W[1, 0])], dt)


def pose_plus(x, delta, dt=LD):
    """PoseLocalParameterization::Plus on x [n, 7], delta [n, 6]"""
    return np.stack([_pose_plus1(np.concatenate([a, b]), dt) for a, b in zip(np.atleast_2d(x), np.atleast_2d(delta))])


def line_orth_plus(x, delta, dt=LD):
    """LineOrthParameterization::Plus on x [n, 4], delta [n, 4]"""
    return np.stack([_orth_plus1(np.concatenate([a, b]), dt) for a, b in zip(np.atleast_2d(x), np.atleast_2d(delta))])


# ---- the losses (ceres loss_function.cc; corrector.cc with rho'' <= 0: residual and Jacobian scaled by sqrt(rho')) -----
def huber(s, delta, dt=LD):
    """HuberLoss(delta) at s = |r|^2 -> rho, sqrt(rho')"""
    s, a = dt(s), dt(delta)
    b = a * a
    if s > b:
        r = np.sqrt(s)
        return 2 * a * r - b, np.sqrt(max(dt(TINY), a / r))
    return s, dt(1)


def cauchy(s, a=1.0, dt=LD):
    """CauchyLoss(a) at s -> rho = b log(1 + s / b), sqrt(rho') = sqrt(1 / (1 + s / b))"""
    s, b = dt(s), dt(a) * dt(a)
    c = 1 / b
    total = 1 + s * c
    return b * np.log(total), np.sqrt(max(dt(TINY), 1 / total))


# ---- ProjectionFactor ----------------------------------------------------------------------------------------------------
PROJ_BLOCKS = dict(i_pos=[0, 1, 2, 7, 8, 9], i_rot=[3, 4, 5, 10, 11, 12], j=list(range(14, 20)) + list(range(21, 27)),
                   ex=list(range(28, 34)) + list(range(35, 41)), invd=[42, 43])
LINE_BLOCKS = dict(pose=list(range(0, 6)) + list(range(7, 13)), ex=list(range(14, 20)) + list(range(21, 27)), orth=list(range(28, 36)))


def _pad7(J6):
    return np.concatenate([J6, np.zeros((J6.shape[0], 1), J6.dtype)], axis=1).ravel()


def _proj1(x, sqrt_info, dt, want_jac=True):
    """x = params [22] | pts_i [3] | pts_j [3] -> r [2] | jac [44]"""
    x = np.asarray(x, dt)
    si = dt(sqrt_info)
    Pi, Qi, Pj, Qj, tic, qic, inv_dep = x[0:3], _q(x[0:7], dt), x[7:10], _q(x[7:14], dt), x[14:17], _q(x[14:21], dt), x[21]
    pts_i, pts_j = x[22:25], x[25:28]
    a = _normalized(pts_j)
    tmp = np.array([0, 0, 1], dt)
    if np.array_equal(a, tmp):
        tmp = np.array([1, 0, 0], dt)
    b1 = _normalized(tmp - a * (a @ tmp))
    tangent_base = np.stack([b1, np.cross(a, b1)])
    pts_camera_i = pts_i / inv_dep
    pts_imu_i = qrot(qic, pts_camera_i) + tic
    pts_w = qrot(Qi, pts_imu_i) + Pi
    pts_imu_j = qrot(qinv(Qj), pts_w - Pj)
    pts_camera_j = qrot(qinv(qic), pts_imu_j - tic)
    r = si * (tangent_base @ (_normalized(pts_camera_j) - _normalized(pts_j)))
    if not want_jac:
        return r
    Ri, Rj, ric = qmat(Qi), qmat(Qj), qmat(qic)
    norm = _norm(pts_camera_j)
    norm_jaco = np.eye(3, dtype=dt) / norm - np.outer(pts_camera_j, pts_camera_j) / (norm * norm * norm)
    reduce = si * (tangent_base @ norm_jaco)
    A = (ric.T @ Rj.T) @ Ri
    jaco_i = np.concatenate([ric.T @ Rj.T, A @ -skew(pts_imu_i)], axis=1)
    jaco_j = np.concatenate([ric.T @ -Rj.T, ric.T @ skew(pts_imu_j)], axis=1)
    tmp_r = A @ ric
    jaco_ex = np.concatenate([ric.T @ (Rj.T @ Ri - np.eye(3, dtype=dt)),
                              -tmp_r @ skew(pts_camera_i) + skew(tmp_r @ pts_camera_i)
                              + skew(ric.T @ (Rj.T @ (Ri @ tic + Pi - Pj) - tic))], axis=1)
    jaco_f = ((((reduce @ ric.T) @ Rj.T) @ Ri) @ ric) @ pts_i * dt(-1) / (inv_dep * inv_dep)
    return np.concatenate([r, _pad7(reduce @ jaco_i), _pad7(reduce @ jaco_j), _pad7(reduce @ jaco_ex), jaco_f])


# ---- lineProjectionFactor / vpProjectionFactor -------------------------------------------------------------------------------
def _line_chain(x, dt):
    twb, Rwb, tbc, Rbc = x[0:3], qmat(_q(x[0:7], dt)), x[7:10], qmat(_q(x[7:14], dt))
    Lw = orth_to_plk(x[14:18], dt)
    Lb = _plk_from_pose(Lw, Rwb, twb)
    return twb, Rwb, tbc, Rbc, Lw, Lb, _plk_from_pose(Lb, Rbc, tbc)


def _line_jac(chain, jaco_e_Lc, dt):
    """the three Jacobian blocks both factors share, from jaco_e_Lc [2, 6] -> jac [36]"""
    twb, Rwb, tbc, Rbc, Lw, Lb, _ = chain
    Z = np.zeros((3, 3), dt)
    invTbc = np.block([[Rbc.T, -Rbc.T @ skew(tbc)], [Z, Rbc.T]])
    nw, dw = Lw[:3], Lw[3:]
    jaco_Lc_pose = np.block([[Rwb.T @ skew(dw), skew(Rwb.T @ (nw + skew(dw) @ twb))], [Z, skew(Rwb.T @ dw)]])
    jaco_Lc_pose = invTbc @ jaco_Lc_pose
    nb, db = Lb[:3], Lb[3:]
    jaco_Lc_ex = np.block([[Rbc.T @ skew(db), skew(Rbc.T @ (nb + skew(db) @ tbc))], [Z, skew(Rbc.T @ db)]])
    Rwc = Rwb @ Rbc
    twc = Rwb @ tbc + twb
    invTwc = np.block([[Rwc.T, -Rwc.T @ skew(twc)], [Z, Rwc.T]])
    u1, u2 = nw / _norm(nw), dw / _norm(dw)
    u3 = np.cross(u1, u2)
    w = np.array([_norm(nw), _norm(dw)], dt)
    w = w / _norm(w)
    K = np.zeros((6, 4), dt)
    K[3:6, 0] = w[1] * u3
    K[0:3, 1] = -w[0] * u3
    K[0:3, 2], K[3:6, 2] = w[0] * u2, -w[1] * u1
    K[0:3, 3], K[3:6, 3] = -w[1] * u1, w[0] * u2
    return np.concatenate([_pad7(jaco_e_Lc @ jaco_Lc_pose), _pad7(jaco_e_Lc @ jaco_Lc_ex), ((jaco_e_Lc @ invTwc) @ K).ravel()])


def _line1(x, sqrt_info, dt, want_jac=True):
    """x = params [18] | obs [4] -> r [2] | jac [36]"""
    x = np.asarray(x, dt)
    si, obs = dt(sqrt_info), x[18:22]
    chain = _line_chain(x, dt)
    nc = chain[6][:3]
    l_norm = nc[0] * nc[0] + nc[1] * nc[1]
    l_sqrtnorm = np.sqrt(l_norm)
    l_trinorm = l_norm * l_sqrtnorm
    e1 = obs[0] * nc[0] + obs[1] * nc[1] + nc[2]
    e2 = obs[2] * nc[0] + obs[3] * nc[1] + nc[2]
    r = si * np.array([e1 / l_sqrtnorm, e2 / l_sqrtnorm], dt)
    if not want_jac:
        return r
    jaco_e_l = si * np.array([[obs[0] / l_sqrtnorm - nc[0] * e1 / l_trinorm, obs[1] / l_sqrtnorm - nc[1] * e1 / l_trinorm, 1 / l_sqrtnorm],
                              [obs[2] / l_sqrtnorm - nc[0] * e2 / l_trinorm, obs[3] / l_sqrtnorm - nc[1] * e2 / l_trinorm, 1 / l_sqrtnorm]], dt)
    return np.concatenate([r, _line_jac(chain, np.concatenate([jaco_e_l, np.zeros((2, 3), dt)], axis=1), dt)])


def _vp1(x, sqrt_info, dt, want_jac=True):
    """x = params [18] | vp [3] -> r [2] | jac [36]"""
    x = np.asarray(x, dt)
    si, ob = dt(sqrt_info), x[18:21]
    chain = _line_chain(x, dt)
    d_c = chain[6][3:]
    vp_2d = np.array([ob[0] / ob[2], ob[1] / ob[2]], dt)
    r = si * np.array([d_c[0] / d_c[2] - vp_2d[0], d_c[1] / d_c[2] - vp_2d[1]], dt)
    if not want_jac:
        return r
    zero = dt(0)
    jaco_e_l = si * np.array([[-1 / ob[2], zero, vp_2d[0]], [zero, -1 / ob[2], vp_2d[1]]], dt)
    return np.concatenate([r, _line_jac(chain, np.concatenate([np.zeros((2, 3), dt), jaco_e_l], axis=1), dt)])


def _batched(f1, params, consts, sqrt_info, dt, want_jac):
    out = np.stack([f1(np.concatenate([p, c]), sqrt_info, dt, want_jac) for p, c in zip(np.atleast_2d(params), np.atleast_2d(consts))])
    return (out[:, :2], out[:, 2:]) if want_jac else (out, None)


def projection(params, pts, sqrt_info=SQRT_INFO["proj"], want_jac=True, dt=LD):
    return _batched(_proj1, params, pts, sqrt_info, dt, want_jac)


def line(params, obs, sqrt_info=SQRT_INFO["line"], want_jac=True, dt=LD):
    return _batched(_line1, params, obs, sqrt_info, dt, want_jac)


def vp(params, vp_obs, sqrt_info=SQRT_INFO["vp"], want_jac=True, dt=LD):
    return _batched(_vp1, params, vp_obs, sqrt_info, dt, want_jac)


# ---- evaluators by kind: f(x [nin], dt) -> out [nout]; x = the float64 inputs of one factor, concatenated --------------------
KINDS = {
    "proj": (lambda x, dt: _proj1(x, SQRT_INFO["proj"], dt), 22),
    "line": (lambda x, dt: _line1(x, SQRT_INFO["line"], dt), 18),
    "vp": (lambda x, dt: _vp1(x, SQRT_INFO["vp"], dt), 18),
    "pose_plus": (_pose_plus1, 7),
    "orth_plus": (_orth_plus1, 4),
    "plk_to_orth": (lambda x, dt: plk_to_orth(x, dt), 6),
    "orth_to_plk": (lambda x, dt: orth_to_plk(x, dt), 4),
}
AS_PLK = ("orth_plus", "plk_to_orth")      # kinds whose output angles are compared as the normalised Pluecker vector


def compared(kind, out, dt=LD):
    """what of an evaluator's output [n, nout] (float64 or dt) is compared: itself, or the normalised Pluecker vector of its angles"""
    out = np.atleast_2d(np.asarray(out, dt))
    return np.stack([plk_unit(a, dt) for a in out]) if kind in AS_PLK else out


def run(kind, X, dt=LD):
    """the evaluator of `kind` on the rows of X (float64) in dtype dt -> out [n, nout]"""
    f = KINDS[kind][0]
    return np.stack([f(x, dt) for x in np.atleast_2d(X)])


def units(kind, X):
    """-> ref [n, m] (long double, as compared), unit [n, m] (float64) of the rows of X"""
    f = KINDS[kind][0]
    g = (lambda x: plk_unit(f(x, LD))) if kind in AS_PLK else (lambda x: f(x, LD))
    refs, us = [], []
    for x in np.atleast_2d(np.asarray(X, np.float64)):
        f0 = g(x)
        u = EPS64 * np.abs(f0)
        for i in np.nonzero(x)[0]:
            xp = x.copy()
            xp[i] = x[i] + np.spacing(abs(x[i]))
            u = u + np.abs(g(xp) - f0)
        refs.append(f0)
        us.append(u.astype(np.float64))
    return np.stack(refs), np.stack(us)


def rho_rows(kind, out, ref, unit):
    """rho per factor and entry [n, m] of an evaluator's output (float64) against units(); kinds compared as Pluecker vectors up to
    the common sign.  An entry with unit 0 gives 0 where the output is exactly 0.0 and inf where it is not"""
    c = compared(kind, out)
    err = np.abs(c - ref)
    if kind in AS_PLK:
        flip = np.abs(c + ref)
        use = flip.max(axis=1) < err.max(axis=1)
        err[use] = flip[use]
    with np.errstate(divide="ignore", invalid="ignore"):
        rr = np.where(unit > 0, err / np.where(unit > 0, unit, 1), np.where(err == 0, 0.0, np.inf))
    return rr.astype(np.float64)


# ---- the cases ---------------------------------------------------------------------------------------------------
NGEN, NEDGE = 64, 4           # factors of a generic case / of an edge case


def _proj_draw(rng):
    """as test_gpu_factors.test_projection_factor_parity draws them"""
    from test_oracle_factors import rand_pose
    Pi, Pj = rand_pose(rng, 0.5), rand_pose(rng, 0.5)
    Pj[3:] = Pi[3:] + 0.1 * rng.normal(size=4)
    Pj[3:] /= np.linalg.norm(Pj[3:])
    return np.concatenate([Pi, Pj, rand_pose(rng, 0.05), [rng.uniform(0.1, 0.5)], rng.uniform(-0.5, 0.5, 2), [1.0],
                           rng.uniform(-0.5, 0.5, 2), [1.0]])


def _line_draw(rng):
    from test_oracle_factors import _line_setup
    pose, ex, orth = _line_setup(rng)
    return np.concatenate([pose, ex, orth])


def _camera(x):
    """Rwc, twc (float64) of params x [>= 14] = pose | ex"""
    Rwb, Rbc = sr.quat_R(x[3:7]), sr.quat_R(x[10:14])
    return Rwb @ Rbc, Rwb @ x[7:10] + x[0:3]


def _orth_of(p1w, dw):
    dw = dw / np.linalg.norm(dw)
    return plk_to_orth(np.concatenate([np.cross(p1w, dw), dw]), np.float64)


def _line_in_camera(x, p1c, dc):
    """x with its line replaced by the one through p1c along dc, both in the camera frame of x"""
    Rwc, twc = _camera(x)
    x = x.copy()
    x[14:18] = _orth_of(Rwc @ np.asarray(p1c, float) + twc, Rwc @ np.asarray(dc, float))
    return x


_DIRS = np.array([[1.0, 0.5], [-1.0, 0.5], [0.5, -1.0], [0.0, 1.0]])      # (u, u / 2) and three more directions off the axis


def _proj_cases(out):
    rng = np.random.default_rng(2101)
    out["p_generic"] = ("proj", np.stack([_proj_draw(rng) for _ in range(NGEN)]))

    def edge(name, edit):
        X = np.stack([_proj_draw(rng) for _ in range(NEDGE)])
        for k, x in enumerate(X):
            edit(x, k)
        out[name] = ("proj", X)

    def put(sl, val):
        def e(x, k):
            x[sl] = val
        return e

    edge("p_j_axis", put(slice(25, 27), 0.0))
    for u in (1e-3, 1e-6, 1e-8, 1e-12):
        def e(x, k, u=u):
            x[25:27] = u * _DIRS[k]
        edge("p_j_off_%g" % u, e)
    edge("p_i_axis", put(slice(22, 24), 0.0))
    edge("p_invd_1e-4", put(21, 1e-4))
    edge("p_invd_10", put(21, 10.0))

    def same(x, k):
        x[7:14] = x[0:7]
    edge("p_same_pose", same)

    def baseline(x, k):
        d = rng.normal(size=3)
        x[7:10] = x[0:3] + 1e-6 * d / np.linalg.norm(d)
    edge("p_baseline_1e-6", baseline)

    def behind(x, k):       # camera j turned by pi about its y axis: Qj = Qi * (w = 0, y = 1)
        qx, qy, qz, qw = x[3:7]
        x[10:14] = [-qz, qw, qx, -qy]
    edge("p_behind", behind)
    for name, sl in (("i", slice(3, 7)), ("j", slice(10, 14)), ("ic", slice(17, 21))):
        def neg(x, k, sl=sl):
            x[sl] = -x[sl]
        edge("p_neg_q%s" % name, neg)

    def nonunit(x, k):
        s = 7 * (k % 3) + 3
        x[s:s + 4] *= 1.0 + 1e-6
    edge("p_q_norm_1+1e-6", nonunit)

    def plused(x, k):
        for s in (0, 7, 14):
            x[s:s + 7] = pose_plus(x[s:s + 7], 0.05 * rng.normal(size=6), np.float64)[0]
    edge("p_q_after_plus", plused)
    edge("p_ex_identity", put(slice(14, 21), [0, 0, 0, 0, 0, 0, 1.0]))

    def far(x, k):         # the observation 50 / sqrt_info off the projection: a residual of 50 px
        x[25:27] = 0.0
        p = np.asarray(x, LD)
        pcj = qrot(qinv(_q(p[14:21], LD)), qrot(qinv(_q(p[7:14], LD)), qrot(_q(p[0:7], LD), qrot(_q(p[14:21], LD), p[22:25] / p[21]) + p[14:17])
                                                  + p[0:3] - p[7:10]) - p[14:17])
        x[25:27] = np.asarray(pcj[:2] / pcj[2], np.float64) + (50.0 / SQRT_INFO["proj"]) * _DIRS[k] / np.linalg.norm(_DIRS[k])
    edge("p_res_50px", far)


def _line_cases(out):
    rng = np.random.default_rng(2102)
    draw = lambda: np.concatenate([_line_draw(rng), rng.uniform(-0.5, 0.5, 4)])
    out["l_generic"] = ("line", np.stack([draw() for _ in range(NGEN)]))

    def edge(name, edit):
        X = np.stack([draw() for _ in range(NEDGE)])
        for k in range(NEDGE):
            X[k] = edit(X[k], k)
        out[name] = ("line", X)

    pts = np.array([[0.02, 0.03, 0.035], [-0.03, 0.01, 0.04], [0.0, 0.0, 0.05], [0.04, -0.02, 0.02]])
    edge("l_near_0.05", lambda x, k: _line_in_camera(x, pts[k], rng.normal(size=3)))
    edge("l_far_100", lambda x, k: _line_in_camera(x, 2000 * pts[k] + [0, 0, 30], rng.normal(size=3)))
    edge("l_dir_axis", lambda x, k: _line_in_camera(x, [0.3, 0.2, 3.0], [1e-6 * _DIRS[k, 0], 1e-6 * _DIRS[k, 1], 1.0]))

    def image_inf(x, k):     # nc ~ (1e-6 c, 1e-6 s, 1): the plane of the line and the camera centre is the image plane's parallel
        c, s = _DIRS[k] / np.linalg.norm(_DIRS[k])
        p1, p2 = np.array([1.0, 0.5, 0.0]), np.array([-0.5, 1.0, 0.0])
        p1[2], p2[2] = -1e-6 * (c * p1[0] + s * p1[1]), -1e-6 * (c * p2[0] + s * p2[1])
        return _line_in_camera(x, p1, p2 - p1)
    edge("l_image_inf", image_inf)

    def origin(dist):
        def e(x, k):
            x = x.copy()
            d = rng.normal(size=3)
            p = np.cross(d, rng.normal(size=3))
            p *= dist / np.linalg.norm(p)
            if dist > 10:      # the camera a few metres from the line
                x[0:3] += p
            x[14:18] = _orth_of(p, d)
            return x
        return e
    edge("l_origin_1e-3", origin(1e-3))
    edge("l_origin_1e3", origin(1e3))
    for name, sign in (("+", 1.0), ("-", -1.0)):
        def gimbal(x, k, sign=sign):
            x = x.copy()
            x[15] = sign * (np.pi / 2 - 1e-8 * (k + 1) / NEDGE)
            return x
        edge("l_orth1_%spi/2" % name, gimbal)

    def equal(x, k):
        x = x.copy()
        x[20:22] = x[18:20]
        return x
    edge("l_obs_equal", equal)

    def on_line(x, k):
        x = x.copy()
        nc = _line_chain(np.asarray(x, LD), LD)[6][:3]
        for s in (18, 20):
            if abs(nc[1]) > abs(nc[0]):
                x[s + 1] = float(-(nc[2] + nc[0] * LD(x[s])) / nc[1])
            else:
                x[s] = float(-(nc[2] + nc[1] * LD(x[s + 1])) / nc[0])
        return x
    edge("l_obs_on_line", on_line)


def _vp_cases(out):
    rng = np.random.default_rng(2103)

    def draw():
        vp_ = rng.normal(size=3)
        vp_[2] = abs(vp_[2]) + 0.5
        return np.concatenate([_line_draw(rng), vp_])
    out["v_generic"] = ("vp", np.stack([draw() for _ in range(16)]))

    def edge(name, edit):
        X = np.stack([draw() for _ in range(NEDGE)])
        for k in range(NEDGE):
            X[k] = edit(X[k], k)
        out[name] = ("vp", X)

    def dz(z):
        def e(x, k):
            c, s = _DIRS[k] / np.linalg.norm(_DIRS[k])
            return _line_in_camera(x, [0.3, -0.2, 4.0], [c, s, z])
        return e
    edge("v_dz_1e-3", dz(1e-3))

    def vp2(x, k):
        x = x.copy()
        x[20] = 1e-3
        return x
    edge("v_vp2_1e-3", vp2)

    def parallel(x, k):
        x = x.copy()
        d_c = _line_chain(np.asarray(x, LD), LD)[6][3:]
        x[18:21] = np.asarray(d_c * LD(1.5 + k), np.float64)
        return x
    edge("v_parallel", parallel)
    edge("v_dz_neg", dz(-1.0))


def _plus_cases(out):
    from test_oracle_factors import rand_pose
    rng = np.random.default_rng(2104)
    pdraw = lambda: np.concatenate([rand_pose(rng), 0.1 * rng.normal(size=6)])
    out["pp_generic"] = ("pose_plus", np.stack([pdraw() for _ in range(16)]))

    def pedge(name, edit):
        X = np.stack([pdraw() for _ in range(NEDGE)])
        for k, x in enumerate(X):
            edit(x, k)
        out[name] = ("pose_plus", X)

    def zero(x, k):
        x[7:13] = 0.0
    pedge("pp_delta_0", zero)
    for name, ang in (("1e-9", 1e-9), ("3", 3.0)):
        def rot(x, k, ang=ang):
            x[10:13] *= ang / np.linalg.norm(x[10:13])
        pedge("pp_rot_%s" % name, rot)

    def wneg(x, k):
        if x[6] > 0:
            x[3:7] = -x[3:7]
    pedge("pp_w_neg", wneg)

    odraw = lambda: np.concatenate([_line_draw(rng)[14:18], 0.1 * rng.normal(size=4)])
    out["op_generic"] = ("orth_plus", np.stack([odraw() for _ in range(16)]))

    def oedge(name, edit, n=NEDGE):
        X = np.stack([odraw() for _ in range(n)])
        for k, x in enumerate(X):
            edit(x, k)
        out[name] = ("orth_plus", X)

    def ozero(x, k):
        x[4:8] = 0.0
    oedge("op_delta_0", ozero)
    for name, sign in (("+", 1.0), ("-", -1.0)):
        def gimbal(x, k, sign=sign):      # theta_1 1e-8 short of +-pi/2, the step's rotation about the local y axis 2e-8 and more
            x[1] = sign * (np.pi / 2 - 1e-8)
            x[4:8] *= 1e-7
            x[5] = -sign * 2e-8 * (k + 1)
        oedge("op_x1_%spi/2_across" % name, gimbal)

    for gap in (1e-9, 1e-8, 1e-7, 1e-6):      # one case per gap: asin(W10) loses sqrt(eps) / gap of the digits of cos(phi)
        def phi(x, k, gap=gap):               # phi + dphi = pi/2 - gap in the first two factors, pi/2 + gap (across) in the others
            x[3] = np.pi / 2 - 1e-3
            x[7] = 1e-3 - (gap if k < 2 else -gap)
        oedge("op_phi_pi/2_%g" % gap, phi)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (kind, X [n, nin]): float64 inputs, one factor per row (parameters | observations or delta).  The plk_to_orth and
    orth_to_plk cases are the lines of the line cases"""
    out = {}
    _proj_cases(out)
    _line_cases(out)
    _vp_cases(out)
    _plus_cases(out)
    for name in ("l_generic", "l_origin_1e-3", "l_origin_1e3", "l_orth1_+pi/2", "l_orth1_-pi/2"):
        orth = out[name][1][:16, 14:18]
        out["o2p_" + name[2:]] = ("orth_to_plk", orth)
        out["p2o_" + name[2:]] = ("plk_to_orth", np.stack([orth_to_plk(a, np.float64) for a in orth]))
    return out


GENERIC = ("p_generic", "l_generic", "v_generic", "pp_generic", "op_generic", "o2p_generic", "p2o_generic")


def by_kind(kind):
    """the cases of one evaluator concatenated: X [N, nin], [(name, first row, rows)]"""
    names = [n for n, (k, _) in cases().items() if k == kind]
    where, m0 = [], 0
    for n in names:
        m = len(cases()[n][1])
        where.append((n, m0, m))
        m0 += m
    return np.concatenate([cases()[n][1] for n in names]), where


@functools.lru_cache(maxsize=None)
def evaluated(name):
    """(kind, X, ref, unit, out64, rho64 [n, m]) of a case: the long-double run, its units, the float64 run and its rho"""
    kind, X = cases()[name]
    ref, unit = units(kind, X)
    out64 = run(kind, X, np.float64)
    return kind, X, ref, unit, out64, rho_rows(kind, out64, ref, unit)


def split(kind, rho):
    """worst rho of the residual and of the Jacobian entries of a factor evaluator; of the output of the others"""
    if kind in ("proj", "line", "vp"):
        return dict(r=float(rho[:, :2].max()), J=float(rho[:, 2:].max()))
    return dict(out=float(rho.max()))


LOSS_CASES = {
    "huber": [1.0 - 1e-12, 1.0 + 1e-12, 0.0, 1e6],       # s in units of delta^2
    "cauchy": [0.0, 1e-20, 1e12],
}


def loss_rows(dt=LD, delta=None):
    """[(loss, s, rho, scale)] over LOSS_CASES in dtype dt"""
    delta = v.default_options().huber_delta if delta is None else delta
    out = [("huber", k * delta * delta) + huber(k * delta * delta, delta, dt) for k in LOSS_CASES["huber"]]
    return out + [("cauchy", s) + cauchy(s, 1.0, dt) for s in LOSS_CASES["cauchy"]]


def loss_yardstick():
    """worst rho of (rho, scale) of the float64 losses; unit eps64 |f| + |f(s + spacing(s)) - f(s)|"""
    delta = v.default_options().huber_delta
    worst = dict(huber=0.0, cauchy=0.0)
    for (name, s, rho, sc), (_, _, rho64, sc64) in zip(loss_rows(LD), loss_rows(np.float64)):
        f = (lambda t: huber(t, delta)) if name == "huber" else (lambda t: cauchy(t, 1.0))
        rp, sp = f(s + np.spacing(s)) if s != 0 else (rho, sc)
        for a, b, c in ((rho, rho64, rp), (sc, sc64, sp)):
            unit = EPS64 * abs(a) + abs(c - a)
            err = abs(LD(b) - a)
            worst[name] = max(worst[name], float(err / unit) if unit > 0 else (0.0 if err == 0 else np.inf))
    return worst


# ---- a window's linearisation with long-double visual rows ------------------------------------------------------------------
class Evaluators:
    """what step_ref.Problem(evaluators=...) calls for the point, line and VP rows: this module in long double"""
    projection_factor = staticmethod(lambda params, pts, sqrt_info: projection(params, pts, sqrt_info))
    line_factor = staticmethod(lambda params, obs, sqrt_info: line(params, obs, sqrt_info))
    vp_factor = staticmethod(lambda params, vp_obs, sqrt_info: vp(params, vp_obs, sqrt_info))


class Evaluators64(Evaluators):
    """the same in float64: the restatement the window yardstick assembles"""
    projection_factor = staticmethod(lambda params, pts, sqrt_info: projection(params, pts, sqrt_info, dt=np.float64))
    line_factor = staticmethod(lambda params, obs, sqrt_info: line(params, obs, sqrt_info, dt=np.float64))
    vp_factor = staticmethod(lambda params, vp_obs, sqrt_info: vp(params, vp_obs, sqrt_info, dt=np.float64))


WINDOW_CASES = ("c", "d", "e", "c_edge")
EDGE = dict(axis=0, off=1, invd=2, huber=3)      # c_edge: which of c's five points carries which edit


def c_edge(w):
    """a copy of step_ref's case c (5 points of 6 observations, 1 line with VP) in which point 0's second observation is exactly on
    the optical axis, point 1's 1e-8 off it, point 2's inverse depth is 1e-3 and point 3's second observation is displaced by
    0.05 (15 px: Huber's linear branch)"""
    w = w.copy()
    off = np.concatenate([[0], np.cumsum(w.point_nobs)]).astype(int)
    w.point_obs[off[EDGE["axis"]] + 1, 0:2] = 0.0
    w.point_obs[off[EDGE["off"]] + 1, 0:2] = [1e-8, 0.5e-8]
    w.inv_depth[EDGE["invd"]] = 1e-3
    w.point_obs[off[EDGE["huber"]] + 1, 0] += 0.05
    return w


@functools.lru_cache(maxsize=None)
def window_cases():
    """id -> (Window, options): step_ref's c, d, e and c_edge"""
    sc = sr.cases()
    out = {k: sc[k] for k in ("c", "d", "e")}
    out["c_edge"] = (c_edge(sc["c"][0]), sc["c"][1])
    return out


def problem(case, evaluators=Evaluators):
    w, opt = window_cases()[case]
    return sr.Problem(w, opt, evaluators=evaluators)


def reference(case, orth=None, invd=None):
    """(Problem, x, Lin) of a window case linearised with the long-double factors at the window's initial state, the line
    parameters replaced by `orth` (the device's read-out) and the inverse depths by `invd` (the uploaded ones) when given"""
    prob = problem(case)
    x = prob.initial_state()
    if orth is not None:
        x = dict(x, orth=np.array(orth, np.float64))
    if invd is not None:
        x = dict(x, invd=np.array(invd, np.float64))
    return prob, x, prob.linearize(x)


def bar_window(case, what):
    """as step_ref.bar: for H and g of c, d, e the worst yardstick of the three (a window's entries collect the rounding of its
    factors in the order the tickets fall); c_edge, whose near-axis observation sets a yardstick four orders above theirs, has
    its own; the costs each their own"""
    y = YARDSTICK_WINDOW[case][what]
    if what in ("H", "g") and case in ("c", "d", "e"):
        y = max(YARDSTICK_WINDOW[c][what] for c in ("c", "d", "e"))
    return MARGIN * max(y, 1.0)


def window_yardstick(case, seed):
    """as step_ref.yardstick: H, g, cost assembled in float64 (this module's float64 factors) in a shuffled order of the residual
    blocks at states one ulp away, against the long-double-factor linearisation"""
    prob, x, lin = reference(case)
    rng = np.random.default_rng(seed)
    H, g, c = problem(case, Evaluators64).assemble64(sr.perturbed(x, rng), order=lambda m: rng.permutation(m))
    return dict(H=sr.rho(H, lin.H, lin.unit_H), g=sr.rho(g, lin.g, lin.unit_g), cost=float(abs(LD(c) - lin.cost)) / lin.unit_cost)


# ---- k_line_opt's first evaluation: sum 1/2 log(1 + s) over the line factors of the triangulated lines -----------------------
def line_opt_rows(w, opt, pose=None, ex=None, plk=None):
    """(params [m, 18], obs [m, 4]) of the line factors onlyLineOpt adds: every observation of every triangulated line, at the
    world orth of the window's camera-frame Pluecker line (float64 states, as the window is uploaded)"""
    pose = w.pose if pose is None else pose
    ex = w.ex_pose if ex is None else ex
    plk = w.line_plk if plk is None else plk
    pose, ex = np.array(pose), np.array(ex)
    for q in list(pose[:, 3:]) + [ex[3:]]:        # vector2double: the quaternion of the normalised quaternion's matrix
        q[:] = sr.R_quat(sr.quat_R(q / np.linalg.norm(q)))
    loff =np.concatenate([[0], np.cumsum(w.line_nobs)]).astype(int)
    P, O = [], []
    ric, tic = sr.quat_R(ex[3:] / np.linalg.norm(ex[3:])), ex[:3]
    for l in np.nonzero(np.asarray(w.line_triangulated[:len(w.line_start)]) != 0)[0]:
        s = int(w.line_start[l])
        Rs = sr.quat_R(pose[s, 3:] / np.linalg.norm(pose[s, 3:]))
        orth = plk_to_orth(sr.plk_to_pose(plk[l], Rs @ ric, pose[s, :3] + Rs @ tic), np.float64)
        ob = w.line_obs[loff[l]:loff[l + 1]]
        for k in range(len(ob)):
            P.append(np.concatenate([pose[s + k], ex, orth]))
            O.append(ob[k, 0:4])
    return np.array(P), np.array(O)


def line_opt_cost(P, O, sqrt_info, dt=LD):
    """sum over the factors of rho / 2, rho = CauchyLoss(1)(|r|^2), in dtype dt, the factors in the given order"""
    r, _ = line(P, O, sqrt_info, want_jac=False, dt=dt)
    total = dt(0)
    for ri in r:
        total = total + cauchy(ri @ ri, 1.0, dt)[0] / 2
    return total


def line_opt_yardstick(seed):
    """rho_ref of case e's first onlyLineOpt cost, unit eps64 x cost: float64 factors in a shuffled order, states and lines one
    ulp away"""
    w, opt = window_cases()["e"]
    P, O = line_opt_rows(w, opt)
    ref = line_opt_cost(P, O, opt.line_factor)
    rng = np.random.default_rng(seed)
    x = sr.perturbed(dict(pose=w.pose, ex=w.ex_pose, plk=w.line_plk), rng)
    P2, O2 = line_opt_rows(w, opt, x["pose"], x["ex"], x["plk"])
    order = rng.permutation(len(P2))
    c64 = line_opt_cost(P2[order], O2[order], opt.line_factor, np.float64)
    return dict(cost=float(abs(LD(c64) - ref) / (EPS64 * ref)))


# Yardsticks of this module's float64 run against its long-double run on the CPU, in the units above (`python tests/vis_ref.py`
# prints these tables).  Factor evaluators: worst rho of the residual and of the Jacobian over the factors of the case; the
# parameterisations and conversions: of the output (orth_plus, plk_to_orth as normalised Pluecker vectors).
YARDSTICK = {
    "p_generic": dict(r=0.515, J=1.73),
    "p_j_axis": dict(r=0.391, J=0.461),
    "p_j_off_0.001": dict(r=44.9, J=64.4),
    "p_j_off_1e-06": dict(r=9.33e+04, J=2.1e+05),
    "p_j_off_1e-08": dict(r=2.86e+06, J=8.17e+06),
    "p_j_off_1e-12": dict(r=0.586, J=0.739),
    "p_i_axis": dict(r=0.438, J=1),
    "p_invd_1e-4": dict(r=0.269, J=0.524),
    "p_invd_10": dict(r=2.33, J=0.852),
    "p_same_pose": dict(r=0.424, J=0.89),
    "p_baseline_1e-6": dict(r=0.445, J=1.09),
    "p_behind": dict(r=0.768, J=1.55),
    "p_neg_qi": dict(r=0.644, J=0.887),
    "p_neg_qj": dict(r=0.243, J=0.501),
    "p_neg_qic": dict(r=0.579, J=0.677),
    "p_q_norm_1+1e-6": dict(r=0.275, J=0.887),
    "p_q_after_plus": dict(r=0.341, J=0.512),
    "p_ex_identity": dict(r=0.71, J=0.917),
    "p_res_50px": dict(r=0.272, J=1.11),
    "l_generic": dict(r=0.403, J=2.47),
    "l_near_0.05": dict(r=0.363, J=0.55),
    "l_far_100": dict(r=0.275, J=2.43),
    "l_dir_axis": dict(r=0.526, J=0.604),
    "l_image_inf": dict(r=0.149, J=5.41),
    "l_origin_1e-3": dict(r=0.0905, J=1.74),
    "l_origin_1e3": dict(r=0.76, J=1.28),
    "l_orth1_+pi/2": dict(r=0.209, J=0.839),
    "l_orth1_-pi/2": dict(r=0.16, J=1.1),
    "l_obs_equal": dict(r=0.134, J=0.552),
    "l_obs_on_line": dict(r=0.16, J=1.38),
    "v_generic": dict(r=0.236, J=0.471),
    "v_dz_1e-3": dict(r=0.0766, J=0.249),
    "v_vp2_1e-3": dict(r=0.187, J=0.342),
    "v_parallel": dict(r=0.183, J=0.293),
    "v_dz_neg": dict(r=0.154, J=0.377),
    "pp_generic": dict(out=0.5),
    "pp_delta_0": dict(out=0.388),
    "pp_rot_1e-9": dict(out=0.252),
    "pp_rot_3": dict(out=0.3),
    "pp_w_neg": dict(out=0.609),
    "op_generic": dict(out=0.789),
    "op_delta_0": dict(out=0),
    "op_x1_+pi/2_across": dict(out=1.62e+10),
    "op_x1_-pi/2_across": dict(out=8.62e+09),
    "op_phi_pi/2_1e-09": dict(out=3.88e+15),
    "op_phi_pi/2_1e-08": dict(out=2.81e+15),
    "op_phi_pi/2_1e-07": dict(out=74),
    "op_phi_pi/2_1e-06": dict(out=1.23e+03),
    "o2p_generic": dict(out=0.495),
    "p2o_generic": dict(out=0.692),
    "o2p_origin_1e-3": dict(out=0.291),
    "p2o_origin_1e-3": dict(out=1.02e+03),
    "o2p_origin_1e3": dict(out=0.407),
    "p2o_origin_1e3": dict(out=0.302),
    "o2p_orth1_+pi/2": dict(out=0.213),
    "p2o_orth1_+pi/2": dict(out=4.33e+15),
    "o2p_orth1_-pi/2": dict(out=0.219),
    "p2o_orth1_-pi/2": dict(out=3.72e+15),
    "loss": dict(huber=0.249, cauchy=0.147),
}
# A window's H, g and cost (step_ref's units) by the float64 factors in a shuffled order at states one ulp away against the
# long-double-factor linearisation, seeds 3000 + position; c_edge_step: the cost at the candidate of c_edge's first step;
# line_opt: case e's first onlyLineOpt cost in eps64 x cost
YARDSTICK_WINDOW = {
    "c": dict(H=1.08e+03, g=326, cost=19.3),
    "d": dict(H=1.41e+03, g=3.95e+03, cost=26.1),
    "e": dict(H=8.31e+03, g=803, cost=49.1),
    "c_edge": dict(H=2.05e+07, g=2.28e+05, cost=2.3e+03),
    "c_edge_step": dict(cost=2.75e+06),
    "line_opt": dict(cost=4.21),
}


def bar(case, what):
    """what a ratio of the oracle or the device may reach on a case: MARGIN * max(the case's yardstick, 1)"""
    y = YARDSTICK[case][what] if case in YARDSTICK else YARDSTICK_WINDOW[case][what]
    return MARGIN * max(y, 1.0)


@functools.lru_cache(maxsize=None)
def candidate(case):
    """(Problem, x_c, Lin at x_c) at x0 [+] delta of the reference's first step on the long-double-factor linearisation"""
    prob, x0, lin = reference(case)
    xc = prob.plus(x0, sr.step(lin.H, lin.g, lin.J)["delta"])
    return prob, xc, prob.linearize(xc)


def measure():
    out = {name: split(evaluated(name)[0], evaluated(name)[5]) for name in cases()}
    out["loss"] = loss_yardstick()
    return out


def measure_window():
    out = {case: window_yardstick(case, 3000 + k) for k, case in enumerate(WINDOW_CASES)}
    prob, xc, lin = candidate("c_edge")
    rng = np.random.default_rng(3000 + len(out))
    _, _, c = problem("c_edge", Evaluators64).assemble64(sr.perturbed(xc, rng), order=lambda m: rng.permutation(m))
    out["c_edge_step"] = dict(cost=float(abs(LD(c) - lin.cost)) / lin.unit_cost)
    out["line_opt"] = line_opt_yardstick(3000 + len(out))
    return out


def _fmt(d):
    return "dict(%s)" % ", ".join("%s=%.3g" % kv for kv in d.items())


if __name__ == "__main__":
    for name, y in measure().items():
        print('    "%s": %s,' % (name, _fmt(y)))
    print()
    for name, y in measure_window().items():
        print('    "%s": %s,' % (name, _fmt(y)))
