"""Sequential NumPy restatement of GlobalOptimization::optimize (globalOpt.cpp:101-259, functors Factors.h) for one pose chain, as
vpl_gf_optimize_batch runs it: ceres' trust-region loop with the Levenberg-Marquardt strategy and Jacobi scaling (the rules of
oracle/problem.cpp, SolveWith<LevenbergMarquardt>), the QuaternionParameterization, the Huber corrector as a plain scaling.

Generic in the dtype (np.float64, np.longdouble), with its own Cholesky.  solver="dense" factors the whole normal matrix;
solver="chain" uses the algebra of the device (csrc/gf_plan.h): every S-th node a separator, the Cholesky chains of the segments,
the Schur complement on the separators -- again a chain -- and the back-substitution of the interiors.

The local Jacobian of a quaternion block is the 6 x 4 derivative of the functor's own arithmetic (the normalisation inside
QuaternionRotatePoint included) times ceres' 4 x 3 Plus Jacobian; edge_jac_closed() is the closed form the device writes.

optimize() also records every (value, threshold) pair that decided something (`decisions`), every rho (`rhos`) and the verdict of
every iteration (`verdicts`), and the first linear system's g, step and model cost change (`first`)."""
import numpy as np

NO_CONVERGENCE, CONVERGENCE, FAILURE = 0, 1, 2
OK = 0
DEFAULT_SEGMENT = 64


def default_options():
    return dict(max_iterations=5, max_consecutive_invalid_steps=5, segment=0, reserved=0, t_var=0.1, q_var=0.01, huber_delta=1.0,
                initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3, function_tolerance=1e-6,
                gradient_tolerance=1e-10, parameter_tolerance=1e-8, min_lm_diagonal=1e-6, max_lm_diagonal=1e32)


# ---- the plan (csrc/gf_plan.h)
def plan(n, S):
    S = min(S, n + 1)
    nsep = n // S
    seps = [j * S + S - 1 for j in range(nsep)]
    segs = [(j * S, min(j * S + S - 1, n)) for j in range(nsep + 1)]
    return seps, segs


# ---- the project's small maths (csrc/vpl_math.h), in the dtype of the argument
def mat2q(m):
    m = m.reshape(9)
    dt = m.dtype.type
    t = m[0] + m[4] + m[8]
    if t > 0:
        t = np.sqrt(t + dt(1))
        w = dt(0.5) * t
        t = dt(0.5) / t
        return np.array([w, (m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t], dtype=dt)
    i = 0
    if m[4] > m[0]:
        i = 1
    if m[8] > m[4 * i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = np.sqrt(m[4 * i] - m[4 * j] - m[4 * k] + dt(1))
    q = np.zeros(4, dtype=dt)
    q[1 + i] = dt(0.5) * t
    t = dt(0.5) / t
    q[0] = (m[3 * k + j] - m[3 * j + k]) * t
    q[1 + j] = (m[3 * j + i] + m[3 * i + j]) * t
    q[1 + k] = (m[3 * k + i] + m[3 * i + k]) * t
    return q


def qmat(q):
    dt = q.dtype.type
    w, x, y, z = q
    tx, ty, tz = dt(2) * x, dt(2) * y, dt(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = dt(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], dtype=dt)


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]],
                    dtype=a.dtype)


def qconj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]], dtype=q.dtype)


def qleft(a):    # a (x) b = qleft(a) b
    w, x, y, z = a
    return np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]], dtype=a.dtype)


def qright(b):   # a (x) b = qright(b) a
    w, x, y, z = b
    return np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]], dtype=b.dtype)


def skew(v):
    z = v.dtype.type(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=v.dtype)


# ---- ceres' QuaternionParameterization on a pose p, q(w, x, y, z); the tangent is (dtheta, dt)
def plus(x, d):
    dt = x.dtype.type
    out = x.copy()
    out[:3] = x[:3] + d[3:6]
    nrm = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if nrm > 0:
        s = np.sin(nrm) / nrm
        out[3:7] = qmul(np.array([np.cos(nrm), s * d[0], s * d[1], s * d[2]], dtype=dt), x[3:7])
    return out


def plus_jacobian(q):
    w, x, y, z = q
    return np.array([[-x, -y, -z], [w, z, -y], [-z, w, x], [y, -x, w]], dtype=q.dtype)


# ---- RelativeRTError: the functor's arithmetic
def _unit_conj(qi):
    c = qconj(qi)
    s = qi.dtype.type(1) / np.sqrt(c.dot(c))
    return c, s, c * s


def _rotate_unit(u, d):
    dt = u.dtype.type
    t2, t3, t4, t5, t6, t7, t8, t9, t1 = u[0] * u[1], u[0] * u[2], u[0] * u[3], -u[1] * u[1], u[1] * u[2], u[1] * u[3], -u[2] * u[2], u[2] * u[3], -u[3] * u[3]
    return np.array([dt(2) * ((t8 + t1) * d[0] + (t6 - t4) * d[1] + (t3 + t7) * d[2]) + d[0],
                     dt(2) * ((t4 + t6) * d[0] + (t5 + t1) * d[1] + (t9 - t2) * d[2]) + d[1],
                     dt(2) * ((t7 - t3) * d[0] + (t2 + t9) * d[1] + (t5 + t8) * d[2]) + d[2]], dtype=dt)


def edge_residual(xi, xj, meas, tv, qv):
    dt = xi.dtype.type
    d = xj[:3] - xi[:3]
    c, s, u = _unit_conj(xi[3:7])
    r = np.zeros(6, dtype=dt)
    r[:3] = (_rotate_unit(u, d) - meas[:3]) / tv
    e = qmul(qconj(meas[3:7]), qmul(c, xj[3:7]))
    r[3:] = dt(2) * e[1:] / qv
    return r


def edge_jac_ambient(xi, xj, meas, tv, qv):
    """the derivative of the functor's arithmetic with respect to q_i (6 x 4), t_i (6 x 3), q_j (6 x 4), t_j (6 x 3)"""
    dt = xi.dtype.type
    two = dt(2)
    d = xj[:3] - xi[:3]
    c, s, u = _unit_conj(xi[3:7])
    u0, u1, u2, u3 = u
    d0, d1, d2 = d
    dfdu = two * np.array([[-u3 * d1 + u2 * d2, u2 * d1 + u3 * d2, -two * u2 * d0 + u1 * d1 + u0 * d2, -two * u3 * d0 - u0 * d1 + u1 * d2],
                           [u3 * d0 - u1 * d2, u2 * d0 - two * u1 * d1 - u0 * d2, u1 * d0 + u3 * d2, u0 * d0 - two * u3 * d1 + u2 * d2],
                           [-u2 * d0 + u1 * d1, u3 * d0 + u0 * d1 - two * u1 * d2, -u0 * d0 + u3 * d1 - two * u2 * d2, u1 * d0 + u2 * d1]], dtype=dt)
    dudc = s * np.eye(4, dtype=dt) - (s * s * s) * np.outer(c, c)
    flip = np.diag(np.array([1, -1, -1, -1], dtype=dt))
    Jqi, Jti, Jqj, Jtj = np.zeros((6, 4), dtype=dt), np.zeros((6, 3), dtype=dt), np.zeros((6, 4), dtype=dt), np.zeros((6, 3), dtype=dt)
    Jqi[:3] = dfdu.dot(dudc).dot(flip) / tv
    R = qmat(u)
    Jtj[:3] = R / tv
    Jti[:3] = -R / tv
    mi = qconj(meas[3:7])
    Jqj[3:] = two * qleft(mi).dot(qleft(c))[1:] / qv
    Jqi[3:] = two * qleft(mi).dot(qright(xj[3:7])).dot(flip)[1:] / qv
    return Jqi, Jti, Jqj, Jtj


def edge_jac_product(xi, xj, meas, tv, qv):
    """the local Jacobians [6][6] over (dtheta, dt) of the two ends: the ambient derivative times ceres' Plus Jacobian"""
    Jqi, Jti, Jqj, Jtj = edge_jac_ambient(xi, xj, meas, tv, qv)
    Ji = np.concatenate([Jqi.dot(plus_jacobian(xi[3:7])), Jti], axis=1)
    Jj = np.concatenate([Jqj.dot(plus_jacobian(xj[3:7])), Jtj], axis=1)
    return Ji, Jj


def edge_jac_closed(xi, xj, meas, tv, qv):
    """the closed form of the device (csrc/gf_kernels.h, gf_edge_eval)"""
    dt = xi.dtype.type
    d = xj[:3] - xi[:3]
    c, s, u = _unit_conj(xi[3:7])
    Rt = qmat(u)
    Ji, Jj = np.zeros((6, 6), dtype=dt), np.zeros((6, 6), dtype=dt)
    Ji[:3, :3] = dt(2) * Rt.dot(skew(d)) / tv
    Ji[:3, 3:] = -Rt / tv
    Jj[:3, 3:] = Rt / tv
    mi = qconj(meas[3:7])
    for col in range(3):
        e = np.zeros(4, dtype=dt)
        e[1 + col] = dt(1)
        f = qmul(mi, qmul(c, qmul(e, xj[3:7])))
        Jj[3:, col] = dt(2) * f[1:] / qv
        Ji[3:, col] = -Jj[3:, col]
    return Ji, Jj


def huber(s, delta):
    dt = type(s)
    b = delta * delta
    if s > b:
        r = np.sqrt(s)
        return dt(2) * delta * r - b, max(dt(np.finfo(np.float64).tiny), delta / r)
    return s, dt(1)


# ---- linear algebra of its own
def cholesky(A):
    n = len(A)
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j].dot(L[j, :j])
        if not (d > 0) or not np.isfinite(d):
            return None
        L[j, j] = np.sqrt(d)
        if n > j + 1:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j].dot(L[j, :j])) / L[j, j]
    return L


def forward(L, Bm):
    Y = np.array(Bm, copy=True)
    for i in range(len(L)):
        Y[i] = (Y[i] - L[i, :i].dot(Y[:i])) / L[i, i]
    return Y


def backward(L, Bm):
    n = len(L)
    Y = np.array(Bm, copy=True)
    for i in range(n - 1, -1, -1):
        Y[i] = (Y[i] - L[i + 1:, i].dot(Y[i + 1:])) / L[i, i]
    return Y


def _chain_forward(D, O, rhs, a, b, n_total, cL):
    """the chain [a, b): Ld, Lo (Lo[k] = O[k] Ld[k]^-T, also for k = b - 1 when k + 1 < n_total), y, WL; None when a pivot fails"""
    Ld, Lo, y, WL = {}, {}, {}, {}
    for k in range(a, b):
        A = D[k].copy()
        if k > a:
            A = A - Lo[k - 1].dot(Lo[k - 1].T)
        Lk = cholesky(A)
        if Lk is None:
            return None
        Ld[k] = Lk
        v = rhs[k].copy()
        if k > a:
            v = v - Lo[k - 1].dot(y[k - 1])
        y[k] = forward(Lk, v)
        if cL is not None:
            WL[k] = forward(Lk, cL if k == a else -Lo[k - 1].dot(WL[k - 1]))
        if k + 1 < n_total:
            Lo[k] = forward(Lk, O[k].T.copy()).T
    return Ld, Lo, y, WL


def _chain_backward(Ld, Lo, y, a, b, n_total, WL, xL, xs):
    for k in range(b - 1, a - 1, -1):
        v = y[k].copy()
        if WL:
            v = v - WL[k].dot(xL)
        if k + 1 < n_total:
            v = v - Lo[k].T.dot(xs[k + 1])
        xs[k] = backward(Ld[k], v)


def solve_chain(D, O, gs, S):
    """D [n] diagonal blocks (scaled, with the LM diagonal), O [n-1] blocks (k+1, k), gs [n] -> y [n][6], or None"""
    n = len(D)
    seps, segs = plan(n, S)
    parts = []
    for j, (a, b) in enumerate(segs):
        res = _chain_forward(D, O, gs, a, b, n, O[a - 1] if j > 0 and a < b else None)
        if res is None:
            return None
        parts.append(res)
    xs = {}
    if seps:
        SD, SO, sr = [], [], []
        for j, s in enumerate(seps):
            Ld0, Lo0, y0, _ = parts[j]
            Ld1, Lo1, y1, WL1 = parts[j + 1]
            a1, b1 = segs[j + 1]
            XR = Lo0[s - 1]
            A = D[s] - XR.dot(XR.T)
            r = gs[s] - XR.dot(y0[s - 1])
            for k in range(a1, b1):
                A = A - WL1[k].T.dot(WL1[k])
                r = r - WL1[k].T.dot(y1[k])
            SD.append(A)
            sr.append(r)
            if j + 1 < len(seps):
                SO.append(-Lo1[b1 - 1].dot(WL1[b1 - 1]))
        res = _chain_forward(SD, SO, sr, 0, len(seps), len(seps), None)
        if res is None:
            return None
        sx = {}
        _chain_backward(res[0], res[1], res[2], 0, len(seps), len(seps), None, None, sx)
        for j, s in enumerate(seps):
            xs[s] = sx[j]
    for j, (a, b) in enumerate(segs):
        Ld, Lo, y, WL = parts[j]
        _chain_backward(Ld, Lo, y, a, b, n, WL if j > 0 else None, xs[a - 1] if j > 0 else None, xs)
    return np.array([xs[k] for k in range(n)])


def solve_dense(D, O, gs):
    n = len(D)
    H = np.zeros((6 * n, 6 * n), dtype=gs.dtype)
    for k in range(n):
        H[6 * k:6 * k + 6, 6 * k:6 * k + 6] = D[k]
        if k + 1 < n:
            H[6 * k + 6:6 * k + 12, 6 * k:6 * k + 6] = O[k]
            H[6 * k:6 * k + 6, 6 * k + 6:6 * k + 12] = O[k].T
    L = cholesky(H)
    if L is None:
        return None
    return backward(L, forward(L, gs.reshape(-1))).reshape(n, 6)


def optimize(local, global_, gps_node=(), gps_xyz=(), gps_accuracy=(), opt=None, dtype=np.float64, solver="chain", S=None):
    dt = dtype
    o = dict(default_options())
    o.update(opt or {})
    if S is None:
        S = o["segment"] if o["segment"] else DEFAULT_SEGMENT
    local = np.asarray(local, dtype=np.float64).reshape(-1, 7).astype(dt)
    n = len(local)
    x = np.asarray(global_, dtype=np.float64).reshape(n, 7).astype(dt)
    gps_node = [int(k) for k in np.asarray(gps_node).reshape(-1)]
    gps_xyz = np.asarray(gps_xyz, dtype=np.float64).reshape(len(gps_node), 3).astype(dt)
    gps_acc = np.asarray(gps_accuracy, dtype=np.float64).reshape(len(gps_node)).astype(dt)
    fix = {k: e for e, k in enumerate(gps_node)}
    P = {k: (dt(v) if isinstance(v, float) else v) for k, v in o.items()}
    tv, qv = P["t_var"], P["q_var"]
    meas = np.zeros((max(n - 1, 0), 7), dtype=dt)
    for k in range(n - 1):
        Ri, Rj = qmat(local[k, 3:7]), qmat(local[k + 1, 3:7])
        meas[k, :3] = Ri.T.dot(local[k + 1, :3] - local[k, :3])
        meas[k, 3:] = mat2q(Ri.T.dot(Rj))
    decisions, rhos, verdicts = [], [], []
    res = dict(status=OK, termination=CONVERGENCE, iterations=0, successful_steps=0, unsuccessful_steps=0, initial_cost=dt(0), final_cost=dt(0),
               decisions=decisions, rhos=rhos, verdicts=verdicts, first=None)

    def fixed_sum(v):
        s = dt(0)
        for a in v:
            s += a
        return s

    def evaluate(xs, jac):
        """per node k: the edge k -> k+1 and the GNSS factor; costs in the order edge 0, fix 0, edge 1, fix 1, ..."""
        er, Ji, Jj = np.zeros((n, 6), dtype=dt), np.zeros((n, 6, 6), dtype=dt), np.zeros((n, 6, 6), dtype=dt)
        gr, gw, cost = np.zeros((n, 3), dtype=dt), np.zeros(n, dtype=dt), np.zeros(2 * n, dtype=dt)
        for k in range(n):
            if k + 1 < n:
                r = edge_residual(xs[k], xs[k + 1], meas[k], tv, qv)
                cost[2 * k] = dt(0.5) * r.dot(r)
                if jac:
                    er[k] = r
                    Ji[k], Jj[k] = edge_jac_product(xs[k], xs[k + 1], meas[k], tv, qv)
            if k in fix:
                e = fix[k]
                r = (xs[k, :3] - gps_xyz[e]) / gps_acc[e]
                sq = r.dot(r)
                rho0, rho1 = sq, dt(1)
                if P["huber_delta"] > 0:
                    decisions.append((sq, P["huber_delta"] * P["huber_delta"]))
                    rho0, rho1 = huber(sq, P["huber_delta"])
                cost[2 * k + 1] = dt(0.5) * rho0
                if jac:
                    sc = np.sqrt(rho1)
                    gr[k], gw[k] = r * sc, sc / gps_acc[e]
        return er, Ji, Jj, gr, gw, cost

    def assemble(lin):
        er, Ji, Jj, gr, gw, _ = lin
        D, O = np.zeros((n, 6, 6), dtype=dt), np.zeros((max(n - 1, 0), 6, 6), dtype=dt)
        g, cn = np.zeros((n, 6), dtype=dt), np.zeros((n, 6), dtype=dt)
        for k in range(n):
            for J, r in (((Jj[k - 1], er[k - 1]),) if k > 0 else ()) + (((Ji[k], er[k]),) if k + 1 < n else ()):
                D[k] += J.T.dot(J)
                g[k] += J.T.dot(r)
                cn[k] += (J * J).sum(axis=0)
            for i in range(3):
                D[k, 3 + i, 3 + i] += gw[k] * gw[k]
                g[k, 3 + i] += gw[k] * gr[k, i]
                cn[k, 3 + i] += gw[k] * gw[k]
            if k + 1 < n:
                O[k] = Jj[k].T.dot(Ji[k])
        return D, O, g, cn

    def plus_all(xs, delta):
        return np.array([plus(xs[k], delta[k]) for k in range(n)], dtype=dt)

    lin = evaluate(x, True)
    x_cost = fixed_sum(lin[5])
    res["initial_cost"] = x_cost
    D, O, g, cn = assemble(lin)
    scale = dt(1) / (dt(1) + np.sqrt(cn))
    x_norm = np.sqrt((x * x).sum())
    gmax = np.abs(x - plus_all(x, -g)).max()
    radius, decrease = P["initial_radius"], dt(2)
    iteration, last_ok, invalid = 0, True, 0
    while True:
        if last_ok:
            res["successful_steps"] += 1
        else:
            res["unsuccessful_steps"] += 1
        if iteration >= o["max_iterations"]:
            res["termination"] = NO_CONVERGENCE
            break
        if last_ok:
            decisions.append((gmax, P["gradient_tolerance"]))
            if gmax <= P["gradient_tolerance"]:
                break
        decisions.append((radius, P["min_radius"]))
        if radius <= P["min_radius"]:
            break
        iteration += 1
        diag = np.minimum(np.maximum(scale * scale * cn, P["min_lm_diagonal"]), P["max_lm_diagonal"])
        Ds = np.array([D[k] * np.outer(scale[k], scale[k]) + np.diag(diag[k] / radius) for k in range(n)], dtype=dt)
        Os = np.array([O[k] * np.outer(scale[k + 1], scale[k]) for k in range(n - 1)], dtype=dt).reshape(max(n - 1, 0), 6, 6)
        y = solve_dense(Ds, Os, g * scale) if solver == "dense" else solve_chain(Ds, Os, g * scale, S)
        valid = y is not None
        if valid:
            delta = -y * scale
            er, Ji, Jj, gr, gw, _ = lin
            mc = dt(0)
            for k in range(n):
                if k + 1 < n:
                    me = Ji[k].dot(delta[k]) + Jj[k].dot(delta[k + 1])
                    mc += (me * (er[k] + me / dt(2))).sum()
                mg = gw[k] * delta[k, 3:]
                mc += (mg * (gr[k] + mg / dt(2))).sum()
            model = -mc
            if res["first"] is None:
                res["first"] = dict(g=g.reshape(-1).copy(), step=delta.reshape(-1).copy(), model=model)
            valid = bool(model > 0)
        if not valid:
            invalid += 1
            verdicts.append("invalid")
            if invalid >= o["max_consecutive_invalid_steps"]:
                res["termination"] = FAILURE
                break
            last_ok = False
            continue
        invalid = 0
        cand = plus_all(x, delta)
        cand_cost = fixed_sum(evaluate(cand, False)[5])
        if not np.isfinite(cand).all() or not np.isfinite(cand_cost):
            cand_cost = dt(np.finfo(np.float64).max)
        d = (x - cand).reshape(-1)
        step_norm = np.sqrt(d.dot(d))
        decisions.append((step_norm, P["parameter_tolerance"] * (x_norm + P["parameter_tolerance"])))
        if step_norm <= P["parameter_tolerance"] * (x_norm + P["parameter_tolerance"]):
            verdicts.append("parameter_tolerance")
            break
        cc = x_cost - cand_cost
        decisions.append((abs(cc), P["function_tolerance"] * x_cost))
        if abs(cc) <= P["function_tolerance"] * x_cost:
            verdicts.append("function_tolerance")
            break
        rho = cc / model
        rhos.append(rho)
        decisions.append((rho, P["min_relative_decrease"]))
        if rho > P["min_relative_decrease"]:
            verdicts.append("accept")
            x, x_cost = cand, cand_cost
            x_norm = np.sqrt((x * x).sum())
            lin = evaluate(x, True)
            D, O, g, cn = assemble(lin)
            gmax = np.abs(x - plus_all(x, -g)).max()
            last_ok = True
            t = dt(2) * rho - dt(1)
            radius = min(P["max_radius"], radius / max(dt(1) / dt(3), dt(1) - t * t * t))
            decrease = dt(2)
        else:
            verdicts.append("reject")
            last_ok = False
            radius = radius / decrease
            decrease = decrease * dt(2)
    res["iterations"] = iteration
    res["final_cost"] = x_cost
    res["pose"] = x
    T = np.eye(4, dtype=dt)
    T[:3, :3] = qmat(x[n - 1, 3:7]).dot(qmat(local[n - 1, 3:7]).T)
    T[:3, 3] = x[n - 1, :3] - T[:3, :3].dot(local[n - 1, :3])
    res["wgps_T_wvio"] = T
    return res


def solution(res):
    """the solution vector the tests compare: the poses, wgps_T_wvio, the final cost"""
    ld = np.longdouble
    return np.concatenate([np.asarray(res["pose"], ld).ravel(), np.asarray(res["wgps_T_wvio"], ld).ravel(), [ld(res["final_cost"])]])


# ---- WGS84 geodetic -> ECEF -> east, north, up at an origin, in the dtype asked for
def local_cartesian(lat0, lon0, h0, lla, dtype=np.float64):
    dt = dtype
    a, f = dt(6378137), dt(1) / dt("298.257223563")
    e2 = f * (dt(2) - f)
    rad = dt(np.pi) if dt is np.float64 else np.arctan(dt(1)) * dt(4)
    rad = rad / dt(180)

    def ecef(lat, lon, h):
        sp, cp, sl, cl = np.sin(lat * rad), np.cos(lat * rad), np.sin(lon * rad), np.cos(lon * rad)
        N = a / np.sqrt(dt(1) - e2 * sp * sp)
        return np.array([(N + h) * cp * cl, (N + h) * cp * sl, (N * (dt(1) - e2) + h) * sp], dtype=dt)

    lat0, lon0, h0 = dt(lat0), dt(lon0), dt(h0)
    o0 = ecef(lat0, lon0, h0)
    sp, cp, sl, cl = np.sin(lat0 * rad), np.cos(lat0 * rad), np.sin(lon0 * rad), np.cos(lon0 * rad)
    out = []
    for row in np.asarray(lla, dtype=np.float64).reshape(-1, 3):
        dx, dy, dz = ecef(dt(row[0]), dt(row[1]), dt(row[2])) - o0
        out.append([-sl * dx + cl * dy, -sp * cl * dx - sp * sl * dy + cp * dz, cp * cl * dx + cp * sl * dy + sp * dz])
    return np.array(out, dtype=dt).reshape(-1, 3), np.array([ecef(dt(r[0]), dt(r[1]), dt(r[2])) for r in np.asarray(lla, dtype=np.float64).reshape(-1, 3)], dtype=dt).reshape(-1, 3)
