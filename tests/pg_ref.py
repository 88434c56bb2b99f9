"""Sequential NumPy restatement of PoseGraph::optimize4DoF (pose_graph.cpp:403-579, functors pose_graph.h:89-250) for one live
sequence, as vpl_pg_optimize_batch runs it: ceres' trust-region loop with the Levenberg-Marquardt strategy and Jacobi scaling
(the rules of oracle/problem.cpp, SolveWith<LevenbergMarquardt>), analytic Jacobians, the Huber corrector as a plain scaling.

Generic in the dtype (np.float64, np.longdouble), with its own Cholesky.  solver="dense" factors the whole normal matrix;
solver="banded" uses the algebra of the device: H = B + U^T U, B = L L^T banded, Y = L^-1 [g, U^T], S = I + Yu^T Yu,
w = S^-1 Yu^T y_g, step = -L^-T (y_g - Yu w).

optimize() also records every (value, threshold) pair that decided something (`decisions`), every rho (`rhos`) and the verdict of
every iteration (`verdicts`), and the first linear system's g, step and model cost change (`first`)."""
import numpy as np

NO_CONVERGENCE, CONVERGENCE, FAILURE = 0, 1, 2
OK, UNSUPPORTED = 0, 1
BW = 4


def default_options():
    return dict(max_iterations=5, max_consecutive_invalid_steps=5, huber_delta=0.1, loop_yaw_scale=10.0, initial_radius=1e4,
                max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3, function_tolerance=1e-6, gradient_tolerance=1e-10,
                parameter_tolerance=1e-8, min_lm_diagonal=1e-6, max_lm_diagonal=1e32)


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


def R2ypr(R):
    dt = R.dtype.type
    pi = dt(np.pi)
    n, o, a = R[:, 0], R[:, 1], R[:, 2]
    y = np.arctan2(n[1], n[0])
    p = np.arctan2(-n[2], n[0] * np.cos(y) + n[1] * np.sin(y))
    r = np.arctan2(a[0] * np.sin(y) - a[1] * np.cos(y), -o[0] * np.sin(y) + o[1] * np.cos(y))
    return np.array([y / pi * dt(180), p / pi * dt(180), r / pi * dt(180)], dtype=dt)


def ypr2R(ypr):
    dt = ypr.dtype.type
    pi = dt(np.pi)
    y, p, r = (v / dt(180) * pi for v in ypr)
    z, o = dt(0), dt(1)
    Rz = np.array([[np.cos(y), -np.sin(y), z], [np.sin(y), np.cos(y), z], [z, z, o]], dtype=dt)
    Ry = np.array([[np.cos(p), z, np.sin(p)], [z, o, z], [-np.sin(p), z, np.cos(p)]], dtype=dt)
    Rx = np.array([[o, z, z], [z, np.cos(r), -np.sin(r)], [z, np.sin(r), np.cos(r)]], dtype=dt)
    return Rz.dot(Ry).dot(Rx)


def norm_angle(a):
    dt = type(a)
    if a > dt(180):
        return a - dt(360)
    if a < dt(-180):
        return a + dt(360)
    return a


# ---- the two cost functors, residual and analytic Jacobians over (yaw, tx, ty, tz) of the two ends
def edge_eval(xa, xb, pra, meas, yaw_div, jac=True, wraps=None):
    dt = xa.dtype.type
    pi = dt(np.pi)
    y, p, q = xa[0] / dt(180) * pi, pra[0] / dt(180) * pi, pra[1] / dt(180) * pi
    sy, cy, sp, cp, sr, cr = np.sin(y), np.cos(y), np.sin(p), np.cos(p), np.sin(q), np.cos(q)
    R = np.array([[cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr], [sy * cp, cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr],
                  [-sp, cp * sr, cp * cr]], dtype=dt)
    tw = xb[1:4] - xa[1:4]
    r = np.zeros(4, dtype=dt)
    r[:3] = R.T.dot(tw) - meas[:3]
    ang = xb[0] - xa[0] - meas[3]
    if wraps is not None:
        wraps.append((abs(ang), dt(180)))
    r[3] = norm_angle(ang) / yaw_div
    if not jac:
        return r, None, None
    Ja, Jb = np.zeros((4, 4), dtype=dt), np.zeros((4, 4), dtype=dt)
    k = pi / dt(180)
    for c in range(3):
        Ja[c, 0] = (-R[1, c] * tw[0] + R[0, c] * tw[1]) * k
        Ja[c, 1:4] = -R[:, c]
        Jb[c, 1:4] = R[:, c]
    Ja[3, 0] = -dt(1) / yaw_div
    Jb[3, 0] = dt(1) / yaw_div
    return r, Ja, Jb


def huber(s, delta):
    dt = type(s)
    b = delta * delta
    if s > b:
        r = np.sqrt(s)
        return dt(2) * delta * r - b, max(dt(np.finfo(np.float64).tiny), delta / r)
    return s, dt(1)


def build_edges(n, loop_local):
    edges = []
    for i in range(1, n):
        for j in range(1, BW + 1):
            if i - j >= 0:
                edges.append((i - j, i, False))
    for i in range(n):
        if loop_local[i] >= 0:
            edges.append((int(loop_local[i]), i, True))
    return edges


# ---- linear algebra of its own
def cholesky(A, band=None):
    n = len(A)
    dt = A.dtype.type
    L = np.zeros_like(A)
    for j in range(n):
        lo = 0 if band is None else max(0, j - band)
        d = A[j, j] - L[j, lo:j].dot(L[j, lo:j])
        if not (d > 0) or not np.isfinite(d):
            return None
        L[j, j] = np.sqrt(d)
        hi = n if band is None else min(n, j + band + 1)
        if hi > j + 1:
            L[j + 1:hi, j] = (A[j + 1:hi, j] - L[j + 1:hi, lo:j].dot(L[j, lo:j])) / L[j, j]
    return L


def forward(L, Bm, band=None):
    Y = np.array(Bm, copy=True)
    for i in range(len(L)):
        lo = 0 if band is None else max(0, i - band)
        Y[i] = (Y[i] - L[i, lo:i].dot(Y[lo:i])) / L[i, i]
    return Y


def backward(L, Bm, band=None):
    n = len(L)
    Y = np.array(Bm, copy=True)
    for i in range(n - 1, -1, -1):
        hi = n if band is None else min(n, i + band + 1)
        Y[i] = (Y[i] - L[i + 1:hi, i].dot(Y[i + 1:hi])) / L[i, i]
    return Y


def solve_system(m, edges, Ja, Jb, r, scale, D2, solver):
    """(Js^T Js + D2) y = Js^T r with Js = J diag(scale) -> y, or None when a factorisation fails"""
    dt = scale.dtype.type
    gs = np.zeros(m, dtype=dt)
    B = np.zeros((m, m), dtype=dt)
    rowsU = []
    for e, (a, b, loop) in enumerate(edges):
        Jrow = np.zeros((4, m), dtype=dt)
        if a >= 1:
            Jrow[:, 4 * (a - 1):4 * a] = Ja[e] * scale[4 * (a - 1):4 * a]
        Jrow[:, 4 * (b - 1):4 * b] = Jb[e] * scale[4 * (b - 1):4 * b]
        gs += Jrow.T.dot(r[e])
        if loop and solver == "banded":
            rowsU.append(Jrow)
        else:
            lo = 4 * (max(a, 1) - 1)
            B[lo:4 * b, lo:4 * b] += Jrow[:, lo:4 * b].T.dot(Jrow[:, lo:4 * b])
    B[np.arange(m), np.arange(m)] += D2
    if solver == "dense":
        L = cholesky(B)
        if L is None:
            return None
        return backward(L, forward(L, gs))
    band = 4 * BW + 3
    L = cholesky(B, band)
    if L is None:
        return None
    yg = forward(L, gs, band)
    if not rowsU:
        return backward(L, yg, band)
    U = np.concatenate(rowsU, axis=0)
    Yu = forward(L, U.T.copy(), band)
    S = np.eye(len(U), dtype=dt) + Yu.T.dot(Yu)
    LS = cholesky(S)
    if LS is None:
        return None
    w = backward(LS, forward(LS, Yu.T.dot(yg)))
    return backward(L, yg - Yu.dot(w), band)


def optimize(vio_T, vio_R, loop_local, loop_info, sequence=None, tail_T=None, tail_R=None, opt=None, dtype=np.float64, solver="banded"):
    dt = dtype
    o = dict(default_options())
    o.update(opt or {})
    n = len(vio_T)
    vio_T = np.asarray(vio_T, dtype=np.float64).reshape(n, 3).astype(dt)
    vio_R = np.asarray(vio_R, dtype=np.float64).reshape(n, 3, 3).astype(dt)
    loop_local = np.asarray(loop_local, dtype=np.int64)
    loop_info = np.asarray(loop_info, dtype=np.float64).reshape(n, 8).astype(dt)
    if sequence is not None and len(set(np.asarray(sequence).tolist())) > 1:
        return dict(status=UNSUPPORTED)
    assert all(loop_local[i] < i for i in range(n))
    P = {k: (dt(v) if isinstance(v, float) else v) for k, v in o.items()}
    Rq = [qmat(mat2q(vio_R[k])) for k in range(n)]
    eul = [R2ypr(Rq[k]) for k in range(n)]
    x = np.array([[eul[k][0], *vio_T[k]] for k in range(n)], dtype=dt)
    pr = np.array([[eul[k][1], eul[k][2]] for k in range(n)], dtype=dt)
    edges = build_edges(n, loop_local)
    meas = np.zeros((len(edges), 4), dtype=dt)
    for e, (a, b, loop) in enumerate(edges):
        if loop:
            meas[e, :3], meas[e, 3] = loop_info[b, :3], loop_info[b, 7]
        else:
            meas[e, :3] = Rq[a].T.dot(vio_T[b] - vio_T[a])
            meas[e, 3] = eul[b][0] - eul[a][0]
    m = 4 * (n - 1)
    decisions, rhos, verdicts = [], [], []
    res = dict(status=OK, termination=CONVERGENCE, iterations=0, successful_steps=0, unsuccessful_steps=0, initial_cost=dt(0), final_cost=dt(0),
               decisions=decisions, rhos=rhos, verdicts=verdicts, first=None, edges=edges)

    def evaluate(xs, jac):
        E = len(edges)
        r, Ja, Jb, cost = np.zeros((E, 4), dtype=dt), np.zeros((E, 4, 4), dtype=dt), np.zeros((E, 4, 4), dtype=dt), np.zeros(E, dtype=dt)
        for e, (a, b, loop) in enumerate(edges):
            re, ja, jb = edge_eval(xs[a], xs[b], pr[a], meas[e], P["loop_yaw_scale"] if loop else dt(1), jac, decisions)
            sq = re.dot(re)
            rho0, rho1 = sq, dt(1)
            if loop and P["huber_delta"] > 0:
                decisions.append((sq, P["huber_delta"] * P["huber_delta"]))
                rho0, rho1 = huber(sq, P["huber_delta"])
            cost[e] = dt(0.5) * rho0
            if jac:
                sc = np.sqrt(rho1)
                r[e], Ja[e], Jb[e] = re * sc, ja * sc, jb * sc
        return r, Ja, Jb, cost

    def fixed_sum(v):
        s = dt(0)
        for a in v:
            s += a
        return s

    def gather(r, Ja, Jb):
        g, cn = np.zeros(m, dtype=dt), np.zeros(m, dtype=dt)
        for e, (a, b, loop) in enumerate(edges):
            for node, J in ((a, Ja[e]), (b, Jb[e])):
                if node >= 1:
                    g[4 * (node - 1):4 * node] += J.T.dot(r[e])
                    cn[4 * (node - 1):4 * node] += (J * J).sum(axis=0)
        return g, cn

    def plus(xs, delta):
        out = xs.copy()
        for k in range(1, n):
            out[k, 0] = norm_angle(xs[k, 0] + delta[4 * (k - 1)])
            out[k, 1:] = xs[k, 1:] + delta[4 * (k - 1) + 1:4 * k]
        return out

    if n > 1:
        r, Ja, Jb, cost = evaluate(x, True)
        x_cost = fixed_sum(cost)
        res["initial_cost"] = x_cost
        g, cn = gather(r, Ja, Jb)
        scale = dt(1) / (dt(1) + np.sqrt(cn))
        x_norm = np.sqrt((x[1:] * x[1:]).sum())
        gmax = np.abs(x[1:].reshape(-1) - plus(x, -g)[1:].reshape(-1)).max()
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
            y = solve_system(m, edges, Ja, Jb, r, scale, diag / radius, solver)
            valid = y is not None
            if valid:
                delta = -y * scale
                mc = dt(0)
                for e, (a, b, loop) in enumerate(edges):
                    me = Jb[e].dot(delta[4 * (b - 1):4 * b])
                    if a >= 1:
                        me = Ja[e].dot(delta[4 * (a - 1):4 * a]) + me
                    mc += (me * (r[e] + me / dt(2))).sum()
                model = -mc
                if res["first"] is None:
                    res["first"] = dict(g=g.copy(), step=delta.copy(), model=model)
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
            cand = plus(x, delta)
            cand_cost = fixed_sum(evaluate(cand, False)[3])
            if not np.isfinite(cand).all() or not np.isfinite(cand_cost):
                cand_cost = dt(np.finfo(np.float64).max)
            d = (x[1:] - cand[1:]).reshape(-1)
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
                x_norm = np.sqrt((x[1:] * x[1:]).sum())
                r, Ja, Jb, cost = evaluate(x, True)
                g, cn = gather(r, Ja, Jb)
                gmax = np.abs(x[1:].reshape(-1) - plus(x, -g)[1:].reshape(-1)).max()
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
    res["x"] = x
    res["T"] = x[:, 1:].copy()
    res["R"] = np.array([ypr2R(np.array([x[k, 0], pr[k, 0], pr[k, 1]], dtype=dt)) for k in range(n)], dtype=dt)
    yaw_drift = R2ypr(res["R"][n - 1])[0] - R2ypr(vio_R[n - 1])[0]
    rd = ypr2R(np.array([yaw_drift, dt(0), dt(0)], dtype=dt))
    td = res["T"][n - 1] - rd.dot(vio_T[n - 1])
    res.update(yaw_drift=yaw_drift, r_drift=rd, t_drift=td)
    if tail_T is not None and len(tail_T):
        tT = np.asarray(tail_T, dtype=np.float64).reshape(-1, 3).astype(dt)
        tR = np.asarray(tail_R, dtype=np.float64).reshape(-1, 3, 3).astype(dt)
        res["tail_T"] = np.array([rd.dot(p) + td for p in tT], dtype=dt)
        res["tail_R"] = np.array([rd.dot(Rm) for Rm in tR], dtype=dt)
    return res


def solution(res):
    """the solution vector the tests compare: T, R, t_drift, r_drift, yaw_drift, final cost"""
    ld = np.longdouble
    return np.concatenate([np.asarray(res["T"], ld).ravel(), np.asarray(res["R"], ld).ravel(), np.asarray(res["t_drift"], ld).ravel(),
                           np.asarray(res["r_drift"], ld).ravel(), [ld(res["yaw_drift"])], [ld(res["final_cost"])]])
