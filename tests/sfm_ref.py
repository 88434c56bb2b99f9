"""NumPy restatement of the vision-only initial structure, the model vpl_init_structure_batch is held to: GlobalSFM::construct
(vins_estimator/src/initial/initial_sfm.cpp:117-312) and the PnP of the non-key image frames (estimator.cpp:432-501).

Written once, generic in the dtype: every function takes `dt` (np.float64 or np.longdouble) and computes in it, so that the
distance between the two runs measures what float64 rounding does to a result.  numpy.linalg does not take long double: the 4 x 4
null vector (one-sided Jacobi), the Cholesky solve and the 3 x 3 inverse are written out here.

What is decided here and on the device in the same way:
  schedule()   which track gets its position at which step of construct and from which two window frames, which tracks every
               PnP of the chain sees -- a function of WHERE observations exist only;
  lm()         ceres' trust-region minimiser with its defaults (Levenberg-Marquardt strategy, Jacobi scaling, initial radius 1e4,
               the radius rule with its growing decrease factor, min_relative_decrease 1e-3, function / gradient / parameter
               tolerances 1e-6 / 1e-10 / 1e-8, 50 iterations), on the residual of ReprojectionError3D with a quaternion under
               QuaternionParameterization; the linear solve eliminates every free point (3 x 3) into the reduced camera system.
               A step whose factorisation fails, whose model does not decrease or that is not finite ends the solve as FAILURE;
  the failure conditions: a key frame's PnP with fewer than 10 points, a non-key frame's with fewer than 6, a BA that ends
               neither in CONVERGENCE nor with final_cost < 5e-3, a FAILURE of any solve.
cv::solvePnP(ITERATIVE, useExtrinsicGuess) is lm() with the points constant and one camera free, points and observations rounded
to float as cv::Point3f / cv::Point2f do."""
import numpy as np

NF = 11
FAIL_KEY_PNP, FAIL_FRAME_PNP, FAIL_BA, FAIL_NUMERIC = 1, 2, 4, 8
NO_CONVERGENCE, CONVERGENCE, FAILURE = 0, 1, 2     # vpl_solve_report's codes
MIN_KEY_PNP, MIN_FRAME_PNP = 10, 6


def require_extended():
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended-precision type here"


# ---- the schedule ----------------------------------------------------------------------------------------------------------
def schedule(l, start, nobs):
    """-> dict: step [N] (1: frame l against 10, 2: l+1..9 against 10, 3: l against l+1..9, 4: l-1..0 against l, 5: first against
    last observation, -1: never), fa / fb [N] the two window frames in the order triangulateTwoFrames takes them, count [11] the
    points each PnP sees (-1: no PnP, or not reached), first_fail the first frame (in the order of the chain) whose count is below
    10 or -1, events: the chain in order, ("tri", f0, f1, tracks) / ("pnp", f, neighbour, tracks)"""
    start, nobs = np.asarray(start, dtype=np.int64), np.asarray(nobs, dtype=np.int64)
    N = len(start)
    state = np.zeros(N, dtype=bool)
    step, fa, fb = (-np.ones(N, dtype=np.int64) for _ in range(3))
    count = -np.ones(NF, dtype=np.int64)
    events = []
    out = dict(step=step, fa=fa, fb=fb, count=count, first_fail=-1, events=events)

    def has(f):
        return (start <= f) & (f < start + nobs)

    def tri(f0, f1, code):
        idx = np.nonzero(~state & has(f0) & has(f1))[0]
        state[idx], step[idx], fa[idx], fb[idx] = True, code, f0, f1
        events.append(("tri", f0, f1, idx))

    def pnp(f, neighbour):
        idx = np.nonzero(state & has(f))[0]
        count[f] = len(idx)
        if len(idx) < MIN_KEY_PNP:
            out["first_fail"] = f
            return False
        events.append(("pnp", f, neighbour, idx))
        return True

    for i in range(l, NF - 1):
        if i > l and not pnp(i, i - 1):
            return out
        tri(i, NF - 1, 1 if i == l else 2)
    for i in range(l + 1, NF - 1):
        tri(l, i, 3)
    for i in range(l - 1, -1, -1):
        if not pnp(i, i + 1):
            return out
        tri(i, l, 4)
    idx = np.nonzero(~state & (nobs >= 2))[0]
    state[idx], step[idx], fa[idx], fb[idx] = True, 5, start[idx], start[idx] + nobs[idx] - 1
    events.append(("last", idx))
    return out


# ---- small algebra ---------------------------------------------------------------------------------------------------------
def _a(x, dt):
    return np.array(x, dtype=dt)


def mat2q(R, dt):
    """Eigen's Quaternion(Matrix3): (w, x, y, z)"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4, dtype=dt)
    if t > 0:
        t = np.sqrt(t + dt(1))
        q[0] = dt(0.5) * t
        t = dt(0.5) / t
        q[1], q[2], q[3] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + dt(1))
        q[1 + i] = dt(0.5) * t
        t = dt(0.5) / t
        q[0] = (R[k, j] - R[j, k]) * t
        q[1 + j] = (R[j, i] + R[i, j]) * t
        q[1 + k] = (R[k, i] + R[i, k]) * t
    return q


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]], dtype=a.dtype)


def qinv(q):
    return np.array([q[0], -q[1], -q[2], -q[3]], dtype=q.dtype) / (q @ q)


def qnormalized(q):
    return q / np.sqrt(q @ q)


def qmats(q):
    """toRotationMatrix of every row of q [n, 4] (w, x, y, z), no normalisation -> [n, 3, 3]"""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3), dtype=q.dtype)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    return R


def qmat(q):
    return qmats(q[None])[0]


def qplus(q, d):
    """QuaternionParameterization::Plus"""
    nd = np.sqrt(d @ d)
    if not nd > 0:
        return q.copy()
    s = np.sin(nd) / nd
    return qmul(np.array([np.cos(nd), s * d[0], s * d[1], s * d[2]], dtype=q.dtype), q)


def null_vector4(A):
    """the right singular vector of the smallest singular value of A [m, 4]: one-sided Jacobi on the columns"""
    A = A.copy()
    dt = A.dtype.type
    V = np.eye(4, dtype=A.dtype)
    tol = dt(1e-15) if A.dtype == np.float64 else dt(8) * np.finfo(A.dtype).eps    # (the device's threshold in float64)
    for _ in range(60):
        rotated = False
        for p in range(3):
            for q in range(p + 1, 4):
                al, be, ga = A[:, p] @ A[:, p], A[:, q] @ A[:, q], A[:, p] @ A[:, q]
                if ga == 0 or abs(ga) <= tol * np.sqrt(al * be):
                    continue
                rotated = True
                zeta = (be - al) / (2 * ga)
                t = (dt(1) if zeta >= 0 else dt(-1)) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = 1 / np.sqrt(1 + t * t)
                s = c * t
                for M in (A, V):
                    a, b = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = c * a - s * b, s * a + c * b
        if not rotated:
            break
    return V[:, int(np.argmin((A * A).sum(0)))]


def triangulate(P0, P1, x0, x1):
    """GlobalSFM::triangulatePoint, P0 / P1 [3, 4]"""
    A = np.stack([x0[0] * P0[2] - P0[0], x0[1] * P0[2] - P0[1], x1[0] * P1[2] - P1[0], x1[1] * P1[2] - P1[1]])
    v = null_vector4(A)
    return v[:3] / v[3]


def chol_solve(A, b):
    """A x = b by Cholesky, None when a pivot is not positive"""
    L = A.copy()
    n = len(b)
    for j in range(n):
        d = L[j, j]
        if not (d > 0 and np.isfinite(d)):
            return None
        d = np.sqrt(d)
        L[j, j] = d
        L[j + 1:, j] /= d
        L[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    y = b.copy()
    for j in range(n):
        y[j] /= L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):
        y[j] /= L[j, j]
        y[:j] -= L[j, :j] * y[j]
    return y


def inv3_spd(V):
    """inverse of a symmetric positive definite 3 x 3, None when it is not"""
    c00 = V[1, 1] * V[2, 2] - V[1, 2] * V[1, 2]
    c01 = V[0, 2] * V[1, 2] - V[0, 1] * V[2, 2]
    c02 = V[0, 1] * V[1, 2] - V[0, 2] * V[1, 1]
    det = V[0, 0] * c00 + V[0, 1] * c01 + V[0, 2] * c02
    if not (det > 0 and V[0, 0] > 0 and np.isfinite(det)):
        return None
    c11 = V[0, 0] * V[2, 2] - V[0, 2] * V[0, 2]
    c12 = V[0, 1] * V[0, 2] - V[0, 0] * V[1, 2]
    c22 = V[0, 0] * V[1, 1] - V[0, 1] * V[0, 1]
    return np.array([[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]], dtype=V.dtype) / det


# ---- the minimiser -----------------------------------------------------------------------------------------------------------
def _evaluate(q, t, X, oc, op, uv, jac):
    """residuals [M, 2] of ReprojectionError3D (the quaternion normalised, as QuaternionRotatePoint does); with jac also the
    Jacobians in the camera's local dims (3 of the rotation: d / d delta of Plus(q, delta) at 0, then the translation) [M, 2, 6] and
    in the point [M, 2, 3]"""
    dt = q.dtype
    R = qmats(q / np.sqrt((q * q).sum(1))[:, None])
    RX = np.einsum("mij,mj->mi", R[oc], X[op])
    P = RX + t[oc]
    iz = 1 / P[:, 2]
    r = np.stack([P[:, 0] * iz - uv[:, 0], P[:, 1] * iz - uv[:, 1]], 1)
    if not jac:
        return r
    M = len(oc)
    D = np.zeros((M, 2, 3), dtype=dt)
    D[:, 0, 0], D[:, 0, 2], D[:, 1, 1], D[:, 1, 2] = iz, -P[:, 0] * iz * iz, iz, -P[:, 1] * iz * iz
    S = np.zeros((M, 3, 3), dtype=dt)    # -2 [R X]x: R(Plus(q, delta)) = (I + 2 [delta]x) R(q) to first order
    S[:, 0, 1], S[:, 0, 2], S[:, 1, 0], S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = 2 * RX[:, 2], -2 * RX[:, 1], -2 * RX[:, 2], 2 * RX[:, 0], 2 * RX[:, 1], -2 * RX[:, 0]
    Jc = np.concatenate([np.einsum("mik,mkj->mij", D, S), D], 2)
    Jp = np.einsum("mik,mkj->mij", D, R[oc])
    return r, Jc, Jp


def lm(q, t, X, oc, op, uv, free_q, free_t, free_pts, dt):
    """Minimises over the cameras' free blocks and (free_pts) every point that has an observation.  q [11, 4], t [11, 3], X [N, 3];
    observation k: camera oc[k], point op[k] (sorted by point), uv[k].  -> dict: q, t, X, iterations, successful_steps, termination,
    initial_cost, final_cost"""
    q, t, X = _a(q, dt), _a(t, dt), _a(X, dt)
    oc, op, uv = np.asarray(oc, dtype=np.int64), np.asarray(op, dtype=np.int64), _a(uv, dt)
    cidx = -np.ones((NF, 6), dtype=np.int64)
    n = 0
    for f in range(NF):
        if free_q[f]:
            cidx[f, :3] = n + np.arange(3)
            n += 3
        if free_t[f]:
            cidx[f, 3:] = n + np.arange(3)
            n += 3
    used = np.unique(op) if free_pts else np.zeros(0, dtype=np.int64)
    obs_of = {int(p): np.nonzero(op == p)[0] for p in used}
    cam_obs = [np.nonzero(oc == f)[0] for f in range(NF)]
    fq = [f for f in range(NF) if free_q[f]]
    ft = [f for f in range(NF) if free_t[f]]

    def state_norm(q_, t_, X_):
        s = dt(0)
        for f in fq:
            s += q_[f] @ q_[f]
        for f in ft:
            s += t_[f] @ t_[f]
        for p in used:
            s += X_[p] @ X_[p]
        return np.sqrt(s)

    def linearise():
        """cost, residuals, Jacobians, the gradient J^T r and the squared column norms, both in local dims and unscaled"""
        r, Jc, Jp = _evaluate(q, t, X, oc, op, uv, True)
        gc, nc = np.zeros((NF, 6), dtype=dt), np.zeros((NF, 6), dtype=dt)
        for f in range(NF):
            o = cam_obs[f]
            gc[f] = np.einsum("mia,mi->a", Jc[o], r[o])
            nc[f] = np.einsum("mia,mia->a", Jc[o], Jc[o])
        gp, npt = np.zeros_like(X), np.zeros_like(X)
        for p in used:
            o = obs_of[int(p)]
            gp[p] = np.einsum("mia,mi->a", Jp[o], r[o])
            npt[p] = np.einsum("mia,mia->a", Jp[o], Jp[o])
        gmax = dt(0)
        for f in fq:
            gmax = max(gmax, np.abs(q[f] - qplus(q[f], -gc[f, :3])).max())
        for f in ft:
            gmax = max(gmax, np.abs(t[f] - (t[f] + -gc[f, 3:])).max())
        for p in used:
            gmax = max(gmax, np.abs(X[p] - (X[p] + -gp[p])).max())
        return dict(cost=(r * r).sum() / 2, r=r, Jc=Jc, Jp=Jp, gc=gc, gp=gp, nc=nc, np=npt, gmax=gmax)

    def compute_step(L, sc, sp, dc, dp, radius):
        """the step in the scaled space: -(J'^T J' + D^2)^-1 J'^T r with D^2 = diagonal / radius; None when a factorisation fails"""
        Jc = L["Jc"] * sc[oc][:, None, :]
        Jp = L["Jp"] * sp[op][:, None, :]
        r = L["r"]
        H, g = np.zeros((n, n), dtype=dt), np.zeros(n, dtype=dt)
        for f in range(NF):
            o, cols = cam_obs[f], cidx[f]
            fr = cols >= 0
            if not len(o) or not fr.any():
                continue
            Hf = np.einsum("mia,mib->ab", Jc[o], Jc[o]) + np.diag(np.sqrt(dc[f] / radius) ** 2)
            H[np.ix_(cols[fr], cols[fr])] += Hf[np.ix_(fr, fr)]
            g[cols[fr]] += np.einsum("mia,mi->a", Jc[o], r[o])[fr]
        for f in range(NF):      # a free block no observation touches: the regularisation alone
            cols = cidx[f]
            if not len(cam_obs[f]):
                for a in range(6):
                    if cols[a] >= 0:
                        H[cols[a], cols[a]] += np.sqrt(dc[f, a] / radius) ** 2
        pts = {}
        for p in used:
            o = obs_of[int(p)]
            V = np.einsum("mia,mib->ab", Jp[o], Jp[o]) + np.diag(np.sqrt(dp[p] / radius) ** 2)
            Vi = inv3_spd(V)
            if Vi is None:
                return None
            gp = np.einsum("mia,mi->a", Jp[o], r[o])
            E = np.einsum("mia,mib->mab", Jc[o], Jp[o]).reshape(-1, 3)
            idx = cidx[oc[o]].reshape(-1)
            E, idx = E[idx >= 0], idx[idx >= 0]
            H[np.ix_(idx, idx)] -= E @ Vi @ E.T
            g[idx] -= E @ (Vi @ gp)
            pts[int(p)] = (Vi, gp, E, idx)
        y = chol_solve(H, g)
        if y is None:
            return None
        stc, stp = np.zeros((NF, 6), dtype=dt), np.zeros_like(X)
        stc[cidx >= 0] = -y[cidx[cidx >= 0]]
        for p, (Vi, gp, E, idx) in pts.items():
            stp[p] = -(Vi @ (gp - E.T @ y[idx]))
        m = np.einsum("mia,ma->mi", Jc, stc[oc]) + np.einsum("mia,ma->mi", Jp, stp[op])
        return stc, stp, -(m * (r + m / 2)).sum()

    L = linearise()
    rep = dict(iterations=0, successful_steps=0, termination=FAILURE, initial_cost=L["cost"])
    if not np.isfinite(L["cost"]) or not np.isfinite(L["gmax"]):
        rep.update(q=q, t=t, X=X, final_cost=L["cost"])
        return rep
    sc, sp = 1 / (1 + np.sqrt(L["nc"])), 1 / (1 + np.sqrt(L["np"]))
    radius, decrease, reuse, successful = dt(1e4), dt(2), False, True
    x_norm = state_norm(q, t, X)
    dc = dp = None
    it = 0
    while True:
        if it >= 50:
            rep["termination"] = NO_CONVERGENCE
            break
        if successful and L["gmax"] <= dt(1e-10):
            rep["termination"] = CONVERGENCE
            break
        if radius <= dt(1e-32):
            rep["termination"] = CONVERGENCE
            break
        it += 1
        if not reuse:
            dc = np.minimum(np.maximum(L["nc"] * sc * sc, dt(1e-6)), dt(1e32))
            dp = np.minimum(np.maximum(L["np"] * sp * sp, dt(1e-6)), dt(1e32))
        st = compute_step(L, sc, sp, dc, dp, radius)
        if st is None or not np.isfinite(st[2]) or not st[2] > 0:
            rep["termination"] = FAILURE
            it -= 1
            break
        stc, stp, model_change = st
        dcam, dpt = stc * sc, stp * sp
        q2, t2, X2 = q.copy(), t.copy(), X.copy()
        for f in fq:
            q2[f] = qplus(q[f], dcam[f, :3])
        for f in ft:
            t2[f] = t[f] + dcam[f, 3:]
        for p in used:
            X2[p] = X[p] + dpt[p]
        r2 = _evaluate(q2, t2, X2, oc, op, uv, False)
        cand = (r2 * r2).sum() / 2
        if not np.isfinite(cand):
            cand = np.finfo(np.float64).max
        step_norm = state_norm(q - q2, t - t2, X - X2)
        if not np.isfinite(step_norm):
            rep["termination"] = FAILURE
            it -= 1
            break
        # a tolerance fires before the iteration is recorded (ceres never pushes the summary of the terminating iteration)
        if step_norm <= dt(1e-8) * (x_norm + dt(1e-8)):
            rep["termination"] = CONVERGENCE
            it -= 1
            break
        change = L["cost"] - cand
        if abs(change) <= dt(1e-6) * L["cost"]:
            rep["termination"] = CONVERGENCE
            it -= 1
            break
        rho = change / model_change
        if rho > dt(1e-3):
            q, t, X = q2, t2, X2
            x_norm = state_norm(q, t, X)
            L = linearise()
            successful = True
            rep["successful_steps"] += 1
            radius = min(dt(1e16), radius / max(dt(1) / 3, 1 - (2 * rho - 1) ** 3))
            decrease, reuse = dt(2), False
        else:
            successful = False
            radius, decrease, reuse = radius / decrease, decrease * 2, True
    rep.update(iterations=it, q=q, t=t, X=X, final_cost=L["cost"])
    return rep


def to_float(x, dt):
    """what cv::Point3f / cv::Point2f keep of a double"""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(dt)


def pnp(q0, t0, X, tracks, uv, dt):
    """solvePnP with the guess (q0, t0) over the points X[tracks] seen at uv: camera slot 0 free, the points constant"""
    q, t = np.zeros((NF, 4), dtype=dt), np.zeros((NF, 3), dtype=dt)
    q[:, 0] = 1
    q[0], t[0] = q0, t0
    free = np.zeros(NF, dtype=bool)
    free[0] = True
    k = len(tracks)
    return lm(q, t, to_float(X[tracks], dt), np.zeros(k, dtype=np.int64), np.arange(k), to_float(uv, dt), free, free, False, dt)


# ---- construct and the frame PnP -------------------------------------------------------------------------------------------
def initial_structure(S, dt):
    """S: n_frames, key [11], l, relative_R [3, 3], relative_T [3], ric [3, 3], track_id / track_start / track_nobs [N], track_obs
    [sum, 2], frame_pts {image frame: (ids [k], xy [k, 2])} for the non-key frames.  -> dict of everything the device hands out,
    the stages behind a failing one zeroed, and `solves`: (iterations, successful steps, termination) of every solve in order"""
    F, l = S["n_frames"], S["l"]
    start, nobs = np.asarray(S["track_start"]), np.asarray(S["track_nobs"])
    N = len(start)
    off = np.concatenate([[0], np.cumsum(nobs)])
    obs = _a(S["track_obs"], dt).reshape(-1, 2)
    plan = schedule(l, start, nobs)
    out = dict(ok=0, fail=0, plan=plan, solves=[], pnp_iterations=-np.ones(NF, dtype=np.int64), frame_iterations=-np.ones(F, dtype=np.int64),
               chain_q=np.zeros((NF, 4), dtype=dt), chain_t=np.zeros((NF, 3), dtype=dt), points_chain=np.zeros((N, 3), dtype=dt),
               ba_q=np.zeros((NF, 4), dtype=dt), ba_t=np.zeros((NF, 3), dtype=dt), points_ba=np.zeros((N, 3), dtype=dt),
               iterations=0, successful_steps=0, termination=0, initial_cost=dt(0), final_cost=dt(0),
               Q=np.zeros((NF, 4), dtype=dt), T=np.zeros((NF, 3), dtype=dt), tracked=np.zeros(0, dtype=np.int64),
               R=np.zeros((F, 3, 3), dtype=dt), Tf=np.zeros((F, 3), dtype=dt))
    if plan["first_fail"] >= 0:
        out["fail"] = FAIL_KEY_PNP
        return out

    def ob(j, f):
        return obs[off[j] + f - start[j]]

    # ---- the chain
    cq, ct = np.zeros((NF, 4), dtype=dt), np.zeros((NF, 3), dtype=dt)
    cq[:, 0] = 1
    ql = _a([1, 0, 0, 0], dt)
    q10 = qmul(ql, mat2q(_a(S["relative_R"], dt).reshape(3, 3), dt))
    cq[l] = qnormalized(qinv(ql))
    cq[NF - 1] = qnormalized(qinv(q10))
    ct[NF - 1] = -(qmat(cq[NF - 1]) @ _a(S["relative_T"], dt))
    X = np.zeros((N, 3), dtype=dt)

    def pose(f):
        return np.concatenate([qmat(cq[f]), ct[f][:, None]], 1)

    for ev in plan["events"]:
        if ev[0] == "tri":
            _, f0, f1, idx = ev
            P0, P1 = pose(f0), pose(f1)
            for j in idx:
                X[j] = triangulate(P0, P1, ob(j, f0), ob(j, f1))
        elif ev[0] == "last":
            for j in ev[1]:
                f0, f1 = start[j], start[j] + nobs[j] - 1
                X[j] = triangulate(pose(f0), pose(f1), ob(j, f0), ob(j, f1))
        else:
            _, f, nb, idx = ev
            rep = pnp(cq[nb], ct[nb], X, idx, np.stack([ob(j, f) for j in idx]), dt)
            out["solves"].append((rep["iterations"], rep["successful_steps"], rep["termination"]))
            out["pnp_iterations"][f] = rep["iterations"]
            if rep["termination"] == FAILURE:
                out["fail"] = FAIL_NUMERIC
                return out
            cq[f], ct[f] = qnormalized(rep["q"][0]), rep["t"][0]
    if not (np.isfinite(X).all() and np.isfinite(cq).all() and np.isfinite(ct).all()):
        out["fail"] = FAIL_NUMERIC
        return out
    out.update(chain_q=cq.copy(), chain_t=ct.copy(), points_chain=X.copy())

    # ---- the full BA
    tri = np.nonzero(plan["step"] >= 0)[0]
    oc = np.concatenate([start[j] + np.arange(nobs[j]) for j in tri])
    op = np.concatenate([np.full(nobs[j], j) for j in tri])
    uv = np.concatenate([obs[off[j]:off[j + 1]] for j in tri])
    free_q, free_t = np.ones(NF, dtype=bool), np.ones(NF, dtype=bool)
    free_q[l] = free_t[l] = free_t[NF - 1] = False
    rep = lm(cq, ct, X, oc, op, uv, free_q, free_t, True, dt)
    out["solves"].append((rep["iterations"], rep["successful_steps"], rep["termination"]))
    out.update(iterations=rep["iterations"], successful_steps=rep["successful_steps"], termination=rep["termination"],
               initial_cost=rep["initial_cost"], final_cost=rep["final_cost"], ba_q=rep["q"], ba_t=rep["t"], points_ba=rep["X"])
    finite = np.isfinite(rep["q"]).all() and np.isfinite(rep["t"]).all() and np.isfinite(rep["X"]).all() and np.isfinite(rep["final_cost"])
    if rep["termination"] == FAILURE or not finite:
        out["fail"] = FAIL_NUMERIC
        return out
    if not (rep["termination"] == CONVERGENCE or rep["final_cost"] < dt(5e-3)):
        out["fail"] = FAIL_BA
        return out
    Q = np.stack([qinv(rep["q"][i]) for i in range(NF)])
    T = np.stack([-(qmat(Q[i]) @ rep["t"][i]) for i in range(NF)])
    out.update(Q=Q, T=T, tracked=tri)

    # ---- every image frame (estimator.cpp:432-501)
    ric = _a(S["ric"], dt).reshape(3, 3)
    key = list(S["key"])
    R, Tf = np.zeros((F, 3, 3), dtype=dt), np.zeros((F, 3), dtype=dt)
    pos = {int(S["track_id"][j]): j for j in tri}
    fail = 0
    for f in range(F):
        if f in key:
            i = key.index(f)
            R[f], Tf[f] = qmat(Q[i]) @ ric.T, T[i]
            continue
        i = min(i for i in range(NF) if key[i] > f)
        ids, xy = S["frame_pts"][f]
        keep = [k for k in range(len(ids)) if int(ids[k]) in pos]
        if len(keep) < MIN_FRAME_PNP:
            fail |= FAIL_FRAME_PNP
            continue
        q0 = qinv(Q[i])
        t0 = -(qmat(q0) @ T[i])
        rp = pnp(q0, t0, rep["X"], np.array([pos[int(ids[k])] for k in keep]), _a(xy, dt).reshape(-1, 2)[keep], dt)
        out["solves"].append((rp["iterations"], rp["successful_steps"], rp["termination"]))
        out["frame_iterations"][f] = rp["iterations"]
        if rp["termination"] == FAILURE or not (np.isfinite(rp["q"][0]).all() and np.isfinite(rp["t"][0]).all()):
            fail |= FAIL_NUMERIC
            continue
        Rp = qmat(qnormalized(rp["q"][0])).T
        R[f], Tf[f] = Rp @ ric.T, Rp @ -rp["t"][0]
    if fail:
        out["fail"] = fail
        return out
    out.update(ok=1, R=R, Tf=Tf)
    return out
