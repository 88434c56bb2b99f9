"""NumPy restatement of the relative pose, the model vpl_init_relative_pose_batch is held to: Estimator::relativePose
(vins_estimator/src/estimator.cpp:590-622) and MotionEstimator::solveRelativeRT (initial/solve_5pts.cpp:193-228), i.e.
cv::findFundamentalMat(FM_RANSAC, 0.3 / 460, 0.99) and cv::recoverPose, over a given sample table.

Written once, generic in the dtype (np.float64 or np.longdouble), as tests/sfm_ref.py is: the distance between the two runs
measures what float64 rounding does to a result.  numpy.linalg does not take long double, so the null space of the 7 x 9 system
(seven Householder reflections of its rows), the cubic, the 3 x 3 SVD and the 4 x 4 null vector (one-sided Jacobi) are written out.

ransac() is the plain sequential loop of RANSACPointSetRegistrator::run: iteration after iteration, root after root in ascending
lambda, a hypothesis wins with good > max(best, 6), a win sets niters = niters_after(good), the loop ends at the first iteration
>= niters.  Only the arithmetic in front of it is batched: the null spaces and the cubic's coefficients of a block of iterations
are computed at once, which changes no number."""
import math

import numpy as np

NF = 11
MAX_ITERS = 1000
FEW_CORRES, LOW_PARALLAX, NO_MODEL, FEW_GOOD, SUCCESS = 0, 1, 2, 3, 4
FAIL_NONE, FAIL_NUMERIC = 1, 8
THRESHOLD2 = (0.3 / 460.0) * (0.3 / 460.0)     # one float64 number for every dtype, as on the device
MAX_DEPTH = 50.0
BLOCK = 32


def niters_after(N, good):
    """cv::RANSACUpdateNumIters(0.99, (N - good) / N, 7, 1000), modules/calib3d/src/ptsetreg.cpp; cvRound: halves to even"""
    ep = min(max((N - good) / N, 0.0), 1.0)
    num = max(1.0 - 0.99, 2.2250738585072014e-308)
    denom = 1.0 - math.pow(1.0 - ep, 7)
    if denom < 2.2250738585072014e-308:
        return 0
    num, denom = math.log(num), math.log(denom)
    if denom >= 0 or -num >= MAX_ITERS * (-denom):
        return MAX_ITERS
    return int(np.rint(num / denom))


def niters_table(N):
    return np.array([niters_after(N, g) for g in range(N + 1)], dtype=np.int64)


def correspondences(start, nobs, obs, i):
    """FeatureManager::getCorresponding(i, 10) -> (tracks [N], a [N, 2] in frame i, b [N, 2] in frame 10), track-list order"""
    start, nobs = np.asarray(start, dtype=np.int64), np.asarray(nobs, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(nobs)[:-1]]) if len(nobs) else np.zeros(0, dtype=np.int64)
    idx = np.nonzero((start <= i) & (start + nobs - 1 >= NF - 1))[0]
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 2)
    return idx, obs[off[idx] + i - start[idx]], obs[off[idx] + NF - 1 - start[idx]]


# ---- the hypotheses of a minimal sample -------------------------------------------------------------------------------------
def null_spaces(P):
    """P [B, 7, 4] = (x1, y1, x2, y2) of B samples -> (f1, f2) [B, 9] each: Q e7, Q e8 with Q the product of the seven Householder
    reflections that take the rows of the 7 x 9 system onto e0 .. e6"""
    dt = P.dtype.type
    x1, y1, x2, y2 = P[:, :, 0], P[:, :, 1], P[:, :, 2], P[:, :, 3]
    a = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], axis=2)
    B = len(a)
    beta = np.zeros((B, 7), dtype=P.dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(7):
            nx = np.sqrt((a[:, k, k:] * a[:, k, k:]).sum(1))
            a[:, k, k] -= np.where(a[:, k, k] >= 0, -nx, nx)
            vv = (a[:, k, k:] * a[:, k, k:]).sum(1)
            beta[:, k] = np.where(vv > 0, dt(2) / vv, dt(0))
            for j in range(k + 1, 7):
                d = (a[:, k, k:] * a[:, j, k:]).sum(1) * beta[:, k]
                a[:, j, k:] -= d[:, None] * a[:, k, k:]
    f = np.zeros((2, B, 9), dtype=P.dtype)
    f[0, :, 7] = 1
    f[1, :, 8] = 1
    for k in range(6, -1, -1):
        for z in f:
            d = (a[:, k, k:] * z[:, k:]).sum(1) * beta[:, k]
            z[:, k:] -= d[:, None] * a[:, k, k:]
    return f[0], f[1]


def _det3(a, b, c):
    return a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) - a[:, 1] * (b[:, 0] * c[:, 2] - b[:, 2] * c[:, 0]) + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])


def pencil(f1, f2):
    """(c3, c2, c1, c0) [B] of det(F2 + lambda (F1 - F2)), by rows"""
    g, h = f1 - f2, f2
    g0, g1, g2, h0, h1, h2 = g[:, 0:3], g[:, 3:6], g[:, 6:9], h[:, 0:3], h[:, 3:6], h[:, 6:9]
    return (_det3(g0, g1, g2), _det3(g0, g1, h2) + _det3(g0, h1, g2) + _det3(h0, g1, g2),
            _det3(g0, h1, h2) + _det3(h0, g1, h2) + _det3(h0, h1, g2), _det3(h0, h1, h2))


def cubic(c3, c2, c1, c0):
    """the real roots of c3 x^3 + c2 x^2 + c1 x + c0, ascending.  A vanishing leading coefficient leaves the quadratic or the
    linear equation; three real roots come from the trigonometric form, one from Cardano's; of a repeated root (discriminant
    exactly zero) only the simple partner is a root here"""
    dt = type(c3)
    if c3 == 0:
        if c2 == 0:
            return [] if c1 == 0 else [-c0 / c1]
        disc = c1 * c1 - dt(4) * c2 * c0
        if disc < 0:
            return []
        if disc == 0:
            return [-c1 / (dt(2) * c2)]
        q = -(c1 + (dt(1) if c1 >= 0 else dt(-1)) * np.sqrt(disc)) / dt(2)
        return sorted([q / c2, c0 / q])
    a, b, c = c2 / c3, c1 / c3, c0 / c3
    Q, R = (a * a - dt(3) * b) / dt(9), (dt(2) * a * a * a - dt(9) * a * b + dt(27) * c) / dt(54)
    Q3 = Q * Q * Q
    d = Q3 - R * R
    if d > 0:
        two_pi = dt(8) * np.arctan(dt(1))
        theta = np.arccos(min(dt(1), max(dt(-1), R / np.sqrt(Q3))))
        m, sh = dt(-2) * np.sqrt(Q), a / dt(3)
        return sorted([m * np.cos(theta / dt(3)) - sh, m * np.cos((theta + two_pi) / dt(3)) - sh, m * np.cos((theta - two_pi) / dt(3)) - sh])
    e = np.cbrt(np.sqrt(-d) + abs(R))
    if R > 0:
        e = -e
    return [(e + (Q / e if e != 0 else dt(0))) - a / dt(3)]


def inlier_mask(F, pts):
    """FMEstimatorCallback::computeError against the squared threshold; F [9], pts [N, 4]"""
    x1, y1, x2, y2 = pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b, c = F[0] * x1 + F[1] * y1 + F[2], F[3] * x1 + F[4] * y1 + F[5], F[6] * x1 + F[7] * y1 + F[8]
        s2 = 1 / (a * a + b * b)
        d2 = x2 * a + y2 * b + c
        a, b, c = F[0] * x2 + F[3] * y2 + F[6], F[1] * x2 + F[4] * y2 + F[7], F[2] * x2 + F[5] * y2 + F[8]
        s1 = 1 / (a * a + b * b)
        d1 = x1 * a + y1 * b + c
        return np.fmax(d1 * d1 * s1, d2 * d2 * s2) <= pts.dtype.type(THRESHOLD2)


def ransac(pts, samples, table):
    """the sequential loop over the sample table [1000, 7] -> dict iterations (niters when the loop ended), best_iteration,
    best_root, inliers, F [9] (unit Frobenius norm) or None, mask [N], hyp [1000, 3] (-1: no such root, or not reached)"""
    N = len(pts)
    hyp = -np.ones((MAX_ITERS, 3), dtype=np.int64)
    niters, best, best_it, best_root, best_F = MAX_ITERS, 0, -1, -1, None
    it = 0
    block = None
    while it < niters:
        if it % BLOCK == 0 or block is None:
            lo = it - it % BLOCK
            f1, f2 = null_spaces(pts[samples[lo:lo + BLOCK]])
            block = (lo, f1, f2, pencil(f1, f2))
        k = it - block[0]
        f1, f2, co = block[1][k], block[2][k], block[3]
        for r, lam in enumerate(cubic(co[0][k], co[1][k], co[2][k], co[3][k])):
            F = lam * f1 + (1 - lam) * f2
            good = int(inlier_mask(F, pts).sum())
            hyp[it, r] = good
            if good > max(best, 6):
                best, best_it, best_root, best_F = good, it, r, F
                niters = int(table[good])
        it += 1
    out = dict(iterations=niters, best_iteration=best_it, best_root=best_root, inliers=0, F=None, mask=np.zeros(N, dtype=bool), hyp=hyp)
    if best_it >= 0:
        F = best_F / np.sqrt((best_F * best_F).sum())
        out.update(F=F, mask=inlier_mask(F, pts))
        out["inliers"] = int(out["mask"].sum())
    return out


# ---- recoverPose ------------------------------------------------------------------------------------------------------------
def _jacobi_tol(dtype):
    return dtype.type(1e-15) if dtype == np.float64 else dtype.type(8) * np.finfo(dtype).eps    # (the device's threshold in float64)


def decompose(F):
    """cv::decomposeEssentialMat by one-sided Jacobi on the columns of F [9] -> (R1, R2 [3, 3], t [3]): F V = B with orthogonal
    columns ordered by falling norm (ties keep the lower column first), u1 / u2 the first two normalised, u3 = u1 x u2, V's
    sign fixed to det +1; R1 = U W V^T, R2 = U W^T V^T, t = u3"""
    dt = F.dtype.type
    B, V = F.reshape(3, 3).copy(), np.eye(3, dtype=F.dtype)
    tol = _jacobi_tol(F.dtype)
    for _ in range(60):
        rotated = False
        for p in range(2):
            for q in range(p + 1, 3):
                al, be, ga = (B[:, p] * B[:, p]).sum(), (B[:, q] * B[:, q]).sum(), (B[:, p] * B[:, q]).sum()
                if ga == 0 or abs(ga) <= tol * np.sqrt(al * be):
                    continue
                rotated = True
                zeta = (be - al) / (2 * ga)
                t = (dt(1) if zeta >= 0 else dt(-1)) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = 1 / np.sqrt(1 + t * t)
                s = c * t
                for M in (B, V):
                    a, b = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = c * a - s * b, s * a + c * b
        if not rotated:
            break
    n2 = (B * B).sum(0)
    o = [0, 1, 2]
    for i, j in ((0, 1), (1, 2), (0, 1)):
        if n2[o[j]] > n2[o[i]]:
            o[i], o[j] = o[j], o[i]
    with np.errstate(divide="ignore", invalid="ignore"):
        u1, u2 = B[:, o[0]] / np.sqrt(n2[o[0]]), B[:, o[1]] / np.sqrt(n2[o[1]])
    u3 = np.cross(u1, u2)
    v1, v2, v3 = V[:, o[0]], V[:, o[1]], V[:, o[2]]
    if v1 @ np.cross(v2, v3) < 0:
        v1, v2, v3 = -v1, -v2, -v3
    a, b, d = np.outer(u1, v2), np.outer(u2, v1), np.outer(u3, v3)
    return a - b + d, b - a + d, u3


def null_vectors4(A):
    """sfm_ref.null_vector4 for every 4 x 4 matrix of A [M, 4, 4] at once: a pair that needs no rotation gets the identity"""
    A = A.copy()
    dt = A.dtype.type
    V = np.broadcast_to(np.eye(4, dtype=A.dtype), A.shape).copy()
    tol = _jacobi_tol(A.dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(60):
            rotated = False
            for p in range(3):
                for q in range(p + 1, 4):
                    al, be, ga = (A[:, :, p] * A[:, :, p]).sum(1), (A[:, :, q] * A[:, :, q]).sum(1), (A[:, :, p] * A[:, :, q]).sum(1)
                    rot = ~((ga == 0) | (np.abs(ga) <= tol * np.sqrt(al * be)))
                    if not rot.any():
                        continue
                    rotated = True
                    zeta = (be - al) / (2 * np.where(rot, ga, dt(1)))
                    t = np.where(zeta >= 0, dt(1), dt(-1)) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
                    c = 1 / np.sqrt(1 + t * t)
                    s = c * t
                    c, s = np.where(rot, c, dt(1))[:, None], np.where(rot, s, dt(0))[:, None]
                    for M in (A, V):
                        a, b = M[:, :, p].copy(), M[:, :, q].copy()
                        M[:, :, p], M[:, :, q] = np.where(rot[:, None], c * a - s * b, a), np.where(rot[:, None], s * a + c * b, b)
            if not rotated:
                break
    cm = np.argmin((A * A).sum(1), axis=1)
    return V[np.arange(len(A)), :, cm]


def in_front(R, t, pts):
    """one of recoverPose's masks: cv::triangulatePoints against [I | 0] and [R | t], z w > 0, z < 50 in the first camera,
    0 < z < 50 in the second (solve_5pts.cpp:79-88)"""
    dt = pts.dtype.type
    x1, y1, x2, y2 = pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]
    M = len(pts)
    A = np.zeros((M, 4, 4), dtype=pts.dtype)
    A[:, 0, 0], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2] = -1, x1, -1, y1
    for c in range(3):
        A[:, 2, c], A[:, 3, c] = x2 * R[2, c] - R[0, c], y2 * R[2, c] - R[1, c]
    A[:, 2, 3], A[:, 3, 3] = x2 * t[2] - t[0], y2 * t[2] - t[1]
    Q = null_vectors4(A)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = Q[:, 2] * Q[:, 3] > 0
        X, Y, Z = Q[:, 0] / Q[:, 3], Q[:, 1] / Q[:, 3], Q[:, 2] / Q[:, 3]
        m &= Z < dt(MAX_DEPTH)
        z2 = R[2, 0] * X + R[2, 1] * Y + R[2, 2] * Z + t[2]
        return m & (z2 > 0) & (z2 < dt(MAX_DEPTH))


def recover_pose(F, pts, mask):
    """-> dict R / T (Rotation = R^T, Translation = -R^T t of solveRelativeRT), good, mask [N], choice 0 .. 3"""
    R1, R2, t = decompose(F)
    masks = [np.zeros(len(pts), dtype=bool) for _ in range(4)]
    sel = np.nonzero(mask)[0]
    for k in range(4):
        R, tt = (R2 if k & 1 else R1), (t if k < 2 else -t)
        if len(sel):
            masks[k][sel] = in_front(R, tt, pts[sel])
    g = [int(m.sum()) for m in masks]
    if g[0] >= g[1] and g[0] >= g[2] and g[0] >= g[3]:
        k = 0
    elif g[1] >= g[0] and g[1] >= g[2] and g[1] >= g[3]:
        k = 1
    elif g[2] >= g[0] and g[2] >= g[1] and g[2] >= g[3]:
        k = 2
    else:
        k = 3
    R, tt = (R2 if k & 1 else R1), (t if k < 2 else -t)
    return dict(R=R.T.copy(), T=-(R.T @ tt), good=g[k], mask=masks[k], choice=k)


# ---- relativePose -----------------------------------------------------------------------------------------------------------
def relative_pose(S, samples, dt):
    """S: dict track_start / track_nobs / track_obs; samples(i, N) -> the sample table [1000, 7] of candidate i over N
    correspondences.  -> dict ok, fail, l, relative_R [3, 3], relative_T [3] and per candidate i = 0 .. 9 the arrays n_corres,
    status, iterations, best_iteration, best_root, inliers, good, choice, average_parallax, F [10, 9], R [10, 3, 3], T [10, 3],
    mask_ransac / mask_pose (lists of [N_i] bool), hyp [10, 1000, 3]"""
    nc = NF - 1
    z = lambda *shape: np.zeros(shape, dtype=dt)
    out = dict(n_corres=np.zeros(nc, dtype=np.int64), status=np.zeros(nc, dtype=np.int64), iterations=np.zeros(nc, dtype=np.int64),
               best_iteration=-np.ones(nc, dtype=np.int64), best_root=-np.ones(nc, dtype=np.int64), inliers=np.zeros(nc, dtype=np.int64),
               good=np.zeros(nc, dtype=np.int64), choice=np.zeros(nc, dtype=np.int64), average_parallax=z(nc), F=z(nc, 9), R=z(nc, 3, 3), T=z(nc, 3),
               mask_ransac=[None] * nc, mask_pose=[None] * nc, hyp=-np.ones((nc, MAX_ITERS, 3), dtype=np.int64))
    numeric = False
    for i in range(nc):
        _, a, b = correspondences(S["track_start"], S["track_nobs"], S["track_obs"], i)
        N = len(a)
        out["n_corres"][i] = N
        out["mask_ransac"][i], out["mask_pose"][i] = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
        bad = not (np.isfinite(a).all() and np.isfinite(b).all())
        numeric = numeric or bad
        ad, bd = a.astype(dt), b.astype(dt)
        par = np.sqrt(((ad - bd) ** 2).sum(1)).sum() / dt(N) if N else dt(0)
        out["average_parallax"][i] = par
        if not N > 20:
            out["status"][i] = FEW_CORRES
            continue
        if not par * dt(460) > dt(30):
            out["status"][i] = LOW_PARALLAX
            continue
        if bad:
            out["status"][i] = NO_MODEL
            continue
        pts = np.concatenate([a, b], axis=1).astype(np.float32).astype(dt)          # cv::Point2f
        r = ransac(pts, samples(i, N), niters_table(N))
        out["iterations"][i], out["best_iteration"][i], out["best_root"][i] = r["iterations"], r["best_iteration"], r["best_root"]
        out["hyp"][i] = r["hyp"]
        if r["F"] is None:
            out["status"][i] = NO_MODEL
            continue
        out["inliers"][i], out["F"][i], out["mask_ransac"][i] = r["inliers"], r["F"], r["mask"]
        p = recover_pose(r["F"], pts, r["mask"])
        out["R"][i], out["T"][i], out["good"][i], out["mask_pose"][i], out["choice"][i] = p["R"], p["T"], p["good"], p["mask"], p["choice"]
        out["status"][i] = SUCCESS if p["good"] > 12 else FEW_GOOD
    won = np.nonzero(out["status"] == SUCCESS)[0]
    fail = FAIL_NUMERIC if numeric else (0 if len(won) else FAIL_NONE)
    out.update(ok=0 if fail else 1, fail=fail, l=-1 if fail else int(won[0]),
               relative_R=z(3, 3) if fail else out["R"][won[0]].copy(), relative_T=z(3) if fail else out["T"][won[0]].copy())
    return out
