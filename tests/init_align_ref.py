"""NumPy restatement of the reference's visual-inertial alignment, the model vpl_init_align_batch is held to:
solveGyroscopeBias, TangentBasis, RefineGravity, LinearAlignment (vins_estimator/src/initial/initial_aligment.cpp:3-207), the state
change of Estimator::visualInitialAlign (estimator.cpp:512-588) and Utility::g2R (utility/utility.cpp:3-13).

Written once, generic in the dtype: every function takes `dt` (np.float64 or np.longdouble) and computes in it, so that the
distance between the two runs measures what float64 rounding does to a result.  The pre-integrations are an input: a list of
objects with sum_dt, delta_p [3], delta_q [4] (x, y, z, w), delta_v [3] and jacobian [225] (row-major 15 x 15), entry f the interval
that ends in image frame f (entry 0 unused) -- capi.Preintegration fits.

Kept as the reference has them: cov_inv = I; the scale column divided by 100, the systems multiplied by 1000; RefineGravity's A and
b zeroed once before its four rounds (round k adds its blocks to 1000 x what round k - 1 solved); Vs[kv] from x.segment<3>(3 kv).
The solve is LDL^T with Eigen's diagonal pivoting."""
import numpy as np

NF = 11
FAIL_GRAVITY, FAIL_SCALE, FAIL_REFINED_SCALE, FAIL_NONFINITE = 1, 2, 4, 8
O_R, O_BG = 3, 12


def require_extended():
    """the extended-precision run needs a long double that is wider than float64"""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended-precision type here"


def _a(x, dt):
    return np.array(x, dtype=dt)


def mat2q(R, dt):
    """Eigen's Quaternion(Matrix3): (w, x, y, z), not normalised"""
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
    n2 = q @ q
    return np.array([q[0], -q[1], -q[2], -q[3]], dtype=q.dtype) / n2


def qmat(q, dt):
    w, x, y, z = q
    two = dt(2)
    return _a([[1 - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
               [two * (x * y + z * w), 1 - two * (x * x + z * z), two * (y * z - x * w)],
               [two * (x * z - y * w), two * (y * z + x * w), 1 - two * (x * x + y * y)]], dt)


def ldlt_solve(A, b):
    """A.ldlt().solve(b): LDL^T with symmetric pivoting on the largest diagonal entry, in A's dtype"""
    A = A.copy()
    n = A.shape[0]
    perm = np.arange(n)
    for j in range(n):
        p = j + int(np.argmax(np.abs(np.diag(A)[j:])))
        if p != j:
            A[[j, p], :] = A[[p, j], :]
            A[:, [j, p]] = A[:, [p, j]]
            perm[[j, p]] = perm[[p, j]]
        d = A[j, j]
        if j + 1 < n:
            c = A[j + 1:, j].copy()
            l = c / d
            A[j + 1:, j + 1:] -= np.outer(l, c)
            A[j + 1:, j] = l
    L = np.tril(A, -1)
    y = b[perm].copy()
    for j in range(n):
        y[j + 1:] -= L[j + 1:, j] * y[j]
    y = y / np.diag(A)
    for j in range(n - 1, -1, -1):
        y[:j] -= L[j, :j] * y[j]
    x = np.zeros_like(y)
    x[perm] = y
    return x


def _pre(p, dt):
    return (dt(p.sum_dt), _a(list(p.delta_p), dt), _a(list(p.delta_q), dt), _a(list(p.delta_v), dt))


def solve_gyroscope_bias(R, pre, dt):
    """:3-37 -> delta_bg"""
    A, b = np.zeros((3, 3), dtype=dt), np.zeros(3, dtype=dt)
    for i in range(len(R) - 1):
        q_ij = mat2q(R[i].T @ R[i + 1], dt)
        J = _a(np.array(list(pre[i + 1].jacobian)).reshape(15, 15)[O_R:O_R + 3, O_BG:O_BG + 3], dt)
        dq = _a(list(pre[i + 1].delta_q), dt)
        tmp_b = dt(2) * qmul(qinv(_a([dq[3], dq[0], dq[1], dq[2]], dt)), q_ij)[1:]
        A += J.T @ J
        b += J.T @ tmp_b
    return ldlt_solve(A, b)


def normalized(v):
    n2 = v @ v
    return v / np.sqrt(n2) if n2 > 0 else v


def tangent_basis(g0, dt):
    a = normalized(g0)
    tmp = _a([0, 0, 1], dt)
    if np.array_equal(a, tmp):
        tmp = _a([1, 0, 0], dt)
    b = normalized(tmp - a * (a @ tmp))
    return np.stack([b, np.cross(a, b)], 1)


def _blocks(R, T, pre, tic, dt, lxly, g0):
    """tmp_A, tmp_b of every interval: LinearAlignment's (lxly None, 10 columns) or RefineGravity's (9 columns)"""
    out = []
    I3 = np.eye(3, dtype=dt)
    for i in range(len(R) - 1):
        sdt, dp, _, dv = _pre(pre[i + 1], dt)
        RiT = R[i].T
        ng = 3 if lxly is None else 2
        tA = np.zeros((6, 7 + ng), dtype=dt)
        tb = np.zeros(6, dtype=dt)
        M1, M2 = RiT * sdt * sdt / dt(2), RiT * sdt
        tA[0:3, 0:3] = -sdt * I3
        tA[0:3, 6:6 + ng] = M1 if lxly is None else M1 @ lxly
        tA[0:3, 6 + ng] = RiT @ (T[i + 1] - T[i]) / dt(100)
        tb[0:3] = dp + RiT @ R[i + 1] @ tic - tic
        tA[3:6, 0:3] = -I3
        tA[3:6, 3:6] = RiT @ R[i + 1]
        tA[3:6, 6:6 + ng] = M2 if lxly is None else M2 @ lxly
        tb[3:6] = dv
        if lxly is not None:
            tb[0:3] = tb[0:3] - M1 @ g0
            tb[3:6] = tb[3:6] - M2 @ g0
        out.append((tA, tb))
    return out


def _add_blocks(A, b, blocks, nt):
    """the arrow assembly (:165-175, :103-113); nt = size of the shared tail (4 or 3)"""
    for i, (tA, tb) in enumerate(blocks):
        rA, rb = tA.T @ tA, tA.T @ tb
        A[3 * i:3 * i + 6, 3 * i:3 * i + 6] += rA[:6, :6]
        b[3 * i:3 * i + 6] += rb[:6]
        A[-nt:, -nt:] += rA[-nt:, -nt:]
        b[-nt:] += rb[-nt:]
        A[3 * i:3 * i + 6, -nt:] += rA[:6, -nt:]
        A[-nt:, 3 * i:3 * i + 6] += rA[-nt:, :6]


def refine_gravity(R, T, pre, tic, g, g_norm, dt):
    """:55-123 -> (g, x)"""
    G = np.sqrt(dt(g_norm) * dt(g_norm))
    g0 = normalized(g) * G
    n = 3 * len(R) + 3
    A, b = np.zeros((n, n), dtype=dt), np.zeros(n, dtype=dt)   # zeroed ONCE (:63-66)
    x = None
    for _ in range(4):
        lxly = tangent_basis(g0, dt)
        _add_blocks(A, b, _blocks(R, T, pre, tic, dt, lxly, g0), 3)
        A = A * dt(1000)
        b = b * dt(1000)
        x = ldlt_solve(A, b)
        g0 = normalized(g0 + lxly @ x[n - 3:n - 1]) * G
    return g0, x


def linear_alignment(R, T, pre, tic, g_norm, dt):
    """:125-197 -> dict(ok, fail, g_linear, s_linear, x_linear, and behind a passed first check: g_refined, s, x)"""
    G = np.sqrt(dt(g_norm) * dt(g_norm))
    n = 3 * len(R) + 4
    A, b = np.zeros((n, n), dtype=dt), np.zeros(n, dtype=dt)
    _add_blocks(A, b, _blocks(R, T, pre, tic, dt, None, None), 4)
    x = ldlt_solve(A * dt(1000), b * dt(1000))
    s = x[n - 1] / dt(100)
    g = x[n - 4:n - 1].copy()
    gn = np.sqrt(g @ g)
    out = dict(ok=False, fail=0, g_linear=g, s_linear=s, x_linear=x)
    if not (np.isfinite(gn) and np.isfinite(s)):
        out["fail"] |= FAIL_NONFINITE
    if abs(gn - G) > 1.0:
        out["fail"] |= FAIL_GRAVITY
    if s < 0:
        out["fail"] |= FAIL_SCALE
    if out["fail"]:
        return out
    g, x = refine_gravity(R, T, pre, tic, g, g_norm, dt)
    s = x[-1] / dt(100)
    out.update(g_refined=g, s=s, x=x)
    if not (np.isfinite(s) and np.all(np.isfinite(g)) and np.all(np.isfinite(x))):
        out["fail"] |= FAIL_NONFINITE
    if s < 0:
        out["fail"] |= FAIL_REFINED_SCALE
    out["ok"] = out["fail"] == 0
    return out


def _pi(dt):
    return np.arctan2(dt(0), dt(-1))


def R2ypr(R, dt):
    n, o, a = R[:, 0], R[:, 1], R[:, 2]
    y = np.arctan2(n[1], n[0])
    p = np.arctan2(-n[2], n[0] * np.cos(y) + n[1] * np.sin(y))
    r = np.arctan2(a[0] * np.sin(y) - a[1] * np.cos(y), -o[0] * np.sin(y) + o[1] * np.cos(y))
    return _a([y, p, r], dt) / _pi(dt) * dt(180)


def ypr2R(ypr, dt):
    y, p, r = _a(ypr, dt) / dt(180) * _pi(dt)
    Rz = _a([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]], dt)
    Ry = _a([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]], dt)
    Rx = _a([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]], dt)
    return Rz @ Ry @ Rx


def from_two_vectors(a, b, dt):
    """Eigen's Quaternion::FromTwoVectors (its branch for opposite vectors is not restated: never met by a test)"""
    v0, v1 = normalized(a), normalized(b)
    c = v1 @ v0
    assert c > -1 + 1e-12
    ax = np.cross(v0, v1)
    s = np.sqrt((dt(1) + c) * dt(2))
    return np.concatenate([[s * dt(0.5)], ax / s]).astype(dt)


def g2R(g, dt):
    R0 = qmat(from_two_vectors(normalized(g), _a([0, 0, 1], dt), dt), dt)
    return ypr2R([-R2ypr(R0, dt)[0], 0, 0], dt) @ R0


def visual_initial_align(R, T, pre, key, bas, bgs, tic, g_norm, dt=np.float64):
    """Estimator::visualInitialAlign on the image frames (R [F,3,3], T [F,3]) and their pre-integrations `pre` -- those the
    alignment reads: for delta_bg the ones under the old bias, for the rest the re-propagated ones, so `pre` is a pair
    (before, after).  -> dict: ok, fail, delta_bg, g_linear, s_linear, x_linear and, as far as the reference gets, s, g_refined, x,
    g, vel [F,3], pose [11,7], speed_bias [11,9]."""
    R, T, tic = _a(R, dt).reshape(-1, 3, 3), _a(T, dt).reshape(-1, 3), _a(tic, dt)
    bas, bgs = _a(bas, dt).reshape(NF, 3), _a(bgs, dt).reshape(NF, 3)
    F = len(R)
    pre_before, pre_after = pre
    dbg = solve_gyroscope_bias(R, pre_before, dt)
    out = linear_alignment(R, T, pre_after, tic, g_norm, dt)
    out["delta_bg"] = dbg
    if not out["ok"]:
        return out
    s, g, x = out["s"], out["g_refined"], out["x"]
    Ps = np.stack([T[key[i]] for i in range(NF)])
    Rs = np.stack([R[key[i]] for i in range(NF)])
    P0 = s * Ps[0] - Rs[0] @ tic
    Ps = np.stack([(s * Ps[i] - Rs[i] @ tic) - P0 for i in range(NF)])
    Vs = np.stack([R[key[kv]] @ x[3 * kv:3 * kv + 3] for kv in range(NF)])   # kv counts key frames
    R0 = g2R(g, dt)
    R0 = ypr2R([-R2ypr(R0 @ Rs[0], dt)[0], 0, 0], dt) @ R0
    pose, sb = np.zeros((NF, 7), dtype=dt), np.zeros((NF, 9), dtype=dt)
    for i in range(NF):
        q = mat2q(R0 @ Rs[i], dt)
        pose[i, :3] = R0 @ Ps[i]
        pose[i, 3:] = [q[1], q[2], q[3], q[0]]
        sb[i, :3] = R0 @ Vs[i]
        sb[i, 3:6] = bas[i]
        sb[i, 6:9] = bgs[i] + dbg
    out.update(g=R0 @ g, vel=x[:3 * F].reshape(F, 3).copy(), pose=pose, speed_bias=sb)
    if not (np.all(np.isfinite(pose)) and np.all(np.isfinite(sb)) and np.all(np.isfinite(out["g"]))):
        out["ok"], out["fail"] = False, out["fail"] | FAIL_NONFINITE
    return out


def build_jobs(n_samples, key):
    """(offset, nsamples, acc0 row) of the image intervals 1..F-1, then of the window intervals 1..10 (acc0 row -1: the
    measurement before the first sample)"""
    F = len(n_samples)
    off = np.zeros(F + 1, dtype=np.int64)
    for f in range(1, F):
        off[f + 1] = off[f] + n_samples[f]
    jobs = [(off[f], n_samples[f], off[f] - 1) for f in range(1, F)]
    for i in range(1, NF):
        a, b = key[i - 1] + 1, key[i]
        jobs.append((off[a], sum(n_samples[a:b + 1]), off[a] - 1))
    return np.array(jobs, dtype=np.int32)
