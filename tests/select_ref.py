"""NumPy restatement of the attention / anticipation feature selector, the model vpl_select_features_batch is held to:
FeatureSelector::select (vins_estimator/src/feature_selector.cpp) with HorizonGenerator::imu (utility/selector/
horizon_generator.cpp:24-68), written from the description of the six steps -- horizon, motion information, depth guess,
per-feature information, greedy selection, id book.

Dense 45 x 45 matrices in the natural order (five states of position, velocity, accelerometer bias), a plain Cholesky loop,
Eigen's slerp / toRotationMatrix / q * v / 3 x 3 cofactor inverse, PinholeCamera::distortion, std::round.  Generic in the dtype
(np.float64 or np.longdouble) like tests/relpose_ref.py: the distance between the two runs measures what float64 rounding does
to a value.  Quaternions are (w, x, y, z); nothing is normalised that the reference does not normalise (Utility::deltaQ is not).

Deviation shared with the device: a candidate whose Cholesky meets a pivot that is not > 0 (or not finite) has f = NaN and is not
selected in that round (Eigen's LLT goes on with an unfinished factor there; the reference logs "logdet returned nan!" in the
cases it notices)."""
import math

import numpy as np

HORIZON = 4
STATE = 9
N45 = STATE * (HORIZON + 1)
POS12 = [STATE * i + k for i in range(1, HORIZON + 1) for k in range(3)]      # the position dimensions of states 1 .. 4
REST33 = [i for i in range(N45) if i not in POS12]
GRAVITY = (0.0, 0.0, -9.80665)
F64_ONE = 1.0 - np.finfo(np.float64).eps      # Eigen's slerp threshold, one float64 number for every dtype, as on the device
TRI12 = [(r, c) for r in range(12) for c in range(r + 1)]    # the packed lower triangle of a 12 x 12 block, row after row


# ---- Eigen's quaternion arithmetic ------------------------------------------------------------------------------------------
def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]], dtype=a.dtype)


def qinv(q):
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return np.array([q[0], -q[1], -q[2], -q[3]], dtype=q.dtype) / n2


def qmat(q):
    w, x, y, z = q
    tx, ty, tz = x + x, y + y, z + z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = q.dtype.type(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], dtype=q.dtype)


def qrot(q, v):
    uv = np.cross(q[1:], v)
    uv = uv + uv
    return v + q[0] * uv + np.cross(q[1:], uv)


def slerp(a, t, b):
    dt = a.dtype.type
    d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]
    ad = abs(d)
    if ad >= dt(F64_ONE):
        s0, s1 = dt(1) - t, t
    else:
        th = np.arccos(ad)
        st = np.sin(th)
        s0, s1 = np.sin((dt(1) - t) * th) / st, np.sin(t * th) / st
    if d < 0:
        s1 = -s1
    return s0 * a + s1 * b


def skew(v):
    z = v.dtype.type(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=v.dtype)


def inv3(m):
    """Eigen's 3 x 3 inverse: the cofactors over the determinant"""
    c = lambda i, j: m[(i + 1) % 3, (j + 1) % 3] * m[(i + 2) % 3, (j + 2) % 3] - m[(i + 1) % 3, (j + 2) % 3] * m[(i + 2) % 3, (j + 1) % 3]
    c00, c10, c20 = c(0, 0), c(1, 0), c(2, 0)
    det = m[0, 0] * c00 + m[1, 0] * c10 + m[2, 0] * c20
    out = np.array([[c(j, i) for j in range(3)] for i in range(3)], dtype=m.dtype)
    return out / det


def inverse(m):
    """general inverse: Gauss-Jordan with partial pivoting"""
    n = len(m)
    a = np.concatenate([m.copy(), np.eye(n, dtype=m.dtype)], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        if p != k:
            a[[k, p]] = a[[p, k]]
        a[k] = a[k] / a[k, k]
        for r in range(n):
            if r != k:
                a[r] = a[r] - a[r, k] * a[k]
    return a[:, n:]


# ---- inputs -----------------------------------------------------------------------------------------------------------------
class Params:
    """vpl_sel_params"""

    def __init__(self, acc_var, acc_bias_var, max_features, init_thresh, width, height, fx, fy, cx, cy, k1, k2, p1, p2, q_ic, t_ic):
        self.acc_var, self.acc_bias_var, self.max_features, self.init_thresh = acc_var, acc_bias_var, int(max_features), int(init_thresh)
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy, self.k1, self.k2, self.p1, self.p2 = fx, fy, cx, cy, k1, k2, p1, p2
        self.q_ic, self.t_ic = np.asarray(q_ic, dtype=np.float64), np.asarray(t_ic, dtype=np.float64)


# ---- step 1: the horizon ----------------------------------------------------------------------------------------------------
def horizon(dt, P0, Q0, P1, Q1, V1, Ba0, acc, gyr, n_imu, delta_imu):
    """-> P [5, 3], Q [5, 4]: states k, k + 1 as given, k + 2 .. k + 4 by constant-a, constant-w propagation"""
    f = lambda a: np.asarray(a, dtype=dt)
    P, Q = np.zeros((5, 3), dtype=dt), np.zeros((5, 4), dtype=dt)
    P[0], Q[0], P[1], Q[1] = f(P0), f(Q0), f(P1), f(Q1)
    d = dt(delta_imu)
    g = f(GRAVITY)
    w = f(gyr) * d
    qimu = np.array([dt(1), w[0] / dt(2), w[1] / dt(2), w[2] / dt(2)], dtype=dt)
    ab = f(acc) - f(Ba0)
    V = f(V1)
    for h in range(2, HORIZON + 1):
        p, q = P[h - 1].copy(), Q[h - 1].copy()
        for _ in range(int(n_imu)):
            q = qmul(q, qimu)
            qa = qrot(q, ab)
            V = V + (g + qa) * d
            p = p + V * d + dt(0.5) * g * d * d + dt(0.5) * qa * d * d
        P[h], Q[h] = p, q
    return P, Q


# ---- step 2: the motion information -----------------------------------------------------------------------------------------
def cov_imu(dt, n_imu, delta_imu, acc_var, acc_bias_var):
    n = int(n_imu)
    c11 = c12 = dt(0)
    for i in range(n):
        jkh = dt(n - i) - dt(0.5)
        c11, c12 = c11 + jkh * jkh, c12 + jkh
    d = dt(delta_imu)
    d2 = d * d
    d3 = d2 * d
    d4 = d3 * d
    av, bv = dt(acc_var), dt(acc_bias_var)
    cov = np.zeros((9, 9), dtype=dt)
    I = np.eye(3, dtype=dt)
    cov[0:3, 0:3] = I * dt(n) * c11 * d4 * av
    cov[0:3, 3:6] = I * c12 * d3 * av
    cov[3:6, 0:3] = cov[0:3, 3:6].T
    cov[3:6, 3:6] = I * dt(n) * d2 * av
    cov[6:9, 6:9] = I * dt(n) * bv
    return cov


def cov_imu_inverse_closed(dt, n_imu, delta_imu, acc_var, acc_bias_var):
    """the inverse of cov_imu from its block structure [[a I, b I, 0], [b I, c I, 0], [0, 0, e I]]"""
    cov = cov_imu(dt, n_imu, delta_imu, acc_var, acc_bias_var)
    a, b, c, e = cov[0, 0], cov[0, 3], cov[3, 3], cov[6, 6]
    det = a * c - b * b
    out = np.zeros((9, 9), dtype=dt)
    I = np.eye(3, dtype=dt)
    out[0:3, 0:3], out[0:3, 3:6], out[3:6, 0:3], out[3:6, 3:6], out[6:9, 6:9] = I * (c / det), I * (-b / det), I * (-b / det), I * (a / det), I / e
    return out


def imu_matrices(dt, Qi, Qj, n_imu, delta_imu, acc_var, acc_bias_var):
    """createLinearImuMatrices -> (covImu^-1, Ablk)"""
    n = int(n_imu)
    N, M = np.zeros((3, 3), dtype=dt), np.zeros((3, 3), dtype=dt)
    for i in range(n):
        R = qmat(slerp(Qi, dt(i) / dt(n), Qj))
        jkh = dt(n - i) - dt(0.5)
        N, M = N + jkh * R, M + R
    d = dt(delta_imu)
    A = -np.eye(9, dtype=dt)
    A[0:3, 3:6] = -np.eye(3, dtype=dt) * dt(n) * d
    A[0:3, 6:9] = N * (d * d)
    A[3:6, 6:9] = M * d
    return inverse(cov_imu(dt, n_imu, delta_imu, acc_var, acc_bias_var)), A


def omega_kkH(dt, Q, n_imu, delta_imu, acc_var, acc_bias_var):
    """calcInfoFromRobotMotion + addOmegaPrior over the horizon's orientations Q [5, 4]"""
    Om = np.zeros((N45, N45), dtype=dt)
    for h in range(1, HORIZON + 1):
        W, A = imu_matrices(dt, Q[h - 1], Q[h], n_imu, delta_imu, acc_var, acc_bias_var)
        a, b = (h - 1) * STATE, h * STATE
        tmp = A.T @ W
        Om[a:a + 9, a:a + 9] += tmp @ A
        Om[a:a + 9, b:b + 9] += tmp
        Om[b:b + 9, a:a + 9] += tmp.T
        Om[b:b + 9, b:b + 9] += W
    Om[0:9, 0:9] += np.eye(9, dtype=dt)
    return Om


# ---- step 3: the depth guess ------------------------------------------------------------------------------------------------
def nn_depth(cloud, x, y):
    """cloud [m, 3] = x, y, depth (float64, as handed over): the depth of the nearest neighbour in (x, y), the lowest index on
    an exact tie; 1.0 for an empty cloud"""
    cloud = np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    if len(cloud) == 0:
        return 1.0
    d2 = (cloud[:, 0] - x) ** 2 + (cloud[:, 1] - y) ** 2
    return float(cloud[int(np.argmin(d2)), 2])


# ---- step 4: the information of one feature ---------------------------------------------------------------------------------
def cround(v):
    """std::round: halves away from zero"""
    v = float(v)
    return int(math.floor(v + 0.5)) if v >= 0 else -int(math.floor(-v + 0.5))


def space_to_plane(dt, par, u):
    x, y = u[0] / u[2], u[1] / u[2]                      # no sign test on u[2]
    k1, k2, p1, p2 = dt(par.k1), dt(par.k2), dt(par.p1), dt(par.p2)
    mx2, my2, mxy = x * x, y * y, x * y
    rho2 = mx2 + my2
    rad = k1 * rho2 + k2 * rho2 * rho2
    dx = x * rad + dt(2) * p1 * mxy + p2 * (rho2 + dt(2) * mx2)
    dy = y * rad + dt(2) * p2 * mxy + p1 * (rho2 + dt(2) * my2)
    return dt(par.fx) * (x + dx) + dt(par.cx), dt(par.fy) * (y + dy) + dt(par.cy)


def in_fov(par, px, py):
    if not (np.isfinite(px) and np.isfinite(py)) or abs(px) > 1e9 or abs(py) > 1e9:
        return False
    u, v = cround(px), cround(py)
    return 0 <= u < par.width and 0 <= v < par.height


def feature_info(dt, par, P, Q, x, y, depth):
    """calcInfoFromFeatures for one feature -> (Delta [45, 45] or None when no future frame sees it, visibility of k+2 .. k+4)"""
    f = lambda a: np.asarray(a, dtype=dt)
    q_ic, t_ic = f(par.q_ic), f(par.t_ic)
    t1 = P[1] + qrot(Q[1], t_ic)
    q1 = qmul(Q[1], q_ic)
    b = f([x, y, 1.0])
    b = b / np.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
    pell = t1 + qrot(q1, b * dt(depth))
    Ch = np.zeros((HORIZON + 1, 3, 3), dtype=dt)
    EtE = np.zeros((3, 3), dtype=dt)
    vis = []
    for h in range(2, HORIZON + 1):
        th = P[h] + qrot(Q[h], t_ic)
        qh = qmul(Q[h], q_ic)
        u = qrot(qinv(qh), pell - th)
        u = u / np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
        px, py = space_to_plane(dt, par, u)
        ok = in_fov(par, px, py)
        vis.append(ok)
        if not ok:
            continue
        Bh = skew(u) @ qmat(qinv(qmul(qh, q_ic)))          # q_IC applied twice, as the reference writes it
        Ch[h] = Bh.T @ Bh
        EtE = EtE + Ch[h]
    if not any(vis):
        return None, vis
    Bh = skew(b) @ qmat(qinv(qmul(q1, q_ic)))
    Ch[1] = Bh.T @ Bh
    EtE = EtE + Ch[1]
    W = inv3(EtE)
    D = np.zeros((N45, N45), dtype=dt)
    for j in range(1, HORIZON + 1):
        for i in range(j, HORIZON + 1):
            Dij = Ch[i] @ W @ Ch[j].T
            if i == j:
                D[9 * i:9 * i + 3, 9 * j:9 * j + 3] = Ch[i] - Dij
            else:
                D[9 * i:9 * i + 3, 9 * j:9 * j + 3] = -Dij
                D[9 * j:9 * j + 3, 9 * i:9 * i + 3] = -Dij.T
    return D, vis


def delta12(D):
    """the packed lower triangle (78) of Delta's 12 x 12 block over POS12: all of Delta that is not zero"""
    return np.array([D[POS12[r], POS12[c]] for r, c in TRI12], dtype=D.dtype)


# ---- step 5: the greedy selection -------------------------------------------------------------------------------------------
def logdet_chol(M):
    """Utility::logdet(M, true) over the lower triangles of a stack M [n, 45, 45]: 2 sum log L_ii by a plain Cholesky loop; NaN
    where a pivot is not > 0"""
    M = np.array(M, copy=True)
    n, N = M.shape[0], M.shape[1]
    ld = np.zeros(n, dtype=M.dtype)
    bad = np.zeros(n, dtype=bool)
    L = np.zeros_like(M)
    for j in range(N):
        x = M[:, j, j] - np.sum(L[:, j, :j] * L[:, j, :j], axis=1)
        bad |= ~(x > 0)
        x = np.where(bad, M.dtype.type(1), x)
        d = np.sqrt(x)
        L[:, j, j] = d
        ld += np.log(d)
        if j + 1 < N:
            L[:, j + 1:, j] = (M[:, j + 1:, j] - np.einsum("nik,nk->ni", L[:, j + 1:, :j], L[:, j, :j])) / d[:, None]
    ld = ld * M.dtype.type(2)
    ld[bad] = np.nan
    return ld


def log_ub(M):
    """sum log diag over a stack"""
    return np.sum(np.log(np.diagonal(M, axis1=1, axis2=2)), axis=1)


def round_values(Omega, OmegaS, cand, deltas, probs):
    """one round: (ub, f) of the candidates `cand` (ids); Omega already holds the used features"""
    dt = Omega.dtype.type
    base = Omega + OmegaS
    M = np.stack([base + dt(probs[c]) * deltas[c] for c in cand])
    return log_ub(M), logdet_chol(M)


def pick(cand, ub, f):
    """the reference's rules over one round's values -> (index into cand or -1, gap between the best and the second-best f
    among the candidates the map keeps).  Equal ub collapse to the highest id; f must be > -1.0; ties in f go to the larger ub."""
    keep = {}
    for k in sorted(range(len(cand)), key=lambda k: cand[k]):
        keep[ub[k]] = k                                   # std::map<double, int>: a later (higher) id overwrites
    order = sorted(keep.values(), key=lambda k: -ub[k])
    best, fmax = -1, -1.0
    for k in order:
        if f[k] > fmax:
            best, fmax = k, f[k]
    fs = sorted([float(f[k]) for k in order if np.isfinite(f[k])], reverse=True)
    gap = fs[0] - fs[1] if len(fs) > 1 else np.inf
    return best, gap


def greedy(Omega_kkH, deltas, probs, deltas_used, kappa, prefix=()):
    """selectInformativeFeatures.  deltas {id: Delta} of the visible new features, probs {id: p}, deltas_used a list.
    prefix: ids forced first (not counted in kappa).  -> dict ids, f (of every selection), rounds: per round (cand, ub, f, gap)"""
    dt = Omega_kkH.dtype.type
    Omega = Omega_kkH.copy()
    for D in deltas_used:
        Omega = Omega + D
    OmegaS = np.zeros_like(Omega)
    black = []
    for c in prefix:
        OmegaS = OmegaS + dt(probs[c]) * deltas[c]
        black.append(c)
    ids, fsel, rounds = [], [], []
    for _ in range(int(kappa)):
        cand = [c for c in sorted(deltas) if c not in black]
        if not cand:
            break
        ub, f = round_values(Omega, OmegaS, cand, deltas, probs)
        k, gap = pick(cand, ub, f)
        rounds.append((cand, ub, f, gap))
        if k < 0:
            break                                         # nothing changes any more: every later round selects nothing either
        OmegaS = OmegaS + dt(probs[cand[k]]) * deltas[cand[k]]
        black.append(cand[k])
        ids.append(cand[k])
        fsel.append(f[k])
    return dict(ids=ids, f=np.array(fsel, dtype=Omega.dtype), rounds=rounds)


# ---- one sequence, steps 1 - 5 ----------------------------------------------------------------------------------------------
def run(dt, par, inp, prefix=(), kappa=None):
    """inp: a select_inputs.Scene (or anything with its members).  -> dict: P, Q, omega [45, 45], deltas {id: Delta}, invisible
    (ids), used (list of Delta, the invisible ones left out), d12_new [n_new, 78] / d12_used [n_used, 78] (zero rows for
    invisible features), depth_new, and greedy()'s result"""
    if inp.horizon is not None:
        hz = np.asarray(inp.horizon, dtype=dt).reshape(5, 7)
        P, Q = hz[:, :3].copy(), hz[:, 3:].copy()
    else:
        P, Q = horizon(dt, inp.P0, inp.Q0, inp.P1, inp.Q1, inp.V1, inp.Ba0, inp.acc, inp.gyr, inp.n_imu, inp.delta_imu)
    Om = omega_kkH(dt, Q, inp.n_imu, inp.delta_imu, par.acc_var, par.acc_bias_var)
    deltas, probs, invisible, depth_new = {}, {}, [], []
    d12_new = np.zeros((len(inp.new_id), 78), dtype=dt)
    for k, (i, x, y, p) in enumerate(zip(inp.new_id, inp.new_x, inp.new_y, inp.new_prob)):
        d = nn_depth(inp.cloud, x, y)
        depth_new.append(d)
        D, _ = feature_info(dt, par, P, Q, x, y, d)
        if D is None:
            invisible.append(int(i))
            continue
        deltas[int(i)], probs[int(i)] = D, p
        d12_new[k] = delta12(D)
    used = []
    d12_used = np.zeros((len(inp.used_x), 78), dtype=dt)
    for k, (x, y) in enumerate(zip(inp.used_x, inp.used_y)):
        D, _ = feature_info(dt, par, P, Q, x, y, nn_depth(inp.cloud, x, y))
        if D is not None:
            used.append(D)
            d12_used[k] = delta12(D)
    out = dict(P=P, Q=Q, omega=Om, deltas=deltas, probs=probs, invisible=invisible, used=used, d12_new=d12_new, d12_used=d12_used,
               depth_new=depth_new)
    out.update(greedy(Om, deltas, probs, used, inp.kappa if kappa is None else kappa, prefix))
    return out


# ---- step 6: the id book ----------------------------------------------------------------------------------------------------
class Book:
    """the members of FeatureSelector that select() keeps between images"""

    def __init__(self, max_features, init_thresh):
        self.max_features, self.init_thresh = int(max_features), int(init_thresh)
        self.last_id, self.tracked, self.first_image = 0, [], True

    def split(self, ids):
        """-> (image, image_new, subset, kappa) before the selection; lastFeatureId_ moves"""
        ids = sorted(set(int(i) for i in ids))
        image = [i for i in ids if i <= self.last_id]
        new = [i for i in ids if i > self.last_id]
        if new:
            self.last_id = new[-1]
        present = set(image)
        subset = sorted(set(i for i in self.tracked if i in present))
        return image, new, subset, max(0, self.max_features - len(subset))

    def finish(self, image, new, subset, initialized, selected):
        """selected: what selectInformativeFeatures returned (read only when initialized) -> the ids handed to the back end"""
        subset = set(subset)
        chosen = []
        if initialized:
            chosen = list(selected)
            subset |= set(chosen)
        elif self.first_image:
            subset = set(new)
            self.tracked.extend(sorted(subset))
            self.first_image = False
        if not initialized and len(subset) < self.init_thresh:
            subset |= set(image)
        self.tracked.extend(chosen)
        return sorted(subset)
