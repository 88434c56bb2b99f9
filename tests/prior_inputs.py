"""Seeded priors, window states and windows for prior_ref.py's tests (test_prior_reference.py, test_gpu_prior_factor.py).

Priors: the smallest sizes that enter each branch of the code that consumes a prior (blocks 6, 9 or 6 wide, in the reference's
order: poses by frame, speed/bias, then the extrinsic):
    n    blocks                          what it enters
    21   pose 2, speed/bias 3, ex        general path (k_solve): step_ref's _later_speed_bias_prior shape
    48   8 poses                         full MFMA tiles in k_prep; last column of lin_prior's register pass
    51   7 poses, speed/bias 0           first columns of the tail loop; partial K-step (51 = 4 x 12 + 3)
    63   9 poses, speed/bias 0           last row of the first row pass
    66   11 poses                        first rows of the second row pass
    75   10 poses, speed/bias 0, ex      the reference's largest; n <= PRH_N at small capacity
    81   11 poses, speed/bias 0, ex      n > PRH_N (76 at most): the += pass of lin_assemble
    111  11 poses, 5 speed/bias          staged in k_prep with nstage = 111 (general path)
    117  11 poses, 5 speed/bias, ex      above PREP_NMAX = 112: k_prep's unstaged loop
    171  everything                      MAXPN, MAXPB
J0 is dense upper triangular plus a diagonal (the prior alone pins its states), r0 is non-zero; variant "u" has rows of unit
scale, "s" row scales spread over 10^[-3, 7] (the reference's priors carry bias rows of about 2e7).  Prior ids: "n75u", "n75s".

State families (the window states x, and the x0 the prior is given):
    general  x0 about 0.05 rad and 0.05 m (speed/bias 0.05) from x; every second quaternion of x0 negated (the product's w < 0);
             pose-like block 0 rotated by 2.5 rad, block 1 displaced by 1e-9 (cancellation in dx; negated too), block 2 with
             |q0| = 1 + 1e-6, block 3 rotated by 2 rad and negated (w = -cos 1); half of the first speed/bias block at 1e-9
    at_x0    x0 = x bit for bit, frame 0 at the origin, the rotations taken from the 24 Hurwitz units {+-1, +-i, +-j, +-k,
             (+-1 +-i +-j +-k) / 2} in the sign Eigen's Quaternion(Matrix3) returns: normalisation, rotation matrix and the way
             back are exact on them, so the device's states are x, dx is exactly 0 and r, g, cost are r0, g0 = J0^T r0, |r0|^2 / 2
    exact    every x0 quaternion (0, 0, 0, 1), positions and speed/bias of x0 multiples of 1/16 up to 1/8, x - x0 multiples of
             1/32: every entry of dx is exact in float64 WHATEVER the window's quaternions are (q0^-1 (x) q = q, term by term), so
             unit(dx) is 2 eps64 |q_k| and eps64 (|x| + |x0|) <= 9 eps64 |dx|, and g0 + H dx is held to little more than
             the linear-algebra unit
Windows: prior-only (no point, no line, every pre-integration with sum_dt > 10 as imu_ref's m3 does for one: no IMU factor), so
that vpl_ba_debug_linearization returns the prior's share and nothing else; and step_ref's case d behind a general-family prior
of 75 and of 81 dims."""
import functools

import numpy as np

import step_ref as sr
import vplines_slam_amd as v

NF = 11
FAMILIES = ("general", "at_x0", "exact")
LAYOUT = {       # (kind, frame): 0 pose, 1 speed/bias, 2 extrinsic
    21: [(0, 2), (1, 3), (2, 0)],
    48: [(0, f) for f in range(8)],
    51: [(0, f) for f in range(7)] + [(1, 0)],
    63: [(0, f) for f in range(9)] + [(1, 0)],
    66: [(0, f) for f in range(11)],
    75: [(0, f) for f in range(10)] + [(1, 0), (2, 0)],
    81: [(0, f) for f in range(11)] + [(1, 0), (2, 0)],
    111: [(0, f) for f in range(11)] + [(1, f) for f in range(5)],
    117: [(0, f) for f in range(11)] + [(1, f) for f in range(5)] + [(2, 0)],
    171: [(0, f) for f in range(11)] + [(1, f) for f in range(11)] + [(2, 0)],
}
SIZES = tuple(LAYOUT)
PRIORS = tuple("n%d%s" % (n, s) for n in SIZES for s in "us")
BATCHES = {"A": (21, 48, 51, 63, 66, 75), "B": (75, 81, 111), "C": (48, 117, 171)}
for _n, _l in LAYOUT.items():
    assert sum(9 if k == 1 else 6 for k, _ in _l) == _n


def pid_of(n, variant="u"):
    return "n%d%s" % (n, variant)


# ---- quaternions (x, y, z, w), Hamilton product ---------------------------------------------------------------------------
def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def qexp(vec):
    a = np.linalg.norm(vec)
    return np.concatenate([np.sin(a / 2) * np.asarray(vec) / a, [np.cos(a / 2)]])


def _unit(rng):
    u = rng.normal(size=3)
    return u / np.linalg.norm(u)


@functools.lru_cache(maxsize=None)
def hurwitz():
    """the 24 rotations whose quaternion has entries in {0, +-1/2, +-1}, in the sign Quaternion(Matrix3) gives them"""
    out = []
    for k in range(4):
        q = np.zeros(4)
        q[k] = 1.0
        out.append(q)
    for s in range(8):
        out.append(np.array([0.5 if s & 1 else -0.5, 0.5 if s & 2 else -0.5, 0.5 if s & 4 else -0.5, 0.5]))
    out = [sr.R_quat(sr.quat_R(q)) for q in out]
    for q in out:     # fixed points of normalise -> matrix -> quaternion, bit for bit
        assert np.array_equal(sr.R_quat(sr.quat_R(q / np.linalg.norm(q))), q) and set(np.abs(q)) <= {0.0, 0.5, 1.0}
    return out


# ---- priors ---------------------------------------------------------------------------------------------------------------
def make_prior(layout, x0, J, r):
    """x0: one array per block (7 numbers of a pose, 9 of a speed/bias)"""
    p = v.Prior()
    p.n_blocks = len(layout)
    idx = 0
    for b, (kind, fr) in enumerate(layout):
        p.block_kind[b], p.block_frame[b], p.block_idx[b] = kind, fr, idx
        for j, val in enumerate(x0[b]):
            p.x0[b][j] = float(val)
        idx += 9 if kind == 1 else 6
    p.n = idx
    assert J.shape == (idx, idx) and r.shape == (idx,)
    Jf = np.ascontiguousarray(J, np.float64).reshape(-1)
    np.ctypeslib.as_array(p.J0)[:idx * idx] = Jf
    np.ctypeslib.as_array(p.r0)[:idx] = r
    return p


def _J_r(n, variant, rng):
    J = np.triu(rng.normal(size=(n, n))) * 0.5 + np.diag(3.0 + rng.uniform(size=n))
    r = rng.normal(size=n) * 0.1
    if variant == "s":
        s = 10.0 ** rng.uniform(-3.0, 7.0, size=n)
        J, r = s[:, None] * J, s * r
    return J, r


def random_states(rng):
    pose = np.zeros((NF, 7))
    for f in range(NF):
        pose[f, :3] = rng.normal(size=3) * 2.0
        pose[f, 3:] = qexp(_unit(rng) * rng.uniform(0.1, 3.0))
    sb = np.concatenate([rng.normal(size=(NF, 3)), 0.1 * rng.normal(size=(NF, 3)), 0.01 * rng.normal(size=(NF, 3))], axis=1)
    ex = np.concatenate([0.05 * rng.normal(size=3), qexp(_unit(rng) * 0.3)])
    return dict(pose=pose, sb=sb, ex=ex)


def _block(x, kind, fr):
    return x["pose"][fr] if kind == 0 else x["sb"][fr] if kind == 1 else x["ex"]


def general_x0(layout, x, rng):
    """the general family's linearisation points around the states x"""
    out, j, first_sb = [], 0, True
    for kind, fr in layout:
        xb = _block(x, kind, fr).copy()
        if kind == 1:
            d = 0.05 * rng.normal(size=9)
            if first_sb:
                d[::2] = 1e-9 * rng.normal(size=5)
                first_sb = False
            out.append(xb - d)
            continue
        step, ang, scale = 0.05, 0.05 * rng.uniform(0.5, 1.5), 1.0
        if j == 0:
            ang = 2.5
        elif j == 1:
            step, ang = 1e-9, 1e-9
        elif j == 2:
            scale = 1.0 + 1e-6
        elif j == 3:
            ang = 2.0
        q0 = qmul(xb[3:] / np.linalg.norm(xb[3:]), qexp(_unit(rng) * ang)) * scale
        if j % 2 == 1:
            q0 = -q0
        out.append(np.concatenate([xb[:3] - step * rng.normal(size=3), q0]))
        j += 1
    return out


def _dyadic(rng, shape, unit, most):
    k = rng.integers(1, most + 1, size=shape) * rng.choice([-1, 1], size=shape)
    return k * unit


@functools.lru_cache(maxsize=None)
def case(pid, family):
    """-> (Prior, x) with x = dict(pose [11, 7], sb [11, 9], ex [7]) the window's states"""
    n, variant = int(pid[1:-1]), pid[-1]
    layout = LAYOUT[n]
    rng = np.random.default_rng(7000 + 10 * n + (5 if variant == "s" else 0) + FAMILIES.index(family))
    J, r = _J_r(n, variant, np.random.default_rng(8000 + 10 * n + (5 if variant == "s" else 0)))    # one J0, r0 for the three families
    x = random_states(rng)
    if family == "general":
        x0 = general_x0(layout, x, rng)
    elif family == "at_x0":
        hw = hurwitz()
        for f in range(NF):
            x["pose"][f, 3:] = hw[int(rng.integers(len(hw)))]
        x["ex"][3:] = hw[int(rng.integers(len(hw)))]
        x["pose"][0, :3] = 0.0       # the gauge fix on the way out, R (P - P0) + P0 with R = 1, is then exact too
        x0 = [_block(x, kind, fr).copy() for kind, fr in layout]
    else:
        ident = np.array([0.0, 0.0, 0.0, 1.0])
        p0, s0 = _dyadic(rng, (NF + 1, 3), 1.0 / 16, 2), _dyadic(rng, (NF, 9), 1.0 / 16, 2)
        p0[rng.uniform(size=p0.shape) < 0.3] = 0.0
        x["pose"][:, :3] = p0[:NF] + _dyadic(rng, (NF, 3), 1.0 / 32, 6)
        x["ex"][:3] = p0[NF] + _dyadic(rng, 3, 1.0 / 32, 6)
        x["sb"] = s0 + _dyadic(rng, (NF, 9), 1.0 / 32, 6)
        for f in range(NF):
            x["pose"][f, 3:] = qexp(_unit(rng) * rng.uniform(0.05, 0.5))
        x0 = [s0[fr] if kind == 1 else np.concatenate([p0[fr if kind == 0 else NF], ident]) for kind, fr in layout]
    return make_prior(layout, x0, J, r), x


def zero_dx_case(pid):
    """the prior's J0 and r0 with identity rotations and zero positions as x0 AND as the window's states: another upload with
    dx exactly 0, whose g has to be the at_x0 family's bit for bit (g0 does not depend on x0)"""
    n, variant = int(pid[1:-1]), pid[-1]
    prior, _ = case(pid, "at_x0")
    x = dict(pose=np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (NF, 1)), sb=np.zeros((NF, 9)), ex=np.array([0, 0, 0, 0, 0, 0, 1.0]))
    return make_prior(LAYOUT[n], [_block(x, kind, fr).copy() for kind, fr in LAYOUT[n]], prior.J(), prior.r()), x


# ---- windows --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bare():
    return sr._generate(0, 0, False, 0)[0]


def window(prior, x):
    """a window whose only residual block is the prior: no point, no line, no IMU factor (sum_dt > 10)"""
    w = _bare().copy()
    w.pose[:], w.speed_bias[:], w.ex_pose[:] = x["pose"], x["sb"], x["ex"]
    for j in range(1, NF):
        w.preint[j].sum_dt = 10.5
    w.prior = prior
    return w


def states_of(w):
    return dict(pose=w.pose.copy(), sb=w.speed_bias.copy(), ex=w.ex_pose.copy())


@functools.lru_cache(maxsize=None)
def around(n, base, variant="u"):
    """a general-family prior of n dims around the states of step_ref's case `base` (a: no landmark, d: 37 points + 11 lines)"""
    w = sr.cases()[base][0]
    rng = np.random.default_rng(9000 + n)
    J, r = _J_r(n, variant, rng)
    return make_prior(LAYOUT[n], general_x0(LAYOUT[n], states_of(w), rng), J, r)


def landmark_window(n):
    w = sr.cases()["d"][0].copy()
    w.prior = around(n, "d")
    return w


@functools.lru_cache(maxsize=None)
def step_window(which):
    """the windows one iteration is run on: "n171u_step" the prior-only window of n = 171 (exact family: the general path, every
    state pinned by the prior), "n75u_imu_step" step_ref's case a -- IMU factors on, no landmark -- behind a prior of 75 dims"""
    if which == "n171u_step":
        prior, x = case("n171u", "exact")
        return window(prior, x), sr._options()
    assert which == "n75u_imu_step"
    w = sr.cases()["a"][0].copy()
    w.prior = around(75, "a")
    return w, sr._options()
