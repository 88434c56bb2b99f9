"""IMU pre-integration in np.longdouble -- the reference test_preint_reference.py checks against the oracle and the device math on
the CPU, and test_gpu_preint.py holds vpl_preintegrate_batch to.

Written from the formulas of IntegrationBase (integration_base.h): the constructor and the noise matrix (:14-28), push_back
(:30-36), midPointIntegration (:54-168) and propagate (:170-198).  Dense 15 x 15 F, 15 x 18 V and 18 x 18 Q exactly as those lines
spell them -- deliberately unlike the kernel's block-sparse, lane-spread form -- delta_q normalised after every sample, acc_0 /
gyr_0 carried from sample to sample.  Quaternions are (w, x, y, z) here, as Eigen spells them; the ABI's delta_q is (x, y, z, w)
(`abi_q`).  Rows and columns of J and P: P 0..2, R 3..5, V 6..8, BA 9..11, BG 12..14.

Units.  Beside the values, `step` carries the forward-error recursion in absolute values:
  U_J <- |F| U_J + |F| |J|,        U_P <- |F| U_P |F|^T + |F| |P| |F|^T + |V| Q |V|^T        (J, P: the values before the step)
and for the deltas the absolute values of their summands, step after step:
  A   = (|Rq| (|a0| + |ba|) + |Rr| (|a1| + |ba|)) / 2                    the summands of un_acc
  U_p <- U_p + |dp| + dt |dv| + dt^2 A / 2
  U_v <- U_v + |dv| + dt A
  U_q <- U_q + max(|dq| (x) |r|) + max |rq|                              the product's summands, and the normalisation
The unit of an output entry is eps64 times that quantity -- the eps sum |terms| convention of step_ref.py and vis_ref.py -- formed
per 3 x 3 block (the largest of the block) for J and P and per vector for the deltas: a rotation matrix' small entries carry the
rounding of its large ones.  An ENTRY whose own recursion is 0 is a structural zero and must be exactly 0.0 (rows 9..14 of J off
the identity, the bias blocks of P off the diagonal, dq_dba); where a whole unit is 0 (the empty interval) the value is exact.

Bar: the suite's 32 units for every implementation, the device included; it holds only while every CPU implementation of YARDSTICK
(the float64 run of this restatement, orc_preintegrate, hc_preintegrate, each against the long-double run) stays below 8 units on
every case of preint_inputs.py.  `python tests/preint_ref.py` prints the table YARDSTICK was copied from, the scan of the
difference step h of check (a) and the halving ratios of checks (a) and (b).

Independent checks of the formulas (long double, test_preint_reference.py):
  (a) `bias_gap`: rows P, R, V of columns 9..14 of J against central differences of (delta_p, delta_q, delta_v) re-integrated at
      ba +- h, bg +- h, the rotation rows through 2 vec(dq(-h)^-1 (x) dq(+h)) / 2h.  h = 1e-6: the long-double difference quotient
      is flat from 1e-4 down to 1e-8 (relative changes below 3e-10; 2e-9 at 1e-3, 1e-8 at 1e-9; the scan is printed by __main__).
  (b) `noise_gap`: G [15, 18 n] by central differences of the final state under additive perturbations of a0, g0, a1, g1 of ONE
      step and of the two bias walks entering as dt n (the biases of the LATER steps and the final bias rows move);
      sum_k G_k Q G_k^T against P, per block, relative to the block.
F is the reference's first-order linearisation: both agree in the limit dt -> 0 only, so one continuous motion is sampled at dt,
dt / 2 and dt / 4 over the same span and every block's gap has to shrink."""
import ctypes as C
import functools

import numpy as np

import imu_ref as ir
import step_ref as sr
import vplines_slam_amd as v

LD = sr.LD
EPS64 = sr.EPS64
BAR = 32.0              # units; what every implementation, the device included, is held to
CPU_BAR = 8.0           # what the CPU implementations of YARDSTICK have to stay below for BAR to stand
H_FD = 1e-6


def noise_of(opt):
    return (opt.acc_n, opt.gyr_n, opt.acc_w, opt.gyr_w)


def noise_matrix(noise, dt):
    """:21-27, the 18 x 18 Q: (acc_n^2, gyr_n^2, acc_n^2, gyr_n^2, acc_w^2, gyr_w^2) x I3"""
    an, gn, aw, gw = (dt(x) for x in noise)
    Q = np.zeros((18, 18), dt)
    for b, s in enumerate((an, gn, an, gn, aw, gw)):
        Q[3 * b:3 * b + 3, 3 * b:3 * b + 3] = (s * s) * np.eye(3, dtype=dt)
    return Q


class State:
    """what IntegrationBase holds between two push_backs (:14-18), in dtype dt, and the recursions of the units"""

    def __init__(self, dt=LD):
        self.dt = dt
        self.sum_dt = dt(0)
        self.dp, self.dv = np.zeros(3, dt), np.zeros(3, dt)
        self.dq = np.array([1, 0, 0, 0], dt)
        self.J, self.P = np.eye(15, dtype=dt), np.zeros((15, 15), dt)
        self.UJ, self.UP = np.zeros((15, 15)), np.zeros((15, 15))
        self.Up, self.Uv, self.Uq = np.zeros(3), np.zeros(3), 0.0
        self.n = 0
        self.abs_dt = 0.0


def _f64(a):
    return np.abs(np.asarray(a)).astype(np.float64)


def step(s, dt, a0, g0, a1, g1, ba, bg, Q, units=True, mutate=None):
    """propagate (:170-198) with midPointIntegration (:54-168) on the state s, in place.  (a0, g0): the previous measurement,
    (a1, g1): the new one -- four separate arguments (check (b) perturbs one of them in one step only).  mutate: a misreading
    applied to THIS restatement, for the sharpness test of checks (a) and (b)"""
    T = s.dt
    dt = T(dt)
    a0, g0, a1, g1, ba, bg = (np.asarray(x, T) for x in (a0, g0, a1, g1, ba, bg))
    half = T(1) / 2
    # :63-69
    un_acc_0 = ir.qrot(s.dq, a0 - ba)
    un_gyr = half * (g0 + g1) - bg
    rq = ir.qmul(s.dq, np.concatenate([[T(1)], un_gyr * dt / 2]))
    un_acc_1 = ir.qrot(rq, a1 - ba)
    un_acc = half * (un_acc_0 + un_acc_1)
    rp = s.dp + s.dv * dt + half * un_acc * dt * dt
    rv = s.dv + un_acc * dt
    # :75-88
    R_w_x, R_a_0_x, R_a_1_x = ir.skew(un_gyr), ir.skew(a0 - ba), ir.skew(a1 - ba)
    Rq, Rr = ir.qmat(s.dq), ir.qmat(rq)
    I3 = np.eye(3, dtype=T)
    ImW = I3 - R_w_x * dt
    if mutate == "no_ImW":
        ImW = I3
    q4, h2 = T(1) / 4, half
    # :90-110
    F = np.zeros((15, 15), T)
    F[0:3, 0:3] = I3
    F[0:3, 3:6] = -q4 * Rq @ R_a_0_x * dt * dt + -q4 * Rr @ R_a_1_x @ ImW * dt * dt
    F[0:3, 6:9] = I3 * dt
    F[0:3, 9:12] = -q4 * (Rq + Rr) * dt * dt
    F[0:3, 12:15] = -q4 * Rr @ R_a_1_x * dt * dt * -dt
    F[3:6, 3:6] = I3 - R_w_x * dt
    F[3:6, 12:15] = -1 * I3 * dt
    F[6:9, 3:6] = -h2 * Rq @ R_a_0_x * dt + -h2 * Rr @ R_a_1_x @ ImW * dt
    F[6:9, 6:9] = I3
    F[6:9, 9:12] = -h2 * (Rq + Rr) * dt
    F[6:9, 12:15] = -h2 * Rr @ R_a_1_x * dt * -dt
    F[9:12, 9:12] = I3
    F[12:15, 12:15] = I3
    if mutate == "dp_dbg_sign":       # a dt^3 term
        F[0:3, 12:15] = -F[0:3, 12:15]
    if mutate == "dtheta_dbg_sign":   # a first-order term
        F[3:6, 12:15] = -F[3:6, 12:15]
    if mutate == "dv_dba_block":      # a first-order term in the wrong block column
        F[6:9, 12:15], F[6:9, 9:12] = F[6:9, 9:12].copy(), F[6:9, 12:15].copy()
    # :113-125
    V = np.zeros((15, 18), T)
    V[0:3, 0:3] = q4 * Rq * dt * dt
    V[0:3, 3:6] = q4 * -Rr @ R_a_1_x * dt * dt * half * dt
    V[0:3, 6:9] = q4 * Rr * dt * dt
    V[0:3, 9:12] = V[0:3, 3:6]
    V[3:6, 3:6] = half * I3 * dt
    V[3:6, 9:12] = half * I3 * dt
    V[6:9, 0:3] = half * Rq * dt
    V[6:9, 3:6] = half * -Rr @ R_a_1_x * dt * half * dt
    V[6:9, 6:9] = half * Rr * dt
    V[6:9, 9:12] = V[6:9, 3:6]
    V[9:12, 12:15] = I3 * dt
    V[12:15, 15:18] = I3 * dt
    if mutate == "b_sign":            # the sign of the dt^3 / 8 term (the kernel's `b`)
        V[0:3, 3:6] = -V[0:3, 3:6]
        V[0:3, 9:12] = -V[0:3, 9:12]
    if mutate == "one_gn":            # the second gyroscope sample's share of the position noise lost (the kernel's 2 gn2 -> gn2)
        V[0:3, 9:12] = 0
    if units:
        aF, aV = _f64(F), _f64(V)
        Q64 = np.asarray(Q, np.float64)
        s.UJ = aF @ s.UJ + aF @ _f64(s.J)
        s.UP = aF @ s.UP @ aF.T + aF @ _f64(s.P) @ aF.T + aV @ Q64 @ aV.T
        A = 0.5 * (_f64(Rq) @ (_f64(a0) + _f64(ba)) + _f64(Rr) @ (_f64(a1) + _f64(ba)))
        d = float(abs(dt))
        s.Up = s.Up + _f64(s.dp) + d * _f64(s.dv) + 0.5 * d * d * A
        s.Uv = s.Uv + _f64(s.dv) + d * A
        s.Uq = s.Uq + float(_f64(ir.qmul(np.abs(s.dq), np.abs(np.concatenate([[T(1)], un_gyr * dt / 2])))).max()) + float(_f64(rq).max())
    # :164-165
    s.J = F @ s.J
    s.P = F @ s.P @ F.T + V @ Q @ V.T
    # :188-196
    s.dp, s.dv = rp, rv
    s.dq = rq / np.sqrt(rq @ rq)
    s.sum_dt = s.sum_dt + dt
    s.n += 1
    s.abs_dt += float(abs(dt))
    return s


def _block_max(U):
    out = np.zeros_like(U)
    for i in range(0, 15, 3):
        for j in range(0, 15, 3):
            out[i:i + 3, j:j + 3] = U[i:i + 3, j:j + 3].max()
    return out


class Result:
    """the outputs of one interval in dtype dt, with the units (float64) where they were carried"""

    def __init__(self, s, ba, bg):
        self.sum_dt, self.dp, self.dv, self.dq, self.J, self.P = s.sum_dt, s.dp, s.dv, s.dq, s.J, s.P
        self.lba, self.lbg = np.asarray(ba, np.float64), np.asarray(bg, np.float64)
        self.n = s.n
        self.unit_dp, self.unit_dv, self.unit_dq = EPS64 * s.Up.max(), EPS64 * s.Uv.max(), EPS64 * s.Uq
        self.unit_J, self.unit_P = EPS64 * _block_max(s.UJ), EPS64 * _block_max(s.UP)
        self.zero_J, self.zero_P = s.UJ == 0, s.UP == 0          # entrywise: structural zeros (of J: off the identity)
        self.unit_sum_dt = s.n * EPS64 * s.abs_dt

    @property
    def abi_q(self):
        return np.array([self.dq[1], self.dq[2], self.dq[3], self.dq[0]], self.dq.dtype)


def integrate(samples, acc0, gyr0, ba, bg, noise, dt=LD, units=True, mutate=None):
    """the constructor (:14-28) and push_back (:30-36) over samples [n][7] = (dt, acc, gyr)"""
    samples = np.asarray(samples, np.float64).reshape(-1, 7).astype(dt)
    s = State(dt)
    Q = noise_matrix(noise, dt)
    a0, g0 = np.asarray(acc0, np.float64).astype(dt), np.asarray(gyr0, np.float64).astype(dt)
    ba, bg = np.asarray(ba, np.float64).astype(dt), np.asarray(bg, np.float64).astype(dt)
    for row in samples:
        step(s, row[0], a0, g0, row[1:4], row[4:7], ba, bg, Q, units, mutate)
        a0, g0 = row[1:4], row[4:7]                             # :195-196
    return Result(s, ba, bg)


# ---- an implementation's output against the long-double run, in units -----------------------------------------------------
class Out:
    """what an implementation returned for one interval (a vpl_preintegration), as arrays"""

    def __init__(self, p):
        a = lambda f: np.array(getattr(p, f), np.float64)
        self.sum_dt = float(p.sum_dt)
        self.dp, self.dv, self.q = a("delta_p"), a("delta_v"), a("delta_q")           # q: x, y, z, w
        self.J, self.P = a("jacobian").reshape(15, 15), a("covariance").reshape(15, 15)
        self.lba, self.lbg = a("linearized_ba"), a("linearized_bg")

    @classmethod
    def of(cls, r):
        """a Result of the restatement (float64 run) in the same form"""
        o = cls.__new__(cls)
        o.sum_dt = float(r.sum_dt)
        o.dp, o.dv, o.q = (np.asarray(x, np.float64) for x in (r.dp, r.dv, r.abi_q))
        o.J, o.P, o.lba, o.lbg = np.asarray(r.J, np.float64), np.asarray(r.P, np.float64), r.lba, r.lbg
        return o


def _ratio(x, ref, unit):
    """max |x - ref| / unit over an array with one unit or an array of them; unit 0: equal bit for bit"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref)
    unit = np.broadcast_to(np.asarray(unit, np.float64), x.shape)
    z = unit == 0
    assert np.array_equal(x[z], np.asarray(ref[z], np.float64)), "an exact entry (unit 0) differs"
    if z.all():
        return 0.0
    return float((np.abs(np.asarray(x, LD) - ref)[~z] / unit[~z]).max())


def errors(out, ref):
    """-> dict of the worst error, in units, of dp, dq, dv, J, P (and `asym`: |P - P^T| of `out` in P's units); asserts the
    structural zeros and sum_dt"""
    assert np.all(out.J[ref.zero_J] == np.eye(15)[ref.zero_J]), "a structural zero of the jacobian (or a one of the identity) is not exact"
    assert np.all(out.P[ref.zero_P] == 0.0), "a structural zero of the covariance is not exact"
    assert abs(LD(out.sum_dt) - ref.sum_dt) <= ref.unit_sum_dt, "sum_dt"
    e = dict(dp=_ratio(out.dp, ref.dp, ref.unit_dp), dq=_ratio(out.q, ref.abi_q, ref.unit_dq),
             dv=_ratio(out.dv, ref.dv, ref.unit_dv), J=_ratio(out.J, ref.J, ref.unit_J), P=_ratio(out.P, ref.P, ref.unit_P))
    e["asym"] = _ratio(out.P - out.P.T, np.zeros((15, 15), LD), ref.unit_P + ref.unit_P.T)
    return e


def worst(e):
    return max(e[k] for k in ("dp", "dq", "dv", "J", "P"))


# ---- the CPU implementations (yardstick) ------------------------------------------------------------------------------------
def _P(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def options(noise):
    opt = v.default_options()
    opt.acc_n, opt.gyr_n, opt.acc_w, opt.gyr_w = noise
    return opt


def _call(fn, c):
    out = v.Preintegration()
    arr = [np.ascontiguousarray(c[k], np.float64) for k in ("samples", "acc0", "gyr0", "ba", "bg")]
    s = arr[0] if len(arr[0]) else np.zeros((1, 7))
    opt = options(c["noise"])
    fn(len(arr[0]), _P(s), _P(arr[1]), _P(arr[2]), _P(arr[3]), _P(arr[4]), C.byref(opt), C.byref(out))
    return Out(out)


def run_oracle(c):
    import oracle_api as o
    return _call(o.load().orc_preintegrate, c)


def run_hostcheck(c, lib):
    """vpl_preint.h::preint_step compiled for the host (test_golden's hostcheck fixture): a third float64 implementation, NOT the
    lane-spread preint_steps the device runs"""
    return _call(lib.hc_preintegrate, c)


def run_f64(c):
    return Out.of(integrate(c["samples"], c["acc0"], c["gyr0"], c["ba"], c["bg"], c["noise"], np.float64, units=False))


@functools.lru_cache(maxsize=None)
def reference(name):
    """the long-double run of a case of preint_inputs.py, computed once and shared"""
    import preint_inputs as pi
    c = pi.cases()[name]
    return integrate(c["samples"], c["acc0"], c["gyr0"], c["ba"], c["bg"], c["noise"], LD)


def measure(lib=None):
    """case -> dict(f64=, oracle=, hostcheck=): the worst error in units of each CPU implementation against long double"""
    import preint_inputs as pi
    out = {}
    for name, c in pi.cases().items():
        ref = reference(name)
        row = dict(f64=worst(errors(run_f64(c), ref)), oracle=worst(errors(run_oracle(c), ref)))
        if lib is not None:
            row["hostcheck"] = worst(errors(run_hostcheck(c, lib), ref))
        out[name] = row
    return out


# ---- check (a): the bias columns of J against central differences --------------------------------------------------------------
def _dtheta(qm, qp):
    """2 vec(qm^-1 (x) qp)"""
    return 2 * ir.qmul(ir.qinv(qm), qp)[1:]


def bias_fd(c, h=H_FD, mutate=None):
    """[9, 6]: d (delta_p, theta, delta_v) / d (ba, bg) by central differences of the restatement, long double"""
    D = np.zeros((9, 6), LD)
    for k in range(6):
        e = np.zeros(6, LD)
        e[k] = LD(h)
        run = lambda sgn: integrate(c["samples"], c["acc0"], c["gyr0"], np.asarray(c["ba"], LD) + sgn * e[:3],
                                    np.asarray(c["bg"], LD) + sgn * e[3:], c["noise"], LD, units=False, mutate=mutate)
        m, p = run(-1), run(+1)
        D[0:3, k], D[3:6, k], D[6:9, k] = (p.dp - m.dp) / (2 * e[k]), _dtheta(m.dq, p.dq) / (2 * e[k]), (p.dv - m.dv) / (2 * e[k])
    return D


BIAS_BLOCKS = {"p_ba": (0, 0), "p_bg": (0, 3), "r_ba": (3, 0), "r_bg": (3, 3), "v_ba": (6, 0), "v_bg": (6, 3)}


def bias_gap(c, h=H_FD, mutate=None):
    """block -> max |J - central difference| / max |central difference| over the block (a block of zeros: the absolute gap)"""
    r = integrate(c["samples"], c["acc0"], c["gyr0"], c["ba"], c["bg"], c["noise"], LD, units=False, mutate=mutate)
    fd = bias_fd(c, h, mutate)
    d = np.abs(r.J[0:9, 9:15] - fd)
    out = {}
    for k, (i, j) in BIAS_BLOCKS.items():
        scale = float(np.abs(fd[i:i + 3, j:j + 3]).max())
        out[k] = float(d[i:i + 3, j:j + 3].max()) / (scale if scale > 1e-9 else 1.0)
    return out


FD_FLOOR = 1e-9     # what the difference quotients themselves are good for, relative (the scan of h: flat to 4e-11 around 1e-6)


def halves(g):
    """the criterion of checks (a) and (b) on a block's gaps at dt, dt / 2, dt / 4: "exact" where the formula IS the derivative
    (linear dependence: all three at the quotient's floor), else each halving shrinks the gap by at least 1.5 and the last is
    below the first.  A wrong sign, block or density leaves a gap of O(1) that does not shrink"""
    if max(g) <= FD_FLOOR:
        return "exact"
    return "shrinks" if g[0] >= 1.5 * g[1] and g[1] >= 1.5 * g[2] and g[2] < g[0] else "stays"


# ---- check (b): V and the layout of the noise against central differences ------------------------------------------------------
def _final(c, k, col, amount):
    """the final (dp, dq, dv, ba_end - ba, bg_end - bg) with noise component `col` (0..17) of step k set to `amount`: additive on
    a0, g0, a1, g1 of that step alone; the bias walks move the biases by dt n AFTER the step (V's dt I, :124-125)"""
    smp = np.asarray(c["samples"], np.float64).astype(LD)
    s = State(LD)
    Q = noise_matrix(c["noise"], LD)
    a0, g0 = np.asarray(c["acc0"], LD), np.asarray(c["gyr0"], LD)
    b = np.concatenate([np.asarray(c["ba"], LD), np.asarray(c["bg"], LD)])
    b0 = b.copy()
    for i, row in enumerate(smp):
        m = [a0, g0, row[1:4], row[4:7]]
        if i == k and col < 12:
            m[col // 3] = m[col // 3].copy()
            m[col // 3][col % 3] += amount
        step(s, row[0], m[0], m[1], m[2], m[3], b[:3], b[3:], Q, units=False)
        if i == k and col >= 12:
            b = b.copy()
            b[col - 12] += row[0] * amount
        a0, g0 = row[1:4], row[4:7]
    return s.dp, s.dq, s.dv, b - b0


def noise_cov(c, h=H_FD):
    """sum_k G_k Q G_k^T [15, 15], G by central differences, long double"""
    n = len(c["samples"])
    Q = noise_matrix(c["noise"], LD)
    S = np.zeros((15, 15), LD)
    h = LD(h)
    for k in range(n):
        G = np.zeros((15, 18), LD)
        for col in range(18):
            hh = h * LD(1e3) if col >= 12 else h          # the walks enter scaled by dt
            m, p = _final(c, k, col, -hh), _final(c, k, col, +hh)
            G[0:3, col], G[3:6, col], G[6:9, col] = (p[0] - m[0]) / (2 * hh), _dtheta(m[1], p[1]) / (2 * hh), (p[2] - m[2]) / (2 * hh)
            G[9:15, col] = (p[3] - m[3]) / (2 * hh)
        S += G @ Q @ G.T
    return S


def noise_gap(c, S=None, mutate=None, noise=None):
    """[5, 5]: per 3 x 3 block, max |P - S| / max |P|, S = sum G Q G^T (noise_cov(c), computed here if not handed in); P = 0
    blocks: the absolute gap.  mutate / noise: a misreading of V, or other densities, on P's side only"""
    r = integrate(c["samples"], c["acc0"], c["gyr0"], c["ba"], c["bg"], noise or c["noise"], LD, units=False, mutate=mutate)
    S = noise_cov(c) if S is None else S
    g = np.zeros((5, 5))
    for i in range(5):
        for j in range(5):
            a, b = r.P[3 * i:3 * i + 3, 3 * j:3 * j + 3], S[3 * i:3 * i + 3, 3 * j:3 * j + 3]
            scale = float(np.abs(a).max())
            g[i, j] = float(np.abs(a - b).max()) / (scale if scale > 0 else 1.0)
    return g


# Worst error of the CPU implementations against the long-double run, in the units above (`python tests/preint_ref.py` prints
# this table; all below CPU_BAR = 8, which is what lets BAR = 32 stand).
YARDSTICK = {
    "n0": dict(f64=0, oracle=0, hostcheck=0),
    "n1": dict(f64=1.2, oracle=1.2, hostcheck=1.2),
    "n2": dict(f64=0.801, oracle=0.801, hostcheck=0.801),
    "n3": dict(f64=0.556, oracle=0.556, hostcheck=0.556),
    "n19": dict(f64=0.358, oracle=0.318, hostcheck=0.318),
    "n20": dict(f64=0.396, oracle=0.499, hostcheck=0.499),
    "n37_jitter": dict(f64=0.208, oracle=0.22, hostcheck=0.22),
    "n64": dict(f64=0.225, oracle=0.207, hostcheck=0.207),
    "n20_dt0": dict(f64=0.47, oracle=0.394, hostcheck=0.394),
    "n64_long": dict(f64=0.0803, oracle=0.0707, hostcheck=0.0707),
    "n20_fast": dict(f64=0.371, oracle=0.371, hostcheck=0.371),
    "n64_fast": dict(f64=0.153, oracle=0.153, hostcheck=0.153),
    "n37_rot": dict(f64=0.341, oracle=0.363, hostcheck=0.363),
    "n20_fall": dict(f64=0.228, oracle=0.228, hostcheck=0.228),
    "n3_fast_jitter": dict(f64=0.756, oracle=0.794, hostcheck=0.794),
    "default20": dict(f64=0.261, oracle=0.261, hostcheck=0.261),
}


if __name__ == "__main__":
    import preint_inputs as pi
    import test_golden
    lib = test_golden.build_hostcheck()
    for name, y in measure(lib).items():
        print('    "%s": dict(f64=%.3g, oracle=%.3g, hostcheck=%.3g),' % (name, y["f64"], y["oracle"], y["hostcheck"]))
    c = pi.halving()[0]
    print("scan of h, check (a): max |d/dh-quotient(h) - quotient(1e-6)| / max |quotient(1e-6)|")
    d0 = bias_fd(c, 1e-6)
    for h in (1e-2, 1e-3, 1e-4, 1e-5, 1e-7, 1e-8, 1e-9, 1e-10, 1e-12):
        print("  h = %-6g %.3g" % (h, float(np.abs(bias_fd(c, h) - d0).max() / np.abs(d0).max())))
    ga = [bias_gap(x) for x in pi.halving()]
    print("check (a): gap at dt, dt/2, dt/4 and the two ratios")
    for k in BIAS_BLOCKS:
        g = [x[k] for x in ga]
        print("  %-5s %.3g %.3g %.3g   %s" % (k, g[0], g[1], g[2], "exact" if halves(g) == "exact" else "%.2f %.2f" % (g[0] / g[1], g[1] / g[2])))
    gb = [noise_gap(x) for x in pi.halving_noise()]
    print("check (b): relative gap per block of P at dt, dt/2, dt/4 and the two ratios")
    names = "P R V BA BG".split()
    for i in range(5):
        for j in range(i, 5):
            g = [x[i, j] for x in gb]
            print("  %-2s %-2s %.3g %.3g %.3g   %s" % (names[i], names[j], g[0], g[1], g[2],
                                                    "exact" if halves(g) == "exact" else "%.2f %.2f" % (g[0] / g[1], g[1] / g[2])))
