"""Named pose chains for the tests of vpl_gf_optimize_batch and of its restatement tests/gf_ref.py.

Every chain is a ground-truth trajectory (a circle walked `turns` times with a slow climb, small pitch and roll), the local (VIO)
poses = the truth with a drift in yaw and position that grows along the chain, the initial global poses = the local ones moved by
one rigid transform (what inputOdom makes of them under the WGPS_T_WVIO of the moment), and GNSS fixes = the truth plus noise.
The inputs are chosen so that every decision of the minimiser is far from its threshold (tests/test_gf_reference.py checks 1e-6
relative).  The shape cases run at S = 4."""
import functools

import numpy as np

import gf_ref


def _quat(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    return np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy])


def make_chain(n, fixes, seed, turns=0.4, radius=8.0, yaw_drift=0.004, t_drift=(0.02, -0.015, 0.003), noise=0.05, accuracy=0.5,
               frame_yaw=0.0, frame_shift=(0.0, 0.0, 0.0), opt=None, segment=4):
    """fixes: the nodes with a GNSS fix.  yaw_drift in radians per node, t_drift in metres per node, frame_yaw in radians"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    ang = 2 * np.pi * turns * k / max(n - 1, 1)
    truth_p = np.stack([radius * np.cos(ang), radius * np.sin(ang), 0.05 * k + 0.2 * np.sin(3 * ang)], axis=1)
    pitch, roll = rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n)
    local = np.zeros((n, 7))
    local[0, :3] = truth_p[0]
    for i in range(1, n):   # the truth's steps, each turned by the yaw error of where it starts, plus a drift per node
        c, s = np.cos(yaw_drift * (i - 1)), np.sin(yaw_drift * (i - 1))
        local[i, :3] = local[i - 1, :3] + np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]).dot(truth_p[i] - truth_p[i - 1]) + np.asarray(t_drift)
    local[:, :3] += rng.normal(0, 1e-3, (n, 3))
    for i in range(n):
        local[i, 3:] = _quat(ang[i] + np.pi / 2 + yaw_drift * i, pitch[i], roll[i])
    fq = _quat(frame_yaw, 0.0, 0.0)
    fR = gf_ref.qmat(fq)
    glob = np.zeros((n, 7))
    glob[:, :3] = local[:, :3].dot(fR.T) + np.asarray(frame_shift)
    for i in range(n):
        glob[i, 3:] = gf_ref.qmul(fq, local[i, 3:])
    fixes = sorted(int(f) for f in fixes)
    xyz = truth_p[fixes] + rng.normal(0, noise, (len(fixes), 3)) if fixes else np.zeros((0, 3))
    o = dict(segment=segment)
    o.update(opt or {})
    return dict(local=local, glob=glob, gps_node=np.array(fixes, dtype=np.int32), gps_xyz=xyz,
                gps_accuracy=np.full(len(fixes), float(accuracy)), opt=o)


def _outlier():
    g = make_chain(24, range(0, 24, 3), 11)
    g["gps_xyz"][4] += np.array([30.0, -40.0, 15.0])
    return g


def _reject(max_iterations=8):
    # a start far from the fixes and a decrease ratio the first steps miss: rejections, then an acceptance
    g = make_chain(20, range(0, 20, 2), 12, turns=1.0, frame_yaw=np.pi / 2, frame_shift=(50.0, 0.0, 0.0), accuracy=0.2)
    g["opt"].update(min_relative_decrease=0.9, max_iterations=max_iterations)
    return g


CASES = {
    # ---- shapes, at S = 4
    "n1": lambda: make_chain(1, [], 1),
    "n1_fix": lambda: make_chain(1, [0], 2, t_drift=(0.3, 0.2, 0.1)),
    "n2": lambda: make_chain(2, [1], 3),
    "n3": lambda: make_chain(3, [0, 2], 4),                               # one segment
    "n4": lambda: make_chain(4, [0, 3], 5),                               # the first separator is also the last node
    "n5": lambda: make_chain(5, [1, 4], 6),
    "n8": lambda: make_chain(8, [0, 3, 7], 7),
    "n9": lambda: make_chain(9, [2, 5, 8], 8),
    "n41": lambda: make_chain(41, range(0, 41, 5), 9, turns=0.9),         # a ragged last segment
    # ---- the fixes, the trajectory, the options
    "fix_places": lambda: make_chain(14, [0, 2, 3, 4, 13], 13),           # beside a separator, on one, behind one, node 0 and n-1
    "fix_everywhere": lambda: make_chain(12, range(12), 14),
    "single_fix": lambda: make_chain(12, [5], 15),                        # rotation about it is held by the LM diagonal only
    "no_fix": lambda: make_chain(12, [], 16),                             # zero cost: the gradient tolerance at iteration 0
    "all_inside": lambda: make_chain(16, range(0, 16, 3), 17, t_drift=(0.004, -0.003, 0.001), yaw_drift=0.001, noise=0.02, accuracy=2.0),
    "all_outside": lambda: make_chain(16, range(0, 16, 3), 18, t_drift=(0.2, -0.15, 0.05), noise=0.01, accuracy=0.05,
                                      frame_shift=(1.0, 0.5, 0.2)),
    "outlier": _outlier,
    "turning": lambda: make_chain(40, range(0, 40, 4), 19, turns=1.3),    # more than 360 degrees
    "yawed_frame": lambda: make_chain(24, range(0, 24, 3), 20, turns=0.7, frame_yaw=np.pi / 2, frame_shift=(50.0, 0.0, 0.0)),
    "reject": _reject,
    "no_convergence": lambda: make_chain(30, range(0, 30, 5), 21, turns=1.0, yaw_drift=0.02, t_drift=(0.1, -0.08, 0.02), accuracy=0.1),
    "ftol": lambda: make_chain(16, range(0, 16, 3), 22, t_drift=(0.0004, -0.0003, 0.0001), yaw_drift=0.0001, noise=0.02, accuracy=1.0),
    "ptol": lambda: make_chain(16, range(0, 16, 3), 23, t_drift=(0.0004, -0.0003, 0.0001), yaw_drift=0.0001, noise=0.02, accuracy=1.0,
                               opt=dict(function_tolerance=0.0, parameter_tolerance=1e-4)),
    "default_segment": lambda: make_chain(2 * gf_ref.DEFAULT_SEGMENT + 3, range(0, 2 * gf_ref.DEFAULT_SEGMENT + 3, 10), 24, turns=1.5,
                                          segment=0),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def ref_case(name, dtype="f64", solver="chain", S=None):
    """the restatement's run of a case; computed once and shared -- callers leave it unchanged"""
    g = case(name)
    dt = np.float64 if dtype == "f64" else np.longdouble
    return gf_ref.optimize(g["local"], g["glob"], g["gps_node"], g["gps_xyz"], g["gps_accuracy"], g["opt"], dt, solver, S)
