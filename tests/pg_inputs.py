"""Named pose graphs for the tests of vpl_pg_optimize_batch and of its restatement tests/pg_ref.py.

Every graph is a ground-truth trajectory (a circle walked `turns` times, small pitch and roll), the VIO poses = the truth with a
drift in yaw and position that grows along the chain, and loop edges measured on the truth (plus noise).  The inputs are chosen so
that every decision of the minimiser is far from its threshold (tests/test_pg_reference.py checks 1e-6 relative)."""
import functools

import numpy as np

import pg_ref


def _ypr2R(y, p, r):
    return pg_ref.ypr2R(np.array([y, p, r], dtype=np.float64))


def make_graph(n, loops, seed, turns=0.9, yaw_drift=0.4, t_drift=(0.03, -0.02, 0.004), noise=0.0, radius=6.0, n_tail=0, twist=None):
    """loops: list of (node, old node).  yaw_drift in degrees per node, t_drift in metres per node; twist(k) = extra yaw error of
    node k in degrees"""
    rng = np.random.default_rng(seed)
    N = n + n_tail
    k = np.arange(N)
    ang = 360.0 * turns * k / max(n - 1, 1)
    gt_yaw = (ang + 90.0 + 180.0) % 360.0 - 180.0
    gt_t = np.stack([radius * np.cos(np.radians(ang)), radius * np.sin(np.radians(ang)), 0.2 * np.sin(np.radians(3 * ang))], axis=1)
    pitch, roll = rng.uniform(-3, 3, N), rng.uniform(-3, 3, N)
    err = yaw_drift * k + (np.array([twist(i) for i in k]) if twist else 0.0)
    vio_R = np.array([_ypr2R(gt_yaw[i] + err[i], pitch[i], roll[i]) for i in range(N)])
    vio_T = np.zeros((N, 3))   # the truth's steps, each turned by the yaw error of where it starts, plus a drift per node
    vio_T[0] = gt_t[0]
    for i in range(1, N):
        vio_T[i] = vio_T[i - 1] + _ypr2R(err[i - 1], 0.0, 0.0).dot(gt_t[i] - gt_t[i - 1]) + np.asarray(t_drift)
    vio_T += rng.normal(0, 1e-3, (N, 3))
    loop_local = -np.ones(n, dtype=np.int32)
    loop_info = np.zeros((n, 8))
    loop_info[:, 3] = 1.0
    for (i, a) in loops:
        Ra = _ypr2R(gt_yaw[a], pitch[a], roll[a])
        loop_local[i] = a
        loop_info[i, :3] = Ra.T.dot(gt_t[i] - gt_t[a]) + rng.normal(0, noise, 3)
        loop_info[i, 7] = pg_ref.norm_angle(np.float64(gt_yaw[i] - gt_yaw[a])) + rng.normal(0, 10 * noise)
    return dict(vio_T=vio_T[:n].copy(), vio_R=vio_R[:n].copy(), loop_local=loop_local, loop_info=loop_info, sequence=None,
                tail_T=vio_T[n:].copy(), tail_R=vio_R[n:].copy(), opt={})


def _outlier():
    g = make_graph(26, [(20, 2), (22, 4), (24, 5), (25, 7)], 11, noise=0.01)
    g["loop_info"][22, :3] += np.array([3.0, -4.0, 1.5])    # metres off
    g["loop_info"][22, 7] = pg_ref.norm_angle(np.float64(g["loop_info"][22, 7] + 120.0))
    return g


def _reject(max_iterations=8):
    # no loss, the second two-thirds of a 20-node circle twisted smoothly by 120 degrees, and a decrease ratio that the second step
    # misses until the radius has shrunk four times: accept, 4 rejections, accept, function tolerance (rho = 1.00009, 0.999775 ..
    # 0.999801, 0.999907 against 0.9999)
    g = make_graph(20, [(19, 0)], 12, turns=1.0, yaw_drift=0.0, t_drift=(0, 0, 0), twist=lambda i: 120.0 * max(0.0, (i - 6.0) / 13.0))
    g["opt"] = dict(huber_delta=0.0, min_relative_decrease=0.9999, max_iterations=max_iterations)
    return g


def _five(yaw_drift, t):
    return make_graph(30, [(22, 1), (24, 3), (26, 4), (28, 7), (29, 9)], 21, turns=1.0, yaw_drift=yaw_drift, t_drift=(t, -t, t / 5))


def _ftol():
    g = make_graph(16, [(13, 1), (15, 3)], 13, yaw_drift=0.002, t_drift=(0.0004, -0.0003, 0.0001), noise=0.02)
    return g


def _mixed_sequence():
    g = make_graph(8, [(7, 1)], 14)
    g["sequence"] = np.array([1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int32)
    return g


CASES = {
    "n1": lambda: make_graph(1, [], 1, n_tail=2),
    "n2": lambda: make_graph(2, [(1, 0)], 2),
    "n5": lambda: make_graph(5, [(4, 1)], 3),
    "n6_loop_to_0": lambda: make_graph(6, [(5, 0)], 4, n_tail=3),
    "n18": lambda: make_graph(18, [(15, 1), (17, 2)], 5),                       # 68 free rows: more than one 64-row tile
    "circle24": lambda: make_graph(24, [(19, 0), (20, 1), (21, 2), (22, 4), (23, 5)], 6, turns=1.0, noise=0.005),   # 20 columns + g
    "n40": lambda: make_graph(40, [(30, 1), (32, 3), (34, 5), (36, 8), (38, 10), (39, 11)], 7, turns=1.0, noise=0.005, n_tail=4),
    "n120": lambda: make_graph(120, [(60 + 3 * k, 2 + 2 * k) for k in range(20)], 16, turns=2.0, yaw_drift=0.1,
                               t_drift=(0.004, -0.003, 0.001), noise=0.003),   # 80 columns: five tiles of S, two work-groups of columns
    "no_loops": lambda: make_graph(12, [], 8),
    "same_old": lambda: make_graph(16, [(13, 2), (14, 2), (15, 4)], 9),
    "three_apart": lambda: make_graph(14, [(9, 6), (13, 1)], 10),
    "yaw_crossing": lambda: make_graph(30, [(24, 12), (29, 17), (27, 3)], 15, turns=2.5, yaw_drift=0.7),
    "outlier": _outlier,
    "reject": _reject,                                  # options of its own
    "no_convergence": lambda: _reject(5),               # the same graph cut off after five iterations, the last four rejected
    "ftol": _ftol,                                      # function tolerance after one step
    "five": lambda: _five(0.08, 0.004),                 # five iterations under the default options
    "ptol": lambda: _five(0.01, 0.0005),                # ends by parameter tolerance
}
UNSUPPORTED = {"mixed_sequence": _mixed_sequence}


@functools.lru_cache(maxsize=None)
def case(name):
    return (CASES.get(name) or UNSUPPORTED[name])()


@functools.lru_cache(maxsize=None)
def ref_case(name, dtype="f64", solver="banded"):
    """the restatement's run of a case; computed once and shared -- callers leave it unchanged"""
    g = case(name)
    dt = np.float64 if dtype == "f64" else np.longdouble
    return pg_ref.optimize(g["vio_T"], g["vio_R"], g["loop_local"], g["loop_info"], g["sequence"], g["tail_T"], g["tail_R"], g["opt"], dt, solver)
