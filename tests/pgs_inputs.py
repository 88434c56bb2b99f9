"""Named pose graphs of several sequences for the tests of vpl_pg_optimize_seq_batch and of its restatement tests/pgs_ref.py.

As in tests/pg_inputs.py every graph is a ground-truth circle; the VIO poses of every run (a stretch of nodes of one sequence) are
the truth with a drift in yaw and position that starts afresh, with a small offset of its own, where the run starts -- a sequence
that has already been shifted into the world frame by its first loop, as PoseGraph::addKeyFrame leaves it.  A run of sequence 0 is
a loaded base map: its poses are the truth.  Loop edges are measured on the truth (plus noise)."""
import functools

import numpy as np

import pg_ref
import pgs_ref
from pg_inputs import _ypr2R


def make_seq_graph(runs, loops, seed, turns=0.9, yaw_drift=0.4, t_drift=(0.03, -0.02, 0.004), noise=0.0, radius=6.0, n_tail=0,
                   start_yaw=1.5, start_t=0.08, twist=None, opt=None):
    """runs: list of (sequence, length); loops: list of (node, old node).  start_yaw (degrees) / start_t (metres): the size of the
    offset a run of a live sequence starts with; twist(k) = extra yaw error of node k in degrees"""
    rng = np.random.default_rng(seed)
    seq = np.concatenate([np.full(ln, s, dtype=np.int32) for s, ln in runs])
    n = len(seq)
    N = n + n_tail
    k = np.arange(N)
    ang = 360.0 * turns * k / max(n - 1, 1)
    gt_yaw = (ang + 90.0 + 180.0) % 360.0 - 180.0
    gt_t = np.stack([radius * np.cos(np.radians(ang)), radius * np.sin(np.radians(ang)), 0.2 * np.sin(np.radians(3 * ang))], axis=1)
    pitch, roll = rng.uniform(-3, 3, N), rng.uniform(-3, 3, N)
    seq_all = np.concatenate([seq, np.full(n_tail, seq[-1], dtype=np.int32)])
    base, err = np.zeros(N), np.zeros(N)   # the yaw error without and with the twist
    vio_T = np.zeros((N, 3))
    for i in range(N):
        if seq_all[i] == 0:
            vio_T[i] = gt_t[i]
            continue
        if i == 0 or seq_all[i] != seq_all[i - 1]:
            base[i] = 0.0 if i == 0 else rng.uniform(-start_yaw, start_yaw)
            vio_T[i] = gt_t[i] + (0.0 if i == 0 else rng.uniform(-start_t, start_t, 3))
        else:
            base[i] = base[i - 1] + yaw_drift
            vio_T[i] = vio_T[i - 1] + _ypr2R(err[i - 1], 0.0, 0.0).dot(gt_t[i] - gt_t[i - 1]) + np.asarray(t_drift)
        err[i] = base[i] + (twist(i) if twist else 0.0)
    vio_R = np.array([_ypr2R(gt_yaw[i] + err[i], pitch[i], roll[i]) for i in range(N)])
    vio_T += rng.normal(0, 1e-3, (N, 3)) * (seq_all != 0)[:, None]
    loop_local = -np.ones(n, dtype=np.int32)
    loop_info = np.zeros((n, 8))
    loop_info[:, 3] = 1.0
    for (i, a) in loops:
        Ra = _ypr2R(gt_yaw[a], pitch[a], roll[a])
        loop_local[i] = a
        loop_info[i, :3] = Ra.T.dot(gt_t[i] - gt_t[a]) + rng.normal(0, noise, 3)
        loop_info[i, 7] = pg_ref.norm_angle(np.float64(gt_yaw[i] - gt_yaw[a])) + rng.normal(0, 10 * noise)
    return dict(vio_T=vio_T[:n].copy(), vio_R=vio_R[:n].copy(), loop_local=loop_local, loop_info=loop_info, sequence=seq,
                tail_T=vio_T[n:].copy(), tail_R=vio_R[n:].copy(), opt=dict(opt or {}))


def _seq_reject(max_iterations=8):
    # tests/pg_inputs.py's `reject` in two sequences: no loss, the later part of the circle twisted smoothly, a decrease ratio the
    # steps miss until the radius has shrunk
    return make_seq_graph([(1, 9), (2, 11)], [(19, 0), (12, 4)], 12, turns=1.0, yaw_drift=0.0, t_drift=(0, 0, 0), start_yaw=0.0, start_t=0.0,
                          twist=lambda i: 120.0 * max(0.0, (i - 6.0) / 13.0),
                          opt=dict(huber_delta=0.0, min_relative_decrease=0.9999, max_iterations=max_iterations))


CASES = {
    "two_seq": lambda: make_seq_graph([(1, 6), (2, 6)], [(9, 2)], 41),
    "two_seq_two_loops": lambda: make_seq_graph([(1, 8), (2, 10)], [(12, 3), (17, 6)], 42, n_tail=3),
    "base_map": lambda: make_seq_graph([(0, 5), (1, 8)], [(4, 0), (8, 1), (11, 3)], 43, n_tail=2),
    "floats": lambda: make_seq_graph([(1, 5), (2, 5), (3, 6)], [(12, 2), (15, 4)], 44),       # the middle sequence has no loop
    "short_runs": lambda: make_seq_graph([(1, 3), (2, 1), (3, 2), (4, 6)], [(3, 1), (5, 2), (9, 0), (11, 4)], 45),
    "two_seq_130": lambda: make_seq_graph([(1, 65), (2, 65)], [(80 + 6 * k, 3 + 5 * k) for k in range(8)], 46, turns=2.0, yaw_drift=0.1,
                                          t_drift=(0.004, -0.003, 0.001), noise=0.003),
    "seq_reject": _seq_reject,                                                                  # options of its own
    "seq_ftol": lambda: make_seq_graph([(1, 8), (2, 8)], [(10, 1), (13, 3), (15, 5)], 47, yaw_drift=0.002, t_drift=(0.0004, -0.0003, 0.0001),
                                       noise=0.02, start_yaw=0.01, start_t=0.002),
}


# ---- scripts for the session (vpl_pgs_*, pgs_ref.PoseGraph): lists of
#      ("add", sequence, vio_T, vio_R, loop_index, loop_info) | ("load", vio_T, vio_R, T, R, loop_index, loop_info) |
#      ("optimize",) | ("update_loop", index, loop_info)
class Truth:
    """a circle of n keyframes, `step` degrees apart, with small pitch and roll; loop(i, a) = loop_info of keyframe i against a"""

    def __init__(self, n, seed, step=20.0, radius=6.0):
        self.rng = np.random.default_rng(seed)
        ang = step * np.arange(n)
        self.yaw = (ang + 90.0 + 180.0) % 360.0 - 180.0
        self.t = np.stack([radius * np.cos(np.radians(ang)), radius * np.sin(np.radians(ang)), 0.2 * np.sin(np.radians(3 * ang))], axis=1)
        self.pitch, self.roll = self.rng.uniform(-3, 3, n), self.rng.uniform(-3, 3, n)
        self.R = np.array([_ypr2R(self.yaw[i], self.pitch[i], self.roll[i]) for i in range(n)])

    def loop(self, i, a, noise=0.0):
        info = np.zeros(8)
        info[:3] = self.R[a].T.dot(self.t[i] - self.t[a]) + self.rng.normal(0, noise, 3)
        info[3:7] = pg_ref.mat2q(self.R[a].T.dot(self.R[i]))
        info[7] = pg_ref.norm_angle(np.float64(self.yaw[i] - self.yaw[a])) + self.rng.normal(0, 10 * noise)
        return info

    def vio(self, ks, yaw_drift=0.4, t_drift=(0.03, -0.02, 0.004), origin_yaw=0.0, origin_t=(0.0, 0.0, 0.0)):
        """VIO poses of the keyframes ks (one run): the truth seen from an origin of its own, with a drift that grows along the run"""
        out, err, P = [], 0.0, None
        for j, k in enumerate(ks):
            if j == 0:
                P = self.t[k].copy()
            else:
                P = P + _ypr2R(err, 0.0, 0.0).dot(self.t[k] - self.t[ks[j - 1]]) + np.asarray(t_drift)
                err += yaw_drift
            Ro = _ypr2R(origin_yaw, 0.0, 0.0)
            out.append((Ro.dot(P + self.rng.normal(0, 1e-3, 3)) + np.asarray(origin_t), Ro.dot(_ypr2R(self.yaw[k] + err, self.pitch[k], self.roll[k]))))
        return out


def _script_single():
    tr = Truth(30, 51)                              # 20 degrees a keyframe: 20 is 20 degrees short of 3, 27 is 20 degrees past 8
    vio = tr.vio(list(range(30)))
    loops = {20: 3, 27: 8}
    ops = []
    for k in range(30):
        a = loops.get(k, -1)
        ops.append(("add", 1, vio[k][0], vio[k][1], a, tr.loop(k, a) if a >= 0 else None))
        if k == 22:
            ops.append(("optimize",))
        if k == 27:
            moved = tr.loop(27, 8, noise=0.01)
            far = moved.copy()
            far[7] = 45.0
            ops += [("update_loop", 27, moved), ("update_loop", 27, far)]     # inside the gate, outside it
        if k == 28:
            ops.append(("optimize",))
    return ops


def _script_second_sequence():
    tr = Truth(24, 52)
    one, two = tr.vio(list(range(12))), tr.vio(list(range(12, 24)), origin_yaw=40.0, origin_t=(3.0, -2.0, 0.5))
    ops = [("add", 1, p, r, -1, None) for p, r in one]
    ops[10] = ("add", 1, one[10][0], one[10][1], 1, tr.loop(10, 1))
    loops = {17: 4, 22: 7}
    for j, (p, r) in enumerate(two):
        k = 12 + j
        a = loops.get(k, -1)
        ops.append(("add", 2, p, r, a, tr.loop(k, a) if a >= 0 else None))
        if k in (18, 22):
            ops.append(("optimize",))
    return ops


def _script_base_map():
    tr = Truth(20, 53)
    ops = []
    for k in range(6):
        a = 1 if k == 5 else -1
        ops.append(("load", tr.t[k], tr.R[k], tr.t[k], tr.R[k], a, tr.loop(k, a) if a >= 0 else None))
    ops.append(("optimize",))                       # a graph of constants alone
    vio = tr.vio(list(range(6, 20)), origin_yaw=-25.0, origin_t=(-1.0, 4.0, 0.2))
    loops = {10: 2, 16: 4}
    for j, (p, r) in enumerate(vio):
        k = 6 + j
        a = loops.get(k, -1)
        ops.append(("add", 1, p, r, a, tr.loop(k, a) if a >= 0 else None))
        if k in (11, 16):
            ops.append(("optimize",))
    return ops


def _script_two_queued():
    tr = Truth(16, 54)
    vio = tr.vio(list(range(16)))
    loops = {10: 4, 13: 2}
    ops = [("add", 1, vio[k][0], vio[k][1], loops.get(k, -1), tr.loop(k, loops[k]) if k in loops else None) for k in range(16)]
    return ops + [("optimize",), ("optimize",)]     # the last queued index (13) from the earliest loop (2); then nothing


def _script_fast_relocalization():
    tr = Truth(16, 55, step=40.0)                   # 12 is where 3 was
    vio = tr.vio(list(range(16)))
    ops = [("add", 1, vio[k][0], vio[k][1], 3 if k == 12 else -1, tr.loop(12, 3) if k == 12 else None) for k in range(14)]
    ops += [("optimize",), ("update_loop", 12, tr.loop(12, 3, noise=0.02))]
    return ops + [("add", 1, vio[k][0], vio[k][1], -1, None) for k in (14, 15)]


SCRIPTS = {"single": _script_single, "second_sequence": _script_second_sequence, "base_map": _script_base_map,
           "two_queued": _script_two_queued, "fast_relocalization": _script_fast_relocalization}
SCRIPT_OPTIONS = {"fast_relocalization": dict(fast_relocalization=True)}


@functools.lru_cache(maxsize=None)
def script(name):
    return SCRIPTS[name]()


@functools.lru_cache(maxsize=None)
def ref_script(name, dtype="f64"):
    """the restatement's replay of a script: (what every step returned, the path after every step, the drift after every step);
    computed once and shared -- callers leave it unchanged"""
    dt = np.float64 if dtype == "f64" else np.longdouble
    pg = pgs_ref.PoseGraph(dtype=dt, **SCRIPT_OPTIONS.get(name, {}))
    returned, paths, drifts = [], [], []
    for op in script(name):
        returned.append(getattr(pg, op[0])(*op[1:]))
        paths.append(pg.path())
        drifts.append((pg.yaw_drift, pg.r_drift.copy(), pg.t_drift.copy()))
    return returned, paths, drifts


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def ref_case(name, dtype="f64", solver="banded"):
    """the restatement's run of a case; computed once and shared -- callers leave it unchanged"""
    g = case(name)
    dt = np.float64 if dtype == "f64" else np.longdouble
    return pgs_ref.optimize(g["vio_T"], g["vio_R"], g["loop_local"], g["loop_info"], g["sequence"], g["tail_T"], g["tail_R"], g["opt"], dt, solver)
