"""Named scenes for the feature selector (tests/select_ref.py is their model): EuRoC-like parameters -- acc_var 0.08,
acc_bias_var 0.0004, 752 x 480, the cam0 intrinsics of tests/test_preproc.py, 10 IMU samples of 5 ms between two images.

scene(name) -> (select_ref.Params, Scene).  reference(name) -> the restatement's float64 and long double runs of the scene, with
the selection bar asserted: in every round of both runs the best f stands at least twice the value bar above the second best
(where nothing may be selected: the best f stands that far below -1), so that two values inside the bar cannot change the order.
A scene that does not meet this is a bug here."""
import functools

import numpy as np

import select_ref as ref

K_BAR = 32.0          # the project's factor between |x64 - x80| and the bar (tests/test_gpu_init_relative_pose.py)
REL_FLOOR = 1e-12     # ... never below this times |x|_inf


def params(acc_var=0.08, acc_bias_var=0.0004, max_features=150, init_thresh=50):
    q = np.array([0.7123, -0.0077, 0.0105, 0.7018])
    return ref.Params(acc_var, acc_bias_var, max_features, init_thresh, 752, 480, 458.654, 457.296, 367.215, 248.375,
                      -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, q / np.linalg.norm(q), [-0.0216401454975, -0.064676986768, 0.00981073058949])


class Scene:
    """the members of one vpl_sel_input"""

    def __init__(self, **kw):
        self.horizon = None
        self.__dict__.update(kw)


def value_bar(x64, x80):
    """K max|x64 - x80| over the compared array, never below 1e-12 |x|_inf"""
    x64, x80 = np.asarray(x64, dtype=np.longdouble), np.asarray(x80, dtype=np.longdouble)
    ok = np.isfinite(x64) & np.isfinite(x80)
    if not ok.any():
        return 0.0
    return float(max(K_BAR * np.abs(x64[ok] - x80[ok]).max(), REL_FLOOR * np.abs(x80[ok]).max()))


def _motion(rng, speed=1.0, yaw_rate=0.2, n_imu=10, delta_imu=0.005):
    """states k and k + 1 of a body that moves along its camera's axis (with a third of that sideways) and turns about the
    camera's y axis"""
    par = params()
    Q0 = np.array([0.9, 0.1, -0.2, 0.38])
    Q0 /= np.linalg.norm(Q0)
    R0 = np.array(ref.qmat(Q0))
    Ric = np.array(ref.qmat(par.q_ic))
    P0 = np.array([1.0, -2.0, 0.5])
    V0 = R0 @ Ric @ np.array([speed / 3.0, 0.05, speed])
    Ba0 = np.array([0.02, -0.01, 0.03])
    gyr = Ric @ np.array([0.02, yaw_rate, -0.03])
    acc = R0.T @ np.array([0.3, -0.2, 9.80665 + 0.1]) + Ba0
    T = n_imu * delta_imu
    P1 = P0 + V0 * T + 0.5 * np.array([0.3, -0.2, 0.1]) * T * T
    V1 = V0 + np.array([0.3, -0.2, 0.1]) * T
    dq = np.concatenate([[1.0], 0.5 * gyr * T])
    Q1 = np.array(ref.qmul(Q0, dq / np.linalg.norm(dq)))
    return dict(P0=P0, Q0=Q0, V0=V0, Ba0=Ba0, P1=P1, Q1=Q1, V1=V1, Ba1=Ba0 + 1e-4, acc=acc, gyr=gyr, n_imu=n_imu, delta_imu=delta_imu)


def _features(rng, n, first_id, span=(0.55, 0.35)):
    x = rng.uniform(-span[0], span[0], n)
    y = rng.uniform(-span[1], span[1], n)
    prob = np.linspace(0.1, 1.0, n)[rng.permutation(n)] if n > 1 else np.array([0.7])     # spread over [0.1, 1]
    return np.arange(first_id, first_id + n, dtype=np.int32), x, y, prob


def _cloud(rng, m, lo=2.0, hi=8.0):
    if m == 0:
        return np.zeros((0, 3))
    return np.stack([rng.uniform(-0.6, 0.6, m), rng.uniform(-0.4, 0.4, m), rng.uniform(lo, hi, m)], axis=1)     # (ties: excluded by construction)


def random_scene(seed, n_new, n_used, n_cloud, kappa, **motion):
    rng = np.random.default_rng(seed)
    m = _motion(rng, **motion)
    ids, x, y, p = _features(rng, n_new, 1000)
    _, ux, uy, _ = _features(rng, n_used, 0)
    return Scene(new_id=ids, new_x=x, new_y=y, new_prob=p, used_x=ux if n_used else np.zeros(0), used_y=uy if n_used else np.zeros(0),
                 cloud=_cloud(rng, n_cloud), kappa=kappa, **m)


GREEDY_THREADS = 256      # SEL_GREEDY_THREADS of csrc/sel_kernels.h


def scene(name):
    par = params()
    if name == "1 candidate":
        return par, random_scene(1, 1, 8, 20, 1)
    if name == "2 identical":
        s = random_scene(2, 2, 8, 20, 2)
        s.new_x[1], s.new_y[1], s.new_prob[1] = s.new_x[0], s.new_y[0], s.new_prob[0]
        return par, s
    if name == "12 candidates":
        return par, random_scene(3, 12, 20, 40, 6)
    if name in ("63 candidates", "64 candidates", "65 candidates"):
        n = int(name.split()[0])
        return par, random_scene(4, n, 30, 60, 4)
    if name == "past the work-group":
        return par, random_scene(5, GREEDY_THREADS + 1, 10, 50, 3)
    if name == "kappa 0":
        return par, random_scene(6, 12, 8, 20, 0)
    if name == "kappa 1":
        return par, random_scene(6, 12, 8, 20, 1)
    if name == "kappa above":
        return par, random_scene(7, 5, 8, 20, 9)
    if name == "invisible":      # a fast turn about the camera's y axis: what stands at one edge leaves at once, on both edges one of the two does
        s = random_scene(8, 6, 6, 20, 3, yaw_rate=2.5)
        s.new_x[0], s.new_y[0] = 0.92, 0.02
        s.new_x[1], s.new_y[1] = -0.92, -0.03
        return par, s
    if name == "behind":         # 6 m/s towards points half a metre away: from k + 2 on they lie behind the camera, and the projection has no sign test
        s = random_scene(9, 6, 4, 0, 3, speed=6.0)
        s.cloud = np.array([[s.new_x[0] + 1e-3, s.new_y[0], 0.5], [s.new_x[1], s.new_y[1] - 1e-3, 0.45], [0.5, 0.3, 4.0], [-0.4, -0.3, 5.0], [0.0, 0.1, 3.0]])
        return par, s
    if name == "empty cloud":
        return par, random_scene(10, 12, 6, 0, 4)
    if name == "cloud of 1":
        return par, random_scene(11, 12, 6, 1, 4)
    if name == "no used":
        return par, random_scene(12, 12, 0, 30, 4)
    if name == "n_imu 1":
        return par, random_scene(13, 12, 8, 30, 4, n_imu=1, delta_imu=0.05)
    if name == "n_imu 2":
        return par, random_scene(13, 12, 8, 30, 4, n_imu=2, delta_imu=0.025)
    if name == "own horizon":
        s = random_scene(14, 12, 8, 30, 4)
        hz = np.zeros((5, 7))
        P, Q = ref.horizon(np.float64, s.P0, s.Q0, s.P1, s.Q1, s.V1, s.Ba0, s.acc, s.gyr, s.n_imu, s.delta_imu)
        hz[:, :3], hz[:, 3:] = P, Q / np.linalg.norm(Q, axis=1)[:, None]
        hz[2:, :3] += np.array([[0.01, -0.02, 0.005], [0.03, -0.01, 0.0], [0.02, 0.02, -0.01]])
        s.horizon = hz
        return par, s
    if name == "huge variances":
        return params(acc_var=1e6, acc_bias_var=1e6), random_scene(15, 12, 0, 30, 4)
    if name == "bench 200":
        return par, random_scene(16, 200, 100, 120, 50)
    raise KeyError(name)


SCENES = ("1 candidate", "2 identical", "12 candidates", "63 candidates", "64 candidates", "65 candidates", "past the work-group",
          "kappa 0", "kappa 1", "kappa above", "invisible", "behind", "empty cloud", "cloud of 1", "no used", "n_imu 1", "n_imu 2",
          "own horizon", "huge variances")
# n_imu = 1 makes the reference's covImu singular (CCt_11 = 1/4, CCt_12 = 1/2: a c - b^2 = 0 exactly; tests/
# test_select_reference.py), its inverse is rounding noise over zero and no value of the scene can be compared with anything: the
# scene is run for what can still be said of it (no overrun, the same bits twice, the counts), and "n_imu 2" carries the values of
# the shortest interval that has any
DEGENERATE = ("n_imu 1",)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict par, scene, r64, r80 (select_ref.run in the two precisions), bar_f [rounds]; asserts the selection bar"""
    par, s = scene(name)
    r64, r80 = ref.run(np.float64, par, s), ref.run(np.longdouble, par, s)
    assert r64["ids"] == r80["ids"] and r64["invisible"] == r80["invisible"], name
    assert len(r64["rounds"]) == len(r80["rounds"]), name
    bars = []
    for (c64, _, f64, g64), (c80, _, f80, g80) in zip(r64["rounds"], r80["rounds"]):
        assert c64 == c80, name
        bar = value_bar(f64, f80)
        bars.append(bar)
        best = float(np.nanmax(np.asarray(f80, dtype=np.float64)))
        if best > -1.0:
            assert min(g64, g80) >= 2 * bar, "%s: gap %.3g below twice the value bar %.3g" % (name, min(g64, g80), bar)
            assert best > -1.0 + 2 * bar, name
        else:
            assert best < -1.0 - 2 * bar, name
    if name == "behind":
        assert behind_and_visible(par, s, r64), "behind: no candidate lies behind a future camera that still counts it as visible"
    return dict(par=par, scene=s, r64=r64, r80=r80, bar_f=bars)


def behind_and_visible(par, s, r):
    """the new features (ids) that some future frame counts as visible while they lie behind its camera (z < 0): the projection
    divides by z without a sign test, so such a frame adds its block like any other.  Those of them that are candidates."""
    out = []
    t1 = r["P"][1] + np.array(ref.qrot(r["Q"][1], par.t_ic))
    q1 = ref.qmul(r["Q"][1], par.q_ic)
    for i, x, y, d in zip(s.new_id, s.new_x, s.new_y, r["depth_new"]):
        b = np.array([x, y, 1.0])
        pell = t1 + np.array(ref.qrot(q1, b / np.linalg.norm(b) * d))
        _, vis = ref.feature_info(np.float64, par, r["P"], r["Q"], x, y, d)
        for h, ok in zip(range(2, 5), vis):
            th = r["P"][h] + np.array(ref.qrot(r["Q"][h], par.t_ic))
            z = np.array(ref.qrot(ref.qinv(ref.qmul(r["Q"][h], par.q_ic)), pell - th))[2]
            if ok and z < 0 and int(i) not in r["invisible"] and int(i) not in out:
                out.append(int(i))
    return out
