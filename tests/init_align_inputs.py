"""Inputs of the visual-inertial alignment tests: the trajectory of test_gpu_sequence.Measurements seen as the caller's SfM sees
it -- rotated by a random Rw and scaled by 1 / SCALE -- with either exact pre-integration deltas from the true states (no device)
or the raw IMU stream (vpl_init_align_batch).  Computed once per argument set and shared; nothing writes into what is returned."""
import functools

import numpy as np

import vplines_slam_amd as v
from test_gpu_sequence import Measurements, quat_R

NF = 11
SCALE = 2.7
KEY11 = tuple(range(11))
KEY40 = (0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 39)
KEY14 = (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13)   # image frames 3, 7 and 11 are not key frames


@functools.lru_cache(maxsize=None)
def measurements(n_frames, seed):
    return Measurements(n_frames, seed=seed)


def random_rotation(rng):
    q = rng.normal(size=4)
    return quat_R(q)


class Pre:
    """the members of a pre-integration the restatement reads"""

    def __init__(self, sum_dt, dp, dq_xyzw, dv, J_R_BG):
        self.sum_dt, self.delta_p, self.delta_q, self.delta_v = sum_dt, dp, dq_xyzw, dv
        J = np.eye(15)
        J[3:6, 12:15] = J_R_BG
        self.jacobian = J.reshape(-1)


def eigen_quat(R):
    """(x, y, z, w) of a rotation matrix with w > 0 (every relative rotation here is small)"""
    w = np.sqrt(1 + R[0, 0] + R[1, 1] + R[2, 2]) / 2
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 4 * w * w]) / (4 * w)


def sfm_frames(M, F, seed):
    """ImageFrame::R = Rw Rs_f, ImageFrame::T = Rw (Ps_f + Rs_f tic) / SCALE for image frames 0 .. F-1 -> (Rw, R, T, tic)"""
    rng = np.random.default_rng(seed)
    Rw = random_rotation(rng)
    tic = M.ex[:3].copy()
    Rs = np.stack([quat_R(M.pose_true[f][3:]) for f in range(F)])
    Ps = np.stack([M.pose_true[f][:3] for f in range(F)])
    R = np.stack([Rw @ Rs[f] for f in range(F)])
    T = np.stack([Rw @ (Ps[f] + Rs[f] @ tic) / SCALE for f in range(F)])
    return Rw, R, T, tic


def exact_pre(M, F, g_norm):
    """delta_p, delta_q, delta_v of every image interval from the TRUE states (IntegrationBase's model, imu_factor.h:60-72), with
    an arbitrary regular O_R, O_BG block: an exact delta_q leaves delta_bg = 0 whatever the block is"""
    G = np.array([0, 0, g_norm])
    pre = [None]
    for f in range(1, F):
        Ri, Rj = quat_R(M.pose_true[f - 1][3:]), quat_R(M.pose_true[f][3:])
        Pi, Pj = M.pose_true[f - 1][:3], M.pose_true[f][:3]
        Vi, Vj = M.sb_true[f - 1][:3], M.sb_true[f][:3]
        dt = float(M.imu[f][:, 0].sum())
        dp = Ri.T @ (Pj - Pi - Vi * dt + 0.5 * G * dt * dt)
        dv = Ri.T @ (Vj - Vi + G * dt)
        pre.append(Pre(dt, dp, eigen_quat(Ri.T @ Rj), dv, -dt * np.eye(3) + 0.01 * np.arange(9).reshape(3, 3)))
    return pre


def imu_stream(M, F, cuts=None):
    """(n_samples [F], samples [sum, 7], acc0, gyr0): the intervals of image frames 1 .. F-1, some cut short (cuts: frame -> number
    of samples); by the reference's construction every interval but the first starts from the last sample before it"""
    imu = [M.imu[f][:(cuts or {}).get(f, len(M.imu[f]))] for f in range(1, F)]
    ns = np.array([0] + [len(s) for s in imu], dtype=np.int32)
    return ns, np.concatenate(imu), M.acc0[1].copy(), M.gyr0[1].copy()


@functools.lru_cache(maxsize=None)
def device_input(F, key, seed=77, cuts=(), flip_T=False, rw_seed=5, n_meas=None):
    """one InitInput from the first F frames of Measurements(n_meas or F): biases of the window a little off zero, linearisation
    biases likewise"""
    M = measurements(n_meas or F, seed)
    _, R, T, tic = sfm_frames(M, F, rw_seed)
    ns, samples, acc0, gyr0 = imu_stream(M, F, dict(cuts))
    rng = np.random.default_rng(1000 + F)
    lin_ba, lin_bg = rng.normal(0, 1e-3, (F, 3)), rng.normal(0, 1e-4, (F, 3))
    bas, bgs = rng.normal(0, 1e-2, (NF, 3)), rng.normal(0, 1e-4, (NF, 3))
    return v.capi.InitInput(R, -T if flip_T else T, ns, samples, acc0, gyr0, lin_ba, lin_bg, np.array(key), bas, bgs, tic)
