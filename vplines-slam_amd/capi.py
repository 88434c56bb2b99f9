"""ctypes bindings of include/vplines_ba.h (the C ABI of the HIP library)."""
import ctypes as C
import time
import os

import numpy as np

from . import _build

NF = 11
MAX_PRIOR_BLOCKS = 23
MAX_PRIOR_DIM = 171
MARGIN_OLD, MARGIN_SECOND_NEW, MARGIN_NONE = 0, 1, -1
PRIOR_PIVOTED_CHOLESKY, PRIOR_EIGEN = 0, 1   # vpl_ba_set_prior_rule
BLOCK_POSE, BLOCK_SPEEDBIAS, BLOCK_EXPOSE = 0, 1, 2

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


class BaOptions(C.Structure):
    _fields_ = [("num_iterations", C.c_int), ("estimate_extrinsic", C.c_int), ("marginalization_flag", C.c_int),
                ("remove_line_outliers", C.c_int), ("focal_length", C.c_double), ("line_factor", C.c_double),
                ("vp_factor", C.c_double), ("g_norm", C.c_double), ("acc_n", C.c_double), ("gyr_n", C.c_double),
                ("acc_w", C.c_double), ("gyr_w", C.c_double), ("huber_delta", C.c_double)]


def default_options():
    """EuRoC values (config/euroc/euroc_config.yaml) with the BASELINE metric's 5 iterations."""
    o = BaOptions()
    o.num_iterations = 5
    o.estimate_extrinsic = 1
    o.marginalization_flag = MARGIN_OLD
    o.remove_line_outliers = 0
    o.focal_length = 460.0
    o.line_factor = 306.666666667
    o.vp_factor = 10.0
    o.g_norm = 9.81007
    o.acc_n, o.gyr_n, o.acc_w, o.gyr_w = 0.08, 0.004, 0.00004, 2.0e-6
    o.huber_delta = 1.0
    return o


class Preintegration(C.Structure):
    _fields_ = [("sum_dt", C.c_double), ("delta_p", C.c_double * 3), ("delta_q", C.c_double * 4),
                ("delta_v", C.c_double * 3), ("linearized_ba", C.c_double * 3), ("linearized_bg", C.c_double * 3),
                ("jacobian", C.c_double * 225), ("covariance", C.c_double * 225)]


class Prior(C.Structure):
    _fields_ = [("n", C.c_int), ("n_blocks", C.c_int), ("block_kind", C.c_int * MAX_PRIOR_BLOCKS),
                ("block_frame", C.c_int * MAX_PRIOR_BLOCKS), ("block_idx", C.c_int * MAX_PRIOR_BLOCKS),
                ("x0", (C.c_double * 9) * MAX_PRIOR_BLOCKS), ("J0", C.c_double * (MAX_PRIOR_DIM * MAX_PRIOR_DIM)),
                ("r0", C.c_double * MAX_PRIOR_DIM)]

    def J(self):
        n = self.n
        return np.ctypeslib.as_array(self.J0)[: n * n].reshape(n, n).copy()

    def r(self):
        return np.ctypeslib.as_array(self.r0)[: self.n].copy()


INIT_MAX_FRAMES = 40
INIT_FAIL_GRAVITY, INIT_FAIL_SCALE, INIT_FAIL_REFINED_SCALE, INIT_FAIL_NONFINITE = 1, 2, 4, 8


class CInitInput(C.Structure):   # vpl_init_input
    _fields_ = [("n_frames", C.c_int), ("R", _dp), ("T", _dp), ("n_samples", _ip), ("samples", _dp),
                ("acc0", C.c_double * 3), ("gyr0", C.c_double * 3), ("lin_ba", _dp), ("lin_bg", _dp),
                ("key", C.c_int * NF), ("bas", (C.c_double * 3) * NF), ("bgs", (C.c_double * 3) * NF),
                ("tic", C.c_double * 3)]


class InitResult(C.Structure):   # vpl_init_result
    _fields_ = [("ok", C.c_int), ("fail", C.c_int), ("delta_bg", C.c_double * 3), ("g_linear", C.c_double * 3),
                ("s_linear", C.c_double), ("s", C.c_double), ("g_refined", C.c_double * 3), ("g", C.c_double * 3),
                ("vel", (C.c_double * 3) * INIT_MAX_FRAMES), ("pose", (C.c_double * 7) * NF),
                ("speed_bias", (C.c_double * 9) * NF)]

    def arrays(self):
        """the array members as numpy copies"""
        return {f: np.array(getattr(self, f)) for f in ("delta_bg", "g_linear", "g_refined", "g", "vel", "pose", "speed_bias")}


class InitInput:
    """numpy-backed owner of one vpl_init_input: what the caller's SfM and IMU buffers hand to the alignment.  R [F,3,3], T [F,3]
    = ImageFrame::R / T; n_samples [F] (entry 0 unused), samples [sum,7] = (dt, acc, gyr) of intervals 1..F-1; acc0 / gyr0 the
    measurement before interval 1; lin_ba / lin_bg [F,3]; key [11]; bas / bgs [11,3]; tic [3]."""

    def __init__(self, R, T, n_samples, samples, acc0, gyr0, lin_ba, lin_bg, key, bas, bgs, tic):
        self.R = _arr(R, np.float64).reshape(-1, 9).copy()
        self.n_frames = self.R.shape[0]
        self.T = _arr(T, np.float64).reshape(-1, 3).copy()
        self.n_samples = _arr(n_samples, np.int32).copy()
        self.samples = _arr(samples, np.float64).reshape(-1, 7).copy()
        self.acc0, self.gyr0 = _arr(acc0, np.float64).copy(), _arr(gyr0, np.float64).copy()
        self.lin_ba = _arr(lin_ba, np.float64).reshape(-1, 3).copy()
        self.lin_bg = _arr(lin_bg, np.float64).reshape(-1, 3).copy()
        self.key = _arr(key, np.int32).copy()
        self.bas, self.bgs = _arr(bas, np.float64).reshape(NF, 3).copy(), _arr(bgs, np.float64).reshape(NF, 3).copy()
        self.tic = _arr(tic, np.float64).copy()

    def to_c(self, ci=None):
        ci = ci if ci is not None else CInitInput()
        ci.n_frames = self.n_frames
        ci.R, ci.T, ci.samples = _p(self.R), _p(self.T), _p(self.samples)
        ci.n_samples = self.n_samples.ctypes.data_as(_ip)
        ci.lin_ba, ci.lin_bg = _p(self.lin_ba), _p(self.lin_bg)
        for k in range(3):
            ci.acc0[k], ci.gyr0[k], ci.tic[k] = self.acc0[k], self.gyr0[k], self.tic[k]
        for i in range(NF):
            ci.key[i] = int(self.key[i])
            for k in range(3):
                ci.bas[i][k], ci.bgs[i][k] = self.bas[i, k], self.bgs[i, k]
        return ci


def init_debug_jobs(n_samples, key):
    """vpl_init_debug_jobs (host only): [F + 9, 3] = (offset, nsamples, acc0 row) of the image intervals 1..F-1, then of the window
    intervals 1..10; the VPL_E_* code instead when the list is refused"""
    lib = load_hip_library()
    n_samples, key = _arr(n_samples, np.int32), _arr(key, np.int32)
    F = len(n_samples)
    jobs = np.zeros((max(F, 0) + 9, 3), dtype=np.int32)
    rc = lib.vpl_init_debug_jobs(F, n_samples.ctypes.data_as(_ip), key.ctypes.data_as(_ip), jobs.ctypes.data_as(_ip))
    return jobs if rc == 0 else rc


SFM_MAX_TRACKS = 1024
SFM_MAX_FRAME_POINTS = 1024
SFM_FAIL_KEY_PNP, SFM_FAIL_FRAME_PNP, SFM_FAIL_BA, SFM_FAIL_NUMERIC = 1, 2, 4, 8


class CSfmInput(C.Structure):   # vpl_sfm_input
    _fields_ = [("n_frames", C.c_int), ("key", C.c_int * NF), ("l", C.c_int), ("relative_R", C.c_double * 9),
                ("relative_T", C.c_double * 3), ("ric", C.c_double * 9), ("n_tracks", C.c_int), ("track_id", _ip),
                ("track_start", _ip), ("track_nobs", _ip), ("track_obs", _dp), ("frame_npts", _ip), ("frame_id", _ip),
                ("frame_xy", _dp)]


class SfmResult(C.Structure):   # vpl_sfm_result
    _fields_ = [("ok", C.c_int), ("fail", C.c_int), ("n_tracked", C.c_int), ("iterations", C.c_int), ("successful_steps", C.c_int),
                ("termination", C.c_int), ("pnp_iterations", C.c_int * NF), ("frame_iterations", C.c_int * INIT_MAX_FRAMES),
                ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("chain_q", (C.c_double * 4) * NF), ("chain_t", (C.c_double * 3) * NF),
                ("ba_q", (C.c_double * 4) * NF), ("ba_t", (C.c_double * 3) * NF),
                ("Q", (C.c_double * 4) * NF), ("T", (C.c_double * 3) * NF),
                ("frame_R", (C.c_double * 9) * INIT_MAX_FRAMES), ("frame_T", (C.c_double * 3) * INIT_MAX_FRAMES)]

    def arrays(self):
        """the array members as numpy copies"""
        return {f: np.array(getattr(self, f)) for f in ("pnp_iterations", "frame_iterations", "chain_q", "chain_t", "ba_q", "ba_t", "Q", "T",
                                                        "frame_R", "frame_T")}


class SfmInput:
    """numpy-backed owner of one vpl_sfm_input: what the feature manager, the image frames and relativePose hand to the initial
    structure.  key [11]; l; relative_R [3,3], relative_T [3]; ric [3,3]; track_id / track_start / track_nobs [N], track_obs [sum,2]
    (track after track); frame_pts {non-key image frame: (ids [k], xy [k,2])}, a missing frame has an empty list."""

    def __init__(self, n_frames, key, l, relative_R, relative_T, ric, track_id, track_start, track_nobs, track_obs, frame_pts=None):
        self.n_frames, self.l = int(n_frames), int(l)
        self.key = _arr(key, np.int32).copy()
        self.relative_R = _arr(relative_R, np.float64).reshape(9).copy()
        self.relative_T = _arr(relative_T, np.float64).reshape(3).copy()
        self.ric = _arr(ric, np.float64).reshape(9).copy()
        self.track_id, self.track_start, self.track_nobs = (_arr(a, np.int32).copy() for a in (track_id, track_start, track_nobs))
        self.track_obs = _arr(track_obs, np.float64).reshape(-1, 2).copy()
        frame_pts = frame_pts or {}
        self.frame_npts = np.zeros(max(self.n_frames, 1), dtype=np.int32)
        ids, xy = [np.zeros(0, dtype=np.int32)], [np.zeros((0, 2))]
        for f in sorted(frame_pts):
            i, x = frame_pts[f]
            self.frame_npts[f] = len(i)
            ids.append(_arr(i, np.int32))
            xy.append(_arr(x, np.float64).reshape(-1, 2))
        self.frame_id, self.frame_xy = np.concatenate(ids).astype(np.int32), np.concatenate(xy).astype(np.float64)

    def to_c(self, ci=None):
        ci = ci if ci is not None else CSfmInput()
        ci.n_frames, ci.l, ci.n_tracks = self.n_frames, self.l, len(self.track_start)
        for i in range(NF):
            ci.key[i] = int(self.key[i])
        for k in range(9):
            ci.relative_R[k], ci.ric[k] = self.relative_R[k], self.ric[k]
        for k in range(3):
            ci.relative_T[k] = self.relative_T[k]
        ci.track_id, ci.track_start, ci.track_nobs = (a.ctypes.data_as(_ip) for a in (self.track_id, self.track_start, self.track_nobs))
        ci.track_obs, ci.frame_xy = _p(self.track_obs), _p(self.frame_xy)
        ci.frame_npts, ci.frame_id = self.frame_npts.ctypes.data_as(_ip), self.frame_id.ctypes.data_as(_ip)
        return ci


def sfm_debug_plan(l, track_start, track_nobs):
    """vpl_sfm_debug_plan (host only): the schedule of GlobalSFM::construct -> dict step / fa / fb [N], count [11], first_fail; the
    VPL_E_* code instead when the tables are refused"""
    lib = load_hip_library()
    start, nobs = _arr(track_start, np.int32), _arr(track_nobs, np.int32)
    n = len(start)
    step, fa, fb = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(3))
    count, first = np.zeros(NF, dtype=np.int32), C.c_int(0)
    rc = lib.vpl_sfm_debug_plan(int(l), n, start.ctypes.data_as(_ip), nobs.ctypes.data_as(_ip), step.ctypes.data_as(_ip),
                                fa.ctypes.data_as(_ip), fb.ctypes.data_as(_ip), count.ctypes.data_as(_ip), C.byref(first))
    return dict(step=step[:n], fa=fa[:n], fb=fb[:n], count=count, first_fail=first.value) if rc == 0 else rc


RELPOSE_MAX_ITERS = 1000
RELPOSE_FEW_CORRES, RELPOSE_LOW_PARALLAX, RELPOSE_NO_MODEL, RELPOSE_FEW_GOOD, RELPOSE_SUCCESS = 0, 1, 2, 3, 4
RELPOSE_FAIL_NONE, RELPOSE_FAIL_NUMERIC = 1, 8
SFM_FAIL_RELATIVE_POSE = 16


class CRelPoseInput(C.Structure):   # vpl_relpose_input
    _fields_ = [("n_tracks", C.c_int), ("track_start", _ip), ("track_nobs", _ip), ("track_obs", _dp), ("seed", C.c_ulonglong)]


class RelPoseCandidate(C.Structure):   # vpl_relpose_candidate
    _fields_ = [("n_corres", C.c_int), ("status", C.c_int), ("iterations", C.c_int), ("best_iteration", C.c_int), ("best_root", C.c_int),
                ("inliers", C.c_int), ("good", C.c_int), ("numeric", C.c_int), ("pose_choice", C.c_int), ("pad_", C.c_int), ("average_parallax", C.c_double),
                ("F", C.c_double * 9), ("R", C.c_double * 9), ("T", C.c_double * 3)]


class RelPoseResult(C.Structure):   # vpl_relpose_result
    _fields_ = [("ok", C.c_int), ("fail", C.c_int), ("l", C.c_int), ("pad_", C.c_int), ("relative_R", C.c_double * 9),
                ("relative_T", C.c_double * 3), ("cand", RelPoseCandidate * (NF - 1))]


class RelPoseInput:
    """numpy-backed owner of one vpl_relpose_input: the track table as SfmInput has it -- track_start / track_nobs [N], track_obs
    [sum,2] (track after track) -- and the seed of the sample stream."""

    def __init__(self, track_start, track_nobs, track_obs, seed=0):
        self.track_start, self.track_nobs = (_arr(a, np.int32).copy() for a in (track_start, track_nobs))
        self.track_obs = _arr(track_obs, np.float64).reshape(-1, 2).copy()
        self.seed = int(seed)

    @classmethod
    def of(cls, sfm_input, seed=0):
        """from the arrays of an SfmInput"""
        return cls(sfm_input.track_start, sfm_input.track_nobs, sfm_input.track_obs, seed)

    def to_c(self, ci=None):
        ci = ci if ci is not None else CRelPoseInput()
        ci.n_tracks, ci.seed = len(self.track_start), self.seed
        ci.track_start, ci.track_nobs = (a.ctypes.data_as(_ip) for a in (self.track_start, self.track_nobs))
        ci.track_obs = _p(self.track_obs)
        return ci


def relpose_debug_plan(seed, i, N):
    """vpl_relpose_debug_plan (host only): the sample stream and the stopping table of candidate frame i over N correspondences ->
    dict samples [1000, 7], niters_after [N + 1]; the VPL_E_* code instead when the arguments are refused"""
    lib = load_hip_library()
    samples = np.zeros((RELPOSE_MAX_ITERS, 7), dtype=np.int32)
    table = np.zeros(max(int(N), 0) + 1, dtype=np.int32)
    rc = lib.vpl_relpose_debug_plan(int(seed), int(i), int(N), samples.ctypes.data_as(_ip), table.ctypes.data_as(_ip))
    return dict(samples=samples, niters_after=table) if rc == 0 else rc


LOOP_MAX_POINTS, LOOP_MAX_ITERS = 1024, 1000   # VPL_LOOP_MAX_POINTS, VPL_LOOP_MAX_ITERS
LOOP_FEW_POINTS, LOOP_NO_MODEL, LOOP_NUMERIC, LOOP_FEW_INLIERS, LOOP_REJECTED, LOOP_CLOSED = 0, 1, 2, 3, 4, 5


class LoopOptions(C.Structure):   # vpl_loop_options
    _fields_ = [("min_loop_num", C.c_int), ("max_iters", C.c_int), ("reproj_error", C.c_double), ("confidence", C.c_double),
                ("max_yaw_deg", C.c_double), ("max_t", C.c_double)]


def default_loop_options():
    o = LoopOptions()
    load_hip_library().vpl_loop_default_options(C.byref(o))
    return o


class CLoopInput(C.Structure):   # vpl_loop_input
    _fields_ = [("count", C.c_int), ("pts3d", C.POINTER(C.c_float)), ("old_norm", C.POINTER(C.c_float)), ("origin_vio_T", C.c_double * 3),
                ("origin_vio_R", C.c_double * 9), ("tic", C.c_double * 3), ("qic", C.c_double * 9), ("seed", C.c_ulonglong)]


class LoopResult(C.Structure):   # vpl_loop_result
    _fields_ = [("has_loop", C.c_int), ("stage", C.c_int), ("ransac_iterations", C.c_int), ("best_inliers", C.c_int),
                ("lm_iterations", C.c_int), ("lm_termination", C.c_int), ("PnP_T_old", C.c_double * 3), ("PnP_R_old", C.c_double * 9),
                ("loop_info", C.c_double * 8)]


class LoopInput:
    """numpy-backed owner of one vpl_loop_input: the lists findConnection has reduced by the match status -- pts3d [k][3],
    old_norm [k][2], kept as float32 -- the current keyframe's origin_vio_T / origin_vio_R, the extrinsics tic / qic (matrices
    [3][3]) and the seed of the sample stream."""

    def __init__(self, pts3d, old_norm, origin_vio_T, origin_vio_R, tic, qic, seed=0):
        self.pts3d = _arr(pts3d, np.float32).reshape(-1, 3).copy()
        self.old_norm = _arr(old_norm, np.float32).reshape(-1, 2).copy()
        if len(self.pts3d) != len(self.old_norm):
            raise ValueError("LoopInput: %d points, %d observations" % (len(self.pts3d), len(self.old_norm)))
        self.origin_vio_T, self.tic = (_arr(a, np.float64).reshape(3).copy() for a in (origin_vio_T, tic))
        self.origin_vio_R, self.qic = (_arr(a, np.float64).reshape(3, 3).copy() for a in (origin_vio_R, qic))
        self.seed = int(seed)

    def to_c(self, ci=None):
        ci = ci if ci is not None else CLoopInput()
        ci.count, ci.seed = len(self.pts3d), self.seed
        fp = C.POINTER(C.c_float)
        ci.pts3d, ci.old_norm = self.pts3d.ctypes.data_as(fp), self.old_norm.ctypes.data_as(fp)
        ci.origin_vio_T[:], ci.tic[:] = self.origin_vio_T.tolist(), self.tic.tolist()
        ci.origin_vio_R[:], ci.qic[:] = self.origin_vio_R.ravel().tolist(), self.qic.ravel().tolist()
        return ci


def loop_debug_plan(seed, N, confidence=0.99, max_iters=100):
    """vpl_loop_debug_plan (host only): the five-point sample stream and the stopping table of a list of N points -> dict samples
    [max_iters, 5], niters_after [N + 1]; the VPL_E_* code instead when the arguments are refused"""
    lib = load_hip_library()
    samples = np.zeros((max(int(max_iters), 1), 5), dtype=np.int32)
    table = np.zeros(max(int(N), 0) + 1, dtype=np.int32)
    rc = lib.vpl_loop_debug_plan(int(seed), int(N), float(confidence), int(max_iters), samples.ctypes.data_as(_ip), table.ctypes.data_as(_ip))
    return dict(samples=samples, niters_after=table) if rc == 0 else rc


PG_MAX_NODES, PG_MAX_LOOPS = 4096, 256   # VPL_PG_MAX_NODES, VPL_PG_MAX_LOOPS
PG_OK, PG_UNSUPPORTED = 0, 1
PG_NO_CONVERGENCE, PG_CONVERGENCE, PG_FAILURE = 0, 1, 2


class PgOptions(C.Structure):   # vpl_pg_options
    _fields_ = [("max_iterations", C.c_int), ("max_consecutive_invalid_steps", C.c_int), ("huber_delta", C.c_double),
                ("loop_yaw_scale", C.c_double), ("initial_radius", C.c_double), ("max_radius", C.c_double), ("min_radius", C.c_double),
                ("min_relative_decrease", C.c_double), ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double), ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double)]


def default_pg_options(**changes):
    o = PgOptions()
    load_hip_library().vpl_pg_default_options(C.byref(o))
    for k, val in changes.items():
        setattr(o, k, val)
    return o


class CPgInput(C.Structure):   # vpl_pg_input
    _fields_ = [("n", C.c_int), ("n_tail", C.c_int), ("vio_T", _dp), ("vio_R", _dp), ("loop_local", _ip), ("loop_info", _dp),
                ("sequence", _ip), ("tail_T", _dp), ("tail_R", _dp)]


class CPgResult(C.Structure):   # vpl_pg_result
    _fields_ = [("status", C.c_int), ("termination", C.c_int), ("iterations", C.c_int), ("successful_steps", C.c_int),
                ("unsuccessful_steps", C.c_int), ("reserved", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("yaw_drift", C.c_double), ("r_drift", C.c_double * 9), ("t_drift", C.c_double * 3), ("T", _dp), ("R", _dp),
                ("tail_T", _dp), ("tail_R", _dp)]


class PoseGraphInput:
    """numpy-backed owner of one vpl_pg_input: the keyframes first_looped_index .. cur_index as local nodes 0 .. n-1 -- vio_T [n][3],
    vio_R [n][3][3], loop_local [n] (-1, or the local index of the old keyframe), loop_info [n][8] as LoopResult.loop_info -- and
    optionally sequence [n] and the later keyframes tail_T / tail_R, which are only drift-corrected."""

    def __init__(self, vio_T, vio_R, loop_local, loop_info, sequence=None, tail_T=None, tail_R=None):
        self.vio_T = _arr(vio_T, np.float64).reshape(-1, 3).copy()
        n = len(self.vio_T)
        self.vio_R = _arr(vio_R, np.float64).reshape(n, 3, 3).copy()
        self.loop_local = _arr(loop_local, np.int32).reshape(n).copy()
        self.loop_info = _arr(loop_info, np.float64).reshape(n, 8).copy()
        self.sequence = None if sequence is None else _arr(sequence, np.int32).reshape(n).copy()
        self.tail_T = np.zeros((0, 3)) if tail_T is None else _arr(tail_T, np.float64).reshape(-1, 3).copy()
        self.tail_R = np.zeros((0, 3, 3)) if tail_R is None else _arr(tail_R, np.float64).reshape(len(self.tail_T), 3, 3).copy()

    def to_c(self, ci=None):
        ci = ci if ci is not None else CPgInput()
        ci.n, ci.n_tail = len(self.vio_T), len(self.tail_T)
        ci.vio_T, ci.vio_R, ci.loop_info = (a.ctypes.data_as(_dp) for a in (self.vio_T, self.vio_R, self.loop_info))
        ci.loop_local = self.loop_local.ctypes.data_as(_ip)
        ci.sequence = self.sequence.ctypes.data_as(_ip) if self.sequence is not None else None
        ci.tail_T = self.tail_T.ctypes.data_as(_dp) if len(self.tail_T) else None
        ci.tail_R = self.tail_R.ctypes.data_as(_dp) if len(self.tail_T) else None
        return ci


class PoseGraphResult:
    """one graph's vpl_pg_result with the arrays it points to: head (CPgResult), T [n][3], R [n][3][3], tail_T, tail_R"""

    def __init__(self, head, T, R, tail_T, tail_R):
        self.head, self.T, self.R, self.tail_T, self.tail_R = head, T, R, tail_T, tail_R

    def __getattr__(self, name):
        return getattr(self.head, name)

    def data(self):
        """every value the call wrote, as bytes (the pointers left out)"""
        h = self.head
        ints = np.array([h.status, h.termination, h.iterations, h.successful_steps, h.unsuccessful_steps], dtype=np.int32)
        dbl = np.array([h.initial_cost, h.final_cost, h.yaw_drift] + list(h.r_drift) + list(h.t_drift))
        return b"".join(a.tobytes() for a in (ints, dbl, self.T, self.R, self.tail_T, self.tail_R))


PGS_MAX_KEYFRAMES = 65536   # VPL_PGS_MAX_KEYFRAMES
PGS_OK, PGS_NOTHING = 0, 2


class PgsOptions(C.Structure):   # vpl_pgs_options
    _fields_ = [("max_keyframes", C.c_int), ("fast_relocalization", C.c_int), ("pg", PgOptions)]


class CPgsKeyframe(C.Structure):   # vpl_pgs_keyframe
    _fields_ = [("sequence", C.c_int), ("loop_index", C.c_int), ("vio_T", C.c_double * 3), ("vio_R", C.c_double * 9),
                ("T", C.c_double * 3), ("R", C.c_double * 9), ("loop_info", C.c_double * 8)]


class CPgsKeyframeOut(C.Structure):   # vpl_pgs_keyframe_out
    _fields_ = [("index", C.c_int), ("optimize_pending", C.c_int), ("vio_T", C.c_double * 3), ("vio_R", C.c_double * 9),
                ("T", C.c_double * 3), ("R", C.c_double * 9), ("w_r_vio", C.c_double * 9), ("w_t_vio", C.c_double * 3)]


class CPgsResult(C.Structure):   # vpl_pgs_result
    _fields_ = [("status", C.c_int), ("termination", C.c_int), ("iterations", C.c_int), ("successful_steps", C.c_int),
                ("unsuccessful_steps", C.c_int), ("n_nodes", C.c_int), ("first_index", C.c_int), ("cur_index", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("yaw_drift", C.c_double), ("r_drift", C.c_double * 9),
                ("t_drift", C.c_double * 3)]


def default_pgs_options(max_keyframes=None, fast_relocalization=None, **pg_changes):
    o = PgsOptions()
    load_hip_library().vpl_pgs_default_options(C.byref(o))
    if max_keyframes is not None:
        o.max_keyframes = int(max_keyframes)
    if fast_relocalization is not None:
        o.fast_relocalization = int(fast_relocalization)
    for k, val in pg_changes.items():
        setattr(o.pg, k, val)
    return o


class PoseGraphSession:
    """vpl_pgs_create .. vpl_pgs_destroy: one PoseGraph with its keyframe list resident on the device, on a Context that outlives
    it.  check=False on a method: a refusal comes back as its VPL_E_* code instead of an exception."""

    def __init__(self, ctx, options=None):
        self.ctx, self.lib, self.h = ctx, ctx.lib, C.c_void_p()
        opt = options if options is not None else default_pgs_options()
        ctx._settle()
        rc = self.lib.vpl_pgs_create(ctx.h, C.byref(opt), C.byref(self.h))
        if rc != 0:
            self.h = None
            ctx._check(rc, "vpl_pgs_create")

    def close(self):
        if self.h:
            self.lib.vpl_pgs_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return int(self.lib.vpl_pgs_size(self.h))

    def _done(self, rc, what, check):
        if rc != 0 and not check:
            return rc
        self.ctx._check(rc, what)
        return None

    @staticmethod
    def _kf(sequence, vio_T, vio_R, loop_index, loop_info, T=None, R=None):
        kf = CPgsKeyframe()
        kf.sequence, kf.loop_index = int(sequence), int(loop_index)
        kf.vio_T[:] = _arr(vio_T, np.float64).reshape(3)
        kf.vio_R[:] = _arr(vio_R, np.float64).reshape(9)
        if T is not None:
            kf.T[:] = _arr(T, np.float64).reshape(3)
            kf.R[:] = _arr(R, np.float64).reshape(9)
        if loop_info is not None:
            kf.loop_info[:] = _arr(loop_info, np.float64).reshape(8)
        return kf

    def _put(self, call, kf, want_out, check):
        out = CPgsKeyframeOut() if want_out else None
        bad = self._done(getattr(self.lib, call)(self.h, C.byref(kf), C.byref(out) if want_out else None), call, check)
        if bad is not None:
            return bad
        if not want_out:
            return None
        return dict(index=out.index, optimize_pending=bool(out.optimize_pending), vio_T=np.array(out.vio_T[:]),
                    vio_R=np.array(out.vio_R[:]).reshape(3, 3), T=np.array(out.T[:]), R=np.array(out.R[:]).reshape(3, 3),
                    w_r_vio=np.array(out.w_r_vio[:]).reshape(3, 3), w_t_vio=np.array(out.w_t_vio[:]))

    def add(self, sequence, vio_T, vio_R, loop_index=-1, loop_info=None, out=True, check=True):
        """addKeyFrame -> dict index, optimize_pending, vio_T, vio_R (shifted), T, R (drift-corrected), w_r_vio, w_t_vio; out=False:
        nothing is copied back or waited for, -> None"""
        return self._put("vpl_pgs_add_keyframe", self._kf(sequence, vio_T, vio_R, loop_index, loop_info), out, check)

    def load(self, vio_T, vio_R, T, R, loop_index=-1, loop_info=None, out=True, check=True):
        """loadKeyFrame: a keyframe of sequence 0 with its stored poses"""
        return self._put("vpl_pgs_load_keyframe", self._kf(0, vio_T, vio_R, loop_index, loop_info, T, R), out, check)

    def optimize(self, check=True):
        """one turn of optimize4DoF -> CPgsResult (status PGS_NOTHING when nothing was queued)"""
        self.ctx._settle()
        res = CPgsResult()
        bad = self._done(self.lib.vpl_pgs_optimize(self.h, C.byref(res)), "vpl_pgs_optimize", check)
        return bad if bad is not None else res

    def update_loop(self, index, loop_info, check=True):
        """updateKeyFrameLoop -> whether the gate let the new loop_info in"""
        li = _arr(loop_info, np.float64).reshape(8).copy()
        ok = C.c_int(0)
        bad = self._done(self.lib.vpl_pgs_update_loop(self.h, int(index), li.ctypes.data_as(_dp), C.byref(ok)), "vpl_pgs_update_loop", check)
        return bad if bad is not None else bool(ok.value)

    def path(self, first=0, count=None, check=True):
        """-> dict T [count][3], R [count][3][3], vio_T, vio_R, loop_info [count][8], sequence, loop_index [count]"""
        count = len(self) - int(first) if count is None else int(count)
        n = max(count, 0)
        d = dict(T=np.zeros((n, 3)), R=np.zeros((n, 3, 3)), vio_T=np.zeros((n, 3)), vio_R=np.zeros((n, 3, 3)), loop_info=np.zeros((n, 8)),
                 sequence=np.zeros(n, dtype=np.int32), loop_index=np.zeros(n, dtype=np.int32))
        self.ctx._settle()
        rc = self.lib.vpl_pgs_get_path(self.h, int(first), count, *(d[k].ctypes.data_as(_dp) for k in ("T", "R", "vio_T", "vio_R", "loop_info")),
                                       d["sequence"].ctypes.data_as(_ip), d["loop_index"].ctypes.data_as(_ip))
        bad = self._done(rc, "vpl_pgs_get_path", check)
        return bad if bad is not None else d

    def drift(self):
        """-> (yaw_drift, r_drift [3][3], t_drift [3])"""
        yaw, r, t = C.c_double(0), np.zeros((3, 3)), np.zeros(3)
        self._done(self.lib.vpl_pgs_get_drift(self.h, C.byref(yaw), r.ctypes.data_as(_dp), t.ctypes.data_as(_dp)), "vpl_pgs_get_drift", True)
        return float(yaw.value), r, t

    def reset(self):
        self._done(self.lib.vpl_pgs_reset(self.h), "vpl_pgs_reset", True)


GF_MAX_NODES = 65536   # VPL_GF_MAX_NODES
GF_NO_CONVERGENCE, GF_CONVERGENCE, GF_FAILURE = 0, 1, 2


class GfOptions(C.Structure):   # vpl_gf_options
    _fields_ = [("max_iterations", C.c_int), ("max_consecutive_invalid_steps", C.c_int), ("segment", C.c_int), ("reserved", C.c_int),
                ("t_var", C.c_double), ("q_var", C.c_double), ("huber_delta", C.c_double), ("initial_radius", C.c_double),
                ("max_radius", C.c_double), ("min_radius", C.c_double), ("min_relative_decrease", C.c_double),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double)]


def default_gf_options(**changes):
    o = GfOptions()
    load_hip_library().vpl_gf_default_options(C.byref(o))
    for k, val in changes.items():
        setattr(o, k, val)
    return o


class CGfInput(C.Structure):   # vpl_gf_input
    _fields_ = [("n", C.c_int), ("n_gps", C.c_int), ("local", _dp), ("glob", _dp), ("gps_node", _ip), ("gps_xyz", _dp),
                ("gps_accuracy", _dp)]


class CGfResult(C.Structure):   # vpl_gf_result
    _fields_ = [("status", C.c_int), ("termination", C.c_int), ("iterations", C.c_int), ("successful_steps", C.c_int),
                ("unsuccessful_steps", C.c_int), ("reserved", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("wgps_T_wvio", C.c_double * 16), ("pose", _dp)]


class GlobalFusionInput:
    """numpy-backed owner of one vpl_gf_input: the odometry poses local [n][7] = p, q(w, x, y, z), the initial global poses
    global_ [n][7], and the GNSS fixes gps_node [n_gps] (strictly ascending), gps_xyz [n_gps][3], gps_accuracy [n_gps]"""

    def __init__(self, local, global_, gps_node=(), gps_xyz=(), gps_accuracy=()):
        self.local = _arr(local, np.float64).reshape(-1, 7).copy()
        n = len(self.local)
        self.global_ = _arr(global_, np.float64).reshape(n, 7).copy()
        self.gps_node = _arr(gps_node, np.int32).reshape(-1).copy()
        m = len(self.gps_node)
        self.gps_xyz = _arr(gps_xyz, np.float64).reshape(m, 3).copy()
        self.gps_accuracy = _arr(gps_accuracy, np.float64).reshape(m).copy()

    def to_c(self, ci=None):
        ci = ci if ci is not None else CGfInput()
        ci.n, ci.n_gps = len(self.local), len(self.gps_node)
        ci.local, ci.glob = self.local.ctypes.data_as(_dp), self.global_.ctypes.data_as(_dp)
        m = len(self.gps_node)
        ci.gps_node = self.gps_node.ctypes.data_as(_ip) if m else None
        ci.gps_xyz = self.gps_xyz.ctypes.data_as(_dp) if m else None
        ci.gps_accuracy = self.gps_accuracy.ctypes.data_as(_dp) if m else None
        return ci


class GlobalFusionResult:
    """one chain's vpl_gf_result with the array it points to: head (CGfResult), pose [n][7]"""

    def __init__(self, head, pose):
        self.head, self.pose = head, pose

    def __getattr__(self, name):
        return getattr(self.head, name)

    @property
    def T(self):
        """wgps_T_wvio as a 4 x 4 array"""
        return np.array(self.head.wgps_T_wvio[:]).reshape(4, 4)

    def data_head(self):
        """every value of the head, as bytes (the pointer left out)"""
        h = self.head
        ints = np.array([h.status, h.termination, h.iterations, h.successful_steps, h.unsuccessful_steps], dtype=np.int32)
        dbl = np.array([h.initial_cost, h.final_cost] + list(h.wgps_T_wvio))
        return ints.tobytes() + dbl.tobytes()

    def data(self):
        """every value the call wrote, as bytes"""
        return self.data_head() + self.pose.tobytes()


def gf_debug_plan(n, segment=0):
    """vpl_gf_debug_plan (host only): the separators and segments of an n-node chain -> dict sep_node [n_sep], seg_bounds [n_seg][2],
    or the VPL_E_* code of a refusal"""
    lib = load_hip_library()
    cap = max(int(n), 0) // 2 + 1
    sep, seg = np.zeros(cap, dtype=np.int32), np.zeros((cap, 2), dtype=np.int32)
    ns, ng = C.c_int(0), C.c_int(0)
    rc = lib.vpl_gf_debug_plan(int(n), int(segment), C.byref(ns), sep.ctypes.data_as(_ip), C.byref(ng), seg.ctypes.data_as(_ip))
    return dict(sep_node=sep[:ns.value].copy(), seg_bounds=seg[:ng.value].copy()) if rc == 0 else rc


def local_cartesian(lat0, lon0, h0, lla):
    """vpl_gf_local_cartesian (host only): WGS84 latitude, longitude (degrees), height [n][3] -> east, north, up [n][3] at the origin"""
    lib = load_hip_library()
    lla = _arr(lla, np.float64).reshape(-1, 3).copy()
    xyz = np.zeros_like(lla)
    rc = lib.vpl_gf_local_cartesian(float(lat0), float(lon0), float(h0), len(lla), lla.ctypes.data_as(_dp), xyz.ctypes.data_as(_dp))
    if rc != 0:
        raise RuntimeError("vpl_gf_local_cartesian failed: %d" % rc)
    return xyz


class GlobalFusionSession:
    """vpl_gf_create .. vpl_gf_destroy: the GlobalOptimization object with the trajectory resident on the device, on a Context that
    outlives it.  check=False on a method: a refusal comes back as its VPL_E_* code instead of an exception."""

    def __init__(self, ctx, max_nodes):
        self.ctx, self.lib, self.h = ctx, ctx.lib, C.c_void_p()
        ctx._settle()
        rc = self.lib.vpl_gf_create(ctx.h, int(max_nodes), C.byref(self.h))
        if rc != 0:
            self.h = None
            ctx._check(rc, "vpl_gf_create")

    def close(self):
        if self.h:
            self.lib.vpl_gf_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _done(self, rc, what, check):
        if rc != 0 and not check:
            return rc
        self.ctx._check(rc, what)
        return None

    def input_odom(self, t, p, q, check=True):
        """inputOdom + getGlobalOdom: -> (global p [3], global q [4] = w, x, y, z)"""
        p, q = _arr(p, np.float64).reshape(3).copy(), _arr(q, np.float64).reshape(4).copy()
        op, oq = np.zeros(3), np.zeros(4)
        rc = self.lib.vpl_gf_input_odom(self.h, float(t), p.ctypes.data_as(_dp), q.ctypes.data_as(_dp), op.ctypes.data_as(_dp), oq.ctypes.data_as(_dp))
        bad = self._done(rc, "vpl_gf_input_odom", check)
        return bad if bad is not None else (op, oq)

    def input_gps(self, t, xyz, accuracy, check=True):
        xyz = _arr(xyz, np.float64).reshape(3).copy()
        return self._done(self.lib.vpl_gf_input_gps(self.h, float(t), xyz.ctypes.data_as(_dp), float(accuracy)), "vpl_gf_input_gps", check)

    def optimize(self, options=None, check=True):
        """-> GlobalFusionResult with the head only (pose is None): the poses stay on the device, see path()"""
        opt = options if options is not None else default_gf_options()
        self.ctx._settle()
        res = CGfResult()
        bad = self._done(self.lib.vpl_gf_optimize(self.h, C.byref(opt), C.byref(res)), "vpl_gf_optimize", check)
        return bad if bad is not None else GlobalFusionResult(res, None)

    def path(self, first, count, check=True):
        out = np.zeros((max(int(count), 0), 7))
        self.ctx._settle()
        bad = self._done(self.lib.vpl_gf_get_path(self.h, int(first), int(count), out.ctypes.data_as(_dp)), "vpl_gf_get_path", check)
        return bad if bad is not None else out


SEL_MAX_FEATURES = 1024   # VPL_SEL_MAX_FEATURES


class SelectParams(C.Structure):   # vpl_sel_params
    """acc_var / acc_bias_var (the reference passes ACC_N, ACC_W), the id book's max_features / init_thresh, the PINHOLE camera with
    its radtan distortion, the extrinsic q_ic (w, x, y, z) / t_ic"""
    _fields_ = [("acc_var", C.c_double), ("acc_bias_var", C.c_double), ("max_features", C.c_int), ("init_thresh", C.c_int),
                ("width", C.c_int), ("height", C.c_int), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("q_ic", C.c_double * 4), ("t_ic", C.c_double * 3)]

    @classmethod
    def of(cls, p):
        """from anything with the members by name (q_ic / t_ic as sequences)"""
        o = cls()
        for f, t in cls._fields_:
            v = getattr(p, f)
            if f in ("q_ic", "t_ic"):
                for k, x in enumerate(v):
                    getattr(o, f)[k] = float(x)
            else:
                setattr(o, f, int(v) if t is C.c_int else float(v))
        return o


class CSelectInput(C.Structure):   # vpl_sel_input
    _fields_ = [("P0", C.c_double * 3), ("Q0", C.c_double * 4), ("V0", C.c_double * 3), ("Ba0", C.c_double * 3),
                ("P1", C.c_double * 3), ("Q1", C.c_double * 4), ("V1", C.c_double * 3), ("Ba1", C.c_double * 3),
                ("acc", C.c_double * 3), ("gyr", C.c_double * 3), ("delta_imu", C.c_double), ("n_imu", C.c_int), ("kappa", C.c_int),
                ("horizon", _dp), ("n_new", C.c_int), ("new_id", _ip), ("new_x", _dp), ("new_y", _dp), ("new_prob", _dp),
                ("n_used", C.c_int), ("used_x", _dp), ("used_y", _dp), ("n_cloud", C.c_int), ("cloud", _dp)]


class SelectResult(C.Structure):   # vpl_sel_result
    _fields_ = [("n_selected", C.c_int), ("n_invisible", C.c_int), ("n_ineligible", C.c_int), ("n_candidates", C.c_int)]


class CSelectFrame(C.Structure):   # vpl_odo_sel_frame
    _fields_ = [("P1", C.c_double * 3), ("Q1", C.c_double * 4), ("V1", C.c_double * 3), ("Ba1", C.c_double * 3), ("acc", C.c_double * 3),
                ("gyr", C.c_double * 3), ("delta_imu", C.c_double), ("n_imu", C.c_int), ("horizon", _dp), ("n_features", C.c_int), ("id", _ip),
                ("x", _dp), ("y", _dp), ("prob", _dp)]


class OdoSelectResult(C.Structure):   # vpl_odo_sel_result
    _fields_ = [("sel", SelectResult), ("initialized", C.c_int), ("n_new", C.c_int), ("n_used", C.c_int), ("kappa", C.c_int),
                ("n_cloud", C.c_int), ("n_out", C.c_int)]


class SelectFrame:
    """numpy-backed owner of one vpl_odo_sel_frame: state k + 1 (P1, Q1 (w, x, y, z), V1, Ba1), acc, unbiased gyr, n_imu, delta_imu,
    horizon (None or [5, 7]) and the image -- id, x, y, prob of every feature the front end reports"""
    _VEC = ("P1", "Q1", "V1", "Ba1", "acc", "gyr")

    def __init__(self, P1, Q1, V1, Ba1, acc, gyr, n_imu, delta_imu, id, x, y, prob, horizon=None):
        for k, a in zip(self._VEC, (P1, Q1, V1, Ba1, acc, gyr)):
            setattr(self, k, _arr(a, np.float64).copy())
        self.n_imu, self.delta_imu = int(n_imu), float(delta_imu)
        self.id = _arr(id, np.int32).copy()
        self.x, self.y, self.prob = (_arr(a, np.float64).copy() for a in (x, y, prob))
        self.horizon = None if horizon is None else _arr(horizon, np.float64).reshape(5, 7).copy()

    def to_c(self, cf):
        for k in self._VEC:
            for j, v in enumerate(getattr(self, k)):
                getattr(cf, k)[j] = v
        cf.delta_imu, cf.n_imu, cf.n_features = self.delta_imu, self.n_imu, len(self.id)
        cf.horizon = _p(self.horizon) if self.horizon is not None else None
        cf.id = self.id.ctypes.data_as(_ip)
        cf.x, cf.y, cf.prob = _p(self.x), _p(self.y), _p(self.prob)
        return cf


class SelectInput:
    """numpy-backed owner of one vpl_sel_input: states k and k + 1 (P, Q (w, x, y, z), V, Ba), acc, unbiased gyr, n_imu, delta_imu,
    horizon (None or [5, 7]), the new features (id, x, y, prob), the used features (x, y), the cloud [m, 3] = x, y, depth, kappa"""
    _VEC = ("P0", "Q0", "V0", "Ba0", "P1", "Q1", "V1", "Ba1", "acc", "gyr")

    def __init__(self, P0, Q0, V0, Ba0, P1, Q1, V1, Ba1, acc, gyr, n_imu, delta_imu, new_id, new_x, new_y, new_prob, used_x=(), used_y=(),
                 cloud=(), kappa=0, horizon=None):
        for k, a in zip(self._VEC, (P0, Q0, V0, Ba0, P1, Q1, V1, Ba1, acc, gyr)):
            setattr(self, k, _arr(a, np.float64).copy())
        self.n_imu, self.delta_imu, self.kappa = int(n_imu), float(delta_imu), int(kappa)
        self.new_id = _arr(new_id, np.int32).copy()
        self.new_x, self.new_y, self.new_prob, self.used_x, self.used_y = (_arr(a, np.float64).copy() for a in (new_x, new_y, new_prob, used_x, used_y))
        self.cloud = _arr(cloud, np.float64).reshape(-1, 3).copy()
        self.horizon = None if horizon is None else _arr(horizon, np.float64).reshape(5, 7).copy()

    @classmethod
    def of(cls, s, **over):
        """from anything with the members by name"""
        kw = {k: getattr(s, k) for k in cls._VEC + ("n_imu", "delta_imu", "new_id", "new_x", "new_y", "new_prob", "used_x", "used_y", "cloud", "kappa", "horizon")}
        kw.update(over)
        return cls(**kw)

    def to_c(self, ci=None):
        ci = ci if ci is not None else CSelectInput()
        for k in self._VEC:
            for j, x in enumerate(getattr(self, k)):
                getattr(ci, k)[j] = x
        ci.delta_imu, ci.n_imu, ci.kappa = self.delta_imu, self.n_imu, self.kappa
        ci.horizon = _p(self.horizon) if self.horizon is not None else None
        ci.n_new, ci.n_used, ci.n_cloud = len(self.new_id), len(self.used_x), len(self.cloud)
        ci.new_id = self.new_id.ctypes.data_as(_ip)
        for k in ("new_x", "new_y", "new_prob", "used_x", "used_y", "cloud"):
            setattr(ci, k, _p(getattr(self, k)))
        return ci


def select_debug_book(max_features, init_thresh, images, initialized, offers):
    """vpl_sel_debug_book (host only): the id book of FeatureSelector::select replayed over a script.  images: a list of id lists;
    initialized: a flag per image; offers: per image the ids that stand in for the greedy selection (the first kappa of them that
    are new are selected).  -> dict n_new, kappa, last_id, n_tracked [n], selected / out (lists of id arrays), tracked (the
    tracked list after the last image); the VPL_E_* code instead when the call is refused"""
    lib = load_hip_library()
    n = len(images)
    ip = lambda a: a.ctypes.data_as(_ip)
    n_ids = np.array([len(a) for a in images], dtype=np.int32)
    n_off = np.array([len(a) for a in offers], dtype=np.int32)
    cat = lambda ls: np.concatenate([np.asarray(a, dtype=np.int32).reshape(-1) for a in ls] + [np.zeros(1, np.int32)])
    ids, off = cat(images), cat(offers)
    init = np.array([1 if f else 0 for f in initialized], dtype=np.uint8)
    max_ids = max([1] + [len(a) for a in images])
    max_tracked = int(n_ids.sum()) + 1
    n_new, kappa, n_sel, n_out, n_tr, last = (np.zeros(n + 1, dtype=np.int32) for _ in range(6))
    sel, out = np.zeros((n + 1, max_ids), dtype=np.int32), np.zeros((n + 1, max_ids), dtype=np.int32)
    tracked = np.zeros(max_tracked, dtype=np.int32)
    rc = lib.vpl_sel_debug_book(int(max_features), int(init_thresh), n, ip(n_ids), ip(ids), init.ctypes.data_as(C.POINTER(C.c_ubyte)), ip(n_off),
                                ip(off), max_ids, ip(n_new), ip(kappa), ip(n_sel), ip(sel), ip(n_out), ip(out), ip(n_tr), ip(last), max_tracked,
                                ip(tracked))
    if rc != 0:
        return rc
    return dict(n_new=n_new[:n], kappa=kappa[:n], last_id=last[:n], n_tracked=n_tr[:n], selected=[sel[i, :n_sel[i]].copy() for i in range(n)],
                out=[out[i, :n_out[i]].copy() for i in range(n)], tracked=tracked[:n_tr[n - 1]].copy() if n else tracked[:0])


class CWindow(C.Structure):
    _fields_ = [("pose", (C.c_double * 7) * NF), ("speed_bias", (C.c_double * 9) * NF), ("ex_pose", C.c_double * 7),
                ("n_points", C.c_int), ("point_start", _ip), ("point_nobs", _ip), ("point_obs", _dp),
                ("inv_depth", _dp),
                ("n_lines", C.c_int), ("line_start", _ip), ("line_nobs", _ip), ("line_obs", _dp), ("line_plk", _dp),
                ("line_removed", _ip), ("line_triangulated", _ip),
                ("preint", Preintegration * NF), ("has_prior", C.c_int), ("prior", C.POINTER(Prior)),
                ("failure_occur", C.c_int), ("last_P0", C.c_double * 3), ("last_R0", C.c_double * 9),
                ("line_orth", C.POINTER(C.c_double))]


class SolveReport(C.Structure):
    _fields_ = [("iterations", C.c_int), ("num_successful_steps", C.c_int), ("termination", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("n_lines_removed", C.c_int),
                ("prior_m", C.c_int), ("prior_n", C.c_int)]


def _arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


class Window:
    """numpy-backed owner of one vpl_window (keeps the arrays alive)."""

    def __init__(self, pose, speed_bias, ex_pose, point_start, point_nobs, point_obs, inv_depth, line_start,
                 line_nobs, line_obs, line_plk, preint=None, prior=None):
        self.pose = _arr(pose, np.float64).reshape(NF, 7).copy()
        self.speed_bias = _arr(speed_bias, np.float64).reshape(NF, 9).copy()
        self.ex_pose = _arr(ex_pose, np.float64).reshape(7).copy()
        self.point_start = _arr(point_start, np.int32).copy()
        self.point_nobs = _arr(point_nobs, np.int32).copy()
        self.point_obs = _arr(point_obs, np.float64).reshape(-1, 3).copy()
        self.inv_depth = _arr(inv_depth, np.float64).copy()
        self.line_start = _arr(line_start, np.int32).copy()
        self.line_nobs = _arr(line_nobs, np.int32).copy()
        self.line_obs = _arr(line_obs, np.float64).reshape(-1, 8).copy()
        self.line_plk = _arr(line_plk, np.float64).reshape(-1, 6).copy()
        self.line_removed = np.zeros(max(len(self.line_start), 1), np.int32)   # out: removeLineOutlier flags
        self.line_triangulated = np.ones(max(len(self.line_start), 1), np.int32)   # is_triangulation (in/out)
        self.preint = preint if preint is not None else (Preintegration * NF)()
        self.prior = prior
        self.failure = None       # (last_P0 [3], last_R0 [3,3]) => failure_occur = 1 (estimator.cpp:818-823)
        self.extra = {}

    def copy(self):
        pre = (Preintegration * NF)()
        C.memmove(pre, self.preint, C.sizeof(pre))
        w = Window(self.pose, self.speed_bias, self.ex_pose, self.point_start, self.point_nobs, self.point_obs,
                   self.inv_depth, self.line_start, self.line_nobs, self.line_obs, self.line_plk, pre, self.prior)
        w.extra = dict(self.extra)
        w.failure = self.failure
        w.line_triangulated[:] = self.line_triangulated
        return w

    def to_c(self, cw=None):
        cw = cw if cw is not None else CWindow()
        C.memmove(cw.pose, self.pose.ctypes.data, NF * 7 * 8)
        C.memmove(cw.speed_bias, self.speed_bias.ctypes.data, NF * 9 * 8)
        C.memmove(cw.ex_pose, self.ex_pose.ctypes.data, 7 * 8)
        cw.n_points = len(self.point_start)
        cw.point_start = self.point_start.ctypes.data_as(_ip)
        cw.point_nobs = self.point_nobs.ctypes.data_as(_ip)
        cw.point_obs = self.point_obs.ctypes.data_as(_dp)
        cw.inv_depth = self.inv_depth.ctypes.data_as(_dp)
        cw.n_lines = len(self.line_start)
        cw.line_start = self.line_start.ctypes.data_as(_ip)
        cw.line_nobs = self.line_nobs.ctypes.data_as(_ip)
        cw.line_obs = self.line_obs.ctypes.data_as(_dp)
        cw.line_plk = self.line_plk.ctypes.data_as(_dp)
        cw.line_removed = self.line_removed.ctypes.data_as(_ip)
        cw.line_triangulated = self.line_triangulated.ctypes.data_as(_ip)
        C.memmove(cw.preint, self.preint, C.sizeof(Preintegration) * NF)
        cw.has_prior = 1 if self.prior is not None else 0
        cw.prior = C.pointer(self.prior) if self.prior is not None else C.POINTER(Prior)()
        cw.line_orth = C.POINTER(C.c_double)()
        cw.failure_occur = 0
        if self.failure is not None:
            cw.failure_occur = 1
            p0 = np.ascontiguousarray(self.failure[0], np.float64).reshape(3)
            r0 = np.ascontiguousarray(self.failure[1], np.float64).reshape(9)
            for k in range(3):
                cw.last_P0[k] = p0[k]
            for k in range(9):
                cw.last_R0[k] = r0[k]
        return cw

    def from_c(self, cw):
        """copy back the in/out fields after a solve"""
        self.pose[:] = np.ctypeslib.as_array(cw.pose).reshape(NF, 7)
        self.speed_bias[:] = np.ctypeslib.as_array(cw.speed_bias).reshape(NF, 9)
        self.ex_pose[:] = np.ctypeslib.as_array(cw.ex_pose)


class OdoFrame(C.Structure):
    """vpl_odo_frame: one image of one sequence (the arrays are the caller's; Session keeps them alive for the call)"""
    _fields_ = [("pose", C.c_double * 7), ("speed_bias", C.c_double * 9), ("preint", Preintegration),
                ("n_points", C.c_int), ("point_id", _ip), ("point_obs", _dp),
                ("n_lines", C.c_int), ("line_id", _ip), ("line_obs", _dp)]


class OdoResult(C.Structure):
    _fields_ = [("pose", (C.c_double * 7) * NF), ("speed_bias", (C.c_double * 9) * NF), ("ex_pose", C.c_double * 7),
                ("line_report", SolveReport), ("report", SolveReport),
                ("n_points_solved", C.c_int), ("n_lines_solved", C.c_int), ("n_point_tracks", C.c_int),
                ("n_line_tracks", C.c_int), ("n_ignored", C.c_int)]


class OdoImuFrame(C.Structure):
    """vpl_odo_imu_frame: one image of one sequence with the IMU samples since the previous image"""
    _fields_ = [("n_samples", C.c_int), ("samples", _dp),
                ("n_points", C.c_int), ("point_id", _ip), ("point_obs", _dp),
                ("n_lines", C.c_int), ("line_id", _ip), ("line_obs", _dp)]


class OdoImuOut(C.Structure):
    """vpl_odo_imu_out: the propagated state of the frame that entered slot 10, sum_dt of slots 9 and 10"""
    _fields_ = [("pose", C.c_double * 7), ("speed_bias", C.c_double * 9), ("sum_dt", C.c_double * 2)]


ODO_D2H_PAD_BYTES = 0    # VPL_ODO_D2H_PAD_BYTES: the session's read-backs are packed without alignment padding


class OdoKeyframeRule(C.Structure):
    """vpl_odo_keyframe_rule: MIN_PARALLAX (keyframe_parallax / FOCAL_LENGTH) and the track count below which every image is a keyframe"""
    _fields_ = [("min_parallax", C.c_double), ("min_track_num", C.c_int)]


class OdoDecision(C.Structure):
    """vpl_odo_decision: addFeatureCheckParallax's decision for the window as it stands, failureDetection's mask of the last solve"""
    _fields_ = [("flag", C.c_int), ("last_track_num", C.c_int), ("parallax_num", C.c_int), ("failure", C.c_int),
                ("parallax_sum", C.c_double), ("parallax_mean", C.c_double)]


class FailureLimits(C.Structure):
    """vpl_failure_limits: the four thresholds of Estimator::failureDetection (every comparison a strict >)"""
    _fields_ = [("max_acc_bias", C.c_double), ("max_gyr_bias", C.c_double), ("max_translation", C.c_double), ("max_z", C.c_double)]


ODO_DECISION_RECORD_BYTES = 24    # VPL_ODO_DECISION_RECORD_BYTES: what a rule-enabled session reads back per sequence and image
FAIL_ACC_BIAS, FAIL_GYR_BIAS, FAIL_TRANSLATION, FAIL_Z = 1, 2, 4, 8


class CSlideTracks(C.Structure):
    _fields_ = [("point_start", _ip), ("point_nobs", _ip), ("point_drop", _ip),
                ("line_start", _ip), ("line_nobs", _ip), ("line_drop", _ip)]


class SlideTracks:
    """vpl_slide_tracks of one window (include/vplines_ba.h)"""

    def __init__(self, n_points, n_lines):
        self.point_start, self.point_nobs, self.point_drop = (np.zeros(n_points, np.int32) for _ in range(3))
        self.line_start, self.line_nobs, self.line_drop = (np.zeros(n_lines, np.int32) for _ in range(3))

    def to_c(self, ct=None):
        ct = ct if ct is not None else CSlideTracks()
        for f, _ in CSlideTracks._fields_:
            setattr(ct, f, getattr(self, f).ctypes.data_as(_ip))
        return ct


_hip = None
PSD_WAVE16, PSD_WAVE48, PSD_WAVE4, PSD_WORKGROUP = 0, 1, 2, 3   # forms of vpl_ba_debug_psd_factor


def load_hip_library():
    """Loads libvplines_hip.so; raises (never falls back) when it is missing."""
    global _hip
    if _hip is not None:
        return _hip
    path = _build.HIP_LIB
    if not os.path.exists(path):
        raise RuntimeError("HIP extension %s is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                           "there is no CPU fallback" % path)
    # PyTorch ships a HIP runtime of its own: in a process that uses both, torch's must be the one that is loaded first (with
    # /opt/rocm's loaded and initialised first, torch.cuda afterwards reports "No HIP GPUs are available" -- seen on the GPU box)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.vpl_ba_default_options.argtypes = [C.POINTER(BaOptions)]
    lib.vpl_ctx_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.vpl_ctx_destroy.argtypes = [vp]
    lib.vpl_ctx_destroy.restype = None
    lib.vpl_ctx_set_stream.argtypes = [vp, vp]
    lib.vpl_ba_set_prior_rule.argtypes = [vp, C.c_int]
    lib.vpl_last_error.argtypes = [vp]
    lib.vpl_last_error.restype = C.c_char_p
    lib.vpl_preintegrate_batch.argtypes = [vp, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp, _dp, C.POINTER(BaOptions),
                                           C.POINTER(Preintegration)]
    lib.vpl_init_align_batch.argtypes = [vp, C.c_int, C.POINTER(CInitInput), C.POINTER(BaOptions), C.POINTER(InitResult),
                                         C.POINTER(Preintegration), C.POINTER(Preintegration)]
    lib.vpl_init_debug_jobs.argtypes = [C.c_int, _ip, _ip, _ip]
    lib.vpl_init_structure_batch.argtypes = [vp, C.c_int, C.POINTER(CSfmInput), C.POINTER(SfmResult), _dp, _dp, _ip, _dp]
    lib.vpl_sfm_debug_plan.argtypes = [C.c_int, C.c_int, _ip, _ip, _ip, _ip, _ip, _ip, _ip]
    _bp = C.POINTER(C.c_ubyte)
    lib.vpl_init_relative_pose_batch.argtypes = [vp, C.c_int, C.POINTER(CRelPoseInput), C.POINTER(RelPoseResult), _bp, _bp, _ip]
    lib.vpl_relpose_debug_plan.argtypes = [C.c_ulonglong, C.c_int, C.c_int, _ip, _ip]
    lib.vpl_loop_default_options.argtypes = [C.POINTER(LoopOptions)]
    lib.vpl_loop_default_options.restype = None
    lib.vpl_loop_verify_batch.argtypes = [vp, C.c_int, C.POINTER(CLoopInput), C.POINTER(LoopOptions), C.POINTER(LoopResult), _bp]
    lib.vpl_loop_debug_plan.argtypes = [C.c_ulonglong, C.c_int, C.c_double, C.c_int, _ip, _ip]
    lib.vpl_pg_default_options.argtypes = [C.POINTER(PgOptions)]
    lib.vpl_pg_default_options.restype = None
    lib.vpl_pg_optimize_batch.argtypes = [vp, C.c_int, C.POINTER(CPgInput), C.POINTER(PgOptions), C.POINTER(CPgResult)]
    lib.vpl_pg_debug_step.argtypes = [vp, C.POINTER(CPgInput), C.POINTER(PgOptions), _dp, _dp, _dp]
    lib.vpl_pg_optimize_seq_batch.argtypes = lib.vpl_pg_optimize_batch.argtypes
    lib.vpl_pg_debug_step_seq.argtypes = lib.vpl_pg_debug_step.argtypes
    lib.vpl_pgs_default_options.argtypes = [C.POINTER(PgsOptions)]
    lib.vpl_pgs_default_options.restype = None
    lib.vpl_pgs_create.argtypes = [vp, C.POINTER(PgsOptions), C.POINTER(vp)]
    lib.vpl_pgs_destroy.argtypes = [vp]
    lib.vpl_pgs_destroy.restype = None
    lib.vpl_pgs_add_keyframe.argtypes = [vp, C.POINTER(CPgsKeyframe), C.POINTER(CPgsKeyframeOut)]
    lib.vpl_pgs_load_keyframe.argtypes = [vp, C.POINTER(CPgsKeyframe), C.POINTER(CPgsKeyframeOut)]
    lib.vpl_pgs_optimize.argtypes = [vp, C.POINTER(CPgsResult)]
    lib.vpl_pgs_update_loop.argtypes = [vp, C.c_int, _dp, C.POINTER(C.c_int)]
    lib.vpl_pgs_get_path.argtypes = [vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip]
    lib.vpl_pgs_get_drift.argtypes = [vp, C.POINTER(C.c_double), _dp, _dp]
    lib.vpl_pgs_size.argtypes = [vp]
    lib.vpl_pgs_reset.argtypes = [vp]
    lib.vpl_gf_default_options.argtypes = [C.POINTER(GfOptions)]
    lib.vpl_gf_default_options.restype = None
    lib.vpl_gf_optimize_batch.argtypes = [vp, C.c_int, C.POINTER(CGfInput), C.POINTER(GfOptions), C.POINTER(CGfResult)]
    lib.vpl_gf_debug_step.argtypes = [vp, C.POINTER(CGfInput), C.POINTER(GfOptions), _dp, _dp, _dp]
    lib.vpl_gf_debug_plan.argtypes = [C.c_int, C.c_int, _ip, _ip, _ip, _ip]
    lib.vpl_gf_local_cartesian.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, _dp, _dp]
    lib.vpl_gf_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
    lib.vpl_gf_destroy.argtypes = [vp]
    lib.vpl_gf_destroy.restype = None
    lib.vpl_gf_input_odom.argtypes = [vp, C.c_double, _dp, _dp, _dp, _dp]
    lib.vpl_gf_input_gps.argtypes = [vp, C.c_double, _dp, C.c_double]
    lib.vpl_gf_optimize.argtypes = [vp, C.POINTER(GfOptions), C.POINTER(CGfResult)]
    lib.vpl_gf_get_path.argtypes = [vp, C.c_int, C.c_int, _dp]
    lib.vpl_init_visual_batch.argtypes = [vp, C.c_int, C.POINTER(CSfmInput), C.POINTER(C.c_ulonglong), C.POINTER(RelPoseResult),
                                          C.POINTER(SfmResult), _dp, _dp, _ip, _dp]
    lib.vpl_select_features_batch.argtypes = [vp, C.c_int, C.POINTER(SelectParams), C.POINTER(CSelectInput), C.POINTER(SelectResult), _ip, _dp]
    lib.vpl_select_debug_values.argtypes = [vp, C.POINTER(SelectParams), C.POINTER(CSelectInput), _ip, C.c_int, _dp, _dp, _dp, _dp]
    lib.vpl_select_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 3
    lib.vpl_sel_debug_book.argtypes = [C.c_int, C.c_int, C.c_int, _ip, _ip, _bp, _ip, _ip, C.c_int] + [_ip] * 8 + [C.c_int, _ip]
    for name in ("vpl_projection_factor_evaluate", "vpl_line_factor_evaluate", "vpl_vp_factor_evaluate"):
        getattr(lib, name).argtypes = [vp, C.c_int, _dp, _dp, C.c_double, _dp, _dp]
    lib.vpl_imu_factor_evaluate.argtypes = [vp, C.c_int, _dp, C.POINTER(Preintegration), C.c_double, _dp, _dp]
    lib.vpl_prior_factor_evaluate.argtypes = [vp, C.POINTER(Prior), _dp, _dp, _dp]
    lib.vpl_pose_plus.argtypes = [vp, C.c_int, _dp, _dp, _dp]
    lib.vpl_line_orth_plus.argtypes = [vp, C.c_int, _dp, _dp, _dp]
    lib.vpl_ba_upload.argtypes = [vp, C.c_int, C.POINTER(CWindow), C.POINTER(BaOptions)]
    lib.vpl_ba_solve.argtypes = [vp]
    lib.vpl_ba_upload_chained.argtypes = [vp, C.c_int, C.POINTER(CWindow), C.POINTER(BaOptions)]
    lib.vpl_ba_reset_state.argtypes = [vp]
    lib.vpl_ba_download.argtypes = [vp, C.c_int, C.POINTER(CWindow), C.POINTER(Prior), C.POINTER(SolveReport)]
    lib.vpl_ctx_synchronize.argtypes = [vp]
    lib.vpl_ba_pack_states_device.argtypes = [vp, C.c_int, vp]
    lib.vpl_ba_solve_windows.argtypes = [vp, C.c_int, C.POINTER(CWindow), C.POINTER(BaOptions), C.POINTER(Prior),
                                         C.POINTER(SolveReport)]
    lib.vpl_ba_triangulate_lines.argtypes = [vp, C.c_int, C.POINTER(CWindow)]
    lib.vpl_ba_marginalize.argtypes = [vp, C.c_int, C.POINTER(CWindow), C.POINTER(BaOptions), C.c_int, C.POINTER(Prior), _ip, _ip]
    lib.vpl_ba_slide_window.argtypes = [vp, C.c_int, C.POINTER(CWindow), C.c_int, C.c_double, C.POINTER(CSlideTracks)]
    lib.vpl_ba_triangulate_points.argtypes = [vp, C.c_int, C.POINTER(CWindow), C.c_double]
    lib.vpl_ba_only_line_opt.argtypes = [vp, C.c_int, C.POINTER(CWindow), C.POINTER(BaOptions), C.POINTER(SolveReport)]
    for name in ("vpl_ba_triangulate_lines", "vpl_ba_marginalize", "vpl_ba_slide_window", "vpl_ba_triangulate_points",
                 "vpl_ba_only_line_opt"):
        getattr(lib, name + "_async").argtypes = getattr(lib, name).argtypes
    lib.vpl_ba_collect.argtypes = [vp]
    lib.vpl_ba_solve_odometry.argtypes = [vp, C.c_int, C.POINTER(CWindow), C.POINTER(BaOptions), C.c_double, C.POINTER(Prior),
                                          C.POINTER(SolveReport), C.POINTER(SolveReport)]
    lib.vpl_ba_enable_kernel_timing.argtypes = [vp, C.c_int]
    lib.vpl_ba_kernel_times.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_char_p), _dp, _ip]
    lib.vpl_ba_launch_profile.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_char_p), _dp, _ip]
    lib.vpl_odo_create.argtypes = [C.POINTER(vp), vp, C.c_int, C.POINTER(BaOptions), C.c_double, C.c_int, C.c_int, C.c_int]
    lib.vpl_odo_destroy.argtypes = [vp]
    lib.vpl_odo_destroy.restype = None
    lib.vpl_odo_set_window.argtypes = [vp, C.c_int, _dp, _dp, _dp, C.POINTER(Preintegration), C.POINTER(OdoFrame)]
    lib.vpl_odo_init.argtypes = [vp, C.POINTER(CInitInput), _dp, C.POINTER(OdoFrame), C.POINTER(InitResult)]
    lib.vpl_odo_keyframe.argtypes = [vp, C.POINTER(OdoFrame), _ip, C.POINTER(OdoResult)]
    lib.vpl_odo_solve.argtypes = [vp, _ip, C.POINTER(OdoResult)]
    lib.vpl_odo_advance.argtypes = [vp, C.POINTER(OdoFrame), C.POINTER(OdoResult)]
    lib.vpl_odo_get_prior.argtypes = [vp, C.c_int, C.POINTER(Prior)]
    lib.vpl_odo_get_states.argtypes = [vp, C.c_int, _dp, _dp, _dp]
    lib.vpl_odo_get_tracks.argtypes = [vp, C.c_int, _ip, _ip, _ip, _ip, _dp, _ip, _ip, _ip, _ip, _ip, _dp]
    lib.vpl_odo_enable_imu.argtypes = [vp, C.c_int]
    lib.vpl_odo_set_imu.argtypes = [vp, C.c_int, C.c_int, _dp, _dp, _dp]
    lib.vpl_odo_advance_imu.argtypes = [vp, C.POINTER(OdoImuFrame), C.POINTER(OdoResult), C.POINTER(OdoImuOut)]
    lib.vpl_odo_keyframe_imu.argtypes = [vp, C.POINTER(OdoImuFrame), _ip, C.POINTER(OdoResult), C.POINTER(OdoImuOut)]
    lib.vpl_odo_get_preint.argtypes = [vp, C.c_int, C.POINTER(Preintegration)]
    _llp = C.POINTER(C.c_longlong)
    lib.vpl_odo_stats.argtypes = [vp, _llp, _llp, _llp]
    lib.vpl_odo_debug_ms.argtypes = [vp, _dp]
    lib.vpl_odo_select.argtypes = [vp, C.POINTER(SelectParams), C.POINTER(CSelectFrame), C.POINTER(OdoSelectResult), _ip, _dp, _ip]
    lib.vpl_odo_debug_tracks.argtypes = [C.c_int, C.c_int, _ip, _ip, _ip, C.POINTER(C.c_ubyte), _ip, _ip, _ip, _ip, _ip, _ip]
    lib.vpl_odo_default_keyframe_rule.argtypes = [C.POINTER(OdoKeyframeRule)]
    lib.vpl_odo_default_keyframe_rule.restype = None
    lib.vpl_odo_enable_keyframe_rule.argtypes = [vp, C.POINTER(OdoKeyframeRule)]
    lib.vpl_odo_get_decision.argtypes = [vp, C.c_int, C.POINTER(OdoDecision)]
    lib.vpl_odo_solve_auto.argtypes = [vp, C.POINTER(OdoResult)]
    lib.vpl_odo_keyframe_auto.argtypes = [vp, C.POINTER(OdoFrame), C.POINTER(OdoResult)]
    lib.vpl_odo_keyframe_imu_auto.argtypes = [vp, C.POINTER(OdoImuFrame), C.POINTER(OdoResult), C.POINTER(OdoImuOut)]
    lib.vpl_failure_default_limits.argtypes = [C.POINTER(FailureLimits)]
    lib.vpl_failure_default_limits.restype = None
    lib.vpl_failure_detection.argtypes = [C.POINTER(FailureLimits), _dp, _dp, _dp]
    lib.vpl_odo_debug_parallax_list.argtypes = [C.c_int, C.c_int, _ip, _ip, _ip, C.POINTER(C.c_ubyte), _ip, _ip, _ip]
    lib.vpl_ba_debug_marg_Ab.argtypes = [vp, C.c_int, _dp, _dp]
    lib.vpl_ba_debug_linearization.argtypes = [vp, C.c_int, _ip, _ip, _ip] + [_dp] * 8
    lib.vpl_ba_debug_step.argtypes = [vp, C.c_int] + [_dp] * 5 + [_ip] + [_dp] * 5
    lib.vpl_ba_debug_allocs.argtypes = [vp, _llp, _llp]
    lib.vpl_ba_debug_psd_factor.argtypes = [vp, C.c_int, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _ip, _ip, _dp, _dp]
    _hip = lib
    return lib


def _p(a):
    return a.ctypes.data_as(_dp)


class Context:
    """One vpl_ctx (device buffers + stream of one GPU)."""

    def __init__(self, device=0, max_windows=1, max_points=256, max_point_obs=2816, max_lines=128,
                 max_line_obs=1408, stream=None):
        self.lib = load_hip_library()
        self.h = C.c_void_p()
        rc = self.lib.vpl_ctx_create(C.byref(self.h), device, max_windows, max_points, max_point_obs, max_lines,
                                     max_line_obs)
        if rc != 0:
            raise RuntimeError("vpl_ctx_create failed: %d" % rc)
        if stream is not None:
            self.set_stream(stream)
        self._cw = None
        self._windows = []

    def debug_guards(self):
        """VPL_DEBUG_GUARDS=1 (set before the context is made): number of device arrays with a write behind their end"""
        return int(self.lib.vpl_ba_debug_guards(self.h))

    def debug_allocs(self):
        """(arrays in the context's allocation record, their payload bytes): the context's own and those of the session it lends
        itself to"""
        n, b = C.c_longlong(0), C.c_longlong(0)
        self._check(self.lib.vpl_ba_debug_allocs(self.h, C.byref(n), C.byref(b)), "vpl_ba_debug_allocs")
        return int(n.value), int(b.value)

    def debug_psd_factor(self, form, threads, cases):
        """vpl_ba_debug_psd_factor: one form of the pivoted Cholesky factorisation of csrc/ba_psd.h (PSD_WAVE16, PSD_WAVE48,
        PSD_WAVE4, PSD_WORKGROUP) on `threads` threads over cases = [(A (n x n), b (n), abs_tol, rel_tol), ...], one launch.
        -> list of (rank, perm (n), J0 (n x n), r0 (n)); J0 and r0 hold NaN where the kernel wrote nothing.  Returns the
        VPL_E_* code instead when the call is refused."""
        import numpy as np
        N, M = len(cases), 80
        ns = np.array([np.asarray(c[0]).shape[0] for c in cases], dtype=np.int32)
        A = np.zeros((N, M * M)); b = np.zeros((N, M)); at = np.zeros(N); rt = np.zeros(N)
        for i, (Ai, bi, ai, ri) in enumerate(cases):
            n = int(ns[i])
            if n <= M:
                A[i, : n * n] = np.asarray(Ai, dtype=np.float64).reshape(-1)
                b[i, :n] = bi
            at[i], rt[i] = ai, ri
        rank = np.zeros(N, dtype=np.int32); perm = np.zeros((N, M), dtype=np.int32)
        J0 = np.zeros((N, M * M)); r0 = np.zeros((N, M))
        ip = lambda a: a.ctypes.data_as(_ip)
        rc = self.lib.vpl_ba_debug_psd_factor(self.h, form, threads, N, ip(ns), _p(A), _p(b), _p(at), _p(rt), ip(rank), ip(perm),
                                              _p(J0), _p(r0))
        if rc != 0:
            return rc
        return [(int(rank[i]), perm[i, : ns[i]].copy(), J0[i, : ns[i] * ns[i]].reshape(ns[i], ns[i]).copy(), r0[i, : ns[i]].copy())
                for i in range(N)]

    TR_FIELDS = ("radius", "mu", "alpha", "a1", "a2", "a3", "model_cost_change", "dogleg_step_norm", "step_norm", "x_norm",
                 "iter", "status", "num_successful", "step_valid")      # tr14 of vpl_ba_debug_step, the last four integers

    def _debug_counts(self, w):
        nP, nL = C.c_int(0), C.c_int(0)
        n = self.lib.vpl_ba_debug_linearization(self.h, w, C.byref(nP), C.byref(nL), *([None] * 9))
        if n < 0:
            self._check(n, "vpl_ba_debug_linearization")
        return n, nP.value, nL.value

    def debug_linearization(self, w):
        """vpl_ba_debug_linearization: the linearisation of window w of the uploaded batch as the step kernels read it.  -> dict:
        n, n_points, n_lines, line_index [n_lines] (the caller's index of every device line), H [n, n], g [n] over the window's
        full index (171 cam dims | inverse depths | line dims in fours), the current states pose [11, 7], speed_bias [11, 9],
        ex_pose [7], inv_depth [n_points], line_orth [n_lines, 4] and x_cost."""
        self._settle()
        n, nP, nL = self._debug_counts(w)
        idx = np.zeros(max(nL, 1), np.int32)
        H, g = np.zeros((n, n)), np.zeros(n)
        pose, sb, ex = np.zeros((NF, 7)), np.zeros((NF, 9)), np.zeros(7)
        invd, orth, cost = np.zeros(max(nP, 1)), np.zeros((max(nL, 1), 4)), np.zeros(1)
        rc = self.lib.vpl_ba_debug_linearization(self.h, w, None, None, idx.ctypes.data_as(_ip), _p(H), _p(g), _p(pose), _p(sb),
                                                 _p(ex), _p(invd), _p(orth), _p(cost))
        if rc != n:
            self._check(rc if rc < 0 else -1, "vpl_ba_debug_linearization")
        return dict(n=n, n_points=nP, n_lines=nL, line_index=idx[:nL].copy(), H=H, g=g, pose=pose, speed_bias=sb, ex_pose=ex,
                    inv_depth=invd[:nP].copy(), line_orth=orth[:nL].copy(), x_cost=float(cost[0]))

    def debug_step(self, w):
        """vpl_ba_debug_step: the step of the last iteration of window w.  -> dict: n, scale / diag / grad / gn [n], the TR_FIELDS
        of the trust-region state (floats, the last four ints), path, and the candidate states pose_c [11, 7], speed_bias_c
        [11, 9], ex_pose_c [7], inv_depth_c [n_points], line_orth_c [n_lines, 4]."""
        self._settle()
        n, nP, nL = self._debug_counts(w)
        scale, diag, grad, gn = (np.zeros(n) for _ in range(4))
        tr, path = np.zeros(14), C.c_int(-1)
        pose, sb, ex = np.zeros((NF, 7)), np.zeros((NF, 9)), np.zeros(7)
        invd, orth = np.zeros(max(nP, 1)), np.zeros((max(nL, 1), 4))
        rc = self.lib.vpl_ba_debug_step(self.h, w, _p(scale), _p(diag), _p(grad), _p(gn), _p(tr), C.byref(path), _p(pose), _p(sb),
                                        _p(ex), _p(invd), _p(orth))
        if rc != n:
            self._check(rc if rc < 0 else -1, "vpl_ba_debug_step")
        out = dict(n=n, scale=scale, diag=diag, grad=grad, gn=gn, path=path.value, pose_c=pose, speed_bias_c=sb, ex_pose_c=ex,
                   inv_depth_c=invd[:nP].copy(), line_orth_c=orth[:nL].copy())
        for k, f in enumerate(self.TR_FIELDS):
            out[f] = float(tr[k]) if k < 10 else int(tr[k])
        return out

    def close(self):
        if self.h and getattr(self, "_odo", None) is not None:
            self._odo._destroy()                   # the session goes before the context it borrows (vpl_odo_destroy reads the context)
        if self.h:
            bad = self.debug_guards() if os.environ.get("VPL_DEBUG_GUARDS") == "1" else 0
            msg = self.lib.vpl_last_error(self.h).decode() if bad else ""
            self.lib.vpl_ctx_destroy(self.h)
            self.h = C.c_void_p()
            if bad:
                import sys
                print("vpl_ba_debug_guards: %d arrays overrun; %s" % (bad, msg), file=sys.stderr)    # (also when closed by __del__)
                raise RuntimeError("vpl_ba_debug_guards: %d arrays overrun; %s" % (bad, msg))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.vpl_last_error(self.h)
            raise RuntimeError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))

    def set_stream(self, stream_ptr):
        self._settle()
        self._check(self.lib.vpl_ctx_set_stream(self.h, C.c_void_p(stream_ptr)), "vpl_ctx_set_stream")

    def set_prior_rule(self, rule):
        """PRIOR_PIVOTED_CHOLESKY (default) or PRIOR_EIGEN (the reference's eigen-decomposed prior); an enqueued call is
        collected first"""
        self._settle()
        self._check(self.lib.vpl_ba_set_prior_rule(self.h, int(rule)), "vpl_ba_set_prior_rule")

    def synchronize(self):
        self._check(self.lib.vpl_ctx_synchronize(self.h), "vpl_ctx_synchronize")
        self._after_collect()

    def collect(self):
        """vpl_ba_collect: completes the call that was enqueued with async_=True (its results are in the Windows / the returned
        objects afterwards)"""
        self._check(self.lib.vpl_ba_collect(self.h), "vpl_ba_collect")
        self._after_collect()

    def _settle(self):
        """an enqueued call is completed before anything else touches the context (the library does the same on its side)"""
        if getattr(self, "_pending_refs", None) is not None:
            self.collect()

    def _after_collect(self):
        fin, self._pending_fin = getattr(self, "_pending_fin", None), None
        self._pending_refs = None
        if fin:
            fin()

    def _call5(self, name, async_, refs, fin, *args):
        """one of the five line-map entry points, synchronous or enqueued (vpl_ba_<name>[_async])"""
        self._settle()
        fn = getattr(self.lib, name + ("_async" if async_ else ""))
        self._check(fn(self.h, *args), name)
        if async_:
            self._pending_refs, self._pending_fin = refs, fin      # keep the C arrays alive until the call is collected
        elif fin:
            fin()

    # ---- single factor evaluators -------------------------------------------------
    def _factor(self, fn, params, consts, sqrt_info, nres, njac, want_jac=True):
        params = _arr(params, np.float64)
        consts = _arr(consts, np.float64)
        n = params.shape[0]
        res = np.zeros((n, nres))
        jac = np.zeros((n, njac)) if want_jac else None
        rc = fn(self.h, n, _p(params), _p(consts), sqrt_info, _p(res), _p(jac) if want_jac else None)
        self._check(rc, fn.__name__)
        return res, jac

    def projection_factor(self, params, pts, sqrt_info=460.0 / 1.5, want_jac=True):
        return self._factor(self.lib.vpl_projection_factor_evaluate, params, pts, sqrt_info, 2, 44, want_jac)

    def line_factor(self, params, obs, sqrt_info=306.666666667, want_jac=True):
        return self._factor(self.lib.vpl_line_factor_evaluate, params, obs, sqrt_info, 2, 36, want_jac)

    def vp_factor(self, params, vp, sqrt_info=10.0, want_jac=True):
        return self._factor(self.lib.vpl_vp_factor_evaluate, params, vp, sqrt_info, 2, 36, want_jac)

    def imu_factor(self, params, pre_array, g_norm=9.81007, want_jac=True):
        params = _arr(params, np.float64)
        n = params.shape[0]
        res = np.zeros((n, 15))
        jac = np.zeros((n, 480)) if want_jac else None
        rc = self.lib.vpl_imu_factor_evaluate(self.h, n, _p(params), pre_array, g_norm, _p(res),
                                              _p(jac) if want_jac else None)
        self._check(rc, "vpl_imu_factor_evaluate")
        return res, jac

    def prior_factor(self, prior, params, want_jac=True):
        params = _arr(params, np.float64)
        n = prior.n
        res = np.zeros(n)
        jac = np.zeros(n * params.size) if want_jac else None
        rc = self.lib.vpl_prior_factor_evaluate(self.h, C.byref(prior), _p(params), _p(res),
                                                _p(jac) if want_jac else None)
        self._check(rc, "vpl_prior_factor_evaluate")
        return res, jac

    def pose_plus(self, x, delta):
        x = _arr(x, np.float64)
        delta = _arr(delta, np.float64)
        out = np.zeros_like(x)
        self._check(self.lib.vpl_pose_plus(self.h, x.shape[0], _p(x), _p(delta), _p(out)), "vpl_pose_plus")
        return out

    def line_orth_plus(self, x, delta):
        x = _arr(x, np.float64)
        delta = _arr(delta, np.float64)
        out = np.zeros_like(x)
        self._check(self.lib.vpl_line_orth_plus(self.h, x.shape[0], _p(x), _p(delta), _p(out)), "vpl_line_orth_plus")
        return out

    def preintegrate(self, offset, nsamples, samples, acc0, gyr0, ba, bg, opt):
        offset = _arr(offset, np.int32)
        nsamples = _arr(nsamples, np.int32)
        n = len(offset)
        out = (Preintegration * n)()
        samples, acc0, gyr0, ba, bg = (_arr(a, np.float64) for a in (samples, acc0, gyr0, ba, bg))
        rc = self.lib.vpl_preintegrate_batch(self.h, n, offset.ctypes.data_as(_ip), nsamples.ctypes.data_as(_ip),
                                             _p(samples), _p(acc0), _p(gyr0), _p(ba), _p(bg), C.byref(opt), out)
        self._check(rc, "vpl_preintegrate_batch")
        return out

    def init_align(self, inputs, opt, want_preint=True, check=True):
        """vpl_init_align_batch over a list of InitInput: the visual-inertial alignment (gyroscope bias, scale, gravity, the state
        change) of every sequence in one call.  -> (results [n] of InitResult, window pre-integrations [n][11], image
        pre-integrations [n][INIT_MAX_FRAMES]); the last two None without want_preint.  check=False: a refusal comes back as its
        VPL_E_* code instead of an exception."""
        self._settle()
        n = len(inputs)
        ci = (CInitInput * n)()
        for i, q in enumerate(inputs):
            if isinstance(q, CInitInput):
                C.memmove(C.byref(ci[i]), C.byref(q), C.sizeof(CInitInput))   # as the caller filled it (tests of the refusals)
            else:
                q.to_c(ci[i])
        res = (InitResult * n)()
        wpre = ((Preintegration * NF) * n)() if want_preint else None
        ipre = ((Preintegration * INIT_MAX_FRAMES) * n)() if want_preint else None
        rc = self.lib.vpl_init_align_batch(self.h, n, ci, C.byref(opt), res,
                                           C.cast(wpre, C.POINTER(Preintegration)) if want_preint else None,
                                           C.cast(ipre, C.POINTER(Preintegration)) if want_preint else None)
        if rc != 0 and not check:
            return rc
        self._check(rc, "vpl_init_align_batch")
        return res, wpre, ipre

    def init_structure(self, inputs, check=True):
        """vpl_init_structure_batch over a list of SfmInput: GlobalSFM::construct and the PnP of the non-key image frames of every
        sequence in one call.  -> (results [n] of SfmResult, points_chain [n, SFM_MAX_TRACKS, 3], points_ba [the same], tracked: per
        sequence (ids [k], xyz [k, 3]) = sfm_tracked_points).  check=False: a refusal comes back as its VPL_E_* code instead of an
        exception."""
        self._settle()
        n = len(inputs)
        ci = (CSfmInput * n)()
        for i, q in enumerate(inputs):
            if isinstance(q, CSfmInput):
                C.memmove(C.byref(ci[i]), C.byref(q), C.sizeof(CSfmInput))   # as the caller filled it (tests of the refusals)
            else:
                q.to_c(ci[i])
        res = (SfmResult * n)()
        pc, pb, txyz = (np.zeros((n, SFM_MAX_TRACKS, 3)) for _ in range(3))
        tid = np.zeros((n, SFM_MAX_TRACKS), dtype=np.int32)
        rc = self.lib.vpl_init_structure_batch(self.h, n, ci, res, _p(pc), _p(pb), tid.ctypes.data_as(_ip), _p(txyz))
        if rc != 0 and not check:
            return rc
        self._check(rc, "vpl_init_structure_batch")
        return res, pc, pb, [(tid[i, :res[i].n_tracked].copy(), txyz[i, :res[i].n_tracked].copy()) for i in range(n)]

    def init_relative_pose(self, inputs, check=True, want_masks=True, want_hyp=True):
        """vpl_init_relative_pose_batch over a list of RelPoseInput: Estimator::relativePose -- the RANSAC of findFundamentalMat and
        recoverPose for every candidate frame 0 .. 9 of every sequence, and the choice of l -- in one call.  -> (results [n] of
        RelPoseResult, mask_ransac [n, 10, SFM_MAX_TRACKS] uint8, mask_pose [the same], hyp_count [n, 10, 1000, 3] int32); the
        optional arrays None when not wanted.  check=False: a refusal comes back as its VPL_E_* code instead of an exception."""
        self._settle()
        n = len(inputs)
        ci = (CRelPoseInput * n)()
        for i, q in enumerate(inputs):
            if isinstance(q, CRelPoseInput):
                C.memmove(C.byref(ci[i]), C.byref(q), C.sizeof(CRelPoseInput))   # as the caller filled it (tests of the refusals)
            else:
                q.to_c(ci[i])
        res = (RelPoseResult * n)()
        m0 = np.zeros((n, NF - 1, SFM_MAX_TRACKS), dtype=np.uint8) if want_masks else None
        m1 = np.zeros((n, NF - 1, SFM_MAX_TRACKS), dtype=np.uint8) if want_masks else None
        hyp = np.zeros((n, NF - 1, RELPOSE_MAX_ITERS, 3), dtype=np.int32) if want_hyp else None
        _bp = C.POINTER(C.c_ubyte)
        rc = self.lib.vpl_init_relative_pose_batch(self.h, n, ci, res, m0.ctypes.data_as(_bp) if want_masks else None,
                                                   m1.ctypes.data_as(_bp) if want_masks else None,
                                                   hyp.ctypes.data_as(_ip) if want_hyp else None)
        if rc != 0 and not check:
            return rc
        self._check(rc, "vpl_init_relative_pose_batch")
        return res, m0, m1, hyp

    def loop_verify(self, inputs, options=None, check=True):
        """vpl_loop_verify_batch over a list of LoopInput: KeyFrame::findConnection from the PnP RANSAC on -- the inliers, PnP_T_old
        / PnP_R_old, loop_info and has_loop of every item -- in one call.  -> (results [n] of LoopResult, status per item [count]
        uint8).  check=False: a refusal comes back as its VPL_E_* code instead of an exception."""
        self._settle()
        n = len(inputs)
        ci = (CLoopInput * n)()
        for i, q in enumerate(inputs):
            if isinstance(q, CLoopInput):
                C.memmove(C.byref(ci[i]), C.byref(q), C.sizeof(CLoopInput))   # as the caller filled it (tests of the refusals)
            else:
                q.to_c(ci[i])
        opt = options if options is not None else default_loop_options()
        res = (LoopResult * n)()
        st = np.zeros((n, LOOP_MAX_POINTS), dtype=np.uint8)
        rc = self.lib.vpl_loop_verify_batch(self.h, n, ci, C.byref(opt), res, st.ctypes.data_as(C.POINTER(C.c_ubyte)))
        if rc != 0 and not check:
            return rc
        self._check(rc, "vpl_loop_verify_batch")
        return res, [st[i, :ci[i].count].copy() for i in range(n)]

    @staticmethod
    def _pg_c(inputs):
        ci = (CPgInput * len(inputs))()
        for i, q in enumerate(inputs):
            if isinstance(q, CPgInput):
                C.memmove(C.byref(ci[i]), C.byref(q), C.sizeof(CPgInput))   # as the caller filled it (tests of the refusals)
            else:
                q.to_c(ci[i])
        return ci

    def pose_graph_optimize(self, inputs, opt=None, check=True, _call="vpl_pg_optimize_batch"):
        """vpl_pg_optimize_batch over a list of PoseGraphInput: PoseGraph::optimize4DoF per graph -- the corrected poses, the drift
        and the drift-corrected tail -- in one call.  -> list of PoseGraphResult.  check=False: a refusal comes back as its
        VPL_E_* code instead of an exception."""
        self._settle()
        n = len(inputs)
        ci = self._pg_c(inputs)
        opt = opt if opt is not None else default_pg_options()
        res = (CPgResult * n)()
        out = []
        for i in range(n):
            nn, nt = max(int(ci[i].n), 0), max(int(ci[i].n_tail), 0)
            arrs = (np.zeros((nn, 3)), np.zeros((nn, 3, 3)), np.zeros((nt, 3)), np.zeros((nt, 3, 3)))
            res[i].T, res[i].R, res[i].tail_T, res[i].tail_R = (a.ctypes.data_as(_dp) for a in arrs)
            out.append(arrs)
        rc = getattr(self.lib, _call)(self.h, n, ci, C.byref(opt), res)
        if rc != 0 and not check:
            return rc
        self._check(rc, _call)
        return [PoseGraphResult(res[i], *out[i]) for i in range(n)]

    def pose_graph_optimize_seq(self, inputs, opt=None, check=True):
        """vpl_pg_optimize_seq_batch: pose_graph_optimize with every graph's `sequence` honoured -- nodes of sequence 0 are
        constant, sequential edges stay inside a sequence, loop edges may join two.  Same arguments, same result."""
        return self.pose_graph_optimize(inputs, opt, check, "vpl_pg_optimize_seq_batch")

    def pose_graph_debug_step(self, q, opt=None, _call="vpl_pg_debug_step"):
        """vpl_pg_debug_step: the first linear solve of one graph -> dict g, step [4 (n - 1)], model_cost_change"""
        self._settle()
        ci = self._pg_c([q])
        opt = opt if opt is not None else default_pg_options()
        m = 4 * (int(ci[0].n) - 1)
        g, step, mc = np.zeros(max(m, 1)), np.zeros(max(m, 1)), np.zeros(1)
        rc = getattr(self.lib, _call)(self.h, ci, C.byref(opt), g.ctypes.data_as(_dp), step.ctypes.data_as(_dp), mc.ctypes.data_as(_dp))
        self._check(rc, _call)
        return dict(g=g[:m], step=step[:m], model_cost_change=float(mc[0]))

    def pose_graph_debug_step_seq(self, q, opt=None):
        """vpl_pg_debug_step_seq: pose_graph_debug_step with the graph's `sequence` honoured"""
        return self.pose_graph_debug_step(q, opt, "vpl_pg_debug_step_seq")

    @staticmethod
    def _gf_c(inputs):
        ci = (CGfInput * len(inputs))()
        for i, q in enumerate(inputs):
            if isinstance(q, CGfInput):
                C.memmove(C.byref(ci[i]), C.byref(q), C.sizeof(CGfInput))   # as the caller filled it (tests of the refusals)
            else:
                q.to_c(ci[i])
        return ci

    def global_fusion(self, inputs, options=None, check=True):
        """vpl_gf_optimize_batch over a list of GlobalFusionInput: GlobalOptimization::optimize per chain -- the global poses and
        WGPS_T_WVIO -- in one call.  -> list of GlobalFusionResult.  check=False: a refusal comes back as its VPL_E_* code instead of
        an exception."""
        self._settle()
        n = len(inputs)
        ci = self._gf_c(inputs)
        opt = options if options is not None else default_gf_options()
        res = (CGfResult * n)()
        out = []
        for i in range(n):
            pose = np.zeros((max(int(ci[i].n), 0), 7))
            res[i].pose = pose.ctypes.data_as(_dp)
            out.append(pose)
        rc = self.lib.vpl_gf_optimize_batch(self.h, n, ci, C.byref(opt), res)
        if rc != 0 and not check:
            return rc
        self._check(rc, "vpl_gf_optimize_batch")
        return [GlobalFusionResult(res[i], out[i]) for i in range(n)]

    def global_fusion_debug_step(self, q, options=None):
        """vpl_gf_debug_step: the first linear solve of one chain -> dict g, step [6 n], model_cost_change"""
        self._settle()
        ci = self._gf_c([q])
        opt = options if options is not None else default_gf_options()
        m = 6 * max(int(ci[0].n), 1)
        g, step, mc = np.zeros(m), np.zeros(m), np.zeros(1)
        rc = self.lib.vpl_gf_debug_step(self.h, ci, C.byref(opt), g.ctypes.data_as(_dp), step.ctypes.data_as(_dp), mc.ctypes.data_as(_dp))
        self._check(rc, "vpl_gf_debug_step")
        return dict(g=g, step=step, model_cost_change=float(mc[0]))

    @staticmethod
    def _select_c(params, inputs):
        par = params if isinstance(params, SelectParams) else SelectParams.of(params)
        ci = (CSelectInput * len(inputs))()
        keep = []
        for i, q in enumerate(inputs):
            if isinstance(q, CSelectInput):
                C.memmove(C.byref(ci[i]), C.byref(q), C.sizeof(CSelectInput))   # as the caller filled it (tests of the refusals)
            else:
                q = q if isinstance(q, SelectInput) else SelectInput.of(q)
                keep.append(q)
                q.to_c(ci[i])
        return par, ci, keep

    def select_features(self, params, inputs, check=True):
        """vpl_select_features_batch over a list of SelectInput (or of objects with its members): FeatureSelector::select's horizon,
        motion information, per-feature information and greedy selection for every sequence in one call.  -> list [n] of dict
        ids (in selection order), f (of every selection), n_invisible, n_ineligible, n_candidates.  check=False: a refusal comes
        back as its VPL_E_* code instead of an exception."""
        self._settle()
        n = len(inputs)
        par, ci, keep = self._select_c(params, inputs)
        res = (SelectResult * max(n, 1))()
        ids = np.zeros((max(n, 1), SEL_MAX_FEATURES), dtype=np.int32)
        f = np.zeros((max(n, 1), SEL_MAX_FEATURES))
        rc = self.lib.vpl_select_features_batch(self.h, n, C.byref(par), ci, res, ids.ctypes.data_as(_ip), _p(f))
        if rc != 0 and not check:
            return rc
        self._check(rc, "vpl_select_features_batch")
        return [dict(ids=ids[i, :res[i].n_selected].copy(), f=f[i, :res[i].n_selected].copy(), n_invisible=res[i].n_invisible,
                     n_ineligible=res[i].n_ineligible, n_candidates=res[i].n_candidates) for i in range(n)]

    def select_debug_values(self, params, inp, prefix=(), check=True):
        """vpl_select_debug_values: one round's f and ub of every new feature of one sequence after the ids of `prefix` have been
        taken (NaN for what is not a candidate), Omega_kkH [45, 45] and the Delta12 [n_new + n_used, 78] of every feature"""
        self._settle()
        par, ci, keep = self._select_c(params, [inp])
        n_new, nf = ci[0].n_new, ci[0].n_new + ci[0].n_used
        pre = _arr(list(prefix), np.int32)
        f, ub = np.zeros(max(n_new, 1)), np.zeros(max(n_new, 1))
        om, d12 = np.zeros((45, 45)), np.zeros((max(nf, 1), 78))
        rc = self.lib.vpl_select_debug_values(self.h, C.byref(par), ci, pre.ctypes.data_as(_ip), len(pre), _p(f), _p(ub), _p(om), _p(d12))
        if rc != 0 and not check:
            return rc
        self._check(rc, "vpl_select_debug_values")
        return dict(f=f[:n_new], ub=ub[:n_new], omega=om, delta12=d12[:nf])

    def select_stats(self):
        """vpl_select_stats: (kernel launches, bytes up, bytes down) of the last selector call"""
        a, b, d = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        self._check(self.lib.vpl_select_stats(self.h, C.byref(a), C.byref(b), C.byref(d)), "vpl_select_stats")
        return int(a.value), int(b.value), int(d.value)

    def init_visual(self, inputs, seeds=None, check=True):
        """The vision-only start in one go: init_relative_pose over the track tables of a list of SfmInput (their l / relative_R /
        relative_T are not read), those three copied into the sequences whose relative pose succeeded, init_structure over these.
        seeds: one per sequence, default 0.  -> (relative-pose results [n] of RelPoseResult, structure: a list [n] with
        (SfmResult, points_chain [SFM_MAX_TRACKS, 3], points_ba, (ids, xyz)) per sequence, None where the relative pose failed).
        vpl_init_visual_batch is the same composition in C."""
        seeds = [0] * len(inputs) if seeds is None else list(seeds)
        rel = self.init_relative_pose([RelPoseInput.of(q, s) for q, s in zip(inputs, seeds)], check=check, want_masks=False, want_hyp=False)
        if isinstance(rel, int):
            return rel
        rel = rel[0]
        go = [i for i in range(len(inputs)) if rel[i].ok]
        filled = []
        for i in go:
            ci = inputs[i].to_c()                     # (points into the arrays of inputs[i])
            ci.l = rel[i].l
            for k in range(9):
                ci.relative_R[k] = rel[i].relative_R[k]
            for k in range(3):
                ci.relative_T[k] = rel[i].relative_T[k]
            filled.append(ci)
        out = [None] * len(inputs)
        if go:
            st = self.init_structure(filled, check=check)
            if isinstance(st, int):
                return st
            res, pc, pb, tr = st
            for k, i in enumerate(go):
                out[i] = (res[k], pc[k], pb[k], tr[k])
        return rel, out

    # ---- window solve ---------------------------------------------------------------
    def upload(self, windows, opt, chained=False):
        """chained=True: vpl_ba_upload_chained -- every window takes the prior the previous solve of this context left for it
        (device resident), the Windows' own .prior is ignored"""
        self._settle()
        n = len(windows)
        cw = (CWindow * n)()
        for i, w in enumerate(windows):
            w.to_c(cw[i])
        self._cw = cw
        self._windows = windows
        if chained:
            self._check(self.lib.vpl_ba_upload_chained(self.h, n, cw, C.byref(opt)), "vpl_ba_upload_chained")
        else:
            self._check(self.lib.vpl_ba_upload(self.h, n, cw, C.byref(opt)), "vpl_ba_upload")

    def solve(self):
        self._check(self.lib.vpl_ba_solve(self.h), "vpl_ba_solve")

    def reset_state(self):
        self._check(self.lib.vpl_ba_reset_state(self.h), "vpl_ba_reset_state")

    def download(self):
        n = len(self._windows)
        if n == 0 or self._cw is None:
            self._check(self.lib.vpl_ba_download(self.h, 0, None, None, None), "vpl_ba_download")   # (refused: nothing uploaded)
        priors = (Prior * n)()
        reports = (SolveReport * n)()
        self._check(self.lib.vpl_ba_download(self.h, n, self._cw, priors, reports), "vpl_ba_download")
        for i, w in enumerate(self._windows):
            w.from_c(self._cw[i])
        return priors, reports

    def solve_windows(self, windows, opt):
        self._settle()
        self.upload(windows, opt)
        self.solve()
        self.synchronize()
        return self.download()

    def solve_odometry(self, windows, opt, init_depth=5.0):
        """vpl_ba_solve_odometry: triangulate || (triangulateLine -> onlyLineOpt) -> solve, in place; (priors, line reports, reports)"""
        self._settle()
        n = len(windows)
        cw = (CWindow * n)()
        for i, w in enumerate(windows):
            w.to_c(cw[i])
        priors = (Prior * n)()
        lreps = (SolveReport * n)()
        reps = (SolveReport * n)()
        t0 = time.perf_counter()
        rc = self.lib.vpl_ba_solve_odometry(self.h, n, cw, C.byref(opt), init_depth, priors, lreps, reps)
        self.last_call_s = time.perf_counter() - t0      # the C call alone (tools/time_odometry.py)
        self._check(rc, "vpl_ba_solve_odometry")
        for i, w in enumerate(windows):
            w.from_c(cw[i])
        return priors, lreps, reps

    def pack_states_device(self, n, data_ptr):
        """vpl_ba_pack_states_device: the [n][183] states of the solved batch into a device buffer (raw pointer)"""
        self._check(self.lib.vpl_ba_pack_states_device(self.h, n, C.c_void_p(data_ptr)), "vpl_ba_pack_states_device")

    def marginalize(self, windows, opt, flag, async_=False):
        """vpl_ba_marginalize: (priors, m, n) of the windows' current states, no solve"""
        n = len(windows)
        cw = (CWindow * n)()
        for i, w in enumerate(windows):
            w.to_c(cw[i])
        priors = (Prior * n)()
        m = np.zeros(n, np.int32)
        nn = np.zeros(n, np.int32)
        self._call5("vpl_ba_marginalize", async_, (cw, windows, priors, m, nn, opt), None, n, cw, C.byref(opt), flag, priors,
                    m.ctypes.data_as(_ip), nn.ctypes.data_as(_ip))
        return priors, m, nn

    def triangulate_lines(self, windows, async_=False):
        """FeatureManager::triangulateLine on the device; updates line_plk / line_triangulated of the Windows in place"""
        n = len(windows)
        cw = (CWindow * n)()
        for i, w in enumerate(windows):
            w.to_c(cw[i])
        self._call5("vpl_ba_triangulate_lines", async_, (cw, windows), None, n, cw)

    def slide_window(self, windows, marginalization_flag, init_depth=5.0, async_=False):
        """Estimator::slideWindow; pose / speed_bias / inv_depth / line_plk of the Windows change in place,
        returns one SlideTracks (new start / nobs / dropped observation per track) per window"""
        n = len(windows)
        cw = (CWindow * n)()
        ct = (CSlideTracks * n)()
        res = []
        for i, w in enumerate(windows):
            w.to_c(cw[i])
            res.append(SlideTracks(len(w.point_start), len(w.line_start)))
            res[-1].to_c(ct[i])
        def fin():
            for i, w in enumerate(windows):
                w.from_c(cw[i])
        self._call5("vpl_ba_slide_window", async_, (cw, ct, windows, res), fin, n, cw, marginalization_flag, init_depth, ct)
        return res

    def triangulate_points(self, windows, init_depth=5.0, async_=False):
        """FeatureManager::triangulate on the device; updates inv_depth of the Windows in place"""
        n = len(windows)
        cw = (CWindow * n)()
        for i, w in enumerate(windows):
            w.to_c(cw[i])
        self._call5("vpl_ba_triangulate_points", async_, (cw, windows), None, n, cw, init_depth)

    def only_line_opt(self, windows, opt, async_=False):
        """Estimator::onlyLineOpt on the device; updates line_plk / line_removed in place, returns the reports"""
        n = len(windows)
        cw = (CWindow * n)()
        for i, w in enumerate(windows):
            w.to_c(cw[i])
        reps = (SolveReport * n)()
        self._call5("vpl_ba_only_line_opt", async_, (cw, windows, reps, opt), None, n, cw, C.byref(opt), reps)
        return reps

    def enable_kernel_timing(self, on=True):
        self._check(self.lib.vpl_ba_enable_kernel_timing(self.h, 1 if on else 0), "vpl_ba_enable_kernel_timing")

    def kernel_times(self):
        cnt = C.c_int(64)
        names = (C.c_char_p * 64)()
        ms = (C.c_double * 64)()
        launches = (C.c_int * 64)()
        self._check(self.lib.vpl_ba_kernel_times(self.h, C.byref(cnt), names, ms, launches), "vpl_ba_kernel_times")
        return {names[i].decode(): (ms[i], launches[i]) for i in range(cnt.value)}

    def launch_profile(self):
        """Launches of the last timed solve, in order: (kernel, ms, (linearised, new step, re-used step, evaluated))."""
        cnt = C.c_int(64)
        names = (C.c_char_p * 64)()
        ms = (C.c_double * 64)()
        act = (C.c_int * 256)()
        self._check(self.lib.vpl_ba_launch_profile(self.h, C.byref(cnt), names, ms, act), "vpl_ba_launch_profile")
        return [(names[i].decode(), ms[i], tuple(act[4 * i + k] for k in range(4))) for i in range(cnt.value)]


class Frame:
    """One image of one sequence for Session: the propagated state, the pre-integration of the interval that ends in it and
    its observations -- point_obs [n][3] (x, y, 1) and line_obs [n][8] (as Window.line_obs) with their feature ids."""

    def __init__(self, point_id=(), point_obs=(), line_id=(), line_obs=(), pose=None, speed_bias=None, preint=None):
        self.point_id = _arr(point_id, np.int32).reshape(-1)
        self.point_obs = _arr(point_obs, np.float64).reshape(-1, 3)
        self.line_id = _arr(line_id, np.int32).reshape(-1)
        self.line_obs = _arr(line_obs, np.float64).reshape(-1, 8)
        assert len(self.point_id) == len(self.point_obs) and len(self.line_id) == len(self.line_obs)
        self.pose = None if pose is None else _arr(pose, np.float64).reshape(7)
        self.speed_bias = None if speed_bias is None else _arr(speed_bias, np.float64).reshape(9)
        self.preint = preint

    def to_c(self, cf):
        if self.pose is not None:
            C.memmove(cf.pose, self.pose.ctypes.data, 56)
        if self.speed_bias is not None:
            C.memmove(cf.speed_bias, self.speed_bias.ctypes.data, 72)
        if self.preint is not None:
            C.memmove(C.byref(cf.preint), C.byref(self.preint), C.sizeof(Preintegration))
        cf.n_points, cf.n_lines = len(self.point_id), len(self.line_id)
        cf.point_id, cf.point_obs = self.point_id.ctypes.data_as(_ip), self.point_obs.ctypes.data_as(_dp)
        cf.line_id, cf.line_obs = self.line_id.ctypes.data_as(_ip), self.line_obs.ctypes.data_as(_dp)


class ImuFrame:
    """One image of one sequence for an IMU-enabled Session: its observations as in Frame, and samples [n][7] = (dt, ax, ay, az,
    gx, gy, gz) of the interval that ends in it -- the session integrates and propagates them on the device."""

    def __init__(self, samples, point_id=(), point_obs=(), line_id=(), line_obs=()):
        self.samples = _arr(samples, np.float64).reshape(-1, 7)
        self.point_id = _arr(point_id, np.int32).reshape(-1)
        self.point_obs = _arr(point_obs, np.float64).reshape(-1, 3)
        self.line_id = _arr(line_id, np.int32).reshape(-1)
        self.line_obs = _arr(line_obs, np.float64).reshape(-1, 8)
        assert len(self.point_id) == len(self.point_obs) and len(self.line_id) == len(self.line_obs)

    def to_c(self, cf):
        cf.n_samples, cf.samples = len(self.samples), self.samples.ctypes.data_as(_dp)
        cf.n_points, cf.n_lines = len(self.point_id), len(self.line_id)
        cf.point_id, cf.point_obs = self.point_id.ctypes.data_as(_ip), self.point_obs.ctypes.data_as(_dp)
        cf.line_id, cf.line_obs = self.line_id.ctypes.data_as(_ip), self.line_obs.ctypes.data_as(_dp)


class Session:
    """vpl_odo: the feature manager and the window of n_seq sequences resident on the device, fed one keyframe at a time
    (include/vplines_ba.h, "keyframe session").  Borrows `ctx` (one session per context) or makes a context of its own from
    ctx_args -- which fails loudly without a GPU, like Context."""

    def __init__(self, ctx=None, n_seq=1, opt=None, init_depth=5.0, line_min_obs=5, max_point_tracks=1024, max_line_tracks=512,
                 **ctx_args):
        self.own_ctx = ctx is None
        if ctx is None:
            ctx_args.setdefault("max_windows", n_seq)
            ctx = Context(**ctx_args)
        self.ctx, self.lib, self.n_seq = ctx, ctx.lib, n_seq
        self.max_point_tracks, self.max_line_tracks = max_point_tracks, max_line_tracks
        opt = opt if opt is not None else default_options()
        self.h = C.c_void_p()
        ctx._settle()
        rc = self.lib.vpl_odo_create(C.byref(self.h), ctx.h, n_seq, C.byref(opt), init_depth, line_min_obs, max_point_tracks,
                                     max_line_tracks)
        if rc != 0:
            msg = self.lib.vpl_last_error(ctx.h)
            raise RuntimeError("vpl_odo_create failed (%d): %s" % (rc, msg.decode() if msg else ""))
        ctx._odo = self        # Context.close() destroys a session that is still open first, whoever is closed or collected first

    def _destroy(self):
        if self.h:
            self.lib.vpl_odo_destroy(self.h)
            self.h = C.c_void_p()
            if getattr(self.ctx, "_odo", None) is self:
                self.ctx._odo = None

    def close(self):
        self._destroy()
        if self.own_ctx and self.ctx is not None:
            ctx, self.ctx = self.ctx, None
            ctx.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_window(self, seq, pose, speed_bias, ex_pose, preint, frames):
        """frames 0..10 of sequence seq: states [11][7] / [11][9], extrinsic, (Preintegration * 11) (entry 0 unused) and 11
        Frames (observations only)"""
        pose, sb, ex = _arr(pose, np.float64).reshape(NF, 7), _arr(speed_bias, np.float64).reshape(NF, 9), _arr(ex_pose, np.float64).reshape(7)
        assert len(frames) == NF
        cf = (OdoFrame * NF)()
        for i, f in enumerate(frames):
            f.to_c(cf[i])
        self.ctx._settle()
        self.ctx._check(self.lib.vpl_odo_set_window(self.h, seq, _p(pose), _p(sb), _p(ex), preint, cf), "vpl_odo_set_window")

    def init(self, inputs, ex_pose, frames, check=True):
        """vpl_odo_init: the session takes its first window from the visual-inertial alignment.  inputs: one InitInput per sequence;
        ex_pose [n_seq][7]; frames: per sequence its 11 Frames (observations only).  -> one InitResult per sequence; a sequence whose
        result is not ok holds no window afterwards.  check=False: a refusal comes back as its VPL_E_* code."""
        n = self.n_seq
        assert len(inputs) == n and len(frames) == n and all(len(f) == NF for f in frames)
        ci = (CInitInput * n)()
        for i, q in enumerate(inputs):
            if isinstance(q, CInitInput):
                C.memmove(C.byref(ci[i]), C.byref(q), C.sizeof(CInitInput))
            else:
                q.to_c(ci[i])
        ex = _arr(ex_pose, np.float64).reshape(n, 7)
        cf = (OdoFrame * (n * NF))()
        for i, fs in enumerate(frames):
            for j, f in enumerate(fs):
                f.to_c(cf[i * NF + j])
        res = (InitResult * n)()
        self.ctx._settle()
        t0 = time.perf_counter()
        rc = self.lib.vpl_odo_init(self.h, ci, _p(ex), cf, res)
        self.last_call_s = time.perf_counter() - t0
        self.last_rc = rc
        if rc != 0 and not check:
            return rc
        self.ctx._check(rc, "vpl_odo_init")
        return res

    def keyframe(self, frames, flags=None):
        """vpl_odo_keyframe: solveOdometry -> removeFailures -> slideWindow(flag) -> the Frames enter slot 10; one
        OdoResult per sequence (states BEFORE the slide)"""
        assert len(frames) == self.n_seq
        cf = (OdoFrame * self.n_seq)()
        for i, f in enumerate(frames):
            f.to_c(cf[i])
        fl = _arr([MARGIN_OLD] * self.n_seq if flags is None else flags, np.int32)
        assert len(fl) == self.n_seq
        res = (OdoResult * self.n_seq)()
        self.ctx._settle()
        t0 = time.perf_counter()
        rc = self.lib.vpl_odo_keyframe(self.h, cf, fl.ctypes.data_as(_ip), res)
        self.last_call_s = time.perf_counter() - t0      # the C call alone (tools/time_session.py)
        self.last_rc = rc
        self.ctx._check(rc, "vpl_odo_keyframe")
        return res

    def solve(self, flags=None):
        """vpl_odo_solve: the first half of keyframe (solveOdometry); the Frames of advance may be built from its results"""
        fl = _arr([MARGIN_OLD] * self.n_seq if flags is None else flags, np.int32)
        assert len(fl) == self.n_seq
        self._res = (OdoResult * self.n_seq)()
        self.ctx._settle()
        t0 = time.perf_counter()
        rc = self.lib.vpl_odo_solve(self.h, fl.ctypes.data_as(_ip), self._res)
        self.last_call_s = time.perf_counter() - t0
        self.last_rc = rc
        self.ctx._check(rc, "vpl_odo_solve")
        return self._res

    def advance(self, frames):
        """vpl_odo_advance: removeFailures -> slideWindow -> the Frames enter slot 10; updates the counts of solve's results"""
        assert len(frames) == self.n_seq
        cf = (OdoFrame * self.n_seq)()
        for i, f in enumerate(frames):
            f.to_c(cf[i])
        self.ctx._settle()
        t0 = time.perf_counter()
        rc = self.lib.vpl_odo_advance(self.h, cf, getattr(self, "_res", None))
        self.last_call_s = time.perf_counter() - t0
        self.last_rc = rc
        self.ctx._check(rc, "vpl_odo_advance")
        return self._res

    # ---- IMU samples in (vpl_odo_enable_imu): pre-integration, merge and propagation on the device ----
    def enable_imu(self, max_samples):
        """vpl_odo_enable_imu: from now on the session takes ImuFrames (keyframe_imu / advance_imu); once per session"""
        self.ctx._settle()
        rc = self.lib.vpl_odo_enable_imu(self.h, int(max_samples))
        self.last_rc = rc
        self.ctx._check(rc, "vpl_odo_enable_imu")

    def set_imu(self, seq, samples10, acc0_10, gyr0_10):
        """vpl_odo_set_imu, after set_window: the samples [n][7] of the interval that ends in frame 10 and linearized_acc / _gyr
        of its pre-integration (the last measurement before that interval)"""
        smp = _arr(samples10, np.float64).reshape(-1, 7)
        a0, g0 = _arr(acc0_10, np.float64).reshape(3), _arr(gyr0_10, np.float64).reshape(3)
        self.ctx._settle()
        rc = self.lib.vpl_odo_set_imu(self.h, seq, len(smp), _p(smp), _p(a0), _p(g0))
        self.last_rc = rc
        self.ctx._check(rc, "vpl_odo_set_imu")

    def _imu_frames(self, frames):
        assert len(frames) == self.n_seq
        cf = (OdoImuFrame * self.n_seq)()
        for i, f in enumerate(frames):
            f.to_c(cf[i])
        return cf

    def keyframe_imu(self, frames, flags=None):
        """vpl_odo_keyframe_imu: keyframe() with ImuFrames; (one OdoResult per sequence, one OdoImuOut per sequence)"""
        cf = self._imu_frames(frames)
        fl = _arr([MARGIN_OLD] * self.n_seq if flags is None else flags, np.int32)
        assert len(fl) == self.n_seq
        res, imu = (OdoResult * self.n_seq)(), (OdoImuOut * self.n_seq)()
        self.ctx._settle()
        t0 = time.perf_counter()
        rc = self.lib.vpl_odo_keyframe_imu(self.h, cf, fl.ctypes.data_as(_ip), res, imu)
        self.last_call_s = time.perf_counter() - t0
        self.last_rc = rc
        self.ctx._check(rc, "vpl_odo_keyframe_imu")
        return res, imu

    def advance_imu(self, frames):
        """vpl_odo_advance_imu, after solve(): (solve's results with the counts updated, one OdoImuOut per sequence)"""
        cf = self._imu_frames(frames)
        imu = (OdoImuOut * self.n_seq)()
        self.ctx._settle()
        t0 = time.perf_counter()
        rc = self.lib.vpl_odo_advance_imu(self.h, cf, getattr(self, "_res", None), imu)
        self.last_call_s = time.perf_counter() - t0
        self.last_rc = rc
        self.ctx._check(rc, "vpl_odo_advance_imu")
        return self._res, imu

    # ---- the keyframe decision and the failure check (vpl_odo_enable_keyframe_rule) ----
    def enable_keyframe_rule(self, min_parallax=None, min_track_num=None):
        """vpl_odo_enable_keyframe_rule: from now on the device decides, image by image, which way the next solve marginalises
        (decision / the _auto calls); None = the reference's default.  A second call replaces the thresholds."""
        r = default_keyframe_rule()
        if min_parallax is not None:
            r.min_parallax = float(min_parallax)
        if min_track_num is not None:
            r.min_track_num = int(min_track_num)
        self.ctx._settle()
        rc = self.lib.vpl_odo_enable_keyframe_rule(self.h, C.byref(r))
        self.last_rc = rc
        self.ctx._check(rc, "vpl_odo_enable_keyframe_rule")

    def decision(self, seq=0):
        """vpl_odo_get_decision: OdoDecision of the window as it stands (and the failure mask of the last solve)"""
        d = OdoDecision()
        rc = self.lib.vpl_odo_get_decision(self.h, seq, C.byref(d))
        self.last_rc = rc
        self.ctx._check(rc, "vpl_odo_get_decision")
        return d

    def solve_auto(self):
        """vpl_odo_solve_auto: solve() with the stored decisions as flags (refused when the sequences disagree)"""
        self._res = (OdoResult * self.n_seq)()
        self.ctx._settle()
        t0 = time.perf_counter()
        rc = self.lib.vpl_odo_solve_auto(self.h, self._res)
        self.last_call_s = time.perf_counter() - t0
        self.last_rc = rc
        self.ctx._check(rc, "vpl_odo_solve_auto")
        return self._res

    def keyframe_auto(self, frames):
        """vpl_odo_keyframe_auto: keyframe() with the stored decisions as flags"""
        assert len(frames) == self.n_seq
        cf = (OdoFrame * self.n_seq)()
        for i, f in enumerate(frames):
            f.to_c(cf[i])
        res = (OdoResult * self.n_seq)()
        self.ctx._settle()
        t0 = time.perf_counter()
        rc = self.lib.vpl_odo_keyframe_auto(self.h, cf, res)
        self.last_call_s = time.perf_counter() - t0
        self.last_rc = rc
        self.ctx._check(rc, "vpl_odo_keyframe_auto")
        return res

    def keyframe_imu_auto(self, frames):
        """vpl_odo_keyframe_imu_auto: keyframe_imu() with the stored decisions as flags"""
        cf = self._imu_frames(frames)
        res, imu = (OdoResult * self.n_seq)(), (OdoImuOut * self.n_seq)()
        self.ctx._settle()
        t0 = time.perf_counter()
        rc = self.lib.vpl_odo_keyframe_imu_auto(self.h, cf, res, imu)
        self.last_call_s = time.perf_counter() - t0
        self.last_rc = rc
        self.ctx._check(rc, "vpl_odo_keyframe_imu_auto")
        return res, imu

    def get_preint(self, seq=0):
        """vpl_odo_get_preint: (Preintegration * 11) as the session holds them (entry 0 zero; jacobian columns 0..8 zero)"""
        out = (Preintegration * NF)()
        self.ctx._check(self.lib.vpl_odo_get_preint(self.h, seq, out), "vpl_odo_get_preint")
        return out

    def get_states(self, seq=0):
        """vpl_odo_get_states: (pose [11, 7], speed_bias [11, 9], ex_pose [7]) as the store holds them"""
        pose, sb, ex = np.zeros((NF, 7)), np.zeros((NF, 9)), np.zeros(7)
        self.ctx._check(self.lib.vpl_odo_get_states(self.h, seq, _p(pose), _p(sb), _p(ex)), "vpl_odo_get_states")
        return pose, sb, ex

    def get_prior(self, seq=0):
        p = Prior()
        self.ctx._check(self.lib.vpl_odo_get_prior(self.h, seq, C.byref(p)), "vpl_odo_get_prior")
        return p

    def get_tracks(self, seq=0):
        """dict: point_id / point_start / point_nobs / inv_depth, line_id / line_start / line_nobs / line_triangulated / line_plk,
        in the feature manager's order"""
        mp, ml = self.max_point_tracks, self.max_line_tracks
        n = (C.c_int * 2)()
        pi, ps, pn = (np.zeros(mp, np.int32) for _ in range(3))
        li, ls, ln, lt = (np.zeros(ml, np.int32) for _ in range(4))
        invd, plk = np.zeros(mp), np.zeros((ml, 6))
        ip = lambda a: a.ctypes.data_as(_ip)
        rc = self.lib.vpl_odo_get_tracks(self.h, seq, C.cast(C.byref(n, 0), _ip), ip(pi), ip(ps), ip(pn), _p(invd),
                                         C.cast(C.byref(n, 4), _ip), ip(li), ip(ls), ip(ln), ip(lt), _p(plk))
        self.ctx._check(rc, "vpl_odo_get_tracks")
        a, b = n[0], n[1]
        return dict(point_id=pi[:a], point_start=ps[:a], point_nobs=pn[:a], inv_depth=invd[:a], line_id=li[:b],
                    line_start=ls[:b], line_nobs=ln[:b], line_triangulated=lt[:b], line_plk=plk[:b])

    def select(self, params, frames, check=True):
        """vpl_odo_select: FeatureSelector::select for the next image of every sequence (one SelectFrame each) -- state k, the
        cloud and the id book are the session's.  Not between solve and advance.  -> list [n_seq] of dict ids (selection order),
        f, out (the ids to hand to advance / keyframe, ascending), initialized, n_new, n_used, kappa, n_cloud, n_invisible,
        n_ineligible, n_candidates.  check=False: a refusal comes back as its VPL_E_* code."""
        n = self.n_seq
        assert len(frames) == n
        par = params if isinstance(params, SelectParams) else SelectParams.of(params)
        cf = (CSelectFrame * n)()
        for i, f in enumerate(frames):
            f.to_c(cf[i])
        res = (OdoSelectResult * n)()
        ids, out = np.zeros((n, SEL_MAX_FEATURES), dtype=np.int32), np.zeros((n, SEL_MAX_FEATURES), dtype=np.int32)
        fs = np.zeros((n, SEL_MAX_FEATURES))
        self.ctx._settle()
        rc = self.lib.vpl_odo_select(self.h, C.byref(par), cf, res, ids.ctypes.data_as(_ip), _p(fs), out.ctypes.data_as(_ip))
        if rc != 0 and not check:
            return rc
        self.ctx._check(rc, "vpl_odo_select")
        return [dict(ids=ids[i, :res[i].sel.n_selected].copy(), f=fs[i, :res[i].sel.n_selected].copy(), out=out[i, :res[i].n_out].copy(),
                     initialized=bool(res[i].initialized), n_new=res[i].n_new, n_used=res[i].n_used, kappa=res[i].kappa,
                     n_cloud=res[i].n_cloud, n_invisible=res[i].sel.n_invisible, n_ineligible=res[i].sel.n_ineligible,
                     n_candidates=res[i].sel.n_candidates) for i in range(n)]

    def stats(self):
        """(h2d_payload_bytes, h2d_table_bytes, d2h_bytes) of the last keyframe"""
        a, b, c = C.c_longlong(), C.c_longlong(), C.c_longlong()
        self.ctx._check(self.lib.vpl_odo_stats(self.h, C.byref(a), C.byref(b), C.byref(c)), "vpl_odo_stats")
        return a.value, b.value, c.value

    def stage_ms(self):
        """wall clock of the last keyframe's stages: triangulations | onlyLineOpt | solve | slide + new frame"""
        ms = np.zeros(4)
        self.ctx._check(self.lib.vpl_odo_debug_ms(self.h, _p(ms)), "vpl_odo_debug_ms")
        return ms


def odo_debug_tracks(max_tracks, flags, frames_ids, erase):
    """vpl_odo_debug_tracks (host only): flags [n_steps], frames_ids: list of id lists, erase [n_steps][max_tracks] uint8.
    Returns rc, status, n_slide, slide [n][max][3], n_tracks, table [n][max][3], ignored"""
    lib = load_hip_library()
    n = len(flags)
    fl = _arr(flags, np.int32)
    n_ids = _arr([len(f) for f in frames_ids], np.int32)
    ids = _arr([i for f in frames_ids for i in f] + [0], np.int32)
    er = _arr(erase, np.uint8).reshape(n, max_tracks)
    status, n_slide, n_tracks, ignored = (np.zeros(max(n, 1), np.int32) for _ in range(4))
    slide, table = (np.full((max(n, 1), max_tracks, 3), -7, np.int32) for _ in range(2))
    ip = lambda a: a.ctypes.data_as(_ip)
    rc = lib.vpl_odo_debug_tracks(max_tracks, n, ip(fl), ip(n_ids), ip(ids), er.ctypes.data_as(C.POINTER(C.c_ubyte)), ip(status),
                                  ip(n_slide), ip(slide), ip(n_tracks), ip(table), ip(ignored))
    return rc, status[:n], n_slide[:n], slide[:n], n_tracks[:n], table[:n], ignored[:n]


def default_keyframe_rule():
    r = OdoKeyframeRule()
    load_hip_library().vpl_odo_default_keyframe_rule(C.byref(r))
    return r


def default_failure_limits():
    l = FailureLimits()
    load_hip_library().vpl_failure_default_limits(C.byref(l))
    return l


def failure_detection(speed_bias10, pose10, last_pose, limits=None):
    """vpl_failure_detection (host only): the FAIL_* mask of Estimator::failureDetection; limits None = the defaults"""
    sb, p, q = _arr(speed_bias10, np.float64).reshape(9), _arr(pose10, np.float64).reshape(7), _arr(last_pose, np.float64).reshape(7)
    return load_hip_library().vpl_failure_detection(None if limits is None else C.byref(limits), _p(sb), _p(p), _p(q))


def odo_debug_parallax_list(max_tracks, flags, frames_ids, erase):
    """vpl_odo_debug_parallax_list (host only), arguments as odo_debug_tracks.  Returns rc, n_list [n_steps] (-1: no decision at
    that step), list [n_steps][max_tracks], last_track_num [n_steps]"""
    lib = load_hip_library()
    n = len(flags)
    fl = _arr(flags, np.int32)
    n_ids = _arr([len(f) for f in frames_ids], np.int32)
    ids = _arr([i for f in frames_ids for i in f] + [0], np.int32)
    er = _arr(erase, np.uint8).reshape(n, max_tracks)
    n_list, last = (np.zeros(max(n, 1), np.int32) for _ in range(2))
    lst = np.full((max(n, 1), max_tracks), -7, np.int32)
    ip = lambda a: a.ctypes.data_as(_ip)
    rc = lib.vpl_odo_debug_parallax_list(max_tracks, n, ip(fl), ip(n_ids), ip(ids), er.ctypes.data_as(C.POINTER(C.c_ubyte)), ip(n_list),
                                         ip(lst), ip(last))
    return rc, n_list[:n], lst[:n], last[:n]
