/*
 * vplines_ba.h -- C ABI of the MI355X-native sliding-window bundle-adjustment path.
 *
 * This header is the drop-in boundary for the back-end hot path of
 * multiplefish/VPLines-SLAM (vins_estimator).  Every entry point names the
 * reference interface it replaces (path:line relative to the reference tree).
 * All signatures use plain pointers and sizes; no C++/torch types cross it.
 *
 * Conventions shared with the reference
 *   - parameter blocks keep the reference's global layouts
 *       pose        [7] = px,py,pz,qx,qy,qz,qw      (estimator.cpp:650-705)
 *       speed/bias  [9] = v, ba, bg
 *       inv. depth  [1]                             (feature_manager.cpp:277-293)
 *       line orth   [4] = psi1,psi2,psi3,phi        (line_geometry.cpp:62-126)
 *   - Jacobians are row-major  num_residuals x global_size, column 6 of every
 *     7-sized pose block is written as zero (projection_factor.cpp:81-88)
 *   - WINDOW_SIZE = 10  => 11 frames  (parameters.h:20)
 *
 * Error handling: every function returns 0 on success and a negative
 * VPL_E_* code otherwise; nothing aborts, nothing falls back to a CPU path.
 * Thread model: one vpl_ctx per host thread / GPU; functions on one context
 * are not re-entrant (the reference calls its solve from exactly one thread,
 * estimator_node.cpp:229).
 */
#ifndef VPLINES_BA_H
#define VPLINES_BA_H

#ifdef __cplusplus
extern "C" {
#endif

#define VPL_WINDOW_SIZE 10
#define VPL_NFRAMES 11
#define VPL_MAX_PRIOR_BLOCKS 23 /* 11 poses + 11 speed/bias + 1 extrinsic */
#define VPL_MAX_PRIOR_DIM 171   /* 11*6 + 11*9 + 6 */

#define VPL_OK 0
#define VPL_E_INVALID -1   /* bad argument / shape mismatch */
#define VPL_E_NODEVICE -2  /* no HIP device or kernel image for it */
#define VPL_E_HIP -3       /* a HIP runtime call failed */
#define VPL_E_CAPACITY -4  /* batch exceeds the capacity given at create */
#define VPL_E_NUMERIC -5   /* non-finite value met where the reference would ROS_BREAK */

/* marginalization_flag of Estimator (estimator.h MarginalizationFlag) */
#define VPL_MARGIN_OLD 0
#define VPL_MARGIN_SECOND_NEW 1
#define VPL_MARGIN_NONE -1

/* kind of a kept parameter block inside a prior */
#define VPL_BLOCK_POSE 0
#define VPL_BLOCK_SPEEDBIAS 1
#define VPL_BLOCK_EXPOSE 2

/* Solver / model constants the reference reads from YAML and parameters.h
 * (parameters.cpp:58-154, estimator.cpp:18-20). */
typedef struct vpl_ba_options {
  int num_iterations;       /* NUM_ITERATIONS -> options.max_num_iterations (estimator.cpp:1211) */
  int estimate_extrinsic;   /* ESTIMATE_EXTRINSIC; 0 => para_Ex_Pose constant (estimator.cpp:1060) */
  int marginalization_flag; /* VPL_MARGIN_* */
  int remove_line_outliers; /* run FeatureManager::removeLineOutlier between solve and marginalisation (0/1) */
  double focal_length;      /* FOCAL_LENGTH; ProjectionFactor::sqrt_info = f/1.5 * I */
  double line_factor;       /* lineProjectionFactor::sqrt_info = line_factor * I */
  double vp_factor;         /* vpProjectionFactor::sqrt_info = vp_factor * I */
  double g_norm;            /* G = (0,0,g_norm) */
  double acc_n, gyr_n, acc_w, gyr_w; /* IMU noise densities (integration_base.h:21-27) */
  double huber_delta;       /* ceres::HuberLoss(1.0) (estimator.cpp:1048) */
} vpl_ba_options;

/* Fills the EuRoC values (config/euroc/euroc_config.yaml:55-63,84-91) with
 * num_iterations = 5 (the BASELINE metric), estimate_extrinsic = 1. */
void vpl_ba_default_options(vpl_ba_options* opt);

/* Result of IntegrationBase (integration_base.h:9-249) for one keyframe interval. */
typedef struct vpl_preintegration {
  double sum_dt;
  double delta_p[3];
  double delta_q[4];          /* x,y,z,w */
  double delta_v[3];
  double linearized_ba[3];
  double linearized_bg[3];
  double jacobian[15 * 15];   /* row-major, state order P,R,V,BA,BG (parameters.h:82-89) */
  double covariance[15 * 15]; /* row-major */
} vpl_preintegration;

/* The linearised prior left by MarginalizationInfo (marginalization_factor.h:46-72):
 * keep_block_{size,idx,data}, linearized_jacobians, linearized_residuals.
 * Blocks are identified by (kind, frame) instead of by address; the order of
 * blocks is deterministic (see DESIGN.md "prior ordering"). */
typedef struct vpl_prior {
  int n;                                   /* number of residuals = kept local dims */
  int n_blocks;
  int block_kind[VPL_MAX_PRIOR_BLOCKS];    /* VPL_BLOCK_* */
  int block_frame[VPL_MAX_PRIOR_BLOCKS];   /* frame index in the window that will USE the prior */
  int block_idx[VPL_MAX_PRIOR_BLOCKS];     /* keep_block_idx - m : first local column */
  double x0[VPL_MAX_PRIOR_BLOCKS][9];      /* keep_block_data (global size 7 or 9) */
  double J0[VPL_MAX_PRIOR_DIM * VPL_MAX_PRIOR_DIM]; /* linearized_jacobians, row-major n x n */
  double r0[VPL_MAX_PRIOR_DIM];            /* linearized_residuals */
} vpl_prior;

/* One sliding window exactly as Estimator::optimizationwithLine() sees it
 * (estimator.cpp:1043-1453): para_* arrays after vector2double(), the feature
 * tracks of FeatureManager that pass the reference's filters, pre-integrations
 * and the last prior.  All arrays are caller-owned host memory. */
typedef struct vpl_window {
  double pose[VPL_NFRAMES][7];       /* para_Pose        (in: initial, out: after double2vector2) */
  double speed_bias[VPL_NFRAMES][9]; /* para_SpeedBias   (in/out) */
  double ex_pose[7];                 /* para_Ex_Pose[0]  (in/out) */

  /* point tracks: FeaturePerId with used_num>=2 && start_frame<WINDOW_SIZE-2
   * (estimator.cpp:1100-1102), in f_manager.feature order */
  int n_points;
  const int* point_start;   /* [n_points] start_frame */
  const int* point_nobs;    /* [n_points] feature_per_frame.size(), consecutive frames from start */
  const double* point_obs;  /* [sum nobs][3]  FeaturePerFrame::point (x,y,1) */
  double* inv_depth;        /* [n_points] para_Feature (in/out) = 1/estimated_depth */

  /* line tracks: used_num>=LINE_MIN_OBS && start_frame<WINDOW_SIZE-2 && is_triangulation
   * (estimator.cpp:1132-1133) */
  int n_lines;
  const int* line_start;    /* [n_lines] */
  const int* line_nobs;     /* [n_lines] */
  const double* line_obs;   /* [sum nobs][8] x1,y1,x2,y2, vp_x,vp_y,vp_z, vp_flag (estimator_node.cpp:375-407) */
  double* line_plk;         /* [n_lines][6] lineFeaturePerId::line_plucker, start-CAMERA frame (in/out) */
  int* line_removed;        /* [n_lines] out, may be NULL: 1 = erased by removeLineOutlier (options.remove_line_outliers) */
  int* line_triangulated;   /* [n_lines] lineFeaturePerId::is_triangulation; NULL = every line is triangulated.  Lines with 0
                             * take no part in the solves (estimator.cpp:1133); vpl_ba_triangulate_lines sets it (in/out) */

  /* pre_integrations[1..10]; entry 0 unused (estimator.cpp:1085-1093) */
  vpl_preintegration preint[VPL_NFRAMES];

  int has_prior;            /* last_marginalization_info != nullptr */
  const vpl_prior* prior;   /* used when has_prior */

  /* Estimator::failure_occur (estimator.cpp:818-823): after a detected failure the gauge fix of double2vector2 restores the
   * yaw / position of last_R0 / last_P0 (the first frame of the last good window) instead of those of the first frame
   * before this solve.  0 = normal operation; last_R0 is row-major 3x3. */
  int failure_occur;
  double last_P0[3];
  double last_R0[9];

  /* Optional: para_LineFeature as the caller holds it -- [n_lines][4] WORLD-frame orthonormal (psi1,psi2,psi3,phi),
   * the block lineProjectionFactor / vpProjectionFactor::Evaluate take (feature_manager.cpp:341-365).  NULL (the normal
   * case): it is derived from line_plk and the start pose, as vector2double does.  Non-NULL: used as is (vpl_ba_marginalize
   * driven factor by factor, host/vpl_factors.hpp MarginalizationInfo); line_plk is then not read. */
  const double* line_orth;
} vpl_window;

/* Per-window solve report (mirrors the fields of ceres::Solver::Summary the
 * reference could log, plus what the marginalisation produced). */
typedef struct vpl_solve_report {
  int iterations;           /* trust-region iterations performed (successful + unsuccessful) */
  int num_successful_steps;
  int termination;          /* 0 no_convergence(max iters), 1 convergence, 2 failure */
  double initial_cost;
  double final_cost;
  int n_lines_removed;      /* by removeLineOutlier */
  int prior_m, prior_n;     /* MarginalizationInfo::m, n */
} vpl_solve_report;

typedef struct vpl_ctx vpl_ctx; /* opaque: device buffers + stream for one GPU */

/* ---- context ------------------------------------------------------------ */
/* Creates a context on HIP device `device` sized for up to `max_windows`
 * windows of up to `max_points` point tracks, `max_point_obs` point
 * observations, `max_lines` / `max_line_obs` likewise per window. */
int vpl_ctx_create(vpl_ctx** out, int device, int max_windows, int max_points, int max_point_obs,
                   int max_lines, int max_line_obs);
void vpl_ctx_destroy(vpl_ctx* ctx);
/* Launch all work of this context on `hip_stream` (a hipStream_t; NULL = default stream).  Work in flight on the stream used
 * so far is completed first (an enqueued call is collected, the old stream synchronised). */
int vpl_ctx_set_stream(vpl_ctx* ctx, void* hip_stream);
const char* vpl_last_error(const vpl_ctx* ctx);

/* ---- IMU pre-integration  (replaces IntegrationBase::push_back/propagate/
 *      midPointIntegration, integration_base.h:30-36,54-198) --------------- */
/* n intervals; interval k has nsamples[k] samples stored at samples + 7*offset[k]
 * as (dt, ax,ay,az, gx,gy,gz); acc0/gyr0/ba/bg are [n][3]. Host in, host out.
 * nsamples[k] == 0 is an empty interval: the identity, a zero covariance, sum_dt 0, and no row of `samples` is read for it.
 * A negative offset[k] or nsamples[k] is VPL_E_INVALID. */
int vpl_preintegrate_batch(vpl_ctx* ctx, int n, const int* offset, const int* nsamples,
                           const double* samples, const double* acc0, const double* gyr0,
                           const double* lin_ba, const double* lin_bg, const vpl_ba_options* opt,
                           vpl_preintegration* out);

/* ---- visual-inertial alignment  (replaces Estimator::visualInitialAlign, estimator.cpp:512-588, with VisualIMUAlignment =
 *      solveGyroscopeBias + LinearAlignment + RefineGravity, initial/initial_aligment.cpp:3-207, and Utility::g2R,
 *      utility.cpp:3-13) for n sequences in one call ------------------------------------------------------------------------ *
 * The vision-only structure before it is vpl_init_structure_batch below (GlobalSFM::construct, the PnP of the non-key frames;
 * relativePose is vpl_init_relative_pose_batch behind it), whose result has the form taken here: ImageFrame::R and ImageFrame::T of every image
 * frame; with them the raw IMU samples between the frames.  On the device, per sequence:
 *   1. the F - 1 image intervals are pre-integrated under (lin_ba, lin_bg), the arithmetic of vpl_preintegrate_batch;
 *   2. solveGyroscopeBias: delta_bg from the 3 x 3 normal equations, summed in frame order; Bgs[i] += delta_bg for the 11 frames;
 *   3. the image intervals are integrated again under (0, Bgs[0]), the ten window intervals -- window interval i spans the image
 *      intervals key[i-1]+1 .. key[i] -- under (0, Bgs[i]): zero accelerometer bias, whatever bas holds, as the reference has it;
 *   4. LinearAlignment (order 3F + 4), four rounds of RefineGravity (order 3F + 3), the state change and the rotation into the
 *      gravity frame (k_init_align, one work-group per sequence).
 * Kept as the reference has them: cov_inv is the identity; the scale column is divided by 100 and every system multiplied by
 * 1000 before it is solved; RefineGravity zeroes A and b ONCE, before its four rounds, so round k solves what the rounds before
 * left (times 1000) plus its own blocks; Vs[kv] = R[key[kv]] * x[3 kv .. 3 kv + 2] with kv counting KEY frames, which is another
 * frame's velocity as soon as a non-key frame lies before it.  The solves are unpivoted LDL^T in float64.
 * A sequence's result has the same bits wherever it sits in the batch and whatever else the batch holds. */
#define VPL_INIT_MAX_FRAMES 40
#define VPL_INIT_FAIL_GRAVITY 1        /* | |g| - g_norm | > 1.0 after LinearAlignment          (initial_aligment.cpp:184) */
#define VPL_INIT_FAIL_SCALE 2          /* s < 0 after LinearAlignment                            (:184) */
#define VPL_INIT_FAIL_REFINED_SCALE 4  /* s < 0 after RefineGravity                              (:193) */
#define VPL_INIT_FAIL_NONFINITE 8      /* a NaN / inf in the solution or in the states it gives */
typedef struct vpl_init_input {
  int n_frames;            /* F = all_image_frame.size(), 11 <= F <= VPL_INIT_MAX_FRAMES */
  const double* R;         /* [F][9] row-major ImageFrame::R = Q_i * RIC^T */
  const double* T;         /* [F][3] ImageFrame::T, the camera position in the SfM frame */
  const int* n_samples;    /* [F] samples of the interval that ENDS in image frame f; entry 0 unused */
  const double* samples;   /* [sum][7] dt, ax, ay, az, gx, gy, gz of intervals 1 .. F-1 one after the other */
  double acc0[3], gyr0[3]; /* the measurement before interval 1; a later interval starts from the last sample of the one before
                              (the convention of vpl_odo_set_imu) */
  const double* lin_ba;    /* [F][3] the bias under which image frame f's pre-integration stands; entry 0 unused */
  const double* lin_bg;    /* [F][3] */
  int key[VPL_NFRAMES];    /* image-frame index of window frame i: strictly increasing, key[0] == 0, key[10] == F - 1 */
  double bas[VPL_NFRAMES][3], bgs[VPL_NFRAMES][3]; /* Bas / Bgs of the window before the alignment */
  double tic[3];           /* TIC[0] */
} vpl_init_input;
typedef struct vpl_init_result {
  int ok;                  /* 1: VisualIMUAlignment returned true and every result is finite */
  int fail;                /* VPL_INIT_FAIL_* mask, 0 when ok */
  double delta_bg[3];      /* applied by the reference before it knows whether the alignment fails: valid either way */
  double g_linear[3];      /* LinearAlignment's gravity (x.segment<3>(n_state - 4)) and scale */
  double s_linear;
  double s;                /* the scale after RefineGravity (x.tail(1) / 100) */
  double g_refined[3];     /* gravity after RefineGravity, SfM frame */
  double g[3];             /* ... after the rotation: R0 * g_refined */
  double vel[VPL_INIT_MAX_FRAMES][3]; /* x.segment<3>(3 f) of the last solve: image frame f's velocity in its own body frame */
  double pose[VPL_NFRAMES][7];        /* Ps / Rs after the state change, the window's parameter-block layout */
  double speed_bias[VPL_NFRAMES][9];  /* Vs, the input Bas, Bgs + delta_bg */
} vpl_init_result;
/* in [n], out [n].  window_preint: NULL or [n][VPL_NFRAMES], pre_integrations[1..10] after step 3 (entry 0 zeroed);
 * image_preint: NULL or [n][VPL_INIT_MAX_FRAMES], the re-propagated image pre-integrations 1 .. F-1 (the other entries zeroed).
 * A sequence that fails (ok = 0) has everything behind the failing stage zeroed; delta_bg, g_linear and s_linear are always set.
 * Host in, host out: one host-to-device copy, the kernels, one copy back and one synchronisation.
 * Refused before anything is launched -- VPL_E_INVALID: null arrays, F < 11, key not as described, an interval with
 * n_samples < 1; VPL_E_CAPACITY: F > VPL_INIT_MAX_FRAMES, n > max_windows.  A non-finite input is not refused: the sequence
 * comes back with ok = 0 and VPL_INIT_FAIL_NONFINITE. */
int vpl_init_align_batch(vpl_ctx* ctx, int n, const vpl_init_input* in, const vpl_ba_options* opt, vpl_init_result* out,
                         vpl_preintegration* window_preint, vpl_preintegration* image_preint);
/* Host only, no device call: the pre-integration jobs of step 3 for one sequence as vpl_init_align_batch builds them --
 * jobs[j][3] = (offset, nsamples, acc0_row) for j = 0 .. F-2 the image intervals 1 .. F-1 and j = F-1 .. F+8 the window
 * intervals 1 .. 10; offset in samples; acc0_row: the sample row whose measurement starts the job (always offset - 1),
 * -1 = the input's acc0 / gyr0.  jobs needs room for F + 9 rows.  Refusals as above. */
int vpl_init_debug_jobs(int n_frames, const int* n_samples, const int* key, int* jobs);

/* ---- vision-only initial structure  (replaces GlobalSFM::construct, initial/initial_sfm.cpp:117-312, and the PnP of every
 *      non-key image frame, estimator.cpp:432-501, inside Estimator::initialStructure) for n sequences in one call ----------- *
 * The relative pose before it (relativePose / solveRelativeRT) is vpl_init_relative_pose_batch below, whose result -- l,
 * relative_R, relative_T -- is an input here; vpl_init_visual_batch runs the two in a row.  What stays with the caller is
 * OpenCV's own random sequence (the device draws its samples from a stream of its own), CalibrationExRotation and the wiring
 * into vpl_odo_init.  R and T of the result have the form vpl_init_input.R / .T take.  Per sequence, on the device:
 *   1. the chain of construct (k_sfm_construct, one work-group per sequence): frames l and 10 from the relative pose; forward,
 *      l+1 .. 9: PnP from the neighbour's pose, triangulation against frame 10; l against l+1 .. 9; backward, l-1 .. 0: PnP,
 *      triangulation against l; what is left from its first and last observation.  Which track is triangulated when and from
 *      which frames, and which tracks a PnP sees, depends on where observations exist only: the host builds that schedule as
 *      integer tables (vpl_sfm_debug_plan) and the device works from them;
 *   2. the full BA in the same launch: 11 cameras, the rotation of l and the translations of l and frame 10 constant, every
 *      triangulated point a 3 x 3 block eliminated into the reduced camera system (57 free dims, tile Cholesky in LDS);
 *   3. the PnP of the non-key image frames (k_sfm_frames, one work-group per frame) from the pose of the key frame
 *      estimator.cpp:440-453 picks, then R / T of every image frame (k_sfm_finish).
 * One Levenberg-Marquardt routine serves all three: ceres' trust-region minimiser with its defaults (Jacobi scaling, initial
 * radius 1e4, min_relative_decrease 1e-3, tolerances 1e-6 / 1e-10 / 1e-8, 50 iterations) on ReprojectionError3D with analytic
 * Jacobians and QuaternionParameterization.  Deviations: cv::solvePnP(ITERATIVE, useExtrinsicGuess) is that routine with the
 * points constant (points and observations rounded to float as cv::Point3f / cv::Point2f do) -- the same minimiser where the
 * problem is well posed, not the same iterates; max_solver_time_in_seconds = 0.2 has no counterpart, only the iteration cap
 * ends a solve that does not converge.  FP64 throughout; every sum in a fixed order.
 * A sequence's result has the same bits wherever it sits in the batch and whatever else the batch holds. */
#define VPL_SFM_MAX_TRACKS 1024        /* point tracks per sequence */
#define VPL_SFM_MAX_FRAME_POINTS 1024  /* (id, x, y) entries of one non-key image frame */
#define VPL_SFM_FAIL_KEY_PNP 1         /* a key frame's PnP saw fewer than 10 points              (initial_sfm.cpp:45-50) */
#define VPL_SFM_FAIL_FRAME_PNP 2       /* a non-key frame's PnP saw fewer than 6                  (estimator.cpp:481) */
#define VPL_SFM_FAIL_BA 4              /* the BA ended neither in CONVERGENCE nor with final_cost < 5e-3 (initial_sfm.cpp:281) */
#define VPL_SFM_FAIL_NUMERIC 8         /* a factorisation failed or a value was not finite */
typedef struct vpl_sfm_input {
  int n_frames;               /* F = all_image_frame.size(), 11 <= F <= VPL_INIT_MAX_FRAMES */
  int key[VPL_NFRAMES];       /* image-frame index of window frame i, as in vpl_init_input */
  int l;                      /* 0 .. 9: the window frame relativePose chose */
  double relative_R[9], relative_T[3]; /* row-major; what relativePose returned */
  double ric[9];              /* RIC[0], row-major */
  int n_tracks;               /* f_manager.feature in list order, <= VPL_SFM_MAX_TRACKS */
  const int* track_id;        /* [n_tracks] feature_id */
  const int* track_start;     /* [n_tracks] start_frame (a window frame) */
  const int* track_nobs;      /* [n_tracks] 1 .. 11 observations in consecutive window frames, start + nobs <= 11 */
  const double* track_obs;    /* [sum nobs][2] (x, y) of feature_per_frame, track after track */
  const int* frame_npts;      /* [F] entries of image frame f's point list; read for non-key frames only */
  const int* frame_id;        /* [sum over the non-key frames, in frame order] feature id */
  const double* frame_xy;     /* [the same][2] */
} vpl_sfm_input;
typedef struct vpl_sfm_result {
  int ok;                     /* 1: construct returned true, every non-key frame's PnP ran, every result is finite */
  int fail;                   /* VPL_SFM_FAIL_* mask, 0 when ok */
  int n_tracked;              /* entries of sfm_tracked_points */
  int iterations, successful_steps, termination; /* of the BA, as vpl_solve_report counts them */
  int pnp_iterations[VPL_NFRAMES];           /* iterations of the key frame's PnP inside the chain, -1: none */
  int frame_iterations[VPL_INIT_MAX_FRAMES]; /* iterations of the non-key image frame's PnP, -1: none */
  double initial_cost, final_cost;           /* of the BA */
  double chain_q[VPL_NFRAMES][4], chain_t[VPL_NFRAMES][3]; /* c_rotation (w, x, y, z) / c_translation after the chain */
  double ba_q[VPL_NFRAMES][4], ba_t[VPL_NFRAMES][3];       /* ... after the BA */
  double Q[VPL_NFRAMES][4], T[VPL_NFRAMES][3];             /* q (w, x, y, z) and T as construct returns them */
  double frame_R[VPL_INIT_MAX_FRAMES][9], frame_T[VPL_INIT_MAX_FRAMES][3]; /* ImageFrame::R / T: vpl_init_input.R / .T */
} vpl_sfm_result;
/* in [n], out [n].  points_chain / points_ba: NULL or [n][VPL_SFM_MAX_TRACKS][3], every track's position after the chain / after
 * the BA (a track that never gets one: zero).  tracked_id / tracked_xyz: NULL or [n][VPL_SFM_MAX_TRACKS] / [..][3],
 * sfm_tracked_points in track order, n_tracked entries.  A sequence that fails (ok = 0) has everything behind the failing stage
 * zeroed -- the chain (a starved key-frame PnP zeroes the chain's own output too), the BA, Q / T and the tracked points, the
 * frames; the other sequences of the batch are untouched by it.  Host in, host out: one host-to-device copy, the kernels, one
 * copy back and one synchronisation.  Refused before anything is launched -- VPL_E_INVALID: null arrays, F < 11, key not as
 * described, l outside 0 .. 9, a track with nobs < 1 or running past frame 10, a negative count; VPL_E_CAPACITY:
 * F > VPL_INIT_MAX_FRAMES, n_tracks > VPL_SFM_MAX_TRACKS, a frame list longer than VPL_SFM_MAX_FRAME_POINTS, n > max_windows. */
int vpl_init_structure_batch(vpl_ctx* ctx, int n, const vpl_sfm_input* in, vpl_sfm_result* out, double* points_chain,
                             double* points_ba, int* tracked_id, double* tracked_xyz);
/* Host only, no device call: the schedule of construct for one sequence as vpl_init_structure_batch builds it.  step [n_tracks]:
 * 1 frame l against frame 10, 2 frames l+1 .. 9 against 10, 3 l against l+1 .. 9, 4 frames l-1 .. 0 against l, 5 first against
 * last observation, -1 the track never gets a position; fa / fb [n_tracks]: the two window frames in the order
 * triangulateTwoFrames takes them (-1 with step -1); count [11]: the points the PnP of window frame i sees, -1 for l and frame 10
 * and for a frame the chain does not reach; *first_fail: the first frame, in the order of the chain, whose count is below 10
 * (the chain ends there and every later track keeps step -1), or -1.  Refusals as above. */
int vpl_sfm_debug_plan(int l, int n_tracks, const int* track_start, const int* track_nobs, int* step, int* fa, int* fb, int* count,
                       int* first_fail);

/* ---- relative pose  (replaces Estimator::relativePose, estimator.cpp:590-622, and MotionEstimator::solveRelativeRT,
 *      initial/solve_5pts.cpp:193-228 -- cv::findFundamentalMat(FM_RANSAC, 0.3 / 460, 0.99) and cv::recoverPose) for n
 *      sequences in one call: the stage in front of vpl_init_structure_batch, whose l / relative_R / relative_T it fills ------- *
 * Per sequence and per candidate window frame i = 0 .. 9 (k_relpose_ransac, one work-group per pair, all of them side by side):
 *   1. getCorresponding(i, 10) in track-list order; corres.size() > 20 and average_parallax * 460 > 30, or the frame is not tried;
 *   2. the RANSAC of findFundamentalMat: 7-point minimal samples, every real root of det(lambda F1 + (1 - lambda) F2) = 0 in
 *      ascending lambda a hypothesis, the error of FMEstimatorCallback::computeError against (0.3 / 460)^2, a hypothesis wins with
 *      good > max(best, 6), confidence 0.99, at most 1000 iterations, the adaptive stop.  256 iterations run at a time, one
 *      lane each; the sequential rule is replayed over their counts in (iteration, root) order, so the result is that of the
 *      sequential loop over the same sample stream;
 *   3. recoverPose (solve_5pts.cpp:30-181): SVD of the winning F, R1 / R2 / +-t, the four cheirality masks ANDed with the RANSAC
 *      mask, the >= cascade; Rotation = R^T, Translation = -R^T t; success with good > 12.
 * k_relpose_finish picks l, the smallest i that succeeded.  Every candidate is evaluated and reported, also those behind l.
 * What replaces OpenCV's random sequence is a counter-based integer stream of `seed`, the candidate, the iteration and the
 * draw (csrc/init_relpose_plan.h; vpl_relpose_debug_plan hands it out): the same rules on another sample stream -- the same
 * answer wherever the problem is well posed, not the same iterates.  Deviations: F is not scaled to F33 = 1 (it is handed out
 * with unit Frobenius norm; nothing downstream depends on its scale); where OpenCV would assert on an empty model the
 * candidate gets VPL_RELPOSE_NO_MODEL; findFundamentalMat's collinearity test of a sample (checkSubset) is not made, a
 * degenerate sample is one more hypothesis that does not win.  FP64 throughout, every sum in a fixed order, no atomics: a
 * sequence's result has the same bits wherever it sits in the batch and whatever else the batch holds. */
#define VPL_RELPOSE_MAX_ITERS 1000
#define VPL_RELPOSE_FEW_CORRES 0       /* corres.size() <= 20: not tried                          (estimator.cpp:598) */
#define VPL_RELPOSE_LOW_PARALLAX 1     /* average_parallax * 460 <= 30: not tried                  (estimator.cpp:613) */
#define VPL_RELPOSE_NO_MODEL 2         /* no hypothesis had more than 6 inliers */
#define VPL_RELPOSE_FEW_GOOD 3         /* recoverPose's count <= 12                                (solve_5pts.cpp:222) */
#define VPL_RELPOSE_SUCCESS 4
#define VPL_RELPOSE_FAIL_NONE 1        /* no candidate frame succeeded: relativePose returns false */
#define VPL_RELPOSE_FAIL_NUMERIC 8     /* a NaN / inf among the correspondences of a candidate */
typedef struct vpl_relpose_input {
  int n_tracks;               /* the track table exactly as vpl_sfm_input has it */
  const int* track_start;     /* [n_tracks] */
  const int* track_nobs;      /* [n_tracks] */
  const double* track_obs;    /* [sum nobs][2] */
  unsigned long long seed;    /* of the sample stream */
} vpl_relpose_input;
typedef struct vpl_relpose_candidate {
  int n_corres;               /* corres.size() */
  int status;                 /* VPL_RELPOSE_* */
  int iterations;             /* niters when the loop ended (0: not tried) */
  int best_iteration, best_root; /* of the winning hypothesis, -1: none */
  int inliers;                /* its inlier count */
  int good;                   /* recoverPose's count */
  int numeric;                /* 1: a correspondence was not finite */
  int pose_choice;            /* which of recoverPose's four poses won the vote: 0 (R1, t), 1 (R2, t), 2 (R1, -t), 3 (R2, -t) */
  int pad_;
  double average_parallax;
  double F[9];                /* the winning F, row-major, x_10^T F x_i = 0, unit Frobenius norm */
  double R[9], T[3];          /* Rotation / Translation of solveRelativeRT for this candidate, row-major */
} vpl_relpose_candidate;
typedef struct vpl_relpose_result {
  int ok;                     /* 1: relativePose returns true */
  int fail;                   /* VPL_RELPOSE_FAIL_* mask, 0 when ok */
  int l;                      /* the smallest i with VPL_RELPOSE_SUCCESS; -1 when ok = 0 */
  int pad_;
  double relative_R[9], relative_T[3]; /* candidate l's R / T, in the form vpl_sfm_input takes; zero when ok = 0 */
  vpl_relpose_candidate cand[VPL_WINDOW_SIZE];
} vpl_relpose_result;
/* in [n], out [n].  mask_ransac / mask_pose: NULL or [n][10][VPL_SFM_MAX_TRACKS] bytes, the inlier mask of the winning
 * hypothesis and the mask recoverPose leaves, in correspondence order (zero behind n_corres and for a candidate without a
 * model).  hyp_count: NULL or [n][10][1000][3], the inlier count of every hypothesis the sequential loop evaluates, -1 for a
 * root that does not exist and for every iteration the loop does not reach.  Host in, host out: one host-to-device copy, the
 * kernels, one copy back and one synchronisation.  Refused before anything is allocated -- VPL_E_INVALID: null arrays, a
 * track with nobs < 1 or running past frame 10, a negative count; VPL_E_CAPACITY: n_tracks > VPL_SFM_MAX_TRACKS,
 * n > max_windows.  A non-finite observation is not refused: the sequence comes back with ok = 0 and
 * VPL_RELPOSE_FAIL_NUMERIC, the other sequences of the batch are untouched by it. */
int vpl_init_relative_pose_batch(vpl_ctx* ctx, int n, const vpl_relpose_input* in, vpl_relpose_result* out,
                                 unsigned char* mask_ransac, unsigned char* mask_pose, int* hyp_count);
/* Host only, no device call: the sample stream and the stopping table of candidate frame i over n_corres correspondences as the
 * kernel uses them.  samples [1000][7]: the indices of every iteration's minimal sample, in the order drawn; niters_after
 * [n_corres + 1]: RANSACUpdateNumIters(0.99, (n_corres - good) / n_corres, 7, 1000) for good = 0 .. n_corres.
 * VPL_E_INVALID: i outside 0 .. 9, n_corres < 7, a null array; VPL_E_CAPACITY: n_corres > VPL_SFM_MAX_TRACKS. */
int vpl_relpose_debug_plan(unsigned long long seed, int i, int n_corres, int* samples, int* niters_after);
/* vpl_init_relative_pose_batch, then vpl_init_structure_batch over the sequences whose relative pose succeeded, with l /
 * relative_R / relative_T taken from it (those members of `in` are not read); the same host-side composition a caller would
 * write.  seeds [n].  rel [n]: the relative pose's results.  A sequence whose relative pose fails has its vpl_sfm_result zeroed
 * but for fail = VPL_SFM_FAIL_RELATIVE_POSE, and zeros in the optional arrays.  Refusals: those of the two calls. */
#define VPL_SFM_FAIL_RELATIVE_POSE 16  /* vpl_init_visual_batch: relativePose returned false */
int vpl_init_visual_batch(vpl_ctx* ctx, int n, const vpl_sfm_input* in, const unsigned long long* seeds, vpl_relpose_result* rel,
                          vpl_sfm_result* out, double* points_chain, double* points_ba, int* tracked_id, double* tracked_xyz);

/* ---- feature selector  (replaces FeatureSelector::select, feature_selector.cpp:71-198, with HorizonGenerator::imu,
 *      utility/selector/horizon_generator.cpp:24-68; use_feature_selector: 1, called at estimator_node.cpp:335-349) for n
 *      sequences in one call: expected-information greedy selection of the new features of an image -------------------------- *
 * Per sequence:
 *   1. the horizon: states k and k + 1 as given, k + 2 .. k + 4 by constant-a, constant-w propagation over n_imu steps of
 *      delta_imu, gravity (0, 0, -9.80665) -- or the caller's own five poses (which also covers the reference's ground-truth mode);
 *   2. Omega_kkH (calcInfoFromRobotMotion, addOmegaPrior), 45 x 45 over five states of position, velocity, accelerometer bias;
 *   3. every feature's depth guess: the depth of its nearest cloud point in (x, y), the lowest index on an exact tie, 1.0 when
 *      the cloud is empty (initKDTree / findNNDepth; the cloud -- x, y, depth in camera k + 1 -- is the caller's here);
 *   4. every feature's Delta (calcInfoFromFeatures): projection into frames k + 2 .. k + 4 by PinholeCamera::spaceToPlane with
 *      the radtan distortion and no sign test on the depth, inFOV with std::round, q_IC applied twice in Bh as the reference
 *      writes it; a feature no future frame sees has no matrix: as a new feature it is never a candidate (n_invisible), as a
 *      used feature it adds nothing;
 *   5. kappa greedy rounds (selectInformativeFeatures): Omega = Omega_kkH + sum of the used features' Delta (no prob on them);
 *      per round and candidate ub = sum log diag(Omega + OmegaS + p Delta) and f = logdet of the same by Cholesky; candidates
 *      with equal ub collapse to the one with the highest id (the reference's std::map; the other is eligible again once that one
 *      is taken); the largest f wins if it is > -1.0 (strictly), ties go to the larger ub; OmegaS += p Delta.  Lazy evaluation is
 *      not reproduced: since ub >= f it selects what evaluating everything selects.
 * The matrices are not factored at 45 x 45 per candidate: Delta, the used sum and OmegaS live in the 12 position dimensions of
 * states 1 .. 4; with those ordered last the 33 x 33 block and its coupling are fixed for the call, are factored once per
 * sequence, and every evaluation is logdet A + a 12 x 12 Cholesky of the Schur complement (csrc/sel_kernels.h).
 * Deviations: a candidate whose Cholesky meets a pivot that is not finite or not > 0 is not eligible in that round and is counted
 * in n_ineligible (Eigen's LLT goes on with an unfinished factor; the reference logs "logdet returned nan!" where it notices);
 * a round that selects nothing ends the loop (no later round could select anything either).  Only the PINHOLE camera model is
 * described by vpl_sel_params.  Three launches per call whatever kappa is; FP64, every sum in a fixed order: a sequence's result
 * has the same bits wherever it sits in the batch. */
#define VPL_SEL_MAX_FEATURES 1024      /* longest list of new features, of used features and of cloud points */
typedef struct vpl_sel_params {
  double acc_var, acc_bias_var;      /* the reference passes ACC_N, ACC_W */
  int max_features, init_thresh;     /* of the id book (vpl_sel_debug_book): kappa = max(0, max_features - |subset|) */
  int width, height;                 /* PINHOLE camera with radtan distortion */
  double fx, fy, cx, cy, k1, k2, p1, p2;
  double q_ic[4];                    /* w, x, y, z */
  double t_ic[3];
} vpl_sel_params;
typedef struct vpl_sel_input {
  double P0[3], Q0[4], V0[3], Ba0[3];   /* state k (slot 10 of the window); quaternions w, x, y, z */
  double P1[3], Q1[4], V1[3], Ba1[3];   /* state k + 1, the IMU-propagated new frame (Ba1 is carried, the reference does not read it) */
  double acc[3], gyr[3];                /* the last accelerometer sample and the unbiased gyroscope sample */
  double delta_imu;                     /* > 0 */
  int n_imu;                            /* >= 1 */
  int kappa;                            /* >= 0: the number of greedy rounds */
  const double* horizon;                /* NULL, or [5][7] = position, quaternion of states k .. k + 4 (then step 1 is skipped) */
  int n_new;
  const int* new_id;                    /* [n_new], distinct */
  const double *new_x, *new_y, *new_prob;   /* [n_new]: normalised image coordinates and the tracking probability */
  int n_used;
  const double *used_x, *used_y;        /* [n_used] */
  int n_cloud;
  const double* cloud;                  /* [n_cloud][3] = x, y (normalised, camera k + 1), depth */
} vpl_sel_input;
typedef struct vpl_sel_result {
  int n_selected;                       /* <= min(kappa, n_new) */
  int n_invisible;                      /* new features no future frame sees */
  int n_ineligible;                     /* evaluations (candidate, round) that met a bad pivot */
  int n_candidates;                     /* n_new - n_invisible */
} vpl_sel_result;
/* in [n], out [n]; selected_id / round_f [n][VPL_SEL_MAX_FEATURES]: the ids in selection order and the f each was selected with,
 * n_selected entries, zero behind.  Host in, host out: one host-to-device copy, three kernels, one copy back and one
 * synchronisation.  Refused before anything is written -- VPL_E_INVALID: null arrays, n_imu < 1, delta_imu not > 0 (the
 * reference produces 0 on its first image through a static, and its result is infinite), a negative count, width or height < 1, an id twice in new_id;
 * VPL_E_CAPACITY: a list longer than VPL_SEL_MAX_FEATURES, n > max_windows. */
int vpl_select_features_batch(vpl_ctx* ctx, int n, const vpl_sel_params* params, const vpl_sel_input* in, vpl_sel_result* out,
                              int* selected_id, double* round_f);
/* One sequence, one round's values after a forced prefix of selections: prefix_id [n_prefix] are taken first, in that order
 * (an id that is not a candidate is passed over).  f / ub [n_new]: the round's values of every new feature, NaN for one that is
 * not a candidate (invisible, in the prefix) and f = NaN for one that is not eligible.  omega45x45 [45 * 45]: Omega_kkH, row-major,
 * natural order.  delta12 [(n_new + n_used)][78]: every feature's Delta over the 12 position dimensions of states 1 .. 4 (rows and
 * columns 9 i .. 9 i + 2, i = 1 .. 4), packed lower triangle row after row; zeros for an invisible feature.  Any output may be
 * NULL.  kappa is not read.  Refusals as above. */
int vpl_select_debug_values(vpl_ctx* ctx, const vpl_sel_params* params, const vpl_sel_input* in, const int* prefix_id, int n_prefix,
                            double* f, double* ub, double* omega45x45, double* delta12);
/* kernel launches and bytes copied each way by the last vpl_select_features_batch / vpl_select_debug_values of the context */
int vpl_select_stats(vpl_ctx* ctx, long long* launches, long long* h2d_bytes, long long* d2h_bytes);
/* Host only, no device call: the id book of select() (lastFeatureId_, trackedFeatures_, firstImage_, init_thresh, kappa) replayed
 * over a script of n_images images (csrc/sel_book.h).  Image s: its feature ids n_ids[s] of ids (one image after the other),
 * initialized[s] (solver_flag == NON_LINEAR), and n_offer[s] of offer standing in for the greedy selection: the first kappa
 * offered ids that are new in this image are "selected".  Out, per image: n_new[s], kappa[s], n_selected[s] and
 * selected[s * max_ids ..], n_out[s] and out_ids[s * max_ids ..] (ascending: what is handed to the back end), n_tracked[s] and
 * last_id[s] after the image; tracked [max_tracked]: the tracked list after the last image, in its order (it only grows).
 * VPL_E_INVALID: null arrays, negative counts; VPL_E_CAPACITY: an image with more than max_ids distinct ids, a tracked list longer
 * than max_tracked. */
int vpl_sel_debug_book(int max_features, int init_thresh, int n_images, const int* n_ids, const int* ids, const unsigned char* initialized,
                       const int* n_offer, const int* offer, int max_ids, int* n_new, int* kappa, int* n_selected, int* selected,
                       int* n_out, int* out_ids, int* n_tracked, int* last_id, int max_tracked, int* tracked);

/* ---- single-factor batch evaluators ------------------------------------- *
 * Each replaces one CostFunction::Evaluate (signature
 *   bool Evaluate(double const* const* parameters, double* residuals, double** jacobians) const )
 * for n factors at once.  Parameter blocks are packed contiguously per factor
 * in the reference's order; residuals [n][R]; jacobians may be NULL, otherwise
 * row-major blocks concatenated per factor in parameter order.              */

/* ProjectionFactor::Evaluate (projection_factor.cpp:26-126), SizedCostFunction<2,7,7,7,1>.
 * params [n][22] = pose_i, pose_j, ex_pose, inv_dep ; pts [n][6] = pts_i, pts_j ;
 * residuals [n][2] ; jac [n][44] = 2x7, 2x7, 2x7, 2x1.  Host pointers. */
int vpl_projection_factor_evaluate(vpl_ctx* ctx, int n, const double* params, const double* pts,
                                   double sqrt_info, double* residuals, double* jac);
/* lineProjectionFactor::Evaluate (line_projection_factor.cpp:251-380), <2,7,7,4>.
 * params [n][18] = pose, ex_pose, orth ; obs [n][4] ; jac [n][36] = 2x7,2x7,2x4. */
int vpl_line_factor_evaluate(vpl_ctx* ctx, int n, const double* params, const double* obs,
                             double sqrt_info, double* residuals, double* jac);
/* vpProjectionFactor::Evaluate (line_projection_factor.cpp:11-153), <2,7,7,4>. obs [n][3]. */
int vpl_vp_factor_evaluate(vpl_ctx* ctx, int n, const double* params, const double* vp,
                           double sqrt_info, double* residuals, double* jac);
/* IMUFactor::Evaluate (imu_factor.h:23-182), <15,7,9,7,9>.
 * params [n][32] = pose_i, sb_i, pose_j, sb_j ; jac [n][480] = 15x7,15x9,15x7,15x9. */
int vpl_imu_factor_evaluate(vpl_ctx* ctx, int n, const double* params, const vpl_preintegration* pre,
                            double g_norm, double* residuals, double* jac);
/* MarginalizationFactor::Evaluate (marginalization_factor.cpp:492-542).
 * params: concatenated kept blocks in prior order (global sizes); residuals [prior->n];
 * jac: for block b a row-major n x global_size matrix, concatenated in block order. */
int vpl_prior_factor_evaluate(vpl_ctx* ctx, const vpl_prior* prior, const double* params,
                              double* residuals, double* jac);

/* PoseLocalParameterization::Plus (pose_local_parameterization.cpp:3-19): x[n][7], delta[n][6]. */
int vpl_pose_plus(vpl_ctx* ctx, int n, const double* x, const double* delta, double* x_plus_delta);
/* LineOrthParameterization::Plus (line_parameterization.cpp:7-93): x[n][4], delta[n][4]. */
int vpl_line_orth_plus(vpl_ctx* ctx, int n, const double* x, const double* delta, double* x_plus_delta);

/* ---- the window solve ---------------------------------------------------- *
 * Replaces the body of Estimator::optimizationwithLine() (estimator.cpp:1043-1453):
 * vector2double -> ceres::Solve(DENSE_SCHUR, DOGLEG, max_num_iterations) ->
 * double2vector2 -> [removeLineOutlier] -> marginalisation -> new prior.
 *
 * Three-phase form so that a bench can keep inputs resident in HBM:
 *   upload  : host windows -> device SoA        (PCIe, not in the timed region)
 *   solve   : everything on device, no host round trip, asynchronous on the stream
 *   download: device -> host windows / priors / reports
 * Refusals (VPL_E_INVALID / VPL_E_CAPACITY, message in vpl_last_error): more windows / points / observations / lines than the
 * context was created for, a track that leaves the window, a point track of one observation, an unknown marginalization_flag,
 * a prior of impossible size.  A refusal that comes after the upload has begun to rewrite the batch leaves the context WITHOUT
 * a batch: solve / download / reset_state return VPL_E_INVALID until the next successful upload.
 * A window with a NaN / inf among its inputs is not refused: its solve fails as ceres fails it (report: termination 2,
 * iterations = num_successful_steps = -1, costs 0; states untouched), the other windows of the batch are unaffected.
 */
int vpl_ba_upload(vpl_ctx* ctx, int n_windows, const vpl_window* windows, const vpl_ba_options* opt);
/* The next windows of a sequence: as vpl_ba_upload, but window i takes the prior that the context's PREVIOUS solve left for
 * window i (MarginalizationInfo of that solve, estimator.cpp:1229-1447 -> last_marginalization_info) -- it stays in HBM,
 * handed from the marginalisation's output to the next solve's input on the device; windows[i].prior / has_prior are
 * ignored.  Needs a previous solve (or vpl_ba_marginalize) of the same batch size with a marginalisation flag other than
 * VPL_MARGIN_NONE and NO upload on the context since (vpl_ba_triangulate_*, vpl_ba_only_line_opt, vpl_ba_slide_window and the
 * stages of vpl_ba_solve_odometry upload too): VPL_E_INVALID otherwise. */
int vpl_ba_upload_chained(vpl_ctx* ctx, int n_windows, const vpl_window* windows, const vpl_ba_options* opt);
int vpl_ba_solve(vpl_ctx* ctx);           /* enqueue one batched solve of the uploaded windows */
int vpl_ba_reset_state(vpl_ctx* ctx);     /* restore the uploaded initial states on device (for repeated timing): enqueues
                                            * nothing -- the next vpl_ba_solve restores as it starts, any other call that reads or
                                            * writes the states first copies them back */
int vpl_ba_download(vpl_ctx* ctx, int n_windows, vpl_window* windows, vpl_prior* priors_out,
                    vpl_solve_report* reports);
int vpl_ctx_synchronize(vpl_ctx* ctx);
/* Host <-> device traffic of upload / download: the arrays are packed into one PINNED staging arena per context; an upload is
 * one host-to-device copy + one scatter kernel, a download one gather kernel + one device-to-host copy.  No pageable memory
 * (neither the library's nor the caller's) is handed to the HIP runtime on the upload / solve / download path.
 * Leg timing: with it enabled the three calls bracket their device work with hipEvents on the context's stream;
 * vpl_ctx_leg_times returns {upload (copy + scatter), solve (all launches), download (gather + copy)} of the last calls in
 * milliseconds of DEVICE time (-1 for a leg that has not run), to be read next to the wall clock of the calls.  While it is on,
 * vpl_ba_solve launches kernel by kernel (no graph replay). */
int vpl_ctx_enable_leg_timing(vpl_ctx* ctx, int enable);
int vpl_ctx_leg_times(vpl_ctx* ctx, double* ms3);
/* States of the solved batch into a caller-owned DEVICE buffer, [n_windows][183] doubles per window: pose[11][7],
 * speed_bias[11][9], ex_pose[7] -- after double2vector2.  Asynchronous on the context's stream.  This is what a multi-GPU
 * run hands to its collective (RCCL all-gather of the batch's results) without a host staging copy. */
int vpl_ba_pack_states_device(vpl_ctx* ctx, int n_windows, void* d_states);

/* Convenience: upload + solve + synchronize + download. */
int vpl_ba_solve_windows(vpl_ctx* ctx, int n_windows, vpl_window* windows, const vpl_ba_options* opt,
                         vpl_prior* priors_out, vpl_solve_report* reports);

/* ---- marginalisation on its own -------------------------------------------------------------------------- *
 * Replaces MarginalizationInfo::{addResidualBlockInfo, preMarginalize, marginalize, getParameterBlocks}
 * (marginalization_factor.cpp:89-129,177-363,458-478) as Estimator::optimizationwithLine() drives them
 * (estimator.cpp:1229-1378 for VPL_MARGIN_OLD, :1380-1447 for VPL_MARGIN_SECOND_NEW), WITHOUT a solve: the factor subset of
 * the flag (MARGIN_OLD: last prior, IMU factor (0,1), the point and line factors of the tracks that start in frame 0; no VP
 * factors -- MARGIN_SECOND_NEW: the last prior alone) is linearised at the windows' CURRENT states, landmarks and dropped
 * blocks are eliminated, and the kept block is returned as the next prior: priors_out[w] = (n, kept-block table with the
 * frames renumbered for the next window, x0, J0, r0), m[w] / n[w] = MarginalizationInfo::m / n (either may be NULL).
 * The windows are not modified.  With VPL_MARGIN_SECOND_NEW a window whose prior does not hold pose WINDOW_SIZE-1 gets its
 * input prior back (estimator.cpp:1385).  Synchronous (upload, kernels, download). */
int vpl_ba_marginalize(vpl_ctx* ctx, int n_windows, const vpl_window* windows, const vpl_ba_options* opt,
                       int marginalization_flag, vpl_prior* priors_out, int* m, int* n);
/* How the kept block A (with b) becomes the next prior (J0, r0) -- marginalization_factor.cpp:349-357, selected per context:
 *   VPL_PRIOR_PIVOTED_CHOLESKY (default): A's pivoted Cholesky factor, cut where a pivot drops below 1e-8.
 *                               The same prior up to an orthogonal Q (J0' = Q J0, r0' = Q r0) where A is well determined;
 *                               it keeps one to five directions fewer than the reference on weakly determined blocks.
 *   VPL_PRIOR_EIGEN:            the reference's rule: SelfAdjointEigenSolver of A (its lower triangle) by a parallel Jacobi
 *                               on the device, eigenvalues S > 1e-8 kept, J0 = sqrt(S) V^T, r0 = S^-1/2 V^T b -- rows in
 *                               ascending eigenvalue order, dropped rows zero, each eigenvector's largest component positive.
 *                               Costs a second kernel (k_prior_eigen) after the factorisation.
 * The rule applies to every entry point that marginalises: vpl_ba_solve / _solve_windows, vpl_ba_marginalize(_async),
 * vpl_ba_solve_odometry, and so the prior vpl_ba_upload_chained hands over.  A pending asynchronous call is collected first:
 * a call runs under the rule that was in force when it was enqueued.  An unknown rule: VPL_E_INVALID. */
#define VPL_PRIOR_PIVOTED_CHOLESKY 0
#define VPL_PRIOR_EIGEN 1
int vpl_ba_set_prior_rule(vpl_ctx* ctx, int rule);

/* ---- line map maintenance that precedes the main solve (estimator.cpp:635-638) -------------------------------- */
/* FeatureManager::triangulateLine (feature_manager.cpp:413-563): lines with line_triangulated[i] == 0 are triangulated
 * from the two observations with the largest plane angle (skipped when cos > 0.998); on success line_plk[i] is written
 * and line_triangulated[i] set.  Synchronous (upload, kernel, download). */
int vpl_ba_triangulate_lines(vpl_ctx* ctx, int n_windows, vpl_window* windows);
/* What Estimator::slideWindow did to the track lists of one window (the lists themselves stay with the caller) */
typedef struct vpl_slide_tracks {
  int* point_start; /* [n_points] start_frame after the slide */
  int* point_nobs;  /* [n_points] observations left; 0 = the track was erased */
  int* point_drop;  /* [n_points] index (within the track) of the observation that was removed, -1 = none */
  int* line_start;  /* [n_lines] */
  int* line_nobs;   /* [n_lines] */
  int* line_drop;   /* [n_lines] */
} vpl_slide_tracks;
/* Estimator::slideWindow (estimator.cpp:1731-1851) of full windows in the NON_LINEAR state.
 * VPL_MARGIN_OLD: pose / speed_bias move one frame down (frame 10 keeps the newest state), then
 *   FeatureManager::removeBackShiftDepth (feature_manager.cpp:800-874): tracks that started in frame 0 lose that observation,
 *   are erased when fewer than two remain, else are re-anchored in the next frame -- inv_depth from the point carried over
 *   (non-positive depth -> init_depth), line_plk by plk_to_pose; all other tracks start one frame earlier.
 * VPL_MARGIN_SECOND_NEW: frame 10 is copied over frame 9, then FeatureManager::removeFront (feature_manager.cpp:915-956).
 * pose, speed_bias, inv_depth, line_plk are updated in place; the new track layout is reported in `tracks`.  The IMU
 * buffers (preint) are the caller's: the reference re-integrates them sample by sample (estimator.cpp:1786-1797).
 * Every track of the FeatureManager may be passed (any length >= 1, any start frame).  Synchronous. */
int vpl_ba_slide_window(vpl_ctx* ctx, int n_windows, vpl_window* windows, int marginalization_flag, double init_depth,
                        vpl_slide_tracks* tracks);
/* FeatureManager::triangulate (feature_manager.cpp:565-621): tracks whose inv_depth is negative (estimated_depth not set,
 * -1 in the reference) get the depth of the DLT / SVD over all their observations; a result below 0.1 becomes init_depth
 * (INIT_DEPTH = 5.0, parameters.cpp:138).  inv_depth is written.  Synchronous. */
int vpl_ba_triangulate_points(vpl_ctx* ctx, int n_windows, vpl_window* windows, double init_depth);
/* Estimator::onlyLineOpt (estimator.cpp:950-1039): line-only Levenberg-Marquardt with the poses and the extrinsic
 * constant, CauchyLoss(1.0), at most options.num_iterations iterations, then double2vector + removeLineOutlier.
 * Updates line_plk / line_removed of the triangulated lines; windows with fewer than four such lines are left untouched
 * (as :1019-1022).  Synchronous (asynchronous variant below). */
int vpl_ba_only_line_opt(vpl_ctx* ctx, int n_windows, vpl_window* windows, const vpl_ba_options* opt,
                         vpl_solve_report* reports);

/* Estimator::solveOdometry (estimator.cpp:624-648) in one call:  f_manager.triangulate  ||  (f_manager.triangulateLine ->
 * onlyLineOpt)  ->  optimizationwithLine.  `windows` are packed as for the single stages (every point track with
 * inv_depth < 0 where estimated_depth is unset; every line track that passes the LINE_MIN_OBS filter with its
 * is_triangulation flag; line_removed writable).  On return: inv_depth / line_plk / line_triangulated / line_removed as the
 * three map stages leave them -- a track erased by removeLineOutlier has line_removed = 1 and line_triangulated = 0 and took
 * no part in the solve -- and states, priors_out and reports as vpl_ba_solve_windows leaves them; line_reports (may be NULL)
 * are onlyLineOpt's.  The stages run back to back (the two triangulations on one upload): which lines take part changes between them
 * and the kernels' layout tables are built on the host from that set. */
int vpl_ba_solve_odometry(vpl_ctx* ctx, int n_windows, vpl_window* windows, const vpl_ba_options* opt, double init_depth,
                          vpl_prior* priors_out, vpl_solve_report* line_reports, vpl_solve_report* reports);
/* wall clock of the three stages of the context's last vpl_ba_solve_odometry, in ms: the two triangulations | onlyLineOpt |
 * optimizationwithLine (tools/time_odometry.py) */
int vpl_ba_debug_odometry_ms(vpl_ctx* ctx, double* ms3);

/* ---- asynchronous variants of the five entry points above -------------------------------------------------------------- *
 * Same arguments, same results, but the call returns as soon as its uploads, kernels and read-backs are ENQUEUED on the
 * context's stream; the results are written into the caller's arrays (windows, tracks, priors_out, m, n, reports) by
 * vpl_ba_collect -- or by the next call on the context that touches the batch (any upload / solve / download, another of
 * these calls, vpl_ctx_synchronize), which completes a pending call first.  The host is free in between (the reference's
 * processImage() does its feature-manager bookkeeping on the host, estimator.cpp:121-200); the arrays a call was given must stay
 * alive, and must not be read, until it has been collected.  One call can be pending per context.  The integer track
 * bookkeeping of vpl_ba_slide_window (`tracks`) is host work and is complete when the call returns; its states, inverse
 * depths and Pluecker lines are not. */
int vpl_ba_triangulate_points_async(vpl_ctx* ctx, int n_windows, vpl_window* windows, double init_depth);
int vpl_ba_triangulate_lines_async(vpl_ctx* ctx, int n_windows, vpl_window* windows);
int vpl_ba_only_line_opt_async(vpl_ctx* ctx, int n_windows, vpl_window* windows, const vpl_ba_options* opt,
                               vpl_solve_report* reports);
int vpl_ba_slide_window_async(vpl_ctx* ctx, int n_windows, vpl_window* windows, int marginalization_flag, double init_depth,
                              vpl_slide_tracks* tracks);
int vpl_ba_marginalize_async(vpl_ctx* ctx, int n_windows, const vpl_window* windows, const vpl_ba_options* opt,
                             int marginalization_flag, vpl_prior* priors_out, int* m, int* n);
/* Completes the pending asynchronous call, if any (waits for the stream, writes the results).  Returns its status. */
int vpl_ba_collect(vpl_ctx* ctx);

/* ---- keyframe session: the feature manager and the window resident on the device ---------------------------------------- *
 * Estimator::processImage's loop (estimator.cpp:121-200, 624-648, 1731-1851) for n_seq independent sequences, one call per
 * keyframe: the session owns what the reference's FeatureManager and window state own -- every track's observations, inverse
 * depth, Pluecker line and triangulation flag, the 11 states, the extrinsic, the 11 pre-integrations and the last prior --
 * in device memory, from keyframe to keyframe.  Per keyframe only the NEW frame travels host -> device (its observations, one
 * state, one pre-integration) beside the kernels' integer layout tables, and only the result struct and a few integers per
 * track (triangulated / erased / depth sign) and per prior block travel back.  The host keeps the integer side of the tracks
 * (id, start, number of observations, triangulated), in insertion order (f_manager.feature is a std::list).
 * The session borrows `ctx` (one session per context; the context's other entry points stay usable between keyframes and the
 * prior rule set on it applies); sequence i is window i of the context's batches, so n_seq <= max_windows, and the tracks one
 * solve takes must fit the context's max_points / max_lines / *_obs. */
typedef struct vpl_odo vpl_odo;
/* max_point_tracks / max_line_tracks: per sequence, ALL tracks of the feature manager, short ones included. */
int vpl_odo_create(vpl_odo** out, vpl_ctx* ctx, int n_seq, const vpl_ba_options* opt, double init_depth, int line_min_obs,
                   int max_point_tracks, int max_line_tracks);
void vpl_odo_destroy(vpl_odo* odo);

typedef struct vpl_odo_frame {   /* one image of one sequence, as processImage() receives it */
  double pose[7], speed_bias[9]; /* the propagated state of the new frame (processIMU's Ps / Rs / Vs / Bas / Bgs) */
  vpl_preintegration preint;     /* of the interval that ends in this frame (the IMU buffers stay the caller's, as for
                                    vpl_ba_slide_window; after VPL_MARGIN_SECOND_NEW slot 9 keeps its pre-integration -- the
                                    IMU form below, vpl_odo_enable_imu, merges it as the reference does) */
  int n_points; const int* point_id; const double* point_obs; /* [n][3]  x,y,1 */
  int n_lines;  const int* line_id;  const double* line_obs;  /* [n][8]  as vpl_window.line_obs */
} vpl_odo_frame;

/* Frames 0..10 of sequence `seq` before its first keyframe (the window the initialisation hands over): states, extrinsic,
 * pre-integrations 1..10 (entry 0 unused) and the observations frame by frame (frames[f]: n_*, *_id, *_obs only).  Replaces
 * whatever the sequence held, its prior included. */
int vpl_odo_set_window(vpl_odo* odo, int seq, const double pose[][7], const double speed_bias[][9], const double ex_pose[7],
                       const vpl_preintegration* preint, const vpl_odo_frame* frames);

/* The session takes its first window from the visual-inertial alignment (vpl_init_align_batch above) instead of from
 * vpl_odo_set_window: Estimator::visualInitialAlign (estimator.cpp:512-588) for every sequence of the session in one call, with
 * the results staying on the device.  in [n_seq]: the alignment's input; ex_pose [n_seq][7]: para_Ex_Pose (its rotation is RIC, its
 * translation should be in.tic); frames [n_seq][11]: the observations of the window's frames (n_*, *_id, *_obs only); out [n_seq].
 *   - the observations enter the store with pose = (T_key, quat(R_key)), extrinsic = (0, qic) and every depth unset (clearDepth),
 *     so that the session's point triangulation is triangulate(Ps, TIC_TMP = 0, RIC) at SfM scale (:540-545); no line is touched;
 *   - the alignment runs (stages 1-4 of vpl_init_align_batch, the same bits);
 *   - for a sequence with ok: states, the true extrinsic and pre_integrations[1..10] enter the store and every point the solve
 *     selects is scaled, estimated_depth *= s -- a depth the 0.1 clamp set to init_depth too, as in the reference (:564-570).  The
 *     sequence then holds a window: no prior, last_P = pose[9], its keyframe decision when the rule is on; in an IMU-enabled session
 *     the samples of window interval 10 become slot 10's buffer (no vpl_odo_set_imu needed);
 *   - a sequence without ok ends WITHOUT a window, whatever it held before.
 * Refusals leave every sequence as it was: those of vpl_init_align_batch and of vpl_odo_set_window, between vpl_odo_solve and
 * vpl_odo_advance (VPL_E_INVALID), the selected tracks beyond the context's capacities, window interval 10 longer than max_samples
 * (VPL_E_CAPACITY).  Not on the per-keyframe path: it synchronises and allocates. */
int vpl_odo_init(vpl_odo* odo, const vpl_init_input* in, const double (*ex_pose)[7], const vpl_odo_frame* frames,
                 vpl_init_result* out);

typedef struct vpl_odo_result {  /* per sequence */
  double pose[VPL_NFRAMES][7], speed_bias[VPL_NFRAMES][9], ex_pose[7]; /* after double2vector2, BEFORE the slide */
  vpl_solve_report line_report, report; /* onlyLineOpt's, the solve's */
  int n_points_solved, n_lines_solved;  /* tracks that took part in the solve */
  int n_point_tracks, n_line_tracks;    /* tracks alive after the slide and the new frame */
  int n_ignored;                        /* observations of an id that had been lost and came back (not continued) */
} vpl_odo_result;

/* One keyframe of every sequence: solveOdometry on the full window (points used_num >= 2 && start < WINDOW_SIZE - 2, lines
 * used_num >= line_min_obs likewise, estimator.cpp:1100-1102, 1132-1133) -> removeFailures (solved points whose inverse depth is
 * not > 0) and the lines the solve's removeLineOutlier erased -> slideWindow(flag) on EVERY track -> the pre-integrations move
 * down -> next[seq] enters slot 10: an id continues its track only if the track's last observation is in slot 9, an unknown id
 * starts a track, an id whose track has a gap is ignored and counted.
 * marginalization_flag[seq]: VPL_MARGIN_OLD or VPL_MARGIN_SECOND_NEW; the batched solve marginalises one way per batch, so all
 * sequences of one call carry the same flag (VPL_E_INVALID otherwise) -- also when the flags are the session's own decisions
 * (vpl_odo_*_auto below): sequences that disagree are refused there, with the count for each flag in vpl_last_error.
 * Refusals leave the session as it was: null arrays, a flag other than the two, a sequence without a window (VPL_E_INVALID);
 * more tracks than the capacities (VPL_E_CAPACITY) -- checked BEFORE the solve, when it is not yet known what the solve will
 * erase: tracks alive + ids of next[seq] that belong to no track <= max_*_tracks, and the solve's selection within the context's
 * capacities.  A non-finite measurement is not refused: the solve fails as it does elsewhere (termination 2). */
int vpl_odo_keyframe(vpl_odo* odo, const vpl_odo_frame* next, const int* marginalization_flag, vpl_odo_result* out);
/* The two halves of vpl_odo_keyframe, for a caller whose new frame depends on the solve -- the reference starts the new
 * interval's pre-integration from the bias the solve has just estimated (estimator.cpp:1786-1797), so `next` cannot be complete
 * before `out` is known:  vpl_odo_solve = solveOdometry (out: n_*_tracks as they are before the slide, n_ignored 0);
 * vpl_odo_advance = removeFailures -> slideWindow(the solve's flag) -> next enters slot 10 (out may be NULL; n_*_tracks and
 * n_ignored are updated).  They alternate: VPL_E_INVALID out of turn; a refused vpl_odo_advance can be repeated. */
int vpl_odo_solve(vpl_odo* odo, const int* marginalization_flag, vpl_odo_result* out);
int vpl_odo_advance(vpl_odo* odo, const vpl_odo_frame* next, vpl_odo_result* out);

/* ---- keyframe session, IMU samples in: pre-integration, merge and propagation on the device -------------------------------- *
 * With the plain calls above the IMU side of processImage stays the caller's: a finished vpl_preintegration and a propagated
 * state per frame -- which needs the bias vpl_odo_solve has just estimated, i.e. a read-back, vpl_preintegrate_batch and a host
 * propagation between the two halves -- and after VPL_MARGIN_SECOND_NEW slot 9 keeps a pre-integration that ends one image early.
 * An IMU-enabled session takes the raw samples instead and does what the estimator does (estimator.cpp:82-117, 1766, 1786-1810):
 *   - the new interval is integrated on the device from the bias the solve has just left in slot 10 (IntegrationBase::push_back,
 *     the arithmetic of vpl_preintegrate_batch bit for bit) and becomes pre_integrations[10];
 *   - the new frame's pose and velocity are propagated on the device from the newest solved state (processIMU, :107-113);
 *   - on VPL_MARGIN_SECOND_NEW the samples slot 10 held are pushed onto pre_integrations[9] (:1786-1799), continuing it under
 *     its own linearisation bias, so that IMU factor (8, 9) spans the interval up to what is now frame 9.
 * vpl_odo_enable_imu: once per session (a second call: VPL_E_INVALID), max_samples >= 1 = the longest interval, in samples.
 * Allocates per sequence the sample buffer of slot 10 ([max_samples][7]) and its linearized_acc / _gyr through the context's
 * guarded allocator; the last measurement seen (the estimator's acc_0 / gyr_0) is the last row of that buffer.  From then on
 * vpl_odo_keyframe / vpl_odo_advance return VPL_E_INVALID (they would desynchronise the IMU book); vpl_odo_solve stays usable.
 * Without it the _imu calls and vpl_odo_set_imu return VPL_E_INVALID. */
int vpl_odo_enable_imu(vpl_odo* odo, int max_samples);
/* After vpl_odo_set_window: samples10 [n10][7] = (dt, ax, ay, az, gx, gy, gz), the samples of the interval that ends in frame 10
 * (dt_buf[10] and its two companions); acc0_10 / gyr0_10 [3] = linearized_acc / linearized_gyr of pre_integrations[10], the last
 * measurement before that interval (by the reference's construction the last sample of interval 9).  The session's last
 * measurement becomes samples10[n10 - 1].  Both are needed because the first image may be a non-keyframe.  n10 < 1:
 * VPL_E_INVALID; n10 > max_samples: VPL_E_CAPACITY.  vpl_odo_set_window on an IMU-enabled session invalidates the sequence's IMU
 * side until this is called again; an _imu call on such a sequence returns VPL_E_INVALID. */
int vpl_odo_set_imu(vpl_odo* odo, int seq, int n10, const double* samples10, const double* acc0_10, const double* gyr0_10);

typedef struct vpl_odo_imu_frame { /* one image of one sequence with the IMU samples since the previous image */
  int n_samples; const double* samples;                       /* [n][7]  dt, ax, ay, az, gx, gy, gz; acc_0 / gyr_0 of the
                                                                 interval are the last measurement the session has seen */
  int n_points; const int* point_id; const double* point_obs; /* as vpl_odo_frame */
  int n_lines;  const int* line_id;  const double* line_obs;
} vpl_odo_imu_frame;
typedef struct vpl_odo_imu_out {   /* per sequence */
  double pose[7], speed_bias[9];   /* the propagated state of the frame that entered slot 10 (what the reference publishes) */
  double sum_dt[2];                /* of pre_integrations[9] and [10] after the call */
} vpl_odo_imu_out;
/* vpl_odo_advance / vpl_odo_keyframe with samples (keyframe_imu = vpl_odo_solve, then advance_imu).  imu_out may be NULL.
 * Refusals as for the plain calls, checked before anything is written, and: NULL samples or n_samples < 1 (an empty interval has
 * zero covariance, which cannot be whitened): VPL_E_INVALID; n_samples > max_samples: VPL_E_CAPACITY.  A non-finite sample is not
 * refused: the next solve fails with termination 2. */
int vpl_odo_advance_imu(vpl_odo* odo, const vpl_odo_imu_frame* next, vpl_odo_result* out, vpl_odo_imu_out* imu_out);
int vpl_odo_keyframe_imu(vpl_odo* odo, const vpl_odo_imu_frame* next, const int* marginalization_flag, vpl_odo_result* out,
                         vpl_odo_imu_out* imu_out);
/* The 11 pre-integrations the session holds (any session), out[VPL_NFRAMES]; entry 0 is zeroed.  jacobian: columns 9..14 (the bias
 * columns, the only ones IMUFactor reads) as held, rows 9..14 of them the identity; columns 0..8 are NOT held by the session and
 * come back zero. */
int vpl_odo_get_preint(vpl_odo* odo, int seq, vpl_preintegration* out);

/* ---- keyframe session: the keyframe decision and the failure check ---------------------------------------------------------- *
 * The two per-image decisions of Estimator::processImage that the session's caller had to take from a feature manager of its own:
 *   - marginalization_flag = addFeatureCheckParallax(frame_count = WINDOW_SIZE, image) ? MARGIN_OLD : MARGIN_SECOND_NEW
 *     (estimator.cpp:126-129, feature_manager.cpp:106-189, compensatedParallax2 :958-996): needs every point track's observations in
 *     frames 8 and 9, which only the device holds;
 *   - failureDetection() (estimator.cpp:902-948, called at :225) on the states the solve returns.
 * vpl_odo_enable_keyframe_rule switches the first on for a session; a session without it behaves, and moves the bytes, it did
 * before.  With it, whenever an image enters slot 10 (vpl_odo_advance / _advance_imu behind the new frame, vpl_odo_set_window) the
 * device decides for the window as it then stands (k_odo_parallax, one more launch) and one record of
 * VPL_ODO_DECISION_RECORD_BYTES per sequence comes back in the synchronisation the call ends in -- in the IMU form in the same copy
 * as the propagated states: vpl_odo_stats' d2h_bytes grows by exactly n_seq * VPL_ODO_DECISION_RECORD_BYTES, the table bytes by
 * 3 ints per sequence + one int per qualifying track (the list the host's book writes, in the one host-to-device copy).
 *   qualifying track: start <= 8 && start + nobs - 1 >= 9 (a track that ends in frame 9 and is not in the new image included);
 *   its parallax: sqrt(du^2 + dv^2), du = x8 / z8 - x9, dv = y8 / z8 - y9 -- the frame-9 observation is NOT divided by its z, as in
 *     the reference; parallax_sum adds them in a fixed order, so a sequence's sum has the same bits wherever it sits in a session;
 *   last_track_num: observations of the new image that continued a track (ids that start a track or are ignored do not count);
 *   flag = VPL_MARGIN_OLD when last_track_num < min_track_num || parallax_num == 0 || parallax_sum / parallax_num >= min_parallax,
 *     else VPL_MARGIN_SECOND_NEW.  (The reference does not compute the sum when last_track_num is small; the record always holds it.)
 * Line tracks take no part.  The decision is advice: the explicit-flag calls keep working on such a session. */
typedef struct vpl_odo_keyframe_rule {
  double min_parallax; /* MIN_PARALLAX = keyframe_parallax / FOCAL_LENGTH (parameters.cpp:79-80) */
  int min_track_num;   /* 20 (feature_manager.cpp:166) */
} vpl_odo_keyframe_rule;
void vpl_odo_default_keyframe_rule(vpl_odo_keyframe_rule* rule); /* 10.0 / 460.0, 20 */
#define VPL_ODO_DECISION_RECORD_BYTES 24
/* Allowed whenever the session is not between vpl_odo_solve and vpl_odo_advance (VPL_E_INVALID there, and for a NULL or NaN
 * threshold).  Sequences that hold a window get their decision computed in this call.  A second call replaces the thresholds and
 * recomputes the decisions.  The first call replaces the session's inbox by one with room for the list (the context's guarded
 * allocator; the smaller one is freed in the same call). */
int vpl_odo_enable_keyframe_rule(vpl_odo* odo, const vpl_odo_keyframe_rule* rule);

#define VPL_FAIL_ACC_BIAS 1     /* |Ba| > max_acc_bias          (estimator.cpp:909) */
#define VPL_FAIL_GYR_BIAS 2     /* |Bg| > max_gyr_bias          (:914) */
#define VPL_FAIL_TRANSLATION 4  /* |P - last_P| > max_translation (:927) */
#define VPL_FAIL_Z 8            /* |P.z - last_P.z| > max_z     (:932) */
typedef struct vpl_failure_limits {
  double max_acc_bias, max_gyr_bias, max_translation, max_z; /* 2.5, 1.0, 5.0, 1.0; every comparison is a strict > */
} vpl_failure_limits;
void vpl_failure_default_limits(vpl_failure_limits* limits);
/* The four conditions under which Estimator::failureDetection returns true, as a bit mask (0: no failure); host only, no device,
 * no state.  speed_bias10 / pose10: frame WINDOW_SIZE after the solve; last_pose: last_P (only its position is read).  limits NULL:
 * the defaults.  A NULL state: VPL_E_INVALID.  The conditions the reference only logs (few tracks, a large rotation) are left out. */
int vpl_failure_detection(const vpl_failure_limits* limits, const double speed_bias10[9], const double pose10[7],
                          const double last_pose[7]);

typedef struct vpl_odo_decision { /* per sequence */
  int flag;              /* VPL_MARGIN_OLD / VPL_MARGIN_SECOND_NEW for the window as it stands */
  int last_track_num, parallax_num;
  int failure;           /* VPL_FAIL_* mask of the sequence's last vpl_odo_solve under the default limits; 0 before the first */
  double parallax_sum;
  double parallax_mean;  /* parallax_sum / parallax_num, 0 when parallax_num == 0 */
} vpl_odo_decision;
/* VPL_E_INVALID when the rule is off or the sequence has no window.  The session keeps last_P per sequence on the host:
 * vpl_odo_set_window stores pose[9] (Ps[9] equals last_P after either slide), every vpl_odo_solve compares with it and then stores
 * the result's pose[10].  The session does nothing else on a failure: the reference restarts the estimator, here the caller
 * decides (vpl_odo_set_window again).  Estimator::failure_occur / last_P0 / last_R0 stay unexposed: clearState() zeroes
 * failure_occur right after it is set (estimator.cpp:75, 228-229), so that gauge path never runs. */
int vpl_odo_get_decision(vpl_odo* odo, int seq, vpl_odo_decision* out);
/* vpl_odo_solve / vpl_odo_keyframe / vpl_odo_keyframe_imu with the stored decisions as marginalization_flag: thin wrappers that
 * build the flag array and call those.  The one-flag rule above holds for them too -- the batched solve marginalises one way per
 * batch -- so when the sequences' decisions disagree the call is refused with VPL_E_INVALID before anything is touched, and
 * vpl_last_error names how many sequences want each flag.  The caller can then pass explicit flags (solving the sequences of one
 * mind together, say); the stored decisions stay readable.  VPL_E_INVALID too when the rule is off or a sequence has no window. */
int vpl_odo_solve_auto(vpl_odo* odo, vpl_odo_result* out);
int vpl_odo_keyframe_auto(vpl_odo* odo, const vpl_odo_frame* next, vpl_odo_result* out);
int vpl_odo_keyframe_imu_auto(vpl_odo* odo, const vpl_odo_imu_frame* next, vpl_odo_result* out, vpl_odo_imu_out* imu_out);

/* What a caller may want to look at; none of it is needed to keep going.  Arrays may be NULL (not wanted); the track arrays
 * need room for max_*_tracks entries.  Tracks come in the feature manager's order. */
int vpl_odo_get_prior(vpl_odo* odo, int seq, vpl_prior* out);   /* n = 0: no prior yet */
/* the window's states as the store holds them: pose [11][7], speed_bias [11][9], ex_pose [7]; VPL_E_INVALID without a window */
int vpl_odo_get_states(vpl_odo* odo, int seq, double (*pose)[7], double (*speed_bias)[9], double* ex_pose);
int vpl_odo_get_tracks(vpl_odo* odo, int seq, int* n_points, int* point_id, int* point_start, int* point_nobs, double* inv_depth,
                       int* n_lines, int* line_id, int* line_start, int* line_nobs, int* line_triangulated, double* line_plk);
/* Host <-> device traffic of the last keyframe: the new frames' doubles | the integer tables (layout tables of the stages, track
 * index tables) | everything that came back.  d2h_bytes is exact: the read-backs are packed without padding
 * (VPL_ODO_D2H_PAD_BYTES of alignment padding). */
#define VPL_ODO_D2H_PAD_BYTES 0
int vpl_odo_stats(vpl_odo* odo, long long* h2d_payload_bytes, long long* h2d_table_bytes, long long* d2h_bytes);

/* ---- the feature selector of a session ----------------------------------- *
 * FeatureSelector::select (see "feature selector" above) for the next image of every sequence of a session, with what the
 * reference reads from the estimator taken from the session instead of the caller:
 *   - state k is slot 10 of the store as it stands (vpl_odo_get_states);
 *   - the cloud of initKDTree is gathered on the device (k_sel_cloud) from the resident point tracks with nobs >= 2,
 *     start < WINDOW_SIZE - 2, start <= 0.75 * WINDOW_SIZE that have taken part in a vpl_odo_solve (solve_flag == 1; a track whose
 *     depth came out <= 0 is erased by the advance that follows the solve): first observation / inv_depth, through the store's
 *     extrinsic and the pose of its start frame into the world, through state k + 1 and q_ic / t_ic of the params into the camera,
 *     normalised; depth = 1 / inv_depth.  A window that has not been solved since vpl_odo_set_window / vpl_odo_init has an empty
 *     cloud: every depth guess is 1.0;
 *   - the id book (lastFeatureId_, trackedFeatures_, firstImage_) is kept per sequence by the session, from its creation on;
 *     `initialized` is true once the sequence holds a window.  For a sequence without one only the book runs (the first image
 *     passes whole, then init_thresh applies) and no state is read.
 * To be called where an image may enter: not between vpl_odo_solve and vpl_odo_advance (VPL_E_INVALID).  The session's windows,
 * tracks, traffic counters (vpl_odo_stats) and launches are not touched; a session that never calls it is what it was.
 * One upload, four launches (k_sel_cloud, then the three of vpl_select_features_batch) and one read-back for the sequences that
 * hold a window; vpl_select_stats counts them.  Refusals, before any book moves: those of vpl_select_features_batch, an image of
 * more than VPL_SEL_MAX_FEATURES features or a cloud of more than VPL_SEL_MAX_FEATURES tracks (VPL_E_CAPACITY). */
typedef struct vpl_odo_sel_frame {
  double P1[3], Q1[4], V1[3], Ba1[3];   /* state k + 1: setNextStateFromImuPropagation (quaternion w, x, y, z) */
  double acc[3], gyr[3];                /* the last accelerometer sample, the unbiased gyroscope sample */
  double delta_imu;                     /* > 0 */
  int n_imu;                            /* >= 1 */
  const double* horizon;                /* NULL or [5][7], as in vpl_sel_input */
  int n_features;                       /* the image: every feature the front end reports */
  const int* id;                        /* [n_features]; an id given twice counts once (its first entry) */
  const double *x, *y, *prob;           /* [n_features] */
} vpl_odo_sel_frame;
typedef struct vpl_odo_sel_result {
  vpl_sel_result sel;                   /* zeros for a sequence without a window */
  int initialized;
  int n_new, n_used, kappa, n_cloud;    /* what the book and the filter handed to the selection */
  int n_out;                            /* ids in out_ids: what goes to the back end */
} vpl_odo_sel_result;
/* frames [n_seq], out [n_seq]; selected_id / round_f [n_seq][VPL_SEL_MAX_FEATURES] as in vpl_select_features_batch; out_ids
 * [n_seq][VPL_SEL_MAX_FEATURES]: the image handed to vpl_odo_advance* / vpl_odo_keyframe* -- the tracked ids that are present and
 * the selected ones, ascending. */
int vpl_odo_select(vpl_odo* odo, const vpl_sel_params* params, const vpl_odo_sel_frame* frames, vpl_odo_sel_result* out,
                   int* selected_id, double* round_f, int* out_ids);
/* wall clock of the stages of the last keyframe in ms: triangulations | onlyLineOpt | solve | slide + new frame */
int vpl_odo_debug_ms(vpl_odo* odo, double* ms4);

/* Host only, no device call (like vpl_ba_debug_point_units): the integer bookkeeping of ONE kind of tracks of ONE sequence
 * replayed from a script, by the code vpl_odo_keyframe runs.  Step s: flag[s] == VPL_MARGIN_NONE -- the window is still filling,
 * the frame enters the next free slot (VPL_E_INVALID once 11 frames are in); otherwise erase[s * max_tracks + i] != 0 erases
 * track i (standing in for the device's decisions), the slide of flag[s] runs on the rest and the frame enters slot 10
 * (VPL_E_INVALID before 11 frames are in).  ids: the frames' ids one after the other, n_ids[s] of step s.
 * Out, per step: status[s] = VPL_OK or VPL_E_CAPACITY (the step was refused by the rule of vpl_odo_keyframe, the table is
 * unchanged); n_slide[s] tracks entered the slide, slide[(s * max_tracks + i) * 3 ..] = their start, nobs (0: erased), dropped
 * observation (-1: none) as vpl_slide_tracks reports them; n_tracks[s] and table[(s * max_tracks + i) * 3 ..] = id, start, nobs
 * after the step; ignored[s]. */
int vpl_odo_debug_tracks(int max_tracks, int n_steps, const int* flag, const int* n_ids, const int* ids, const unsigned char* erase,
                         int* status, int* n_slide, int* slide, int* n_tracks, int* table, int* ignored);
/* The same replay (same arguments in, same refusals) for what the keyframe rule reads off the book: per step, once 11 frames are in
 * and the step was not refused, n_list[s] and list[s * max_tracks + i] = the qualifying tracks as the device is told them
 * (track | (8 - start) << 20, in the book's order) and last_track_num[s]; n_list[s] = -1 for a step while the window fills or a
 * refused one (last_track_num[s] = 0). */
int vpl_odo_debug_parallax_list(int max_tracks, int n_steps, const int* flag, const int* n_ids, const int* ids,
                                const unsigned char* erase, int* n_list, int* list, int* last_track_num);

/* ---- read-out of one window's linearisation and trust-region step (tests/test_gpu_step_kernels.py) ------------------------ *
 * Debug access to the buffers the step kernels read and write, for window `window` of the uploaded batch.  Both calls complete
 * whatever is enqueued on the context, wait for its stream, copy device buffers and launch nothing.  The window's full index
 * has n = 171 + n_points + 4 n_lines entries: the cam dims (frame f: pose 15 f + 0..5, speed/bias 15 f + 6..14; extrinsic
 * 165..170), the inverse depths in the window's track order, the orthonormal line parameters in fours -- of the lines that
 * travelled: device line l is the caller's line line_index[l] (untriangulated lines take no part in a solve).  Both return n,
 * or a VPL_E_* code.
 * vpl_ba_debug_linearization: H [n][n] (dense, symmetric: the packed camera Hessian, the landmark blocks and the compact W rows
 * expanded on the host) and g [n] of the last linearisation; the current states x_pose [11][7], x_speed_bias [11][9],
 * x_ex_pose [7], x_inv_depth [n_points], x_line_orth [n_lines][4] (world frame) and the cost at x.  With H or g NULL only the
 * counts and line_index (n_lines entries, may be NULL) are written: call it once to size the arrays.
 * vpl_ba_debug_step: jacobi scale, diagonal, scaled gradient and Gauss-Newton step of the last iteration ([n] each);
 * tr14 = radius, mu, alpha, a1 (|gradient|^2), a2 (|gn|^2), a3 (gradient . gn), model_cost_change, dogleg_step_norm, step_norm,
 * x_norm, iter, status, num_successful, step_valid (1 between the step kernel and k_cost, which clears it: 0 after a solve);
 * path (0: k_schur / k_chol / k_back, 1: k_solve for the whole solve,
 * 2: k_solve for this iteration) and the candidate states, shaped like x_*.  Any output pointer may be NULL. */
int vpl_ba_debug_linearization(vpl_ctx* ctx, int window, int* n_points, int* n_lines, int* line_index, double* H, double* g,
                               double* x_pose, double* x_speed_bias, double* x_ex_pose, double* x_inv_depth, double* x_line_orth,
                               double* x_cost);
int vpl_ba_debug_step(vpl_ctx* ctx, int window, double* scale, double* diag, double* grad, double* gn, double* tr14, int* path,
                      double* cand_pose, double* cand_speed_bias, double* cand_ex_pose, double* cand_inv_depth,
                      double* cand_line_orth);

/* ---- instrumentation (bench.py) ------------------------------------------ */
/* Per-kernel device time of the last solve measured with hipEvents on the
 * context's stream. names/ms arrays of length *count on input; count updated. */
int vpl_ba_enable_kernel_timing(vpl_ctx* ctx, int enable);
int vpl_ba_kernel_times(vpl_ctx* ctx, int* count, const char** names, double* total_ms, int* launches);
/* Per-launch profile of the last solve that ran with kernel timing enabled: kernel name, device time [ms] and the
 * number of windows that did work in that launch, active[i][4] = (linearised, new Gauss-Newton step, re-used step of a
 * rejected iteration, candidate evaluated).  Arrays of length *count on input; count updated. */
int vpl_ba_launch_profile(vpl_ctx* ctx, int* count, const char** names, double* ms, int* active);

/* ---- layout self-check (host only, no device call; tests/test_point_units.py) ---------------------------------- *
 * The point factors of a window are packed into work units whose Hessian tiles are committed in a host-assigned ticket
 * order (csrc/ba_pack.h).  vpl_ba_debug_point_units builds the tables exactly as vpl_ba_upload does:
 * lane_table [max_rounds][512][2], unit_table [max_rounds][32][8][2] (descriptor, seq | seq0 << 16).
 * vpl_ba_debug_point_chains replays the commit chains of the solve pass (marg_pass = 0) or of the MARGIN_OLD pass
 * (marg_pass = 1, first rounds0 rounds) wave by wave: 1 = every wave finishes, 0 = a wave would wait forever. */
int vpl_ba_debug_point_units(int n_points, const int* point_start, const int* point_nobs, int max_rounds,
                             int* lane_table, int* unit_table, int* rounds, int* rounds0);
int vpl_ba_debug_point_chains(const int* unit_table, int rounds, int rounds0, int marg_pass);

/* ------------------------------------------------------------------------------------------------------------
 * Loop verification: KeyFrame::findConnection from the PnP on (pose_graph/src/keyframe.cpp:406-516) for a batch of
 * (current keyframe, candidate) pairs, on the lists already reduced by the descriptor match (vpl_lc_match_batch of
 * vplines_frontend.h and the reduceVector calls behind it).  In the reference's order:
 *   1. count > min_loop_num, or nothing runs (stage VPL_LOOP_FEW_POINTS, has_loop 0, status all 0);
 *   2. PnPRANSAC (:200-256): cv::solvePnPRansac(pts3d, old_norm, K = I, no distortion, useExtrinsicGuess = true, max_iters,
 *      reproj_error, confidence) from the guess R_w_c^-1, -R_w_c^-1 T_w_c of the current camera (origin_vio_R qic,
 *      origin_vio_T + origin_vio_R tic); status = its inliers; PnP_R_old = R_pnp^T qic^T, PnP_T_old = -R_pnp^T t_pnp - PnP_R_old tic;
 *   3. the number of inliers > min_loop_num (else VPL_LOOP_FEW_INLIERS: pose and status stand, has_loop 0);
 *   4. relative_t = PnP_R_old^T (origin_vio_T - PnP_T_old), relative_q = Quaterniond(PnP_R_old^T origin_vio_R),
 *      relative_yaw = normalizeAngle(R2ypr(origin_vio_R).x - R2ypr(PnP_R_old).x) in degrees -> loop_info [8] = t, q (w x y z), yaw
 *      (written whenever step 4 is reached; the reference stores it only when the loop is accepted);
 *   5. has_loop = |relative_yaw| < max_yaw_deg and |relative_t| < max_t (else VPL_LOOP_REJECTED).
 * The RANSAC is stated as vpl_init_relative_pose_batch states its own -- OpenCV is not available to compare against:
 *   sample    five distinct indices (OpenCV's model_points for more than four points) from the integer stream of
 *             vpl_relpose_debug_plan with candidate 0 and the item's seed (csrc/loop_plan.h; vpl_loop_debug_plan hands it out);
 *   model     not OpenCV's minimal solver but the PnP of vpl_init_structure_batch (the Levenberg-Marquardt minimiser sfm_lm, the
 *             points constant, six free dims) on the five points, started from the extrinsic guess; a solve that ends in FAILURE
 *             yields no model;
 *   error     the squared reprojection distance in the normalised plane, compared in double with reproj_error^2 (<=);
 *   update    a model replaces the best only with strictly more inliers (and more than four); the iteration cap is then read
 *             from RANSACUpdateNumIters(confidence, (N - good) / N, 5, max_iters) and never rises;
 *   final     the same minimiser on all inliers of the best model, started from that model; status is the best model's mask;
 *             a final solve that ends in FAILURE is VPL_LOOP_NUMERIC (has_loop 0, the pose is not written);
 *   no model  when no sample yields one: VPL_LOOP_NO_MODEL, has_loop 0, status all 0.
 * The result is that of the sequential loop over the stream.  No max_solver_time; rotations travel as quaternions (mat2q), not
 * through cv::Rodrigues.  count <= VPL_LOOP_MAX_POINTS; n <= max_windows.
 * ------------------------------------------------------------------------------------------------------------ */
#define VPL_LOOP_MAX_POINTS 1024
#define VPL_LOOP_MAX_ITERS 1000       /* the largest max_iters accepted */
#define VPL_LOOP_FEW_POINTS 0
#define VPL_LOOP_NO_MODEL 1
#define VPL_LOOP_NUMERIC 2
#define VPL_LOOP_FEW_INLIERS 3
#define VPL_LOOP_REJECTED 4
#define VPL_LOOP_CLOSED 5
typedef struct vpl_loop_options {
  int min_loop_num;        /* MIN_LOOP_NUM = 25 */
  int max_iters;           /* 100 */
  double reproj_error;     /* 10.0 / 460.0 */
  double confidence;       /* 0.99 */
  double max_yaw_deg;      /* 30 */
  double max_t;            /* 20 */
} vpl_loop_options;
void vpl_loop_default_options(vpl_loop_options* opt);
typedef struct vpl_loop_input {
  int count;
  const float* pts3d;      /* [count][3] matched_3d, as cv::Point3f holds them */
  const float* old_norm;   /* [count][2] matched_2d_old_norm, as cv::Point2f holds them */
  double origin_vio_T[3], origin_vio_R[9], tic[3], qic[9];   /* matrices row-major */
  unsigned long long seed;
} vpl_loop_input;
typedef struct vpl_loop_result {
  int has_loop, stage;                 /* VPL_LOOP_* : where findConnection ended */
  int ransac_iterations, best_inliers; /* iterations the loop ran | inliers of the best model = entries set in status */
  int lm_iterations, lm_termination;   /* the final solve: ceres-style iteration count, vpl_solve_report's termination codes */
  double PnP_T_old[3], PnP_R_old[9], loop_info[8];
} vpl_loop_result;
/* in [n], out [n]; status [n][VPL_LOOP_MAX_POINTS] bytes, the first count entries of a row are written.  One copy each way, one
 * synchronisation.  VPL_E_INVALID: null pointers, a negative count, options out of range (max_iters outside 1 .. VPL_LOOP_MAX_ITERS,
 * min_loop_num < 4, reproj_error or confidence not in (0, ..)); VPL_E_CAPACITY: count > VPL_LOOP_MAX_POINTS, n > max_windows. */
int vpl_loop_verify_batch(vpl_ctx* ctx, int n, const vpl_loop_input* in, const vpl_loop_options* opt, vpl_loop_result* out,
                          unsigned char* status);
/* host only: samples [max_iters][5] of the stream for a list of n_points and niters_after [n_points + 1].
 * VPL_E_INVALID: n_points < 5, max_iters outside 1 .. VPL_LOOP_MAX_ITERS, a null array; VPL_E_CAPACITY: n_points > VPL_LOOP_MAX_POINTS */
int vpl_loop_debug_plan(unsigned long long seed, int n_points, double confidence, int max_iters, int* samples, int* niters_after);

/* ---- pose-graph optimisation: PoseGraph::optimize4DoF (pose_graph.cpp:403-579, functors pose_graph.h:89-250) for a batch of
 * independent graphs of one live sequence each.  Per graph the keyframes first_looped_index .. cur_index are the local nodes
 * 0 .. n-1; a node's parameters are its yaw in degrees and t, pitch and roll of R2ypr(qmat(mat2q(vio_R))) stay fixed, node 0 is
 * constant.  Edges: FourDOFError between i and i-j, j = 1..4 (no loss), measured on the incoming poses; FourDOFWeightError of
 * loop_info (t, and yaw / loop_yaw_scale) under HuberLoss(huber_delta) between a node and loop_local[node] < node.  Minimiser:
 * ceres' trust-region loop with the Levenberg-Marquardt strategy and Jacobi scaling (the rules of oracle/problem.cpp,
 * SolveWith<LevenbergMarquardt>), the normal equations solved directly in f64 by a block-banded Cholesky of the sequential part
 * and a capacitance system of the loop edges.  All max_iterations rounds are enqueued at once; nothing is read back
 * between them.  Then yaw_drift / r_drift / t_drift as at :549-557 from node n-1, and the tail poses r_drift P + t_drift,
 * r_drift R (:562-571).  A graph whose `sequence` values differ is not run (VPL_PG_UNSUPPORTED: a loaded map or a second session
 * gives a floating chain).  n = 1 comes back with zero iterations.  Limits VPL_PG_MAX_NODES / VPL_PG_MAX_LOOPS per graph. */
#define VPL_PG_MAX_NODES 4096
#define VPL_PG_MAX_LOOPS 256
#define VPL_PG_OK 0
#define VPL_PG_UNSUPPORTED 1
#define VPL_PG_NO_CONVERGENCE 0   /* termination, ceres' TerminationType as oracle/problem.h numbers it */
#define VPL_PG_CONVERGENCE 1
#define VPL_PG_FAILURE 2
typedef struct vpl_pg_options {
  int max_iterations;              /* options.max_num_iterations = 5 (pose_graph.cpp:437) */
  int max_consecutive_invalid_steps; /* 5 */
  double huber_delta;              /* HuberLoss(0.1); <= 0: no loss on the loop edges */
  double loop_yaw_scale;           /* 10: the loop edge's yaw residual is divided by it */
  double initial_radius, max_radius, min_radius;   /* 1e4, 1e16, 1e-32 */
  double min_relative_decrease;    /* 1e-3 */
  double function_tolerance, gradient_tolerance, parameter_tolerance; /* 1e-6, 1e-10, 1e-8 */
  double min_lm_diagonal, max_lm_diagonal;         /* 1e-6, 1e32 */
} vpl_pg_options;
void vpl_pg_default_options(vpl_pg_options* opt);
typedef struct vpl_pg_input {
  int n, n_tail;
  const double* vio_T;     /* [n][3] */
  const double* vio_R;     /* [n][9] row-major */
  const int* loop_local;   /* [n]: -1, or the local index of the old keyframe (< the node's own) */
  const double* loop_info; /* [n][8] = t, q, yaw as vpl_loop_result writes it; t and yaw are read, rows without a loop are not */
  const int* sequence;     /* NULL, or [n] */
  const double* tail_T;    /* NULL when n_tail = 0, or [n_tail][3]: later keyframes, only drift-corrected */
  const double* tail_R;    /* [n_tail][9] */
} vpl_pg_input;
typedef struct vpl_pg_result {
  int status, termination;   /* VPL_PG_OK / VPL_PG_UNSUPPORTED | VPL_PG_* termination */
  int iterations;            /* the number of the iteration the minimiser ended in */
  int successful_steps, unsuccessful_steps;   /* as ceres counts them: iteration 0 is a successful one */
  int reserved;
  double initial_cost, final_cost;
  double yaw_drift, r_drift[9], t_drift[3];
  double* T;                 /* caller's [n][3], written */
  double* R;                 /* caller's [n][9], written */
  double* tail_T;            /* caller's [n_tail][3] / [n_tail][9], written; may be NULL when n_tail = 0 */
  double* tail_R;
} vpl_pg_result;
/* in [n_graphs], out [n_graphs] with the four arrays of every out[] set by the caller.  One copy each way, one synchronisation.
 * VPL_E_INVALID: null arrays, n < 1, loop_local >= own index, options out of range; VPL_E_CAPACITY: n > VPL_PG_MAX_NODES, more
 * than VPL_PG_MAX_LOOPS loops, n_graphs > max_windows. */
int vpl_pg_optimize_batch(vpl_ctx* ctx, int n_graphs, const vpl_pg_input* in, const vpl_pg_options* opt, vpl_pg_result* out);
/* test access: the first linear solve of one graph.  g [4(n-1)] = J^T r in parameter units, step [4(n-1)] = the first trust-region
 * step in parameter units (Jacobi scale applied), model_cost_change [1]; the order of the unknowns is (yaw, tx, ty, tz) of node 1,
 * node 2, ...  Same refusals as the batch call; VPL_E_NUMERIC when the factorisation fails. */
int vpl_pg_debug_step(vpl_ctx* ctx, const vpl_pg_input* in, const vpl_pg_options* opt, double* g, double* step, double* model_cost_change);

/* ---- the same optimisation over several sequences: a graph that holds a loaded base map (sequence 0) or more than one run, as
 * pose_graph.cpp:447-519 builds it.  Same structs, same limits and refusals as vpl_pg_optimize_batch, which is unchanged; in
 * addition VPL_E_INVALID for a negative `sequence` value.  sequence == NULL: every node is of sequence 1.
 *   - A node is constant if it is local node 0 or its sequence is 0 (:473-477).
 *   - The sequential edge (i, i-j), j = 1..4, exists only if sequence[i] == sequence[i-j] (:482); it is measured on the incoming
 *     poses.  A loop edge may join two sequences.
 *   - An edge, sequential or loop, whose two ends are both constant is not part of the problem: it enters no cost, no gradient
 *     and no tolerance test.  ceres drops it from the reduced program too, but adds its fixed cost back into the costs it
 *     reports; this call does NOT, so initial_cost / final_cost are the minimiser's own.
 *   - A free node that no edge of the problem touches is not an unknown (ceres drops the unused parameter block).
 *   - x_norm, the step norm and the gradient maximum run over the free nodes.  A constant node comes back with its incoming T,
 *     bit for bit, and R = ypr2R(R2ypr(qmat(mat2q(vio_R)))), as a free node would with a zero step.
 *   - The drift is taken at node n-1 and applied to the tail, as in vpl_pg_optimize_batch.
 * On a graph whose sequences are all equal and non-zero the result is, byte for byte, that of vpl_pg_optimize_batch.  No
 * floating-point atomics, a fixed summation order: a call repeats bit for bit, wherever the graph stands in the batch. */
int vpl_pg_optimize_seq_batch(vpl_ctx* ctx, int n_graphs, const vpl_pg_input* in, const vpl_pg_options* opt, vpl_pg_result* out);
/* test access, as vpl_pg_debug_step, with `sequence` honoured: a constant node's entries of g and step are zero */
int vpl_pg_debug_step_seq(vpl_ctx* ctx, const vpl_pg_input* in, const vpl_pg_options* opt, double* g, double* step, double* model_cost_change);

/* ---- the pose-graph session: one PoseGraph with its keyframe list resident on the device -- per keyframe the shifted VIO pose,
 * the pose and loop_info; beside them w_r_vio / w_t_vio and the drift.  The host keeps the integers: the index, sequence_cnt,
 * sequence_loop, earliest_loop_index, the queue, every keyframe's sequence and loop.  Doubles cross the bus only when the caller
 * asks for them.  Several sessions may share a context; their device arrays go with the context, like those of vpl_gf_*, so a
 * session is destroyed before its context.  The caller keeps what findConnection needs (descriptors, points) and runs
 * vpl_ld_detect / vpl_loop_verify_batch first: they work on the original VIO pose, which the shift does not touch.
 * Not here: savePoseGraph / loadPoseGraph (file formats), the descriptors, visualisation, the 2 s sleep of the optimisation thread. */
#define VPL_PGS_MAX_KEYFRAMES 65536
#define VPL_PGS_OK 0
#define VPL_PGS_NOTHING 2          /* vpl_pgs_optimize: nothing was queued, nothing was launched or changed */
typedef struct vpl_pgs_session vpl_pgs_session;
typedef struct vpl_pgs_options {
  int max_keyframes;               /* 1 .. VPL_PGS_MAX_KEYFRAMES, default 8192 */
  int fast_relocalization;         /* FAST_RELOCALIZATION, default 0: vpl_pgs_update_loop overwrites the drift */
  vpl_pg_options pg;
} vpl_pgs_options;
typedef struct vpl_pgs_keyframe {
  int sequence;                    /* add: sequence_cnt or sequence_cnt + 1, >= 1; load: not read (the keyframe is of sequence 0) */
  int loop_index;                  /* -1, or the index of the old keyframe the caller's findConnection accepted */
  double vio_T[3], vio_R[9];       /* the VIO pose (row-major R) */
  double T[3], R[9];               /* load only: the stored pose */
  double loop_info[8];             /* t, q (w, x, y, z), yaw as vpl_loop_result writes it; read only when there is a loop */
} vpl_pgs_keyframe;
typedef struct vpl_pgs_keyframe_out {
  int index, optimize_pending;
  double vio_T[3], vio_R[9];       /* the shifted VIO pose */
  double T[3], R[9];               /* the drift-corrected pose */
  double w_r_vio[9], w_t_vio[3];
} vpl_pgs_keyframe_out;
typedef struct vpl_pgs_result {    /* a vpl_pg_result without the arrays */
  int status, termination;         /* VPL_PGS_OK / VPL_PGS_NOTHING | VPL_PG_* termination */
  int iterations, successful_steps, unsuccessful_steps;
  int n_nodes, first_index, cur_index;   /* the keyframes first_index .. cur_index were the nodes */
  double initial_cost, final_cost;
  double yaw_drift, r_drift[9], t_drift[3];
} vpl_pgs_result;
void vpl_pgs_default_options(vpl_pgs_options* opt);
/* VPL_E_INVALID: max_keyframes < 1, pose-graph options out of range; VPL_E_CAPACITY: max_keyframes > VPL_PGS_MAX_KEYFRAMES */
int vpl_pgs_create(vpl_ctx* ctx, const vpl_pgs_options* opt, vpl_pgs_session** out);
void vpl_pgs_destroy(vpl_pgs_session* h);
/* addKeyFrame (pose_graph.cpp:42-136) in one launch: the new-sequence rule (:47-57), the shift by w_r_vio / w_t_vio, the index; on
 * a loop earliest_loop_index and the queue, and -- when the loop ties the sequence to an older one for the first time -- w_r_vio /
 * w_t_vio from the old keyframe's VIO pose and the shift of the current and of every stored keyframe of the sequence (:85-124);
 * then the pose r_drift vio_P + t_drift, r_drift vio_R.  out may be NULL: then nothing is copied back and nothing waited for.
 * Refused, with the session unchanged -- VPL_E_INVALID: a sequence that is not sequence_cnt or sequence_cnt + 1 or is < 1, a
 * loop_index outside -1 .. index - 1; VPL_E_CAPACITY: keyframe max_keyframes + 1. */
int vpl_pgs_add_keyframe(vpl_pgs_session* h, const vpl_pgs_keyframe* kf, vpl_pgs_keyframe_out* out);
/* loadKeyFrame (:213-287): a keyframe of sequence 0, its VIO pose and pose as given -- no shift, no drift -- with the same loop
 * bookkeeping and queueing.  out->w_r_vio / w_t_vio are the session's, unchanged. */
int vpl_pgs_load_keyframe(vpl_pgs_session* h, const vpl_pgs_keyframe* kf, vpl_pgs_keyframe_out* out);
/* one turn of optimize4DoF's loop body (:407-573).  Nothing queued: status = VPL_PGS_NOTHING, no launch.  Otherwise the LAST queued
 * index is cur_index, earliest_loop_index is first_index, the queue is emptied; a kernel gathers the nodes and their loop
 * measurements from the list, the rounds of vpl_pg_optimize_seq_batch run on them (the result is that call's, byte for byte),
 * a kernel writes the poses back, takes the drift and applies it to every later keyframe in place.  One small upload (the
 * graph's integers), one copy back (the head), one synchronisation.  VPL_E_CAPACITY: more than VPL_PG_MAX_NODES nodes or
 * VPL_PG_MAX_LOOPS loops in the range; the queue and the list are then as they were. */
int vpl_pgs_optimize(vpl_pgs_session* h, vpl_pgs_result* result);
/* updateKeyFrameLoop (:889-922): behind KeyFrame::updateLoop's gate (|yaw| < 30, |t| < 20; *accepted says whether it held, may be
 * NULL) the keyframe's loop_info is replaced and, with fast_relocalization, the drift is overwritten from the old keyframe's
 * pose.  VPL_E_INVALID: no such keyframe, or one without a loop. */
int vpl_pgs_update_loop(vpl_pgs_session* h, int index, const double* loop_info, int* accepted);
/* the keyframes first .. first + count - 1: T [count][3], R [count][9], vio_T, vio_R, loop_info [count][8], sequence [count],
 * loop_index [count]; any pointer may be NULL.  One synchronisation if a double array is asked for. */
int vpl_pgs_get_path(vpl_pgs_session* h, int first, int count, double* T, double* R, double* vio_T, double* vio_R, double* loop_info,
                     int* sequence, int* loop_index);
int vpl_pgs_get_drift(vpl_pgs_session* h, double* yaw_drift, double* r_drift, double* t_drift);
int vpl_pgs_size(const vpl_pgs_session* h);   /* the number of keyframes */
int vpl_pgs_reset(vpl_pgs_session* h);        /* an empty PoseGraph again; the capacity and the options stay */

/* ---- global fusion: GlobalOptimization::optimize (globalOpt.cpp:101-259, functors Factors.h) for a batch of independent pose
 * chains.  Per chain the nodes 0 .. n-1 are the odometry poses in time order; a node's parameters are its quaternion (w, x, y, z;
 * ceres' QuaternionParameterization, tangent size 3: q <- [cos|d|, sin|d| / |d| d] (x) q) and t, no node is constant.  Edge
 * k -> k+1: RelativeRTError, measured on the local poses as iPj = R_i^T (p_j - p_i), iQj = mat2q(R_i^T R_j) with the project's
 * qmat / mat2q; rows (R(q_i)^T (t_j - t_i) - iPj) / t_var and 2 vec(iQj^-1 (x) q_i^-1 (x) q_j) / q_var, no loss.  GNSS factor of a
 * node: TError, (t - xyz) / accuracy under HuberLoss(huber_delta).  Minimiser: ceres' trust-region loop with the Levenberg-Marquardt
 * strategy and Jacobi scaling (the rules of oracle/problem.cpp, SolveWith<LevenbergMarquardt>).  The normal matrix is
 * block-tridiagonal with 6 x 6 blocks; it is solved directly in f64 by a substructured Cholesky: every `segment`-th node is a
 * separator, the segments between them are factored side by side, the Schur complement on the separators is again a chain
 * (csrc/gf_plan.h, DESIGN.md "Global fusion").  All max_iterations + 1 rounds are enqueued at once; nothing is read back between
 * them.  Then wgps_T_wvio = T_global(n-1) T_local(n-1)^-1, row-major 4 x 4.  Poses are [7] = p, q(w, x, y, z); the returned
 * quaternions are as Plus leaves them.  A chain with a non-finite input pose comes back with termination VPL_GF_FAILURE, its poses
 * as given and wgps_T_wvio the identity; its neighbours in the batch run. */
#define VPL_GF_MAX_NODES 65536
#define VPL_GF_OK 0
#define VPL_GF_NO_CONVERGENCE 0   /* termination, ceres' TerminationType as oracle/problem.h numbers it */
#define VPL_GF_CONVERGENCE 1
#define VPL_GF_FAILURE 2
typedef struct vpl_gf_options {
  int max_iterations;              /* options.max_num_iterations = 5 (globalOpt.cpp:116) */
  int max_consecutive_invalid_steps; /* 5 */
  int segment;                     /* S of the substructured solve: 0 = the default (64, the fastest of 32 / 64 / 128 at 16384
                                      nodes: DESIGN.md), otherwise >= 2; S > n: one segment, the serial chain */
  int reserved;
  double t_var, q_var;             /* 0.1, 0.01 (globalOpt.cpp:167) */
  double huber_delta;              /* HuberLoss(1.0); <= 0: no loss on the GNSS factors */
  double initial_radius, max_radius, min_radius;   /* 1e4, 1e16, 1e-32 */
  double min_relative_decrease;    /* 1e-3 */
  double function_tolerance, gradient_tolerance, parameter_tolerance; /* 1e-6, 1e-10, 1e-8 */
  double min_lm_diagonal, max_lm_diagonal;         /* 1e-6, 1e32 */
} vpl_gf_options;
void vpl_gf_default_options(vpl_gf_options* opt);
typedef struct vpl_gf_input {
  int n, n_gps;
  const double* local;        /* [n][7]: the odometry (VIO) poses */
  const double* global;       /* [n][7]: the initial global poses (globalPoseMap) */
  const int* gps_node;        /* [n_gps], strictly ascending, in 0 .. n-1; may be NULL when n_gps = 0, like the next two */
  const double* gps_xyz;      /* [n_gps][3] */
  const double* gps_accuracy; /* [n_gps], > 0 */
} vpl_gf_input;
typedef struct vpl_gf_result {
  int status, termination;   /* VPL_GF_OK | VPL_GF_* termination */
  int iterations;            /* the number of the iteration the minimiser ended in */
  int successful_steps, unsuccessful_steps;   /* as ceres counts them: iteration 0 is a successful one */
  int reserved;
  double initial_cost, final_cost;
  double wgps_T_wvio[16];
  double* pose;              /* caller's [n][7], written */
} vpl_gf_result;
/* in [n_chains], out [n_chains] with every out[].pose set by the caller.  One copy each way, one synchronisation.
 * VPL_E_INVALID: null arrays, n < 1, gps_node out of range or not ascending, an accuracy that is not positive, options out of
 * range, segment other than 0 or >= 2; VPL_E_CAPACITY: n > VPL_GF_MAX_NODES, n_chains > max_windows. */
int vpl_gf_optimize_batch(vpl_ctx* ctx, int n_chains, const vpl_gf_input* in, const vpl_gf_options* opt, vpl_gf_result* out);
/* test access: the first linear solve of one chain.  g [6 n] = J^T r in parameter units, step [6 n] = the first trust-region step in
 * parameter units (Jacobi scale applied), model_cost_change [1]; the order of the unknowns is (dtheta, dt) of node 0, node 1, ...
 * Same refusals as the batch call; VPL_E_NUMERIC when the factorisation fails. */
int vpl_gf_debug_step(vpl_ctx* ctx, const vpl_gf_input* in, const vpl_gf_options* opt, double* g, double* step, double* model_cost_change);
/* host only: the plan of (n, segment): n_sep [1] and sep_node [n / 2] (the first n_sep written), n_seg [1] and seg_bounds
 * [n / 2 + 1][2] (first and one past the last interior node of the first n_seg segments).  VPL_E_INVALID: null pointers, n < 1,
 * segment other than 0 or >= 2; VPL_E_CAPACITY: n > VPL_GF_MAX_NODES. */
int vpl_gf_debug_plan(int n, int segment, int* n_sep, int* sep_node, int* n_seg, int* seg_bounds);
/* host only, replaces GPS2XYZ: WGS84 geodetic (latitude, longitude in degrees, height in metres) -> ECEF -> east, north, up at the
 * origin (lat0, lon0, h0), in closed form in f64 (a = 6378137, f = 1 / 298.257223563).  lla [n][3] -> xyz [n][3].
 * VPL_E_INVALID: null arrays, n < 0. */
int vpl_gf_local_cartesian(double lat0, double lon0, double h0, int n, const double* lla, double* xyz);

/* The session: the GlobalOptimization object with the trajectory resident on the device.  It runs the batch call's kernels on its
 * own arrays (sized for max_nodes) and adds none.  The context must outlive it.
 *   vpl_gf_input_odom   inputOdom + getGlobalOdom: appends the local pose (t strictly increasing) and, on the host, the global pose
 *                       WGPS_T_WVIO makes of it -- q = mat2q(R qmat(q)), p = R p + t -- which it returns.
 *   vpl_gf_input_gps    inputGPS with the position already local (vpl_gf_local_cartesian): a fix of the node whose time is t, in
 *                       place of an earlier one; a t that no node has is stored and never used.
 *   vpl_gf_optimize     uploads the poses and fixes that came since the last call (and one chain descriptor), runs the solve, and
 *                       reads back the result head alone (result->pose is not touched); the global poses of every node and
 *                       WGPS_T_WVIO are the solved ones from then on.  Equal, byte for byte, to vpl_gf_optimize_batch on the
 *                       same local poses, fixes, and global poses carried forward.
 *   vpl_gf_get_path     global poses [count][7] of the nodes first .. first + count - 1.
 * VPL_E_INVALID: null pointers, a time that does not increase, a non-finite pose or fix, an accuracy that is not positive, no node
 * yet, a path range beyond the last node, options out of range; VPL_E_CAPACITY: max_nodes > VPL_GF_MAX_NODES, a node beyond
 * max_nodes. */
typedef struct vpl_gf_session vpl_gf_session;
int vpl_gf_create(vpl_ctx* ctx, int max_nodes, vpl_gf_session** out);
void vpl_gf_destroy(vpl_gf_session* h);
int vpl_gf_input_odom(vpl_gf_session* h, double t, const double* p, const double* q, double* out_p, double* out_q);
int vpl_gf_input_gps(vpl_gf_session* h, double t, const double* xyz, double accuracy);
int vpl_gf_optimize(vpl_gf_session* h, const vpl_gf_options* opt, vpl_gf_result* result);
int vpl_gf_get_path(vpl_gf_session* h, int first, int count, double* out);

#ifdef __cplusplus
}
#endif
#endif /* VPLINES_BA_H */
