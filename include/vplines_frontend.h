/*
 * vplines_frontend.h -- C ABI of the MI355X-native line front-end (EDLines extractor + KLT line matcher).
 *
 * Drop-in boundary for the line detector of multiplefish/VPLines-SLAM:
 *   int EDLineDetector::EDline(cv::Mat& image, std::vector<Line>& lines, bool smoothed)
 *        line_matching/src/edline_detector.h:82-84, edline_detector.cpp:1176-1198
 * as it is called by LineFeatureTracker::readImage (feature_tracker/src/line_feature_tracker.cpp:87)
 * with smoothed = true on 8-bit single-channel, undistorted + CLAHE'd frames.  Images arrive as raw
 * row-major uint8 buffers (cv::Mat::data of a continuous CV_8UC1 matrix); lines leave in the numeric
 * layout of struct Line (line_matching/src/line.h:8-17).
 *
 * smoothed = false -- the reference's default (edline_detector.h:79-81) and the path of its two demo programs -- runs
 * cv::GaussianBlur(image, Size(ksize, ksize), sigma) first (edline_detector.cpp:82-84): vpl_edlines_detect_ex.
 * Functions return 0 or a negative VPL_E_* code (same codes as vplines_ba.h); nothing falls back to a CPU path.
 */
#ifndef VPLINES_FRONTEND_H
#define VPLINES_FRONTEND_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* EDLineParam, edline_detector.h:33-41 (ksize / sigma: the Gaussian pre-blur of smoothed = false; unused with smoothed = true) */
typedef struct vpl_edline_param {
  int ksize;
  float sigma;
  float gradientThreshold;   /* production: 30 (line_feature_tracker_node.cpp:203) */
  float anchorThreshold;     /* 5 */
  int scanIntervals;         /* 2 */
  int minLineLen;            /* min_line_length = 35 */
  double lineFitErrThreshold;/* line_fit_err = 1.8 */
} vpl_edline_param;

/* numeric part of struct Line (line.h:8-17) */
typedef struct vpl_line {
  float line_endpoint[4];    /* x1,y1,x2,y2 */
  double line_equation[3];   /* w1 x + w2 y + w3 = 0, w1^2 + w2^2 = 1 */
  float center[2];
  float length;
} vpl_line;

typedef struct vpl_fe_ctx vpl_fe_ctx;   /* opaque: device buffers for a batch of frames of one size */

void vpl_edline_default_param(vpl_edline_param* p);   /* {5, 1, 30, 5, 2, 35, 1.8} */

/* width, height >= 7 (the smallest frame with a FAST candidate, vpl_lc_keyframe_batch); the line detector takes frames from 8 x 8 */
int vpl_fe_create(vpl_fe_ctx** out, int device, int max_images, int width, int height, int max_lines_per_image);
void vpl_fe_destroy(vpl_fe_ctx* ctx);
int vpl_fe_set_stream(vpl_fe_ctx* ctx, void* hip_stream);   /* (work in flight on the stream used so far is completed first) */
int vpl_fe_synchronize(vpl_fe_ctx* ctx);
const char* vpl_fe_last_error(const vpl_fe_ctx* ctx);

/* ---- image preparation of LineFeatureTracker::readImage (feature_tracker/src/line_feature_tracker.cpp:62-68) ----
 *   cv::remap(_img, img, undist_map1_, undist_map2_, CV_INTER_LINEAR);  createCLAHE(3.0, Size(8,8))->apply(img, img);
 * vpl_pre_set_maps: the CV_32FC1 maps of PinholeCamera::initUndistortRectifyMap (line_feature_tracker.cpp:32), [H][W]
 *   each; NULL, NULL = no remap.  vpl_pre_upload: raw 8-bit frames [n][H][W].  vpl_pre_run (asynchronous): remap
 *   (INTER_LINEAR, BORDER_CONSTANT 0), then CLAHE when `equalize` (reference: clip 3.0, 8 x 8 tiles); the result
 *   REPLACES the frame batch that vpl_edlines_detect / vpl_match_run work on, so the raw frames never come back to the
 *   host.  vpl_pre_download copies the prepared frames out (tests, display). */
int vpl_pre_set_maps(vpl_fe_ctx* ctx, const float* map_x, const float* map_y);
int vpl_pre_upload(vpl_fe_ctx* ctx, int n_images, const uint8_t* raw_images);
int vpl_pre_run(vpl_fe_ctx* ctx, int equalize, double clip_limit, int tiles_x, int tiles_y);
int vpl_pre_download(vpl_fe_ctx* ctx, int n_images, uint8_t* images);
/* upload + run + (images != NULL ? download : synchronize) */
int vpl_pre_batch(vpl_fe_ctx* ctx, int n_images, const uint8_t* raw_images, int equalize, double clip_limit, int tiles_x,
                  int tiles_y, uint8_t* images);

/* instrumentation (bench.py): device time of every kernel launch of vpl_edlines_detect / vpl_match_run since timing was
 * enabled, measured with hipEvents on the context's stream, in launch order.  Arrays of length *count on input. */
int vpl_fe_enable_kernel_timing(vpl_fe_ctx* ctx, int enable);
int vpl_fe_kernel_times(vpl_fe_ctx* ctx, int* count, const char** names, double* ms);

/* three-phase form (inputs resident in HBM while timing) */
int vpl_edlines_upload(vpl_fe_ctx* ctx, int n_images, const uint8_t* images /* [n][H][W] */);
int vpl_edlines_detect(vpl_fe_ctx* ctx, const vpl_edline_param* param);   /* enqueue; asynchronous */
/* The reference collects lines in a std::vector; here a frame holds max_lines_per_image of them (vpl_fe_create).  A frame in
 * which the detector found more is refused: VPL_E_CAPACITY with the frame and its count in vpl_fe_last_error -- from this call
 * and from vpl_match_download when the match took its lines from the detector (vpl_match_from_detected); `lines` / `counts`
 * are written all the same (the lines that arrived first, in no defined selection). */
int vpl_edlines_download(vpl_fe_ctx* ctx, int n_images, vpl_line* lines /* [n][max_lines] */, int* counts /* [n] */);

/* EDline(image, lines, smoothed) with the flag as an argument.  smoothed == 0: the Gaussian pre-blur of EdgeDrawing
 * (edline_detector.cpp:82-84) runs first, fused with the gradient stage -- OpenCV's bit-exact 8-bit GaussianBlur: taps in 8.8
 * fixed point, rows then columns, BORDER_REFLECT_101.  ksize must be odd and <= 7 (ksize <= 0 with sigma > 0: OpenCV's automatic
 * size); frames of at least 8 x 8.
 * OpenCV published two roundings of the taps; vpl_fe_set_blur_kernel selects one per context:
 *   VPL_BLUR_NORMALISED (default): 3.4.9+ / 4.2+, taps sum to 256 (5, sigma 1: 14 62 104 62 14) -- the one that reproduces the
 *                                  reference's own output line_matching/data/edline_result.png (tests/golden/README.md);
 *   VPL_BLUR_OPENCV_341:           3.4.1 - 3.4.8 / 4.0 - 4.1, cvRound(256 g_i) (14 63 103 63 14; the README's 3.4.2). */
#define VPL_BLUR_NORMALISED 0
#define VPL_BLUR_OPENCV_341 1
int vpl_fe_set_blur_kernel(vpl_fe_ctx* ctx, int mode);
int vpl_edlines_detect_ex(vpl_fe_ctx* ctx, const vpl_edline_param* param, int smoothed);   /* enqueue; asynchronous */
int vpl_edlines_detect_batch_ex(vpl_fe_ctx* ctx, int n_images, const uint8_t* images, const vpl_edline_param* param, int smoothed,
                                vpl_line* lines, int* counts);
/* test access: keep a copy of the blurred frames of smoothed == 0 detections (off by default: the blurred frame otherwise
 * never leaves the work-group's LDS) and read one back */
int vpl_fe_keep_blurred(vpl_fe_ctx* ctx, int enable);
int vpl_edlines_debug_blurred(vpl_fe_ctx* ctx, int img, uint8_t* blurred /* [H*W] */);

/* EDline(image, lines, smoothed=true) for a batch: upload + detect + synchronize + download.
 * Lines of one image are returned in edge-chain order (the reference's order is the nondeterministic
 * arrival order of its worker threads, edline_detector.cpp:1080-1084). */
int vpl_edlines_detect_batch(vpl_fe_ctx* ctx, int n_images, const uint8_t* images, const vpl_edline_param* param,
                             vpl_line* lines, int* counts);

/* LineMatching::LineFilter(lines, distance_threshold, parallel_threshold = sin 3 deg) (line_matching.h:35-37,
 * line_matching.cpp:167-264; the reference's demo calls it between detector and matcher, test_line_matching.cpp:57,74): in
 * order of decreasing length, a line removes every shorter one that is nearly parallel to it and has an end point closer than
 * distance_threshold.  Lines of equal length are taken in index order (the reference's std::sort leaves their order open).
 * _detected: on the lines of the last detect where they lie in HBM (asynchronous; vpl_edlines_download / vpl_match_from_detected
 * then see the filtered lists).  _batch: caller-owned lists [n][max_lines], counts [n], both in / out (uses the context's
 * line table: the last detect's lines are overwritten).  max_lines_per_image <= 8192. */
#define VPL_LINE_FILTER_PARALLEL_DEFAULT 0.0348994967f
int vpl_line_filter_detected(vpl_fe_ctx* ctx, float distance_threshold, float parallel_threshold);
int vpl_line_filter_batch(vpl_fe_ctx* ctx, int n_images, vpl_line* lines, int* counts, float distance_threshold,
                          float parallel_threshold);

/* test access to the intermediate stages of image `img` of the last detect (any pointer may be NULL):
 * dx, dy, gImg [H*W int16]; dirImg [H*W uint8]; anchors [2*cap uint32 x,y] ; chains xC,yC [cap uint32], sId [cap/20+2] */
int vpl_edlines_debug_stage(vpl_fe_ctx* ctx, int img, int16_t* dx, int16_t* dy, int16_t* gImg, uint8_t* dirImg,
                            uint32_t* anchors, int* n_anchors, uint32_t* chain_x, uint32_t* chain_y, uint32_t* sId,
                            int* n_edges);
/* routing counters of image `img` of the last detect: steps walked, LDS tile loads, walks started, shader cycles */
int vpl_edlines_debug_route_stats(vpl_fe_ctx* ctx, int img, unsigned long long* out4);

/* ------------------------------------------------------------------------------------------------------------
 * KLT line matching.  Drop-in boundary:
 *   bool LineMatching::Matching(img_ref, img_cur, lines_ref, lines_cur, line_ref_to_line_cur, K_ref, K_cur, T_cur_ref,
 *                               illumination_adapt, topological_filter, ...)
 *        line_matching/src/line_matching.h:21-33, line_matching.cpp:605-690
 * as called by LineFeatureTracker::match_line_match (feature_tracker/src/line_feature_tracker.cpp:291-314) with
 * K_ref = K_cur = T_cur_ref = NULL, illumination_adapt = true, topological_filter = true.  The KLT inside is
 * KLT::calc2D (klt.cpp:491-628) with a 13x13 window, 4 pyramid levels, 30 iterations / eps 0.001, minEig 1e-4.
 * Images are the frames uploaded with vpl_edlines_upload (a pair names two of them by index); lines are passed by the
 * caller, as in the reference (they may have been filtered on the host after detection).
 * ------------------------------------------------------------------------------------------------------------ */

/* LineMatching ctor arguments (line_matching.h:14-18), the two Matching() flags, TopologicalFilter defaults (:45-47) */
typedef struct vpl_match_param {
  int step;                          /* 10 */
  float closest_line_threshold;      /* 0.5 */
  float line_matching_ratio;         /* 0.4 */
  float line_distance_error_ratio;   /* 3 */
  float klt_error_threshold;         /* 40 */
  int illumination_adapt;            /* 1 in the tracker */
  int topological_filter;            /* 1 in the tracker */
  float topo_distance_threshold;     /* 15 */
  float topo_length_tolerate_ratio;  /* 0.2 */
  float topo_violation_ratio;        /* 0.05 */
} vpl_match_param;

void vpl_match_default_param(vpl_match_param* p);

/* device buffers for up to max_pairs pairs, max_kps key points per pair (Anchors() output, ~ sum(len/step + 2)) */
int vpl_match_reserve(vpl_fe_ctx* ctx, int max_pairs, int max_kps);

/* three-phase form.  lines_ref / lines_cur: [n_pairs][max_lines_per_image] (the stride given to vpl_fe_create). */
int vpl_match_upload(vpl_fe_ctx* ctx, int n_pairs, const int* ref_image, const int* cur_image,
                     const vpl_line* lines_ref, const int* n_ref, const vpl_line* lines_cur, const int* n_cur);
/* The lines of this context's last vpl_edlines_detect as the matcher's input, device to device: what
 * LineFeatureTracker::readImage does between detector and matcher (line_feature_tracker.cpp:110-118, :290-322) without the lines
 * leaving HBM.  At most max_lines lines per frame take part (the first ones in the detector's order).  Asynchronous.
 * vpl_match_counts: how many lines of each pair's frames take part (sizes of the rows vpl_match_download fills). */
int vpl_match_from_detected(vpl_fe_ctx* ctx, int n_pairs, const int* ref_image, const int* cur_image, int max_lines);
int vpl_match_counts(vpl_fe_ctx* ctx, int n_pairs, int* n_ref, int* n_cur);
int vpl_match_run(vpl_fe_ctx* ctx, const vpl_match_param* param);   /* enqueue; asynchronous */
/* line_ref_to_line_cur [n_pairs][max_lines] (-1 = unmatched; rows of pairs with matched == 0 are left untouched, as
 * Matching() leaves its output vector when it returns false); matched [n_pairs] = Matching()'s return value.
 * VPL_E_CAPACITY if a pair produced more key points than max_kps. */
int vpl_match_download(vpl_fe_ctx* ctx, int n_pairs, int* line_ref_to_line_cur, int* matched);

/* Matching() for a batch of pairs: images [n_images][H][W] are uploaded, then upload + run + synchronize + download */
int vpl_line_match_batch(vpl_fe_ctx* ctx, int n_images, const uint8_t* images, int n_pairs, const int* ref_image,
                         const int* cur_image, const vpl_line* lines_ref, const int* n_ref, const vpl_line* lines_cur,
                         const int* n_cur, const vpl_match_param* param, int* line_ref_to_line_cur, int* matched);

/* test access (any pointer may be NULL): key points of pair `pair` of the last run (LineMatching::getPointMatchResult,
 * line_matching.h:60-65): kps_ref, kps_cur [2*n_kps], status, err, kp2line_cur [n_kps] */
int vpl_match_debug_kps(vpl_fe_ctx* ctx, int pair, int cap, float* kps_ref, float* kps_cur, uint8_t* status, float* err,
                        int* kp2line_cur, int* n_kps);
/* pyramid level `level` of image `img` without its border: pixels [h*w], derivative [h*w*2]; *w, *h; returns
 * VPL_E_INVALID for a level that was not built */
int vpl_match_debug_level(vpl_fe_ctx* ctx, int img, int level, uint8_t* pixels, int16_t* deriv, int* w, int* h);

/* ---- vanishing points: vanishing_point_detection::run_vanishing_point_detection
 * (feature_tracker/src/vanishing_point_detection.cpp:37-66, called at line_feature_tracker.cpp:237-266) for a batch of frames.
 *   hyp_lines [n][max_lines]  the lines the 2-line hypotheses and the sphere grid are built from (`lines`: verticalLine or
 *                             all lines, :240-243);  all_lines [n][max_lines]  the lines that are classified
 *   f, cx, cy                 init(K(0,0), K(0,2), K(1,2), 0.5) (line_feature_tracker.cpp:33)
 *   seeds [n]                 the reference calls srand(time(NULL)) in every frame (:107); here the caller supplies the
 *                             seed and the device generates glibc's rand() stream for it
 *   first_frame [n]           frame_count == 0 (no vps[1]/vps[2] swap, :318-339)
 *   vps [n][3][3]             the three unit vectors;  vp_ids [n][max_lines]  per line 0..2 = its VP, 3 = none
 *   status [n]                0, or -1 when no hypothesis can be drawn (fewer than two lines, or only parallel ones -- the
 *                             reference does not return in that case); vps are 0 and every id is 3 then
 * Defined where the reference is not: a query index past the end of lx (:411-416, :428-431) means "no query line".
 * Synchronous. */
int vpl_vp_detect_batch(vpl_fe_ctx* ctx, int n_frames, const vpl_line* hyp_lines, const int* n_hyp, const vpl_line* all_lines,
                        const int* n_all, float f, float cx, float cy, const uint32_t* seeds, const int* first_frame,
                        double* vps, int* vp_ids, int* status);
/* test access after vpl_vp_detect_batch (any pointer may be NULL): smoothed sphere grid [90][360], the drawn line pairs
 * [105][2], index of the winning hypothesis, rand() calls made by the hypothesis stage */
int vpl_vp_debug(vpl_fe_ctx* ctx, int frame, double* grid, int* pairs, int* best_idx, int* drawn);

/* ---- list handling of LineFeatureTracker::readImage after the match (line_feature_tracker.cpp:96-229) ----
 * Host-side integer bookkeeping (no device work, no context): id propagation from the previous frame's lines through
 * line_ref_to_line_cur, fresh ids for the unmatched lines, and the max_h_lines / max_v_lines quota.  The reference's
 * behaviour is kept as written: a match to detection 0 is ignored (`mt > 0`, :121); t_cnt is read with the NEW frame's
 * index (:123) from a vector that keeps the previous frame's detection count (n_tcnt_prev; a read past its end, which
 * the reference leaves undefined, counts as 0); new lines are classed with the 3.14-based angle test of :166.
 *   ends_new   [n_new][4]  end points of the new frame's detections
 *   id_prev    [n_prev]    lineID of the previous frame's (kept) lines;  prev_to_new [n_prev] their match, -1 = none
 *   keep, id_out (capacity n_new): the new frame's kept lines as indices into the detections and their ids;
 *   tcnt_out   [n_new]     t_cnt in detection order.  *allfeature_cnt is advanced by the number of fresh ids.
 *   vertical_new (capacity n_new), n_vertical_new: may be NULL; the reference's `verticalLine` (:151-176), i.e. every
 *              new line of the v class whether the quota keeps it or not (the test on tracked lines at :151 is never true)
 * Returns the number of kept lines, or a negative VPL_E_* code. */
int vpl_line_track_ids(int n_new, const float* ends_new, int n_prev, const int* id_prev, const int* tcnt_prev, int n_tcnt_prev,
                       const int* prev_to_new, int max_h_lines, int max_v_lines, int* allfeature_cnt, int* keep, int* id_out,
                       int* tcnt_out, int* vertical_new, int* n_vertical_new);

/* ------------------------------------------------------------------------------------------------------------
 * Point front-end, detection.  Drop-in boundary:
 *   cvmodified::goodFeaturesToTrack(image, corners, scores, maxCorners, 0.01, minDistance, mask)
 *        feature_tracker/src/cvmodified/cvmodified.cpp:38-216, blockSize 3, gradientSize 3, no Harris
 * as FeatureTracker::detect_features calls it, for a batch of frames: the cornerMinEigenVal plane, its maximum under the mask,
 * THRESH_TOZERO at 0.01 max, the 3 x 3 local-maximum test inside the mask, the descending sort (equal scores: the higher
 * linear pixel index first, greaterThanPtr :16-21) and the greedy min-distance selection until max_corners are kept.
 * vpl_pt_reserve (once per context) fixes the capacity of a frame's candidate list (<= 16384), the row length
 * max_corners of the detector's outputs (<= 2048) and the row length max_points of a tracked point list (<= 1024).  A frame
 * with more candidates than the list holds is refused -- VPL_E_CAPACITY for the call, the frame and its count in
 * vpl_fe_last_error, no output written -- never cut short.
 *   images      [n][H][W], or NULL: the n frames that lie in the context's image slots (after vpl_edlines_upload / vpl_pre_run)
 *   masks       [n][H][W] 8-bit planes, non-zero = allowed (NULL: no frame has one); use_mask [n] (NULL: every frame uses its plane)
 *   max_corners [n] in 1 .. the reserved max_corners;  min_distance [n] >= 0 (below 1: no suppression)
 *   corners     [n][max_corners][2] integer pixel positions (x, y) as float, in the order kept;  scores [n][max_corners] the
 *               min-eigenvalue of each;  counts [n].  Rows past counts[i] are left as they were.
 * Two host-to-device copies (frames, parameters; a third for the masks), one copy back, one synchronisation.  The float
 * arithmetic OpenCV leaves to its build (Sobel scale and tap order, the box sum) is stated in csrc/pt_kernels.h.
 * vpl_pt_debug_detect: test access to frame `img` of the last call (any pointer may be NULL): the plane [H*W], the number
 * of candidates found.
 * ------------------------------------------------------------------------------------------------------------ */
int vpl_pt_reserve(vpl_fe_ctx* ctx, int max_candidates, int max_corners, int max_points);
int vpl_pt_detect_batch(vpl_fe_ctx* ctx, int n_images, const uint8_t* images, const uint8_t* masks, const int* use_mask,
                        const int* max_corners, const double* min_distance, float* corners, float* scores, int* counts);
int vpl_pt_debug_detect(vpl_fe_ctx* ctx, int img, float* eig, int* n_candidates);

/* cv::calcOpticalFlowPyrLK(prev, next, pts, next_pts, status, err, Size(21, 21), 3) with OpenCV's defaults (30 iterations or a
 * step of 0.01, minEigThreshold 1e-4, no initial flow) as FeatureTracker::readImage calls it (feature_tracker.cpp:139), for a
 * batch of image pairs.  The images are those in the context's slots (vpl_edlines_upload, or the result of vpl_pre_run); a
 * pair names two of them.  Pyramid levels are halved until four stand or the next would be no larger than the window; the
 * window I, dIx, dIy in 16-bit fixed point from W_BITS = 14 weights; the level-0 min-eigenvalue test and the out-of-image
 * tests clear status.  err is not produced.  The float sums over the window run row by row: each row left to right, the 21
 * row sums top to bottom (csrc/pt_kernels.h); OpenCV's own order depends on its SIMD build.
 *   prev_image, next_image [n];  prev_pts [n][max_points][2];  counts [n] (0 is allowed)
 *   next_pts [n][max_points][2], status [n][max_points]: the first counts[i] entries of a row are written
 * Frames must be larger than 21 x 21; n_pairs <= max_images.  One copy each way, one synchronisation. */
int vpl_pt_flow_batch(vpl_fe_ctx* ctx, int n_pairs, const int* prev_image, const int* next_image, const float* prev_pts,
                      const int* counts, float* next_pts, uint8_t* status);

/* FeatureTracker::rejectWithF (feature_tracker/src/feature_tracker.cpp:226-261) for a batch of point lists: both lists are
 * lifted through the camera model (PinholeCamera::liftProjective with k1, k2, p1, p2: the recursive distortion removal, 8
 * steps), re-projected to focal_length x / z + COL / 2, focal_length y / z + ROW / 2 (COL, ROW: the context's frame size) and
 * rounded to float; cv::findFundamentalMat(FM_RANSAC, f_threshold, 0.99) decides.  The estimator is the one of
 * vpl_init_relative_pose_batch (vplines_ba.h: the 7-point solver, the symmetric epipolar error, RANSACUpdateNumIters, the
 * integer sample stream of vpl_relpose_debug_plan with candidate 0 and the caller's seed), its deviations included.
 *   cur_pts, forw_pts [n][max_points][2] pixel positions;  counts [n];  seeds [n]
 *   status [n][max_points]: 1 = kept; the first counts[i] entries of a row are written.  A list of fewer than 8 points passes
 *   unchanged (all 1).  A list for which no sample yields a model -- where the reference reads a mask OpenCV did not write --
 *   loses every point (all 0).
 * One copy each way, one synchronisation. */
typedef struct vpl_pt_camera {
  double fx, fy, cx, cy;
  double k1, k2, p1, p2;
} vpl_pt_camera;
int vpl_pt_reject_f_batch(vpl_fe_ctx* ctx, int n_lists, const float* cur_pts, const float* forw_pts, const int* counts,
                          const vpl_pt_camera* cam, double focal_length, double f_threshold, const unsigned long long* seeds,
                          uint8_t* status);

/* ------------------------------------------------------------------------------------------------------------
 * Tracker session: LineFeatureTracker::readImage (line_feature_tracker.cpp:57-286) and the wire format of
 * line_feature_tracker_node.cpp:77-153 for n_seq independent cameras or sequences, one call per image.  What survives
 * from frame to frame -- the prepared image of the last frame taken over, its kept lines, ids, t_cnt, allfeature_cnt
 * and the VP stage's frame counter -- lives in HBM.  vpl_trk_frame copies the raw frames and one VP seed per sequence
 * down, the observations and one result per sequence back (one copy each way), and synchronises once, at the end.
 * The semantics are those of the host mirror vplhost::LineFeatureTracker (vplines-slam_amd/host/vpl_frontend.hpp),
 * quirks included:
 *   - first image of a sequence: every detected line is kept, in the detector's order, with fresh ids; t_cnt 0; no
 *     match, no quota, no VP stage; the VP part of every observation is 0;
 *   - a frame without a detected line: lines_exist = 0, no rows; it is NOT taken over (the next frame is matched
 *     against the last frame that had lines);
 *   - a FIRST frame without lines followed by a frame with lines: as in the mirror, the second frame is no "first
 *     image" any more and there is nothing to match against, so all its lines are kept with id -1, t_cnt 0, no VP stage,
 *     and allfeature_cnt is untouched; the frame after it matches against those lines, and because vpl_line_track_ids
 *     reads an inherited id of -1 as "no id", every line then gets a fresh id (its t_cnt still counts up);
 *   - otherwise: Matching() against the kept lines of the last frame taken over, then vpl_line_track_ids as written
 *     (see above), then the VP stage when more than two lines are kept: hypotheses from verticalLine when it has more
 *     than two entries, else from the kept lines; first_frame = this sequence's VP stage has not run before; a status
 *     other than 0 classifies every line as "none";
 *   - observation row j: the end points of kept line j as (x - cx) / fx, (y - cy) / fy in float, widened; then the VP
 *     entry of kept line 0 for EVERY row (node.cpp:104-109): (v0, v1, v2, v2 / v2) when classified, zeros otherwise.
 * The session borrows the context (one session per context; destroy the session before the context -- vpl_fe_destroy
 * destroys a session that is still open, whose pointer is invalid from then on) and uses image
 * slots [0, n_seq) for the new frames and [n_seq, 2 n_seq) for the previous ones, so the context needs
 * max_images >= 2 * n_seq and vpl_match_reserve(ctx, >= n_seq, max_kps).  Other calls on the context between two frames
 * overwrite what the session keeps in those slots; vpl_pre_set_maps is the exception and is what sets the maps.
 * Undistortion maps are optional: without them (vpl_pre_set_maps never called, or with NULL) the frames are not
 * remapped, exactly as in the mirror; no option depends on them, so their absence is never an error.
 * Refusals: VPL_E_INVALID for null pointers, n_seq < 1, options out of range (fx or fy 0, a negative quota, a bad CLAHE
 * grid, bad detector / matcher parameters) or a second session on one context; VPL_E_CAPACITY when max_images < 2 n_seq,
 * when vpl_match_reserve has not been called for n_seq pairs, when max_lines_per_image > 1024 (the VP stage's limit),
 * when a frame yields more lines than max_lines_per_image or a pair more key points than max_kps.  A refused
 * vpl_trk_frame leaves every sequence as it was: the new state is written beside the old and taken over on the device
 * only when no sequence of the call overflowed.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct vpl_trk vpl_trk;
typedef struct vpl_trk_options {
  vpl_edline_param ed;
  vpl_match_param match;
  int max_h_lines, max_v_lines;   /* the quota of :178-229 (euroc_config.yaml: 25, 25) */
  int equalize;                   /* CLAHE of :62-68 */
  double clip_limit;              /* 3.0 */
  int tiles_x, tiles_y;           /* 8, 8 */
  float fx, fy, cx, cy;           /* K_ of readIntrinsicParameter: end-point normalisation, and fx, cx, cy for the VP stage */
} vpl_trk_options;
void vpl_trk_default_options(vpl_trk_options* opt);   /* detector / matcher defaults, 25 / 25, CLAHE 3.0 8 x 8, K = identity */
int vpl_trk_create(vpl_trk** out, vpl_fe_ctx* ctx, int n_seq, const vpl_trk_options* opt);
void vpl_trk_destroy(vpl_trk* trk);
/* the sequence starts again with its next frame (first image, VP counter 0); allfeature_cnt is kept.  Asynchronous. */
int vpl_trk_reset(vpl_trk* trk, int seq);

typedef struct vpl_trk_result {   /* per sequence */
  int n_detected, n_lines;        /* the detector's lines | lines kept = rows of line_id / line_obs */
  int lines_exist;                /* the mirror's lines_exit: 0 = nothing detected, the frame was not taken over */
  int matched, n_tracked;         /* Matching()'s return value | kept lines that continue an id */
  int vp_ran, vp_status;          /* the VP stage ran (more than two kept lines) | its status */
  double vps[9];                  /* 0 when the stage did not run */
  int allfeature_cnt;
} vpl_trk_result;
/* raw [n_seq][H][W]; vp_seed [n_seq] (consumed only by sequences whose VP stage runs, as the mirror's vp_seed());
 * res [n_seq]; line_id [n_seq][max_lines], line_obs [n_seq][max_lines][8]: the first n_lines rows of a sequence are written */
int vpl_trk_frame(vpl_trk* trk, const uint8_t* raw, const uint32_t* vp_seed, vpl_trk_result* res, int* line_id, double* line_obs);
/* test access, any pointer may be NULL: what curframe_ holds after the last call -- img [H*W], lines / ids [max_lines]
 * (the kept ones first; the rest is not defined), t_cnt [max_lines] with its length *n_tcnt -- and the last accepted
 * call's match vector [max_lines] (-1 past the previous frame's kept lines, or when Matching() returned false) and VP
 * ids [max_lines] (3 past the kept lines, or when the stage did not run).  Synchronous. */
int vpl_trk_get_frame(vpl_trk* trk, int seq, uint8_t* img, vpl_line* lines, int* ids, int* t_cnt, int* n_tcnt, int* match,
                      int* vp_ids);
/* test access: the session's id kernel alone on the arguments of vpl_line_track_ids (at most 4096 entries per list) */
int vpl_trk_debug_ids(vpl_fe_ctx* ctx, int n_new, const float* ends_new, int n_prev, const int* id_prev, const int* tcnt_prev,
                      int n_tcnt_prev, const int* prev_to_new, int max_h_lines, int max_v_lines, int* allfeature_cnt, int* keep,
                      int* id_out, int* tcnt_out, int* vertical_new, int* n_vertical_new);

/* ------------------------------------------------------------------------------------------------------------
 * Point tracker session: FeatureTracker::readImage (feature_tracker/src/feature_tracker.cpp:107-224) and updateID (:263-273)
 * for n_seq independent cameras, one call per image; the counterpart of vpl_trk_*.  What survives from image to image lives
 * in HBM: the prepared previous image, cur_pts, ids, track_cnt, forw_scores, the previous undistorted points by id, prev_time
 * and the per-sequence id counter.  vpl_ptrk_frame copies the raw frames, times, publish flags and seeds down (one copy),
 * the results and rows back (one copy) and synchronises once.  Per sequence, in the reference's order: CLAHE; LK from cur_pts
 * (vpl_pt_flow_batch's kernels); the inBorder test (cvRound, border 1); compaction; track_cnt++.  When publish[i] is set:
 * rejectWithF with seed[i]; setMask; detection of max_cnt - kept corners under that mask; addPoints (id -1, track_cnt 1).
 * Then undistortedPoints (un-points, velocity against the previous image's points by id, score / max score) and updateID in
 * list order.  Rows are written for published frames, for the points with track_cnt > 1, in list order:
 *   row_id [n_seq][max_points];  rows [n_seq][max_points][7] = x, y (undistorted: float widened, what vpl_odo_frame.pt_xy1
 *   takes with a 1 behind them), u, v, vx, vy, prob
 * Kept as the reference has it, or stated where it leaves something open:
 *   - setMask orders by falling track_cnt with std::sort, which is not stable; here equal counts keep their list order;
 *   - the filled circle is OpenCV's integer midpoint walk (csrc/pt_plan.h), restated from its description, not pinned by a run;
 *   - prob of EVERY row is forw_un_scores[0] (feature_tracker_node.cpp:154 indexes with the camera); the per-point values are
 *     in vpl_ptrk_get_frame;
 *   - vx, vy: float difference of the two un-points, divided by dt in double, stored as cv::Point2f;
 *   - the id counter is per sequence (the reference's static n_id serves NUM_OF_CAM = 1); no stereo branch;
 *   - the node's first-image skip, first-publication skip and FREQ rule stay with the caller, who passes publish.
 * The session borrows the context: image slots [0, n_seq) for the new frames, [n_seq, 2 n_seq) for the previous ones, so
 * max_images >= 2 n_seq; vpl_pt_reserve with max_points and max_corners >= max_cnt; no undistortion maps.  One point session
 * per context (a second is VPL_E_INVALID).  VPL_E_CAPACITY when a published frame yields more corner candidates than
 * max_candidates: a refused call leaves every sequence as it was.  vpl_ptrk_reset: the sequence starts again with its next
 * image and keeps its id counter.  vpl_ptrk_set_mask: the fisheye mask [H][W] setMask starts from (NULL: all 255).
 * vpl_ptrk_get_frame: test access to the state (any pointer may be NULL; arrays of max_points entries).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct vpl_ptrk vpl_ptrk;
typedef struct vpl_ptrk_options {
  int max_cnt, min_dist;            /* 150, 30 */
  double f_threshold, focal_length; /* 1.0, 460 */
  int equalize;                     /* 1 */
  double clip_limit;                /* 3.0 */
  int tiles_x, tiles_y;             /* 8, 8 */
  double fx, fy, cx, cy, k1, k2, p1, p2;
} vpl_ptrk_options;
typedef struct vpl_ptrk_result {    /* counts after each stage */
  int tracked, after_border, after_f, after_mask, detected, published;
} vpl_ptrk_result;
void vpl_ptrk_default_options(vpl_ptrk_options* opt);
int vpl_ptrk_create(vpl_ptrk** out, vpl_fe_ctx* ctx, int n_seq, const vpl_ptrk_options* opt);
void vpl_ptrk_destroy(vpl_ptrk* trk);
int vpl_ptrk_set_mask(vpl_ptrk* trk, const uint8_t* fisheye_mask);
int vpl_ptrk_reset(vpl_ptrk* trk, int seq);
int vpl_ptrk_frame(vpl_ptrk* trk, const uint8_t* raw, const double* time, const int* publish, const unsigned long long* seed,
                   vpl_ptrk_result* res, int* row_id, double* rows);
int vpl_ptrk_get_frame(vpl_ptrk* trk, int seq, int* n, float* pts, int* ids, int* track_cnt, float* scores, float* un_pts,
                       float* un_scores, int* next_id);

/* ------------------------------------------------------------------------------------------------------------
 * Loop-closure front-end: what a pose_graph KeyFrame computes from its image, and the descriptor search of a loop candidate,
 * for a batch of frames / of pairs.  Stage calls, host in and host out; nothing depends on where an item sits in the batch and
 * the same inputs give the same bits twice.
 *   KeyFrame::KeyFrame (pose_graph/src/keyframe.cpp:14-41): computeWindowBRIEFPoint (:75-85) and computeBRIEFPoint (:87-113)
 *        -> vpl_lc_keyframe_batch
 *   KeyFrame::searchByBRIEFDes / searchInAera (:121-171), the first step of findConnection (:259-520)
 *        -> vpl_lc_match_batch
 * vpl_lc_reserve (once per context) fixes the row length max_keypoints of a frame's FAST list (1 .. 65535: an index travels in
 * 16 bits of the search key) and max_window_points of a window point list (1 .. 1024).  The 15 EuRoC frames (752 x 480) under
 * tests/golden hold 2572 .. 3330 FAST corners at threshold 20; 8192 is a comfortable row for such frames.  A frame with more corners
 * than the row holds is refused -- VPL_E_CAPACITY for the call, the frame and its count in vpl_fe_last_error, no output written
 * -- never cut short.
 * vpl_lc_set_pattern: the BRIEF test pairs as integers (the reference reads them from its settings file brief_pattern.yml:
 * x1, y1, x2, y2).  n_bits must be 256.  The library ships no pattern: vpl_lc_keyframe_batch before it is VPL_E_INVALID.
 * A descriptor is four 64-bit words; bit i of the reference's bitset is bit i % 64 of word i / 64.
 *
 * vpl_lc_keyframe_batch:
 *   images       [n][H][W], or NULL: the n frames in the context's image slots
 *   window_pts   [n][max_window_points][2] the window's tracked points in pixels (point_2d_uv);  window_counts [n] (0 is allowed)
 *   cam          the camera model of m_camera->liftProjective;  fast_threshold: 20 in the reference (0 .. 255)
 *   keypoints      [n][max_keypoints][2] cv::FAST(image, keypoints, fast_threshold, true): pixel positions in raster order
 *   keypoints_norm [n][max_keypoints][2] the lifted x / z, y / z rounded to float as cv::Point2f does
 *   kp_counts [n];  brief [n][max_keypoints][4];  window_brief [n][max_window_points][4]
 *   Rows past kp_counts[i] / window_counts[i] are left as they were.
 * Two copies down (the frames when passed, the window lists), one copy back, one synchronisation.
 * What OpenCV leaves to its version or build is stated in csrc/lc_kernels.h, from its description and not pinned by a run: the
 * float arithmetic of GaussianBlur(9 x 9, sigma 2), and FAST's score and list order.
 * vpl_lc_debug_frame: test access to frame `img` of the last call (any pointer may be NULL): the blurred plane [H*W] and the
 * FAST score plane [H*W] (0 = no corner).
 *
 * vpl_lc_match_batch, per pair (n_pairs <= max_images):
 *   window_brief [n][max_window_points][4], window_counts [n]: the current keyframe's window descriptors
 *   old_brief [n][max_keypoints][4], old_keypoints, old_keypoints_norm [n][max_keypoints][2], old_counts [n]: the candidate's
 *   matched_2d_old, matched_2d_old_norm [n][max_window_points][2]: the old point of least Hamming distance among those below 128
 *   (the first index on a tie), taken when that distance is below 80, else (0, 0);  status [n][max_window_points] 1 / 0
 *   best_dist, best_index [n][max_window_points] (may be NULL; tests): 128 / -1 when no distance was below 128
 *   The first window_counts[i] entries of a row are written.  Counts of 0 are legal on either side.
 * One copy each way, one synchronisation.
 * ------------------------------------------------------------------------------------------------------------ */
int vpl_lc_reserve(vpl_fe_ctx* ctx, int max_keypoints, int max_window_points);
int vpl_lc_set_pattern(vpl_fe_ctx* ctx, int n_bits, const int* x1, const int* y1, const int* x2, const int* y2);
int vpl_lc_keyframe_batch(vpl_fe_ctx* ctx, int n_images, const uint8_t* images, const float* window_pts, const int* window_counts,
                          const vpl_pt_camera* cam, int fast_threshold, float* keypoints, float* keypoints_norm, int* kp_counts,
                          unsigned long long* brief, unsigned long long* window_brief);
int vpl_lc_debug_frame(vpl_fe_ctx* ctx, int img, uint8_t* blurred, uint8_t* score);
int vpl_lc_match_batch(vpl_fe_ctx* ctx, int n_pairs, const unsigned long long* window_brief, const int* window_counts,
                       const unsigned long long* old_brief, const float* old_keypoints, const float* old_keypoints_norm,
                       const int* old_counts, float* matched_2d_old, float* matched_2d_old_norm, uint8_t* status, int* best_dist,
                       int* best_index);

/* ------------------------------------------------------------------------------------------------------------
 * Loop detector session: PoseGraph::detectLoop (pose_graph/src/pose_graph.cpp:304-386) and addKeyFrameIntoVoc (:388-401) -- the
 * DBoW2 vocabulary, the keyframe database and the query that names a loop candidate -- for n_db independent databases (one per
 * PoseGraph) that share one vocabulary, one call per keyframe; everything stays on the device.  The step between
 * vpl_lc_keyframe_batch and vpl_lc_match_batch.  The session borrows the context (one per context; vpl_fe_destroy destroys a
 * session that is still open).
 *
 * Vocabulary.  vpl_ld_load_vocabulary reads the reference's binary file (ThirdParty/VocabularyBinary.hpp, loadBin,
 * TemplatedVocabulary.h:1509-1561): six int32 k, L, scoringType, weightingType, nNodes, nWords; nNodes records of 48 bytes
 * (int32 nodeId, int32 parentId, double weight, uint64 descriptor[4]); nWords records of 8 bytes (int32 nodeId, int32 wordId).
 * vpl_ld_set_vocabulary takes the same content from arrays.  The root is node 0 and not listed; a node's children are in list
 * order; a descriptor has the bit layout vpl_lc_keyframe_batch writes.  The tree need not be regular.  The descent of a
 * descriptor starts at the root, takes the child of least Hamming distance (the first on a tie) and stops at the first node
 * without children; its word and weight are that leaf's.  Refused with VPL_E_INVALID, the reason in vpl_fe_last_error, the
 * session unchanged: a node id outside 1 .. nNodes or given twice, a parent that is not a node, a cycle, a leaf without a word,
 * a word on an inner node, a node with two words, a word id outside 0 .. nWords - 1 or given twice, a node deeper than 16
 * levels, a truncated file, a scoring other than L1_NORM (0).  Weighting 0 .. 3 = TF_IDF, TF, IDF, BINARY.  A vocabulary without
 * nodes is legal and gives empty bags.  Setting a vocabulary empties every database.  The reference's own file
 * (support_files/brief_k10L6.bin) was never available to this project: the layout is restated from the sources that read it.
 *
 * vpl_ld_detect, per database d with counts[d] >= 0 (a negative count leaves the database untouched), in the reference's order:
 *   transform (TemplatedVocabulary.h:1065-1121): words with a weight > 0; TF_IDF and TF add the weight once per occurrence by
 *     repeated addition, IDF and BINARY set it once; the L1 norm summed in ascending word id, every value divided by it (left
 *     as it is when the norm is 0);
 *   queryL1 (TemplatedDatabase.h:656-723) with max_id = frame_index[d] - recent: entry e takes part if e < max_id || max_id == -1
 *     || e == n_entries - 1; it is a result if it shares a word with the query; raw score = the sum over the shared words in
 *     ascending word id of fabs(q - v) - fabs(q) - fabs(v); the max_results smallest by (raw score, entry id) -- the reference
 *     sorts by the score alone and leaves ties to std::sort -- with score = -raw / 2;
 *   db.add: the bag becomes entry n_entries (an empty bag too); then loop_index by pose_graph.cpp:348-384: found if
 *     scores[0] > neighbour_score and some scores[i >= 1] > loop_score, reported only if frame_index[d] > recent, as ids[0]
 *     replaced by any result of smaller id with a score > loop_score; else -1.
 *   brief [n_db][max_keypoints][4], counts [n_db], frame_index [n_db], res [n_db] (entry -1, nothing else, for a skipped database)
 * vpl_ld_add: addKeyFrameIntoVoc, the transform and db.add without the query (res may be NULL).
 * vpl_ld_detect_fe: vpl_ld_detect on the descriptor rows and counts the last vpl_lc_keyframe_batch on the session's context left on
 *   the device, image slot i to database i; VPL_E_INVALID unless that call took n_db images with rows of max_keypoints.
 * vpl_ld_reset empties one database (asynchronous).  vpl_ld_size: its number of entries.  vpl_ld_get_bow (tests): a stored bag,
 *   words ascending; arrays of max_keypoints entries.
 * VPL_E_CAPACITY, the database named in vpl_fe_last_error, NO database of the call changed: a count above max_keypoints, entry
 * max_keyframes + 1, a bag that does not fit into what is left of max_words_total (a stored bag takes its own length; none is
 * cut short).  VPL_E_INVALID before a vocabulary is set.  One copy down (the rows; frame_index alone for _fe), one copy back,
 * one synchronisation.  All arithmetic is f64 in the stated order: scores and bag values are the reference's bits.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct vpl_ld vpl_ld;
typedef struct vpl_ld_options {
  int max_keyframes;        /* per database (2048) */
  int max_keypoints;        /* row length of a descriptor list, <= 8192 (8192) */
  int max_words_total;      /* per database: the pool of the stored bags (2048 * 3000) */
  int max_results;          /* 4 (1 .. 4) */
  int recent;               /* 50 */
  double neighbour_score;   /* 0.05 */
  double loop_score;        /* 0.015 */
} vpl_ld_options;
typedef struct vpl_ld_result {
  int loop_index;           /* detectLoop's return value */
  int n_results;
  int ids[4];               /* -1 past n_results */
  double scores[4];         /* 0 past n_results */
  int n_words;              /* length of the new bag */
  int entry;                /* the id the keyframe got */
} vpl_ld_result;
void vpl_ld_default_options(vpl_ld_options* opt);
int vpl_ld_create(vpl_ld** out, vpl_fe_ctx* ctx, int n_db, const vpl_ld_options* opt);
void vpl_ld_destroy(vpl_ld* ld);
int vpl_ld_set_vocabulary(vpl_ld* ld, int k, int L, int scoring, int weighting, int n_nodes, const int* node_id, const int* parent_id,
                          const double* weight, const unsigned long long* descriptor, int n_words, const int* word_node,
                          const int* word_id);
int vpl_ld_load_vocabulary(vpl_ld* ld, const char* path);
int vpl_ld_detect(vpl_ld* ld, const unsigned long long* brief, const int* counts, const int* frame_index, vpl_ld_result* res);
int vpl_ld_detect_fe(vpl_ld* ld, const int* frame_index, vpl_ld_result* res);
int vpl_ld_add(vpl_ld* ld, const unsigned long long* brief, const int* counts, vpl_ld_result* res);
int vpl_ld_reset(vpl_ld* ld, int db);
int vpl_ld_size(vpl_ld* ld, int db);
int vpl_ld_get_bow(vpl_ld* ld, int db, int entry, int* n, int* words, double* values);

#ifdef __cplusplus
}
#endif
#endif /* VPLINES_FRONTEND_H */
