// Loop verification on the device (vpl_loop_verify_batch): KeyFrame::findConnection from the PnP on
// (pose_graph/src/keyframe.cpp:406-516) -- PnPRANSAC (:200-256), the MIN_LOOP_NUM gates, the relative pose and its acceptance.
//
// k_loop_verify.  Launch: grid (n items), SFM_THREADS = 256 threads.  LDS: 28 280 B, SfmLds (sfm_lm's workspace) + 112 B (the guess and
// the best model).  The work-group owns one item and runs the RANSAC as the sequential loop it is: per iteration the five-point
// sample of the item's stream (loop_plan.h), ONE statement of the minimiser -- sfm_lm of init_sfm.h with the points constant and
// camera slot 0 free, the PnP of vpl_init_structure_batch -- from the extrinsic guess, then the inlier count with a lane per point
// (every 256th).  A model replaces the best only with strictly more inliers (and more than four), and then the iteration cap
// is read from the stopping table.  The final pose is the same minimiser on all inliers of the best model, started from it.
// Global workspace per item: the points and observations widened from float, sfm_lm's 56 doubles per observation, the five
// integer lists of a DevSfmProb (rewritten by lane 0 for every sample and for the final solve) and the current model's mask.
// FP64.  Nothing depends on where an item sits in the batch.
#pragma once
#include "init_sfm.h"
#include "loop_plan.h"

namespace vpl {

// per item, offsets into its integer table: camera slot, point, observation row of every observation, c_off [12], c_list
constexpr int LV_O_CAM = 0, LV_O_PT = VPL_LOOP_MAX_POINTS, LV_O_UV = 2 * VPL_LOOP_MAX_POINTS, LV_C_OFF = 3 * VPL_LOOP_MAX_POINTS,
              LV_C_LIST = 3 * VPL_LOOP_MAX_POINTS + 16, LV_ITAB = 4 * VPL_LOOP_MAX_POINTS + 16;

struct DevLoopItem {
  int count, nit;             // nit: where niters_after [count + 1] stands in the call's table (count > min_loop_num)
  unsigned long long seed;
  double vioT[3], vioR[9], tic[3], qic[9];
};
struct DevLoopArgs {
  const DevLoopItem* items;
  const int* tables;
  double* X;                  // [n][MAX][3]
  double* uv;                 // [n][MAX][2]
  double* wo;                 // [n][MAX][SFM_OBS_WS]
  int* itab;                  // [n][LV_ITAB]
  unsigned char* cur;         // [n][MAX] the mask of the model under test
  unsigned char* status;      // [n][MAX] the mask of the best model
  vpl_loop_result* out;
  vpl_loop_options opt;
};

__device__ __forceinline__ DevSfmProb loop_problem(int nobs) {
  DevSfmProb P{};
  P.nobs = nobs; P.npt = 0;
  P.o_cam = LV_O_CAM; P.o_pt = LV_O_PT; P.o_uv = LV_O_UV; P.c_off = LV_C_OFF; P.c_list = LV_C_LIST;
  P.free_q = 1; P.free_t = 1; P.uv0 = 0;
  return P;
}

__global__ __launch_bounds__(SFM_THREADS) void k_loop_verify(DevLoopArgs A) {
  __shared__ SfmLds L;
  __shared__ double guess[7], best[7];
  const int s = blockIdx.x, tid = threadIdx.x;
  const DevLoopItem& q = A.items[s];
  vpl_loop_result& o = A.out[s];
  const int N = q.count;
  // (the host has zeroed out[s] and status[s]: stage VPL_LOOP_FEW_POINTS, has_loop 0)
  if (!(N > A.opt.min_loop_num)) return;
  double* X = A.X + (size_t)s * VPL_LOOP_MAX_POINTS * 3;
  double* uv = A.uv + (size_t)s * VPL_LOOP_MAX_POINTS * 2;
  double* wo = A.wo + (size_t)s * VPL_LOOP_MAX_POINTS * SFM_OBS_WS;
  int* itab = A.itab + (size_t)s * LV_ITAB;
  unsigned char* cur = A.cur + (size_t)s * VPL_LOOP_MAX_POINTS;
  unsigned char* status = A.status + (size_t)s * VPL_LOOP_MAX_POINTS;
  const int* table = A.tables + q.nit;
  const double thr2 = A.opt.reproj_error * A.opt.reproj_error;
  for (int k = tid; k < VPL_LOOP_MAX_POINTS; k += SFM_THREADS) { itab[LV_O_CAM + k] = 0; itab[LV_C_LIST + k] = k; }
  if (tid < VPL_NFRAMES) {
    sfm_storeq(L.cq + 4 * tid, Q4{1.0, 0.0, 0.0, 0.0});
    sfm_store3(L.ct + 3 * tid, V3{0.0, 0.0, 0.0});
  }
  // (the item's poses are read where lane 0 needs them, here and after the final solve: nothing of them lives across sfm_lm)
  if (tid == 0) {   // the extrinsic guess of PnPRANSAC (:212-216): the inverse of the current camera's pose
    M3 qic, vioR;
    for (int k = 0; k < 9; ++k) { qic.m[k] = q.qic[k]; vioR.m[k] = q.vioR[k]; }
    const V3 tic = sfm_load3(q.tic), vioT = sfm_load3(q.vioT);
    const M3 Rwc = mul(vioR, qic);
    const V3 Twc = vioT + mul(vioR, tic);
    sfm_storeq(guess, qnormalized(mat2q(transpose(Rwc))));
    sfm_store3(guess + 4, -mulT(Rwc, Twc));
  }
  __syncthreads();
  int niters = A.opt.max_iters, best_good = 0, ran = 0;
  for (int it = 0; it < niters; ++it) {
    if (tid == 0) {
      int idx[LOOP_SAMPLE] = {-1, -1, -1, -1, -1};
      loop_sample(q.seed, it, N, idx);
      for (int k = 0; k < LOOP_SAMPLE; ++k) { itab[LV_O_PT + k] = idx[k]; itab[LV_O_UV + k] = idx[k]; }
      itab[LV_C_OFF] = 0;
      for (int f = 1; f <= VPL_NFRAMES; ++f) itab[LV_C_OFF + f] = LOOP_SAMPLE;
      for (int k = 0; k < 4; ++k) L.cq[k] = guess[k];
      for (int k = 0; k < 3; ++k) L.ct[k] = guess[4 + k];
    }
    __syncthreads();
    const SfmReport rep = sfm_lm(loop_problem(LOOP_SAMPLE), itab, uv, X, wo, nullptr, L);
    ran = it + 1;
    if (rep.termination == SFM_FAILURE || !sfm_finite(L.cq, 4) || !sfm_finite(L.ct, 3)) { __syncthreads(); continue; }
    // the squared reprojection distance in the normalised plane, compared in double
    const M3 R = qmat(qnormalized(sfm_loadq(L.cq)));
    const V3 t = sfm_load3(L.ct);
    double good = 0.0;
    for (int p = tid; p < N; p += SFM_THREADS) {
      const V3 c = mul(R, sfm_load3(X + 3 * p)) + t;
      const double iz = 1.0 / c.z, ex = c.x * iz - uv[2 * p], ey = c.y * iz - uv[2 * p + 1];
      const bool in = ex * ex + ey * ey <= thr2;
      cur[p] = in ? 1 : 0;
      good += in ? 1.0 : 0.0;
    }
    const int g = (int)block_sum(good, L.red);
    if (g > max(best_good, LOOP_SAMPLE - 1)) {
      best_good = g;
      niters = min(niters, table[g]);
      for (int p = tid; p < N; p += SFM_THREADS) status[p] = cur[p];   // (a lane's own entries)
      if (tid == 0) {
        for (int k = 0; k < 4; ++k) best[k] = L.cq[k];
        for (int k = 0; k < 3; ++k) best[4 + k] = L.ct[k];
      }
    }
    __syncthreads();
  }
  if (tid == 0) { o.ransac_iterations = ran; o.best_inliers = best_good; }
  if (best_good == 0) {   // no sample gave a model: status stays 0
    if (tid == 0) o.stage = VPL_LOOP_NO_MODEL;
    return;
  }
  // ---- the final solve on the inliers of the best model, in list order
  if (tid == 0) {
    int m = 0;
    for (int p = 0; p < N; ++p)
      if (status[p]) { itab[LV_O_PT + m] = p; itab[LV_O_UV + m] = p; ++m; }
    itab[LV_C_OFF] = 0;
    for (int f = 1; f <= VPL_NFRAMES; ++f) itab[LV_C_OFF + f] = m;
    for (int k = 0; k < 4; ++k) L.cq[k] = best[k];
    for (int k = 0; k < 3; ++k) L.ct[k] = best[4 + k];
  }
  __syncthreads();
  const SfmReport rep = sfm_lm(loop_problem(best_good), itab, uv, X, wo, nullptr, L);
  if (tid != 0) return;
  o.lm_iterations = rep.iterations;
  o.lm_termination = rep.termination;
  if (rep.termination == SFM_FAILURE || !sfm_finite(L.cq, 4) || !sfm_finite(L.ct, 3)) { o.stage = VPL_LOOP_NUMERIC; return; }
  // PnP_R_old, PnP_T_old (:245-254)
  M3 qic, vioR;
  for (int k = 0; k < 9; ++k) { qic.m[k] = q.qic[k]; vioR.m[k] = q.vioR[k]; }
  const V3 tic = sfm_load3(q.tic), vioT = sfm_load3(q.vioT);
  const M3 Rpnp = qmat(qnormalized(sfm_loadq(L.cq)));
  const M3 Rwc_old = transpose(Rpnp);
  const V3 Twc_old = mul(Rwc_old, -sfm_load3(L.ct));
  const M3 Rold = mul(Rwc_old, transpose(qic));
  const V3 Told = Twc_old - mul(Rold, tic);
  for (int k = 0; k < 9; ++k) o.PnP_R_old[k] = Rold.m[k];
  sfm_store3(o.PnP_T_old, Told);
  if (!(best_good > A.opt.min_loop_num)) { o.stage = VPL_LOOP_FEW_INLIERS; return; }
  // the relative pose and its acceptance (:472-487)
  const V3 rt = mulT(Rold, vioT - Told);
  const Q4 rq = mat2q(mulTA(Rold, vioR));
  const double d = R2ypr(vioR).x - R2ypr(Rold).x;
  const double yaw = d > 0 ? d - 360.0 * floor((d + 180.0) / 360.0) : d + 360.0 * floor((-d + 180.0) / 360.0);   // normalizeAngle
  o.loop_info[0] = rt.x; o.loop_info[1] = rt.y; o.loop_info[2] = rt.z;
  o.loop_info[3] = rq.w; o.loop_info[4] = rq.x; o.loop_info[5] = rq.y; o.loop_info[6] = rq.z;
  o.loop_info[7] = yaw;
  const bool ok = fabs(yaw) < A.opt.max_yaw_deg && norm(rt) < A.opt.max_t;
  o.has_loop = ok ? 1 : 0;
  o.stage = ok ? VPL_LOOP_CLOSED : VPL_LOOP_REJECTED;
}

}  // namespace vpl
