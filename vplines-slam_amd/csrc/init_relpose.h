// Relative pose on the device (vpl_init_relative_pose_batch): Estimator::relativePose (vins_estimator/src/estimator.cpp:590-622)
// and MotionEstimator::solveRelativeRT (initial/solve_5pts.cpp:193-228) -- cv::findFundamentalMat(FM_RANSAC) and cv::recoverPose.
//   k_relpose_ransac  one work-group of 256 per (sequence, candidate window frame i): getCorresponding(i, 10) compacted into LDS,
//                     the two gates, the RANSAC in rounds of 256 iterations (one lane each), recoverPose;
//   k_relpose_finish  one wave per sequence: l, the smallest i that succeeded.
// A lane's hypothesis: its seven points fill the 7 x 9 system; seven Householder reflections of its rows (the 63 entries in
// registers, every index a constant after unrolling) leave the two-dimensional null space as Q e7, Q e8 = F1, F2;
// det(lambda F1 + (1 - lambda) F2) is a cubic in lambda, solved in closed form; every real root, in ascending lambda, is scored
// over all correspondences, which every lane reads from the same LDS address.  After a round one lane replays the sequential
// rule over the round's counts in (iteration, root) order -- a hypothesis wins with good > max(best, 6), a win sets niters from
// the host's table (init_relpose_plan.h), the loop ends at the first iteration >= niters -- so the result is that of a
// sequential loop over the same stream; what ran past the stop is discarded.
// FP64, wave64.  Every sum has a fixed order, there are no atomics, nothing depends on where a sequence sits in the batch.
#pragma once
#include "vplines_ba.h"
#include "vpl_math.h"
#include "ba_common.h"
#include "ba_lineopt.h"
#include "init_relpose_plan.h"
#include "relpose_f7.h"

namespace vpl {

constexpr int REL_NCAND = VPL_WINDOW_SIZE;
constexpr int REL_TRACKS_PER_LANE = VPL_SFM_MAX_TRACKS / REL_THREADS;
static_assert(REL_TRACKS_PER_LANE * REL_THREADS == VPL_SFM_MAX_TRACKS, "every lane gathers the same number of tracks");
constexpr double REL_THRESHOLD = 0.3 / 460.0;   // solve_5pts.cpp:205
constexpr double REL_FOCAL = 460.0, REL_MIN_PARALLAX = 30.0;   // estimator.cpp:613
constexpr double REL_MAX_DEPTH = 50.0;          // solve_5pts.cpp:77

// One sequence; the integers are offsets into the call's integer table, uv0 into its table of doubles.
struct DevRelSeq {
  int N;                          // tracks
  int t_start, t_nobs, t_off;     // [N] tables
  int uv0;
  int nit[REL_NCAND];             // niters_after [n_corres + 1] of candidate i, -1: the candidate is not tried
  int ncor[REL_NCAND];            // n_corres as the host counted it
  int pad_;
  unsigned long long seed;
};
struct DevRelArgs {
  const DevRelSeq* seqs;
  const int* itab;
  const double* dtab;
  vpl_relpose_result* out;
  unsigned char* mask_ransac;     // null or [n][10][VPL_SFM_MAX_TRACKS]
  unsigned char* mask_pose;
  int* hyp;                       // null or [n][10][1000][3], preset to -1
};

struct RelLds {
  double pt[4 * VPL_SFM_MAX_TRACKS];   // x_i, y_i, x_10, y_10 per correspondence, rounded to float
  double red[24];
  double R1[9], R2[9], t[3];           // decomposeEssentialMat
  RelRansacLds R;                      // the loop's state, the winning hypothesis in R.F
  int scan[REL_THREADS + 1];
  unsigned char m0[VPL_SFM_MAX_TRACKS], m1[VPL_SFM_MAX_TRACKS];
};

// cv::decomposeEssentialMat (solve_5pts.cpp:5-28) by one-sided Jacobi on the columns of F: F V = B with orthogonal columns,
// the columns ordered by falling norm, u1 / u2 the first two normalised, u3 = u1 x u2 (det U = +1 by construction), V's sign
// fixed to det +1.  R1 = U W V^T, R2 = U W^T V^T, t = u3.
__device__ inline void rel_decompose(const double* F, double* R1, double* R2, double* t) {
  double B[9], V[9];
  for (int k = 0; k < 9; ++k) { B[k] = F[k]; V[k] = (k % 4 == 0) ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0, be = 0, ga = 0;
        for (int r = 0; r < 3; ++r) { al += B[3 * r + p] * B[3 * r + p]; be += B[3 * r + q] * B[3 * r + q]; ga += B[3 * r + p] * B[3 * r + q]; }
        if (ga == 0.0 || fabs(ga) <= 1e-15 * sqrt(al * be)) continue;
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + tt * tt), sn = c * tt;
        for (int r = 0; r < 3; ++r) {
          double x = B[3 * r + p], y = B[3 * r + q];
          B[3 * r + p] = c * x - sn * y; B[3 * r + q] = sn * x + c * y;
          x = V[3 * r + p]; y = V[3 * r + q];
          V[3 * r + p] = c * x - sn * y; V[3 * r + q] = sn * x + c * y;
        }
      }
    if (!rotated) break;
  }
  double n2[3];
  for (int c = 0; c < 3; ++c) n2[c] = B[c] * B[c] + B[3 + c] * B[3 + c] + B[6 + c] * B[6 + c];
  int o[3] = {0, 1, 2};   // falling norm, ties keep the lower column first
  if (n2[o[1]] > n2[o[0]]) { const int s = o[0]; o[0] = o[1]; o[1] = s; }
  if (n2[o[2]] > n2[o[1]]) { const int s = o[1]; o[1] = o[2]; o[2] = s; }
  if (n2[o[1]] > n2[o[0]]) { const int s = o[0]; o[0] = o[1]; o[1] = s; }
  const double s1 = sqrt(n2[o[0]]), s2 = sqrt(n2[o[1]]);
  const V3 u1{B[o[0]] / s1, B[3 + o[0]] / s1, B[6 + o[0]] / s1}, u2{B[o[1]] / s2, B[3 + o[1]] / s2, B[6 + o[1]] / s2};
  const V3 u3 = cross(u1, u2);
  V3 v1{V[o[0]], V[3 + o[0]], V[6 + o[0]]}, v2{V[o[1]], V[3 + o[1]], V[6 + o[1]]}, v3{V[o[2]], V[3 + o[2]], V[6 + o[2]]};
  if (dot(v1, cross(v2, v3)) < 0.0) { v1 = -v1; v2 = -v2; v3 = -v3; }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double a = get(u1, r) * get(v2, c), b = get(u2, r) * get(v1, c), d = get(u3, r) * get(v3, c);
      R1[3 * r + c] = a - b + d;
      R2[3 * r + c] = b - a + d;
    }
  t[0] = u3.x; t[1] = u3.y; t[2] = u3.z;
}

// one of recoverPose's four masks for one correspondence: cv::triangulatePoints against [I | 0] and [R | t], then
// z w > 0, z < 50 in the first camera, 0 < z < 50 in the second (solve_5pts.cpp:79-88)
__device__ inline bool rel_in_front(const double* R, double tx, double ty, double tz, double x1, double y1, double x2, double y2) {
  double A[16], V[16];
  A[0] = -1.0; A[1] = 0.0; A[2] = x1; A[3] = 0.0;
  A[4] = 0.0; A[5] = -1.0; A[6] = y1; A[7] = 0.0;
  for (int c = 0; c < 3; ++c) {
    A[8 + c] = x2 * R[6 + c] - R[c];
    A[12 + c] = y2 * R[6 + c] - R[3 + c];
  }
  A[11] = x2 * tz - tx;
  A[15] = y2 * tz - ty;
  const int cm = dlt_null_column(A, 4, V);
  const double qx = V[cm], qy = V[4 + cm], qz = V[8 + cm], qw = V[12 + cm];
  bool m = qz * qw > 0.0;
  const double X = qx / qw, Y = qy / qw, Z = qz / qw;
  m = m && Z < REL_MAX_DEPTH;
  const double z2 = R[6] * X + R[7] * Y + R[8] * Z + tz;
  return m && z2 > 0.0 && z2 < REL_MAX_DEPTH;
}

__global__ __launch_bounds__(REL_THREADS) void k_relpose_ransac(DevRelArgs A) {
  __shared__ RelLds L;
  const int cand = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const DevRelSeq& q = A.seqs[s];
  const int* itab = A.itab;
  vpl_relpose_candidate& o = A.out[s].cand[cand];
  const size_t slot = (size_t)s * REL_NCAND + cand;
  // ---- getCorresponding(cand, 10) in track-list order: a track covers both frames when it starts at or before cand and
  //      ends in frame 10 (feature_manager.cpp:219)
  int mine = 0;
  bool has[REL_TRACKS_PER_LANE];
#pragma unroll
  for (int k = 0; k < REL_TRACKS_PER_LANE; ++k) {
    const int j = REL_TRACKS_PER_LANE * tid + k;
    has[k] = j < q.N && itab[q.t_start + j] <= cand && itab[q.t_start + j] + itab[q.t_nobs + j] - 1 >= VPL_WINDOW_SIZE;
    mine += has[k] ? 1 : 0;
  }
  L.scan[tid + 1] = mine;
  __syncthreads();
  if (tid == 0) {
    L.scan[0] = 0;
    for (int k = 0; k < REL_THREADS; ++k) L.scan[k + 1] += L.scan[k];
  }
  __syncthreads();
  const int N = L.scan[REL_THREADS];
  double par = 0.0, bad = 0.0;
  {
    int at = L.scan[tid];
    const double* obs = A.dtab + q.uv0;
#pragma unroll
    for (int k = 0; k < REL_TRACKS_PER_LANE; ++k) {
      if (!has[k]) continue;
      const int j = REL_TRACKS_PER_LANE * tid + k;
      const int st = itab[q.t_start + j], off = itab[q.t_off + j];
      const double* a = obs + 2 * (size_t)(off + cand - st);
      const double* b = obs + 2 * (size_t)(off + VPL_WINDOW_SIZE - st);
      const double dx = a[0] - b[0], dy = a[1] - b[1];
      par += sqrt(dx * dx + dy * dy);
      if (!(isfinite(a[0]) && isfinite(a[1]) && isfinite(b[0]) && isfinite(b[1]))) bad = 1.0;
      double* p = L.pt + 4 * at;   // cv::Point2f
      p[0] = (double)(float)a[0]; p[1] = (double)(float)a[1]; p[2] = (double)(float)b[0]; p[3] = (double)(float)b[1];
      ++at;
    }
  }
  par = block_sum(par, L.red);
  bad = block_sum(bad, L.red);
  const double average_parallax = N > 0 ? par / N : 0.0;
  int status = VPL_RELPOSE_SUCCESS;
  if (!(N > RELPOSE_MIN_CORRES)) status = VPL_RELPOSE_FEW_CORRES;
  else if (!(average_parallax * REL_FOCAL > REL_MIN_PARALLAX)) status = VPL_RELPOSE_LOW_PARALLAX;
  // a correspondence that is not finite gives no model (k_relpose_finish fails the sequence); so does a table the host did not
  // send, which cannot be: the two counts of the correspondences are the same function of the same integers
  const bool run = status == VPL_RELPOSE_SUCCESS && !(bad > 0.0) && q.nit[cand] >= 0 && q.ncor[cand] == N;
  if (status == VPL_RELPOSE_SUCCESS && !run) status = VPL_RELPOSE_NO_MODEL;
  if (tid == 0) {
    o.n_corres = N;
    o.average_parallax = average_parallax;
    o.numeric = bad > 0.0 ? 1 : 0;
    o.best_iteration = o.best_root = -1;
    o.status = status;
  }
  if (!run) return;
  const int* niters_after = itab + q.nit[cand];
  // ---- the RANSAC, 256 iterations at a time (relpose_f7.h)
  rel_ransac_run(L.pt, N, q.seed, cand, niters_after, REL_THRESHOLD * REL_THRESHOLD, L.R, A.hyp ? A.hyp + slot * RELPOSE_MAX_ITERS * 3 : nullptr);
  const int best_it = L.R.st[RS_BEST_IT];
  if (tid == 0) {
    o.iterations = L.R.st[RS_NITERS];
    o.best_iteration = best_it; o.best_root = L.R.st[RS_BEST_ROOT];
  }
  if (best_it < 0) {
    if (tid == 0) o.status = VPL_RELPOSE_NO_MODEL;
    return;
  }
  // ---- the winner's mask (findInliers), then recoverPose
  double Fw[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Fw[k] = L.R.F[k];
  double inl = 0.0;
  for (int p = tid; p < N; p += REL_THREADS) {
    const bool m = rel_inlier(Fw, L.pt[4 * p], L.pt[4 * p + 1], L.pt[4 * p + 2], L.pt[4 * p + 3], REL_THRESHOLD * REL_THRESHOLD);
    L.m0[p] = m ? 1 : 0;
    inl += m ? 1.0 : 0.0;
  }
  inl = block_sum(inl, L.red);
  if (tid == 0) rel_decompose(L.R.F, L.R1, L.R2, L.t);
  __syncthreads();
  double g[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = tid; p < N; p += REL_THREADS) {
    const double x1 = L.pt[4 * p], y1 = L.pt[4 * p + 1], x2 = L.pt[4 * p + 2], y2 = L.pt[4 * p + 3];
    int code = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double sg = k < 2 ? 1.0 : -1.0;
      const bool m = L.m0[p] && rel_in_front((k & 1) ? L.R2 : L.R1, sg * L.t[0], sg * L.t[1], sg * L.t[2], x1, y1, x2, y2);
      code |= m ? 1 << k : 0;
      g[k] += m ? 1.0 : 0.0;
    }
    L.m1[p] = (unsigned char)code;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) g[k] = block_sum(g[k], L.red);
  int pick = 3;   // the cascade of solve_5pts.cpp:152-181
  if (g[0] >= g[1] && g[0] >= g[2] && g[0] >= g[3]) pick = 0;
  else if (g[1] >= g[0] && g[1] >= g[2] && g[1] >= g[3]) pick = 1;
  else if (g[2] >= g[0] && g[2] >= g[1] && g[2] >= g[3]) pick = 2;
  const int good = (int)g[pick];
  for (int p = tid; p < N; p += REL_THREADS) {
    const unsigned char m = (L.m1[p] >> pick) & 1;
    if (A.mask_ransac) A.mask_ransac[slot * VPL_SFM_MAX_TRACKS + p] = L.m0[p];
    if (A.mask_pose) A.mask_pose[slot * VPL_SFM_MAX_TRACKS + p] = m;
  }
  if (tid == 0) {
    const double* R = (pick & 1) ? L.R2 : L.R1;
    const double sg = pick < 2 ? 1.0 : -1.0;
    const V3 t{sg * L.t[0], sg * L.t[1], sg * L.t[2]};
    M3 Rm;
    for (int k = 0; k < 9; ++k) { Rm.m[k] = R[k]; o.F[k] = L.R.F[k]; }
    const M3 Rt = transpose(Rm);          // Rotation = R^T, Translation = -R^T t (solve_5pts.cpp:220-221)
    const V3 T = -mul(Rt, t);
    for (int k = 0; k < 9; ++k) o.R[k] = Rt.m[k];
    o.T[0] = T.x; o.T[1] = T.y; o.T[2] = T.z;
    o.inliers = (int)inl;
    o.good = good;
    o.pose_choice = pick;
    o.status = good > RELPOSE_MIN_GOOD ? VPL_RELPOSE_SUCCESS : VPL_RELPOSE_FEW_GOOD;
  }
}

__global__ __launch_bounds__(64) void k_relpose_finish(DevRelArgs A) {
  vpl_relpose_result& o = A.out[blockIdx.x];
  if (threadIdx.x != 0) return;
  int l = -1, fail = 0;
  for (int i = REL_NCAND - 1; i >= 0; --i) {
    const vpl_relpose_candidate& c = o.cand[i];
    if (c.numeric) fail |= VPL_RELPOSE_FAIL_NUMERIC;
    if (c.status == VPL_RELPOSE_SUCCESS) l = i;
  }
  if (!fail && l < 0) fail = VPL_RELPOSE_FAIL_NONE;
  o.fail = fail;
  o.ok = fail ? 0 : 1;
  o.l = fail ? -1 : l;
  for (int k = 0; k < 9; ++k) o.relative_R[k] = fail ? 0.0 : o.cand[l].R[k];
  for (int k = 0; k < 3; ++k) o.relative_T[k] = fail ? 0.0 : o.cand[l].T[k];
}

}  // namespace vpl
