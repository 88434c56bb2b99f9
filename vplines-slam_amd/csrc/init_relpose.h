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

namespace vpl {

constexpr int REL_THREADS = 256;
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
  double F[9];                         // the winning hypothesis
  double R1[9], R2[9], t[3];           // decomposeEssentialMat
  int cnt[3 * REL_THREADS];            // the round's inlier counts, (iteration, root)
  int scan[REL_THREADS + 1];
  int st[8];                           // niters, best, best_it, best_root, n_eval, winning lane of the round, -, -
  unsigned char m0[VPL_SFM_MAX_TRACKS], m1[VPL_SFM_MAX_TRACKS];
};
enum { RS_NITERS = 0, RS_BEST = 1, RS_BEST_IT = 2, RS_BEST_ROOT = 3, RS_NEVAL = 4, RS_WIN_LANE = 5 };

// FMEstimatorCallback::computeError (modules/calib3d/src/fundam.cpp) for one correspondence against the squared threshold
__device__ __forceinline__ bool rel_inlier(const double (&F)[9], double x1, double y1, double x2, double y2) {
  double a = F[0] * x1 + F[1] * y1 + F[2];
  double b = F[3] * x1 + F[4] * y1 + F[5];
  double c = F[6] * x1 + F[7] * y1 + F[8];
  const double s2 = 1.0 / (a * a + b * b);
  const double d2 = x2 * a + y2 * b + c;
  a = F[0] * x2 + F[3] * y2 + F[6];
  b = F[1] * x2 + F[4] * y2 + F[7];
  c = F[2] * x2 + F[5] * y2 + F[8];
  const double s1 = 1.0 / (a * a + b * b);
  const double d1 = x1 * a + y1 * b + c;
  return fmax(d1 * d1 * s1, d2 * d2 * s2) <= REL_THRESHOLD * REL_THRESHOLD;
}

__device__ __forceinline__ double rel_det3(const double* a, const double* b, const double* c) {
  return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// The real roots of c3 x^3 + c2 x^2 + c1 x + c0 in ascending order -> their number.  A vanishing leading coefficient leaves
// the quadratic (or the linear equation); three real roots come from the trigonometric form, one from Cardano's; of a
// repeated root (discriminant exactly zero) only the simple partner is a root here.
__device__ __forceinline__ int rel_cubic(double c3, double c2, double c1, double c0, double (&x)[3]) {
  x[0] = x[1] = x[2] = 0.0;
  if (c3 == 0.0) {
    if (c2 == 0.0) {
      if (c1 == 0.0) return 0;
      x[0] = -c0 / c1;
      return 1;
    }
    const double disc = c1 * c1 - 4.0 * c2 * c0;
    if (disc < 0.0) return 0;
    if (disc == 0.0) { x[0] = -c1 / (2.0 * c2); return 1; }
    const double q = -(c1 + (c1 >= 0.0 ? 1.0 : -1.0) * sqrt(disc)) / 2.0;
    const double r0 = q / c2, r1 = c0 / q;
    x[0] = fmin(r0, r1); x[1] = fmax(r0, r1);
    return 2;
  }
  const double a = c2 / c3, b = c1 / c3, c = c0 / c3;
  const double Q = (a * a - 3.0 * b) / 9.0, R = (2.0 * a * a * a - 9.0 * a * b + 27.0 * c) / 54.0;
  const double Q3 = Q * Q * Q, d = Q3 - R * R;
  if (d > 0.0) {
    const double two_pi = 6.283185307179586476925286766559;
    const double theta = acos(fmin(1.0, fmax(-1.0, R / sqrt(Q3)))), m = -2.0 * sqrt(Q), sh = a / 3.0;
    double r0 = m * cos(theta / 3.0) - sh, r1 = m * cos((theta + two_pi) / 3.0) - sh, r2 = m * cos((theta - two_pi) / 3.0) - sh;
    double t;
    if (r1 < r0) { t = r0; r0 = r1; r1 = t; }
    if (r2 < r1) { t = r1; r1 = r2; r2 = t; }
    if (r1 < r0) { t = r0; r0 = r1; r1 = t; }
    x[0] = r0; x[1] = r1; x[2] = r2;
    return 3;
  }
  double e = cbrt(sqrt(-d) + fabs(R));
  if (R > 0.0) e = -e;
  x[0] = (e + (e != 0.0 ? Q / e : 0.0)) - a / 3.0;
  return 1;
}

// The hypotheses of one minimal sample: F[r] for the nroots real roots, in ascending lambda.
__device__ __forceinline__ int rel_seven_point(const double* pt, const int (&idx)[RELPOSE_SAMPLE], double (&F)[3][9]) {
  double a[7][9];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const double* p = pt + 4 * idx[k];
    const double x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    a[k][0] = x2 * x1; a[k][1] = x2 * y1; a[k][2] = x2;
    a[k][3] = y2 * x1; a[k][4] = y2 * y1; a[k][5] = y2;
    a[k][6] = x1; a[k][7] = y1; a[k][8] = 1.0;
  }
  // Householder on the rows: reflection k maps row k onto e_k and is kept in its place (entries k .. 8)
  double beta[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    double s = 0.0;
#pragma unroll
    for (int r = k; r < 9; ++r) s += a[k][r] * a[k][r];
    const double nx = sqrt(s);
    a[k][k] -= a[k][k] >= 0.0 ? -nx : nx;
    double vv = 0.0;
#pragma unroll
    for (int r = k; r < 9; ++r) vv += a[k][r] * a[k][r];
    beta[k] = vv > 0.0 ? 2.0 / vv : 0.0;
#pragma unroll
    for (int j = k + 1; j < 7; ++j) {
      double d = 0.0;
#pragma unroll
      for (int r = k; r < 9; ++r) d += a[k][r] * a[j][r];
      d *= beta[k];
#pragma unroll
      for (int r = k; r < 9; ++r) a[j][r] -= d * a[k][r];
    }
  }
  // the null space: Q e7, Q e8 with Q = H0 H1 .. H6
  double f1[9], f2[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) { f1[r] = r == 7 ? 1.0 : 0.0; f2[r] = r == 8 ? 1.0 : 0.0; }
#pragma unroll
  for (int k = 6; k >= 0; --k) {
    double d1 = 0.0, d2 = 0.0;
#pragma unroll
    for (int r = k; r < 9; ++r) { d1 += a[k][r] * f1[r]; d2 += a[k][r] * f2[r]; }
    d1 *= beta[k]; d2 *= beta[k];
#pragma unroll
    for (int r = k; r < 9; ++r) { f1[r] -= d1 * a[k][r]; f2[r] -= d2 * a[k][r]; }
  }
  // det(F2 + lambda G), G = F1 - F2, by rows
  double g[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) g[r] = f1[r] - f2[r];
  const double* h = f2;
  const double c0 = rel_det3(h, h + 3, h + 6);
  const double c1 = rel_det3(g, h + 3, h + 6) + rel_det3(h, g + 3, h + 6) + rel_det3(h, h + 3, g + 6);
  const double c2 = rel_det3(g, g + 3, h + 6) + rel_det3(g, h + 3, g + 6) + rel_det3(h, g + 3, g + 6);
  const double c3 = rel_det3(g, g + 3, g + 6);
  double x[3];
  const int nroots = rel_cubic(c3, c2, c1, c0, x);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 9; ++k) F[r][k] = r < nroots ? x[r] * f1[k] + (1.0 - x[r]) * f2[k] : 0.0;
  return nroots;
}

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
  // ---- the RANSAC, 256 iterations at a time
  if (tid == 0) {
    L.st[RS_NITERS] = RELPOSE_MAX_ITERS; L.st[RS_BEST] = 0; L.st[RS_BEST_IT] = -1; L.st[RS_BEST_ROOT] = -1; L.st[RS_NEVAL] = 0;
  }
  __syncthreads();
  for (int base = 0; base < RELPOSE_MAX_ITERS; base += REL_THREADS) {
    const int niters = L.st[RS_NITERS];
    if (base >= niters) break;
    const int it = base + tid;
    double F[3][9];
    int cnt[3] = {-1, -1, -1};
    if (it < niters) {
      int idx[RELPOSE_SAMPLE] = {-1, -1, -1, -1, -1, -1, -1};
      relpose_sample(q.seed, cand, it, N, idx);
      const int nroots = rel_seven_point(L.pt, idx, F);
#pragma unroll
      for (int r = 0; r < 3; ++r) cnt[r] = r < nroots ? 0 : -1;
      for (int p = 0; p < N; ++p) {
        const double x1 = L.pt[4 * p], y1 = L.pt[4 * p + 1], x2 = L.pt[4 * p + 2], y2 = L.pt[4 * p + 3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
          if (r < nroots) cnt[r] += rel_inlier(F[r], x1, y1, x2, y2) ? 1 : 0;
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) L.cnt[3 * tid + r] = cnt[r];
    __syncthreads();
    if (tid == 0) {   // the sequential rule over the round (modules/calib3d/src/ptsetreg.cpp, RANSACPointSetRegistrator::run)
      int nit = niters, best = L.st[RS_BEST], win = -1;
      for (int k = 0; k < REL_THREADS; ++k) {
        if (base + k >= nit) break;
        L.st[RS_NEVAL] = base + k + 1;
        for (int r = 0; r < 3; ++r) {
          const int good = L.cnt[3 * k + r];
          if (good > (best > RELPOSE_SAMPLE - 1 ? best : RELPOSE_SAMPLE - 1)) {
            best = good;
            L.st[RS_BEST_IT] = base + k; L.st[RS_BEST_ROOT] = r;
            win = k;
            nit = niters_after[good];
          }
        }
      }
      L.st[RS_NITERS] = nit; L.st[RS_BEST] = best; L.st[RS_WIN_LANE] = win;
    }
    __syncthreads();
    if (tid == L.st[RS_WIN_LANE]) {
      const int root = L.st[RS_BEST_ROOT];
      double n2 = 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double f = root == 0 ? F[0][k] : (root == 1 ? F[1][k] : F[2][k]);
        n2 += f * f;
      }
      const double n = sqrt(n2);
#pragma unroll
      for (int k = 0; k < 9; ++k) L.F[k] = (root == 0 ? F[0][k] : (root == 1 ? F[1][k] : F[2][k])) / n;
    }
    if (A.hyp && it < L.st[RS_NEVAL]) {
      int* h = A.hyp + (slot * RELPOSE_MAX_ITERS + it) * 3;
#pragma unroll
      for (int r = 0; r < 3; ++r) h[r] = cnt[r];
    }
    __syncthreads();
  }
  const int best_it = L.st[RS_BEST_IT];
  if (tid == 0) {
    o.iterations = L.st[RS_NITERS];
    o.best_iteration = best_it; o.best_root = L.st[RS_BEST_ROOT];
  }
  if (best_it < 0) {
    if (tid == 0) o.status = VPL_RELPOSE_NO_MODEL;
    return;
  }
  // ---- the winner's mask (findInliers), then recoverPose
  double Fw[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Fw[k] = L.F[k];
  double inl = 0.0;
  for (int p = tid; p < N; p += REL_THREADS) {
    const bool m = rel_inlier(Fw, L.pt[4 * p], L.pt[4 * p + 1], L.pt[4 * p + 2], L.pt[4 * p + 3]);
    L.m0[p] = m ? 1 : 0;
    inl += m ? 1.0 : 0.0;
  }
  inl = block_sum(inl, L.red);
  if (tid == 0) rel_decompose(L.F, L.R1, L.R2, L.t);
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
    for (int k = 0; k < 9; ++k) { Rm.m[k] = R[k]; o.F[k] = L.F[k]; }
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
