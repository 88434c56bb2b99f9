// The fundamental-matrix estimator of cv::findFundamentalMat(FM_RANSAC) as the device runs it: the hypotheses of a minimal
// sample of seven correspondences (Householder null space of the 7 x 9 system, the cubic of det(lambda F1 + (1 - lambda) F2) in
// closed form) and the symmetric epipolar inlier test.  Shared by the relative pose of the initialisation (init_relpose.h,
// threshold 0.3 / 460 on normalised coordinates) and the point tracker's rejectWithF (pt_kernels.h, F_THRESHOLD pixels on the
// virtual pinhole image): one copy of the arithmetic, FP64, every sum in a fixed order.
#pragma once
#include "vpl_math.h"
#include "init_relpose_plan.h"

namespace vpl {

// FMEstimatorCallback::computeError (modules/calib3d/src/fundam.cpp) for one correspondence against the squared threshold thr2
__device__ __forceinline__ bool rel_inlier(const double (&F)[9], double x1, double y1, double x2, double y2, double thr2) {
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
  return fmax(d1 * d1 * s1, d2 * d2 * s2) <= thr2;
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

constexpr int REL_THREADS = 256;

// what the loop keeps in LDS
struct RelRansacLds {
  double F[9];                 // the winning hypothesis, unit Frobenius norm
  int cnt[3 * REL_THREADS];    // the round's inlier counts, (iteration, root)
  int st[8];                   // niters, best, best_it, best_root, n_eval, winning lane of the round, -, -
};
enum { RS_NITERS = 0, RS_BEST = 1, RS_BEST_IT = 2, RS_BEST_ROOT = 3, RS_NEVAL = 4, RS_WIN_LANE = 5 };

// RANSACPointSetRegistrator::run (modules/calib3d/src/ptsetreg.cpp) by a work-group of REL_THREADS, every lane of which calls:
// rounds of REL_THREADS iterations, one lane each; after a round one lane replays the sequential rule over the round's counts
// in (iteration, root) order -- a hypothesis wins with good > max(best, 6), a win sets niters from the table, the loop ends at
// the first iteration >= niters.  pt [4 N] (x1, y1, x2, y2) in LDS; niters_after [N + 1]; hyp: null or [1000][3], preset to -1.
// On return (behind a barrier) R.st holds the loop's end and the winner (RS_BEST_IT < 0: none), R.F the winner.
__device__ __forceinline__ void rel_ransac_run(const double* pt, int N, unsigned long long seed, int cand, const int* niters_after,
                                               double thr2, RelRansacLds& R, int* hyp) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    R.st[RS_NITERS] = RELPOSE_MAX_ITERS; R.st[RS_BEST] = 0; R.st[RS_BEST_IT] = -1; R.st[RS_BEST_ROOT] = -1; R.st[RS_NEVAL] = 0;
  }
  __syncthreads();
  for (int base = 0; base < RELPOSE_MAX_ITERS; base += REL_THREADS) {
    const int niters = R.st[RS_NITERS];
    if (base >= niters) break;
    const int it = base + tid;
    double F[3][9];
    int cnt[3] = {-1, -1, -1};
    if (it < niters) {
      int idx[RELPOSE_SAMPLE] = {-1, -1, -1, -1, -1, -1, -1};
      relpose_sample(seed, cand, it, N, idx);
      const int nroots = rel_seven_point(pt, idx, F);
#pragma unroll
      for (int r = 0; r < 3; ++r) cnt[r] = r < nroots ? 0 : -1;
      for (int p = 0; p < N; ++p) {
        const double x1 = pt[4 * p], y1 = pt[4 * p + 1], x2 = pt[4 * p + 2], y2 = pt[4 * p + 3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
          if (r < nroots) cnt[r] += rel_inlier(F[r], x1, y1, x2, y2, thr2) ? 1 : 0;
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) R.cnt[3 * tid + r] = cnt[r];
    __syncthreads();
    if (tid == 0) {   // the sequential rule over the round (modules/calib3d/src/ptsetreg.cpp, RANSACPointSetRegistrator::run)
      int nit = niters, best = R.st[RS_BEST], win = -1;
      for (int k = 0; k < REL_THREADS; ++k) {
        if (base + k >= nit) break;
        R.st[RS_NEVAL] = base + k + 1;
        for (int r = 0; r < 3; ++r) {
          const int good = R.cnt[3 * k + r];
          if (good > (best > RELPOSE_SAMPLE - 1 ? best : RELPOSE_SAMPLE - 1)) {
            best = good;
            R.st[RS_BEST_IT] = base + k; R.st[RS_BEST_ROOT] = r;
            win = k;
            nit = niters_after[good];
          }
        }
      }
      R.st[RS_NITERS] = nit; R.st[RS_BEST] = best; R.st[RS_WIN_LANE] = win;
    }
    __syncthreads();
    if (tid == R.st[RS_WIN_LANE]) {
      const int root = R.st[RS_BEST_ROOT];
      double n2 = 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double f = root == 0 ? F[0][k] : (root == 1 ? F[1][k] : F[2][k]);
        n2 += f * f;
      }
      const double n = sqrt(n2);
#pragma unroll
      for (int k = 0; k < 9; ++k) R.F[k] = (root == 0 ? F[0][k] : (root == 1 ? F[1][k] : F[2][k])) / n;
    }
    if (hyp && it < R.st[RS_NEVAL]) {
      int* h = hyp + (size_t)it * 3;
#pragma unroll
      for (int r = 0; r < 3; ++r) h[r] = cnt[r];
    }
    __syncthreads();
  }
}

}  // namespace vpl
