// Device side of the feature selector (vpl_select_features_batch; FeatureSelector::select of the reference,
// vins_estimator/src/feature_selector.cpp, and HorizonGenerator::imu, utility/selector/horizon_generator.cpp:24-68): expected-
// information greedy selection of new features over a horizon of four future frames.  FP64 throughout, every sum in a fixed order,
// no global atomics: a sequence's result has the same bits wherever it sits in a batch.
//
// The 45 x 45 matrices (five states of position, velocity, accelerometer bias) are never factored per candidate.  Every feature's
// Delta, their sums and the selection's OmegaS are non-zero only in the 12 position dimensions of states 1 .. 4 (sel_nat below).
// With those ordered last, M = [[A, B], [B^T, C]] has A (33 x 33) and B fixed for the whole call, so
//   logdet M = logdet A + logdet(S0 + U + S_sel + p Delta12),   S0 = C0 - B^T A^-1 B,  U = sum of the used features' Delta12,
// a 12 x 12 Cholesky per candidate and round.  The upper bound sum log diag(M) keeps the 33 fixed diagonal entries as one number.
//   k_sel_prep    one work-group per sequence: horizon, the four IMU pairs, Omega_kkH, the factor of A, S0
//   k_sel_info    one lane per feature (new and used): depth guess, three projections, Delta12 (packed lower triangle, 78)
//   k_sel_greedy  one work-group per sequence: U, then all kappa rounds -- ub, Cholesky and f per candidate, the reference's
//                 rules in a work-group argmax, S_sel += p Delta12
#pragma once
#include <hip/hip_runtime.h>

#include "vplines_ba.h"
#include "vpl_math.h"

namespace vpl {

constexpr int SEL_H = 4, SEL_N = 45, SEL_NA = 33, SEL_NP = 12, SEL_TRI = 78;
constexpr int SEL_PREP_THREADS = 64, SEL_INFO_THREADS = 64, SEL_GREEDY_THREADS = 256;
constexpr int SEL_WORK = 35 + 2 + SEL_TRI + SEL_NP;        // per sequence: horizon | logdet A, sum log diag A-part | S0 | diag C0
constexpr int SEL_W_LDA = 35, SEL_W_S0 = 37, SEL_W_DC = SEL_W_S0 + SEL_TRI;

// natural index of reduced index r: the 33 other dimensions in their order, then the 12 positions of states 1 .. 4
__host__ __device__ inline int sel_nat(int r) {
  if (r >= SEL_NA) { const int k = r - SEL_NA; return 9 * (1 + k / 3) + k % 3; }
  return r < 9 ? r : 9 * (1 + (r - 9) / 6) + 3 + (r - 9) % 6;
}
__host__ __device__ constexpr int sel_tri(int r, int c) { return r * (r + 1) / 2 + c; }   // r >= c

struct DevSelSeq {
  double st[33];      // P0 Q0 V0 Ba0 | P1 Q1 V1 Ba1 | acc gyr | delta_imu   (quaternions w, x, y, z)
  double hz[35];      // the caller's horizon [5][7] = position, quaternion
  int has_hz, n_imu, kappa, n_new, n_used, n_cloud;
  int feat0;          // first feature (new, then used) in the feature arrays
  int cloud0;         // first cloud point
  int prefix0, n_prefix;   // debug: ids forced first (index into the integer table)
};
struct DevSelArgs {
  vpl_sel_params par;
  const DevSelSeq* seqs;
  const double *fx, *fy, *fp;    // per feature: x, y, prob (used: prob unused)
  const int* fid;                // per feature: id (used: -1)
  const double* cloud;           // [..][3]
  const int* itab;               // prefixes
  int ftot;                      // features of the whole batch: the stride of d12
  double* work;                  // [n][SEL_WORK]
  double* omega;                 // [n][45 * 45]
  double* d12;                   // [78][ftot]
  int* vis;                      // [ftot]
  vpl_sel_result* res;           // [n]
  int* sel_id;                   // [n][VPL_SEL_MAX_FEATURES]
  double* sel_f;                 // [n][VPL_SEL_MAX_FEATURES]
  double *dbg_f, *dbg_ub;        // debug: [ftot], one round's values of every new feature
  int debug;
};

__device__ inline Q4 sel_q(const double* p) { return Q4{p[0], p[1], p[2], p[3]}; }
__device__ inline V3 sel_v(const double* p) { return V3{p[0], p[1], p[2]}; }

// Eigen's Quaternion::slerp
__device__ inline Q4 sel_slerp(Q4 a, double t, Q4 b) {
  const double one = 1.0 - 2.220446049250313e-16;
  const double d = a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z, ad = fabs(d);
  double s0, s1;
  if (ad >= one) { s0 = 1.0 - t; s1 = t; }
  else { const double th = acos(ad), st = sin(th); s0 = sin((1.0 - t) * th) / st; s1 = sin(t * th) / st; }
  if (d < 0) s1 = -s1;
  return Q4{s0 * a.w + s1 * b.w, s0 * a.x + s1 * b.x, s0 * a.y + s1 * b.y, s0 * a.z + s1 * b.z};
}

__global__ __launch_bounds__(SEL_PREP_THREADS) void k_sel_prep(DevSelArgs A) {
  const int s = blockIdx.x, t = threadIdx.x;
  const DevSelSeq& q = A.seqs[s];
  __shared__ double hz[35], Om[SEL_N * SEL_N], part[SEL_PREP_THREADS * 18], NM[18], Ab[81], W[81], T[81], LA[SEL_NA * SEL_NA], Y[SEL_NA * SEL_NP];
  double* work = A.work + (size_t)s * SEL_WORK;
  const int n = q.n_imu;
  const double dimu = q.st[32];
  // ---- the horizon: states k, k + 1 as given, k + 2 .. k + 4 by constant-a, constant-w propagation (one lane: a chain)
  if (t == 0) {
    if (q.has_hz) {
      for (int i = 0; i < 35; ++i) hz[i] = q.hz[i];
    } else {
      for (int i = 0; i < 3; ++i) { hz[i] = q.st[i]; hz[7 + i] = q.st[13 + i]; }
      for (int i = 0; i < 4; ++i) { hz[3 + i] = q.st[3 + i]; hz[10 + i] = q.st[16 + i]; }
      const V3 g{0.0, 0.0, -9.80665};
      const V3 ab = sel_v(q.st + 26) - sel_v(q.st + 10);          // a - Ba of state k
      const V3 w = sel_v(q.st + 29) * dimu;
      const Q4 qimu{1.0, w.x / 2.0, w.y / 2.0, w.z / 2.0};        // Utility::deltaQ: not normalised
      V3 v = sel_v(q.st + 20);
      for (int h = 2; h <= SEL_H; ++h) {
        V3 p = sel_v(hz + 7 * (h - 1));
        Q4 r = sel_q(hz + 7 * (h - 1) + 3);
        for (int i = 0; i < n; ++i) {
          r = qmul(r, qimu);
          const V3 qa = qrot(r, ab);
          v = v + (g + qa) * dimu;
          p = p + v * dimu + 0.5 * g * dimu * dimu + 0.5 * qa * dimu * dimu;
        }
        hz[7 * h] = p.x; hz[7 * h + 1] = p.y; hz[7 * h + 2] = p.z;
        hz[7 * h + 3] = r.w; hz[7 * h + 4] = r.x; hz[7 * h + 5] = r.y; hz[7 * h + 6] = r.z;
      }
    }
  }
  for (int i = t; i < SEL_N * SEL_N; i += SEL_PREP_THREADS) Om[i] = 0.0;
  // ---- covImu^-1 in closed form from its blocks [[a I, b I, 0], [b I, c I, 0], [0, 0, e I]]
  double c11 = 0.0, c12 = 0.0;
  for (int i = 0; i < n; ++i) { const double jkh = (double)(n - i) - 0.5; c11 += jkh * jkh; c12 += jkh; }
  const double d2 = dimu * dimu, d3 = d2 * dimu, d4 = d3 * dimu;
  const double ca = (double)n * c11 * d4 * A.par.acc_var, cb = c12 * d3 * A.par.acc_var, cc = (double)n * d2 * A.par.acc_var,
               ce = (double)n * A.par.acc_bias_var, det = ca * cc - cb * cb;
  for (int e = t; e < 81; e += SEL_PREP_THREADS) {
    const int r = e / 9, c = e % 9;
    double w = 0.0;
    if (r % 3 == c % 3) {
      const int br = r / 3, bc = c / 3;
      if (br == 0 && bc == 0) w = cc / det;
      else if (br == 1 && bc == 1) w = ca / det;
      else if (br + bc == 1) w = -cb / det;
      else if (br == 2 && bc == 2) w = 1.0 / ce;
    }
    W[e] = w;
  }
  __syncthreads();
  if (t < 35) work[t] = hz[t];
  // ---- the four IMU pairs: slerps over lanes, the lanes' sums added in lane order
  for (int h = 1; h <= SEL_H; ++h) {
    const Q4 qi = sel_q(hz + 7 * (h - 1) + 3), qj = sel_q(hz + 7 * h + 3);
    double acc[18];
    for (int k = 0; k < 18; ++k) acc[k] = 0.0;
    for (int i = t; i < n; i += SEL_PREP_THREADS) {
      const M3 R = qmat(sel_slerp(qi, (double)i / (double)n, qj));
      const double jkh = (double)(n - i) - 0.5;
      for (int k = 0; k < 9; ++k) { acc[k] += jkh * R.m[k]; acc[9 + k] += R.m[k]; }
    }
    for (int k = 0; k < 18; ++k) part[t * 18 + k] = acc[k];
    __syncthreads();
    if (t < 18) {
      double sum = 0.0;
      for (int l = 0; l < SEL_PREP_THREADS; ++l) sum += part[l * 18 + t];
      NM[t] = sum * (t < 9 ? d2 : dimu);
    }
    __syncthreads();
    for (int e = t; e < 81; e += SEL_PREP_THREADS) {          // Ablk
      const int r = e / 9, c = e % 9;
      double a = r == c ? -1.0 : 0.0;
      if (r < 3 && c >= 3 && c < 6 && r == c - 3) a = -(double)n * dimu;
      if (r < 3 && c >= 6) a = NM[3 * r + (c - 6)];
      if (r >= 3 && r < 6 && c >= 6) a = NM[9 + 3 * (r - 3) + (c - 6)];
      Ab[e] = a;
    }
    __syncthreads();
    for (int e = t; e < 81; e += SEL_PREP_THREADS) {          // tmp = Ablk^T Omega
      const int r = e / 9, c = e % 9;
      double sum = 0.0;
      for (int k = 0; k < 9; ++k) sum += Ab[9 * k + r] * W[9 * k + c];
      T[e] = sum;
    }
    __syncthreads();
    const int a0 = 9 * (h - 1), b0 = 9 * h;
    for (int e = t; e < 81; e += SEL_PREP_THREADS) {
      const int r = e / 9, c = e % 9;
      double sum = 0.0;
      for (int k = 0; k < 9; ++k) sum += T[9 * r + k] * Ab[9 * k + c];
      Om[(a0 + r) * SEL_N + a0 + c] += sum;
      Om[(a0 + r) * SEL_N + b0 + c] += T[e];
      Om[(b0 + c) * SEL_N + a0 + r] += T[e];
      Om[(b0 + r) * SEL_N + b0 + c] += W[e];
    }
    __syncthreads();
  }
  if (t < 9) Om[t * SEL_N + t] += 1.0;                        // addOmegaPrior
  __syncthreads();
  for (int i = t; i < SEL_N * SEL_N; i += SEL_PREP_THREADS) A.omega[(size_t)s * SEL_N * SEL_N + i] = Om[i];
  // ---- A = L L^T (lower triangle of Omega, as LLT reads it), Y = L^-1 B, S0 = C0 - Y^T Y
  for (int e = t; e < SEL_NA * SEL_NA; e += SEL_PREP_THREADS) {
    const int r = e / SEL_NA, c = e % SEL_NA;
    LA[e] = r >= c ? Om[sel_nat(r) * SEL_N + sel_nat(c)] : 0.0;
  }
  for (int e = t; e < SEL_NA * SEL_NP; e += SEL_PREP_THREADS) {
    const int r = e / SEL_NP, c = e % SEL_NP;
    Y[e] = Om[sel_nat(SEL_NA + c) * SEL_N + sel_nat(r)];      // lower triangle: the position rows lie below
  }
  __syncthreads();
  for (int j = 0; j < SEL_NA; ++j) {
    const double d = sqrt(LA[j * SEL_NA + j]);                // (not > 0: NaN from here on, every candidate is ineligible)
    __syncthreads();
    if (t == 0) LA[j * SEL_NA + j] = d;
    for (int i = j + 1 + t; i < SEL_NA; i += SEL_PREP_THREADS) LA[i * SEL_NA + j] /= d;
    __syncthreads();
    for (int i = j + 1 + t; i < SEL_NA; i += SEL_PREP_THREADS) {
      const double lij = LA[i * SEL_NA + j];
      for (int k = j + 1; k <= i; ++k) LA[i * SEL_NA + k] -= lij * LA[k * SEL_NA + j];
    }
    __syncthreads();
  }
  if (t < SEL_NP)
    for (int i = 0; i < SEL_NA; ++i) {
      double sum = Y[i * SEL_NP + t];
      for (int k = 0; k < i; ++k) sum -= LA[i * SEL_NA + k] * Y[k * SEL_NP + t];
      Y[i * SEL_NP + t] = sum / LA[i * SEL_NA + i];
    }
  __syncthreads();
  for (int e = t; e < SEL_NP * SEL_NP; e += SEL_PREP_THREADS) {
    const int r = e / SEL_NP, c = e % SEL_NP;
    if (r < c) continue;
    double sum = 0.0;
    for (int k = 0; k < SEL_NA; ++k) sum += Y[k * SEL_NP + r] * Y[k * SEL_NP + c];
    work[SEL_W_S0 + sel_tri(r, c)] = Om[sel_nat(SEL_NA + r) * SEL_N + sel_nat(SEL_NA + c)] - sum;
    if (r == c) work[SEL_W_DC + r] = Om[sel_nat(SEL_NA + r) * SEL_N + sel_nat(SEL_NA + r)];
  }
  if (t == 0) {
    double ld = 0.0, lu = 0.0;
    for (int j = 0; j < SEL_NA; ++j) { ld += log(LA[j * SEL_NA + j]); lu += log(Om[sel_nat(j) * SEL_N + sel_nat(j)]); }
    work[SEL_W_LDA] = 2.0 * ld;
    work[SEL_W_LDA + 1] = lu;
  }
}

// PinholeCamera::spaceToPlane with the radtan distortion; no sign test on the depth, as the reference
__device__ inline void sel_project(const vpl_sel_params& P, V3 u, double* px, double* py) {
  const double x = u.x / u.z, y = u.y / u.z;
  const double mx2 = x * x, my2 = y * y, mxy = x * y, rho2 = mx2 + my2, rad = P.k1 * rho2 + P.k2 * rho2 * rho2;
  const double dx = x * rad + 2.0 * P.p1 * mxy + P.p2 * (rho2 + 2.0 * mx2), dy = y * rad + 2.0 * P.p2 * mxy + P.p1 * (rho2 + 2.0 * my2);
  *px = P.fx * (x + dx) + P.cx;
  *py = P.fy * (y + dy) + P.cy;
}
// FeatureSelector::inFOV: std::round, border 0 (a pixel that is not finite or far outside int's range is outside)
__device__ inline bool sel_in_fov(const vpl_sel_params& P, double px, double py) {
  if (!(fabs(px) <= 1e9) || !(fabs(py) <= 1e9)) return false;
  const int u = (int)round(px), v = (int)round(py);
  return 0 <= u && u < P.width && 0 <= v && v < P.height;
}
__device__ inline M3 sel_inv3(const M3& m) {      // Eigen's 3 x 3 inverse: the cofactors over the determinant
  auto cof = [&](int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m.m[3 * i1 + j1] * m.m[3 * i2 + j2] - m.m[3 * i1 + j2] * m.m[3 * i2 + j1];
  };
  const double det = m.m[0] * cof(0, 0) + m.m[3] * cof(1, 0) + m.m[6] * cof(2, 0);
  M3 o;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o.m[3 * i + j] = cof(j, i) / det;
  return o;
}

__global__ __launch_bounds__(SEL_INFO_THREADS) void k_sel_info(DevSelArgs A) {
  const int s = blockIdx.y, k = blockIdx.x * SEL_INFO_THREADS + threadIdx.x;
  const DevSelSeq& q = A.seqs[s];
  if (k >= q.n_new + q.n_used) return;
  const int g = q.feat0 + k;
  const double* hz = A.work + (size_t)s * SEL_WORK;
  const double x = A.fx[g], y = A.fy[g];
  // depth guess: the nearest cloud point in (x, y), the lowest index on an exact tie; 1.0 without a cloud
  double depth = 1.0, best = 0.0;
  for (int i = 0; i < q.n_cloud; ++i) {
    const double* c = A.cloud + 3 * (size_t)(q.cloud0 + i);
    const double dx = c[0] - x, dy = c[1] - y, d = dx * dx + dy * dy;
    if (i == 0 || d < best) { best = d; depth = c[2]; }
  }
  const Q4 qic = sel_q(A.par.q_ic);
  const V3 tic = sel_v(A.par.t_ic);
  const Q4 Q1 = sel_q(hz + 7 + 3), q1 = qmul(Q1, qic);
  const V3 t1 = sel_v(hz + 7) + qrot(Q1, tic);
  const double nb = sqrt(x * x + y * y + 1.0);
  const V3 b{x / nb, y / nb, 1.0 / nb};                      // Eigen's normalized() divides
  const V3 pell = t1 + qrot(q1, b * depth);
  M3 Ch[SEL_H];
  M3 EtE;
  for (int i = 0; i < 9; ++i) EtE.m[i] = 0.0;
  int nvis = 0;
#pragma unroll
  for (int h = 2; h <= SEL_H; ++h) {
    const Q4 Qh = sel_q(hz + 7 * h + 3), qh = qmul(Qh, qic);
    const V3 th = sel_v(hz + 7 * h) + qrot(Qh, tic);
    V3 u = qrot(qinv(qh), pell - th);
    const double nu = norm(u);
    u = V3{u.x / nu, u.y / nu, u.z / nu};
    double px, py;
    sel_project(A.par, u, &px, &py);
    const bool ok = sel_in_fov(A.par, px, py);
    const M3 Bh = mul(skew(u), qmat(qinv(qmul(qh, qic))));    // q_IC applied twice, as the reference writes it
    const M3 C = mulTA(Bh, Bh);
    for (int i = 0; i < 9; ++i) { Ch[h - 1].m[i] = ok ? C.m[i] : 0.0; }
    if (ok) { for (int i = 0; i < 9; ++i) EtE.m[i] += C.m[i]; ++nvis; }
  }
  A.vis[g] = nvis > 0;
  if (nvis == 0) {      // no matrix: never a candidate, nothing to add as a used feature
    for (int e = 0; e < SEL_TRI; ++e) A.d12[(size_t)e * A.ftot + g] = 0.0;
    return;
  }
  {
    const M3 Bh = mul(skew(b), qmat(qinv(qmul(q1, qic))));
    Ch[0] = mulTA(Bh, Bh);
    for (int i = 0; i < 9; ++i) EtE.m[i] += Ch[0].m[i];
  }
  const M3 Wm = sel_inv3(EtE);
#pragma unroll
  for (int j = 0; j < SEL_H; ++j)
#pragma unroll
    for (int i = j; i < SEL_H; ++i) {
      const M3 D = mul(mul(Ch[i], Wm), transpose(Ch[j]));      // Ci W Cj^T
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (i == j && c > r) continue;
          const double v = i == j ? Ch[i].m[3 * r + c] - D.m[3 * r + c] : -D.m[3 * r + c];
          A.d12[(size_t)sel_tri(3 * i + r, 3 * j + c) * A.ftot + g] = v;
        }
    }
}

// sum of logarithms as one logarithm: the factors' mantissas multiplied, their exponents added (12 factors: the product of the
// mantissas stays above 2^-12).  One log call per sum instead of one per term keeps k_sel_greedy's registers for the triangle.
struct SelLogSum {
  double m = 1.0;
  int e = 0;
  __device__ __forceinline__ void mul(double x) { int k; m *= frexp(x, &k); e += k; }
  __device__ __forceinline__ double value() const { return log(m) + (double)e * 0.6931471805599453094; }
};

// 12 x 12 Cholesky over the packed lower triangle in registers (every index a constant once unrolled): 2 sum log L_ii = sum log of
// the pivots, false at a pivot that is not finite or not > 0
__device__ __forceinline__ bool sel_chol12(double (&a)[SEL_TRI], double* logdet) {
  SelLogSum ls;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < SEL_NP; ++j) {
    double x = a[sel_tri(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) x -= a[sel_tri(j, k)] * a[sel_tri(j, k)];
    ok = ok && x > 0.0 && x <= 1.79769313486231570e308;
    ls.mul(x);
    const double inv = 1.0 / sqrt(x);
#pragma unroll
    for (int i = j + 1; i < SEL_NP; ++i) {
      double v = a[sel_tri(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= a[sel_tri(i, k)] * a[sel_tri(j, k)];
      a[sel_tri(i, j)] = v * inv;
    }
  }
  *logdet = ls.value();
  return ok;
}

// candidate states of k_sel_greedy
constexpr unsigned char SEL_CAND = 0, SEL_INVISIBLE = 1, SEL_TAKEN = 2;

__global__ __launch_bounds__(SEL_GREEDY_THREADS) void k_sel_greedy(DevSelArgs A) {
  const int s = blockIdx.x, t = threadIdx.x;
  const DevSelSeq& q = A.seqs[s];
  const int nn = q.n_new, g0 = q.feat0;
  const double* work = A.work + (size_t)s * SEL_WORK;
  __shared__ double ub[VPL_SEL_MAX_FEATURES], fv[VPL_SEL_MAX_FEATURES];
  __shared__ int id[VPL_SEL_MAX_FEATURES];
  __shared__ unsigned char state[VPL_SEL_MAX_FEATURES], skip[VPL_SEL_MAX_FEATURES];   // skip: set aside in this round's argmax
  __shared__ double S0U[SEL_TRI], Ssel[SEL_TRI], DU[SEL_NP], base[SEL_TRI], baseD[SEL_NP];   // base = S0U + Ssel, baseD = DU + diag Ssel
  __shared__ double rf[SEL_GREEDY_THREADS], ru[SEL_GREEDY_THREADS];
  __shared__ int ri[SEL_GREEDY_THREADS];
  __shared__ int n_inel, n_invis, winner;
  const double ldA = work[SEL_W_LDA], luA = work[SEL_W_LDA + 1];
  if (t == 0) { n_inel = 0; n_invis = 0; winner = -1; }
  __syncthreads();
  {
    int inv = 0;
    for (int c = t; c < nn; c += SEL_GREEDY_THREADS) {
      id[c] = A.fid[g0 + c];
      const bool v = A.vis[g0 + c] != 0;
      state[c] = v ? SEL_CAND : SEL_INVISIBLE;
      inv += v ? 0 : 1;
    }
    if (inv) atomicAdd(&n_invis, inv);
  }
  // U: the used features' information, added one after the other in list order (an invisible one holds zeros)
  if (t < SEL_TRI) {
    double v = work[SEL_W_S0 + t];
    for (int k = 0; k < q.n_used; ++k) v += A.d12[(size_t)t * A.ftot + g0 + nn + k];
    S0U[t] = v;
    Ssel[t] = 0.0;
  } else if (t < SEL_TRI + SEL_NP) {
    const int r = t - SEL_TRI;
    double v = work[SEL_W_DC + r];
    for (int k = 0; k < q.n_used; ++k) v += A.d12[(size_t)sel_tri(r, r) * A.ftot + g0 + nn + k];
    DU[r] = v;
  }
  __syncthreads();
  // what every evaluation starts from, in the reference's order of sums: (Omega + OmegaS) + p Delta
  auto refresh = [&]() {
    if (t < SEL_TRI) {
      base[t] = S0U[t] + Ssel[t];
      for (int r = 0; r < SEL_NP; ++r)
        if (sel_tri(r, r) == t) baseD[r] = DU[r] + Ssel[t];
    }
  };
  refresh();
  __syncthreads();
  // debug: a forced prefix of selections, in its order
  for (int k = 0; k < q.n_prefix; ++k) {
    const int want = A.itab[q.prefix0 + k];
    for (int c = t; c < nn; c += SEL_GREEDY_THREADS)
      if (id[c] == want && state[c] == SEL_CAND) winner = c;      // (ids are distinct: one writer)
    __syncthreads();
    const int w = winner;
    if (w >= 0 && t < SEL_TRI) Ssel[t] += A.fp[g0 + w] * A.d12[(size_t)t * A.ftot + g0 + w];
    refresh();
    __syncthreads();
    if (t == 0) { if (w >= 0) state[w] = SEL_TAKEN; winner = -1; }
    __syncthreads();
  }
  const int rounds = A.debug ? 1 : min(q.kappa, nn);
  int n_sel = 0;
  for (int round = 0; round < rounds; ++round) {
    int inel = 0;
    for (int c = t; c < nn; c += SEL_GREEDY_THREADS) {
      if (state[c] != SEL_CAND) continue;
      const double p = A.fp[g0 + c];
      double dg[SEL_NP];      // the twelve diagonal entries first, all in flight at once: ub needs nothing else
#pragma unroll
      for (int r = 0; r < SEL_NP; ++r) dg[r] = A.d12[(size_t)sel_tri(r, r) * A.ftot + g0 + c];
      SelLogSum us;
      bool upos = true;
#pragma unroll
      for (int r = 0; r < SEL_NP; ++r) {
        const double v = baseD[r] + p * dg[r];
        upos = upos && v > 0.0;
        us.mul(v);
      }
      const double u = upos ? luA + us.value() : __builtin_nan("");
      __builtin_amdgcn_sched_barrier(0);      // the triangle's 78 loads stay behind ub: hoisted above it they cost scratch
      double a[SEL_TRI];
#pragma unroll
      for (int e = 0; e < SEL_TRI; ++e) a[e] = base[e] + p * A.d12[(size_t)e * A.ftot + g0 + c];
      double ld;
      const bool ok = sel_chol12(a, &ld);
      const double f = ldA + ld;
      const bool fin = ok && f == f && fabs(f) <= 1.79769313486231570e308;
      ub[c] = u;
      fv[c] = fin ? f : __builtin_nan("");
      skip[c] = 0;
      inel += fin ? 0 : 1;
    }
    if (inel) atomicAdd(&n_inel, inel);
    __syncthreads();
    if (A.debug) break;
    // the reference's rules: the largest f that is > -1.0, ties to the larger ub; equal ub collapse to the highest id (std::map),
    // so a winner that shares its ub with a candidate of a higher id was never in the map: it is set aside for this round and
    // the argmax is taken again
    int w;
    for (;;) {
      double bf = -1.0, bu = 0.0;
      int bi = -1;
      for (int c = t; c < nn; c += SEL_GREEDY_THREADS) {
        if (state[c] != SEL_CAND || skip[c]) continue;
        const double f = fv[c], u = ub[c];
        if (!(f > -1.0)) continue;
        if (bi < 0 || f > bf || (f == bf && (u > bu || (u == bu && id[c] > id[bi])))) { bf = f; bu = u; bi = c; }
      }
      rf[t] = bf; ru[t] = bu; ri[t] = bi;
      __syncthreads();
      for (int h = SEL_GREEDY_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) {
          const int o = ri[t + h], m = ri[t];
          if (o >= 0 && (m < 0 || rf[t + h] > rf[t] || (rf[t + h] == rf[t] && (ru[t + h] > ru[t] || (ru[t + h] == ru[t] && id[o] > id[m]))))) {
            rf[t] = rf[t + h]; ru[t] = ru[t + h]; ri[t] = o;
          }
        }
        __syncthreads();
      }
      w = ri[0];
      if (w < 0) break;
      int hidden = 0;
      for (int o = t; o < nn; o += SEL_GREEDY_THREADS) hidden |= state[o] == SEL_CAND && ub[o] == ub[w] && id[o] > id[w];
      hidden = __syncthreads_or(hidden);
      if (!hidden) break;
      if (t == 0) skip[w] = 1;
      __syncthreads();
    }
    if (w < 0) break;      // nothing changes any more: every later round would select nothing either
    if (t < SEL_TRI) Ssel[t] += A.fp[g0 + w] * A.d12[(size_t)t * A.ftot + g0 + w];
    refresh();
    if (t == 0) {
      state[w] = SEL_TAKEN;
      A.sel_id[(size_t)s * VPL_SEL_MAX_FEATURES + n_sel] = id[w];
      A.sel_f[(size_t)s * VPL_SEL_MAX_FEATURES + n_sel] = rf[0];
    }
    ++n_sel;
    __syncthreads();
  }
  if (A.debug)
    for (int c = t; c < nn; c += SEL_GREEDY_THREADS) {
      const bool cand = state[c] == SEL_CAND;
      A.dbg_f[g0 + c] = cand ? fv[c] : __builtin_nan("");
      A.dbg_ub[g0 + c] = cand ? ub[c] : __builtin_nan("");
    }
  if (t == 0) {
    vpl_sel_result r;
    r.n_selected = n_sel;
    r.n_invisible = n_invis;
    r.n_ineligible = n_inel;
    r.n_candidates = nn - n_invis;
    A.res[s] = r;
  }
}

// ---- the session's side (vpl_odo_select): state k and the cloud come from the resident store, not from the caller ------------
// tab: per batch entry [3] = the session's sequence, where its list starts in tab, its length (= the entry's n_cloud); a list
// entry is track | start frame << 20, the tracks the host's filter let through (initKDTree, feature_selector.cpp:561-566).
struct DevSelGather {
  const double *pobs, *invd, *pose, *sb, *ex;   // of the OdoStore (csrc/ba_odo.h): [seq][maxPT][11][3] [seq][maxPT] [seq][77] [seq][99] [seq][7]
  int maxPT;
  const int* tab;
};
constexpr int SEL_CLOUD_THREADS = 256;
// One work-group per batch entry, before k_sel_prep: state k = slot 10 of the store into the entry's record, and every listed
// track's first observation, scaled to its depth, through the world into camera k + 1 and normalised (no sign test, as there).
__global__ __launch_bounds__(SEL_CLOUD_THREADS) void k_sel_cloud(DevSelArgs A, DevSelGather G, DevSelSeq* seqs, double* cloud) {
  const int b = blockIdx.x, t = threadIdx.x;
  const int seq = G.tab[3 * b], l0 = G.tab[3 * b + 1], n = G.tab[3 * b + 2];
  DevSelSeq& q = seqs[b];
  const double* pose = G.pose + (size_t)seq * 77;
  const double* sb = G.sb + (size_t)seq * 99;
  if (t < 3) { q.st[t] = pose[70 + t]; q.st[7 + t] = sb[90 + t]; q.st[10 + t] = sb[93 + t]; }
  if (t < 4) q.st[3 + t] = pose[70 + (t == 0 ? 6 : 2 + t)];          // the store keeps x, y, z, w
  const Q4 qic_s = qpose(G.ex + (size_t)seq * 7), qic = sel_q(A.par.q_ic), Q1 = sel_q(q.st + 16);
  const V3 tic_s = sel_v(G.ex + (size_t)seq * 7), tic = sel_v(A.par.t_ic), P1 = sel_v(q.st + 13);
  for (int j = t; j < n; j += SEL_CLOUD_THREADS) {
    const int e = G.tab[l0 + j], tr = e & 0xFFFFF, f = e >> 20;
    const size_t ti = (size_t)seq * G.maxPT + tr;
    const double depth = 1.0 / G.invd[ti];
    const V3 pi = sel_v(G.pobs + ti * 33) * depth;
    const V3 w = qrot(qpose(pose + 7 * f), qrot(qic_s, pi) + tic_s) + sel_v(pose + 7 * f);
    const V3 pc = qrot(qinv(qic), qrot(qinv(Q1), w - P1) - tic);
    double* o = cloud + 3 * (size_t)(q.cloud0 + j);
    o[0] = pc.x / pc.z; o[1] = pc.y / pc.z; o[2] = depth;
  }
}

}  // namespace vpl
