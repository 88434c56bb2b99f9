// k_prior_eigen : the reference's factor of the kept block (marginalization_factor.cpp:349-357) --
//                 SelfAdjointEigenSolver of A, eigenvalues above kMargEps kept, J0 = sqrt(S) V^T, r0 = S^-1/2 V^T b --
//                 for contexts that select VPL_PRIOR_EIGEN (vpl_ba_set_prior_rule).  It runs after k_marg, reads the kept
//                 block k_marg left in mg_A / mg_b and overwrites that window's mg_J0 / mg_r0; k_marg itself is unchanged.
#pragma once
#include "ba_common.h"
#include "ba_marg.h"

namespace vpl {

constexpr int PRIOR_EIG_THREADS = 256;
constexpr int PRIOR_EIG_MAX_SWEEPS = 40;   // the oracle allows 100; kept blocks of up to 80 dims converge in about ten

// LDS layout of k_prior_eigen, shared by host (size) and device (offsets), from ONE value: the batch's largest kept size.
// Every window of the batch is laid out with the same strides; a window's own order only sets how much of them it uses.
struct PriorEigLayout {
  int m, ld, h, nblk;              // padded (even) order, odd row stride, pairs per step, 2 x 2 blocks with P <= Q
  int A, Vt, cs, d, b, sq, red;    // offsets in doubles: A (m x ld), V^T (m x ld), {c, s, t} per pair, eigenvalues, b,
                                   // signed sqrt(S) per eigenvector, reduction space
  int nd;                          // doubles in all; the ints follow
  int pq, blk, rk, flag;           // offsets in ints: (p, q) per pair, block table, rank per eigenvalue, status
  size_t bytes;
};
__host__ __device__ inline PriorEigLayout prior_eig_layout(int nmax) {
  PriorEigLayout L;
  const int n = nmax < 2 ? 2 : nmax;
  L.m = n + (n & 1);
  L.ld = L.m | 1;
  L.h = L.m / 2;
  L.nblk = L.h * (L.h + 1) / 2;
  L.A = 0;
  L.Vt = L.A + L.m * L.ld;
  L.cs = L.Vt + L.m * L.ld;
  L.d = L.cs + 3 * L.h;
  L.b = L.d + L.m;
  L.sq = L.b + L.m;
  L.red = L.sq + L.m;
  L.nd = L.red + 2 * PRIOR_EIG_THREADS;
  L.pq = 0;
  L.blk = L.pq + 2 * L.h;
  L.rk = L.blk + L.nblk;
  L.flag = L.rk + L.m;
  L.bytes = (size_t)L.nd * sizeof(double) + (size_t)(L.flag + 1) * sizeof(int);
  return L;
}

// One work-group per window.  Parallel two-sided cyclic Jacobi on the full symmetric matrix (the kept block is indefinite at
// rounding level, so neither a Cholesky start nor psd_spectral_factor applies).  Round-robin ordering: the order is padded to
// even m with an idle index, every step applies m/2 disjoint rotations, m - 1 steps make a sweep.  A step is two phases, two
// barriers: one lane per pair computes (c, s) with sym_eigen's formulas; then every 2 x 2 block (P, Q), P <= Q, becomes
// R_P^T A[P,Q] R_Q (written to both triangles, so A stays exactly symmetric) and V[:, P] <- V[:, P] R_P.  The stopping test is
// the oracle's, before every sweep, on a fixed-order block reduction; at most PRIOR_EIG_MAX_SWEEPS sweeps.  A window whose
// block holds a NaN / inf gets NaN in every entry of J0 and r0.  Eigenvalues ascending, ties by index (the solver's order);
// each eigenvector's largest component (lowest index on ties) positive.  Fixed schedule, no atomics: a window's bits do not
// depend on the batch it is solved in.
__global__ __launch_bounds__(PRIOR_EIG_THREADS) void k_prior_eigen(DevBatch B, int nmax) {
  constexpr int T = PRIOR_EIG_THREADS;
  extern __shared__ double sm[];
  const int w = blockIdx.x, tid = threadIdx.x;
  const int n = B.mg_n[w];
  if (n <= 0 || n > nmax || n > MAXKEEP) return;   // (n == 0: MARGIN_SECOND_NEW pass-through; k_marg did nothing either)
  const PriorEigLayout L = prior_eig_layout(nmax);
  const int ld = L.ld;
  const int m = n + (n & 1), h = m / 2, nb = h * (h + 1) / 2;   // this window's own schedule
  double* A = sm + L.A;
  double* Vt = sm + L.Vt;    // row k = eigenvector k
  double* cs = sm + L.cs;
  double* d = sm + L.d;
  double* b = sm + L.b;
  double* sq = sm + L.sq;
  double* red = sm + L.red;
  int* ism = reinterpret_cast<int*>(sm + L.nd);
  int* pq = ism + L.pq;
  int* blk = ism + L.blk;
  int* rk = ism + L.rk;
  const double* Ag = B.mg_A + (size_t)w * MAXKEEP * MAXKEEP;   // n x n, stride n
  const double* bg = B.mg_b + (size_t)w * MAXKEEP;
  double* J0 = B.mg_J0 + (size_t)w * MAXKEEP * MAXKEEP;
  double* r0 = B.mg_r0 + (size_t)w * MAXKEEP;

  // the symmetric matrix from the lower triangle (as the solver reads it); the idle index is a zero row and column
  for (int it = tid; it < m * m; it += T) {
    const int i = it / m, j = it % m;
    double a = 0.0;
    if (i < n && j < n) a = i >= j ? Ag[i * n + j] : Ag[j * n + i];
    A[i * ld + j] = a;
    Vt[i * ld + j] = i == j ? 1.0 : 0.0;
  }
  if (tid < m) b[tid] = tid < n ? bg[tid] : 0.0;
  for (int it = tid; it < h * h; it += T) {
    const int P = it / h, Q = it % h;
    if (P <= Q) blk[P * h - P * (P - 1) / 2 + (Q - P)] = P | Q << 8;
  }
  __syncthreads();

  bool finite = true;
  for (int sweep = 0;; ++sweep) {
    double off = 0.0, dg = 0.0;
    for (int it = tid; it < n * n; it += T) {
      const int i = it / n, j = it % n;
      const double a = A[i * ld + j];
      if (i < j) off += a * a;
      else if (i == j) dg += a * a;
    }
    red[tid] = off;
    red[T + tid] = dg;
    __syncthreads();
    for (int s = T / 2; s > 0; s >>= 1) {
      if (tid < s) { red[tid] += red[tid + s]; red[T + tid] += red[T + tid + s]; }
      __syncthreads();
    }
    off = red[0];
    dg = red[T];
    if (!(off + dg <= 1.7976931348623157e308)) { finite = false; break; }   // NaN or inf (the same value in every lane)
    if (off <= 1e-60 || off <= 1e-34 * dg || sweep == PRIOR_EIG_MAX_SWEEPS) break;
    for (int r = 0; r < m - 1; ++r) {
      if (tid < h) {   // phase 1: pair tid of step r (circle method: index m-1 fixed, the others turn)
        const int k = tid;
        const int u = k == 0 ? m - 1 : (r + k) % (m - 1);
        const int v = k == 0 ? r : (r - k + m - 1) % (m - 1);
        const int p = u < v ? u : v, q = u < v ? v : u;
        double c = 1.0, s = 0.0, t = 0.0;
        const double apq = A[p * ld + q];
        if (apq != 0.0) {
          const double theta = (A[q * ld + q] - A[p * ld + p]) / (2.0 * apq);
          t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          c = 1.0 / sqrt(t * t + 1.0);
          s = t * c;
        }
        pq[2 * k] = p;
        pq[2 * k + 1] = q;
        cs[3 * k] = c;
        cs[3 * k + 1] = s;
        cs[3 * k + 2] = t;
      }
      __syncthreads();
      for (int it = tid; it < nb + h * n; it += T) {   // phase 2: the blocks of A, then the columns of V
        if (it < nb) {
          const int P = blk[it] & 255, Q = blk[it] >> 8;
          const int p1 = pq[2 * P], q1 = pq[2 * P + 1];
          if (P == Q) {
            const double apq = A[p1 * ld + q1], t = cs[3 * P + 2];
            A[p1 * ld + p1] -= t * apq;
            A[q1 * ld + q1] += t * apq;
            A[p1 * ld + q1] = 0.0;
            A[q1 * ld + p1] = 0.0;
          } else {
            const int p2 = pq[2 * Q], q2 = pq[2 * Q + 1];
            const double c1 = cs[3 * P], s1 = cs[3 * P + 1], c2 = cs[3 * Q], s2 = cs[3 * Q + 1];
            const double m00 = A[p1 * ld + p2], m01 = A[p1 * ld + q2], m10 = A[q1 * ld + p2], m11 = A[q1 * ld + q2];
            // columns first (A R_Q), then rows (R_P^T ...), in sym_eigen's order; R = [c s; -s c]
            const double n00 = c2 * m00 - s2 * m01, n01 = s2 * m00 + c2 * m01;
            const double n10 = c2 * m10 - s2 * m11, n11 = s2 * m10 + c2 * m11;
            const double o00 = c1 * n00 - s1 * n10, o10 = s1 * n00 + c1 * n10;
            const double o01 = c1 * n01 - s1 * n11, o11 = s1 * n01 + c1 * n11;
            A[p1 * ld + p2] = o00; A[p1 * ld + q2] = o01; A[q1 * ld + p2] = o10; A[q1 * ld + q2] = o11;
            A[p2 * ld + p1] = o00; A[q2 * ld + p1] = o01; A[p2 * ld + q1] = o10; A[q2 * ld + q1] = o11;
          }
        } else {
          const int j = it - nb, k = j / n, i = j % n;
          const int p = pq[2 * k], q = pq[2 * k + 1];
          const double c = cs[3 * k], s = cs[3 * k + 1];
          const double x = Vt[p * ld + i], y = Vt[q * ld + i];
          Vt[p * ld + i] = c * x - s * y;
          Vt[q * ld + i] = s * x + c * y;
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (!finite) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int it = tid; it < n * n; it += T) J0[it] = nan;
    if (tid < n) r0[tid] = nan;
    return;
  }
  if (tid < n) d[tid] = A[tid * ld + tid];
  __syncthreads();
  if (tid < n) {
    const double di = d[tid];
    int r = 0;   // ascending, ties by index: a permutation (every d is finite here)
    for (int j = 0; j < n; ++j) r += (d[j] < di || (d[j] == di && j < tid)) ? 1 : 0;
    rk[tid] = r;
    const double* v = Vt + tid * ld;
    int jm = 0;
    double am = fabs(v[0]);
    for (int j = 1; j < n; ++j)
      if (fabs(v[j]) > am) { am = fabs(v[j]); jm = j; }
    const double sgn = v[jm] < 0.0 ? -1.0 : 1.0;
    double vb = 0.0;
    for (int j = 0; j < n; ++j) vb += v[j] * b[j];
    const bool keep = di > kMargEps;
    sq[tid] = keep ? sgn * sqrt(di) : 0.0;
    r0[r] = keep ? sgn * sqrt(1.0 / di) * vb : 0.0;
  }
  __syncthreads();
  for (int it = tid; it < n * n; it += T) {
    const int k = it / n, j = it % n;
    J0[rk[k] * n + j] = sq[k] * Vt[k * ld + j];
  }
}

}  // namespace vpl
