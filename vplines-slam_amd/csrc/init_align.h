// Visual-inertial alignment on the device (vpl_init_align_batch): solveGyroscopeBias, LinearAlignment, RefineGravity
// (vins_estimator/src/initial/initial_aligment.cpp:3-207), the state change of Estimator::visualInitialAlign
// (estimator.cpp:525-583) and Utility::g2R (utility.cpp:3-13).  The pre-integrations around them are k_preintegrate's.
//   k_init_gyro_bias  one work-group per sequence: the 3 x 3 normal equations summed in frame order by one lane, delta_bg, and the
//                     linearisation gyroscope bias of every job of the re-propagation (image intervals: Bgs[0], window interval
//                     i: Bgs[i]);
//   k_init_align      one work-group per sequence: the two dense systems assembled and solved in LDS, the state change.
// Nothing here depends on where a sequence sits in the batch or on what else the batch holds, except the row stride of the LDS
// matrix (the launch's largest order), which no arithmetic sees.
#pragma once
#include "vplines_ba.h"
#include "vpl_math.h"
#include "ba_types.h"
#include "ba_odo.h"

namespace vpl {

constexpr int INIT_MAXF = VPL_INIT_MAX_FRAMES;
constexpr int INIT_THREADS = 256;
constexpr int INIT_NMAX = 3 * INIT_MAXF + 4;   // LinearAlignment's order at the cap: 124

// One sequence as the kernels read it.  frame0: its first row in the R / T arrays; job0: its first image job (image job j is
// the interval that ends in image frame j + 1); wjob0: its first window job (window job i - 1 is window interval i).
struct DevInitSeq {
  int F, frame0, job0, wjob0;
  int key[VPL_NFRAMES];
  int pad_;
  double tic[3], bas[VPL_NFRAMES * 3], bgs[VPL_NFRAMES * 3];
};

// Per image interval i (frames i, i + 1), in LDS.  Fixed part: what does not change between the five solves; derived part: the
// gravity columns and the right-hand side of the solve at hand.
constexpr int IR_DT = 0, IR_RIT = 1, IR_RR = 10, IR_DT3 = 19, IR_BP0 = 22, IR_DV = 25;   // dt | R_i^T | R_i^T R_j | R_i^T (T_j - T_i) / 100 | delta_p + R_i^T R_j tic - tic | delta_v
constexpr int IR_GP = 28, IR_GV = 37, IR_BP = 46, IR_BV = 49;                          // 3 x 3 (ng columns used) | 3 x 3 | rhs rows 0..2 | rhs rows 3..5
constexpr int INIT_REC = 52;

// LDS of k_init_align, in doubles: records | x | the column being eliminated | small state | the matrix.  Rows 0 .. n - 1 of the
// matrix are A's lower triangle, row n is b; the row stride ld is the launch's largest order, so every sequence of a launch
// agrees with the host about where the matrix ends.
constexpr int IL_REC = 0, IL_X = IL_REC + (INIT_MAXF - 1) * INIT_REC, IL_COL = IL_X + 128, IL_MISC = IL_COL + 128, IL_A = IL_MISC + 32;
constexpr int IM_G0 = 0, IM_LXLY = 3, IM_FAIL = 9;
__host__ __device__ constexpr size_t init_lds_bytes(int ld) { return (size_t)(IL_A + (ld + 1) * ld) * sizeof(double); }
static_assert(init_lds_bytes(INIT_NMAX) <= 159 * 1024, "k_init_align's LDS at the cap of 40 image frames");

__device__ __forceinline__ M3 init_load33(const double* p) { return M3{{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]}}; }
__device__ __forceinline__ V3 init_load3(const double* p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ void init_store33(double* p, const M3& A) {
#pragma unroll
  for (int k = 0; k < 9; ++k) p[k] = A.m[k];
}
__device__ __forceinline__ void init_store3(double* p, V3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
// Eigen's normalized(): v / sqrt(v . v) when that is positive
__device__ __forceinline__ V3 init_normalized(V3 v) {
  const double n2 = dot(v, v);
  if (n2 > 0.0) { const double n = sqrt(n2); return V3{v.x / n, v.y / n, v.z / n}; }
  return v;
}
__device__ __forceinline__ bool init_finite3(V3 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// ---- solveGyroscopeBias (:3-37) ---------------------------------------------------------------------------------------------
// pre1: the image pre-integrations under the input's linearisation bias (k_preintegrate carries the 15 x 15 jacobian out in the
// sqrt_info slot).  lbg3 [jobs][3]: the gyroscope bias each job of the re-propagation is linearised at.
__global__ __launch_bounds__(64) void k_init_gyro_bias(const DevInitSeq* seqs, const double* Rall, const DevPreint* pre1, double* lbg3,
                                                       vpl_init_result* out) {
  const DevInitSeq& q = seqs[blockIdx.x];
  __shared__ double dbg[3];
  if (threadIdx.x == 0) {
    M3 A{{0, 0, 0, 0, 0, 0, 0, 0, 0}};
    V3 b{0, 0, 0};
    for (int i = 0; i + 1 < q.F; ++i) {
      const M3 Ri = init_load33(Rall + (size_t)(q.frame0 + i) * 9), Rj = init_load33(Rall + (size_t)(q.frame0 + i + 1) * 9);
      const Q4 qij = odo_mat2q(mulTA(Ri, Rj));
      const DevPreint& p = pre1[q.job0 + i];
      M3 J;   // jacobian.block<3, 3>(O_R, O_BG)
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) J.m[3 * r + cc] = p.sqrt_info[(3 + r) * 15 + 12 + cc];
      const Q4 e = qmul(qinv(Q4{p.dq[3], p.dq[0], p.dq[1], p.dq[2]}), qij);
      const V3 tb{2.0 * e.x, 2.0 * e.y, 2.0 * e.z};
      const M3 JtJ = mulTA(J, J);
      const V3 Jtb = mulT(J, tb);
#pragma unroll
      for (int k = 0; k < 9; ++k) A.m[k] += JtJ.m[k];
      b = b + Jtb;
    }
    // A.ldlt().solve(b), unpivoted, on the lower triangle
    const double d0 = A.m[0], l10 = A.m[3] / d0, l20 = A.m[6] / d0;
    const double d1 = A.m[4] - l10 * A.m[3], l21 = (A.m[7] - l20 * A.m[3]) / d1;
    const double d2 = A.m[8] - l20 * A.m[6] - l21 * (l21 * d1);
    const double y0 = b.x, y1 = b.y - l10 * y0, y2 = b.z - l20 * y0 - l21 * y1;
    const double x2 = y2 / d2, x1 = y1 / d1 - l21 * x2, x0 = y0 / d0 - l10 * x1 - l20 * x2;
    dbg[0] = x0; dbg[1] = x1; dbg[2] = x2;
    vpl_init_result& o = out[blockIdx.x];
    o.delta_bg[0] = x0; o.delta_bg[1] = x1; o.delta_bg[2] = x2;
  }
  __syncthreads();
  // repropagate(0, Bgs[0]) of every image interval (:32-36), repropagate(0, Bgs[i]) of the window's (estimator.cpp:548-551)
  for (int j = threadIdx.x; j < 3 * (q.F - 1); j += 64) lbg3[(size_t)q.job0 * 3 + j] = q.bgs[j % 3] + dbg[j % 3];
  for (int j = threadIdx.x; j < 3 * VPL_WINDOW_SIZE; j += 64) lbg3[(size_t)q.wjob0 * 3 + j] = q.bgs[3 + j] + dbg[j % 3];
}

// ---- the dense systems --------------------------------------------------------------------------------------------------------
// Element (k, l) of an interval's tmp_A | tmp_b (6 rows): local columns 0..2 the velocity of frame i, 3..5 of frame i + 1,
// 6 .. 5 + ng the gravity (ng = 3: LinearAlignment, 2: RefineGravity's tangent plane), 6 + ng the scale, 7 + ng the right-hand side
__device__ __forceinline__ double init_elem(const double* r, int k, int l, int ng) {
  const bool top = k < 3;
  const int kk = top ? k : k - 3;
  if (l < 3) return l == kk ? (top ? -r[IR_DT] : -1.0) : 0.0;
  if (l < 6) return top ? 0.0 : r[IR_RR + 3 * kk + (l - 3)];
  if (l < 6 + ng) return r[(top ? IR_GP : IR_GV) + 3 * kk + (l - 6)];
  if (l == 6 + ng) return top ? r[IR_DT3 + kk] : 0.0;
  return r[(top ? IR_BP : IR_BV) + kk];
}
// Assembly of A's lower triangle and of b (row n) into LDS: one owner per entry, the contributing intervals -- at most two in
// the block-tridiagonal part, all F - 1 in the arrow's border and corner -- added in increasing order; then the entry times 1000.
// acc: RefineGravity's A and b, which the reference zeroes once before its four rounds: the entry starts from what the round
// before left (first: from zero) and what it becomes is kept for the next round.
__device__ __forceinline__ void init_assemble(const double* rec, double* A, int ld, int F, int ng, double* acc, bool first) {
  const int m = 3 * F, n = m + ng + 1;
  for (int idx = threadIdx.x; idx < (n + 1) * n; idx += INIT_THREADS) {
    const int r = idx / n, c = idx - r * n;
    if (c > r) continue;
    const int fr = r < m ? r / 3 : -1, fc = c / 3;   // (c <= r: when r is a velocity row so is c)
    int lo = 0, hi = F - 2;
    if (r < m) { lo = max(fr - 1, 0); hi = min(fc, F - 2); }
    else if (c < m) { lo = max(fc - 1, 0); hi = min(fc, F - 2); }
    double a = (acc && !first) ? acc[(size_t)r * ld + c] : 0.0;
    for (int i = lo; i <= hi; ++i) {
      const double* ri = rec + i * INIT_REC;
      const int la = r < m ? (fr - i) * 3 + r % 3 : 6 + (r - m);
      const int lb = c < m ? (fc - i) * 3 + c % 3 : 6 + (c - m);
      double t = 0.0;
      for (int k = 0; k < 6; ++k) t += init_elem(ri, k, la, ng) * init_elem(ri, k, lb, ng);
      a += t;
    }
    a *= 1000.0;
    A[r * ld + c] = a;
    if (acc) acc[(size_t)r * ld + c] = a;
  }
}
// Right-looking LDL^T without pivoting on rows 0 .. n - 1, row n (b) carried along, so that it ends as D^-1 L^-1 b; then
// L^T x = that, column by column.  One column per step, the trailing update spread over the group as 16 x 16.
__device__ __forceinline__ void init_solve(double* A, int ld, int n, double* col, double* x) {
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  for (int j = 0; j < n; ++j) {
    const double d = A[j * ld + j];
    for (int i = j + 1 + threadIdx.x; i <= n; i += INIT_THREADS) {
      const double t = A[i * ld + j];
      col[i] = t;
      A[i * ld + j] = t / d;
    }
    __syncthreads();
    for (int i = j + 1 + ty; i <= n; i += 16) {
      const double li = A[i * ld + j];
      const int kend = i < n ? i : n - 1;
      for (int k = j + 1 + tx; k <= kend; k += 16) A[i * ld + k] -= li * col[k];
    }
    __syncthreads();
  }
  for (int k = threadIdx.x; k < n; k += INIT_THREADS) x[k] = A[n * ld + k];
  __syncthreads();
  for (int j = n - 1; j > 0; --j) {
    const double xj = x[j];
    for (int k = threadIdx.x; k < j; k += INIT_THREADS) x[k] -= A[j * ld + k] * xj;
    __syncthreads();
  }
}

// Eigen's Quaternion::FromTwoVectors(a, b).  (Its branch for a = -b takes the axis from an SVD; here, for that set of measure
// zero, the axis is a x e_x or a x e_y.)
__device__ __forceinline__ Q4 init_from_two_vectors(V3 a, V3 b) {
  const V3 v0 = init_normalized(a), v1 = init_normalized(b);
  const double c = dot(v1, v0);
  if (c < -1.0 + 1e-12) {
    V3 ax = cross(v0, V3{1, 0, 0});
    if (dot(ax, ax) < 1e-6) ax = cross(v0, V3{0, 1, 0});
    ax = init_normalized(ax);
    return Q4{0.0, ax.x, ax.y, ax.z};
  }
  const V3 ax = cross(v0, v1);
  const double s = sqrt((1.0 + c) * 2.0), inv = 1.0 / s;
  return Q4{s * 0.5, ax.x * inv, ax.y * inv, ax.z * inv};
}

// pre3: the re-propagated pre-integrations (image jobs, then window jobs); acc [sequence][(ld + 1) * ld]: RefineGravity's
// accumulated system.  Dynamic LDS: init_lds_bytes(ld), ld >= the largest 3 F + 4 of the launch.
__global__ __launch_bounds__(INIT_THREADS) void k_init_align(const DevInitSeq* seqs, const double* Rall, const double* Tall,
                                                             const DevPreint* pre3, double* acc_all, int ld, double g_norm,
                                                             vpl_init_result* out) {
  extern __shared__ double init_lds[];
  double* rec = init_lds + IL_REC;
  double* xs = init_lds + IL_X;
  double* col = init_lds + IL_COL;
  double* misc = init_lds + IL_MISC;
  double* A = init_lds + IL_A;
  const DevInitSeq& q = seqs[blockIdx.x];
  vpl_init_result& o = out[blockIdx.x];
  double* acc = acc_all + (size_t)blockIdx.x * (ld + 1) * ld;
  const int tid = threadIdx.x, F = q.F, m = 3 * F, nI = F - 1;
  const double* Rq = Rall + (size_t)q.frame0 * 9;
  const double* Tq = Tall + (size_t)q.frame0 * 3;
  const double G = sqrt(g_norm * g_norm);   // G.norm()

  // ---- the intervals' records, with LinearAlignment's gravity columns and right-hand side (:142-157)
  if (tid < nI) {
    double* r = rec + tid * INIT_REC;
    const M3 Ri = init_load33(Rq + tid * 9), Rj = init_load33(Rq + (tid + 1) * 9);
    const V3 Ti = init_load3(Tq + tid * 3), Tj = init_load3(Tq + (tid + 1) * 3), tic = init_load3(q.tic);
    const DevPreint& p = pre3[q.job0 + tid];
    const double dt = p.sum_dt;
    const M3 RiT = transpose(Ri), RR = mulTA(Ri, Rj);
    const V3 dT = mulT(Ri, Tj - Ti);
    const V3 bp = init_load3(p.dp) + mul(RR, tic) - tic;
    r[IR_DT] = dt;
    init_store33(r + IR_RIT, RiT);
    init_store33(r + IR_RR, RR);
    init_store3(r + IR_DT3, V3{dT.x / 100.0, dT.y / 100.0, dT.z / 100.0});
    init_store3(r + IR_BP0, bp);
    init_store3(r + IR_DV, init_load3(p.dv));
#pragma unroll
    for (int k = 0; k < 9; ++k) { r[IR_GP + k] = RiT.m[k] * dt * dt / 2; r[IR_GV + k] = RiT.m[k] * dt; }
    init_store3(r + IR_BP, bp);
    init_store3(r + IR_BV, init_load3(p.dv));
  }
  if (tid == 0) {
    o.ok = 0; o.fail = 0;
    misc[IM_FAIL] = 0.0;
  }
  __syncthreads();

  // ---- a. LinearAlignment (:125-187)
  init_assemble(rec, A, ld, F, 3, nullptr, true);
  __syncthreads();
  init_solve(A, ld, m + 4, col, xs);
  if (tid == 0) {
    const V3 g{xs[m], xs[m + 1], xs[m + 2]};
    const double s = xs[m + 3] / 100.0, gn = norm(g);
    int fail = 0;
    if (!isfinite(gn) || !isfinite(s)) fail |= VPL_INIT_FAIL_NONFINITE;
    if (fabs(gn - G) > 1.0) fail |= VPL_INIT_FAIL_GRAVITY;
    if (s < 0) fail |= VPL_INIT_FAIL_SCALE;
    init_store3(o.g_linear, g);
    o.s_linear = s;
    o.fail = fail;
    misc[IM_FAIL] = fail ? 1.0 : 0.0;
    init_store3(misc + IM_G0, init_normalized(g) * G);   // RefineGravity's g0 (:57)
  }
  __syncthreads();
  if (misc[IM_FAIL] != 0.0) return;   // (the same for the whole group)

  // ---- b. RefineGravity (:55-123)
  for (int round = 0; round < 4; ++round) {
    if (tid == 0) {   // TangentBasis (:40-53)
      const V3 g0 = init_load3(misc + IM_G0), a = init_normalized(g0);
      V3 tmp{0, 0, 1};
      if (a.x == 0.0 && a.y == 0.0 && a.z == 1.0) tmp = V3{1, 0, 0};
      const V3 b = init_normalized(tmp - a * dot(a, tmp)), c = cross(a, b);
      misc[IM_LXLY + 0] = b.x; misc[IM_LXLY + 1] = c.x;
      misc[IM_LXLY + 2] = b.y; misc[IM_LXLY + 3] = c.y;
      misc[IM_LXLY + 4] = b.z; misc[IM_LXLY + 5] = c.z;
    }
    __syncthreads();
    if (tid < nI) {
      double* r = rec + tid * INIT_REC;
      const double dt = r[IR_DT];
      const V3 g0 = init_load3(misc + IM_G0);
      const M3 RiT = init_load33(r + IR_RIT);
      M3 M1, M2;
#pragma unroll
      for (int k = 0; k < 9; ++k) { M1.m[k] = RiT.m[k] * dt * dt / 2; M2.m[k] = RiT.m[k] * dt; }
      const double* L = misc + IM_LXLY;
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
          r[IR_GP + 3 * k + cc] = M1.m[3 * k] * L[cc] + M1.m[3 * k + 1] * L[2 + cc] + M1.m[3 * k + 2] * L[4 + cc];
          r[IR_GV + 3 * k + cc] = M2.m[3 * k] * L[cc] + M2.m[3 * k + 1] * L[2 + cc] + M2.m[3 * k + 2] * L[4 + cc];
        }
      init_store3(r + IR_BP, init_load3(r + IR_BP0) - mul(M1, g0));
      init_store3(r + IR_BV, init_load3(r + IR_DV) - mul(M2, g0));
    }
    __syncthreads();
    init_assemble(rec, A, ld, F, 2, acc, round == 0);
    __syncthreads();
    init_solve(A, ld, m + 3, col, xs);
    if (tid == 0) {
      const V3 g0 = init_load3(misc + IM_G0);
      const double* L = misc + IM_LXLY;
      const double d0 = xs[m], d1 = xs[m + 1];
      const V3 step{L[0] * d0 + L[1] * d1, L[2] * d0 + L[3] * d1, L[4] * d0 + L[5] * d1};
      init_store3(misc + IM_G0, init_normalized(g0 + step) * G);
    }
    __syncthreads();
  }

  // ---- c. the refined scale and the state change (:190-196, estimator.cpp:525-583)
  if (tid == 0) {
    const double s = xs[m + 2] / 100.0;
    const V3 g = init_load3(misc + IM_G0);
    bool finite = isfinite(s) && init_finite3(g);
    for (int k = 0; k < m + 2; ++k) finite = finite && isfinite(xs[k]);
    int fail = 0;
    if (!finite) fail |= VPL_INIT_FAIL_NONFINITE;
    if (s < 0.0) fail |= VPL_INIT_FAIL_REFINED_SCALE;
    o.s = s;
    init_store3(o.g_refined, g);
    if (!fail) {
      // Utility::g2R, then the yaw of R0 * Rs[0] removed (:572-575)
      M3 R0 = qmat(init_from_two_vectors(init_normalized(g), V3{0, 0, 1.0}));
      R0 = mul(ypr2R(V3{-R2ypr(R0).x, 0, 0}), R0);
      const M3 Rs0 = init_load33(Rq + q.key[0] * 9);
      R0 = mul(ypr2R(V3{-R2ypr(mul(R0, Rs0)).x, 0, 0}), R0);
      init_store3(o.g, mul(R0, g));
      const V3 tic = init_load3(q.tic);
      const V3 P0 = init_load3(Tq + q.key[0] * 3) * s - mul(Rs0, tic);
      for (int i = 0; i < VPL_NFRAMES; ++i) {
        const M3 Ri = init_load33(Rq + q.key[i] * 9);
        const V3 Pi = (init_load3(Tq + q.key[i] * 3) * s - mul(Ri, tic)) - P0;
        const V3 Vi = mul(Ri, V3{xs[3 * i], xs[3 * i + 1], xs[3 * i + 2]});   // kv counts key frames (:554-563)
        const V3 P = mul(R0, Pi), V = mul(R0, Vi);
        const Q4 qq = odo_mat2q(mul(R0, Ri));
        double* ps = o.pose[i];
        double* sb = o.speed_bias[i];
        ps[0] = P.x; ps[1] = P.y; ps[2] = P.z; ps[3] = qq.x; ps[4] = qq.y; ps[5] = qq.z; ps[6] = qq.w;
        sb[0] = V.x; sb[1] = V.y; sb[2] = V.z;
        for (int k = 0; k < 3; ++k) { sb[3 + k] = q.bas[3 * i + k]; sb[6 + k] = q.bgs[3 * i + k] + o.delta_bg[k]; }
        for (int k = 0; k < 7; ++k) finite = finite && isfinite(ps[k]);
        for (int k = 0; k < 9; ++k) finite = finite && isfinite(sb[k]);
      }
      finite = finite && init_finite3(init_load3(o.g));
      if (!finite) fail |= VPL_INIT_FAIL_NONFINITE;
    }
    o.fail = fail;
    o.ok = fail ? 0 : 1;
    misc[IM_FAIL] = fail ? 1.0 : 0.0;
  }
  __syncthreads();
  if (misc[IM_FAIL] != 0.0) {   // nothing behind a failing stage is handed out
    double* z = o.g;
    const int nz = 3 + INIT_MAXF * 3 + VPL_NFRAMES * 16;   // g, vel, pose, speed_bias: contiguous in vpl_init_result
    for (int k = tid; k < nz; k += INIT_THREADS) z[k] = 0.0;
    return;
  }
  for (int k = tid; k < m; k += INIT_THREADS) o.vel[k / 3][k % 3] = xs[k];
}

}  // namespace vpl
