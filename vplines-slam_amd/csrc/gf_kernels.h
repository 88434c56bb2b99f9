// Device side of the global fusion (vpl_gf_optimize_batch; DESIGN.md, "Global fusion"): ceres' trust-region loop with the
// Levenberg-Marquardt strategy on the pose chain of GlobalOptimization::optimize, the block-tridiagonal normal equations solved by a
// substructured Cholesky (gf_plan.h): phase A = k_gf_seg_factor, one lane per segment walks the Cholesky chain of the segment's
// interior and forward-solves g and the coupling to the left separator; phase B = k_gf_schur (the Schur complement on the
// separators, one lane per entry) and k_gf_sep (its chain and two substitutions, one lane per chain of the batch); phase C =
// k_gf_seg_back, one lane per segment back-substitutes the interior.
// One round = k_gf_edges<0>, k_gf_asm, k_gf_head, A, B, C, k_gf_cand, k_gf_edges<1>, k_gf_decide; the host enqueues
// max_iterations + 1 rounds and k_gf_finish.  blockIdx.y is the chain; a chain that has ended has GF_DONE set and its work-groups
// leave at once.  f64 throughout, no atomics: every sum has a fixed order.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#include "gf_plan.h"
#include "pg_kernels.h"
#include "vpl_math.h"
#include "vplines_ba.h"

namespace vpl {

enum GfCtl {
  GF_DONE = 0, GF_ITER, GF_RADIUS, GF_DECREASE, GF_X_COST, GF_X_NORM, GF_NEED_LIN, GF_SUCC, GF_UNSUCC, GF_TERM, GF_INVALID,
  GF_MODEL, GF_STEP_OK, GF_INITIAL, GF_LAST_OK, GF_GMAX, GF_CAND_COST, GF_RHO
};

struct GfChain {
  GfLayout L;
  size_t w, out;                 // the chain's workspace and its output (the head, then the poses [n][7]), in doubles
  size_t loc, glo, gxyz, gacc;   // in doubles from `in`: local [n][7], global [n][7], per node the fix's xyz [n][3] and accuracy [n] (0: none)
  int run;                       // 0: a non-finite input, nothing runs
  int resident;                  // 1 (a session): the solved poses go back into `glo`, only the head goes to `out`
};
struct GfArgs {
  const GfChain* ch;
  double* ws;
  double* in;
  double* out;
  vpl_gf_options opt;
};

constexpr int GF_THREADS = 256;

#define GF_CHAIN(A)                       \
  const GfChain& G = (A).ch[blockIdx.y];  \
  const GfLayout& L = G.L;                \
  const GfPlan& p = L.p;                  \
  double* const w = (A).ws + G.w;         \
  double* const ctl = w + L.ctl;          \
  (void)p

__device__ __forceinline__ Q4 gf_q(const double* x) { return Q4{x[3], x[4], x[5], x[6]}; }   // a pose is p, q(w, x, y, z)
__device__ __forceinline__ Q4 gf_conj(Q4 q) { return Q4{q.w, -q.x, -q.y, -q.z}; }

// ceres' QuaternionParameterization::Plus on the quaternion, t + dt on the rest: out = Plus(x, sign d), d = (dtheta, dt)
__device__ __forceinline__ void gf_plus(const double* x, const double* d, double sign, double* out) {
  const double a = sign * d[0], b = sign * d[1], c = sign * d[2];
  const double nrm = sqrt(a * a + b * b + c * c);
  const Q4 q = gf_q(x);
  Q4 r = q;
  if (nrm > 0.0) {
    const double s = sin(nrm) / nrm;
    r = qmul(Q4{cos(nrm), s * a, s * b, s * c}, q);
  }
  out[0] = x[0] + sign * d[3]; out[1] = x[1] + sign * d[4]; out[2] = x[2] + sign * d[5];
  out[3] = r.w; out[4] = r.x; out[5] = r.y; out[6] = r.z;
}

// RelativeRTError (Factors.h:52-114) between xi and xj, meas = iPj (3), iQj (4).  Ji, Jj [6][6] row-major over (dtheta, dt) of
// the two ends, in closed form, or null: with u = q_i / |q_i| and d = t_j - t_i the rows 0..2 have 2 R(u)^T [d]x / t_var and
// -+ R(u)^T / t_var, the rows 3..5 the columns 2 vec(iQj^-1 (x) q_i^-1 (x) [0, e_c] (x) q_j) / q_var for j and their negatives for i
__device__ __forceinline__ void gf_edge_eval(const double* xi, const double* xj, const double* meas, double tv, double qv, double r[6],
                                             double* Ji, double* Jj) {
  const V3 d{xj[0] - xi[0], xj[1] - xi[1], xj[2] - xi[2]};
  const Q4 qi = gf_q(xi), qj = gf_q(xj), ci = gf_conj(qi);
  // ceres::QuaternionRotatePoint: the quaternion is normalised first
  const double sc = 1.0 / sqrt(ci.w * ci.w + ci.x * ci.x + ci.y * ci.y + ci.z * ci.z);
  const Q4 u{ci.w * sc, ci.x * sc, ci.y * sc, ci.z * sc};
  const double t2 = u.w * u.x, t3 = u.w * u.y, t4 = u.w * u.z, t5 = -u.x * u.x, t6 = u.x * u.y, t7 = u.x * u.z, t8 = -u.y * u.y,
               t9 = u.y * u.z, t1 = -u.z * u.z;
  const double p0 = 2.0 * ((t8 + t1) * d.x + (t6 - t4) * d.y + (t3 + t7) * d.z) + d.x;
  const double p1 = 2.0 * ((t4 + t6) * d.x + (t5 + t1) * d.y + (t9 - t2) * d.z) + d.y;
  const double p2 = 2.0 * ((t7 - t3) * d.x + (t2 + t9) * d.y + (t5 + t8) * d.z) + d.z;
  r[0] = (p0 - meas[0]) / tv; r[1] = (p1 - meas[1]) / tv; r[2] = (p2 - meas[2]) / tv;
  const Q4 mi = gf_conj(Q4{meas[3], meas[4], meas[5], meas[6]});
  const Q4 e = qmul(mi, qmul(ci, qj));
  r[3] = 2.0 * e.x / qv; r[4] = 2.0 * e.y / qv; r[5] = 2.0 * e.z / qv;
  if (!Ji) return;
  const M3 Rt = qmat(u);   // R(q_i / |q_i|)^T
  const M3 A = mul_skew(Rt, d);
#pragma unroll
  for (int i = 0; i < 36; ++i) { Ji[i] = 0.0; Jj[i] = 0.0; }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      Ji[6 * a + b] = 2.0 * A.m[3 * a + b] / tv;
      Ji[6 * a + 3 + b] = -Rt.m[3 * a + b] / tv;
      Jj[6 * a + 3 + b] = Rt.m[3 * a + b] / tv;
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const Q4 ec{0.0, c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0};
    const Q4 f = qmul(mi, qmul(ci, qmul(ec, qj)));
    const double v[3] = {2.0 * f.x / qv, 2.0 * f.y / qv, 2.0 * f.z / qv};
#pragma unroll
    for (int a = 0; a < 3; ++a) { Jj[6 * (3 + a) + c] = v[a]; Ji[6 * (3 + a) + c] = -v[a]; }
  }
}

// ---- 6 x 6 pieces of the chains: the Cholesky factor in place (lower; false when a pivot is not positive and finite), L^-1 v, L^-T v
__device__ __forceinline__ bool gf_chol6(double* A) {
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[7 * j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= A[6 * j + k] * A[6 * j + k];
    if (!(d > 0.0) || !(d < DBL_MAX)) return false;
    const double piv = sqrt(d);
    A[7 * j] = piv;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = A[6 * i + j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= A[6 * i + k] * A[6 * j + k];
      A[6 * i + j] = v / piv;
    }
  }
  return true;
}
__device__ __forceinline__ void gf_fwd6(const double* Lm, double* v) {
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int c = 0; c < r; ++c) v[r] -= Lm[6 * r + c] * v[c];
    v[r] = v[r] / Lm[7 * r];
  }
}
__device__ __forceinline__ void gf_bwd6(const double* Lm, double* v) {
#pragma unroll
  for (int c = 5; c >= 0; --c) {
#pragma unroll
    for (int r = c + 1; r < 6; ++r) v[c] -= Lm[6 * r + c] * v[r];
    v[c] = v[c] / Lm[7 * c];
  }
}

// What a chain walks.  SEG: the nodes of the normal matrix -- D, O unscaled as k_gf_asm left them, scaled and given the LM diagonal
// on the way in; otherwise the separator system as k_gf_schur left it.
struct GfBlocks {
  const double *D, *O, *rhs, *scale, *cn;
  double inv_radius, min_diag, max_diag;
};
template <bool SEG>
__device__ __forceinline__ void gf_load_diag(const GfBlocks& B, int k, double* A) {
  const double* Dk = B.D + 36 * (size_t)k;
  if (!SEG) {
#pragma unroll
    for (int i = 0; i < 36; ++i) A[i] = Dk[i];
    return;
  }
  const double* s = B.scale + 6 * (size_t)k;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) A[6 * r + c] = Dk[6 * r + c] * s[r] * s[c];
#pragma unroll
  for (int c = 0; c < 6; ++c) A[7 * c] += fmin(fmax(s[c] * s[c] * B.cn[6 * (size_t)k + c], B.min_diag), B.max_diag) * B.inv_radius;
}
// element (r, c) of block (k + 1, k)
template <bool SEG>
__device__ __forceinline__ double gf_off(const GfBlocks& B, int k, int r, int c) {
  const double v = B.O[36 * (size_t)k + 6 * r + c];
  return SEG ? v * B.scale[6 * (size_t)(k + 1) + r] * B.scale[6 * (size_t)k + c] : v;
}

// The chain [a, b) of a block-tridiagonal system whose blocks run to n_total: Ld_k = chol(D_k - Lo_{k-1} Lo_{k-1}^T),
// Lo_k = O_k Ld_k^-T (also for k = b - 1 when k + 1 < n_total: the coupling to what follows the chain), y = L^-1 rhs, and with WL
// the six columns L^-1 [O_{a-1}; 0; ...] of the coupling to block a - 1.  false when a pivot fails.
template <bool SEG>
__device__ __forceinline__ bool gf_chain_forward(const GfBlocks& B, int a, int b, int n_total, double* Ld, double* Lo, double* y, double* WL) {
  double X[36], yp[6];
  for (int k = a; k < b; ++k) {
    double A[36];
    gf_load_diag<SEG>(B, k, A);
    if (k > a) {
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) {
          double s = 0.0;
#pragma unroll
          for (int i = 0; i < 6; ++i) s += X[6 * r + i] * X[6 * c + i];
          A[6 * r + c] -= s;
        }
    }
    if (!gf_chol6(A)) return false;
    double* Lk = Ld + 36 * (size_t)k;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) Lk[6 * r + c] = c <= r ? A[6 * r + c] : 0.0;
    double v[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      v[r] = B.rhs[6 * (size_t)k + r] * (SEG ? B.scale[6 * (size_t)k + r] : 1.0);
      if (k > a) {
#pragma unroll
        for (int i = 0; i < 6; ++i) v[r] -= X[6 * r + i] * yp[i];
      }
    }
    gf_fwd6(A, v);
#pragma unroll
    for (int r = 0; r < 6; ++r) { y[6 * (size_t)k + r] = v[r]; yp[r] = v[r]; }
    if (WL) {
      double* Wk = WL + 36 * (size_t)k;
      const double* Wp = Wk - 36;
      for (int c = 0; c < 6; ++c) {
        double col[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          if (k == a) col[r] = gf_off<SEG>(B, a - 1, r, c);
          else {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 6; ++i) s += X[6 * r + i] * Wp[6 * i + c];
            col[r] = -s;
          }
        }
        gf_fwd6(A, col);
#pragma unroll
        for (int r = 0; r < 6; ++r) Wk[6 * r + c] = col[r];
      }
    }
    if (k + 1 < n_total) {
      double* Xk = Lo + 36 * (size_t)k;
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double row[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) row[c] = gf_off<SEG>(B, k, r, c);
        gf_fwd6(A, row);
#pragma unroll
        for (int c = 0; c < 6; ++c) { X[6 * r + c] = row[c]; Xk[6 * r + c] = row[c]; }
      }
    }
  }
  return true;
}

// x_k = Ld_k^-T (y_k - WL_k xL - Lo_k^T x_{k+1}) for k = b - 1 .. a; x_b is read from xs when b < n_total
__device__ __forceinline__ void gf_chain_backward(const double* Ld, const double* Lo, const double* y, int a, int b, int n_total,
                                                  const double* WL, const double* xL, double* xs) {
  double xn[6];
  bool have = b < n_total;
  if (have) {
#pragma unroll
    for (int i = 0; i < 6; ++i) xn[i] = xs[6 * (size_t)b + i];
  }
  for (int k = b - 1; k >= a; --k) {
    double v[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) v[c] = y[6 * (size_t)k + c];
    if (WL) {
      const double* Wk = WL + 36 * (size_t)k;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) v[r] -= Wk[6 * r + c] * xL[c];
    }
    if (have) {
      const double* Xk = Lo + 36 * (size_t)k;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) v[c] -= Xk[6 * r + c] * xn[r];
    }
    gf_bwd6(Ld + 36 * (size_t)k, v);
#pragma unroll
    for (int c = 0; c < 6; ++c) { xs[6 * (size_t)k + c] = v[c]; xn[c] = v[c]; }
    have = true;
  }
}

__device__ __forceinline__ GfBlocks gf_node_blocks(const GfArgs& A, const GfLayout& L, double* w, const double* ctl) {
  GfBlocks B;
  B.D = w + L.D; B.O = w + L.O; B.rhs = w + L.g; B.scale = w + L.scale; B.cn = w + L.cn;
  B.inv_radius = 1.0 / ctl[GF_RADIUS]; B.min_diag = A.opt.min_lm_diagonal; B.max_diag = A.opt.max_lm_diagonal;
  return B;
}

// ---- the start: the state = the incoming global poses, the measurements of the edges from the local poses, the control block
__global__ __launch_bounds__(GF_THREADS) void k_gf_init(GfArgs A) {
  GF_CHAIN(A);
  const int n = p.n, k = blockIdx.x * GF_THREADS + threadIdx.x;
  if (k == 0) {
    for (int i = 0; i < GF_CTL; ++i) ctl[i] = 0.0;
    ctl[GF_DONE] = G.run ? 0.0 : 1.0;
    ctl[GF_TERM] = (double)(G.run ? VPL_GF_CONVERGENCE : VPL_GF_FAILURE);
    ctl[GF_RADIUS] = A.opt.initial_radius; ctl[GF_DECREASE] = 2.0; ctl[GF_NEED_LIN] = 1.0; ctl[GF_LAST_OK] = 1.0;
  }
  if (!G.run || k >= n) return;
  const double *loc = A.in + G.loc, *glo = A.in + G.glo;
  for (int i = 0; i < 7; ++i) w[L.x + 7 * (size_t)k + i] = glo[7 * (size_t)k + i];
  if (k + 1 >= n) return;
  const double *a = loc + 7 * (size_t)k, *b = a + 7;
  const M3 Ri = qmat(gf_q(a)), Rj = qmat(gf_q(b));
  const V3 rel = mulT(Ri, V3{b[0] - a[0], b[1] - a[1], b[2] - a[2]});
  const Q4 q = mat2q(mulTA(Ri, Rj));
  double* me = w + L.meas + 7 * (size_t)k;
  me[0] = rel.x; me[1] = rel.y; me[2] = rel.z; me[3] = q.w; me[4] = q.x; me[5] = q.y; me[6] = q.z;
}

// ---- one lane per node k: the edge k -> k + 1 and the node's GNSS factor.  MODE 0: residuals, Jacobians, corrector and costs at
//      x; MODE 1: the costs at the candidate.  Cost slots: 2 k the edge, 2 k + 1 the GNSS factor (0 where there is none)
template <int MODE>
__global__ __launch_bounds__(GF_THREADS) void k_gf_edges(GfArgs A) {
  GF_CHAIN(A);
  if (ctl[GF_DONE] != 0.0) return;
  if (MODE == 0 ? ctl[GF_NEED_LIN] == 0.0 : ctl[GF_STEP_OK] == 0.0) return;
  const int n = p.n, k = blockIdx.x * GF_THREADS + threadIdx.x;
  if (k >= n) return;
  const double* xs = w + (MODE == 0 ? L.x : L.cand);
  double* cost = w + (MODE == 0 ? L.ecost : L.ecand);
  double ce = 0.0, cg = 0.0;
  if (k + 1 < n) {
    double r[6], Ji[36], Jj[36];
    gf_edge_eval(xs + 7 * (size_t)k, xs + 7 * (size_t)(k + 1), w + L.meas + 7 * (size_t)k, A.opt.t_var, A.opt.q_var, r,
                 MODE == 0 ? Ji : nullptr, MODE == 0 ? Jj : nullptr);
    double sq = 0.0;
    for (int i = 0; i < 6; ++i) sq += r[i] * r[i];
    ce = 0.5 * sq;
    if (MODE == 0) {
      for (int i = 0; i < 6; ++i) w[L.er + 6 * (size_t)k + i] = r[i];
      for (int i = 0; i < 36; ++i) { w[L.eJi + 36 * (size_t)k + i] = Ji[i]; w[L.eJj + 36 * (size_t)k + i] = Jj[i]; }
    }
  }
  const double* gxyz = A.in + G.gxyz;
  const double acc = A.in[G.gacc + k];
  if (acc > 0.0) {
    double r[3], sq = 0.0;
    for (int i = 0; i < 3; ++i) { r[i] = (xs[7 * (size_t)k + i] - gxyz[3 * (size_t)k + i]) / acc; sq += r[i] * r[i]; }
    double rho0 = sq, rho1 = 1.0;
    if (A.opt.huber_delta > 0.0) pg_huber(sq, A.opt.huber_delta, rho0, rho1);
    cg = 0.5 * rho0;
    if (MODE == 0) {
      const double sc = sqrt(rho1);   // the corrector with rho'' <= 0: a plain scaling
      for (int i = 0; i < 3; ++i) w[L.gr + 3 * (size_t)k + i] = r[i] * sc;
      w[L.gw + k] = sc / acc;
    }
  } else if (MODE == 0) {
    for (int i = 0; i < 3; ++i) w[L.gr + 3 * (size_t)k + i] = 0.0;
    w[L.gw + k] = 0.0;
  }
  cost[2 * (size_t)k] = ce; cost[2 * (size_t)k + 1] = cg;
}

// ---- one lane per node: its diagonal block D_k and O_k = block (k + 1, k) (unscaled, without the LM diagonal), g, the column
//      norms and in iteration 0 the Jacobi scale.  A node gathers in this order: the edge it ends, the edge it starts, its GNSS factor
__global__ __launch_bounds__(GF_THREADS) void k_gf_asm(GfArgs A) {
  GF_CHAIN(A);
  if (ctl[GF_DONE] != 0.0 || ctl[GF_NEED_LIN] == 0.0) return;
  const int n = p.n, k = blockIdx.x * GF_THREADS + threadIdx.x;
  if (k >= n) return;
  double D[36], g[6], cn[6];
  for (int i = 0; i < 36; ++i) D[i] = 0.0;
  for (int i = 0; i < 6; ++i) { g[i] = 0.0; cn[i] = 0.0; }
  auto gather = [&](const double* J, const double* r) {
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) s += J[6 * i + a] * J[6 * i + b];
        D[6 * a + b] += s;
      }
      double gs = 0.0, cs = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) { gs += J[6 * i + a] * r[i]; cs += J[6 * i + a] * J[6 * i + a]; }
      g[a] += gs; cn[a] += cs;
    }
  };
  if (k > 0) gather(w + L.eJj + 36 * (size_t)(k - 1), w + L.er + 6 * (size_t)(k - 1));
  if (k + 1 < n) gather(w + L.eJi + 36 * (size_t)k, w + L.er + 6 * (size_t)k);
  const double gw = w[L.gw + k];
  for (int i = 0; i < 3; ++i) {
    D[7 * (3 + i)] += gw * gw; g[3 + i] += gw * w[L.gr + 3 * (size_t)k + i]; cn[3 + i] += gw * gw;
  }
  for (int i = 0; i < 36; ++i) w[L.D + 36 * (size_t)k + i] = D[i];
  for (int i = 0; i < 6; ++i) {
    w[L.g + 6 * (size_t)k + i] = g[i]; w[L.cn + 6 * (size_t)k + i] = cn[i];
    if (ctl[GF_ITER] == 0.0) w[L.scale + 6 * (size_t)k + i] = 1.0 / (1.0 + sqrt(cn[i]));
  }
  if (k + 1 < n) {
    const double *Ji = w + L.eJi + 36 * (size_t)k, *Jj = w + L.eJj + 36 * (size_t)k;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) s += Jj[6 * i + a] * Ji[6 * i + b];
        w[L.O + 36 * (size_t)k + 6 * a + b] = s;
      }
  }
}

template <int T>
__device__ __forceinline__ double gf_block_reduce(double s, double* red, bool take_max) {
  __syncthreads();
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = T / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] = take_max ? fmax(red[threadIdx.x], red[threadIdx.x + h]) : red[threadIdx.x] + red[threadIdx.x + h];
    __syncthreads();
  }
  return red[0];
}

// ---- one work-group per chain: the head of the iteration (ceres' FinalizeIterationAndCheckIfMinimizerCanContinue)
__global__ __launch_bounds__(GF_THREADS) void k_gf_head(GfArgs A) {
  GF_CHAIN(A);
  if (ctl[GF_DONE] != 0.0) return;
  __shared__ double red[GF_THREADS];
  const int tid = threadIdx.x, n = p.n;
  const double* x = w + L.x;
  if (ctl[GF_NEED_LIN] != 0.0) {
    if (ctl[GF_ITER] == 0.0) {
      const double cost = pg_block_sum<GF_THREADS>(w + L.ecost, 2 * n, red);
      double s = 0.0;
      for (int i = tid; i < 7 * n; i += GF_THREADS) s += x[i] * x[i];
      const double xn = sqrt(gf_block_reduce<GF_THREADS>(s, red, false));
      if (tid == 0) { ctl[GF_X_COST] = cost; ctl[GF_INITIAL] = cost; ctl[GF_X_NORM] = xn; }
    }
    double gm = 0.0;   // max |x - Plus(x, -g)|
    for (int k = tid; k < n; k += GF_THREADS) {
      double moved[7];
      gf_plus(x + 7 * (size_t)k, w + L.g + 6 * (size_t)k, -1.0, moved);
      for (int i = 0; i < 7; ++i) gm = fmax(gm, fabs(x[7 * (size_t)k + i] - moved[i]));
    }
    gm = gf_block_reduce<GF_THREADS>(gm, red, true);
    if (tid == 0) ctl[GF_GMAX] = gm;
  }
  __syncthreads();
  if (tid == 0) {
    if (ctl[GF_LAST_OK] != 0.0) ctl[GF_SUCC] += 1.0; else ctl[GF_UNSUCC] += 1.0;
    if (ctl[GF_ITER] >= (double)A.opt.max_iterations) { ctl[GF_TERM] = (double)VPL_GF_NO_CONVERGENCE; ctl[GF_DONE] = 1.0; }
    else if (ctl[GF_LAST_OK] != 0.0 && ctl[GF_GMAX] <= A.opt.gradient_tolerance) { ctl[GF_TERM] = (double)VPL_GF_CONVERGENCE; ctl[GF_DONE] = 1.0; }
    else if (ctl[GF_RADIUS] <= A.opt.min_radius) { ctl[GF_TERM] = (double)VPL_GF_CONVERGENCE; ctl[GF_DONE] = 1.0; }
    else ctl[GF_ITER] += 1.0;
    ctl[GF_NEED_LIN] = 0.0;
  }
}

// ---- phase A, one lane per segment: the Cholesky chain of the interior, y = L^-1 g, WL = L^-1 (coupling to the left separator);
//      the coupling to the right separator is Lo of the segment's last node
__global__ __launch_bounds__(64) void k_gf_seg_factor(GfArgs A) {
  GF_CHAIN(A);
  if (ctl[GF_DONE] != 0.0) return;
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= p.nseg) return;
  int a, b;
  gf_seg_bounds(p, j, a, b);
  const GfBlocks B = gf_node_blocks(A, L, w, ctl);
  const bool ok = gf_chain_forward<true>(B, a, b, p.n, w + L.Ld, w + L.Lo, w + L.y, gf_seg_has_left(p, j) ? w + L.WL : nullptr);
  w[L.segok + j] = ok ? 1.0 : 0.0;
}

// ---- phase B, assembly: the Schur complement on the separators, one lane per entry.  Per separator j (node s, segment j before it,
//      segment j + 1 after it) the items 0..35 = SD = Hs(s, s) - Lo_{s-1} Lo_{s-1}^T - sum_k WL_k^T WL_k over segment j + 1 in node
//      order, 36..71 = SO = block (separator j + 1, separator j) = -Lo_e WL_e at the last node e of segment j + 1, 72..77 the right side
constexpr int GF_SCHUR_ITEMS = 80;
__global__ __launch_bounds__(GF_THREADS) void k_gf_schur(GfArgs A) {
  GF_CHAIN(A);
  if (ctl[GF_DONE] != 0.0) return;
  const int t = blockIdx.x * GF_THREADS + threadIdx.x, j = t / GF_SCHUR_ITEMS, item = t % GF_SCHUR_ITEMS;
  if (j >= p.nsep || item >= 78) return;
  const int s = gf_sep_node(p, j);
  int a1, b1;
  gf_seg_bounds(p, j + 1, a1, b1);
  const double *Lo = w + L.Lo, *WL = w + L.WL, *y = w + L.y;
  const double* XR = Lo + 36 * (size_t)(s - 1);
  if (item < 36) {
    const int r = item / 6, c = item % 6;
    const double *sc = w + L.scale + 6 * (size_t)s, *cn = w + L.cn + 6 * (size_t)s;
    double v = w[L.D + 36 * (size_t)s + item] * sc[r] * sc[c];
    if (r == c) v += fmin(fmax(sc[c] * sc[c] * cn[c], A.opt.min_lm_diagonal), A.opt.max_lm_diagonal) * (1.0 / ctl[GF_RADIUS]);
    double q = 0.0;
    for (int i = 0; i < 6; ++i) q += XR[6 * r + i] * XR[6 * c + i];
    v -= q;
    for (int k = a1; k < b1; ++k) {
      const double* Wk = WL + 36 * (size_t)k;
      double u = 0.0;
      for (int i = 0; i < 6; ++i) u += Wk[6 * i + r] * Wk[6 * i + c];
      v -= u;
    }
    w[L.SD + 36 * (size_t)j + item] = v;
  } else if (item < 72) {
    if (j + 1 >= p.nsep) return;
    const int r = (item - 36) / 6, c = (item - 36) % 6, e = b1 - 1;
    double q = 0.0;
    for (int i = 0; i < 6; ++i) q += Lo[36 * (size_t)e + 6 * r + i] * WL[36 * (size_t)e + 6 * i + c];
    w[L.SO + 36 * (size_t)j + (item - 36)] = -q;
  } else {
    const int r = item - 72;
    double v = w[L.g + 6 * (size_t)s + r] * w[L.scale + 6 * (size_t)s + r];
    double q = 0.0;
    for (int i = 0; i < 6; ++i) q += XR[6 * r + i] * y[6 * (size_t)(s - 1) + i];
    v -= q;
    for (int k = a1; k < b1; ++k) {
      double u = 0.0;
      for (int i = 0; i < 6; ++i) u += WL[36 * (size_t)k + 6 * i + r] * y[6 * (size_t)k + i];
      v -= u;
    }
    w[L.srhs + 6 * (size_t)j + r] = v;
  }
}

// ---- phase B, the chain: one work-group (one wave) per chain of the batch.  Every lane looks at the segments' verdicts, lane 0
//      walks the separator chain, its two substitutions, and hands the separators' solution to the nodes
__global__ __launch_bounds__(64) void k_gf_sep(GfArgs A) {
  GF_CHAIN(A);
  if (ctl[GF_DONE] != 0.0) return;
  __shared__ double red[64];
  double bad = 0.0;
  for (int j = threadIdx.x; j < p.nseg; j += 64) bad = fmax(bad, w[L.segok + j] == 0.0 ? 1.0 : 0.0);
  bad = gf_block_reduce<64>(bad, red, true);
  if (threadIdx.x != 0) return;
  bool ok = bad == 0.0;
  if (ok && p.nsep > 0) {
    GfBlocks B{};
    B.D = w + L.SD; B.O = w + L.SO; B.rhs = w + L.srhs;
    ok = gf_chain_forward<false>(B, 0, p.nsep, p.nsep, w + L.SLd, w + L.SLo, w + L.sy, nullptr);
    if (ok) {
      gf_chain_backward(w + L.SLd, w + L.SLo, w + L.sy, 0, p.nsep, p.nsep, nullptr, nullptr, w + L.sx);
      for (int j = 0; j < p.nsep; ++j)
        for (int i = 0; i < 6; ++i) w[L.xsol + 6 * (size_t)gf_sep_node(p, j) + i] = w[L.sx + 6 * (size_t)j + i];
    }
  }
  ctl[GF_STEP_OK] = ok ? 1.0 : 0.0;
}

// ---- phase C, one lane per segment: the interior's solution from its two separators'
__global__ __launch_bounds__(64) void k_gf_seg_back(GfArgs A) {
  GF_CHAIN(A);
  if (ctl[GF_DONE] != 0.0 || ctl[GF_STEP_OK] == 0.0) return;
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= p.nseg) return;
  int a, b;
  gf_seg_bounds(p, j, a, b);
  double xL[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const bool left = gf_seg_has_left(p, j);
  if (left)
    for (int i = 0; i < 6; ++i) xL[i] = w[L.xsol + 6 * (size_t)(a - 1) + i];
  gf_chain_backward(w + L.Ld, w + L.Lo, w + L.y, a, b, p.n, left ? w + L.WL : nullptr, xL, w + L.xsol);
}

// ---- one lane per node: the step delta = -scale x, the candidate Plus(x, delta), and the terms m (r + m / 2), m = J delta, of the
//      model cost change of the edge the node starts and of its GNSS factor
__global__ __launch_bounds__(GF_THREADS) void k_gf_cand(GfArgs A) {
  GF_CHAIN(A);
  if (ctl[GF_DONE] != 0.0 || ctl[GF_STEP_OK] == 0.0) return;
  const int n = p.n, k = blockIdx.x * GF_THREADS + threadIdx.x;
  if (k >= n) return;
  double d[6], dn[6];
  for (int i = 0; i < 6; ++i) {
    d[i] = -w[L.xsol + 6 * (size_t)k + i] * w[L.scale + 6 * (size_t)k + i];
    w[L.delta + 6 * (size_t)k + i] = d[i];
  }
  gf_plus(w + L.x + 7 * (size_t)k, d, 1.0, w + L.cand + 7 * (size_t)k);
  double me = 0.0, mg = 0.0;
  if (k + 1 < n) {
    for (int i = 0; i < 6; ++i) dn[i] = -w[L.xsol + 6 * (size_t)(k + 1) + i] * w[L.scale + 6 * (size_t)(k + 1) + i];
    const double *Ji = w + L.eJi + 36 * (size_t)k, *Jj = w + L.eJj + 36 * (size_t)k, *r = w + L.er + 6 * (size_t)k;
    for (int i = 0; i < 6; ++i) {
      double mi = 0.0;
      for (int c = 0; c < 6; ++c) mi += Ji[6 * i + c] * d[c];
      for (int c = 0; c < 6; ++c) mi += Jj[6 * i + c] * dn[c];
      me += mi * (r[i] + mi / 2.0);
    }
  }
  const double gw = w[L.gw + k];
  for (int i = 0; i < 3; ++i) {
    const double mi = gw * d[3 + i];
    mg += mi * (w[L.gr + 3 * (size_t)k + i] + mi / 2.0);
  }
  w[L.emod + 2 * (size_t)k] = me; w[L.emod + 2 * (size_t)k + 1] = mg;
}

// ---- one work-group per chain: the model cost change and the candidate's cost in fixed order, the tolerance tests, rho, the
//      radius, accept or keep x
__global__ __launch_bounds__(GF_THREADS) void k_gf_decide(GfArgs A) {
  GF_CHAIN(A);
  if (ctl[GF_DONE] != 0.0) return;
  __shared__ double red[GF_THREADS];
  const int tid = threadIdx.x, n = p.n;
  double model = 0.0;
  bool valid = ctl[GF_STEP_OK] != 0.0;
  if (valid) {
    model = -pg_block_sum<GF_THREADS>(w + L.emod, 2 * n, red);
    valid = model > 0.0;
  }
  __syncthreads();
  if (!valid) {   // HandleInvalidStep; the LM strategy's StepIsInvalid does nothing
    if (tid == 0) {
      ctl[GF_MODEL] = model;
      ctl[GF_INVALID] += 1.0;
      if (ctl[GF_INVALID] >= (double)A.opt.max_consecutive_invalid_steps) { ctl[GF_TERM] = (double)VPL_GF_FAILURE; ctl[GF_DONE] = 1.0; }
      ctl[GF_LAST_OK] = 0.0;
    }
    return;
  }
  double cand_cost = pg_block_sum<GF_THREADS>(w + L.ecand, 2 * n, red);
  double s = 0.0, bad = 0.0;
  for (int i = tid; i < 7 * n; i += GF_THREADS) {
    const double c = w[L.cand + i], d = w[L.x + i] - c;
    s += d * d;
    if (!(fabs(c) <= DBL_MAX)) bad = 1.0;
  }
  const double step_norm = sqrt(gf_block_reduce<GF_THREADS>(s, red, false));
  bad = gf_block_reduce<GF_THREADS>(bad, red, true);
  if (bad != 0.0 || !(fabs(cand_cost) <= DBL_MAX)) cand_cost = DBL_MAX;
  const double x_cost = ctl[GF_X_COST], x_norm = ctl[GF_X_NORM];
  int verdict = 0;   // 1: parameter tolerance, 2: function tolerance, 3: accepted, 4: rejected
  const double cc = x_cost - cand_cost, rho = cc / model;
  if (step_norm <= A.opt.parameter_tolerance * (x_norm + A.opt.parameter_tolerance)) verdict = 1;
  else if (fabs(cc) <= A.opt.function_tolerance * x_cost) verdict = 2;
  else verdict = rho > A.opt.min_relative_decrease ? 3 : 4;
  double xn = 0.0;
  if (verdict == 3) {
    double s2 = 0.0;
    for (int i = tid; i < 7 * n; i += GF_THREADS) { const double c = w[L.cand + i]; w[L.x + i] = c; s2 += c * c; }
    xn = sqrt(gf_block_reduce<GF_THREADS>(s2, red, false));
  }
  __syncthreads();   // (every thread has read the control block)
  if (tid != 0) return;
  ctl[GF_MODEL] = model; ctl[GF_INVALID] = 0.0; ctl[GF_CAND_COST] = cand_cost; ctl[GF_RHO] = rho;
  if (verdict <= 2) { ctl[GF_TERM] = (double)VPL_GF_CONVERGENCE; ctl[GF_DONE] = 1.0; return; }
  if (verdict == 3) {
    const double t = 2.0 * rho - 1.0;
    ctl[GF_X_COST] = cand_cost; ctl[GF_X_NORM] = xn; ctl[GF_NEED_LIN] = 1.0; ctl[GF_LAST_OK] = 1.0;
    ctl[GF_RADIUS] = fmin(A.opt.max_radius, ctl[GF_RADIUS] / fmax(1.0 / 3.0, 1.0 - t * t * t));
    ctl[GF_DECREASE] = 2.0;
  } else {
    ctl[GF_LAST_OK] = 0.0;
    ctl[GF_RADIUS] = ctl[GF_RADIUS] / ctl[GF_DECREASE];
    ctl[GF_DECREASE] *= 2.0;
  }
}

// ---- the result: the head, the poses, WGPS_T_WVIO = T_global(n-1) T_local(n-1)^-1 (globalOpt.cpp:239-248)
__global__ __launch_bounds__(GF_THREADS) void k_gf_finish(GfArgs A) {
  GF_CHAIN(A);
  double* out = A.out + G.out;
  const int n = p.n, k = blockIdx.x * GF_THREADS + threadIdx.x;
  const double* loc = A.in + G.loc;
  double* glo = A.in + G.glo;
  if (k < n && G.resident && G.run)
    for (int i = 0; i < 7; ++i) glo[7 * (size_t)k + i] = w[L.x + 7 * (size_t)k + i];
  if (k < n && !G.resident)
    for (int i = 0; i < 7; ++i) out[GF_HEAD + 7 * (size_t)k + i] = G.run ? w[L.x + 7 * (size_t)k + i] : glo[7 * (size_t)k + i];
  if (k != 0) return;
  out[0] = (double)VPL_GF_OK; out[1] = ctl[GF_TERM]; out[2] = ctl[GF_ITER]; out[3] = ctl[GF_SUCC]; out[4] = ctl[GF_UNSUCC];
  out[5] = ctl[GF_INITIAL]; out[6] = ctl[GF_X_COST];
  double* T = out + 8;
  for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
  if (!G.run) return;
  const double *xg = w + L.x + 7 * (size_t)(n - 1), *xl = loc + 7 * (size_t)(n - 1);
  const M3 R = mul(qmat(gf_q(xg)), transpose(qmat(gf_q(xl))));
  const V3 t = V3{xg[0], xg[1], xg[2]} - mul(R, V3{xl[0], xl[1], xl[2]});
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) T[4 * r + c] = R.m[3 * r + c];
  T[3] = t.x; T[7] = t.y; T[11] = t.z;
}

}  // namespace vpl
