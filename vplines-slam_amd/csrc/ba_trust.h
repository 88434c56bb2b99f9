// What the general path (solve_body, ba_solve.h) and the fast path (schur_body / back_body, ba_step.h) of the trust-region
// step have in common, once: Jacobi scaling with the dogleg diagonal / gradient, the regularised 4x4 line block, the landmark
// back-substitution, the dogleg step with the candidate x (+) delta.  All of it is inlined into its callers and templated on
// the work-group's thread count T.  A statement is the unit of rounding (-ffp-contract=on contracts within one only).
// Restates ceres-solver 1.12 DoglegStrategy::ComputeStep / TrustRegionMinimizer (see ba_solve.h).
#pragma once
#include "ba_common.h"

namespace vpl {

// ceres defaults (solver.h, 1.12)
constexpr double kMinDiag = 1e-6, kMaxDiag = 1e32, kMaxMu = 1.0, kMuIncrease = 10.0;
constexpr double kMinRelDecrease = 1e-3, kFuncTol = 1e-6, kParamTol = 1e-8, kMinRadius = 1e-32;
constexpr int kMaxInvalid = 5;

__device__ __forceinline__ void chol4(double* A, bool& ok) {   // packed lower 4x4, in place
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double d = A[tri(j, j)];
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < j) d -= A[tri(j, k)] * A[tri(j, k)];
    if (!(d > 0.0)) { ok = false; d = 1.0; }
    d = sqrt(d);
    A[tri(j, j)] = d;
#pragma unroll
    for (int i = 0; i < 4; ++i) if (i > j) {
      double s2 = A[tri(i, j)];
#pragma unroll
      for (int k = 0; k < 4; ++k) if (k < j) s2 -= A[tri(i, k)] * A[tri(j, k)];
      A[tri(i, j)] = s2 / d;
    }
  }
}

// The list k_cost of THIS iteration fills is emptied by the first kernel of the step (k_cost runs after that whole kernel).
__device__ __forceinline__ void empty_next_order(const DevBatch& B) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { B.ord_cnt[2 * ((B.ord_it + 1) & 1)] = 0; B.ord_cnt[2 * ((B.ord_it + 1) & 1) + 1] = 0; }
}

// ---- jacobi scaling (iteration 0 only), diagonal_, gradient_ ---------------------------------------------------------
// Stores scale / diagonal_ / gradient_ of every dimension to HBM, the unscaled-space vector of gradient_ / diagonal_ of
// the camera dims to uc (176), and what it works out for the landmarks (scale, diagonal, gradient, and their H blocks) to
// LDS as well: kP (nP x 4: s, d, g, H_pp) and kL (nL x 28: s(4), d(4), g(4), H_ll(16)) -- the landmark constants of the
// first factorisation attempt read it there instead of loading back from HBM what was stored a moment ago.  KEEP: the
// camera dims' scale and diagonal also go to sc / dg (176 each, LDS).  a1, q: this thread's part of |gradient_|^2 and of
// the landmark part of the Cauchy denominator u^T H u; the caller sums them over the work-group.
template <int T, bool KEEP>
__device__ __forceinline__ void scale_and_gradient(const DevBatch& B, const int w, const bool first, double* kP, double* kL, double* uc,
                                                   double* sc, double* dg, double& a1, double& q) {
  const int tid = threadIdx.x;
  const int nP = B.nP[w], nL = B.nL[w];
  const size_t fb = (size_t)w * B.nfull;
  double* gscale = B.scale + fb;
  double* gdiag = B.diag + fb;
  double* ggrad = B.grad + fb;
  const double* Hcc = B.Hcc + (size_t)w * NCP;
  const double* gc = B.gc + (size_t)w * NC;
  const int LP = NC, LL = NC + B.maxP;   // offsets of the landmark sections in the full index
  // The inputs of this thread's first point and first line are requested BEFORE the camera entries are worked out and
  // stored: the three loops below otherwise pay three global round trips back to back (the compiler may not move the
  // later loops' loads above the earlier loops' stores).
  double pre_hp = 0.0, pre_sp = 0.0, pre_gp = 0.0, pre_Hl[16], pre_sl[4], pre_gl[4];
  if (tid < nP) {
    const size_t pi = (size_t)w * B.maxP + tid;
    pre_hp = B.Hpp[pi]; pre_gp = B.gp[pi];
    if (!first) pre_sp = gscale[LP + tid];
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) pre_Hl[k] = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) { pre_sl[a] = 0.0; pre_gl[a] = 0.0; }
  if (tid < nL) {
    const size_t li = (size_t)w * B.maxL + tid;
#pragma unroll
    for (int k = 0; k < 16; ++k) pre_Hl[k] = B.Hll[li * 16 + k];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      pre_gl[a] = B.gl[li * 4 + a];
      if (!first) pre_sl[a] = gscale[LL + 4 * tid + a];
    }
  }
  for (int c = tid; c < 176; c += T) {
    double s = 0.0, d = 1.0, g = 0.0;
    if (c < NC) {
      const double h = Hcc[tri(c, c)];
      s = first ? 1.0 / (1.0 + sqrt(h)) : gscale[c];
      if (first) gscale[c] = s;
      d = sqrt(fmin(fmax(s * s * h, kMinDiag), kMaxDiag));
      g = s * gc[c] / d;
      gdiag[c] = d; ggrad[c] = g;
      a1 += g * g;
    }
    if constexpr (KEEP) { sc[c] = s; dg[c] = d; }
    uc[c] = s * g / d;   // unscaled-space vector of gradient_/diagonal_
  }
  for (int p = tid; p < nP; p += T) {
    const size_t pi = (size_t)w * B.maxP + p;
    const bool pre = p == tid;   // this thread's first point was requested together with its camera entry (above)
    const double h = pre ? pre_hp : B.Hpp[pi];
    const double s = first ? 1.0 / (1.0 + sqrt(h)) : (pre ? pre_sp : gscale[LP + p]);
    if (first) gscale[LP + p] = s;
    const double d = sqrt(fmin(fmax(s * s * h, kMinDiag), kMaxDiag));
    const double g = s * (pre ? pre_gp : B.gp[pi]) / d;
    gdiag[LP + p] = d; ggrad[LP + p] = g;
    kP[4 * p] = s; kP[4 * p + 1] = d; kP[4 * p + 2] = g; kP[4 * p + 3] = h;
    a1 += g * g;
    const double u = s * g / d;
    q += u * h * u;
  }
  for (int l = tid; l < nL; l += T) {
    const size_t li = (size_t)w * B.maxL + l;
    const bool pre = l == tid;
    double Hl[16], sl4[4], gl4[4];
#pragma unroll
    for (int k = 0; k < 16; ++k) Hl[k] = pre ? pre_Hl[k] : B.Hll[li * 16 + k];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      sl4[a] = first ? 0.0 : (pre ? pre_sl[a] : gscale[LL + 4 * l + a]);
      gl4[a] = pre ? pre_gl[a] : B.gl[li * 4 + a];
    }
    double u[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const double h = Hl[5 * a];
      const double s = first ? 1.0 / (1.0 + sqrt(h)) : sl4[a];
      if (first) gscale[LL + 4 * l + a] = s;
      const double d = sqrt(fmin(fmax(s * s * h, kMinDiag), kMaxDiag));
      const double g = s * gl4[a] / d;
      gdiag[LL + 4 * l + a] = d; ggrad[LL + 4 * l + a] = g;
      kL[28 * l + a] = s; kL[28 * l + 4 + a] = d; kL[28 * l + 8 + a] = g;
      a1 += g * g;
      u[a] = s * g / d;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) kL[28 * l + 12 + k] = Hl[k];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      double hu = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) hu += Hl[4 * a + b] * u[b];
      q += u[a] * hu;
    }
  }
}

// ---- the regularised block of line l: A_l = S H S + mu D^2 = C C^T --------------------------------------------------
// C goes to lch (HBM: the back substitution reads it) and, with the off-diagonals pre-divided by the diagonal, to lC (LDS);
// lS = jacobi scale / diagonal of C, so that the row solve multiplies and never divides; lE = C^T (u ./ s) with
// u = s g~ / d  =>  u / s = g~ / d.  The caller has loaded s4, d4, g4, Hl (LDS on the first attempt, HBM on a retry) and
// keeps the factor A.  Returns false when the block is not positive definite.
__device__ __forceinline__ bool line_block(const double (&s4)[4], const double (&d4)[4], const double (&g4)[4], const double (&Hl)[16],
                                           const double mu, const int l, double* lch, double* lC, double* lS, double* lE, double (&A)[10]) {
  int t = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) if (b <= a) {
      A[t] = s4[a] * s4[b] * Hl[4 * a + b];
      if (a == b) A[t] += mu * d4[a] * d4[a];
      ++t;
    }
  bool ok = true;
  chol4(A, ok);
  double us[4];
#pragma unroll
  for (int k = 0; k < 10; ++k) { lch[l * 10 + k] = A[k]; lC[l * 10 + k] = A[k]; }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const double rd = 1.0 / A[tri(a, a)];
    lS[4 * l + a] = s4[a] * rd;   // x_a = (s_a w_a - sum_q C_aq x_q) / C_aa = lS_a w_a - sum_q (C_aq / C_aa) x_q
    us[a] = g4[a] / d4[a];
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) if (qd < a) lC[l * 10 + tri(a, qd)] = A[tri(a, qd)] * rd;
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    double s2 = 0;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) if (qd >= a) s2 += A[tri(qd, a)] * us[qd];
    lE[4 * l + a] = s2;
  }
  return ok;
}

// ---- landmark back substitution y_l = A_l^-1 S_l (g_l - W_l S_c y_c) -------------------------------------------------
// 8 lanes per landmark row, so that every row of W is read as one contiguous segment; NH row groups per trip, whose loads
// are in flight together.  uc holds S_c y_c (UC_CAM: in camera order; otherwise in vis order, W's column order), pSt / lSt
// the start frame of every track.  The Gauss-Newton step of the landmarks goes to B.gn and to lgn (LDS); a2, a3 gather this
// thread's part of |gn|^2 and gradient_^T gn.  Points and lines are two calls: the general path has a stamp between them.
template <int T, int NH, bool UC_CAM>
__device__ __forceinline__ void back_substitute_points(const DevBatch& B, const int w, const double mu, const double* uc, const int* pSt,
                                                       double* lgn, double& a2, double& a3) {
  const int tid = threadIdx.x;
  const int nP = B.nP[w], WS = B.WS;
  const size_t fb = (size_t)w * B.nfull;
  const double* gscale = B.scale + fb;
  const double* gdiag = B.diag + fb;
  const double* ggrad = B.grad + fb;
  double* ggn = B.gn + fb;
  const int LP = NC;
  const int sub = tid & 7, grp = tid >> 3;   // T / 8 row groups per pass
  const int nblk = WS / 6;
  for (int p0 = 0; p0 < nP; p0 += NH * (T / 8)) {
    double wyv[NH], sv[NH], dv[NH], hv[NH], gv2[NH], grv[NH];
    size_t piv[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int p = p0 + h * (T / 8) + grp;
      piv[h] = (size_t)w * B.maxP + (p < nP ? p : 0);
      wyv[h] = 0.0; sv[h] = dv[h] = 1.0; hv[h] = gv2[h] = grv[h] = 0.0;
      if (p < nP) {
        // compact row: 6-blocks of the frames start .. start + maxTrack - 1, then the extrinsic block
        const int s0 = pSt[p];
        for (int blk = sub; blk < nblk; blk += 8) {
          const bool exb = blk == nblk - 1;
          const int vb = exb ? 66 : 6 * (s0 + blk);
          if (!exb && vb >= 66) continue;               // slot of a frame past the window
          const double* Wr = B.Wp + piv[h] * WS + 6 * blk;
#pragma unroll
          for (int k = 0; k < 6; ++k) wyv[h] += Wr[k] * uc[UC_CAM ? vis2cam(vb + k) : vb + k];
        }
        if (sub == 0) {
          sv[h] = gscale[LP + p]; dv[h] = gdiag[LP + p]; hv[h] = B.Hpp[piv[h]]; gv2[h] = B.gp[piv[h]];
          grv[h] = ggrad[LP + p];
        }
      }
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int p = p0 + h * (T / 8) + grp;
      double wy = wyv[h];
      wy += __shfl_xor(wy, 1, 64); wy += __shfl_xor(wy, 2, 64); wy += __shfl_xor(wy, 4, 64);
      if (p < nP && sub == 0) {
        const double s = sv[h], d = dv[h];
        const double Al = s * s * hv[h] + mu * d * d;
        const double y = s * (gv2[h] - wy) / Al;
        const double gnv = -d * y;
        ggn[LP + p] = gnv; lgn[LP + p] = gnv;
        a2 += gnv * gnv;
        a3 += grv[h] * gnv;
      }
    }
  }
}
// Lines: each row's W entries and g_l are requested together; the rows' right-hand sides s (g_l - W_l u_c) go to lrhs (LDS,
// 4 nL), and after ONE WORK-GROUP BARRIER one pass with a lane per line does the 4x4 triangular solves -- done by the leader
// lane of each group they were a chain of 8 divisions per 64 rows.
template <int T, int NH, bool UC_CAM>
__device__ __forceinline__ void back_substitute_lines(const DevBatch& B, const int w, const double* uc, const int* lSt, double* lrhs,
                                                      double* lgn, double& a2, double& a3) {
  const int tid = threadIdx.x;
  const int nL = B.nL[w], WS = B.WS;
  const size_t fb = (size_t)w * B.nfull;
  const double* gscale = B.scale + fb;
  const double* gdiag = B.diag + fb;
  const double* ggrad = B.grad + fb;
  double* ggn = B.gn + fb;
  const double* lch = B.lchol + (size_t)w * B.maxL * 10;
  const int LL = NC + B.maxP;
  const int sub = tid & 7, grp = tid >> 3;
  const int nblk = WS / 6;
  for (int r0 = 0; r0 < 4 * nL; r0 += NH * (T / 8)) {
    double wyv[NH], glv[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int r = r0 + h * (T / 8) + grp, l = r >> 2, a = r & 3;
      wyv[h] = 0.0; glv[h] = 0.0;
      if (l < nL) {
        const size_t li = (size_t)w * B.maxL + l;
        const int s0 = lSt[l];
        for (int blk = sub; blk < nblk; blk += 8) {
          const bool exb = blk == nblk - 1;
          const int vb = exb ? 66 : 6 * (s0 + blk);
          if (!exb && vb >= 66) continue;
          const double* Wr = B.Wl + (li * 4 + a) * WS + 6 * blk;
#pragma unroll
          for (int k = 0; k < 6; ++k) wyv[h] += Wr[k] * uc[UC_CAM ? vis2cam(vb + k) : vb + k];
        }
        if (sub == 0) glv[h] = B.gl[li * 4 + a];
      }
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int r = r0 + h * (T / 8) + grp;
      double wy = wyv[h];
      wy += __shfl_xor(wy, 1, 64); wy += __shfl_xor(wy, 2, 64); wy += __shfl_xor(wy, 4, 64);
      if (r < 4 * nL && sub == 0) lrhs[r] = gscale[LL + r] * (glv[h] - wy);
    }
  }
  __syncthreads();
  for (int l = tid; l < nL; l += T) {
    double C[10], t4[4], gd4[4], gr4[4];   // the factor, diagonal and gradient come from HBM: one batch, before the chain
#pragma unroll
    for (int k = 0; k < 10; ++k) C[k] = lch[l * 10 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) { gd4[k] = gdiag[LL + 4 * l + k]; gr4[k] = ggrad[LL + 4 * l + k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) t4[k] = lrhs[4 * l + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double s2 = t4[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) if (j < k) s2 -= C[tri(k, j)] * t4[j];
      t4[k] = s2 / C[tri(k, k)];
    }
#pragma unroll
    for (int k = 3; k >= 0; --k) {
      double s2 = t4[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) if (j > k) s2 -= C[tri(j, k)] * t4[j];
      t4[k] = s2 / C[tri(k, k)];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double gnv = -gd4[k] * t4[k];
      ggn[LL + 4 * l + k] = gnv; lgn[LL + 4 * l + k] = gnv;
      a2 += gnv * gnv;
      a3 += gr4[k] * gnv;
    }
  }
}

// TrustRegionMinimizer::HandleInvalidStep (thread 0): the step is not taken and the next one regularises more.
__device__ __forceinline__ void handle_invalid_step(const DevBatch& B, TrState* tr) {
  tr->step_valid = 0;
  tr->iter += 1;
  tr->num_invalid += 1;
  if (tr->num_invalid >= kMaxInvalid) { tr->status = 2; tr->iter -= 1; }   // FAILURE breaks before the iteration is recorded
  else if (tr->iter >= B.opt.num_iterations) tr->status = 3;
  tr->mu *= kMuIncrease;   // StepIsInvalid
  tr->reuse = 0;
}

// ---- DoglegStrategy::ComputeTraditionalDoglegStep, the model cost change, the candidate x (+) delta -----------------
// From tr's radius, alpha, a1, a2, a3, mu and the Gauss-Newton step: lgn (LDS, scaled space) or, for a window that re-uses
// the step of a rejected iteration (reuse0), B.gn.  gdelta (LDS, nfull) receives step * jacobi scale; red is block_sum's
// workspace.  An invalid step (no decrease of the model) is recorded and nothing else written.
template <int T>
__device__ __forceinline__ void dogleg_step_and_candidate(const DevBatch& B, const int w, const bool reuse0, const double* lgn, double* gdelta,
                                                          double* red) {
  const int tid = threadIdx.x;
  TrState* tr = &B.tr[w];
  const int nP = B.nP[w], nL = B.nL[w];
  const size_t fb = (size_t)w * B.nfull;
  const double* gscale = B.scale + fb;
  const double* gdiag = B.diag + fb;
  const double* ggrad = B.grad + fb;
  const double* ggn = B.gn + fb;
  const int LP = NC, LL = NC + B.maxP;
  const double radius = tr->radius, alpha = tr->alpha, a1 = tr->a1, a2 = tr->a2, a3 = tr->a3, mu = tr->mu;
  const double gradient_norm = sqrt(a1), gauss_newton_norm = sqrt(a2);
  double c1, c2, dnorm;   // step (scaled space, before /diag) = -c1 * gradient_ + c2 * gauss_newton_step
  if (gauss_newton_norm <= radius) {
    c1 = 0.0; c2 = 1.0; dnorm = gauss_newton_norm;
  } else if (gradient_norm * alpha >= radius) {
    c1 = radius / gradient_norm; c2 = 0.0; dnorm = radius;
  } else {
    const double b_dot_a = -alpha * a3;
    const double a_sq = (alpha * gradient_norm) * (alpha * gradient_norm);
    const double bma = a_sq - 2 * b_dot_a + a2;
    const double c = b_dot_a - a_sq;
    const double d = sqrt(c * c + bma * (radius * radius - a_sq));
    const double beta = (c <= 0) ? (d - c) / bma : (radius * radius - a_sq) / (d + c);
    c1 = alpha * (1.0 - beta); c2 = beta;
    dnorm = sqrt(c1 * c1 * a1 - 2.0 * c1 * c2 * a3 + c2 * c2 * a2);
  }
  // model_cost_change = -(step^T gs + 1/2 step^T Hs step) with Hs y = gs - mu D^2 y folded in
  //   step = -c1 v - c2 y,  v = gradient_/diag, y = -gn/diag
  const double q_cauchy = a1 / alpha;                 // v^T Hs v
  const double sg = -c1 * a1 + c2 * a3;               // step^T gs
  const double vHy = a1 + mu * a3;
  const double yHy = -a3 - mu * a2;
  const double sHs = c1 * c1 * q_cauchy + 2.0 * c1 * c2 * vHy + c2 * c2 * yHy;
  const double model_cost_change = -(sg + 0.5 * sHs);
  if (!(model_cost_change > 0.0)) {
    if (tid == 0) handle_invalid_step(B, tr);
    return;
  }
  // ---- delta = step * jacobi scale; candidate = Plus(x, delta) -----------------------------------
  const int nfull_used = NC + B.maxP + 4 * nL;
  for (int k = tid; k < nfull_used; k += T) {
    const bool live = k < NC || (k >= LP && k < LP + nP) || k >= LL;
    if (live) gdelta[k] = gscale[k] * (-c1 * ggrad[k] + c2 * (reuse0 ? ggn[k] : lgn[k])) / gdiag[k];   // (a re-used step comes from HBM)
  }
  __syncthreads();
  double sn = 0.0, xn = 0.0;
  const bool ex_free = B.opt.estimate_extrinsic != 0;
  if (tid < NF + 1) {
    const bool isex = tid == NF;
    const double* x = isex ? B.ex + (size_t)w * 7 : B.pose + ((size_t)w * NF + tid) * 7;
    double* xc = isex ? B.ex_c + (size_t)w * 7 : B.pose_c + ((size_t)w * NF + tid) * 7;
    if (isex && !ex_free) {
      for (int k = 0; k < 7; ++k) xc[k] = x[k];
    } else {
      double out[7];
      pose_plus(x, gdelta + (isex ? 165 : 15 * tid), out);
      for (int k = 0; k < 7; ++k) { xc[k] = out[k]; sn += (x[k] - out[k]) * (x[k] - out[k]); xn += x[k] * x[k]; }
    }
  } else if (tid >= 64 && tid < 64 + NF) {
    const int f = tid - 64;
    const double* x = B.sb + ((size_t)w * NF + f) * 9;
    double* xc = B.sb_c + ((size_t)w * NF + f) * 9;
    for (int k = 0; k < 9; ++k) {
      const double d = gdelta[15 * f + 6 + k];
      xc[k] = x[k] + d;
      sn += d * d; xn += x[k] * x[k];
    }
  }
  for (int p = tid; p < nP; p += T) {
    const size_t pi = (size_t)w * B.maxP + p;
    const double d = gdelta[LP + p];
    B.invd_c[pi] = B.invd[pi] + d;
    sn += d * d; xn += B.invd[pi] * B.invd[pi];
  }
  for (int l = tid; l < nL; l += T) {
    const size_t li = (size_t)w * B.maxL + l;
    double out[4];
    line_orth_plus(B.orth + li * 4, gdelta + LL + 4 * l, out);
    for (int k = 0; k < 4; ++k) {
      const double x = B.orth[li * 4 + k];
      B.orth_c[li * 4 + k] = out[k];
      sn += (x - out[k]) * (x - out[k]); xn += x * x;
    }
    const Plk Lc_ = orth_to_plk(out);     // the candidate's world Pluecker line, once per line (B.lw_c)
    double* lwc = B.lw_c + li * 6;
    lwc[0] = Lc_.n.x; lwc[1] = Lc_.n.y; lwc[2] = Lc_.n.z; lwc[3] = Lc_.v.x; lwc[4] = Lc_.v.y; lwc[5] = Lc_.v.z;
  }
  sn = block_sum(sn, red);
  xn = block_sum(xn, red);
  VPL_STAMP(B, w, 7);
  if (tid == 0) {
    tr->dogleg_step_norm = dnorm;
    tr->model_cost_change = model_cost_change;
    tr->step_norm = sqrt(sn);
    tr->x_norm = sqrt(xn);
    tr->step_valid = 1;
    tr->num_invalid = 0;
  }
}

}  // namespace vpl
