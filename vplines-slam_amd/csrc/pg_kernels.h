// Device side of the pose-graph optimisation (vpl_pg_optimize_batch; DESIGN.md, "Pose-graph optimisation"): ceres' trust-region
// loop with the Levenberg-Marquardt strategy on the 4-DoF graph of PoseGraph::optimize4DoF, the normal equations H = B + U^T U
// solved by a block-banded Cholesky of B (sequential edges and the LM diagonal) and a capacitance system of the loop edges.
// One round = k_pg_edges<0>, k_pg_asm, k_pg_factor, k_pg_cols, k_pg_cap, k_pg_capsolve, k_pg_back, k_pg_edges<1>, k_pg_decide;
// the host enqueues max_iterations + 1 rounds and k_pg_finish.  blockIdx.y is the graph; a graph that has ended has PG_DONE set
// and its work-groups leave at once.  f64 throughout, no atomics: every sum has the order pg_plan.h fixes.
// SEQ (vpl_pg_optimize_seq_batch): the graph spans several sequences.  Every node keeps its slot; pg_node_flags (pg_plan.h) marks the
// constant nodes and the sequential edges that exist.  A masked edge writes nothing, so its residual, Jacobians and costs stay the
// zeros the workspace starts with; a constant end's Jacobian is stored as zero, which leaves its block of B, its g and its column
// norms zero and its Jacobi scale 1; k_pg_factor gives it a unit diagonal, so its step is zero; the norms skip it.  With SEQ
// false the kernels are what they were, and on a graph of one non-zero sequence SEQ changes no operation.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#include "pg_plan.h"
#include "vpl_math.h"
#include "vplines_ba.h"

namespace vpl {

enum PgCtl {
  PG_DONE = 0, PG_ITER, PG_RADIUS, PG_DECREASE, PG_X_COST, PG_X_NORM, PG_NEED_LIN, PG_SUCC, PG_UNSUCC, PG_TERM, PG_INVALID,
  PG_MODEL, PG_STEP_OK, PG_INITIAL, PG_LAST_OK, PG_GMAX, PG_STEP_VALID, PG_CAND_COST, PG_RHO
};

struct PgGraph {
  PgLayout p;
  size_t w, iw, in, out;   // the graph's workspace (doubles), integer block, packed input (doubles), packed output (doubles)
  int n_tail, run;         // run = 0: VPL_PG_UNSUPPORTED, nothing runs
};
struct PgArgs {
  const PgGraph* gr;
  double* ws;
  const int* ints;
  const double* in;
  double* out;
  vpl_pg_options opt;
};

constexpr int PG_THREADS = 256;

__device__ __forceinline__ double pg_norm_angle(double a) { return a > 180.0 ? a - 360.0 : (a < -180.0 ? a + 360.0 : a); }

// ends of edge slot s: false for a sequential slot that has no edge
__device__ __forceinline__ bool pg_ends(const PgLayout& p, const int* ints, int s, int& a, int& b, bool& loop) {
  if (s < 4 * p.nb) {
    const int i = s / 4 + 1, j = s % 4 + 1;
    a = i - j; b = i; loop = false;
    return a >= 0;
  }
  const int e = s - 4 * p.nb;
  a = ints[p.loop_ab + 2 * e]; b = ints[p.loop_ab + 2 * e + 1]; loop = true;
  return true;
}

// FourDOFError / FourDOFWeightError (pose_graph.h:159-248): xa, xb = (yaw, t) of the two ends, pra = pitch, roll of a.  Ja, Jb
// [4][4] row-major over (yaw, tx, ty, tz), or null
__device__ __forceinline__ void pg_eval(const double* xa, const double* xb, const double* pra, const double* meas, double yaw_div,
                                        double r[4], double* Ja, double* Jb) {
  const double y = xa[0] / 180.0 * M_PI, p = pra[0] / 180.0 * M_PI, q = pra[1] / 180.0 * M_PI;
  const double sy = sin(y), cy = cos(y), sp = sin(p), cp = cos(p), sr = sin(q), cr = cos(q);
  double R[9];
  R[0] = cy * cp; R[1] = -sy * cr + cy * sp * sr; R[2] = sy * sr + cy * sp * cr;
  R[3] = sy * cp; R[4] = cy * cr + sy * sp * sr;  R[5] = -cy * sr + sy * sp * cr;
  R[6] = -sp;     R[7] = cp * sr;                 R[8] = cp * cr;
  const double t0 = xb[1] - xa[1], t1 = xb[2] - xa[2], t2 = xb[3] - xa[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) r[c] = (R[c] * t0 + R[3 + c] * t1 + R[6 + c] * t2) - meas[c];
  r[3] = pg_norm_angle(xb[0] - xa[0] - meas[3]) / yaw_div;
  if (Ja) {
    const double k = M_PI / 180.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Ja[4 * c] = (-R[3 + c] * t0 + R[c] * t1) * k;   // d R^T / d yaw: row 0 of dR is -row 1 of R, row 1 is row 0
      Jb[4 * c] = 0.0;
#pragma unroll
      for (int d = 0; d < 3; ++d) { Ja[4 * c + 1 + d] = -R[3 * d + c]; Jb[4 * c + 1 + d] = R[3 * d + c]; }
    }
    Ja[12] = -1.0 / yaw_div; Jb[12] = 1.0 / yaw_div;
#pragma unroll
    for (int d = 1; d < 4; ++d) { Ja[12 + d] = 0.0; Jb[12 + d] = 0.0; }
  }
}

// ceres HuberLoss(delta) at s: rho and rho'
__device__ __forceinline__ void pg_huber(double s, double delta, double& rho0, double& rho1) {
  const double b = delta * delta;
  if (s > b) {
    const double r = sqrt(s);
    rho0 = 2.0 * delta * r - b;
    rho1 = fmax(DBL_MIN, delta / r);
  } else {
    rho0 = s; rho1 = 1.0;
  }
}

// sum of v[0 .. count) by the work-group in a fixed order: thread t adds t, t + T, ..., then a tree over the T partial sums
template <int T>
__device__ __forceinline__ double pg_block_sum(const double* v, int count, double* red) {
  double s = 0.0;
  for (int i = threadIdx.x; i < count; i += T) s += v[i];
  __syncthreads();
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = T / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  return red[0];
}

// SEQ: is edge slot s with the ends a < b part of the problem
__device__ __forceinline__ bool pg_edge_active(const int* fl, int a, int b, bool loop) {
  if (loop) return !((fl[a] & PG_NODE_CONST0) && (fl[b] & PG_NODE_CONST0));
  return (fl[b] >> (b - a)) & 1;
}

#define PG_GRAPH(A)                                 \
  const PgGraph& G = (A).gr[blockIdx.y];            \
  const PgLayout& p = G.p;                          \
  double* const w = (A).ws + G.w;                   \
  const int* const ints = (A).ints + G.iw;          \
  double* const ctl = w + p.ctl;                    \
  (void)ints

// ---- the start: state, fixed angles, the measurements of the sequential edges from the incoming poses, the control block
__global__ __launch_bounds__(PG_THREADS) void k_pg_init(PgArgs A) {
  PG_GRAPH(A);
  const double* in = A.in + G.in;
  const double *vT = in, *vR = in + 3 * (size_t)p.n, *li = in + 12 * (size_t)p.n;
  const int t = blockIdx.x * PG_THREADS + threadIdx.x;
  auto rot = [&](int k) { M3 R; for (int i = 0; i < 9; ++i) R.m[i] = vR[9 * (size_t)k + i]; return qmat(mat2q(R)); };
  if (t == 0) {
    ctl[PG_DONE] = (!G.run || p.n == 1) ? 1.0 : 0.0;
    ctl[PG_TERM] = (double)VPL_PG_CONVERGENCE;
    ctl[PG_RADIUS] = A.opt.initial_radius; ctl[PG_DECREASE] = 2.0; ctl[PG_NEED_LIN] = 1.0; ctl[PG_LAST_OK] = 1.0;
  }
  if (!G.run) return;
  if (t < p.n) {
    const V3 e = R2ypr(rot(t));
    w[p.x + 4 * t] = e.x;
    for (int i = 0; i < 3; ++i) w[p.x + 4 * t + 1 + i] = vT[3 * t + i];
    w[p.pr + 2 * t] = e.y; w[p.pr + 2 * t + 1] = e.z;
  }
  if (t < p.E) {
    int a, b; bool loop;
    if (!pg_ends(p, ints, t, a, b, loop)) return;
    double* me = w + p.meas + 4 * (size_t)t;
    if (loop) {
      const int e = t - 4 * p.nb;
      for (int i = 0; i < 4; ++i) me[i] = li[4 * e + i];
    } else {
      const M3 Ra = rot(a);
      const V3 rel = mulT(Ra, V3{vT[3 * b] - vT[3 * a], vT[3 * b + 1] - vT[3 * a + 1], vT[3 * b + 2] - vT[3 * a + 2]});
      me[0] = rel.x; me[1] = rel.y; me[2] = rel.z;
      me[3] = R2ypr(rot(b)).x - R2ypr(Ra).x;
    }
  }
}

// ---- one lane per edge.  MODE 0: residual, Jacobians, corrector and cost at x; MODE 1: the cost at the candidate
template <int MODE, bool SEQ>
__global__ __launch_bounds__(PG_THREADS) void k_pg_edges(PgArgs A) {
  PG_GRAPH(A);
  if (ctl[PG_DONE] != 0.0) return;
  if (MODE == 0 ? ctl[PG_NEED_LIN] == 0.0 : ctl[PG_STEP_VALID] == 0.0) return;
  const int t = blockIdx.x * PG_THREADS + threadIdx.x;
  if (t >= p.E) return;
  int a, b; bool loop;
  if (!pg_ends(p, ints, t, a, b, loop)) return;
  const int* fl = ints + p.itotal;   // SEQ: the node flags stand behind the graph's integer block
  if (SEQ && !pg_edge_active(fl, a, b, loop)) return;
  const double* xs = w + (MODE == 0 ? p.x : p.cand);
  double r[4], Ja[16], Jb[16];
  pg_eval(xs + 4 * a, xs + 4 * b, w + p.pr + 2 * a, w + p.meas + 4 * (size_t)t, loop ? A.opt.loop_yaw_scale : 1.0, r,
          MODE == 0 ? Ja : nullptr, MODE == 0 ? Jb : nullptr);
  const double sq = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3];
  double rho0 = sq, rho1 = 1.0;
  if (loop && A.opt.huber_delta > 0.0) pg_huber(sq, A.opt.huber_delta, rho0, rho1);
  if (MODE == 1) { w[p.ecand + t] = 0.5 * rho0; return; }
  w[p.ecost + t] = 0.5 * rho0;
  const double sc = sqrt(rho1);   // the corrector with rho'' <= 0: a plain scaling
  for (int i = 0; i < 4; ++i) w[p.er + 4 * (size_t)t + i] = r[i] * sc;
  const bool ca = SEQ && (fl[a] & PG_NODE_CONST), cb = SEQ && (fl[b] & PG_NODE_CONST);
  for (int i = 0; i < 16; ++i) {
    w[p.eJa + 16 * (size_t)t + i] = ca ? 0.0 : Ja[i] * sc;
    w[p.eJb + 16 * (size_t)t + i] = cb ? 0.0 : Jb[i] * sc;
  }
}

// ---- sixteen lanes per unknown node: its block column of B (unscaled, without the LM diagonal), its g and column norms, and in
//      iteration 0 the Jacobi scale
__global__ __launch_bounds__(PG_THREADS) void k_pg_asm(PgArgs A) {
  PG_GRAPH(A);
  if (ctl[PG_DONE] != 0.0 || ctl[PG_NEED_LIN] == 0.0) return;
  const int t = blockIdx.x * PG_THREADS + threadIdx.x;
  const int q = t >> 4, r = (t >> 2) & 3, c = t & 3;
  if (q >= p.nb) return;
  const int k = q + 1;
  int sl[8];
  pg_seq_incident(p.n, k, sl);
  const double *eJa = w + p.eJa, *eJb = w + p.eJb, *er = w + p.er;
  double d0 = 0.0;
  for (int u = 0; u < 8; ++u) {
    if (sl[u] < 0) continue;
    const double* J = (u < 4 ? eJb : eJa) + 16 * (size_t)sl[u];
    for (int i = 0; i < 4; ++i) d0 += J[4 * i + r] * J[4 * i + c];
  }
  double* Bq = w + p.B + (size_t)q * (PG_BW + 1) * 16;
  Bq[4 * r + c] = d0;
  for (int d = 1; d <= PG_BW; ++d) {
    const int s = sl[PG_BW + d - 1];
    double v = 0.0;
    if (s >= 0)
      for (int i = 0; i < 4; ++i) v += eJb[16 * (size_t)s + 4 * i + r] * eJa[16 * (size_t)s + 4 * i + c];
    Bq[16 * d + 4 * r + c] = v;
  }
  if (r != 0) return;
  double gs = 0.0, cn = 0.0;
  auto gather = [&](const double* J, const double* rr) {
    for (int i = 0; i < 4; ++i) { const double v = J[4 * i + c]; gs += v * rr[i]; cn += v * v; }
  };
  for (int u = 0; u < 8; ++u)
    if (sl[u] >= 0) gather((u < 4 ? eJb : eJa) + 16 * (size_t)sl[u], er + 4 * (size_t)sl[u]);
  for (int at = ints[p.inc_ptr + k]; at < ints[p.inc_ptr + k + 1]; ++at) {
    const int ent = ints[p.inc + at];
    const size_t s = (size_t)(4 * p.nb + (ent >> 1));
    gather(((ent & 1) ? eJb : eJa) + 16 * s, er + 4 * s);
  }
  w[p.g + 4 * q + c] = gs;
  w[p.cn + 4 * q + c] = cn;
  if (ctl[PG_ITER] == 0.0) w[p.scale + 4 * q + c] = 1.0 / (1.0 + sqrt(cn));
}

// ---- one work-group (one wave) per graph: the head of the iteration (ceres' FinalizeIterationAndCheckIfMinimizerCanContinue), then
//      the band Cholesky B = L L^T walking the chain, the 20 x 20 window of the current and the next four block columns in LDS
constexpr int PG_WIN = 4 * (PG_BW + 1);
template <bool SEQ>
__global__ __launch_bounds__(64) void k_pg_factor(PgArgs A) {
  PG_GRAPH(A);
  if (ctl[PG_DONE] != 0.0) return;
  __shared__ double W[PG_WIN * PG_WIN];
  __shared__ double P[PG_WIN * 4];
  __shared__ double red[64];
  const int l = threadIdx.x;
  const double* x = w + p.x;
  const int* fl = ints + p.itotal;   // SEQ: the node flags stand behind the graph's integer block
  auto is_const = [&](int k) { return SEQ && (fl[k] & PG_NODE_CONST); };   // node k
  if (ctl[PG_NEED_LIN] != 0.0) {
    if (ctl[PG_ITER] == 0.0) {
      const double cost = pg_block_sum<64>(w + p.ecost, p.E, red);
      double s = 0.0;
      for (int i = l; i < p.m; i += 64)
        if (!is_const(1 + (i >> 2))) s += x[4 + i] * x[4 + i];
      __syncthreads();
      red[l] = s;
      __syncthreads();
      for (int h = 32; h > 0; h >>= 1) { if (l < h) red[l] += red[l + h]; __syncthreads(); }
      if (l == 0) { ctl[PG_X_COST] = cost; ctl[PG_INITIAL] = cost; ctl[PG_X_NORM] = sqrt(red[0]); }
      __syncthreads();
    }
    double gm = 0.0;   // max |x - Plus(x, -g)|
    for (int i = l; i < p.m; i += 64) {
      if (is_const(1 + (i >> 2))) continue;
      const double xi = x[4 + i], gi = w[p.g + i];
      const double moved = (i & 3) == 0 ? pg_norm_angle(xi - gi) : xi - gi;
      gm = fmax(gm, fabs(xi - moved));
    }
    red[l] = gm;
    __syncthreads();
    for (int h = 32; h > 0; h >>= 1) { if (l < h) red[l] = fmax(red[l], red[l + h]); __syncthreads(); }
    if (l == 0) ctl[PG_GMAX] = red[0];
  }
  __syncthreads();
  if (l == 0) {
    if (ctl[PG_LAST_OK] != 0.0) ctl[PG_SUCC] += 1.0; else ctl[PG_UNSUCC] += 1.0;
    if (ctl[PG_ITER] >= (double)A.opt.max_iterations) { ctl[PG_TERM] = (double)VPL_PG_NO_CONVERGENCE; ctl[PG_DONE] = 1.0; }
    else if (ctl[PG_LAST_OK] != 0.0 && ctl[PG_GMAX] <= A.opt.gradient_tolerance) { ctl[PG_TERM] = (double)VPL_PG_CONVERGENCE; ctl[PG_DONE] = 1.0; }
    else if (ctl[PG_RADIUS] <= A.opt.min_radius) { ctl[PG_TERM] = (double)VPL_PG_CONVERGENCE; ctl[PG_DONE] = 1.0; }
    else ctl[PG_ITER] += 1.0;
    ctl[PG_NEED_LIN] = 0.0;
  }
  __syncthreads();
  if (ctl[PG_DONE] != 0.0) return;
  // ---- the factorisation
  const double radius = ctl[PG_RADIUS];
  const double *Bu = w + p.B, *scale = w + p.scale, *cn = w + p.cn;
  double* Lb = w + p.Lb;
  const int nb = p.nb;
  // element (r, c) of block (Pb, Qb), Qb <= Pb <= Qb + 4, scaled, the LM diagonal added; 0 outside the matrix
  auto elem = [&](int Pb, int Qb, int r, int c) -> double {
    if (Pb >= nb) return 0.0;
    if (is_const(Qb + 1) && Pb == Qb) return r == c ? 1.0 : 0.0;
    const double sr = scale[4 * Pb + r], sc = scale[4 * Qb + c];
    double v = Bu[((size_t)Qb * (PG_BW + 1) + (Pb - Qb)) * 16 + 4 * r + c] * sr * sc;
    if (Pb == Qb && r == c) v += fmin(fmax(sc * sc * cn[4 * Qb + c], A.opt.min_lm_diagonal), A.opt.max_lm_diagonal) / radius;
    return v;
  };
  auto slot = [](int gr, int gc) { return (gr % PG_WIN) * PG_WIN + (gc % PG_WIN); };
  auto load_row = [&](int Pb) {   // block row Pb of the window: blocks (Pb, Pb - 4 .. Pb)
    for (int i = l; i < (PG_BW + 1) * 16; i += 64) {
      const int Qb = Pb - PG_BW + i / 16, r = (i >> 2) & 3, c = i & 3;
      if (Qb >= 0) W[slot(4 * Pb + r, 4 * Qb + c)] = elem(Pb, Qb, r, c);
    }
  };
  for (int Pb = 0; Pb <= PG_BW; ++Pb) load_row(Pb);
  __syncthreads();
  bool ok = true;
  for (int q = 0; q < nb; ++q) {
    double pv[4];
    for (int k = 0; k < 4; ++k) pv[k] = l < PG_WIN ? W[slot(4 * q + l, 4 * q + k)] : 0.0;
    for (int k = 0; k < 4; ++k) {
      const double dk = __shfl(pv[k], k, 64);
      if (!(dk > 0.0) || !(dk < DBL_MAX)) { ok = false; break; }
      const double piv = sqrt(dk);
      if (l == k) pv[k] = piv; else if (l > k) pv[k] = pv[k] / piv;
      for (int c = k + 1; c < 4; ++c) {
        const double lc = __shfl(pv[k], c, 64);
        if (l >= c) pv[c] -= pv[k] * lc;
      }
    }
    if (!ok) break;   // (uniform: dk is the same in every lane)
    if (l < PG_WIN) {
      const int d = l >> 2, r = l & 3;
      for (int c = 0; c < 4; ++c) {
        const double v = (d == 0 && c > r) ? 0.0 : pv[c];
        P[4 * l + c] = v;
        if (q + d < nb) Lb[((size_t)q * (PG_BW + 1) + d) * 16 + 4 * r + c] = v;
      }
    }
    __syncthreads();
    for (int idx = l; idx < 256; idx += 64) {
      const int i = 4 + (idx >> 4), j = 4 + (idx & 15);
      if (j <= i) {
        double s = 0.0;
        for (int k = 0; k < 4; ++k) s += P[4 * i + k] * P[4 * j + k];
        W[slot(4 * q + i, 4 * q + j)] -= s;
      }
    }
    __syncthreads();
    load_row(q + PG_BW + 1);
    __syncthreads();
  }
  if (l == 0) ctl[PG_STEP_OK] = ok ? 1.0 : 0.0;
}

// ---- forward substitution L Y = [U^T, g]: one lane per column; column LP is g (into yg), columns 4e .. 4e + 3 the rows of loop
//      edge e, the others padding.  A column starts at the block row of its first non-zero; the rows of L are the same for every lane
__global__ __launch_bounds__(64) void k_pg_cols(PgArgs A) {
  PG_GRAPH(A);
  if (ctl[PG_DONE] != 0.0 || ctl[PG_STEP_OK] == 0.0) return;
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col > p.LP) return;
  const int nb = p.nb, LP = p.LP;
  const double *Lb = w + p.Lb, *scale = w + p.scale;
  const bool isg = col == LP;
  const int e = col >> 2, kres = col & 3;
  int qa = -1, qb = -1, start = nb;
  const double *Ja = nullptr, *Jb = nullptr;
  if (isg) start = 0;
  else if (e < p.L) {
    const size_t s = (size_t)(4 * nb + e);
    qa = ints[p.loop_ab + 2 * e] - 1; qb = ints[p.loop_ab + 2 * e + 1] - 1;
    Ja = w + p.eJa + 16 * s + 4 * kres; Jb = w + p.eJb + 16 * s + 4 * kres;
    start = qa >= 0 ? qa : qb;
  }
  double h[PG_BW][4];
  for (int d = 0; d < PG_BW; ++d) for (int c = 0; c < 4; ++c) h[d][c] = 0.0;
  for (int Pb = 0; Pb < nb; ++Pb) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (Pb >= start) {
      for (int r = 0; r < 4; ++r) {
        if (isg) v[r] = w[p.g + 4 * Pb + r] * scale[4 * Pb + r];
        else if (Pb == qa) v[r] = Ja[r] * scale[4 * Pb + r];
        else if (Pb == qb) v[r] = Jb[r] * scale[4 * Pb + r];
      }
#pragma unroll
      for (int d = 1; d <= PG_BW; ++d) {
        if (Pb - d < 0) continue;
        const double* Lk = Lb + ((size_t)(Pb - d) * (PG_BW + 1) + d) * 16;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) v[r] -= Lk[4 * r + c] * h[d - 1][c];
      }
      const double* Ld = Lb + (size_t)Pb * (PG_BW + 1) * 16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = 0; c < r; ++c) v[r] -= Ld[4 * r + c] * v[c];
        v[r] = v[r] / Ld[5 * r];
      }
#pragma unroll
      for (int d = PG_BW - 1; d > 0; --d)
#pragma unroll
        for (int c = 0; c < 4; ++c) h[d][c] = h[d - 1][c];
#pragma unroll
      for (int c = 0; c < 4; ++c) h[0][c] = v[c];
    }
    for (int r = 0; r < 4; ++r) {
      if (isg) w[p.yg + 4 * Pb + r] = v[r];
      else w[p.Y + (size_t)(4 * Pb + r) * LP + col] = v[r];
    }
  }
}

// ---- S = I + Yu^T Yu, one wave per 16 x 16 tile of the lower triangle, v_mfma_f64_16x16x4_f64 down the rows of Y
__global__ __launch_bounds__(64) void k_pg_cap(PgArgs A, int tiles) {
  PG_GRAPH(A);
  if (ctl[PG_DONE] != 0.0 || ctl[PG_STEP_OK] == 0.0 || p.L == 0) return;
  const int I = blockIdx.x / tiles, J = blockIdx.x % tiles, T = p.LP / 16;
  if (I >= T || J > I) return;
  const int l = threadIdx.x, lc = l & 15, lk = l >> 4;
  const size_t LP = (size_t)p.LP;
  const double* Y = w + p.Y;
  typedef double d4 __attribute__((ext_vector_type(4)));
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < p.m; k0 += 4) {   // (m is a multiple of 4)
    const double* row = Y + (size_t)(k0 + lk) * LP;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(row[16 * I + lc], row[16 * J + lc], acc, 0, 0, 0);
  }
  double* S = w + p.S;
  for (int v = 0; v < 4; ++v) {
    const int i = lk + 4 * v;   // C[lk + 4 v][lc]
    S[(size_t)(16 * I + i) * LP + 16 * J + lc] = acc[v] + ((I == J && i == lc) ? 1.0 : 0.0);
  }
}

// ---- one work-group per graph: rhs = Yu^T y_g, the blocked Cholesky of S (panels of 16, the trailing update by MFMA), w = S^-1 rhs
__global__ __launch_bounds__(PG_THREADS) void k_pg_capsolve(PgArgs A) {
  PG_GRAPH(A);
  if (ctl[PG_DONE] != 0.0 || ctl[PG_STEP_OK] == 0.0 || p.L == 0) return;
  __shared__ double D[16 * 17];
  __shared__ double rs[4 * PG_MAX_LOOPS];
  __shared__ int bad;
  const int tid = threadIdx.x, LPi = p.LP, T = LPi / 16;
  const size_t LP = (size_t)LPi;
  const double *Y = w + p.Y, *yg = w + p.yg;
  double* S = w + p.S;
  for (int c = tid; c < LPi; c += PG_THREADS) {
    double s = 0.0;
    for (int row = 0; row < p.m; ++row) s += Y[(size_t)row * LP + c] * yg[row];
    rs[c] = s;
  }
  if (tid == 0) bad = 0;
  __syncthreads();
  typedef double d4 __attribute__((ext_vector_type(4)));
  for (int J = 0; J < T; ++J) {
    const int i = tid >> 4, j = tid & 15;
    D[17 * i + j] = S[(size_t)(16 * J + i) * LP + 16 * J + j];
    __syncthreads();
    for (int k = 0; k < 16; ++k) {
      if (tid == 0) {
        const double dk = D[17 * k + k];
        if (!(dk > 0.0) || !(dk < DBL_MAX)) bad = 1;
        D[17 * k + k] = sqrt(dk);
      }
      __syncthreads();
      if (tid > k && tid < 16) D[17 * tid + k] = D[17 * tid + k] / D[17 * k + k];
      __syncthreads();
      if (j > k && i >= j) D[17 * i + j] -= D[17 * i + k] * D[17 * j + k];
      __syncthreads();
    }
    if (bad) break;   // (shared: uniform)
    S[(size_t)(16 * J + i) * LP + 16 * J + j] = j <= i ? D[17 * i + j] : 0.0;
    // the panel below: one thread per row solves x L11^T = a
    for (int r = 16 * (J + 1) + tid; r < LPi; r += PG_THREADS) {
      double* a = S + (size_t)r * LP + 16 * J;
      double xr[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) xr[c] = a[c];
#pragma unroll
      for (int c = 0; c < 16; ++c) {
#pragma unroll
        for (int k = 0; k < c; ++k) xr[c] -= xr[k] * D[17 * c + k];
        xr[c] = xr[c] / D[17 * c + c];
      }
#pragma unroll
      for (int c = 0; c < 16; ++c) a[c] = xr[c];
    }
    __syncthreads();
    // trailing update S[I2][J2] -= P[I2] P[J2]^T over the tiles J < J2 <= I2, one wave per tile
    const int wv = tid >> 6, l = tid & 63, lc = l & 15, lk = l >> 4, nt = T - J - 1;
    for (int t = wv; t < nt * nt; t += PG_THREADS / 64) {
      const int I2 = J + 1 + t / nt, J2 = J + 1 + t % nt;
      if (J2 > I2) continue;
      d4 acc = {0.0, 0.0, 0.0, 0.0};
      const double* pa = S + (size_t)(16 * I2 + lc) * LP + 16 * J + lk;
      const double* pb = S + (size_t)(16 * J2 + lc) * LP + 16 * J + lk;
#pragma unroll
      for (int k0 = 0; k0 < 16; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[k0], pb[k0], acc, 0, 0, 0);
      for (int v = 0; v < 4; ++v) S[(size_t)(16 * I2 + lk + 4 * v) * LP + 16 * J2 + lc] -= acc[v];
    }
    __syncthreads();
  }
  if (bad) { if (tid == 0) ctl[PG_STEP_OK] = 0.0; return; }
  // L z = rhs, then L^T w = z, in LDS
  for (int jc = 0; jc < LPi; ++jc) {
    if (tid == 0) rs[jc] = rs[jc] / S[(size_t)jc * LP + jc];
    __syncthreads();
    const double zj = rs[jc];
    for (int r = jc + 1 + tid; r < LPi; r += PG_THREADS) rs[r] -= S[(size_t)r * LP + jc] * zj;
    __syncthreads();
  }
  for (int jc = LPi - 1; jc >= 0; --jc) {
    if (tid == 0) rs[jc] = rs[jc] / S[(size_t)jc * LP + jc];
    __syncthreads();
    const double wj = rs[jc];
    for (int r = tid; r < jc; r += PG_THREADS) rs[r] -= S[(size_t)jc * LP + r] * wj;
    __syncthreads();
  }
  for (int c = tid; c < LPi; c += PG_THREADS) w[p.rhs + c] = rs[c];
}

// ---- one work-group per graph: z = y_g - Yu w, the backward substitution, delta = -scale L^-T z, the model cost change
//      -sum m (r + m / 2) with m = J delta per edge, and the candidate Plus(x, delta)
__global__ __launch_bounds__(PG_THREADS) void k_pg_back(PgArgs A) {
  PG_GRAPH(A);
  if (ctl[PG_DONE] != 0.0) return;
  __shared__ double red[PG_THREADS];
  const int tid = threadIdx.x, nb = p.nb;
  if (ctl[PG_STEP_OK] == 0.0) { if (tid == 0) ctl[PG_STEP_VALID] = 0.0; return; }
  const size_t LP = (size_t)p.LP;
  for (int row = tid; row < p.m; row += PG_THREADS) {
    double s = w[p.yg + row];
    const double* Yr = w + p.Y + (size_t)row * LP;
    for (int c = 0; c < 4 * p.L; ++c) s -= Yr[c] * w[p.rhs + c];
    w[p.z + row] = s;
  }
  __syncthreads();
  if (tid == 0) {
    const double* Lb = w + p.Lb;
    double h[PG_BW][4];
    for (int d = 0; d < PG_BW; ++d) for (int c = 0; c < 4; ++c) h[d][c] = 0.0;
    for (int Pb = nb - 1; Pb >= 0; --Pb) {
      double v[4];
      for (int c = 0; c < 4; ++c) v[c] = w[p.z + 4 * Pb + c];
#pragma unroll
      for (int d = 1; d <= PG_BW; ++d) {
        if (Pb + d >= nb) continue;
        const double* Lk = Lb + ((size_t)Pb * (PG_BW + 1) + d) * 16;   // block (Pb + d, Pb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) v[c] -= Lk[4 * r + c] * h[d - 1][r];
      }
      const double* Ld = Lb + (size_t)Pb * (PG_BW + 1) * 16;
#pragma unroll
      for (int c = 3; c >= 0; --c) {
#pragma unroll
        for (int r = c + 1; r < 4; ++r) v[c] -= Ld[4 * r + c] * v[r];
        v[c] = v[c] / Ld[5 * c];
      }
#pragma unroll
      for (int d = PG_BW - 1; d > 0; --d)
#pragma unroll
        for (int c = 0; c < 4; ++c) h[d][c] = h[d - 1][c];
#pragma unroll
      for (int c = 0; c < 4; ++c) { h[0][c] = v[c]; w[p.delta + 4 * Pb + c] = -v[c] * w[p.scale + 4 * Pb + c]; }
    }
  }
  __syncthreads();
  const double* dl = w + p.delta;
  for (int s = tid; s < p.E; s += PG_THREADS) {
    int a, b; bool loop;
    double acc = 0.0;
    if (pg_ends(p, ints, s, a, b, loop)) {
      const double *Ja = w + p.eJa + 16 * (size_t)s, *Jb = w + p.eJb + 16 * (size_t)s, *r = w + p.er + 4 * (size_t)s;
      for (int i = 0; i < 4; ++i) {
        double mi = 0.0;
        if (a >= 1) for (int c = 0; c < 4; ++c) mi += Ja[4 * i + c] * dl[4 * (a - 1) + c];
        for (int c = 0; c < 4; ++c) mi += Jb[4 * i + c] * dl[4 * (b - 1) + c];
        acc += mi * (r[i] + mi / 2.0);
      }
    }
    w[p.emod + s] = acc;
  }
  for (int i = tid; i < 4 * p.n; i += PG_THREADS) {
    const double xi = w[p.x + i];
    if (i < 4) { w[p.cand + i] = xi; continue; }
    const double moved = xi + dl[i - 4];
    w[p.cand + i] = (i & 3) == 0 ? pg_norm_angle(moved) : moved;
  }
  __syncthreads();
  const double mc = -pg_block_sum<PG_THREADS>(w + p.emod, p.E, red);
  if (tid == 0) { ctl[PG_MODEL] = mc; ctl[PG_STEP_VALID] = mc > 0.0 ? 1.0 : 0.0; }
}

// ---- one work-group per graph: the candidate's cost in fixed order, the tolerance tests, rho, the radius, accept or keep x
template <bool SEQ>
__global__ __launch_bounds__(PG_THREADS) void k_pg_decide(PgArgs A) {
  PG_GRAPH(A);
  if (ctl[PG_DONE] != 0.0) return;
  __shared__ double red[PG_THREADS];
  const int tid = threadIdx.x;
  if (ctl[PG_STEP_VALID] == 0.0) {   // HandleInvalidStep; the LM strategy's StepIsInvalid does nothing
    if (tid == 0) {
      ctl[PG_INVALID] += 1.0;
      if (ctl[PG_INVALID] >= (double)A.opt.max_consecutive_invalid_steps) { ctl[PG_TERM] = (double)VPL_PG_FAILURE; ctl[PG_DONE] = 1.0; }
      ctl[PG_LAST_OK] = 0.0;
    }
    return;
  }
  const int* fl = ints + p.itotal;   // SEQ: the node flags stand behind the graph's integer block
  auto is_const = [&](int k) { return SEQ && (fl[k] & PG_NODE_CONST); };   // node k
  double cand_cost = pg_block_sum<PG_THREADS>(w + p.ecand, p.E, red);
  double s = 0.0, bad = 0.0;
  for (int i = tid; i < p.m; i += PG_THREADS) {
    if (is_const(1 + (i >> 2))) continue;
    const double c = w[p.cand + 4 + i], d = w[p.x + 4 + i] - c;
    s += d * d;
    if (!(fabs(c) <= DBL_MAX)) bad = 1.0;
  }
  __syncthreads();
  red[tid] = s;
  __syncthreads();
  for (int h = PG_THREADS / 2; h > 0; h >>= 1) { if (tid < h) red[tid] += red[tid + h]; __syncthreads(); }
  const double step_norm = sqrt(red[0]);
  __syncthreads();
  red[tid] = bad;
  __syncthreads();
  for (int h = PG_THREADS / 2; h > 0; h >>= 1) { if (tid < h) red[tid] = fmax(red[tid], red[tid + h]); __syncthreads(); }
  if (red[0] != 0.0 || !(fabs(cand_cost) <= DBL_MAX)) cand_cost = DBL_MAX;
  __syncthreads();
  const double x_cost = ctl[PG_X_COST];
  int verdict = 0;   // 1: parameter tolerance, 2: function tolerance, 3: accepted, 4: rejected
  const double cc = x_cost - cand_cost, rho = cc / ctl[PG_MODEL];
  if (step_norm <= A.opt.parameter_tolerance * (ctl[PG_X_NORM] + A.opt.parameter_tolerance)) verdict = 1;
  else if (fabs(cc) <= A.opt.function_tolerance * x_cost) verdict = 2;
  else verdict = rho > A.opt.min_relative_decrease ? 3 : 4;
  double xn = 0.0;
  if (verdict == 3) {
    double s2 = 0.0;
    for (int i = tid; i < p.m; i += PG_THREADS) {
      if (is_const(1 + (i >> 2))) continue;
      const double c = w[p.cand + 4 + i]; w[p.x + 4 + i] = c; s2 += c * c;
    }
    __syncthreads();
    red[tid] = s2;
    __syncthreads();
    for (int h = PG_THREADS / 2; h > 0; h >>= 1) { if (tid < h) red[tid] += red[tid + h]; __syncthreads(); }
    xn = sqrt(red[0]);
  }
  if (tid != 0) return;
  ctl[PG_INVALID] = 0.0; ctl[PG_CAND_COST] = cand_cost; ctl[PG_RHO] = rho;
  if (verdict <= 2) { ctl[PG_TERM] = (double)VPL_PG_CONVERGENCE; ctl[PG_DONE] = 1.0; return; }
  if (verdict == 3) {
    const double t = 2.0 * rho - 1.0;
    ctl[PG_X_COST] = cand_cost; ctl[PG_X_NORM] = xn; ctl[PG_NEED_LIN] = 1.0; ctl[PG_LAST_OK] = 1.0;
    ctl[PG_RADIUS] = fmin(A.opt.max_radius, ctl[PG_RADIUS] / fmax(1.0 / 3.0, 1.0 - t * t * t));
    ctl[PG_DECREASE] = 2.0;
  } else {
    ctl[PG_LAST_OK] = 0.0;
    ctl[PG_RADIUS] = ctl[PG_RADIUS] / ctl[PG_DECREASE];
    ctl[PG_DECREASE] *= 2.0;
  }
}

// ---- the result: head, T, R = ypr2R(yaw, pitch0, roll0), the drift at node n-1, the tail
__global__ __launch_bounds__(PG_THREADS) void k_pg_finish(PgArgs A) {
  PG_GRAPH(A);
  double* out = A.out + G.out;
  const int tid = threadIdx.x, n = p.n;
  if (!G.run) { if (tid == 0) out[0] = (double)VPL_PG_UNSUPPORTED; return; }
  const double* in = A.in + G.in;
  const double *vT = in, *vR = in + 3 * (size_t)n, *tT = in + 12 * (size_t)n + 4 * (size_t)p.L, *tR = tT + 3 * (size_t)G.n_tail;
  double *oT = out + PG_HEAD, *oR = oT + 3 * (size_t)n, *otT = oR + 9 * (size_t)n, *otR = otT + 3 * (size_t)G.n_tail;
  auto pose = [&](int k) { return ypr2R(V3{w[p.x + 4 * k], w[p.pr + 2 * k], w[p.pr + 2 * k + 1]}); };
  for (int k = tid; k < n; k += PG_THREADS) {
    const M3 R = pose(k);
    for (int i = 0; i < 9; ++i) oR[9 * (size_t)k + i] = R.m[i];
    for (int i = 0; i < 3; ++i) oT[3 * (size_t)k + i] = w[p.x + 4 * k + 1 + i];
  }
  // the drift (pose_graph.cpp:549-557), by every thread alike: the tail needs it
  M3 Rv;
  for (int i = 0; i < 9; ++i) Rv.m[i] = vR[9 * (size_t)(n - 1) + i];
  const double yaw_drift = R2ypr(pose(n - 1)).x - R2ypr(Rv).x;
  const M3 rd = ypr2R(V3{yaw_drift, 0.0, 0.0});
  const V3 ct{w[p.x + 4 * (n - 1) + 1], w[p.x + 4 * (n - 1) + 2], w[p.x + 4 * (n - 1) + 3]};
  const V3 td = ct - mul(rd, V3{vT[3 * (n - 1)], vT[3 * (n - 1) + 1], vT[3 * (n - 1) + 2]});
  for (int k = tid; k < G.n_tail; k += PG_THREADS) {
    M3 R;
    for (int i = 0; i < 9; ++i) R.m[i] = tR[9 * (size_t)k + i];
    const V3 P = mul(rd, V3{tT[3 * k], tT[3 * k + 1], tT[3 * k + 2]}) + td;
    const M3 Rn = mul(rd, R);
    otT[3 * (size_t)k] = P.x; otT[3 * (size_t)k + 1] = P.y; otT[3 * (size_t)k + 2] = P.z;
    for (int i = 0; i < 9; ++i) otR[9 * (size_t)k + i] = Rn.m[i];
  }
  if (tid != 0) return;
  out[0] = (double)VPL_PG_OK; out[1] = ctl[PG_TERM]; out[2] = ctl[PG_ITER]; out[3] = ctl[PG_SUCC]; out[4] = ctl[PG_UNSUCC];
  out[5] = ctl[PG_INITIAL]; out[6] = ctl[PG_X_COST]; out[7] = yaw_drift;
  for (int i = 0; i < 9; ++i) out[8 + i] = rd.m[i];
  out[17] = td.x; out[18] = td.y; out[19] = td.z;
}

}  // namespace vpl
