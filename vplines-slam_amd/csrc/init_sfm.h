// Vision-only initial structure on the device (vpl_init_structure_batch): GlobalSFM::construct
// (vins_estimator/src/initial/initial_sfm.cpp:117-312) and the PnP of the non-key image frames (estimator.cpp:432-501).
//   k_sfm_construct  one work-group per sequence: the chain (PnP of the key frames, triangulation by the 4 x 4 null vector) from
//                    the host's schedule (init_sfm_plan.h), then the full BA;
//   k_sfm_frames     one work-group per non-key image frame: its PnP from the pose of the key frame estimator.cpp:440-453 picks;
//   k_sfm_finish     one wave per sequence: R / T of every image frame, the frame stage's failures.
// sfm_lm is the one minimiser behind the three solves: ceres' TrustRegionMinimizer with the Levenberg-Marquardt strategy and
// its defaults, the rules as k_line_opt (ba_lineopt.h) and the LM branch of oracle/problem.cpp state them, on
// ReprojectionError3D (initial_sfm.h:25-54) with analytic Jacobians and QuaternionParameterization.  A problem is a list of
// observations (camera slot, point, image point), a mask of free camera blocks and either free points -- each a 3 x 3 block
// eliminated into the reduced camera system -- or constant ones (PnP: rounded to float, as cv::Point3f / cv::Point2f do).
// FP64, wave64.  Every sum has a fixed order: per observation list in list order, over the work-group by block_sum.  Nothing
// depends on where a sequence sits in the batch.
#pragma once
#include "vplines_ba.h"
#include "vpl_math.h"
#include "ba_common.h"
#include "ba_solve.h"
#include "ba_lineopt.h"
#include "init_sfm_plan.h"

namespace vpl {

constexpr int SFM_THREADS = 256;
constexpr int SFM_NC = 6 * VPL_NFRAMES;     // local camera dims, constant blocks included
constexpr int SFM_NT = 4;                   // 16-tiles of the reduced camera system: 57 free dims of the BA and the rhs row
constexpr int SFM_NMAX = 16 * SFM_NT - 1;
static_assert(SFM_NC - 9 <= SFM_NMAX, "the BA's 57 free camera dims and the right-hand-side row fit four tiles");
// per observation, in doubles: r | Jc 2 x 6 (rotation, translation) | Jp 2 x 3 | W = Jc'^T Jp' 6 x 3 | Z = W V^-1 6 x 3
constexpr int SO_R = 0, SO_JC = 2, SO_JP = 14, SO_W = 20, SO_Z = 38, SFM_OBS_WS = 56;
// per free point: x | candidate | V^-1 (xx xy xz yy yz zz) | gradient | squared column norms | Jacobi scale | diagonal | step
constexpr int SP_X = 0, SP_X2 = 3, SP_VI = 6, SP_G = 12, SP_N = 15, SP_S = 18, SP_D = 21, SP_ST = 24, SFM_PT_WS = 27;
enum { SFM_NO_CONVERGENCE = 0, SFM_CONVERGENCE = 1, SFM_FAILURE = 2 };   // vpl_solve_report's codes
enum { SFM_STAGE_NONE = 0, SFM_STAGE_CHAIN = 1, SFM_STAGE_BA_RAN = 2, SFM_STAGE_BA_OK = 3 };

// One least-squares problem; the integers are offsets into the call's integer table, uv0 into its table of doubles.
struct DevSfmProb {
  int nobs, npt;              // npt = 0: the points are constant, rounded to float, and read by track index
  int o_cam, o_pt, o_uv;      // per observation: camera slot, point (free: index into the point list, constant: track), row of uv
  int p_trk, p_o0, p_n, p_c0; // per free point: its track, first observation, number of observations, first camera slot
  int c_off, c_list;          // c_off [12]: the observations of camera slot f are c_list[c_off[f] .. c_off[f + 1])
  int free_q, free_t;         // bit f: the rotation / translation of camera slot f is free
  int uv0;
  int pad_[2];
};
struct DevSfmEvent {
  int kind, f0, f1, list0, n, prob;
};
struct DevSfmSeq {
  int F, l, N, first_fail, frame_fail;
  int key[VPL_NFRAMES];
  int t_start, t_nobs, t_off, t_step;   // [N] tables
  int ev0, nev, ba_prob, uv0;
  int fr0, nfr;                          // its non-key frames
  int pad_;
  size_t ws_obs, ws_pt;                  // first observation / point of its workspaces
  double relR[9], relT[3], ric[9];
};
struct DevSfmFrame {
  int seq, f, guess, prob;
  size_t ws_obs;
};
struct DevSfmArgs {
  const DevSfmSeq* seqs;
  const DevSfmEvent* events;
  const DevSfmProb* probs;
  const DevSfmFrame* frames;
  const int* itab;
  const double* dtab;
  double* wo;            // [observations][SFM_OBS_WS]
  double* wp;            // [points][SFM_PT_WS]
  double* X;             // [n][VPL_SFM_MAX_TRACKS][3] the points: the chain's while it runs, then the BA's
  double* Xchain;        // the same after the chain
  int* stage;            // [n] SFM_STAGE_*
  int* frame_bad;        // [frames] the frame's PnP failed
  vpl_sfm_result* out;
};

struct SfmLds {
  double cq[4 * VPL_NFRAMES], ct[3 * VPL_NFRAMES], cq2[4 * VPL_NFRAMES], ct2[3 * VPL_NFRAMES];
  double gc[SFM_NC], nc[SFM_NC], sc[SFM_NC], dc[SFM_NC], stc[SFM_NC];
  double yv[16 * SFM_NT], isd[16 * SFM_NT], Linv[256], red[24];
  double S[SFM_NT * (SFM_NT + 1) / 2 * 256];
  int ridx[SFM_NC], rmap[SFM_NC], flag[4];
};
struct SfmReport {
  int iterations, successful, termination;
  double initial_cost, final_cost;
};

__device__ __forceinline__ Q4 sfm_loadq(const double* p) { return Q4{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void sfm_storeq(double* p, Q4 q) { p[0] = q.w; p[1] = q.x; p[2] = q.y; p[3] = q.z; }
__device__ __forceinline__ V3 sfm_load3(const double* p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ void sfm_store3(double* p, V3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
// QuaternionParameterization::Plus
__device__ __forceinline__ Q4 sfm_qplus(Q4 q, V3 d) {
  const double nd = sqrt(dot(d, d));
  if (!(nd > 0.0)) return q;
  const double s = sin(nd) / nd;
  return qmul(Q4{cos(nd), s * d.x, s * d.y, s * d.z}, q);
}
__device__ __forceinline__ double sfm_to_float(double x) { return (double)(float)x; }

// ReprojectionError3D of observation k under the cameras (cq, ct) and the current (cand = 0) or candidate points; jac: the
// Jacobians too, the rotation's in the local dims of Plus at delta = 0 -- R(Plus(q, delta)) = (I + 2 [delta]x) R(q) to first order
__device__ __forceinline__ void sfm_observation(const DevSfmProb& P, const int* itab, const double* dtab, const double* X, const double* wp,
                                                const double* cq, const double* ct, int k, int cand, bool jac, double* w) {
  const int f = itab[P.o_cam + k], j = itab[P.o_pt + k];
  const double* uv = dtab + P.uv0 + 2 * (size_t)itab[P.o_uv + k];
  V3 x;
  double u = uv[0], v = uv[1];
  if (P.npt) {
    x = sfm_load3(wp + (size_t)j * SFM_PT_WS + (cand ? SP_X2 : SP_X));
  } else {
    x = V3{sfm_to_float(X[3 * j]), sfm_to_float(X[3 * j + 1]), sfm_to_float(X[3 * j + 2])};
    u = sfm_to_float(u); v = sfm_to_float(v);
  }
  const M3 R = qmat(qnormalized(sfm_loadq(cq + 4 * f)));
  const V3 rx = mul(R, x), p = rx + sfm_load3(ct + 3 * f);
  const double iz = 1.0 / p.z;
  w[SO_R] = p.x * iz - u;
  w[SO_R + 1] = p.y * iz - v;
  if (!jac) return;
  const double d02 = -p.x * iz * iz, d12 = -p.y * iz * iz;
  double* jc = w + SO_JC;
  jc[0] = d02 * (2.0 * rx.y);                 jc[1] = iz * (2.0 * rx.z) + d02 * (-2.0 * rx.x); jc[2] = iz * (-2.0 * rx.y);
  jc[3] = iz; jc[4] = 0.0; jc[5] = d02;
  jc[6] = iz * (-2.0 * rx.z) + d12 * (2.0 * rx.y); jc[7] = d12 * (-2.0 * rx.x);               jc[8] = iz * (2.0 * rx.x);
  jc[9] = 0.0; jc[10] = iz; jc[11] = d12;
  double* jp = w + SO_JP;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    jp[c] = iz * R.m[c] + d02 * R.m[6 + c];
    jp[3 + c] = iz * R.m[3 + c] + d12 * R.m[6 + c];
  }
}

// squared norm of the free blocks of (a - b), b may be null: ceres' x_norm and step_norm
__device__ __forceinline__ double sfm_state_norm2(const DevSfmProb& P, const double* wp, const double* aq, const double* at, const double* bq,
                                                  const double* bt, int xa, int xb, double* red) {
  double s = 0.0;
  const int tid = threadIdx.x;
  if (tid < VPL_NFRAMES) {
    if (P.free_q >> tid & 1)
      for (int k = 0; k < 4; ++k) { const double d = aq[4 * tid + k] - (bq ? bq[4 * tid + k] : 0.0); s += d * d; }
    if (P.free_t >> tid & 1)
      for (int k = 0; k < 3; ++k) { const double d = at[3 * tid + k] - (bt ? bt[3 * tid + k] : 0.0); s += d * d; }
  }
  for (int u = tid; u < P.npt; u += SFM_THREADS) {
    const double* w = wp + (size_t)u * SFM_PT_WS;
    for (int k = 0; k < 3; ++k) { const double d = w[xa + k] - (xb >= 0 ? w[xb + k] : 0.0); s += d * d; }
  }
  return block_sum(s, red);
}

// Residuals, Jacobians, cost, gradient, squared column norms and ceres' gradient max norm at the current state.
__device__ __forceinline__ void sfm_linearise(const DevSfmProb& P, const int* itab, const double* dtab, const double* X, double* wo, double* wp,
                                              SfmLds& L, double& cost, double& gmax) {
  const int tid = threadIdx.x;
  double c = 0.0;
  for (int k = tid; k < P.nobs; k += SFM_THREADS) {
    double* w = wo + (size_t)k * SFM_OBS_WS;
    sfm_observation(P, itab, dtab, X, wp, L.cq, L.ct, k, 0, true, w);
    c += w[SO_R] * w[SO_R] + w[SO_R + 1] * w[SO_R + 1];
  }
  cost = block_sum(c, L.red) / 2.0;   // (its barriers order the stores above before the reads below)
  for (int idx = tid; idx < SFM_NC; idx += SFM_THREADS) {
    const int f = idx / 6, a = idx - 6 * f;
    double g = 0.0, n2 = 0.0;
    for (int kk = itab[P.c_off + f]; kk < itab[P.c_off + f + 1]; ++kk) {
      const double* w = wo + (size_t)itab[P.c_list + kk] * SFM_OBS_WS;
      const double j0 = w[SO_JC + a], j1 = w[SO_JC + 6 + a];
      g += j0 * w[SO_R] + j1 * w[SO_R + 1];
      n2 += j0 * j0 + j1 * j1;
    }
    L.gc[idx] = g; L.nc[idx] = n2;
  }
  double m = 0.0;
  for (int u = tid; u < P.npt; u += SFM_THREADS) {
    double* pw = wp + (size_t)u * SFM_PT_WS;
    double g[3] = {0, 0, 0}, n2[3] = {0, 0, 0};
    const int o0 = itab[P.p_o0 + u], no = itab[P.p_n + u];
    for (int o = o0; o < o0 + no; ++o) {
      const double* w = wo + (size_t)o * SFM_OBS_WS;
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) {
        g[cc] += w[SO_JP + cc] * w[SO_R] + w[SO_JP + 3 + cc] * w[SO_R + 1];
        n2[cc] += w[SO_JP + cc] * w[SO_JP + cc] + w[SO_JP + 3 + cc] * w[SO_JP + 3 + cc];
      }
    }
    for (int cc = 0; cc < 3; ++cc) {
      pw[SP_G + cc] = g[cc]; pw[SP_N + cc] = n2[cc];
      m = fmax(m, fabs(pw[SP_X + cc] - (pw[SP_X + cc] + -g[cc])));
    }
  }
  __syncthreads();
  if (tid < VPL_NFRAMES) {
    if (P.free_q >> tid & 1) {
      const Q4 q = sfm_loadq(L.cq + 4 * tid);
      const Q4 p = sfm_qplus(q, V3{-L.gc[6 * tid], -L.gc[6 * tid + 1], -L.gc[6 * tid + 2]});
      m = fmax(fmax(m, fabs(q.w - p.w)), fmax(fabs(q.x - p.x), fmax(fabs(q.y - p.y), fabs(q.z - p.z))));
    }
    if (P.free_t >> tid & 1)
      for (int k = 0; k < 3; ++k) m = fmax(m, fabs(L.ct[3 * tid + k] - (L.ct[3 * tid + k] + -L.gc[6 * tid + 3 + k])));
  }
  gmax = block_max(m, L.red);
}

// The Levenberg-Marquardt step in the Jacobi-scaled space into L.stc / the points' SP_ST; false: a factorisation failed.
__device__ __forceinline__ bool sfm_compute_step(const DevSfmProb& P, const int* itab, double* wo, double* wp, SfmLds& L, int n, double radius,
                                                 double& model_change) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nt = (n + 1 + 15) >> 4;
  if (tid < 4) L.flag[tid] = 0;
  __syncthreads();
  // ---- the points' 3 x 3 blocks: V = Jp'^T Jp' + D^2, inverted through its Cholesky factor
  for (int u = tid; u < P.npt; u += SFM_THREADS) {
    double* pw = wp + (size_t)u * SFM_PT_WS;
    const double s0 = pw[SP_S], s1 = pw[SP_S + 1], s2 = pw[SP_S + 2];
    double v00 = 0, v10 = 0, v11 = 0, v20 = 0, v21 = 0, v22 = 0;
    const int o0 = itab[P.p_o0 + u], no = itab[P.p_n + u];
    for (int o = o0; o < o0 + no; ++o) {
      const double* w = wo + (size_t)o * SFM_OBS_WS + SO_JP;
      const double a0 = w[0] * s0, a1 = w[1] * s1, a2 = w[2] * s2, b0 = w[3] * s0, b1 = w[4] * s1, b2 = w[5] * s2;
      v00 += a0 * a0 + b0 * b0; v10 += a1 * a0 + b1 * b0; v11 += a1 * a1 + b1 * b1;
      v20 += a2 * a0 + b2 * b0; v21 += a2 * a1 + b2 * b1; v22 += a2 * a2 + b2 * b2;
    }
    const double l0 = sqrt(pw[SP_D] / radius), l1 = sqrt(pw[SP_D + 1] / radius), l2 = sqrt(pw[SP_D + 2] / radius);
    v00 += l0 * l0; v11 += l1 * l1; v22 += l2 * l2;
    bool bad = !(v00 > 0.0);
    const double c00 = sqrt(v00), c10 = v10 / c00, c20 = v20 / c00;
    const double d1 = v11 - c10 * c10;
    bad = bad || !(d1 > 0.0);
    const double c11 = sqrt(d1), c21 = (v21 - c20 * c10) / c11;
    const double d2 = v22 - c20 * c20 - c21 * c21;
    bad = bad || !(d2 > 0.0);
    const double c22 = sqrt(d2);
    // C^-1 (lower), then V^-1 = C^-T C^-1
    const double i00 = 1.0 / c00, i11 = 1.0 / c11, i22 = 1.0 / c22;
    const double i10 = -c10 * i00 * i11, i21 = -c21 * i11 * i22, i20 = -(c20 * i00 + c21 * i10) * i22;
    pw[SP_VI + 0] = i00 * i00 + i10 * i10 + i20 * i20;
    pw[SP_VI + 1] = i10 * i11 + i20 * i21;
    pw[SP_VI + 2] = i20 * i22;
    pw[SP_VI + 3] = i11 * i11 + i21 * i21;
    pw[SP_VI + 4] = i21 * i22;
    pw[SP_VI + 5] = i22 * i22;
    if (bad) L.flag[1] = 1;
  }
  __syncthreads();
  if (L.flag[1]) return false;
  // ---- W = Jc'^T Jp' and Z = W V^-1 per observation
  if (P.npt)
    for (int k = tid; k < P.nobs; k += SFM_THREADS) {
      double* w = wo + (size_t)k * SFM_OBS_WS;
      const int f = itab[P.o_cam + k];
      const double* pw = wp + (size_t)itab[P.o_pt + k] * SFM_PT_WS;
      const double p0[3] = {w[SO_JP] * pw[SP_S], w[SO_JP + 1] * pw[SP_S + 1], w[SO_JP + 2] * pw[SP_S + 2]};
      const double p1[3] = {w[SO_JP + 3] * pw[SP_S], w[SO_JP + 4] * pw[SP_S + 1], w[SO_JP + 5] * pw[SP_S + 2]};
      const double* vi = pw + SP_VI;
      for (int a = 0; a < 6; ++a) {
        const double s = L.sc[6 * f + a], j0 = w[SO_JC + a] * s, j1 = w[SO_JC + 6 + a] * s;
        const double w0 = j0 * p0[0] + j1 * p1[0], w1 = j0 * p0[1] + j1 * p1[1], w2 = j0 * p0[2] + j1 * p1[2];
        w[SO_W + 3 * a] = w0; w[SO_W + 3 * a + 1] = w1; w[SO_W + 3 * a + 2] = w2;
        w[SO_Z + 3 * a] = w0 * vi[0] + w1 * vi[1] + w2 * vi[2];
        w[SO_Z + 3 * a + 1] = w0 * vi[1] + w1 * vi[3] + w2 * vi[4];
        w[SO_Z + 3 * a + 2] = w0 * vi[2] + w1 * vi[4] + w2 * vi[5];
      }
    }
  for (int i = tid; i < nt * (nt + 1) / 2 * 256; i += SFM_THREADS) L.S[i] = 0.0;
  __syncthreads();
  // ---- the reduced camera system, one owner per entry of the lower triangle and of the right-hand-side row n:
  //      S = Hcc' + Dc^2 - sum over the points of W V^-1 W^T, the row g' - sum of W V^-1 gp'
  const int ntri = n * (n + 1) / 2;
  for (int e = tid; e < ntri + n; e += SFM_THREADS) {
    int i, j;
    if (e < ntri) tri_decode(e, i, j); else { i = n; j = e - ntri; }
    const int cb = L.rmap[j], g = cb / 6, b = cb - 6 * g;
    double val = 0.0;
    if (i < n) {
      const int ca = L.rmap[i], f = ca / 6, a = ca - 6 * f;
      if (f == g) {
        for (int kk = itab[P.c_off + f]; kk < itab[P.c_off + f + 1]; ++kk) {
          const double* w = wo + (size_t)itab[P.c_list + kk] * SFM_OBS_WS + SO_JC;
          val += w[a] * w[b] + w[6 + a] * w[6 + b];
        }
        val *= L.sc[ca] * L.sc[cb];
        if (i == j) { const double lm = sqrt(L.dc[ca] / radius); val += lm * lm; }
      }
      for (int u = 0; u < P.npt; ++u) {
        const int c0 = itab[P.p_c0 + u], no = itab[P.p_n + u];
        if (f < c0 || f >= c0 + no || g < c0 || g >= c0 + no) continue;
        const int o0 = itab[P.p_o0 + u];
        const double* z = wo + (size_t)(o0 + f - c0) * SFM_OBS_WS + SO_Z + 3 * a;
        const double* w = wo + (size_t)(o0 + g - c0) * SFM_OBS_WS + SO_W + 3 * b;
        val -= z[0] * w[0] + z[1] * w[1] + z[2] * w[2];
      }
      L.S[tix(i, j)] = val;
      if ((i >> 4) == (j >> 4) && i != j) L.S[tix(j, i)] = val;   // diagonal tiles are kept as full squares
    } else {
      val = L.gc[cb] * L.sc[cb];
      if (P.npt)
        for (int kk = itab[P.c_off + g]; kk < itab[P.c_off + g + 1]; ++kk) {
          const int k = itab[P.c_list + kk];
          const double* z = wo + (size_t)k * SFM_OBS_WS + SO_Z + 3 * b;
          const double* pw = wp + (size_t)itab[P.o_pt + k] * SFM_PT_WS;
          val -= z[0] * (pw[SP_G] * pw[SP_S]) + z[1] * (pw[SP_G + 1] * pw[SP_S + 1]) + z[2] * (pw[SP_G + 2] * pw[SP_S + 2]);
        }
      L.S[tix(n, j)] = val;
    }
  }
  for (int r = n + 1 + tid; r < 16 * nt; r += SFM_THREADS) L.S[tix(r, r)] = 1.0;   // padding rows: unit pivots, never used
  __syncthreads();
  if (!tile_cholesky(L.S, L.Linv, L.isd, L.flag, nt, n, SFM_THREADS / 64, lane, wv, nullptr)) return false;
  tile_back_substitute(L.S, L.isd, L.yv, nt, n, tid, SFM_THREADS, lane, wv);
  for (int idx = tid; idx < SFM_NC; idx += SFM_THREADS) L.stc[idx] = L.ridx[idx] >= 0 ? -L.yv[L.ridx[idx]] : 0.0;
  __syncthreads();
  // ---- the points' steps: -V^-1 (gp' - W^T y)
  for (int u = tid; u < P.npt; u += SFM_THREADS) {
    double* pw = wp + (size_t)u * SFM_PT_WS;
    double t[3] = {pw[SP_G] * pw[SP_S], pw[SP_G + 1] * pw[SP_S + 1], pw[SP_G + 2] * pw[SP_S + 2]};
    const int o0 = itab[P.p_o0 + u], no = itab[P.p_n + u], c0 = itab[P.p_c0 + u];
    for (int o = 0; o < no; ++o) {
      const double* w = wo + (size_t)(o0 + o) * SFM_OBS_WS + SO_W;
      for (int a = 0; a < 6; ++a) {
        const double y = -L.stc[6 * (c0 + o) + a];
        t[0] -= w[3 * a] * y; t[1] -= w[3 * a + 1] * y; t[2] -= w[3 * a + 2] * y;
      }
    }
    const double* vi = pw + SP_VI;
    pw[SP_ST] = -(vi[0] * t[0] + vi[1] * t[1] + vi[2] * t[2]);
    pw[SP_ST + 1] = -(vi[1] * t[0] + vi[3] * t[1] + vi[4] * t[2]);
    pw[SP_ST + 2] = -(vi[2] * t[0] + vi[4] * t[1] + vi[5] * t[2]);
  }
  __syncthreads();
  // ---- model_cost_change = -sum m (r + m / 2), m = J' step
  double mc = 0.0;
  for (int k = tid; k < P.nobs; k += SFM_THREADS) {
    const double* w = wo + (size_t)k * SFM_OBS_WS;
    const int f = itab[P.o_cam + k];
    double m0 = 0.0, m1 = 0.0;
    for (int a = 0; a < 6; ++a) {
      const double s = L.sc[6 * f + a] * L.stc[6 * f + a];
      m0 += w[SO_JC + a] * s; m1 += w[SO_JC + 6 + a] * s;
    }
    if (P.npt) {
      const double* pw = wp + (size_t)itab[P.o_pt + k] * SFM_PT_WS;
      for (int cc = 0; cc < 3; ++cc) {
        const double s = pw[SP_S + cc] * pw[SP_ST + cc];
        m0 += w[SO_JP + cc] * s; m1 += w[SO_JP + 3 + cc] * s;
      }
    }
    mc += m0 * (w[SO_R] + m0 / 2.0) + m1 * (w[SO_R + 1] + m1 / 2.0);
  }
  model_change = -block_sum(mc, L.red);
  return true;
}

// Minimises from the cameras in L.cq / L.ct and, with free points, from the points' SP_X; leaves the minimiser there.  X: the
// constant points by track.  Every thread of the work-group calls it and gets the same report.
__device__ __forceinline__ SfmReport sfm_lm(const DevSfmProb& P, const int* itab, const double* dtab, const double* X, double* wo, double* wp,
                                            SfmLds& L) {
  const int tid = threadIdx.x;
  // reduced index of every free camera dim, in camera order
  if (tid == 0) {
    int n = 0;
    for (int f = 0; f < VPL_NFRAMES; ++f)
      for (int a = 0; a < 6; ++a) {
        const bool fr = ((a < 3 ? P.free_q : P.free_t) >> f & 1) != 0;
        L.ridx[6 * f + a] = fr ? n : -1;
        if (fr) L.rmap[n++] = 6 * f + a;
      }
    L.flag[2] = n;
  }
  __syncthreads();
  const int n = L.flag[2];
  SfmReport rep{0, 0, SFM_FAILURE, 0.0, 0.0};
  double cost, gmax;
  sfm_linearise(P, itab, dtab, X, wo, wp, L, cost, gmax);
  rep.initial_cost = rep.final_cost = cost;
  if (!isfinite(cost) || n < 1 || n > SFM_NMAX) return rep;
  for (int idx = tid; idx < SFM_NC; idx += SFM_THREADS) L.sc[idx] = 1.0 / (1.0 + sqrt(L.nc[idx]));
  for (int u = tid; u < P.npt; u += SFM_THREADS) {
    double* pw = wp + (size_t)u * SFM_PT_WS;
    for (int cc = 0; cc < 3; ++cc) pw[SP_S + cc] = 1.0 / (1.0 + sqrt(pw[SP_N + cc]));
  }
  double x_norm = sqrt(sfm_state_norm2(P, wp, L.cq, L.ct, nullptr, nullptr, SP_X, -1, L.red));
  double radius = 1e4, decrease_factor = 2.0;
  bool reuse_diagonal = false, last_successful = true;
  int iter = 0, status;
  for (;;) {
    if (iter >= 50) { status = SFM_NO_CONVERGENCE; break; }
    if (last_successful && gmax <= 1e-10) { status = SFM_CONVERGENCE; break; }
    if (radius <= 1e-32) { status = SFM_CONVERGENCE; break; }
    ++iter;
    if (!reuse_diagonal) {
      for (int idx = tid; idx < SFM_NC; idx += SFM_THREADS) L.dc[idx] = fmin(fmax(L.nc[idx] * L.sc[idx] * L.sc[idx], 1e-6), 1e32);
      for (int u = tid; u < P.npt; u += SFM_THREADS) {
        double* pw = wp + (size_t)u * SFM_PT_WS;
        for (int cc = 0; cc < 3; ++cc) pw[SP_D + cc] = fmin(fmax(pw[SP_N + cc] * pw[SP_S + cc] * pw[SP_S + cc], 1e-6), 1e32);
      }
    }
    __syncthreads();
    double model_change = 0.0;
    // an invalid step repeats itself bit for bit until ceres gives up (StepIsInvalid is empty for this strategy): FAILURE at once
    if (!sfm_compute_step(P, itab, wo, wp, L, n, radius, model_change) || !isfinite(model_change) || !(model_change > 0.0)) {
      status = SFM_FAILURE; --iter; break;
    }
    // ---- candidate = Plus(x, step * scale), its cost
    if (tid < VPL_NFRAMES) {
      const double* st = L.stc + 6 * tid;
      const double* s = L.sc + 6 * tid;
      Q4 q = sfm_loadq(L.cq + 4 * tid);
      if (P.free_q >> tid & 1) q = sfm_qplus(q, V3{st[0] * s[0], st[1] * s[1], st[2] * s[2]});
      sfm_storeq(L.cq2 + 4 * tid, q);
      for (int k = 0; k < 3; ++k) L.ct2[3 * tid + k] = (P.free_t >> tid & 1) ? L.ct[3 * tid + k] + st[3 + k] * s[3 + k] : L.ct[3 * tid + k];
    }
    for (int u = tid; u < P.npt; u += SFM_THREADS) {
      double* pw = wp + (size_t)u * SFM_PT_WS;
      for (int cc = 0; cc < 3; ++cc) pw[SP_X2 + cc] = pw[SP_X + cc] + pw[SP_ST + cc] * pw[SP_S + cc];
    }
    __syncthreads();
    double c = 0.0;
    for (int k = tid; k < P.nobs; k += SFM_THREADS) {
      double r[2];
      sfm_observation(P, itab, dtab, X, wp, L.cq2, L.ct2, k, 1, false, r);
      c += r[0] * r[0] + r[1] * r[1];
    }
    double cand_cost = block_sum(c, L.red) / 2.0;
    if (!isfinite(cand_cost)) cand_cost = 1.7976931348623157e308;
    const double step_norm = sqrt(sfm_state_norm2(P, wp, L.cq, L.ct, L.cq2, L.ct2, SP_X, SP_X2, L.red));
    if (!isfinite(step_norm)) { status = SFM_FAILURE; --iter; break; }
    // a tolerance fires before the iteration is recorded
    if (step_norm <= 1e-8 * (x_norm + 1e-8)) { status = SFM_CONVERGENCE; --iter; break; }
    if (fabs(cost - cand_cost) <= 1e-6 * cost) { status = SFM_CONVERGENCE; --iter; break; }
    const double rho = (cost - cand_cost) / model_change;
    if (rho > 1e-3) {
      for (int k = tid; k < 4 * VPL_NFRAMES; k += SFM_THREADS) L.cq[k] = L.cq2[k];
      for (int k = tid; k < 3 * VPL_NFRAMES; k += SFM_THREADS) L.ct[k] = L.ct2[k];
      for (int u = tid; u < P.npt; u += SFM_THREADS) {
        double* pw = wp + (size_t)u * SFM_PT_WS;
        for (int cc = 0; cc < 3; ++cc) pw[SP_X + cc] = pw[SP_X2 + cc];
      }
      __syncthreads();
      x_norm = sqrt(sfm_state_norm2(P, wp, L.cq, L.ct, nullptr, nullptr, SP_X, -1, L.red));
      sfm_linearise(P, itab, dtab, X, wo, wp, L, cost, gmax);
      if (!isfinite(cost)) { status = SFM_FAILURE; break; }
      last_successful = true;
      ++rep.successful;
      radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * rho - 1.0, 3.0)));
      decrease_factor = 2.0;
      reuse_diagonal = false;
    } else {
      last_successful = false;
      radius = radius / decrease_factor;
      decrease_factor *= 2.0;
      reuse_diagonal = true;
    }
  }
  rep.iterations = iter;
  rep.termination = status;
  rep.final_cost = cost;
  __syncthreads();
  return rep;
}

// GlobalSFM::triangulatePoint from the cameras (cq normalised, ct) of window frames f0, f1
__device__ __forceinline__ V3 sfm_triangulate(const double* cq, const double* ct, int f0, int f1, const double* x0, const double* x1) {
  const M3 R0 = qmat(sfm_loadq(cq + 4 * f0)), R1 = qmat(sfm_loadq(cq + 4 * f1));
  const double* t0 = ct + 3 * f0;
  const double* t1 = ct + 3 * f1;
  double A[16], V[16];
  for (int c = 0; c < 4; ++c) {
    const double p00 = c < 3 ? R0.m[c] : t0[0], p01 = c < 3 ? R0.m[3 + c] : t0[1], p02 = c < 3 ? R0.m[6 + c] : t0[2];
    const double p10 = c < 3 ? R1.m[c] : t1[0], p11 = c < 3 ? R1.m[3 + c] : t1[1], p12 = c < 3 ? R1.m[6 + c] : t1[2];
    A[c] = x0[0] * p02 - p00;
    A[4 + c] = x0[1] * p02 - p01;
    A[8 + c] = x1[0] * p12 - p10;
    A[12 + c] = x1[1] * p12 - p11;
  }
  const int cm = dlt_null_column(A, 4, V);
  const double w = V[12 + cm];
  return V3{V[cm] / w, V[4 + cm] / w, V[8 + cm] / w};
}

__device__ __forceinline__ bool sfm_finite(const double* p, int n) {
  bool ok = true;
  for (int k = 0; k < n; ++k) ok = ok && isfinite(p[k]);
  return ok;
}

__global__ __launch_bounds__(SFM_THREADS) void k_sfm_construct(DevSfmArgs A) {
  __shared__ SfmLds L;
  const int s = blockIdx.x, tid = threadIdx.x;
  const DevSfmSeq& q = A.seqs[s];
  vpl_sfm_result& o = A.out[s];
  const int* itab = A.itab;
  double* X = A.X + (size_t)s * VPL_SFM_MAX_TRACKS * 3;
  double* Xc = A.Xchain + (size_t)s * VPL_SFM_MAX_TRACKS * 3;
  double* wo = A.wo + q.ws_obs * SFM_OBS_WS;
  double* wp = A.wp + q.ws_pt * SFM_PT_WS;
  for (int k = tid; k < VPL_NFRAMES; k += SFM_THREADS) o.pnp_iterations[k] = -1;
  for (int k = tid; k < VPL_INIT_MAX_FRAMES; k += SFM_THREADS) o.frame_iterations[k] = -1;
  if (q.first_fail >= 0) {   // a starved PnP: construct returns false there, nothing is handed out
    if (tid == 0) o.fail = VPL_SFM_FAIL_KEY_PNP;
    return;
  }
  // ---- frames l and 10 from the relative pose (:125-153)
  if (tid < VPL_NFRAMES) {
    sfm_storeq(L.cq + 4 * tid, Q4{1.0, 0.0, 0.0, 0.0});
    sfm_store3(L.ct + 3 * tid, V3{0.0, 0.0, 0.0});
  }
  __syncthreads();
  if (tid == 0) {
    M3 Rr;
    for (int k = 0; k < 9; ++k) Rr.m[k] = q.relR[k];
    const Q4 c10 = qnormalized(qinv(mat2q(Rr)));
    sfm_storeq(L.cq + 4 * VPL_WINDOW_SIZE, c10);
    sfm_store3(L.ct + 3 * VPL_WINDOW_SIZE, -mul(qmat(c10), sfm_load3(q.relT)));
  }
  __syncthreads();
  // ---- the chain, event by event
  const double* obs = A.dtab + q.uv0;
  for (int e = 0; e < q.nev; ++e) {
    const DevSfmEvent ev = A.events[q.ev0 + e];
    if (ev.kind == SFM_EV_PNP) {
      if (tid == 0) {
        for (int k = 0; k < 4; ++k) L.cq[4 * ev.f0 + k] = L.cq[4 * ev.f1 + k];
        for (int k = 0; k < 3; ++k) L.ct[3 * ev.f0 + k] = L.ct[3 * ev.f1 + k];
      }
      __syncthreads();
      const SfmReport rep = sfm_lm(A.probs[ev.prob], itab, A.dtab, X, wo, wp, L);
      if (tid == 0) {
        o.pnp_iterations[ev.f0] = rep.iterations;
        sfm_storeq(L.cq + 4 * ev.f0, qnormalized(sfm_loadq(L.cq + 4 * ev.f0)));
      }
      if (rep.termination == SFM_FAILURE) {
        if (tid == 0) o.fail = VPL_SFM_FAIL_NUMERIC;
        return;
      }
      __syncthreads();
    } else {
      for (int kk = tid; kk < ev.n; kk += SFM_THREADS) {
        const int j = itab[ev.list0 + kk];
        const int st = itab[q.t_start + j], no = itab[q.t_nobs + j], off = itab[q.t_off + j];
        const int f0 = ev.kind == SFM_EV_TRI ? ev.f0 : st, f1 = ev.kind == SFM_EV_TRI ? ev.f1 : st + no - 1;
        sfm_store3(X + 3 * j, sfm_triangulate(L.cq, L.ct, f0, f1, obs + 2 * (size_t)(off + f0 - st), obs + 2 * (size_t)(off + f1 - st)));
      }
      __syncthreads();
    }
  }
  // ---- what the chain leaves
  double bad = 0.0;
  for (int j = tid; j < q.N; j += SFM_THREADS)
    if (itab[q.t_step + j] >= 0 && !sfm_finite(X + 3 * j, 3)) bad = 1.0;
  if (tid == 0 && !(sfm_finite(L.cq, 4 * VPL_NFRAMES) && sfm_finite(L.ct, 3 * VPL_NFRAMES))) bad = 1.0;
  if (block_sum(bad, L.red) > 0.0) {
    if (tid == 0) o.fail = VPL_SFM_FAIL_NUMERIC;
    return;
  }
  for (int k = tid; k < 4 * VPL_NFRAMES; k += SFM_THREADS) o.chain_q[k / 4][k % 4] = L.cq[k];
  for (int k = tid; k < 3 * VPL_NFRAMES; k += SFM_THREADS) o.chain_t[k / 3][k % 3] = L.ct[k];
  for (int k = tid; k < 3 * q.N; k += SFM_THREADS) Xc[k] = itab[q.t_step + k / 3] >= 0 ? X[k] : 0.0;
  if (tid == 0) A.stage[s] = SFM_STAGE_CHAIN;
  // ---- the full BA (:232-289)
  const DevSfmProb& B = A.probs[q.ba_prob];
  for (int u = tid; u < B.npt; u += SFM_THREADS) sfm_store3(wp + (size_t)u * SFM_PT_WS + SP_X, sfm_load3(X + 3 * itab[B.p_trk + u]));
  __syncthreads();
  const SfmReport rep = sfm_lm(B, itab, A.dtab, X, wo, wp, L);
  for (int u = tid; u < B.npt; u += SFM_THREADS) sfm_store3(X + 3 * itab[B.p_trk + u], sfm_load3(wp + (size_t)u * SFM_PT_WS + SP_X));
  for (int k = tid; k < 4 * VPL_NFRAMES; k += SFM_THREADS) o.ba_q[k / 4][k % 4] = L.cq[k];
  for (int k = tid; k < 3 * VPL_NFRAMES; k += SFM_THREADS) o.ba_t[k / 3][k % 3] = L.ct[k];
  bad = 0.0;
  for (int u = tid; u < B.npt; u += SFM_THREADS)
    if (!sfm_finite(wp + (size_t)u * SFM_PT_WS + SP_X, 3)) bad = 1.0;
  if (tid == 0 && !(sfm_finite(L.cq, 4 * VPL_NFRAMES) && sfm_finite(L.ct, 3 * VPL_NFRAMES) && isfinite(rep.final_cost))) bad = 1.0;
  bad = block_sum(bad, L.red);
  int fail = 0;
  if (rep.termination == SFM_FAILURE || bad > 0.0) fail = VPL_SFM_FAIL_NUMERIC;
  else if (!(rep.termination == SFM_CONVERGENCE || rep.final_cost < 5e-3)) fail = VPL_SFM_FAIL_BA;
  if (tid == 0) {
    o.iterations = rep.iterations; o.successful_steps = rep.successful; o.termination = rep.termination;
    o.initial_cost = rep.initial_cost; o.final_cost = rep.final_cost;
    o.fail = fail;
    A.stage[s] = fail ? SFM_STAGE_BA_RAN : SFM_STAGE_BA_OK;
  }
  if (fail) return;
  // ---- q, T as construct returns them (:290-304)
  if (tid < VPL_NFRAMES) {
    const Q4 qi = qinv(sfm_loadq(L.cq + 4 * tid));
    sfm_storeq(o.Q[tid], qi);
    sfm_store3(o.T[tid], -mul(qmat(qi), sfm_load3(L.ct + 3 * tid)));
  }
  if (tid == 0) o.n_tracked = B.npt;
}

__global__ __launch_bounds__(SFM_THREADS) void k_sfm_frames(DevSfmArgs A) {
  __shared__ SfmLds L;
  const DevSfmFrame& fr = A.frames[blockIdx.x];
  const DevSfmSeq& q = A.seqs[fr.seq];
  vpl_sfm_result& o = A.out[fr.seq];
  const int tid = threadIdx.x;
  if (o.fail != 0 || q.frame_fail) return;   // the sequence failed before, or fails whatever this frame gives
  if (tid < VPL_NFRAMES) {
    sfm_storeq(L.cq + 4 * tid, Q4{1.0, 0.0, 0.0, 0.0});
    sfm_store3(L.ct + 3 * tid, V3{0.0, 0.0, 0.0});
  }
  __syncthreads();
  if (tid == 0) {   // the guess (:452-453)
    const Q4 q0 = qinv(sfm_loadq(o.Q[fr.guess]));
    sfm_storeq(L.cq, q0);
    sfm_store3(L.ct, -mul(qmat(q0), sfm_load3(o.T[fr.guess])));
  }
  __syncthreads();
  const SfmReport rep = sfm_lm(A.probs[fr.prob], A.itab, A.dtab, A.X + (size_t)fr.seq * VPL_SFM_MAX_TRACKS * 3, A.wo + fr.ws_obs * SFM_OBS_WS,
                               nullptr, L);
  if (tid == 0) {
    o.frame_iterations[fr.f] = rep.iterations;
    if (rep.termination == SFM_FAILURE || !sfm_finite(L.cq, 4) || !sfm_finite(L.ct, 3)) {
      A.frame_bad[blockIdx.x] = 1;
    } else {   // :492-500
      const M3 Rp = transpose(qmat(qnormalized(sfm_loadq(L.cq))));
      M3 ric;
      for (int k = 0; k < 9; ++k) ric.m[k] = q.ric[k];
      const M3 R = mul(Rp, transpose(ric));
      for (int k = 0; k < 9; ++k) o.frame_R[fr.f][k] = R.m[k];
      sfm_store3(o.frame_T[fr.f], mul(Rp, -sfm_load3(L.ct)));
    }
  }
}

__global__ __launch_bounds__(64) void k_sfm_finish(DevSfmArgs A) {
  const DevSfmSeq& q = A.seqs[blockIdx.x];
  vpl_sfm_result& o = A.out[blockIdx.x];
  const int tid = threadIdx.x;
  __shared__ int fail_s;
  if (o.fail != 0) return;
  if (tid == 0) {
    int fail = q.frame_fail ? VPL_SFM_FAIL_FRAME_PNP : 0;
    for (int k = 0; k < q.nfr; ++k)
      if (A.frame_bad[q.fr0 + k]) fail |= VPL_SFM_FAIL_NUMERIC;
    fail_s = fail;
    o.fail = fail;
    o.ok = fail ? 0 : 1;
  }
  __syncthreads();
  if (fail_s) {   // nothing of the frame stage is handed out
    for (int k = tid; k < VPL_INIT_MAX_FRAMES * 9; k += 64) o.frame_R[0][k] = 0.0;
    for (int k = tid; k < VPL_INIT_MAX_FRAMES * 3; k += 64) o.frame_T[0][k] = 0.0;
    return;
  }
  if (tid < VPL_NFRAMES) {   // the key frames (:443-444)
    M3 ric;
    for (int k = 0; k < 9; ++k) ric.m[k] = q.ric[k];
    const M3 R = mul(qmat(sfm_loadq(o.Q[tid])), transpose(ric));
    const int f = q.key[tid];
    for (int k = 0; k < 9; ++k) o.frame_R[f][k] = R.m[k];
    for (int k = 0; k < 3; ++k) o.frame_T[f][k] = o.T[tid][k];
  }
}

}  // namespace vpl
