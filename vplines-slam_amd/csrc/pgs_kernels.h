// Device side of the pose-graph session (vpl_pgs_*; DESIGN.md, "Pose-graph session"): the keyframe list of PoseGraph resident on
// the device -- per keyframe the shifted VIO pose, the pose and loop_info -- and the state that goes with it, w_r_vio / w_t_vio
// and the drift.  k_pgs_add is addKeyFrame / loadKeyFrame, k_pgs_gather and k_pgs_scatter stand around the rounds of
// pg_kernels.h in one turn of optimize4DoF, k_pgs_update_loop is updateKeyFrameLoop.
// The state has two copies: a launch reads one and writes the other, the host swaps them after every launch that writes, so the
// lanes that all need the state never race with the one that renews it.  f64, no atomics; what several lanes need they each
// compute from the same operands by the same code.
#pragma once
#include <hip/hip_runtime.h>

#include "pg_kernels.h"

namespace vpl {

constexpr int PGS_THREADS = 256;
constexpr int PGS_STATE = 32;   // doubles of one copy of the state
enum PgsSt { PGS_W_R = 0, PGS_W_T = 9, PGS_R_DRIFT = 12, PGS_T_DRIFT = 21, PGS_YAW_DRIFT = 24 };
constexpr int PGS_OUT = 48;     // doubles of the record of vpl_pgs_add_keyframe: vio_T, vio_R, T, R, w_r_vio, w_t_vio

struct PgsList {
  double *vT, *vR, *T, *R, *li;   // [cap][3], [cap][9], [cap][3], [cap][9], [cap][8]
  int* seq;                       // [cap]
};

struct PgsAddArgs {
  PgsList L;
  const double* st_in;
  double *st_out, *out;   // out: null, or PGS_OUT doubles
  int index, sequence, loop_index, new_sequence, shift_list, load;
  double vio_T[3], vio_R[9], T[3], R[9], loop_info[8];
};

__device__ __forceinline__ M3 pgs_m3(const double* p) { M3 R; for (int i = 0; i < 9; ++i) R.m[i] = p[i]; return R; }
__device__ __forceinline__ V3 pgs_v3(const double* p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ void pgs_put(double* p, const M3& R) { for (int i = 0; i < 9; ++i) p[i] = R.m[i]; }
__device__ __forceinline__ void pgs_put(double* p, V3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }

// shift_yaw / shift_r / shift_t (pose_graph.cpp:85-101, :897-914): the old keyframe's pose (oP, oR) and the loop's relative pose
// against the current keyframe's VIO pose (P, R)
__device__ __forceinline__ void pgs_shift(V3 oP, const M3& oR, const double* li, V3 P, const M3& R, double& yaw, M3& sr, V3& stv) {
  const V3 wP = mul(oR, pgs_v3(li)) + oP;
  const M3 wR = mul(oR, qmat(Q4{li[3], li[4], li[5], li[6]}));
  yaw = R2ypr(wR).x - R2ypr(R).x;
  sr = ypr2R(V3{yaw, 0.0, 0.0});
  stv = wP - mul(mul(wR, transpose(R)), P);
}

// ---- addKeyFrame (pose_graph.cpp:42-136) / loadKeyFrame (:213-287).  Every lane follows the new keyframe as far as the shift of
//      the list needs; lane 0 stores it, the state and the record; with shift_list lane k also shifts stored keyframe k if it is of
//      the new keyframe's sequence (the old keyframe of the loop is of another one, so nobody reads what another lane writes)
__global__ __launch_bounds__(PGS_THREADS) void k_pgs_add(PgsAddArgs A) {
  const int t = blockIdx.x * PGS_THREADS + threadIdx.x;
  const PgsList& L = A.L;
  M3 w_r = pgs_m3(A.st_in + PGS_W_R), r_drift = pgs_m3(A.st_in + PGS_R_DRIFT);
  V3 w_t = pgs_v3(A.st_in + PGS_W_T), t_drift = pgs_v3(A.st_in + PGS_T_DRIFT);
  double yaw_drift = A.st_in[PGS_YAW_DRIFT];
  if (A.new_sequence) {
    for (int i = 0; i < 9; ++i) w_r.m[i] = (i % 4 == 0) ? 1.0 : 0.0;
    r_drift = w_r;
    w_t = V3{0.0, 0.0, 0.0}; t_drift = w_t;
    // (yaw_drift is not reset at :47-57)
  }
  V3 P = pgs_v3(A.vio_T);
  M3 R = pgs_m3(A.vio_R);
  if (!A.load) { P = mul(w_r, P) + w_t; R = mul(w_r, R); }
  if (!A.load && A.shift_list) {
    double yaw; M3 sr; V3 stv;
    pgs_shift(pgs_v3(L.vT + 3 * (size_t)A.loop_index), pgs_m3(L.vR + 9 * (size_t)A.loop_index), A.loop_info, P, R, yaw, sr, stv);
    w_r = sr; w_t = stv;
    P = mul(w_r, P) + w_t; R = mul(w_r, R);
    if (t < A.index && L.seq[t] == A.sequence) {
      pgs_put(L.vT + 3 * (size_t)t, mul(w_r, pgs_v3(L.vT + 3 * (size_t)t)) + w_t);
      pgs_put(L.vR + 9 * (size_t)t, mul(w_r, pgs_m3(L.vR + 9 * (size_t)t)));
    }
  }
  if (t != 0) return;
  const V3 pT = A.load ? pgs_v3(A.T) : mul(r_drift, P) + t_drift;
  const M3 pR = A.load ? pgs_m3(A.R) : mul(r_drift, R);
  const size_t k = (size_t)A.index;
  pgs_put(L.vT + 3 * k, P); pgs_put(L.vR + 9 * k, R); pgs_put(L.T + 3 * k, pT); pgs_put(L.R + 9 * k, pR);
  for (int i = 0; i < 8; ++i) L.li[8 * k + i] = A.loop_index >= 0 ? A.loop_info[i] : 0.0;
  L.seq[k] = A.sequence;
  pgs_put(A.st_out + PGS_W_R, w_r); pgs_put(A.st_out + PGS_W_T, w_t);
  pgs_put(A.st_out + PGS_R_DRIFT, r_drift); pgs_put(A.st_out + PGS_T_DRIFT, t_drift);
  A.st_out[PGS_YAW_DRIFT] = yaw_drift;
  if (A.out) {
    pgs_put(A.out, P); pgs_put(A.out + 3, R); pgs_put(A.out + 12, pT); pgs_put(A.out + 15, pR);
    pgs_put(A.out + 24, w_r); pgs_put(A.out + 33, w_t);
  }
}

// ---- updateKeyFrameLoop (:889-922) behind its gate, which the host has taken: the keyframe's loop_info is replaced; fast: the drift
//      is overwritten from the old keyframe's POSE
struct PgsLoopArgs {
  PgsList L;
  const double* st_in;
  double* st_out;
  int index, old_index, fast;
  double loop_info[8];
};
__global__ __launch_bounds__(64) void k_pgs_update_loop(PgsLoopArgs A) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const PgsList& L = A.L;
  const size_t k = (size_t)A.index, o = (size_t)A.old_index;
  for (int i = 0; i < 8; ++i) L.li[8 * k + i] = A.loop_info[i];
  for (int i = 0; i < PGS_STATE; ++i) A.st_out[i] = A.st_in[i];
  if (!A.fast) return;
  double yaw; M3 sr; V3 stv;
  pgs_shift(pgs_v3(L.T + 3 * o), pgs_m3(L.R + 9 * o), A.loop_info, pgs_v3(L.vT + 3 * k), pgs_m3(L.vR + 9 * k), yaw, sr, stv);
  A.st_out[PGS_YAW_DRIFT] = yaw;
  pgs_put(A.st_out + PGS_R_DRIFT, sr); pgs_put(A.st_out + PGS_T_DRIFT, stv);
}

// ---- one turn of optimize4DoF: the keyframes first .. first + n - 1 and their loop measurements from the list into the packed
//      input of graph 0 (vio_T | vio_R | t and yaw of every loop edge; no tail: k_pgs_scatter corrects the later keyframes in place)
struct PgsTurnArgs {
  PgsList L;
  PgArgs pg;             // the one graph of the rounds; pg.in and pg.out are written here
  const double* st_in;
  double* st_out;
  int first, size;       // the first keyframe of the range, the keyframes in the list
};
__global__ __launch_bounds__(PGS_THREADS) void k_pgs_gather(PgsTurnArgs A) {
  const PgGraph& G = A.pg.gr[0];
  const PgLayout& p = G.p;
  double* in = const_cast<double*>(A.pg.in) + G.in;
  const int t = blockIdx.x * PGS_THREADS + threadIdx.x, n = p.n;
  const PgsList& L = A.L;
  if (t < n) {
    const size_t k = (size_t)(A.first + t);
    for (int i = 0; i < 3; ++i) in[3 * (size_t)t + i] = L.vT[3 * k + i];
    for (int i = 0; i < 9; ++i) in[3 * (size_t)n + 9 * (size_t)t + i] = L.vR[9 * k + i];
  }
  if (t < p.L) {
    const size_t k = (size_t)(A.first + (A.pg.ints + G.iw)[p.loop_ab + 2 * t + 1]);
    double* l4 = in + 12 * (size_t)n + 4 * (size_t)t;
    l4[0] = L.li[8 * k]; l4[1] = L.li[8 * k + 1]; l4[2] = L.li[8 * k + 2]; l4[3] = L.li[8 * k + 7];
  }
}

// ---- behind k_pg_finish: the poses of the range back into the list (:533-547), the drift into the state (:549-557), and every later
//      keyframe corrected in place (:562-571)
__global__ __launch_bounds__(PGS_THREADS) void k_pgs_scatter(PgsTurnArgs A) {
  const PgGraph& G = A.pg.gr[0];
  const int n = G.p.n, t = blockIdx.x * PGS_THREADS + threadIdx.x;
  const double* out = A.pg.out + G.out;
  const PgsList& L = A.L;
  const size_t k = (size_t)A.first + (size_t)t;
  if (t < n) {
    for (int i = 0; i < 3; ++i) L.T[3 * k + i] = out[PG_HEAD + 3 * (size_t)t + i];
    for (int i = 0; i < 9; ++i) L.R[9 * k + i] = out[PG_HEAD + 3 * (size_t)n + 9 * (size_t)t + i];
  } else if (k < (size_t)A.size) {
    const M3 rd = pgs_m3(out + 8);
    const V3 td = pgs_v3(out + 17);
    pgs_put(L.T + 3 * k, mul(rd, pgs_v3(L.vT + 3 * k)) + td);
    pgs_put(L.R + 9 * k, mul(rd, pgs_m3(L.vR + 9 * k)));
  }
  if (t != 0) return;
  for (int i = 0; i < PGS_STATE; ++i) A.st_out[i] = A.st_in[i];
  A.st_out[PGS_YAW_DRIFT] = out[7];
  for (int i = 0; i < 9; ++i) A.st_out[PGS_R_DRIFT + i] = out[8 + i];
  for (int i = 0; i < 3; ++i) A.st_out[PGS_T_DRIFT + i] = out[17 + i];
}

}  // namespace vpl
