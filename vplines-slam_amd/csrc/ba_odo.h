// Device side of a keyframe session (include/vplines_ba.h, vpl_odo_*): the feature manager's observations, inverse depths,
// Pluecker lines and triangulation flags, the 11 states, the extrinsic and the 11 pre-integrations of n_seq sequences stay in
// HBM from keyframe to keyframe (OdoStore); these kernels move them between the store and the batch (DevBatch) the existing
// stages work on.  All of them are small and memory bound: one work-group column per sequence, plain loads and stores.
//
// Store layout: a track owns a fixed slot of 11 observation records (a track never holds more than the window's 11 frames), so
// the track's index in the host's book (odo_tracks.h) is its address and no observation offsets have to be kept or compacted:
//   pobs [seq][maxPT][11][3]   lobs [seq][maxLT][11][8] (64-byte records)   invd [seq][maxPT]   plk [seq][maxLT][6]   tri [seq][maxLT]
// Records are read and written whole by consecutive lanes of consecutive doubles (the loops below run over doubles, not over
// records), so a wave touches contiguous 512-byte runs whatever the record size.
// The slide reads one store and writes the other (the host swaps them): a stable compaction in place would have track j's
// writer race track j's reader.
#pragma once
#include "ba_types.h"
#include "ba_lineopt.h"
#include "ba_factors.h"
#include "vplines_ba.h"

namespace vpl {

constexpr int ODO_THREADS = 256;
constexpr int ODO_PRE_D = sizeof(DevPreint) / 8;            // a DevPreint is all doubles
constexpr int ODO_RAW_PRE_D = sizeof(vpl_preintegration) / 8;

struct OdoStore {
  double *pobs, *lobs, *invd, *plk;
  int* tri;
  double *pose, *sb, *ex;   // [seq][77] [seq][99] [seq][7]
  DevPreint* pre;           // [seq][11]
  int maxPT, maxLT;
};

// The prior a session keeps between keyframes (the marginalisation's output, device to device)
// The IMU side of a session that takes raw samples (vpl_odo_enable_imu), per sequence: the samples of the interval that ends in
// slot 10 (dt_buf / linear_acceleration_buf / angular_velocity_buf [WINDOW_SIZE]), their count, and linearized_acc / _gyr of
// pre_integrations[10].  The last measurement seen (the estimator's acc_0 / gyr_0) is the last row of smp.  Two of them, swapped
// with the stores.
struct OdoImu {
  double *smp, *lin;        // [seq][max][7] dt, acc, gyr   [seq][6]
  int* n;                   // [seq]
  int max;
};

struct OdoPrior {
  double *J0, *r0, *x0;     // [seq][MAXKEEP^2] compact n x n, [seq][MAXKEEP], [seq][MAXPB * 9]
};

// ---- store -> batch: exactly what pack_window + the upload's copy put there for the equivalent vpl_window ---------------
// psrc [W][maxP], lsrc [W][maxL]: selected track (device line) -> store track.  The integer tables (nP, nL, pt_*, ln_*, lo_ln,
// nLO) have been uploaded by the host before this runs.
__global__ __launch_bounds__(ODO_THREADS) void k_odo_gather(DevBatch B, OdoStore S, const int* __restrict__ psrc,
                                                            const int* __restrict__ lsrc) {
  const int w = blockIdx.x, tid = threadIdx.x;
  const int nP = B.nP[w], nL = B.nL[w];
  for (int i = tid; i < 77; i += ODO_THREADS) { const double v = S.pose[w * 77 + i]; B.pose[w * 77 + i] = v; B.pose_0[w * 77 + i] = v; }
  for (int i = tid; i < 99; i += ODO_THREADS) { const double v = S.sb[w * 99 + i]; B.sb[w * 99 + i] = v; B.sb_0[w * 99 + i] = v; }
  for (int i = tid; i < 7; i += ODO_THREADS) { const double v = S.ex[w * 7 + i]; B.ex[w * 7 + i] = v; B.ex_0[w * 7 + i] = v; }
  for (int i = tid; i < 13; i += ODO_THREADS) B.fail_ref[w * 13 + i] = 0.0;
  for (int i = tid; i < B.maxL * 4; i += ODO_THREADS) B.orth[(size_t)w * B.maxL * 4 + i] = 0.0;
  {
    const double* src = reinterpret_cast<const double*>(S.pre + (size_t)w * NF);
    double* dst = reinterpret_cast<double*>(B.pre + (size_t)w * NF);
    for (int i = tid; i < NF * ODO_PRE_D; i += ODO_THREADS) dst[i] = src[i];
  }
  for (int p = tid; p < B.maxP; p += ODO_THREADS) {
    const size_t pi = (size_t)w * B.maxP + p;
    const double v = p < nP ? S.invd[(size_t)w * S.maxPT + psrc[pi]] : 1.0;
    B.invd[pi] = v; B.invd_0[pi] = v;
  }
  for (int i = tid; i < B.maxL * 6; i += ODO_THREADS) {
    const int l = i / 6;
    const size_t li = (size_t)w * B.maxL + l;
    const double v = l < nL ? S.plk[((size_t)w * S.maxLT + lsrc[li]) * 6 + i % 6] : 0.0;
    B.plk[li * 6 + i % 6] = v; B.plk_0[li * 6 + i % 6] = v;
  }
  // point observations: track p's nobs records go to pt_off[p]; the rest of the array is zero, as the upload leaves it
  int nPO = 0;
  if (nP > 0) nPO = B.pt_off[(size_t)w * B.maxP + nP - 1] + B.pt_nobs[(size_t)w * B.maxP + nP - 1];
  double* po = B.pt_obs + (size_t)w * B.maxPO * 3;
  for (int i = tid; i < nP * NF * 3; i += ODO_THREADS) {
    const int p = i / (NF * 3), r = i % (NF * 3);
    const size_t pi = (size_t)w * B.maxP + p;
    if (r < B.pt_nobs[pi] * 3) po[(size_t)B.pt_off[pi] * 3 + r] = S.pobs[((size_t)w * S.maxPT + psrc[pi]) * NF * 3 + r];
  }
  for (int i = nPO * 3 + tid; i < B.maxPO * 3; i += ODO_THREADS) po[i] = 0.0;
  // line observations: lo_ln names the line of every observation
  const int nLO = B.nLO[w];
  double* lo = B.ln_obs + (size_t)w * B.maxLO * 8;
  for (int i = tid; i < B.maxLO * 8; i += ODO_THREADS) {
    const int o = i >> 3;
    double v = 0.0;
    if (o < nLO) {
      const size_t li = (size_t)w * B.maxL + B.lo_ln[(size_t)w * B.maxLO + o];
      v = S.lobs[(((size_t)w * S.maxLT + lsrc[li]) * NF + (o - B.ln_off[li])) * 8 + (i & 7)];
    }
    lo[i] = v;
  }
}

// the session's prior into the batch's input prior (the block table went through the host); has[w] = 0: no prior yet
__global__ __launch_bounds__(ODO_THREADS) void k_odo_prior_load(DevBatch B, OdoPrior P, const int* __restrict__ has) {
  const int w = blockIdx.x;
  if (!has[w]) return;
  const int n = B.pr_n[w];
  double* Jo = B.pr_J0 + (size_t)w * B.prS;
  const double* J = P.J0 + (size_t)w * MAXKEEP * MAXKEEP;
  for (int i = threadIdx.x; i < n * n; i += ODO_THREADS) Jo[i] = J[i];
  for (int i = threadIdx.x; i < n; i += ODO_THREADS) B.pr_r0[(size_t)w * MAXPN + i] = P.r0[(size_t)w * MAXKEEP + i];
  for (int i = threadIdx.x; i < MAXPB * 9; i += ODO_THREADS) B.pr_x0[(size_t)w * MAXPB * 9 + i] = P.x0[(size_t)w * MAXPB * 9 + i];
}

// ---- batch -> store, after each stage; the integer decisions the host's book needs go to `flags` (read back) ------------
// after the two triangulations (all selected lines in the batch): every selected point's inverse depth; a line that was not
// triangulated and now is takes its Pluecker vector.  flags: the windows' lines one after the other, is_triangulation afterwards.
__device__ inline int odo_prefix(const int* __restrict__ a, int w) {   // (a few dozen sequences at most)
  int s = 0;
  for (int v = 0; v < w; ++v) s += a[v];
  return s;
}
__global__ __launch_bounds__(ODO_THREADS) void k_odo_scatter_tri(DevBatch B, OdoStore S, const int* __restrict__ psrc,
                                                                 const int* __restrict__ lsrc, int* __restrict__ flags) {
  const int w = blockIdx.x;
  const int nP = B.nP[w], nL = B.nL[w];
  const int foff = odo_prefix(B.nL, w);
  for (int p = threadIdx.x; p < nP; p += ODO_THREADS) {
    const size_t pi = (size_t)w * B.maxP + p;
    S.invd[(size_t)w * S.maxPT + psrc[pi]] = B.invd[pi];
  }
  for (int l = threadIdx.x; l < nL; l += ODO_THREADS) {
    const size_t li = (size_t)w * B.maxL + l, t = (size_t)w * S.maxLT + lsrc[li];
    int tri = S.tri[t];
    if (!tri && B.ln_tri[li]) {
      for (int k = 0; k < 6; ++k) S.plk[t * 6 + k] = B.plk[li * 6 + k];
      S.tri[t] = tri = 1;
    }
    flags[foff + l] = tri;
  }
}

__device__ inline void odo_report(vpl_solve_report& r, const TrState& t) {   // fill_report of the host side
  r.iterations = t.iter;
  r.num_successful_steps = t.num_successful;
  r.termination = t.status == 1 ? 1 : t.status == 2 ? 2 : 0;
  r.initial_cost = t.initial_cost;
  r.final_cost = t.x_cost;
  r.n_lines_removed = 0;   // (counted by the host from the flags)
  r.prior_m = 0;
  r.prior_n = 0;
}

// after onlyLineOpt (the triangulated lines in the batch): windows with fewer than four lines are left untouched; otherwise a
// line removeLineOutlier erased loses its triangulation flag and keeps its vector, the others take the optimised one.
// flags: the windows' lines one after the other, 1 = erased.  res[w].line_report: onlyLineOpt's.
__global__ __launch_bounds__(ODO_THREADS) void k_odo_scatter_lopt(DevBatch B, OdoStore S, const int* __restrict__ lsrc,
                                                                  int* __restrict__ flags, vpl_odo_result* __restrict__ res) {
  const int w = blockIdx.x;
  const int nL = B.nL[w];
  const int foff = odo_prefix(B.nL, w);
  if (threadIdx.x == 0) {
    vpl_solve_report r;
    TrState zero = {};
    odo_report(r, nL < 4 ? zero : B.tr[w]);
    res[w].line_report = r;
  }
  for (int l = threadIdx.x; l < nL; l += ODO_THREADS) {
    const size_t li = (size_t)w * B.maxL + l, t = (size_t)w * S.maxLT + lsrc[li];
    const int rem = nL < 4 ? 0 : B.ln_removed[li];
    flags[foff + l] = rem;
    if (nL < 4) continue;
    if (rem) S.tri[t] = 0;
    else
      for (int k = 0; k < 6; ++k) S.plk[t * 6 + k] = B.plk[li * 6 + k];
  }
}

// after the solve: states, inverse depths, the Pluecker vectors of the lines the solve did not erase; res[w]: states and
// report.  marg[w] = 1 + the host's count of kept blocks: the marginalisation wrote a new prior for this window (0: it did
// not) -- it is copied into the session's buffer.  flags, three parts, each the windows one after the other:
//   nP ints: inverse depth > 0 (removeFailures keeps the track)
//   per window with a new prior 2 + 3 * (marg[w] - 1) ints: n, n_blocks, kind[], frame[], idx[] (packed by n_blocks)
//   nL ints: erased by the solve's removeLineOutlier (the host reads them only when that is switched on)
__device__ inline int odo_ptab_len(int m) { return m ? 2 + 3 * (m - 1) : 0; }
__global__ __launch_bounds__(ODO_THREADS) void k_odo_scatter_solve(DevBatch B, OdoStore S, const int* __restrict__ psrc,
                                                                   const int* __restrict__ lsrc, int* __restrict__ flags,
                                                                   vpl_odo_result* __restrict__ res, OdoPrior P,
                                                                   const int* __restrict__ marg) {
  const int w = blockIdx.x, tid = threadIdx.x;
  const int nP = B.nP[w], nL = B.nL[w];
  int offP = 0, totP = 0, offT = 0, totT = 0, offL = 0;
  for (int v = 0; v < B.nW; ++v) {
    const int p = B.nP[v], t = odo_ptab_len(marg[v]);
    if (v < w) { offP += p; offT += t; offL += B.nL[v]; }
    totP += p; totT += t;
  }
  double* rp = &res[w].pose[0][0];
  double* rs = &res[w].speed_bias[0][0];
  for (int i = tid; i < 77; i += ODO_THREADS) { const double v = B.pose[w * 77 + i]; S.pose[w * 77 + i] = v; rp[i] = v; }
  for (int i = tid; i < 99; i += ODO_THREADS) { const double v = B.sb[w * 99 + i]; S.sb[w * 99 + i] = v; rs[i] = v; }
  for (int i = tid; i < 7; i += ODO_THREADS) { const double v = B.ex[w * 7 + i]; S.ex[w * 7 + i] = v; res[w].ex_pose[i] = v; }
  for (int p = tid; p < nP; p += ODO_THREADS) {
    const size_t pi = (size_t)w * B.maxP + p;
    const double v = B.invd[pi];
    S.invd[(size_t)w * S.maxPT + psrc[pi]] = v;
    flags[offP + p] = v > 0 ? 1 : 0;
  }
  for (int l = tid; l < nL; l += ODO_THREADS) {
    const size_t li = (size_t)w * B.maxL + l, t = (size_t)w * S.maxLT + lsrc[li];
    const int rem = B.ln_removed[li];
    flags[totP + totT + offL + l] = rem;
    if (!rem)
      for (int k = 0; k < 6; ++k) S.plk[t * 6 + k] = B.plk[li * 6 + k];
  }
  const int n = marg[w] ? B.mg_n[w] : 0, nb = marg[w] ? min(B.mg_nb[w], marg[w] - 1) : 0;
  if (tid == 0) {
    vpl_solve_report r;
    odo_report(r, B.tr[w]);
    r.prior_m = B.mg_m[w];
    r.prior_n = n;
    res[w].report = r;
  }
  if (!marg[w]) return;
  int* pt = flags + totP + offT;
  if (tid == 0) { pt[0] = n; pt[1] = nb; }
  for (int b = tid; b < nb && b < MAXPB; b += ODO_THREADS) {
    pt[2 + b] = B.mg_kind[w * MAXPB + b];
    pt[2 + nb + b] = B.mg_frame[w * MAXPB + b];
    pt[2 + 2 * nb + b] = B.mg_idx[w * MAXPB + b];
  }
  const double* J = B.mg_J0 + (size_t)w * MAXKEEP * MAXKEEP;
  double* Jo = P.J0 + (size_t)w * MAXKEEP * MAXKEEP;
  for (int i = tid; i < n * n; i += ODO_THREADS) Jo[i] = J[i];
  for (int i = tid; i < n; i += ODO_THREADS) P.r0[(size_t)w * MAXKEEP + i] = B.mg_r0[(size_t)w * MAXKEEP + i];
  for (int i = tid; i < MAXPB * 9; i += ODO_THREADS) P.x0[(size_t)w * MAXPB * 9 + i] = B.mg_x0[(size_t)w * MAXPB * 9 + i];
}

// ---- Estimator::slideWindow on the store: from store A into store B ---------------------------------------------------
// pmv [seq][maxPT], lmv [seq][maxLT]: new track j = odo_pack_move(store track, dropped observation, re-anchor) (odo_tracks.h);
// cnt [seq][2] = tracks after the slide.  The re-anchoring is k_slide_shift's (slide_frames / slide_point_invd / slide_line_plk)
// on frame 0, frame 1 and the extrinsic as the solve left them.  States: MARGIN_OLD frames 1..10 -> 0..9 (10 keeps its state)
// and pre-integrations 2..10 -> 1..9; MARGIN_SECOND_NEW frame 10 -> 9.  grid (n_seq, ODO_SLIDE_Y).
constexpr int ODO_SLIDE_Y = 4;
__global__ __launch_bounds__(ODO_THREADS) void k_odo_slide(OdoStore A, OdoStore D, const int* __restrict__ pmv, const int* __restrict__ lmv,
                                                           const int* __restrict__ cnt, int second_new, double init_depth) {
  const int w = blockIdx.x;
  const int tid = blockIdx.y * ODO_THREADS + threadIdx.x, nthr = ODO_SLIDE_Y * ODO_THREADS;
  const int nP = cnt[2 * w], nL = cnt[2 * w + 1];
  double f[21];
  for (int i = 0; i < 14; ++i) f[i] = A.pose[w * 77 + i];
  for (int i = 0; i < 7; ++i) f[14 + i] = A.ex[w * 7 + i];
  // (the frames are only needed by lanes that re-anchor a track; they are cheap next to the copies)
  const SlideFrames F = slide_frames(f);
  for (int j = tid; j < nP; j += nthr) {
    const int m = pmv[(size_t)w * A.maxPT + j];
    const size_t s = (size_t)w * A.maxPT + (m & 0xFFFFF), d = (size_t)w * D.maxPT + j;
    const double* o = A.pobs + s * NF * 3;
    double v = A.invd[s];
    if (m >> 24 & 1) v = slide_point_invd(F, o[0], o[1], o[2], v, init_depth);
    D.invd[d] = v;
  }
  for (int j = tid; j < nL; j += nthr) {
    const int m = lmv[(size_t)w * A.maxLT + j];
    const size_t s = (size_t)w * A.maxLT + (m & 0xFFFFF), d = (size_t)w * D.maxLT + j;
    Plk L{V3{A.plk[s * 6], A.plk[s * 6 + 1], A.plk[s * 6 + 2]}, V3{A.plk[s * 6 + 3], A.plk[s * 6 + 4], A.plk[s * 6 + 5]}};
    if (m >> 24 & 1) L = slide_line_plk(F, L);
    D.plk[d * 6] = L.n.x; D.plk[d * 6 + 1] = L.n.y; D.plk[d * 6 + 2] = L.n.z;
    D.plk[d * 6 + 3] = L.v.x; D.plk[d * 6 + 4] = L.v.y; D.plk[d * 6 + 5] = L.v.z;
    D.tri[d] = A.tri[s];
  }
  // observation records: consecutive lanes take consecutive doubles of a track's slot
  for (int i = tid; i < nP * NF * 3; i += nthr) {
    const int j = i / (NF * 3), r = i % (NF * 3), k = r / 3;
    const int m = pmv[(size_t)w * A.maxPT + j];
    const int drop = (m >> 20 & 15) - 1;
    const int ks = (drop >= 0 && k >= drop) ? k + 1 : k;
    D.pobs[((size_t)w * D.maxPT + j) * NF * 3 + r] = ks < NF ? A.pobs[(((size_t)w * A.maxPT + (m & 0xFFFFF)) * NF + ks) * 3 + r % 3] : 0.0;
  }
  for (int i = tid; i < nL * NF * 8; i += nthr) {
    const int j = i / (NF * 8), r = i % (NF * 8), k = r >> 3;
    const int m = lmv[(size_t)w * A.maxLT + j];
    const int drop = (m >> 20 & 15) - 1;
    const int ks = (drop >= 0 && k >= drop) ? k + 1 : k;
    D.lobs[((size_t)w * D.maxLT + j) * NF * 8 + r] = ks < NF ? A.lobs[(((size_t)w * A.maxLT + (m & 0xFFFFF)) * NF + ks) * 8 + (r & 7)] : 0.0;
  }
  for (int i = tid; i < NF * 7; i += nthr) {
    const int fr = i / 7;
    const int src = second_new ? (fr == NF - 2 ? NF - 1 : fr) : (fr < NF - 1 ? fr + 1 : fr);
    D.pose[w * 77 + i] = A.pose[w * 77 + src * 7 + i % 7];
  }
  for (int i = tid; i < NF * 9; i += nthr) {
    const int fr = i / 9;
    const int src = second_new ? (fr == NF - 2 ? NF - 1 : fr) : (fr < NF - 1 ? fr + 1 : fr);
    D.sb[w * 99 + i] = A.sb[w * 99 + src * 9 + i % 9];
  }
  for (int i = tid; i < 7; i += nthr) D.ex[w * 7 + i] = A.ex[w * 7 + i];
  const double* ps = reinterpret_cast<const double*>(A.pre + (size_t)w * NF);
  double* pd = reinterpret_cast<double*>(D.pre + (size_t)w * NF);
  for (int i = tid; i < NF * ODO_PRE_D; i += nthr) {
    const int fr = i / ODO_PRE_D;
    const int src = (!second_new && fr >= 1 && fr < NF - 1) ? fr + 1 : fr;
    pd[i] = ps[(size_t)src * ODO_PRE_D + i % ODO_PRE_D];
  }
}

// ---- the new frame into slot 10 ------------------------------------------------------------------------------------------
// hdr [seq][6] = payload offset (doubles), n_points, n_lines, offset of the point entries in tab, of the line entries, n_samples.
// Payload of a sequence, n_samples < 0 (vpl_odo_advance): pose[7], speed_bias[9], the vpl_preintegration as the caller holds it,
// point observations [n][3], line observations [n][8]; n_samples >= 0 (vpl_odo_advance_imu): samples [n_samples][7], then the
// observations -- state and pre-integration of slot 10 are k_odo_imu's.
// tab entry of an observation: track | k << 20 | isnew << 24 (odo_add_frame), -1 = ignored.
// One lane per observation; a track that starts here gets inv_depth = -1, plk = 0, tri = 0.
constexpr int ODO_HDR = 6;
__global__ __launch_bounds__(ODO_THREADS) void k_odo_append(OdoStore S, const double* __restrict__ payload, const int* __restrict__ hdr,
                                                            const int* __restrict__ tab) {
  const int w = blockIdx.x, tid = threadIdx.x;
  const int* h = hdr + ODO_HDR * w;
  const double* in = payload + h[0];
  const int nP = h[1], nL = h[2];
  if (h[5] < 0) {
    for (int i = tid; i < 7; i += ODO_THREADS) S.pose[w * 77 + (NF - 1) * 7 + i] = in[i];
    for (int i = tid; i < 9; i += ODO_THREADS) S.sb[w * 99 + (NF - 1) * 9 + i] = in[7 + i];
    // to_dev_preint of the host side: the first 17 doubles as they are, five 3 x 3 blocks of the Jacobian, the covariance
    const double* r = in + 16;
    double* d = reinterpret_cast<double*>(S.pre + (size_t)w * NF + (NF - 1));
    const double* jac = r + 17;
    const double* cov = r + 17 + 225;
    for (int i = tid; i < ODO_PRE_D; i += ODO_THREADS) {
      double v = 0.0;                                   // sqrt_info (k_prep writes it)
      if (i < 17) v = r[i];
      else if (i < 17 + 45) {
        const int b = (i - 17) / 9, e = (i - 17) % 9;   // dp_dba, dp_dbg, dq_dbg, dv_dba, dv_dbg
        const int r0 = b < 2 ? 0 : b == 2 ? 3 : 6, c0 = (b == 0 || b == 3) ? 9 : 12;
        v = jac[(r0 + e / 3) * 15 + c0 + e % 3];
      } else if (i < 17 + 45 + 225) v = cov[i - 62];
      d[i] = v;
    }
  }
  const double* pin = in + (h[5] < 0 ? 16 + ODO_RAW_PRE_D : 7 * h[5]);
  for (int i = tid; i < nP; i += ODO_THREADS) {
    const int e = tab[h[3] + i];
    if (e < 0) continue;
    const size_t t = (size_t)w * S.maxPT + (e & 0xFFFFF);
    double* o = S.pobs + (t * NF + (e >> 20 & 15)) * 3;
    o[0] = pin[3 * i]; o[1] = pin[3 * i + 1]; o[2] = pin[3 * i + 2];
    if (e >> 24 & 1) S.invd[t] = -1.0;
  }
  const double* lin = pin + (size_t)nP * 3;
  for (int i = tid; i < nL * 8; i += ODO_THREADS) {
    const int e = tab[h[4] + (i >> 3)];
    if (e < 0) continue;
    const size_t t = (size_t)w * S.maxLT + (e & 0xFFFFF);
    S.lobs[(t * NF + (e >> 20 & 15)) * 8 + (i & 7)] = lin[i];
    if ((e >> 24 & 1) && (i & 7) < 6) S.plk[t * 6 + (i & 7)] = 0.0;
    if ((e >> 24 & 1) && (i & 7) == 6) S.tri[t] = 0;
  }
}

// ---- vpl_odo_init: the alignment's results enter the store, device to device.  For a sequence the alignment accepted: the
// states, the true extrinsic and pre_integrations[1..10] -- k_preintegrate's output (pre3w [seq][10], the 15 x 15 jacobian in the
// sqrt_info slot) in the store's form, as to_dev_preint makes it -- and every point the triangulation selected scaled:
// estimated_depth *= s (estimator.cpp:564-570), a clamped init_depth included.  sum_dt [seq][11] goes back to the host's book.
// A sequence that failed is left as the triangulation left it; the host drops its window.
__global__ __launch_bounds__(ODO_THREADS) void k_odo_init_finish(DevBatch B, OdoStore S, const int* __restrict__ psrc,
                                                                 const vpl_init_result* __restrict__ res, const DevPreint* __restrict__ pre3w,
                                                                 const double* __restrict__ ex, double* __restrict__ sum_dt) {
  const int w = blockIdx.x, tid = threadIdx.x;
  const vpl_init_result& r = res[w];
  if (!r.ok) return;
  const double* rp = &r.pose[0][0];
  const double* rs = &r.speed_bias[0][0];
  for (int i = tid; i < 77; i += ODO_THREADS) S.pose[w * 77 + i] = rp[i];
  for (int i = tid; i < 99; i += ODO_THREADS) S.sb[w * 99 + i] = rs[i];
  for (int i = tid; i < 7; i += ODO_THREADS) S.ex[w * 7 + i] = ex[w * 7 + i];
  for (int i = tid; i < NF * ODO_PRE_D; i += ODO_THREADS) {
    const int f = i / ODO_PRE_D, k = i % ODO_PRE_D;
    double v = 0.0;                                     // entry 0, and sqrt_info (k_prep writes it)
    if (f > 0) {
      const DevPreint& src = pre3w[(size_t)w * (NF - 1) + f - 1];
      const double* q = reinterpret_cast<const double*>(&src);
      if (k < 17) v = q[k];
      else if (k < 17 + 45) {
        const int b = (k - 17) / 9, e = (k - 17) % 9;   // dp_dba, dp_dbg, dq_dbg, dv_dba, dv_dbg
        const int r0 = b < 2 ? 0 : b == 2 ? 3 : 6, c0 = (b == 0 || b == 3) ? 9 : 12;
        v = src.sqrt_info[(r0 + e / 3) * 15 + c0 + e % 3];
      } else if (k < 17 + 45 + 225) v = src.cov[k - 62];
      if (k == 0) sum_dt[w * NF + f] = v;
    } else if (k == 0) sum_dt[w * NF] = 0.0;
    reinterpret_cast<double*>(S.pre + (size_t)w * NF)[i] = v;
  }
  const double s = r.s;
  for (int p = tid; p < B.nP[w]; p += ODO_THREADS) {
    const size_t t = (size_t)w * S.maxPT + psrc[(size_t)w * B.maxP + p];
    S.invd[t] = 1.0 / ((1.0 / S.invd[t]) * s);
  }
}

// ---- the IMU side of the new frame (vpl_odo_advance_imu), after k_odo_slide: one wave per sequence, 16 lanes per integration
// as in k_preintegrate, whose step body it shares (preint_steps).  A / IA: the store and IMU side before the slide (read);
// D / ID: after it (D as k_odo_slide left it).
//   group 0, VPL_MARGIN_SECOND_NEW only: D.pre[9] CONTINUED over the samples slot 10 held -- push_back sample by sample on slot 9's
//     deltas, covariance and bias columns of the jacobian under slot 9's linearisation bias, the first mid-point from IA.lin (the
//     last sample of interval 9): estimator.cpp:1786-1799.  Columns 9..14 of J are all IMUFactor reads and all DevPreint holds;
//     J <- F J acts column by column, rows 9..14 of those columns are the identity and the dq_dba block is zero, so continuing
//     them alone is exact (the lanes of columns 0..8 carry values nobody stores).
//   group 1: D.pre[10] from the identity over the new samples, linearised at D.sb[10][3..8] -- the bias the solve has just
//     estimated, which both slides leave in slot 10 (estimator.cpp:1766, :1810); sqrt_info = 0 (k_prep writes it).
//   group 2, one lane: processIMU's propagation (estimator.cpp:107-113) of D.pose[10], D.sb[10][0..2] over the new samples, the
//     rotation carried as a matrix like Rs[j] and converted once, as vector2double does.
// The new samples become ID's buffer; out [seq][18] = the propagated pose[7], speed_bias[9], sum_dt of slots 9 and 10.
constexpr int ODO_IMU_OUT_D = 18;
// mat2q (Eigen's Quaternion(Matrix3), what vector2double applies to Rs) with the three cases of its second branch written out:
// the same arithmetic, and no run-time index into the matrix, which would put it on the stack
__device__ __forceinline__ Q4 odo_mat2q(const M3& m) {
  const double* a = m.m;
  double t = a[0] + a[4] + a[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    const double h = 0.5 / t;
    return Q4{0.5 * t, (a[7] - a[5]) * h, (a[2] - a[6]) * h, (a[3] - a[1]) * h};
  }
  const int i = a[8] > (a[4] > a[0] ? a[4] : a[0]) ? 2 : (a[4] > a[0] ? 1 : 0);
  if (i == 0) {
    t = sqrt(a[0] - a[4] - a[8] + 1.0);
    const double h = 0.5 / t;
    return Q4{(a[7] - a[5]) * h, 0.5 * t, (a[3] + a[1]) * h, (a[6] + a[2]) * h};
  }
  if (i == 1) {
    t = sqrt(a[4] - a[8] - a[0] + 1.0);
    const double h = 0.5 / t;
    return Q4{(a[2] - a[6]) * h, (a[1] + a[3]) * h, 0.5 * t, (a[7] + a[5]) * h};
  }
  t = sqrt(a[8] - a[0] - a[4] + 1.0);
  const double h = 0.5 / t;
  return Q4{(a[3] - a[1]) * h, (a[2] + a[6]) * h, (a[5] + a[7]) * h, 0.5 * t};
}
__device__ __forceinline__ void odo_store_preint(DevPreint& o, const PreintLane& s, int j, V3 ba, V3 bg, bool zero_sqrt_info) {
  if (j >= 15) return;
  if (j == 0) {
    o.sum_dt = s.sum_dt;
    o.dp[0] = s.dp.x; o.dp[1] = s.dp.y; o.dp[2] = s.dp.z;
    o.dv[0] = s.dv.x; o.dv[1] = s.dv.y; o.dv[2] = s.dv.z;
    o.dq[0] = s.dq.x; o.dq[1] = s.dq.y; o.dq[2] = s.dq.z; o.dq[3] = s.dq.w;
    o.lba[0] = ba.x; o.lba[1] = ba.y; o.lba[2] = ba.z;
    o.lbg[0] = bg.x; o.lbg[1] = bg.y; o.lbg[2] = bg.z;
  }
#pragma unroll
  for (int r = 0; r < 15; ++r) o.cov[r * 15 + j] = s.Pc[r];
  if (zero_sqrt_info)
    for (int r = 0; r < 15; ++r) o.sqrt_info[r * 15 + j] = 0.0;
  if (j >= 9) {   // column j of J: rows 0..2, 3..5 (bg columns only), 6..8 of the block that holds it
    const bool isbg = j >= 12;
    const int c = j - (isbg ? 12 : 9);
    double* bp = isbg ? o.dp_dbg : o.dp_dba;
    double* bv = isbg ? o.dv_dbg : o.dv_dba;
    bp[c] = s.Jc[0]; bp[3 + c] = s.Jc[1]; bp[6 + c] = s.Jc[2];
    bv[c] = s.Jc[6]; bv[3 + c] = s.Jc[7]; bv[6 + c] = s.Jc[8];
    if (isbg) { o.dq_dbg[c] = s.Jc[3]; o.dq_dbg[3 + c] = s.Jc[4]; o.dq_dbg[6 + c] = s.Jc[5]; }
  }
}
__global__ __launch_bounds__(64) void k_odo_imu(OdoStore D, OdoImu IA, OdoImu ID, const double* __restrict__ payload,
                                                const int* __restrict__ hdr, int second_new, double an2, double gn2, double aw2,
                                                double gw2, double g_norm, double* __restrict__ out) {
  __shared__ double tile[4][15 * PREINT_GROUP];
  const int w = blockIdx.x;
  const int grp = threadIdx.x / PREINT_GROUP, j = threadIdx.x % PREINT_GROUP;
  const int jc = j < 15 ? j : 14;
  const double* nsp = payload + hdr[ODO_HDR * w];                  // the new samples
  const int nn = hdr[ODO_HDR * w + 5];
  const double* osp = IA.smp + (size_t)w * IA.max * 7;             // the samples slot 10 held
  const int no = IA.n[w];
  const V3 la{osp[7 * (no - 1) + 1], osp[7 * (no - 1) + 2], osp[7 * (no - 1) + 3]};   // the last measurement seen
  const V3 lg{osp[7 * (no - 1) + 4], osp[7 * (no - 1) + 5], osp[7 * (no - 1) + 6]};
  DevPreint& p9 = D.pre[(size_t)w * NF + NF - 2];
  const double* sb10 = D.sb + w * 99 + (NF - 1) * 9;
  const V3 nba{sb10[3], sb10[4], sb10[5]}, nbg{sb10[6], sb10[7], sb10[8]};
  PreintLane s;
  preint_identity(s, jc, la, lg);
  V3 ba = nba, bg = nbg;
  const double* sp = nsp;
  int ns = grp == 1 ? nn : 0;
  if (grp == 0 && second_new) {
    sp = osp; ns = no;
    ba = V3{p9.lba[0], p9.lba[1], p9.lba[2]}; bg = V3{p9.lbg[0], p9.lbg[1], p9.lbg[2]};
    s.a0 = V3{IA.lin[w * 6], IA.lin[w * 6 + 1], IA.lin[w * 6 + 2]};
    s.g0 = V3{IA.lin[w * 6 + 3], IA.lin[w * 6 + 4], IA.lin[w * 6 + 5]};
    s.sum_dt = p9.sum_dt;
    s.dp = V3{p9.dp[0], p9.dp[1], p9.dp[2]}; s.dv = V3{p9.dv[0], p9.dv[1], p9.dv[2]};
    s.dq = Q4{p9.dq[3], p9.dq[0], p9.dq[1], p9.dq[2]};
#pragma unroll
    for (int r = 0; r < 15; ++r) s.Pc[r] = p9.cov[r * 15 + jc];
    if (jc >= 9) {
      const bool isbg = jc >= 12;
      const int c = jc - (isbg ? 12 : 9);
      const double* bp = isbg ? p9.dp_dbg : p9.dp_dba;
      const double* bv = isbg ? p9.dv_dbg : p9.dv_dba;
      s.Jc[0] = bp[c]; s.Jc[1] = bp[3 + c]; s.Jc[2] = bp[6 + c];
      s.Jc[3] = isbg ? p9.dq_dbg[c] : 0.0; s.Jc[4] = isbg ? p9.dq_dbg[3 + c] : 0.0; s.Jc[5] = isbg ? p9.dq_dbg[6 + c] : 0.0;
      s.Jc[6] = bv[c]; s.Jc[7] = bv[3 + c]; s.Jc[8] = bv[6 + c];
    }
  }
  int nmax = ns;
  nmax = max(nmax, __shfl_xor(nmax, 16, 64));
  nmax = max(nmax, __shfl_xor(nmax, 32, 64));
  preint_steps(s, j, sp, ns, nmax, ba, bg, an2, gn2, aw2, gw2, tile[grp]);
  double* o = out + (size_t)w * ODO_IMU_OUT_D;
  if (grp == 0) {
    if (second_new) odo_store_preint(p9, s, j, ba, bg, false);
    if (j == 0) o[16] = second_new ? s.sum_dt : p9.sum_dt;
  } else if (grp == 1) {
    odo_store_preint(D.pre[(size_t)w * NF + NF - 1], s, j, ba, bg, true);
    if (j == 0) o[17] = s.sum_dt;
  } else if (grp == 2) {
    if (j == 0) {
      double* pose = D.pose + w * 77 + (NF - 1) * 7;
      double* sb = D.sb + w * 99 + (NF - 1) * 9;
      M3 R = qmat(qnormalized(qpose(pose)));
      V3 P{pose[0], pose[1], pose[2]}, V{sb[0], sb[1], sb[2]}, a0 = la, g0 = lg;
      const V3 g{0.0, 0.0, g_norm};
      for (int k = 0; k < nn; ++k) {
        const double dt = nsp[7 * k];
        const V3 a1{nsp[7 * k + 1], nsp[7 * k + 2], nsp[7 * k + 3]}, g1{nsp[7 * k + 4], nsp[7 * k + 5], nsp[7 * k + 6]};
        const V3 un_acc_0 = mul(R, a0 - nba) - g;
        const V3 un_gyr = 0.5 * (g0 + g1) - nbg;
        R = mul(R, qmat(deltaQ(un_gyr * dt)));
        const V3 un_acc_1 = mul(R, a1 - nba) - g;
        const V3 un_acc = 0.5 * (un_acc_0 + un_acc_1);
        P = P + dt * V + 0.5 * dt * dt * un_acc;
        V = V + dt * un_acc;
        a0 = a1; g0 = g1;
      }
      const Q4 q = odo_mat2q(R);
      pose[0] = P.x; pose[1] = P.y; pose[2] = P.z; pose[3] = q.x; pose[4] = q.y; pose[5] = q.z; pose[6] = q.w;
      sb[0] = V.x; sb[1] = V.y; sb[2] = V.z;
      o[0] = P.x; o[1] = P.y; o[2] = P.z; o[3] = q.x; o[4] = q.y; o[5] = q.z; o[6] = q.w;
      o[7] = V.x; o[8] = V.y; o[9] = V.z;
      o[10] = nba.x; o[11] = nba.y; o[12] = nba.z; o[13] = nbg.x; o[14] = nbg.y; o[15] = nbg.z;
    }
  } else {
    // the new interval becomes slot 10's buffer, the measurement before it its linearized_acc / _gyr
    double* dsp = ID.smp + (size_t)w * ID.max * 7;
    for (int i = j; i < 7 * nn; i += PREINT_GROUP) dsp[i] = nsp[i];
    if (j == 0) ID.n[w] = nn;
    if (j < 3) { ID.lin[w * 6 + j] = get(la, j); ID.lin[w * 6 + 3 + j] = get(lg, j); }
  }
}

// ---- the keyframe decision (vpl_odo_enable_keyframe_rule): FeatureManager::addFeatureCheckParallax's return value for the window
// as it stands with the new image in slot 10 (feature_manager.cpp:166-188), behind k_odo_append.  One work-group per sequence;
// block b works on sequence seq0 + b of the store and on entry b of par and out.
// par [b][3] = offset of the sequence's list in tab, its entries, last_track_num (odo_parallax_list: the host's book knows which
// tracks qualify and where their frame-8 observation lies; the observations themselves are only here).
// Per track compensatedParallax2 (feature_manager.cpp:958-996) as it is written: the frame-8 observation divided by its z, the
// frame-9 observation as stored; the compensated variant is the same expression, so the min of the two is that expression.
// The sum has one shape whatever the session looks like: lane t adds entries t, t + 256, ... in list order (a lane without an
// entry adds nothing), the 64 lanes of a wave are folded by the xor butterfly 32, 16, .. 1, and lane 0 adds the four waves as
// (w0 + w1) + (w2 + w3).  No atomics; the bits depend on the list and the observations alone.
struct OdoParallaxRec {   // VPL_ODO_DECISION_RECORD_BYTES
  int flag, last_track_num, parallax_num, reserved;
  double parallax_sum;
};
static_assert(sizeof(OdoParallaxRec) == VPL_ODO_DECISION_RECORD_BYTES, "the decision record is part of the documented traffic");
constexpr int ODO_PAR_HDR = 3;
static_assert(ODO_THREADS == 4 * 64, "k_odo_parallax combines four waves");
__global__ __launch_bounds__(ODO_THREADS) void k_odo_parallax(OdoStore S, const int* __restrict__ tab, const int* __restrict__ par, int seq0,
                                                              double min_parallax, int min_track_num, OdoParallaxRec* __restrict__ out) {
  __shared__ double wave_sum[ODO_THREADS / 64];
  const int b = blockIdx.x, w = seq0 + b, tid = threadIdx.x;
  const int* list = tab + par[ODO_PAR_HDR * b];
  const int n = par[ODO_PAR_HDR * b + 1];
  const double* po = S.pobs + (size_t)w * S.maxPT * NF * 3;
  double acc = 0.0;
  for (int i = tid; i < n; i += ODO_THREADS) {
    const int e = list[i];
    const double* o = po + ((size_t)(e & 0xFFFFF) * NF + (e >> 20 & 15)) * 3;   // frame 8's record, frame 9's behind it
    const double u_i = o[0] / o[2], v_i = o[1] / o[2];
    const double du = u_i - o[3], dv = v_i - o[4];
    const double d = sqrt(du * du + dv * dv);
    acc += 0.0 < d ? d : 0.0;   // max(ans = 0, .) of std::max: a NaN counts as zero
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((tid & 63) == 0) wave_sum[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    const double sum = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
    const int last = par[ODO_PAR_HDR * b + 2];
    OdoParallaxRec r;
    r.flag = (last < min_track_num || n == 0 || sum / n >= min_parallax) ? VPL_MARGIN_OLD : VPL_MARGIN_SECOND_NEW;
    r.last_track_num = last;
    r.parallax_num = n;
    r.reserved = 0;
    r.parallax_sum = sum;
    out[b] = r;
  }
}

}  // namespace vpl
