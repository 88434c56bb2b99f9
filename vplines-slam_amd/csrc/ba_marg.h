// k_gauge : Estimator::double2vector2 (estimator.cpp:810-900) -- yaw/position gauge fix of the
//           whole window, lines carried through setLineOrth (feature_manager.cpp:367-388), then
//           the vector2double() round trip the reference performs before marginalising (:1233).
// k_marg  : MarginalizationInfo::marginalize (marginalization_factor.cpp:177-363) on the normal
//           equations k_lin<MARG> assembled: landmark elimination, eigen pseudo-inverse of the
//           oldest frame's 15 dims, eigen decomposition of the kept block -> J0, r0.
//           Its LDS layout is ba_marg_layout.h, its factorisations and the write-out of the prior are ba_psd.h.
// k_prior_handoff, k_prior_restride, k_pack_states: the small kernels around them.
#pragma once
#include "ba_common.h"
#include "ba_marg_layout.h"
#include "ba_psd.h"

namespace vpl {

// ---------------------------------------------------------------------------------------------------
// k_gauge
__device__ __forceinline__ void gauge_body(const DevBatch& B, const int w) {
  const int tid = threadIdx.x;
  __shared__ double rd[9], p0a[3], p0b[3], newpose[NF * 7], newex[7];
  const double* gz = B.gauge + (size_t)w * 4;
  double* pose = B.pose + (size_t)w * 77;
  double* sb = B.sb + (size_t)w * 99;
  double* ex = B.ex + (size_t)w * 7;
  if (tid == 0) {
    V3 ypr00 = R2ypr(qmat(qpose(pose)));
    double y_diff = gz[0] - ypr00.x;
    M3 R = ypr2R(V3{y_diff, 0, 0});
    for (int k = 0; k < 9; ++k) rd[k] = R.m[k];
    for (int k = 0; k < 3; ++k) { p0a[k] = pose[k]; p0b[k] = gz[1 + k]; }
  }
  __syncthreads();
  M3 rot_diff;
  for (int k = 0; k < 9; ++k) rot_diff.m[k] = rd[k];
  V3 P0a{p0a[0], p0a[1], p0a[2]}, P0b{p0b[0], p0b[1], p0b[2]};
  if (tid < NF) {
    const double* x = pose + 7 * tid;
    M3 Rs = mul(rot_diff, qmat(qnormalized(qpose(x))));
    V3 Ps = mul(rot_diff, V3{x[0] - P0a.x, x[1] - P0a.y, x[2] - P0a.z}) + P0b;
    Q4 q = mat2q(Rs);   // what the next vector2double() writes
    double* o = newpose + 7 * tid;
    o[0] = Ps.x; o[1] = Ps.y; o[2] = Ps.z; o[3] = q.x; o[4] = q.y; o[5] = q.z; o[6] = q.w;
    double* s = sb + 9 * tid;
    V3 V = mul(rot_diff, V3{s[0], s[1], s[2]});
    s[0] = V.x; s[1] = V.y; s[2] = V.z;
  }
  if (tid == NF) {
    Q4 q = mat2q(qmat(qpose(ex)));   // ric = q.toRotationMatrix(); para = Quaterniond(ric)
    for (int k = 0; k < 3; ++k) newex[k] = ex[k];
    newex[3] = q.x; newex[4] = q.y; newex[5] = q.z; newex[6] = q.w;
  }
  __syncthreads();
  // lines: orth (world, optimised gauge) -> rotate back -> start camera frame -> orth again
  const int nL = B.nL[w];
  V3 tw1b = P0a;
  V3 twow1 = -mul(rot_diff, tw1b) + P0b;
  for (int l = tid; l < nL; l += blockDim.x) {
    const size_t li = (size_t)w * B.maxL + l;
    Plk Lw1 = orth_to_plk(B.orth + li * 4);
    Plk Lwo = plk_to_pose(Lw1, rot_diff, twow1);
    double o4[4];
    plk_to_orth(Lwo, o4);
    Plk Lw = orth_to_plk(o4);
    const int s = B.ln_start[li];
    // Rs[s] as stored by double2vector2 is rot_diff * R(q): rebuild it the same way from the OLD pose
    const double* xo = pose + 7 * s;
    M3 Rs = mul(rot_diff, qmat(qnormalized(qpose(xo))));
    V3 Ps{newpose[7 * s], newpose[7 * s + 1], newpose[7 * s + 2]};
    M3 ric = qmat(qpose(ex));
    V3 tic{ex[0], ex[1], ex[2]};
    V3 twc = Ps + mul(Rs, tic);
    M3 Rwc = mul(Rs, ric);
    Plk Lc = plk_from_pose(Lw, Rwc, twc);
    double* pl = B.plk + li * 6;
    pl[0] = Lc.n.x; pl[1] = Lc.n.y; pl[2] = Lc.n.z; pl[3] = Lc.v.x; pl[4] = Lc.v.y; pl[5] = Lc.v.z;
    // vector2double() before the marginalisation: getLineOrthVector on the updated state
    Plk Lw2 = plk_to_pose(Lc, Rwc, twc);
    plk_to_orth(Lw2, B.orth + li * 4);
    {   // the marginalisation pass of k_lin reads the Pluecker image of these parameters (B.lw)
      const Plk Lq = orth_to_plk(B.orth + li * 4);
      double* o = B.lw + li * 6;
      o[0] = Lq.n.x; o[1] = Lq.n.y; o[2] = Lq.n.z; o[3] = Lq.v.x; o[4] = Lq.v.y; o[5] = Lq.v.z;
    }

    // FeatureManager::removeLineOutlier (feature_manager.cpp:702-798) on the gauge-fixed state
    int erase = 0;
    if (B.opt.remove_line_outliers) {
      const double* ob0 = B.ln_obs + ((size_t)w * B.maxLO + B.ln_off[li]) * 8;
      const V3 p11{ob0[0], ob0[1], 1.0}, p21{ob0[2], ob0[3], 1.0};
      const V3 cr = cross(p11, p21);
      const double lnn = sqrt(cr.x * cr.x + cr.y * cr.y);
      const double lx = cr.x / lnn, ly = cr.y / lnn;
      const V3 p12{p11.x + lx, p11.y + ly, 1.0}, p22{p21.x + lx, p21.y + ly, 1.0};
      const V3 cam{0, 0, 0};
      // pi_from_ppp (line_geometry.cpp:134-139) ; Lc = [skew(nc) vc; -vc^T 0]
      const V3 n1 = cross(cam - p12, p11 - p12), n2 = cross(cam - p22, p21 - p22);
      const double d1 = -dot(p12, cross(cam, p11)), d2 = -dot(p22, cross(cam, p21));
      const V3 e1x = mul(skew(Lc.n), n1) + Lc.v * d1, e2x = mul(skew(Lc.n), n2) + Lc.v * d2;
      const double e1w = -dot(Lc.v, n1), e2w = -dot(Lc.v, n2);
      const V3 e1{e1x.x / e1w, e1x.y / e1w, e1x.z / e1w}, e2{e2x.x / e2w, e2x.y / e2w, e2x.z / e2w};
      if (e1.z < 0 || e2.z < 0) erase = 1;
      else if (norm(e1 - e2) > 10) erase = 1;
      else {
        const Plk line_w = plk_to_pose(Lc, Rwc, twc);
        double allerr = 0;
        const int no = B.ln_nobs[li];
        for (int k = 0; k < no; ++k) {
          const int j = s + k;
          const double* xj = pose + 7 * j;
          const M3 Rj = mul(rot_diff, qmat(qnormalized(qpose(xj))));
          const V3 Pj{newpose[7 * j], newpose[7 * j + 1], newpose[7 * j + 2]};
          const V3 t1 = Pj + mul(Rj, tic);
          const M3 R1 = mul(Rj, ric);
          const Plk lc = plk_from_pose(line_w, R1, t1);   // feature_manager.cpp:390-411
          const double sql = sqrt(lc.n.x * lc.n.x + lc.n.y * lc.n.y);
          const V3 nn{lc.n.x / sql, lc.n.y / sql, lc.n.z / sql};
          const double* ob = ob0 + 8 * k;
          const double err = (fabs(nn.x * ob[0] + nn.y * ob[1] + nn.z) + fabs(nn.x * ob[2] + nn.y * ob[3] + nn.z)) / 2.0;
          if (allerr < err) allerr = err;
        }
        if (allerr > 3.0 / 500.0) erase = 1;
      }
    }
    B.ln_removed[li] = erase;
  }
  __syncthreads();
  for (int i = tid; i < 77; i += blockDim.x) pose[i] = newpose[i];
  for (int i = tid; i < 7; i += blockDim.x) ex[i] = newex[i];
  // erased lines add no factor to the marginalisation: the kept-block table may shrink
  if (tid == 0 && B.opt.remove_line_outliers && B.opt.marginalization_flag == 0) {
    KeepSrc S;
    S.nP = B.nP[w]; S.pt_start = B.pt_start + (size_t)w * B.maxP; S.pt_nobs = B.pt_nobs + (size_t)w * B.maxP;
    S.nL = nL; S.ln_start = B.ln_start + (size_t)w * B.maxL; S.ln_nobs = B.ln_nobs + (size_t)w * B.maxL;
    S.ln_removed = B.ln_removed + (size_t)w * B.maxL;
    S.pr_nb = B.pr_n[w] > 0 ? B.pr_nb[w] : 0; S.pr_kind = B.pr_kind + (size_t)w * MAXPB; S.pr_frame = B.pr_frame + (size_t)w * MAXPB;
    S.imu01 = B.pre[(size_t)w * NF + 1].sum_dt < 10.0;
    keep_tables_old(S, B.mg_kind + (size_t)w * MAXPB, B.mg_frame + (size_t)w * MAXPB, B.mg_idx + (size_t)w * MAXPB,
                    B.mg_cam + (size_t)w * MAXPB, B.mg_n + w, B.mg_nb + w, B.mg_m + w);
  }
}
__global__ __launch_bounds__(128) void k_gauge(DevBatch B) { gauge_body(B, blockIdx.x); }

// ---------------------------------------------------------------------------------------------------
// k_marg.  marg_body carves the dynamic LDS by ba_marg_layout.h (the layout the host sized the dispatch with) and lists its
// phases; each phase is a function of the LDS arrays it uses, the barriers between phases stand in the list.
constexpr int MARG_THREADS = 512;
constexpr double kMargEps = 1e-8;   // marginalization_factor.h:67
#ifndef VPL_MARG_NOISE_REL
#define VPL_MARG_NOISE_REL 0.0
#endif
constexpr double kMargNoiseRel = VPL_MARG_NOISE_REL;   // pivots of the kept block below this fraction of its largest diagonal are noise

// phase 1: the dense map and the frame-0 landmark lists
// dense order: [sb_0 (9), pose_0 (6) | kept blocks in canonical order]  (the reference moves the
// pose-like marginalised blocks behind the landmarks in descending index order, :291-309)
// MARGIN_SECOND_NEW: [pose_9 (6) | kept blocks], no landmarks (estimator.cpp:1387-1405)
template <int T>
__device__ __forceinline__ void marg_dense_map(const DevBatch& B, const int w, const int md, const int nb, const int nL, const bool second_new,
                                               const int LOFF, int* dmap, int* lst, int* s_np0, int* s_nl0) {
  const int tid = threadIdx.x;
  if (tid < md) dmap[tid] = second_new ? 15 * (NF - 2) + tid : (tid < 9 ? 6 + tid : tid - 9);
  if (tid < nb) {
    const int kind = B.mg_kind[(size_t)w * MAXPB + tid];
    const int base = B.mg_cam[(size_t)w * MAXPB + tid], idx = B.mg_idx[(size_t)w * MAXPB + tid];
    const int ls = kind == 1 ? 9 : 6;
    for (int k = 0; k < ls; ++k) dmap[md + idx + k] = base + k;
  }
  // landmarks that start in frame 0: the points are the first bucket of the start-frame sort (k_lin leaves H_pp = 0 on a
  // track without factors: its row is staged as zeros), the lines are compacted in order by wave 0
  if (tid >= 64 && !second_new) {
    const int np0 = min(LOFF, B.ps_cnt[(size_t)w * (NF + 1) + 1]);
    for (int a = tid - 64; a < np0; a += T - 64) lst[a] = B.ps_list[(size_t)w * B.maxP + a];
    if (tid == 64) *s_np0 = np0;
  }
  if (tid < 64) {
    int c = 0;
    if (!second_new)
      for (int l0 = 0; l0 < nL; l0 += 64) {
        const int l = l0 + tid;
        const bool on = l < nL && B.ln_start[(size_t)w * B.maxL + l] == 0 && B.ln_nobs[(size_t)w * B.maxL + l] >= 2 &&
                        !B.ln_removed[(size_t)w * B.maxL + l];
        const unsigned long long m = __ballot(on);
        if (on && c + __popcll(m & ((1ull << tid) - 1ull)) < LOFF) lst[LOFF + c + __popcll(m & ((1ull << tid) - 1ull))] = l;
        c += __popcll(m);
      }
    if (tid == 0) { *s_nl0 = min(c, LOFF); if (second_new) *s_np0 = 0; }
  }
}

// phase 2: Ad, bv gathered from Hcc, gc through dmap; the dense dims with a visual index (vlist, their count in s_flag[2]) and
// the inverse map vinv (visual column -> dense index or -1).  One barrier inside, between the clearing of vinv and its entries.
template <int T>
__device__ __forceinline__ void marg_gather(const DevBatch& B, const int w, const int nd, const int ldd, const int* dmap, double* Ad, double* bv,
                                            int* vlist, int* vinv, int* s_flag) {
  const int tid = threadIdx.x;
  const double* Hcc = B.Hcc + (size_t)w * NCP;
  const double* gc = B.gc + (size_t)w * NC;
  for (int base = 0; base < nd * nd; base += 8 * T) {   // eight global loads in flight per lane, then the LDS stores
    double hv[8];
    int dst[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int it = base + u * T + tid;
      dst[u] = -1;
      hv[u] = 0.0;
      if (it < nd * nd) {
        const int i = it / nd, j = it - i * nd;
        const int ci = dmap[i], cj = dmap[j];
        dst[u] = i * ldd + j;
        hv[u] = ci >= cj ? Hcc[tri(ci, cj)] : Hcc[tri(cj, ci)];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (dst[u] >= 0) Ad[dst[u]] = hv[u];
  }
  VPL_STAMP(B, w, 38);
  for (int i = tid; i < nd; i += T) bv[i] = gc[dmap[i]];
  if (tid < 64) {   // (wave 0: ballots and prefix counts; one thread walking the nd entries cost 17 k cycles)
    const int lane = tid;
    const bool f0 = lane < nd && cam2vis(dmap[lane]) >= 0;
    const bool f1 = lane + 64 < nd && cam2vis(dmap[lane + 64]) >= 0;
    const unsigned long long m0 = __ballot(f0), m1 = __ballot(f1);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (f0) vlist[__popcll(m0 & below)] = lane;
    if (f1) vlist[__popcll(m0) + __popcll(m1 & below)] = lane + 64;
    if (lane == 0) s_flag[2] = __popcll(m0) + __popcll(m1);
  } else if (tid < 64 + MARG_VINV_INTS) {
    vinv[tid - 64] = -1;
  }
  __syncthreads();
  for (int i = tid; i < nd; i += T) {
    const int vi = cam2vis(dmap[i]);
    if (vi >= 0) vinv[vi] = i;
  }
}

// phase 3: one staging pass of cnt point rows, X = C^-1 [W | g] (C C^T = H_ll: a scalar per point).
// Per-row constants first (one lane per landmark: its scale or 4x4 factor, its start frame), then the elements with
// one global load each, four in flight per lane.  Loading them per element put two dependent global latencies into
// every trip of the element loop and repeated the 4x4 Cholesky of a line 73 times.  One barrier inside, behind the constants.
template <int T>
__device__ __forceinline__ void marg_stage_points(const DevBatch& B, const int w, const int cnt, const int* plist, double* rs, int* rstart,
                                                  int* rland, double* tile) {
  const int tid = threadIdx.x;
  if (tid < cnt) {
    const int p = plist[tid];
    const size_t pi = (size_t)w * B.maxP + p;
    const double hpp = B.Hpp[pi];
    rs[tid] = hpp != 0.0 ? 1.0 / sqrt(hpp) : 0.0;
    rstart[tid] = B.pt_start[pi];
    rland[tid] = p;
  }
  __syncthreads();
  for (int it0 = tid; it0 < cnt * 73; it0 += 4 * T) {
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int it = it0 + u * T;
      v[u] = 0.0;
      if (it < cnt * 73) {
        const int rr = it / 73, c = it - rr * 73;
        const size_t pi = (size_t)w * B.maxP + rland[rr];
        const int cc = c < NV ? wcol(c, rstart[rr], B.WS) : 0;
        if (cc >= 0) v[u] = c < NV ? B.Wp[pi * B.WS + cc] : B.gp[pi];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int it = it0 + u * T;
      if (it < cnt * 73) {
        const int rr = it / 73, c = it - rr * 73;
        tile[rr * MARG_ROW + c] = rs[rr] * v[u];
      }
    }
  }
}

// phase 4: one staging pass of cnt lines, four rows each, through the 4 x 4 Cholesky factor of the line's H_ll (one lane per
// line, kept packed in lineC).  One barrier inside, behind the constants.
template <int T>
__device__ __forceinline__ void marg_stage_lines(const DevBatch& B, const int w, const int cnt, const int* llist, double* lineC, int* rstart,
                                                 int* rland, double* tile) {
  const int tid = threadIdx.x;
  if (tid < cnt) {
    const int l = llist[tid];
    const size_t li = (size_t)w * B.maxL + l;
    const double* Hl = B.Hll + li * 16;
    double Cc[10];
    int t = 0;
    for (int a = 0; a < 4; ++a)
      for (int cc = 0; cc <= a; ++cc, ++t) Cc[t] = Hl[4 * a + cc];
    for (int jj = 0; jj < 4; ++jj) {
      double d = Cc[tri(jj, jj)];
      for (int k = 0; k < jj; ++k) d -= Cc[tri(jj, k)] * Cc[tri(jj, k)];
      d = sqrt(d);
      Cc[tri(jj, jj)] = d;
      for (int ii = jj + 1; ii < 4; ++ii) {
        double s2 = Cc[tri(ii, jj)];
        for (int k = 0; k < jj; ++k) s2 -= Cc[tri(ii, k)] * Cc[tri(jj, k)];
        Cc[tri(ii, jj)] = s2 / d;
      }
    }
    for (int q = 0; q < 10; ++q) lineC[10 * tid + q] = Cc[q];
    rstart[tid] = B.ln_start[li];
    rland[tid] = l;
  }
  __syncthreads();
  for (int it = tid; it < cnt * 73; it += T) {
    const int ll = it / 73, c = it - ll * 73;
    const size_t li = (size_t)w * B.maxL + rland[ll];
    const double* Cc = lineC + 10 * ll;
    const int cc = c < NV ? wcol(c, rstart[ll], B.WS) : 0;
    double wv4[4], x[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) wv4[a] = cc < 0 ? 0.0 : (c < NV ? B.Wl[(li * 4 + a) * B.WS + cc] : B.gl[li * 4 + a]);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      double s2 = wv4[a];
#pragma unroll
      for (int k = 0; k < 4; ++k) if (k < a) s2 -= Cc[tri(a, k)] * x[k];
      x[a] = s2 / Cc[tri(a, a)];
      tile[(4 * ll + a) * MARG_ROW + c] = x[a];
    }
  }
}

// phase 5: A -= X^T X, b -= X^T z of the nrows staged rows.
// X^T X of the staged rows on the FP64 matrix cores: 73 columns (72 visual dims + the rhs) = 5 x 5 tiles of 16, the 15
// lower ones over the 8 waves; C[a][b] = sum_r X[r][a] X[r][b] with the A lane (kk, m) supplying X[4 ks + kk][16 ta + m].
// Only the dense dims with a visual index couple to the landmarks: vinv maps a visual column to its dense index.
template <int T>
__device__ __forceinline__ void marg_xtx(const int nrows, const double* tile, const int* vinv, double* Ad, const int ldd, double* bv) {
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6, m = lane & 15, kk = lane >> 4;
  const int ksteps = (nrows + 3) >> 2;
#pragma unroll 1
  for (int tix2 = wv; tix2 < 15; tix2 += T / 64) {
    int ta, tb;
    tri_decode(tix2, ta, tb);
    const int ca = 16 * ta + m, cb = 16 * tb + m;
    typedef double v4dm __attribute__((ext_vector_type(4)));
    v4dm acc = {0, 0, 0, 0};
    for (int ks = 0; ks < ksteps; ++ks) {
      const int r = 4 * ks + kk;
      const double av = (r < nrows && ca < 73) ? tile[r * MARG_ROW + ca] : 0.0;
      const double bw = (r < nrows && cb < 73) ? tile[r * MARG_ROW + cb] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bw, acc, 0, 0, 0);
    }
    const double vals[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int a2 = 16 * ta + kk + 4 * v, b2 = cb;
      if (b2 >= 72 || a2 > 72) continue;
      const int j = vinv[b2];
      if (j < 0) continue;
      if (a2 == 72) { bv[j] -= vals[v]; continue; }
      const int i = vinv[a2];
      if (i < 0) continue;
      Ad[i * ldd + j] -= vals[v];
      if (ta != tb) Ad[j * ldd + i] -= vals[v];   // (inside a diagonal tile the mirror entry has a lane of its own)
    }
  }
}

// phase 6: out(i, :) = Arm(i, :) Amm^-1 for a positive definite Amm, from its pivoted Cholesky factor in E15:  L L^T x = P a,
// one lane per row.  Compile-time loop bounds (md <= 15 guards) keep x in registers and the reads of L broadcast and pipelined;
// reciprocal diagonals from LDS: with run-time bounds x lived in scratch and every step paid an LDS round trip and a division
// (30 k cycles for 45 rows).  One barrier inside, behind rdiag.
template <int T>
__device__ __forceinline__ void marg_elim_cholesky(const int n, const int md, const int ldd, const double* Ad, const double* E15, const int* perm,
                                                   double* rdiag, double* out) {
  const int tid = threadIdx.x;
  if (tid < md) rdiag[tid] = 1.0 / E15[tid * MARG_E15_LD + tid];
  __syncthreads();
  for (int i = tid; i < n; i += T) {
    double x[15];
#pragma unroll
    for (int t = 0; t < 15; ++t) {
      x[t] = 0.0;
      if (t < md) {
        double s2 = Ad[(md + i) * ldd + perm[t]];
#pragma unroll
        for (int k = 0; k < t; ++k) s2 -= E15[t * MARG_E15_LD + k] * x[k];
        x[t] = s2 * rdiag[t];
      }
    }
#pragma unroll
    for (int t = 14; t >= 0; --t) {
      if (t < md) {
        double s2 = x[t];
#pragma unroll
        for (int k = t + 1; k < 15; ++k) if (k < md) s2 -= E15[k * MARG_E15_LD + t] * x[k];
        x[t] = s2 * rdiag[t];
      }
    }
#pragma unroll
    for (int t = 0; t < 15; ++t) if (t < md) out[i * 16 + perm[t]] = x[t];
  }
}

// phase 7: the same through the eigen pseudo-inverse (:334-346), from the spectral factor B of Amm in E15 (Amm = B B^T, b_k
// orthogonal, |b_k|^2 = lam_k):  out(n x md) = Arm * Amm^+ :  first Y = Arm * B (n x md), then out = (Y ./ lambda^2) * B^T.
// One barrier inside, behind Y.
template <int T>
__device__ __forceinline__ void marg_elim_spectral(const int n, const int md, const int ldd, const double* Ad, const double* E15, const int* perm,
                                                   const double* lam, double* Y, double* out) {
  const int tid = threadIdx.x;
  for (int it = tid; it < n * md; it += T) {
    const int i = it / md, k = it % md;
    double s = 0;
    for (int t = 0; t < md; ++t) s += Ad[(md + i) * ldd + perm[t]] * E15[t * MARG_E15_LD + k];
    Y[i * 16 + k] = lam[k] > kMargEps ? s / (lam[k] * lam[k]) : 0.0;
  }
  __syncthreads();
  for (int it = tid; it < n * md; it += T) {
    const int i = it / md, t = it % md;   // column perm[t] of out
    double s = 0;
    for (int k = 0; k < md; ++k) s += Y[i * 16 + k] * E15[t * MARG_E15_LD + k];
    out[i * 16 + perm[t]] = s;
  }
}

// phase 8: the kept block  G <- Arr - X * Amr ; b <- brr - X * bmm  (X = Arm Amm^+), out to mg_A / mg_b as it is and into
// G / bv, where the copy the factorisation works on is symmetrised (the reference eigen-decomposes A as it is).  Two
// barriers inside: bv is read whole before its head is rewritten; the lower triangle of G before the upper.
template <int T>
__device__ __forceinline__ void marg_kept_block(const DevBatch& B, const int w, const int n, const int md, const int ldd, const int ldm,
                                                const double* Ad, const double* X, double* bv, double* G) {
  const int tid = threadIdx.x;
  double* Aout = B.mg_A + (size_t)w * MAXKEEP * MAXKEEP;
  double* bout = B.mg_b + (size_t)w * MAXKEEP;
  for (int it = tid; it < n * n; it += T) {
    const int i = it / n, j = it % n;
    double s = 0;
    for (int k = 0; k < md; ++k) s += X[i * 16 + k] * Ad[k * ldd + md + j];
    const double v = Ad[(md + i) * ldd + md + j] - s;
    Aout[i * n + j] = v;
    G[i * ldm + j] = v;
  }
  double bkeep = 0.0;   // (n <= MAXKEEP < T: one entry per thread; read back from HBM it cost a store completion + a round trip)
  if (tid < n) {
    double s = 0;
    for (int k = 0; k < md; ++k) s += X[tid * 16 + k] * bv[k];
    bkeep = bv[md + tid] - s;
    bout[tid] = bkeep;
  }
  __syncthreads();
  if (tid < n) bv[tid] = bkeep;
  for (int it = tid; it < n * n; it += T) {
    const int i = it / n, j = it % n;
    if (i > j) G[i * ldm + j] = 0.5 * (G[i * ldm + j] + G[j * ldm + i]);
  }
  __syncthreads();
  for (int it = tid; it < n * n; it += T) {
    const int i = it / n, j = it % n;
    if (i < j) G[i * ldm + j] = G[j * ldm + i];
  }
}

// phase 9: factor of the kept block (:349-357), the form chosen by n and the thread count.
// The reference sets J0 = sqrt(S) V^T, r0 = S^-1/2 V^T b from A = V S V^T.  The prior enters every later computation
// only through |r0 + J0 dx|^2, i.e. through J0^T J0 = A and J0^T r0 = (b projected on range A); any J0' = Q J0,
// r0' = Q r0 with Q orthogonal is the same prior.  The pivoted Cholesky factor is such a pair and needs no
// eigen-iteration:  P A P^T = L L^T,  J0 = L^T P^T,  L(0:r,0:r) r0 = (P b)(0:r)  (the forward substitution rides along).
// The kept block is the difference of numbers five orders larger (A = Arr - Arm Amm^+ Amr after the landmark
// elimination): what the reference's eigen-solver reports below ~1e-10 lambda_max of it is rounding noise of either
// sign (it keeps the positive part above 1e-8 with a negligible weight).  Pivots below max(1e-8, 1e-9 max diagonal)
// end the factorisation; the trailing block is treated as zero.
// kept blocks of up to 48 dims: one wave, whole columns in registers; up to 76 (the reference's steady state is 75): four
// waves with half columns (round 4); the work-group version remains for 77..80 and behind VPL_MARG_WG_FACTOR (A/B runs).
// scratch: what the register forms ask for (MargLayout::fG); col: the work-group version's pivot column (MargLayout::wgcol).
template <int T>
__device__ __forceinline__ int marg_factor_kept(const DevBatch& B, const int w, const int n, const int ldm, double* G, double* bv, int* perm,
                                                double* scratch, double* red, double* col, int* s_flag, int* s_phase) {
  int rank;
#ifdef VPL_MARG_WG_FACTOR
  constexpr bool use_wave4 = false;
#else
  constexpr bool use_wave4 = T >= 512;   // eight waves: two column groups x four row slices
#endif
  if (n <= PSD_NMAX_WAVE) rank = psd_pivoted_cholesky_wave<PSD_NMAX_WAVE>(G, n, ldm, perm, s_flag, kMargNoiseRel, kMargEps, bv, scratch);
  else if (use_wave4 && n <= PSD_WAVE4_NH * PSD_WAVE4_NQ) {
#ifdef VPL_STAMPS
    rank = psd_pivoted_cholesky_wave4<PSD_WAVE4_NH, PSD_WAVE4_NQ>(G, n, ldm, perm, s_flag, kMargNoiseRel, kMargEps, bv, scratch, s_phase, B.dbg + (size_t)w * 64 + 40);
#else
    rank = psd_pivoted_cholesky_wave4<PSD_WAVE4_NH, PSD_WAVE4_NQ>(G, n, ldm, perm, s_flag, kMargNoiseRel, kMargEps, bv, scratch, s_phase);
#endif
    // a hand-shake that timed out (never observed) leaves G and bv as they were -- the columns live in registers until the
    // routine's last pass: the work-group version takes over
    if (rank < 0) rank = psd_pivoted_cholesky(G, n, ldm, perm, red, s_flag, kMargNoiseRel, kMargEps, bv, col);
  } else rank = psd_pivoted_cholesky(G, n, ldm, perm, red, s_flag, kMargNoiseRel, kMargEps, bv, col);
  return rank;
}

// phase 10 (behind marg_write_prior): x0 of the kept blocks, the linearisation point (preMarginalize copies, :110-129)
__device__ __forceinline__ void marg_x0(const DevBatch& B, const int w, const int nb) {
  const int tid = threadIdx.x;
  if (tid < nb) {
    const int kind = B.mg_kind[(size_t)w * MAXPB + tid];
    const int base = B.mg_cam[(size_t)w * MAXPB + tid];
    const double* x = kind == 0 ? B.pose + ((size_t)w * NF + base / 15) * 7
                      : kind == 1 ? B.sb + ((size_t)w * NF + base / 15) * 9 : B.ex + (size_t)w * 7;
    const int gs = kind == 1 ? 9 : 7;
    for (int k = 0; k < 9; ++k) B.mg_x0[((size_t)w * MAXPB + tid) * 9 + k] = k < gs ? x[k] : 0.0;
  }
}

template <int T>
__device__ __forceinline__ void marg_body(const DevBatch& B, const int w, double* sm) {
  const int tid = threadIdx.x;
  const int nL = B.nL[w];
  const int nb = B.mg_nb[w];
  const int n = B.mg_n[w];
  if (n == 0) return;   // MARGIN_SECOND_NEW without pose[WINDOW_SIZE-1] in the prior: nothing to do (estimator.cpp:1385)
  const bool second_new = B.opt.marginalization_flag == 1;
  const int md = second_new ? 6 : MARG_MD;   // dims marginalised through the pseudo-inverse
  // the window's own layout; the dispatch holds the largest of every n up to the batch's (marg_lds_doubles)
  const MargLayoutT<double*> L = marg_layout_at(sm, n, T == 256, md);
  const int nd = L.nd, ldd = L.ldd, ldm = L.ldm, MTROWS = L.mtrows, LOFF = L.loff;
  double* G = L.G.at;
  double* Ad = L.Ad.at;
  double* tile = L.tile.at;
  double* E15 = L.E15.at;
  double* bv = L.bv.at;
  double* tmp = L.tmp.at;
  double* lam = L.lam.at;
  double* red = L.red.at;
  int* perm = (int*)L.perm.at;
  int* dmap = (int*)L.dmap.at;
  int* lst = (int*)L.lst.at;
  __shared__ int s_np0, s_nl0, s_flag[4], s_phase[4];

  marg_dense_map<T>(B, w, md, nb, nL, second_new, LOFF, dmap, lst, &s_np0, &s_nl0);
  __syncthreads();
  VPL_STAMP(B, w, 32);
  // ---- landmark elimination (plain inverse of the block-diagonal landmark part, :316-326) --------
  // rows X = C^-1 [W | g] per start-frame-0 landmark (C C^T = H_ll); A = Hcc - X^T X, b = gc - X^T z
  // tmp, first tenants: vlist and vinv (tmp's owner, Arm Amm^-1, arrives behind the last X^T X)
  int* vlist = (int*)L.vlist.at;
  int* vinv = (int*)L.vinv.at;
  marg_gather<T>(B, w, nd, ldd, dmap, Ad, bv, vlist, vinv, s_flag);   // (one barrier inside)
  __syncthreads();
  const int np0 = s_np0, nl0 = s_nl0;
  VPL_STAMP(B, w, 39);
  // tmp, second tenants, beside vinv: the constants of the rows of one pass.  A pass writes them behind the barrier that ends
  // the X^T X of the pass before (nobody reads them there any more) and reads them behind the barrier inside its staging.
  double* rs = L.rs.at;
  double* lineC = L.lineC.at;
  int* rstart = (int*)L.rstart.at;
  int* rland = (int*)L.rland.at;
  for (int base = 0; base < np0 + nl0; ) {
    int nrows;
    if (base < np0) {
      const int cnt = min(MTROWS, np0 - base);
      nrows = cnt;
      marg_stage_points<T>(B, w, cnt, lst + base, rs, rstart, rland, tile);   // (one barrier inside)
      base += cnt;
    } else {
      const int l0 = base - np0;
      const int cnt = min(MTROWS / 4, nl0 - l0);
      nrows = 4 * cnt;
      marg_stage_lines<T>(B, w, cnt, lst + LOFF + l0, lineC, rstart, rland, tile);   // (one barrier inside)
      base += cnt;
    }
    __syncthreads();   // the rows are staged
    VPL_STAMP(B, w, base <= np0 ? 29 : 30);
    marg_xtx<T>(nrows, tile, vinv, Ad, ldd, bv);
    __syncthreads();   // tile and the row constants are free for the next pass; behind the last pass tile goes to Y and the
                       // 15 x 15 factorisation, tmp to Arm Amm^-1
  }

  VPL_STAMP(B, w, 33);
  // ---- marginalise the md pose-like dims through the eigen pseudo-inverse (:329-346) ----------
  //      Amm^+ = sum_{lambda_k > eps} b_k b_k^T / lambda_k^2   with Amm = B B^T, b_k orthogonal, |b_k|^2 = lambda_k
  for (int it = tid; it < md * md; it += T) {
    const int i = it / md, j = it % md;
    E15[i * MARG_E15_LD + j] = 0.5 * (Ad[i * ldd + j] + Ad[j * ldd + i]);
  }
  __syncthreads();
  // Positive definite Amm (every eigenvalue far above the reference's 1e-8): the pseudo-inverse is the inverse and two
  // triangular solves per row of Arm replace the eigen-decomposition.  A rank-deficient Amm (a pivot at the rounding
  // level) takes the spectral route, which reproduces the eigenvalue test of :334-346.
  // tile, second tenants (handed over by the barrier that ended the last X^T X, or by the one above for a window without
  // frame-0 landmarks): Y and the scratch of the 15 x 15 factorisations.  BOTH start at tile: the factorisation below
  // overwrites the copy of Amm that Y keeps for the fallback.
  double* Y = L.Y.at;
  double* f15 = L.f15.at;
  for (int it = tid; it < md * md; it += T) Y[it] = E15[(it / md) * MARG_E15_LD + it % md];   // keep a copy for the fallback
  __syncthreads();
  const int rank_mm = psd_pivoted_cholesky_wave<PSD_NMAX_AMM>(E15, md, MARG_E15_LD, perm, s_flag, 0.0, kMargEps, nullptr, f15);
  if (rank_mm == md) {
    VPL_STAMP(B, w, 34);
    // lam, first tenant: rdiag, the md reciprocals of the diagonal of L (its owner, the pivot column of the work-group
    // factorisation of the kept block, arrives behind the barriers of marg_kept_block)
    double* rdiag = L.rdiag.at;
    marg_elim_cholesky<T>(n, md, ldd, Ad, E15, perm, rdiag, tmp);   // (one barrier inside)
    __syncthreads();
  } else {
    for (int it = tid; it < md * md; it += T) E15[(it / md) * MARG_E15_LD + it % md] = Y[it];
    __syncthreads();
    // lam: the eigenvalues (rdiag is not written on this route)
    psd_spectral_factor(E15, md, MARG_E15_LD, perm, lam, red, s_flag, 0.0, f15);
    VPL_STAMP(B, w, 34);
    marg_elim_spectral<T>(n, md, ldd, Ad, E15, perm, lam, Y, tmp);   // (one barrier inside; the routine's last barrier freed f15 for Y)
    __syncthreads();
  }
  marg_kept_block<T>(B, w, n, md, ldd, ldm, Ad, tmp, bv, G);   // (two barriers inside)
  __syncthreads();   // the kept block is in G: Ad (the dense block) goes to the scratch of the register forms, lam to the
                     // pivot column of the work-group version
  VPL_STAMP(B, w, 35);
  const int rank = marg_factor_kept<T>(B, w, n, ldm, G, bv, perm, L.fG.at, red, L.wgcol.at, s_flag, s_phase);
  VPL_STAMP(B, w, 36);
  marg_write_prior<T>(B.mg_J0 + (size_t)w * MAXKEEP * MAXKEEP, B.mg_r0 + (size_t)w * MAXKEEP, G, bv, perm, n, ldm, rank);
  marg_x0(B, w, nb);
  VPL_STAMP(B, w, 37);
}
template <int T>
__global__ __launch_bounds__(T) void k_marg(DevBatch B) {
  extern __shared__ double sm[];
  marg_body<T>(B, blockIdx.x, sm);
}

// ---------------------------------------------------------------------------------------------------
// Prior hand-over, re-stride and state pack: the small kernels around the marginalisation.

// Prior handoff on the device (vpl_ba_upload_chained): the prior the previous solve's marginalisation left in mg_* becomes the
// prior of the window that is about to be solved -- J0 (n x n, re-strided from MAXKEEP^2 to the batch's prS), r0, x0.  The
// block tables travel through the host (a few ints per window; upload builds its layout tables from them).
// keep[w] != 0: the window keeps the prior it already has in pr_* (MARGIN_SECOND_NEW left it untouched, estimator.cpp:1385).
__global__ void k_prior_handoff(DevBatch B, const int* keep) {
  const int w = blockIdx.x;
  if (keep[w]) return;
  const int n = B.mg_n[w];
  const double* J = B.mg_J0 + (size_t)w * MAXKEEP * MAXKEEP;
  double* Jo = B.pr_J0 + (size_t)w * B.prS;
  for (int i = threadIdx.x; i < n * n; i += blockDim.x) Jo[i] = J[i];
  for (int i = threadIdx.x; i < n; i += blockDim.x) B.pr_r0[(size_t)w * MAXPN + i] = B.mg_r0[(size_t)w * MAXKEEP + i];
  for (int i = threadIdx.x; i < MAXPB * 9; i += blockDim.x) B.pr_x0[(size_t)w * MAXPB * 9 + i] = B.mg_x0[(size_t)w * MAXPB * 9 + i];
}

// Chained upload whose batch stride of pr_J0 changed: the windows that KEEP their prior have J0 at w * old_prS.  phase 0 copies
// their n x n into tmp[w][MAXPN^2], phase 1 (next launch) back to w * B.prS.  pr_n still holds the kept prior's size (the new
// tables are scattered after this).
__global__ void k_prior_restride(DevBatch B, const int* keep, int old_prS, double* tmp, int phase) {
  const int w = blockIdx.x;
  if (!keep[w]) return;
  const int n = B.pr_n[w];
  double* T = tmp + (size_t)w * MAXPN * MAXPN;
  if (phase == 0) {
    const double* J = B.pr_J0 + (size_t)w * old_prS;
    for (int i = threadIdx.x; i < n * n; i += blockDim.x) T[i] = J[i];
  } else {
    double* J = B.pr_J0 + (size_t)w * B.prS;
    for (int i = threadIdx.x; i < n * n; i += blockDim.x) J[i] = T[i];
  }
}

// Per-window states of the solved batch as one [nW][183] device array (pose 77 | speed/bias 99 | extrinsic 7): what the
// multi-GPU run all-gathers over RCCL, packed on the device so that the collective reads HBM, not a host staging copy.
__global__ void k_pack_states(DevBatch B, double* out) {
  const int w = blockIdx.x;
  for (int i = threadIdx.x; i < 183; i += blockDim.x)
    out[(size_t)w * 183 + i] = i < 77 ? B.pose[(size_t)w * 77 + i] : (i < 176 ? B.sb[(size_t)w * 99 + (i - 77)] : B.ex[(size_t)w * 7 + (i - 176)]);
}

}  // namespace vpl
