// The upload of a window batch (vpl_ba_upload, vpl_ba_upload_chained and the upload inside every other window entry point of
// vplines_ba.hip), as named phases around ONE host-to-device copy of the staging arena (ba_stage.h).  An upload has one integer
// side, always built here on the host from the windows' tracks (take_tables / pack_tracks, the layout tables, the prior's and
// the kept blocks' tables), and ONE OF TWO sources for its doubles:
//   values : the caller's arrays, packed into the arena (take_values / pack_values);
//   gather : the store of a keyframe session (ba_session.h), on the device already -- the arena carries the index tables
//            (take_gather / pack_gather) and k_odo_gather / k_odo_prior_load run behind the scatter.
// The choice is made in take_upload, stage_upload and upload_body, nowhere else.
#pragma once
#include "ba_ctx.h"
#include "ba_odo.h"
#include "ba_pack.h"
#include "host_common.h"

static void to_dev_preint(const vpl_preintegration& p, DevPreint& d) {
  d.sum_dt = p.sum_dt;
  for (int k = 0; k < 3; ++k) { d.dp[k] = p.delta_p[k]; d.dv[k] = p.delta_v[k]; d.lba[k] = p.linearized_ba[k]; d.lbg[k] = p.linearized_bg[k]; }
  for (int k = 0; k < 4; ++k) d.dq[k] = p.delta_q[k];
  auto blk = [&](double* o, int r0, int c0) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) o[3 * i + j] = p.jacobian[(r0 + i) * 15 + c0 + j];
  };
  blk(d.dp_dba, 0, 9); blk(d.dp_dbg, 0, 12); blk(d.dq_dbg, 3, 12); blk(d.dv_dba, 6, 9); blk(d.dv_dbg, 6, 12);
  std::memcpy(d.cov, p.covariance, sizeof(d.cov));
  std::memset(d.sqrt_info, 0, sizeof(d.sqrt_info));
}

// The arrays one upload packs, pieces of the pinned arena (Stage).  take_upload and take_units are the one description of their
// sizes and stage_upload the one list of where they go: upload_bound is a dry run of the three.
struct UploadArena {
  Span<double> pose, sb, ex, invd, plk, pt_obs, ln_obs, fail_ref, orth, pr_x0, pr_r0;
  Span<int> nP, nL, pt_start, pt_nobs, pt_off, ln_start, ln_nobs, ln_off, ln_tri, pu_cnt, pu_cnt0, sk_tab, sk_wave, path, nLO, lo_ln,
      ll_tab, ll_np, ps_list, ps_cnt, orth_in, pr_n, pr_nb, pr_kind, pr_frame, pr_idx, mg_n, mg_nb, mg_kind, mg_frame, mg_idx, mg_cam, mg_m;
  Span<DevPreint> pre;
  std::vector<Span<double>> J0;                  // per window: J0 of the incoming prior (empty: none, or a chained upload)
  std::vector<Span<int>> pu_lane, pu_sub;        // per window: the first rounds of its point work units (same count for all)
  Span<int> odo_psrc, odo_lsrc, odo_has, odo_marg;   // session upload: the gather's index tables, who gets a new prior
};

// block table of a prior that stays on the device (chained upload)
struct HostTab {
  int n = 0, nb = 0, kind[MAXPB], frame[MAXPB], idx[MAXPB];
  bool keep = false;                             // MARGIN_SECOND_NEW passed this window's prior through: pr_*, not mg_*
};

// The gather source: an upload on behalf of a keyframe session (vpl_odo_*).  The windows carry the INTEGER side only (track
// starts and lengths, triangulation flags, preint[1].sum_dt); every double of the batch -- states, observations, inverse depths,
// lines, pre-integrations, the prior's values -- is on the device already and is gathered from the session's store behind the
// upload's scatter (k_odo_gather, k_odo_prior_load).  Window w is sequence w.
struct OdoSrc {
  OdoStore store;
  OdoPrior prior;
  int *d_psrc, *d_lsrc, *d_has, *d_marg;         // [W][maxP], [W][maxL]: selected track -> store track; [W]: has a prior; [W]: 1 + kept
                                                 // blocks of the prior this batch's marginalisation writes (0: none)
  const std::vector<int>* psrc;                  // per window: store track of point track p
  const std::vector<int>* lsrc;                  // per window: store track of the CALLER's line l
  const HostTab* tab;                            // per window: block table of the session's prior (null: this upload takes no prior)
  const unsigned char* has;                      // per window: the session holds a prior
};

// the integer side, the same for every upload (orth_in: 0 unless the caller's values come as orth lines, pack_values)
static void take_tables(Stage& S, UploadArena& A, const DevBatch& B, size_t W) {
  A.nP = S.take<int>(W); A.nL = S.take<int>(W);
  A.pt_start = S.take<int>(W * B.maxP, 0); A.pt_nobs = S.take<int>(W * B.maxP, 0); A.pt_off = S.take<int>(W * B.maxP, 0);
  A.ln_start = S.take<int>(W * B.maxL, 0); A.ln_nobs = S.take<int>(W * B.maxL, 0); A.ln_off = S.take<int>(W * B.maxL, 0);
  A.ln_tri = S.take<int>(W * B.maxL, 1);
  A.pu_cnt = S.take<int>(W, 0); A.pu_cnt0 = S.take<int>(W, 0);
  A.sk_tab = S.take<int>(W * B.maxKS * 4, 0); A.sk_wave = S.take<int>(W * 8 * SK_WSTRIDE, -1); A.path = S.take<int>(W, 0);
  A.nLO = S.take<int>(W, 0); A.lo_ln = S.take<int>(W * B.maxLO, 0); A.ll_tab = S.take<int>(W * B.llSlots * 2, -1); A.ll_np = S.take<int>(W, 0);
  A.ps_list = S.take<int>(W * B.maxP, 0); A.ps_cnt = S.take<int>(W * (NF + 1), 0);
  A.orth_in = S.take<int>(W, 0);
  A.pr_n = S.take<int>(W, 0); A.pr_nb = S.take<int>(W, 0);
  A.pr_kind = S.take<int>(W * MAXPB, 0); A.pr_frame = S.take<int>(W * MAXPB, 0); A.pr_idx = S.take<int>(W * MAXPB, 0);
  A.mg_n = S.take<int>(W, 0); A.mg_nb = S.take<int>(W, 0); A.mg_kind = S.take<int>(W * MAXPB, 0); A.mg_frame = S.take<int>(W * MAXPB, 0);
  A.mg_idx = S.take<int>(W * MAXPB, 0); A.mg_cam = S.take<int>(W * MAXPB, 0);
  A.mg_m = S.take<int>(W);
}
// the caller's doubles (chained: the priors' values stay on the device, no J0 travels)
static void take_values(Stage& S, UploadArena& A, const DevBatch& B, size_t W, const vpl_window* win, bool chained) {
  A.pose = S.take<double>(W * 77); A.sb = S.take<double>(W * 99); A.ex = S.take<double>(W * 7); A.invd = S.take<double>(W * B.maxP, 1.0);
  A.plk = S.take<double>(W * B.maxL * 6, 0.0);
  A.pt_obs = S.take<double>(W * B.maxPO * 3, 0.0); A.ln_obs = S.take<double>(W * B.maxLO * 8, 0.0);
  A.pre = S.take<DevPreint>(W * NF);
  A.fail_ref = S.take<double>(W * 13, 0.0); A.orth = S.take<double>(W * B.maxL * 4, 0.0);
  A.pr_x0 = S.take<double>(W * MAXPB * 9, 0.0); A.pr_r0 = S.take<double>(W * MAXPN, 0.0);
  A.J0.assign(W, Span<double>());
  for (size_t w = 0; w < W; ++w)
    if (!chained && win[w].has_prior && win[w].prior && win[w].prior->n > 0) A.J0[w] = S.take<double>((size_t)win[w].prior->n * win[w].prior->n);
}
// the session's index tables
static void take_gather(Stage& S, UploadArena& A, const DevBatch& B, size_t W) {
  A.odo_psrc = S.take<int>(W * B.maxP, 0); A.odo_lsrc = S.take<int>(W * B.maxL, 0); A.odo_has = S.take<int>(W, 0); A.odo_marg = S.take<int>(W, 0);
}
static void take_upload(Stage& S, UploadArena& A, const DevBatch& B, size_t W, const vpl_window* win, bool chained, const OdoSrc* odo) {
  take_tables(S, A, B, W);
  if (odo) take_gather(S, A, B, W);
  else take_values(S, A, B, W, win, chained);
}
static void take_units(Stage& S, UploadArena& A, size_t W, int rounds) {
  A.pu_lane.clear();
  A.pu_sub.clear();
  if (rounds <= 0) return;
  for (size_t w = 0; w < W; ++w) A.pu_lane.push_back(S.take<int>((size_t)rounds * 1024));
  for (size_t w = 0; w < W; ++w) A.pu_sub.push_back(S.take<int>((size_t)rounds * 512));
}
// every piece to its device array(s): the segments of the upload's one copy
static void stage_upload(Stage& S, const UploadArena& A, const DevBatch& B, size_t W, bool same_layout, bool chained, const OdoSrc* odo) {
  // (a session upload: the double arrays were not taken -- empty pieces make no segment -- and the gather's tables go along)
  S.put(B.pose, A.pose); S.put(B.sb, A.sb); S.put(B.ex, A.ex); S.put(B.invd, A.invd);
  S.put(B.plk, A.plk); S.put(B.fail_ref, A.fail_ref); S.put(B.orth_in, A.orth_in); S.put(B.orth, A.orth);
  S.put(B.pose_0, A.pose); S.put(B.sb_0, A.sb); S.put(B.ex_0, A.ex); S.put(B.invd_0, A.invd); S.put(B.plk_0, A.plk);
  S.put(B.pt_obs, A.pt_obs);
  if (odo) { S.put(odo->d_psrc, A.odo_psrc); S.put(odo->d_lsrc, A.odo_lsrc); S.put(odo->d_has, A.odo_has); S.put(odo->d_marg, A.odo_marg); }
  if (!same_layout) {
    S.put(B.nP, A.nP); S.put(B.nL, A.nL);
    S.put(B.pt_start, A.pt_start); S.put(B.pt_nobs, A.pt_nobs); S.put(B.pt_off, A.pt_off);
    S.put(B.ps_list, A.ps_list); S.put(B.ps_cnt, A.ps_cnt);
    for (size_t w = 0; w < A.pu_lane.size(); ++w) {
      S.put(B.pu_lane + w * (size_t)B.maxPR * 1024, A.pu_lane[w]);
      S.put(B.pu_sub + w * (size_t)B.maxPR * 512, A.pu_sub[w]);
    }
    S.put(B.pu_cnt, A.pu_cnt); S.put(B.pu_cnt0, A.pu_cnt0);
    S.put(B.ln_start, A.ln_start); S.put(B.ln_nobs, A.ln_nobs); S.put(B.ln_off, A.ln_off);
    S.put(B.nLO, A.nLO); S.put(B.lo_ln, A.lo_ln);
    S.put(B.ll_tab, A.ll_tab); S.put(B.ll_np, A.ll_np);
    S.put(B.sk_tab, A.sk_tab); S.put(B.sk_wave, A.sk_wave);
  }
  S.put(B.ln_obs, A.ln_obs); S.put(B.ln_tri, A.ln_tri);
  S.put(B.pre, A.pre);
  S.put(B.pr_n, A.pr_n); S.put(B.pr_nb, A.pr_nb); S.put(B.pr_kind, A.pr_kind); S.put(B.pr_frame, A.pr_frame); S.put(B.pr_idx, A.pr_idx);
  if (!chained) {
    S.put(B.pr_x0, A.pr_x0); S.put(B.pr_r0, A.pr_r0);
    for (size_t w = 0; w < W; ++w) S.put(B.pr_J0 + w * (size_t)B.prS, A.J0[w]);
  }
  S.put(B.mg_n, A.mg_n); S.put(B.mg_nb, A.mg_nb); S.put(B.mg_kind, A.mg_kind);
  S.put(B.mg_frame, A.mg_frame); S.put(B.mg_idx, A.mg_idx); S.put(B.mg_cam, A.mg_cam); S.put(B.mg_m, A.mg_m);
  S.put(B.path, A.path);
}
// the arena an upload needs: its pieces, with every window's point work units at the capacity, and its segment table
static size_t upload_bound(const DevBatch& B, size_t W, const vpl_window* win, bool same_layout, bool chained, const OdoSrc* odo) {
  Stage dry;
  dry.dry = true;
  UploadArena A;
  take_upload(dry, A, B, W, win, chained, odo);
  take_units(dry, A, W, B.maxPR);
  stage_upload(dry, A, B, W, same_layout, chained, odo);
  return dry.bound();
}

// 1. the refusals that leave the previous batch as it was
static int upload_check(vpl_ctx* c, int nW, const vpl_window* win, const vpl_ba_options* opt, bool chained) {
  if (!c || !win || !opt || nW < 1) return VPL_E_INVALID;
  if (nW > c->maxW) return fail(c, VPL_E_CAPACITY, "more windows than max_windows");
  if (opt->marginalization_flag != VPL_MARGIN_OLD && opt->marginalization_flag != VPL_MARGIN_SECOND_NEW &&
      opt->marginalization_flag != VPL_MARGIN_NONE)
    return fail(c, VPL_E_INVALID, "unknown marginalization_flag");
  HIPCHK(c, hipSetDevice(c->device));
  { const int rs = settle_call(c); if (rs) return rs; }   // an asynchronous call whose results have not been collected yet
  // chained: the priors of THIS batch size must be resident, i.e. the context's last upload was solved (or marginalised) with a
  // marginalisation and nothing was uploaded since (any upload rewrites mg_n / mg_nb / mg_kind, the tables of the NEXT prior)
  if (chained && (!c->prior_resident || c->prior_resident_nW != nW))
    return fail(c, VPL_E_INVALID, "upload_chained: needs a previous solve of the same batch size with a marginalisation, and no upload since");
  return VPL_OK;
}

// 2. chained upload: window w takes the prior the context's previous solve left for window w (device resident); only its
// block table comes through the host -- the ten tables in one gather and one device-to-host copy of the arena
static int read_resident_priors(vpl_ctx* c, size_t W, std::vector<HostTab>& tab) {
  const DevBatch& B = c->B;
  int* const src[10] = {B.mg_n, B.mg_nb, B.mg_kind, B.mg_frame, B.mg_idx, B.pr_n, B.pr_nb, B.pr_kind, B.pr_frame, B.pr_idx};
  Span<int> t[10];   // [0, 5): mg_* (the next prior), [5, 10): pr_* (the prior a pass-through window keeps)
  auto plan = [&](Stage& S) {
    for (int k = 0; k < 10; ++k) {
      t[k] = S.take<int>(k % 5 < 2 ? W : W * MAXPB);
      S.from_device(t[k].p, src[k], t[k].n);
    }
  };
  HIPCHK(c, stage_plan(c->stage, plan));
  HIPCHK(c, stage_run(c->stage, c->stream, false));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  tab.resize(W);
  for (size_t w = 0; w < W; ++w) {
    HostTab& T = tab[w];
    T.keep = c->h_passthrough[w] >= 0;      // MARGIN_SECOND_NEW left this window's prior as it was
    const Span<int>* s = t + (T.keep ? 5 : 0);
    T.n = s[0][w];
    T.nb = s[1][w];
    if (T.n < 0 || T.n > MAXPN || T.nb < 0 || T.nb > MAXPB) return fail(c, VPL_E_INVALID, "upload_chained: resident prior table out of range");
    for (int b = 0; b < T.nb; ++b) {
      T.kind[b] = s[2][w * MAXPB + b];
      T.frame[b] = s[3][w * MAXPB + b];
      T.idx[b] = s[4][w * MAXPB + b];
    }
  }
  return VPL_OK;
}

// 3. batch strides: of the prior matrices (the largest prior) and of the compact W rows (the longest track); zero fill only where
// some slot has no writer
static int batch_strides(vpl_ctx* c, size_t W, const vpl_window* win, const vpl_ba_options* opt, const HostTab* ctab) {
  DevBatch& B = c->B;
  int nmax = 1;
  for (size_t w = 0; w < W; ++w) {
    if (ctab) nmax = std::max(nmax, ctab[w].n);
    else if (win[w].has_prior && win[w].prior) nmax = std::max(nmax, win[w].prior->n);
  }
  if (nmax > MAXPN) return fail(c, VPL_E_CAPACITY, "prior larger than MAXPN");
  B.prS = (nmax * nmax + 7) & ~7;
  int maxTrack = 2, minTrack = NF;
  for (size_t w = 0; w < W; ++w) {
    for (int p = 0; p < win[w].n_points; ++p) { maxTrack = std::max(maxTrack, win[w].point_nobs[p]); minTrack = std::min(minTrack, win[w].point_nobs[p]); }
    for (int l = 0; l < win[w].n_lines; ++l) { maxTrack = std::max(maxTrack, win[w].line_nobs[l]); minTrack = std::min(minTrack, win[w].line_nobs[l]); }
  }
  maxTrack = std::min(maxTrack, (int)NF);
  B.WS = 6 * maxTrack + 6;
  // the line phase's lane layout is each window's own (build_layout); k_lin's gate `lane / llNLW < llK` in front of its table
  // load stays open for every lane, the table alone says which lanes have an observation (-1: none)
  B.llK = 64;
  B.llNLW = 1;
  B.wfill = (minTrack != maxTrack || opt->remove_line_outliers) ? 1 : 0;
  return VPL_OK;
}

// 4. signature of the track layout: when it is the last upload's, the lane / unit / K-step tables and the index arrays on the
// device are the right ones.  The decision is an exact comparison of the integers the layout is made of (anything weaker would
// reuse lane / unit / K-step tables of another track layout: out-of-range reads -- ADVICE r3).
static bool layout_unchanged(vpl_ctx* c, size_t W, const vpl_window* win, bool all_lines) {
  const DevBatch& B = c->B;
  std::vector<int> key = {(int)W, B.WS, B.llK, B.llNLW, B.wfill, all_lines ? 1 : 0, B.maxP, B.maxL};
  key.reserve(16 + W * 8);
  for (size_t w = 0; w < W; ++w) {
    const vpl_window& v = win[w];
    key.push_back(v.n_points); key.push_back(v.n_lines);
    const bool hp = v.n_points > 0 && v.point_start && v.point_nobs, hl = v.n_lines > 0 && v.line_start && v.line_nobs;
    const bool ht = v.n_lines > 0 && v.line_triangulated;
    key.push_back((hp ? 1 : 0) | (hl ? 2 : 0) | (ht ? 4 : 0));   // which arrays follow
    if (hp) { key.insert(key.end(), v.point_start, v.point_start + v.n_points); key.insert(key.end(), v.point_nobs, v.point_nobs + v.n_points); }
    if (hl) { key.insert(key.end(), v.line_start, v.line_start + v.n_lines); key.insert(key.end(), v.line_nobs, v.line_nobs + v.n_lines); }
    if (ht) key.insert(key.end(), v.line_triangulated, v.line_triangulated + v.n_lines);
  }
  const bool same = c->layout_valid && key == c->layout_key;
  c->layout_key.swap(key);
  c->layout_valid = false;       // becomes valid when this upload has gone through
  return same;
}

// 5. the tracks of window w: range checks, the capacity refusals, the integer tables; h_lmap[w][dl] is the caller's index of
// device line dl
static int pack_tracks(vpl_ctx* c, UploadArena& A, size_t w, const vpl_window& v, bool all_lines) {
  const DevBatch& B = c->B;
  if (v.n_points > B.maxP || v.n_lines > B.maxL) return fail(c, VPL_E_CAPACITY, "too many tracks for the context");
  A.nP[w] = v.n_points;
  c->h_nP[w] = v.n_points;
  int off = 0;
  for (int p = 0; p < v.n_points; ++p) {
    const int s = v.point_start[p], no = v.point_nobs[p];
    if (s < 0 || no < 2 || s + no > NF) return fail(c, VPL_E_INVALID, "point track outside the window");
    if (off + no > B.maxPO) return fail(c, VPL_E_CAPACITY, "too many point observations");
    A.pt_start[w * B.maxP + p] = s; A.pt_nobs[w * B.maxP + p] = no; A.pt_off[w * B.maxP + p] = off;
    off += no;
  }
  off = 0;
  int nl = 0;
  std::vector<int>& lmap = c->h_lmap[w];
  lmap.clear();
  for (int l = 0; l < v.n_lines; ++l) {
    const int s = v.line_start[l], no = v.line_nobs[l];
    if (s < 0 || no < 1 || s + no > NF) return fail(c, VPL_E_INVALID, "line track outside the window");
    const int tri_flag = (!v.line_triangulated || v.line_triangulated[l]) ? 1 : 0;
    // lines that are not triangulated take no part in the solves (estimator.cpp:1133); they travel only for
    // vpl_ba_triangulate_lines
    if (all_lines || tri_flag) {
      if (off + no > B.maxLO) return fail(c, VPL_E_CAPACITY, "too many line observations");
      const size_t dl = w * B.maxL + nl;
      A.ln_start[dl] = s; A.ln_nobs[dl] = no; A.ln_off[dl] = off; A.ln_tri[dl] = tri_flag;
      for (int k = 0; k < no; ++k) A.lo_ln[w * B.maxLO + off + k] = nl;
      off += no;
      lmap.push_back(l);
      ++nl;
    }
  }
  A.nL[w] = nl;
  c->h_nL[w] = nl;
  A.nLO[w] = off;
  return VPL_OK;
}
// ... and its doubles, from one of the two sources.  The caller's arrays: states, the observations and values of the tracks
// pack_tracks took (a line's observations lie at its offset among ALL of the caller's lines), pre-integrations
static void pack_values(const vpl_ctx* c, UploadArena& A, size_t w, const vpl_window& v) {
  const DevBatch& B = c->B;
  std::memcpy(&A.pose[w * 77], v.pose, 77 * 8);
  std::memcpy(&A.sb[w * 99], v.speed_bias, 99 * 8);
  std::memcpy(&A.ex[w * 7], v.ex_pose, 7 * 8);
  if (v.failure_occur) {
    A.fail_ref[w * 13] = 1.0;
    std::memcpy(&A.fail_ref[w * 13 + 1], v.last_P0, 3 * 8);
    std::memcpy(&A.fail_ref[w * 13 + 4], v.last_R0, 9 * 8);
  }
  for (int p = 0; p < v.n_points; ++p) {
    const int off = A.pt_off[w * B.maxP + p], no = v.point_nobs[p];
    std::memcpy(&A.pt_obs[(w * B.maxPO + off) * 3], v.point_obs + (size_t)off * 3, (size_t)no * 3 * 8);
    A.invd[w * B.maxP + p] = v.inv_depth[p];
  }
  const std::vector<int>& lmap = c->h_lmap[w];
  size_t nl = 0;
  int woff = 0;
  for (int l = 0; nl < lmap.size(); woff += v.line_nobs[l], ++l) {
    if (l != lmap[nl]) continue;
    const size_t dl = w * B.maxL + nl++;
    std::memcpy(&A.ln_obs[(w * B.maxLO + A.ln_off[dl]) * 8], v.line_obs + (size_t)woff * 8, (size_t)v.line_nobs[l] * 8 * 8);
    if (v.line_orth) std::memcpy(&A.orth[dl * 4], v.line_orth + (size_t)l * 4, 4 * 8);
    else std::memcpy(&A.plk[dl * 6], v.line_plk + (size_t)l * 6, 6 * 8);
  }
  A.orth_in[w] = v.line_orth ? 1 : 0;
  for (int j = 0; j < NF; ++j) to_dev_preint(v.preint[j], A.pre[w * NF + j]);
}
// The session's store: which of its tracks each selected track is, and whether the session holds a prior for the window
static void pack_gather(const vpl_ctx* c, UploadArena& A, size_t w, const vpl_window& v, const OdoSrc& odo) {
  const DevBatch& B = c->B;
  for (int p = 0; p < v.n_points; ++p) A.odo_psrc[w * B.maxP + p] = odo.psrc[w][p];
  const std::vector<int>& lmap = c->h_lmap[w];
  for (size_t dl = 0; dl < lmap.size(); ++dl) A.odo_lsrc[w * B.maxL + dl] = odo.lsrc[w][lmap[dl]];
  A.odo_has[w] = (odo.tab && odo.has[w]) ? 1 : 0;
}

// 6. layout tables of window w: the point work units of k_lin (into lane / sub, maxPR rounds), the K-steps of k_schur and the
// lane layout of the line phase (ba_pack.h)
static int build_layout(vpl_ctx* c, UploadArena& A, size_t w, const vpl_window& v, int* lane, int* sub, long* wide_w, long* total_w) {
  const DevBatch& B = c->B;
  int* list = &A.ps_list[w * B.maxP];
  int* cnt = &A.ps_cnt[w * (NF + 1)];
  sort_points_by_start(v.n_points, v.point_start, v.point_nobs, list, cnt);
  PointUnitLayout PL;
  if (!pack_point_units(v.point_nobs, &A.pt_off[w * B.maxP], list, cnt, B.maxPR, lane, sub, &PL))
    return fail(c, VPL_E_CAPACITY, "point work-unit table too small");
  A.pu_cnt[w] = PL.rounds;
  A.pu_cnt0[w] = PL.rounds0;
  // a pass that waited for a ticket owned by a unit it never runs would spin forever on the device: replay both chains
  if (!point_unit_chains_finish(sub, PL, false) || !point_unit_chains_finish(sub, PL, true))
    return fail(c, VPL_E_INVALID, "internal: commit-ticket order of the point work units is not executable");
  // K-steps of k_schur: landmark rows by start frame, dealt to the waves, flush tickets; rows wider than the 6-frame view of
  // k_schur<3>: entries with a longer track are flagged wide (k_schur_mixed)
  const int nl = A.nL[w];
  if (pack_schur_ksteps(v.n_points, list, cnt, nl, &A.ln_start[w * B.maxL], B.maxKS, &A.sk_tab[w * B.maxKS * 4],
                        &A.sk_wave[w * 8 * SK_WSTRIDE], SCHUR_THREADS / 64, v.point_nobs, &A.ln_nobs[w * B.maxL],
                        B.WS + 2 > 48 ? SCHUR_NARROW_FRAMES : 0, wide_w, total_w) < 0)
    return fail(c, VPL_E_CAPACITY, "K-step table of the landmark elimination too small");
  // lane layout of the line phase: NLW whole tracks per wave, k-major; tracks in the caller's order (tracks that start in the
  // same frame side by side would pile their LDS adds onto the same addresses).  NLW = 64 / (the longest line track of THIS
  // window): the lanes a window's factors sit in, and with them the order of its sums, are the window's own and not the batch's
  // -- a window gives in any batch what it gives alone.  The device goes by the table: slots without an observation hold -1.
  int KL = 1;
  for (int l = 0; l < v.n_lines; ++l) KL = std::max(KL, std::min(v.line_nobs[l], (int)NF));
  const int NLW = 64 / KL, perPass = 8 * NLW;
  const int np = (nl + perPass - 1) / perPass;
  if (np * 512 > B.llSlots) return fail(c, VPL_E_CAPACITY, "line layout table too small");
  A.ll_np[w] = np;
  for (int dl = 0; dl < nl; ++dl) {
    const int pass = dl / perPass, wave = (dl % perPass) / NLW, i = dl % NLW;
    const int no = std::min(A.ln_nobs[w * B.maxL + dl], (int)NF);
    for (int k = 0; k < no; ++k) {      // (observation, line | k << 16 | start frame << 20): everything a lane's loads need
      int* e = &A.ll_tab[2 * ((size_t)w * B.llSlots + pass * 512 + wave * 64 + k * NLW + i)];
      e[0] = A.ln_off[w * B.maxL + dl] + k;
      e[1] = dl | k << 16 | A.ln_start[w * B.maxL + dl] << 20;
    }
  }
  return VPL_OK;
}

// 7. the incoming prior of window w: its block table (T: the resident one of a chained upload) or the caller's vpl_prior
static int pack_prior(vpl_ctx* c, UploadArena& A, size_t w, const vpl_window& v, const HostTab* T) {
  if (T) {
    A.pr_n[w] = T->n; A.pr_nb[w] = T->nb;
    c->maxPriorN = std::max(c->maxPriorN, T->n);
    for (int b = 0; b < T->nb; ++b) {
      A.pr_kind[w * MAXPB + b] = T->kind[b]; A.pr_frame[w * MAXPB + b] = T->frame[b]; A.pr_idx[w * MAXPB + b] = T->idx[b];
      if (T->kind[b] == 1 && T->frame[b] != 0) A.path[w] = 1;
    }
    return VPL_OK;
  }
  if (!v.has_prior || !v.prior) return VPL_OK;
  const vpl_prior& pr = *v.prior;
  if (pr.n < 0 || pr.n > MAXPN || pr.n_blocks < 0 || pr.n_blocks > MAXPB) return fail(c, VPL_E_INVALID, "bad prior");
  A.pr_n[w] = pr.n; A.pr_nb[w] = pr.n_blocks;
  // k_chol's elimination order keeps speed/bias 0 in its dense part; a prior that ties another frame's speed/bias block
  // (never produced by the reference's marginalisation) takes the general path
  for (int b = 0; b < pr.n_blocks; ++b)
    if (pr.block_kind[b] == 1 && pr.block_frame[b] != 0) A.path[w] = 1;
  c->maxPriorN = std::max(c->maxPriorN, pr.n);
  for (int b = 0; b < pr.n_blocks; ++b) {
    A.pr_kind[w * MAXPB + b] = pr.block_kind[b];
    A.pr_frame[w * MAXPB + b] = pr.block_frame[b];
    A.pr_idx[w * MAXPB + b] = pr.block_idx[b];
    std::memcpy(&A.pr_x0[(w * MAXPB + b) * 9], pr.x0[b], 9 * 8);
    if (pr.block_kind[b] < 0 || pr.block_kind[b] > 2 || pr.block_frame[b] < 0 || pr.block_frame[b] >= NF)
      return fail(c, VPL_E_INVALID, "bad prior block");
  }
  std::memcpy(&A.pr_r0[w * MAXPN], pr.r0, (size_t)pr.n * 8);
  if (pr.n > 0) std::memcpy(A.J0[w].p, pr.J0, (size_t)pr.n * pr.n * 8);
  return VPL_OK;
}

// 8. kept blocks of window w's next prior in the canonical (address) order of the reference's para_* layout
static int keep_blocks(vpl_ctx* c, UploadArena& A, size_t w, const vpl_window& v, const HostTab* T) {
  const DevBatch& B = c->B;
  int* kd = &A.mg_kind[w * MAXPB]; int* fr = &A.mg_frame[w * MAXPB]; int* ix = &A.mg_idx[w * MAXPB]; int* cm = &A.mg_cam[w * MAXPB];
  const int pnb = T ? T->nb : ((v.has_prior && v.prior) ? v.prior->n_blocks : 0);
  const int* pk = pnb ? (T ? T->kind : v.prior->block_kind) : nullptr;
  const int* pf = pnb ? (T ? T->frame : v.prior->block_frame) : nullptr;
  c->h_passthrough[w] = -1;
  if (c->opt.marginalization_flag == VPL_MARGIN_OLD) {
    KeepSrc S;
    S.nP = v.n_points; S.pt_start = v.point_start; S.pt_nobs = v.point_nobs;
    S.nL = A.nL[w]; S.ln_start = &A.ln_start[w * B.maxL]; S.ln_nobs = &A.ln_nobs[w * B.maxL]; S.ln_removed = nullptr;
    S.pr_nb = pnb; S.pr_kind = pk; S.pr_frame = pf;
    S.imu01 = v.preint[1].sum_dt < 10.0;
    int mm = 0;
    keep_tables_old(S, kd, fr, ix, cm, &A.mg_n[w], &A.mg_nb[w], &mm);
    c->h_mg_m[w] = mm;
  } else if (c->opt.marginalization_flag == VPL_MARGIN_SECOND_NEW) {
    const int rc = pnb ? keep_tables_second_new(pnb, pk, pf, kd, fr, ix, cm, &A.mg_n[w], &A.mg_nb[w]) : 0;
    if (rc < 0) return fail(c, VPL_E_INVALID, "MARGIN_SECOND_NEW: the prior holds the speed/bias of frame WINDOW_SIZE-1");
    if (rc == 1) { c->h_mg_m[w] = 6; c->any_second_new = true; }
    else if (pnb) {   // the reference leaves last_marginalization_info as it is (estimator.cpp:1385)
      c->h_passthrough[w] = (int)c->h_pass_priors.size();
      if (T) {          // the prior lives on the device only: the pass-through entry carries its table (download refetches the rest)
        vpl_prior hp;
        std::memset(&hp, 0, sizeof(int) * (2 + 3 * VPL_MAX_PRIOR_BLOCKS));
        hp.n = -1;      // marker: not available on the host
        c->h_pass_priors.push_back(hp);
      } else {
        c->h_pass_priors.push_back(*v.prior);
      }
    }
  }
  if (A.mg_n[w] > MAXKEEP) return fail(c, VPL_E_CAPACITY, "marginalisation keeps more than MAXKEEP dims");
  return VPL_OK;
}

// 9. the k_marg variant: kept blocks of up to 48 dims (the one-wave factorisations) whose workspace fits 79 KB take 256
// threads, two work-groups per CU.  The workspace is the largest layout of any kept size up to the batch's (marg_lds_doubles):
// every work-group lays out for its own n, which the device may have shrunk
static int choose_marg(vpl_ctx* c, const Span<int>& mg_n, size_t W) {
  const DevBatch& B = c->B;
  int nmax = 0;
  for (size_t w = 0; w < W; ++w) nmax = std::max(nmax, mg_n[w]);
  c->marg_nmax = nmax;
  c->marg_small = nmax <= 48 && B.maxP <= 256 && B.maxL <= 256 &&
                  (size_t)marg_lds_doubles(nmax, true) * sizeof(double) <= MARG_LDS_SMALL && std::getenv("VPL_BA_MARG_BIG") == nullptr;
  c->marg_smem = (size_t)marg_lds_doubles(nmax, c->marg_small) * sizeof(double);
  if (c->marg_smem > MARG_LDS_MAX) return fail(c, VPL_E_CAPACITY, "marginalisation workspace exceeds LDS");
  return VPL_OK;
}

// the first max-over-the-batch rounds of every window's point work units, packed into the arena (rounds a window does not use
// travel too: idle lanes, empty slots)
static void pack_units(Stage& S, UploadArena& A, size_t W, int maxPR, const int* lane, const int* sub) {
  int rmax = 0;
  for (size_t w = 0; w < W; ++w) rmax = std::max(rmax, A.pu_cnt[w]);
  take_units(S, A, W, rmax);
  for (size_t w = 0; w < A.pu_lane.size(); ++w) {
    int* l = A.pu_lane[w].p;
    int* u = A.pu_sub[w].p;
    std::memcpy(l, lane + w * maxPR * 1024, (size_t)A.pu_cnt[w] * 4096);
    std::memcpy(u, sub + w * maxPR * 512, (size_t)A.pu_cnt[w] * 2048);
    std::fill(l + (size_t)A.pu_cnt[w] * 1024, l + (size_t)rmax * 1024, -1);
    std::fill(u + (size_t)A.pu_cnt[w] * 512, u + (size_t)rmax * 512, 0);
  }
}

// 10. chained upload: the values of the priors move device to device, before the upload's scatter overwrites mg_* with the
// next solve's tables
static int hand_over_priors(vpl_ctx* c, const std::vector<HostTab>& ctab, int prev_prS) {
  const DevBatch& B = c->B;
  const int nW = (int)ctab.size();
  std::vector<int> keep(nW);
  for (int w = 0; w < nW; ++w) keep[w] = ctab[w].keep ? 1 : 0;
  DevBuf dkeep;
  HIPCHK(c, dkeep.alloc(nW * 4));
  HIPCHK(c, hipMemcpyAsync(dkeep.p, keep.data(), nW * 4, hipMemcpyHostToDevice, c->stream));
  if (B.prS != prev_prS && std::any_of(keep.begin(), keep.end(), [](int k) { return k != 0; })) {
    // windows that keep their prior (MARGIN_SECOND_NEW pass-through) have J0 at the PREVIOUS batch stride: move them through
    // a scratch copy (old and new locations of different windows overlap) -- ADVICE r3
    DevBuf tmp;
    HIPCHK(c, tmp.alloc(nW * (size_t)MAXPN * MAXPN * 8));
    hipLaunchKernelGGL(k_prior_restride, dim3(nW), dim3(256), 0, c->stream, B, (const int*)dkeep.p, prev_prS, tmp.d(), 0);
    hipLaunchKernelGGL(k_prior_restride, dim3(nW), dim3(256), 0, c->stream, B, (const int*)dkeep.p, prev_prS, tmp.d(), 1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  hipLaunchKernelGGL(k_prior_handoff, dim3(nW), dim3(256), 0, c->stream, B, (const int*)dkeep.p);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VPL_OK;
}

static int upload_body(vpl_ctx* c, int nW, const vpl_window* win, const vpl_ba_options* opt, bool all_lines, bool chained,
                       const OdoSrc* odo) {
  int rc = upload_check(c, nW, win, opt, chained);
  if (rc) return rc;
  const int prev_prS = c->B.prS;
  c->prior_resident = false;
  (void)restore_event(c, RESTORE_EV_UPLOAD);   // (issues nothing: the snapshots a pending restore would copy are rewritten below)
  if (c->leg_timing) HIPCHK(c, hipEventRecord(c->leg_ev[0], c->stream));
  drop_graph(c);
  c->upload_open = true;   // from here on a refusal leaves the context with no batch (upload_impl)
  c->opt = *opt;
  c->nW = nW;
  DevBatch& B = c->B;
  B.nW = nW;
  B.opt.num_iterations = opt->num_iterations;
  B.opt.estimate_extrinsic = opt->estimate_extrinsic;
  B.opt.marginalization_flag = opt->marginalization_flag;
  B.opt.remove_line_outliers = opt->remove_line_outliers;
  B.opt.sqrt_info_point = opt->focal_length / 1.5;
  B.opt.sqrt_info_line = opt->line_factor;
  B.opt.sqrt_info_vp = opt->vp_factor;
  B.opt.g_norm = opt->g_norm;
  B.opt.huber_delta = opt->huber_delta;
  const size_t W = nW;
  std::vector<HostTab> ctab;
  if (chained && (rc = read_resident_priors(c, W, ctab))) return rc;
  // a session's prior is resident like a chained one, in the session's own buffer: its table is the host's copy, its values
  // are loaded behind the scatter
  const bool dev_prior = chained || odo;
  if (odo) {
    ctab.assign(W, HostTab());
    for (size_t w = 0; w < W; ++w)
      if (odo->tab && odo->has[w]) ctab[w] = odo->tab[w];
  }
  c->h_mg_m.assign(W, 0);
  c->maxPriorN = 0;
  c->h_passthrough.assign(W, -1);
  c->h_pass_priors.clear();
  c->any_second_new = false;
  c->h_nP.assign(W, 0);
  c->h_nL.assign(W, 0);
  c->h_lmap.resize(W);
  if ((rc = batch_strides(c, W, win, opt, dev_prior ? ctab.data() : nullptr))) return rc;
  const bool same_layout = layout_unchanged(c, W, win, all_lines);
  // every array that travels is packed straight into the context's pinned arena
  Stage& SG = c->stage;
  HIPCHK(c, SG.reserve(upload_bound(B, W, win, same_layout, dev_prior, odo)));
  UploadArena A;
  take_upload(SG, A, B, W, win, dev_prior, odo);
  // (plain heap, no value-initialisation: only the rounds a window uses are filled and packed into the arena)
  std::unique_ptr<int[]> lane(new int[W * B.maxPR * 1024]), sub(new int[W * B.maxPR * 512]);
  long schur_wide_w = 0, schur_total_w = 0;   // matrix-core weight of the wide entries / of all entries of k_schur's table
  for (size_t w = 0; w < W; ++w) {
    const HostTab* T = dev_prior ? &ctab[w] : nullptr;
    if ((rc = pack_tracks(c, A, w, win[w], all_lines))) return rc;
    if (odo) pack_gather(c, A, w, win[w], *odo);
    else pack_values(c, A, w, win[w]);
    if (!same_layout &&
        (rc = build_layout(c, A, w, win[w], &lane[w * B.maxPR * 1024], &sub[w * B.maxPR * 512], &schur_wide_w, &schur_total_w)))
      return rc;
    if ((rc = pack_prior(c, A, w, win[w], T))) return rc;
    if ((rc = keep_blocks(c, A, w, win[w], T))) return rc;
  }
  if ((rc = choose_marg(c, A.mg_n, W))) return rc;
  if (!same_layout) pack_units(SG, A, W, B.maxPR, lane.get(), sub.get());
  std::memcpy(A.mg_m.p, c->h_mg_m.data(), W * 4);
  c->h_mg_n.assign(A.mg_n.begin(), A.mg_n.end());
  c->h_mg_nb.assign(A.mg_nb.begin(), A.mg_nb.end());
  if (odo)
    for (size_t w = 0; w < W; ++w)
      A.odo_marg[w] = (opt->marginalization_flag != VPL_MARGIN_NONE && c->h_passthrough[w] < 0) ? 1 + A.mg_nb[w] : 0;
  // k_schur_mixed pays five passes over the rows of a wide entry: measured (tools/bench_tracks.py, 512 windows) 0.52 ms per step
  // with a tenth of the point tracks long, 3.2 ms with every track long, against 1.5 - 1.65 ms of k_schur<5> either way
  if (!same_layout) c->schur_mostly_wide = schur_total_w > 0 && 20 * schur_wide_w > 7 * schur_total_w;
  if (c->force_general) std::fill(A.path.begin(), A.path.end(), 1);
  // k_lin writes the entries of Hcc outside the fast path's pattern only for windows of the general path; a batch that had
  // one may have left values there, in slots whose next windows count on zeros (ba_ctx.h).  On the stream, in front of the
  // scatter and so of the first linearisation of the new batch.
  if (c->hcc_general) HIPCHK(c, hipMemsetAsync(B.Hcc, 0, (size_t)c->maxW * NCP * sizeof(double), c->stream));
  c->hcc_general = std::any_of(A.path.begin(), A.path.end(), [](int p) { return p != 0; });
  if (SG.overflow) return fail(c, VPL_E_CAPACITY, "internal: staging arena bound too small");
  stage_upload(SG, A, B, W, same_layout, dev_prior, odo);
  if (chained && (rc = hand_over_priors(c, ctab, prev_prS))) return rc;
  // ONE host-to-device copy of the arena, ONE kernel that scatters its pieces into the batch's arrays
  HIPCHK(c, stage_run(c->stage, c->stream, true, &c->last_upload_bytes));
  if (odo) {   // the doubles of the batch: from the session's store and prior, behind the tables they are indexed by
    hipLaunchKernelGGL(k_odo_gather, dim3(nW), dim3(ODO_THREADS), 0, c->stream, B, odo->store, (const int*)odo->d_psrc, (const int*)odo->d_lsrc);
    if (odo->tab) hipLaunchKernelGGL(k_odo_prior_load, dim3(nW), dim3(ODO_THREADS), 0, c->stream, B, odo->prior, (const int*)odo->d_has);
    HIPCHK(c, hipGetLastError());
  }
  if (c->leg_timing) HIPCHK(c, hipEventRecord(c->leg_ev[1], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the arena is free for the next call from here on
  c->layout_valid = true;
  return VPL_OK;
}
// An upload that is refused half way (a track outside the window in the third window, a prior of impossible size) has already
// rewritten part of the batch's host tables and its size: the context then holds NO batch -- solve / download / reset return
// VPL_E_INVALID until the next successful upload -- instead of running the new size on the old device data.  A refusal before
// anything was touched (too many windows, unknown flag, no resident prior for a chained upload) leaves the previous batch as it was.
static int upload_impl(vpl_ctx* c, int nW, const vpl_window* win, const vpl_ba_options* opt, bool all_lines, bool chained = false,
                       const OdoSrc* odo = nullptr) {
  const int rc = upload_body(c, nW, win, opt, all_lines, chained, odo);
  if (c) {
    if (rc != VPL_OK && c->upload_open) { c->nW = 0; c->prior_resident = false; }
    c->upload_open = false;
  }
  return rc;
}
