// The keyframe session (vpl_odo_* of include/vplines_ba.h); vplines_ba.hip includes this once, behind the window entry points
// whose stages it runs.
// The reference's FeatureManager + window state for n_seq sequences, resident on the device (csrc/ba_odo.h); the host keeps
// the integer side of the tracks (csrc/odo_tracks.h), from which the existing host code builds the kernels' layout tables.
// A keyframe runs the stages of vpl_ba_solve_odometry -- the same uploads of tables, the same launches -- with every double
// of the batch gathered from the store instead of packed from the caller's arrays, and the results scattered back into it.
#pragma once
#include "ba_upload.h"
#include "odo_tracks.h"

struct OdoSeq {
  OdoBook P, L;
  double sum_dt[NF] = {};          // of the 11 pre-integrations (the kept-block table asks for preint[1].sum_dt)
  HostTab prior;                   // block table of the prior the session holds on the device
  bool has_prior = false, set = false;
  bool imu_set = false;            // vpl_odo_set_imu since the last vpl_odo_set_window (IMU-enabled sessions)
  // the keyframe decision of the window as it stands (vpl_odo_enable_keyframe_rule) and the failure check's memory
  OdoParallaxRec dec = {};
  bool dec_set = false;
  double last_pose[7] = {};        // Estimator::last_P (failureDetection): pose[9] of vpl_odo_set_window, then pose[10] of every solve
  int failure = 0;                 // VPL_FAIL_* of the last solve, default limits
  SelBook sel_book;                // vpl_odo_select: the selector's id book, from the session's creation on
};

// What vpl_odo_solve's last copy left in h_out behind the results, for vpl_odo_advance to read: offsets in ints of the three
// sections -- one flag per solved point | 2 + 3 * (blocks) ints of prior table per marginalised sequence | one flag per solved
// line (with remove_line_outliers) -- and how many points and lines each sequence solved
struct OdoOutbox {
  size_t point_flags = 0, prior_tabs = 0, line_flags = 0, end = 0;
  std::vector<int> nP, nL;
};

struct vpl_odo {
  vpl_ctx* c = nullptr;
  int nS = 0, line_min_obs = 0, maxPT = 0, maxLT = 0;
  vpl_ba_options opt;
  double init_depth = 5.0;
  OdoStore st[2];
  int cur = 0;
  OdoPrior prior;
  int *d_psrc = nullptr, *d_lsrc = nullptr, *d_has = nullptr, *d_marg = nullptr;
  char *d_in = nullptr, *h_in = nullptr, *d_out = nullptr, *h_out = nullptr;   // new frames + slide tables in | results + flags out (h_*: pinned)
  size_t in_cap = 0, out_cap = 0;  // (every device array is recorded in the context with the session as its owner: vpl_odo_destroy)
  // vpl_odo_enable_imu: the IMU side (two, swapped with the stores)
  bool imu = false;
  int max_samples = 0;
  OdoImu im[2] = {};
  // vpl_odo_enable_keyframe_rule: thresholds
  bool rule = false;
  vpl_odo_keyframe_rule kf_rule = {};
  std::vector<OdoSeq> seq;
  // the integer-only windows handed to the uploads, and what they point to
  std::vector<vpl_window> win;
  std::vector<std::vector<int>> pstart, pnobs, lstart, lnobs, ltri, psrc, lsrc;
  std::vector<HostTab> tabs;
  std::vector<unsigned char> has;
  long long h2d_payload = 0, h2d_table = 0, d2h = 0;
  double ms[4] = {0, 0, 0, 0};
  // between vpl_odo_solve and vpl_odo_advance: what the solve decided (its flags are in h_out) and on which batch
  bool solved = false;
  int flag = VPL_MARGIN_OLD, remove_line_outliers = 0;
  OdoOutbox box;
  std::vector<std::vector<int>> s_lmap;
};

// the outbox: nS results, then ints (flags of the stages; after the solve's last copy the three sections of OdoOutbox)
struct OdoOutViews {
  vpl_odo_result *d_res, *h_res;
  int *d_flags, *h_flags;
};
static OdoOutViews odo_out_views(const vpl_odo* o) {
  const size_t res = (size_t)o->nS * sizeof(vpl_odo_result);
  return OdoOutViews{reinterpret_cast<vpl_odo_result*>(o->d_out), reinterpret_cast<vpl_odo_result*>(o->h_out),
                     reinterpret_cast<int*>(o->d_out + res), reinterpret_cast<int*>(o->h_out + res)};
}

// Bytes of the inbox, the one place that knows them.  Per sequence: the doubles of a new frame -- pose + speed/bias +
// pre-integration or, when they are more, max_samples rows of 7, then one observation per track -- and the ints of the tables:
// header and two counts, one entry per observation and per track (the slide's moves), with the keyframe rule its header and one
// entry per point track.  odo_check_next bounds a frame's observations and samples by the same capacities.
static size_t odo_inbox_bytes(size_t nS, size_t maxPT, size_t maxLT, size_t max_samples, bool rule) {
  const size_t head = std::max<size_t>(16 + ODO_RAW_PRE_D, 7 * max_samples);
  return nS * (8 * (head + 3 * maxPT + 8 * maxLT) + 4 * (ODO_HDR + 2 + 2 * (maxPT + maxLT)) + (rule ? 4 * (ODO_PAR_HDR + maxPT) : 0)) + 64;
}

// The inbox for max_samples and the rule on or off: a new device and a new pinned buffer are swapped in and both old ones freed
// at once; nothing is done when the size stays.  On failure what was got is released and the session is as it was.  The stream
// is idle (odo_quiesce).
static int odo_resize_inbox(vpl_odo* o, int max_samples, bool rule) {
  vpl_ctx* c = o->c;
  const size_t cap = odo_inbox_bytes(o->nS, o->maxPT, o->maxLT, max_samples, rule);
  if (cap == o->in_cap) return VPL_OK;
  char *din = nullptr, *hin = nullptr;
  hipError_t e = dalloc(c, &din, cap, o);
  if (e == hipSuccess) e = hipHostMalloc((void**)&hin, cap, hipHostMallocDefault);
  if (e != hipSuccess) { dfree(c, din); return VPL_E_HIP; }
  dfree(c, o->d_in);
  if (o->h_in) (void)hipHostFree(o->h_in);
  o->d_in = din; o->h_in = hin; o->in_cap = cap;
  return VPL_OK;
}

// every entry point off the keyframe path starts here: the device, the asynchronous call that is still pending, an idle stream
static int odo_quiesce(vpl_odo* o) {
  vpl_ctx* c = o->c;
  HIPCHK(c, hipSetDevice(c->device));
  { const int rs = settle(c); if (rs) return rs; }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VPL_OK;
}

static int odo_alloc_store(vpl_odo* o, OdoStore& S, size_t nS, int maxPT, int maxLT) {
  vpl_ctx* c = o->c;
  hipError_t e = hipSuccess;
  S.maxPT = maxPT; S.maxLT = maxLT;
#define OAL(ptr, n) if (e == hipSuccess) e = dalloc(c, &S.ptr, (size_t)(n), o)
  OAL(pobs, nS * maxPT * NF * 3); OAL(lobs, nS * maxLT * NF * 8); OAL(invd, nS * maxPT); OAL(plk, nS * maxLT * 6); OAL(tri, nS * maxLT);
  OAL(pose, nS * 77); OAL(sb, nS * 99); OAL(ex, nS * 7); OAL(pre, nS * NF);
#undef OAL
  return e == hipSuccess ? VPL_OK : VPL_E_HIP;
}

static OdoSrc odo_src(vpl_odo* o, bool with_prior) {
  OdoSrc s;
  s.store = o->st[o->cur];
  s.prior = o->prior;
  s.d_psrc = o->d_psrc; s.d_lsrc = o->d_lsrc; s.d_has = o->d_has; s.d_marg = o->d_marg;
  s.psrc = o->psrc.data(); s.lsrc = o->lsrc.data();
  s.tab = with_prior ? o->tabs.data() : nullptr;
  s.has = o->has.data();
  return s;
}

// the tracks the solve takes (estimator.cpp:1100-1102, 1132-1133) as integer-only windows; lines with their flags
static void odo_select(vpl_odo* o) {
  for (int w = 0; w < o->nS; ++w) {
    OdoSeq& q = o->seq[w];
    auto &ps = o->pstart[w], &pn = o->pnobs[w], &px = o->psrc[w], &ls = o->lstart[w], &ln = o->lnobs[w], &lt = o->ltri[w], &lx = o->lsrc[w];
    ps.clear(); pn.clear(); px.clear(); ls.clear(); ln.clear(); lt.clear(); lx.clear();
    for (size_t i = 0; i < q.P.t.size(); ++i) {
      const OdoTrack& t = q.P.t[i];
      if (t.nobs >= 2 && t.start < NF - 3) { ps.push_back(t.start); pn.push_back(t.nobs); px.push_back((int)i); }
    }
    for (size_t i = 0; i < q.L.t.size(); ++i) {
      const OdoTrack& t = q.L.t[i];
      if (t.nobs >= o->line_min_obs && t.start < NF - 3) { ls.push_back(t.start); ln.push_back(t.nobs); lt.push_back(t.tri); lx.push_back((int)i); }
    }
    vpl_window& v = o->win[w];
    v.n_points = (int)ps.size(); v.point_start = ps.data(); v.point_nobs = pn.data();
    v.n_lines = (int)ls.size(); v.line_start = ls.data(); v.line_nobs = ln.data(); v.line_triangulated = lt.data();
    v.preint[1].sum_dt = q.sum_dt[1];
    o->tabs[w] = q.prior;
    o->has[w] = q.has_prior ? 1 : 0;
  }
}

// the observations of one image, whichever frame struct carries them
struct OdoObs {
  int n_points; const int* point_id; const double* point_obs;
  int n_lines; const int* line_id; const double* line_obs;
};
static OdoObs odo_obs(const vpl_odo_frame& f) { return OdoObs{f.n_points, f.point_id, f.point_obs, f.n_lines, f.line_id, f.line_obs}; }
static OdoObs odo_obs(const vpl_odo_imu_frame& f) { return OdoObs{f.n_points, f.point_id, f.point_obs, f.n_lines, f.line_id, f.line_obs}; }
static int odo_check_frame(const OdoObs& f) {
  if (f.n_points < 0 || f.n_lines < 0) return VPL_E_INVALID;
  if (f.n_points > 0 && (!f.point_id || !f.point_obs)) return VPL_E_INVALID;
  if (f.n_lines > 0 && (!f.line_id || !f.line_obs)) return VPL_E_INVALID;
  return VPL_OK;
}
// The new frames of one call.  What enters slot 10 beside the observations is chosen HERE and nowhere else: the caller's state
// and finished pre-integration (vpl_odo_advance), or raw samples the device integrates and propagates (vpl_odo_advance_imu).
struct OdoNext {
  const vpl_odo_frame* plain = nullptr;
  const vpl_odo_imu_frame* imu = nullptr;
  OdoObs obs(int w) const { return plain ? odo_obs(plain[w]) : odo_obs(imu[w]); }
  int n_samples(int w) const { return plain ? -1 : imu[w].n_samples; }                 // hdr[5] of k_odo_append
  size_t head(int w) const { return plain ? 16 + ODO_RAW_PRE_D : 7 * (size_t)imu[w].n_samples; }   // doubles before the observations
  void write_head(int w, double* d) const {
    if (plain) { std::memcpy(d, plain[w].pose, 56); std::memcpy(d + 7, plain[w].speed_bias, 72); std::memcpy(d + 16, &plain[w].preint, sizeof(plain[w].preint)); }
    else std::memcpy(d, imu[w].samples, 56 * (size_t)imu[w].n_samples);
  }
};

// ---- the keyframe rule (vpl_odo_enable_keyframe_rule) ------------------------------------------------------------------------
// k_odo_parallax's tables for sequences seq0 .. seq0 + n - 1 at dst, which lies tab_off ints into the table the kernel is given:
// par [n][3], then the lists (odo_parallax_list).  Returns the ints written -- at most n * (3 + max_point_tracks), the room
// vpl_odo_enable_keyframe_rule adds to the inbox.
static size_t odo_write_parallax_tab(vpl_odo* o, int seq0, int n, int* dst, size_t tab_off) {
  size_t k = (size_t)ODO_PAR_HDR * n;
  for (int b = 0; b < n; ++b) {
    int* h = dst + ODO_PAR_HDR * b;
    h[0] = (int)(tab_off + k);
    h[1] = odo_parallax_list(o->seq[seq0 + b].P, dst + k, &h[2]);
    k += h[1];
  }
  return k;
}
static void odo_read_decisions(vpl_odo* o, int seq0, int n, const char* recs) {
  for (int b = 0; b < n; ++b) {
    OdoSeq& q = o->seq[seq0 + b];
    std::memcpy(&q.dec, recs + sizeof(OdoParallaxRec) * b, sizeof(OdoParallaxRec));
    q.dec_set = q.set;
  }
}
// the decision of sequences that already hold a window (vpl_odo_set_window, vpl_odo_enable_keyframe_rule): tables down, one
// launch, records back, synchronous; not on the per-keyframe path and not counted in vpl_odo_stats.  The caller has set the device
// and is not between vpl_odo_solve and vpl_odo_advance (the flags of a solve wait in h_out).
static int odo_decide(vpl_odo* o, int seq0, int n) {
  vpl_ctx* c = o->c;
  hipStream_t s = c->stream;
  const size_t nt = odo_write_parallax_tab(o, seq0, n, reinterpret_cast<int*>(o->h_in), 0);
  HIPCHK(c, hipMemcpyAsync(o->d_in, o->h_in, nt * 4, hipMemcpyHostToDevice, s));
  const int* d_tab = reinterpret_cast<const int*>(o->d_in);
  hipLaunchKernelGGL(k_odo_parallax, dim3(n), dim3(ODO_THREADS), 0, s, o->st[o->cur], d_tab, d_tab, seq0, o->kf_rule.min_parallax,
                     o->kf_rule.min_track_num, reinterpret_cast<OdoParallaxRec*>(o->d_out));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(o->h_out, o->d_out, (size_t)n * sizeof(OdoParallaxRec), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  odo_read_decisions(o, seq0, n, o->h_out);
  return VPL_OK;
}

// the books of a window's eleven frames, built on copies (a refusal leaves the sequence as it was); pd / ld: per frame and
// observation, its place in the store (track | frame << 20, -1 = ignored)
static int odo_build_books(vpl_odo* o, const vpl_odo_frame* frames, OdoBook& P, OdoBook& L, std::vector<std::vector<int>>& pd,
                           std::vector<std::vector<int>>& ld, const char* who) {
  vpl_ctx* c = o->c;
  pd.assign(NF, std::vector<int>()); ld.assign(NF, std::vector<int>());
  for (int f = 0; f < NF; ++f) {
    if ((int)P.t.size() + odo_count_unknown(P, frames[f].n_points, frames[f].point_id) > o->maxPT ||
        (int)L.t.size() + odo_count_unknown(L, frames[f].n_lines, frames[f].line_id) > o->maxLT)
      return fail(c, VPL_E_CAPACITY, std::string(who) + ": more tracks than the session's capacity");
    pd[f].resize(frames[f].n_points); ld[f].resize(frames[f].n_lines);
    odo_add_frame(P, f, frames[f].n_points, frames[f].point_id, pd[f].data());
    odo_add_frame(L, f, frames[f].n_lines, frames[f].line_id, ld[f].data());
  }
  return VPL_OK;
}
// an image of the sequence's tracks in the store, copied array by array (not on the per-keyframe path): the observations, every
// depth unset, no line triangulated
static int odo_upload_tracks(vpl_odo* o, int seq, const OdoBook& P, const OdoBook& L, const std::vector<std::vector<int>>& pd,
                             const std::vector<std::vector<int>>& ld, const vpl_odo_frame* frames) {
  vpl_ctx* c = o->c;
  const OdoStore& S = o->st[o->cur];
  const size_t nP = P.t.size(), nL = L.t.size();
  std::vector<double> pobs(std::max<size_t>(nP, 1) * NF * 3, 0.0), lobs(std::max<size_t>(nL, 1) * NF * 8, 0.0), invd(std::max<size_t>(nP, 1), -1.0),
      plk(std::max<size_t>(nL, 1) * 6, 0.0);
  std::vector<int> tri(std::max<size_t>(nL, 1), 0);
  for (int f = 0; f < NF; ++f) {
    for (int i = 0; i < frames[f].n_points; ++i) {
      const int e = pd[f][i];
      if (e >= 0) std::memcpy(&pobs[((size_t)(e & 0xFFFFF) * NF + (e >> 20 & 15)) * 3], frames[f].point_obs + 3 * (size_t)i, 24);
    }
    for (int i = 0; i < frames[f].n_lines; ++i) {
      const int e = ld[f][i];
      if (e >= 0) std::memcpy(&lobs[((size_t)(e & 0xFFFFF) * NF + (e >> 20 & 15)) * 8], frames[f].line_obs + 8 * (size_t)i, 64);
    }
  }
  const size_t q = seq;
  HIPCHK(c, hipMemcpy(S.pobs + q * S.maxPT * NF * 3, pobs.data(), nP * NF * 3 * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(S.lobs + q * S.maxLT * NF * 8, lobs.data(), nL * NF * 8 * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(S.invd + q * S.maxPT, invd.data(), nP * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(S.plk + q * S.maxLT * 6, plk.data(), nL * 6 * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(S.tri + q * S.maxLT, tri.data(), nL * 4, hipMemcpyHostToDevice));
  return VPL_OK;
}

extern "C" {

int vpl_odo_create(vpl_odo** out, vpl_ctx* c, int n_seq, const vpl_ba_options* opt, double init_depth, int line_min_obs,
                   int max_point_tracks, int max_line_tracks) {
  if (!out || !c || !opt || n_seq < 1 || !(init_depth > 0.0) || line_min_obs < 1 || max_point_tracks < 1 || max_line_tracks < 1)
    return VPL_E_INVALID;
  if (max_point_tracks >= (1 << 20) || max_line_tracks >= (1 << 20)) return fail(c, VPL_E_CAPACITY, "odo: at most 2^20 - 1 tracks per sequence");
  if (c->odo) return fail(c, VPL_E_INVALID, "odo: the context already lends itself to a session");
  if (n_seq > c->maxW) return fail(c, VPL_E_CAPACITY, "odo: more sequences than the context's max_windows");
  vpl_odo* o = new vpl_odo();
  o->c = c; o->nS = n_seq; o->opt = *opt; o->init_depth = init_depth; o->line_min_obs = line_min_obs;
  o->maxPT = max_point_tracks; o->maxLT = max_line_tracks;
  { const int rq = odo_quiesce(o); if (rq) { delete o; return rq; } }
  const size_t nS = n_seq;
  int rc = odo_alloc_store(o, o->st[0], nS, o->maxPT, o->maxLT);
  if (!rc) rc = odo_alloc_store(o, o->st[1], nS, o->maxPT, o->maxLT);
  hipError_t e = hipSuccess;
  // out, per sequence: the result, three flags per track, the prior's block table (in: odo_inbox_bytes)
  o->out_cap = nS * (sizeof(vpl_odo_result) + 4 * (3 * ((size_t)o->maxPT + o->maxLT) + 2 + 3 * MAXPB));
  if (!rc) {
    if (e == hipSuccess) e = dalloc(c, &o->prior.J0, nS * MAXKEEP * MAXKEEP, o);
    if (e == hipSuccess) e = dalloc(c, &o->prior.r0, nS * MAXKEEP, o);
    if (e == hipSuccess) e = dalloc(c, &o->prior.x0, nS * MAXPB * 9, o);
    if (e == hipSuccess) e = dalloc(c, &o->d_psrc, nS * c->B.maxP, o);
    if (e == hipSuccess) e = dalloc(c, &o->d_lsrc, nS * c->B.maxL, o);
    if (e == hipSuccess) e = dalloc(c, &o->d_has, nS, o);
    if (e == hipSuccess) e = dalloc(c, &o->d_marg, nS, o);
    if (e == hipSuccess) e = dalloc(c, &o->d_out, o->out_cap, o);
    if (e == hipSuccess) e = hipHostMalloc((void**)&o->h_out, o->out_cap, hipHostMallocDefault);
    if (e == hipSuccess && odo_resize_inbox(o, 0, false)) e = hipErrorOutOfMemory;
  }
  if (rc || e != hipSuccess) {
    c->odo = o;              // (so that destroy releases through the one path)
    vpl_odo_destroy(o);
    return rc ? rc : fail(c, VPL_E_HIP, "odo: device allocation failed");
  }
  o->seq.resize(nS);
  o->win.resize(nS);
  for (auto& v : o->win) std::memset(&v, 0, sizeof(v));
  o->pstart.resize(nS); o->pnobs.resize(nS); o->lstart.resize(nS); o->lnobs.resize(nS); o->ltri.resize(nS); o->psrc.resize(nS); o->lsrc.resize(nS);
  o->tabs.resize(nS); o->has.assign(nS, 0);
  c->odo = o;
  *out = o;
  return VPL_OK;
}

void vpl_odo_destroy(vpl_odo* o) {
  if (!o) return;
  vpl_ctx* c = o->c;
  (void)odo_quiesce(o);   // (teardown: a failure has nobody to be reported to)
  dfree_owner(c, o);
  if (o->h_in) (void)hipHostFree(o->h_in);
  if (o->h_out) (void)hipHostFree(o->h_out);
  if (c->odo == o) c->odo = nullptr;
  delete o;
}

int vpl_odo_set_window(vpl_odo* o, int seq, const double pose[][7], const double speed_bias[][9], const double ex_pose[7],
                       const vpl_preintegration* preint, const vpl_odo_frame* frames) {
  if (!o || seq < 0 || seq >= o->nS || !pose || !speed_bias || !ex_pose || !preint || !frames) return VPL_E_INVALID;
  vpl_ctx* c = o->c;
  for (int f = 0; f < NF; ++f)
    if (odo_check_frame(odo_obs(frames[f]))) return fail(c, VPL_E_INVALID, "odo_set_window: null observation array");
  // the bookkeeping on a copy: a refusal leaves the sequence as it was
  OdoBook P, L;
  std::vector<std::vector<int>> pd, ld;
  { const int rb = odo_build_books(o, frames, P, L, pd, ld, "odo_set_window"); if (rb) return rb; }
  { const int rq = odo_quiesce(o); if (rq) return rq; }
  const OdoStore& S = o->st[o->cur];
  { const int ru = odo_upload_tracks(o, seq, P, L, pd, ld, frames); if (ru) return ru; }
  std::vector<DevPreint> pre(NF);
  std::memset(pre.data(), 0, sizeof(DevPreint) * NF);
  for (int f = 1; f < NF; ++f) to_dev_preint(preint[f], pre[f]);
  const size_t q = seq;
  HIPCHK(c, hipMemcpy(S.pose + q * 77, pose, 77 * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(S.sb + q * 99, speed_bias, 99 * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(S.ex + q * 7, ex_pose, 7 * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(S.pre + q * NF, pre.data(), sizeof(DevPreint) * NF, hipMemcpyHostToDevice));
  OdoSeq& Q = o->seq[seq];
  Q.P = std::move(P); Q.L = std::move(L);
  Q.sum_dt[0] = 0.0;
  for (int f = 1; f < NF; ++f) Q.sum_dt[f] = preint[f].sum_dt;
  Q.prior = HostTab();
  Q.has_prior = false;
  Q.set = true;
  Q.imu_set = false;
  std::memcpy(Q.last_pose, pose[NF - 2], 56);
  Q.failure = 0;
  Q.dec_set = false;
  o->solved = false;
  return o->rule ? odo_decide(o, seq, 1) : VPL_OK;
}

// the refusals of a new frame: null arrays, more tracks than the session holds (counted on the book as it stands)
// ... and on the IMU form: the session's mode, a sequence without its IMU side, the sample arrays
static int odo_check_next(vpl_odo* o, const OdoNext& next) {
  vpl_ctx* c = o->c;
  if (o->imu != (next.imu != nullptr))
    return fail(c, VPL_E_INVALID, o->imu ? "odo: the session takes IMU samples (vpl_odo_advance_imu / vpl_odo_keyframe_imu)"
                                         : "odo: the session does not take IMU samples (vpl_odo_enable_imu)");
  for (int w = 0; w < o->nS; ++w) {
    const OdoObs f = next.obs(w);
    if (odo_check_frame(f)) return fail(c, VPL_E_INVALID, "odo: null observation array");
    if (next.imu) {
      if (!o->seq[w].imu_set) return fail(c, VPL_E_INVALID, "odo: a sequence has no IMU side (vpl_odo_set_imu after vpl_odo_set_window)");
      if (!next.imu[w].samples || next.imu[w].n_samples < 1) return fail(c, VPL_E_INVALID, "odo: an interval needs at least one IMU sample");
      if (next.imu[w].n_samples > o->max_samples) return fail(c, VPL_E_CAPACITY, "odo: more IMU samples in an interval than max_samples");
    }
    // (the inbox holds one observation per track and frame)
    if (f.n_points > o->maxPT || f.n_lines > o->maxLT) return fail(c, VPL_E_CAPACITY, "odo: more observations in a frame than tracks in the session");
    const OdoSeq& q = o->seq[w];
    if ((int)q.P.t.size() + odo_count_unknown(q.P, f.n_points, f.point_id) > o->maxPT ||
        (int)q.L.t.size() + odo_count_unknown(q.L, f.n_lines, f.line_id) > o->maxLT)
      return fail(c, VPL_E_CAPACITY, "odo: more tracks than the session's capacity");
  }
  return VPL_OK;
}

int vpl_odo_solve(vpl_odo* o, const int* flags, vpl_odo_result* out) {
  if (!o || !flags || !out) return VPL_E_INVALID;
  vpl_ctx* c = o->c;
  const int nS = o->nS;
  const int flag = flags[0];
  if (flag != VPL_MARGIN_OLD && flag != VPL_MARGIN_SECOND_NEW) return fail(c, VPL_E_INVALID, "odo_solve: marginalization_flag");
  if (o->solved) return fail(c, VPL_E_INVALID, "odo_solve: the window has been solved and not advanced (vpl_odo_advance)");
  for (int w = 0; w < nS; ++w) {
    if (flags[w] != flag) return fail(c, VPL_E_INVALID, "odo_solve: the sequences of one call must carry the same marginalization_flag");
    if (!o->seq[w].set) return fail(c, VPL_E_INVALID, "odo_solve: a sequence has no window (vpl_odo_set_window)");
  }
  if (c->maxL > LOPT_THREADS) return fail(c, VPL_E_CAPACITY, "onlyLineOpt handles at most 256 lines per window");
  // capacities, before anything is touched
  odo_select(o);
  const DevBatch& B = c->B;
  bool any_lines = false;
  for (int w = 0; w < nS; ++w) {
    long po = 0, lo = 0;
    for (int n : o->pnobs[w]) po += n;
    for (int n : o->lnobs[w]) lo += n;
    if ((int)o->pstart[w].size() > B.maxP || (int)o->lstart[w].size() > B.maxL || po > B.maxPO || lo > B.maxLO)
      return fail(c, VPL_E_CAPACITY, "odo_solve: the solve's tracks exceed the context's capacities");
    any_lines = any_lines || !o->lstart[w].empty();
  }
  HIPCHK(c, hipSetDevice(c->device));
  { const int rs = settle(c); if (rs) return rs; }
  using oclk = std::chrono::steady_clock;
  auto t0 = oclk::now();
  auto lap = [&](int k) { const auto t = oclk::now(); o->ms[k] = std::chrono::duration<double, std::milli>(t - t0).count(); t0 = t; };
  hipStream_t s = c->stream;
  const dim3 grid(nS), blk(ODO_THREADS);
  const OdoStore S = o->st[o->cur];
  const OdoOutViews V = odo_out_views(o);
  vpl_odo_result* const d_res = V.d_res;
  int* const d_flags = V.d_flags;
  const int* const h_flags = V.h_flags;
  o->h2d_payload = o->h2d_table = o->d2h = 0;
  vpl_ba_options solve_opt = o->opt;
  solve_opt.marginalization_flag = flag;
  int rc;

  // 1. f_manager.triangulate || f_manager.triangulateLine: every selected point, every selected line with its flag
  {
    vpl_ba_options topt;
    vpl_ba_default_options(&topt);
    topt.marginalization_flag = VPL_MARGIN_NONE;
    const OdoSrc src = odo_src(o, false);
    if ((rc = upload_impl(c, nS, o->win.data(), &topt, true, false, &src))) return rc;
    o->h2d_table += (long long)c->last_upload_bytes;
    launch_triangulate(c, nS, true, any_lines, o->init_depth);
    hipLaunchKernelGGL(k_odo_scatter_tri, grid, blk, 0, s, c->B, S, (const int*)o->d_psrc, (const int*)o->d_lsrc, d_flags);
    HIPCHK(c, hipGetLastError());
    if (any_lines) {
      size_t nl = 0;
      for (int w = 0; w < nS; ++w) nl += o->lstart[w].size();
      HIPCHK(c, hipMemcpyAsync(V.h_flags, d_flags, nl * 4, hipMemcpyDeviceToHost, s));
      o->d2h += (long long)nl * 4;
      HIPCHK(c, hipStreamSynchronize(s));
      size_t k = 0;
      for (int w = 0; w < nS; ++w)
        for (size_t l = 0; l < o->lstart[w].size(); ++l, ++k) {
          o->ltri[w][l] = h_flags[k];
          o->seq[w].L.t[o->lsrc[w][l]].tri = h_flags[k];
        }
    }
  }
  lap(0);

  // 2. onlyLineOpt on the triangulated lines, uploaded with the solve's options (the batch stays for the solve when no line is erased)
  bool batch_resident = false;
  std::vector<int> lrem1(nS, 0);
  if (any_lines) {
    const OdoSrc src = odo_src(o, true);
    if ((rc = upload_impl(c, nS, o->win.data(), &solve_opt, false, false, &src))) return rc;
    o->h2d_table += (long long)c->last_upload_bytes;
    launch_line_opt(c, nS);
    hipLaunchKernelGGL(k_odo_scatter_lopt, grid, blk, 0, s, c->B, S, (const int*)o->d_lsrc, d_flags, d_res);
    HIPCHK(c, hipGetLastError());
    size_t nl = 0;
    for (int w = 0; w < nS; ++w) nl += c->h_nL[w];
    if (nl) HIPCHK(c, hipMemcpyAsync(V.h_flags, d_flags, nl * 4, hipMemcpyDeviceToHost, s));
    o->d2h += (long long)nl * 4;
    HIPCHK(c, hipStreamSynchronize(s));
    bool erased = false;
    size_t k = 0;
    for (int w = 0; w < nS; ++w)
      for (int dl = 0; dl < c->h_nL[w]; ++dl, ++k)
        if (h_flags[k]) {   // f_manager.removeLineOutlier erased the track's line (estimator.cpp:1037): it takes no part in the solve
          const int l = c->h_lmap[w][dl];
          o->ltri[w][l] = 0;
          o->seq[w].L.t[o->lsrc[w][l]].tri = 0;
          ++lrem1[w];
          erased = true;
        }
    batch_resident = !erased;
  }
  lap(1);

  // 3. optimizationwithLine: on the batch where it lies, or on a fresh upload of the lines that are left
  if (batch_resident) {
    if ((rc = reuse_line_opt_batch(c))) return rc;
  } else {
    const OdoSrc src = odo_src(o, true);
    if ((rc = upload_impl(c, nS, o->win.data(), &solve_opt, false, false, &src))) return rc;
    o->h2d_table += (long long)c->last_upload_bytes;
  }
  if ((rc = vpl_ba_solve(c))) return rc;
  c->prior_resident = false;   // (the session keeps the prior in its own buffer; the batch is rewritten before the next solve)
  hipLaunchKernelGGL(k_odo_scatter_solve, grid, blk, 0, s, c->B, S, (const int*)o->d_psrc, (const int*)o->d_lsrc, d_flags, d_res,
                     o->prior, (const int*)o->d_marg);
  HIPCHK(c, hipGetLastError());
  // what k_odo_scatter_solve wrote behind the results: the layout, here and nowhere else
  OdoOutbox& box = o->box;
  box.nP = c->h_nP; box.nL = c->h_nL;
  std::vector<int> marg(nS, 0);
  {
    size_t totP = 0, totT = 0, totL = 0;
    for (int w = 0; w < nS; ++w) {
      totP += c->h_nP[w]; totL += c->h_nL[w];
      marg[w] = c->h_passthrough[w] < 0 ? 1 + c->h_mg_nb[w] : 0;
      totT += marg[w] ? 2 + 3 * (marg[w] - 1) : 0;
    }
    box.point_flags = 0; box.prior_tabs = totP; box.line_flags = totP + totT;
    box.end = box.line_flags + (solve_opt.remove_line_outliers ? totL : 0);
    const size_t bytes = (size_t)nS * sizeof(vpl_odo_result) + 4 * box.end;
    HIPCHK(c, hipMemcpyAsync(o->h_out, o->d_out, bytes, hipMemcpyDeviceToHost, s));
    o->d2h += (long long)bytes;
    HIPCHK(c, hipStreamSynchronize(s));
  }
  lap(2);

  // the results, and the prior the marginalisation left: its block table (the values stayed on the device)
  o->s_lmap = c->h_lmap;
  o->flag = flag; o->remove_line_outliers = solve_opt.remove_line_outliers;
  size_t kT = 0, kL = 0;
  for (int w = 0; w < nS; ++w) {
    OdoSeq& q = o->seq[w];
    vpl_odo_result& r = out[w];
    r = V.h_res[w];
    if (o->lstart[w].empty()) std::memset(&r.line_report, 0, sizeof(r.line_report));
    r.line_report.n_lines_removed = lrem1[w];
    r.n_points_solved = c->h_nP[w];
    for (int i : o->psrc[w]) q.P.t[i].solved = 1;   // setDepth: solve_flag (vpl_odo_select's cloud)
    r.n_lines_solved = c->h_nL[w];
    r.n_point_tracks = (int)q.P.t.size();
    r.n_line_tracks = (int)q.L.t.size();
    r.n_ignored = 0;
    q.failure = vpl_failure_detection(nullptr, r.speed_bias[NF - 1], r.pose[NF - 1], q.last_pose);
    std::memcpy(q.last_pose, r.pose[NF - 1], 56);
    int lrem2 = 0;
    if (solve_opt.remove_line_outliers)
      for (int dl = 0; dl < c->h_nL[w]; ++dl) lrem2 += h_flags[box.line_flags + kL + dl] ? 1 : 0;
    kL += c->h_nL[w];
    r.report.n_lines_removed = lrem2;
    if (marg[w]) {
      const int* pt = h_flags + box.prior_tabs + kT;
      kT += 2 + 3 * (marg[w] - 1);
      HostTab T;
      T.n = pt[0]; T.nb = pt[1];
      if (T.n < 0 || T.n > MAXKEEP || T.nb < 0 || T.nb > marg[w] - 1) return fail(c, VPL_E_HIP, "odo_solve: prior table out of range");
      for (int b = 0; b < T.nb; ++b) { T.kind[b] = pt[2 + b]; T.frame[b] = pt[2 + T.nb + b]; T.idx[b] = pt[2 + 2 * T.nb + b]; }
      q.prior = T;
      q.has_prior = T.n > 0;
    } else {
      r.report.prior_n = q.has_prior ? q.prior.n : 0;   // MARGIN_SECOND_NEW left the prior as it was (estimator.cpp:1385)
    }
  }
  o->solved = true;
  return VPL_OK;
}

}  // extern "C"

// vpl_odo_advance / vpl_odo_advance_imu
static int odo_advance_impl(vpl_odo* o, const OdoNext& next, vpl_odo_result* out, vpl_odo_imu_out* imu_out) {
  vpl_ctx* c = o->c;
  if (!o->solved) return fail(c, VPL_E_INVALID, "odo_advance: no solved window (vpl_odo_solve)");
  { const int rn = odo_check_next(o, next); if (rn) return rn; }
  const int nS = o->nS, flag = o->flag;
  HIPCHK(c, hipSetDevice(c->device));
  { const int rs = settle(c); if (rs) return rs; }
  using oclk = std::chrono::steady_clock;
  const auto t0 = oclk::now();
  hipStream_t s = c->stream;
  const dim3 grid(nS), blk(ODO_THREADS);
  const OdoStore S = o->st[o->cur];
  const int* const h_flags = odo_out_views(o).h_flags;
  const OdoOutbox& box = o->box;
  // 4. the book: removeFailures and the solve's removeLineOutlier, the slide, the new frame -- and the tables that tell the
  // device what moved where; then ONE copy host -> device (the new frames' doubles, then the tables) and two launches
  double* pay = reinterpret_cast<double*>(o->h_in);
  size_t npay = 0;
  for (int w = 0; w < nS; ++w) npay += next.head(w) + 3 * (size_t)next.obs(w).n_points + 8 * (size_t)next.obs(w).n_lines;
  int* tab = reinterpret_cast<int*>(o->h_in + npay * 8);
  size_t ntab = 0;
  int* hdr = tab; ntab += ODO_HDR * (size_t)nS;
  int* cnt = tab + ntab; ntab += 2 * (size_t)nS;
  int* pmv = tab + ntab; ntab += (size_t)nS * o->maxPT;
  int* lmv = tab + ntab; ntab += (size_t)nS * o->maxLT;
  int* ent = tab + ntab;
  size_t nent = 0, poff = 0, kP = 0, kL = 0;
  std::vector<OdoMove> mv;
  std::vector<unsigned char> er;
  for (int w = 0; w < nS; ++w) {
    OdoSeq& q = o->seq[w];
    vpl_odo_result scratch;
    vpl_odo_result& r = out ? out[w] : scratch;
    // removeFailures: solved points whose inverse depth is not > 0 (feature_manager.cpp:254-263)
    er.assign(q.P.t.size(), 0);
    for (int p = 0; p < box.nP[w]; ++p, ++kP)
      if (!h_flags[box.point_flags + kP]) er[o->psrc[w][p]] = 1;
    odo_erase_slide(q.P, er.data(), flag == VPL_MARGIN_SECOND_NEW, mv, nullptr);
    cnt[2 * w] = (int)mv.size();
    for (size_t j = 0; j < mv.size(); ++j) pmv[(size_t)w * o->maxPT + j] = odo_pack_move(mv[j]);
    // the lines the solve's removeLineOutlier erased
    er.assign(q.L.t.size(), 0);
    if (o->remove_line_outliers)
      for (int dl = 0; dl < box.nL[w]; ++dl)
        if (h_flags[box.line_flags + kL + dl]) er[o->lsrc[w][o->s_lmap[w][dl]]] = 1;
    kL += box.nL[w];
    odo_erase_slide(q.L, er.data(), flag == VPL_MARGIN_SECOND_NEW, mv, nullptr);
    cnt[2 * w + 1] = (int)mv.size();
    for (size_t j = 0; j < mv.size(); ++j) lmv[(size_t)w * o->maxLT + j] = odo_pack_move(mv[j]);
    // pre-integrations: MARGIN_OLD moves 2..10 down, the new interval enters slot 10 (from samples: the device's sum_dt of
    // slots 9 and 10 comes back below)
    if (flag == VPL_MARGIN_OLD)
      for (int j = 1; j < NF - 1; ++j) q.sum_dt[j] = q.sum_dt[j + 1];
    if (next.plain) q.sum_dt[NF - 1] = next.plain[w].preint.sum_dt;
    // the new frame
    const OdoObs f = next.obs(w);
    int* h = hdr + ODO_HDR * w;
    h[0] = (int)poff; h[1] = f.n_points; h[2] = f.n_lines;
    h[3] = (int)(ntab + nent); h[4] = (int)(ntab + nent + f.n_points); h[5] = next.n_samples(w);
    r.n_ignored = odo_add_frame(q.P, NF - 1, f.n_points, f.point_id, ent + nent);
    r.n_ignored += odo_add_frame(q.L, NF - 1, f.n_lines, f.line_id, ent + nent + f.n_points);
    nent += (size_t)f.n_points + f.n_lines;
    r.n_point_tracks = (int)q.P.t.size();
    r.n_line_tracks = (int)q.L.t.size();
    double* d = pay + poff;
    next.write_head(w, d);
    d += next.head(w);
    if (f.n_points) std::memcpy(d, f.point_obs, (size_t)f.n_points * 24);
    if (f.n_lines) std::memcpy(d + 3 * (size_t)f.n_points, f.line_obs, (size_t)f.n_lines * 64);
    poff += next.head(w) + 3 * (size_t)f.n_points + 8 * (size_t)f.n_lines;
  }
  // the keyframe rule: what the book knows of the window with the new image in it rides behind the other tables
  size_t npar = 0;
  if (o->rule) npar = odo_write_parallax_tab(o, 0, nS, ent + nent, ntab + nent);
  const size_t in_bytes = npay * 8 + (ntab + nent + npar) * 4;   // (within in_cap: odo_inbox_bytes and odo_check_next go by the same capacities)
  HIPCHK(c, hipMemcpyAsync(o->d_in, o->h_in, in_bytes, hipMemcpyHostToDevice, s));
  o->h2d_payload = (long long)npay * 8;
  o->h2d_table += (long long)(ntab + nent + npar) * 4;
  const int* d_tab = reinterpret_cast<const int*>(o->d_in + npay * 8);
  const OdoStore D = o->st[o->cur ^ 1];
  hipLaunchKernelGGL(k_odo_slide, dim3(nS, ODO_SLIDE_Y), blk, 0, s, S, D, d_tab + (pmv - tab), d_tab + (lmv - tab), d_tab + (cnt - tab),
                     flag == VPL_MARGIN_SECOND_NEW ? 1 : 0, o->init_depth);
  hipLaunchKernelGGL(k_odo_append, grid, blk, 0, s, D, reinterpret_cast<const double*>(o->d_in), d_tab, d_tab);
  if (next.imu) {   // merge into slot 9 (MARGIN_SECOND_NEW), the new interval, the propagated state: 18 doubles per sequence come back
    const vpl_ba_options& p = o->opt;
    hipLaunchKernelGGL(k_odo_imu, grid, dim3(64), 0, s, D, o->im[o->cur], o->im[o->cur ^ 1], reinterpret_cast<const double*>(o->d_in), d_tab,
                       flag == VPL_MARGIN_SECOND_NEW ? 1 : 0, p.acc_n * p.acc_n, p.gyr_n * p.gyr_n, p.acc_w * p.acc_w, p.gyr_w * p.gyr_w,
                       p.g_norm, reinterpret_cast<double*>(o->d_out));
  }
  // what comes back: the 18 doubles per sequence of the IMU form, the decision records behind them, in one copy
  const size_t imu_bytes = next.imu ? (size_t)nS * ODO_IMU_OUT_D * 8 : 0, dec_bytes = o->rule ? (size_t)nS * sizeof(OdoParallaxRec) : 0;
  if (o->rule)
    hipLaunchKernelGGL(k_odo_parallax, grid, blk, 0, s, D, d_tab, d_tab + (ent + nent - tab), 0, o->kf_rule.min_parallax, o->kf_rule.min_track_num,
                       reinterpret_cast<OdoParallaxRec*>(o->d_out + imu_bytes));
  if (imu_bytes + dec_bytes) {
    HIPCHK(c, hipMemcpyAsync(o->h_out, o->d_out, imu_bytes + dec_bytes, hipMemcpyDeviceToHost, s));
    o->d2h += (long long)(imu_bytes + dec_bytes);
  }
  HIPCHK(c, hipGetLastError());
  o->cur ^= 1;
  // (the pinned inbox is rewritten by the next keyframe: the copy above must have left it)
  HIPCHK(c, hipStreamSynchronize(s));
  if (next.imu) {
    const double* r = reinterpret_cast<const double*>(o->h_out);
    for (int w = 0; w < nS; ++w, r += ODO_IMU_OUT_D) {
      // the mirror that decides whether IMU factor (0, 1) is in the marginalisation: the device's own sums, bit for bit
      o->seq[w].sum_dt[NF - 2] = r[16];
      o->seq[w].sum_dt[NF - 1] = r[17];
      if (imu_out) { std::memcpy(imu_out[w].pose, r, 56); std::memcpy(imu_out[w].speed_bias, r + 7, 72); imu_out[w].sum_dt[0] = r[16]; imu_out[w].sum_dt[1] = r[17]; }
    }
  }
  if (o->rule) odo_read_decisions(o, 0, nS, o->h_out + imu_bytes);
  o->solved = false;
  o->ms[3] = std::chrono::duration<double, std::milli>(oclk::now() - t0).count();
  return VPL_OK;
}

static int odo_keyframe_impl(vpl_odo* o, const OdoNext& next, const int* flags, vpl_odo_result* out, vpl_odo_imu_out* imu_out) {
  if (o->solved) return fail(o->c, VPL_E_INVALID, "odo_keyframe: the window has been solved and not advanced (vpl_odo_advance)");
  int rc = odo_check_next(o, next);
  if (!rc) rc = vpl_odo_solve(o, flags, out);
  if (!rc) rc = odo_advance_impl(o, next, out, imu_out);
  return rc;
}

extern "C" {

int vpl_odo_advance(vpl_odo* o, const vpl_odo_frame* next, vpl_odo_result* out) {
  if (!o || !next) return VPL_E_INVALID;
  OdoNext n;
  n.plain = next;
  return odo_advance_impl(o, n, out, nullptr);
}
int vpl_odo_keyframe(vpl_odo* o, const vpl_odo_frame* next, const int* flags, vpl_odo_result* out) {
  if (!o || !next || !flags || !out) return VPL_E_INVALID;
  OdoNext n;
  n.plain = next;
  return odo_keyframe_impl(o, n, flags, out, nullptr);
}
int vpl_odo_advance_imu(vpl_odo* o, const vpl_odo_imu_frame* next, vpl_odo_result* out, vpl_odo_imu_out* imu_out) {
  if (!o || !next) return VPL_E_INVALID;
  OdoNext n;
  n.imu = next;
  return odo_advance_impl(o, n, out, imu_out);
}
int vpl_odo_keyframe_imu(vpl_odo* o, const vpl_odo_imu_frame* next, const int* flags, vpl_odo_result* out, vpl_odo_imu_out* imu_out) {
  if (!o || !next || !flags || !out) return VPL_E_INVALID;
  OdoNext n;
  n.imu = next;
  return odo_keyframe_impl(o, n, flags, out, imu_out);
}

// The IMU side: allocated once, through the context's guarded allocator; the inbox is replaced by a larger one when max_samples
// rows outweigh the state + pre-integration they replace.  A failure leaves nothing behind: a second call is a first call
int vpl_odo_enable_imu(vpl_odo* o, int max_samples) {
  if (!o || max_samples < 1) return VPL_E_INVALID;
  vpl_ctx* c = o->c;
  if (o->imu) return fail(c, VPL_E_INVALID, "odo_enable_imu: already enabled");
  if (o->solved) return fail(c, VPL_E_INVALID, "odo_enable_imu: between vpl_odo_solve and vpl_odo_advance");
  { const int rq = odo_quiesce(o); if (rq) return rq; }
  const size_t nS = o->nS;
  hipError_t e = hipSuccess;
  for (OdoImu& m : o->im) {
    m.max = max_samples;
    if (e == hipSuccess) e = dalloc(c, &m.smp, nS * max_samples * 7, o);
    if (e == hipSuccess) e = dalloc(c, &m.lin, nS * 6, o);
    if (e == hipSuccess) e = dalloc(c, &m.n, nS, o);
  }
  if (e != hipSuccess || odo_resize_inbox(o, max_samples, o->rule)) {
    for (OdoImu& m : o->im) { dfree(c, m.smp); dfree(c, m.lin); dfree(c, m.n); m = OdoImu{}; }
    return fail(c, VPL_E_HIP, "odo_enable_imu: allocation failed");
  }
  o->max_samples = max_samples;
  o->imu = true;
  for (OdoSeq& q : o->seq) q.imu_set = false;
  return VPL_OK;
}

int vpl_odo_set_imu(vpl_odo* o, int seq, int n10, const double* samples10, const double* acc0_10, const double* gyr0_10) {
  if (!o || seq < 0 || seq >= o->nS || !samples10 || !acc0_10 || !gyr0_10) return VPL_E_INVALID;
  vpl_ctx* c = o->c;
  if (!o->imu) return fail(c, VPL_E_INVALID, "odo_set_imu: the session does not take IMU samples (vpl_odo_enable_imu)");
  if (!o->seq[seq].set) return fail(c, VPL_E_INVALID, "odo_set_imu: the sequence has no window (vpl_odo_set_window)");
  if (n10 < 1) return fail(c, VPL_E_INVALID, "odo_set_imu: an interval needs at least one IMU sample");
  if (n10 > o->max_samples) return fail(c, VPL_E_CAPACITY, "odo_set_imu: more IMU samples than max_samples");
  { const int rq = odo_quiesce(o); if (rq) return rq; }
  const OdoImu& m = o->im[o->cur];
  double lin[6];
  std::memcpy(lin, acc0_10, 24); std::memcpy(lin + 3, gyr0_10, 24);
  HIPCHK(c, hipMemcpy(m.smp + (size_t)seq * m.max * 7, samples10, (size_t)n10 * 56, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(m.lin + (size_t)seq * 6, lin, 48, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(m.n + seq, &n10, 4, hipMemcpyHostToDevice));
  o->seq[seq].imu_set = true;
  return VPL_OK;
}

// ---- the session's first window from the visual-inertial alignment (csrc/init_align_host.h) -------------------------------------
int vpl_odo_init(vpl_odo* o, const vpl_init_input* in, const double (*ex_pose)[7], const vpl_odo_frame* frames, vpl_init_result* out) {
  if (!o || !in || !ex_pose || !frames || !out) return VPL_E_INVALID;
  vpl_ctx* c = o->c;
  const int nS = o->nS;
  if (o->solved) return fail(c, VPL_E_INVALID, "odo_init: between vpl_odo_solve and vpl_odo_advance");
  // 1. every refusal, on copies: the alignment's, the books', the IMU buffer's, the capacities of the triangulation's batch
  { const int ri = init_check_inputs(c, nS, in); if (ri) return ri; }
  std::vector<OdoBook> P(nS), L(nS);
  std::vector<std::vector<std::vector<int>>> pd(nS), ld(nS);
  std::vector<int> job10(3 * (size_t)nS);
  for (int w = 0; w < nS; ++w) {
    const vpl_odo_frame* fw = frames + (size_t)w * NF;
    for (int f = 0; f < NF; ++f)
      if (odo_check_frame(odo_obs(fw[f]))) return fail(c, VPL_E_INVALID, "odo_init: null observation array");
    const int rb = odo_build_books(o, fw, P[w], L[w], pd[w], ld[w], "odo_init");
    if (rb) return rb;
    const int F = in[w].n_frames;
    std::vector<int> jobs((size_t)(F + 9) * 3);
    init_build_jobs(F, in[w].n_samples, in[w].key, jobs.data());
    std::memcpy(&job10[3 * (size_t)w], &jobs[3 * (size_t)(F + 8)], 12);   // window interval 10
    if (o->imu && job10[3 * (size_t)w + 1] > o->max_samples) return fail(c, VPL_E_CAPACITY, "odo_init: window interval 10 holds more IMU samples than max_samples");
  }
  for (int w = 0; w < nS; ++w) { std::swap(o->seq[w].P, P[w]); std::swap(o->seq[w].L, L[w]); }
  odo_select(o);
  {
    const DevBatch& B = c->B;
    bool fits = true;
    for (int w = 0; w < nS; ++w) {
      long po = 0, lo = 0;
      for (int n : o->pnobs[w]) po += n;
      for (int n : o->lnobs[w]) lo += n;
      fits = fits && (int)o->pstart[w].size() <= B.maxP && (int)o->lstart[w].size() <= B.maxL && po <= B.maxPO && lo <= B.maxLO;
    }
    if (!fits) {
      for (int w = 0; w < nS; ++w) { std::swap(o->seq[w].P, P[w]); std::swap(o->seq[w].L, L[w]); }
      odo_select(o);   // the selection of the books that stay
      return fail(c, VPL_E_CAPACITY, "odo_init: the selected tracks exceed the context's capacities");
    }
  }
  // from here on the sequences are rewritten: one that does not come out aligned holds no window
  auto drop = [&](int w) {
    OdoSeq& q = o->seq[w];
    q.P = OdoBook(); q.L = OdoBook();
    q.set = false; q.imu_set = false; q.has_prior = false; q.prior = HostTab(); q.dec_set = false; q.failure = 0;
  };
  auto drop_all = [&](int rc) { for (int w = 0; w < nS; ++w) drop(w); return rc; };
  o->solved = false;
  { const int rq = odo_quiesce(o); if (rq) return drop_all(rq); }
  const OdoStore S = o->st[o->cur];
  hipStream_t s = c->stream;
  // 2. the observations, on the SfM camera frames: pose = (T_key, quat(R_key)), extrinsic = (0, qic), every depth unset
  for (int w = 0; w < nS; ++w) {
    const int ru = odo_upload_tracks(o, w, o->seq[w].P, o->seq[w].L, pd[w], ld[w], frames + (size_t)w * NF);
    if (ru) return drop_all(ru);
    double pose[NF][7], ex0[7] = {0, 0, 0, ex_pose[w][3], ex_pose[w][4], ex_pose[w][5], ex_pose[w][6]};
    for (int i = 0; i < NF; ++i) {
      const double* R = in[w].R + 9 * (size_t)in[w].key[i];
      const double* T = in[w].T + 3 * (size_t)in[w].key[i];
      M3 Rm;
      for (int k = 0; k < 9; ++k) Rm.m[k] = R[k];
      const Q4 q = mat2q(Rm);
      pose[i][0] = T[0]; pose[i][1] = T[1]; pose[i][2] = T[2]; pose[i][3] = q.x; pose[i][4] = q.y; pose[i][5] = q.z; pose[i][6] = q.w;
    }
    if (hipMemcpy(S.pose + (size_t)w * 77, pose, 77 * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(S.ex + (size_t)w * 7, ex0, 7 * 8, hipMemcpyHostToDevice) != hipSuccess)
      return drop_all(fail(c, VPL_E_HIP, "odo_init: upload of the SfM frames failed"));
  }
  // 3. the alignment, its results staying on the device
  InitDevice D;
  const void* owner = &D;
  std::vector<vpl_init_result> res(nS);
  std::vector<double> sum_dt((size_t)nS * NF, 0.0);
  auto run = [&]() -> int {
    int rc = init_enqueue(c, nS, in, &o->opt, owner, D);
    if (rc) return rc;
    // 4. the session's own point triangulation on that store; no line is touched
    vpl_ba_options topt;
    vpl_ba_default_options(&topt);
    topt.marginalization_flag = VPL_MARGIN_NONE;
    const OdoSrc src = odo_src(o, false);
    if ((rc = upload_impl(c, nS, o->win.data(), &topt, true, false, &src))) return rc;
    launch_triangulate(c, nS, true, false, o->init_depth);
    hipLaunchKernelGGL(k_odo_scatter_tri, dim3(nS), dim3(ODO_THREADS), 0, s, c->B, S, (const int*)o->d_psrc, (const int*)o->d_lsrc,
                       odo_out_views(o).d_flags);
    // 5. states, extrinsic, pre-integrations and the scale into the store
    double* d_ex = nullptr;   // [nS][7] the true extrinsics | [nS][11] sum_dt back
    HIPCHK(c, dalloc(c, &d_ex, (size_t)nS * (7 + NF), owner));
    HIPCHK(c, hipMemcpyAsync(d_ex, ex_pose, (size_t)nS * 56, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_odo_init_finish, dim3(nS), dim3(ODO_THREADS), 0, s, c->B, S, (const int*)o->d_psrc,
                       (const vpl_init_result*)D.results(), (const DevPreint*)(D.pre3() + D.J1), (const double*)d_ex, d_ex + (size_t)nS * 7);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(res.data(), D.results(), (size_t)nS * sizeof(vpl_init_result), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(sum_dt.data(), d_ex + (size_t)nS * 7, (size_t)nS * NF * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    int hits = 0;
    if ((rc = init_guard_hits(c, owner, &hits))) return rc;
    return hits ? fail(c, VPL_E_HIP, "odo_init: guard behind " + std::to_string(hits) + " device array(s) overwritten") : VPL_OK;
  };
  const int rr = run();
  dfree_owner(c, owner);
  if (rr) return drop_all(rr);
  // 6. the host's side of every sequence
  for (int w = 0; w < nS; ++w) {
    out[w] = res[w];
    if (!res[w].ok) { drop(w); continue; }
    OdoSeq& Q = o->seq[w];
    for (int f = 0; f < NF; ++f) Q.sum_dt[f] = sum_dt[(size_t)w * NF + f];
    Q.prior = HostTab();
    Q.has_prior = false;
    Q.set = true;
    Q.imu_set = false;
    std::memcpy(Q.last_pose, res[w].pose[NF - 2], 56);
    Q.failure = 0;
    Q.dec_set = false;
    if (o->imu) {   // the samples of window interval 10 are slot 10's buffer, what starts them its linearized_acc / _gyr
      const int* j = &job10[3 * (size_t)w];
      const double* first = j[2] < 0 ? nullptr : in[w].samples + 7 * (size_t)j[2];
      double lin[6];
      for (int k = 0; k < 3; ++k) { lin[k] = first ? first[1 + k] : in[w].acc0[k]; lin[3 + k] = first ? first[4 + k] : in[w].gyr0[k]; }
      const OdoImu& m = o->im[o->cur];
      if (hipMemcpy(m.smp + (size_t)w * m.max * 7, in[w].samples + 7 * (size_t)j[0], (size_t)j[1] * 56, hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(m.lin + (size_t)w * 6, lin, 48, hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(m.n + w, &j[1], 4, hipMemcpyHostToDevice) != hipSuccess)
        return drop_all(fail(c, VPL_E_HIP, "odo_init: upload of the IMU buffer failed"));
      Q.imu_set = true;
    }
  }
  if (o->rule)
    for (int w = 0; w < nS; ++w)
      if (o->seq[w].set) { const int rd = odo_decide(o, w, 1); if (rd) return drop_all(rd); }
  return VPL_OK;
}

// ---- the keyframe decision and the failure check ------------------------------------------------------------------------------
void vpl_odo_default_keyframe_rule(vpl_odo_keyframe_rule* r) {
  if (!r) return;
  r->min_parallax = 10.0 / 460.0;
  r->min_track_num = 20;
}

// The inbox was sized at create without the list; the first call replaces it by one with room for it (odo_resize_inbox: the
// smaller one is freed at once)
int vpl_odo_enable_keyframe_rule(vpl_odo* o, const vpl_odo_keyframe_rule* rule) {
  if (!o || !rule) return VPL_E_INVALID;
  vpl_ctx* c = o->c;
  if (!(rule->min_parallax == rule->min_parallax)) return fail(c, VPL_E_INVALID, "odo_enable_keyframe_rule: min_parallax is not a number");
  if (o->solved) return fail(c, VPL_E_INVALID, "odo_enable_keyframe_rule: between vpl_odo_solve and vpl_odo_advance");
  { const int rq = odo_quiesce(o); if (rq) return rq; }
  if (!o->rule) {
    if (odo_resize_inbox(o, o->max_samples, true)) return fail(c, VPL_E_HIP, "odo_enable_keyframe_rule: allocation failed");
    o->rule = true;
  }
  o->kf_rule = *rule;
  return odo_decide(o, 0, o->nS);
}

void vpl_failure_default_limits(vpl_failure_limits* l) {
  if (!l) return;
  l->max_acc_bias = 2.5; l->max_gyr_bias = 1.0; l->max_translation = 5.0; l->max_z = 1.0;
}

// Estimator::failureDetection (estimator.cpp:909-936): Eigen's norm() is the square root of the sum of squares, taken in order
int vpl_failure_detection(const vpl_failure_limits* limits, const double* sb, const double* pose, const double* last_pose) {
  if (!sb || !pose || !last_pose) return VPL_E_INVALID;
  vpl_failure_limits l;
  if (limits) l = *limits; else vpl_failure_default_limits(&l);
  const auto norm3 = [](double x, double y, double z) { return std::sqrt(x * x + y * y + z * z); };
  const double dx = pose[0] - last_pose[0], dy = pose[1] - last_pose[1], dz = pose[2] - last_pose[2];
  int mask = 0;
  if (norm3(sb[3], sb[4], sb[5]) > l.max_acc_bias) mask |= VPL_FAIL_ACC_BIAS;
  if (norm3(sb[6], sb[7], sb[8]) > l.max_gyr_bias) mask |= VPL_FAIL_GYR_BIAS;
  if (norm3(dx, dy, dz) > l.max_translation) mask |= VPL_FAIL_TRANSLATION;
  if (std::fabs(dz) > l.max_z) mask |= VPL_FAIL_Z;
  return mask;
}

int vpl_odo_get_decision(vpl_odo* o, int seq, vpl_odo_decision* out) {
  if (!o || seq < 0 || seq >= o->nS || !out) return VPL_E_INVALID;
  vpl_ctx* c = o->c;
  if (!o->rule) return fail(c, VPL_E_INVALID, "odo_get_decision: the keyframe rule is off (vpl_odo_enable_keyframe_rule)");
  const OdoSeq& q = o->seq[seq];
  if (!q.set || !q.dec_set) return fail(c, VPL_E_INVALID, "odo_get_decision: the sequence has no window (vpl_odo_set_window)");
  out->flag = q.dec.flag;
  out->last_track_num = q.dec.last_track_num;
  out->parallax_num = q.dec.parallax_num;
  out->failure = q.failure;
  out->parallax_sum = q.dec.parallax_sum;
  out->parallax_mean = q.dec.parallax_num ? q.dec.parallax_sum / q.dec.parallax_num : 0.0;
  return VPL_OK;
}

}  // extern "C"

// the flag array of an _auto call: the stored decisions, when there is one for every sequence and they agree
static int odo_auto_flags(vpl_odo* o, std::vector<int>& flags) {
  vpl_ctx* c = o->c;
  if (!o->rule) return fail(c, VPL_E_INVALID, "odo: the keyframe rule is off (vpl_odo_enable_keyframe_rule)");
  int n_old = 0, n_new = 0;
  flags.resize(o->nS);
  for (int w = 0; w < o->nS; ++w) {
    const OdoSeq& q = o->seq[w];
    if (!q.set || !q.dec_set) return fail(c, VPL_E_INVALID, "odo: a sequence has no window (vpl_odo_set_window)");
    flags[w] = q.dec.flag;
    ++(q.dec.flag == VPL_MARGIN_OLD ? n_old : n_new);
  }
  if (n_old && n_new)
    return fail(c, VPL_E_INVALID, "odo: the sequences' keyframe decisions disagree (" + std::to_string(n_old) + " want VPL_MARGIN_OLD, " +
                                      std::to_string(n_new) + " VPL_MARGIN_SECOND_NEW) and the batched solve marginalises one way per batch: pass explicit flags");
  return VPL_OK;
}

extern "C" {

int vpl_odo_solve_auto(vpl_odo* o, vpl_odo_result* out) {
  if (!o || !out) return VPL_E_INVALID;
  std::vector<int> flags;
  const int rc = odo_auto_flags(o, flags);
  return rc ? rc : vpl_odo_solve(o, flags.data(), out);
}
int vpl_odo_keyframe_auto(vpl_odo* o, const vpl_odo_frame* next, vpl_odo_result* out) {
  if (!o || !next || !out) return VPL_E_INVALID;
  std::vector<int> flags;
  const int rc = odo_auto_flags(o, flags);
  return rc ? rc : vpl_odo_keyframe(o, next, flags.data(), out);
}
int vpl_odo_keyframe_imu_auto(vpl_odo* o, const vpl_odo_imu_frame* next, vpl_odo_result* out, vpl_odo_imu_out* imu_out) {
  if (!o || !next || !out) return VPL_E_INVALID;
  std::vector<int> flags;
  const int rc = odo_auto_flags(o, flags);
  return rc ? rc : vpl_odo_keyframe_imu(o, next, flags.data(), out, imu_out);
}

// the inverse of to_dev_preint for what DevPreint holds: columns 0..8 of the jacobian are not held and come back zero
int vpl_odo_get_preint(vpl_odo* o, int seq, vpl_preintegration* out) {
  if (!o || seq < 0 || seq >= o->nS || !out) return VPL_E_INVALID;
  vpl_ctx* c = o->c;
  if (!o->seq[seq].set) return fail(c, VPL_E_INVALID, "odo_get_preint: the sequence has no window (vpl_odo_set_window)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<DevPreint> h(NF);
  HIPCHK(c, hipMemcpy(h.data(), o->st[o->cur].pre + (size_t)seq * NF, sizeof(DevPreint) * NF, hipMemcpyDeviceToHost));
  std::memset(out, 0, sizeof(vpl_preintegration) * NF);
  for (int f = 1; f < NF; ++f) {
    const DevPreint& d = h[f];
    vpl_preintegration& p = out[f];
    std::memcpy(&p, &d, 17 * 8);   // sum_dt, delta_p, delta_q, delta_v, linearized_ba, linearized_bg: the same 17 doubles
    const double* blk[5] = {d.dp_dba, d.dp_dbg, d.dq_dbg, d.dv_dba, d.dv_dbg};
    const int r0[5] = {0, 0, 3, 6, 6}, c0[5] = {9, 12, 12, 9, 12};
    for (int b = 0; b < 5; ++b)
      for (int e = 0; e < 9; ++e) p.jacobian[(r0[b] + e / 3) * 15 + c0[b] + e % 3] = blk[b][e];
    for (int k = 9; k < 15; ++k) p.jacobian[k * 15 + k] = 1.0;
    std::memcpy(p.covariance, d.cov, sizeof(p.covariance));
  }
  return VPL_OK;
}

int vpl_odo_get_states(vpl_odo* o, int seq, double (*pose)[7], double (*speed_bias)[9], double* ex_pose) {
  if (!o || seq < 0 || seq >= o->nS || !pose || !speed_bias || !ex_pose) return VPL_E_INVALID;
  vpl_ctx* c = o->c;
  if (!o->seq[seq].set) return fail(c, VPL_E_INVALID, "odo_get_states: the sequence has no window");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const OdoStore& S = o->st[o->cur];
  HIPCHK(c, hipMemcpy(pose, S.pose + (size_t)seq * 77, 77 * 8, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(speed_bias, S.sb + (size_t)seq * 99, 99 * 8, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(ex_pose, S.ex + (size_t)seq * 7, 7 * 8, hipMemcpyDeviceToHost));
  return VPL_OK;
}

int vpl_odo_get_prior(vpl_odo* o, int seq, vpl_prior* out) {
  if (!o || seq < 0 || seq >= o->nS || !out) return VPL_E_INVALID;
  vpl_ctx* c = o->c;
  std::memset(out, 0, sizeof(int) * (2 + 3 * VPL_MAX_PRIOR_BLOCKS));
  const OdoSeq& q = o->seq[seq];
  if (!q.has_prior) return VPL_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const HostTab& T = q.prior;
  out->n = T.n; out->n_blocks = T.nb;
  for (int b = 0; b < T.nb; ++b) { out->block_kind[b] = T.kind[b]; out->block_frame[b] = T.frame[b]; out->block_idx[b] = T.idx[b]; }
  std::vector<double> x0(MAXPB * 9);
  HIPCHK(c, hipMemcpy(x0.data(), o->prior.x0 + (size_t)seq * MAXPB * 9, MAXPB * 9 * 8, hipMemcpyDeviceToHost));
  for (int b = 0; b < T.nb; ++b) std::memcpy(out->x0[b], &x0[(size_t)b * 9], 72);
  HIPCHK(c, hipMemcpy(out->J0, o->prior.J0 + (size_t)seq * MAXKEEP * MAXKEEP, (size_t)T.n * T.n * 8, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(out->r0, o->prior.r0 + (size_t)seq * MAXKEEP, (size_t)T.n * 8, hipMemcpyDeviceToHost));
  return VPL_OK;
}

int vpl_odo_get_tracks(vpl_odo* o, int seq, int* n_points, int* point_id, int* point_start, int* point_nobs, double* inv_depth,
                       int* n_lines, int* line_id, int* line_start, int* line_nobs, int* line_triangulated, double* line_plk) {
  if (!o || seq < 0 || seq >= o->nS) return VPL_E_INVALID;
  vpl_ctx* c = o->c;
  const OdoSeq& q = o->seq[seq];
  const OdoStore& S = o->st[o->cur];
  const size_t nP = q.P.t.size(), nL = q.L.t.size();
  if (n_points) *n_points = (int)nP;
  if (n_lines) *n_lines = (int)nL;
  for (size_t i = 0; i < nP; ++i) {
    if (point_id) point_id[i] = q.P.t[i].id;
    if (point_start) point_start[i] = q.P.t[i].start;
    if (point_nobs) point_nobs[i] = q.P.t[i].nobs;
  }
  for (size_t i = 0; i < nL; ++i) {
    if (line_id) line_id[i] = q.L.t[i].id;
    if (line_start) line_start[i] = q.L.t[i].start;
    if (line_nobs) line_nobs[i] = q.L.t[i].nobs;
    if (line_triangulated) line_triangulated[i] = q.L.t[i].tri;
  }
  if (!inv_depth && !line_plk) return VPL_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (inv_depth && nP) HIPCHK(c, hipMemcpy(inv_depth, S.invd + (size_t)seq * S.maxPT, nP * 8, hipMemcpyDeviceToHost));
  if (line_plk && nL) HIPCHK(c, hipMemcpy(line_plk, S.plk + (size_t)seq * S.maxLT * 6, nL * 6 * 8, hipMemcpyDeviceToHost));
  return VPL_OK;
}

// FeatureSelector::select for the next image of every sequence: the book on the host, state k and the cloud from the store
int vpl_odo_select(vpl_odo* o, const vpl_sel_params* par, const vpl_odo_sel_frame* frames, vpl_odo_sel_result* out, int* selected_id,
                   double* round_f, int* out_ids) {
  if (!o || !par || !frames || !out || !selected_id || !round_f || !out_ids) return VPL_E_INVALID;
  vpl_ctx* c = o->c;
  const int nS = o->nS;
  if (o->solved) return fail(c, VPL_E_INVALID, "odo_select: the window has been solved and not advanced (vpl_odo_advance)");
  for (int w = 0; w < nS; ++w) {
    const vpl_odo_sel_frame& f = frames[w];
    if (f.n_features < 0 || (f.n_features && (!f.id || !f.x || !f.y || !f.prob))) return fail(c, VPL_E_INVALID, "odo_select: null array or negative count");
    if (f.n_features > VPL_SEL_MAX_FEATURES) return fail(c, VPL_E_CAPACITY, "odo_select: an image of more than VPL_SEL_MAX_FEATURES features");
  }
  // the books move on copies: a refusal below leaves every sequence as it was
  struct Job {
    SelBook book;
    SelImage im;
    std::vector<int> new_id;
    std::vector<double> nx, ny, np, ux, uy;
    int entry = -1, n_cloud = 0;
  };
  std::vector<Job> jobs(nS);
  std::vector<vpl_sel_input> in;
  SelGather gs;
  std::vector<std::vector<int>> lists;
  for (int w = 0; w < nS; ++w) {
    const vpl_odo_sel_frame& f = frames[w];
    Job& j = jobs[w];
    j.book = o->seq[w].sel_book;
    j.book.max_features = par->max_features;
    j.book.init_thresh = par->init_thresh;
    sel_book_split(j.book, f.id, f.n_features, j.im);
    if (!o->seq[w].set) continue;
    std::unordered_map<int, int> at;          // id -> its first entry in the image
    for (int i = f.n_features - 1; i >= 0; --i) at[f.id[i]] = i;
    for (int fid : j.im.image_new) { const int i = at[fid]; j.new_id.push_back(fid); j.nx.push_back(f.x[i]); j.ny.push_back(f.y[i]); j.np.push_back(f.prob[i]); }
    for (int fid : j.im.subset) { const int i = at[fid]; j.ux.push_back(f.x[i]); j.uy.push_back(f.y[i]); }
    lists.emplace_back();
    odo_cloud_list(o->seq[w].P, lists.back());
    if ((int)lists.back().size() > VPL_SEL_MAX_FEATURES) return fail(c, VPL_E_CAPACITY, "odo_select: a cloud of more than VPL_SEL_MAX_FEATURES tracks");
    j.n_cloud = (int)lists.back().size();
    j.entry = (int)in.size();
    vpl_sel_input q{};
    std::memcpy(q.P1, f.P1, 24); std::memcpy(q.Q1, f.Q1, 32); std::memcpy(q.V1, f.V1, 24); std::memcpy(q.Ba1, f.Ba1, 24);
    std::memcpy(q.acc, f.acc, 24); std::memcpy(q.gyr, f.gyr, 24);
    q.Q0[0] = 1.0;                            // (state k is written by k_sel_cloud)
    q.delta_imu = f.delta_imu; q.n_imu = f.n_imu; q.kappa = j.im.kappa; q.horizon = f.horizon;
    q.n_new = (int)j.new_id.size(); q.n_used = (int)j.ux.size(); q.n_cloud = j.n_cloud;
    in.push_back(q);
  }
  const int n = (int)in.size();
  for (int w = 0; w < nS; ++w) {              // (the vectors no longer move)
    Job& j = jobs[w];
    if (j.entry < 0) continue;
    vpl_sel_input& q = in[j.entry];
    q.new_id = j.new_id.data(); q.new_x = j.nx.data(); q.new_y = j.ny.data(); q.new_prob = j.np.data();
    q.used_x = j.ux.data(); q.used_y = j.uy.data();
  }
  std::vector<vpl_sel_result> res(std::max(n, 1));
  std::vector<int> ids((size_t)std::max(n, 1) * VPL_SEL_MAX_FEATURES, 0);
  std::vector<double> fs((size_t)std::max(n, 1) * VPL_SEL_MAX_FEATURES, 0.0);
  if (n) {
    const OdoStore& S = o->st[o->cur];
    gs.G = DevSelGather{S.pobs, S.invd, S.pose, S.sb, S.ex, S.maxPT, nullptr};
    gs.tab.assign(3 * (size_t)n, 0);
    for (int w = 0; w < nS; ++w) {
      const Job& j = jobs[w];
      if (j.entry < 0) continue;
      const std::vector<int>& l = lists[j.entry];
      gs.tab[3 * j.entry] = w; gs.tab[3 * j.entry + 1] = (int)gs.tab.size(); gs.tab[3 * j.entry + 2] = (int)l.size();
      gs.tab.insert(gs.tab.end(), l.begin(), l.end());
    }
    const int rc = sel_run(c, n, par, in.data(), res.data(), ids.data(), fs.data(), nullptr, &gs);
    if (rc) return rc;
  }
  for (int w = 0; w < nS; ++w) {
    Job& j = jobs[w];
    vpl_odo_sel_result& r = out[w];
    std::memset(&r, 0, sizeof r);
    int* sid = selected_id + (size_t)w * VPL_SEL_MAX_FEATURES;
    double* sf = round_f + (size_t)w * VPL_SEL_MAX_FEATURES;
    std::fill(sid, sid + VPL_SEL_MAX_FEATURES, 0);
    std::fill(sf, sf + VPL_SEL_MAX_FEATURES, 0.0);
    const bool init = j.entry >= 0;
    if (init) {
      r.sel = res[j.entry];
      std::memcpy(sid, &ids[(size_t)j.entry * VPL_SEL_MAX_FEATURES], VPL_SEL_MAX_FEATURES * 4);
      std::memcpy(sf, &fs[(size_t)j.entry * VPL_SEL_MAX_FEATURES], VPL_SEL_MAX_FEATURES * 8);
    }
    std::vector<int> image;
    sel_book_finish(j.book, j.im, init, sid, r.sel.n_selected, image);
    r.initialized = init ? 1 : 0;
    r.n_new = (int)j.im.image_new.size(); r.n_used = (int)j.im.subset.size(); r.kappa = j.im.kappa; r.n_cloud = j.n_cloud;
    r.n_out = (int)image.size();
    int* oi = out_ids + (size_t)w * VPL_SEL_MAX_FEATURES;
    std::fill(oi, oi + VPL_SEL_MAX_FEATURES, 0);
    std::copy(image.begin(), image.end(), oi);
    o->seq[w].sel_book = j.book;
  }
  return VPL_OK;
}

int vpl_odo_stats(vpl_odo* o, long long* h2d_payload_bytes, long long* h2d_table_bytes, long long* d2h_bytes) {
  if (!o) return VPL_E_INVALID;
  if (h2d_payload_bytes) *h2d_payload_bytes = o->h2d_payload;
  if (h2d_table_bytes) *h2d_table_bytes = o->h2d_table;
  if (d2h_bytes) *d2h_bytes = o->d2h;
  return VPL_OK;
}
int vpl_odo_debug_ms(vpl_odo* o, double* ms4) {
  if (!o || !ms4) return VPL_E_INVALID;
  for (int k = 0; k < 4; ++k) ms4[k] = o->ms[k];
  return VPL_OK;
}

}  // extern "C"

// Host only: the book of one kind of tracks of one sequence replayed from a script (tests/test_odo_tracks.py); slide: [max_tracks][3]
// per step, may be null.  after(s, book, status, n_slide, ignored, frames in the window) reports each step.
template <class F>
static int odo_replay(int max_tracks, int n_steps, const int* flag, const int* n_ids, const int* ids, const unsigned char* erase, int* slide,
                      F&& after) {
  OdoBook b;
  int frames = 0;
  std::vector<OdoMove> mv;
  for (int s = 0; s < n_steps; ids += n_ids[s], ++s) {
    if (n_ids[s] < 0) return VPL_E_INVALID;
    const bool filling = flag[s] == VPL_MARGIN_NONE;
    if (!filling && flag[s] != VPL_MARGIN_OLD && flag[s] != VPL_MARGIN_SECOND_NEW) return VPL_E_INVALID;
    if (filling ? frames >= NF : frames < NF) return VPL_E_INVALID;
    int status = VPL_OK, n_slide = 0, ignored = 0;
    if ((int)b.t.size() + odo_count_unknown(b, n_ids[s], ids) > max_tracks) status = VPL_E_CAPACITY;
    else {
      if (!filling) n_slide = odo_erase_slide(b, erase + (size_t)s * max_tracks, flag[s] == VPL_MARGIN_SECOND_NEW, mv, slide ? slide + (size_t)s * max_tracks * 3 : nullptr);
      ignored = odo_add_frame(b, filling ? frames : NF - 1, n_ids[s], ids, nullptr);
      if (filling) ++frames;
    }
    after(s, b, status, n_slide, ignored, frames);
  }
  return VPL_OK;
}

extern "C" {

int vpl_odo_debug_tracks(int max_tracks, int n_steps, const int* flag, const int* n_ids, const int* ids, const unsigned char* erase,
                         int* status, int* n_slide, int* slide, int* n_tracks, int* table, int* ignored) {
  if (max_tracks < 1 || n_steps < 0 || !flag || !n_ids || !ids || !erase || !status || !n_slide || !slide || !n_tracks || !table || !ignored)
    return VPL_E_INVALID;
  return odo_replay(max_tracks, n_steps, flag, n_ids, ids, erase, slide, [&](int s, const OdoBook& b, int st, int nsl, int ig, int) {
    status[s] = st; n_slide[s] = nsl; ignored[s] = ig;
    n_tracks[s] = (int)b.t.size();
    for (size_t i = 0; i < b.t.size(); ++i) {
      int* e = table + ((size_t)s * max_tracks + i) * 3;
      e[0] = b.t[i].id; e[1] = b.t[i].start; e[2] = b.t[i].nobs;
    }
  });
}

// ... and what the keyframe rule reads off the book after each step (tests/test_odo_keyframe_rule_api.py)
int vpl_odo_debug_parallax_list(int max_tracks, int n_steps, const int* flag, const int* n_ids, const int* ids, const unsigned char* erase,
                                int* n_list, int* list, int* last_track_num) {
  if (max_tracks < 1 || n_steps < 0 || !flag || !n_ids || !ids || !erase || !n_list || !list || !last_track_num) return VPL_E_INVALID;
  return odo_replay(max_tracks, n_steps, flag, n_ids, ids, erase, nullptr, [&](int s, const OdoBook& b, int st, int, int, int frames) {
    n_list[s] = -1; last_track_num[s] = 0;
    if (st == VPL_OK && frames == NF) n_list[s] = odo_parallax_list(b, list + (size_t)s * max_tracks, &last_track_num[s]);
  });
}

}  // extern "C"
