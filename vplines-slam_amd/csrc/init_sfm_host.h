// Host side of the vision-only initial structure (vpl_init_structure_batch, vpl_sfm_debug_plan): the refusals, the schedule of
// construct and the observation tables of every solve as integers, the one packed upload and the one read-back.  Included once by
// vplines_ba.hip, behind ba_ctx.h and init_align_host.h.
#pragma once
#include <unordered_map>

#include "init_sfm.h"

// the refusals of one sequence, before anything is allocated
static int sfm_check_input(const vpl_sfm_input& q, std::string& msg) {
  const int F = q.n_frames;
  if (F < VPL_NFRAMES) { msg = "sfm: fewer than 11 image frames"; return VPL_E_INVALID; }
  if (F > VPL_INIT_MAX_FRAMES) { msg = "sfm: more than VPL_INIT_MAX_FRAMES image frames"; return VPL_E_CAPACITY; }
  if (q.key[0] != 0 || q.key[VPL_WINDOW_SIZE] != F - 1) { msg = "sfm: key[0] != 0 or key[10] != F - 1"; return VPL_E_INVALID; }
  for (int i = 1; i < VPL_NFRAMES; ++i)
    if (q.key[i] <= q.key[i - 1]) { msg = "sfm: key not strictly increasing"; return VPL_E_INVALID; }
  const int rc = sfm_check_tracks(q.l, q.n_tracks, q.track_start, q.track_nobs, msg);
  if (rc) return rc;
  if (q.n_tracks && (!q.track_id || !q.track_obs)) { msg = "sfm: null track_id / track_obs"; return VPL_E_INVALID; }
  if (F > VPL_NFRAMES) {
    if (!q.frame_npts) { msg = "sfm: null frame_npts"; return VPL_E_INVALID; }
    int ki = 0;
    size_t total = 0;
    for (int f = 0; f < F; ++f) {
      if (ki < VPL_NFRAMES && q.key[ki] == f) { ++ki; continue; }
      if (q.frame_npts[f] < 0) { msg = "sfm: a negative frame_npts"; return VPL_E_INVALID; }
      if (q.frame_npts[f] > VPL_SFM_MAX_FRAME_POINTS) { msg = "sfm: a frame list longer than VPL_SFM_MAX_FRAME_POINTS"; return VPL_E_CAPACITY; }
      total += q.frame_npts[f];
    }
    if (total && (!q.frame_id || !q.frame_xy)) { msg = "sfm: null frame_id / frame_xy"; return VPL_E_INVALID; }
  }
  return VPL_OK;
}

// The tables of a call as the host packs them: integers and doubles the kernels read by offset, and the records that hold the
// offsets.
struct SfmPack {
  std::vector<int> itab;
  std::vector<double> dtab;
  std::vector<DevSfmSeq> seqs;
  std::vector<DevSfmEvent> events;
  std::vector<DevSfmProb> probs;
  std::vector<DevSfmFrame> frames;
  std::vector<std::vector<int>> tracked;   // per sequence: the tracks that get a position
  size_t n_ws_obs = 0, n_ws_pt = 0;
  int put(const std::vector<int>& v) { const int at = (int)itab.size(); itab.insert(itab.end(), v.begin(), v.end()); return at; }
};

// a PnP over `n` (track, uv row) pairs: camera slot `slot` free, the points constant
static int sfm_add_pnp(SfmPack& K, int slot, const std::vector<int>& trk, const std::vector<int>& uvrow, int uv0) {
  const int n = (int)trk.size();
  DevSfmProb P{};
  P.nobs = n; P.npt = 0;
  P.o_cam = K.put(std::vector<int>(n, slot));
  P.o_pt = K.put(trk);
  P.o_uv = K.put(uvrow);
  std::vector<int> off(VPL_NFRAMES + 1, 0), list(n);
  for (int f = slot + 1; f <= VPL_NFRAMES; ++f) off[f] = n;
  for (int k = 0; k < n; ++k) list[k] = k;
  P.c_off = K.put(off);
  P.c_list = K.put(list);
  P.free_q = P.free_t = 1 << slot;
  P.uv0 = uv0;
  K.probs.push_back(P);
  return (int)K.probs.size() - 1;
}

static void sfm_pack_sequence(SfmPack& K, int s, const vpl_sfm_input& q) {
  const int N = q.n_tracks, F = q.n_frames, l = q.l;
  SfmPlan plan;
  sfm_build_plan(l, N, q.track_start, q.track_nobs, plan);
  DevSfmSeq d{};
  d.F = F; d.l = l; d.N = N; d.first_fail = plan.first_fail;
  for (int i = 0; i < VPL_NFRAMES; ++i) d.key[i] = q.key[i];
  for (int k = 0; k < 9; ++k) { d.relR[k] = q.relative_R[k]; d.ric[k] = q.ric[k]; }
  for (int k = 0; k < 3; ++k) d.relT[k] = q.relative_T[k];
  std::vector<int> off(N);
  int nob = 0;
  for (int j = 0; j < N; ++j) { off[j] = nob; nob += q.track_nobs[j]; }
  d.t_start = K.put(std::vector<int>(q.track_start, q.track_start + N));
  d.t_nobs = K.put(std::vector<int>(q.track_nobs, q.track_nobs + N));
  d.t_off = K.put(off);
  d.t_step = K.put(plan.step);
  d.uv0 = (int)K.dtab.size();
  K.dtab.insert(K.dtab.end(), q.track_obs, q.track_obs + 2 * (size_t)nob);
  // ---- the chain's events; a PnP carries its problem
  const int list_base = K.put(plan.lists);
  d.ev0 = (int)K.events.size();
  size_t max_obs = 0;
  for (const SfmEvent& e : plan.events) {
    DevSfmEvent de{e.kind, e.f0, e.f1, list_base + e.list0, e.n, -1};
    if (e.kind == SFM_EV_PNP) {
      std::vector<int> trk(plan.lists.begin() + e.list0, plan.lists.begin() + e.list0 + e.n), row(e.n);
      for (int k = 0; k < e.n; ++k) row[k] = off[trk[k]] + e.f0 - q.track_start[trk[k]];
      de.prob = sfm_add_pnp(K, e.f0, trk, row, d.uv0);
      max_obs = std::max(max_obs, (size_t)e.n);
    }
    K.events.push_back(de);
  }
  d.nev = (int)K.events.size() - d.ev0;
  // ---- the BA: every observation of every track that gets a position, track after track
  std::vector<int>& tracked = K.tracked[s];
  {
    DevSfmProb P{};
    std::vector<int> o_cam, o_pt, o_uv, p_trk, p_o0, p_n, p_c0;
    for (int j = 0; j < N; ++j) {
      if (plan.step[j] < 0) continue;
      tracked.push_back(j);
      p_trk.push_back(j); p_o0.push_back((int)o_cam.size()); p_n.push_back(q.track_nobs[j]); p_c0.push_back(q.track_start[j]);
      for (int k = 0; k < q.track_nobs[j]; ++k) {
        o_cam.push_back(q.track_start[j] + k); o_pt.push_back((int)p_trk.size() - 1); o_uv.push_back(off[j] + k);
      }
    }
    P.nobs = (int)o_cam.size(); P.npt = (int)p_trk.size();
    std::vector<int> coff(VPL_NFRAMES + 1, 0), clist(P.nobs);
    for (int k = 0; k < P.nobs; ++k) ++coff[o_cam[k] + 1];
    for (int f = 0; f < VPL_NFRAMES; ++f) coff[f + 1] += coff[f];
    std::vector<int> fill(coff.begin(), coff.end() - 1);
    for (int k = 0; k < P.nobs; ++k) clist[fill[o_cam[k]]++] = k;
    P.o_cam = K.put(o_cam); P.o_pt = K.put(o_pt); P.o_uv = K.put(o_uv);
    P.p_trk = K.put(p_trk); P.p_o0 = K.put(p_o0); P.p_n = K.put(p_n); P.p_c0 = K.put(p_c0);
    P.c_off = K.put(coff); P.c_list = K.put(clist);
    const int all = (1 << VPL_NFRAMES) - 1;
    P.free_q = all & ~(1 << l);
    P.free_t = all & ~(1 << l) & ~(1 << VPL_WINDOW_SIZE);
    P.uv0 = d.uv0;
    K.probs.push_back(P);
    d.ba_prob = (int)K.probs.size() - 1;
    max_obs = std::max(max_obs, (size_t)P.nobs);
    d.ws_obs = K.n_ws_obs; K.n_ws_obs += max_obs;
    d.ws_pt = K.n_ws_pt; K.n_ws_pt += P.npt;
  }
  // ---- the non-key image frames: the entries of their lists whose id is in sfm_tracked_points
  d.fr0 = (int)K.frames.size();
  std::unordered_map<int, int> pos;
  for (int j : tracked) pos[q.track_id[j]] = j;
  size_t row0 = 0;
  const int fuv0 = (int)K.dtab.size();
  int ki = 0;
  for (int f = 0; f < F; ++f) {
    if (ki < VPL_NFRAMES && q.key[ki] == f) { ++ki; continue; }
    const int np = q.frame_npts[f];
    std::vector<int> trk, row;
    for (int k = 0; k < np; ++k) {
      auto it = pos.find(q.frame_id[row0 + k]);
      if (it != pos.end()) { trk.push_back(it->second); row.push_back((int)(row0 + k)); }
    }
    row0 += np;
    DevSfmFrame fr{};
    fr.seq = s; fr.f = f; fr.guess = ki;   // the first key frame behind it (:448-451)
    if ((int)trk.size() < SFM_MIN_FRAME_PNP) {
      d.frame_fail = 1;
      fr.prob = -1;
    } else {
      fr.prob = sfm_add_pnp(K, 0, trk, row, fuv0);
      fr.ws_obs = K.n_ws_obs;
      K.n_ws_obs += trk.size();
    }
    K.frames.push_back(fr);
  }
  if (row0) K.dtab.insert(K.dtab.end(), q.frame_xy, q.frame_xy + 2 * row0);
  d.nfr = (int)K.frames.size() - d.fr0;
  K.seqs.push_back(d);
}

extern "C" {

int vpl_sfm_debug_plan(int l, int n_tracks, const int* track_start, const int* track_nobs, int* step, int* fa, int* fb, int* count,
                       int* first_fail) {
  if (!count || !first_fail || (n_tracks > 0 && (!step || !fa || !fb))) return VPL_E_INVALID;
  std::string msg;
  const int rc = sfm_check_tracks(l, n_tracks, track_start, track_nobs, msg);
  if (rc) return rc;
  SfmPlan plan;
  sfm_build_plan(l, n_tracks, track_start, track_nobs, plan);
  for (int j = 0; j < n_tracks; ++j) { step[j] = plan.step[j]; fa[j] = plan.fa[j]; fb[j] = plan.fb[j]; }
  for (int f = 0; f < VPL_NFRAMES; ++f) count[f] = plan.count[f];
  *first_fail = plan.first_fail;
  return VPL_OK;
}

int vpl_init_structure_batch(vpl_ctx* c, int n, const vpl_sfm_input* in, vpl_sfm_result* out, double* points_chain, double* points_ba,
                             int* tracked_id, double* tracked_xyz) {
  if (!c || n < 0 || !in || !out) return VPL_E_INVALID;
  if (n == 0) return VPL_OK;
  if (n > c->maxW) return fail(c, VPL_E_CAPACITY, "sfm: more sequences than max_windows");
  for (int s = 0; s < n; ++s) {
    std::string msg;
    const int rc = sfm_check_input(in[s], msg);
    if (rc) return fail(c, rc, msg + " (sequence " + std::to_string(s) + ")");
  }
  const int rs = settle(c);
  if (rs) return rs;
  SfmPack K;
  K.tracked.resize(n);
  for (int s = 0; s < n; ++s) sfm_pack_sequence(K, s, in[s]);
  // ---- the packed upload: doubles | sequences | events | problems | frames | integers
  auto up64 = [](size_t b) { return (b + 63) & ~(size_t)63; };
  const size_t nfr = K.frames.size();
  const size_t b_seq = up64(K.dtab.size() * 8), b_ev = up64(b_seq + K.seqs.size() * sizeof(DevSfmSeq)),
               b_pr = up64(b_ev + K.events.size() * sizeof(DevSfmEvent)), b_fr = up64(b_pr + K.probs.size() * sizeof(DevSfmProb)),
               b_it = up64(b_fr + nfr * sizeof(DevSfmFrame)), bytes = b_it + K.itab.size() * 4;
  std::vector<char> buf(bytes, 0);
  if (!K.dtab.empty()) std::memcpy(buf.data(), K.dtab.data(), K.dtab.size() * 8);
  std::memcpy(buf.data() + b_seq, K.seqs.data(), K.seqs.size() * sizeof(DevSfmSeq));
  if (!K.events.empty()) std::memcpy(buf.data() + b_ev, K.events.data(), K.events.size() * sizeof(DevSfmEvent));
  std::memcpy(buf.data() + b_pr, K.probs.data(), K.probs.size() * sizeof(DevSfmProb));
  if (nfr) std::memcpy(buf.data() + b_fr, K.frames.data(), nfr * sizeof(DevSfmFrame));
  if (!K.itab.empty()) std::memcpy(buf.data() + b_it, K.itab.data(), K.itab.size() * 4);
  // ---- the read-back: results | stage | the points after the BA | after the chain
  const size_t npts = (size_t)n * VPL_SFM_MAX_TRACKS * 3;
  const size_t o_stage = up64((size_t)n * sizeof(vpl_sfm_result)), o_X = up64(o_stage + (size_t)n * 4), o_Xc = o_X + npts * 8,
               out_bytes = o_Xc + npts * 8;
  const void* owner = &K;
  char *d_in = nullptr, *d_out = nullptr;
  double *d_wo = nullptr, *d_wp = nullptr;
  int* d_bad = nullptr;
  std::vector<char> h(out_bytes);
  auto run = [&]() -> int {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, dalloc(c, &d_in, bytes, owner));
    HIPCHK(c, dalloc(c, &d_out, out_bytes, owner));
    HIPCHK(c, dalloc(c, &d_wo, std::max<size_t>(K.n_ws_obs, 1) * SFM_OBS_WS, owner));
    HIPCHK(c, dalloc(c, &d_wp, std::max<size_t>(K.n_ws_pt, 1) * SFM_PT_WS, owner));
    HIPCHK(c, dalloc(c, &d_bad, std::max<size_t>(nfr, 1), owner));
    // (the allocator's zeroing runs on the null stream: what the kernels rely on is zeroed again in stream order)
    HIPCHK(c, hipMemsetAsync(d_out, 0, out_bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(d_bad, 0, std::max<size_t>(nfr, 1) * 4, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_in, buf.data(), bytes, hipMemcpyHostToDevice, c->stream));
    DevSfmArgs A;
    A.dtab = (const double*)d_in;
    A.seqs = (const DevSfmSeq*)(d_in + b_seq);
    A.events = (const DevSfmEvent*)(d_in + b_ev);
    A.probs = (const DevSfmProb*)(d_in + b_pr);
    A.frames = (const DevSfmFrame*)(d_in + b_fr);
    A.itab = (const int*)(d_in + b_it);
    A.wo = d_wo; A.wp = d_wp;
    A.out = (vpl_sfm_result*)d_out;
    A.stage = (int*)(d_out + o_stage);
    A.X = (double*)(d_out + o_X);
    A.Xchain = (double*)(d_out + o_Xc);
    A.frame_bad = d_bad;
    { KTimer t(c, "k_sfm_construct"); hipLaunchKernelGGL(k_sfm_construct, dim3(n), dim3(SFM_THREADS), 0, c->stream, A); }
    if (nfr) { KTimer t(c, "k_sfm_frames"); hipLaunchKernelGGL(k_sfm_frames, dim3((unsigned)nfr), dim3(SFM_THREADS), 0, c->stream, A); }
    { KTimer t(c, "k_sfm_finish"); hipLaunchKernelGGL(k_sfm_finish, dim3(n), dim3(64), 0, c->stream, A); }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h.data(), d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int hits = 0;
    const int rg = init_guard_hits(c, owner, &hits);
    if (rg) return rg;
    if (hits) return fail(c, VPL_E_HIP, "sfm: guard behind " + std::to_string(hits) + " device array(s) overwritten");
    return VPL_OK;
  };
  const int rc = run();
  dfree_owner(c, owner);
  if (rc) return rc;
  std::memcpy(out, h.data(), (size_t)n * sizeof(vpl_sfm_result));
  const int* stage = (const int*)(h.data() + o_stage);
  const double* X = (const double*)(h.data() + o_X);
  const double* Xc = (const double*)(h.data() + o_Xc);
  const size_t per = (size_t)VPL_SFM_MAX_TRACKS * 3;
  for (int s = 0; s < n; ++s) {
    // the chain's working points are not an output before the BA has run; the tracked points not before it has passed
    if (points_chain) std::memcpy(points_chain + s * per, Xc + s * per, per * 8);
    if (points_ba) {
      std::memset(points_ba + s * per, 0, per * 8);
      if (stage[s] >= SFM_STAGE_BA_RAN)
        for (int j : K.tracked[s]) std::memcpy(points_ba + s * per + 3 * (size_t)j, X + s * per + 3 * (size_t)j, 24);
    }
    if (tracked_id) std::memset(tracked_id + (size_t)s * VPL_SFM_MAX_TRACKS, 0, (size_t)VPL_SFM_MAX_TRACKS * 4);
    if (tracked_xyz) std::memset(tracked_xyz + s * per, 0, per * 8);
    if (stage[s] == SFM_STAGE_BA_OK) {
      int k = 0;
      for (int j : K.tracked[s]) {
        if (tracked_id) tracked_id[(size_t)s * VPL_SFM_MAX_TRACKS + k] = in[s].track_id[j];
        if (tracked_xyz) std::memcpy(tracked_xyz + s * per + 3 * (size_t)k, X + s * per + 3 * (size_t)j, 24);
        ++k;
      }
    }
  }
  return VPL_OK;
}

}  // extern "C"
