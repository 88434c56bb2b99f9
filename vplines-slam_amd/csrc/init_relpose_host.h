// Host side of the relative pose (vpl_init_relative_pose_batch, vpl_relpose_debug_plan, vpl_init_visual_batch): the refusals,
// the stopping table of every candidate that is tried, the one packed upload and the one read-back.  Included once by
// vplines_ba.hip, behind init_sfm_host.h.
#pragma once
#include "init_relpose.h"

// the refusals of one sequence, before anything is allocated: those vpl_init_structure_batch applies to the track table
static int relpose_check_input(const vpl_relpose_input& q, std::string& msg) {
  const int rc = sfm_check_tracks(0, q.n_tracks, q.track_start, q.track_nobs, msg);
  if (rc) return rc;
  if (q.n_tracks && !q.track_obs) { msg = "relpose: null track_obs"; return VPL_E_INVALID; }
  return VPL_OK;
}

extern "C" {

int vpl_relpose_debug_plan(unsigned long long seed, int i, int n_corres, int* samples, int* niters_after) {
  if (!samples || !niters_after || i < 0 || i >= REL_NCAND || n_corres < RELPOSE_SAMPLE) return VPL_E_INVALID;
  if (n_corres > VPL_SFM_MAX_TRACKS) return VPL_E_CAPACITY;
  for (int it = 0; it < RELPOSE_MAX_ITERS; ++it) {
    int idx[RELPOSE_SAMPLE] = {-1, -1, -1, -1, -1, -1, -1};
    relpose_sample(seed, i, it, n_corres, idx);
    for (int k = 0; k < RELPOSE_SAMPLE; ++k) samples[RELPOSE_SAMPLE * it + k] = idx[k];
  }
  relpose_niters_table(n_corres, niters_after);
  return VPL_OK;
}

int vpl_init_relative_pose_batch(vpl_ctx* c, int n, const vpl_relpose_input* in, vpl_relpose_result* out, unsigned char* mask_ransac,
                                 unsigned char* mask_pose, int* hyp_count) {
  if (!c || n < 0 || !in || !out) return VPL_E_INVALID;
  if (n == 0) return VPL_OK;
  if (n > c->maxW) return fail(c, VPL_E_CAPACITY, "relpose: more sequences than max_windows");
  for (int s = 0; s < n; ++s) {
    std::string msg;
    const int rc = relpose_check_input(in[s], msg);
    if (rc) return fail(c, rc, msg + " (sequence " + std::to_string(s) + ")");
  }
  const int rs = settle(c);
  if (rs) return rs;
  // ---- the tables: per sequence the track table; niters_after of every count that is tried
  std::vector<int> itab;
  std::vector<double> dtab;
  std::vector<DevRelSeq> seqs(n);
  std::unordered_map<int, int> table_at;   // n_corres -> where its niters_after stands in itab
  auto put = [&](const int* p, int k) { const int at = (int)itab.size(); itab.insert(itab.end(), p, p + k); return at; };
  for (int s = 0; s < n; ++s) {
    const vpl_relpose_input& q = in[s];
    const int N = q.n_tracks;
    DevRelSeq d{};
    d.N = N;
    d.seed = q.seed;
    std::vector<int> off(N);
    int nob = 0;
    for (int j = 0; j < N; ++j) { off[j] = nob; nob += q.track_nobs[j]; }
    d.t_start = put(q.track_start, N);
    d.t_nobs = put(q.track_nobs, N);
    d.t_off = put(off.data(), N);
    d.uv0 = (int)dtab.size();
    if (nob) dtab.insert(dtab.end(), q.track_obs, q.track_obs + 2 * (size_t)nob);
    for (int i = 0; i < REL_NCAND; ++i) {
      int m = 0;
      for (int j = 0; j < N; ++j) m += q.track_start[j] <= i && q.track_start[j] + q.track_nobs[j] - 1 >= VPL_WINDOW_SIZE;
      d.ncor[i] = m;
      d.nit[i] = -1;
      if (m > RELPOSE_MIN_CORRES) {   // one table per count: its pow and log are the host's only arithmetic
        auto it = table_at.find(m);
        if (it == table_at.end()) {
          std::vector<int> t(m + 1);
          relpose_niters_table(m, t.data());
          it = table_at.emplace(m, put(t.data(), m + 1)).first;
        }
        d.nit[i] = it->second;
      }
    }
    seqs[s] = d;
  }
  // ---- the packed upload: doubles | sequences | integers
  auto up64 = [](size_t b) { return (b + 63) & ~(size_t)63; };
  const size_t b_seq = up64(dtab.size() * 8), b_it = up64(b_seq + seqs.size() * sizeof(DevRelSeq)), bytes = b_it + std::max<size_t>(itab.size(), 1) * 4;
  std::vector<char> buf(bytes, 0);
  if (!dtab.empty()) std::memcpy(buf.data(), dtab.data(), dtab.size() * 8);
  std::memcpy(buf.data() + b_seq, seqs.data(), seqs.size() * sizeof(DevRelSeq));
  if (!itab.empty()) std::memcpy(buf.data() + b_it, itab.data(), itab.size() * 4);
  // ---- the read-back: results | mask after RANSAC | mask after recoverPose | the hypotheses' counts
  const size_t n_mask = (size_t)n * REL_NCAND * VPL_SFM_MAX_TRACKS, n_hyp = (size_t)n * REL_NCAND * RELPOSE_MAX_ITERS * 3;
  const size_t o_m0 = up64((size_t)n * sizeof(vpl_relpose_result)), o_m1 = up64(o_m0 + (mask_ransac ? n_mask : 0)),
               o_hyp = up64(o_m1 + (mask_pose ? n_mask : 0)), out_bytes = o_hyp + (hyp_count ? n_hyp * 4 : 0);
  const void* owner = &seqs;
  char *d_in = nullptr, *d_out = nullptr;
  std::vector<char> h(out_bytes);
  auto run = [&]() -> int {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, dalloc(c, &d_in, bytes, owner));
    HIPCHK(c, dalloc(c, &d_out, out_bytes, owner));
    // (the allocator's zeroing runs on the null stream: what the kernels rely on is set again in stream order)
    HIPCHK(c, hipMemsetAsync(d_out, 0, o_hyp, c->stream));
    if (hyp_count) HIPCHK(c, hipMemsetAsync(d_out + o_hyp, 0xFF, n_hyp * 4, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_in, buf.data(), bytes, hipMemcpyHostToDevice, c->stream));
    DevRelArgs A;
    A.dtab = (const double*)d_in;
    A.seqs = (const DevRelSeq*)(d_in + b_seq);
    A.itab = (const int*)(d_in + b_it);
    A.out = (vpl_relpose_result*)d_out;
    A.mask_ransac = mask_ransac ? (unsigned char*)(d_out + o_m0) : nullptr;
    A.mask_pose = mask_pose ? (unsigned char*)(d_out + o_m1) : nullptr;
    A.hyp = hyp_count ? (int*)(d_out + o_hyp) : nullptr;
    { KTimer t(c, "k_relpose_ransac"); hipLaunchKernelGGL(k_relpose_ransac, dim3(REL_NCAND, n), dim3(REL_THREADS), 0, c->stream, A); }
    { KTimer t(c, "k_relpose_finish"); hipLaunchKernelGGL(k_relpose_finish, dim3(n), dim3(64), 0, c->stream, A); }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h.data(), d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int hits = 0;
    const int rg = init_guard_hits(c, owner, &hits);
    if (rg) return rg;
    if (hits) return fail(c, VPL_E_HIP, "relpose: guard behind " + std::to_string(hits) + " device array(s) overwritten");
    return VPL_OK;
  };
  const int rc = run();
  dfree_owner(c, owner);
  if (rc) return rc;
  std::memcpy(out, h.data(), (size_t)n * sizeof(vpl_relpose_result));
  if (mask_ransac) std::memcpy(mask_ransac, h.data() + o_m0, n_mask);
  if (mask_pose) std::memcpy(mask_pose, h.data() + o_m1, n_mask);
  if (hyp_count) std::memcpy(hyp_count, h.data() + o_hyp, n_hyp * 4);
  return VPL_OK;
}

int vpl_init_visual_batch(vpl_ctx* c, int n, const vpl_sfm_input* in, const unsigned long long* seeds, vpl_relpose_result* rel,
                          vpl_sfm_result* out, double* points_chain, double* points_ba, int* tracked_id, double* tracked_xyz) {
  if (!c || n < 0 || !in || !seeds || !rel || !out) return VPL_E_INVALID;
  if (n == 0) return VPL_OK;
  if (n > c->maxW) return fail(c, VPL_E_CAPACITY, "visual: more sequences than max_windows");
  for (int s = 0; s < n; ++s) {   // what the structure call would refuse is refused before the relative pose runs
    vpl_sfm_input q = in[s];
    q.l = 0;
    std::string msg;
    const int rc = sfm_check_input(q, msg);
    if (rc) return fail(c, rc, msg + " (sequence " + std::to_string(s) + ")");
  }
  std::vector<vpl_relpose_input> ri(n);
  for (int s = 0; s < n; ++s) ri[s] = vpl_relpose_input{in[s].n_tracks, in[s].track_start, in[s].track_nobs, in[s].track_obs, seeds[s]};
  int rc = vpl_init_relative_pose_batch(c, n, ri.data(), rel, nullptr, nullptr, nullptr);
  if (rc) return rc;
  // the sequences that go on, with what relativePose found
  std::vector<vpl_sfm_input> si;
  std::vector<int> at;
  for (int s = 0; s < n; ++s) {
    if (!rel[s].ok) continue;
    vpl_sfm_input q = in[s];
    q.l = rel[s].l;
    std::memcpy(q.relative_R, rel[s].relative_R, sizeof q.relative_R);
    std::memcpy(q.relative_T, rel[s].relative_T, sizeof q.relative_T);
    si.push_back(q);
    at.push_back(s);
  }
  const int m = (int)si.size();
  const size_t per = (size_t)VPL_SFM_MAX_TRACKS * 3;
  std::vector<vpl_sfm_result> so(m);
  std::vector<double> pc(points_chain ? m * per : 0), pb(points_ba ? m * per : 0), tx(tracked_xyz ? m * per : 0);
  std::vector<int> ti(tracked_id ? (size_t)m * VPL_SFM_MAX_TRACKS : 0);
  if (m) {
    rc = vpl_init_structure_batch(c, m, si.data(), so.data(), points_chain ? pc.data() : nullptr, points_ba ? pb.data() : nullptr,
                                  tracked_id ? ti.data() : nullptr, tracked_xyz ? tx.data() : nullptr);
    if (rc) return rc;
  }
  std::memset(out, 0, (size_t)n * sizeof(vpl_sfm_result));
  if (points_chain) std::memset(points_chain, 0, n * per * 8);
  if (points_ba) std::memset(points_ba, 0, n * per * 8);
  if (tracked_xyz) std::memset(tracked_xyz, 0, n * per * 8);
  if (tracked_id) std::memset(tracked_id, 0, (size_t)n * VPL_SFM_MAX_TRACKS * 4);
  for (int s = 0; s < n; ++s) out[s].fail = VPL_SFM_FAIL_RELATIVE_POSE;
  for (int k = 0; k < m; ++k) {
    const int s = at[k];
    out[s] = so[k];
    if (points_chain) std::memcpy(points_chain + s * per, pc.data() + k * per, per * 8);
    if (points_ba) std::memcpy(points_ba + s * per, pb.data() + k * per, per * 8);
    if (tracked_xyz) std::memcpy(tracked_xyz + s * per, tx.data() + k * per, per * 8);
    if (tracked_id) std::memcpy(tracked_id + (size_t)s * VPL_SFM_MAX_TRACKS, ti.data() + (size_t)k * VPL_SFM_MAX_TRACKS, (size_t)VPL_SFM_MAX_TRACKS * 4);
  }
  return VPL_OK;
}

}  // extern "C"
