// Host side of the feature selector (vpl_select_features_batch, vpl_select_debug_values, vpl_select_stats, vpl_sel_debug_book):
// the refusals, the one packed upload, the three launches and the one read-back.  Included once by vplines_ba.hip, behind
// init_relpose_host.h.  vpl_odo_select (ba_session.h) runs the same sel_run with a fourth launch in front, k_sel_cloud.
#pragma once
#include "sel_kernels.h"
#include "sel_book.h"

// vpl_odo_select: the store the cloud and state k are gathered from (k_sel_cloud), and the table that says which tracks
struct SelGather {
  DevSelGather G;
  std::vector<int> tab;
};

// the refusals of one sequence, before anything is allocated.  gathered: the cloud is the session's, q.cloud is not read
static int sel_check_input(const vpl_sel_input& q, bool gathered, std::string& msg) {
  if (q.n_new < 0 || q.n_used < 0 || q.n_cloud < 0 || q.kappa < 0) { msg = "select: negative count"; return VPL_E_INVALID; }
  if (q.n_new > VPL_SEL_MAX_FEATURES || q.n_used > VPL_SEL_MAX_FEATURES || q.n_cloud > VPL_SEL_MAX_FEATURES) {
    msg = "select: a list longer than VPL_SEL_MAX_FEATURES";
    return VPL_E_CAPACITY;
  }
  if ((q.n_new && (!q.new_id || !q.new_x || !q.new_y || !q.new_prob)) || (q.n_used && (!q.used_x || !q.used_y)) || (q.n_cloud && !q.cloud && !gathered)) {
    msg = "select: null array";
    return VPL_E_INVALID;
  }
  if (q.n_imu < 1) { msg = "select: n_imu < 1"; return VPL_E_INVALID; }
  if (!(q.delta_imu > 0.0)) { msg = "select: delta_imu is not > 0"; return VPL_E_INVALID; }
  std::vector<int> ids(q.new_id, q.new_id + q.n_new);        // the collapse rule and the forced prefix tell candidates apart by id
  std::sort(ids.begin(), ids.end());
  if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) { msg = "select: new_id holds an id twice"; return VPL_E_INVALID; }
  return VPL_OK;
}

// what the two entry points share.  dbg: one sequence, a forced prefix, one round's values
struct SelDebug {
  const int* prefix_id;
  int n_prefix;
  double *f, *ub, *omega, *d12;
};
static int sel_run(vpl_ctx* c, int n, const vpl_sel_params* par, const vpl_sel_input* in, vpl_sel_result* out, int* selected_id,
                   double* round_f, const SelDebug* dbg, const SelGather* gs = nullptr) {
  if (n == 0) return VPL_OK;
  if (n > c->maxW) return fail(c, VPL_E_CAPACITY, "select: more sequences than max_windows");
  if (par->width < 1 || par->height < 1) return fail(c, VPL_E_INVALID, "select: image size");
  for (int s = 0; s < n; ++s) {
    std::string msg;
    const int rc = sel_check_input(in[s], gs != nullptr, msg);
    if (rc) return fail(c, rc, msg + " (sequence " + std::to_string(s) + ")");
  }
  const int rs = settle(c);
  if (rs) return rs;
  // ---- the tables: per sequence its record; the features of the whole batch (new, then used) side by side; the clouds
  std::vector<DevSelSeq> seqs(n);
  std::vector<double> fx, fy, fp, cloud;
  std::vector<int> fid, itab;
  int max_nf = 0;
  for (int s = 0; s < n; ++s) {
    const vpl_sel_input& q = in[s];
    DevSelSeq d{};
    double* st = d.st;
    auto put = [&](const double* p, int k) { std::memcpy(st, p, k * 8); st += k; };
    put(q.P0, 3); put(q.Q0, 4); put(q.V0, 3); put(q.Ba0, 3); put(q.P1, 3); put(q.Q1, 4); put(q.V1, 3); put(q.Ba1, 3);
    put(q.acc, 3); put(q.gyr, 3); put(&q.delta_imu, 1);
    d.has_hz = q.horizon ? 1 : 0;
    if (q.horizon) std::memcpy(d.hz, q.horizon, sizeof d.hz);
    d.n_imu = q.n_imu; d.kappa = q.kappa; d.n_new = q.n_new; d.n_used = q.n_used; d.n_cloud = q.n_cloud;
    d.feat0 = (int)fx.size();
    d.cloud0 = (int)cloud.size() / 3;
    d.prefix0 = (int)itab.size();
    d.n_prefix = dbg ? dbg->n_prefix : 0;
    if (dbg && dbg->n_prefix) itab.insert(itab.end(), dbg->prefix_id, dbg->prefix_id + dbg->n_prefix);
    fx.insert(fx.end(), q.new_x, q.new_x + q.n_new); fx.insert(fx.end(), q.used_x, q.used_x + q.n_used);
    fy.insert(fy.end(), q.new_y, q.new_y + q.n_new); fy.insert(fy.end(), q.used_y, q.used_y + q.n_used);
    fp.insert(fp.end(), q.new_prob, q.new_prob + q.n_new); fp.insert(fp.end(), q.n_used, 0.0);
    fid.insert(fid.end(), q.new_id, q.new_id + q.n_new); fid.insert(fid.end(), q.n_used, -1);
    if (q.n_cloud && gs) cloud.resize(cloud.size() + 3 * (size_t)q.n_cloud, 0.0);      // k_sel_cloud fills it
    else if (q.n_cloud) cloud.insert(cloud.end(), q.cloud, q.cloud + 3 * (size_t)q.n_cloud);
    max_nf = std::max(max_nf, q.n_new + q.n_used);
    seqs[s] = d;
  }
  const size_t F = fx.size(), Fa = std::max<size_t>(F, 1);
  // ---- the packed upload: x | y | prob | cloud | sequences | ids | prefixes | the session's gather table
  auto up64 = [](size_t b) { return (b + 63) & ~(size_t)63; };
  const size_t b_y = up64(Fa * 8), b_p = up64(b_y + Fa * 8), b_cl = up64(b_p + Fa * 8), b_seq = up64(b_cl + std::max<size_t>(cloud.size(), 1) * 8),
               b_id = up64(b_seq + seqs.size() * sizeof(DevSelSeq)), b_it = up64(b_id + Fa * 4), b_gt = up64(b_it + std::max<size_t>(itab.size(), 1) * 4), bytes = b_gt + (gs ? gs->tab.size() * 4 : 0);
  std::vector<char> buf(bytes, 0);
  if (F) {
    std::memcpy(buf.data(), fx.data(), F * 8);
    std::memcpy(buf.data() + b_y, fy.data(), F * 8);
    std::memcpy(buf.data() + b_p, fp.data(), F * 8);
    std::memcpy(buf.data() + b_id, fid.data(), F * 4);
  }
  if (!cloud.empty()) std::memcpy(buf.data() + b_cl, cloud.data(), cloud.size() * 8);
  std::memcpy(buf.data() + b_seq, seqs.data(), seqs.size() * sizeof(DevSelSeq));
  if (!itab.empty()) std::memcpy(buf.data() + b_it, itab.data(), itab.size() * 4);
  if (gs && !gs->tab.empty()) std::memcpy(buf.data() + b_gt, gs->tab.data(), gs->tab.size() * 4);
  // ---- the read-back: results | ids | f  (debug: f | ub | Omega_kkH | Delta12 instead)
  const size_t o_id = up64((size_t)n * sizeof(vpl_sel_result)), o_f = up64(o_id + (size_t)n * VPL_SEL_MAX_FEATURES * 4),
               o_end = o_f + (size_t)n * VPL_SEL_MAX_FEATURES * 8;
  const size_t g_ub = up64(Fa * 8), g_end = g_ub + Fa * 8;                 // debug values, in an array of their own
  const void* owner = &seqs;
  char *d_in = nullptr, *d_out = nullptr, *d_dbg = nullptr;
  double *d_work = nullptr, *d_omega = nullptr, *d_d12 = nullptr;
  int* d_vis = nullptr;
  std::vector<char> h(o_end), hg(dbg ? g_end : 0);
  std::vector<double> h_d12(dbg && dbg->d12 ? Fa * SEL_TRI : 0);
  long long down = 0, launches = 0;
  auto run = [&]() -> int {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, dalloc(c, &d_in, bytes, owner));
    HIPCHK(c, dalloc(c, &d_out, o_end, owner));
    HIPCHK(c, dalloc(c, &d_work, (size_t)n * SEL_WORK, owner));
    HIPCHK(c, dalloc(c, &d_omega, (size_t)n * SEL_N * SEL_N, owner));
    HIPCHK(c, dalloc(c, &d_d12, Fa * SEL_TRI, owner));
    HIPCHK(c, dalloc(c, &d_vis, Fa, owner));
    if (dbg) HIPCHK(c, dalloc(c, &d_dbg, g_end, owner));
    // (the allocator's zeroing runs on the null stream: what the kernels rely on is set again in stream order)
    HIPCHK(c, hipMemsetAsync(d_out, 0, o_end, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_in, buf.data(), bytes, hipMemcpyHostToDevice, c->stream));
    DevSelArgs A{};
    A.par = *par;
    A.fx = (const double*)d_in; A.fy = (const double*)(d_in + b_y); A.fp = (const double*)(d_in + b_p);
    A.cloud = (const double*)(d_in + b_cl);
    A.seqs = (const DevSelSeq*)(d_in + b_seq);
    A.fid = (const int*)(d_in + b_id);
    A.itab = (const int*)(d_in + b_it);
    A.ftot = (int)Fa;
    A.work = d_work; A.omega = d_omega; A.d12 = d_d12; A.vis = d_vis;
    A.res = (vpl_sel_result*)d_out;
    A.sel_id = (int*)(d_out + o_id);
    A.sel_f = (double*)(d_out + o_f);
    A.dbg_f = dbg ? (double*)d_dbg : nullptr;
    A.dbg_ub = dbg ? (double*)(d_dbg + g_ub) : nullptr;
    A.debug = dbg ? 1 : 0;
    if (gs) {
      DevSelGather G = gs->G;
      G.tab = (const int*)(d_in + b_gt);
      KTimer t(c, "k_sel_cloud");
      hipLaunchKernelGGL(k_sel_cloud, dim3(n), dim3(SEL_CLOUD_THREADS), 0, c->stream, A, G, (DevSelSeq*)(d_in + b_seq), (double*)(d_in + b_cl));
      ++launches;
    }
    { KTimer t(c, "k_sel_prep"); hipLaunchKernelGGL(k_sel_prep, dim3(n), dim3(SEL_PREP_THREADS), 0, c->stream, A); ++launches; }
    { KTimer t(c, "k_sel_info");
      hipLaunchKernelGGL(k_sel_info, dim3(std::max(1, (max_nf + SEL_INFO_THREADS - 1) / SEL_INFO_THREADS), n), dim3(SEL_INFO_THREADS), 0, c->stream, A);
      ++launches; }
    { KTimer t(c, "k_sel_greedy"); hipLaunchKernelGGL(k_sel_greedy, dim3(n), dim3(SEL_GREEDY_THREADS), 0, c->stream, A); ++launches; }
    HIPCHK(c, hipGetLastError());
    if (!dbg) {
      HIPCHK(c, hipMemcpyAsync(h.data(), d_out, o_end, hipMemcpyDeviceToHost, c->stream));
      down += (long long)o_end;
    } else {
      HIPCHK(c, hipMemcpyAsync(hg.data(), d_dbg, g_end, hipMemcpyDeviceToHost, c->stream));
      down += (long long)g_end;
      if (dbg->omega) { HIPCHK(c, hipMemcpyAsync(dbg->omega, d_omega, SEL_N * SEL_N * 8, hipMemcpyDeviceToHost, c->stream)); down += SEL_N * SEL_N * 8; }
      if (dbg->d12) { HIPCHK(c, hipMemcpyAsync(h_d12.data(), d_d12, h_d12.size() * 8, hipMemcpyDeviceToHost, c->stream)); down += (long long)h_d12.size() * 8; }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int hits = 0;
    const int rg = init_guard_hits(c, owner, &hits);
    if (rg) return rg;
    if (hits) return fail(c, VPL_E_HIP, "select: guard behind " + std::to_string(hits) + " device array(s) overwritten");
    return VPL_OK;
  };
  const int rc = run();
  dfree_owner(c, owner);
  if (rc) return rc;
  c->sel_stats[0] = launches; c->sel_stats[1] = (long long)bytes; c->sel_stats[2] = down;
  if (!dbg) {
    std::memcpy(out, h.data(), (size_t)n * sizeof(vpl_sel_result));
    std::memcpy(selected_id, h.data() + o_id, (size_t)n * VPL_SEL_MAX_FEATURES * 4);
    std::memcpy(round_f, h.data() + o_f, (size_t)n * VPL_SEL_MAX_FEATURES * 8);
  } else {
    const int nn = in[0].n_new;
    if (dbg->f && nn) std::memcpy(dbg->f, hg.data(), (size_t)nn * 8);
    if (dbg->ub && nn) std::memcpy(dbg->ub, hg.data() + g_ub, (size_t)nn * 8);
    if (dbg->d12)      // the device keeps entry e of every feature side by side: feature after feature for the caller
      for (size_t g = 0; g < F; ++g)
        for (int e = 0; e < SEL_TRI; ++e) dbg->d12[g * SEL_TRI + e] = h_d12[(size_t)e * Fa + g];
  }
  return VPL_OK;
}

extern "C" {

int vpl_select_features_batch(vpl_ctx* c, int n, const vpl_sel_params* par, const vpl_sel_input* in, vpl_sel_result* out, int* selected_id,
                              double* round_f) {
  if (!c || n < 0 || !par || !in || !out || !selected_id || !round_f) return VPL_E_INVALID;
  return sel_run(c, n, par, in, out, selected_id, round_f, nullptr);
}

int vpl_select_debug_values(vpl_ctx* c, const vpl_sel_params* par, const vpl_sel_input* in, const int* prefix_id, int n_prefix, double* f,
                            double* ub, double* omega45x45, double* delta12) {
  if (!c || !par || !in || n_prefix < 0 || (n_prefix && !prefix_id)) return VPL_E_INVALID;
  if (n_prefix > VPL_SEL_MAX_FEATURES) return fail(c, VPL_E_CAPACITY, "select: a prefix longer than VPL_SEL_MAX_FEATURES");
  const SelDebug dbg{prefix_id, n_prefix, f, ub, omega45x45, delta12};
  return sel_run(c, 1, par, in, nullptr, nullptr, nullptr, &dbg);
}

int vpl_select_stats(vpl_ctx* c, long long* launches, long long* h2d_bytes, long long* d2h_bytes) {
  if (!c || !launches || !h2d_bytes || !d2h_bytes) return VPL_E_INVALID;
  *launches = c->sel_stats[0];
  *h2d_bytes = c->sel_stats[1];
  *d2h_bytes = c->sel_stats[2];
  return VPL_OK;
}

int vpl_sel_debug_book(int max_features, int init_thresh, int n_images, const int* n_ids, const int* ids, const unsigned char* initialized,
                       const int* n_offer, const int* offer, int max_ids, int* n_new, int* kappa, int* n_selected, int* selected,
                       int* n_out, int* out_ids, int* n_tracked, int* last_id, int max_tracked, int* tracked) {
  return sel_book_replay(max_features, init_thresh, n_images, n_ids, ids, initialized, n_offer, offer, max_ids, n_new, kappa, n_selected,
                         selected, n_out, out_ids, n_tracked, last_id, max_tracked, tracked);
}

}  // extern "C"
