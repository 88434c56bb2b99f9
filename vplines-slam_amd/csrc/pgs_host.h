// Host side of the pose-graph session (vpl_pgs_*): PoseGraph's keyframe list resident on the device.  The integers stay here
// (pgs_plan.h), the doubles on the device (pgs_kernels.h); a call of vpl_pgs_optimize uploads one graph's integer block, never
// poses.  Included once by vplines_ba.hip, behind pg_host.h, whose rounds (pg_enqueue_rounds) it runs.
#pragma once
#include "pgs_kernels.h"
#include "pgs_plan.h"

static_assert(vpl::PGS_OK == VPL_OK && vpl::PGS_INVALID == VPL_E_INVALID && vpl::PGS_CAPACITY == VPL_E_CAPACITY, "pgs_plan.h and vplines_ba.h disagree");
static_assert(vpl::PGS_MAX_KEYFRAMES == VPL_PGS_MAX_KEYFRAMES, "pgs_plan.h and vplines_ba.h disagree");

struct vpl_pgs_session {
  vpl_ctx* c = nullptr;
  vpl_pgs_options opt;
  vpl::PgsPlan plan;
  vpl::PgsList L{};
  int nmax = 0;                      // the most nodes one optimisation can have: min(max_keyframes, VPL_PG_MAX_NODES)
  int cur = 0;                       // which copy of the state is current
  double *d_list = nullptr, *d_st = nullptr, *d_rec = nullptr, *d_in = nullptr, *d_out = nullptr, *d_ws = nullptr;
  size_t ws_cap = 0;                 // doubles d_ws holds (it grows with the largest graph met)
  char* d_small = nullptr;           // the graph and its integer block
  size_t small_bytes = 0;
  const double* st_in() const { return d_st + (size_t)cur * vpl::PGS_STATE; }
  double* st_out() const { return d_st + (size_t)(1 - cur) * vpl::PGS_STATE; }
};

namespace vpl {

static int pgs_guards(vpl_pgs_session* h) {
  int hits = 0;
  const int rg = init_guard_hits(h->c, h, &hits);
  if (rg) return rg;
  if (hits) return fail(h->c, VPL_E_HIP, "pose-graph session: guard behind " + std::to_string(hits) + " device array(s) overwritten");
  return VPL_OK;
}

// the state at the start: w_r_vio = r_drift = I, w_t_vio = t_drift = 0 (pose_graph.cpp:8-19)
static int pgs_upload_state(vpl_pgs_session* h) {
  vpl_ctx* c = h->c;
  double st[2 * PGS_STATE] = {};
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < 3; ++i) { st[k * PGS_STATE + PGS_W_R + 4 * i] = 1.0; st[k * PGS_STATE + PGS_R_DRIFT + 4 * i] = 1.0; }
  HIPCHK(c, hipMemcpyAsync(h->d_st, st, sizeof st, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  h->cur = 0;
  return VPL_OK;
}

// addKeyFrame (load = false) and loadKeyFrame
static int pgs_add_or_load(vpl_pgs_session* h, const vpl_pgs_keyframe* kf, vpl_pgs_keyframe_out* out, bool load) {
  if (!h || !kf) return VPL_E_INVALID;
  vpl_ctx* c = h->c;
  { const int rs = settle(c); if (rs) return rs; }
  PgsAddStep st;
  int rc;
  if (load) rc = pgs_load(h->plan, kf->loop_index, st.index);
  else rc = pgs_add(h->plan, kf->sequence, kf->loop_index, st);
  if (rc == PGS_CAPACITY) return fail(c, rc, "pose-graph session: max_keyframes reached");
  if (rc) return fail(c, rc, load ? "pose-graph session: loop_index outside 0 .. index - 1"
                                  : "pose-graph session: sequence not sequence_cnt or sequence_cnt + 1, or loop_index outside 0 .. index - 1");
  HIPCHK(c, hipSetDevice(c->device));
  PgsAddArgs A;
  A.L = h->L; A.st_in = h->st_in(); A.st_out = h->st_out(); A.out = out ? h->d_rec : nullptr;
  A.index = st.index; A.sequence = load ? 0 : kf->sequence; A.loop_index = kf->loop_index;
  A.new_sequence = st.new_sequence; A.shift_list = st.shift_list; A.load = load ? 1 : 0;
  std::memcpy(A.vio_T, kf->vio_T, sizeof A.vio_T); std::memcpy(A.vio_R, kf->vio_R, sizeof A.vio_R);
  std::memcpy(A.T, kf->T, sizeof A.T); std::memcpy(A.R, kf->R, sizeof A.R);
  std::memcpy(A.loop_info, kf->loop_info, sizeof A.loop_info);
  const int lanes = st.shift_list ? std::max(st.index, 1) : 1;
  { KTimer t(c, "k_pgs_add"); hipLaunchKernelGGL(k_pgs_add, dim3((lanes + PGS_THREADS - 1) / PGS_THREADS), dim3(PGS_THREADS), 0, c->stream, A); }
  HIPCHK(c, hipGetLastError());
  h->cur = 1 - h->cur;
  if (!out) return VPL_OK;
  double rec[PGS_OUT];
  HIPCHK(c, hipMemcpyAsync(rec, h->d_rec, sizeof rec, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  { const int rg = pgs_guards(h); if (rg) return rg; }
  out->index = st.index; out->optimize_pending = h->plan.pending >= 0 ? 1 : 0;
  std::memcpy(out->vio_T, rec, 3 * 8); std::memcpy(out->vio_R, rec + 3, 9 * 8); std::memcpy(out->T, rec + 12, 3 * 8);
  std::memcpy(out->R, rec + 15, 9 * 8); std::memcpy(out->w_r_vio, rec + 24, 9 * 8); std::memcpy(out->w_t_vio, rec + 33, 3 * 8);
  return VPL_OK;
}

}  // namespace vpl

extern "C" {

void vpl_pgs_default_options(vpl_pgs_options* o) {
  if (!o) return;
  o->max_keyframes = 8192; o->fast_relocalization = 0;
  vpl_pg_default_options(&o->pg);
}

int vpl_pgs_create(vpl_ctx* c, const vpl_pgs_options* opt, vpl_pgs_session** out) {
  if (!c || !opt || !out) return VPL_E_INVALID;
  if (opt->max_keyframes < 1) return vpl::fail(c, VPL_E_INVALID, "pose-graph session: max_keyframes < 1");
  if (opt->max_keyframes > VPL_PGS_MAX_KEYFRAMES) return vpl::fail(c, VPL_E_CAPACITY, "pose-graph session: more than VPL_PGS_MAX_KEYFRAMES keyframes");
  if (!vpl::pg_options_ok(&opt->pg)) return vpl::fail(c, VPL_E_INVALID, "pose-graph session: options out of range");
  { const int rs = settle(c); if (rs) return rs; }
  vpl_pgs_session* h = new vpl_pgs_session();
  h->c = c; h->opt = *opt; h->plan.cap = opt->max_keyframes;
  h->nmax = std::min(opt->max_keyframes, VPL_PG_MAX_NODES);
  const size_t cap = (size_t)opt->max_keyframes, nmax = (size_t)h->nmax;
  const vpl::PgLayout big = vpl::pg_layout(h->nmax, VPL_PG_MAX_LOOPS);
  h->small_bytes = 64 * ((sizeof(vpl::PgGraph) + 63) / 64) + (big.itotal + vpl::pg_up8(nmax)) * 4;
  hipError_t e = hipSetDevice(c->device);
  if (e == hipSuccess) e = vpl::dalloc(c, &h->d_list, 32 * cap, h);
  if (e == hipSuccess) e = vpl::dalloc(c, &h->L.seq, cap, h);
  if (e == hipSuccess) e = vpl::dalloc(c, &h->d_st, (size_t)2 * vpl::PGS_STATE, h);
  if (e == hipSuccess) e = vpl::dalloc(c, &h->d_rec, (size_t)vpl::PGS_OUT, h);
  if (e == hipSuccess) e = vpl::dalloc(c, &h->d_in, vpl::pg_up8(12 * nmax + 4 * (size_t)VPL_PG_MAX_LOOPS), h);
  if (e == hipSuccess) e = vpl::dalloc(c, &h->d_out, vpl::pg_up8(vpl::PG_HEAD + 12 * nmax), h);
  if (e == hipSuccess) e = vpl::dalloc(c, &h->d_small, h->small_bytes, h);
  int rc = e == hipSuccess ? VPL_OK : vpl::fail(c, VPL_E_HIP, "pose-graph session: device allocation failed");
  if (!rc) {
    h->L.vT = h->d_list; h->L.vR = h->d_list + 3 * cap; h->L.T = h->d_list + 12 * cap; h->L.R = h->d_list + 15 * cap; h->L.li = h->d_list + 24 * cap;
    rc = vpl::pgs_upload_state(h);
  }
  if (rc) {
    vpl::dfree_owner(c, h);
    delete h;
    return rc;
  }
  *out = h;
  return VPL_OK;
}

void vpl_pgs_destroy(vpl_pgs_session* h) {
  if (!h) return;
  (void)hipSetDevice(h->c->device);
  (void)hipStreamSynchronize(h->c->stream);   // (teardown: a failure has nobody to be reported to)
  vpl::dfree_owner(h->c, h);
  delete h;
}

int vpl_pgs_reset(vpl_pgs_session* h) {
  if (!h) return VPL_E_INVALID;
  { const int rs = settle(h->c); if (rs) return rs; }
  HIPCHK(h->c, hipSetDevice(h->c->device));
  HIPCHK(h->c, hipStreamSynchronize(h->c->stream));
  vpl::pgs_reset(h->plan);
  return vpl::pgs_upload_state(h);
}

int vpl_pgs_size(const vpl_pgs_session* h) { return h ? h->plan.size() : VPL_E_INVALID; }

int vpl_pgs_add_keyframe(vpl_pgs_session* h, const vpl_pgs_keyframe* kf, vpl_pgs_keyframe_out* out) {
  return vpl::pgs_add_or_load(h, kf, out, false);
}

int vpl_pgs_load_keyframe(vpl_pgs_session* h, const vpl_pgs_keyframe* kf, vpl_pgs_keyframe_out* out) {
  return vpl::pgs_add_or_load(h, kf, out, true);
}

int vpl_pgs_optimize(vpl_pgs_session* h, vpl_pgs_result* result) {
  using namespace vpl;
  if (!h || !result) return VPL_E_INVALID;
  vpl_ctx* c = h->c;
  { const int rs = settle(c); if (rs) return rs; }
  std::memset(result, 0, sizeof *result);
  result->first_index = -1; result->cur_index = -1;
  int first = -1, cur = -1;
  std::vector<int> li, la;
  const int took = pgs_take(h->plan, first, cur, li, la);
  if (took == PGS_CAPACITY) return fail(c, VPL_E_CAPACITY, "pose-graph session: more than VPL_PG_MAX_NODES nodes or VPL_PG_MAX_LOOPS loops between the earliest loop and the last queued keyframe");
  if (took == 0) { result->status = VPL_PGS_NOTHING; return VPL_OK; }
  const int n = cur - first + 1;
  PgGraph G{};
  G.p = pg_layout(n, (int)li.size());
  G.n_tail = 0; G.run = 1;
  const size_t b_int = 64 * ((sizeof(PgGraph) + 63) / 64), bytes = b_int + (G.p.itotal + pg_up8((size_t)n)) * 4;
  if (bytes > h->small_bytes) return fail(c, VPL_E_CAPACITY, "pose-graph session: integer block larger than planned");
  std::vector<char> buf(bytes, 0);
  std::memcpy(buf.data(), &G, sizeof G);
  int* ints = (int*)(buf.data() + b_int);
  pg_fill_ints(G.p, li.data(), la.data(), ints);
  pg_node_flags(n, h->plan.seq.data() + first, G.p.L, li.data(), la.data(), ints + G.p.itotal);
  HIPCHK(c, hipSetDevice(c->device));
  if (G.p.total > h->ws_cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    dfree(c, h->d_ws);
    h->d_ws = nullptr; h->ws_cap = 0;
    HIPCHK(c, dalloc(c, &h->d_ws, G.p.total, h));
    h->ws_cap = G.p.total;
  }
  const size_t outs = PG_HEAD + 12 * (size_t)n;
  HIPCHK(c, hipMemsetAsync(h->d_ws, 0, G.p.total * 8, c->stream));
  HIPCHK(c, hipMemsetAsync(h->d_out, 0, outs * 8, c->stream));
  HIPCHK(c, hipMemcpyAsync(h->d_small, buf.data(), bytes, hipMemcpyHostToDevice, c->stream));
  PgsTurnArgs T;
  T.L = h->L; T.st_in = h->st_in(); T.st_out = h->st_out(); T.first = first; T.size = h->plan.size();
  T.pg.gr = (const PgGraph*)h->d_small; T.pg.ws = h->d_ws; T.pg.ints = (const int*)(h->d_small + b_int); T.pg.in = h->d_in; T.pg.out = h->d_out;
  T.pg.opt = h->opt.pg;
  PgDims dims;
  dims.n_graphs = 1; dims.maxE = std::max(1, G.p.E); dims.maxn = n; dims.maxnb = std::max(1, G.p.nb); dims.maxLP = G.p.LP;
  { KTimer t(c, "k_pgs_gather"); hipLaunchKernelGGL(k_pgs_gather, dim3((std::max(n, G.p.L) + PGS_THREADS - 1) / PGS_THREADS), dim3(PGS_THREADS), 0, c->stream, T); }
  pg_enqueue_rounds<true>(c, T.pg, dims, false);
  { KTimer t(c, "k_pg_finish"); hipLaunchKernelGGL(k_pg_finish, dim3(1, 1), dim3(PG_THREADS), 0, c->stream, T.pg); }
  { KTimer t(c, "k_pgs_scatter"); hipLaunchKernelGGL(k_pgs_scatter, dim3((T.size - first + PGS_THREADS - 1) / PGS_THREADS), dim3(PGS_THREADS), 0, c->stream, T); }
  HIPCHK(c, hipGetLastError());
  h->cur = 1 - h->cur;
  double o[PG_HEAD];
  HIPCHK(c, hipMemcpyAsync(o, h->d_out, sizeof o, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  { const int rg = pgs_guards(h); if (rg) return rg; }
  result->status = VPL_PGS_OK; result->termination = (int)o[1]; result->iterations = (int)o[2]; result->successful_steps = (int)o[3];
  result->unsuccessful_steps = (int)o[4]; result->n_nodes = n; result->first_index = first; result->cur_index = cur;
  result->initial_cost = o[5]; result->final_cost = o[6]; result->yaw_drift = o[7];
  std::memcpy(result->r_drift, o + 8, 9 * 8); std::memcpy(result->t_drift, o + 17, 3 * 8);
  return VPL_OK;
}

int vpl_pgs_update_loop(vpl_pgs_session* h, int index, const double* loop_info, int* accepted) {
  using namespace vpl;
  if (!h || !loop_info) return VPL_E_INVALID;
  vpl_ctx* c = h->c;
  if (index < 0 || index >= h->plan.size() || h->plan.loop_index[index] < 0)
    return fail(c, VPL_E_INVALID, "pose-graph session: update_loop of a keyframe that is not there or has no loop");
  { const int rs = settle(c); if (rs) return rs; }
  // KeyFrame::updateLoop's gate (keyframe.cpp:571-578), which is updateKeyFrameLoop's too (:893)
  const double t2 = loop_info[0] * loop_info[0] + loop_info[1] * loop_info[1] + loop_info[2] * loop_info[2];
  const bool ok = std::fabs(loop_info[7]) < 30.0 && std::sqrt(t2) < 20.0;
  if (accepted) *accepted = ok ? 1 : 0;
  if (!ok) return VPL_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PgsLoopArgs A;
  A.L = h->L; A.st_in = h->st_in(); A.st_out = h->st_out(); A.index = index; A.old_index = h->plan.loop_index[index];
  A.fast = h->opt.fast_relocalization ? 1 : 0;
  std::memcpy(A.loop_info, loop_info, sizeof A.loop_info);
  { KTimer t(c, "k_pgs_update_loop"); hipLaunchKernelGGL(k_pgs_update_loop, dim3(1), dim3(64), 0, c->stream, A); }
  HIPCHK(c, hipGetLastError());
  h->cur = 1 - h->cur;
  return VPL_OK;
}

int vpl_pgs_get_path(vpl_pgs_session* h, int first, int count, double* T, double* R, double* vio_T, double* vio_R, double* loop_info,
                     int* sequence, int* loop_index) {
  if (!h || first < 0 || count < 0) return VPL_E_INVALID;
  vpl_ctx* c = h->c;
  if ((long long)first + count > h->plan.size()) return vpl::fail(c, VPL_E_INVALID, "pose-graph session: path range beyond the last keyframe");
  if (!count) return VPL_OK;
  const size_t a = (size_t)first, n = (size_t)count;
  if (sequence) std::memcpy(sequence, h->plan.seq.data() + a, n * sizeof(int));
  if (loop_index) std::memcpy(loop_index, h->plan.loop_index.data() + a, n * sizeof(int));
  if (!T && !R && !vio_T && !vio_R && !loop_info) return VPL_OK;
  { const int rs = settle(c); if (rs) return rs; }
  HIPCHK(c, hipSetDevice(c->device));
  if (T) HIPCHK(c, hipMemcpyAsync(T, h->L.T + 3 * a, 3 * n * 8, hipMemcpyDeviceToHost, c->stream));
  if (R) HIPCHK(c, hipMemcpyAsync(R, h->L.R + 9 * a, 9 * n * 8, hipMemcpyDeviceToHost, c->stream));
  if (vio_T) HIPCHK(c, hipMemcpyAsync(vio_T, h->L.vT + 3 * a, 3 * n * 8, hipMemcpyDeviceToHost, c->stream));
  if (vio_R) HIPCHK(c, hipMemcpyAsync(vio_R, h->L.vR + 9 * a, 9 * n * 8, hipMemcpyDeviceToHost, c->stream));
  if (loop_info) HIPCHK(c, hipMemcpyAsync(loop_info, h->L.li + 8 * a, 8 * n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VPL_OK;
}

int vpl_pgs_get_drift(vpl_pgs_session* h, double* yaw_drift, double* r_drift, double* t_drift) {
  if (!h || !yaw_drift || !r_drift || !t_drift) return VPL_E_INVALID;
  vpl_ctx* c = h->c;
  { const int rs = settle(c); if (rs) return rs; }
  HIPCHK(c, hipSetDevice(c->device));
  double st[vpl::PGS_STATE];
  HIPCHK(c, hipMemcpyAsync(st, h->st_in(), sizeof st, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *yaw_drift = st[vpl::PGS_YAW_DRIFT];
  std::memcpy(r_drift, st + vpl::PGS_R_DRIFT, 9 * 8); std::memcpy(t_drift, st + vpl::PGS_T_DRIFT, 3 * 8);
  return VPL_OK;
}

}  // extern "C"
