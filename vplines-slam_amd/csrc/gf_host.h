// Host side of the global fusion (vpl_gf_optimize_batch, vpl_gf_debug_step, vpl_gf_debug_plan, vpl_gf_local_cartesian): the
// refusals, one plan per chain (gf_plan.h), the one packed upload, the rounds enqueued without a look at the device, the one
// read-back; and the session (vpl_gf_create .. vpl_gf_destroy) that runs the same launches on arrays it keeps on the device.
// Included once by vplines_ba.hip, behind pg_host.h.
#pragma once
#include "gf_kernels.h"

static_assert(vpl::GF_MAX_NODES == VPL_GF_MAX_NODES, "gf_plan.h and vplines_ba.h disagree");

extern "C" {

void vpl_gf_default_options(vpl_gf_options* o) {
  if (!o) return;
  o->max_iterations = 5; o->max_consecutive_invalid_steps = 5; o->segment = 0; o->reserved = 0;
  o->t_var = 0.1; o->q_var = 0.01; o->huber_delta = 1.0;
  o->initial_radius = 1e4; o->max_radius = 1e16; o->min_radius = 1e-32; o->min_relative_decrease = 1e-3;
  o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
  o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32;
}

}  // extern "C"

namespace vpl {

struct GfDebugOut { double *g, *step, *model; };

static bool gf_segment_ok(int segment) { return segment == 0 || segment >= 2; }
static int gf_segment(int segment) { return segment == 0 ? GF_DEFAULT_SEGMENT : segment; }

// the launches of one call on the context's stream: the start, `rounds` rounds, and (finish) the result
static void gf_enqueue(vpl_ctx* c, const GfArgs& A, int n, int maxn, int maxseg, int maxsep, int rounds, bool finish) {
  const dim3 one(1, n), per_node((maxn + GF_THREADS - 1) / GF_THREADS, n), per_seg((maxseg + 63) / 64, n),
      per_item((std::max(maxsep, 1) * GF_SCHUR_ITEMS + GF_THREADS - 1) / GF_THREADS, n);
  hipStream_t st = c->stream;
  { KTimer t(c, "k_gf_init"); hipLaunchKernelGGL(k_gf_init, per_node, dim3(GF_THREADS), 0, st, A); }
  for (int it = 0; it < rounds; ++it) {
    { KTimer t(c, "k_gf_lin"); hipLaunchKernelGGL(k_gf_edges<0>, per_node, dim3(GF_THREADS), 0, st, A);
      hipLaunchKernelGGL(k_gf_asm, per_node, dim3(GF_THREADS), 0, st, A);
      hipLaunchKernelGGL(k_gf_head, one, dim3(GF_THREADS), 0, st, A); }
    { KTimer t(c, "k_gf_seg_factor"); hipLaunchKernelGGL(k_gf_seg_factor, per_seg, dim3(64), 0, st, A); }
    if (maxsep) { KTimer t(c, "k_gf_schur"); hipLaunchKernelGGL(k_gf_schur, per_item, dim3(GF_THREADS), 0, st, A); }
    { KTimer t(c, "k_gf_sep"); hipLaunchKernelGGL(k_gf_sep, one, dim3(64), 0, st, A); }
    { KTimer t(c, "k_gf_seg_back"); hipLaunchKernelGGL(k_gf_seg_back, per_seg, dim3(64), 0, st, A); }
    { KTimer t(c, "k_gf_decide"); hipLaunchKernelGGL(k_gf_cand, per_node, dim3(GF_THREADS), 0, st, A);
      hipLaunchKernelGGL(k_gf_edges<1>, per_node, dim3(GF_THREADS), 0, st, A);
      hipLaunchKernelGGL(k_gf_decide, one, dim3(GF_THREADS), 0, st, A); }
  }
  if (finish) { KTimer t(c, "k_gf_finish"); hipLaunchKernelGGL(k_gf_finish, per_node, dim3(GF_THREADS), 0, st, A); }
}

static bool gf_options_ok(const vpl_gf_options* opt) {
  auto pos = [](double v) { return v > 0.0 && std::isfinite(v); };
  return !(opt->max_iterations < 0 || opt->max_iterations > 1000 || opt->max_consecutive_invalid_steps < 1 || !gf_segment_ok(opt->segment) ||
           !pos(opt->t_var) || !pos(opt->q_var) || !std::isfinite(opt->huber_delta) || !pos(opt->initial_radius) || !pos(opt->max_radius) ||
           !(opt->min_radius >= 0.0) || !std::isfinite(opt->min_relative_decrease) || !(opt->function_tolerance >= 0.0) ||
           !(opt->gradient_tolerance >= 0.0) || !(opt->parameter_tolerance >= 0.0) || !pos(opt->min_lm_diagonal) ||
           !(opt->max_lm_diagonal >= opt->min_lm_diagonal));
}
static void gf_read_head(const double* o, vpl_gf_result& r) {
  r.status = (int)o[0]; r.termination = (int)o[1]; r.iterations = (int)o[2]; r.successful_steps = (int)o[3];
  r.unsuccessful_steps = (int)o[4]; r.reserved = 0; r.initial_cost = o[5]; r.final_cost = o[6];
  std::memcpy(r.wgps_T_wvio, o + 8, 16 * 8);
}

// the whole call; dbg: one round of chain 0, then g, step and the model cost change are handed out
static int gf_run(vpl_ctx* c, int n, const vpl_gf_input* in, const vpl_gf_options* opt, vpl_gf_result* out, const GfDebugOut* dbg) {
  if (!c || n < 0 || !in || !opt || (!out && !dbg)) return VPL_E_INVALID;
  if (n == 0) return VPL_OK;
  if (n > c->maxW) return fail(c, VPL_E_CAPACITY, "global fusion: more chains than max_windows");
  auto pos = [](double v) { return v > 0.0 && std::isfinite(v); };
  if (!gf_options_ok(opt)) return fail(c, VPL_E_INVALID, "global fusion: options out of range");
  const int S = gf_segment(opt->segment);
  std::vector<GfChain> ch(n);
  size_t ws = 0, ins = 0, outs = 0;
  int maxn = 1, maxseg = 1, maxsep = 0;
  for (int s = 0; s < n; ++s) {
    const vpl_gf_input& q = in[s];
    const std::string at = " (chain " + std::to_string(s) + ")";
    if (q.n < 1 || q.n_gps < 0 || !q.local || !q.global || (q.n_gps && (!q.gps_node || !q.gps_xyz || !q.gps_accuracy)))
      return fail(c, VPL_E_INVALID, "global fusion: null arrays or bad counts" + at);
    if (out && !out[s].pose) return fail(c, VPL_E_INVALID, "global fusion: null result array" + at);
    if (q.n > VPL_GF_MAX_NODES) return fail(c, VPL_E_CAPACITY, "global fusion: more than VPL_GF_MAX_NODES nodes" + at);
    for (int e = 0; e < q.n_gps; ++e) {
      if (q.gps_node[e] < 0 || q.gps_node[e] >= q.n || (e && q.gps_node[e] <= q.gps_node[e - 1]))
        return fail(c, VPL_E_INVALID, "global fusion: gps_node out of range or not ascending" + at);
      if (!pos(q.gps_accuracy[e])) return fail(c, VPL_E_INVALID, "global fusion: an accuracy that is not positive" + at);
    }
    GfChain& G = ch[s];
    G.run = 1;
    for (size_t i = 0; i < 7 * (size_t)q.n; ++i)
      if (!std::isfinite(q.local[i]) || !std::isfinite(q.global[i])) { G.run = 0; break; }
    G.L = gf_layout(q.n, S);
    G.resident = 0;
    G.w = ws; G.out = outs;
    G.loc = ins; G.glo = ins + 7 * (size_t)q.n; G.gxyz = ins + 14 * (size_t)q.n; G.gacc = ins + 17 * (size_t)q.n;
    ws += G.L.total; ins += gf_up8(18 * (size_t)q.n); outs += gf_up8(GF_HEAD + 7 * (size_t)q.n);
    maxn = std::max(maxn, q.n); maxseg = std::max(maxseg, G.L.p.nseg); maxsep = std::max(maxsep, G.L.p.nsep);
  }
  const int rs = settle(c);
  if (rs) return rs;
  // ---- the packed upload: inputs (doubles) | chains
  auto up64 = [](size_t b) { return (b + 63) & ~(size_t)63; };
  const size_t b_ch = up64(ins * 8), bytes = b_ch + (size_t)n * sizeof(GfChain);
  std::vector<char> buf(bytes, 0);
  for (int s = 0; s < n; ++s) {
    const vpl_gf_input& q = in[s];
    const size_t nn = (size_t)q.n;
    double* d = (double*)buf.data() + ch[s].loc;
    std::memcpy(d, q.local, 7 * nn * 8);
    std::memcpy(d + 7 * nn, q.global, 7 * nn * 8);
    for (int e = 0; e < q.n_gps; ++e) {   // per node: xyz, and the accuracy (0: no fix)
      const size_t k = (size_t)q.gps_node[e];
      std::memcpy(d + 14 * nn + 3 * k, q.gps_xyz + 3 * (size_t)e, 3 * 8);
      d[17 * nn + k] = std::isfinite(q.gps_xyz[3 * e]) && std::isfinite(q.gps_xyz[3 * e + 1]) && std::isfinite(q.gps_xyz[3 * e + 2]) ? q.gps_accuracy[e] : 0.0;
      if (d[17 * nn + k] == 0.0) ch[s].run = 0;
    }
  }
  std::memcpy(buf.data() + b_ch, ch.data(), (size_t)n * sizeof(GfChain));
  const void* owner = &ch;
  char* d_in = nullptr;
  double *d_ws = nullptr, *d_out = nullptr;
  std::vector<double> h(outs);
  auto run = [&]() -> int {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, dalloc(c, &d_in, bytes, owner));
    HIPCHK(c, dalloc(c, &d_ws, ws, owner));
    HIPCHK(c, dalloc(c, &d_out, outs, owner));
    // (the allocator's zeroing runs on the null stream: what the kernels rely on is set again in stream order)
    HIPCHK(c, hipMemsetAsync(d_ws, 0, ws * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(d_out, 0, outs * 8, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_in, buf.data(), bytes, hipMemcpyHostToDevice, c->stream));
    GfArgs A;
    A.ch = (const GfChain*)(d_in + b_ch); A.ws = d_ws; A.in = (double*)d_in; A.out = d_out;
    A.opt = *opt;
    hipStream_t st = c->stream;
    gf_enqueue(c, A, n, maxn, maxseg, maxsep, dbg ? 1 : opt->max_iterations + 1, !dbg);
    HIPCHK(c, hipGetLastError());
    if (dbg) {
      const GfLayout& L = ch[0].L;
      const size_t m = 6 * (size_t)L.p.n;
      double ctl[GF_CTL];
      HIPCHK(c, hipMemcpyAsync(dbg->g, d_ws + L.g, m * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipMemcpyAsync(dbg->step, d_ws + L.delta, m * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipMemcpyAsync(ctl, d_ws + L.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipStreamSynchronize(st));
      *dbg->model = ctl[GF_MODEL];
      if (ctl[GF_STEP_OK] == 0.0) return fail(c, VPL_E_NUMERIC, "global fusion: no first step (the chain ended at once, or the factorisation failed)");
    } else {
      HIPCHK(c, hipMemcpyAsync(h.data(), d_out, outs * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipStreamSynchronize(st));
    }
    int hits = 0;
    const int rg = init_guard_hits(c, owner, &hits);
    if (rg) return rg;
    if (hits) return fail(c, VPL_E_HIP, "global fusion: guard behind " + std::to_string(hits) + " device array(s) overwritten");
    return VPL_OK;
  };
  const int rc = run();
  dfree_owner(c, owner);
  if (rc || dbg) return rc;
  for (int s = 0; s < n; ++s) {
    const double* o = h.data() + ch[s].out;
    vpl_gf_result& r = out[s];
    gf_read_head(o, r);
    std::memcpy(r.pose, o + GF_HEAD, 7 * (size_t)in[s].n * 8);
  }
  return VPL_OK;
}

}  // namespace vpl

extern "C" {

int vpl_gf_optimize_batch(vpl_ctx* c, int n, const vpl_gf_input* in, const vpl_gf_options* opt, vpl_gf_result* out) {
  if (!out) return VPL_E_INVALID;
  return vpl::gf_run(c, n, in, opt, out, nullptr);
}

int vpl_gf_debug_step(vpl_ctx* c, const vpl_gf_input* in, const vpl_gf_options* opt, double* g, double* step, double* model_cost_change) {
  if (!in || !g || !step || !model_cost_change) return VPL_E_INVALID;
  const vpl::GfDebugOut dbg{g, step, model_cost_change};
  return vpl::gf_run(c, 1, in, opt, nullptr, &dbg);
}

int vpl_gf_debug_plan(int n, int segment, int* n_sep, int* sep_node, int* n_seg, int* seg_bounds) {
  if (!n_sep || !sep_node || !n_seg || !seg_bounds || n < 1 || !vpl::gf_segment_ok(segment)) return VPL_E_INVALID;
  if (n > VPL_GF_MAX_NODES) return VPL_E_CAPACITY;
  const vpl::GfPlan p = vpl::gf_plan(n, vpl::gf_segment(segment));
  *n_sep = p.nsep; *n_seg = p.nseg;
  for (int j = 0; j < p.nsep; ++j) sep_node[j] = vpl::gf_sep_node(p, j);
  for (int j = 0; j < p.nseg; ++j) vpl::gf_seg_bounds(p, j, seg_bounds[2 * j], seg_bounds[2 * j + 1]);
  return VPL_OK;
}

int vpl_gf_local_cartesian(double lat0, double lon0, double h0, int n, const double* lla, double* xyz) {
  if (n < 0 || (n && (!lla || !xyz))) return VPL_E_INVALID;
  const double a = 6378137.0, f = 1.0 / 298.257223563, e2 = f * (2.0 - f), rad = M_PI / 180.0;
  auto ecef = [&](double lat, double lon, double h, double* o) {
    const double sp = std::sin(lat * rad), cp = std::cos(lat * rad), sl = std::sin(lon * rad), cl = std::cos(lon * rad);
    const double N = a / std::sqrt(1.0 - e2 * sp * sp);
    o[0] = (N + h) * cp * cl; o[1] = (N + h) * cp * sl; o[2] = (N * (1.0 - e2) + h) * sp;
  };
  double o0[3];
  ecef(lat0, lon0, h0, o0);
  const double sp = std::sin(lat0 * rad), cp = std::cos(lat0 * rad), sl = std::sin(lon0 * rad), cl = std::cos(lon0 * rad);
  for (int i = 0; i < n; ++i) {
    double o[3];
    ecef(lla[3 * i], lla[3 * i + 1], lla[3 * i + 2], o);
    const double dx = o[0] - o0[0], dy = o[1] - o0[1], dz = o[2] - o0[2];
    xyz[3 * i] = -sl * dx + cl * dy;
    xyz[3 * i + 1] = -sp * cl * dx - sp * sl * dy + cp * dz;
    xyz[3 * i + 2] = cp * cl * dx + cp * sl * dy + sp * dz;
  }
  return VPL_OK;
}

}  // extern "C"

// ---- the session: GlobalOptimization with the trajectory resident on the device.  The arrays hold max_nodes nodes; a call of
//      vpl_gf_optimize uploads the nodes and fixes that came since the last one, runs the batch call's kernels on the resident arrays
//      (the solved poses go back into the global array) and reads back the result head alone.
struct vpl_gf_session {
  vpl_ctx* c = nullptr;
  int cap = 0, n = 0, n_up = 0;          // capacity, nodes, nodes already on the device
  int fix_lo = 1, fix_hi = 0;            // the nodes whose fix changed since the last upload (lo > hi: none)
  std::vector<double> ts, loc, glo, gxyz, gacc;   // per node; glo: what inputOdom made of the node, read until it is uploaded
  std::vector<double> unmatched;         // t, xyz, accuracy of the fixes no node has the time of: stored, never used
  double T[16];                          // WGPS_T_WVIO, row-major
  double *d_in = nullptr, *d_ws = nullptr, *d_out = nullptr;
  vpl::GfChain* d_ch = nullptr;
};

namespace vpl {

static int gf_session_flush(vpl_gf_session* h) {
  vpl_ctx* c = h->c;
  const size_t cap = (size_t)h->cap;
  HIPCHK(c, hipSetDevice(c->device));
  if (h->n > h->n_up) {
    const size_t a = (size_t)h->n_up, cnt = (size_t)(h->n - h->n_up);
    HIPCHK(c, hipMemcpyAsync(h->d_in + 7 * a, h->loc.data() + 7 * a, 7 * cnt * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(h->d_in + 7 * cap + 7 * a, h->glo.data() + 7 * a, 7 * cnt * 8, hipMemcpyHostToDevice, c->stream));
    // (their "no fix" too)
    if (h->fix_lo > h->fix_hi) { h->fix_lo = h->n_up; h->fix_hi = h->n - 1; }
    else { h->fix_lo = std::min(h->fix_lo, h->n_up); h->fix_hi = h->n - 1; }
  }
  if (h->fix_lo <= h->fix_hi) {
    const size_t a = (size_t)h->fix_lo, cnt = (size_t)(h->fix_hi - h->fix_lo + 1);
    HIPCHK(c, hipMemcpyAsync(h->d_in + 14 * cap + 3 * a, h->gxyz.data() + 3 * a, 3 * cnt * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(h->d_in + 17 * cap + a, h->gacc.data() + a, cnt * 8, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));   // (the host copies may change from here on)
  h->n_up = h->n; h->fix_lo = 1; h->fix_hi = 0;
  return VPL_OK;
}

}  // namespace vpl

extern "C" {

int vpl_gf_create(vpl_ctx* c, int max_nodes, vpl_gf_session** out) {
  if (!c || !out || max_nodes < 1) return VPL_E_INVALID;
  if (max_nodes > VPL_GF_MAX_NODES) return vpl::fail(c, VPL_E_CAPACITY, "global fusion session: more than VPL_GF_MAX_NODES nodes");
  { const int rs = settle(c); if (rs) return rs; }
  vpl_gf_session* h = new vpl_gf_session();
  h->c = c; h->cap = max_nodes;
  const size_t cap = (size_t)max_nodes;
  h->ts.resize(cap); h->loc.resize(7 * cap); h->glo.resize(7 * cap); h->gxyz.assign(3 * cap, 0.0); h->gacc.assign(cap, 0.0);
  for (int i = 0; i < 16; ++i) h->T[i] = (i % 5 == 0) ? 1.0 : 0.0;
  hipError_t e = hipSetDevice(c->device);
  // the workspace of the largest plan: the one with the most separators, S = 2
  if (e == hipSuccess) e = vpl::dalloc(c, &h->d_in, 18 * cap, h);
  if (e == hipSuccess) e = vpl::dalloc(c, &h->d_ws, vpl::gf_layout(max_nodes, 2).total, h);
  if (e == hipSuccess) e = vpl::dalloc(c, &h->d_out, (size_t)vpl::GF_HEAD, h);
  if (e == hipSuccess) e = vpl::dalloc(c, &h->d_ch, (size_t)1, h);
  if (e != hipSuccess) {
    vpl::dfree_owner(c, h);
    delete h;
    return vpl::fail(c, VPL_E_HIP, "global fusion session: device allocation failed");
  }
  *out = h;
  return VPL_OK;
}

void vpl_gf_destroy(vpl_gf_session* h) {
  if (!h) return;
  (void)hipSetDevice(h->c->device);
  (void)hipStreamSynchronize(h->c->stream);   // (teardown: a failure has nobody to be reported to)
  vpl::dfree_owner(h->c, h);
  delete h;
}

int vpl_gf_input_odom(vpl_gf_session* h, double t, const double* p, const double* q, double* out_p, double* out_q) {
  if (!h || !p || !q || !out_p || !out_q) return VPL_E_INVALID;
  vpl_ctx* c = h->c;
  if (!std::isfinite(t) || (h->n && !(t > h->ts[h->n - 1]))) return vpl::fail(c, VPL_E_INVALID, "global fusion session: timestamps must increase");
  for (int i = 0; i < 3; ++i) if (!std::isfinite(p[i])) return vpl::fail(c, VPL_E_INVALID, "global fusion session: a pose that is not finite");
  for (int i = 0; i < 4; ++i) if (!std::isfinite(q[i])) return vpl::fail(c, VPL_E_INVALID, "global fusion session: a pose that is not finite");
  if (h->n >= h->cap) return vpl::fail(c, VPL_E_CAPACITY, "global fusion session: max_nodes reached");
  // inputOdom (globalOpt.cpp:51-66): globalQ = Quaterniond(R OdomQ.toRotationMatrix()), globalP = R OdomP + t
  vpl::M3 R;
  for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) R.m[3 * r + k] = h->T[4 * r + k];
  const vpl::Q4 gq = vpl::mat2q(vpl::mul(R, vpl::qmat(vpl::Q4{q[0], q[1], q[2], q[3]})));
  const vpl::V3 gp = vpl::mul(R, vpl::V3{p[0], p[1], p[2]}) + vpl::V3{h->T[3], h->T[7], h->T[11]};
  const size_t k = (size_t)h->n;
  h->ts[k] = t;
  double* l = h->loc.data() + 7 * k;
  double* g = h->glo.data() + 7 * k;
  l[0] = p[0]; l[1] = p[1]; l[2] = p[2]; l[3] = q[0]; l[4] = q[1]; l[5] = q[2]; l[6] = q[3];
  g[0] = gp.x; g[1] = gp.y; g[2] = gp.z; g[3] = gq.w; g[4] = gq.x; g[5] = gq.y; g[6] = gq.z;
  h->gacc[k] = 0.0;
  ++h->n;
  out_p[0] = gp.x; out_p[1] = gp.y; out_p[2] = gp.z;
  out_q[0] = gq.w; out_q[1] = gq.x; out_q[2] = gq.y; out_q[3] = gq.z;
  return VPL_OK;
}

int vpl_gf_input_gps(vpl_gf_session* h, double t, const double* xyz, double accuracy) {
  if (!h || !xyz) return VPL_E_INVALID;
  if (!(accuracy > 0.0) || !std::isfinite(accuracy) || !std::isfinite(xyz[0]) || !std::isfinite(xyz[1]) || !std::isfinite(xyz[2]))
    return vpl::fail(h->c, VPL_E_INVALID, "global fusion session: a fix that is not finite, or an accuracy that is not positive");
  const auto end = h->ts.begin() + h->n;
  const auto it = std::lower_bound(h->ts.begin(), end, t);
  if (it == end || *it != t) {   // GPSPositionMap keeps it; no node will ever ask for it
    h->unmatched.insert(h->unmatched.end(), {t, xyz[0], xyz[1], xyz[2], accuracy});
    return VPL_OK;
  }
  const int k = (int)(it - h->ts.begin());
  std::memcpy(h->gxyz.data() + 3 * (size_t)k, xyz, 3 * 8);
  h->gacc[k] = accuracy;
  if (h->fix_lo > h->fix_hi) { h->fix_lo = k; h->fix_hi = k; }
  else { h->fix_lo = std::min(h->fix_lo, k); h->fix_hi = std::max(h->fix_hi, k); }
  return VPL_OK;
}

int vpl_gf_optimize(vpl_gf_session* h, const vpl_gf_options* opt, vpl_gf_result* result) {
  if (!h || !opt || !result) return VPL_E_INVALID;
  vpl_ctx* c = h->c;
  if (h->n < 1) return vpl::fail(c, VPL_E_INVALID, "global fusion session: no node yet");
  if (!vpl::gf_options_ok(opt)) return vpl::fail(c, VPL_E_INVALID, "global fusion session: options out of range");
  { const int rs = settle(c); if (rs) return rs; }
  { const int rf = vpl::gf_session_flush(h); if (rf) return rf; }
  const size_t cap = (size_t)h->cap;
  vpl::GfChain G;
  G.L = vpl::gf_layout(h->n, vpl::gf_segment(opt->segment));
  G.w = 0; G.out = 0; G.loc = 0; G.glo = 7 * cap; G.gxyz = 14 * cap; G.gacc = 17 * cap; G.run = 1; G.resident = 1;
  HIPCHK(c, hipMemcpyAsync(h->d_ch, &G, sizeof G, hipMemcpyHostToDevice, c->stream));
  vpl::GfArgs A;
  A.ch = h->d_ch; A.ws = h->d_ws; A.in = h->d_in; A.out = h->d_out; A.opt = *opt;
  vpl::gf_enqueue(c, A, 1, h->n, G.L.p.nseg, G.L.p.nsep, opt->max_iterations + 1, true);
  HIPCHK(c, hipGetLastError());
  double head[vpl::GF_HEAD];
  HIPCHK(c, hipMemcpyAsync(head, h->d_out, sizeof head, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int hits = 0;
  const int rg = init_guard_hits(c, h, &hits);
  if (rg) return rg;
  if (hits) return vpl::fail(c, VPL_E_HIP, "global fusion session: guard behind " + std::to_string(hits) + " device array(s) overwritten");
  double* keep = result->pose;
  vpl::gf_read_head(head, *result);
  result->pose = keep;
  std::memcpy(h->T, result->wgps_T_wvio, sizeof h->T);
  return VPL_OK;
}

int vpl_gf_get_path(vpl_gf_session* h, int first, int count, double* out) {
  if (!h || first < 0 || count < 0 || (count && !out)) return VPL_E_INVALID;
  vpl_ctx* c = h->c;
  if ((long long)first + count > h->n) return vpl::fail(c, VPL_E_INVALID, "global fusion session: path range beyond the last node");
  if (!count) return VPL_OK;
  { const int rs = settle(c); if (rs) return rs; }
  { const int rf = vpl::gf_session_flush(h); if (rf) return rf; }
  HIPCHK(c, hipMemcpyAsync(out, h->d_in + 7 * (size_t)h->cap + 7 * (size_t)first, 7 * (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VPL_OK;
}

}  // extern "C"
