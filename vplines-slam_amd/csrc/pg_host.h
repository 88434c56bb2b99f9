// Host side of the pose-graph optimisation (vpl_pg_optimize_batch, vpl_pg_optimize_seq_batch, vpl_pg_debug_step[_seq]): the refusals, one plan per graph
// (pg_plan.h), the one packed upload, the rounds enqueued without a look at the device, the one read-back.  Included once by
// vplines_ba.hip, behind loop_host.h.
#pragma once
#include "pg_kernels.h"

static_assert(vpl::PG_MAX_NODES == VPL_PG_MAX_NODES && vpl::PG_MAX_LOOPS == VPL_PG_MAX_LOOPS, "pg_plan.h and vplines_ba.h disagree");

extern "C" {

void vpl_pg_default_options(vpl_pg_options* o) {
  if (!o) return;
  o->max_iterations = 5; o->max_consecutive_invalid_steps = 5; o->huber_delta = 0.1; o->loop_yaw_scale = 10.0;
  o->initial_radius = 1e4; o->max_radius = 1e16; o->min_radius = 1e-32; o->min_relative_decrease = 1e-3;
  o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
  o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32;
}

}  // extern "C"

namespace vpl {

struct PgDebugOut { double *g, *step, *model; };

static bool pg_options_ok(const vpl_pg_options* opt) {
  auto pos = [](double v) { return v > 0.0 && std::isfinite(v); };
  return !(opt->max_iterations < 0 || opt->max_iterations > 1000 || opt->max_consecutive_invalid_steps < 1 || !std::isfinite(opt->huber_delta) ||
           !pos(opt->loop_yaw_scale) || !pos(opt->initial_radius) || !pos(opt->max_radius) || !(opt->min_radius >= 0.0) ||
           !std::isfinite(opt->min_relative_decrease) || !(opt->function_tolerance >= 0.0) || !(opt->gradient_tolerance >= 0.0) ||
           !(opt->parameter_tolerance >= 0.0) || !pos(opt->min_lm_diagonal) || !(opt->max_lm_diagonal >= opt->min_lm_diagonal));
}

// the largest graph of a batch: what the grids are sized by
struct PgDims { int n_graphs = 0, maxE = 1, maxn = 1, maxnb = 1, maxLP = 0; };

// k_pg_init and the rounds, enqueued on the context's stream over an input block, graphs and integer blocks that are on the device
// (A); nothing is read back.  SEQ: the graphs carry node flags (vpl_pg_optimize_seq_batch).  first_only: one round, up to k_pg_back
template <bool SEQ>
static void pg_enqueue_rounds(vpl_ctx* c, const PgArgs& A, const PgDims& d, bool first_only) {
  const int n = d.n_graphs;
  const dim3 one(1, n), per_edge((d.maxE + PG_THREADS - 1) / PG_THREADS, n), per_node((16 * d.maxnb + PG_THREADS - 1) / PG_THREADS, n);
  const int tiles = d.maxLP / 16;
  { KTimer t(c, "k_pg_init"); hipLaunchKernelGGL(k_pg_init, dim3((std::max(d.maxE, d.maxn) + PG_THREADS - 1) / PG_THREADS, n), dim3(PG_THREADS), 0, c->stream, A); }
  const int rounds = first_only ? 1 : A.opt.max_iterations + 1;
  for (int it = 0; it < rounds; ++it) {
    { KTimer t(c, "k_pg_lin"); hipLaunchKernelGGL((k_pg_edges<0, SEQ>), per_edge, dim3(PG_THREADS), 0, c->stream, A);
      hipLaunchKernelGGL(k_pg_asm, per_node, dim3(PG_THREADS), 0, c->stream, A); }
    { KTimer t(c, "k_pg_factor"); hipLaunchKernelGGL(k_pg_factor<SEQ>, one, dim3(64), 0, c->stream, A); }
    { KTimer t(c, "k_pg_cols"); hipLaunchKernelGGL(k_pg_cols, dim3(d.maxLP / 64 + 1, n), dim3(64), 0, c->stream, A); }
    if (tiles) {
      KTimer t(c, "k_pg_cap");
      hipLaunchKernelGGL(k_pg_cap, dim3(tiles * tiles, n), dim3(64), 0, c->stream, A, tiles);
      hipLaunchKernelGGL(k_pg_capsolve, one, dim3(PG_THREADS), 0, c->stream, A);
    }
    { KTimer t(c, "k_pg_back"); hipLaunchKernelGGL(k_pg_back, one, dim3(PG_THREADS), 0, c->stream, A); }
    if (first_only) break;
    { KTimer t(c, "k_pg_decide"); hipLaunchKernelGGL((k_pg_edges<1, SEQ>), per_edge, dim3(PG_THREADS), 0, c->stream, A);
      hipLaunchKernelGGL(k_pg_decide<SEQ>, one, dim3(PG_THREADS), 0, c->stream, A); }
  }
}

// the whole call; dbg: stop after the first linear solve of graph 0 and hand out g, step and the model cost change.  seq: honour
// `sequence` (vpl_pg_optimize_seq_batch) instead of refusing a graph whose sequences differ
static int pg_run(vpl_ctx* c, int n, const vpl_pg_input* in, const vpl_pg_options* opt, vpl_pg_result* out, const PgDebugOut* dbg, bool seq) {
  if (!c || n < 0 || !in || !opt || (!out && !dbg)) return VPL_E_INVALID;
  if (n == 0) return VPL_OK;
  if (n > c->maxW) return fail(c, VPL_E_CAPACITY, "pose graph: more graphs than max_windows");
  if (!pg_options_ok(opt)) return fail(c, VPL_E_INVALID, "pose graph: options out of range");
  std::vector<PgGraph> gr(n);
  std::vector<std::vector<int>> li(n), la(n);
  size_t ws = 0, is = 0, ins = 0, outs = 0;
  PgDims dims;
  dims.n_graphs = n;
  for (int s = 0; s < n; ++s) {
    const vpl_pg_input& q = in[s];
    const std::string at = " (graph " + std::to_string(s) + ")";
    if (q.n < 1 || q.n_tail < 0 || !q.vio_T || !q.vio_R || !q.loop_local || !q.loop_info || (q.n_tail && (!q.tail_T || !q.tail_R)))
      return fail(c, VPL_E_INVALID, "pose graph: null arrays or bad counts" + at);
    if (out && (!out[s].T || !out[s].R || (q.n_tail && (!out[s].tail_T || !out[s].tail_R))))
      return fail(c, VPL_E_INVALID, "pose graph: null result arrays" + at);
    if (q.n > VPL_PG_MAX_NODES) return fail(c, VPL_E_CAPACITY, "pose graph: more than VPL_PG_MAX_NODES nodes" + at);
    bool run = true;
    for (int k = 0; k < q.n; ++k) {
      if (q.loop_local[k] >= k) return fail(c, VPL_E_INVALID, "pose graph: loop_local not smaller than the node's own index" + at);
      if (q.loop_local[k] >= 0) { li[s].push_back(k); la[s].push_back(q.loop_local[k]); }
      if (seq && q.sequence && q.sequence[k] < 0) return fail(c, VPL_E_INVALID, "pose graph: negative sequence" + at);
      if (!seq && q.sequence && q.sequence[k] != q.sequence[0]) run = false;
    }
    if ((int)li[s].size() > VPL_PG_MAX_LOOPS) return fail(c, VPL_E_CAPACITY, "pose graph: more than VPL_PG_MAX_LOOPS loops" + at);
    PgGraph& G = gr[s];
    G.run = run ? 1 : 0;
    if (!run) { li[s].clear(); la[s].clear(); }
    G.p = run ? pg_layout(q.n, (int)li[s].size()) : pg_layout(1, 0);
    G.n_tail = run ? q.n_tail : 0;
    G.w = ws; G.iw = is; G.in = ins; G.out = outs;
    ws += G.p.total; is += G.p.itotal + (seq ? pg_up8((size_t)G.p.n) : 0);   // (seq: the node flags behind the integer block)
    ins += pg_up8(12 * (size_t)G.p.n + 4 * (size_t)G.p.L + 12 * (size_t)G.n_tail);
    outs += pg_up8(PG_HEAD + 12 * (size_t)G.p.n + 12 * (size_t)G.n_tail);
    dims.maxE = std::max(dims.maxE, G.p.E); dims.maxn = std::max(dims.maxn, G.p.n);
    dims.maxnb = std::max(dims.maxnb, G.p.nb); dims.maxLP = std::max(dims.maxLP, G.p.LP);
  }
  const int rs = settle(c);
  if (rs) return rs;
  // ---- the packed upload: inputs (doubles) | graphs | integer blocks
  auto up64 = [](size_t b) { return (b + 63) & ~(size_t)63; };
  const size_t b_gr = up64(ins * 8), b_int = up64(b_gr + (size_t)n * sizeof(PgGraph)), bytes = b_int + std::max<size_t>(is, 1) * 4;
  std::vector<char> buf(bytes, 0);
  for (int s = 0; s < n; ++s) {
    const PgGraph& G = gr[s];
    const vpl_pg_input& q = in[s];
    double* d = (double*)buf.data() + G.in;
    if (G.run) {
      std::memcpy(d, q.vio_T, 3 * (size_t)q.n * 8);
      std::memcpy(d + 3 * (size_t)q.n, q.vio_R, 9 * (size_t)q.n * 8);
      double* l4 = d + 12 * (size_t)q.n;
      for (int e = 0; e < G.p.L; ++e) {
        const double* info = q.loop_info + 8 * (size_t)li[s][e];
        l4[4 * e] = info[0]; l4[4 * e + 1] = info[1]; l4[4 * e + 2] = info[2]; l4[4 * e + 3] = info[7];
      }
      if (q.n_tail) {
        std::memcpy(l4 + 4 * (size_t)G.p.L, q.tail_T, 3 * (size_t)q.n_tail * 8);
        std::memcpy(l4 + 4 * (size_t)G.p.L + 3 * (size_t)q.n_tail, q.tail_R, 9 * (size_t)q.n_tail * 8);
      }
    }
    pg_fill_ints(G.p, li[s].data(), la[s].data(), (int*)(buf.data() + b_int) + G.iw);
    if (seq) pg_node_flags(G.p.n, q.sequence, G.p.L, li[s].data(), la[s].data(), (int*)(buf.data() + b_int) + G.iw + G.p.itotal);
  }
  std::memcpy(buf.data() + b_gr, gr.data(), (size_t)n * sizeof(PgGraph));
  const void* owner = &gr;
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
    PgArgs A;
    A.gr = (const PgGraph*)(d_in + b_gr); A.ws = d_ws; A.ints = (const int*)(d_in + b_int); A.in = (const double*)d_in; A.out = d_out;
    A.opt = *opt;
    const dim3 one(1, n);
    if (seq) pg_enqueue_rounds<true>(c, A, dims, dbg != nullptr);
    else pg_enqueue_rounds<false>(c, A, dims, dbg != nullptr);
    HIPCHK(c, hipGetLastError());
    if (dbg) {
      const PgLayout& p = gr[0].p;
      double ctl[PG_CTL];
      HIPCHK(c, hipMemcpyAsync(dbg->g, d_ws + p.g, (size_t)p.m * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(dbg->step, d_ws + p.delta, (size_t)p.m * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(ctl, d_ws + p.ctl, sizeof ctl, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      *dbg->model = ctl[PG_MODEL];
      if (ctl[PG_STEP_OK] == 0.0) return fail(c, VPL_E_NUMERIC, "pose graph: the factorisation failed");
    } else {
      { KTimer t(c, "k_pg_finish"); hipLaunchKernelGGL(k_pg_finish, one, dim3(PG_THREADS), 0, c->stream, A); }
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(h.data(), d_out, outs * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    int hits = 0;
    const int rg = init_guard_hits(c, owner, &hits);
    if (rg) return rg;
    if (hits) return fail(c, VPL_E_HIP, "pose graph: guard behind " + std::to_string(hits) + " device array(s) overwritten");
    return VPL_OK;
  };
  const int rc = run();
  dfree_owner(c, owner);
  if (rc || dbg) return rc;
  for (int s = 0; s < n; ++s) {
    const PgGraph& G = gr[s];
    const double* o = h.data() + G.out;
    vpl_pg_result& r = out[s];
    r.status = (int)o[0]; r.termination = (int)o[1]; r.iterations = (int)o[2]; r.successful_steps = (int)o[3];
    r.unsuccessful_steps = (int)o[4]; r.reserved = 0; r.initial_cost = o[5]; r.final_cost = o[6]; r.yaw_drift = o[7];
    std::memcpy(r.r_drift, o + 8, 9 * 8); std::memcpy(r.t_drift, o + 17, 3 * 8);
    if (!G.run) continue;
    const size_t nn = (size_t)G.p.n, nt = (size_t)G.n_tail;
    std::memcpy(r.T, o + PG_HEAD, 3 * nn * 8); std::memcpy(r.R, o + PG_HEAD + 3 * nn, 9 * nn * 8);
    if (nt) { std::memcpy(r.tail_T, o + PG_HEAD + 12 * nn, 3 * nt * 8); std::memcpy(r.tail_R, o + PG_HEAD + 12 * nn + 3 * nt, 9 * nt * 8); }
  }
  return VPL_OK;
}

}  // namespace vpl

extern "C" {

int vpl_pg_optimize_batch(vpl_ctx* c, int n, const vpl_pg_input* in, const vpl_pg_options* opt, vpl_pg_result* out) {
  if (!out) return VPL_E_INVALID;
  return vpl::pg_run(c, n, in, opt, out, nullptr, false);
}

int vpl_pg_optimize_seq_batch(vpl_ctx* c, int n, const vpl_pg_input* in, const vpl_pg_options* opt, vpl_pg_result* out) {
  if (!out) return VPL_E_INVALID;
  return vpl::pg_run(c, n, in, opt, out, nullptr, true);
}

int vpl_pg_debug_step(vpl_ctx* c, const vpl_pg_input* in, const vpl_pg_options* opt, double* g, double* step, double* model_cost_change) {
  if (!in || !g || !step || !model_cost_change) return VPL_E_INVALID;
  if (in->n < 2) return VPL_E_INVALID;
  const vpl::PgDebugOut dbg{g, step, model_cost_change};
  return vpl::pg_run(c, 1, in, opt, nullptr, &dbg, false);
}

int vpl_pg_debug_step_seq(vpl_ctx* c, const vpl_pg_input* in, const vpl_pg_options* opt, double* g, double* step, double* model_cost_change) {
  if (!in || !g || !step || !model_cost_change) return VPL_E_INVALID;
  if (in->n < 2) return VPL_E_INVALID;
  const vpl::PgDebugOut dbg{g, step, model_cost_change};
  return vpl::pg_run(c, 1, in, opt, nullptr, &dbg, true);
}

}  // extern "C"
