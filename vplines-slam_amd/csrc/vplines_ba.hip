// C ABI of the MI355X-native bundle-adjustment path (include/vplines_ba.h).
// Host side: packs caller-owned windows into the device SoA of ba_types.h, enqueues the
// kernel sequence of one batched solve on the context's stream, unpacks results.
// One translation unit.  This file: context create / destroy and the setters, pre-integration and the single-factor evaluators,
// the launch sequences, the window entry points, download and prior fetch, the debug entry points.  Included once each, like the
// kernel headers: ba_stage.h (staging arena), ba_ctx.h (vpl_ctx), ba_upload.h (the upload), init_align_host.h, init_sfm_host.h and
// init_relpose_host.h (vpl_init_*), loop_host.h, pg_host.h, pgs_host.h and gf_host.h (vpl_loop_*, vpl_pg_*, vpl_pgs_*, vpl_gf_*), sel_host.h (vpl_select_*,
// vpl_sel_*), ba_session.h (vpl_odo_*).
// There is no CPU compute path in this library: every entry point that computes launches
// HIP kernels and reports VPL_E_NODEVICE / VPL_E_HIP when that is impossible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vplines_ba.h"
#include "ba_types.h"
#include "ba_lin.h"
#include "ba_pack.h"
#include "ba_solve.h"
#include "ba_step.h"
#include "ba_marg.h"
#include "ba_prior_eig.h"
#include "ba_lineopt.h"
#include "ba_factors.h"
#include "ba_odo.h"
#include "odo_tracks.h"
#include "host_common.h"

using namespace vpl;

// the host side by concern, each included here once, behind the using-directive they rely on: the staging arena, the
// context, the upload
#include "ba_stage.h"
#include "ba_ctx.h"
#include "ba_upload.h"
#include "init_align_host.h"
#include "init_sfm_host.h"
#include "init_relpose_host.h"
#include "loop_host.h"
#include "pg_host.h"
#include "pgs_host.h"
#include "gf_host.h"
#include "sel_host.h"

template <typename Launch>
static int eval_generic(vpl_ctx* c, int n, const double* params, int psz, const double* consts, int csz, int nres,
                        int njac, double* residuals, double* jac, Launch launch) {
  if (!c || n < 0 || !params || !consts || !residuals) return VPL_E_INVALID;
  if (n == 0) return VPL_OK;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf dp, dc, dr, dj;
  HIPCHK(c, dp.alloc((size_t)n * psz * 8));
  HIPCHK(c, dc.alloc((size_t)n * csz * 8));
  HIPCHK(c, dr.alloc((size_t)n * nres * 8));
  if (jac) HIPCHK(c, dj.alloc((size_t)n * njac * 8));
  HIPCHK(c, hipMemcpyAsync(dp.p, params, (size_t)n * psz * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dc.p, consts, (size_t)n * csz * 8, hipMemcpyHostToDevice, c->stream));
  launch(dp.d(), dc.d(), dr.d(), jac ? dj.d() : nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(residuals, dr.p, (size_t)n * nres * 8, hipMemcpyDeviceToHost, c->stream));
  if (jac) HIPCHK(c, hipMemcpyAsync(jac, dj.p, (size_t)n * njac * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VPL_OK;
}

// ---- pieces shared by the entry points ----------------------------------------------------------------
// device line dl of window w is the caller's line h_lmap[w][dl]: the Pluecker vectors (plk: the window's [maxL][6]) go back for
// the lines keep(dl, l) selects
template <typename Keep>
static void scatter_lines(const vpl_ctx* c, size_t w, vpl_window& v, const double* plk, Keep keep) {
  const std::vector<int>& lmap = c->h_lmap[w];
  for (size_t dl = 0; dl < lmap.size(); ++dl)
    if (keep((int)dl, lmap[dl])) std::memcpy(v.line_plk + (size_t)lmap[dl] * 6, plk + dl * 6, 6 * 8);
}
// ... after a solve: the lines k_gauge erased (removeLineOutlier) keep the caller's value and are flagged in line_removed;
// returns how many were erased
static int scatter_solved_lines(const vpl_ctx* c, size_t w, vpl_window& v, const double* plk, const int* removed) {
  if (v.line_removed) std::fill(v.line_removed, v.line_removed + v.n_lines, 0);
  int n = 0;
  scatter_lines(c, w, v, plk, [&](int dl, int l) {
    if (v.line_removed) v.line_removed[l] = removed[dl] ? 1 : 0;
    n += removed[dl] ? 1 : 0;
    return !removed[dl];
  });
  return n;
}
static void fill_report(vpl_solve_report& r, const TrState& t) {
  std::memset(&r, 0, sizeof(r));
  r.iterations = t.iter;
  r.num_successful_steps = t.num_successful;
  r.termination = t.status == 1 ? 1 : t.status == 2 ? 2 : 0;
  r.initial_cost = t.initial_cost;
  r.final_cost = t.x_cost;
}

extern "C" {

void vpl_ba_default_options(vpl_ba_options* o) {
  o->num_iterations = 5;
  o->estimate_extrinsic = 1;
  o->marginalization_flag = VPL_MARGIN_OLD;
  o->remove_line_outliers = 0;
  o->focal_length = 460.0;
  o->line_factor = 306.666666667;
  o->vp_factor = 10.0;
  o->g_norm = 9.81007;
  o->acc_n = 0.08; o->gyr_n = 0.004; o->acc_w = 0.00004; o->gyr_w = 2.0e-6;
  o->huber_delta = 1.0;
}

// everything vpl_ctx_create does after the device checks; on failure vpl_ctx_create frees what was allocated
static int ctx_init(vpl_ctx* c, int device, int max_windows, int max_points, int max_point_obs, int max_lines, int max_line_obs) {
  { const char* g = getenv("VPL_DEBUG_GUARDS"); c->guards = g && g[0] == '1'; }
  c->device = device;
  c->maxW = max_windows;
  c->maxP = max_points > 0 ? (max_points + 1) & ~1 : 2;   // even: k_solve streams the gradient entries in 16-byte units
  c->maxPO = max_point_obs > 0 ? max_point_obs : 1;
  c->maxL = max_lines > 0 ? max_lines : 1;
  c->maxLO = max_line_obs > 0 ? max_line_obs : 1;
  if (!solve_layout_fits(c->maxP, c->maxL)) return VPL_E_CAPACITY;
  if (solve_smem(c->maxP, c->maxL) > 159 * 1024) return VPL_E_CAPACITY;
  DevBatch& B = c->B;
  std::memset(&B, 0, sizeof(B));
  B.maxP = c->maxP; B.maxPO = c->maxPO; B.maxL = c->maxL; B.maxLO = c->maxLO;
  B.nfull = NC + B.maxP + 4 * B.maxL;
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0) ncu = 256;
    if (const char* sv = std::getenv("VPL_BA_LIN_SPLIT")) ncu = std::atoi(sv) ? 1 << 30 : 0;   // 1: always two work-groups per window, 0: never (A/B runs, tests)
    B.ncu = ncu;
  }
  B.maxPR = max_point_unit_rounds(B.maxP, B.maxPO);
  B.maxKS = max_schur_ksteps(B.maxP, B.maxL);
  B.llSlots = line_lane_slots(B.maxL);
  // One hipMalloc per array, in this order (vpl_ba_debug_guards names an array by its index).  (Measured alternative, round 2:
  // all ~90 arrays out of one arena, with and without skewed offsets -- k_cost, the kernel closest to the bandwidth roof, then
  // runs at 0.30 ms per step in EVERY process, whereas with separate allocations it is 0.24 ms in most processes and 0.30 ms in
  // some: the difference is where the driver places the buffers, not the code.  DESIGN.md section 8.)
  const size_t W = max_windows;
  hipError_t e = hipSuccess;
#define AL(ptr, n) if (e == hipSuccess) e = dalloc(c, &B.ptr, (size_t)(n))
  AL(pose, W * 77); AL(sb, W * 99); AL(ex, W * 7); AL(invd, W * B.maxP); AL(orth, W * B.maxL * 4);
  AL(pose_c, W * 77); AL(sb_c, W * 99); AL(ex_c, W * 7); AL(invd_c, W * B.maxP); AL(orth_c, W * B.maxL * 4); AL(lw, W * B.maxL * 6); AL(lw_c, W * B.maxL * 6);
  AL(lin_part, W * LIN_PART); AL(lin_pcost, W); AL(lin_flag, W);
  AL(pose_0, W * 77); AL(sb_0, W * 99); AL(ex_0, W * 7); AL(invd_0, W * B.maxP); AL(plk_0, W * B.maxL * 6);
  AL(plk, W * B.maxL * 6); AL(gauge, W * 4); AL(fail_ref, W * 13); AL(orth_in, W);
  AL(nP, W); AL(nL, W);
  AL(pt_start, W * B.maxP); AL(pt_nobs, W * B.maxP); AL(pt_off, W * B.maxP); AL(pt_obs, W * B.maxPO * 3);
  AL(ps_list, W * B.maxP); AL(ps_cnt, W * (NF + 1)); AL(pu_lane, W * B.maxPR * 1024); AL(pu_sub, W * B.maxPR * 512); AL(pu_cnt, W); AL(pu_cnt0, W);
  AL(ln_start, W * B.maxL); AL(ln_nobs, W * B.maxL); AL(ln_off, W * B.maxL); AL(ln_obs, W * B.maxLO * 8);
  AL(nLO, W); AL(lo_ln, W * B.maxLO);
  AL(ll_tab, W * B.llSlots * 2); AL(ll_np, W);
  AL(pre, W * NF);
  AL(pr_n, W); AL(pr_nb, W); AL(pr_kind, W * MAXPB); AL(pr_frame, W * MAXPB); AL(pr_idx, W * MAXPB);
  AL(pr_x0, W * MAXPB * 9); AL(pr_J0, W * MAXPN * MAXPN); AL(pr_r0, W * MAXPN); AL(pr_H, W * MAXPN * MAXPN); AL(pr_g0, W * MAXPN);
  AL(pr_map, W * MAXPN);
  AL(Hcc, W * NCP); AL(gc, W * NC); AL(asm_tab, 2 * NCP); AL(Hpp, W * B.maxP); AL(gp, W * B.maxP); AL(Wp, W * B.maxP * NV);
  AL(Hll, W * B.maxL * 16); AL(gl, W * B.maxL * 4); AL(Wl, W * B.maxL * 4 * NV); AL(lchol, W * B.maxL * 10);
  AL(tr, W);
  AL(scale, W * B.nfull); AL(diag, W * B.nfull); AL(grad, W * B.nfull); AL(gn, W * B.nfull);
  AL(mg_n, W); AL(mg_nb, W); AL(mg_kind, W * MAXPB); AL(mg_frame, W * MAXPB); AL(mg_idx, W * MAXPB);
  AL(mg_cam, W * MAXPB); AL(mg_x0, W * MAXPB * 9); AL(mg_J0, W * MAXKEEP * MAXKEEP); AL(mg_r0, W * MAXKEEP);
  AL(mg_A, W * MAXKEEP * MAXKEEP); AL(mg_b, W * MAXKEEP); AL(mg_m, W); AL(dbg, W * 64); AL(ln_removed, W * B.maxL); AL(ln_tri, W * B.maxL);
  if (e == hipSuccess) e = dalloc(c, &c->d_act, (size_t)ACT_SLOTS * 4);
  AL(order, 2 * W); AL(ord_cnt, 4);
  AL(sk_tab, W * B.maxKS * 4); AL(sk_wave, W * 8 * SK_WSTRIDE); AL(sacc, W * SACC_N); AL(nz_tab, NZ_N); AL(ycs, W * 176); AL(sx, W * 8); AL(path, W);
#undef AL
  if (e != hipSuccess) return VPL_E_HIP;
  if (lin_smem_base(c->maxP, c->maxL) > LIN_LDS_BUDGET) return VPL_E_CAPACITY;
  B.prhN = lin_prh_n(c->maxP, c->maxL);
  {   // non-zero pattern of the packed cam Hessian of a fast-path window, and the static tables of the assembly passes of
      // k_lin over the pattern and over its complement: one predicate for the three (ba_asm_pattern.h)
    std::vector<int> nz, tab;
    asm_build_tables(nz, tab);
    if ((int)nz.size() != NZ_N || (int)tab.size() != 2 * NCP) return VPL_E_HIP;
    if (hipMemcpy(B.asm_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return VPL_E_HIP;
    if (hipMemcpy(B.nz_tab, nz.data(), nz.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return VPL_E_HIP;
  }
  // the attribute is per kernel, not per context: never lower what a larger context of this process has asked for
  static size_t lin_max = 0, solve_max = 0, schur_max = 0, back_max = 0, step_max = 0;
  lin_max = std::max(lin_max, lin_smem(c->maxP, c->maxL));
  solve_max = std::max(solve_max, solve_smem(c->maxP, c->maxL));
  schur_max = std::max(schur_max, schur_smem(c->maxP, c->maxL));
  back_max = std::max(back_max, back_smem(c->maxP, c->maxL));
  step_max = std::max(step_max, step_smem(c->maxP, c->maxL));
  if (schur_max > 159 * 1024 || back_max > 159 * 1024) return VPL_E_CAPACITY;
  const std::pair<const void*, size_t> lds[] = {
      {(const void*)k_lin2, lin_max}, {(const void*)k_lin<1>, lin_max}, {(const void*)k_lin<2>, lin_max},
      {(const void*)k_solve, solve_max}, {(const void*)k_schur<3>, schur_max}, {(const void*)k_schur<5>, schur_max},
      {(const void*)k_schur_mixed, schur_max}, {(const void*)k_chol, chol_smem()}, {(const void*)k_back, back_max},
      {(const void*)k_step<3, false>, step_max}, {(const void*)k_step<3, true>, step_max}, {(const void*)k_step<5, false>, step_max},
      {(const void*)k_prep, PREP_SMEM}, {(const void*)k_marg<MARG_THREADS>, MARG_LDS_MAX}, {(const void*)k_marg<256>, MARG_LDS_SMALL},
      {(const void*)k_prior_eigen, prior_eig_layout(MAXKEEP).bytes}, {(const void*)k_init_align, init_lds_bytes(INIT_NMAX)}};
  for (const auto& k : lds)
    if (hipFuncSetAttribute(k.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.second) != hipSuccess) return VPL_E_HIP;
  vpl_ba_default_options(&c->opt);
  if (const char* gv = std::getenv("VPL_BA_GRAPH")) c->use_graph = std::atoi(gv) != 0;
  if (const char* gv = std::getenv("VPL_BA_GENERAL")) c->force_general = std::atoi(gv) != 0;
  if (const char* gv = std::getenv("VPL_BA_STEP_FUSED")) c->step_fused = std::atoi(gv) != 0;
  if (const char* gv = std::getenv("VPL_BA_RESET_FOLD")) c->restore_fold = std::atoi(gv) != 0;
  if (const char* gv = std::getenv("VPL_BA_SCHUR_WIDE")) { c->schur_wide_all = std::atoi(gv) > 0; c->schur_never_wide = std::atoi(gv) < 0; }
  return VPL_OK;
}

int vpl_ctx_create(vpl_ctx** out, int device, int max_windows, int max_points, int max_point_obs, int max_lines,
                   int max_line_obs) {
  if (!out || max_windows < 1 || max_points < 0 || max_lines < 0) return VPL_E_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || device >= ndev) return VPL_E_NODEVICE;
  if (hipSetDevice(device) != hipSuccess) return VPL_E_NODEVICE;
  vpl_ctx* c = new vpl_ctx();
  const int rc = ctx_init(c, device, max_windows, max_points, max_point_obs, max_lines, max_line_obs);
  if (rc != VPL_OK) {
    free_arrays(c);
    delete c;
    return rc;
  }
  *out = c;
  return VPL_OK;
}

void vpl_ctx_destroy(vpl_ctx* c) {
  if (!c) return;
  // (teardown: a failure has nobody to be reported to)
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  (void)restore_event(c, RESTORE_EV_DESTROY);   // (a pending restore is dropped: nobody can observe the states any more)
  drop_graph(c);
  free_arrays(c);
  c->stage.release();
  for (hipEvent_t& e : c->leg_ev) if (e) (void)hipEventDestroy(e);
  delete c;
}

int vpl_ctx_set_stream(vpl_ctx* c, void* s) {
  if (!c) return VPL_E_INVALID;
  // what is in flight on the stream so far is completed first (an enqueued call would otherwise be collected behind a
  // synchronisation of the NEW stream, and a later download would not be ordered behind a solve on the old one)
  const int rs = settle_call(c);
  if (rs) return rs;
  if (c->stream != (hipStream_t)s) {
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipStreamSynchronize(c->stream);   // (an old stream the caller has destroyed already has nothing in flight)
    (void)hipGetLastError();
  }
  drop_graph(c);
  c->stream = (hipStream_t)s;
  // a pending restore is issued on the NEW stream (everything on the old one has completed; the old one may be gone)
  return restore_event(c, RESTORE_EV_OBSERVE);
}
// the rule that turns the kept block into the next prior (k_marg's pivoted Cholesky, or k_prior_eigen behind it); a call already
// enqueued is collected first, so that every call runs under the rule in force when it was enqueued
int vpl_ba_set_prior_rule(vpl_ctx* c, int rule) {
  if (!c || (rule != VPL_PRIOR_PIVOTED_CHOLESKY && rule != VPL_PRIOR_EIGEN)) return VPL_E_INVALID;
  const int rs = settle(c);
  if (rs) return rs;
  drop_graph(c);   // the launch sequence of a solve changes: the next vpl_ba_solve captures it again
  c->prior_rule = rule;
  return VPL_OK;
}
const char* vpl_last_error(const vpl_ctx* c) { return c ? c->err.c_str() : "null context"; }

// device time of the legs of the last vpl_ba_upload / vpl_ba_solve / vpl_ba_download (hipEvents on the context's stream around
// each call's device work: copy + scatter | the solve's launches | gather + copy), next to the wall clock a caller measures
int vpl_ctx_enable_leg_timing(vpl_ctx* c, int enable) {
  if (!c) return VPL_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  if (enable)
    for (hipEvent_t& e : c->leg_ev) if (!e) HIPCHK(c, hipEventCreate(&e));
  c->leg_timing = enable != 0;
  return VPL_OK;
}
int vpl_ctx_leg_times(vpl_ctx* c, double* ms3) {
  if (!c || !ms3 || !c->leg_timing) return VPL_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 3; ++k) {
    float ms = 0.f;
    const hipError_t e = hipEventElapsedTime(&ms, c->leg_ev[2 * k], c->leg_ev[2 * k + 1]);
    ms3[k] = e == hipSuccess ? (double)ms : -1.0;   // -1: that leg has not run with timing on
  }
  return VPL_OK;
}

int vpl_ctx_synchronize(vpl_ctx* c) {
  if (!c) return VPL_E_INVALID;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return settle(c);
}
int vpl_ba_collect(vpl_ctx* c) {
  if (!c) return VPL_E_INVALID;
  return settle(c);
}

// ---- IMU pre-integration ---------------------------------------------------------------------------
int vpl_preintegrate_batch(vpl_ctx* c, int n, const int* offset, const int* nsamples, const double* samples,
                           const double* acc0, const double* gyr0, const double* lin_ba, const double* lin_bg,
                           const vpl_ba_options* opt, vpl_preintegration* out) {
  if (!c || n < 0 || !opt) return VPL_E_INVALID;
  if (n == 0) return VPL_OK;
  if (!offset || !nsamples) return VPL_E_INVALID;
  for (int i = 0; i < n; ++i)
    if (offset[i] < 0 || nsamples[i] < 0) return VPL_E_INVALID;   // before anything is sized by them; nsamples[i] == 0 is an empty interval
  HIPCHK(c, hipSetDevice(c->device));
  size_t total = 0;
  for (int i = 0; i < n; ++i) total = std::max(total, (size_t)offset[i] + nsamples[i]);
  DevBuf d_off, d_ns, d_s, d_a, d_g, d_ba, d_bg, d_out;
  HIPCHK(c, d_off.alloc(n * sizeof(int)));
  HIPCHK(c, d_ns.alloc(n * sizeof(int)));
  HIPCHK(c, d_s.alloc(total * 7 * sizeof(double) + 8));
  HIPCHK(c, d_a.alloc(n * 3 * sizeof(double)));
  HIPCHK(c, d_g.alloc(n * 3 * sizeof(double)));
  HIPCHK(c, d_ba.alloc(n * 3 * sizeof(double)));
  HIPCHK(c, d_bg.alloc(n * 3 * sizeof(double)));
  HIPCHK(c, d_out.alloc(n * sizeof(DevPreint)));
  HIPCHK(c, hipMemcpyAsync(d_off.p, offset, n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_ns.p, nsamples, n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_s.p, samples, total * 7 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_a.p, acc0, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_g.p, gyr0, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_ba.p, lin_ba, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_bg.p, lin_bg, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  launch_preintegrate(c, n, (const int*)d_off.p, (const int*)d_ns.p, d_s.d(), d_a.d(), d_g.d(), d_ba.d(), d_bg.d(), opt, (DevPreint*)d_out.p);
  HIPCHK(c, hipGetLastError());
  std::vector<DevPreint> h(n);
  HIPCHK(c, hipMemcpyAsync(h.data(), d_out.p, n * sizeof(DevPreint), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; ++i) from_preintegrate_out(h[i], out[i]);
  return VPL_OK;
}

// ---- single-factor evaluators ------------------------------------------------------------------------
int vpl_projection_factor_evaluate(vpl_ctx* c, int n, const double* params, const double* pts, double sqrt_info,
                                   double* residuals, double* jac) {
  return eval_generic(c, n, params, 22, pts, 6, 2, 44, residuals, jac, [&](double* p, double* k, double* r, double* j) {
    hipLaunchKernelGGL(k_eval_projection, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, p, k, sqrt_info, r, j);
  });
}
int vpl_line_factor_evaluate(vpl_ctx* c, int n, const double* params, const double* obs, double sqrt_info,
                             double* residuals, double* jac) {
  return eval_generic(c, n, params, 18, obs, 4, 2, 36, residuals, jac, [&](double* p, double* k, double* r, double* j) {
    hipLaunchKernelGGL(k_eval_line<0>, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, p, k, sqrt_info, r, j);
  });
}
int vpl_vp_factor_evaluate(vpl_ctx* c, int n, const double* params, const double* vp, double sqrt_info,
                           double* residuals, double* jac) {
  return eval_generic(c, n, params, 18, vp, 3, 2, 36, residuals, jac, [&](double* p, double* k, double* r, double* j) {
    hipLaunchKernelGGL(k_eval_line<1>, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, p, k, sqrt_info, r, j);
  });
}
int vpl_imu_factor_evaluate(vpl_ctx* c, int n, const double* params, const vpl_preintegration* pre, double g_norm,
                            double* residuals, double* jac) {
  if (!c || n < 0 || !params || !pre || !residuals) return VPL_E_INVALID;
  if (n == 0) return VPL_OK;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<DevPreint> h(n);
  for (int i = 0; i < n; ++i) to_dev_preint(pre[i], h[i]);
  DevBuf dp, dpre, dr, dj, ds;
  HIPCHK(c, dp.alloc((size_t)n * 32 * 8));
  HIPCHK(c, dpre.alloc((size_t)n * sizeof(DevPreint)));
  HIPCHK(c, dr.alloc((size_t)n * 15 * 8));
  HIPCHK(c, ds.alloc((size_t)n * 675 * 8));
  if (jac) HIPCHK(c, dj.alloc((size_t)n * 480 * 8));
  HIPCHK(c, hipMemcpyAsync(dp.p, params, (size_t)n * 32 * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dpre.p, h.data(), (size_t)n * sizeof(DevPreint), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_eval_imu, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, dp.d(), (const DevPreint*)dpre.p,
                     g_norm, dr.d(), jac ? dj.d() : nullptr, ds.d());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(residuals, dr.p, (size_t)n * 15 * 8, hipMemcpyDeviceToHost, c->stream));
  if (jac) HIPCHK(c, hipMemcpyAsync(jac, dj.p, (size_t)n * 480 * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VPL_OK;
}
int vpl_prior_factor_evaluate(vpl_ctx* c, const vpl_prior* pr, const double* params, double* residuals, double* jac) {
  if (!c || !pr || !params || !residuals || pr->n < 0 || pr->n > MAXPN || pr->n_blocks > MAXPB) return VPL_E_INVALID;
  if (pr->n == 0) return VPL_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int n = pr->n, nb = pr->n_blocks;
  int psz = 0;
  for (int b = 0; b < nb; ++b) psz += pr->block_kind[b] == VPL_BLOCK_SPEEDBIAS ? 9 : 7;
  DevBuf dk, di, dx0, dJ, dr0, dp, dr, dj;
  HIPCHK(c, dk.alloc(nb * 4)); HIPCHK(c, di.alloc(nb * 4)); HIPCHK(c, dx0.alloc(nb * 9 * 8));
  HIPCHK(c, dJ.alloc((size_t)n * n * 8)); HIPCHK(c, dr0.alloc(n * 8)); HIPCHK(c, dp.alloc(psz * 8));
  HIPCHK(c, dr.alloc(n * 8));
  if (jac) HIPCHK(c, dj.alloc((size_t)n * psz * 8));
  HIPCHK(c, hipMemcpyAsync(dk.p, pr->block_kind, nb * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(di.p, pr->block_idx, nb * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dx0.p, pr->x0, nb * 9 * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dJ.p, pr->J0, (size_t)n * n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dr0.p, pr->r0, n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dp.p, params, psz * 8, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_eval_prior, dim3(1), dim3(256), 0, c->stream, n, nb, (const int*)dk.p, (const int*)di.p, dx0.d(),
                     dJ.d(), dr0.d(), dp.d(), dr.d(), jac ? dj.d() : nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(residuals, dr.p, n * 8, hipMemcpyDeviceToHost, c->stream));
  if (jac) HIPCHK(c, hipMemcpyAsync(jac, dj.p, (size_t)n * psz * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VPL_OK;
}
int vpl_pose_plus(vpl_ctx* c, int n, const double* x, const double* delta, double* out) {
  return eval_generic(c, n, x, 7, delta, 6, 7, 0, out, nullptr, [&](double* p, double* k, double* r, double*) {
    hipLaunchKernelGGL(k_eval_pose_plus, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, p, k, r);
  });
}
int vpl_line_orth_plus(vpl_ctx* c, int n, const double* x, const double* delta, double* out) {
  return eval_generic(c, n, x, 4, delta, 4, 4, 0, out, nullptr, [&](double* p, double* k, double* r, double*) {
    hipLaunchKernelGGL(k_eval_orth_plus, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, p, k, r);
  });
}

// ---- window batch: upload (ba_upload.h) / solve / download --------------------------------------------------
// enqueues nothing (ba_restore.h): the next vpl_ba_solve restores inside k_prep, any other call that touches the states first
// issues the copies.  VPL_BA_RESET_FOLD=0: the copies at once.
int vpl_ba_reset_state(vpl_ctx* c) {
  if (c) { const int rs = settle_call(c); if (rs) return rs; }
  if (!c || c->nW < 1) return VPL_E_INVALID;
  return restore_event(c, RESTORE_EV_RESET);
}

int vpl_ba_upload(vpl_ctx* c, int nW, const vpl_window* win, const vpl_ba_options* opt) {
  return upload_impl(c, nW, win, opt, false);
}
int vpl_ba_upload_chained(vpl_ctx* c, int nW, const vpl_window* win, const vpl_ba_options* opt) {
  return upload_impl(c, nW, win, opt, false, true);
}

// k_prep: whitening matrices, q <- Quaterniond(R(q)), the world orth of the lines and J0^T J0 of the incoming prior; restore
// (a RestoreMode): every work-group first takes its window's states from the snapshots of the upload
static void launch_prep(vpl_ctx* c, const DevBatch& B, int nw, hipStream_t s, int restore = RESTORE_NONE) {
  KTimer t(c, "k_prep");
  hipLaunchKernelGGL(k_prep, dim3(nw), dim3(PREP_THREADS), prep_smem(c->maxPriorN), s, B, std::min(c->maxPriorN, PREP_NMAX), restore);
}
// the marginalisation of the uploaded flag: k_lin<1|2> linearises its factor subset at the current states, k_marg eliminates
// and factors the kept block (VPL_PRIOR_EIGEN: k_prior_eigen then replaces the factor by the reference's).  Nothing runs for MARGIN_NONE, nor for MARGIN_SECOND_NEW when every window passes its prior through.
static void launch_marg(vpl_ctx* c, DevBatch& B, int nw, hipStream_t s) {
  const bool old = c->opt.marginalization_flag == VPL_MARGIN_OLD;
  if (!old && !c->any_second_new) return;
  const dim3 grid(nw);
  { KTimer t(c, "k_lin_marg");
    if (old) hipLaunchKernelGGL(k_lin<1>, grid, dim3(LIN_THREADS), lin_smem(c->maxP, c->maxL), s, B);
    else hipLaunchKernelGGL(k_lin<2>, grid, dim3(LIN_THREADS), lin_smem(c->maxP, c->maxL), s, B); }
  ++B.launch;
  { KTimer t(c, "k_marg");
    if (c->marg_small) hipLaunchKernelGGL(k_marg<256>, grid, dim3(256), c->marg_smem, s, B);
    else hipLaunchKernelGGL(k_marg<MARG_THREADS>, grid, dim3(MARG_THREADS), c->marg_smem, s, B); }
  if (c->prior_rule == VPL_PRIOR_EIGEN) {   // the reference's factor of the kept block k_marg left in mg_A / mg_b
    KTimer t(c, "k_prior_eigen");
    hipLaunchKernelGGL(k_prior_eigen, grid, dim3(PRIOR_EIG_THREADS), prior_eig_layout(c->marg_nmax).bytes, s, B, c->marg_nmax);
  }
}
// FeatureManager::triangulate (points: k_triangulate_points, inverse depths back) and / or ::triangulateLine (lines:
// k_triangulate, flags + Pluecker vectors back) for a batch, on ONE upload with every line (the two touch different arrays:
// what solveOdometry's two threads start with)
// the kernels of the two triangulations on the uploaded batch (every line in it)
static void launch_triangulate(vpl_ctx* c, int nW, bool points, bool lines, double init_depth) {
  const DevBatch& B = c->B;
  hipStream_t s = c->stream;
  if (points) { KTimer t(c, "k_triangulate_points"); hipLaunchKernelGGL(k_triangulate_points, dim3(nW), dim3(128), 0, s, B, init_depth); }
  if (lines) { KTimer t(c, "k_triangulate"); hipLaunchKernelGGL(k_triangulate, dim3(nW), dim3(128), 0, s, B); }
}
static int triangulate_impl(vpl_ctx* c, int nW, vpl_window* win, bool points, bool lines, double init_depth, bool async) {
  if (!c || !win || nW < 1 || (points && !(init_depth > 0.0))) return VPL_E_INVALID;
  if (lines)
    for (int w = 0; w < nW; ++w)
      if (win[w].n_lines > 0 && !win[w].line_triangulated) return fail(c, VPL_E_INVALID, "line_triangulated is required");
  vpl_ba_options opt;
  vpl_ba_default_options(&opt);
  opt.marginalization_flag = VPL_MARGIN_NONE;
  int rc = upload_impl(c, nW, win, &opt, true);
  if (rc) return rc;
  DevBatch& B = c->B;
  hipStream_t s = c->stream;
  launch_triangulate(c, nW, points, lines, init_depth);
  HIPCHK(c, hipGetLastError());
  const size_t W = nW;
  struct Out { std::vector<double> invd, plk; std::vector<int> tri; };
  auto out = std::make_shared<Out>();
  if (points) {
    out->invd.resize(W * B.maxP);
    HIPCHK(c, hipMemcpyAsync(out->invd.data(), B.invd, out->invd.size() * 8, hipMemcpyDeviceToHost, s));
  }
  if (lines) {
    out->plk.resize(W * B.maxL * 6);
    out->tri.resize(W * B.maxL);
    HIPCHK(c, hipMemcpyAsync(out->plk.data(), B.plk, out->plk.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(out->tri.data(), B.ln_tri, out->tri.size() * 4, hipMemcpyDeviceToHost, s));
  }
  const int maxP = B.maxP, maxL = B.maxL;
  return finish_or_defer(c, async, [c, win, W, out, points, lines, maxP, maxL, s]() -> int {
    HIPCHK(c, hipStreamSynchronize(s));
    for (size_t w = 0; w < W; ++w) {
      vpl_window& v = win[w];
      if (points)
        for (int p = 0; p < v.n_points; ++p) v.inv_depth[p] = out->invd[w * maxP + p];
      if (lines) {
        const int* tri = &out->tri[w * maxL];
        scatter_lines(c, w, v, &out->plk[w * maxL * 6], [&](int dl, int l) {
          if (v.line_triangulated[l] || !tri[dl]) return false;
          v.line_triangulated[l] = 1;
          return true;
        });
      }
    }
    return VPL_OK;
  });
}
int vpl_ba_triangulate_lines(vpl_ctx* c, int nW, vpl_window* win) { return triangulate_impl(c, nW, win, false, true, 0.0, false); }
int vpl_ba_triangulate_lines_async(vpl_ctx* c, int nW, vpl_window* win) { return triangulate_impl(c, nW, win, false, true, 0.0, true); }
int vpl_ba_triangulate_points(vpl_ctx* c, int nW, vpl_window* win, double init_depth) {
  return triangulate_impl(c, nW, win, true, false, init_depth, false);
}
int vpl_ba_triangulate_points_async(vpl_ctx* c, int nW, vpl_window* win, double init_depth) {
  return triangulate_impl(c, nW, win, true, false, init_depth, true);
}

// Estimator::slideWindow for a batch.  The list bookkeeping (start frames, dropped observations, erased tracks) is integer
// work on the caller's arrays and is done here on the host; the re-anchoring arithmetic of removeBackShiftDepth runs in
// k_slide_shift over the gathered start-frame-0 survivors of all windows.
static int slide_window_impl(vpl_ctx* c, int nW, vpl_window* win, int flag, double init_depth, vpl_slide_tracks* out, bool async) {
  if (!c || !win || !out || nW < 1 || !(init_depth > 0.0)) return VPL_E_INVALID;
  if (flag != VPL_MARGIN_OLD && flag != VPL_MARGIN_SECOND_NEW) return fail(c, VPL_E_INVALID, "slide_window: marginalization_flag");
  constexpr int WS = VPL_NFRAMES - 1;
  for (int w = 0; w < nW; ++w) {
    const vpl_window& W = win[w];
    const vpl_slide_tracks& O = out[w];
    if ((W.n_points && (!O.point_start || !O.point_nobs || !O.point_drop || !W.point_start || !W.point_nobs || !W.point_obs || !W.inv_depth)) ||
        (W.n_lines && (!O.line_start || !O.line_nobs || !O.line_drop || !W.line_start || !W.line_nobs || !W.line_plk)))
      return fail(c, VPL_E_INVALID, "slide_window: null track array");
    for (int i = 0; i < W.n_points; ++i)
      if (W.point_nobs[i] < 1 || W.point_start[i] < 0 || W.point_start[i] + W.point_nobs[i] > VPL_NFRAMES)
        return fail(c, VPL_E_INVALID, "slide_window: point track outside the window");
    for (int i = 0; i < W.n_lines; ++i)
      if (W.line_nobs[i] < 1 || W.line_start[i] < 0 || W.line_start[i] + W.line_nobs[i] > VPL_NFRAMES)
        return fail(c, VPL_E_INVALID, "slide_window: line track outside the window");
  }
  HIPCHK(c, hipSetDevice(c->device));
  { const int rs = settle(c); if (rs) return rs; }
  // the per-track rule of the slide for both flags: odo_slide_track (csrc/odo_tracks.h), the session's
  const int second_new = flag == VPL_MARGIN_SECOND_NEW ? 1 : 0;
  for (int w = 0; w < nW; ++w) {
    const vpl_window& W = win[w];
    const vpl_slide_tracks& O = out[w];
    for (int i = 0; i < W.n_points; ++i) odo_slide_track(second_new, W.point_start[i], W.point_nobs[i], &O.point_start[i], &O.point_nobs[i], &O.point_drop[i]);
    for (int i = 0; i < W.n_lines; ++i) odo_slide_track(second_new, W.line_start[i], W.line_nobs[i], &O.line_start[i], &O.line_nobs[i], &O.line_drop[i]);
  }
  if (second_new) {   // removeFront(frame_count = WINDOW_SIZE): no arithmetic
    for (int w = 0; w < nW; ++w) {
      std::memcpy(win[w].pose[WS - 1], win[w].pose[WS], sizeof(win[w].pose[0]));
      std::memcpy(win[w].speed_bias[WS - 1], win[w].speed_bias[WS], sizeof(win[w].speed_bias[0]));
    }
    return VPL_OK;
  }
  struct SlideJob {
    std::vector<double> fr, pd, ld;
    std::vector<int> pw, lw, pidx, lidx;
    DevBuf dfr, dpw, dpd, dlw, dld;
  };
  auto job = std::make_shared<SlideJob>();
  std::vector<double>&fr = job->fr, &pd = job->pd, &ld = job->ld;
  std::vector<int>&pw = job->pw, &lw = job->lw, &pidx = job->pidx, &lidx = job->lidx;
  fr.resize((size_t)nW * 21);
  for (int w = 0; w < nW; ++w) {
    const vpl_window& W = win[w];
    std::memcpy(&fr[(size_t)w * 21], W.pose[0], 56);
    std::memcpy(&fr[(size_t)w * 21 + 7], W.pose[1], 56);
    std::memcpy(&fr[(size_t)w * 21 + 14], W.ex_pose, 56);
    size_t off = 0;
    // the survivors that started in frame 0 (their first observation leaves) are re-anchored
    for (int i = 0; i < W.n_points; off += W.point_nobs[i], ++i) {
      if (out[w].point_drop[i] != 0 || !out[w].point_nobs[i]) continue;
      pw.push_back(w); pidx.push_back(i);
      pd.insert(pd.end(), {W.point_obs[3 * off], W.point_obs[3 * off + 1], W.point_obs[3 * off + 2], W.inv_depth[i]});
    }
    for (int i = 0; i < W.n_lines; ++i) {
      if (out[w].line_drop[i] != 0 || !out[w].line_nobs[i]) continue;
      lw.push_back(w); lidx.push_back(i);
      ld.insert(ld.end(), W.line_plk + 6 * i, W.line_plk + 6 * i + 6);
    }
  }
  const int nPts = (int)pw.size(), nLns = (int)lw.size();
  hipStream_t s = c->stream;
  if (nPts + nLns > 0) {
    DevBuf &dfr = job->dfr, &dpw = job->dpw, &dpd = job->dpd, &dlw = job->dlw, &dld = job->dld;
    HIPCHK(c, dfr.alloc(fr.size() * 8)); HIPCHK(c, dpw.alloc(pw.size() * 4)); HIPCHK(c, dpd.alloc(pd.size() * 8));
    HIPCHK(c, dlw.alloc(lw.size() * 4)); HIPCHK(c, dld.alloc(ld.size() * 8));
    HIPCHK(c, hipMemcpyAsync(dfr.p, fr.data(), fr.size() * 8, hipMemcpyHostToDevice, s));
    if (nPts) { HIPCHK(c, hipMemcpyAsync(dpw.p, pw.data(), pw.size() * 4, hipMemcpyHostToDevice, s));
                HIPCHK(c, hipMemcpyAsync(dpd.p, pd.data(), pd.size() * 8, hipMemcpyHostToDevice, s)); }
    if (nLns) { HIPCHK(c, hipMemcpyAsync(dlw.p, lw.data(), lw.size() * 4, hipMemcpyHostToDevice, s));
                HIPCHK(c, hipMemcpyAsync(dld.p, ld.data(), ld.size() * 8, hipMemcpyHostToDevice, s)); }
    { KTimer t(c, "k_slide_shift");
      hipLaunchKernelGGL(k_slide_shift, dim3((nPts + nLns + 255) / 256), dim3(256), 0, s, dfr.d(), nPts, (const int*)dpw.p, dpd.d(),
                         nLns, (const int*)dlw.p, dld.d(), init_depth); }
    HIPCHK(c, hipGetLastError());
    if (nPts) HIPCHK(c, hipMemcpyAsync(pd.data(), dpd.p, pd.size() * 8, hipMemcpyDeviceToHost, s));
    if (nLns) HIPCHK(c, hipMemcpyAsync(ld.data(), dld.p, ld.size() * 8, hipMemcpyDeviceToHost, s));
  }
  // (the job owns the staging vectors and the device buffers until the results have been scattered)
  return finish_or_defer(c, async, [c, win, nW, job, nPts, nLns, s]() -> int {
    if (nPts + nLns > 0) {
      HIPCHK(c, hipStreamSynchronize(s));
      for (int k = 0; k < nPts; ++k) win[job->pw[k]].inv_depth[job->pidx[k]] = job->pd[(size_t)k * 4 + 3];
      for (int k = 0; k < nLns; ++k) std::memcpy(win[job->lw[k]].line_plk + 6 * job->lidx[k], &job->ld[(size_t)k * 6], 48);
    }
    for (int w = 0; w < nW; ++w) {
      std::memmove(win[w].pose[0], win[w].pose[1], sizeof(win[w].pose[0]) * WS);            // frames 1..10 -> 0..9, 10 stays
      std::memmove(win[w].speed_bias[0], win[w].speed_bias[1], sizeof(win[w].speed_bias[0]) * WS);
    }
    return VPL_OK;
  });
}
int vpl_ba_slide_window(vpl_ctx* c, int nW, vpl_window* win, int flag, double init_depth, vpl_slide_tracks* out) {
  return slide_window_impl(c, nW, win, flag, init_depth, out, false);
}
int vpl_ba_slide_window_async(vpl_ctx* c, int nW, vpl_window* win, int flag, double init_depth, vpl_slide_tracks* out) {
  return slide_window_impl(c, nW, win, flag, init_depth, out, true);
}

// Estimator::onlyLineOpt for a batch: upload (triangulated lines), k_prep (world orth of the lines), k_line_opt (the LM
// loop), k_gauge (setLineOrth + removeLineOutlier; the gauge transform is the identity, the poses did not move)
// solve_opt != nullptr (vpl_ba_solve_odometry): the upload is made with the options of the solve that FOLLOWS, so that the
// batch -- layout tables, observations, prior, kept-block tables -- can stay where it is for that solve when onlyLineOpt
// erases no line; the line kernels run on a copy of the batch descriptor with onlyLineOpt's own flags.
// the kernels of onlyLineOpt on the uploaded batch (its triangulated lines): they run on a copy of the batch descriptor with
// onlyLineOpt's own flags -- no marginalisation, removeLineOutlier at the end (estimator.cpp:1037)
static void launch_line_opt(vpl_ctx* c, int nW) {
  DevBatch B = c->B;
  B.opt.marginalization_flag = VPL_MARGIN_NONE;
  B.opt.remove_line_outliers = 1;
  const dim3 grid(nW);
  hipStream_t s = c->stream;
  launch_prep(c, B, nW, s);
  {
    KTimer t(c, "k_line_opt");
    if (4 * c->maxL <= LOPT_THREADS) hipLaunchKernelGGL(k_line_opt<4>, grid, dim3(LOPT_THREADS), 0, s, B);
    else if (2 * c->maxL <= LOPT_THREADS) hipLaunchKernelGGL(k_line_opt<2>, grid, dim3(LOPT_THREADS), 0, s, B);
    else hipLaunchKernelGGL(k_line_opt<1>, grid, dim3(LOPT_THREADS), 0, s, B);
  }
  { KTimer t(c, "k_gauge"); hipLaunchKernelGGL(k_gauge, grid, dim3(128), 0, s, B); }
}
static int only_line_opt_impl(vpl_ctx* c, int nW, vpl_window* win, const vpl_ba_options* opt_in, vpl_solve_report* reports, bool async,
                              const vpl_ba_options* solve_opt = nullptr) {
  if (!c || !win || !opt_in || nW < 1) return VPL_E_INVALID;
  if (c->maxL > LOPT_THREADS) return fail(c, VPL_E_CAPACITY, "onlyLineOpt handles at most 256 lines per window");
  vpl_ba_options opt = *opt_in;
  opt.marginalization_flag = VPL_MARGIN_NONE;
  opt.remove_line_outliers = 1;          // f_manager.removeLineOutlier at the end of onlyLineOpt (estimator.cpp:1037)
  int rc = upload_impl(c, nW, win, solve_opt ? solve_opt : &opt, false);
  if (rc) return rc;
  const DevBatch& B = c->B;
  hipStream_t s = c->stream;
  launch_line_opt(c, nW);
  HIPCHK(c, hipGetLastError());
  const size_t W = nW;
  auto plk = std::make_shared<std::vector<double>>(W * B.maxL * 6);
  auto removed = std::make_shared<std::vector<int>>(W * B.maxL);
  auto tr = std::make_shared<std::vector<TrState>>(W);
  HIPCHK(c, hipMemcpyAsync(plk->data(), B.plk, plk->size() * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(removed->data(), B.ln_removed, removed->size() * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(tr->data(), B.tr, W * sizeof(TrState), hipMemcpyDeviceToHost, s));
  const int maxL = B.maxL;
  return finish_or_defer(c, async, [c, win, reports, W, plk, removed, tr, maxL, s]() -> int {
    HIPCHK(c, hipStreamSynchronize(s));
    for (size_t w = 0; w < W; ++w) {
      vpl_window& v = win[w];
      if (reports) std::memset(&reports[w], 0, sizeof(reports[w]));
      if (c->h_lmap[w].size() < 4) {       // "if (feature_index < 3) return;" -- nothing is touched
        if (v.line_removed) std::fill(v.line_removed, v.line_removed + v.n_lines, 0);
        continue;
      }
      const int nrem = scatter_solved_lines(c, w, v, &(*plk)[w * maxL * 6], &(*removed)[w * maxL]);
      if (reports) {
        fill_report(reports[w], (*tr)[w]);
        reports[w].n_lines_removed = nrem;
      }
    }
    return VPL_OK;
  });
}
int vpl_ba_only_line_opt(vpl_ctx* c, int nW, vpl_window* win, const vpl_ba_options* opt, vpl_solve_report* reports) {
  return only_line_opt_impl(c, nW, win, opt, reports, false);
}
int vpl_ba_only_line_opt_async(vpl_ctx* c, int nW, vpl_window* win, const vpl_ba_options* opt, vpl_solve_report* reports) {
  return only_line_opt_impl(c, nW, win, opt, reports, true);
}

// The whole solve of the windows [w0, w0 + nw) on stream s; restore: see launch_prep
static void launch_solve(vpl_ctx* c, int w0, int nw, hipStream_t s, int restore) {
  DevBatch B = c->B;
  B.ord_it = 0;
  // with kernel timing on, every launch also counts the windows that did work in it (vpl_ba_launch_profile)
  B.act = c->timing ? c->d_act : nullptr;
  B.launch = 0;
  B.step_fused = c->step_fused && !c->timing;
  if (c->timing) { c->ltimes.clear(); (void)hipMemsetAsync(c->d_act, 0, sizeof(int) * ACT_SLOTS * 4, s); }   // (counts only)
  const dim3 grid(nw);
  launch_prep(c, B, nw, s, restore);
  ++B.launch;
  { KTimer t(c, "k_lin"); hipLaunchKernelGGL(k_lin2, dim3(16 * ((nw + 7) / 8)), dim3(LIN_THREADS), lin_smem(c->maxP, c->maxL), s, B); }
  ++B.launch;
  // The shape of the landmark elimination: three column tiles when every compact row fits them; for rows wider than 6 frames
  // all five, or (few long tracks) the mixed form: narrow view for the entries of short tracks, all tiles for the flagged ones.
  const bool narrow = B.WS + 2 <= 48, wide = !narrow && (c->schur_wide_all || (c->schur_mostly_wide && !c->schur_never_wide));
  const int ntc = wide ? 5 : 3;
  void (*const kstep)(DevBatch) = narrow ? k_step<3, false> : wide ? k_step<5, false> : k_step<3, true>;
  void (*const kschur)(DevBatch) = narrow ? k_schur<3> : wide ? k_schur<5> : k_schur_mixed;
  for (int it = 0; it < c->opt.num_iterations; ++it) {
    B.ord_it = it;      // k_solve / k_cost of iteration `it` walk order[it & 1]; k_cost fills order[(it + 1) & 1]
    // the step: landmark elimination -> reduced camera system -> landmark back-substitution + dogleg + candidate; the general
    // path (windows flagged in B.path only) after it, or before the back-substitution in the three-launch form.
    // One launch (k_step) unless the solve is timed kernel by kernel: the timing mode attributes time and active windows
    // per phase (vpl_ba_launch_profile) and issues the same bodies as three launches -- the same bits.
    if (B.step_fused) {
      hipLaunchKernelGGL(kstep, grid, dim3(SCHUR_THREADS), step_smem(B.maxP, B.maxL, ntc), s, B);
      ++B.launch;
      hipLaunchKernelGGL(k_solve, grid, dim3(SOLVE_THREADS), solve_smem(B.maxP, B.maxL), s, B);
      ++B.launch;
    } else {
      { KTimer t(c, "k_schur"); hipLaunchKernelGGL(kschur, grid, dim3(SCHUR_THREADS), schur_smem(B.maxP, B.maxL, ntc), s, B); }
      ++B.launch;
      { KTimer t(c, "k_chol"); hipLaunchKernelGGL(k_chol, grid, dim3(CHOL_THREADS), chol_smem(), s, B); }
      ++B.launch;
      { KTimer t(c, "k_solve"); hipLaunchKernelGGL(k_solve, grid, dim3(SOLVE_THREADS), solve_smem(B.maxP, B.maxL), s, B); }
      ++B.launch;
      { KTimer t(c, "k_back"); hipLaunchKernelGGL(k_back, grid, dim3(BACK_THREADS), back_smem(B.maxP, B.maxL), s, B); }
      ++B.launch;
    }
    { KTimer t(c, "k_cost"); hipLaunchKernelGGL(k_cost, grid, dim3(COST_THREADS), 0, s, B); }
    ++B.launch;
    if (it + 1 < c->opt.num_iterations) {
      B.ord_it = it + 1;
      KTimer t(c, "k_lin");
      hipLaunchKernelGGL(k_lin2, dim3(16 * ((nw + 7) / 8)), dim3(LIN_THREADS), lin_smem(c->maxP, c->maxL), s, B);
    }
    if (it + 1 < c->opt.num_iterations) ++B.launch;
  }
  B.ord_it = 0;
  { KTimer t(c, "k_gauge"); hipLaunchKernelGGL(k_gauge, grid, dim3(128), 0, s, B); }
  ++B.launch;
  launch_marg(c, B, nw, s);
}

// vpl_ba_solve: the kernel-per-phase sequence over the whole batch, asynchronous on the context's stream.
int vpl_ba_solve(vpl_ctx* c) {
  if (c) { const int rs = settle_call(c); if (rs) return rs; }
  if (!c || c->nW < 1) return VPL_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  int restore = RESTORE_NONE;      // a pending vpl_ba_reset_state: k_prep's work-groups restore their windows
  { const int rr = restore_event(c, RESTORE_EV_SOLVE, &restore); if (rr) return rr; }
  if (c->opt.marginalization_flag != VPL_MARGIN_NONE) { c->prior_resident = true; c->prior_resident_nW = c->nW; }
  if (c->leg_timing) {
    HIPCHK(c, hipEventRecord(c->leg_ev[2], c->stream));
    launch_solve(c, 0, c->nW, c->stream, restore);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->leg_ev[3], c->stream));
    return VPL_OK;
  }
  if (c->use_graph && !c->timing && c->stream != nullptr) {   // (the legacy default stream cannot be captured)
    hipGraphExec_t& exec = c->graph_exec[restore];   // (the restore mode is a kernel argument: one instance per mode)
    if (!exec) {
      hipGraph_t graph = nullptr;
      HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
      launch_solve(c, 0, c->nW, c->stream, restore);
      HIPCHK(c, hipStreamEndCapture(c->stream, &graph));
      hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      (void)hipGraphDestroy(graph);   // (the instance does not need it)
      if (e != hipSuccess) { exec = nullptr; return fail(c, VPL_E_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e)); }
    }
    HIPCHK(c, hipGraphLaunch(exec, c->stream));
    return VPL_OK;
  }
  launch_solve(c, 0, c->nW, c->stream, restore);
  HIPCHK(c, hipGetLastError());
  return VPL_OK;
}

// priors of the last marginalisation (k_marg) of the uploaded batch -> host; mn[2 w] = m, mn[2 w + 1] = n.
// Two steps around ONE device-to-host copy of the staging arena: plan (pieces of the arena + gather segments, a stage_plan), then
// -- after stage_run and a stream synchronisation -- finish (scatter into the caller's vpl_prior structs).
struct PriorFetch {
  Span<int> mg_n, mg_nb, mg_kind, mg_frame, mg_idx, mg_m;
  Span<double> mg_x0, mg_r0;
  std::vector<Span<double>> J0;   // per window: the host-side bound of the kept dims, squared
};
static void prior_fetch_plan(vpl_ctx* c, int nW, PriorFetch& F, Stage& S) {
  const DevBatch& B = c->B;
  const size_t W = nW;
  F.mg_m = S.take<int>(W); F.mg_n = S.take<int>(W); F.mg_nb = S.take<int>(W);
  F.mg_kind = S.take<int>(W * MAXPB); F.mg_frame = S.take<int>(W * MAXPB); F.mg_idx = S.take<int>(W * MAXPB);
  F.mg_x0 = S.take<double>(W * MAXPB * 9); F.mg_r0 = S.take<double>(W * MAXKEEP);
  S.from_device(F.mg_m.p, B.mg_m, W); S.from_device(F.mg_n.p, B.mg_n, W); S.from_device(F.mg_nb.p, B.mg_nb, W);
  S.from_device(F.mg_kind.p, B.mg_kind, W * MAXPB); S.from_device(F.mg_frame.p, B.mg_frame, W * MAXPB);
  S.from_device(F.mg_idx.p, B.mg_idx, W * MAXPB);
  S.from_device(F.mg_x0.p, B.mg_x0, W * MAXPB * 9); S.from_device(F.mg_r0.p, B.mg_r0, W * MAXKEEP);
  F.J0.resize(W);
  for (size_t w = 0; w < W; ++w) {
    const int n = w < c->h_mg_n.size() ? std::min(std::max(c->h_mg_n[w], 0), (int)MAXKEEP) : (int)MAXKEEP;
    F.J0[w] = S.take<double>((size_t)n * n);
    S.from_device(F.J0[w].p, B.mg_J0 + w * (size_t)MAXKEEP * MAXKEEP, (size_t)n * n);
  }
}
static int prior_fetch_finish(vpl_ctx* c, int nW, const PriorFetch& F, vpl_prior* priors, std::vector<int>& mn) {
  DevBatch& B = c->B;
  const size_t W = nW;
  const Span<int>&mg_n = F.mg_n, &mg_nb = F.mg_nb, &mg_kind = F.mg_kind, &mg_frame = F.mg_frame, &mg_idx = F.mg_idx, &mg_m = F.mg_m;
  const Span<double>& mg_x0 = F.mg_x0, &mg_r0 = F.mg_r0;
  mn.assign(2 * W, 0);
  for (size_t w = 0; w < W; ++w) {
    mn[2 * w] = mg_m[w];
    if (c->h_passthrough[w] >= 0) {   // MARGIN_SECOND_NEW without pose WINDOW_SIZE-1 in the prior: the prior stays (estimator.cpp:1385)
      priors[w] = c->h_pass_priors[c->h_passthrough[w]];
      if (priors[w].n < 0) {          // chained upload: the untouched prior lives on the device only
        vpl_prior& p = priors[w];
        std::memset(&p, 0, sizeof(int) * (2 + 3 * VPL_MAX_PRIOR_BLOCKS));
        HIPCHK(c, hipMemcpy(&p.n, B.pr_n + w, 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&p.n_blocks, B.pr_nb + w, 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(p.block_kind, B.pr_kind + w * MAXPB, MAXPB * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(p.block_frame, B.pr_frame + w * MAXPB, MAXPB * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(p.block_idx, B.pr_idx + w * MAXPB, MAXPB * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(p.x0, B.pr_x0 + w * MAXPB * 9, MAXPB * 9 * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(p.J0, B.pr_J0 + w * (size_t)B.prS, (size_t)p.n * p.n * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(p.r0, B.pr_r0 + w * MAXPN, (size_t)p.n * 8, hipMemcpyDeviceToHost));
      }
      mn[2 * w + 1] = priors[w].n;
      continue;
    }
    vpl_prior& p = priors[w];
    std::memset(&p, 0, sizeof(int) * (2 + 3 * VPL_MAX_PRIOR_BLOCKS));
    const int n = mg_n[w];
    p.n = n; p.n_blocks = mg_nb[w];
    mn[2 * w + 1] = n;
    for (int b = 0; b < p.n_blocks; ++b) {
      p.block_kind[b] = mg_kind[w * MAXPB + b];
      p.block_frame[b] = mg_frame[w * MAXPB + b];
      p.block_idx[b] = mg_idx[w * MAXPB + b];
      std::memcpy(p.x0[b], &mg_x0[(w * MAXPB + b) * 9], 9 * 8);
    }
    if ((size_t)n * n > F.J0[w].n) return fail(c, VPL_E_HIP, "internal: the device kept more prior dims than the host's bound");
    std::memcpy(p.J0, F.J0[w].p, (size_t)n * n * 8);
    std::memcpy(p.r0, &mg_r0[w * MAXKEEP], (size_t)n * 8);
  }
  return VPL_OK;
}
static int fetch_priors(vpl_ctx* c, int nW, vpl_prior* priors, std::vector<int>& mn) {
  PriorFetch F;
  auto plan = [&](Stage& S) { prior_fetch_plan(c, nW, F, S); };
  HIPCHK(c, stage_plan(c->stage, plan));
  HIPCHK(c, stage_run(c->stage, c->stream, false));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return prior_fetch_finish(c, nW, F, priors, mn);
}

// States of the uploaded batch -> caller's DEVICE buffer [nW][183], asynchronous on the context's stream
int vpl_ba_pack_states_device(vpl_ctx* c, int nW, void* d_states) {
  if (c) { const int rs = settle(c); if (rs) return rs; }
  if (!c || nW != c->nW || !d_states) return VPL_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(k_pack_states, dim3(nW), dim3(192), 0, c->stream, c->B, (double*)d_states);
  HIPCHK(c, hipGetLastError());
  return VPL_OK;
}

int vpl_ba_download(vpl_ctx* c, int nW, vpl_window* win, vpl_prior* priors, vpl_solve_report* reports) {
  if (c) { const int rs = settle(c); if (rs) return rs; }
  if (!c || nW != c->nW || !win) return VPL_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  DevBatch& B = c->B;
  const size_t W = nW;
  const bool marg = priors != nullptr && c->opt.marginalization_flag != VPL_MARGIN_NONE;
  hipStream_t s = c->stream;
  if (c->leg_timing) HIPCHK(c, hipEventRecord(c->leg_ev[4], s));
  // one gather kernel into the device arena, ONE device-to-host copy into the pinned arena
  Span<double> pose, sb, ex, invd, plk;
  Span<TrState> tr;
  Span<int> mg_m, removed;
  PriorFetch F;
  auto plan = [&](Stage& S) {
    pose = S.take<double>(W * 77); sb = S.take<double>(W * 99); ex = S.take<double>(W * 7); invd = S.take<double>(W * B.maxP);
    plk = S.take<double>(W * B.maxL * 6);
    tr = S.take<TrState>(W);
    mg_m = S.take<int>(W); removed = S.take<int>(W * B.maxL);
    S.from_device(pose.p, B.pose, W * 77); S.from_device(sb.p, B.sb, W * 99); S.from_device(ex.p, B.ex, W * 7);
    S.from_device(invd.p, B.invd, W * B.maxP); S.from_device(plk.p, B.plk, W * B.maxL * 6); S.from_device(tr.p, B.tr, W);
    S.from_device(mg_m.p, B.mg_m, W); S.from_device(removed.p, B.ln_removed, W * B.maxL);
    if (marg) prior_fetch_plan(c, nW, F, S);
  };
  HIPCHK(c, stage_plan(c->stage, plan));
  HIPCHK(c, stage_run(c->stage, c->stream, false));
  if (c->leg_timing) HIPCHK(c, hipEventRecord(c->leg_ev[5], s));
  HIPCHK(c, hipStreamSynchronize(s));
  std::vector<int> mn;
  if (marg) {
    const int rc = prior_fetch_finish(c, nW, F, priors, mn);
    if (rc) return rc;
  }
  for (size_t w = 0; w < W; ++w) {
    vpl_window& v = win[w];
    std::memcpy(v.pose, &pose[w * 77], 77 * 8);
    std::memcpy(v.speed_bias, &sb[w * 99], 99 * 8);
    std::memcpy(v.ex_pose, &ex[w * 7], 7 * 8);
    for (int p = 0; p < v.n_points; ++p) v.inv_depth[p] = invd[w * B.maxP + p];
    // erased tracks keep the caller's value (they are gone from f_manager)
    const int nrem = scatter_solved_lines(c, w, v, &plk[w * B.maxL * 6], &removed[w * B.maxL]);
    if (reports) {
      vpl_solve_report& r = reports[w];
      fill_report(r, tr[w]);
      r.prior_m = mg_m[w];
      r.prior_n = marg ? mn[2 * w + 1] : 0;
      r.n_lines_removed = nrem;
    }
  }
  return VPL_OK;
}

// MarginalizationInfo::{addResidualBlockInfo, preMarginalize, marginalize} for a batch of windows WITHOUT a solve
// (marginalization_factor.cpp:89-129,177-363 as driven by estimator.cpp:1229-1447): the factor subset of the flag is
// linearised at the windows' current states (k_lin<1|2>), the landmarks and the dropped frame are eliminated and the kept
// block is factored into (J0, r0) (k_marg).  The states are not touched.
static int marginalize_impl(vpl_ctx* c, int nW, const vpl_window* win, const vpl_ba_options* opt_in, int marginalization_flag,
                            vpl_prior* priors, int* m_out, int* n_out, bool async) {
  if (!c || !win || !opt_in || !priors || nW < 1) return VPL_E_INVALID;
  if (marginalization_flag != VPL_MARGIN_OLD && marginalization_flag != VPL_MARGIN_SECOND_NEW)
    return fail(c, VPL_E_INVALID, "vpl_ba_marginalize: flag must be VPL_MARGIN_OLD or VPL_MARGIN_SECOND_NEW");
  vpl_ba_options opt = *opt_in;
  opt.marginalization_flag = marginalization_flag;
  opt.remove_line_outliers = 0;
  int rc = upload_impl(c, nW, win, &opt, false);
  if (rc) return rc;
  DevBatch B = c->B;
  B.ord_it = 0; B.act = nullptr; B.launch = 0;
  hipStream_t s = c->stream;
  // no line of this call is erased (remove_line_outliers = 0 above): the flags k_lin<MARG> and k_marg read are written by
  // k_gauge, which runs in a solve only -- without this they would be those of the batch the context solved before
  HIPCHK(c, hipMemsetAsync(B.ln_removed, 0, (size_t)nW * B.maxL * sizeof(int), s));
  // k_prep runs the vector2double() the reference runs before it marginalises (estimator.cpp:1233)
  launch_prep(c, B, nW, s);
  launch_marg(c, B, nW, s);   // (B.act is null: the launch counter it steps is not read)
  c->prior_resident = true; c->prior_resident_nW = nW;
  HIPCHK(c, hipGetLastError());
  // (the priors are fetched from the device when the call completes: any later call on the context completes this one first)
  return finish_or_defer(c, async, [c, nW, priors, m_out, n_out]() -> int {
    std::vector<int> mn;
    const int rf = fetch_priors(c, nW, priors, mn);
    if (rf) return rf;
    for (int w = 0; w < nW; ++w) {
      if (m_out) m_out[w] = mn[2 * w];
      if (n_out) n_out[w] = mn[2 * w + 1];
    }
    return VPL_OK;
  });
}
int vpl_ba_marginalize(vpl_ctx* c, int nW, const vpl_window* win, const vpl_ba_options* opt, int marginalization_flag,
                       vpl_prior* priors, int* m_out, int* n_out) {
  return marginalize_impl(c, nW, win, opt, marginalization_flag, priors, m_out, n_out, false);
}
int vpl_ba_marginalize_async(vpl_ctx* c, int nW, const vpl_window* win, const vpl_ba_options* opt, int marginalization_flag,
                             vpl_prior* priors, int* m_out, int* n_out) {
  return marginalize_impl(c, nW, win, opt, marginalization_flag, priors, m_out, n_out, true);
}

int vpl_ba_solve_windows(vpl_ctx* c, int nW, vpl_window* win, const vpl_ba_options* opt, vpl_prior* priors,
                         vpl_solve_report* reports) {
  int rc = vpl_ba_upload(c, nW, win, opt);
  if (rc) return rc;
  rc = vpl_ba_solve(c);
  if (rc) return rc;
  rc = vpl_ctx_synchronize(c);
  if (rc) return rc;
  return vpl_ba_download(c, nW, win, priors, reports);
}

// Stage 3 of solveOdometry on the batch onlyLineOpt was uploaded with (the final solve's options) when it erased no line.
// What a fresh upload would put on the device is there already: the layout tables, observations, prior and kept-block tables
// of this very line set, the optimised Pluecker vectors (the caller's copy, or the session's, was written from B.plk), and
// -- after this restore -- the states k_prep re-normalised in place.  Same bits as the four-stage call.
static int reuse_line_opt_batch(vpl_ctx* c) {
  HIPCHK(c, hipMemsetAsync(c->B.ln_removed, 0, (size_t)c->nW * c->B.maxL * 4, c->stream));
  return restore_event(c, RESTORE_EV_REUSE);
}

// Estimator::solveOdometry (estimator.cpp:624-648) for a batch, in one call: triangulate || (triangulateLine -> onlyLineOpt)
// -> optimizationwithLine.  The two line stages change WHICH lines take part (newly triangulated ones join, the ones
// removeLineOutlier erases leave), and the lane / unit / K-step tables of the kernels are built on the host from that set: the
// stages are the entry points above run back to back on the caller's arrays (the two triangulations share one upload).
int vpl_ba_solve_odometry(vpl_ctx* c, int nW, vpl_window* win, const vpl_ba_options* opt, double init_depth,
                          vpl_prior* priors, vpl_solve_report* line_reports, vpl_solve_report* reports) {
  if (!c || !win || !opt || nW < 1) return VPL_E_INVALID;
  bool any_lines = false;
  for (int w = 0; w < nW; ++w)
    if (win[w].n_lines > 0) {
      any_lines = true;
      if (!win[w].line_triangulated || !win[w].line_removed)
        return fail(c, VPL_E_INVALID, "solve_odometry: line_triangulated and line_removed are required for windows with lines");
    }
  using oclk = std::chrono::steady_clock;
  const auto t0 = oclk::now();
  int rc = triangulate_impl(c, nW, win, true, any_lines, init_depth, false);
  if (rc) return rc;
  const auto t1 = oclk::now();
  c->odo_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
  c->odo_ms[1] = 0.0;
  bool batch_resident = false;
  if (any_lines) {
    bool orth_given = false;
    for (int w = 0; w < nW; ++w) orth_given = orth_given || win[w].line_orth != nullptr;
    // uploaded with the FINAL solve's options: when no line is erased the same batch is solved where it lies (round 4)
    rc = only_line_opt_impl(c, nW, win, opt, line_reports, false, orth_given ? nullptr : opt);
    c->odo_ms[1] = std::chrono::duration<double, std::milli>(oclk::now() - t1).count();
    if (rc) return rc;
    // f_manager.removeLineOutlier erased these tracks (estimator.cpp:1037): they take no part in the solve
    bool erased = false;
    for (int w = 0; w < nW; ++w)
      for (int l = 0; l < win[w].n_lines; ++l)
        if (win[w].line_removed[l]) { win[w].line_triangulated[l] = 0; erased = true; }
    batch_resident = !erased && !orth_given;
  } else if (line_reports) {
    std::memset(line_reports, 0, sizeof(vpl_solve_report) * (size_t)nW);
  }
  const auto t2 = oclk::now();
  // optimizationwithLine: on the batch where it lies, or on a fresh upload of the lines that are left
  rc = batch_resident ? reuse_line_opt_batch(c) : vpl_ba_upload(c, nW, win, opt);
  if (!rc) rc = vpl_ba_solve(c);
  if (!rc) rc = vpl_ctx_synchronize(c);
  if (!rc) rc = vpl_ba_download(c, nW, win, priors, reports);
  c->odo_ms[2] = std::chrono::duration<double, std::milli>(oclk::now() - t2).count();
  return rc;
}
// wall clock of the three stages of the last vpl_ba_solve_odometry: triangulation | onlyLineOpt | optimizationwithLine (ms)
int vpl_ba_debug_odometry_ms(vpl_ctx* c, double* ms3) {
  if (!c || !ms3) return VPL_E_INVALID;
  for (int k = 0; k < 3; ++k) ms3[k] = c->odo_ms[k];
  return VPL_OK;
}

// Debug/test access to the marginalisation invariants (A, b before the final eigen-decomposition),
// mirroring the reference's commented check at marginalization_factor.cpp:361-362.
int vpl_ba_debug_marg_Ab(vpl_ctx* c, int w, double* A, double* b) {
  if (!c || w < 0 || w >= c->nW) return VPL_E_INVALID;
  int n = 0;
  HIPCHK(c, hipMemcpy(&n, c->B.mg_n + w, 4, hipMemcpyDeviceToHost));
  std::vector<double> t((size_t)n * n);
  HIPCHK(c, hipMemcpy(A, c->B.mg_A + (size_t)w * MAXKEEP * MAXKEEP, (size_t)n * n * 8, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(b, c->B.mg_b + (size_t)w * MAXKEEP, (size_t)n * 8, hipMemcpyDeviceToHost));
  return n;
}

// Debug/test access to what the trust-region step kernels read and write for ONE window of the uploaded batch (tests/
// test_gpu_step_kernels.py): both calls complete whatever is enqueued on the context, wait for its stream, copy device
// buffers and launch nothing.  Full index of the window: 171 cam dims | nP inverse depths | 4 nL line dims -- the window's own
// counts, not the context's strides; device line l is the caller's line line_index[l] (untriangulated lines do not travel).
static int debug_window_ready(vpl_ctx* c, int w) {
  if (!c) return VPL_E_INVALID;
  const int rs = settle(c);
  if (rs) return rs;
  if (c->upload_open || w < 0 || w >= c->nW || (size_t)w >= c->h_nP.size() || (size_t)w >= c->h_lmap.size())
    return fail(c, VPL_E_INVALID, "debug read-out: no such window in the uploaded batch");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VPL_OK;
}
static hipError_t debug_fetch_d(std::vector<double>& dst, const double* src, size_t n) {
  dst.assign(n ? n : 1, 0.0);
  return n ? hipMemcpy(dst.data(), src, n * 8, hipMemcpyDeviceToHost) : hipSuccess;
}
static hipError_t debug_fetch_i(std::vector<int>& dst, const int* src, size_t n) {
  dst.assign(n ? n : 1, 0);
  return n ? hipMemcpy(dst.data(), src, n * 4, hipMemcpyDeviceToHost) : hipSuccess;
}
// the five state arrays of window w (x: B.pose ..., the candidate: B.pose_c ...) in the window's own counts
static int debug_states(vpl_ctx* c, int w, int nP, int nL, const double* dpose, const double* dsb, const double* dex,
                        const double* dinvd, const double* dorth, double* pose, double* sb, double* ex, double* invd, double* orth) {
  const DevBatch& B = c->B;
  if (pose) HIPCHK(c, hipMemcpy(pose, dpose + (size_t)w * 77, 77 * 8, hipMemcpyDeviceToHost));
  if (sb) HIPCHK(c, hipMemcpy(sb, dsb + (size_t)w * 99, 99 * 8, hipMemcpyDeviceToHost));
  if (ex) HIPCHK(c, hipMemcpy(ex, dex + (size_t)w * 7, 7 * 8, hipMemcpyDeviceToHost));
  if (invd && nP) HIPCHK(c, hipMemcpy(invd, dinvd + (size_t)w * B.maxP, (size_t)nP * 8, hipMemcpyDeviceToHost));
  if (orth && nL) HIPCHK(c, hipMemcpy(orth, dorth + (size_t)w * B.maxL * 4, (size_t)nL * 4 * 8, hipMemcpyDeviceToHost));
  return VPL_OK;
}
// a vector over the context's full index [171 | maxP | 4 maxL] -> the window's [171 | nP | 4 nL]
static int debug_full_vector(vpl_ctx* c, int w, int nP, int nL, const double* dsrc, double* out) {
  if (!out) return VPL_OK;
  const DevBatch& B = c->B;
  const double* src = dsrc + (size_t)w * B.nfull;
  HIPCHK(c, hipMemcpy(out, src, NC * 8, hipMemcpyDeviceToHost));
  if (nP) HIPCHK(c, hipMemcpy(out + NC, src + NC, (size_t)nP * 8, hipMemcpyDeviceToHost));
  if (nL) HIPCHK(c, hipMemcpy(out + NC + nP, src + NC + B.maxP, (size_t)nL * 4 * 8, hipMemcpyDeviceToHost));
  return VPL_OK;
}

// The linearisation k_lin left for window w, expanded on the host into the dense symmetric H [n][n] and g [n] over the full
// index: the packed camera Hessian, the diagonal landmark blocks, and the compact W rows of every landmark spread over the
// camera columns of the frames they cover (wcol, vis2cam).  Slots of a compact row that no factor writes are read like every
// other: the step kernels read them too.  x_*: the current states, x_cost: TrState::x_cost.  Returns n; H = NULL: only the
// counts (n_points, n_lines) and n, nothing is read from the device.
int vpl_ba_debug_linearization(vpl_ctx* c, int w, int* n_points, int* n_lines, int* line_index, double* H, double* g,
                               double* x_pose, double* x_speed_bias, double* x_ex_pose, double* x_inv_depth, double* x_line_orth,
                               double* x_cost) {
  const int rc = debug_window_ready(c, w);
  if (rc) return rc;
  const DevBatch& B = c->B;
  const int nP = c->h_nP[w], nL = (int)c->h_lmap[w].size();
  const int n = NC + nP + 4 * nL;
  if (nP < 0 || nP > B.maxP || nL > B.maxL) return fail(c, VPL_E_INVALID, "debug read-out: counts outside the context's capacity");
  if (n_points) *n_points = nP;
  if (n_lines) *n_lines = nL;
  if (line_index) for (int l = 0; l < nL; ++l) line_index[l] = c->h_lmap[w][l];
  if (!H || !g) return n;
  const int WS = B.WS;
  std::vector<double> Hcc, gc, Hpp, gp, Wp, Hll, gl, Wl;
  std::vector<int> ps, ls;
  HIPCHK(c, debug_fetch_d(Hcc, B.Hcc + (size_t)w * NCP, NCP));
  HIPCHK(c, debug_fetch_d(gc, B.gc + (size_t)w * NC, NC));
  HIPCHK(c, debug_fetch_d(Hpp, B.Hpp + (size_t)w * B.maxP, nP));
  HIPCHK(c, debug_fetch_d(gp, B.gp + (size_t)w * B.maxP, nP));
  HIPCHK(c, debug_fetch_d(Wp, B.Wp + (size_t)w * B.maxP * WS, (size_t)nP * WS));
  HIPCHK(c, debug_fetch_d(Hll, B.Hll + (size_t)w * B.maxL * 16, (size_t)nL * 16));
  HIPCHK(c, debug_fetch_d(gl, B.gl + (size_t)w * B.maxL * 4, (size_t)nL * 4));
  HIPCHK(c, debug_fetch_d(Wl, B.Wl + (size_t)w * B.maxL * 4 * WS, (size_t)nL * 4 * WS));
  HIPCHK(c, debug_fetch_i(ps, B.pt_start + (size_t)w * B.maxP, nP));
  HIPCHK(c, debug_fetch_i(ls, B.ln_start + (size_t)w * B.maxL, nL));
  std::fill(H, H + (size_t)n * n, 0.0);
  auto put = [&](int r, int k, double v) { H[(size_t)r * n + k] = v; H[(size_t)k * n + r] = v; };
  for (int r = 0; r < NC; ++r) {
    g[r] = gc[r];
    for (int k = 0; k <= r; ++k) put(r, k, Hcc[tri(r, k)]);
  }
  for (int p = 0; p < nP; ++p) {
    const int k = NC + p;
    g[k] = gp[p];
    H[(size_t)k * n + k] = Hpp[p];
    if (ps[p] < 0 || ps[p] >= NF) return fail(c, VPL_E_INVALID, "debug read-out: start frame of a point track outside the window");
    for (int v = 0; v < NV; ++v) {
      const int cc = wcol(v, ps[p], WS);
      if (cc >= 0) put(vis2cam(v), k, Wp[(size_t)p * WS + cc]);
    }
  }
  for (int l = 0; l < nL; ++l) {
    if (ls[l] < 0 || ls[l] >= NF) return fail(c, VPL_E_INVALID, "debug read-out: start frame of a line track outside the window");
    for (int a = 0; a < 4; ++a) {
      const int k = NC + nP + 4 * l + a;
      g[k] = gl[4 * l + a];
      for (int b = 0; b < 4; ++b) H[(size_t)k * n + NC + nP + 4 * l + b] = Hll[16 * l + 4 * a + b];
      for (int v = 0; v < NV; ++v) {
        const int cc = wcol(v, ls[l], WS);
        if (cc >= 0) put(vis2cam(v), k, Wl[((size_t)l * 4 + a) * WS + cc]);
      }
    }
  }
  const int rs = debug_states(c, w, nP, nL, B.pose, B.sb, B.ex, B.invd, B.orth, x_pose, x_speed_bias, x_ex_pose, x_inv_depth, x_line_orth);
  if (rs) return rs;
  if (x_cost) {
    TrState t;
    HIPCHK(c, hipMemcpy(&t, B.tr + w, sizeof(t), hipMemcpyDeviceToHost));
    *x_cost = t.x_cost;
  }
  return n;
}

// The step the kernels of the last iteration computed for window w: jacobi scale, diagonal_, gradient_ and the Gauss-Newton step
// over the full index ([n] each, n as above), the trust-region state as 14 doubles (radius, mu, alpha, a1, a2, a3,
// model_cost_change, dogleg_step_norm, step_norm, x_norm, iter, status, num_successful, step_valid), the window's path flag
// and the candidate states.  Returns n.
int vpl_ba_debug_step(vpl_ctx* c, int w, double* scale, double* diag, double* grad, double* gn, double* tr14, int* path,
                      double* cand_pose, double* cand_speed_bias, double* cand_ex_pose, double* cand_inv_depth,
                      double* cand_line_orth) {
  const int rc = debug_window_ready(c, w);
  if (rc) return rc;
  const DevBatch& B = c->B;
  const int nP = c->h_nP[w], nL = (int)c->h_lmap[w].size();
  if (nP < 0 || nP > B.maxP || nL > B.maxL) return fail(c, VPL_E_INVALID, "debug read-out: counts outside the context's capacity");
  int rs = debug_full_vector(c, w, nP, nL, B.scale, scale);
  if (!rs) rs = debug_full_vector(c, w, nP, nL, B.diag, diag);
  if (!rs) rs = debug_full_vector(c, w, nP, nL, B.grad, grad);
  if (!rs) rs = debug_full_vector(c, w, nP, nL, B.gn, gn);
  if (rs) return rs;
  if (tr14) {
    TrState t;
    HIPCHK(c, hipMemcpy(&t, B.tr + w, sizeof(t), hipMemcpyDeviceToHost));
    const double v[14] = {t.radius, t.mu, t.alpha, t.a1, t.a2, t.a3, t.model_cost_change, t.dogleg_step_norm, t.step_norm, t.x_norm,
                          (double)t.iter, (double)t.status, (double)t.num_successful, (double)t.step_valid};
    std::memcpy(tr14, v, sizeof(v));
  }
  if (path) HIPCHK(c, hipMemcpy(path, B.path + w, 4, hipMemcpyDeviceToHost));
  rs = debug_states(c, w, nP, nL, B.pose_c, B.sb_c, B.ex_c, B.invd_c, B.orth_c, cand_pose, cand_speed_bias, cand_ex_pose,
                    cand_inv_depth, cand_line_orth);
  return rs ? rs : NC + nP + 4 * nL;
}

// Debug/test access to the pivoted Cholesky factorisations of ba_psd.h on caller-supplied matrices (k_psd_factor): n_cases
// work-groups in one launch.  form 0: psd_pivoted_cholesky_wave<16> (256 threads, n <= 16); 1: _wave<48> (256 or 512, n <= 48);
// 2: _wave4<19, 4> (512, n <= 76: on fewer than eight waves it would wait out its poll limit); 3: the work-group version (256 or
// 512, n <= 80).  Any other pairing: VPL_E_INVALID, nothing is launched.  A, J0: [case][80 * 80] holding n x n row-major; b, r0,
// perm: [case][80].  J0 and r0 are filled with NaN (all bits set) before the launch: what the kernel does not write stays visible.
// rank[case] = -1: wave4 gave up a wait (nothing else written for that case).
int vpl_ba_debug_psd_factor(vpl_ctx* c, int form, int threads, int n_cases, const int* n, const double* A, const double* b,
                            const double* abs_tol, const double* rel_tol, int* rank, int* perm, double* J0, double* r0) {
  if (!c || n_cases < 1 || !n || !A || !b || !abs_tol || !rel_tol || !rank || !perm || !J0 || !r0) return VPL_E_INVALID;
  const int nlim = form == 0 ? 16 : form == 1 ? 48 : form == 2 ? 76 : form == 3 ? MAXKEEP : 0;
  const bool pairing = (form == 0 && threads == 256) || (form == 2 && threads == 512) ||
                       ((form == 1 || form == 3) && (threads == 256 || threads == 512));
  if (!pairing) return fail(c, VPL_E_INVALID, "debug_psd_factor: this form does not run on this many threads");
  int nmax = 0;
  for (int i = 0; i < n_cases; ++i) {
    if (n[i] < 1 || n[i] > nlim) return fail(c, VPL_E_INVALID, "debug_psd_factor: n outside the form's range");
    nmax = std::max(nmax, n[i]);
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t N = (size_t)n_cases, M2 = (size_t)MAXKEEP * MAXKEEP;
  DevBuf dn, dA, db, dat, drt, drank, dperm, dJ, dr;
  HIPCHK(c, dn.alloc(N * 4)); HIPCHK(c, dA.alloc(N * M2 * 8)); HIPCHK(c, db.alloc(N * MAXKEEP * 8));
  HIPCHK(c, dat.alloc(N * 8)); HIPCHK(c, drt.alloc(N * 8)); HIPCHK(c, drank.alloc(N * 4)); HIPCHK(c, dperm.alloc(N * MAXKEEP * 4));
  HIPCHK(c, dJ.alloc(N * M2 * 8)); HIPCHK(c, dr.alloc(N * MAXKEEP * 8));
  HIPCHK(c, hipMemcpyAsync(dn.p, n, N * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dA.p, A, N * M2 * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(db.p, b, N * MAXKEEP * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dat.p, abs_tol, N * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(drt.p, rel_tol, N * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(drank.p, 0xff, N * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(dperm.p, 0xff, N * MAXKEEP * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(dJ.p, 0xff, N * M2 * 8, c->stream));
  HIPCHK(c, hipMemsetAsync(dr.p, 0xff, N * MAXKEEP * 8, c->stream));
  const size_t smem = (size_t)psd_test_lds_doubles(nmax) * sizeof(double);
  const void* kern = threads == 256 ? (const void*)k_psd_factor<256> : (const void*)k_psd_factor<512>;
  HIPCHK(c, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, psd_test_lds_doubles(MAXKEEP) * (int)sizeof(double)));
  if (threads == 256)
    hipLaunchKernelGGL(k_psd_factor<256>, dim3(n_cases), dim3(256), smem, c->stream, form, (const int*)dn.p, dA.d(), db.d(), dat.d(),
                       drt.d(), (int*)drank.p, (int*)dperm.p, dJ.d(), dr.d());
  else
    hipLaunchKernelGGL(k_psd_factor<512>, dim3(n_cases), dim3(512), smem, c->stream, form, (const int*)dn.p, dA.d(), db.d(), dat.d(),
                       drt.d(), (int*)drank.p, (int*)dperm.p, dJ.d(), dr.d());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(rank, drank.p, N * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(perm, dperm.p, N * MAXKEEP * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(J0, dJ.p, N * M2 * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(r0, dr.p, N * MAXKEEP * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VPL_OK;
}

// Debug aid of the randomised sweeps (tools/fuzz_*.py with VPL_DEBUG_GUARDS=1 in the environment when the context is made): the
// 64 bytes behind every device array then hold 0xA5; returns how many arrays have had theirs written to (a kernel ran past the
// end of an array), the first one named in vpl_last_error by its allocation index and size.
int vpl_ba_debug_guards(vpl_ctx* c) { return debug_guards(c); }
// Test access (not in the header): the arrays in the context's allocation record and their payload bytes
int vpl_ba_debug_allocs(vpl_ctx* c, long long* n_arrays, long long* payload_bytes) { return debug_allocs(c, n_arrays, payload_bytes); }

int vpl_ba_debug_stamps(vpl_ctx* c, int w, long long* out) {
  HIPCHK(c, hipMemcpy(out, c->B.dbg + (size_t)w * 64, 64 * 8, hipMemcpyDeviceToHost));
  return VPL_OK;
}

// Host-only (no device call): the point work-unit tables upload builds for one window, and a replay of their commit chains.
int vpl_ba_debug_point_units(int n_points, const int* point_start, const int* point_nobs, int max_rounds, int* lane_table,
                             int* unit_table, int* rounds, int* rounds0) {
  if (n_points < 0 || !point_start || !point_nobs || !lane_table || !unit_table || !rounds || !rounds0 || max_rounds < 1) return VPL_E_INVALID;
  std::vector<int> off(n_points + 1, 0), list(n_points + 1, 0);
  int cnt[NF + 1];
  int o = 0;
  for (int p = 0; p < n_points; ++p) {
    if (point_start[p] < 0 || point_nobs[p] < 2 || point_start[p] + point_nobs[p] > NF) return VPL_E_INVALID;
    off[p] = o; o += point_nobs[p];
  }
  sort_points_by_start(n_points, point_start, point_nobs, list.data(), cnt);
  PointUnitLayout PL;
  if (!pack_point_units(point_nobs, off.data(), list.data(), cnt, max_rounds, lane_table, unit_table, &PL)) return VPL_E_CAPACITY;
  *rounds = PL.rounds; *rounds0 = PL.rounds0;
  return VPL_OK;
}
int vpl_ba_debug_point_chains(const int* unit_table, int rounds, int rounds0, int marg_pass) {
  if (!unit_table || rounds < 0 || rounds0 < 0 || rounds0 > rounds) return VPL_E_INVALID;
  PointUnitLayout PL;
  PL.rounds = rounds; PL.rounds0 = rounds0;
  return point_unit_chains_finish(unit_table, PL, marg_pass != 0) ? 1 : 0;
}

int vpl_ba_enable_kernel_timing(vpl_ctx* c, int enable) {
  if (!c) return VPL_E_INVALID;
  c->timing = enable != 0;
  c->ktimes.clear();
  return VPL_OK;
}
int vpl_ba_kernel_times(vpl_ctx* c, int* count, const char** names, double* total_ms, int* launches) {
  if (!c || !count) return VPL_E_INVALID;
  int cap = *count, i = 0;
  c->kname_store.clear();
  for (auto& kv : c->ktimes) c->kname_store.push_back(kv.first);
  for (auto& kv : c->ktimes) {
    if (i >= cap) break;
    names[i] = c->kname_store[i].c_str();
    total_ms[i] = kv.second.first;
    launches[i] = kv.second.second;
    ++i;
  }
  *count = i;
  return VPL_OK;
}

// Per-launch profile of the LAST solve run with kernel timing enabled: kernel name, device time and the number of windows
// that did work in the launch (k_lin: linearised; k_solve: [1] computed a new Gauss-Newton step, [2] re-used the step of a
// rejected iteration; k_cost: evaluated a candidate).  active is [count][4] in the order k_lin, k_solve new, k_solve
// re-used, k_cost.
int vpl_ba_launch_profile(vpl_ctx* c, int* count, const char** names, double* ms, int* active) {
  if (!c || !count || !names || !ms || !active) return VPL_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<int> act((size_t)ACT_SLOTS * 4);
  HIPCHK(c, hipMemcpy(act.data(), c->d_act, act.size() * sizeof(int), hipMemcpyDeviceToHost));
  const int n = std::min(*count, (int)c->ltimes.size());
  for (int i = 0; i < n; ++i) {
    names[i] = c->ltimes[i].first;
    ms[i] = c->ltimes[i].second;
    for (int k = 0; k < 4; ++k) active[4 * i + k] = i < ACT_SLOTS ? act[4 * i + k] : 0;
  }
  *count = n;
  return VPL_OK;
}

}  // extern "C"

#include "ba_session.h"   // the keyframe session: drives launch_triangulate, launch_line_opt, vpl_ba_solve and the upload
