// C ABI of the MI355X-native bundle-adjustment path (include/vplines_ba.h).
// Host side: packs caller-owned windows into the device SoA of ba_types.h, enqueues the
// kernel sequence of one batched solve on the context's stream, unpacks results.
// There is no CPU compute path in this library: every entry point that computes launches
// HIP kernels and reports VPL_E_NODEVICE / VPL_E_HIP when that is impossible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
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

// ---- staging ------------------------------------------------------------------------------------------------------------
// Host <-> device traffic of the window entry points goes through ONE pinned host arena and ONE device arena per context:
//   upload   : the host packs every array into the pinned arena, ONE hipMemcpyAsync moves it to the device arena, ONE kernel
//              (k_copy_segments) scatters the pieces into the batch's arrays;
//   download : one kernel gathers the result arrays into the device arena, ONE hipMemcpyAsync brings it to the pinned arena,
//              the host scatters into the caller's structs.
// Round 3 issued ~45 hipMemcpyAsync per upload and ~17 per download straight from / into pageable std::vectors and the
// caller's vpl_prior structs: each pageable copy above the runtime's staging threshold pins and unpins its pages (a kernel
// driver call that can quiesce the process's queues), which showed up as 26 ms instead of 1.4 in the solve leg of a
// 64-window call on the round-3 driver box.  The library now hands pageable memory to the runtime nowhere
// on the upload / solve / download path.
struct CopySeg {
  const char* src;
  char* dst;
  unsigned bytes;
  unsigned u0;   // index of the segment's first 16-byte unit in the launch
};
static_assert(sizeof(CopySeg) == 24, "CopySeg layout");

// one thread per 16-byte unit; the segment of a unit by binary search over the (<= few thousand) prefix entries
__global__ __launch_bounds__(256) void k_copy_segments(const CopySeg* tab, int nseg, unsigned total_units) {
  for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < total_units; u += gridDim.x * 256u) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tab[mid].u0 <= u) lo = mid; else hi = mid - 1;
    }
    const CopySeg sg = tab[lo];
    const unsigned off = (u - sg.u0) * 16u;
    const unsigned rem = sg.bytes - off;
    const char* src = sg.src + off;
    char* dst = sg.dst + off;
    if (rem >= 16u && (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {
      *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    } else {   // tails and 4- / 8-byte aligned pieces (every array is made of 4- or 8-byte elements)
      const unsigned nb = rem < 16u ? rem : 16u;
      for (unsigned b = 0; b < nb; b += 4) *reinterpret_cast<uint32_t*>(dst + b) = *reinterpret_cast<const uint32_t*>(src + b);
    }
  }
}

template <typename T>
struct Span {   // a piece of the pinned arena with the few std::vector members the packing code uses
  T* p = nullptr;
  size_t n = 0;
  T& operator[](size_t i) const { return p[i]; }
  T* data() const { return p; }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  T* begin() const { return p; }
  T* end() const { return p + n; }
};

// The arena's bound is never written down: a call runs its takes and segments once on a DRY stage, which only counts them,
// and reserves what that run used (stage_plan; the upload: upload_bound).  A take past the bound hands out host scratch and
// flags `overflow`, which stage_run refuses, so a wrong bound is an error and never a write past the arena.
struct Stage {
  char* h = nullptr;   // hipHostMalloc
  char* d = nullptr;   // hipMalloc
  size_t cap = 0, used = 0;
  std::vector<CopySeg> segs;
  unsigned units = 0;
  bool overflow = false;
  bool dry = false;                                  // sizing run: takes are empty pieces, nothing is allocated or written
  std::vector<std::unique_ptr<char[]>> spill;        // pieces taken past the bound

  hipError_t reserve(size_t need) {
    used = 0; segs.clear(); units = 0; overflow = false; spill.clear();
    if (need <= cap) return hipSuccess;
    release();
    const size_t want = need + need / 4 + (1u << 16);
    hipError_t e = hipHostMalloc((void**)&h, want, hipHostMallocDefault);
    if (e != hipSuccess) return e;
    e = hipMalloc((void**)&d, want);
    if (e != hipSuccess) return e;
    cap = want;
    return hipSuccess;
  }
  void release() {
    if (h) (void)hipHostFree(h);   // (the old arena is dropped either way)
    if (d) (void)hipFree(d);
    h = d = nullptr; cap = 0;
  }
  // what a reserve must cover for the takes and segments so far: the data, and the segment table stage_run appends
  size_t bound() const { return ((used + 63) & ~(size_t)63) + segs.size() * sizeof(CopySeg); }
  template <typename T>
  Span<T> take(size_t n) {   // uninitialised
    used = (used + 63) & ~(size_t)63;
    Span<T> sp;
    sp.n = n;
    if (!dry && used + n * sizeof(T) <= cap) sp.p = reinterpret_cast<T*>(h + used);
    else if (!dry) { overflow = true; spill.emplace_back(new char[n * sizeof(T) + 1]); sp.p = reinterpret_cast<T*>(spill.back().get()); }
    used += n * sizeof(T);
    return sp;
  }
  template <typename T>
  Span<T> take(size_t n, T fill) {
    Span<T> sp = take<T>(n);
    if (!dry) std::fill(sp.begin(), sp.end(), fill);
    return sp;
  }
  char* dev_of(const void* host_ptr) const { return d + (reinterpret_cast<const char*>(host_ptr) - h); }
  void seg(const void* src, void* dst, size_t bytes) {
    if (!bytes) return;
    CopySeg c{reinterpret_cast<const char*>(src), reinterpret_cast<char*>(dst), (unsigned)bytes, units};
    units += (unsigned)((bytes + 15) / 16);
    segs.push_back(c);
  }
  // upload: a piece of the arena (host address) to a device array
  template <typename T>
  void to_device(T* dev_dst, const T* host_src, size_t n) { seg(dev_of(host_src), dev_dst, n * sizeof(T)); }
  // download: a device array to a piece of the arena (host address)
  template <typename T>
  void from_device(T* host_dst, const T* dev_src, size_t n) { seg(dev_src, dev_of(host_dst), n * sizeof(T)); }
  template <typename T>
  void put(T* dev_dst, const Span<T>& src) { to_device(dev_dst, src.p, src.n); }
};

// sizes the arena by a dry run of `plan` (its takes and segments), reserves that, and runs `plan` on the arena
template <typename Plan>
static hipError_t stage_plan(Stage& S, const Plan& plan) {
  Stage dry;
  dry.dry = true;
  plan(dry);
  const hipError_t e = S.reserve(dry.bound());
  if (e == hipSuccess) plan(S);
  return e;
}

struct vpl_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int maxW = 0, maxP = 0, maxPO = 0, maxL = 0, maxLO = 0;
  DevBatch B;
  std::vector<void*> allocs;
  std::vector<size_t> alloc_bytes;   // payload of allocs[i]; 64 pad bytes follow (VPL_DEBUG_GUARDS=1: filled with 0xA5, vpl_ba_debug_guards)
  bool guards = false;
  int nW = 0;
  vpl_ba_options opt;
  std::string err;
  bool timing = false;
  std::map<std::string, std::pair<double, int>> ktimes;
  std::vector<std::pair<const char*, double>> ltimes;   // (kernel, ms) of every launch of the last timed solve, in order
  int* d_act = nullptr;                                 // [ACT_SLOTS][4] activity counters of those launches
  // the ~19 launches of one solve as a hipGraph, captured on the first vpl_ba_solve after an upload (the kernel arguments --
  // the batch descriptor by value -- are fixed until the next upload); VPL_BA_GRAPH=0 launches kernel by kernel
  hipGraphExec_t graph_exec = nullptr;
  bool use_graph = true;
  // signature of the track layout (start frames, lengths, selected lines) of the last upload: when the next batch has the same
  // one -- the usual case between two solves of a tracker that lost and gained nothing, and every repetition of a benchmark --
  // the host-built lane / unit / K-step tables and the index arrays already on the device are the right ones and are neither
  // rebuilt nor uploaded again
  unsigned long long layout_sig = 0;
  std::vector<int> layout_key;                   // the integers the signature was made of (exact comparison on a hash match)
  bool layout_valid = false;
  bool force_general = false;                    // VPL_BA_GENERAL=1: every window takes k_solve (A/B runs, tests of the general path)
  bool schur_mostly_wide = false;                // more than 35 % of the landmark elimination's weight sits in wide entries: k_schur<5>
  bool schur_never_wide = false;                 // VPL_BA_SCHUR_WIDE=-1: k_schur_mixed whatever the share of wide entries (A/B runs)
  bool schur_wide_all = false;                   // VPL_BA_SCHUR_WIDE=1: round 3's k_schur<5> for batches with long tracks (A/B runs, tests)
  std::vector<std::string> kname_store;
  // host-side marg structure of the uploaded windows
  std::vector<int> h_mg_m;
  std::vector<int> h_passthrough;              // MARGIN_SECOND_NEW: window keeps its input prior (index into h_pass_priors or -1)
  std::vector<vpl_prior> h_pass_priors;
  bool any_second_new = false;
  std::vector<int> h_nP, h_nL;
  std::vector<std::vector<int>> h_lmap;          // per window: device line index -> index in the vpl_window arrays
  size_t marg_smem = 0;
  int marg_nmax = 0;                             // largest kept block of the uploaded batch (k_prior_eigen's LDS layout)
  int prior_rule = VPL_PRIOR_PIVOTED_CHOLESKY;   // vpl_ba_set_prior_rule
  bool marg_small = false;                       // k_marg<256> (two work-groups per CU) instead of k_marg<512>
  int maxPriorN = 0;                             // largest prior of the uploaded batch (k_prep stages J0 in LDS)
  // asynchronous variants of the line-map entry points: the host-side completion (wait for the stream, scatter the staged
  // results into the caller's arrays) of the call that was enqueued last; run by vpl_ba_collect or by the next call that
  // touches the batch
  std::function<int()> pending;
  bool upload_open = false;                      // an upload has started to rewrite the host tables of the batch and has not finished
  bool prior_resident = false;                   // the last solve / marginalisation of the uploaded batch left its priors in mg_* (vpl_ba_upload_chained)
  int prior_resident_nW = 0;
  double odo_ms[3] = {0, 0, 0};                  // vpl_ba_debug_odometry_ms
  Stage stage;                                   // pinned + device staging arenas of upload / download
  std::vector<int> h_mg_n;                       // kept dims of the next prior as the host computed them (>= the device's)
  // device time of the last upload / solve / download (hipEvents on the context's stream), vpl_ctx_enable_leg_timing
  bool leg_timing = false;
  hipEvent_t leg_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<int> h_mg_nb;                      // kept blocks of the next prior as the host laid them out
  size_t last_upload_bytes = 0;                  // what the last upload's one host-to-device copy moved
  struct vpl_odo* odo = nullptr;                 // the keyframe session that borrows this context (one per context)
};

// appends the segment table to the arena, moves arena (upload: data + table, download: table only) and runs the copy kernel
static hipError_t stage_run(vpl_ctx* c, bool upload) {
  Stage& S = c->stage;
  if (S.overflow) return hipErrorOutOfMemory;
  if (S.segs.empty()) return hipSuccess;
  const size_t data_end = S.used;
  Span<CopySeg> tab = S.take<CopySeg>(S.segs.size());
  if (S.overflow) return hipErrorOutOfMemory;
  std::memcpy(tab.p, S.segs.data(), S.segs.size() * sizeof(CopySeg));
  const size_t tab_off = reinterpret_cast<char*>(tab.p) - S.h;
  hipError_t e;
  if (upload) c->last_upload_bytes = S.used;
  if (upload) e = hipMemcpyAsync(S.d, S.h, S.used, hipMemcpyHostToDevice, c->stream);
  else e = hipMemcpyAsync(S.d + tab_off, S.h + tab_off, S.segs.size() * sizeof(CopySeg), hipMemcpyHostToDevice, c->stream);
  if (e != hipSuccess) return e;
  const unsigned blocks = std::min<unsigned>((S.units + 255) / 256, 2048u);
  hipLaunchKernelGGL(k_copy_segments, dim3(blocks), dim3(256), 0, c->stream, reinterpret_cast<const CopySeg*>(S.d + tab_off),
                     (int)S.segs.size(), S.units);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (!upload) e = hipMemcpyAsync(S.h, S.d, data_end, hipMemcpyDeviceToHost, c->stream);
  return e;
}

static void drop_graph(vpl_ctx* c) {
  if (c->graph_exec) { (void)hipGraphExecDestroy(c->graph_exec); c->graph_exec = nullptr; }
}

// completes the asynchronous call that is still pending on this context, if any
static int settle(vpl_ctx* c) {
  if (!c || !c->pending) return VPL_OK;
  std::function<int()> fin;
  fin.swap(c->pending);
  return fin();
}
// the tail of an entry point: now, or (asynchronous variant) when the caller collects
static int finish_or_defer(vpl_ctx* c, bool async, std::function<int()> fin) {
  if (!async) return fin();
  c->pending = std::move(fin);
  return VPL_OK;
}

// ---- helpers -----------------------------------------------------------------------------------
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

struct KTimer {
  vpl_ctx* c;
  const char* name;
  hipEvent_t a = nullptr, b = nullptr;
  KTimer(vpl_ctx* c_, const char* n) : c(c_), name(n) {
    // (a timing aid: a failed event call leaves a time of 0 and nothing else)
    if (c->timing) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); (void)hipEventRecord(a, c->stream); }
  }
  ~KTimer() {
    if (c->timing) {
      (void)hipEventRecord(b, c->stream);
      (void)hipEventSynchronize(b);
      float ms = 0;
      (void)hipEventElapsedTime(&ms, a, b);
      auto& e = c->ktimes[name];
      e.first += ms;
      e.second += 1;
      c->ltimes.emplace_back(name, (double)ms);
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
    }
  }
};

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
  double* d() { return (double*)p; }
};

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
  // k_solve keeps 2 doubles per point and 18 per line in the LDS space behind its two staging buffers
  if (2 * c->maxP + 18 * c->maxL > NAP - 2 * CROWS * CW) return VPL_E_CAPACITY;
  // ... and 4 doubles per point and 28 per line in the staging buffers' space between the scaling and the first chunk
  if (4 * c->maxP + 28 * c->maxL > 2 * CROWS * CW) return VPL_E_CAPACITY;
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
  {   // static table of the assembly pass of k_lin
    std::vector<int> tab(2 * NCP);
    for (int r = 0, e2 = 0; r < NC; ++r)
      for (int cc = 0; cc <= r; ++cc, ++e2) lin_asm_entry(r, cc, &tab[2 * e2]);
    if (hipMemcpy(B.asm_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return VPL_E_HIP;
  }
  {   // non-zero pattern of the packed cam Hessian of a fast-path window (ba_types.h)
    std::vector<int> nz;
    for (int r = 0; r < NC; ++r)
      for (int cc = 0; cc <= r; ++cc) {
        const bool vis = cam2vis(r) >= 0 && cam2vis(cc) >= 0;
        const int fr = r < 165 ? r / 15 : -1, fc = cc < 165 ? cc / 15 : -1;
        const bool band = fr >= 0 && fc >= 0 && (fr == fc || fr == fc + 1);
        const bool sb0 = cc >= 6 && cc < 15 && cam2vis(r) >= 0;
        if (vis || band || sb0) nz.push_back(tri(r, cc) | r << 14 | cc << 22);
      }
    if ((int)nz.size() != NZ_N || hipMemcpy(B.nz_tab, nz.data(), nz.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return VPL_E_HIP;
  }
  // the attribute is per kernel, not per context: never lower what a larger context of this process has asked for
  static size_t lin_max = 0, solve_max = 0, schur_max = 0, back_max = 0;
  lin_max = std::max(lin_max, lin_smem(c->maxP, c->maxL));
  solve_max = std::max(solve_max, solve_smem(c->maxP, c->maxL));
  schur_max = std::max(schur_max, schur_smem(c->maxP, c->maxL));
  back_max = std::max(back_max, back_smem(c->maxP, c->maxL));
  if (schur_max > 159 * 1024 || back_max > 159 * 1024) return VPL_E_CAPACITY;
  const std::pair<const void*, size_t> lds[] = {
      {(const void*)k_lin2, lin_max}, {(const void*)k_lin<1>, lin_max}, {(const void*)k_lin<2>, lin_max},
      {(const void*)k_solve, solve_max}, {(const void*)k_schur<3>, schur_max}, {(const void*)k_schur<5>, schur_max},
      {(const void*)k_schur_mixed, schur_max}, {(const void*)k_chol, CHOL_SMEM}, {(const void*)k_back, back_max},
      {(const void*)k_prep, PREP_SMEM}, {(const void*)k_marg<MARG_THREADS>, 159 * 1024}, {(const void*)k_marg<256>, MARG_LDS_SMALL},
      {(const void*)k_prior_eigen, prior_eig_layout(MAXKEEP).bytes}};
  for (const auto& k : lds)
    if (hipFuncSetAttribute(k.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.second) != hipSuccess) return VPL_E_HIP;
  vpl_ba_default_options(&c->opt);
  if (const char* gv = std::getenv("VPL_BA_GRAPH")) c->use_graph = std::atoi(gv) != 0;
  if (const char* gv = std::getenv("VPL_BA_GENERAL")) c->force_general = std::atoi(gv) != 0;
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
  const int rs = settle(c);
  if (rs) return rs;
  if (c->stream != (hipStream_t)s) {
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipStreamSynchronize(c->stream);   // (an old stream the caller has destroyed already has nothing in flight)
    (void)hipGetLastError();
  }
  drop_graph(c);
  c->stream = (hipStream_t)s;
  return VPL_OK;
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
  { KTimer t(c, "k_preintegrate");
    hipLaunchKernelGGL(k_preintegrate, dim3((n + 3) / 4), dim3(64), 0, c->stream, n, (const int*)d_off.p, (const int*)d_ns.p, d_s.d(),
                       d_a.d(), d_g.d(), d_ba.d(), d_bg.d(), opt->acc_n * opt->acc_n, opt->gyr_n * opt->gyr_n,
                       opt->acc_w * opt->acc_w, opt->gyr_w * opt->gyr_w, (DevPreint*)d_out.p); }
  HIPCHK(c, hipGetLastError());
  std::vector<DevPreint> h(n);
  HIPCHK(c, hipMemcpyAsync(h.data(), d_out.p, n * sizeof(DevPreint), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; ++i) {
    vpl_preintegration& o = out[i];
    o.sum_dt = h[i].sum_dt;
    for (int k = 0; k < 3; ++k) { o.delta_p[k] = h[i].dp[k]; o.delta_v[k] = h[i].dv[k]; o.linearized_ba[k] = h[i].lba[k]; o.linearized_bg[k] = h[i].lbg[k]; }
    for (int k = 0; k < 4; ++k) o.delta_q[k] = h[i].dq[k];
    std::memcpy(o.jacobian, h[i].sqrt_info, sizeof(o.jacobian));   // k_preintegrate carries J out in this slot
    std::memcpy(o.covariance, h[i].cov, sizeof(o.covariance));
  }
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

// ---- window batch: upload / solve / download ------------------------------------------------------------
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

// An upload on behalf of a keyframe session (vpl_odo_*): the windows carry the INTEGER side only (track starts and lengths,
// triangulation flags, preint[1].sum_dt); every double of the batch -- states, observations, inverse depths, lines,
// pre-integrations, the prior's values -- is on the device already and is gathered from the session's store behind the upload's
// scatter (k_odo_gather, k_odo_prior_load).  Window w is sequence w.
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

static void take_upload(Stage& S, UploadArena& A, const DevBatch& B, size_t W, const vpl_window* win, bool chained, bool odo) {
  if (!odo) {
    A.pose = S.take<double>(W * 77); A.sb = S.take<double>(W * 99); A.ex = S.take<double>(W * 7); A.invd = S.take<double>(W * B.maxP, 1.0);
    A.plk = S.take<double>(W * B.maxL * 6, 0.0);
  } else {
    A.odo_psrc = S.take<int>(W * B.maxP, 0); A.odo_lsrc = S.take<int>(W * B.maxL, 0); A.odo_has = S.take<int>(W, 0); A.odo_marg = S.take<int>(W, 0);
  }
  A.nP = S.take<int>(W); A.nL = S.take<int>(W);
  A.pt_start = S.take<int>(W * B.maxP, 0); A.pt_nobs = S.take<int>(W * B.maxP, 0); A.pt_off = S.take<int>(W * B.maxP, 0);
  A.ln_start = S.take<int>(W * B.maxL, 0); A.ln_nobs = S.take<int>(W * B.maxL, 0); A.ln_off = S.take<int>(W * B.maxL, 0);
  A.ln_tri = S.take<int>(W * B.maxL, 1);
  A.pu_cnt = S.take<int>(W, 0); A.pu_cnt0 = S.take<int>(W, 0);
  A.sk_tab = S.take<int>(W * B.maxKS * 4, 0); A.sk_wave = S.take<int>(W * 8 * SK_WSTRIDE, -1); A.path = S.take<int>(W, 0);
  A.nLO = S.take<int>(W, 0); A.lo_ln = S.take<int>(W * B.maxLO, 0); A.ll_tab = S.take<int>(W * B.llSlots * 2, -1); A.ll_np = S.take<int>(W, 0);
  A.ps_list = S.take<int>(W * B.maxP, 0); A.ps_cnt = S.take<int>(W * (NF + 1), 0);
  if (!odo) {
    A.pt_obs = S.take<double>(W * B.maxPO * 3, 0.0); A.ln_obs = S.take<double>(W * B.maxLO * 8, 0.0);
    A.pre = S.take<DevPreint>(W * NF);
    A.fail_ref = S.take<double>(W * 13, 0.0); A.orth = S.take<double>(W * B.maxL * 4, 0.0);
  }
  A.orth_in = S.take<int>(W, 0);
  A.pr_n = S.take<int>(W, 0); A.pr_nb = S.take<int>(W, 0);
  A.pr_kind = S.take<int>(W * MAXPB, 0); A.pr_frame = S.take<int>(W * MAXPB, 0); A.pr_idx = S.take<int>(W * MAXPB, 0);
  if (!odo) { A.pr_x0 = S.take<double>(W * MAXPB * 9, 0.0); A.pr_r0 = S.take<double>(W * MAXPN, 0.0); }
  A.mg_n = S.take<int>(W, 0); A.mg_nb = S.take<int>(W, 0); A.mg_kind = S.take<int>(W * MAXPB, 0); A.mg_frame = S.take<int>(W * MAXPB, 0);
  A.mg_idx = S.take<int>(W * MAXPB, 0); A.mg_cam = S.take<int>(W * MAXPB, 0);
  A.mg_m = S.take<int>(W);
  A.J0.assign(W, Span<double>());
  for (size_t w = 0; w < W; ++w)
    if (!chained && win[w].has_prior && win[w].prior && win[w].prior->n > 0) A.J0[w] = S.take<double>((size_t)win[w].prior->n * win[w].prior->n);
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
  take_upload(dry, A, B, W, win, chained, odo != nullptr);
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
  { const int rs = settle(c); if (rs) return rs; }   // an asynchronous call whose results have not been collected yet
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
  HIPCHK(c, stage_run(c, false));
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
  int maxLineTrack = 1;
  for (size_t w = 0; w < W; ++w)
    for (int l = 0; l < win[w].n_lines; ++l) maxLineTrack = std::max(maxLineTrack, std::min(win[w].line_nobs[l], (int)NF));
  B.llK = maxLineTrack;
  B.llNLW = 64 / maxLineTrack;
  B.wfill = (minTrack != maxTrack || opt->remove_line_outliers) ? 1 : 0;
  return VPL_OK;
}

// 4. signature of the track layout: when it is the last upload's, the lane / unit / K-step tables and the index arrays on the
// device are the right ones.  The hash only finds the candidate; the decision is an exact comparison of the hashed integers
// (a collision would reuse lane / unit / K-step tables of another track layout: out-of-range reads -- ADVICE r3).
static bool layout_unchanged(vpl_ctx* c, size_t W, const vpl_window* win, bool all_lines) {
  const DevBatch& B = c->B;
  unsigned long long h = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } };
  const int hdr[8] = {(int)W, B.WS, B.llK, B.llNLW, B.wfill, all_lines ? 1 : 0, B.maxP, B.maxL};
  mix(hdr, sizeof(hdr));
  std::vector<int> key;
  key.reserve(16 + W * 8);
  key.insert(key.end(), hdr, hdr + 8);
  for (size_t w = 0; w < W; ++w) {
    const vpl_window& v = win[w];
    mix(&v.n_points, 4); mix(&v.n_lines, 4);
    key.push_back(v.n_points); key.push_back(v.n_lines);
    const bool hp = v.n_points > 0 && v.point_start && v.point_nobs, hl = v.n_lines > 0 && v.line_start && v.line_nobs;
    const bool ht = v.n_lines > 0 && v.line_triangulated;
    key.push_back((hp ? 1 : 0) | (hl ? 2 : 0) | (ht ? 4 : 0));   // which arrays follow
    if (hp) {
      mix(v.point_start, 4 * (size_t)v.n_points); mix(v.point_nobs, 4 * (size_t)v.n_points);
      key.insert(key.end(), v.point_start, v.point_start + v.n_points); key.insert(key.end(), v.point_nobs, v.point_nobs + v.n_points);
    }
    if (hl) {
      mix(v.line_start, 4 * (size_t)v.n_lines); mix(v.line_nobs, 4 * (size_t)v.n_lines);
      key.insert(key.end(), v.line_start, v.line_start + v.n_lines); key.insert(key.end(), v.line_nobs, v.line_nobs + v.n_lines);
    }
    if (ht) {
      mix(v.line_triangulated, 4 * (size_t)v.n_lines);
      key.insert(key.end(), v.line_triangulated, v.line_triangulated + v.n_lines);
    }
  }
  const bool same = c->layout_valid && h == c->layout_sig && key == c->layout_key && std::getenv("VPL_BA_NO_LAYOUT_CACHE") == nullptr;
  c->layout_sig = h;
  c->layout_key.swap(key);
  c->layout_valid = false;       // becomes valid when this upload has gone through
  return same;
}

// 5. states, tracks and observations of window w; h_lmap[w][dl] is the caller's index of device line dl
static int pack_window(vpl_ctx* c, UploadArena& A, size_t w, const vpl_window& v, bool all_lines, const OdoSrc* odo) {
  const DevBatch& B = c->B;
  if (v.n_points > B.maxP || v.n_lines > B.maxL) return fail(c, VPL_E_CAPACITY, "too many tracks for the context");
  if (!odo) {
    std::memcpy(&A.pose[w * 77], v.pose, 77 * 8);
    std::memcpy(&A.sb[w * 99], v.speed_bias, 99 * 8);
    std::memcpy(&A.ex[w * 7], v.ex_pose, 7 * 8);
  }
  if (!odo && v.failure_occur) {
    A.fail_ref[w * 13] = 1.0;
    std::memcpy(&A.fail_ref[w * 13 + 1], v.last_P0, 3 * 8);
    std::memcpy(&A.fail_ref[w * 13 + 4], v.last_R0, 9 * 8);
  }
  A.nP[w] = v.n_points;
  c->h_nP[w] = v.n_points;
  int off = 0;
  for (int p = 0; p < v.n_points; ++p) {
    const int s = v.point_start[p], no = v.point_nobs[p];
    if (s < 0 || no < 2 || s + no > NF) return fail(c, VPL_E_INVALID, "point track outside the window");
    if (off + no > B.maxPO) return fail(c, VPL_E_CAPACITY, "too many point observations");
    A.pt_start[w * B.maxP + p] = s; A.pt_nobs[w * B.maxP + p] = no; A.pt_off[w * B.maxP + p] = off;
    if (!odo) {
      std::memcpy(&A.pt_obs[(w * B.maxPO + off) * 3], v.point_obs + (size_t)off * 3, (size_t)no * 3 * 8);
      A.invd[w * B.maxP + p] = v.inv_depth[p];
    } else {
      A.odo_psrc[w * B.maxP + p] = odo->psrc[w][p];
    }
    off += no;
  }
  off = 0;
  int woff = 0, nl = 0;
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
      if (odo) A.odo_lsrc[dl] = odo->lsrc[w][l];
      else {
        std::memcpy(&A.ln_obs[(w * B.maxLO + off) * 8], v.line_obs + (size_t)woff * 8, (size_t)no * 8 * 8);
        if (v.line_orth) std::memcpy(&A.orth[dl * 4], v.line_orth + (size_t)l * 4, 4 * 8);
        else std::memcpy(&A.plk[dl * 6], v.line_plk + (size_t)l * 6, 6 * 8);
      }
      for (int k = 0; k < no; ++k) A.lo_ln[w * B.maxLO + off + k] = nl;
      off += no;
      lmap.push_back(l);
      ++nl;
    }
    woff += no;
  }
  A.nL[w] = nl;
  A.orth_in[w] = (!odo && v.line_orth) ? 1 : 0;
  c->h_nL[w] = nl;
  A.nLO[w] = off;
  if (odo) A.odo_has[w] = (odo->tab && odo->has[w]) ? 1 : 0;
  else
    for (int j = 0; j < NF; ++j) to_dev_preint(v.preint[j], A.pre[w * NF + j]);
  return VPL_OK;
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
  // lane layout of the line phase: llNLW whole tracks per wave, k-major; tracks in the caller's order (tracks that start in the
  // same frame side by side would pile their LDS adds onto the same addresses)
  const int NLW = B.llNLW, perPass = 8 * NLW;
  A.ll_np[w] = (nl + perPass - 1) / perPass;
  if (A.ll_np[w] * 512 > B.llSlots) return fail(c, VPL_E_CAPACITY, "line layout table too small");
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
// threads, two work-groups per CU
static int choose_marg(vpl_ctx* c, const Span<int>& mg_n, size_t W) {
  const DevBatch& B = c->B;
  int nmax = 0;
  for (size_t w = 0; w < W; ++w) nmax = std::max(nmax, mg_n[w]);
  c->marg_nmax = nmax;
  c->marg_small = nmax <= 48 && B.maxP <= 256 && B.maxL <= 256 &&
                  (size_t)marg_layout(nmax, true).total * sizeof(double) <= MARG_LDS_SMALL && std::getenv("VPL_BA_MARG_BIG") == nullptr;
  c->marg_smem = (size_t)marg_layout(nmax, c->marg_small).total * sizeof(double);
  if (c->marg_smem > 159 * 1024) return fail(c, VPL_E_CAPACITY, "marginalisation workspace exceeds LDS");
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
  take_upload(SG, A, B, W, win, dev_prior, odo != nullptr);
  // (plain heap, no value-initialisation: only the rounds a window uses are filled and packed into the arena)
  std::unique_ptr<int[]> lane(new int[W * B.maxPR * 1024]), sub(new int[W * B.maxPR * 512]);
  long schur_wide_w = 0, schur_total_w = 0;   // matrix-core weight of the wide entries / of all entries of k_schur's table
  for (size_t w = 0; w < W; ++w) {
    const HostTab* T = dev_prior ? &ctab[w] : nullptr;
    if ((rc = pack_window(c, A, w, win[w], all_lines, odo))) return rc;
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
  if (SG.overflow) return fail(c, VPL_E_CAPACITY, "internal: staging arena bound too small");
  stage_upload(SG, A, B, W, same_layout, dev_prior, odo);
  if (chained && (rc = hand_over_priors(c, ctab, prev_prS))) return rc;
  // ONE host-to-device copy of the arena, ONE kernel that scatters its pieces into the batch's arrays
  HIPCHK(c, stage_run(c, true));
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

// the states of the uploaded batch back to what the upload put there (pose, sb, ex, invd and, with `plk`, the lines)
static int restore_states(vpl_ctx* c, bool plk) {
  const DevBatch& B = c->B;
  const size_t W = c->nW;
  HIPCHK(c, hipMemcpyAsync(B.pose, B.pose_0, W * 77 * 8, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(B.sb, B.sb_0, W * 99 * 8, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(B.ex, B.ex_0, W * 7 * 8, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(B.invd, B.invd_0, W * B.maxP * 8, hipMemcpyDeviceToDevice, c->stream));
  if (plk) HIPCHK(c, hipMemcpyAsync(B.plk, B.plk_0, W * B.maxL * 6 * 8, hipMemcpyDeviceToDevice, c->stream));
  return VPL_OK;
}

int vpl_ba_reset_state(vpl_ctx* c) {
  if (c) { const int rs = settle(c); if (rs) return rs; }
  if (!c || c->nW < 1) return VPL_E_INVALID;
  return restore_states(c, true);
}

int vpl_ba_upload(vpl_ctx* c, int nW, const vpl_window* win, const vpl_ba_options* opt) {
  return upload_impl(c, nW, win, opt, false);
}
int vpl_ba_upload_chained(vpl_ctx* c, int nW, const vpl_window* win, const vpl_ba_options* opt) {
  return upload_impl(c, nW, win, opt, false, true);
}

// k_prep: whitening matrices, q <- Quaterniond(R(q)), the world orth of the lines and J0^T J0 of the incoming prior
static void launch_prep(vpl_ctx* c, const DevBatch& B, int nw, hipStream_t s) {
  KTimer t(c, "k_prep");
  hipLaunchKernelGGL(k_prep, dim3(nw), dim3(PREP_THREADS), prep_smem(c->maxPriorN), s, B, std::min(c->maxPriorN, PREP_NMAX));
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
  if (flag == VPL_MARGIN_SECOND_NEW) {
    // removeFront(frame_count = WINDOW_SIZE): no arithmetic
    auto front = [](int n, const int* start, const int* nobs, int* ostart, int* onobs, int* odrop) {
      for (int i = 0; i < n; ++i) {
        ostart[i] = start[i]; onobs[i] = nobs[i]; odrop[i] = -1;
        if (start[i] == WS) { ostart[i] = WS - 1; continue; }
        if (start[i] + nobs[i] - 1 < WS - 1) continue;
        odrop[i] = WS - 1 - start[i];
        onobs[i] = nobs[i] - 1;
      }
    };
    for (int w = 0; w < nW; ++w) {
      front(win[w].n_points, win[w].point_start, win[w].point_nobs, out[w].point_start, out[w].point_nobs, out[w].point_drop);
      front(win[w].n_lines, win[w].line_start, win[w].line_nobs, out[w].line_start, out[w].line_nobs, out[w].line_drop);
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
    for (int i = 0; i < W.n_points; off += W.point_nobs[i], ++i) {
      out[w].point_drop[i] = -1;
      if (W.point_start[i] != 0) { out[w].point_start[i] = W.point_start[i] - 1; out[w].point_nobs[i] = W.point_nobs[i]; continue; }
      out[w].point_drop[i] = 0;
      out[w].point_start[i] = 0;
      out[w].point_nobs[i] = W.point_nobs[i] - 1 < 2 ? 0 : W.point_nobs[i] - 1;
      if (!out[w].point_nobs[i]) continue;
      pw.push_back(w); pidx.push_back(i);
      pd.insert(pd.end(), {W.point_obs[3 * off], W.point_obs[3 * off + 1], W.point_obs[3 * off + 2], W.inv_depth[i]});
    }
    for (int i = 0; i < W.n_lines; ++i) {
      out[w].line_drop[i] = -1;
      if (W.line_start[i] != 0) { out[w].line_start[i] = W.line_start[i] - 1; out[w].line_nobs[i] = W.line_nobs[i]; continue; }
      out[w].line_drop[i] = 0;
      out[w].line_start[i] = 0;
      out[w].line_nobs[i] = W.line_nobs[i] - 1 < 2 ? 0 : W.line_nobs[i] - 1;
      if (!out[w].line_nobs[i]) continue;
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

// The whole solve of the windows [w0, w0 + nw) on stream s
static void launch_solve(vpl_ctx* c, int w0, int nw, hipStream_t s) {
  DevBatch B = c->B;
  B.ord_it = 0;
  // with kernel timing on, every launch also counts the windows that did work in it (vpl_ba_launch_profile)
  B.act = c->timing ? c->d_act : nullptr;
  B.launch = 0;
  if (c->timing) { c->ltimes.clear(); (void)hipMemsetAsync(c->d_act, 0, sizeof(int) * ACT_SLOTS * 4, s); }   // (counts only)
  const dim3 grid(nw);
  launch_prep(c, B, nw, s);
  ++B.launch;
  { KTimer t(c, "k_lin"); hipLaunchKernelGGL(k_lin2, dim3(16 * ((nw + 7) / 8)), dim3(LIN_THREADS), lin_smem(c->maxP, c->maxL), s, B); }
  ++B.launch;
  for (int it = 0; it < c->opt.num_iterations; ++it) {
    B.ord_it = it;      // k_solve / k_cost of iteration `it` walk order[it & 1]; k_cost fills order[(it + 1) & 1]
    // the step: landmark elimination -> reduced camera system -> (general path: windows flagged in B.path only) -> landmark
    // back-substitution + dogleg + candidate.
    { KTimer t(c, "k_schur");
      if (B.WS + 2 <= 48) hipLaunchKernelGGL(k_schur<3>, grid, dim3(SCHUR_THREADS), schur_smem(B.maxP, B.maxL, 3), s, B);
      else if (c->schur_wide_all || (c->schur_mostly_wide && !c->schur_never_wide)) hipLaunchKernelGGL(k_schur<5>, grid, dim3(SCHUR_THREADS), schur_smem(B.maxP, B.maxL, 5), s, B);
      // rows wider than 6 frames: narrow view for the entries of short tracks, all tiles for the flagged ones (round 4)
      else hipLaunchKernelGGL(k_schur_mixed, grid, dim3(SCHUR_THREADS), schur_smem(B.maxP, B.maxL, 3), s, B); }
    ++B.launch;
    { KTimer t(c, "k_chol"); hipLaunchKernelGGL(k_chol, grid, dim3(CHOL_THREADS), CHOL_SMEM, s, B); }
    ++B.launch;
    { KTimer t(c, "k_solve"); hipLaunchKernelGGL(k_solve, grid, dim3(SOLVE_THREADS), solve_smem(B.maxP, B.maxL), s, B); }
    ++B.launch;
    { KTimer t(c, "k_back"); hipLaunchKernelGGL(k_back, grid, dim3(BACK_THREADS), back_smem(B.maxP, B.maxL), s, B); }
    ++B.launch;
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
  if (c) { const int rs = settle(c); if (rs) return rs; }
  if (!c || c->nW < 1) return VPL_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->opt.marginalization_flag != VPL_MARGIN_NONE) { c->prior_resident = true; c->prior_resident_nW = c->nW; }
  if (c->leg_timing) {
    HIPCHK(c, hipEventRecord(c->leg_ev[2], c->stream));
    launch_solve(c, 0, c->nW, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->leg_ev[3], c->stream));
    return VPL_OK;
  }
  if (c->use_graph && !c->timing && c->stream != nullptr) {   // (the legacy default stream cannot be captured)
    if (!c->graph_exec) {
      hipGraph_t graph = nullptr;
      HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
      launch_solve(c, 0, c->nW, c->stream);
      HIPCHK(c, hipStreamEndCapture(c->stream, &graph));
      hipError_t e = hipGraphInstantiate(&c->graph_exec, graph, nullptr, nullptr, 0);
      (void)hipGraphDestroy(graph);   // (the instance does not need it)
      if (e != hipSuccess) { c->graph_exec = nullptr; return fail(c, VPL_E_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e)); }
    }
    HIPCHK(c, hipGraphLaunch(c->graph_exec, c->stream));
    return VPL_OK;
  }
  launch_solve(c, 0, c->nW, c->stream);
  HIPCHK(c, hipGetLastError());
  return VPL_OK;
}

// priors of the last marginalisation (k_marg) of the uploaded batch -> host; mn[2 w] = m, mn[2 w + 1] = n.
// Two steps around ONE device-to-host copy of the staging arena: plan (pieces of the arena + gather segments, a stage_plan), then
// -- after stage_run(c, false) and a stream synchronisation -- finish (scatter into the caller's vpl_prior structs).
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
  HIPCHK(c, stage_run(c, false));
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
  HIPCHK(c, stage_run(c, false));
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
    rc = only_line_opt_impl(c, nW, win, opt, line_reports, false, (orth_given || std::getenv("VPL_BA_ODO_REUPLOAD")) ? nullptr : opt);
    c->odo_ms[1] = std::chrono::duration<double, std::milli>(oclk::now() - t1).count();
    if (rc) return rc;
    // f_manager.removeLineOutlier erased these tracks (estimator.cpp:1037): they take no part in the solve
    bool erased = false;
    for (int w = 0; w < nW; ++w)
      for (int l = 0; l < win[w].n_lines; ++l)
        if (win[w].line_removed[l]) { win[w].line_triangulated[l] = 0; erased = true; }
    batch_resident = !erased && !orth_given && !std::getenv("VPL_BA_ODO_REUPLOAD");
  } else if (line_reports) {
    std::memset(line_reports, 0, sizeof(vpl_solve_report) * (size_t)nW);
  }
  const auto t2 = oclk::now();
  if (batch_resident) {
    // What a fresh upload of the caller's arrays would put on the device is there already: the layout tables, observations,
    // prior and kept-block tables of this very line set, the optimised Pluecker vectors (the caller's copy was downloaded
    // from B.plk), and -- after this restore -- the states k_prep re-normalised in place.  Same bits as the four-stage call.
    if ((rc = restore_states(c, false))) return rc;
    HIPCHK(c, hipMemsetAsync(c->B.ln_removed, 0, (size_t)nW * c->B.maxL * 4, c->stream));
    rc = vpl_ba_solve(c);
    if (!rc) rc = vpl_ctx_synchronize(c);
    if (!rc) rc = vpl_ba_download(c, nW, win, priors, reports);
  } else {
    rc = vpl_ba_solve_windows(c, nW, win, opt, priors, reports);
  }
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

// Debug aid of the randomised sweeps (tools/fuzz_*.py with VPL_DEBUG_GUARDS=1 in the environment when the context is made): the
// 64 bytes behind every device array then hold 0xA5; returns how many arrays have had theirs written to (a kernel ran past the
// end of an array), the first one named in vpl_last_error by its allocation index and size.
int vpl_ba_debug_guards(vpl_ctx* c) { return debug_guards(c); }

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

// ---- keyframe session (vpl_odo_*) -------------------------------------------------------------------------------------
// The reference's FeatureManager + window state for n_seq sequences, resident on the device (csrc/ba_odo.h); the host keeps
// the integer side of the tracks (csrc/odo_tracks.h), from which the existing host code builds the kernels' layout tables.
// A keyframe runs the stages of vpl_ba_solve_odometry -- the same uploads of tables, the same launches -- with every double
// of the batch gathered from the store instead of packed from the caller's arrays, and the results scattered back into it.
struct OdoSeq {
  OdoBook P, L;
  double sum_dt[NF] = {};          // of the 11 pre-integrations (the kept-block table asks for preint[1].sum_dt)
  HostTab prior;                   // block table of the prior the session holds on the device
  bool has_prior = false, set = false;
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
  size_t in_cap = 0, out_cap = 0;
  size_t alloc0 = 0, alloc1 = 0;   // the session's arrays in the context's allocation record
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
  std::vector<int> s_nP, s_nL;
  std::vector<std::vector<int>> s_lmap;
  size_t s_totP = 0, s_totT = 0;
};

static size_t odo_result_bytes(int nS) { return (size_t)nS * sizeof(vpl_odo_result); }

static int odo_alloc_store(vpl_ctx* c, OdoStore& S, size_t nS, int maxPT, int maxLT) {
  hipError_t e = hipSuccess;
  S.maxPT = maxPT; S.maxLT = maxLT;
#define OAL(ptr, n) if (e == hipSuccess) e = dalloc(c, &S.ptr, (size_t)(n))
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

static int odo_check_frame(const vpl_odo_frame& f) {
  if (f.n_points < 0 || f.n_lines < 0) return VPL_E_INVALID;
  if (f.n_points > 0 && (!f.point_id || !f.point_obs)) return VPL_E_INVALID;
  if (f.n_lines > 0 && (!f.line_id || !f.line_obs)) return VPL_E_INVALID;
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
  HIPCHK(c, hipSetDevice(c->device));
  { const int rs = settle(c); if (rs) return rs; }
  vpl_odo* o = new vpl_odo();
  o->c = c; o->nS = n_seq; o->opt = *opt; o->init_depth = init_depth; o->line_min_obs = line_min_obs;
  o->maxPT = max_point_tracks; o->maxLT = max_line_tracks;
  const size_t nS = n_seq;
  o->alloc0 = c->allocs.size();
  int rc = odo_alloc_store(c, o->st[0], nS, o->maxPT, o->maxLT);
  if (!rc) rc = odo_alloc_store(c, o->st[1], nS, o->maxPT, o->maxLT);
  hipError_t e = hipSuccess;
  // per sequence in: pose + speed/bias + pre-integration + one observation per track, header, one table entry per observation
  // and per track (the slide's moves), two counts; out: the result, three flags per track, the prior's block table
  o->in_cap = nS * (8 * (16 + ODO_RAW_PRE_D + 3 * (size_t)o->maxPT + 8 * (size_t)o->maxLT) + 4 * (8 + 2 * ((size_t)o->maxPT + o->maxLT))) + 64;
  o->out_cap = odo_result_bytes(n_seq) + nS * 4 * (3 * ((size_t)o->maxPT + o->maxLT) + 2 + 3 * MAXPB);
  char *din = nullptr, *dout = nullptr;
  if (!rc) {
    if (e == hipSuccess) e = dalloc(c, &o->prior.J0, nS * MAXKEEP * MAXKEEP);
    if (e == hipSuccess) e = dalloc(c, &o->prior.r0, nS * MAXKEEP);
    if (e == hipSuccess) e = dalloc(c, &o->prior.x0, nS * MAXPB * 9);
    if (e == hipSuccess) e = dalloc(c, &o->d_psrc, nS * c->B.maxP);
    if (e == hipSuccess) e = dalloc(c, &o->d_lsrc, nS * c->B.maxL);
    if (e == hipSuccess) e = dalloc(c, &o->d_has, nS);
    if (e == hipSuccess) e = dalloc(c, &o->d_marg, nS);
    if (e == hipSuccess) e = dalloc(c, &din, o->in_cap);
    if (e == hipSuccess) e = dalloc(c, &dout, o->out_cap);
    if (e == hipSuccess) e = hipHostMalloc((void**)&o->h_in, o->in_cap, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&o->h_out, o->out_cap, hipHostMallocDefault);
  }
  o->d_in = din; o->d_out = dout;
  o->alloc1 = c->allocs.size();
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
  // (teardown: a failure has nobody to be reported to)
  (void)hipSetDevice(c->device);
  (void)settle(c);
  (void)hipStreamSynchronize(c->stream);
  for (size_t i = o->alloc0; i < o->alloc1 && i < c->allocs.size(); ++i) (void)hipFree(c->allocs[i]);
  if (o->alloc1 <= c->allocs.size()) {
    c->allocs.erase(c->allocs.begin() + o->alloc0, c->allocs.begin() + o->alloc1);
    c->alloc_bytes.erase(c->alloc_bytes.begin() + o->alloc0, c->alloc_bytes.begin() + o->alloc1);
  }
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
    if (odo_check_frame(frames[f])) return fail(c, VPL_E_INVALID, "odo_set_window: null observation array");
  // the bookkeeping on a copy: a refusal leaves the sequence as it was
  OdoBook P, L;
  std::vector<std::vector<int>> pd(NF), ld(NF);
  for (int f = 0; f < NF; ++f) {
    if ((int)P.t.size() + odo_count_unknown(P, frames[f].n_points, frames[f].point_id) > o->maxPT ||
        (int)L.t.size() + odo_count_unknown(L, frames[f].n_lines, frames[f].line_id) > o->maxLT)
      return fail(c, VPL_E_CAPACITY, "odo_set_window: more tracks than the session's capacity");
    pd[f].resize(frames[f].n_points); ld[f].resize(frames[f].n_lines);
    odo_add_frame(P, f, frames[f].n_points, frames[f].point_id, pd[f].data());
    odo_add_frame(L, f, frames[f].n_lines, frames[f].line_id, ld[f].data());
  }
  HIPCHK(c, hipSetDevice(c->device));
  { const int rs = settle(c); if (rs) return rs; }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // an image of the sequence's part of the store, copied array by array (not on the per-keyframe path)
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
  std::vector<DevPreint> pre(NF);
  std::memset(pre.data(), 0, sizeof(DevPreint) * NF);
  for (int f = 1; f < NF; ++f) to_dev_preint(preint[f], pre[f]);
  const size_t q = seq;
  HIPCHK(c, hipMemcpy(S.pobs + q * S.maxPT * NF * 3, pobs.data(), nP * NF * 3 * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(S.lobs + q * S.maxLT * NF * 8, lobs.data(), nL * NF * 8 * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(S.invd + q * S.maxPT, invd.data(), nP * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(S.plk + q * S.maxLT * 6, plk.data(), nL * 6 * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(S.tri + q * S.maxLT, tri.data(), nL * 4, hipMemcpyHostToDevice));
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
  o->solved = false;
  return VPL_OK;
}

// the refusals of a new frame: null arrays, more tracks than the session holds (counted on the book as it stands)
static int odo_check_next(vpl_odo* o, const vpl_odo_frame* next) {
  vpl_ctx* c = o->c;
  for (int w = 0; w < o->nS; ++w) {
    if (odo_check_frame(next[w])) return fail(c, VPL_E_INVALID, "odo: null observation array");
    // (the inbox holds one observation per track and frame)
    if (next[w].n_points > o->maxPT || next[w].n_lines > o->maxLT) return fail(c, VPL_E_CAPACITY, "odo: more observations in a frame than tracks in the session");
    const OdoSeq& q = o->seq[w];
    if ((int)q.P.t.size() + odo_count_unknown(q.P, next[w].n_points, next[w].point_id) > o->maxPT ||
        (int)q.L.t.size() + odo_count_unknown(q.L, next[w].n_lines, next[w].line_id) > o->maxLT)
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
  vpl_odo_result* d_res = reinterpret_cast<vpl_odo_result*>(o->d_out);
  int* d_flags = reinterpret_cast<int*>(o->d_out + odo_result_bytes(nS));
  const int* h_flags = reinterpret_cast<const int*>(o->h_out + odo_result_bytes(nS));
  const vpl_odo_result* h_res = reinterpret_cast<const vpl_odo_result*>(o->h_out);
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
      HIPCHK(c, hipMemcpyAsync(o->h_out + odo_result_bytes(nS), d_flags, nl * 4, hipMemcpyDeviceToHost, s));
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
    if (nl) HIPCHK(c, hipMemcpyAsync(o->h_out + odo_result_bytes(nS), d_flags, nl * 4, hipMemcpyDeviceToHost, s));
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
    batch_resident = !erased && !std::getenv("VPL_BA_ODO_REUPLOAD");
  }
  lap(1);

  // 3. optimizationwithLine: on the batch where it lies, or on a fresh upload of the lines that are left
  if (batch_resident) {
    if ((rc = restore_states(c, false))) return rc;
    HIPCHK(c, hipMemsetAsync(c->B.ln_removed, 0, (size_t)nS * c->B.maxL * 4, s));
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
  size_t totP = 0, totT = 0, totL = 0;
  std::vector<int> marg(nS, 0);
  for (int w = 0; w < nS; ++w) {
    totP += c->h_nP[w]; totL += c->h_nL[w];
    marg[w] = c->h_passthrough[w] < 0 ? 1 + c->h_mg_nb[w] : 0;
    totT += marg[w] ? 2 + 3 * (marg[w] - 1) : 0;
  }
  {
    const size_t bytes = odo_result_bytes(nS) + 4 * (totP + totT + (solve_opt.remove_line_outliers ? totL : 0));
    HIPCHK(c, hipMemcpyAsync(o->h_out, o->d_out, bytes, hipMemcpyDeviceToHost, s));
    o->d2h += (long long)bytes;
    HIPCHK(c, hipStreamSynchronize(s));
  }
  lap(2);

  // the results, and the prior the marginalisation left: its block table (the values stayed on the device)
  o->s_nP = c->h_nP; o->s_nL = c->h_nL; o->s_lmap = c->h_lmap;
  o->s_totP = totP; o->s_totT = totT;
  o->flag = flag; o->remove_line_outliers = solve_opt.remove_line_outliers;
  size_t kT = 0, kL = 0;
  for (int w = 0; w < nS; ++w) {
    OdoSeq& q = o->seq[w];
    vpl_odo_result& r = out[w];
    r = h_res[w];
    if (o->lstart[w].empty()) std::memset(&r.line_report, 0, sizeof(r.line_report));
    r.line_report.n_lines_removed = lrem1[w];
    r.n_points_solved = c->h_nP[w];
    r.n_lines_solved = c->h_nL[w];
    r.n_point_tracks = (int)q.P.t.size();
    r.n_line_tracks = (int)q.L.t.size();
    r.n_ignored = 0;
    int lrem2 = 0;
    if (solve_opt.remove_line_outliers)
      for (int dl = 0; dl < c->h_nL[w]; ++dl) lrem2 += h_flags[totP + totT + kL + dl] ? 1 : 0;
    kL += c->h_nL[w];
    r.report.n_lines_removed = lrem2;
    if (marg[w]) {
      const int* pt = h_flags + totP + kT;
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

int vpl_odo_advance(vpl_odo* o, const vpl_odo_frame* next, vpl_odo_result* out) {
  if (!o || !next) return VPL_E_INVALID;
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
  const int* h_flags = reinterpret_cast<const int*>(o->h_out + odo_result_bytes(nS));
  const size_t totP = o->s_totP, totT = o->s_totT;
  // 4. the book: removeFailures and the solve's removeLineOutlier, the slide, the new frame -- and the tables that tell the
  // device what moved where; then ONE copy host -> device (the new frames' doubles, then the tables) and two launches
  double* pay = reinterpret_cast<double*>(o->h_in);
  size_t npay = 0;
  for (int w = 0; w < nS; ++w) npay += 16 + ODO_RAW_PRE_D + 3 * (size_t)next[w].n_points + 8 * (size_t)next[w].n_lines;
  int* tab = reinterpret_cast<int*>(o->h_in + npay * 8);
  size_t ntab = 0;
  int* hdr = tab; ntab += 5 * (size_t)nS;
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
    for (int p = 0; p < o->s_nP[w]; ++p, ++kP)
      if (!h_flags[kP]) er[o->psrc[w][p]] = 1;
    odo_erase_slide(q.P, er.data(), flag == VPL_MARGIN_SECOND_NEW, mv, nullptr);
    cnt[2 * w] = (int)mv.size();
    for (size_t j = 0; j < mv.size(); ++j) pmv[(size_t)w * o->maxPT + j] = odo_pack_move(mv[j]);
    // the lines the solve's removeLineOutlier erased
    er.assign(q.L.t.size(), 0);
    if (o->remove_line_outliers)
      for (int dl = 0; dl < o->s_nL[w]; ++dl)
        if (h_flags[totP + totT + kL + dl]) er[o->lsrc[w][o->s_lmap[w][dl]]] = 1;
    kL += o->s_nL[w];
    odo_erase_slide(q.L, er.data(), flag == VPL_MARGIN_SECOND_NEW, mv, nullptr);
    cnt[2 * w + 1] = (int)mv.size();
    for (size_t j = 0; j < mv.size(); ++j) lmv[(size_t)w * o->maxLT + j] = odo_pack_move(mv[j]);
    // pre-integrations: MARGIN_OLD moves 2..10 down, the new interval enters slot 10
    if (flag == VPL_MARGIN_OLD)
      for (int j = 1; j < NF - 1; ++j) q.sum_dt[j] = q.sum_dt[j + 1];
    q.sum_dt[NF - 1] = next[w].preint.sum_dt;
    // the new frame
    const vpl_odo_frame& f = next[w];
    hdr[5 * w] = (int)poff; hdr[5 * w + 1] = f.n_points; hdr[5 * w + 2] = f.n_lines;
    hdr[5 * w + 3] = (int)(ntab + nent); hdr[5 * w + 4] = (int)(ntab + nent + f.n_points);
    r.n_ignored = odo_add_frame(q.P, NF - 1, f.n_points, f.point_id, ent + nent);
    r.n_ignored += odo_add_frame(q.L, NF - 1, f.n_lines, f.line_id, ent + nent + f.n_points);
    nent += (size_t)f.n_points + f.n_lines;
    r.n_point_tracks = (int)q.P.t.size();
    r.n_line_tracks = (int)q.L.t.size();
    double* d = pay + poff;
    std::memcpy(d, f.pose, 56); std::memcpy(d + 7, f.speed_bias, 72); std::memcpy(d + 16, &f.preint, sizeof(f.preint));
    if (f.n_points) std::memcpy(d + 16 + ODO_RAW_PRE_D, f.point_obs, (size_t)f.n_points * 24);
    if (f.n_lines) std::memcpy(d + 16 + ODO_RAW_PRE_D + 3 * (size_t)f.n_points, f.line_obs, (size_t)f.n_lines * 64);
    poff += 16 + ODO_RAW_PRE_D + 3 * (size_t)f.n_points + 8 * (size_t)f.n_lines;
  }
  const size_t in_bytes = npay * 8 + (ntab + nent) * 4;   // (within in_cap: odo_check_next bounds a frame's observations)
  HIPCHK(c, hipMemcpyAsync(o->d_in, o->h_in, in_bytes, hipMemcpyHostToDevice, s));
  o->h2d_payload = (long long)npay * 8;
  o->h2d_table += (long long)(ntab + nent) * 4;
  const int* d_tab = reinterpret_cast<const int*>(o->d_in + npay * 8);
  const OdoStore D = o->st[o->cur ^ 1];
  hipLaunchKernelGGL(k_odo_slide, dim3(nS, ODO_SLIDE_Y), blk, 0, s, S, D, d_tab + (pmv - tab), d_tab + (lmv - tab), d_tab + (cnt - tab),
                     flag == VPL_MARGIN_SECOND_NEW ? 1 : 0, o->init_depth);
  hipLaunchKernelGGL(k_odo_append, grid, blk, 0, s, D, reinterpret_cast<const double*>(o->d_in), d_tab, d_tab);
  HIPCHK(c, hipGetLastError());
  o->cur ^= 1;
  // (the pinned inbox is rewritten by the next keyframe: the copy above must have left it)
  HIPCHK(c, hipStreamSynchronize(s));
  o->solved = false;
  o->ms[3] = std::chrono::duration<double, std::milli>(oclk::now() - t0).count();
  return VPL_OK;
}

int vpl_odo_keyframe(vpl_odo* o, const vpl_odo_frame* next, const int* flags, vpl_odo_result* out) {
  if (!o || !next || !flags || !out) return VPL_E_INVALID;
  if (o->solved) return fail(o->c, VPL_E_INVALID, "odo_keyframe: the window has been solved and not advanced (vpl_odo_advance)");
  int rc = odo_check_next(o, next);
  if (!rc) rc = vpl_odo_solve(o, flags, out);
  if (!rc) rc = vpl_odo_advance(o, next, out);
  return rc;
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

// Host only: the book of one kind of tracks of one sequence replayed from a script (tests/test_odo_tracks.py)
int vpl_odo_debug_tracks(int max_tracks, int n_steps, const int* flag, const int* n_ids, const int* ids, const unsigned char* erase,
                         int* status, int* n_slide, int* slide, int* n_tracks, int* table, int* ignored) {
  if (max_tracks < 1 || n_steps < 0 || !flag || !n_ids || !ids || !erase || !status || !n_slide || !slide || !n_tracks || !table || !ignored)
    return VPL_E_INVALID;
  OdoBook b;
  int frames = 0;
  std::vector<OdoMove> mv;
  for (int s = 0; s < n_steps; ids += n_ids[s], ++s) {
    if (n_ids[s] < 0) return VPL_E_INVALID;
    const bool filling = flag[s] == VPL_MARGIN_NONE;
    if (!filling && flag[s] != VPL_MARGIN_OLD && flag[s] != VPL_MARGIN_SECOND_NEW) return VPL_E_INVALID;
    if (filling ? frames >= NF : frames < NF) return VPL_E_INVALID;
    status[s] = VPL_OK; n_slide[s] = 0; ignored[s] = 0;
    if ((int)b.t.size() + odo_count_unknown(b, n_ids[s], ids) > max_tracks) status[s] = VPL_E_CAPACITY;
    else {
      if (!filling) n_slide[s] = odo_erase_slide(b, erase + (size_t)s * max_tracks, flag[s] == VPL_MARGIN_SECOND_NEW, mv, slide + (size_t)s * max_tracks * 3);
      ignored[s] = odo_add_frame(b, filling ? frames : NF - 1, n_ids[s], ids, nullptr);
      if (filling) ++frames;
    }
    n_tracks[s] = (int)b.t.size();
    for (size_t i = 0; i < b.t.size(); ++i) {
      int* e = table + ((size_t)s * max_tracks + i) * 3;
      e[0] = b.t[i].id; e[1] = b.t[i].start; e[2] = b.t[i].nobs;
    }
  }
  return VPL_OK;
}

}  // extern "C"
