// The bundle-adjustment context (the opaque vpl_ctx of include/vplines_ba.h) and the small pieces every entry point of
// vplines_ba.hip leans on: the captured graph's lifetime, the completion of asynchronous calls, the kernel timer, a device
// buffer that frees itself.  vpl_ctx is not part of the ABI.
#pragma once
#include <functional>
#include <map>
#include <string>

#include "vplines_ba.h"
#include "ba_types.h"
#include "ba_stage.h"
#include "ba_restore.h"

struct vpl_ctx {
  // ---- device, stream, the batch's arrays
  int device = 0;
  hipStream_t stream = nullptr;
  DevBatch B;
  std::vector<DevAlloc> allocs;      // host_common.h: the context's own arrays (owner null), then those of the session that borrows it
  bool guards = false;
  std::string err;
  long long sel_stats[3] = {0, 0, 0};   // vpl_select_stats: launches, bytes up, bytes down of the last selector call
  // ---- capacities
  int maxW = 0, maxP = 0, maxPO = 0, maxL = 0, maxLO = 0;
  // ---- the uploaded batch's host tables
  int nW = 0;
  vpl_ba_options opt;
  bool upload_open = false;                      // an upload has started to rewrite the host tables of the batch and has not finished
  std::vector<int> h_nP, h_nL;
  std::vector<std::vector<int>> h_lmap;          // per window: device line index -> index in the vpl_window arrays
  // host-side marg structure of the uploaded windows
  std::vector<int> h_mg_m;
  std::vector<int> h_mg_n;                       // kept dims of the next prior as the host computed them (>= the device's)
  std::vector<int> h_mg_nb;                      // kept blocks of the next prior as the host laid them out
  std::vector<int> h_passthrough;              // MARGIN_SECOND_NEW: window keeps its input prior (index into h_pass_priors or -1)
  std::vector<vpl_prior> h_pass_priors;
  bool any_second_new = false;
  int maxPriorN = 0;                             // largest prior of the uploaded batch (k_prep stages J0 in LDS)
  // a window of the uploaded batch takes the general path (B.path == 1, VPL_BA_GENERAL=1 included): k_lin may store to entries
  // of Hcc outside the fast path's pattern, which every other window expects to hold the zeros Hcc was allocated with -- the
  // next upload zero-fills Hcc
  bool hcc_general = false;
  bool prior_resident = false;                   // the last solve / marginalisation of the uploaded batch left its priors in mg_* (vpl_ba_upload_chained)
  int prior_resident_nW = 0;
  // signature of the track layout (start frames, lengths, selected lines) of the last upload: when the next batch has the same
  // one -- the usual case between two solves of a tracker that lost and gained nothing, and every repetition of a benchmark --
  // the host-built lane / unit / K-step tables and the index arrays already on the device are the right ones and are neither
  // rebuilt nor uploaded again
  std::vector<int> layout_key;                   // the integers the signature is made of
  bool layout_valid = false;
  // ---- launch choices
  bool force_general = false;                    // VPL_BA_GENERAL=1: every window takes k_solve (A/B runs, tests of the general path)
  bool schur_mostly_wide = false;                // more than 35 % of the landmark elimination's weight sits in wide entries: k_schur<5>
  bool schur_never_wide = false;                 // VPL_BA_SCHUR_WIDE=-1: k_schur_mixed whatever the share of wide entries (A/B runs)
  bool schur_wide_all = false;                   // VPL_BA_SCHUR_WIDE=1: round 3's k_schur<5> for batches with long tracks (A/B runs, tests)
  bool step_fused = true;                        // VPL_BA_STEP_FUSED=0: the step as k_schur, k_chol, k_back instead of k_step (A/B runs, tests); a timed solve always is
  size_t marg_smem = 0;
  int marg_nmax = 0;                             // largest kept block of the uploaded batch (k_prior_eigen's LDS layout)
  bool marg_small = false;                       // k_marg<256> (two work-groups per CU) instead of k_marg<512>
  int prior_rule = VPL_PRIOR_PIVOTED_CHOLESKY;   // vpl_ba_set_prior_rule
  // ---- graph
  // the ~19 launches of one solve as a hipGraph, captured on the first vpl_ba_solve after an upload (the kernel arguments --
  // the batch descriptor by value -- are fixed until the next upload); VPL_BA_GRAPH=0 launches kernel by kernel
  // k_prep's restore mode is one of those arguments: one instance per RestoreMode, each captured on its first use
  hipGraphExec_t graph_exec[3] = {nullptr, nullptr, nullptr};
  bool use_graph = true;
  // ---- pending restore (ba_restore.h)
  int restore_pending = RESTORE_NONE;            // vpl_ba_reset_state was called and nothing has restored the states yet
  bool restore_fold = true;                      // VPL_BA_RESET_FOLD=0: vpl_ba_reset_state issues its five copies at once (A/B runs, tests)
  // ---- timing
  bool timing = false;
  std::map<std::string, std::pair<double, int>> ktimes;
  std::vector<std::pair<const char*, double>> ltimes;   // (kernel, ms) of every launch of the last timed solve, in order
  int* d_act = nullptr;                                 // [ACT_SLOTS][4] activity counters of those launches
  std::vector<std::string> kname_store;
  // device time of the last upload / solve / download (hipEvents on the context's stream), vpl_ctx_enable_leg_timing
  bool leg_timing = false;
  hipEvent_t leg_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double odo_ms[3] = {0, 0, 0};                  // vpl_ba_debug_odometry_ms
  // ---- asynchronous completion
  // asynchronous variants of the line-map entry points: the host-side completion (wait for the stream, scatter the staged
  // results into the caller's arrays) of the call that was enqueued last; run by vpl_ba_collect or by the next call that
  // touches the batch
  std::function<int()> pending;
  // ---- staging
  Stage stage;                                   // pinned + device staging arenas of upload / download
  size_t last_upload_bytes = 0;                  // what the last upload's one host-to-device copy moved
  // ---- session
  struct vpl_odo* odo = nullptr;                 // the keyframe session that borrows this context (one per context)
};

static void drop_graph(vpl_ctx* c) {
  for (hipGraphExec_t& g : c->graph_exec)
    if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
}

// the states of the uploaded batch back to what the upload put there (pose, sb, ex, invd and, RESTORE_LINES, the lines)
static int restore_states(vpl_ctx* c, int mode) {
  if (mode == RESTORE_NONE || c->nW < 1) return VPL_OK;
  const DevBatch& B = c->B;
  const size_t W = c->nW;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(B.pose, B.pose_0, W * 77 * 8, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(B.sb, B.sb_0, W * 99 * 8, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(B.ex, B.ex_0, W * 7 * 8, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(B.invd, B.invd_0, W * B.maxP * 8, hipMemcpyDeviceToDevice, c->stream));
  if (mode == RESTORE_LINES) HIPCHK(c, hipMemcpyAsync(B.plk, B.plk_0, W * B.maxL * 6 * 8, hipMemcpyDeviceToDevice, c->stream));
  return VPL_OK;
}
// one call's effect on the pending restore (restore_step, ba_restore.h): issues the copies it asks for; *prep, if given,
// receives the mode the caller has to hand to k_prep
static int restore_event(vpl_ctx* c, RestoreEvent ev, int* prep = nullptr) {
  const RestoreStep s = restore_step(c->restore_pending, ev, c->restore_fold);
  c->restore_pending = s.pending;
  if (prep) *prep = s.prep;
  return restore_states(c, s.flush);
}

// completes the asynchronous call that is still pending on this context, if any
static int settle_call(vpl_ctx* c) {
  if (!c || !c->pending) return VPL_OK;
  std::function<int()> fin;
  fin.swap(c->pending);
  return fin();
}
// ... and brings the states up to date: what every entry point starts with, except those that deal with the pending restore
// themselves (vpl_ba_reset_state, vpl_ba_solve, the upload, vpl_ctx_set_stream)
static int settle(vpl_ctx* c) {
  if (!c) return VPL_OK;
  const int rs = settle_call(c);
  if (rs) return rs;
  return restore_event(c, RESTORE_EV_OBSERVE);
}
// the tail of an entry point: now, or (asynchronous variant) when the caller collects
static int finish_or_defer(vpl_ctx* c, bool async, std::function<int()> fin) {
  if (!async) return fin();
  c->pending = std::move(fin);
  return VPL_OK;
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
