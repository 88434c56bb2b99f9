// Host side of the visual-inertial alignment (vpl_init_align_batch, vpl_init_debug_jobs): the refusals, the job lists of the two
// pre-integration launches, the one packed upload and the one read-back.  Included once by vplines_ba.hip, behind ba_ctx.h.
#pragma once
#include "init_align.h"

// k_preintegrate on device arrays: n intervals, interval k = nsamples[k] samples at samples + 7 * offset[k]
static void launch_preintegrate(vpl_ctx* c, int n, const int* d_offset, const int* d_nsamples, const double* d_samples,
                                const double* d_acc0, const double* d_gyr0, const double* d_lba, const double* d_lbg,
                                const vpl_ba_options* opt, DevPreint* d_out) {
  KTimer t(c, "k_preintegrate");
  hipLaunchKernelGGL(k_preintegrate, dim3((n + 3) / 4), dim3(64), 0, c->stream, n, d_offset, d_nsamples, d_samples, d_acc0, d_gyr0,
                     d_lba, d_lbg, opt->acc_n * opt->acc_n, opt->gyr_n * opt->gyr_n, opt->acc_w * opt->acc_w, opt->gyr_w * opt->gyr_w,
                     d_out);
}
// what k_preintegrate leaves, as the ABI's struct (the 15 x 15 jacobian travels in the sqrt_info slot)
static void from_preintegrate_out(const DevPreint& h, vpl_preintegration& o) {
  o.sum_dt = h.sum_dt;
  for (int k = 0; k < 3; ++k) { o.delta_p[k] = h.dp[k]; o.delta_v[k] = h.dv[k]; o.linearized_ba[k] = h.lba[k]; o.linearized_bg[k] = h.lbg[k]; }
  for (int k = 0; k < 4; ++k) o.delta_q[k] = h.dq[k];
  std::memcpy(o.jacobian, h.sqrt_info, sizeof(o.jacobian));
  std::memcpy(o.covariance, h.cov, sizeof(o.covariance));
}

// the refusals that need nothing but the frame list; msg names the first one met
static int init_check_frames(int F, const int* n_samples, const int* key, std::string& msg) {
  if (!n_samples || !key) { msg = "init: null n_samples / key"; return VPL_E_INVALID; }
  if (F < VPL_NFRAMES) { msg = "init: fewer than 11 image frames"; return VPL_E_INVALID; }
  if (F > VPL_INIT_MAX_FRAMES) { msg = "init: more than VPL_INIT_MAX_FRAMES image frames"; return VPL_E_CAPACITY; }
  if (key[0] != 0 || key[VPL_WINDOW_SIZE] != F - 1) { msg = "init: key[0] != 0 or key[10] != F - 1"; return VPL_E_INVALID; }
  for (int i = 1; i < VPL_NFRAMES; ++i)
    if (key[i] <= key[i - 1]) { msg = "init: key not strictly increasing"; return VPL_E_INVALID; }
  for (int f = 1; f < F; ++f)
    if (n_samples[f] < 1) { msg = "init: an interval without samples"; return VPL_E_INVALID; }
  return VPL_OK;
}
// jobs [F + 9][3] = (offset, nsamples, acc0 row) of the image intervals 1 .. F-1, then of the window intervals 1 .. 10: window
// interval i is the contiguous sample range of the image intervals key[i-1]+1 .. key[i] and starts from what the first of them
// starts from
static void init_build_jobs(int F, const int* n_samples, const int* key, int* jobs) {
  std::vector<int> off(F + 1, 0);
  for (int f = 1; f < F; ++f) off[f + 1] = off[f] + n_samples[f];
  for (int f = 1; f < F; ++f) {
    int* j = jobs + 3 * (f - 1);
    j[0] = off[f]; j[1] = n_samples[f]; j[2] = off[f] - 1;
  }
  for (int i = 1; i < VPL_NFRAMES; ++i) {
    int* j = jobs + 3 * (F - 1 + i - 1);
    j[0] = off[key[i - 1] + 1]; j[1] = off[key[i] + 1] - off[key[i - 1] + 1]; j[2] = j[0] - 1;
  }
}

// the pads behind the arrays `owner` took (VPL_DEBUG_GUARDS=1): how many were written to
static int init_guard_hits(vpl_ctx* c, const void* owner, int* hits) {
  *hits = 0;
  if (!c->guards) return VPL_OK;
  unsigned char pad[64];
  for (const DevAlloc& a : c->allocs) {
    if (a.owner != owner) continue;
    HIPCHK(c, hipMemcpy(pad, (char*)a.p + a.bytes, 64, hipMemcpyDeviceToHost));
    bool hit = false;
    for (int k = 0; k < 64; ++k) hit |= pad[k] != 0xA5;
    *hits += hit ? 1 : 0;
  }
  return VPL_OK;
}

// The device side of one alignment call: what stages 1-4 read and leave.  The arrays are taken through the context's guarded
// allocator under `owner` and given back with dfree_owner.
struct InitDevice {
  char* in = nullptr;               // the packed upload
  double* lba3 = nullptr;           // zero: the re-propagation's accelerometer bias
  double* lbg3 = nullptr;
  DevPreint* pre1 = nullptr;
  double* acc = nullptr;
  char* outb = nullptr;             // vpl_init_result [n] | DevPreint [n3]
  size_t res_bytes = 0;
  int n = 0, J1 = 0, n3 = 0, ld = 0;
  std::vector<int> F, job0;
  std::vector<char> hbuf;           // the upload's host side, alive until the call's synchronisation
  vpl_init_result* results() const { return (vpl_init_result*)outb; }
  DevPreint* pre3() const { return (DevPreint*)(outb + res_bytes); }
};

// the refusals of every sequence of a call, before anything is allocated
static int init_check_inputs(vpl_ctx* c, int n, const vpl_init_input* in) {
  for (int s = 0; s < n; ++s) {
    const vpl_init_input& q = in[s];
    if (!q.R || !q.T || !q.samples || !q.lin_ba || !q.lin_bg) return fail(c, VPL_E_INVALID, "init: null array in sequence " + std::to_string(s));
    std::string msg;
    const int rc = init_check_frames(q.n_frames, q.n_samples, q.key, msg);
    if (rc) return fail(c, rc, msg + " (sequence " + std::to_string(s) + ")");
  }
  return VPL_OK;
}

// checks every sequence, packs, uploads (one copy) and enqueues stages 1-4 on the context's stream
static int init_enqueue(vpl_ctx* c, int n, const vpl_init_input* in, const vpl_ba_options* opt, const void* owner, InitDevice& D) {
  { const int rc = init_check_inputs(c, n, in); if (rc) return rc; }
  size_t nF = 0, nS = 0;
  int Fmax = 0;
  D.n = n; D.F.resize(n); D.job0.resize(n);
  for (int s = 0; s < n; ++s) {
    D.F[s] = in[s].n_frames;
    D.job0[s] = (int)nF - s;
    nF += in[s].n_frames;
    Fmax = std::max(Fmax, in[s].n_frames);
    for (int f = 1; f < in[s].n_frames; ++f) nS += in[s].n_samples[f];
  }
  const int J1 = (int)nF - n, n3 = J1 + VPL_WINDOW_SIZE * n, ld = 3 * Fmax + 4;
  D.J1 = J1; D.n3 = n3; D.ld = ld;
  // ---- the packed upload: doubles, then the sequence records, then the integers
  const size_t o_samples = 0, o_acc0 = o_samples + nS * 7, o_gyr0 = o_acc0 + (size_t)n3 * 3, o_lba1 = o_gyr0 + (size_t)n3 * 3,
               o_lbg1 = o_lba1 + (size_t)J1 * 3, o_R = o_lbg1 + (size_t)J1 * 3, o_T = o_R + nF * 9, n_dbl = o_T + nF * 3;
  const size_t b_seq = n_dbl * 8, b_off = b_seq + (size_t)n * sizeof(DevInitSeq), b_ns = b_off + (size_t)n3 * 4, bytes = b_ns + (size_t)n3 * 4;
  std::vector<char>& buf = D.hbuf;
  buf.assign(bytes, 0);
  double* hd = (double*)buf.data();
  DevInitSeq* hs = (DevInitSeq*)(buf.data() + b_seq);
  int* h_off = (int*)(buf.data() + b_off);
  int* h_ns = (int*)(buf.data() + b_ns);
  std::vector<int> jobs;
  size_t frame0 = 0, samp0 = 0;
  for (int s = 0; s < n; ++s) {
    const vpl_init_input& q = in[s];
    const int F = q.n_frames;
    jobs.assign((size_t)(F + 9) * 3, 0);
    init_build_jobs(F, q.n_samples, q.key, jobs.data());
    size_t ns = 0;
    for (int f = 1; f < F; ++f) ns += q.n_samples[f];
    std::memcpy(hd + o_samples + samp0 * 7, q.samples, ns * 7 * 8);
    std::memcpy(hd + o_R + frame0 * 9, q.R, (size_t)F * 9 * 8);
    std::memcpy(hd + o_T + frame0 * 3, q.T, (size_t)F * 3 * 8);
    for (int j = 0; j < F + 9; ++j) {
      const int dj = j < F - 1 ? D.job0[s] + j : J1 + VPL_WINDOW_SIZE * s + (j - (F - 1));
      h_off[dj] = (int)samp0 + jobs[3 * j];
      h_ns[dj] = jobs[3 * j + 1];
      const int row = jobs[3 * j + 2];
      for (int k = 0; k < 3; ++k) {
        hd[o_acc0 + (size_t)dj * 3 + k] = row < 0 ? q.acc0[k] : q.samples[(size_t)row * 7 + 1 + k];
        hd[o_gyr0 + (size_t)dj * 3 + k] = row < 0 ? q.gyr0[k] : q.samples[(size_t)row * 7 + 4 + k];
      }
      if (j < F - 1)
        for (int k = 0; k < 3; ++k) {
          hd[o_lba1 + (size_t)dj * 3 + k] = q.lin_ba[3 * (j + 1) + k];
          hd[o_lbg1 + (size_t)dj * 3 + k] = q.lin_bg[3 * (j + 1) + k];
        }
    }
    DevInitSeq& d = hs[s];
    d.F = F; d.frame0 = (int)frame0; d.job0 = D.job0[s]; d.wjob0 = J1 + VPL_WINDOW_SIZE * s;
    for (int i = 0; i < VPL_NFRAMES; ++i) {
      d.key[i] = q.key[i];
      for (int k = 0; k < 3; ++k) { d.bas[3 * i + k] = q.bas[i][k]; d.bgs[3 * i + k] = q.bgs[i][k]; }
    }
    for (int k = 0; k < 3; ++k) d.tic[k] = q.tic[k];
    frame0 += F; samp0 += ns;
  }
  // ---- device arrays
  HIPCHK(c, hipSetDevice(c->device));
  D.res_bytes = ((size_t)n * sizeof(vpl_init_result) + 63) & ~(size_t)63;
  HIPCHK(c, dalloc(c, &D.in, bytes, owner));
  HIPCHK(c, dalloc(c, &D.lba3, (size_t)n3 * 3, owner));
  HIPCHK(c, dalloc(c, &D.lbg3, (size_t)n3 * 3, owner));
  HIPCHK(c, dalloc(c, &D.pre1, (size_t)J1, owner));
  HIPCHK(c, dalloc(c, &D.acc, (size_t)n * (ld + 1) * ld, owner));
  HIPCHK(c, dalloc(c, &D.outb, D.res_bytes + (size_t)n3 * sizeof(DevPreint), owner));
  // the zeros the kernels rely on, ordered before them on the context's stream (the allocator's own run on the null stream)
  HIPCHK(c, hipMemsetAsync(D.lba3, 0, (size_t)n3 * 3 * sizeof(double), c->stream));
  HIPCHK(c, hipMemsetAsync(D.outb, 0, D.res_bytes, c->stream));
  HIPCHK(c, hipMemcpyAsync(D.in, buf.data(), bytes, hipMemcpyHostToDevice, c->stream));
  const double* dd = (const double*)D.in;
  const DevInitSeq* ds = (const DevInitSeq*)(D.in + b_seq);
  const int* d_off = (const int*)(D.in + b_off);
  const int* d_ns = (const int*)(D.in + b_ns);
  // 1. the image intervals under the bias they stand at
  launch_preintegrate(c, J1, d_off, d_ns, dd + o_samples, dd + o_acc0, dd + o_gyr0, dd + o_lba1, dd + o_lbg1, opt, D.pre1);
  // 2. solveGyroscopeBias
  hipLaunchKernelGGL(k_init_gyro_bias, dim3(n), dim3(64), 0, c->stream, ds, dd + o_R, (const DevPreint*)D.pre1, D.lbg3, D.results());
  // 3. image and window intervals again, under (0, Bgs[0]) and (0, Bgs[i])
  launch_preintegrate(c, n3, d_off, d_ns, dd + o_samples, dd + o_acc0, dd + o_gyr0, D.lba3, D.lbg3, opt, D.pre3());
  // 4. LinearAlignment, RefineGravity, the state change
  hipLaunchKernelGGL(k_init_align, dim3(n), dim3(INIT_THREADS), init_lds_bytes(ld), c->stream, ds, dd + o_R, dd + o_T,
                     (const DevPreint*)D.pre3(), D.acc, ld, opt->g_norm, D.results());
  HIPCHK(c, hipGetLastError());
  return VPL_OK;
}

extern "C" {

int vpl_init_debug_jobs(int n_frames, const int* n_samples, const int* key, int* jobs) {
  if (!jobs) return VPL_E_INVALID;
  std::string msg;
  const int rc = init_check_frames(n_frames, n_samples, key, msg);
  if (rc) return rc;
  init_build_jobs(n_frames, n_samples, key, jobs);
  return VPL_OK;
}

int vpl_init_align_batch(vpl_ctx* c, int n, const vpl_init_input* in, const vpl_ba_options* opt, vpl_init_result* out,
                         vpl_preintegration* window_preint, vpl_preintegration* image_preint) {
  if (!c || n < 0 || !in || !opt || !out) return VPL_E_INVALID;
  if (n == 0) return VPL_OK;
  if (n > c->maxW) return fail(c, VPL_E_CAPACITY, "init: more sequences than max_windows");
  const int rs = settle(c);
  if (rs) return rs;
  InitDevice D;
  const void* owner = &D;
  int rc = init_enqueue(c, n, in, opt, owner, D);
  std::vector<char> h;
  if (rc == VPL_OK) {
    const bool want_pre = window_preint || image_preint;
    h.resize(want_pre ? D.res_bytes + (size_t)D.n3 * sizeof(DevPreint) : D.res_bytes);
    hipError_t e = hipMemcpyAsync(h.data(), D.outb, h.size(), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(c, VPL_E_HIP, std::string("init: ") + hipGetErrorString(e));
  }
  if (rc == VPL_OK) {
    int hits = 0;
    rc = init_guard_hits(c, owner, &hits);
    if (rc == VPL_OK && hits) rc = fail(c, VPL_E_HIP, "init: guard behind " + std::to_string(hits) + " device array(s) overwritten");
  }
  dfree_owner(c, owner);
  if (rc) return rc;
  std::memcpy(out, h.data(), (size_t)n * sizeof(vpl_init_result));
  const DevPreint* p3 = (const DevPreint*)(h.data() + D.res_bytes);
  for (int s = 0; s < n; ++s) {
    if (window_preint) {
      vpl_preintegration* w = window_preint + (size_t)s * VPL_NFRAMES;
      std::memset(w, 0, sizeof(vpl_preintegration));
      for (int i = 1; i < VPL_NFRAMES; ++i) from_preintegrate_out(p3[D.J1 + VPL_WINDOW_SIZE * s + i - 1], w[i]);
    }
    if (image_preint) {
      vpl_preintegration* w = image_preint + (size_t)s * VPL_INIT_MAX_FRAMES;
      std::memset(w, 0, sizeof(vpl_preintegration) * VPL_INIT_MAX_FRAMES);
      for (int f = 1; f < D.F[s]; ++f) from_preintegrate_out(p3[D.job0[s] + f - 1], w[f]);
    }
  }
  return VPL_OK;
}

}  // extern "C"
