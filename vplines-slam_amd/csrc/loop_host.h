// Host side of the loop verification (vpl_loop_verify_batch, vpl_loop_debug_plan): the refusals, the stopping table of every list
// length that runs, the one packed upload and the one read-back.  Included once by vplines_ba.hip, behind init_relpose_host.h.
#pragma once
#include <unordered_map>

#include "loop_verify.h"

extern "C" {

void vpl_loop_default_options(vpl_loop_options* o) {
  if (!o) return;
  o->min_loop_num = 25; o->max_iters = 100; o->reproj_error = 10.0 / 460.0; o->confidence = 0.99; o->max_yaw_deg = 30.0; o->max_t = 20.0;
}

int vpl_loop_debug_plan(unsigned long long seed, int n_points, double confidence, int max_iters, int* samples, int* niters_after) {
  if (!samples || !niters_after || n_points < LOOP_SAMPLE || max_iters < 1 || max_iters > VPL_LOOP_MAX_ITERS) return VPL_E_INVALID;
  if (n_points > VPL_LOOP_MAX_POINTS) return VPL_E_CAPACITY;
  for (int it = 0; it < max_iters; ++it) {
    int idx[LOOP_SAMPLE] = {-1, -1, -1, -1, -1};
    loop_sample(seed, it, n_points, idx);
    for (int k = 0; k < LOOP_SAMPLE; ++k) samples[LOOP_SAMPLE * it + k] = idx[k];
  }
  loop_niters_table(n_points, confidence, max_iters, niters_after);
  return VPL_OK;
}

int vpl_loop_verify_batch(vpl_ctx* c, int n, const vpl_loop_input* in, const vpl_loop_options* opt, vpl_loop_result* out,
                          unsigned char* status) {
  if (!c || n < 0 || !in || !opt || !out || !status) return VPL_E_INVALID;
  if (n == 0) return VPL_OK;
  if (n > c->maxW) return fail(c, VPL_E_CAPACITY, "loop: more items than max_windows");
  if (opt->max_iters < 1 || opt->max_iters > VPL_LOOP_MAX_ITERS || opt->min_loop_num < LOOP_SAMPLE - 1 || !(opt->reproj_error > 0.0) ||
      !(opt->confidence > 0.0) || !std::isfinite(opt->reproj_error) || !std::isfinite(opt->confidence))
    return fail(c, VPL_E_INVALID, "loop: options out of range");
  for (int s = 0; s < n; ++s) {
    if (in[s].count < 0 || (in[s].count && (!in[s].pts3d || !in[s].old_norm)))
      return fail(c, VPL_E_INVALID, "loop: negative count or null lists (item " + std::to_string(s) + ")");
    if (in[s].count > VPL_LOOP_MAX_POINTS) return fail(c, VPL_E_CAPACITY, "loop: more than VPL_LOOP_MAX_POINTS points (item " + std::to_string(s) + ")");
  }
  const int rs = settle(c);
  if (rs) return rs;
  // ---- the packed upload: points | observations (both widened: the device computes in double) | items | tables
  const size_t MP = VPL_LOOP_MAX_POINTS;
  std::vector<DevLoopItem> items(n);
  std::vector<int> tables;
  std::unordered_map<int, int> table_at;
  std::vector<double> X((size_t)n * MP * 3, 0.0), uv((size_t)n * MP * 2, 0.0);
  for (int s = 0; s < n; ++s) {
    const vpl_loop_input& q = in[s];
    DevLoopItem d{};
    d.count = q.count; d.seed = q.seed; d.nit = 0;
    std::memcpy(d.vioT, q.origin_vio_T, sizeof d.vioT); std::memcpy(d.vioR, q.origin_vio_R, sizeof d.vioR);
    std::memcpy(d.tic, q.tic, sizeof d.tic); std::memcpy(d.qic, q.qic, sizeof d.qic);
    for (int k = 0; k < 3 * q.count; ++k) X[(size_t)s * MP * 3 + k] = (double)q.pts3d[k];
    for (int k = 0; k < 2 * q.count; ++k) uv[(size_t)s * MP * 2 + k] = (double)q.old_norm[k];
    if (q.count > opt->min_loop_num) {
      auto it = table_at.find(q.count);
      if (it == table_at.end()) {
        const int at = (int)tables.size();
        tables.resize(at + q.count + 1);
        loop_niters_table(q.count, opt->confidence, opt->max_iters, tables.data() + at);
        it = table_at.emplace(q.count, at).first;
      }
      d.nit = it->second;
    }
    items[s] = d;
  }
  auto up64 = [](size_t b) { return (b + 63) & ~(size_t)63; };
  const size_t b_uv = up64(X.size() * 8), b_items = up64(b_uv + uv.size() * 8), b_tab = up64(b_items + items.size() * sizeof(DevLoopItem)),
               bytes = b_tab + std::max<size_t>(tables.size(), 1) * 4;
  std::vector<char> buf(bytes, 0);
  std::memcpy(buf.data(), X.data(), X.size() * 8);
  std::memcpy(buf.data() + b_uv, uv.data(), uv.size() * 8);
  std::memcpy(buf.data() + b_items, items.data(), items.size() * sizeof(DevLoopItem));
  if (!tables.empty()) std::memcpy(buf.data() + b_tab, tables.data(), tables.size() * 4);
  // ---- the read-back: results | status
  const size_t o_st = up64((size_t)n * sizeof(vpl_loop_result)), out_bytes = o_st + (size_t)n * MP;
  const void* owner = &items;
  char *d_in = nullptr, *d_out = nullptr, *d_cur = nullptr;
  double* d_wo = nullptr;
  int* d_itab = nullptr;
  std::vector<char> h(out_bytes);
  auto run = [&]() -> int {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, dalloc(c, &d_in, bytes, owner));
    HIPCHK(c, dalloc(c, &d_out, out_bytes, owner));
    HIPCHK(c, dalloc(c, &d_wo, (size_t)n * MP * SFM_OBS_WS, owner));
    HIPCHK(c, dalloc(c, &d_itab, (size_t)n * LV_ITAB, owner));
    HIPCHK(c, dalloc(c, &d_cur, (size_t)n * MP, owner));
    // (the allocator's zeroing runs on the null stream: what the kernel relies on is set again in stream order)
    HIPCHK(c, hipMemsetAsync(d_out, 0, out_bytes, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_in, buf.data(), bytes, hipMemcpyHostToDevice, c->stream));
    DevLoopArgs A;
    A.X = (double*)d_in; A.uv = (double*)(d_in + b_uv);
    A.items = (const DevLoopItem*)(d_in + b_items); A.tables = (const int*)(d_in + b_tab);
    A.wo = d_wo; A.itab = d_itab; A.cur = (unsigned char*)d_cur;
    A.out = (vpl_loop_result*)d_out; A.status = (unsigned char*)(d_out + o_st);
    A.opt = *opt;
    { KTimer t(c, "k_loop_verify"); hipLaunchKernelGGL(k_loop_verify, dim3(n), dim3(SFM_THREADS), 0, c->stream, A); }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h.data(), d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int hits = 0;
    const int rg = init_guard_hits(c, owner, &hits);
    if (rg) return rg;
    if (hits) return fail(c, VPL_E_HIP, "loop: guard behind " + std::to_string(hits) + " device array(s) overwritten");
    return VPL_OK;
  };
  const int rc = run();
  dfree_owner(c, owner);
  if (rc) return rc;
  std::memcpy(out, h.data(), (size_t)n * sizeof(vpl_loop_result));
  for (int s = 0; s < n; ++s) std::memcpy(status + (size_t)s * MP, h.data() + o_st + (size_t)s * MP, (size_t)in[s].count);
  return VPL_OK;
}

}  // extern "C"
