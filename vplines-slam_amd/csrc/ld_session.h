// Loop detector session (vpl_ld_*): the host side of ld_kernels.h.  Included at the end of vplines_frontend.hip.
#pragma once

struct vpl_ld {
  vpl_fe_ctx* c = nullptr;
  int nDb = 0;
  vpl_ld_options opt;
  vpl::LdBatch B;
  bool haveVocab = false;
  std::vector<int> nEntries;          // host mirror of the databases' lengths (sizes the scoring grid; exact: a refused call adds nothing)
  unsigned char* d_in = nullptr;      // counts [nDb], frame_index [nDb] (padded to 16 bytes), descriptor rows [nDb][MK][4]
  size_t in_bytes = 0, brief_off = 0;
  int bagP = 0;                       // k_ld_bag's LDS is laid out for this many word ids
  size_t bagSmem = 0;
  // the vocabulary's arrays
  int *d_childBegin = nullptr, *d_childCount = nullptr, *d_word = nullptr, *d_table = nullptr;
  unsigned long long* d_desc = nullptr;
  double* d_wordWeight = nullptr;
};

extern "C" {

void vpl_ld_default_options(vpl_ld_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->max_keyframes = 2048; o->max_keypoints = 8192; o->max_words_total = 2048 * 3000;
  o->max_results = 4; o->recent = 50; o->neighbour_score = 0.05; o->loop_score = 0.015;
}

void vpl_ld_destroy(vpl_ld* t) {
  if (!t) return;
  vpl_fe_ctx* c = t->c;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  dfree_owner(c, t);
  if (c->ld == t) c->ld = nullptr;
  delete t;
}

static int ld_alloc(vpl_ld* t) {
  using namespace vpl;
  vpl_fe_ctx* c = t->c;
  LdBatch& B = t->B;
  const size_t nDb = t->nDb, MK = B.MK, KF = B.maxKf, PL = B.pool;
  HIPCHK(c, dalloc(c, &B.dWord, nDb * MK, t)); HIPCHK(c, dalloc(c, &B.qWord, nDb * MK, t)); HIPCHK(c, dalloc(c, &B.qVal, nDb * MK, t));
  HIPCHK(c, dalloc(c, &B.qN, nDb, t)); HIPCHK(c, dalloc(c, &B.flag, nDb, t)); HIPCHK(c, dalloc(c, &B.nEntries, nDb, t));
  HIPCHK(c, dalloc(c, &B.poolUsed, nDb, t)); HIPCHK(c, dalloc(c, &B.entryOff, nDb * (KF + 1), t));
  HIPCHK(c, dalloc(c, &B.poolWord, nDb * PL, t)); HIPCHK(c, dalloc(c, &B.poolVal, nDb * PL, t));
  HIPCHK(c, dalloc(c, &B.raw, nDb * KF, t)); HIPCHK(c, dalloc(c, &B.hit, nDb * KF, t)); HIPCHK(c, dalloc(c, &B.out, nDb, t));
  HIPCHK(c, dalloc(c, &t->d_in, t->in_bytes, t));
  return VPL_OK;
}

int vpl_ld_create(vpl_ld** out, vpl_fe_ctx* c, int n_db, const vpl_ld_options* opt) {
  using namespace vpl;
  if (!out || !c || !opt || n_db < 1) return VPL_E_INVALID;
  if (c->ld) return fail(c, VPL_E_INVALID, "ld: the context already lends itself to a loop detector session");
  if (opt->max_keyframes < 1 || opt->max_keypoints < 1 || opt->max_words_total < 1 || opt->max_results < 1 ||
      opt->max_results > LD_MAX_RESULTS || opt->recent < 0)
    return fail(c, VPL_E_INVALID, "ld: options out of range (max_results is 1 .. 4)");
  if (opt->max_keypoints > LD_MAX_KEYPOINTS) return fail(c, VPL_E_CAPACITY, "ld: max_keypoints above 8192, what the bag kernel sorts in LDS");
  if ((long long)opt->max_keyframes * n_db > 0x7fffffffLL / 2 || (long long)opt->max_words_total * n_db > 0x7fffffffLL)
    return fail(c, VPL_E_CAPACITY, "ld: n_db x max_keyframes or n_db x max_words_total too large");
  HIPCHK(c, hipSetDevice(c->device));
  vpl_ld* t = new vpl_ld();
  t->c = c; t->nDb = n_db; t->opt = *opt;
  t->nEntries.assign(n_db, 0);
  LdBatch& B = t->B;
  std::memset(&B, 0, sizeof(B));
  B.nDb = n_db; B.MK = opt->max_keypoints; B.maxKf = opt->max_keyframes; B.pool = opt->max_words_total;
  B.maxResults = opt->max_results; B.recent = opt->recent; B.neighbourScore = opt->neighbour_score; B.loopScore = opt->loop_score;
  t->brief_off = ((size_t)n_db * 8 + 15) & ~(size_t)15;
  t->in_bytes = t->brief_off + (size_t)n_db * B.MK * 32;
  t->bagP = 1;
  while (t->bagP < B.MK) t->bagP <<= 1;
  t->bagSmem = (size_t)t->bagP * 16 + 16;
  c->ld = t;
  int rc = ld_alloc(t);
  if (!rc && t->bagSmem > 48 * 1024) {
    static size_t bag_max = 0;   // per kernel, never lowered by a later, smaller session
    if (t->bagSmem > bag_max) {
      const hipError_t e = hipFuncSetAttribute((const void*)k_ld_bag, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t->bagSmem);
      if (e != hipSuccess) rc = fail(c, VPL_E_HIP, std::string("ld: ") + hipGetErrorString(e)); else bag_max = t->bagSmem;
    }
  }
  if (rc) { vpl_ld_destroy(t); return rc; }
  *out = t;
  return VPL_OK;
}

// every database empty (device and mirror).  Asynchronous.
static int ld_clear(vpl_ld* t) {
  vpl_fe_ctx* c = t->c;
  HIPCHK(c, hipMemsetAsync(t->B.nEntries, 0, (size_t)t->nDb * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(t->B.poolUsed, 0, (size_t)t->nDb * 4, c->stream));
  std::fill(t->nEntries.begin(), t->nEntries.end(), 0);
  return VPL_OK;
}

static int ld_take_vocabulary(vpl_ld* t, const vpl::LdVocabRaw& raw) {
  using namespace vpl;
  vpl_fe_ctx* c = t->c;
  LdVocabFlat f;
  std::string why;
  if (!ld_flatten(raw, f, why)) return fail(c, VPL_E_INVALID, why);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // the new arrays beside the old ones, which go only when all of the new stand
  const size_t mark = c->allocs.size(), nF = f.nFlat, nW = f.nWords;
  int *cb = nullptr, *cc = nullptr, *wd = nullptr, *tb = nullptr;
  unsigned long long* ds = nullptr;
  double* ww = nullptr;
  hipError_t e = hipSuccess;
#define AL(ptr, n) if (e == hipSuccess) e = dalloc(c, &ptr, (size_t)(n), t)
  AL(cb, nF); AL(cc, nF); AL(wd, nF); AL(ds, nF * 4); AL(ww, nW); AL(tb, (size_t)t->nDb * nW);
#undef AL
  if (e == hipSuccess) e = hipMemcpy(cb, f.childBegin.data(), nF * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(cc, f.childCount.data(), nF * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(wd, f.word.data(), nF * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(ds, f.desc.data(), nF * 32, hipMemcpyHostToDevice);
  if (e == hipSuccess && nW) e = hipMemcpy(ww, f.wordWeight.data(), nW * 8, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    std::vector<void*> mine;
    for (size_t k = mark; k < c->allocs.size(); ++k) mine.push_back(c->allocs[k].p);
    for (void* q : mine) dfree(c, q);
    return fail(c, VPL_E_HIP, std::string("ld: vocabulary upload: ") + hipGetErrorString(e));
  }
  dfree(c, t->d_childBegin); dfree(c, t->d_childCount); dfree(c, t->d_word); dfree(c, t->d_desc); dfree(c, t->d_wordWeight); dfree(c, t->d_table);
  t->d_childBegin = cb; t->d_childCount = cc; t->d_word = wd; t->d_desc = ds; t->d_wordWeight = ww; t->d_table = tb;
  LdVocabDev& V = t->B.V;
  V.nFlat = f.nFlat; V.nWords = f.nWords; V.weighting = f.weighting;
  V.childBegin = cb; V.childCount = cc; V.word = wd; V.desc = ds; V.wordWeight = ww;
  t->B.table = tb;
  t->haveVocab = true;
  return ld_clear(t);   // setVocabulary clears the database
}

int vpl_ld_set_vocabulary(vpl_ld* t, int k, int L, int scoring, int weighting, int n_nodes, const int* node_id, const int* parent_id,
                          const double* weight, const unsigned long long* descriptor, int n_words, const int* word_node,
                          const int* word_id) {
  if (!t) return VPL_E_INVALID;
  vpl_fe_ctx* c = t->c;
  if (n_nodes < 0 || n_words < 0 || (n_nodes > 0 && (!node_id || !parent_id || !weight || !descriptor)) || (n_words > 0 && (!word_node || !word_id)))
    return vpl::fail(c, VPL_E_INVALID, "ld: vocabulary arrays missing");
  vpl::LdVocabRaw raw;
  raw.k = k; raw.L = L; raw.scoring = scoring; raw.weighting = weighting;
  if (n_nodes > 0) {
    raw.nodeId.assign(node_id, node_id + n_nodes); raw.parentId.assign(parent_id, parent_id + n_nodes);
    raw.weight.assign(weight, weight + n_nodes); raw.desc.assign(descriptor, descriptor + (size_t)n_nodes * 4);
  }
  if (n_words > 0) { raw.wordNode.assign(word_node, word_node + n_words); raw.wordId.assign(word_id, word_id + n_words); }
  return ld_take_vocabulary(t, raw);
}

int vpl_ld_load_vocabulary(vpl_ld* t, const char* path) {
  if (!t) return VPL_E_INVALID;
  if (!path) return vpl::fail(t->c, VPL_E_INVALID, "ld: no path");
  vpl::LdVocabRaw raw;
  std::string why;
  if (!vpl::ld_read_file(path, raw, why)) return vpl::fail(t->c, VPL_E_INVALID, why);
  return ld_take_vocabulary(t, raw);
}

int vpl_ld_reset(vpl_ld* t, int db) {
  if (!t || db < 0 || db >= t->nDb) return VPL_E_INVALID;
  vpl_fe_ctx* c = t->c;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemsetAsync(t->B.nEntries + db, 0, 4, c->stream));
  HIPCHK(c, hipMemsetAsync(t->B.poolUsed + db, 0, 4, c->stream));
  t->nEntries[db] = 0;
  return VPL_OK;
}

// the kernels of one call on B.brief / B.counts / B.frameIndex, the copy back, the one synchronisation, the refusals
static int ld_run(vpl_ld* t, const int* host_counts, int do_query, vpl_ld_result* res) {
  using namespace vpl;
  vpl_fe_ctx* c = t->c;
  hipStream_t s = c->stream;
  LdBatch& B = t->B;
  const int nDb = t->nDb, MK = B.MK;
  B.doQuery = do_query;
  { FeTimer tm(c, "k_ld_descend"); hipLaunchKernelGGL(k_ld_descend, dim3((MK + 256 / LD_LANES - 1) / (256 / LD_LANES), nDb), dim3(256), 0, s, B); }
  { FeTimer tm(c, "k_ld_bag"); hipLaunchKernelGGL(k_ld_bag, dim3(nDb), dim3(256), t->bagSmem, s, B, t->bagP); }
  int most = 0;   // (host_counts == NULL: the counts are on the device only, every database may take part)
  for (int d = 0; d < nDb; ++d)
    if (!host_counts || host_counts[d] >= 0) most = std::max(most, t->nEntries[d]);
  if (do_query && most > 0) {
    { FeTimer tm(c, "k_ld_scatter"); hipLaunchKernelGGL(k_ld_scatter, dim3((MK + 255) / 256, nDb), dim3(256), 0, s, B); }
    { FeTimer tm(c, "k_ld_score"); hipLaunchKernelGGL(k_ld_score, dim3((most + 3) / 4, nDb), dim3(256), 0, s, B); }
  } else {
    B.doQuery = 0;   // nothing stored anywhere: no table to fill or clear
  }
  { FeTimer tm(c, "k_ld_decide"); hipLaunchKernelGGL(k_ld_decide, dim3(nDb), dim3(256), 0, s, B); }
  HIPCHK(c, hipGetLastError());
  std::vector<LdOut> out(nDb);
  HIPCHK(c, hipMemcpyAsync(out.data(), B.out, (size_t)nDb * sizeof(LdOut), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  for (int d = 0; d < nDb; ++d) {
    if (out[d].flag == 1)
      return fail(c, VPL_E_CAPACITY, "ld: database " + std::to_string(d) + " holds " + std::to_string(out[d].have) + " keyframes, max_keyframes is " +
                                         std::to_string(B.maxKf));
    if (out[d].flag == 2)
      return fail(c, VPL_E_CAPACITY, "ld: database " + std::to_string(d) + ": a bag of " + std::to_string(out[d].n_words) + " words behind " +
                                         std::to_string(out[d].have) + " stored ones, max_words_total is " + std::to_string(B.pool));
  }
  for (int d = 0; d < nDb; ++d) {
    const LdOut& o = out[d];
    if (o.entry >= 0) t->nEntries[d] = o.entry + 1;
    if (!res) continue;
    vpl_ld_result& r = res[d];
    r.loop_index = o.loop_index; r.n_results = o.n_results; r.n_words = o.n_words; r.entry = o.entry;
    for (int k = 0; k < LD_MAX_RESULTS; ++k) { r.ids[k] = o.ids[k]; r.scores[k] = o.scores[k]; }
  }
  return VPL_OK;
}

static int ld_from_host(vpl_ld* t, const unsigned long long* brief, const int* counts, const int* frame_index, int do_query,
                        vpl_ld_result* res) {
  using namespace vpl;
  vpl_fe_ctx* c = t->c;
  if (!t->haveVocab) return fail(c, VPL_E_INVALID, "ld: no vocabulary (vpl_ld_set_vocabulary or vpl_ld_load_vocabulary first)");
  LdBatch& B = t->B;
  const int nDb = t->nDb, MK = B.MK;
  for (int d = 0; d < nDb; ++d)
    if (counts[d] > MK)
      return fail(c, VPL_E_CAPACITY, "ld: database " + std::to_string(d) + ": " + std::to_string(counts[d]) + " descriptors, max_keypoints is " + std::to_string(MK));
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<unsigned char> in(t->in_bytes);
  std::memcpy(in.data(), counts, (size_t)nDb * 4);
  if (frame_index) std::memcpy(in.data() + (size_t)nDb * 4, frame_index, (size_t)nDb * 4);
  for (int d = 0; d < nDb; ++d)
    if (counts[d] > 0) std::memcpy(in.data() + t->brief_off + (size_t)d * MK * 32, brief + (size_t)d * MK * 4, (size_t)counts[d] * 32);
  HIPCHK(c, hipMemcpyAsync(t->d_in, in.data(), t->in_bytes, hipMemcpyHostToDevice, c->stream));
  B.counts = (const int*)t->d_in; B.frameIndex = (const int*)(t->d_in + (size_t)nDb * 4);
  B.brief = (const unsigned long long*)(t->d_in + t->brief_off);
  return ld_run(t, counts, do_query, res);   // (synchronises: `in` may go)
}

int vpl_ld_detect(vpl_ld* t, const unsigned long long* brief, const int* counts, const int* frame_index, vpl_ld_result* res) {
  if (!t || !brief || !counts || !frame_index || !res) return VPL_E_INVALID;
  return ld_from_host(t, brief, counts, frame_index, 1, res);
}

int vpl_ld_add(vpl_ld* t, const unsigned long long* brief, const int* counts, vpl_ld_result* res) {
  if (!t || !brief || !counts) return VPL_E_INVALID;
  return ld_from_host(t, brief, counts, nullptr, 0, res);
}

int vpl_ld_detect_fe(vpl_ld* t, const int* frame_index, vpl_ld_result* res) {
  using namespace vpl;
  if (!t || !frame_index || !res) return VPL_E_INVALID;
  vpl_fe_ctx* c = t->c;
  if (!t->haveVocab) return fail(c, VPL_E_INVALID, "ld: no vocabulary (vpl_ld_set_vocabulary or vpl_ld_load_vocabulary first)");
  if (!c->lcReserved || !c->lcRowsValid) return fail(c, VPL_E_INVALID, "ld: no descriptor rows of a vpl_lc_keyframe_batch on the device");
  if (c->lcN != t->nDb)
    return fail(c, VPL_E_INVALID, "ld: the last vpl_lc_keyframe_batch took " + std::to_string(c->lcN) + " images, the session has " + std::to_string(t->nDb) + " databases");
  if (c->L.capKp != t->B.MK)
    return fail(c, VPL_E_INVALID, "ld: rows of " + std::to_string(c->L.capKp) + " keypoints (vpl_lc_reserve), the session's max_keypoints is " + std::to_string(t->B.MK));
  HIPCHK(c, hipSetDevice(c->device));
  LdBatch& B = t->B;
  const int nDb = t->nDb;
  HIPCHK(c, hipMemcpyAsync(t->d_in + (size_t)nDb * 4, frame_index, (size_t)nDb * 4, hipMemcpyHostToDevice, c->stream));
  B.counts = c->L.count; B.frameIndex = (const int*)(t->d_in + (size_t)nDb * 4); B.brief = c->L.brief;
  return ld_run(t, nullptr, 1, res);   // (synchronises before frame_index can go)
}

int vpl_ld_get_bow(vpl_ld* t, int db, int entry, int* n, int* words, double* values) {
  using namespace vpl;
  if (!t || !n || db < 0 || db >= t->nDb) return VPL_E_INVALID;
  vpl_fe_ctx* c = t->c;
  if (entry < 0 || entry >= t->nEntries[db]) return fail(c, VPL_E_INVALID, "ld: database " + std::to_string(db) + " has no entry " + std::to_string(entry));
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int off[2];
  HIPCHK(c, hipMemcpy(off, t->B.entryOff + (size_t)db * (t->B.maxKf + 1) + entry, 8, hipMemcpyDeviceToHost));
  const size_t m = off[1] - off[0], at = (size_t)db * t->B.pool + off[0];
  *n = (int)m;
  if (m && words) HIPCHK(c, hipMemcpy(words, t->B.poolWord + at, m * 4, hipMemcpyDeviceToHost));
  if (m && values) HIPCHK(c, hipMemcpy(values, t->B.poolVal + at, m * 8, hipMemcpyDeviceToHost));
  return VPL_OK;
}

int vpl_ld_size(vpl_ld* t, int db) { return (!t || db < 0 || db >= t->nDb) ? VPL_E_INVALID : t->nEntries[db]; }

}  // extern "C"
