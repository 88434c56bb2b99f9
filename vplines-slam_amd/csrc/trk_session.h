// Tracker session (vpl_trk_*, include/vplines_frontend.h): LineFeatureTracker::readImage for n_seq independent sequences, one
// call per image, with everything that survives from frame to frame in HBM.  Included once by vplines_frontend.hip, behind
// the context and the launch helpers (pre_launch, ed_launch, lm_launch, vp_launch) it calls.  The specification is the host
// mirror vplhost::LineFeatureTracker (host/vpl_frontend.hpp:227-334); DESIGN.md "Tracker session" has the layout.
//
//   image slots of the context   [0, nS) the new frames (k_pre_*, k_ed_* work there), [nS, 2 nS) the last frame of every
//                                sequence that was taken over (the matcher's reference image)
//   TrkStore st                  what curframe_ holds: kept lines, ids, t_cnt (detection order, with its own length) and the
//                                counters; `nx` is the same store written beside it by k_trk_ids, copied over `st` by
//                                k_trk_take only when the whole call is accepted
//   one frame                    H2D (raw frames + seeds) -> k_pre_* -> k_ed_* -> k_trk_pairs -> k_lm_* -> k_trk_ids -> k_vp_*
//                                -> k_trk_emit -> k_trk_take -> D2H (results, ids, observation rows) -> one synchronisation
#pragma once

namespace vpl {

#pragma clang fp contract(off)   // the end-point normalisation is the mirror's float arithmetic

// header of a sequence's store
enum { TRK_NKEPT = 0, TRK_NTCNT, TRK_ALLCNT, TRK_VPCOUNT, TRK_STARTED,
       // written by k_trk_ids beside the state (nx only): what this frame did
       TRK_EXIST, TRK_NNEW, TRK_VPRAN, TRK_NTRACKED, TRK_NVERT, TRK_HDR = 16 };
// header of a sequence's record in the read-back buffer
enum { TRK_O_FOUND = 0, TRK_O_NDET, TRK_O_NLINES, TRK_O_EXIST, TRK_O_MATCHED, TRK_O_NTRACKED, TRK_O_VPRAN, TRK_O_VPSTATUS,
       TRK_O_ALLCNT, TRK_O_VALID, TRK_O_INTS = 16 };
constexpr int TRK_LINE_F = sizeof(vpl_line) / sizeof(float);   // a vpl_line in floats (the end points come first)
static_assert(sizeof(vpl_line) == 56 && TRK_LINE_F == 14, "vpl_line layout");

struct TrkStore {
  vpl_line* kept;   // [nS][ML]
  int* ids;         // [nS][ML]
  int* tcnt;        // [nS][ML]
  int* hdr;         // [nS][TRK_HDR]
};

// bytes of one sequence's record in the read-back buffer: ints | vps[9] | ids[ML] | obs[ML][8]
__host__ __device__ inline size_t trk_rec_ids(void) { return TRK_O_INTS * 4 + 9 * 8; }
__host__ __device__ inline size_t trk_rec_obs(int ML) { return trk_rec_ids() + (((size_t)ML * 4 + 7) & ~(size_t)7); }
__host__ __device__ inline size_t trk_rec_bytes(int ML) { return trk_rec_obs(ML) + (size_t)ML * 64; }

// The matcher's input, as k_lm_take_lines builds it for the other hand-over: reference lines = the kept table of the
// sequence, current lines = the new frame's rows of the sorted table; pair i = (slot nS + i, slot i).  A sequence without
// kept lines enters with an empty reference list, which k_lm_anchors answers with valid = 0 and no key point.
__global__ __launch_bounds__(256) void k_trk_pairs(TrkStore st, const vpl_line* sorted, const int* sortedCnt, int ML, int nS,
                                                   int* refImg, int* curImg, vpl_line* linesRef, vpl_line* linesCur, int* nRef,
                                                   int* nCur) {
  const int i = blockIdx.x, side = blockIdx.y;
  const int m = min(side ? sortedCnt[i] : st.hdr[i * TRK_HDR + TRK_NKEPT], ML);
  if (threadIdx.x == 0) {
    if (side) { nCur[i] = m; curImg[i] = i; } else { nRef[i] = m; refImg[i] = nS + i; }
  }
  vpl_line* dst = (side ? linesCur : linesRef) + (size_t)i * ML;
  const vpl_line* src = (side ? sorted : st.kept) + (size_t)i * ML;
  for (int k = threadIdx.x; k < m; k += blockDim.x) dst[k] = src[k];
}

struct TrkIds {
  int ML, maxH, maxV;
  // the new frame's detections: end points at ends[(s * ML + i) * endStride]
  const float* ends; int endStride;
  const int* nNew;        // [nS]
  // the match against the previous frame's kept lines
  const int* nPrev;       // [nS]
  const int* valid;       // [nS] Matching()'s return value (NULL: true)
  const int* p2n;         // [nS][ML]
  TrkStore st, nx;        // st.kept / nx.kept may be NULL (debug entry: no line records)
  int* keep;              // [nS][ML] kept lines as indices into the detections
  int* vert;              // [nS][ML] verticalLine as indices into the detections
  // session only (NULL otherwise): the line records and the VP stage's inputs
  const vpl_line* sorted;
  float *hypEnds, *allEnds;   // [nS][ML][4]
  int *nHyp, *nAll, *first;   // [nS]
  const uint32_t* seedIn; uint32_t* seed;
};

// the "h" class of line_feature_tracker.cpp:166 / :185 as vpl_line_track_ids computes it: segAngle in float (atan2f of
// float differences), compared in double with the 3.14-based borders
__device__ inline bool trk_h_class(const float* e) {
  const double a = (double)vp_seg_angle(e);
  return (a >= 3.14 / 4.0 && a <= 3 * 3.14 / 4.0) || (a <= -3.14 / 4.0 && a >= -3 * 3.14 / 4.0);
}

// The id / t_cnt / quota step of readImage (:96-229) for one sequence per work-group, vpl_line_track_ids as written plus the
// two cases the mirror handles around it (first image: all lines, fresh ids; nothing kept so far: all lines, ids -1).
// Dynamic LDS: 2 * ML ints.  Frames with more lines than threads are looped over; the three stable compactions are ranks
// counted over the class array in LDS (<= 1024 lines: cheaper than a scan's barriers).
__global__ __launch_bounds__(256) void k_trk_ids(TrkIds A) {
  extern __shared__ int trk_sm[];
  __shared__ int cnt[5];   // tracked, fresh h, fresh v, tracked of the h class, tracked of the v class
  const int s = blockIdx.x, tid = threadIdx.x, ML = A.ML;
  int* sid = trk_sm;
  int* scat = trk_sm + ML;
  const int* hdr = A.st.hdr + s * TRK_HDR;
  const int nNew = min(A.nNew[s], ML);
  const int allcnt = hdr[TRK_ALLCNT], vpCount = hdr[TRK_VPCOUNT], nTcntPrev = min(hdr[TRK_NTCNT], ML);
  // 0: the sequence's first image | 1: curframe_ holds no line (ids stay -1) | 2: match, ids, quota
  const int mode = !hdr[TRK_STARTED] ? 0 : hdr[TRK_NKEPT] == 0 ? 1 : 2;
  const float* ends = A.ends + (size_t)s * ML * A.endStride;
  const int* idPrev = A.st.ids + (size_t)s * ML;
  const int* tcPrev = A.st.tcnt + (size_t)s * ML;
  int* idOut = A.nx.ids + (size_t)s * ML;
  int* tcOut = A.nx.tcnt + (size_t)s * ML;
  int* keep = A.keep + (size_t)s * ML;
  int* vert = A.vert + (size_t)s * ML;

  if (tid < 5) cnt[tid] = 0;
  for (int i = tid; i < nNew; i += blockDim.x) sid[i] = -1;
  __syncthreads();
  if (mode == 2 && (!A.valid || A.valid[s] == 1)) {
    // two previous lines on one detection: the later one wins = the largest k
    const int nPrev = min(A.nPrev[s], ML);
    const int* p2n = A.p2n + (size_t)s * ML;
    for (int k = tid; k < nPrev; k += blockDim.x) {
      const int mt = p2n[k];
      if (mt > 0 && mt < nNew) atomicMax(&sid[mt], k);
    }
  }
  __syncthreads();
  for (int i = tid; i < nNew; i += blockDim.x) {
    const int w = sid[i];
    int id = -1, tc = 0, cat = 0;
    if (mode == 0) id = allcnt + i;
    if (mode == 2) {
      if (w >= 0) { id = idPrev[w]; tc = (i < nTcntPrev ? tcPrev[i] : 0) + 1; }
      const bool h = trk_h_class(ends + (size_t)i * A.endStride);
      if (id == -1) cat = h ? 1 : 2; else atomicAdd(&cnt[h ? 3 : 4], 1);
    }
    atomicAdd(&cnt[cat], 1);
    tcOut[i] = tc;
    sid[i] = id;
    scat[i] = cat;
  }
  __syncthreads();
  const int nT = cnt[0], nFH = cnt[1], nFV = cnt[2];
  const int takeH = mode == 2 ? min(max(A.maxH - cnt[3], 0), nFH) : 0;
  const int takeV = mode == 2 ? min(max(A.maxV - cnt[4], 0), nFV) : 0;
  const int nKeep = nT + takeH + takeV;
  const bool vpRun = mode == 2 && nKeep > 2;
  const bool hypVert = nFV > 2;
  float* hyp = A.hypEnds ? A.hypEnds + (size_t)s * ML * 4 : nullptr;
  float* all = A.allEnds ? A.allEnds + (size_t)s * ML * 4 : nullptr;
  for (int i = tid; i < nNew; i += blockDim.x) {
    int c0 = 0, c1 = 0, c2 = 0;
    for (int j = 0; j < i; ++j) { const int c = scat[j]; c0 += c == 0; c1 += c == 1; c2 += c == 2; }
    const int cat = scat[i];
    const float* e = ends + (size_t)i * A.endStride;
    int id = sid[i], pos = -1;
    if (cat == 0) pos = c0;
    else {
      id = allcnt + c1 + c2;                       // fresh ids in detection order
      if (cat == 1) { if (c1 < takeH) pos = nT + c1; }
      else {
        vert[c2] = i;
        if (c2 < takeV) pos = nT + takeH + c2;
        if (hyp && hypVert) for (int q = 0; q < 4; ++q) hyp[4 * c2 + q] = e[q];
      }
    }
    if (pos >= 0) {
      keep[pos] = i;
      idOut[pos] = id;
      if (A.sorted) A.nx.kept[(size_t)s * ML + pos] = A.sorted[(size_t)s * ML + i];
      if (all) for (int q = 0; q < 4; ++q) all[4 * pos + q] = e[q];
      if (hyp && !hypVert) for (int q = 0; q < 4; ++q) hyp[4 * pos + q] = e[q];
    }
  }
  if (tid == 0) {
    int* o = A.nx.hdr + s * TRK_HDR;
    o[TRK_NKEPT] = nKeep;
    o[TRK_NTCNT] = nNew;
    o[TRK_ALLCNT] = allcnt + (mode == 0 ? nNew : nFH + nFV);
    o[TRK_VPCOUNT] = vpCount + (vpRun ? 1 : 0);
    o[TRK_STARTED] = 1;
    o[TRK_EXIST] = nNew > 0;
    o[TRK_NNEW] = nNew;
    o[TRK_VPRAN] = vpRun;
    o[TRK_NTRACKED] = mode == 2 ? nT : 0;
    o[TRK_NVERT] = nFV;
    if (A.nHyp) {   // a sequence whose VP stage must not run enters it without lines: status -1, nothing classified
      A.nHyp[s] = vpRun ? (hypVert ? nFV : nKeep) : 0;
      A.nAll[s] = vpRun ? nKeep : 0;
      A.first[s] = vpCount == 0;
      A.seed[s] = A.seedIn[s];
    }
  }
}

struct TrkEmit {
  int nS, ML;
  float fx, fy, cx, cy;
  const int* found;       // [nS] lines the detector found (may exceed ML)
  const int* valid;       // [nS] of the matcher: -1 = more key points than max_kps
  const int* nRef;        // [nS]
  const int* r2c;         // [nS][ML]
  const int *vpStatus, *vpIds; const double* vps;
  TrkStore st, nx;
  char* out;              // [nS] records (trk_rec_bytes)
  int* take;              // [nS] this sequence's new state replaces the old
  int *dbgMatch, *dbgVp;  // [nS][ML] test access
};

// Results, ids and observation rows of one sequence into the read-back buffer, and the decision whether the call is
// accepted: a frame with more lines than the table holds, or a pair with more key points than max_kps, refuses the whole
// call, and then nothing is taken over.
__global__ __launch_bounds__(256) void k_trk_emit(TrkEmit E) {
  __shared__ int bad;
  const int s = blockIdx.x, tid = threadIdx.x, ML = E.ML;
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int q = tid; q < E.nS; q += blockDim.x)
    if (E.found[q] > ML || E.valid[q] < 0) atomicOr(&bad, 1);
  __syncthreads();
  const bool ok = !bad;
  const int* hn = E.nx.hdr + s * TRK_HDR;
  const int nKeep = hn[TRK_NKEPT], exist = hn[TRK_EXIST], vpRan = hn[TRK_VPRAN];
  char* rec = E.out + (size_t)s * trk_rec_bytes(ML);
  int* oi = (int*)rec;
  double* ov = (double*)(rec + TRK_O_INTS * 4);
  int* oid = (int*)(rec + trk_rec_ids());
  double* obs = (double*)(rec + trk_rec_obs(ML));
  const int status = vpRan ? E.vpStatus[s] : 0;
  if (tid == 0) {
    oi[TRK_O_FOUND] = E.found[s];
    oi[TRK_O_NDET] = hn[TRK_NNEW];
    oi[TRK_O_NLINES] = exist ? nKeep : 0;
    oi[TRK_O_EXIST] = exist;
    oi[TRK_O_MATCHED] = E.valid[s] == 1;
    oi[TRK_O_NTRACKED] = hn[TRK_NTRACKED];
    oi[TRK_O_VPRAN] = vpRan;
    oi[TRK_O_VPSTATUS] = status;
    oi[TRK_O_ALLCNT] = ok && exist ? hn[TRK_ALLCNT] : E.st.hdr[s * TRK_HDR + TRK_ALLCNT];
    oi[TRK_O_VALID] = E.valid[s];
    E.take[s] = ok && exist;
    if (ok && !exist) E.st.hdr[s * TRK_HDR + TRK_STARTED] = 1;   // the mirror's forwframe_ exists from the first call on
  }
  if (tid < 9) ov[tid] = vpRan ? E.vps[s * 9 + tid] : 0.0;
  // the VP part every row carries: the entry of kept line 0 (line_feature_tracker_node.cpp:104-109)
  double vp4[4] = {0.0, 0.0, 0.0, 0.0};
  if (vpRan && nKeep > 0) {
    const int id0 = status == 0 ? E.vpIds[(size_t)s * ML] : 3;
    if (id0 != 3) {
      const double* v = E.vps + s * 9 + 3 * id0;
      vp4[0] = v[0]; vp4[1] = v[1]; vp4[2] = v[2]; vp4[3] = v[2] / v[2];
    }
  }
  const vpl_line* K = E.nx.kept + (size_t)s * ML;
  const int* ids = E.nx.ids + (size_t)s * ML;
  for (int j = tid; j < (exist ? nKeep : 0); j += blockDim.x) {
    const float* e = K[j].line_endpoint;
    double* o = obs + (size_t)j * 8;
    o[0] = (double)((e[0] - E.cx) / E.fx);
    o[1] = (double)((e[1] - E.cy) / E.fy);
    o[2] = (double)((e[2] - E.cx) / E.fx);
    o[3] = (double)((e[3] - E.cy) / E.fy);
    for (int q = 0; q < 4; ++q) o[4 + q] = vp4[q];
    oid[j] = ids[j];
  }
  if (ok) {
    const int nm = E.valid[s] == 1 ? min(E.nRef[s], ML) : 0;
    for (int k = tid; k < ML; k += blockDim.x) {
      E.dbgMatch[(size_t)s * ML + k] = k < nm ? E.r2c[(size_t)s * ML + k] : -1;
      E.dbgVp[(size_t)s * ML + k] = vpRan && k < nKeep && status == 0 ? E.vpIds[(size_t)s * ML + k] : 3;
    }
  }
}

// The accepted sequences' new state over the old: the prepared frame from slot s to slot nS + s (16 bytes per lane per trip
// where the frame size allows, bytes otherwise), and by the first work-group of a sequence the tables and the header.
__global__ __launch_bounds__(256) void k_trk_take(TrkStore st, TrkStore nx, const int* take, uint8_t* img, size_t PX, int nS, int ML) {
  const int s = blockIdx.y;
  if (!take[s]) return;
  const uint8_t* src = img + (size_t)s * PX;
  uint8_t* dst = img + ((size_t)nS + s) * PX;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, T = (size_t)gridDim.x * blockDim.x;
  if (PX % 16 == 0) {
    for (size_t i = t; i < PX / 16; i += T) ((uint4*)dst)[i] = ((const uint4*)src)[i];
  } else {
    for (size_t i = t; i < PX; i += T) dst[i] = src[i];
  }
  if (blockIdx.x != 0) return;
  const int* hn = nx.hdr + s * TRK_HDR;
  const int nKeep = min(hn[TRK_NKEPT], ML), nTc = min(hn[TRK_NTCNT], ML);
  for (int k = threadIdx.x; k < nKeep; k += blockDim.x) {
    st.kept[(size_t)s * ML + k] = nx.kept[(size_t)s * ML + k];
    st.ids[(size_t)s * ML + k] = nx.ids[(size_t)s * ML + k];
  }
  for (int k = threadIdx.x; k < nTc; k += blockDim.x) st.tcnt[(size_t)s * ML + k] = nx.tcnt[(size_t)s * ML + k];
  if (threadIdx.x <= TRK_STARTED) st.hdr[s * TRK_HDR + threadIdx.x] = hn[threadIdx.x];
}

}  // namespace vpl

struct vpl_trk {
  vpl_fe_ctx* c = nullptr;
  int nS = 0;
  vpl_trk_options opt;
  TrkStore st, nx;
  int *d_keep = nullptr, *d_vert = nullptr, *d_take = nullptr, *d_dbgMatch = nullptr, *d_dbgVp = nullptr;
  char *d_in = nullptr, *d_out = nullptr;   // raw frames | seeds;  the records
  char *h_in = nullptr, *h_out = nullptr;   // pinned
  size_t in_bytes = 0, out_bytes = 0, seed_off = 0;
};

// (every device array of the session is recorded in the context with the session as its owner: vpl_trk_destroy)
static int trk_alloc_store(vpl_trk* t, TrkStore& S, size_t nS, size_t ML) {
  vpl_fe_ctx* c = t->c;
  HIPCHK(c, dalloc(c, &S.kept, nS * ML, t));
  HIPCHK(c, dalloc(c, &S.ids, nS * ML, t));
  HIPCHK(c, dalloc(c, &S.tcnt, nS * ML, t));
  HIPCHK(c, dalloc(c, &S.hdr, nS * TRK_HDR, t));
  return VPL_OK;
}

static int trk_alloc(vpl_trk* t) {
  vpl_fe_ctx* c = t->c;
  const size_t nS = t->nS, ML = c->maxLines;
  int rc = trk_alloc_store(t, t->st, nS, ML);
  if (rc) return rc;
  rc = trk_alloc_store(t, t->nx, nS, ML);
  if (rc) return rc;
  HIPCHK(c, dalloc(c, &t->d_keep, nS * ML, t));
  HIPCHK(c, dalloc(c, &t->d_vert, nS * ML, t));
  HIPCHK(c, dalloc(c, &t->d_take, nS, t));
  HIPCHK(c, dalloc(c, &t->d_dbgMatch, nS * ML, t));
  HIPCHK(c, dalloc(c, &t->d_dbgVp, nS * ML, t));
  HIPCHK(c, dalloc(c, &t->d_in, t->in_bytes, t));
  HIPCHK(c, dalloc(c, &t->d_out, t->out_bytes, t));
  HIPCHK(c, hipHostMalloc((void**)&t->h_in, t->in_bytes, hipHostMallocDefault));
  HIPCHK(c, hipHostMalloc((void**)&t->h_out, t->out_bytes, hipHostMallocDefault));
  return VPL_OK;
}

extern "C" {

void vpl_trk_default_options(vpl_trk_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  vpl_edline_default_param(&o->ed);
  vpl_match_default_param(&o->match);
  o->max_h_lines = 25; o->max_v_lines = 25;             // config/euroc/euroc_config.yaml:85-86
  o->equalize = 1; o->clip_limit = 3.0; o->tiles_x = 8; o->tiles_y = 8;
  o->fx = 1.f; o->fy = 1.f; o->cx = 0.f; o->cy = 0.f;
}

int vpl_trk_create(vpl_trk** out, vpl_fe_ctx* c, int n_seq, const vpl_trk_options* opt) {
  if (!out || !c || !opt || n_seq < 1) return VPL_E_INVALID;
  if (c->trk) return fail(c, VPL_E_INVALID, "trk: the context already lends itself to a session");
  if (opt->max_h_lines < 0 || opt->max_v_lines < 0 || !(opt->fx != 0.f) || !(opt->fy != 0.f) || opt->ed.scanIntervals < 1 ||
      opt->ed.minLineLen < 2 || opt->match.step < 1 ||
      (opt->equalize && (opt->tiles_x < 1 || opt->tiles_y < 1 || opt->tiles_x > c->W || opt->tiles_y > c->H)))
    return fail(c, VPL_E_INVALID, "trk: bad options");
  if (c->maxN / 2 < n_seq) return fail(c, VPL_E_CAPACITY, "trk: the context needs max_images >= 2 * n_seq");
  if (!c->lmReserved || c->maxPairs < n_seq) return fail(c, VPL_E_CAPACITY, "trk: vpl_match_reserve for at least n_seq pairs first");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int rc = vp_reserve(c);
  if (!rc) rc = pre_reserve(c);
  if (rc) return rc;
  vpl_trk* t = new vpl_trk();
  t->c = c; t->nS = n_seq; t->opt = *opt;
  std::memset(&t->st, 0, sizeof(t->st));
  std::memset(&t->nx, 0, sizeof(t->nx));
  const size_t PX = (size_t)c->W * c->H;
  t->seed_off = ((size_t)n_seq * PX + 15) & ~(size_t)15;
  t->in_bytes = t->seed_off + (size_t)n_seq * 4;
  t->out_bytes = (size_t)n_seq * trk_rec_bytes(c->maxLines);
  rc = trk_alloc(t);
  c->trk = t;
  if (rc) { vpl_trk_destroy(t); return rc; }
  *out = t;
  return VPL_OK;
}

void vpl_trk_destroy(vpl_trk* t) {
  if (!t) return;
  vpl_fe_ctx* c = t->c;
  // (teardown: a failure has nobody to be reported to)
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  dfree_owner(c, t);   // (what the context allocated for itself while the session was open -- d_blur, a grown d_lut -- stays)
  if (t->h_in) (void)hipHostFree(t->h_in);
  if (t->h_out) (void)hipHostFree(t->h_out);
  if (c->trk == t) c->trk = nullptr;
  delete t;
}

int vpl_trk_reset(vpl_trk* t, int seq) {
  if (!t || seq < 0 || seq >= t->nS) return VPL_E_INVALID;
  vpl_fe_ctx* c = t->c;
  HIPCHK(c, hipSetDevice(c->device));
  int* h = t->st.hdr + (size_t)seq * TRK_HDR;
  // everything but allfeature_cnt: no kept line, no t_cnt, the VP counter at 0, the next image is a first image
  HIPCHK(c, hipMemsetAsync(h + TRK_NKEPT, 0, 2 * sizeof(int), c->stream));
  HIPCHK(c, hipMemsetAsync(h + TRK_VPCOUNT, 0, 2 * sizeof(int), c->stream));
  return VPL_OK;
}

int vpl_trk_frame(vpl_trk* t, const uint8_t* raw, const uint32_t* vp_seed, vpl_trk_result* res, int* line_id, double* line_obs) {
  if (!t || !raw || !vp_seed || !res || !line_id || !line_obs) return VPL_E_INVALID;
  vpl_fe_ctx* c = t->c;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int nS = t->nS, ML = c->maxLines;
  const size_t PX = (size_t)c->W * c->H;
  const vpl_trk_options& o = t->opt;
  // down: the raw frames and the seeds, one copy
  std::memcpy(t->h_in, raw, (size_t)nS * PX);
  std::memcpy(t->h_in + t->seed_off, vp_seed, (size_t)nS * 4);
  HIPCHK(c, hipMemcpyAsync(t->d_in, t->h_in, t->in_bytes, hipMemcpyHostToDevice, s));
  c->n = 2 * nS; c->B.N = 2 * nS; c->nPairs = nS; c->vpN = nS; c->matchFromDetected = false;
  int rc = pre_launch(c, nS, (const uint8_t*)t->d_in, o.equalize, o.clip_limit, o.tiles_x, o.tiles_y);
  if (!rc) rc = ed_launch(c, &o.ed, 1, nS);
  if (rc) return rc;
  hipLaunchKernelGGL(k_trk_pairs, dim3(nS, 2), dim3(256), 0, s, t->st, c->d_sorted, c->d_sortedCnt, ML, nS, c->d_refImg, c->d_curImg,
                     c->d_linesRef, c->d_linesCur, c->d_nRef, c->d_nCur);
  rc = lm_launch(c, &o.match, 2 * nS, nS);
  if (rc) return rc;
  TrkIds A;
  std::memset(&A, 0, sizeof(A));
  A.ML = ML; A.maxH = o.max_h_lines; A.maxV = o.max_v_lines;
  A.ends = (const float*)c->d_sorted; A.endStride = TRK_LINE_F;
  A.nNew = c->d_sortedCnt; A.nPrev = c->d_nRef; A.valid = c->M.valid; A.p2n = c->M.r2c;
  A.st = t->st; A.nx = t->nx; A.keep = t->d_keep; A.vert = t->d_vert;
  A.sorted = c->d_sorted; A.hypEnds = c->d_vpHyp; A.allEnds = c->d_vpAll;
  A.nHyp = c->d_vpNHyp; A.nAll = c->d_vpNAll; A.first = c->d_vpFirst;
  A.seedIn = (const uint32_t*)(t->d_in + t->seed_off); A.seed = c->d_vpSeed;
  hipLaunchKernelGGL(k_trk_ids, dim3(nS), dim3(256), (size_t)ML * 8, s, A);
  rc = vp_launch(c, nS, o.fx, o.cx, o.cy);
  if (rc) return rc;
  TrkEmit E;
  std::memset(&E, 0, sizeof(E));
  E.nS = nS; E.ML = ML; E.fx = o.fx; E.fy = o.fy; E.cx = o.cx; E.cy = o.cy;
  E.found = c->B.nLines; E.valid = c->M.valid; E.nRef = c->d_nRef; E.r2c = c->M.r2c;
  E.vpStatus = c->V.status; E.vpIds = c->V.ids; E.vps = c->V.vps;
  E.st = t->st; E.nx = t->nx; E.out = t->d_out; E.take = t->d_take; E.dbgMatch = t->d_dbgMatch; E.dbgVp = t->d_dbgVp;
  hipLaunchKernelGGL(k_trk_emit, dim3(nS), dim3(256), 0, s, E);
  hipLaunchKernelGGL(k_trk_take, dim3(16, nS), dim3(256), 0, s, t->st, t->nx, t->d_take, (uint8_t*)c->B.img, PX, nS, ML);
  HIPCHK(c, hipGetLastError());
  // up: one copy, one synchronisation
  HIPCHK(c, hipMemcpyAsync(t->h_out, t->d_out, t->out_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  const size_t RB = trk_rec_bytes(ML);
  for (int q = 0; q < nS; ++q) {
    const int* oi = (const int*)(t->h_out + q * RB);
    if (oi[TRK_O_FOUND] > ML)
      return fail(c, VPL_E_CAPACITY, "trk: sequence " + std::to_string(q) + ": " + std::to_string(oi[TRK_O_FOUND]) +
                                         " lines found, max_lines_per_image is " + std::to_string(ML));
    if (oi[TRK_O_VALID] < 0) return fail(c, VPL_E_CAPACITY, "trk: sequence " + std::to_string(q) + ": more key points than max_kps");
  }
  for (int q = 0; q < nS; ++q) {
    const char* rec = t->h_out + q * RB;
    const int* oi = (const int*)rec;
    vpl_trk_result& r = res[q];
    r.n_detected = oi[TRK_O_NDET]; r.n_lines = oi[TRK_O_NLINES]; r.lines_exist = oi[TRK_O_EXIST];
    r.matched = oi[TRK_O_MATCHED]; r.n_tracked = oi[TRK_O_NTRACKED]; r.vp_ran = oi[TRK_O_VPRAN]; r.vp_status = oi[TRK_O_VPSTATUS];
    std::memcpy(r.vps, rec + TRK_O_INTS * 4, 72);
    r.allfeature_cnt = oi[TRK_O_ALLCNT];
    std::memcpy(line_id + (size_t)q * ML, rec + trk_rec_ids(), (size_t)r.n_lines * 4);
    std::memcpy(line_obs + (size_t)q * ML * 8, rec + trk_rec_obs(ML), (size_t)r.n_lines * 64);
  }
  return VPL_OK;
}

int vpl_trk_get_frame(vpl_trk* t, int seq, uint8_t* img, vpl_line* lines, int* ids, int* t_cnt, int* n_tcnt, int* match, int* vp_ids) {
  if (!t || seq < 0 || seq >= t->nS) return VPL_E_INVALID;
  vpl_fe_ctx* c = t->c;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t ML = c->maxLines, PX = (size_t)c->W * c->H, o = (size_t)seq * ML;
  if (img) HIPCHK(c, hipMemcpy(img, c->B.img + ((size_t)t->nS + seq) * PX, PX, hipMemcpyDeviceToHost));
  if (lines) HIPCHK(c, hipMemcpy(lines, t->st.kept + o, ML * sizeof(vpl_line), hipMemcpyDeviceToHost));
  if (ids) HIPCHK(c, hipMemcpy(ids, t->st.ids + o, ML * 4, hipMemcpyDeviceToHost));
  if (t_cnt) HIPCHK(c, hipMemcpy(t_cnt, t->st.tcnt + o, ML * 4, hipMemcpyDeviceToHost));
  if (n_tcnt) HIPCHK(c, hipMemcpy(n_tcnt, t->st.hdr + (size_t)seq * TRK_HDR + TRK_NTCNT, 4, hipMemcpyDeviceToHost));
  if (match) HIPCHK(c, hipMemcpy(match, t->d_dbgMatch + o, ML * 4, hipMemcpyDeviceToHost));
  if (vp_ids) HIPCHK(c, hipMemcpy(vp_ids, t->d_dbgVp + o, ML * 4, hipMemcpyDeviceToHost));
  return VPL_OK;
}

// Test access: k_trk_ids alone on the arguments of vpl_line_track_ids (one sequence that has kept lines, so that the
// match / quota path runs whatever n_prev is).  Synchronous; the buffers are the call's own.
int vpl_trk_debug_ids(vpl_fe_ctx* c, int n_new, const float* ends, int n_prev, const int* id_prev, const int* tcnt_prev, int n_tcnt_prev,
                      const int* prev_to_new, int max_h, int max_v, int* allfeature_cnt, int* keep, int* id_out, int* tcnt_out,
                      int* vertical_new, int* n_vertical_new) {
  if (!c || n_new < 0 || n_prev < 0 || n_tcnt_prev < 0 || !allfeature_cnt || (n_new && (!ends || !keep || !id_out || !tcnt_out)) ||
      (n_prev && (!id_prev || !prev_to_new)) || (n_tcnt_prev && !tcnt_prev))
    return VPL_E_INVALID;
  const int ML = std::max(std::max(n_new, n_prev), std::max(n_tcnt_prev, 1));
  if (ML > 4096) return fail(c, VPL_E_CAPACITY, "trk_debug_ids: more than 4096 entries");
  HIPCHK(c, hipSetDevice(c->device));
  // ends [ML][4] floats | ints: nNew, nPrev, p2n[ML], st.ids[ML], st.tcnt[ML], st.hdr, nx.ids[ML], nx.tcnt[ML], nx.hdr, keep[ML], vert[ML]
  const size_t nInts = 2 + 7 * (size_t)ML + 2 * TRK_HDR, bytes = (size_t)ML * 16 + nInts * 4;
  std::vector<char> h(bytes, 0);
  float* he = (float*)h.data();
  int* hi = (int*)(h.data() + (size_t)ML * 16);
  if (n_new) std::memcpy(he, ends, (size_t)n_new * 16);
  int *hp2n = hi + 2, *hids = hp2n + ML, *htc = hids + ML, *hhdr = htc + ML;
  hi[0] = n_new; hi[1] = n_prev;
  if (n_prev) { std::memcpy(hp2n, prev_to_new, (size_t)n_prev * 4); std::memcpy(hids, id_prev, (size_t)n_prev * 4); }
  if (n_tcnt_prev) std::memcpy(htc, tcnt_prev, (size_t)n_tcnt_prev * 4);
  hhdr[TRK_NKEPT] = 1; hhdr[TRK_NTCNT] = n_tcnt_prev; hhdr[TRK_ALLCNT] = *allfeature_cnt; hhdr[TRK_STARTED] = 1;
  char* d = nullptr;
  HIPCHK(c, hipMalloc((void**)&d, bytes));
  hipError_t e = hipMemcpyAsync(d, h.data(), bytes, hipMemcpyHostToDevice, c->stream);
  float* de = (float*)d;
  int* di = (int*)(d + (size_t)ML * 16);
  TrkIds A;
  std::memset(&A, 0, sizeof(A));
  A.ML = ML; A.maxH = max_h; A.maxV = max_v; A.ends = de; A.endStride = 4;
  A.nNew = di; A.nPrev = di + 1; A.p2n = di + 2;
  A.st.ids = di + 2 + ML; A.st.tcnt = A.st.ids + ML; A.st.hdr = A.st.tcnt + ML;
  A.nx.ids = A.st.hdr + TRK_HDR; A.nx.tcnt = A.nx.ids + ML; A.nx.hdr = A.nx.tcnt + ML;
  A.keep = A.nx.hdr + TRK_HDR; A.vert = A.keep + ML;
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_trk_ids, dim3(1), dim3(256), (size_t)ML * 8, c->stream, A);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d, bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  HIPCHK(c, e);
  const int *oids = hhdr + TRK_HDR, *otc = oids + ML, *ohdr = otc + ML, *okeep = ohdr + TRK_HDR, *overt = okeep + ML;
  const int n_keep = ohdr[TRK_NKEPT];
  if (n_keep) { std::memcpy(keep, okeep, (size_t)n_keep * 4); std::memcpy(id_out, oids, (size_t)n_keep * 4); }
  if (n_new) std::memcpy(tcnt_out, otc, (size_t)n_new * 4);
  *allfeature_cnt = ohdr[TRK_ALLCNT];
  if (vertical_new && n_vertical_new) {
    if (ohdr[TRK_NVERT]) std::memcpy(vertical_new, overt, (size_t)ohdr[TRK_NVERT] * 4);
    *n_vertical_new = ohdr[TRK_NVERT];
  }
  return n_keep;
}

}  // extern "C"
