// Point tracker session (vpl_ptrk_*): FeatureTracker::readImage (feature_tracker/src/feature_tracker.cpp:107-224) and updateID
// (:263-273) for n_seq independent cameras, one call per image, the tracker's lists resident in HBM.  Included once by
// vplines_frontend.hip, behind the stage calls it composes: pre_launch (CLAHE), lm_pyr_launch<PT_WIN> + k_pt_flow,
// k_pt_reject_f, pt_detect_launch.  The list handling between them is four small kernels, one work-group per sequence:
//   k_ptrk_begin   the flow stage's counts from the state
//   k_ptrk_track   status &= inBorder (cvRound, border 1), stable compaction, track_cnt++                       (:141-173)
//   k_ptrk_mask    compaction by rejectWithF's status; setMask (:37-82): order by falling track_cnt -- STABLY, the earlier list
//                  position first, where the reference's std::sort leaves equal counts in whatever order libstdc++ does --
//                  then point after point: kept when its mask pixel is 255, and then a filled circle of radius min_dist
//                  (pt_circle_half_widths) is cleared around it; the detector's parameters (max_cnt - kept corners under that mask)
//   k_ptrk_finish  addPoints (id -1, track_cnt 1); undistortedPoints (:317-371): un-points, score / max score, velocity against
//                  the previous image's (id, un-point) list; updateID in list order; the published rows; the new state beside the old
//   k_ptrk_take    when no sequence of the call overflowed: new state over old, the prepared frame into the previous-image slot
// A frame travels as: one upload (times, seeds, publish flags, raw frames), one download (flags, results, rows), one
// synchronisation.  Image slots [0, n_seq) hold the new frames, [n_seq, 2 n_seq) the previous ones.
#pragma once

namespace vpl {

constexpr int PTRK_HDR = 4;      // per sequence: points, entries of the previous (id, un-point) list, next id, -
constexpr int PTRK_RES = 8;      // per sequence in the download: tracked, after border, after F, after mask, detected, published, rows, -
constexpr int PTRK_ROW = 7;      // x, y (undistorted), u, v, vx, vy, prob

struct PtrkStore {   // rows of MP entries per sequence
  int* hdr;          // [nS][PTRK_HDR]
  double* time;      // [nS] prev_time
  float* pts;        // [nS][MP][2] cur_pts
  int* ids;          // [nS][MP]
  int* cnt;          // [nS][MP] track_cnt
  float* sc;         // [nS][MP] forw_scores
  float* un;         // [nS][MP][2] cur_un_pts
  float* usc;        // [nS][MP] forw_un_scores
  int* mapId;        // [nS][MP] ids as undistortedPoints saw them (before updateID): the keys of prev_un_pts_map
};

struct PtrkBatch {
  int nS, MP, W, H;
  int maxCnt, minDist;
  PtrkStore st, nx;
  // the call's inputs
  const double* time;           // [nS]
  const int* publish;           // [nS]
  // flow stage
  int* flowCnt;                 // [nS]
  const float* flowNext;        // [nS][MP][2]
  const uint8_t* flowStatus;    // [nS][MP]
  // after the border test: rejectWithF's input
  float *wcur, *wforw;          // [nS][MP][2]
  int *wid, *wcnt;              // [nS][MP]
  float* wsc;
  int* rejCnt;                  // [nS]
  const uint8_t* rejStatus;     // [nS][MP]
  // after setMask
  float* kpts;                  // [nS][MP][2]
  int *kid, *kcnt;
  float* ksc;
  int* kn;                      // [nS]
  uint8_t* mask;                // [nS][H][W]
  const uint8_t* fisheye;       // null or [H][W]
  const int* circle;            // [2 minDist + 1] half-widths
  // detector
  int* detMaxCorners;           // [nS]
  int* detUseMask;              // [nS] = 1
  double* detMinDist;           // [nS]
  const float* detCorners;      // [nS][capCorners][2]
  const float* detScores;
  const int* detCount;
  int capCorners;
  PtCamera cam;
  // download
  int* flags;                   // [nS] 1: the detector's candidate list overflowed
  int* res;                     // [nS][PTRK_RES]
  int* rowId;                   // [nS][MP]
  double* rows;                 // [nS][MP][PTRK_ROW]
};

__global__ void k_ptrk_begin(PtrkBatch B) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < B.nS) B.flowCnt[s] = B.st.hdr[s * PTRK_HDR];
}

// the place of entry i among the entries with keep != 0, in list order; n <= MP entries, flags in LDS
__device__ inline int ptrk_rank(const int* keep, int i) {
  int r = 0;
  for (int j = 0; j < i; ++j) r += keep[j] ? 1 : 0;
  return r;
}

__global__ __launch_bounds__(256) void k_ptrk_track(PtrkBatch B) {
  extern __shared__ int ptrk_lds[];
  int* keep = ptrk_lds;
  __shared__ int total[2];
  const int s = blockIdx.x, tid = threadIdx.x, MP = B.MP;
  const int n = B.st.hdr[s * PTRK_HDR];
  const size_t o = (size_t)s * MP;
  if (tid == 0) total[0] = total[1] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const bool st = B.flowStatus[o + i] != 0;
    const int x = __float2int_rn(B.flowNext[2 * (o + i)]), y = __float2int_rn(B.flowNext[2 * (o + i) + 1]);   // inBorder :5-11
    const bool in = 1 <= x && x < B.W - 1 && 1 <= y && y < B.H - 1;
    keep[i] = st && in;
    if (st) atomicAdd(&total[0], 1);
    if (st && in) atomicAdd(&total[1], 1);
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    if (!keep[i]) continue;
    const size_t d = o + ptrk_rank(keep, i);
    B.wcur[2 * d] = B.st.pts[2 * (o + i)]; B.wcur[2 * d + 1] = B.st.pts[2 * (o + i) + 1];
    B.wforw[2 * d] = B.flowNext[2 * (o + i)]; B.wforw[2 * d + 1] = B.flowNext[2 * (o + i) + 1];
    B.wid[d] = B.st.ids[o + i];
    B.wcnt[d] = B.st.cnt[o + i] + 1;
    B.wsc[d] = B.st.sc[o + i];
  }
  if (tid == 0) {
    B.rejCnt[s] = total[1];
    B.res[s * PTRK_RES] = total[0];
    B.res[s * PTRK_RES + 1] = total[1];
  }
}

// dynamic LDS: 11 MP ints (keep, then two sets of x, y, id, cnt, score)
__global__ __launch_bounds__(256) void k_ptrk_mask(PtrkBatch B) {
  extern __shared__ int ptrk_lds[];
  const int s = blockIdx.x, tid = threadIdx.x, MP = B.MP, W = B.W, H = B.H;
  int* keep = ptrk_lds;
  float* ax = (float*)(ptrk_lds + MP); float* ay = (float*)(ptrk_lds + 2 * MP);
  int* aid = ptrk_lds + 3 * MP; int* acn = ptrk_lds + 4 * MP; float* asc = (float*)(ptrk_lds + 5 * MP);
  float* bx = (float*)(ptrk_lds + 6 * MP); float* by = (float*)(ptrk_lds + 7 * MP);
  int* bid = ptrk_lds + 8 * MP; int* bcn = ptrk_lds + 9 * MP; float* bsc = (float*)(ptrk_lds + 10 * MP);
  __shared__ int m1, nk, take;
  const size_t o = (size_t)s * MP;
  const int m = B.rejCnt[s];
  const bool pub = B.publish[s] != 0;
  for (int i = tid; i < m; i += 256) keep[i] = pub ? B.rejStatus[o + i] : 1;
  if (tid == 0) { m1 = 0; nk = 0; }
  __syncthreads();
  for (int i = tid; i < m; i += 256) {
    if (!keep[i]) continue;
    const int d = ptrk_rank(keep, i);
    ax[d] = B.wforw[2 * (o + i)]; ay[d] = B.wforw[2 * (o + i) + 1];
    aid[d] = B.wid[o + i]; acn[d] = B.wcnt[o + i]; asc[d] = B.wsc[o + i];
    atomicAdd(&m1, 1);
  }
  __syncthreads();
  const int mF = m1;
  if (tid == 0) { B.res[s * PTRK_RES + 2] = mF; B.detUseMask[s] = 1; B.detMinDist[s] = (double)B.minDist; }
  if (!pub) {
    for (int i = tid; i < mF; i += 256) {
      B.kpts[2 * (o + i)] = ax[i]; B.kpts[2 * (o + i) + 1] = ay[i];
      B.kid[o + i] = aid[i]; B.kcnt[o + i] = acn[i]; B.ksc[o + i] = asc[i];
    }
    if (tid == 0) { B.kn[s] = mF; B.res[s * PTRK_RES + 3] = mF; B.detMaxCorners[s] = 0; }
    return;
  }
  // falling track_cnt, equal counts in list order
  for (int i = tid; i < mF; i += 256) {
    int r = 0;
    for (int j = 0; j < mF; ++j) r += (acn[j] > acn[i] || (acn[j] == acn[i] && j < i)) ? 1 : 0;
    bx[r] = ax[i]; by[r] = ay[i]; bid[r] = aid[i]; bcn[r] = acn[i]; bsc[r] = asc[i];
  }
  uint8_t* mask = B.mask + (size_t)s * W * H;
  for (int p = tid; p < W * H; p += 256) mask[p] = B.fisheye ? B.fisheye[p] : (uint8_t)255;
  __syncthreads();
  const int r = B.minDist, D = 2 * r + 1;
  for (int k = 0; k < mF; ++k) {
    const int cx = __float2int_rn(bx[k]), cy = __float2int_rn(by[k]);   // cv::Point(Point2f): cvRound
    if (tid == 0) take = mask[(size_t)cy * W + cx] == 255;
    __syncthreads();
    if (take) {
      if (tid == 0) {
        const size_t d = o + nk;
        B.kpts[2 * d] = bx[k]; B.kpts[2 * d + 1] = by[k]; B.kid[d] = bid[k]; B.kcnt[d] = bcn[k]; B.ksc[d] = bsc[k];
        ++nk;
      }
      for (int e = tid; e < D * D; e += 256) {
        const int j = e / D, dx = e - j * D - r;
        const int x = cx + dx, y = cy + j - r;
        if (abs(dx) <= B.circle[j] && x >= 0 && x < W && y >= 0 && y < H) mask[(size_t)y * W + x] = 0;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    B.kn[s] = nk;
    B.res[s * PTRK_RES + 3] = nk;
    B.detMaxCorners[s] = max(B.maxCnt - nk, 0);
  }
}

__global__ __launch_bounds__(256) void k_ptrk_finish(PtrkBatch B) {
  __shared__ float maxProb;
  __shared__ int nAll;
  const int s = blockIdx.x, tid = threadIdx.x, MP = B.MP;
  const size_t o = (size_t)s * MP;
  const bool pub = B.publish[s] != 0;
  const int kn = B.kn[s];
  const int want = B.detMaxCorners[s];
  const int det = (pub && want > 0) ? B.detCount[s] : 0;
  const bool over = det < 0;
  const int nd = over ? 0 : det;
  const int n = kn + nd;   // <= max_cnt <= MP
  int* hdr = B.nx.hdr + s * PTRK_HDR;
  const int* hd0 = B.st.hdr + s * PTRK_HDR;
  // addPoints (:84-105) behind the kept ones
  for (int i = tid; i < n; i += 256) {
    const bool fresh = i >= kn;
    const size_t c = (size_t)s * B.capCorners + (i - kn);
    B.nx.pts[2 * (o + i)] = fresh ? B.detCorners[2 * c] : B.kpts[2 * (o + i)];
    B.nx.pts[2 * (o + i) + 1] = fresh ? B.detCorners[2 * c + 1] : B.kpts[2 * (o + i) + 1];
    B.nx.ids[o + i] = fresh ? -1 : B.kid[o + i];
    B.nx.cnt[o + i] = fresh ? 1 : B.kcnt[o + i];
    B.nx.sc[o + i] = fresh ? B.detScores[c] : B.ksc[o + i];
  }
  __syncthreads();
  if (tid == 0) {
    float mx = 1.0f;   // max_element of an empty list: 1.0
    for (int i = 0; i < n; ++i) mx = i == 0 ? B.nx.sc[o] : fmaxf(mx, B.nx.sc[o + i]);
    maxProb = mx;
    nAll = n;
  }
  __syncthreads();
  // undistortedPoints (:317-371)
  const int nPrev = hd0[1];
  const double dt = B.time[s] - B.st.time[s];
  double* rows = B.rows + o * PTRK_ROW;
  for (int i = tid; i < n; i += 256) {
    double mx, my;
    pt_lift(B.cam, (double)B.nx.pts[2 * (o + i)], (double)B.nx.pts[2 * (o + i) + 1], mx, my);
    const float ux = (float)mx, uy = (float)my;   // cv::Point2f(b.x() / b.z(), b.y() / b.z()), z = 1
    B.nx.un[2 * (o + i)] = ux; B.nx.un[2 * (o + i) + 1] = uy;
    B.nx.usc[o + i] = B.nx.sc[o + i] / maxProb;
    const int id = B.nx.ids[o + i];
    B.nx.mapId[o + i] = id;
    float vx = 0.f, vy = 0.f;
    if (nPrev > 0 && id != -1)
      for (int j = 0; j < nPrev; ++j)
        if (B.st.mapId[o + j] == id) {   // (pts_velocity is a vector of cv::Point2f)
          vx = (float)((double)(ux - B.st.un[2 * (o + j)]) / dt);
          vy = (float)((double)(uy - B.st.un[2 * (o + j) + 1]) / dt);
          break;
        }
    // the row in list position; compacted below
    double* r = rows + (size_t)i * PTRK_ROW;
    r[0] = (double)ux; r[1] = (double)uy; r[2] = (double)B.nx.pts[2 * (o + i)]; r[3] = (double)B.nx.pts[2 * (o + i) + 1];
    r[4] = (double)vx; r[5] = (double)vy;
  }
  __syncthreads();
  if (tid == 0) {
    // updateID (:263-273) in list order, then the rows of the points with track_cnt > 1 (feature_tracker_node.cpp:130-160); a
    // row only ever moves towards the front
    int next = hd0[2], nr = 0;
    const double prob = n > 0 ? (double)B.nx.usc[o] : 0.0;   // forw_un_scores[0] for every row (node.cpp:154 indexes with the camera)
    for (int i = 0; i < n; ++i) {
      if (B.nx.ids[o + i] == -1) B.nx.ids[o + i] = next++;
      if (pub && B.nx.cnt[o + i] > 1) {
        double* d = rows + (size_t)nr * PTRK_ROW;
        const double* r = rows + (size_t)i * PTRK_ROW;
        for (int q = 0; q < 6; ++q) d[q] = r[q];
        d[6] = prob;
        B.rowId[o + nr] = B.nx.ids[o + i];
        ++nr;
      }
    }
    hdr[0] = n; hdr[1] = n; hdr[2] = next; hdr[3] = 0;
    B.nx.time[s] = B.time[s];
    B.flags[s] = over ? 1 : 0;
    B.res[s * PTRK_RES + 4] = nd;
    B.res[s * PTRK_RES + 5] = nr;
    B.res[s * PTRK_RES + 6] = over ? B.detCount[s] : 0;
    B.res[s * PTRK_RES + 7] = 0;
  }
}

// grid (16, nS): nothing is taken over when any sequence of the call overflowed
__global__ __launch_bounds__(256) void k_ptrk_take(PtrkBatch B, uint8_t* img) {
  for (int q = 0; q < B.nS; ++q)
    if (B.flags[q]) return;
  const int s = blockIdx.y, tid = threadIdx.x, MP = B.MP;
  const size_t PX = (size_t)B.W * B.H;
  const uint8_t* src = img + (size_t)s * PX;
  uint8_t* dst = img + (size_t)(B.nS + s) * PX;
  for (size_t p = (size_t)blockIdx.x * 256 + tid; p < PX; p += (size_t)gridDim.x * 256) dst[p] = src[p];
  if (blockIdx.x != 0) return;
  const size_t o = (size_t)s * MP;
  const int n = B.nx.hdr[s * PTRK_HDR];
  for (int i = tid; i < n; i += 256) {
    B.st.pts[2 * (o + i)] = B.nx.pts[2 * (o + i)]; B.st.pts[2 * (o + i) + 1] = B.nx.pts[2 * (o + i) + 1];
    B.st.un[2 * (o + i)] = B.nx.un[2 * (o + i)]; B.st.un[2 * (o + i) + 1] = B.nx.un[2 * (o + i) + 1];
    B.st.ids[o + i] = B.nx.ids[o + i]; B.st.cnt[o + i] = B.nx.cnt[o + i]; B.st.sc[o + i] = B.nx.sc[o + i];
    B.st.usc[o + i] = B.nx.usc[o + i]; B.st.mapId[o + i] = B.nx.mapId[o + i];
  }
  if (tid < PTRK_HDR) B.st.hdr[s * PTRK_HDR + tid] = B.nx.hdr[s * PTRK_HDR + tid];
  if (tid == 0) B.st.time[s] = B.nx.time[s];
}

}  // namespace vpl

struct vpl_ptrk {
  vpl_fe_ctx* c = nullptr;
  int nS = 0;
  vpl_ptrk_options opt;
  vpl::PtrkBatch B;
  unsigned char* d_in = nullptr;      // times [nS], seeds [nS], publish [nS] (padded to 16 bytes), raw frames
  unsigned char* d_out = nullptr;     // rows [nS][MP][7] doubles, then flags [nS], res [nS][8], row ids [nS][MP]
  size_t in_bytes = 0, out_bytes = 0, raw_off = 0;
  int* d_pairImg = nullptr;           // [2 nS]: previous-image slots, then new-image slots
  float* d_flowNext = nullptr;
  uint8_t* d_flowStatus = nullptr;
  uint8_t* d_rejStatus = nullptr;
  int* d_tabs = nullptr;              // offsets by count [MP + 1], then niters_after of every count 8 .. MP
  uint8_t* d_fisheye = nullptr;
  float *d_detCorners = nullptr, *d_detScores = nullptr;
  int *d_detCount = nullptr, *d_detFound = nullptr;
};

extern "C" {

void vpl_ptrk_default_options(vpl_ptrk_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->max_cnt = 150; o->min_dist = 30; o->f_threshold = 1.0; o->focal_length = 460.0;
  o->equalize = 1; o->clip_limit = 3.0; o->tiles_x = 8; o->tiles_y = 8;
  o->fx = o->fy = 1.0;
}

void vpl_ptrk_destroy(vpl_ptrk* t) {
  if (!t) return;
  vpl_fe_ctx* c = t->c;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  dfree_owner(c, t);
  if (c->ptrk == t) c->ptrk = nullptr;
  delete t;
}

static int ptrk_alloc(vpl_ptrk* t) {
  using namespace vpl;
  vpl_fe_ctx* c = t->c;
  PtrkBatch& B = t->B;
  const size_t nS = t->nS, MP = B.MP, PX = (size_t)c->W * c->H;
  for (PtrkStore* S : {&B.st, &B.nx}) {
    HIPCHK(c, dalloc(c, &S->hdr, nS * PTRK_HDR, t)); HIPCHK(c, dalloc(c, &S->time, nS, t));
    HIPCHK(c, dalloc(c, &S->pts, nS * MP * 2, t)); HIPCHK(c, dalloc(c, &S->ids, nS * MP, t)); HIPCHK(c, dalloc(c, &S->cnt, nS * MP, t));
    HIPCHK(c, dalloc(c, &S->sc, nS * MP, t)); HIPCHK(c, dalloc(c, &S->un, nS * MP * 2, t)); HIPCHK(c, dalloc(c, &S->usc, nS * MP, t));
    HIPCHK(c, dalloc(c, &S->mapId, nS * MP, t));
  }
  HIPCHK(c, dalloc(c, &B.flowCnt, nS, t)); HIPCHK(c, dalloc(c, &t->d_flowNext, nS * MP * 2, t)); HIPCHK(c, dalloc(c, &t->d_flowStatus, nS * MP, t));
  HIPCHK(c, dalloc(c, &B.wcur, nS * MP * 2, t)); HIPCHK(c, dalloc(c, &B.wforw, nS * MP * 2, t)); HIPCHK(c, dalloc(c, &B.wid, nS * MP, t));
  HIPCHK(c, dalloc(c, &B.wcnt, nS * MP, t)); HIPCHK(c, dalloc(c, &B.wsc, nS * MP, t)); HIPCHK(c, dalloc(c, &B.rejCnt, nS, t));
  HIPCHK(c, dalloc(c, &t->d_rejStatus, nS * MP, t));
  HIPCHK(c, dalloc(c, &B.kpts, nS * MP * 2, t)); HIPCHK(c, dalloc(c, &B.kid, nS * MP, t)); HIPCHK(c, dalloc(c, &B.kcnt, nS * MP, t));
  HIPCHK(c, dalloc(c, &B.ksc, nS * MP, t)); HIPCHK(c, dalloc(c, &B.kn, nS, t)); HIPCHK(c, dalloc(c, &B.mask, nS * PX, t));
  HIPCHK(c, dalloc(c, &B.detMaxCorners, nS, t)); HIPCHK(c, dalloc(c, &B.detUseMask, nS, t)); HIPCHK(c, dalloc(c, &B.detMinDist, nS, t));
  HIPCHK(c, dalloc(c, &t->d_detCorners, nS * c->P.capCorners * 2, t)); HIPCHK(c, dalloc(c, &t->d_detScores, nS * c->P.capCorners, t));
  HIPCHK(c, dalloc(c, &t->d_detCount, nS, t)); HIPCHK(c, dalloc(c, &t->d_detFound, nS, t));
  HIPCHK(c, dalloc(c, &t->d_pairImg, 2 * nS, t));
  HIPCHK(c, dalloc(c, &t->d_in, t->in_bytes, t)); HIPCHK(c, dalloc(c, &t->d_out, t->out_bytes, t));
  // the circle of setMask, the slots of the pairs, the stopping table of every list length
  std::vector<int> circle(2 * B.minDist + 1), pairs(2 * nS), tabs(MP + 1, 0);
  pt_circle_half_widths(B.minDist, circle.data());
  for (size_t s = 0; s < nS; ++s) { pairs[s] = (int)(nS + s); pairs[nS + s] = (int)s; }
  for (int n = 8; n <= (int)MP; ++n) {
    tabs[n] = (int)tabs.size();
    tabs.resize(tabs.size() + n + 1);
    relpose_niters_table(n, tabs.data() + tabs[n]);
  }
  int* d_circle = nullptr;
  HIPCHK(c, dalloc(c, &d_circle, circle.size(), t)); HIPCHK(c, dalloc(c, &t->d_tabs, tabs.size(), t));
  HIPCHK(c, hipMemcpy(d_circle, circle.data(), circle.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(t->d_tabs, tabs.data(), tabs.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(t->d_pairImg, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice));
  B.circle = d_circle;
  return VPL_OK;
}

int vpl_ptrk_create(vpl_ptrk** out, vpl_fe_ctx* c, int n_seq, const vpl_ptrk_options* opt) {
  using namespace vpl;
  if (!out || !c || !opt || n_seq < 1) return VPL_E_INVALID;
  if (c->ptrk) return fail(c, VPL_E_INVALID, "ptrk: the context already lends itself to a point tracker session");
  if (!c->ptReserved || !c->ptFlowReserved) return fail(c, VPL_E_INVALID, "ptrk: vpl_pt_reserve first (frames larger than 21 x 21)");
  if (opt->max_cnt < 1 || opt->min_dist < 1 || opt->min_dist > 1024 || !(opt->f_threshold > 0.0) || opt->fx == 0.0 || opt->fy == 0.0 ||
      (opt->equalize && (opt->tiles_x < 1 || opt->tiles_y < 1 || opt->tiles_x > c->W || opt->tiles_y > c->H)))
    return fail(c, VPL_E_INVALID, "ptrk: options out of range");
  if (c->maxN < 2 * n_seq) return fail(c, VPL_E_CAPACITY, "ptrk: the context needs max_images >= 2 n_seq");
  if (opt->max_cnt > c->ptMaxPoints || opt->max_cnt > c->P.capCorners)
    return fail(c, VPL_E_CAPACITY, "ptrk: max_cnt above the reserved max_points or max_corners");
  HIPCHK(c, hipSetDevice(c->device));
  vpl_ptrk* t = new vpl_ptrk();
  t->c = c; t->nS = n_seq; t->opt = *opt;
  PtrkBatch& B = t->B;
  std::memset(&B, 0, sizeof(B));
  B.nS = n_seq; B.MP = c->ptMaxPoints; B.W = c->W; B.H = c->H; B.maxCnt = opt->max_cnt; B.minDist = opt->min_dist;
  const size_t nS = n_seq, MP = B.MP, PX = (size_t)c->W * c->H;
  t->raw_off = (nS * 20 + 15) & ~(size_t)15;
  t->in_bytes = t->raw_off + nS * PX;
  t->out_bytes = nS * MP * PTRK_ROW * 8 + nS * (1 + PTRK_RES + MP) * 4;
  c->ptrk = t;
  const int rc = ptrk_alloc(t);
  if (rc) { vpl_ptrk_destroy(t); return rc; }
  B.time = (const double*)t->d_in;
  B.publish = (const int*)(t->d_in + nS * 16);
  B.flowNext = t->d_flowNext; B.flowStatus = t->d_flowStatus; B.rejStatus = t->d_rejStatus;
  B.detCorners = t->d_detCorners; B.detScores = t->d_detScores; B.detCount = t->d_detCount; B.capCorners = c->P.capCorners;
  vpl_pt_camera k = {opt->fx, opt->fy, opt->cx, opt->cy, opt->k1, opt->k2, opt->p1, opt->p2};
  B.cam = pt_camera(k);
  B.rows = (double*)t->d_out;
  B.flags = (int*)(t->d_out + nS * MP * PTRK_ROW * 8);
  B.res = B.flags + nS;
  B.rowId = B.res + nS * PTRK_RES;
  *out = t;
  return VPL_OK;
}

int vpl_ptrk_set_mask(vpl_ptrk* t, const uint8_t* fisheye_mask) {
  if (!t) return VPL_E_INVALID;
  vpl_fe_ctx* c = t->c;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!fisheye_mask) { t->B.fisheye = nullptr; return VPL_OK; }
  const size_t PX = (size_t)c->W * c->H;
  if (!t->d_fisheye) HIPCHK(c, dalloc(c, &t->d_fisheye, PX, t));
  HIPCHK(c, hipMemcpy(t->d_fisheye, fisheye_mask, PX, hipMemcpyHostToDevice));
  t->B.fisheye = t->d_fisheye;
  return VPL_OK;
}

// the sequence starts again with its next image (no points, no previous un-points); its id counter is kept.  Asynchronous.
int vpl_ptrk_reset(vpl_ptrk* t, int seq) {
  if (!t || seq < 0 || seq >= t->nS) return VPL_E_INVALID;
  vpl_fe_ctx* c = t->c;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemsetAsync(t->B.st.hdr + seq * vpl::PTRK_HDR, 0, 8, c->stream));
  return VPL_OK;
}

int vpl_ptrk_frame(vpl_ptrk* t, const uint8_t* raw, const double* time, const int* publish, const unsigned long long* seed,
                   vpl_ptrk_result* res, int* row_id, double* rows) {
  using namespace vpl;
  if (!t || !raw || !time || !publish || !seed || !res || !row_id || !rows) return VPL_E_INVALID;
  vpl_fe_ctx* c = t->c;
  if (c->haveMaps) return fail(c, VPL_E_INVALID, "ptrk: the point tracker works on distorted frames; the context must hold no undistortion maps");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  PtrkBatch& B = t->B;
  const int nS = t->nS, MP = B.MP;
  const size_t PX = (size_t)c->W * c->H;
  std::vector<unsigned char> in(t->in_bytes);
  std::memcpy(in.data(), time, (size_t)nS * 8);
  std::memcpy(in.data() + (size_t)nS * 8, seed, (size_t)nS * 8);
  std::memcpy(in.data() + (size_t)nS * 16, publish, (size_t)nS * 4);
  std::memcpy(in.data() + t->raw_off, raw, (size_t)nS * PX);
  HIPCHK(c, hipMemcpyAsync(t->d_in, in.data(), t->in_bytes, hipMemcpyHostToDevice, s));
  c->n = 2 * nS; c->B.N = 2 * nS;
  // CLAHE into slots [0, nS)
  { const int rc = pre_launch(c, nS, t->d_in + t->raw_off, t->opt.equalize, t->opt.clip_limit, t->opt.tiles_x, t->opt.tiles_y); if (rc) return rc; }
  // LK from the previous frames
  hipLaunchKernelGGL(k_ptrk_begin, dim3((nS + 63) / 64), dim3(64), 0, s, B);
  c->ptPyr.N = 2 * nS;
  lm_pyr_launch<PT_WIN>(c, c->ptPyr, "k_lm_pyramid_b21", "k_lm_scharr_b21");
  {
    PtFlowBatch F;
    std::memset(&F, 0, sizeof(F));
    F.P = c->ptPyr; F.nPairs = nS; F.maxPts = MP;
    F.prevImg = t->d_pairImg; F.nextImg = t->d_pairImg + nS; F.cnt = B.flowCnt;
    F.prev = B.st.pts; F.next = t->d_flowNext; F.status = t->d_flowStatus;
    const double eps = std::min(std::max(0.01, 0.), 10.);
    F.epsilon = eps * eps; F.minEigThreshold = 1e-4f;
    FeTimer tm(c, "k_pt_flow");
    hipLaunchKernelGGL(k_pt_flow, dim3((B.maxCnt + PT_PER_WAVE - 1) / PT_PER_WAVE, nS), dim3(64), 0, s, F);
  }
  { FeTimer tm(c, "k_ptrk_track"); hipLaunchKernelGGL(k_ptrk_track, dim3(nS), dim3(256), (size_t)MP * 4, s, B); }
  {
    PtRejBatch R;
    std::memset(&R, 0, sizeof(R));
    R.seed = (const unsigned long long*)(t->d_in + (size_t)nS * 8);
    R.cur = B.wcur; R.forw = B.wforw; R.cnt = B.rejCnt; R.enable = B.publish; R.offByCount = t->d_tabs; R.itab = t->d_tabs;
    R.status = t->d_rejStatus; R.maxPts = MP; R.cam = B.cam;
    R.focal = t->opt.focal_length; R.halfCol = c->W / 2.0; R.halfRow = c->H / 2.0; R.thr2 = t->opt.f_threshold * t->opt.f_threshold;
    FeTimer tm(c, "k_pt_reject_f");
    hipLaunchKernelGGL(k_pt_reject_f, dim3(nS), dim3(REL_THREADS), 0, s, R);
  }
  { FeTimer tm(c, "k_ptrk_mask"); hipLaunchKernelGGL(k_ptrk_mask, dim3(nS), dim3(256), (size_t)MP * 11 * 4, s, B); }
  // detect_features under the mask
  {
    PtBatch& P = c->P;
    P.mask = B.mask; P.useMask = B.detUseMask; P.maxCorners = B.detMaxCorners; P.minDist = B.detMinDist;
    P.count = t->d_detCount; P.found = t->d_detFound; P.corners = t->d_detCorners; P.scores = t->d_detScores;
    const int rc = pt_detect_launch(c, nS);
    if (rc) return rc;
  }
  { FeTimer tm(c, "k_ptrk_finish"); hipLaunchKernelGGL(k_ptrk_finish, dim3(nS), dim3(256), 0, s, B); }
  { FeTimer tm(c, "k_ptrk_take"); hipLaunchKernelGGL(k_ptrk_take, dim3(16, nS), dim3(256), 0, s, B, (uint8_t*)c->B.img); }
  HIPCHK(c, hipGetLastError());
  std::vector<unsigned char> out(t->out_bytes);
  HIPCHK(c, hipMemcpyAsync(out.data(), t->d_out, t->out_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  const double* hrows = (const double*)out.data();
  const int* hflags = (const int*)(out.data() + (size_t)nS * MP * PTRK_ROW * 8);
  const int* hres = hflags + nS;
  const int* hid = hres + (size_t)nS * PTRK_RES;
  for (int i = 0; i < nS; ++i)
    if (hflags[i])
      return fail(c, VPL_E_CAPACITY, "ptrk: sequence " + std::to_string(i) + ": " + std::to_string(hres[i * PTRK_RES + 6]) +
                                         " corner candidates, max_candidates is " + std::to_string(c->P.capCand));
  for (int i = 0; i < nS; ++i) {
    const int* r = hres + (size_t)i * PTRK_RES;
    res[i].tracked = r[0]; res[i].after_border = r[1]; res[i].after_f = r[2]; res[i].after_mask = r[3]; res[i].detected = r[4];
    res[i].published = r[5];
    std::memcpy(row_id + (size_t)i * MP, hid + (size_t)i * MP, (size_t)r[5] * 4);
    std::memcpy(rows + (size_t)i * MP * PTRK_ROW, hrows + (size_t)i * MP * PTRK_ROW, (size_t)r[5] * PTRK_ROW * 8);
  }
  return VPL_OK;
}

int vpl_ptrk_get_frame(vpl_ptrk* t, int seq, int* n, float* pts, int* ids, int* track_cnt, float* scores, float* un_pts,
                       float* un_scores, int* next_id) {
  using namespace vpl;
  if (!t || seq < 0 || seq >= t->nS) return VPL_E_INVALID;
  vpl_fe_ctx* c = t->c;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const PtrkStore& S = t->B.st;
  int hdr[PTRK_HDR];
  HIPCHK(c, hipMemcpy(hdr, S.hdr + seq * PTRK_HDR, sizeof(hdr), hipMemcpyDeviceToHost));
  if (n) *n = hdr[0];
  if (next_id) *next_id = hdr[2];
  const size_t o = (size_t)seq * t->B.MP, m = hdr[0];
  if (m == 0) return VPL_OK;
  if (pts) HIPCHK(c, hipMemcpy(pts, S.pts + 2 * o, m * 8, hipMemcpyDeviceToHost));
  if (ids) HIPCHK(c, hipMemcpy(ids, S.ids + o, m * 4, hipMemcpyDeviceToHost));
  if (track_cnt) HIPCHK(c, hipMemcpy(track_cnt, S.cnt + o, m * 4, hipMemcpyDeviceToHost));
  if (scores) HIPCHK(c, hipMemcpy(scores, S.sc + o, m * 4, hipMemcpyDeviceToHost));
  if (un_pts) HIPCHK(c, hipMemcpy(un_pts, S.un + 2 * o, m * 8, hipMemcpyDeviceToHost));
  if (un_scores) HIPCHK(c, hipMemcpy(un_scores, S.usc + o, m * 4, hipMemcpyDeviceToHost));
  return VPL_OK;
}

}  // extern "C"
