// Point front-end: the three OpenCV calls of FeatureTracker::readImage (feature_tracker/src/feature_tracker.cpp:107-224) for a
// batch of frames -- detection (below), pyramidal LK (k_pt_flow) and rejectWithF (k_pt_reject_f), each under its own heading.
//
// DETECTION: cvmodified::goodFeaturesToTrack (feature_tracker/src/cvmodified/cvmodified.cpp:38-216) as
// FeatureTracker::detect_features calls it -- blockSize 3, gradientSize 3, no Harris, qualityLevel 0.01.  Two streaming kernels
// and one work-group per frame:
//   k_pt_mineig    the cornerMinEigenVal plane (4 B out per pixel, the 5 x 5 image footprint through LDS) and, in the same
//                  pass, the masked maximum (one atomicMax per wave on an order-preserving integer image of the float);
//   k_pt_localmax  THRESH_TOZERO at 0.01 max, the 3 x 3 dilation test of :78-93 under the mask, and the compaction of the
//                  surviving pixels into a candidate list (one atomicAdd per wave);
//   k_pt_select    the descending sort of greaterThanPtr (:16-21) as a bitonic sort in LDS, then the greedy min-distance
//                  pass of :109-196 on wave 0.
// THE ARITHMETIC (what OpenCV leaves to its build is fixed here and restated in tests/pt_ref.py; DESIGN.md marks it unpinned):
//   Sobel 3 x 3 of the 8-bit frame into float with s = float(1 / 3060) (2^(aperture-1) * blockSize * 255) folded into the
//   smoothing taps, BORDER_REFLECT_101, rows first:
//       Dx = 2s * d[y] + s * (d[y-1] + d[y+1]),  d = p[x+1] - p[x-1];    Dy = r[y+1] - r[y-1],  r = 2s * p[x] + s * (p[x-1] + p[x+1])
//   every product and sum rounded to float on its own (contraction off);  Dx Dx, Dx Dy, Dy Dy rounded to float, their 3 x 3 sums
//   (BORDER_REFLECT_101 on the product planes) accumulated in double row by row, left to right, and rounded to float once;
//   a = 0.5 Sxx, b = Sxy, c = 0.5 Syy,  eig = (a + c) - sqrt((a - c)^2 + b^2)  in float, the root correctly rounded (taken in
//   double and rounded: 53 >= 2 * 24 + 2 bits make the double rounding harmless).
// THE GREEDY PASS tests a candidate against EVERY corner kept so far instead of the 3 x 3 cells of the reference's grid of
// cell_size = cvRound(minDistance).  The result is the same: a kept corner closer than minDistance differs by at most
// ceil(minDistance) - 1 <= cell_size pixels in x and in y, so it lies in a neighbouring cell and the grid finds it too; a
// corner the grid finds is by definition closer than minDistance.  The decision for candidate k depends only on the kept ones
// before it, so a wave takes 64 candidates at once: each lane tests its own against the kept list (LDS), then the survivors are
// taken over in order, each striking the later lanes of the chunk it is too close to.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lm_kernels.h"    // LmPyr and its kernels, lm_weights, lm_load_bytes
#include "pre_kernels.h"   // pre_reflect101
#include "pt_plan.h"
#include "relpose_f7.h"

namespace vpl {

#pragma clang fp contract(off)   // the float arithmetic above, un-fused

constexpr int PT_TW = 32, PT_TH = 8;   // k_pt_mineig: a work-group's tile of the plane
constexpr int PT_SELECT_THREADS = 1024;

struct PtBatch {
  int N, W, H;
  const uint8_t* img;        // [N][H][W]
  const uint8_t* mask;       // [N][H][W], read for frames with useMask != 0 (may be null when no frame has one)
  const int* useMask;        // [N]
  const int* maxCorners;     // [N] >= 1
  const double* minDist;     // [N] >= 0
  float* eig;                // [N][H][W]
  uint32_t* maxKey;          // [N] pt_key of the masked maximum, 0 = no pixel under the mask (zeroed before every run)
  int* nCand;                // [N] candidates found (zeroed before every run); may exceed capCand: the list is then cut
  unsigned long long* keys;  // [N][capCand] (pt_key(score) << 32 | linear pixel index), in no order
  int capCand;               // pt_plan.h: at most PT_MAX_CANDIDATES
  int capCorners;            // row length of corners / scores
  float* corners;            // [N][capCorners][2]
  float* scores;             // [N][capCorners]
  int* count;                // [N] corners kept, or -1: the candidate list overflowed and nothing was selected
  int* found;                // [N] nCand as k_pt_select saw it (travels with the results)
};

// an unsigned image of a float that orders like the float (and is never 0 for a number)
__device__ inline uint32_t pt_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float pt_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// cvmodified.cpp:167-172: float dx = x - m[j].x, dy = y - m[j].y;  dx * dx + dy * dy < minDistance (squared, a double)
__device__ inline bool pt_too_close(int x, int y, int kx, int ky, double md2) {
  const float dx = (float)x - (float)kx, dy = (float)y - (float)ky;
  return (double)(dx * dx + dy * dy) < md2;
}

__global__ __launch_bounds__(PT_TW * PT_TH) void k_pt_mineig(PtBatch B) {
  __shared__ float sdx[PT_TH + 2][PT_TW + 2], sdy[PT_TH + 2][PT_TW + 2];
  const int n = blockIdx.z, W = B.W, H = B.H;
  const size_t PX = (size_t)W * H;
  const uint8_t* __restrict__ im = B.img + n * PX;
  const int x0 = blockIdx.x * PT_TW, y0 = blockIdx.y * PT_TH;
  const float s = (float)(1.0 / 3060.0), s2 = 2.0f * s;
  // the derivatives at the pixels the box sum reads: plane coordinates first reflected (the box filter's border), the image
  // reads of the Sobel reflected again (its own border)
  for (int e = threadIdx.x; e < (PT_TH + 2) * (PT_TW + 2); e += PT_TW * PT_TH) {
    const int j = e / (PT_TW + 2), i = e - j * (PT_TW + 2);
    const int cx = pre_reflect101(x0 - 1 + i, W), cy = pre_reflect101(y0 - 1 + j, H);
    const int xm = pre_reflect101(cx - 1, W), xp = pre_reflect101(cx + 1, W);
    const uint8_t* r0 = im + (size_t)pre_reflect101(cy - 1, H) * W;
    const uint8_t* r1 = im + (size_t)cy * W;
    const uint8_t* r2 = im + (size_t)pre_reflect101(cy + 1, H) * W;
    const float d0 = (float)r0[xp] - (float)r0[xm], d1 = (float)r1[xp] - (float)r1[xm], d2 = (float)r2[xp] - (float)r2[xm];
    const float t0 = s2 * (float)r0[cx] + s * ((float)r0[xm] + (float)r0[xp]);
    const float t2 = s2 * (float)r2[cx] + s * ((float)r2[xm] + (float)r2[xp]);
    sdx[j][i] = s2 * d1 + s * (d0 + d2);
    sdy[j][i] = t2 - t0;
  }
  __syncthreads();
  const int tx = threadIdx.x % PT_TW, ty = threadIdx.x / PT_TW;
  const int x = x0 + tx, y = y0 + ty;
  const bool in = x < W && y < H;
  double axx = 0, axy = 0, ayy = 0;
  for (int j = 0; j < 3; ++j)
    for (int i = 0; i < 3; ++i) {
      const float dx = sdx[ty + j][tx + i], dy = sdy[ty + j][tx + i];
      const float pxx = dx * dx, pxy = dx * dy, pyy = dy * dy;
      axx = axx + (double)pxx; axy = axy + (double)pxy; ayy = ayy + (double)pyy;
    }
  const float a = (float)axx * 0.5f, b = (float)axy, c = (float)ayy * 0.5f;
  const float amc = a - c;
  const float q = amc * amc + b * b;
  const float eig = (a + c) - (float)sqrt((double)q);
  uint32_t key = 0;
  if (in) {
    const size_t p = (size_t)y * W + x;
    B.eig[n * PX + p] = eig;
    if (!B.useMask[n] || B.mask[n * PX + p]) key = pt_key(eig);
  }
  for (int o = 32; o > 0; o >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, o, 64));
  if ((threadIdx.x & 63) == 0 && key) atomicMax(B.maxKey + n, key);
}

// one lane per pixel; border pixels and lanes past the frame take part in the wave's ballot only
__global__ __launch_bounds__(256) void k_pt_localmax(PtBatch B) {
  const int n = blockIdx.y, W = B.W, H = B.H;
  const size_t PX = (size_t)W * H;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int y = (int)(g / W), x = (int)(g - (size_t)y * W);
  const uint32_t mk = B.maxKey[n];
  const float maxVal = mk ? pt_unkey(mk) : 0.0f;
  const float thr = (float)((double)maxVal * 0.01);   // threshold(eig, eig, maxVal * qualityLevel, 0, THRESH_TOZERO)
  bool cand = false;
  float v = 0.0f;
  if (g < PX && x >= 1 && y >= 1 && x < W - 1 && y < H - 1) {
    const float* __restrict__ e = B.eig + n * PX + g;
    v = e[0] > thr ? e[0] : 0.0f;
    if (v != 0.0f && (!B.useMask[n] || B.mask[n * PX + g])) {
      float d = v;
      for (int j = -1; j <= 1; ++j)
        for (int i = -1; i <= 1; ++i) {
          const float w = e[j * W + i];
          d = fmaxf(d, w > thr ? w : 0.0f);
        }
      cand = v == d;
    }
  }
  const unsigned long long m = __ballot(cand);
  if (m == 0) return;
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == __ffsll((long long)m) - 1) base = atomicAdd(B.nCand + n, __popcll(m));
  base = __shfl(base, __ffsll((long long)m) - 1, 64);
  if (cand) {
    const int pos = base + __popcll(m & ((1ull << lane) - 1));
    if (pos < B.capCand) B.keys[(size_t)n * B.capCand + pos] = ((unsigned long long)pt_key(v) << 32) | (unsigned long long)g;
  }
}

// One work-group per frame.  Dynamic LDS (pt_select_lds_bytes): the keys, padded with zeros to a power of two, then the kept
// corners as (x, y) pairs.
__global__ __launch_bounds__(PT_SELECT_THREADS) void k_pt_select(PtBatch B) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pt_smem[];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int m = B.nCand[n];
  if (tid == 0) B.found[n] = m;
  if (m > B.capCand) {
    if (tid == 0) B.count[n] = -1;
    return;
  }
  const int P = pt_sort_size(m);
  unsigned long long* K = (unsigned long long*)pt_smem;
  int* kept = (int*)(pt_smem + (size_t)pt_sort_size(B.capCand) * 8);
  const unsigned long long* src = B.keys + (size_t)n * B.capCand;
  for (int k = tid; k < P; k += PT_SELECT_THREADS) K[k] = k < m ? src[k] : 0ull;
  __syncthreads();
  // bitonic sort, descending (keys are unique: the pixel index is part of them; the padding sinks to the end)
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (P >> 1); t += PT_SELECT_THREADS) {
        const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), hi = lo | stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long a = K[lo], b = K[hi];
        if ((a < b) == desc) { K[lo] = b; K[hi] = a; }
      }
      __syncthreads();
    }
  if (tid >= 64) return;
  // the greedy pass on wave 0
  const int lane = tid, W = B.W;
  const int maxC = min(B.maxCorners[n], B.capCorners);
  const double md = B.minDist[n], md2 = md * md;
  const bool suppress = md >= 1.0;
  float* oc = B.corners + (size_t)n * B.capCorners * 2;
  float* os = B.scores + (size_t)n * B.capCorners;
  int nk = 0;
  for (int base = 0; base < m && nk < maxC; base += 64) {
    const int k = base + lane;
    const unsigned long long key = k < m ? K[k] : 0ull;
    const int idx = (int)(uint32_t)key, y = idx / W, x = idx - y * W;
    bool alive = k < m;
    if (suppress)
      for (int j = 0; j < nk; ++j)
        if (pt_too_close(x, y, kept[2 * j], kept[2 * j + 1], md2)) alive = false;
    unsigned long long live = __ballot(alive);
    while (live && nk < maxC) {
      const int L = __ffsll((long long)live) - 1;
      const int lx = __shfl(x, L, 64), ly = __shfl(y, L, 64);
      if (lane == L) {
        kept[2 * nk] = x; kept[2 * nk + 1] = y;
        oc[2 * nk] = (float)x; oc[2 * nk + 1] = (float)y;
        os[nk] = pt_unkey((uint32_t)(key >> 32));
        alive = false;
      }
      ++nk;
      if (suppress && alive && pt_too_close(x, y, lx, ly, md2)) alive = false;
      live = __ballot(alive);
    }
    // the kept list written by single lanes is read by all of them in the next chunk
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  if (lane == 0) B.count[n] = nk;
}

// ---------------------------------------------------------------------------------------------------------------
// cv::calcOpticalFlowPyrLK(prev, next, pts, winSize 21 x 21, maxLevel 3), OpenCV's defaults: 30 iterations or a step of 0.01,
// minEigThreshold 1e-4, no initial flow -- the loop of line_matching/src/lk_tracker_invoker_ori.cpp on the padded pyramid and
// Scharr planes that k_lm_level0 / k_lm_down / k_lm_scharr build with a border of 21 (an LmPyr of its own, the same kernels).
// LAYOUT: 21 lanes per point, one window ROW each; three points per wave (lane 63 idles).  A lane keeps its row of the I, dIx
// and dIy window -- 16-bit fixed point from the W_BITS = 14 weights -- in 63 registers for the whole level and reads its two
// rows of J (22 bytes each) afresh in every iteration; there is no LDS.  The scalar state of a point (position, A, D, the
// step) is computed by all of its 21 lanes redundantly from the same numbers, so a group's control flow is uniform.
// SUMMATION ORDER of A11, A12, A22, b1, b2 (OpenCV leaves it to its SIMD build): each window row summed left to right in float
// by its lane, then the 21 row sums added top to bottom, ((r0 + r1) + r2) + ..., by a chain of shuffles that every lane of the
// group runs.  tests/pt_ref.py states the same order.  Contraction is off.
// err is not produced; the range test in front of its loop, which clears status, is.
// ---------------------------------------------------------------------------------------------------------------
constexpr int PT_WIN = 21;
constexpr int PT_LK_MAXCOUNT = 30;
constexpr int PT_PER_WAVE = 64 / PT_WIN;

struct PtFlowBatch {
  LmPyr P;                 // border PT_WIN
  int nPairs, maxPts;
  const int* prevImg;      // [nPairs] image slots
  const int* nextImg;
  const int* cnt;          // [nPairs]
  const float* prev;       // [nPairs][maxPts][2]
  float* next;             // [nPairs][maxPts][2]
  uint8_t* status;         // [nPairs][maxPts]
  double epsilon;          // criteria.epsilon squared
  float minEigThreshold;
};

// the 21 row sums of a group added top to bottom; every lane of the wave calls, every lane of a group gets the same sum
__device__ __forceinline__ float pt_rows_sum(float r, int gbase) {
  float t = __shfl(r, gbase, 64);
#pragma unroll
  for (int k = 1; k < PT_WIN; ++k) t = t + __shfl(r, gbase + k, 64);
  return t;
}

__global__ __launch_bounds__(64) void k_pt_flow(PtFlowBatch B) {
  const int pair = blockIdx.y, lane = threadIdx.x;
  const int n = B.cnt[pair];
  if ((int)blockIdx.x * PT_PER_WAVE >= n) return;
  const int g = lane / PT_WIN, row = lane - g * PT_WIN;
  const int gbase = min(g, PT_PER_WAVE - 1) * PT_WIN;
  const int idx = blockIdx.x * PT_PER_WAVE + g;
  const bool have = g < PT_PER_WAVE && idx < n;
  const LmPyr& P = B.P;
  const uint8_t* pyrI = P.pyr + (size_t)B.prevImg[pair] * P.pyrSize;
  const uint8_t* pyrJ = P.pyr + (size_t)B.nextImg[pair] * P.pyrSize;
  const int16_t* derI = P.der + (size_t)B.prevImg[pair] * P.pyrSize * 2;
  const size_t o = (size_t)pair * B.maxPts + idx;
  const float p0x = have ? B.prev[2 * o] : 0.f, p0y = have ? B.prev[2 * o + 1] : 0.f;
  const float halfWin = (PT_WIN - 1) * 0.5f;
  const float FLT_SCALE = 1.f / (1 << 20);
  float outx = 0.f, outy = 0.f;
  bool st = true;

  for (int level = P.nLevels - 1; level >= 0; --level) {
    const int S = P.ls[level], w = P.lw[level], h = P.lh[level];
    const uint8_t* Ip = pyrI + P.loff[level];
    const uint8_t* Jp = pyrJ + P.loff[level];
    const int16_t* Dp = derI + P.loff[level] * 2;
    const float lscale = (float)(1. / (1 << level));
    float prevx = p0x * lscale, prevy = p0y * lscale;
    float nx, ny;
    if (level == P.nLevels - 1) { nx = prevx; ny = prevy; }
    else { nx = outx * 2.f; ny = outy * 2.f; }
    outx = nx; outy = ny;
    prevx -= halfWin; prevy -= halfWin;
    const int ipx = (int)floorf(prevx), ipy = (int)floorf(prevy);
    bool run = have;
    if (run && (ipx < -PT_WIN || ipx >= w || ipy < -PT_WIN || ipy >= h)) {
      if (level == 0) st = false;
      run = false;
    }
    // this lane's row of the I / dIx / dIy window and of the three sums
    int Iw[PT_WIN], Dx[PT_WIN], Dy[PT_WIN];
    float rA11 = 0.f, rA12 = 0.f, rA22 = 0.f;
#pragma unroll
    for (int x = 0; x < PT_WIN; ++x) { Iw[x] = 0; Dx[x] = 0; Dy[x] = 0; }
    if (run) {
      const LmWeights wt = lm_weights(prevx - ipx, prevy - ipy);
      const size_t at = (size_t)(ipy + row + P.border) * S + (ipx + P.border);
      int v0[PT_WIN + 1], v1[PT_WIN + 1];
      lm_load_bytes<PT_WIN + 1>(Ip + at, v0);
      lm_load_bytes<PT_WIN + 1>(Ip + at + S, v1);
      const int* d0 = (const int*)(Dp + at * 2);   // (dx, dy) pairs, 4-byte aligned
      const int* d1 = d0 + S;
      int e0 = d0[0], e1 = d1[0];
#pragma unroll
      for (int x = 0; x < PT_WIN; ++x) {
        const int f0 = d0[x + 1], f1 = d1[x + 1];
        const int ival = (v0[x] * wt.w00 + v0[x + 1] * wt.w01 + v1[x] * wt.w10 + v1[x + 1] * wt.w11 + (1 << 8)) >> 9;
        const int ixval = ((short)e0 * wt.w00 + (short)f0 * wt.w01 + (short)e1 * wt.w10 + (short)f1 * wt.w11 + (1 << 13)) >> 14;
        const int iyval = ((e0 >> 16) * wt.w00 + (f0 >> 16) * wt.w01 + (e1 >> 16) * wt.w10 + (f1 >> 16) * wt.w11 + (1 << 13)) >> 14;
        Iw[x] = (short)ival; Dx[x] = (short)ixval; Dy[x] = (short)iyval;
        rA11 += (float)(ixval * ixval);
        rA12 += (float)(ixval * iyval);
        rA22 += (float)(iyval * iyval);
        e0 = f0; e1 = f1;
      }
    }
    const float A11 = pt_rows_sum(rA11, gbase) * FLT_SCALE, A12 = pt_rows_sum(rA12, gbase) * FLT_SCALE,
                A22 = pt_rows_sum(rA22, gbase) * FLT_SCALE;
    float D = A11 * A22 - A12 * A12;
    const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (2 * PT_WIN * PT_WIN);
    if (run && (minEig < B.minEigThreshold || D < 1.1920928955078125e-07f)) {
      if (level == 0) st = false;
      run = false;
    }
    D = 1.f / D;
    nx -= halfWin; ny -= halfWin;
    float pdx = 0.f, pdy = 0.f;
    bool iterating = run;
    for (int j = 0; j < PT_LK_MAXCOUNT; ++j) {
      if (!__any(iterating)) break;
      const int inx = (int)floorf(nx), iny = (int)floorf(ny);
      if (iterating && (inx < -halfWin || inx >= w || iny < -halfWin || iny >= h)) {
        if (level == 0) st = false;
        iterating = false;
      }
      float rb1 = 0.f, rb2 = 0.f;
      if (iterating) {
        const LmWeights wt = lm_weights(nx - inx, ny - iny);
        const uint8_t* r = Jp + (size_t)(iny + row + P.border) * S + (inx + P.border);
        int v0[PT_WIN + 1], v1[PT_WIN + 1];
        lm_load_bytes<PT_WIN + 1>(r, v0);
        lm_load_bytes<PT_WIN + 1>(r + S, v1);
#pragma unroll
        for (int x = 0; x < PT_WIN; ++x) {
          const int diff = ((v0[x] * wt.w00 + v0[x + 1] * wt.w01 + v1[x] * wt.w10 + v1[x + 1] * wt.w11 + (1 << 8)) >> 9) - Iw[x];
          rb1 += (float)(diff * Dx[x]);
          rb2 += (float)(diff * Dy[x]);
        }
      }
      const float b1 = pt_rows_sum(rb1, gbase) * FLT_SCALE, b2 = pt_rows_sum(rb2, gbase) * FLT_SCALE;
      if (iterating) {
        const float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
        nx += dx; ny += dy;
        outx = nx + halfWin; outy = ny + halfWin;
        if ((double)dx * dx + (double)dy * dy <= B.epsilon) iterating = false;
        else if (j > 0 && fabsf(dx + pdx) < 0.01 && fabsf(dy + pdy) < 0.01) {
          outx -= dx * 0.5f; outy -= dy * 0.5f;
          iterating = false;
        }
        pdx = dx; pdy = dy;
      }
    }
    if (iterating && level == 0) st = false;   // maxCount iterations without meeting a stopping rule
    if (level == 0 && st && run) {             // the range test in front of the err loop
      const float fx = outx - halfWin, fy = outy - halfWin;
      const int ix = (int)floorf(fx), iy = (int)floorf(fy);
      if (ix < -PT_WIN || ix >= w || iy < -PT_WIN || iy >= h) st = false;
    }
  }
  if (have && row == 0) {
    B.next[2 * o] = outx; B.next[2 * o + 1] = outy;
    B.status[o] = st ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// rejectWithF (feature_tracker.cpp:226-261): both point lists lifted through the camera model, re-projected onto the virtual
// pinhole image FOCAL_LENGTH x / z + COL / 2, FOCAL_LENGTH y / z + ROW / 2, rounded to float (cv::Point2f), then
// cv::findFundamentalMat(FM_RANSAC, F_THRESHOLD, 0.99) as relpose_f7.h runs it: candidate 0 of the caller's seed.
// One work-group of REL_THREADS per list.  A list of fewer than 8 points passes unchanged; a list for which no sample gives a
// model (the reference then reads a mask OpenCV never wrote) loses every point.
// ---------------------------------------------------------------------------------------------------------------
struct PtCamera {   // PinholeCamera with k1, k2, p1, p2 (camera_models/PinholeCamera.cc)
  double inv_K11, inv_K13, inv_K22, inv_K23;   // 1 / fx, -cx / fx, 1 / fy, -cy / fy
  double k1, k2, p1, p2;
};

// PinholeCamera::distortion (:646-662)
__device__ inline void pt_distortion(const PtCamera& c, double x, double y, double& dx, double& dy) {
  const double mx2 = x * x, my2 = y * y, mxy = x * y;
  const double rho2 = mx2 + my2;
  const double rad = c.k1 * rho2 + c.k2 * rho2 * rho2;
  dx = x * rad + 2.0 * c.p1 * mxy + c.p2 * (rho2 + 2.0 * mx2);
  dy = y * rad + 2.0 * c.p2 * mxy + c.p1 * (rho2 + 2.0 * my2);
}

// PinholeCamera::liftProjective (:450-510): the recursive distortion model, 8 steps; the ray is (mx, my, 1)
__device__ inline void pt_lift(const PtCamera& c, double u, double v, double& mx, double& my) {
  const double mx_d = c.inv_K11 * u + c.inv_K13, my_d = c.inv_K22 * v + c.inv_K23;
  double dx, dy;
  pt_distortion(c, mx_d, my_d, dx, dy);
  mx = mx_d - dx; my = my_d - dy;
  for (int i = 1; i < 8; ++i) {
    pt_distortion(c, mx, my, dx, dy);
    mx = mx_d - dx; my = my_d - dy;
  }
}

struct PtRejBatch {
  const unsigned long long* seed;   // [n]
  const float* cur;                 // [n][maxPts][2]
  const float* forw;
  const int* cnt;                   // [n]
  const int* nitOff;                // [n] where niters_after [cnt + 1] of the list starts in itab (lists of 8 points and more)
  const int* offByCount;            // or, when the counts are known on the device only: [maxPts + 1] the start of every count's table
  const int* enable;                // null, or [n]: a list with 0 here passes unchanged (a frame that is not published)
  const int* itab;
  uint8_t* status;                  // [n][maxPts]
  int maxPts;                       // <= PT_MAX_POINTS
  PtCamera cam;
  double focal, halfCol, halfRow;   // FOCAL_LENGTH, COL / 2.0, ROW / 2.0
  double thr2;                      // F_THRESHOLD squared
};

__global__ __launch_bounds__(REL_THREADS) void k_pt_reject_f(PtRejBatch B) {
  __shared__ double pt[4 * PT_MAX_POINTS];
  __shared__ RelRansacLds R;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int N = B.cnt[s];
  uint8_t* status = B.status + (size_t)s * B.maxPts;
  if (N < 8 || (B.enable && !B.enable[s])) {
    for (int p = tid; p < N; p += REL_THREADS) status[p] = 1;
    return;
  }
  const float* cur = B.cur + (size_t)s * B.maxPts * 2;
  const float* forw = B.forw + (size_t)s * B.maxPts * 2;
  for (int p = tid; p < N; p += REL_THREADS) {
    double x, y;   // the ray is (x, y, 1): x / z is x
    pt_lift(B.cam, (double)cur[2 * p], (double)cur[2 * p + 1], x, y);
    pt[4 * p] = (double)(float)(B.focal * x + B.halfCol);
    pt[4 * p + 1] = (double)(float)(B.focal * y + B.halfRow);
    pt_lift(B.cam, (double)forw[2 * p], (double)forw[2 * p + 1], x, y);
    pt[4 * p + 2] = (double)(float)(B.focal * x + B.halfCol);
    pt[4 * p + 3] = (double)(float)(B.focal * y + B.halfRow);
  }
  __syncthreads();
  rel_ransac_run(pt, N, B.seed[s], 0, B.itab + (B.offByCount ? B.offByCount[N] : B.nitOff[s]), B.thr2, R, nullptr);
  if (R.st[RS_BEST_IT] < 0) {
    for (int p = tid; p < N; p += REL_THREADS) status[p] = 0;
    return;
  }
  double Fw[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Fw[k] = R.F[k];
  for (int p = tid; p < N; p += REL_THREADS)
    status[p] = rel_inlier(Fw, pt[4 * p], pt[4 * p + 1], pt[4 * p + 2], pt[4 * p + 3], B.thr2) ? 1 : 0;
}

}  // namespace vpl
