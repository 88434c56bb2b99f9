// Loop-closure front-end: what KeyFrame::KeyFrame (pose_graph/src/keyframe.cpp:14-41, computeWindowBRIEFPoint :75-85,
// computeBRIEFPoint :87-113) and KeyFrame::searchByBRIEFDes (:121-171) do per keyframe, for a batch of frames / of pairs.
//   k_lc_blur     cv::GaussianBlur(9 x 9, sigma 2) of DVision::BRIEF::compute (ThirdParty/DVision/BRIEF.cpp:43-60)
//   k_lc_fast     cv::FAST(image, keypoints, t, true): the score plane (0 = no corner)
//   k_lc_rows, k_lc_scan, k_lc_scatter   non-maximum suppression and the ORDERED compaction (raster order) of the survivors
//   k_lc_brief    BRIEF.cpp:83-105 on the blurred plane, for the FAST list and for the window list
//   k_lc_match    searchInAera for every window descriptor of a pair
// STATED HERE, NOT PINNED BY A RUN OF OPENCV (DESIGN.md lists them as deviations; tests/lc_ref.py restates them):
//   the blur  -- OpenCV's 8-bit GaussianBlur is a float filter or a fixed-point one depending on its version.  Here: the taps
//     g_i = exp(-x^2 / (2 sigma^2)), x = -4 .. 4, divided by their sum in double and rounded to float; BORDER_REFLECT_101; the row
//     pass first, r = ((g_0 p_0 + g_1 p_1) + g_2 p_2) + ... in float, every product and sum rounded on its own (contraction off),
//     then the column pass over the float rows in the same way, top to bottom; the result rounded half to even (cvRound) and
//     saturated to 0 .. 255;
//   FAST  -- 9-16 on the Bresenham circle of radius 3: a pixel at least 3 from every border is a corner at threshold t when 9
//     contiguous circle pixels are all > v + t or all < v - t.  Its score is the largest threshold at which it still passes:
//     max(A, B) - 1 with d_k = v - p_k, A = max over the 16 arcs of nine of min d, B = max over the arcs of min -d
//     (cornerScore<16>).  A corner survives when its score is strictly greater than the scores of its 8 neighbours (non-corners
//     score 0).  The list is in raster order: rows top to bottom, x ascending.
// BRIEF as written in the reference: x = (int)(pt.x + m_x[i]), a float sum truncated toward zero (so a sum in (-1, 0) lands on
// column 0 and is inside); a test with an end outside the image leaves its bit 0; bit = I(y1, x1) < I(y2, x2).  Sums that are
// not finite or beyond +-2^30 (where the C conversion is undefined) count as outside.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pre_kernels.h"   // pre_reflect101
#include "pt_kernels.h"    // PtCamera, pt_lift

namespace vpl {

#pragma clang fp contract(off)   // the blur's float arithmetic, un-fused

constexpr int LC_TW = 32, LC_TH = 8;        // a work-group's tile of k_lc_blur and k_lc_fast
constexpr int LC_BLUR_R = 4;                // 9 x 9
constexpr int LC_BITS = 256;                // BRIEF tests per descriptor
constexpr int LC_MAX_KEYPOINTS = 65535;     // an old index travels in 16 bits of k_lc_match's key
constexpr int LC_MAX_WINDOW = 1024;         // k_lc_match keeps one key per window descriptor in LDS
constexpr int LC_MATCH_TILE = 1024;         // old descriptors staged per round of k_lc_match: 32 KB
constexpr int LC_BRIEF_BLOCKS = 32;         // k_lc_brief: work-groups per (frame, list)

struct LcBatch {
  int N, W, H;
  const uint8_t* img;              // [N][H][W] the context's image slots
  uint8_t* blur;                   // [N][H][W]
  uint8_t* score;                  // [N][H][W] FAST score, 0 = no corner
  int* rowOff;                     // [N][H] survivors per row; after k_lc_scan the row's first position in the list
  int* count;                      // [N] keypoints, or -1: more than capKp were found and nothing was written
  int* found;                      // [N] survivors found
  int threshold;
  int capKp, capWin;
  float* kp;                       // [N][capKp][2]
  float* kpNorm;                   // [N][capKp][2]
  unsigned long long* brief;       // [N][capKp][4]
  const float* winPts;             // [N][capWin][2]
  const int* winCnt;               // [N]
  unsigned long long* winBrief;    // [N][capWin][4]
  const int* pat;                  // [4][256]: x1, y1, x2, y2
  float taps[2 * LC_BLUR_R + 1];
  PtCamera cam;
};

// Launch: grid (ceil(W / 32), ceil(H / 8), N), 256 threads.  LDS: 640 B of the 16 x 40 source tile (halo 4, coordinates
// reflected) + 2 KB of its 16 x 32 float row sums.  A lane owns two row sums, then one output pixel.
__global__ __launch_bounds__(LC_TW * LC_TH) void k_lc_blur(LcBatch B) {
  constexpr int R = LC_BLUR_R, RW = LC_TW + 2 * R, RH = LC_TH + 2 * R;
  __shared__ uint8_t raw[RH][RW];
  __shared__ float rowp[RH][LC_TW];
  const int n = blockIdx.z, W = B.W, H = B.H;
  const size_t PX = (size_t)W * H;
  const uint8_t* __restrict__ im = B.img + n * PX;
  const int x0 = blockIdx.x * LC_TW, y0 = blockIdx.y * LC_TH;
  for (int e = threadIdx.x; e < RH * RW; e += LC_TW * LC_TH) {
    const int j = e / RW, i = e - j * RW;
    raw[j][i] = im[(size_t)pre_reflect101(y0 - R + j, H) * W + pre_reflect101(x0 - R + i, W)];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < RH * LC_TW; e += LC_TW * LC_TH) {
    const int j = e / LC_TW, i = e - j * LC_TW;
    float a = B.taps[0] * (float)raw[j][i];
#pragma unroll
    for (int k = 1; k <= 2 * R; ++k) a = a + B.taps[k] * (float)raw[j][i + k];
    rowp[j][i] = a;
  }
  __syncthreads();
  const int tx = threadIdx.x % LC_TW, ty = threadIdx.x / LC_TW;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= W || y >= H) return;
  float a = B.taps[0] * rowp[ty][tx];
#pragma unroll
  for (int k = 1; k <= 2 * R; ++k) a = a + B.taps[k] * rowp[ty + k][tx];
  const int v = __float2int_rn(a);   // half to even
  B.blur[n * PX + (size_t)y * W + x] = (uint8_t)min(max(v, 0), 255);
}

// Launch: grid (ceil(W / 32), ceil(H / 8), N), 256 threads.  LDS: 532 B, the 14 x 38 tile with its 3-pixel halo (coordinates
// clamped: a pixel whose circle leaves the image is no candidate and reads nothing of it).  A lane owns one pixel.
__global__ __launch_bounds__(LC_TW * LC_TH) void k_lc_fast(LcBatch B) {
  constexpr int RW = LC_TW + 6, RH = LC_TH + 6;
  __shared__ uint8_t raw[RH][RW];
  const int n = blockIdx.z, W = B.W, H = B.H;
  const size_t PX = (size_t)W * H;
  const uint8_t* __restrict__ im = B.img + n * PX;
  const int x0 = blockIdx.x * LC_TW, y0 = blockIdx.y * LC_TH;
  for (int e = threadIdx.x; e < RH * RW; e += LC_TW * LC_TH) {
    const int j = e / RW, i = e - j * RW;
    raw[j][i] = im[(size_t)min(max(y0 - 3 + j, 0), H - 1) * W + min(max(x0 - 3 + i, 0), W - 1)];
  }
  __syncthreads();
  const int tx = threadIdx.x % LC_TW, ty = threadIdx.x / LC_TW;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= W || y >= H) return;
  int score = 0;
  if (x >= 3 && y >= 3 && x < W - 3 && y < H - 3) {
    constexpr int ox[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int oy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    const int v = raw[ty + 3][tx + 3];
    int d[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) d[k] = v - (int)raw[ty + 3 + oy[k]][tx + 3 + ox[k]];
    // min and max over the nine entries from k on (cyclic), by doubling: 2, 4, 8, then the ninth
    int lo[16], hi[16], l2[16], h2[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { lo[k] = min(d[k], d[(k + 1) & 15]); hi[k] = max(d[k], d[(k + 1) & 15]); }
#pragma unroll
    for (int k = 0; k < 16; ++k) { l2[k] = min(lo[k], lo[(k + 2) & 15]); h2[k] = max(hi[k], hi[(k + 2) & 15]); }
#pragma unroll
    for (int k = 0; k < 16; ++k) { lo[k] = min(l2[k], l2[(k + 4) & 15]); hi[k] = max(h2[k], h2[(k + 4) & 15]); }
    int A = -255, Bm = 255;   // A = max over arcs of min d;  Bm = min over arcs of max d = -(max over arcs of min -d)
#pragma unroll
    for (int k = 0; k < 16; ++k) { A = max(A, min(lo[k], d[(k + 8) & 15])); Bm = min(Bm, max(hi[k], d[(k + 8) & 15])); }
    const int best = max(A, -Bm);
    if (best > B.threshold) score = best - 1;
  }
  B.score[n * PX + (size_t)y * W + x] = (uint8_t)score;
}

// a corner whose score is strictly greater than its 8 neighbours' (scores are 0 within 3 pixels of the border, so a pixel with
// a score has all 8 neighbours inside the image)
__device__ inline bool lc_survives(const uint8_t* __restrict__ sc, int W, int x, int y) {
  const uint8_t* p = sc + (size_t)y * W + x;
  const int s = p[0];
  if (s == 0) return false;
  return s > p[-1] && s > p[1] && s > p[-W - 1] && s > p[-W] && s > p[-W + 1] && s > p[W - 1] && s > p[W] && s > p[W + 1];
}

// Launch: grid (H, N), one wave.  No LDS.  The wave owns one image row, a lane every 64th pixel of it.
__global__ __launch_bounds__(64) void k_lc_rows(LcBatch B) {
  const int y = blockIdx.x, n = blockIdx.y, W = B.W;
  const uint8_t* sc = B.score + (size_t)n * W * B.H;
  int cnt = 0;
  for (int xb = 0; xb < W; xb += 64) {
    const int x = xb + (int)threadIdx.x;
    const bool s = x < W && lc_survives(sc, W, x, y);
    cnt += __popcll(__ballot(s));
  }
  if (threadIdx.x == 0) B.rowOff[(size_t)n * B.H + y] = cnt;
}

// Launch: grid (N), 256 threads.  LDS: 1 KB.  A lane owns a run of ceil(H / 256) consecutive rows; exclusive scan of the row
// counts in place, the total into found / count.
__global__ __launch_bounds__(256) void k_lc_scan(LcBatch B) {
  __shared__ int part[256];
  const int n = blockIdx.x, H = B.H, t = threadIdx.x;
  int* ro = B.rowOff + (size_t)n * H;
  const int per = (H + 255) / 256, r0 = min(t * per, H), r1 = min(r0 + per, H);
  int sum = 0;
  for (int r = r0; r < r1; ++r) sum += ro[r];
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int at = part[t] - sum;
  for (int r = r0; r < r1; ++r) { const int c = ro[r]; ro[r] = at; at += c; }
  if (t == 255) {
    const int total = part[255];
    B.found[n] = total;
    B.count[n] = total <= B.capKp ? total : -1;
  }
}

// Launch: grid (H, N), one wave.  No LDS.  The wave owns one image row and writes its survivors, x ascending, from the row's
// position on: the pixel position and its lifted ray x / z, y / z rounded to float (cv::Point2f).
__global__ __launch_bounds__(64) void k_lc_scatter(LcBatch B) {
  const int y = blockIdx.x, n = blockIdx.y, W = B.W;
  if (B.count[n] < 0) return;
  const uint8_t* sc = B.score + (size_t)n * W * B.H;
  int at = B.rowOff[(size_t)n * B.H + y];
  float* kp = B.kp + (size_t)n * B.capKp * 2;
  float* kn = B.kpNorm + (size_t)n * B.capKp * 2;
  for (int xb = 0; xb < W; xb += 64) {
    const int x = xb + (int)threadIdx.x;
    const bool s = x < W && lc_survives(sc, W, x, y);
    const unsigned long long m = __ballot(s);
    if (s) {
      const int k = at + __popcll(m & ((1ull << threadIdx.x) - 1ull));
      kp[2 * k] = (float)x; kp[2 * k + 1] = (float)y;
      double mx, my;
      pt_lift(B.cam, (double)(float)x, (double)(float)y, mx, my);
      kn[2 * k] = (float)mx; kn[2 * k + 1] = (float)my;
    }
    at += __popcll(m);
  }
}

// (int)(pt + offset) of BRIEF.cpp:90-93; false = outside [0, len)
__device__ inline bool lc_brief_coord(float p, int off, int len, int& out) {
  const float s = p + (float)off;
  if (!(s > -1073741824.0f && s < 1073741824.0f)) return false;
  out = (int)s;   // toward zero
  return out >= 0 && out < len;
}

// Launch: grid (LC_BRIEF_BLOCKS, N, 2), 256 threads.  No LDS.  blockIdx.z: 0 = the FAST list, 1 = the window list.  A wave owns
// every (4 * LC_BRIEF_BLOCKS)-th keypoint of its list, a lane the tests l, 64 + l, 128 + l, 192 + l: four ballots are the four words.
__global__ __launch_bounds__(256) void k_lc_brief(LcBatch B) {
  const int n = blockIdx.y, list = blockIdx.z, W = B.W, H = B.H;
  const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int cap = list ? B.capWin : B.capKp;
  const int cnt = list ? B.winCnt[n] : B.count[n];
  const float* pts = (list ? B.winPts : B.kp) + (size_t)n * cap * 2;
  unsigned long long* out = (list ? B.winBrief : B.brief) + (size_t)n * cap * 4;
  const uint8_t* __restrict__ im = B.blur + (size_t)n * W * H;
  int px1[4], py1[4], px2[4], py2[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int i = w * 64 + lane;
    px1[w] = B.pat[i]; py1[w] = B.pat[LC_BITS + i]; px2[w] = B.pat[2 * LC_BITS + i]; py2[w] = B.pat[3 * LC_BITS + i];
  }
  for (int k = wave; k < cnt; k += 4 * LC_BRIEF_BLOCKS) {
    const float x = pts[2 * k], y = pts[2 * k + 1];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      int x1, y1, x2, y2;
      bool bit = false;
      // (all four conversions are made: & not &&, one exit for the ballot)
      const bool in = lc_brief_coord(x, px1[w], W, x1) & lc_brief_coord(y, py1[w], H, y1) & lc_brief_coord(x, px2[w], W, x2) &
                      lc_brief_coord(y, py2[w], H, y2);
      if (in) bit = im[(size_t)y1 * W + x1] < im[(size_t)y2 * W + x2];
      const unsigned long long word = __ballot(bit);
      if (lane == 0) out[(size_t)k * 4 + w] = word;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// searchByBRIEFDes (keyframe.cpp:152-171): per window descriptor the old descriptor of least Hamming distance among those
// below 128, the first index on a tie (bestDist = 128, strict <), accepted below 80.
// ---------------------------------------------------------------------------------------------------------------
struct LcMatchBatch {
  int nPairs, capKp, capWin;
  const unsigned long long* winBrief;   // [n][capWin][4]
  const unsigned long long* oldBrief;   // [n][capKp][4]
  const float* oldKp;                   // [n][capKp][2]
  const float* oldNorm;                 // [n][capKp][2]
  const int* winCnt;                    // [n]
  const int* oldCnt;                    // [n]
  float* m2d;                           // [n][capWin][2]
  float* m2dNorm;                       // [n][capWin][2]
  int* bestDist;                        // [n][capWin]
  int* bestIndex;                       // [n][capWin]
  uint8_t* status;                      // [n][capWin]
};

// Launch: grid (n_pairs), 256 threads.  LDS: 32 KB, one tile of LC_MATCH_TILE old descriptors word-major ([4][tile]: lanes read
// consecutive 8-byte words), + 4 KB, the best key of every window descriptor.  The old list is taken tile by tile.  A wave owns
// every 4th window descriptor (its four words in registers), a lane every 64th old descriptor of the tile; the key
// (distance << 16) | index is minimised over the lanes, so the smallest distance wins and, among equals, the lowest index.  A
// distance of 128 or more never beats the initial key 128 << 16.
__global__ __launch_bounds__(256) void k_lc_match(LcMatchBatch B) {
  __shared__ unsigned long long tile[4][LC_MATCH_TILE];
  __shared__ uint32_t best[LC_MAX_WINDOW];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nw = B.winCnt[p], no = B.oldCnt[p];
  const unsigned long long* wb = B.winBrief + (size_t)p * B.capWin * 4;
  const unsigned long long* ob = B.oldBrief + (size_t)p * B.capKp * 4;
  for (int w = tid; w < nw; w += 256) best[w] = 128u << 16;
  for (int t0 = 0; t0 < no; t0 += LC_MATCH_TILE) {
    const int tn = min(LC_MATCH_TILE, no - t0);
    __syncthreads();   // the previous tile has been read; `best` is initialised
    for (int e = tid; e < tn * 4; e += 256) tile[e & 3][e >> 2] = ob[(size_t)t0 * 4 + e];
    __syncthreads();
    for (int w = wave; w < nw; w += 4) {
      const unsigned long long a0 = wb[4 * w], a1 = wb[4 * w + 1], a2 = wb[4 * w + 2], a3 = wb[4 * w + 3];
      uint32_t key = 128u << 16;
      for (int j = lane; j < tn; j += 64) {
        const int dist = __popcll(a0 ^ tile[0][j]) + __popcll(a1 ^ tile[1][j]) + __popcll(a2 ^ tile[2][j]) + __popcll(a3 ^ tile[3][j]);
        key = min(key, ((uint32_t)dist << 16) | (uint32_t)(t0 + j));
      }
      for (int o = 32; o > 0; o >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, o, 64));
      if (lane == 0) best[w] = min(best[w], key);   // (only this wave touches best[w])
    }
  }
  __syncthreads();
  const float* okp = B.oldKp + (size_t)p * B.capKp * 2;
  const float* onr = B.oldNorm + (size_t)p * B.capKp * 2;
  for (int w = tid; w < nw; w += 256) {
    const uint32_t key = best[w];
    const int dist = (int)(key >> 16);
    const int idx = dist < 128 ? (int)(key & 0xffffu) : -1;
    const bool ok = idx >= 0 && dist < 80;
    const size_t o = (size_t)p * B.capWin + w;
    B.bestDist[o] = dist < 128 ? dist : 128;
    B.bestIndex[o] = idx;
    B.status[o] = ok ? 1 : 0;
    B.m2d[2 * o] = ok ? okp[2 * idx] : 0.f;
    B.m2d[2 * o + 1] = ok ? okp[2 * idx + 1] : 0.f;
    B.m2dNorm[2 * o] = ok ? onr[2 * idx] : 0.f;
    B.m2dNorm[2 * o + 1] = ok ? onr[2 * idx + 1] : 0.f;
  }
}

}  // namespace vpl
