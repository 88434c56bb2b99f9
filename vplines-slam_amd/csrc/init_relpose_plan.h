// The sample stream and the stopping table of the relative-pose RANSAC (vpl_init_relative_pose_batch, init_relpose.h) as integers.
// Plain C++, no HIP: the same functions run on the host (vpl_relpose_debug_plan) and in the kernel, and
// tests/native/relpose_plan_check.cpp walks them under the sanitizers.
//
// The stream.  Every draw is a function of four integers and of nothing else:
//     h = mix(mix(mix(mix(seed) ^ candidate) ^ iteration) ^ counter)
// with mix the finaliser of splitmix64 (z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
// z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31), all in unsigned 64-bit arithmetic.  candidate is the window frame
// i = 0 .. 9 the hypothesis pairs with frame 10 -- not the sequence's place in a batch, which the stream never sees.  The
// index of a draw among N correspondences is the upper half of h, multiplied by N, shifted down by 32 bits: 0 .. N - 1, no
// floating point, a bias below N / 2^32.  The sample of iteration `it` is drawn with counter = 0, 1, 2, ...: a draw that
// repeats an index already in the sample is dropped and the next counter is taken, until seven distinct indices stand in the
// order they were drawn.  N >= 7 always ends; the expected number of draws at N = 21 is 8.2.
//
// The table.  niters_after[good], good = 0 .. N, is OpenCV's RANSACUpdateNumIters(0.99, (N - good) / N, 7, 1000)
// (modules/calib3d/src/ptsetreg.cpp): the only place of the estimator that needs pow and log.  The host evaluates it once per
// N; the device reads integers.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "vpl_math.h"

namespace vpl {

constexpr int RELPOSE_SAMPLE = 7;          // the minimal sample of the fundamental matrix
constexpr int RELPOSE_MAX_ITERS = 1000;    // cv::findFundamentalMat's maxIters
constexpr int RELPOSE_MIN_CORRES = 20;     // relativePose tries a frame with MORE correspondences (estimator.cpp:598)
constexpr int RELPOSE_MIN_GOOD = 12;       // solveRelativeRT succeeds with MORE points in front (solve_5pts.cpp:222)

VPL_HD uint64_t relpose_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// draw number `counter` of iteration `it` of candidate frame `cand`: an index below n
VPL_HD int relpose_draw(uint64_t seed, int cand, int it, int counter, int n) {
  uint64_t h = relpose_mix(seed);
  h = relpose_mix(h ^ (uint64_t)(uint32_t)cand);
  h = relpose_mix(h ^ (uint64_t)(uint32_t)it);
  h = relpose_mix(h ^ (uint64_t)(uint32_t)counter);
  return (int)(((h >> 32) * (uint64_t)(uint32_t)n) >> 32);
}

// the seven distinct indices of iteration `it`, in the order drawn; n >= RELPOSE_SAMPLE
VPL_HD void relpose_sample(uint64_t seed, int cand, int it, int n, int (&idx)[RELPOSE_SAMPLE]) {
  int have = 0, counter = 0;
#pragma unroll 1
  while (have < RELPOSE_SAMPLE) {
    const int d = relpose_draw(seed, cand, it, counter++, n);
    bool seen = false;
#pragma unroll
    for (int k = 0; k < RELPOSE_SAMPLE; ++k) seen = seen || (k < have && idx[k] == d);
    if (seen) continue;
#pragma unroll
    for (int k = 0; k < RELPOSE_SAMPLE; ++k)
      if (k == have) idx[k] = d;
    ++have;
  }
}

// (host) RANSACUpdateNumIters(p = 0.99, ep = (n - good) / n, modelPoints = 7, maxIters = 1000); cvRound rounds halves to even
inline int relpose_niters_after(int n, int good) {
  const double p = 0.99;
  double ep = (double)(n - good) / (double)n;
  ep = ep < 0.0 ? 0.0 : (ep > 1.0 ? 1.0 : ep);
  double num = 1.0 - p > DBL_MIN ? 1.0 - p : DBL_MIN;
  double denom = 1.0 - pow(1.0 - ep, (double)RELPOSE_SAMPLE);
  if (denom < DBL_MIN) return 0;
  num = log(num);
  denom = log(denom);
  if (denom >= 0.0 || -num >= RELPOSE_MAX_ITERS * (-denom)) return RELPOSE_MAX_ITERS;
  return (int)nearbyint(num / denom);
}

// table [n + 1]
inline void relpose_niters_table(int n, int* table) {
  for (int good = 0; good <= n; ++good) table[good] = relpose_niters_after(n, good);
}

}  // namespace vpl
