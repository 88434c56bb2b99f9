// The sample stream and the stopping table of the loop verification's PnP RANSAC (vpl_loop_verify_batch, loop_verify.h) as
// integers.  Plain C++, no HIP: the same functions run on the host (vpl_loop_debug_plan) and in the kernel, and
// tests/native/loop_plan_check.cpp walks them under the sanitizers.
//
// The stream is the one of init_relpose_plan.h, read with candidate 0 and the item's seed: the sample of iteration `it` is drawn
// with counter = 0, 1, 2, ... of relpose_draw(seed, 0, it, counter, n); a draw that repeats an index already in the sample is
// dropped and the next counter is taken, until five distinct indices stand in the order they were drawn (five: the model_points
// of cv::solvePnPRansac for more than four points).  n >= 5 always ends.
//
// The table.  niters_after[good], good = 0 .. n, is OpenCV's RANSACUpdateNumIters(confidence, (n - good) / n, 5, max_iters)
// (modules/calib3d/src/ptsetreg.cpp); the reference passes confidence 0.99 and max_iters 100.  The host evaluates it once per n;
// the device reads integers.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "init_relpose_plan.h"

namespace vpl {

constexpr int LOOP_SAMPLE = 5;   // model_points of solvePnPRansac for more than four points

// the five distinct indices of iteration `it`, in the order drawn; n >= LOOP_SAMPLE
VPL_HD void loop_sample(uint64_t seed, int it, int n, int (&idx)[LOOP_SAMPLE]) {
  int have = 0, counter = 0;
#pragma unroll 1
  while (have < LOOP_SAMPLE) {
    const int d = relpose_draw(seed, 0, it, counter++, n);
    bool seen = false;
#pragma unroll
    for (int k = 0; k < LOOP_SAMPLE; ++k) seen = seen || (k < have && idx[k] == d);
    if (seen) continue;
#pragma unroll
    for (int k = 0; k < LOOP_SAMPLE; ++k)
      if (k == have) idx[k] = d;
    ++have;
  }
}

// (host) RANSACUpdateNumIters(p = confidence, ep = (n - good) / n, modelPoints = 5, maxIters = max_iters); cvRound rounds halves to even
inline int loop_niters_after(int n, int good, double confidence, int max_iters) {
  double p = confidence < 0.0 ? 0.0 : (confidence > 1.0 ? 1.0 : confidence);
  double ep = (double)(n - good) / (double)n;
  ep = ep < 0.0 ? 0.0 : (ep > 1.0 ? 1.0 : ep);
  double num = 1.0 - p > DBL_MIN ? 1.0 - p : DBL_MIN;
  double denom = 1.0 - pow(1.0 - ep, (double)LOOP_SAMPLE);
  if (denom < DBL_MIN) return 0;
  num = log(num);
  denom = log(denom);
  if (denom >= 0.0 || -num >= max_iters * (-denom)) return max_iters;
  return (int)nearbyint(num / denom);
}

// table [n + 1]
inline void loop_niters_table(int n, double confidence, int max_iters, int* table) {
  for (int good = 0; good <= n; ++good) table[good] = loop_niters_after(n, good, confidence, max_iters);
}

}  // namespace vpl
