// The sample stream and the stopping table of the relative-pose RANSAC (csrc/init_relpose_plan.h), walked over a few thousand
// (seed, N) pairs under the address and undefined-behaviour sanitizers: every sample has seven distinct indices inside the
// correspondence list, the stream is a function of its four integers alone, every entry of the table is an iteration count the
// device may use as a loop bound and the table never rises with the number of inliers.  No GPU.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vplines_ba.h"
#include "init_relpose_plan.h"

using namespace vpl;

static unsigned long long rng_state = 88172645463325252ull;
static unsigned long long rnd64() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}
#define REQUIRE(cond)                                                             \
  do {                                                                            \
    if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); return 1; } \
  } while (0)

int main() {
  int pairs = 0;
  long long samples = 0;
  std::vector<int> hist(VPL_SFM_MAX_TRACKS, 0);
  for (int rep = 0; rep < 3000; ++rep) {
    // the smallest list that can be sampled, the smallest that is tried, the sizes around a wave, the cap, and anything between
    static const int fixed[] = {RELPOSE_SAMPLE, RELPOSE_SAMPLE + 1, 21, 22, 63, 64, 65, VPL_SFM_MAX_TRACKS - 1, VPL_SFM_MAX_TRACKS};
    const int nfixed = (int)(sizeof fixed / sizeof fixed[0]);
    const int n = rep < nfixed ? fixed[rep] : RELPOSE_SAMPLE + (int)(rnd64() % (VPL_SFM_MAX_TRACKS - RELPOSE_SAMPLE + 1));
    const unsigned long long seed = rep % 7 == 0 ? 0ull : (rep % 7 == 1 ? ~0ull : rnd64());
    const int cand = (int)(rnd64() % VPL_WINDOW_SIZE);
    ++pairs;
    // every 40th iteration of the stream, the first and the last among them
    for (int step = 0; step <= 25; ++step) {
      const int it = step == 25 ? RELPOSE_MAX_ITERS - 1 : 40 * step;
      int idx[RELPOSE_SAMPLE] = {-1, -1, -1, -1, -1, -1, -1}, again[RELPOSE_SAMPLE] = {-1, -1, -1, -1, -1, -1, -1};
      relpose_sample(seed, cand, it, n, idx);
      relpose_sample(seed, cand, it, n, again);
      for (int k = 0; k < RELPOSE_SAMPLE; ++k) {
        REQUIRE(idx[k] >= 0 && idx[k] < n && idx[k] == again[k]);
        for (int j = 0; j < k; ++j) REQUIRE(idx[j] != idx[k]);
        if (n == VPL_SFM_MAX_TRACKS) ++hist[idx[k]];
      }
      ++samples;
    }
    std::vector<int> table(n + 1, -1);
    relpose_niters_table(n, table.data());
    REQUIRE(table[0] == RELPOSE_MAX_ITERS && table[n] == 0);
    for (int g = 0; g <= n; ++g) {
      REQUIRE(table[g] >= 0 && table[g] <= RELPOSE_MAX_ITERS);
      if (g) REQUIRE(table[g] <= table[g - 1]);
    }
  }
  // two streams that differ in one of the four integers differ
  {
    int a[RELPOSE_SAMPLE] = {0}, b[RELPOSE_SAMPLE] = {0};
    int same = 0;
    for (int k = 0; k < 64; ++k) {
      relpose_sample(5, 3, k, 1024, a);
      relpose_sample(5, 4, k, 1024, b);
      same += a[0] == b[0];
      relpose_sample(6, 3, k, 1024, b);
      same += a[0] == b[0];
      relpose_sample(5, 3, k + 1, 1024, b);
      same += a[0] == b[0];
    }
    REQUIRE(same < 8);
  }
  // at the cap every index is reachable and none is favoured grossly
  {
    long long total = 0;
    int mx = 0;
    for (int h : hist) { total += h; mx = h > mx ? h : mx; }
    REQUIRE(total > 0 && mx < 40 * (total / VPL_SFM_MAX_TRACKS + 1));
  }
  std::printf("relpose plan ok: %d (seed, N) pairs, %lld samples\n", pairs, samples);
  return 0;
}
