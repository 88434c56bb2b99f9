// The five-point sample stream and the stopping table of the loop verification's RANSAC (csrc/loop_plan.h), walked under the
// address and undefined-behaviour sanitizers: every sample has five distinct indices inside the list, the stream is a function
// of (seed, iteration, N) alone, N = 5 ends, the table is a loop bound that never rises with the number of inliers.  With
// arguments "seed N confidence max_iters" it prints the samples and the table for the test to compare with its own.  No GPU.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vplines_ba.h"
#include "loop_plan.h"

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

int main(int argc, char** argv) {
  if (argc == 5) {   // dump: one line per sample, then the table on one line
    const unsigned long long seed = std::strtoull(argv[1], nullptr, 10);
    const int n = std::atoi(argv[2]), max_iters = std::atoi(argv[4]);
    const double confidence = std::atof(argv[3]);
    REQUIRE(n >= LOOP_SAMPLE && n <= VPL_LOOP_MAX_POINTS && max_iters >= 1 && max_iters <= VPL_LOOP_MAX_ITERS);
    for (int it = 0; it < max_iters; ++it) {
      int idx[LOOP_SAMPLE] = {-1, -1, -1, -1, -1};
      loop_sample(seed, it, n, idx);
      std::printf("s %d %d %d %d %d\n", idx[0], idx[1], idx[2], idx[3], idx[4]);
    }
    std::vector<int> table(n + 1, -1);
    loop_niters_table(n, confidence, max_iters, table.data());
    std::printf("t");
    for (int g = 0; g <= n; ++g) std::printf(" %d", table[g]);
    std::printf("\n");
    return 0;
  }
  int pairs = 0;
  long long samples = 0;
  for (int rep = 0; rep < 2000; ++rep) {
    static const int fixed[] = {LOOP_SAMPLE, LOOP_SAMPLE + 1, 25, 26, 63, 64, 65, VPL_LOOP_MAX_POINTS - 1, VPL_LOOP_MAX_POINTS};
    const int nfixed = (int)(sizeof fixed / sizeof fixed[0]);
    const int n = rep < nfixed ? fixed[rep] : LOOP_SAMPLE + (int)(rnd64() % (VPL_LOOP_MAX_POINTS - LOOP_SAMPLE + 1));
    const unsigned long long seed = rep % 7 == 0 ? 0ull : (rep % 7 == 1 ? ~0ull : rnd64());
    ++pairs;
    for (int step = 0; step <= 10; ++step) {
      const int it = step == 10 ? VPL_LOOP_MAX_ITERS - 1 : 10 * step;
      int idx[LOOP_SAMPLE] = {-1, -1, -1, -1, -1}, again[LOOP_SAMPLE] = {-1, -1, -1, -1, -1};
      loop_sample(seed, it, n, idx);
      loop_sample(seed, it, n, again);
      for (int k = 0; k < LOOP_SAMPLE; ++k) {
        REQUIRE(idx[k] >= 0 && idx[k] < n && idx[k] == again[k]);
        for (int j = 0; j < k; ++j) REQUIRE(idx[j] != idx[k]);
      }
      ++samples;
    }
    const int max_iters = rep % 3 == 0 ? 100 : 1 + (int)(rnd64() % VPL_LOOP_MAX_ITERS);
    std::vector<int> table(n + 1, -1);
    loop_niters_table(n, 0.99, max_iters, table.data());
    REQUIRE(table[0] == max_iters && table[n] == 0);
    for (int g = 0; g <= n; ++g) {
      REQUIRE(table[g] >= 0 && table[g] <= max_iters);
      if (g) REQUIRE(table[g] <= table[g - 1]);
    }
  }
  // the stream is the relative pose's with candidate 0: the first draw of an iteration is the first index of its sample
  {
    int a[LOOP_SAMPLE] = {0}, b[LOOP_SAMPLE] = {0};
    int same = 0;
    for (int k = 0; k < 64; ++k) {
      loop_sample(5, k, 1024, a);
      REQUIRE(a[0] == relpose_draw(5, 0, k, 0, 1024));
      loop_sample(6, k, 1024, b);
      same += a[0] == b[0];
      loop_sample(5, k + 1, 1024, b);
      same += a[0] == b[0];
    }
    REQUIRE(same < 8);
  }
  std::printf("loop plan ok: %d (seed, N) pairs, %lld samples\n", pairs, samples);
  return 0;
}
