// The sizes of the point detector (csrc/pt_plan.h) walked under the address and undefined-behaviour sanitizers: the sort
// length is the power of two at or above the candidate count and never below a wave, the LDS of k_pt_select fits the CU at
// every admitted capacity and is refused above it, and the circle table of every radius up to 64 is symmetric, as wide as
// 2 r + 1 in the middle, monotone towards the poles and inside the disc.  No GPU.
#include <cstdio>
#include <vector>

#include "pt_plan.h"

using namespace vpl;

#define REQUIRE(cond)                                                             \
  do {                                                                            \
    if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); return 1; } \
  } while (0)

int main() {
  for (int n = 0; n <= PT_MAX_CANDIDATES; ++n) {
    const int p = pt_sort_size(n);
    REQUIRE(p >= n && p >= PT_MIN_SORT && (p & (p - 1)) == 0);
    REQUIRE(p == PT_MIN_SORT || p / 2 < n);
  }
  const size_t lds_cu = 160 * 1024;
  REQUIRE(pt_select_lds_bytes(PT_MAX_CANDIDATES, PT_MAX_CORNERS) <= lds_cu);
  REQUIRE(pt_select_lds_bytes(1, 1) == (size_t)PT_MIN_SORT * 8 + 8);
  for (int cand = 1; cand <= PT_MAX_CANDIDATES; cand += 37)
    for (int cor = 1; cor <= PT_MAX_CORNERS; cor += 89) {
      REQUIRE(pt_capacities_ok(cand, cor, 1 + (cand + cor) % PT_MAX_POINTS));
      const size_t b = pt_select_lds_bytes(cand, cor);
      REQUIRE(b <= lds_cu && b % 8 == 0);
      REQUIRE((size_t)pt_sort_size(cand) * 8 % 16 == 0);   // the kept list starts 16-byte aligned behind the keys
    }
  REQUIRE(!pt_capacities_ok(0, 1, 1) && !pt_capacities_ok(1, 0, 1) && !pt_capacities_ok(1, 1, 0) &&
          !pt_capacities_ok(PT_MAX_CANDIDATES + 1, 1, 1) && !pt_capacities_ok(1, PT_MAX_CORNERS + 1, 1) &&
          !pt_capacities_ok(1, 1, PT_MAX_POINTS + 1) && !pt_capacities_ok(-5, -5, -5));
  // the reject stage's upload: every section starts on a multiple of its element size, the tables fit behind the lists
  for (int n = 1; n <= 64; n += 7)
    for (int mp = 1; mp <= PT_MAX_POINTS; mp += 31) {
      const size_t seeds = (size_t)n * 8, lists = 2 * (size_t)n * mp * 8, ints = 2 * (size_t)n * 4, tables = (size_t)n * (mp + 1) * 4;
      REQUIRE(pt_reject_upload_bytes(n, mp) == seeds + lists + ints + tables);
      REQUIRE(seeds % 8 == 0 && (seeds + lists) % 4 == 0);
    }
  REQUIRE(4 * (size_t)PT_MAX_POINTS * 8 + 4096 <= 64 * 1024);   // k_pt_reject_f's static LDS

  int radii = 0;
  for (int r = 0; r <= 64; ++r) {
    std::vector<int> hw(2 * r + 1, -1);
    pt_circle_half_widths(r, hw.data());
    REQUIRE(hw[r] == r);
    for (int j = 0; j <= 2 * r; ++j) {
      REQUIRE(hw[j] >= 0 && hw[j] == hw[2 * r - j]);
      if (j > 0 && j <= r) REQUIRE(hw[j] >= hw[j - 1]);
      const long long dy = j - r, w = hw[j];
      REQUIRE(w * w + dy * dy <= (long long)r * r + r);
      REQUIRE((w + 1) * (w + 1) + dy * dy > (long long)r * r - r);
    }
    ++radii;
  }
  {
    int hw[61];
    pt_circle_half_widths(30, hw);
    static const int want[31] = {0, 7, 10, 13, 14, 16, 18, 19, 20, 21, 22, 23, 24, 24, 25, 25, 26, 27, 27, 27, 28, 28, 28, 29, 29, 29, 29, 29, 29, 29, 30};
    for (int j = 0; j <= 30; ++j) REQUIRE(hw[j] == want[j]);   // the same table tests/pt_ref.py builds
  }
  std::printf("pt plan ok: %d sort sizes, %d radii\n", PT_MAX_CANDIDATES + 1, radii);
  return 0;
}
