// The schedule of GlobalSFM::construct as the host builds it (csrc/init_sfm_plan.h), walked over a few hundred random track tables
// and every l under the address and undefined-behaviour sanitizers: every index the device will follow lies inside its table, and
// the tables agree with each other.  No GPU.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "init_sfm_plan.h"

using namespace vpl;

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd(unsigned n) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (unsigned)(rng_state % n);
}
#define REQUIRE(cond)                                                             \
  do {                                                                            \
    if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); return 1; } \
  } while (0)

int main() {
  int plans = 0, starved = 0;
  for (int rep = 0; rep < 300; ++rep) {
    // sparse tables starve a PnP, dense ones do not; the cap once
    const int n = rep == 0 ? VPL_SFM_MAX_TRACKS : (rep % 3 == 0 ? (int)rnd(20) : 20 + (int)rnd(120));
    std::vector<int> start(n), nobs(n);
    for (int j = 0; j < n; ++j) {
      if (rnd(2)) {   // over most of the window
        start[j] = (int)rnd(3);
        nobs[j] = VPL_NFRAMES - start[j] - (int)rnd(3);
      } else {
        start[j] = (int)rnd(VPL_NFRAMES);
        nobs[j] = 1 + (int)rnd(VPL_NFRAMES - start[j]);
      }
    }
    for (int l = 0; l < VPL_WINDOW_SIZE; ++l) {
      std::string msg;
      REQUIRE(sfm_check_tracks(l, n, start.data(), nobs.data(), msg) == VPL_OK);
      SfmPlan P;
      sfm_build_plan(l, n, start.data(), nobs.data(), P);
      ++plans;
      REQUIRE((int)P.step.size() == n && (int)P.fa.size() == n && (int)P.fb.size() == n);
      std::vector<int> when(n, -1);   // the event that gives the track its position
      size_t used = 0;
      for (size_t e = 0; e < P.events.size(); ++e) {
        const SfmEvent& ev = P.events[e];
        REQUIRE(ev.list0 == (int)used && ev.n >= 0 && used + ev.n <= P.lists.size());
        used += ev.n;
        for (int k = 0; k < ev.n; ++k) {
          const int j = P.lists[ev.list0 + k];
          REQUIRE(j >= 0 && j < n);
          if (ev.kind == SFM_EV_PNP) {
            REQUIRE(when[j] >= 0 && start[j] <= ev.f0 && ev.f0 < start[j] + nobs[j]);   // triangulated before, seen in the frame
          } else {
            REQUIRE(when[j] < 0);
            when[j] = (int)e;
            const int f0 = ev.kind == SFM_EV_TRI ? ev.f0 : start[j], f1 = ev.kind == SFM_EV_TRI ? ev.f1 : start[j] + nobs[j] - 1;
            REQUIRE(P.fa[j] == f0 && P.fb[j] == f1 && f0 != f1);
            REQUIRE(start[j] <= f0 && f0 < start[j] + nobs[j] && start[j] <= f1 && f1 < start[j] + nobs[j]);
            REQUIRE(P.step[j] >= 1 && P.step[j] <= 5 && (P.step[j] == 5) == (ev.kind == SFM_EV_LAST));
          }
        }
        if (ev.kind == SFM_EV_PNP) {
          REQUIRE(ev.f0 >= 0 && ev.f0 < VPL_WINDOW_SIZE && ev.f0 != l && (ev.f1 == ev.f0 - 1 || ev.f1 == ev.f0 + 1));
          REQUIRE(P.count[ev.f0] == ev.n && ev.n >= SFM_MIN_KEY_PNP);
        }
      }
      REQUIRE(used == P.lists.size());
      for (int j = 0; j < n; ++j) REQUIRE((when[j] >= 0) == (P.step[j] >= 0) && (P.step[j] >= 0 || (P.fa[j] == -1 && P.fb[j] == -1)));
      REQUIRE(P.count[l] == -1 && P.count[VPL_WINDOW_SIZE] == -1);
      if (P.first_fail >= 0) {
        ++starved;
        REQUIRE(P.first_fail != l && P.first_fail < VPL_WINDOW_SIZE && P.count[P.first_fail] >= 0 && P.count[P.first_fail] < SFM_MIN_KEY_PNP);
      } else {
        REQUIRE(!P.events.empty() && P.events.back().kind == SFM_EV_LAST);
        for (int f = 0; f < VPL_WINDOW_SIZE; ++f) REQUIRE(f == l || P.count[f] >= SFM_MIN_KEY_PNP);
        for (int j = 0; j < n; ++j) REQUIRE((P.step[j] >= 0) == (nobs[j] >= 2));
      }
    }
  }
  // the refusals
  {
    std::string msg;
    const int s1[1] = {9}, n3[1] = {3}, n0[1] = {0}, n2[1] = {2};
    REQUIRE(sfm_check_tracks(10, 1, s1, n2, msg) == VPL_E_INVALID);
    REQUIRE(sfm_check_tracks(-1, 1, s1, n2, msg) == VPL_E_INVALID);
    REQUIRE(sfm_check_tracks(3, 1, s1, n3, msg) == VPL_E_INVALID);
    REQUIRE(sfm_check_tracks(3, 1, s1, n0, msg) == VPL_E_INVALID);
    REQUIRE(sfm_check_tracks(3, 1, nullptr, n2, msg) == VPL_E_INVALID);
    REQUIRE(sfm_check_tracks(3, VPL_SFM_MAX_TRACKS + 1, s1, n2, msg) == VPL_E_CAPACITY);
    REQUIRE(sfm_check_tracks(3, 1, s1, n2, msg) == VPL_OK);
  }
  REQUIRE(starved > 100 && plans - starved > 100);
  std::printf("sfm plan ok: %d plans, %d of them starved\n", plans, starved);
  return 0;
}
