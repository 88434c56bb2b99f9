// The schedule of GlobalSFM::construct (initial/initial_sfm.cpp:117-312) as integer tables: which track is triangulated at
// which step and from which two window frames, and which tracks every PnP of the chain sees.  All of it follows from l and from
// where observations exist (a track covers the window frames start .. start + nobs - 1), never from their values, so the host
// builds it once and the device works from it (init_sfm.h); vpl_sfm_debug_plan hands it out.  Plain C++, no HIP:
// tests/native/sfm_plan_check.cpp walks it under the sanitizers.
#pragma once
#include <string>
#include <vector>

#include "vplines_ba.h"

namespace vpl {

constexpr int SFM_MIN_KEY_PNP = 10;     // solveFrameByPnP returns false below (initial_sfm.cpp:48)
constexpr int SFM_MIN_FRAME_PNP = 6;    // estimator.cpp:481
enum { SFM_EV_TRI = 0, SFM_EV_PNP = 1, SFM_EV_LAST = 2 };

// One event of the chain.  TRI: the tracks list0 .. list0 + n - 1 of `lists` are triangulated from window frames f0, f1 (point0
// from f0).  PNP: window frame f0 is solved from the pose of f1 over those tracks.  LAST: the tracks are triangulated from
// their first and last observation.
struct SfmEvent {
  int kind, f0, f1, list0, n;
};
struct SfmPlan {
  std::vector<int> step, fa, fb;   // per track
  int count[VPL_NFRAMES];
  int first_fail = -1;
  std::vector<SfmEvent> events;
  std::vector<int> lists;
};

// the refusals that need nothing but the track tables; msg names the first one met
inline int sfm_check_tracks(int l, int n_tracks, const int* start, const int* nobs, std::string& msg) {
  if (l < 0 || l > VPL_WINDOW_SIZE - 1) { msg = "sfm: l outside 0 .. 9"; return VPL_E_INVALID; }
  if (n_tracks < 0) { msg = "sfm: negative n_tracks"; return VPL_E_INVALID; }
  if (n_tracks > VPL_SFM_MAX_TRACKS) { msg = "sfm: more than VPL_SFM_MAX_TRACKS tracks"; return VPL_E_CAPACITY; }
  if (n_tracks && (!start || !nobs)) { msg = "sfm: null track_start / track_nobs"; return VPL_E_INVALID; }
  for (int j = 0; j < n_tracks; ++j) {
    if (start[j] < 0 || start[j] > VPL_WINDOW_SIZE || nobs[j] < 1) { msg = "sfm: a track outside the window or without observations"; return VPL_E_INVALID; }
    if (nobs[j] > VPL_NFRAMES - start[j]) { msg = "sfm: a track running past frame 10"; return VPL_E_INVALID; }
  }
  return VPL_OK;
}

inline void sfm_build_plan(int l, int n, const int* start, const int* nobs, SfmPlan& P) {
  const int last = VPL_NFRAMES - 1;
  P.step.assign(n, -1); P.fa.assign(n, -1); P.fb.assign(n, -1);
  P.events.clear(); P.lists.clear();
  P.first_fail = -1;
  for (int f = 0; f < VPL_NFRAMES; ++f) P.count[f] = -1;
  std::vector<char> state(n, 0);
  auto has = [&](int j, int f) { return start[j] <= f && f < start[j] + nobs[j]; };
  auto tri = [&](int f0, int f1, int code) {
    SfmEvent e{SFM_EV_TRI, f0, f1, (int)P.lists.size(), 0};
    for (int j = 0; j < n; ++j)
      if (!state[j] && has(j, f0) && has(j, f1)) {
        state[j] = 1; P.step[j] = code; P.fa[j] = f0; P.fb[j] = f1;
        P.lists.push_back(j);
        ++e.n;
      }
    P.events.push_back(e);
  };
  auto pnp = [&](int f, int neighbour) {
    SfmEvent e{SFM_EV_PNP, f, neighbour, (int)P.lists.size(), 0};
    for (int j = 0; j < n; ++j)
      if (state[j] && has(j, f)) { P.lists.push_back(j); ++e.n; }
    P.count[f] = e.n;
    if (e.n < SFM_MIN_KEY_PNP) {
      P.lists.resize(e.list0);
      P.first_fail = f;
      return false;
    }
    P.events.push_back(e);
    return true;
  };
  // 1 / 2: forward, each frame against the last
  for (int i = l; i < last; ++i) {
    if (i > l && !pnp(i, i - 1)) return;
    tri(i, last, i == l ? 1 : 2);
  }
  // 3: l against l + 1 .. 9
  for (int i = l + 1; i < last; ++i) tri(l, i, 3);
  // 4: backward, each frame against l
  for (int i = l - 1; i >= 0; --i) {
    if (!pnp(i, i + 1)) return;
    tri(i, l, 4);
  }
  // 5: whatever is left, first against last observation
  SfmEvent e{SFM_EV_LAST, -1, -1, (int)P.lists.size(), 0};
  for (int j = 0; j < n; ++j)
    if (!state[j] && nobs[j] >= 2) {
      state[j] = 1; P.step[j] = 5; P.fa[j] = start[j]; P.fb[j] = start[j] + nobs[j] - 1;
      P.lists.push_back(j);
      ++e.n;
    }
  P.events.push_back(e);
}

}  // namespace vpl
