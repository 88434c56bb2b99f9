// Integer bookkeeping of a keyframe session (include/vplines_ba.h, vpl_odo_*): the reference's FeatureManager reduced to what
// the device needs to be told -- per track (id, start frame, number of observations, triangulated), in insertion order
// (f_manager.feature is a std::list; erasing is a stable compaction).  Host only, no HIP: vpl_odo_keyframe and
// vpl_odo_debug_tracks run the same three steps
//   odo_erase_slide : removeFailures / removeLineOutlier decisions + Estimator::slideWindow's removeBackShiftDepth / removeFront
//   odo_add_frame   : FeatureManager::addFeatureCheckParallax, the track part
//   odo_count_unknown : what the capacity check counts
// A track's observations live in a fixed slot of VPL_NFRAMES records on the device, so its index in the book is its address.
#pragma once
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace vpl {

constexpr int ODO_NF = 11;   // VPL_NFRAMES

struct OdoTrack {
  int id, start, nobs, tri;
  int solved = 0;   // point tracks: has taken part in a vpl_odo_solve (FeaturePerId::solve_flag == 1; a depth that came out
                    // <= 0 erases the track at the next advance, removeFailures).  Read by vpl_odo_select's cloud filter only
};

struct OdoBook {   // one kind of tracks (points or lines) of one sequence
  std::vector<OdoTrack> t;
  std::unordered_map<int, int> at;   // id -> index in t
  void reindex() {
    at.clear();
    for (size_t i = 0; i < t.size(); ++i) at[t[i].id] = (int)i;
  }
};

// new track j is the store's track `src`; drop: index of the observation that leaves (-1: none); reanchor: the track started
// in the marginalised frame and survives (inverse depth / Pluecker line move to the next frame)
struct OdoMove {
  int src, drop, reanchor;
};
inline int odo_pack_move(const OdoMove& m) { return m.src | (m.drop + 1) << 20 | m.reanchor << 24; }

// ids of a frame that belong to no track of the book: each would start a track
inline int odo_count_unknown(const OdoBook& b, int n, const int* ids) {
  std::unordered_set<int> seen;
  int k = 0;
  for (int i = 0; i < n; ++i)
    if (!b.at.count(ids[i]) && seen.insert(ids[i]).second) ++k;
  return k;
}

// what the slide does to one track: start / nobs afterwards (nobs 0: erased) and the observation that leaves
inline void odo_slide_track(int flag_second_new, int start, int nobs, int* ostart, int* onobs, int* odrop) {
  constexpr int WS = ODO_NF - 1;
  *ostart = start; *onobs = nobs; *odrop = -1;
  if (!flag_second_new) {                    // removeBackShiftDepth (feature_manager.cpp:800-874)
    if (start != 0) { *ostart = start - 1; return; }
    *odrop = 0;
    *onobs = nobs - 1 < 2 ? 0 : nobs - 1;
    return;
  }
  if (start == WS) { *ostart = WS - 1; return; }   // removeFront(frame_count = WINDOW_SIZE) (feature_manager.cpp:915-956)
  if (start + nobs - 1 < WS - 1) return;
  *odrop = WS - 1 - start;
  *onobs = nobs - 1;
}

// erase[i] != 0: track i leaves before the slide (may be null); then the slide on every remaining track; then the stable
// compaction.  mv[j] says where new track j comes from.  slide_out (may be null): [3] ints (start, nobs, drop) per track that
// entered the slide, in order -- the shape of vpl_slide_tracks.  Returns how many tracks entered the slide.
inline int odo_erase_slide(OdoBook& b, const unsigned char* erase, bool second_new, std::vector<OdoMove>& mv, int* slide_out) {
  mv.clear();
  std::vector<OdoTrack> nt;
  nt.reserve(b.t.size());
  int entered = 0;
  for (size_t i = 0; i < b.t.size(); ++i) {
    if (erase && erase[i]) continue;
    const OdoTrack& t = b.t[i];
    int s, n, d;
    odo_slide_track(second_new ? 1 : 0, t.start, t.nobs, &s, &n, &d);
    if (slide_out) { slide_out[3 * entered] = s; slide_out[3 * entered + 1] = n; slide_out[3 * entered + 2] = d; }
    ++entered;
    if (n == 0) continue;
    mv.push_back(OdoMove{(int)i, d, (!second_new && t.start == 0) ? 1 : 0});
    nt.push_back(OdoTrack{t.id, s, n, t.tri, t.solved});
  }
  b.t.swap(nt);
  b.reindex();
  return entered;
}

// The observations of one frame that enters `slot`: an id continues its track only when the track's last observation is in the
// previous slot, an unknown id starts a track, an id whose track has a gap is ignored.  dest[i] = track | k << 20 | isnew << 24
// (k: the observation's index within the track) or -1 (ignored).  Returns the number of ignored observations.
inline int odo_add_frame(OdoBook& b, int slot, int n, const int* ids, int* dest) {
  int ignored = 0;
  for (int i = 0; i < n; ++i) {
    auto it = b.at.find(ids[i]);
    if (it == b.at.end()) {
      const int j = (int)b.t.size();
      b.t.push_back(OdoTrack{ids[i], slot, 1, 0});
      b.at[ids[i]] = j;
      if (dest) dest[i] = j | 0 << 20 | 1 << 24;
    } else {
      OdoTrack& t = b.t[it->second];
      if (t.start + t.nobs == slot) {
        if (dest) dest[i] = it->second | t.nobs << 20;
        ++t.nobs;
      } else {
        if (dest) dest[i] = -1;
        ++ignored;
      }
    }
  }
  return ignored;
}

// What addFeatureCheckParallax(frame_count = WINDOW_SIZE, image) decides on (feature_manager.cpp:166-188), read off the point
// book once the new image is in slot 10.  list (room for one int per track): the tracks with start <= 8 whose last observation is
// in frame 9 or later, in the book's order, as track | (8 - start) << 20 -- the index of the frame-8 observation within the track;
// the frame-9 observation follows it.  *last_track_num: the observations of the new image that continued a track, i.e. the tracks
// that began before slot 10 and end in it (an id continues at most one track, once).  Returns the number of list entries.
inline int odo_parallax_list(const OdoBook& b, int* list, int* last_track_num) {
  constexpr int WS = ODO_NF - 1;
  int n = 0, last = 0;
  for (size_t i = 0; i < b.t.size(); ++i) {
    const OdoTrack& t = b.t[i];
    if (t.start <= WS - 2 && t.start + t.nobs - 1 >= WS - 1) list[n++] = (int)i | (WS - 2 - t.start) << 20;
    if (t.start < WS && t.start + t.nobs - 1 == WS) ++last;
  }
  *last_track_num = last;
  return n;
}

// The point tracks FeatureSelector::initKDTree takes into its cloud (feature_selector.cpp:561-566): used_num >= 2,
// start_frame < WINDOW_SIZE - 2, start_frame <= 0.75 * WINDOW_SIZE, solve_flag == 1.  list: track | start << 20, in the book's order
inline void odo_cloud_list(const OdoBook& b, std::vector<int>& list) {
  constexpr int WS = ODO_NF - 1;
  for (size_t i = 0; i < b.t.size(); ++i) {
    const OdoTrack& t = b.t[i];
    if (t.nobs >= 2 && t.start < WS - 2 && 4 * t.start <= 3 * WS && t.solved) list.push_back((int)i | t.start << 20);
  }
}

}  // namespace vpl
