// The id book of the feature selector, host only (no device, no HIP): the members FeatureSelector::select keeps between images
// (feature_selector.cpp:71-198) -- lastFeatureId_, trackedFeatures_, firstImage_ -- and what select() does with them around the
// greedy selection.  vpl_sel_debug_book replays it over a script; tests/native/sel_book_check.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <vector>

#include "vplines_ba.h"

namespace vpl {

struct SelBook {
  int max_features = 0, init_thresh = 0;
  int last_id = 0;                 // lastFeatureId_
  bool first_image = true;         // firstImage_
  std::vector<int> tracked;        // trackedFeatures_: only grows
};
// one image between sel_book_split and sel_book_finish: std::map order everywhere, i.e. ascending ids
struct SelImage {
  std::vector<int> image;          // the ids not above lastFeatureId_
  std::vector<int> image_new;      // the ids above it
  std::vector<int> subset;         // the tracked ids that are present in the image
  int kappa = 0;                   // max(0, max_features - |subset|)
};

// splitOnFeatureId, the move of lastFeatureId_, the subset and kappa
inline void sel_book_split(SelBook& b, const int* ids, int n, SelImage& im) {
  std::vector<int> all(ids, ids + n);
  std::sort(all.begin(), all.end());
  all.erase(std::unique(all.begin(), all.end()), all.end());
  const auto cut = std::upper_bound(all.begin(), all.end(), b.last_id);
  im.image.assign(all.begin(), cut);
  im.image_new.assign(cut, all.end());
  if (!im.image_new.empty()) b.last_id = im.image_new.back();
  im.subset.clear();
  for (int fid : b.tracked)
    if (std::binary_search(im.image.begin(), im.image.end(), fid)) im.subset.push_back(fid);
  std::sort(im.subset.begin(), im.subset.end());
  im.subset.erase(std::unique(im.subset.begin(), im.subset.end()), im.subset.end());
  im.kappa = std::max(0, b.max_features - (int)im.subset.size());
}

// the rest of select(): `selected` is what the greedy selection returned (read only when initialized); out: the ids handed to
// the back end, ascending
inline void sel_book_finish(SelBook& b, const SelImage& im, bool initialized, const int* selected, int n_selected, std::vector<int>& out) {
  out = im.subset;
  int n_chosen = 0;
  if (initialized) {
    n_chosen = n_selected;
    out.insert(out.end(), selected, selected + n_selected);
  } else if (b.first_image) {
    out = im.image_new;                                     // the whole image initialises
    b.tracked.insert(b.tracked.end(), out.begin(), out.end());
    b.first_image = false;
  }
  if (!initialized && (int)out.size() < b.init_thresh) out.insert(out.end(), im.image.begin(), im.image.end());
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
  b.tracked.insert(b.tracked.end(), selected, selected + n_chosen);
}

// vpl_sel_debug_book (include/vplines_ba.h)
inline int sel_book_replay(int max_features, int init_thresh, int n_images, const int* n_ids, const int* ids, const unsigned char* initialized,
                           const int* n_offer, const int* offer, int max_ids, int* n_new, int* kappa, int* n_selected, int* selected,
                           int* n_out, int* out_ids, int* n_tracked, int* last_id, int max_tracked, int* tracked) {
  if (n_images < 0 || max_ids < 0 || max_tracked < 0 || !n_ids || !ids || !initialized || !n_offer || !offer || !n_new || !kappa ||
      !n_selected || !selected || !n_out || !out_ids || !n_tracked || !last_id || !tracked)
    return VPL_E_INVALID;
  for (int s = 0; s < n_images; ++s)
    if (n_ids[s] < 0 || n_offer[s] < 0) return VPL_E_INVALID;
  SelBook b;
  b.max_features = max_features;
  b.init_thresh = init_thresh;
  size_t at = 0, oat = 0;
  for (int s = 0; s < n_images; at += n_ids[s], oat += n_offer[s], ++s) {
    SelImage im;
    sel_book_split(b, ids + at, n_ids[s], im);
    if ((int)(im.image.size() + im.image_new.size()) > max_ids) return VPL_E_CAPACITY;
    std::vector<int> sel;
    for (int k = 0; k < n_offer[s] && (int)sel.size() < im.kappa; ++k) {
      const int fid = offer[oat + k];
      if (std::binary_search(im.image_new.begin(), im.image_new.end(), fid) && std::find(sel.begin(), sel.end(), fid) == sel.end()) sel.push_back(fid);
    }
    if (!initialized[s]) sel.clear();
    std::vector<int> out;
    sel_book_finish(b, im, initialized[s] != 0, sel.data(), (int)sel.size(), out);
    n_new[s] = (int)im.image_new.size();
    kappa[s] = im.kappa;
    n_selected[s] = (int)sel.size();
    std::copy(sel.begin(), sel.end(), selected + (size_t)s * max_ids);
    n_out[s] = (int)out.size();
    std::copy(out.begin(), out.end(), out_ids + (size_t)s * max_ids);
    n_tracked[s] = (int)b.tracked.size();
    last_id[s] = b.last_id;
  }
  if ((int)b.tracked.size() > max_tracked) return VPL_E_CAPACITY;
  std::copy(b.tracked.begin(), b.tracked.end(), tracked);
  return VPL_OK;
}

}  // namespace vpl
