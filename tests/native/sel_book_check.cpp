// The id book of the feature selector (csrc/sel_book.h), replayed over random scripts under the address and undefined-behaviour
// sanitizers: ids that come, go and come back, uninitialised stretches, offers with repeats and strangers, kappa down to 0, the
// capacity refusals with arrays of exactly the stated size.  Every image: the selection is new, within kappa and among the
// offers; what is handed out is ascending, distinct and present in the image; the tracked list only grows.  No GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vplines_ba.h"
#include "sel_book.h"

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
  long long images = 0;
  for (int rep = 0; rep < 400; ++rep) {
    const int n_images = 1 + (int)(rnd64() % 12), max_features = (int)(rnd64() % 30), init_thresh = (int)(rnd64() % 20);
    std::vector<int> n_ids(n_images), n_offer(n_images), ids, offer;
    std::vector<unsigned char> init(n_images);
    int next = 1, max_ids = 1;
    std::vector<int> alive;
    for (int s = 0; s < n_images; ++s) {
      std::vector<int> img;
      for (int a : alive)
        if (rnd64() % 4) img.push_back(a);                       // some disappear (and may come back: alive keeps them)
      const int fresh = (int)(rnd64() % 15);
      for (int k = 0; k < fresh; ++k) { img.push_back(next); alive.push_back(next); next += 1 + (int)(rnd64() % 3); }
      if (!img.empty() && rnd64() % 3 == 0) img.push_back(img[0]);   // a repeated id
      std::vector<int> off;
      for (int a : img)
        if (rnd64() % 2) off.push_back(a);
      off.push_back(1000000 + s);                                // a stranger
      n_ids[s] = (int)img.size();
      n_offer[s] = (int)off.size();
      ids.insert(ids.end(), img.begin(), img.end());
      offer.insert(offer.end(), off.begin(), off.end());
      init[s] = s >= 2 && rnd64() % 3 != 0;
      std::sort(img.begin(), img.end());
      max_ids = std::max(max_ids, (int)(std::unique(img.begin(), img.end()) - img.begin()));
    }
    ids.push_back(0);
    offer.push_back(0);
    const int max_tracked = (int)ids.size();
    std::vector<int> n_new(n_images), kappa(n_images), n_sel(n_images), n_out(n_images), n_tr(n_images), last(n_images);
    std::vector<int> sel((size_t)n_images * max_ids), out((size_t)n_images * max_ids), tracked(max_tracked);
    const int rc = sel_book_replay(max_features, init_thresh, n_images, n_ids.data(), ids.data(), init.data(), n_offer.data(), offer.data(), max_ids,
                                   n_new.data(), kappa.data(), n_sel.data(), sel.data(), n_out.data(), out.data(), n_tr.data(), last.data(),
                                   max_tracked, tracked.data());
    REQUIRE(rc == VPL_OK);
    size_t at = 0;
    int prev_tr = 0, prev_last = 0;
    for (int s = 0; s < n_images; at += n_ids[s], ++s, ++images) {
      std::vector<int> img(ids.begin() + at, ids.begin() + at + n_ids[s]);
      REQUIRE(kappa[s] >= 0 && kappa[s] <= max_features && n_sel[s] <= kappa[s] && n_new[s] <= n_ids[s]);
      REQUIRE(n_tr[s] >= prev_tr && last[s] >= prev_last);
      if (!init[s]) REQUIRE(n_sel[s] == 0);
      for (int k = 0; k < n_sel[s]; ++k) {
        const int fid = sel[(size_t)s * max_ids + k];
        REQUIRE(fid > prev_last && std::find(img.begin(), img.end(), fid) != img.end());
      }
      REQUIRE(n_out[s] <= max_ids);
      for (int k = 0; k < n_out[s]; ++k) {
        const int fid = out[(size_t)s * max_ids + k];
        REQUIRE(std::find(img.begin(), img.end(), fid) != img.end());
        if (k) REQUIRE(fid > out[(size_t)s * max_ids + k - 1]);
      }
      prev_tr = n_tr[s];
      prev_last = last[s];
    }
    // one id too many for max_ids, one tracked id too many for max_tracked: refused, nothing written past the arrays
    if (max_ids > 1)
      REQUIRE(sel_book_replay(max_features, init_thresh, n_images, n_ids.data(), ids.data(), init.data(), n_offer.data(), offer.data(), max_ids - 1,
                              n_new.data(), kappa.data(), n_sel.data(), sel.data(), n_out.data(), out.data(), n_tr.data(), last.data(), max_tracked,
                              tracked.data()) == VPL_E_CAPACITY);
    if (prev_tr > 0) {
      std::vector<int> small(prev_tr - 1 > 0 ? prev_tr - 1 : 1);
      REQUIRE(sel_book_replay(max_features, init_thresh, n_images, n_ids.data(), ids.data(), init.data(), n_offer.data(), offer.data(), max_ids,
                              n_new.data(), kappa.data(), n_sel.data(), sel.data(), n_out.data(), out.data(), n_tr.data(), last.data(), prev_tr - 1,
                              small.data()) == VPL_E_CAPACITY);
    }
  }
  REQUIRE(sel_book_replay(10, 5, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, 4, nullptr) == VPL_E_INVALID);
  std::printf("sel book ok: %lld images\n", images);
  return 0;
}
