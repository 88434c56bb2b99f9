// Sizes of the point detector (pt_kernels.h) as integers.  Plain C++, no HIP: the same functions size the launch on the host
// and index the LDS in the kernel, and tests/native/pt_plan_check.cpp walks them under the sanitizers.
//
// Capacities.  The candidate list of a frame (pixels that pass the quality threshold and the 3 x 3 maximum test) has
// max_candidates entries, fixed by vpl_pt_reserve.  k_pt_select sorts it in LDS as 64-bit keys padded to a power of two, so
// max_candidates <= PT_MAX_CANDIDATES = 16384 (128 KB of the CU's 160 KB); the kept corners, two ints each, follow the keys,
// so max_corners <= PT_MAX_CORNERS = 2048 (16 KB).  A 752 x 480 EuRoC frame yields 3 000 - 3 500 candidates.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "vpl_math.h"   // VPL_HD

namespace vpl {

constexpr int PT_MAX_CANDIDATES = 16384;
constexpr int PT_MAX_CORNERS = 2048;
constexpr int PT_MAX_POINTS = 1024;   // a tracked point list: k_pt_reject_f keeps (x1, y1, x2, y2) of each as doubles in LDS (32 KB)
constexpr int PT_MIN_SORT = 64;   // one wave's worth: the smallest bitonic network k_pt_select runs

// the length the bitonic sort runs over for n candidates: the power of two at or above max(n, PT_MIN_SORT)
VPL_HD int pt_sort_size(int n) {
  int p = PT_MIN_SORT;
  while (p < n) p <<= 1;
  return p;
}

// dynamic LDS of k_pt_select for a context reserved with these capacities
VPL_HD size_t pt_select_lds_bytes(int max_candidates, int max_corners) {
  return (size_t)pt_sort_size(max_candidates) * 8 + (size_t)max_corners * 2 * sizeof(int);
}

// The pixel set of a filled circle of integer radius r as OpenCV's integer midpoint walk fills it (imgproc/drawing.cpp,
// Circle(): err = 0, dx = r, dy = 0, plus = 1, minus = 2 r - 1; every step fills rows cy -+ dy over cx -+ dx and rows cy -+ dx
// over cx -+ dy, then dy++, err += plus, plus += 2, and once err > 0: err -= minus, dx--, minus -= 2), as half-widths per row:
// row cy + (j - r) covers cx - hw[j] .. cx + hw[j], j = 0 .. 2 r.  The walk's set, not dx^2 + dy^2 <= r^2 evaluated per
// pixel: the two need not agree at every radius.  Restated from the algorithm; no run of cv::circle pins it.
inline void pt_circle_half_widths(int r, int* hw /* [2 r + 1] */) {
  for (int j = 0; j <= 2 * r; ++j) hw[j] = 0;
  int err = 0, dx = r, dy = 0, plus = 1, minus = (r << 1) - 1;
  while (dx >= dy) {
    const int rows[2] = {dy, dx}, half[2] = {dx, dy};
    for (int k = 0; k < 2; ++k) {
      if (hw[r + rows[k]] < half[k]) hw[r + rows[k]] = half[k];
      if (hw[r - rows[k]] < half[k]) hw[r - rows[k]] = half[k];
    }
    ++dy;
    err += plus;
    plus += 2;
    const int mask = (err <= 0) - 1;
    err -= minus & mask;
    dx += mask;
    minus -= mask & 2;
  }
}

inline bool pt_capacities_ok(int max_candidates, int max_corners, int max_points) {
  return max_candidates >= 1 && max_candidates <= PT_MAX_CANDIDATES && max_corners >= 1 && max_corners <= PT_MAX_CORNERS &&
         max_points >= 1 && max_points <= PT_MAX_POINTS;
}

// bytes of the one upload of vpl_pt_reject_f_batch for n lists of at most max_points: seeds, the two point lists, counts, table
// offsets, then niters_after [count + 1] per list
inline size_t pt_reject_upload_bytes(int n, int max_points) {
  return (size_t)n * (8 + 2 * (size_t)max_points * 8 + 4 + 4 + ((size_t)max_points + 1) * 4);
}

}  // namespace vpl
