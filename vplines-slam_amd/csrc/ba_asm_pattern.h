// The static side of k_lin's assembly of the packed camera Hessian Hcc (lin_assemble, ba_lin.h): where an entry's terms come
// from, which entries the factors of a fast-path window can fill, and the tables the context builds from the two.  Plain C++:
// the device code, the context (vplines_ba.hip) and the host-only check (tests/native/asm_pattern_check.cpp) include it.
#pragma once
#include <vector>

#include "ba_types.h"

namespace vpl {

#ifdef __HIPCC__
#define VPL_ASM_HD __host__ __device__ __forceinline__
#else
#define VPL_ASM_HD inline
#endif

// cam index -> vis index or -1
VPL_ASM_HD int cam2vis(int c) {
  if (c >= 165) return 66 + (c - 165);
  int o = c % 15;
  return o < 6 ? 6 * (c / 15) + o : -1;
}

// The vis Hessian in LDS: lower block triangle of 12 x 12 blocks of 6 x 6 (frames 0..10, extrinsic), every block stored
// full -- 78 blocks = 2808 doubles instead of the 72 x 72 square.  Entry (r, c), r >= c in vis indices:
constexpr int HV_DOUBLES = 78 * 36;
VPL_ASM_HD int hvi(int r, int c) {
  const int br = r / 6, bc = c / 6;
  return 36 * (br * (br + 1) / 2 + bc) + 6 * (r - 6 * br) + (c - 6 * bc);
}

// Static description of packed cam-Hessian entry (r, c), r >= c, for the assembly pass of k_lin (the same for every
// window; built once per context):  x = (index into the LDS vis Hessian + 1) | (index into the LDS IMU blocks + 1) << 16,
// 0 meaning "no such source";  y = r | c << 8 | tri(r, c) << 16.  IMU blocks: 11 diagonal 15x15 lower triangles (120 each),
// then 10 sub-diagonal full blocks (225 each).
inline void lin_asm_entry(int r, int c, int* out) {
  int hv = 0, im = 0;
  const int vr = cam2vis(r), vc = cam2vis(c);
  if (vr >= 0 && vc >= 0) hv = hvi(vr, vc) + 1;
  if (r < 165) {
    const int fr = r / 15, ar = r - 15 * fr, fc = c / 15, bc = c - 15 * fc;
    if (fc == fr) im = 120 * fr + ar * (ar + 1) / 2 + bc + 1;
    else if (fc == fr - 1) im = 11 * 120 + 225 * (fr - 1) + 15 * ar + bc + 1;
  }
  out[0] = hv | im << 16;
  out[1] = r | c << 8 | tri(r, c) << 16;
}

// Whether the factors of a fast-path window (B.path != 1: the prior's only speed/bias block is frame 0's) can fill entry
// (r, c), r >= c: vis x vis (the visual factors; the prior's pose and extrinsic blocks), the 15-dim frame blocks and their
// sub-diagonal neighbours (the IMU factors; the prior's speed/bias 0 against pose 0 and itself), speed/bias 0 against every
// vis dim (the prior).  NZ_N entries of the NCP; the others are the complement.
inline bool asm_in_pattern(int r, int c) {
  const bool vis = cam2vis(r) >= 0 && cam2vis(c) >= 0;
  const int fr = r < 165 ? r / 15 : -1, fc = c < 165 ? c / 15 : -1;
  const bool band = fr >= 0 && fc >= 0 && (fr == fc || fr == fc + 1);
  const bool sb0 = c >= 6 && c < 15 && cam2vis(r) >= 0;
  return vis || band || sb0;
}
constexpr int NZ_C = NCP - NZ_N;   // the complement: 8559 entries

// The tables of a context, all from asm_in_pattern and in increasing packed index: nz (B.nz_tab) holds the pattern as
// idx | r << 14 | c << 22; asm_tab (B.asm_tab) holds the lin_asm_entry pairs of the NZ_N pattern entries -- pass A of
// lin_assemble, every window -- and behind them those of the NZ_C complement entries -- pass B, windows of the general path.
inline void asm_build_tables(std::vector<int>& nz, std::vector<int>& asm_tab) {
  nz.clear();
  std::vector<int> pat, comp;
  for (int r = 0; r < NC; ++r)
    for (int c = 0; c <= r; ++c) {
      int d[2];
      lin_asm_entry(r, c, d);
      std::vector<int>& t = asm_in_pattern(r, c) ? pat : comp;
      t.push_back(d[0]); t.push_back(d[1]);
      if (asm_in_pattern(r, c)) nz.push_back(tri(r, c) | r << 14 | c << 22);
    }
  asm_tab = pat;
  asm_tab.insert(asm_tab.end(), comp.begin(), comp.end());
}

}  // namespace vpl
