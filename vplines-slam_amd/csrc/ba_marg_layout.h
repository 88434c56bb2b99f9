// LDS layout of k_marg, once, for the host (the size of the dispatch) and the device (every pointer marg_body uses).
// Plain C++: tests/native/marg_layout_check.cpp includes it without HIP and checks, for every kept size and both forms, that the
// regions tile [0, total), that every tenant stays inside the region it borrows and that the dispatch covers every window.
#pragma once
#include "ba_layout.h"
#include "ba_limits.h"

namespace vpl {

constexpr int MARG_MD = 15;            // dims marginalised through the pseudo-inverse: sb_0 (9) + pose_0 (6); 6 under MARGIN_SECOND_NEW
constexpr int MTROWS_MAX = 96;         // landmark rows staged per elimination pass: 96 where the prior leaves the LDS for it (every pass
                                       // costs two global round trips and three barriers), 64 or 32 for large priors
constexpr int MARG_ROW = 74;           // row stride of a staged landmark row: 72 visual dims + the rhs, padded
constexpr int MARG_E15_LD = 17;        // row stride of the marginalised block Amm (md x md, md <= 15)
constexpr int MARG_E15_DOUBLES = 16 * MARG_E15_LD;
constexpr int MARG_TMP_MIN = 640;      // tmp is max(nd * 16, this): the row constants below end at 128 + 96 + 240 + 96 = 560
constexpr int MARG_RED_DOUBLES = 24;   // reduction words of the work-group factorisation
constexpr int MARG_VLIST_INTS = 96;    // tenants of tmp, first: vlist (nd <= MAXKEEP + 15 = 95 dense dims with a visual index) ...
constexpr int MARG_VINV_INTS = 72;     // ... and vinv (visual column -> dense index or -1) behind it
constexpr int MARG_ROWC = 128;         // tenants of tmp, second: the row constants of a staging pass start here (vinv is live beside them)
constexpr int MARG_LINEC_DOUBLES = 10 * (MTROWS_MAX / 4);   // the packed 4 x 4 factor of every staged line
constexpr int PSD_WAVE4_META = 24;     // psd_pivoted_cholesky_wave4: candidates of two pivot steps and the tail counts, behind its column
// the template arguments marg_body gives the register forms of the pivoted Cholesky (ba_psd.h): the column length NMAX of the
// one-wave form for Amm and for the kept block, and the NQ row slices of NH rows of the column-slice form
constexpr int PSD_NMAX_AMM = 16, PSD_NMAX_WAVE = 48, PSD_WAVE4_NH = 19, PSD_WAVE4_NQ = 4;

// small = the 256-thread form of k_marg: at most 79 KB, so that two work-groups share a CU (most of the kernel is a lone
// wave factoring a 15 x 15 and the kept block while the other waves wait: a second window on the CU uses the idle SIMDs);
// its landmark lists hold 256 entries per kind.  MARG_LDS_MAX: what a dispatch may ask for at all.
constexpr size_t MARG_LDS_BIG = 150 * 1024, MARG_LDS_SMALL = 79 * 1024, MARG_LDS_MAX = 159 * 1024;

// LDS scratch (doubles) the register forms of the pivoted Cholesky ask for in their signature comments: the factor by rows
// (n x ld), the pivot column (NMAX) and, wave4 only, its meta words
VPL_LAYOUT_HD inline int psd_scratch_doubles(int n, int ld, int nmax, bool wave4) { return n * ld + nmax + (wave4 ? PSD_WAVE4_META : 0); }
// the form marg_body picks for a kept block of n dims on T threads needs this much of Ad (the work-group version: none)
VPL_LAYOUT_HD inline int marg_factor_scratch(int n, int ld, bool small) {
  return n <= PSD_NMAX_WAVE                        ? psd_scratch_doubles(n, ld, PSD_NMAX_WAVE, false)
         : (!small && n <= PSD_WAVE4_NH * PSD_WAVE4_NQ) ? psd_scratch_doubles(n, ld, PSD_WAVE4_NH * PSD_WAVE4_NQ, true)
                                                        : 0;
}

// One text for two readers (ba_layout.h): P = int on the host (MargLayout, what the size of the dispatch and the CPU check read)
// and P = double* on the device (marg_body's pointers).
template <class P> using MargSpanT = LdsSpanT<P>;

template <class P> struct MargLayoutT {
  typedef MargSpanT<P> MargSpan;
  int ldm, EB, nd, ldd, total, mtrows, loff;
  // ---- regions, in carve order; each begins where the one before it ends, spare ends at total ----
  MargSpan G;      // n x ldm: kept block -> its factor
  MargSpan Ad;     // nd x ldd: dense pre-marginalisation matrix
  MargSpan tile;   // mtrows x MARG_ROW: staged landmark rows
  MargSpan E15;    // 15 x 17: Amm -> its factor
  MargSpan bv;     // nd: right-hand side
  MargSpan tmp;    // max(nd * 16, 640)
  MargSpan lam;    // max(n, 2) + 16
  MargSpan red;    // 24
  MargSpan perm;   // ints: max(n, 16), rounded up to a double
  MargSpan dmap;   // ints: nd, rounded up to a double
  MargSpan lst;    // ints: 2 x loff, frame-0 points | frame-0 lines
  MargSpan spare;  // the slack the sum of this layout has always had (total is part of the rule that picks mtrows)
  // ---- tenants: who else lives in a region, and when (the barriers are named in marg_body) ----
  MargSpan vlist, vinv;                 // tmp, from the gather to the last X^T X: dense dims with a visual index, and the inverse map
  MargSpan rs, lineC, rstart, rland;    // tmp behind vinv, within one staging pass: point scales, line factors, start frames, indices (ints)
  MargSpan ArmAmm;                      // tmp after the elimination: Arm Amm^-1 (n x 16)
  MargSpan Y;                           // tile after the elimination: copy of Amm, then Arm B (n x 16) on the spectral route
  MargSpan f15;                         // tile after the elimination: scratch of the 15 x 15 factorisation
  MargSpan rdiag;                       // lam between the two factorisations: reciprocal diagonal of Amm's factor
  MargSpan wgcol;                       // lam: pivot column of the work-group factorisation
  MargSpan fG;                          // Ad after the kept block has left it: scratch of the register forms
};

typedef MargSpanT<int> MargSpan;
typedef MargLayoutT<int> MargLayout;

// the carve for `mtrows` staged rows and nd = md + n dense dims from `base` on; returns its end
template <class P> VPL_LAYOUT_HD inline P marg_carve(MargLayoutT<P>& L, P base, int n, int mtrows, int md) {
  const int nn = n < 2 ? 2 : n;
  L.nd = md + n;
  P o = base;
  lds_put(L.G, o, L.EB);
  lds_put(L.Ad, o, L.nd * L.ldd);
  lds_put(L.tile, o, mtrows * MARG_ROW);
  lds_put(L.E15, o, MARG_E15_DOUBLES);
  lds_put(L.bv, o, L.nd);
  lds_put(L.tmp, o, L.nd * 16 < MARG_TMP_MIN ? MARG_TMP_MIN : L.nd * 16);
  lds_put(L.lam, o, nn + 16);
  lds_put(L.red, o, MARG_RED_DOUBLES);
  lds_put(L.perm, o, ((n < 16 ? 16 : n) + 1) / 2);
  lds_put(L.dmap, o, (L.nd + 1) / 2);
  lds_put(L.lst, o, L.loff);
  lds_put(L.spare, o, (nn + L.nd + 16) / 2 + 4 - L.perm.len - L.dmap.len);
  return o;
}

// md: the dims a window marginalises through the pseudo-inverse (MARG_MD, or 6 under MARGIN_SECOND_NEW): the regions that hold
// nd = md + n entries are carved for that nd; total and mtrows are those of md = MARG_MD, the largest, which is what the host asks
template <class P> VPL_LAYOUT_HD inline MargLayoutT<P> marg_layout_at(P base, int n, bool small, int md = MARG_MD) {
  MargLayoutT<P> L;
  L.loff = small ? 256 : 1024;
  const int nn = n < 2 ? 2 : n;
  L.ldm = nn | 1;                       // odd row stride
  L.EB = nn * L.ldm;
  L.ldd = (MARG_MD + n) | 1;
  const int fixed = (int)(marg_carve(L, base, n, 0, MARG_MD) - base);
  L.mtrows = MTROWS_MAX;
  while (L.mtrows > 32 && (size_t)(fixed + L.mtrows * MARG_ROW) * sizeof(double) > (small ? MARG_LDS_SMALL : MARG_LDS_BIG)) L.mtrows -= 32;
  L.total = (int)(marg_carve(L, base, n, L.mtrows, MARG_MD) - base);
  if (md != MARG_MD) marg_carve(L, base, n, L.mtrows, md);
  L.vlist = {L.tmp.at, MARG_VLIST_INTS / 2};
  L.vinv = {L.vlist.at + L.vlist.len, MARG_VINV_INTS / 2};
  L.rs = {L.tmp.at + MARG_ROWC, MTROWS_MAX};
  L.lineC = {L.rs.at + L.rs.len, MARG_LINEC_DOUBLES};
  L.rstart = {L.lineC.at + L.lineC.len, L.mtrows / 2};
  L.rland = {L.rstart.at + L.rstart.len, L.mtrows / 2};
  L.ArmAmm = {L.tmp.at, n * 16};
  L.Y = {L.tile.at, n * 16 < MARG_MD * MARG_MD ? MARG_MD * MARG_MD : n * 16};
  L.f15 = {L.tile.at, psd_scratch_doubles(MARG_MD, MARG_E15_LD, PSD_NMAX_AMM, false)};
  L.rdiag = {L.lam.at, MARG_MD};
  L.wgcol = {L.lam.at, n};
  L.fG = {L.Ad.at, marg_factor_scratch(n, L.ldm, small)};
  return L;
}
VPL_LAYOUT_HD inline MargLayout marg_layout(int n, bool small = false) { return marg_layout_at<int>(0, n, small); }

// Dynamic LDS (doubles) of a k_marg launch over windows that keep at most nmax dims.  Every work-group lays out for its own n,
// mtrows grows as n shrinks and k_gauge may shrink n on the device (removeLineOutlier): total is not monotone in n, and the
// maximum runs over every n, not over the sizes the host saw.
inline int marg_lds_doubles(int nmax, bool small) {
  int d = marg_layout(nmax, small).total;
  for (int n = 1; n < nmax; ++n) {
    const int t = marg_layout(n, small).total;
    if (t > d) d = t;
  }
  return d;
}

}  // namespace vpl
