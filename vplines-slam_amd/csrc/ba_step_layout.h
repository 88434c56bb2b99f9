// LDS layouts of the trust-region step kernels, once, for the host (the size of every dispatch, the capacity rule of
// vpl_ctx_create) and the device (every pointer schur_body, chol_body, back_body of ba_step.h and solve_body of ba_solve.h use).
// Plain C++: tests/native/step_layout_check.cpp includes it without HIP and checks, for every capacity a context may have, that
// the regions of each layout tile [0, total), that every tenant stays inside the region it borrows, and that the totals are
// what the hand-written sums were.  `spare` regions are slack those sums have always had: kept, so that no dispatch moves.
#pragma once
#include "ba_layout.h"
#include "ba_limits.h"

namespace vpl {

constexpr int LDS_CAM = 176;                 // a vector over the cam dims: NC = 171 padded to 11 tiles of 16
constexpr int LDS_RED = 24;                  // reduction words of block_sum
// dims of a window: cam | inverse depths | line orth (4 each).  The layouts take it as an argument: the device has it as
// B.nfull, one scalar load; as a sum of its own it cost k_back two spilled SGPRs and k_step<3, false> 36 B of scratch.
VPL_LAYOUT_HD inline int step_nfull(int maxP, int maxL) { return NC + maxP + 4 * maxL; }

// ---- k_schur --------------------------------------------------------------------------------------------------------
constexpr int CSQ_LD = 80;                   // row stride of the compact system in k_schur's LDS
constexpr int CSQ_N = 74 * CSQ_LD + 32;      // (+ slack: adds of exact zeros for frame slots past the window land behind a row's end)

template <class P> struct SchurLayoutT {
  typedef LdsSpanT<P> Span;
  size_t total;    // bytes
  // ---- regions, in carve order ----
  Span r1;         // max(4 maxP + 28 maxL, CSQ_N): kP | kL, then Cacc
  Span pS;         // maxP      s / sqrt(A)
  Span pE;         // maxP      e = u / (s / sqrt(A))
  Span lC;         // maxL x 10 Cholesky factor of the line block, off-diagonals pre-divided
  Span lS;         // maxL x 4  jacobi scale / diagonal of C
  Span lE;         // maxL x 4  e = C^T (u ./ s)
  Span lG;         // maxL x 4  g column of X: C^-1 S g_l
  Span pG;         // maxP      g column of X: (s / sqrt(A)) g_p
  Span uc;         // 176       unscaled-space vector of gradient_ / diagonal_ (cam dims)
  Span red;        // 24
  Span tick;       // 2 ints    ticket of the flushes
  Span flag;       // 2 ints    [0] a landmark block is not positive definite
  Span pad;        // what brings etab to 16 bytes (its entries are read as int4): nothing for an even maxP
  Span etab;       // maxKS int4: the window's K-step table
  Span ftab;       // NLT x 4 x 64 ints: flush targets of the accumulator entries
  Span spare;      // 16 bytes less the pad
  // ---- tenants of r1 ----
  Span kP;         // maxP x 4: s, d, g, H_pp                     from the scaling to the landmark constants
  Span kL;         // maxL x 28: s(4), d(4), g(4), H_ll(16)       (as kP)
  Span Cacc;       // CSQ_N: the compact system as a 74 x 80 row-major square (lower part used), from the barrier behind the
                   // landmark constants ("constants complete" in schur_body) on
};

// ntc: 16-column tiles of the compact row (3 or 5); maxKS: max_schur_ksteps(maxP, maxL) of ba_pack.h
template <class P> VPL_LAYOUT_HD inline SchurLayoutT<P> schur_layout_at(P base, int maxP, int maxL, int maxKS, int ntc) {
  SchurLayoutT<P> L;
  const int nlt = ntc * (ntc + 1) / 2;
  const int kpl = 4 * maxP + 28 * maxL;
  P o = base;
  lds_put(L.r1, o, kpl > CSQ_N ? kpl : CSQ_N);
  lds_put(L.pS, o, maxP);
  lds_put(L.pE, o, maxP);
  lds_put(L.lC, o, 10 * maxL);
  lds_put(L.lS, o, 4 * maxL);
  lds_put(L.lE, o, 4 * maxL);
  lds_put(L.lG, o, 4 * maxL);
  lds_put(L.pG, o, maxP);
  lds_put(L.uc, o, LDS_CAM);
  lds_put(L.red, o, LDS_RED);
  lds_put(L.tick, o, 1);
  lds_put(L.flag, o, 1);
  const P a = lds_align16(o);
  lds_put(L.pad, o, (int)(a - o));
  lds_put(L.etab, o, 2 * maxKS);
  lds_put(L.ftab, o, nlt * 4 * 64 / 2);
  lds_put(L.spare, o, 2 - L.pad.len);
  L.total = (size_t)(o - base) * sizeof(double);
  L.kP = {L.r1.at, 4 * maxP};
  L.kL = {L.kP.at + L.kP.len, 28 * maxL};
  L.Cacc = {L.r1.at, CSQ_N};
  return L;
}

// ---- k_chol ---------------------------------------------------------------------------------------------------------
constexpr int DN = 90;                       // dense dims (rhs row = DN)
constexpr int DNT = 6;                       // 16x16 tiles per dimension of the dense system (96 >= 91)
constexpr int DNAP = DNT * (DNT + 1) / 2 * 256;   // tile-major lower storage (5376 doubles)
// The chains' X rows are stored in DENSE coordinates, five tile columns per chain: chain A tile columns 0, 1, 2, 4, 5 (dense
// 0..47, 64..95), chain B 1..5 (dense 16..95).  Columns a chain never writes stay zero.
constexpr int XLD = 80;                      // row stride of the X rows: five tile columns
constexpr int XROWS_A = 36, XROWS_B = 48;    // 4 x 9 rows ; 5 x 9 rows padded to a multiple of 4

template <class P> struct CholLayoutT {
  typedef LdsSpanT<P> Span;
  size_t total;    // bytes
  // ---- regions, in carve order ----
  Span XS;         // max((XROWS_A + XROWS_B) * XLD, DNAP): the chains' X rows, then the dense system
  Span scv;        // 176  jacobi scale of the cam dims
  Span dgv;        // 176  dogleg diagonal
  Span ycam;       // 176  solution, cam-indexed (scaled space)
  Span yv;         // 96   dense solution
  Span isd;        // 96   1 / L_jj of the dense factor
  Span Linv;       // 256  inverse of the current diagonal tile's factor
  Span red;        // 24
  Span flag;       // 8 ints: [0] failure, [1], [2] blocks finished by chain A / B
  Span rsL;        // 2 x 5 x 9: 1 / L_kk of the chains' pivot blocks (for the back-substitution)
  Span spare;      // 6 doubles and 128 ints nobody addresses
  // ---- tenants of XS ----
  Span XA;         // chain A's X rows (36 x XLD)    until the barrier "the X rows are dead" of chol_body
  Span XBm;        // chain B's behind them (48 x XLD)
  Span S;          // the dense system, tile-major lower, once the partner waves hold it in registers
};

template <class P> VPL_LAYOUT_HD inline CholLayoutT<P> chol_layout_at(P base) {
  CholLayoutT<P> L;
  constexpr int XR = (XROWS_A + XROWS_B) * XLD;
  P o = base;
  lds_put(L.XS, o, XR > DNAP ? XR : DNAP);
  lds_put(L.scv, o, LDS_CAM);
  lds_put(L.dgv, o, LDS_CAM);
  lds_put(L.ycam, o, LDS_CAM);
  lds_put(L.yv, o, 16 * DNT);
  lds_put(L.isd, o, 16 * DNT);
  lds_put(L.Linv, o, 256);
  lds_put(L.red, o, LDS_RED);
  lds_put(L.flag, o, 4);
  lds_put(L.rsL, o, 2 * 5 * 9);
  lds_put(L.spare, o, 6 + 128 / 2);
  L.total = (size_t)(o - base) * sizeof(double);
  L.XA = {L.XS.at, XROWS_A * XLD};
  L.XBm = {L.XA.at + L.XA.len, XROWS_B * XLD};
  L.S = {L.XS.at, DNAP};
  return L;
}

// ---- k_back ---------------------------------------------------------------------------------------------------------
template <class P> struct BackLayoutT {
  typedef LdsSpanT<P> Span;
  size_t total;    // bytes
  Span uc;         // 176    S_c y_c
  Span lrhs;       // 4 maxL right-hand sides of the lines
  Span lgn;        // nfull  Gauss-Newton step (scaled space)
  Span gdelta;     // nfull  step * jacobi scale
  Span red;        // 24
  LdsIntsT<P> pSt; // maxP ints (maxP is even): start frame of every point track
  LdsIntsT<P> lSt; // maxL ints: same for the lines; the layout ends with its last int
};

template <class P> VPL_LAYOUT_HD inline BackLayoutT<P> back_layout_at(P base, int maxP, int maxL, int nfull) {
  BackLayoutT<P> L;
  P o = base;
  lds_put(L.uc, o, LDS_CAM);
  lds_put(L.lrhs, o, 4 * maxL);
  lds_put(L.lgn, o, nfull);
  lds_put(L.gdelta, o, nfull);
  lds_put(L.red, o, LDS_RED);
  lds_put(L.pSt, o, maxP);
  lds_put(L.lSt, o, maxL);
  L.total = (size_t)(L.lSt.at - base) * sizeof(double) + (size_t)maxL * sizeof(int);
  return L;
}

// ---- k_solve --------------------------------------------------------------------------------------------------------
constexpr int NT16 = 11;                     // 16x16 tiles per dimension (176 >= 172)
constexpr int NTILES = NT16 * (NT16 + 1) / 2;  // lower-triangular tile count (66)
constexpr int NAP = NTILES * 256;            // tile-major lower storage of the reduced system (16896 doubles)
// Compact "vis" system used by the Schur accumulation: 72 vis dims + rhs column (72) + Cauchy
// column (73), padded to 80 = 5 tiles of 16.
constexpr int CW = 80;             // staged row width (doubles)
constexpr int CROWS = 64;          // landmark rows per staged chunk

template <class P> struct SolveLayoutT {
  typedef LdsSpanT<P> Span;
  size_t total;    // bytes
  // ---- regions, in carve order ----
  Span S;          // NAP tile-major lower (row NC = rhs)
  Span sc;         // 176 jacobi scale of cam dims
  Span dg;         // 176 dogleg diagonal of cam dims
  Span uc;         // 176 work vector (u for the Cauchy point, later S_c y_c)
  Span yv;         // 176 solution of the reduced system / z
  Span isd;        // 176 1/L_jj
  Span Linv;       // 256 inverse of the current diagonal tile's factor (swizzled tile)
  Span red;        // 24
  Span flag;       // 4 ints
  LdsIntsT<P> pSt; // maxP ints (maxP is even): start frame of every point track (column map of the compact W rows)
  LdsIntsT<P> lSt; // maxL ints: same for the lines; the layout ends with its last int
  // ---- tenants of S, each until the reduced system is written over it (solve_body names the barriers) ----
  Span buf0, buf1;         // two staging buffers of CROWS x CW landmark rows
  Span kP, kL;             // in the staging buffers' space between the scaling and the first chunk: maxP x 4, maxL x 28
  Span pS, pE, lC, lS, lE; // behind the staging buffers, while chunks are staged: maxP, maxP, maxL x 10, maxL x 4, maxL x 4
  Span lrhs, lgn, gdelta;  // after the factorisation: 4 maxL right-hand sides of the lines, nfull, nfull
};

template <class P> VPL_LAYOUT_HD inline SolveLayoutT<P> solve_layout_at(P base, int maxP, int maxL, int nfull) {
  SolveLayoutT<P> L;
  P o = base;
  lds_put(L.S, o, NAP);
  lds_put(L.sc, o, LDS_CAM);
  lds_put(L.dg, o, LDS_CAM);
  lds_put(L.uc, o, LDS_CAM);
  lds_put(L.yv, o, LDS_CAM);
  lds_put(L.isd, o, LDS_CAM);
  lds_put(L.Linv, o, 256);
  lds_put(L.red, o, LDS_RED);
  lds_put(L.flag, o, 2);
  lds_put(L.pSt, o, maxP);
  lds_put(L.lSt, o, maxL);
  L.total = (size_t)(L.lSt.at - base) * sizeof(double) + (size_t)maxL * sizeof(int);
  L.buf0 = {L.S.at, CROWS * CW};
  L.buf1 = {L.buf0.at + L.buf0.len, CROWS * CW};
  L.kP = {L.S.at, 4 * maxP};
  L.kL = {L.kP.at + L.kP.len, 28 * maxL};
  L.pS = {L.buf1.at + L.buf1.len, maxP};
  L.pE = {L.pS.at + L.pS.len, maxP};
  L.lC = {L.pE.at + L.pE.len, 10 * maxL};
  L.lS = {L.lC.at + L.lC.len, 4 * maxL};
  L.lE = {L.lS.at + L.lS.len, 4 * maxL};
  L.lrhs = {L.S.at, 4 * maxL};
  L.lgn = {L.lrhs.at + L.lrhs.len, nfull};
  L.gdelta = {L.lgn.at + L.lgn.len, nfull};
  return L;
}
static_assert(2 * CROWS * CW <= NAP, "the two staging buffers alias the reduced-system storage");

// ---- what the host asks ---------------------------------------------------------------------------------------------
template <class P> VPL_LAYOUT_HD inline bool lds_ends_inside(const LdsSpanT<P>& t, P host_end) { return t.at + t.len <= host_end; }

// The capacity rule of a context: every tenant of k_solve's S ends inside the region it borrows -- kP | kL inside the two
// staging buffers, pS .. lE inside S behind them, lrhs | lgn | gdelta inside S.
inline bool solve_layout_fits(int maxP, int maxL) {
  const SolveLayoutT<int> L = solve_layout_at<int>(0, maxP, maxL, step_nfull(maxP, maxL));
  return lds_ends_inside(L.kL, L.buf1.at + L.buf1.len) && lds_ends_inside(L.lE, L.S.at + L.S.len) &&
         lds_ends_inside(L.gdelta, L.S.at + L.S.len);
}

inline size_t schur_lds_bytes(int maxP, int maxL, int maxKS, int ntc) { return schur_layout_at<int>(0, maxP, maxL, maxKS, ntc).total; }
inline size_t chol_lds_bytes() { return chol_layout_at<int>(0).total; }
inline size_t back_lds_bytes(int maxP, int maxL) { return back_layout_at<int>(0, maxP, maxL, step_nfull(maxP, maxL)).total; }
inline size_t solve_lds_bytes(int maxP, int maxL) { return solve_layout_at<int>(0, maxP, maxL, step_nfull(maxP, maxL)).total; }
// k_step runs the three bodies in one LDS block: the largest of their layouts
inline size_t step_lds_bytes(int maxP, int maxL, int maxKS, int ntc) {
  const size_t a = schur_lds_bytes(maxP, maxL, maxKS, ntc), b = chol_lds_bytes(), c = back_lds_bytes(maxP, maxL);
  return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

}  // namespace vpl
