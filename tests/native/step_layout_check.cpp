// Host-only check of the LDS layouts of the step kernels (csrc/ba_step_layout.h; tests/test_step_layout.py builds and runs it
// with g++ -fsanitize=address,undefined).  For every even maxP in 2..2048, every maxL in 1..256 and both tile counts: the regions
// of each layout tile [0, total), regions of doubles start on 8 bytes and etab on 16, every tenant ends inside the region it
// borrows, and the totals are the sums the size functions held before the layouts were a carve, restated here literally: no
// dispatch moves.  The capacity rule of a context (solve_layout_fits) is the two inequalities it replaced; pairs a context
// refuses are checked for that and skipped for the rest.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "ba_pack.h"
#include "ba_step_layout.h"

using namespace vpl;

static int fails = 0;
static int maxP = 0, maxL = 0, ntc = 0;
#define CHECK(cond) do { if (!(cond)) { if (fails < 50) std::printf("FAILED %s:%d: %s  (maxP = %d, maxL = %d, ntc = %d)\n", __FILE__, __LINE__, #cond, maxP, maxL, ntc); ++fails; } } while (0)

typedef LdsSpanT<int> Span;
typedef LdsIntsT<int> Ints;
// a region as bytes [b0, b1)
struct Bytes { size_t b0, b1; };
static Bytes bytes(const Span& s) { return {(size_t)s.at * 8, (size_t)(s.at + s.len) * 8}; }
static Bytes bytes(const Ints& s) { return {(size_t)s.at * 8, (size_t)s.at * 8 + (size_t)s.n * 4}; }
static bool inside(const Span& t, const Span& host) { return t.len >= 0 && t.at >= host.at && t.at + t.len <= host.at + host.len; }
static bool before(const Span& a, const Span& b) { return a.at + a.len <= b.at; }

// regions: ordered, disjoint, without holes, from 0 to total; offsets count doubles, so a region of doubles starts on 8 bytes
static void check_tiling(const Bytes* reg, int nreg, size_t total) {
  CHECK(reg[0].b0 == 0);
  for (int i = 0; i < nreg; ++i) {
    CHECK(reg[i].b1 >= reg[i].b0 && reg[i].b0 % 8 == 0);
    if (i + 1 < nreg) CHECK(reg[i].b1 == reg[i + 1].b0);
  }
  CHECK(reg[nreg - 1].b1 == total);
}

// ---- the sums as the size functions held them ----
static size_t old_schur_smem(int maxP, int maxL, int ntc) {
  const int r1 = std::max(4 * maxP + 28 * maxL, 74 * 80 + 32);
  const int maxKS = maxP / 4 + maxL + NF + 2;
  return (size_t)(r1 + 3 * maxP + 22 * maxL + 176 + 24) * sizeof(double) + (size_t)(8 + 4 * maxKS + ntc * (ntc + 1) / 2 * 256) * sizeof(int);
}
static size_t old_chol_smem() {
  const int XROWS_A = 36, XROWS_B = 48, XLD = 80, DNAP = 6 * 7 / 2 * 256;
  return (size_t)(((XROWS_A + XROWS_B) * XLD > DNAP ? (XROWS_A + XROWS_B) * XLD : DNAP) + 3 * 176 + 2 * 96 + 256 + 24 + 96) * sizeof(double) + (8 + 128) * sizeof(int);
}
static size_t old_back_smem(int maxP, int maxL) {
  const int nfull = NC + maxP + 4 * maxL;
  return (size_t)(176 + 4 * maxL + 2 * nfull + 24) * sizeof(double) + (size_t)(maxP + maxL) * sizeof(int);
}
static size_t old_solve_smem(int maxP, int maxL) {
  const int NAP = 66 * 256;
  return (size_t)(NAP + 5 * 176 + 256 + 24) * sizeof(double) + 4 * sizeof(int) + (size_t)(maxP + maxL) * sizeof(int);
}
// the two rules vpl_ctx_create held: k_solve keeps 2 doubles per point and 18 per line behind its two staging buffers, and 4
// per point and 28 per line in the staging buffers' space
static bool old_fits(int maxP, int maxL) {
  const int NAP = 66 * 256, CROWS = 64, CW = 80;
  return !(2 * maxP + 18 * maxL > NAP - 2 * CROWS * CW) && !(4 * maxP + 28 * maxL > 2 * CROWS * CW);
}

static void check_schur() {
  const int maxKS = max_schur_ksteps(maxP, maxL);
  const SchurLayoutT<int> L = schur_layout_at<int>(0, maxP, maxL, maxKS, ntc);
  const Bytes reg[] = {bytes(L.r1), bytes(L.pS), bytes(L.pE), bytes(L.lC), bytes(L.lS), bytes(L.lE), bytes(L.lG), bytes(L.pG), bytes(L.uc),
                       bytes(L.red), bytes(L.tick), bytes(L.flag), bytes(L.pad), bytes(L.etab), bytes(L.ftab), bytes(L.spare)};
  check_tiling(reg, (int)(sizeof(reg) / sizeof(reg[0])), L.total);
  CHECK(L.total == old_schur_smem(maxP, maxL, ntc));
  CHECK(L.total == schur_lds_bytes(maxP, maxL, maxKS, ntc));
  CHECK(bytes(L.etab).b0 % 16 == 0 && L.pad.len >= 0 && L.pad.len <= 1 && L.spare.len >= 0);
  CHECK(L.pad.len == 0 && L.spare.len == 2);   // an even maxP: everything in front of etab is an even number of doubles
  // what schur_body keeps in them
  const int nlt = ntc * (ntc + 1) / 2;
  CHECK(L.pS.len >= maxP && L.pE.len >= maxP && L.pG.len >= maxP && L.lC.len >= 10 * maxL && L.lS.len >= 4 * maxL && L.lE.len >= 4 * maxL &&
        L.lG.len >= 4 * maxL);
  CHECK(L.uc.len >= 176 && L.red.len >= 17 && 2 * L.tick.len >= 1 && 2 * L.flag.len >= 1);
  CHECK(L.etab.len * 8 == maxKS * 16 && L.ftab.len * 8 == nlt * 4 * 64 * 4);
  // tenants of r1: kP | kL side by side, Cacc after them
  CHECK(inside(L.kP, L.r1) && inside(L.kL, L.r1) && before(L.kP, L.kL) && inside(L.Cacc, L.r1));
  CHECK(L.kP.len == 4 * maxP && L.kL.len == 28 * maxL && L.Cacc.len == CSQ_N && CSQ_N >= 74 * CSQ_LD);
  CHECK(L.r1.len == std::max(L.kP.len + L.kL.len, L.Cacc.len));
}

static void check_chol() {
  const CholLayoutT<int> L = chol_layout_at<int>(0);
  const Bytes reg[] = {bytes(L.XS), bytes(L.scv), bytes(L.dgv), bytes(L.ycam), bytes(L.yv), bytes(L.isd), bytes(L.Linv), bytes(L.red),
                       bytes(L.flag), bytes(L.rsL), bytes(L.spare)};
  check_tiling(reg, (int)(sizeof(reg) / sizeof(reg[0])), L.total);
  CHECK(L.total == old_chol_smem() && L.total == chol_lds_bytes());
  CHECK(L.scv.len >= 176 && L.dgv.len >= 176 && L.ycam.len >= 176 && L.yv.len >= 16 * DNT && L.isd.len >= 16 * DNT && L.Linv.len >= 256);
  CHECK(L.red.len >= 17 && 2 * L.flag.len >= 4 && L.rsL.len >= 2 * 5 * 9 && L.spare.len == 6 + 64);
  CHECK(inside(L.XA, L.XS) && inside(L.XBm, L.XS) && before(L.XA, L.XBm) && inside(L.S, L.XS));
  CHECK(L.XA.len == XROWS_A * XLD && L.XBm.len == XROWS_B * XLD && L.S.len == DNAP && DNAP == DNT * (DNT + 1) / 2 * 256 && 16 * DNT > DN);
  CHECK(XROWS_A >= 4 * 9 && XROWS_B >= 5 * 9 && XROWS_A % 4 == 0 && XROWS_B % 4 == 0 && XLD >= 5 * 16);
}

static void check_back() {
  const int nfull = step_nfull(maxP, maxL);
  const BackLayoutT<int> L = back_layout_at<int>(0, maxP, maxL, nfull);
  const Bytes reg[] = {bytes(L.uc), bytes(L.lrhs), bytes(L.lgn), bytes(L.gdelta), bytes(L.red), bytes(L.pSt), bytes(L.lSt)};
  check_tiling(reg, (int)(sizeof(reg) / sizeof(reg[0])), L.total);
  CHECK(L.total == old_back_smem(maxP, maxL) && L.total == back_lds_bytes(maxP, maxL));
  CHECK(nfull == NC + maxP + 4 * maxL);
  CHECK(L.uc.len >= 176 && L.lrhs.len >= 4 * maxL && L.lgn.len >= nfull && L.gdelta.len >= nfull && L.red.len >= 17);
  CHECK(L.pSt.n == maxP && L.lSt.n == maxL);
}

static void check_solve() {
  const int nfull = step_nfull(maxP, maxL);
  const SolveLayoutT<int> L = solve_layout_at<int>(0, maxP, maxL, nfull);
  const Bytes reg[] = {bytes(L.S), bytes(L.sc), bytes(L.dg), bytes(L.uc), bytes(L.yv), bytes(L.isd), bytes(L.Linv), bytes(L.red),
                       bytes(L.flag), bytes(L.pSt), bytes(L.lSt)};
  check_tiling(reg, (int)(sizeof(reg) / sizeof(reg[0])), L.total);
  CHECK(L.total == old_solve_smem(maxP, maxL) && L.total == solve_lds_bytes(maxP, maxL));
  CHECK(L.S.len == NAP && NAP == NT16 * (NT16 + 1) / 2 * 256 && 16 * NT16 > NC);
  CHECK(L.sc.len >= 176 && L.dg.len >= 176 && L.uc.len >= 176 && L.yv.len >= 16 * NT16 && L.isd.len >= 16 * NT16 && L.Linv.len >= 256);
  CHECK(L.red.len >= 17 && 2 * L.flag.len >= 2 && L.pSt.n == maxP && L.lSt.n == maxL);
  // the staging buffers; kP | kL end inside them (live between the scaling and the first chunk)
  CHECK(inside(L.buf0, L.S) && inside(L.buf1, L.S) && before(L.buf0, L.buf1) && L.buf0.len == CROWS * CW && L.buf1.len == CROWS * CW);
  CHECK(L.kP.at == L.buf0.at && before(L.kP, L.kL) && L.kP.len == 4 * maxP && L.kL.len == 28 * maxL);
  CHECK(L.kL.at + L.kL.len <= L.buf1.at + L.buf1.len);
  // pS .. lE behind the staging buffers, live while chunks are staged: they end inside S
  const Span* c[] = {&L.pS, &L.pE, &L.lC, &L.lS, &L.lE};
  CHECK(before(L.buf1, L.pS));
  for (int i = 0; i < 5; ++i) {
    CHECK(inside(*c[i], L.S));
    if (i + 1 < 5) CHECK(before(*c[i], *c[i + 1]));
  }
  CHECK(L.pS.len == maxP && L.pE.len == maxP && L.lC.len == 10 * maxL && L.lS.len == 4 * maxL && L.lE.len == 4 * maxL);
  // after the factorisation: lrhs | lgn | gdelta inside S
  CHECK(inside(L.lrhs, L.S) && inside(L.lgn, L.S) && inside(L.gdelta, L.S) && before(L.lrhs, L.lgn) && before(L.lgn, L.gdelta));
  CHECK(L.lrhs.len == 4 * maxL && L.lgn.len == nfull && L.gdelta.len == nfull);
}

int main() {
  check_chol();
  int accepted = 0, beyond_r1 = 0;
  for (maxP = 2; maxP <= 2048; maxP += 2)
    for (maxL = 1; maxL <= 256; ++maxL) {
      ntc = 0;
      const bool fits = solve_layout_fits(maxP, maxL);
      CHECK(fits == old_fits(maxP, maxL));
      // what vpl_ctx_create accepts: the rule above, and k_solve, k_schur (sized for ntc = 5) and k_back within 159 KiB
      const size_t lim = 159 * 1024;
      if (!fits || old_solve_smem(maxP, maxL) > lim || old_schur_smem(maxP, maxL, 5) > lim || old_back_smem(maxP, maxL) > lim) continue;
      ++accepted;
      if (4 * maxP + 28 * maxL > CSQ_N) ++beyond_r1;
      check_back();
      check_solve();
      for (ntc = 3; ntc <= 5; ntc += 2) {
        check_schur();
        const int maxKS = max_schur_ksteps(maxP, maxL);
        const size_t st = step_lds_bytes(maxP, maxL, maxKS, ntc);
        CHECK(st == std::max(std::max(schur_lds_bytes(maxP, maxL, maxKS, ntc), chol_lds_bytes()), back_lds_bytes(maxP, maxL)));
        CHECK(st == std::max(std::max(old_schur_smem(maxP, maxL, ntc), old_chol_smem()), old_back_smem(maxP, maxL)));
        CHECK(st <= lim);
      }
    }
  maxP = 200; maxL = 80; ntc = 3;
  // the benchmark shape: two work-groups of k_step share the 160 KiB of a CU, with 10 720 B to spare
  const size_t bench = step_lds_bytes(200, 80, max_schur_ksteps(200, 80), 3);
  CHECK(bench == 76560);
  CHECK(2 * bench <= 160 * 1024 && 160 * 1024 - 2 * bench == 10720);
  // the capacity of the GPU test that puts schur_body on the other side of r1
  CHECK(solve_layout_fits(60, 214) && 4 * 60 + 28 * 214 > CSQ_N && step_lds_bytes(60, 214, max_schur_ksteps(60, 214), 5) <= 159 * 1024);
  CHECK(accepted > 0 && beyond_r1 > 0);
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("step layout ok (%d capacities accepted, %d of them with kP | kL larger than the compact system)\n", accepted, beyond_r1);
  return 0;
}
