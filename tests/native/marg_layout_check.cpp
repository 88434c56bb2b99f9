// Host-only check of k_marg's LDS layout (csrc/ba_marg_layout.h; tests/test_marg_layout.py builds and runs it with
// g++ -fsanitize=address,undefined).  For every kept size 0..MAXKEEP and both forms of the kernel: the regions tile [0, total),
// the int arrays hold what marg_body writes into them, every tenant ends inside the region it borrows, the scratch each
// factorisation asks for in its signature comment fits where marg_body puts it, and the dispatch (marg_lds_doubles) covers the
// layout of every window it may meet.  The sum the layout had before it was a carve is restated here: total must not move,
// it is part of the rule that picks mtrows.
#include <cstdio>
#include <cstdlib>

#include "ba_marg_layout.h"

using namespace vpl;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s  (n = %d, small = %d)\n", __FILE__, __LINE__, #cond, n, (int)small); ++fails; } } while (0)

static bool inside(const MargSpan& t, const MargSpan& host) { return t.len >= 0 && t.at >= host.at && t.at + t.len <= host.at + host.len; }
static bool before(const MargSpan& a, const MargSpan& b) { return a.at + a.len <= b.at; }

// the layout's size as marg_layout summed it up to now
static int old_total(int n, bool small) {
  const int loff = small ? 256 : 1024;
  const int nn = n < 2 ? 2 : n;
  const int EB = nn * (nn | 1), nd = 15 + n, ldd = nd | 1;
  const int fixed = EB + nd * ldd + 16 * 17 + nd + (nd * 16 < 640 ? 640 : nd * 16) + nn + 16 + 24 + (nn + nd + 2 * loff + 16) / 2 + 4;
  int mtrows = 96;
  while (mtrows > 32 && (size_t)(fixed + mtrows * 74) * 8 > (small ? (size_t)79 * 1024 : (size_t)150 * 1024)) mtrows -= 32;
  return fixed + mtrows * 74;
}

static void check_layout(const int n, const bool small) {
  const MargLayout L = marg_layout(n, small);
  // regions: ordered, disjoint, without holes, from 0 to total.  Offsets are counted in doubles: 8-byte aligned by construction.
  const MargSpan* reg[] = {&L.G, &L.Ad, &L.tile, &L.E15, &L.bv, &L.tmp, &L.lam, &L.red, &L.perm, &L.dmap, &L.lst, &L.spare};
  const int nreg = (int)(sizeof(reg) / sizeof(reg[0]));
  CHECK(reg[0]->at == 0);
  for (int i = 0; i < nreg; ++i) {
    CHECK(reg[i]->len > 0 || (reg[i] == &L.spare && reg[i]->len >= 0));
    if (i + 1 < nreg) CHECK(reg[i]->at + reg[i]->len == reg[i + 1]->at);
  }
  CHECK(L.spare.at + L.spare.len == L.total);
  CHECK(L.total == old_total(n, small));
  CHECK(L.mtrows == 32 || L.mtrows == 64 || L.mtrows == 96);
  // MARGIN_SECOND_NEW (6 + n dense dims): the same regions, none larger, inside the same total
  {
    const MargLayout S = marg_layout_at<int>(0, n, small, 6);
    CHECK(S.total == L.total && S.mtrows == L.mtrows && S.ldd == L.ldd && S.nd == 6 + n);
    CHECK(S.spare.len >= 0 && S.spare.at + S.spare.len <= L.total);
    CHECK(S.Ad.len == S.nd * S.ldd && S.bv.len == S.nd && 2 * S.dmap.len >= S.nd && S.tmp.len >= S.nd * 16 && S.tmp.len >= MARG_TMP_MIN);
    CHECK(2 * S.perm.len >= (n < 16 ? 16 : n) && S.lst.len == L.lst.len && S.tile.len == L.tile.len);
    CHECK(S.fG.at == S.Ad.at && S.fG.len <= S.Ad.len);
  }
  // what marg_body keeps in them (nd = 15 + n is the larger of its two cases)
  const int nd = MARG_MD + n, nn = n < 2 ? 2 : n;
  CHECK(L.nd == nd && L.ldd >= nd && L.ldm >= nn);
  CHECK(L.G.len >= nn * L.ldm);
  CHECK(L.Ad.len >= nd * L.ldd);
  CHECK(L.tile.len == L.mtrows * MARG_ROW && MARG_ROW >= 73);
  CHECK(L.E15.len >= MARG_MD * MARG_E15_LD && MARG_E15_LD >= MARG_MD);
  CHECK(L.bv.len >= nd);
  CHECK(L.red.len >= 1);
  CHECK(2 * L.perm.len >= (n < 16 ? 16 : n));
  CHECK(2 * L.dmap.len >= nd);
  CHECK(2 * L.lst.len == 2 * L.loff);
  // tenants of tmp: vlist | vinv, and beside them rs | lineC | rstart | rland -- all live together during the elimination
  CHECK(inside(L.vlist, L.tmp) && inside(L.vinv, L.tmp) && inside(L.rs, L.tmp) && inside(L.lineC, L.tmp) && inside(L.rstart, L.tmp) &&
        inside(L.rland, L.tmp));
  CHECK(before(L.vlist, L.vinv) && before(L.vinv, L.rs) && before(L.rs, L.lineC) && before(L.lineC, L.rstart) && before(L.rstart, L.rland));
  CHECK(2 * L.vlist.len >= nd && 2 * L.vinv.len >= 72);
  CHECK(L.rs.len >= L.mtrows && L.lineC.len >= 10 * (L.mtrows / 4) && 2 * L.rstart.len >= L.mtrows && 2 * L.rland.len >= L.mtrows);
  CHECK(inside(L.ArmAmm, L.tmp) && L.ArmAmm.len >= n * 16);
  // tenants of tile
  CHECK(inside(L.Y, L.tile) && L.Y.len >= n * 16 && L.Y.len >= MARG_MD * MARG_MD);
  CHECK(inside(L.f15, L.tile));
  CHECK(L.f15.len == MARG_MD * MARG_E15_LD + 16);                      // psd_pivoted_cholesky_wave<16>: n x ld + NMAX
  // tenants of lam
  CHECK(inside(L.rdiag, L.lam) && L.rdiag.len >= MARG_MD);
  CHECK(inside(L.wgcol, L.lam) && L.wgcol.len >= n);                   // psd_pivoted_cholesky: n doubles
  CHECK(L.lam.len >= MARG_MD);                                         // the eigenvalues of the spectral route
  // Ad as the scratch of the form marg_factor_kept picks
  CHECK(inside(L.fG, L.Ad));
  if (n <= 48) CHECK(L.fG.len == n * L.ldm + 48);                      // wave<48>: n x ld + NMAX
  else if (!small && n <= 76) CHECK(L.fG.len == n * L.ldm + 76 + 24);  // wave4<19, 4>: n x ld + NMAX + 24
  else CHECK(L.fG.len == 0);
}

int main() {
  for (int small = 0; small < 2; ++small)
    for (int n = 0; n <= MAXKEEP; ++n) check_layout(n, small != 0);
  // the dispatch covers every window of the batch, and every window the device may shrink
  for (int small = 0; small < 2; ++small)
    for (int nmax = 0; nmax <= MAXKEEP; ++nmax) {
      const int d = marg_lds_doubles(nmax, small != 0);
      for (int n = 0; n <= nmax; ++n) CHECK(d >= marg_layout(n, small != 0).total);
      const size_t bytes = (size_t)d * sizeof(double);
      const int n = nmax;
      // choose_marg's acceptance: the 256-thread form for nmax <= 48 that fit MARG_LDS_SMALL, anything up to MARG_LDS_MAX
      if (small && nmax <= 48 && bytes <= MARG_LDS_SMALL)
        for (int k = 0; k <= nmax; ++k) CHECK((size_t)marg_layout(k, true).total * sizeof(double) <= MARG_LDS_SMALL);
      if (bytes <= MARG_LDS_MAX)
        for (int k = 0; k <= nmax; ++k) CHECK((size_t)marg_layout(k, small != 0).total * sizeof(double) <= 159 * 1024);
    }
  {
    // the figures of the change: the windows a dispatch sized for the batch's largest kept size alone did not cover ...
    const int n = 0;
    const bool small = false;
    CHECK(marg_layout(39, true).total * 8 == 67536 && marg_layout(33, true).total * 8 == 77168);
    CHECK(marg_layout(69, false).total * 8 == 137520 && marg_layout(57, false).total * 8 == 146416 && marg_layout(63, false).total * 8 == 141392);
    CHECK(marg_lds_doubles(39, true) * 8 >= 77168 && marg_lds_doubles(69, false) * 8 >= 146416);
    // ... the benchmark's k_marg<256> (n = 45) still below MARG_LDS_SMALL, the steady state's k_marg<512> (n = 75) as it was
    CHECK(marg_layout(45, true).total * 8 == 78000 && marg_lds_doubles(45, true) * 8 == 80408 && MARG_LDS_SMALL == 80896);
    CHECK(marg_layout(75, false).total * 8 == 153744 && marg_lds_doubles(75, false) * 8 == 153744);
    // no batch changes its form or is newly refused: the larger dispatch passes the limits wherever the batch's own layout did
    for (int nmax = 0; nmax <= MAXKEEP; ++nmax) {
      CHECK(((size_t)marg_lds_doubles(nmax, true) * 8 <= MARG_LDS_SMALL) == ((size_t)old_total(nmax, true) * 8 <= MARG_LDS_SMALL) || nmax > 48);
      CHECK(((size_t)marg_lds_doubles(nmax, false) * 8 <= MARG_LDS_MAX) == ((size_t)old_total(nmax, false) * 8 <= MARG_LDS_MAX));
    }
    CHECK((size_t)marg_lds_doubles(76, false) * 8 <= MARG_LDS_MAX);   // every size the column-slice factorisation takes
  }
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("marg layout ok\n");
  return 0;
}
