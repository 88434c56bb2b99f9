// Host-only check of the static tables of k_lin's assembly of the packed camera Hessian (csrc/ba_asm_pattern.h;
// tests/test_asm_pattern.py builds and runs it with g++ -fsanitize=address,undefined).  k_lin stores the entries of table A (the
// pattern a fast-path window's factors can fill) for every window and those of table B (the complement) only for windows of
// the general path; everything else relies on B's entries holding zeros.  So: A and B partition the triangle, A is the set
// k_schur's Cauchy pass walks (nz_tab), no entry of B has a visual or an IMU source, and no prior a fast-path window can carry
// reaches an entry of B -- while a prior with a later frame's speed/bias does, which is why pass B exists.
#include <cstdio>
#include <set>
#include <vector>

#include "ba_asm_pattern.h"

using namespace vpl;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { if (fails < 50) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

struct Entry { int hv, im, r, c, e; };
static Entry decode(const int* d) { return {d[0] & 0xffff, d[0] >> 16, d[1] & 255, (d[1] >> 8) & 255, d[1] >> 16}; }

// cam dims of a prior's kept blocks as prep_body maps them: pose of frame fr -> 15 fr + 0..5, speed/bias -> 15 fr + 6..14,
// extrinsic -> 165..170
static void add_block(std::vector<int>& dims, int kind, int fr) {
  const int base = kind == 0 ? 15 * fr : kind == 1 ? 15 * fr + 6 : 165;
  for (int k = 0; k < (kind == 1 ? 9 : 6); ++k) dims.push_back(base + k);
}
// how many pairs of the dims fall outside the pattern
static int pairs_outside(const std::vector<int>& dims, const std::vector<char>& inA) {
  int n = 0;
  for (int a : dims)
    for (int b : dims)
      if (a >= b && !inA[tri(a, b)]) ++n;
  return n;
}

int main() {
  std::vector<int> nz, tab;
  asm_build_tables(nz, tab);
  CHECK((int)nz.size() == NZ_N);
  CHECK((int)tab.size() == 2 * NCP);
  CHECK(NZ_N + NZ_C == NCP && NZ_C == 8559);
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }

  // A and B: sorted, disjoint, together 0 .. NCP-1; every entry describes the (r, c) of its packed index
  std::vector<char> inA(NCP, 0), inB(NCP, 0);
  for (int part = 0; part < 2; ++part) {
    const int i0 = part ? NZ_N : 0, i1 = part ? NCP : NZ_N;
    int last = -1;
    for (int i = i0; i < i1; ++i) {
      const Entry t = decode(&tab[2 * i]);
      CHECK(t.e > last);
      last = t.e;
      CHECK(t.e >= 0 && t.e < NCP && t.r < NC && t.c <= t.r && tri(t.r, t.c) == t.e);
      if (t.e < 0 || t.e >= NCP) continue;
      CHECK(!inA[t.e] && !inB[t.e]);
      (part ? inB : inA)[t.e] = 1;
      int ref[2];
      lin_asm_entry(t.r, t.c, ref);
      CHECK(ref[0] == tab[2 * i] && ref[1] == tab[2 * i + 1]);
      CHECK(t.hv >= 0 && t.hv <= HV_DOUBLES && t.im >= 0 && t.im <= 11 * 120 + 10 * 225);
      CHECK(asm_in_pattern(t.r, t.c) == (part == 0));
      if (part) CHECK(t.hv == 0 && t.im == 0);   // nothing but a prior of the general path has a term there
    }
  }
  for (int e = 0; e < NCP; ++e) CHECK(inA[e] != inB[e]);

  // A is nz_tab's index set, in its order
  for (int i = 0; i < NZ_N; ++i) {
    const Entry t = decode(&tab[2 * i]);
    CHECK((nz[i] & 0x3fff) == t.e && ((nz[i] >> 14) & 255) == t.r && (nz[i] >> 22) == t.c);
  }
  // every source some entry of the triangle names is named by an entry of A (B names none): the visual and IMU terms are complete
  {
    std::set<int> hvA, imA;
    for (int i = 0; i < NZ_N; ++i) { const Entry t = decode(&tab[2 * i]); if (t.hv) hvA.insert(t.hv); if (t.im) imA.insert(t.im); }
    CHECK((int)hvA.size() == NV * (NV + 1) / 2);
    CHECK((int)imA.size() == 11 * 120 + 10 * 225);
  }

  // every prior a fast-path window can have: any subset of the 11 pose blocks, speed/bias 0 and the extrinsic
  for (int mask = 0; mask < (1 << 13); ++mask) {
    std::vector<int> dims;
    for (int f = 0; f < NF; ++f) if (mask >> f & 1) add_block(dims, 0, f);
    if (mask >> 11 & 1) add_block(dims, 1, 0);
    if (mask >> 12 & 1) add_block(dims, 2, 0);
    const int out = pairs_outside(dims, inA);
    if (out) { CHECK(out == 0); std::printf("  block mask 0x%x: %d pairs outside the pattern\n", mask, out); break; }
  }
  // ... and why pass B exists: a later frame's speed/bias block ties entries outside the pattern (each of frames 1..10)
  for (int f = 1; f < NF; ++f) {
    std::vector<int> dims;
    for (int g = 0; g < NF; ++g) add_block(dims, 0, g);
    add_block(dims, 1, 0);
    add_block(dims, 1, f);
    add_block(dims, 2, 0);
    CHECK(pairs_outside(dims, inA) > 0);
  }
  {
    std::vector<int> dims;
    add_block(dims, 0, 0);
    add_block(dims, 1, 3);
    CHECK(pairs_outside(dims, inA) > 0);
  }
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("asm pattern ok: %d pattern entries, %d complement entries\n", NZ_N, NZ_C);
  return 0;
}
