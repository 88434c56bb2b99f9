// Stand-alone check of csrc/gf_plan.h (no GPU), built with -fsanitize=address,undefined by tests/test_gf_plan.py: for every
// n <= 200 and S in 2..9 plus the default, every node is in exactly one segment or is a separator, the segments hold at most
// S - 1 nodes and lie between their separators, every one of the n - 1 couplings is counted once (inside a segment, or as a
// segment's left or right coupling), and the regions of the workspace tile without overlap.
#include <cstdio>
#include <vector>

#include "gf_plan.h"

using namespace vpl;

#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) { std::printf("FAILED %s (line %d, n %d, S %d)\n", #c, __LINE__, n, S); return 1; } \
  } while (0)

static int check(int n, int S) {
  const GfPlan p = gf_plan(n, S);
  CHECK(p.n == n && p.S == (S > n + 1 ? n + 1 : S) && p.nsep == n / p.S && p.nseg == p.nsep + 1);
  if (n < S) CHECK(p.nsep == 0);
  std::vector<int> owner(n, 0), coupling(n > 1 ? n - 1 : 0, 0);   // exact-size heap blocks: the sanitizer sees any index past them
  for (int j = 0; j < p.nsep; ++j) {
    const int s = gf_sep_node(p, j);
    CHECK(s >= 0 && s < n && gf_is_sep(p, s) && (j == 0 || s - gf_sep_node(p, j - 1) == p.S));
    ++owner[s];
  }
  int next = 0;
  for (int j = 0; j < p.nseg; ++j) {
    int a, b;
    gf_seg_bounds(p, j, a, b);
    CHECK(a == next && a <= b && b <= n && b - a <= p.S - 1);
    CHECK(j == p.nsep || b - a == p.S - 1);                 // only the last segment is ragged or empty
    CHECK(gf_seg_has_left(p, j) == (a > 0) && gf_seg_has_right(p, j) == (b < n));
    if (gf_seg_has_left(p, j)) CHECK(gf_sep_node(p, j - 1) == a - 1);
    if (gf_seg_has_right(p, j)) CHECK(gf_sep_node(p, j) == b);
    for (int k = a; k < b; ++k) { CHECK(!gf_is_sep(p, k)); ++owner[k]; }
    for (int k = a; k + 1 < b; ++k) ++coupling[k];          // O_k inside the segment
    if (a < b && gf_seg_has_left(p, j)) ++coupling[a - 1];  // O of the left separator, into the segment's first node
    if (a < b && gf_seg_has_right(p, j)) ++coupling[b - 1]; // O of the segment's last node, into the right separator
    next = b + 1;
  }
  CHECK(next == n || next == n + 1);
  for (int k = 0; k < n; ++k) CHECK(owner[k] == 1);
  for (int k = 0; k + 1 < n; ++k) CHECK(coupling[k] == 1);
  const GfLayout L = gf_layout(n, S);
  const size_t nn = n, ns = L.p.nsep, ng = L.p.nseg;
  const size_t off[] = {L.ctl, L.x, L.cand, L.meas, L.er, L.eJi, L.eJj, L.gr, L.gw, L.ecost, L.ecand, L.emod, L.scale, L.cn, L.g, L.D,
                        L.O, L.Ld, L.Lo, L.y, L.WL, L.segok, L.SD, L.SO, L.srhs, L.SLd, L.SLo, L.sy, L.sx, L.xsol, L.delta};
  const size_t len[] = {(size_t)GF_CTL, 7 * nn, 7 * nn, 7 * nn, 6 * nn, 36 * nn, 36 * nn, 3 * nn, nn, 2 * nn, 2 * nn, 2 * nn, 6 * nn,
                        6 * nn, 6 * nn, 36 * nn, 36 * nn, 36 * nn, 36 * nn, 6 * nn, 36 * nn, ng, 36 * ns, 36 * ns, 6 * ns, 36 * ns,
                        36 * ns, 6 * ns, 6 * ns, 6 * nn, 6 * nn};
  static_assert(sizeof off == sizeof len, "one length per region");
  size_t at = 0;
  for (size_t i = 0; i < sizeof off / sizeof off[0]; ++i) {
    CHECK(off[i] == at && off[i] % 8 == 0);   // in order, aligned, nothing between but the padding
    at = gf_up8(off[i] + len[i]);
  }
  CHECK(at == L.total);
  return 0;
}

int main() {
  for (int n = 1; n <= 200; ++n) {
    for (int S = 2; S <= 9; ++S)
      if (check(n, S)) return 1;
    if (check(n, GF_DEFAULT_SEGMENT)) return 1;
    if ((n >= 2 && check(n, n)) || check(n, n + 1) || check(n, GF_MAX_NODES + 1)) return 1;   // S >= n: the last node a separator, or none
  }
  {
    const int n = 4, S = 4;
    int a, b;
    const GfPlan p = gf_plan(n, S);
    gf_seg_bounds(p, 1, a, b);
    CHECK(p.nsep == 1 && gf_sep_node(p, 0) == 3 && a == 4 && b == 4);   // the first separator is also the last node
  }
  std::printf("gf plan ok\n");
  return 0;
}
