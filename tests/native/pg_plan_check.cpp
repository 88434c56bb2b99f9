// Stand-alone check of csrc/pg_plan.h (no GPU), built with -fsanitize=address,undefined by tests/test_pg_plan.py: for every
// n <= 70 and random loop sets, a node's incident lists cover every edge exactly twice (once for an edge that ends at the constant
// node 0, whose list nobody gathers), the regions of the workspace and of the integer block tile without overlap, and the sizes
// are monotone in n and L.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "pg_plan.h"

using namespace vpl;

#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) { std::printf("FAILED %s (line %d, n %d, L %d)\n", #c, __LINE__, n, L); return 1; } \
  } while (0)

static int check_layout(int n, int L) {
  const PgLayout p = pg_layout(n, L);
  CHECK(p.nb == n - 1 && p.m == 4 * (n - 1) && p.LP >= 4 * L && p.LP % 16 == 0 && p.LP < 4 * L + 16 && p.E == 4 * (n - 1) + L);
  const size_t nn = n, m = p.m, E = p.E, nb = p.nb, LP = p.LP;
  const size_t off[] = {p.ctl, p.x, p.cand, p.pr, p.meas, p.er, p.eJa, p.eJb, p.ecost, p.ecand, p.emod, p.scale, p.cn, p.g, p.B, p.Lb,
                        p.yg, p.Y, p.S, p.rhs, p.z, p.delta};
  const size_t len[] = {(size_t)PG_CTL, 4 * nn, 4 * nn, 2 * nn, 4 * E, 4 * E, 16 * E, 16 * E, E, E, E, m, m, m, nb * 80, nb * 80,
                        m, m * LP, LP * LP, LP, m, m};
  size_t at = 0;
  for (size_t i = 0; i < sizeof off / sizeof off[0]; ++i) {
    CHECK(off[i] == at && off[i] % 8 == 0);   // in order, aligned, nothing between but the padding
    at = pg_up8(off[i] + len[i]);
  }
  CHECK(at == p.total);
  CHECK(p.loop_ab == 0 && p.inc_ptr == pg_up8(2 * (size_t)L) && p.inc == pg_up8(p.inc_ptr + nn + 1) && p.itotal == pg_up8(p.inc + 2 * (size_t)L));
  return 0;
}

int main() {
  std::mt19937 rng(7);
  size_t prev_total = 0;
  for (int n = 1; n <= 70; ++n) {
    {
      const int L = 0;
      const PgLayout p = pg_layout(n, 0);
      CHECK(p.total > prev_total);                      // monotone in n
      prev_total = p.total;
      size_t prevL = p.total, previ = p.itotal;
      for (int l = 1; l <= n - 1 && l <= 40; ++l) {
        const PgLayout q = pg_layout(n, l);
        CHECK(q.total >= prevL && q.itotal >= previ && q.total > p.total);   // monotone in L
        prevL = q.total; previ = q.itotal;
      }
    }
    for (int trial = 0; trial < 6; ++trial) {
      // a random loop set: every node but 0 may close onto one older node
      std::vector<int> li, la;
      for (int i = 1; i < n; ++i)
        if (rng() % 3 == 0 || trial == 5) { li.push_back(i); la.push_back(trial == 4 ? 0 : (int)(rng() % i)); }
      const int L = (int)li.size();
      if (check_layout(n, L)) return 1;
      const PgLayout p = pg_layout(n, L);
      // exact-size heap blocks: the sanitizer sees any write past the block the layout sizes
      std::vector<int> ints(p.itotal ? p.itotal : 1, -7);
      pg_fill_ints(p, li.data(), la.data(), ints.data());
      std::vector<int> seen(p.E, 0);
      for (int k = 0; k < n; ++k) {
        int sl[8];
        pg_seq_incident(n, k, sl);
        for (int u = 0; u < 8; ++u) {
          if (sl[u] < 0) continue;
          CHECK(sl[u] < 4 * p.nb);
          const int i = sl[u] / 4 + 1, j = sl[u] % 4 + 1;
          CHECK(pg_seq_valid(n, i, j) && (u < 4 ? i == k && j == u + 1 : i - j == k && j == u - 3));
          if (k >= 1) ++seen[sl[u]];
        }
        const int* ptr = ints.data() + p.inc_ptr;
        CHECK(ptr[k] <= ptr[k + 1] && ptr[k + 1] <= 2 * L);
        int last = -1;
        for (int at = ptr[k]; at < ptr[k + 1]; ++at) {
          const int ent = ints[p.inc + at], e = ent >> 1;
          CHECK(e >= 0 && e < L && ent > last);      // ascending: the order is fixed
          last = ent;
          CHECK(ints[p.loop_ab + 2 * e + (ent & 1)] == k);
          if (k >= 1) ++seen[4 * p.nb + e];
        }
      }
      CHECK(ints[p.inc_ptr] == 0 && ints[p.inc_ptr + n] == 2 * L);
      for (int s = 0; s < p.E; ++s) {
        int want;
        if (s < 4 * p.nb) {
          const int i = s / 4 + 1, j = s % 4 + 1;
          want = !pg_seq_valid(n, i, j) ? 0 : (i - j == 0 ? 1 : 2);
        } else {
          want = la[s - 4 * p.nb] == 0 ? 1 : 2;
        }
        CHECK(seen[s] == want);
      }
    }
  }
  std::printf("pg plan ok\n");
  return 0;
}
