// Stand-alone check of csrc/pgs_plan.h (no GPU), built with -fsanitize=address,undefined by tests/test_pgs_plan.py: random scripts
// of add / load / loop / optimise / reset go through the plan and through a naive model that follows PoseGraph's own text -- a
// queue that is drained to its last entry, a sequence_loop vector, a scan for the earliest loop -- and after every step the two
// agree: the sequence rule, sequence_loop, earliest_loop_index, the last-queued rule, the range and loop lists of an
// optimisation, and the refusals, which leave the state alone.  Then the node flags of pg_plan.h against their definition.
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <random>
#include <vector>

#include "pgs_plan.h"

using namespace vpl;

#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) { std::printf("FAILED %s (line %d, script %d, step %d)\n", #c, __LINE__, script, step); return 1; } \
  } while (0)

struct Model {
  int cap;
  int sequence_cnt = 0, earliest = -1;
  std::vector<int> sequence_loop{0}, seq, loop;
  std::queue<int> buf;
};

static bool same(const PgsPlan& p, const Model& m) {
  if (p.size() != (int)m.seq.size() || p.sequence_cnt != m.sequence_cnt || p.earliest_loop_index != m.earliest) return false;
  if (p.sequence_loop != m.sequence_loop || p.seq != m.seq || p.loop_index != m.loop) return false;
  return (p.pending < 0) == m.buf.empty() && (m.buf.empty() || p.pending == m.buf.back());
}

static int run_scripts() {
  std::mt19937 rng(11);
  int step = 0;
  for (int script = 0; script < 400; ++script) {
    const int cap = 1 + (int)(rng() % 60);
    PgsPlan p;
    p.cap = cap;
    Model m;
    m.cap = cap;
    const int steps = 20 + (int)(rng() % 120);
    for (step = 0; step < steps; ++step) {
      const int what = (int)(rng() % 100);
      const int size = (int)m.seq.size();
      if (what < 55) {   // add: mostly a legal sequence, sometimes not; mostly no loop, sometimes a legal one, sometimes not
        int sequence = m.sequence_cnt + (rng() % 8 == 0 ? 1 : 0);
        if (m.sequence_cnt == 0) sequence = 1;
        if (rng() % 12 == 0) sequence = (int)(rng() % 6) - 1;
        int loop = -1;
        if (rng() % 4 == 0 && size > 0) loop = (int)(rng() % size);
        if (rng() % 15 == 0) loop = size + (int)(rng() % 3) - (rng() % 2 ? 0 : size + 2);
        const PgsPlan before = p;
        PgsAddStep st;
        const int rc = pgs_add(p, sequence, loop, st);
        const bool bad_seq = sequence < 1 || (sequence != m.sequence_cnt && sequence != m.sequence_cnt + 1);
        const bool bad_loop = loop < -1 || loop >= size;
        if (bad_seq || bad_loop) { CHECK(rc == PGS_INVALID); }
        else if (size >= cap) { CHECK(rc == PGS_CAPACITY); }
        else {
          CHECK(rc == PGS_OK && st.index == size);
          bool new_seq = false, shift = false;
          if (m.sequence_cnt != sequence) { ++m.sequence_cnt; m.sequence_loop.push_back(0); new_seq = true; }
          if (loop != -1) {
            if (m.earliest > loop || m.earliest == -1) m.earliest = loop;
            if (m.seq[loop] != sequence && m.sequence_loop[sequence] == 0) { shift = true; m.sequence_loop[sequence] = 1; }
            m.buf.push(size);
          }
          m.seq.push_back(sequence); m.loop.push_back(loop);
          CHECK(st.new_sequence == (new_seq ? 1 : 0) && st.shift_list == (shift ? 1 : 0));
        }
        if (rc != PGS_OK) {
          CHECK(before.seq == p.seq && before.loop_index == p.loop_index && before.sequence_loop == p.sequence_loop);
          CHECK(before.sequence_cnt == p.sequence_cnt && before.pending == p.pending && before.earliest_loop_index == p.earliest_loop_index);
        }
      } else if (what < 70) {   // load
        int loop = -1;
        if (rng() % 3 == 0 && size > 0) loop = (int)(rng() % size);
        if (rng() % 10 == 0) loop = size + (int)(rng() % 2);
        int index = -7;
        const int rc = pgs_load(p, loop, index);
        if (loop >= size) { CHECK(rc == PGS_INVALID && index == -7); }
        else if (size >= cap) { CHECK(rc == PGS_CAPACITY && index == -7); }
        else {
          CHECK(rc == PGS_OK && index == size);
          if (loop != -1) {
            if (m.earliest > loop || m.earliest == -1) m.earliest = loop;
            m.buf.push(size);
          }
          m.seq.push_back(0); m.loop.push_back(loop);
        }
      } else if (what < 95) {   // optimise
        int first = -5, cur = -5;
        std::vector<int> li{-9}, la{-9};
        const int rc = pgs_take(p, first, cur, li, la);
        int mc = -1, mf = -1;
        while (!m.buf.empty()) { mc = m.buf.front(); mf = m.earliest; m.buf.pop(); }
        if (mc == -1) { CHECK(rc == 0 && first == -5 && cur == -5 && li.size() == 1); }
        else {
          CHECK(rc == 1 && first == mf && cur == mc && li.size() == la.size());
          size_t e = 0;
          for (int k = mf; k <= mc; ++k)
            if (m.loop[k] >= 0) { CHECK(e < li.size() && li[e] == k - mf && la[e] == m.loop[k] - mf && la[e] >= 0 && la[e] < li[e]); ++e; }
          CHECK(e == li.size());
        }
      } else {   // reset
        pgs_reset(p);
        m = Model();
        m.cap = cap;
        CHECK(p.cap == cap);
      }
      CHECK(same(p, m));
    }
  }
  // the capacity of one optimisation: the range and the loops; a refusal keeps the queue
  {
    const int script = -1;
    PgsPlan p;
    p.cap = PG_MAX_NODES + 10;
    PgsAddStep st;
    for (int k = 0; k < PG_MAX_NODES; ++k) CHECK(pgs_add(p, 1, -1, st) == PGS_OK);
    CHECK(pgs_add(p, 1, 0, st) == PGS_OK);   // 4097 nodes in the range
    int first = -5, cur = -5;
    std::vector<int> li, la;
    CHECK(pgs_take(p, first, cur, li, la) == PGS_CAPACITY && p.pending == PG_MAX_NODES && first == -5 && li.empty());
    pgs_reset(p);
    for (int k = 0; k < PG_MAX_LOOPS + 2; ++k) CHECK(pgs_add(p, 1, k ? k - 1 : -1, st) == PGS_OK);
    CHECK(pgs_take(p, first, cur, li, la) == PGS_CAPACITY && p.pending == PG_MAX_LOOPS + 1);
    pgs_reset(p);
    for (int k = 0; k < PG_MAX_LOOPS + 1; ++k) CHECK(pgs_add(p, 1, k ? k - 1 : -1, st) == PGS_OK);
    CHECK(pgs_take(p, first, cur, li, la) == 1 && (int)li.size() == PG_MAX_LOOPS && first == 0 && cur == PG_MAX_LOOPS && p.pending == -1);
  }
  return 0;
}

static int check_flags() {
  std::mt19937 rng(13);
  int step = 0;
  for (int script = 0; script < 600; ++script) {
    const int n = 1 + (int)(rng() % 40);
    std::vector<int> seq(n), li, la;
    int s = (int)(rng() % 3);
    for (int k = 0; k < n; ++k) { if (rng() % 4 == 0) s = (int)(rng() % 4); seq[k] = s; }
    for (int k = 1; k < n; ++k)
      if (rng() % 5 == 0) { li.push_back(k); la.push_back((int)(rng() % k)); }
    const bool null_seq = rng() % 7 == 0;
    std::vector<int> fl(n, -1);
    pg_node_flags(n, null_seq ? nullptr : seq.data(), (int)li.size(), li.data(), la.data(), fl.data());
    auto sq = [&](int k) { return null_seq ? 1 : seq[k]; };
    auto c0 = [&](int k) { return k == 0 || sq(k) == 0; };
    std::vector<int> touched(n, 0);
    for (step = 0; step < n; ++step) {
      const int k = step;
      CHECK(((fl[k] & PG_NODE_CONST0) != 0) == c0(k));
      for (int j = 1; j <= PG_BW; ++j) {
        const bool act = k - j >= 0 && sq(k) == sq(k - j) && !(c0(k) && c0(k - j));
        CHECK((((fl[k] >> j) & 1) != 0) == act);
        if (act) { touched[k] = 1; touched[k - j] = 1; }
      }
      CHECK((fl[k] & ~(PG_NODE_CONST | PG_NODE_CONST0 | 30)) == 0);
    }
    for (size_t e = 0; e < li.size(); ++e)
      if (!(c0(li[e]) && c0(la[e]))) { touched[li[e]] = 1; touched[la[e]] = 1; }
    for (step = 0; step < n; ++step) CHECK(((fl[step] & PG_NODE_CONST) != 0) == (c0(step) || !touched[step]));
  }
  return 0;
}

int main() {
  if (run_scripts()) return 1;
  if (check_flags()) return 1;
  std::printf("pgs plan ok\n");
  return 0;
}
