// Plan of one pose graph (vpl_pg_optimize_batch): the edge slots, the fixed order in which a node gathers its incident edges, and
// the layout of the graph's workspace.  Plain C++ for the host, which builds it, sizes the dispatch and packs it, and for the
// device, which takes every offset from it; tests/native/pg_plan_check.cpp walks it under the sanitizers.
//
// Nodes 0 .. n-1; node 0 is constant, node k >= 1 is unknown block k-1 of four columns (yaw, tx, ty, tz).
// Edge slots: the sequential edge between node i and node i-j (j = 1..4) has slot 4 (i-1) + (j-1), valid when i-j >= 0; loop edge e
// has slot 4 (n-1) + e.  Every edge has an earlier end a and a later end b.
// A node gathers, in this order: the sequential edges it ends (j = 1..4), the sequential edges it starts (j = 1..4), its loop
// edges in the order of the node's list (ascending edge number; the end it is of each edge travels with the entry).
#pragma once
#include <cstddef>

#ifdef __HIPCC__
#define PG_HD __host__ __device__ __forceinline__
#else
#define PG_HD inline
#endif

namespace vpl {

constexpr int PG_MAX_NODES = 4096, PG_MAX_LOOPS = 256;
constexpr int PG_BW = 4;             // half-bandwidth of B in blocks
constexpr int PG_CTL = 32;           // doubles of the control block
constexpr int PG_HEAD = 24;          // doubles of the result head

PG_HD int pg_seq_slot(int i, int j) { return 4 * (i - 1) + (j - 1); }
PG_HD bool pg_seq_valid(int n, int i, int j) { return i >= 1 && i < n && j >= 1 && j <= PG_BW && i - j >= 0; }
// the sequential slots node k gathers: out[0..3] the edges it ends (as b), out[4..7] the edges it starts (as a); -1 where there is none
PG_HD void pg_seq_incident(int n, int k, int out[8]) {
  for (int j = 1; j <= PG_BW; ++j) {
    out[j - 1] = pg_seq_valid(n, k, j) ? pg_seq_slot(k, j) : -1;
    out[PG_BW + j - 1] = pg_seq_valid(n, k + j, j) ? pg_seq_slot(k + j, j) : -1;
  }
}

struct PgLayout {
  int n, L, nb, m, LP, E;
  // offsets in doubles from the graph's workspace
  size_t ctl, x, cand, pr, meas, er, eJa, eJb, ecost, ecand, emod, scale, cn, g, B, Lb, yg, Y, S, rhs, z, delta, total;
  // offsets in ints from the graph's integer block: the two ends of every loop edge, the start of every node's loop list, the lists
  size_t loop_ab, inc_ptr, inc, itotal;
};

PG_HD size_t pg_up8(size_t v) { return (v + 7) & ~(size_t)7; }

inline PgLayout pg_layout(int n, int L) {
  PgLayout p{};
  p.n = n; p.L = L; p.nb = n - 1; p.m = 4 * p.nb; p.LP = (4 * L + 15) & ~15; p.E = 4 * p.nb + L;
  size_t at = 0;
  auto take = [&at](size_t count) { const size_t o = at; at = pg_up8(at + count); return o; };
  const size_t n_ = (size_t)n, m = (size_t)p.m, E = (size_t)p.E, nb = (size_t)p.nb, LP = (size_t)p.LP;
  p.ctl = take(PG_CTL);
  p.x = take(4 * n_); p.cand = take(4 * n_); p.pr = take(2 * n_);
  p.meas = take(4 * E); p.er = take(4 * E); p.eJa = take(16 * E); p.eJb = take(16 * E);
  p.ecost = take(E); p.ecand = take(E); p.emod = take(E);
  p.scale = take(m); p.cn = take(m); p.g = take(m);
  p.B = take(nb * (PG_BW + 1) * 16); p.Lb = take(nb * (PG_BW + 1) * 16);
  p.yg = take(m); p.Y = take(m * LP); p.S = take(LP * LP); p.rhs = take(LP); p.z = take(m); p.delta = take(m);
  p.total = at;
  size_t it = 0;
  auto itake = [&it](size_t count) { const size_t o = it; it = pg_up8(it + count); return o; };
  p.loop_ab = itake(2 * (size_t)L); p.inc_ptr = itake(n_ + 1); p.inc = itake(2 * (size_t)L);
  p.itotal = it;
  return p;
}

// fills the integer block from the loop list (node i, old node a < i per edge, edges in ascending order of i as the caller's nodes
// give them): entry of a node's list = 2 edge + end (0: the node is the edge's a, 1: its b)
inline void pg_fill_ints(const PgLayout& p, const int* loop_i, const int* loop_a, int* ints) {
  int* ab = ints + p.loop_ab;
  int* ptr = ints + p.inc_ptr;
  int* inc = ints + p.inc;
  for (int k = 0; k <= p.n; ++k) ptr[k] = 0;
  for (int e = 0; e < p.L; ++e) { ab[2 * e] = loop_a[e]; ab[2 * e + 1] = loop_i[e]; ++ptr[loop_a[e] + 1]; ++ptr[loop_i[e] + 1]; }
  for (int k = 0; k < p.n; ++k) ptr[k + 1] += ptr[k];
  for (int k = 0; k < p.n; ++k) {
    int at = ptr[k];
    for (int e = 0; e < p.L; ++e) {
      if (loop_a[e] == k) inc[at++] = 2 * e;
      if (loop_i[e] == k) inc[at++] = 2 * e + 1;
    }
  }
}

// ---- several sequences (vpl_pg_optimize_seq_batch; pose_graph.cpp:447-519).  One int per node:
// PG_NODE_CONST0: the node is local node 0 or of sequence 0 (:473-477).  Bit j = 1..4: the sequential edge (k, k-j) is part of the
// problem -- both ends of one sequence (:482) and not both PG_NODE_CONST0.  A loop edge is part of the problem unless both its
// ends are PG_NODE_CONST0.  PG_NODE_CONST: the node is not an unknown -- it is PG_NODE_CONST0, or no edge of the problem touches it
// (ceres drops an unused parameter block from the reduced program).  sequence == nullptr: every node is of sequence 1.
constexpr int PG_NODE_CONST = 1, PG_NODE_CONST0 = 1 << 5;

inline void pg_node_flags(int n, const int* sequence, int L, const int* loop_i, const int* loop_a, int* flags) {
  auto seq = [sequence](int k) { return sequence ? sequence[k] : 1; };
  auto const0 = [&seq](int k) { return k == 0 || seq(k) == 0; };
  for (int k = 0; k < n; ++k) flags[k] = const0(k) ? PG_NODE_CONST0 : 0;
  // (bit 6 marks a node some edge of the problem touches; it is cleared again below)
  constexpr int touched = 1 << 6;
  for (int k = 1; k < n; ++k)
    for (int j = 1; j <= PG_BW && k - j >= 0; ++j)
      if (seq(k) == seq(k - j) && !(const0(k) && const0(k - j))) { flags[k] |= (1 << j) | touched; flags[k - j] |= touched; }
  for (int e = 0; e < L; ++e)
    if (!(const0(loop_i[e]) && const0(loop_a[e]))) { flags[loop_i[e]] |= touched; flags[loop_a[e]] |= touched; }
  for (int k = 0; k < n; ++k) {
    if ((flags[k] & PG_NODE_CONST0) || !(flags[k] & touched)) flags[k] |= PG_NODE_CONST;
    flags[k] &= ~touched;
  }
}

}  // namespace vpl
