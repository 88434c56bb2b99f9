// Plan of one pose chain of the global fusion (vpl_gf_optimize_batch): which nodes are separators, the segments between them, and
// the layout of the chain's workspace.  A function of (n, S) only.  Plain C++ for the host, which sizes the dispatch from it, and
// for the device, which takes every index from it; tests/native/gf_plan_check.cpp walks it under the sanitizers.
//
// Nodes 0 .. n-1 in time order, every node an unknown block of six columns (dtheta, dt).  Node k is a separator when
// k % S == S - 1: separator j is node j S + S - 1, there are n / S of them.  Segment j = the nodes [j S, min(j S + S - 1, n)), at
// most S - 1 of them, between separator j - 1 (none for j = 0) and separator j (none for the last segment, j = n / S, which is
// empty when S divides n).  n < S: one segment, no separator -- the serial chain.
// The normal matrix is block-tridiagonal: D_k on the diagonal, O_k = block (k + 1, k) below it, so a segment's interior couples
// to its left separator through O of the separator (into the segment's first node) and to its right separator through O of its
// last node; each of the n - 1 couplings belongs to exactly one of: the interior of a segment, its left or its right coupling.
#pragma once
#include <cstddef>

#ifdef __HIPCC__
#define GF_HD __host__ __device__ __forceinline__
#else
#define GF_HD inline
#endif

namespace vpl {

constexpr int GF_MAX_NODES = 65536;
constexpr int GF_DEFAULT_SEGMENT = 64;   // (measured against 32 and 128: DESIGN.md, "Global fusion")
constexpr int GF_CTL = 32;               // doubles of the control block
constexpr int GF_HEAD = 24;              // doubles of the result head

struct GfPlan { int n, S, nsep, nseg; };

// S >= 2; an S beyond n + 1 gives the plan of n + 1
GF_HD GfPlan gf_plan(int n, int S) {
  GfPlan p;
  p.n = n; p.S = S > n + 1 ? n + 1 : S; p.nsep = n / p.S; p.nseg = p.nsep + 1;
  return p;
}
GF_HD int gf_sep_node(const GfPlan& p, int j) { return j * p.S + p.S - 1; }
GF_HD bool gf_is_sep(const GfPlan& p, int k) { return k % p.S == p.S - 1; }
// the interior nodes [a, b) of segment j
GF_HD void gf_seg_bounds(const GfPlan& p, int j, int& a, int& b) {
  a = j * p.S;
  b = a + p.S - 1 < p.n ? a + p.S - 1 : p.n;
}
GF_HD bool gf_seg_has_left(const GfPlan&, int j) { return j > 0; }
GF_HD bool gf_seg_has_right(const GfPlan& p, int j) { return j < p.nsep; }

struct GfLayout {
  GfPlan p;
  // offsets in doubles from the chain's workspace
  size_t ctl, x, cand, meas, er, eJi, eJj, gr, gw, ecost, ecand, emod, scale, cn, g, D, O, Ld, Lo, y, WL, segok, SD, SO, srhs, SLd,
      SLo, sy, sx, xsol, delta, total;
};

GF_HD size_t gf_up8(size_t v) { return (v + 7) & ~(size_t)7; }

inline GfLayout gf_layout(int n, int S) {
  GfLayout L{};
  L.p = gf_plan(n, S);
  size_t at = 0;
  auto take = [&at](size_t count) { const size_t o = at; at = gf_up8(at + count); return o; };
  const size_t n_ = (size_t)n, ns = (size_t)L.p.nsep, ng = (size_t)L.p.nseg;
  L.ctl = take(GF_CTL);
  L.x = take(7 * n_); L.cand = take(7 * n_); L.meas = take(7 * n_);
  L.er = take(6 * n_); L.eJi = take(36 * n_); L.eJj = take(36 * n_); L.gr = take(3 * n_); L.gw = take(n_);
  L.ecost = take(2 * n_); L.ecand = take(2 * n_); L.emod = take(2 * n_);
  L.scale = take(6 * n_); L.cn = take(6 * n_); L.g = take(6 * n_);
  L.D = take(36 * n_); L.O = take(36 * n_); L.Ld = take(36 * n_); L.Lo = take(36 * n_); L.y = take(6 * n_); L.WL = take(36 * n_);
  L.segok = take(ng);
  L.SD = take(36 * ns); L.SO = take(36 * ns); L.srhs = take(6 * ns); L.SLd = take(36 * ns); L.SLo = take(36 * ns);
  L.sy = take(6 * ns); L.sx = take(6 * ns);
  L.xsol = take(6 * n_); L.delta = take(6 * n_);
  L.total = at;
  return L;
}

}  // namespace vpl
