// Host bookkeeping of the pose-graph session (vpl_pgs_*; DESIGN.md, "Pose-graph session"): what PoseGraph keeps in integers --
// global_index, sequence_cnt, sequence_loop, earliest_loop_index, the optimisation queue, and per keyframe its sequence and its
// loop -- with the decisions addKeyFrame / loadKeyFrame / optimize4DoF take from them (pose_graph.cpp:42-136, :213-287, :407-417).
// The doubles live on the device (pgs_kernels.h).  Plain C++, no HIP: tests/native/pgs_plan_check.cpp runs random scripts
// through it against a naive model under the sanitizers.  A refused step leaves the plan as it was.
#pragma once
#include <vector>

#include "pg_plan.h"

namespace vpl {

constexpr int PGS_OK = 0, PGS_INVALID = -1, PGS_CAPACITY = -4;   // (the values of VPL_OK, VPL_E_INVALID, VPL_E_CAPACITY)
constexpr int PGS_MAX_KEYFRAMES = 65536;

struct PgsPlan {
  int cap = 0;
  int sequence_cnt = 0;
  int earliest_loop_index = -1;
  int pending = -1;                  // the last queued index (optimize4DoF drains the queue and keeps the last), or -1
  std::vector<int> sequence_loop{0};
  std::vector<int> seq, loop_index;  // per keyframe; loop_index -1: no loop.  global_index = seq.size()
  int size() const { return (int)seq.size(); }
};

// what the device is to do for one accepted keyframe
struct PgsAddStep {
  int index = -1;
  int new_sequence = 0;   // :47-57: w_r_vio / w_t_vio and the drift start again at the identity
  int shift_list = 0;     // :103-124: the loop ties a sequence to an older one for the first time -- w_r_vio / w_t_vio are set from it and
                          //           the current and every stored keyframe of the sequence are shifted
};

inline void pgs_reset(PgsPlan& p) {
  const int cap = p.cap;
  p = PgsPlan();
  p.cap = cap;
}

// loop bookkeeping common to addKeyFrame and loadKeyFrame (:82-83, :125-127)
inline void pgs_note_loop(PgsPlan& p, int index, int loop_index) {
  if (loop_index < 0) return;
  if (p.earliest_loop_index > loop_index || p.earliest_loop_index == -1) p.earliest_loop_index = loop_index;
  p.pending = index;
}

// addKeyFrame.  sequence must be sequence_cnt or sequence_cnt + 1 and >= 1 (the reference's sequence_cnt++ would lose track of
// anything else); loop_index is -1 or an older keyframe
inline int pgs_add(PgsPlan& p, int sequence, int loop_index, PgsAddStep& st) {
  if (sequence < 1 || (sequence != p.sequence_cnt && sequence != p.sequence_cnt + 1)) return PGS_INVALID;
  if (loop_index < -1 || loop_index >= p.size()) return PGS_INVALID;
  if (p.size() >= p.cap) return PGS_CAPACITY;
  st = PgsAddStep();
  if (sequence != p.sequence_cnt) { ++p.sequence_cnt; p.sequence_loop.push_back(0); st.new_sequence = 1; }
  st.index = p.size();
  if (loop_index >= 0 && p.seq[loop_index] != sequence && p.sequence_loop[sequence] == 0) { st.shift_list = 1; p.sequence_loop[sequence] = 1; }
  pgs_note_loop(p, st.index, loop_index);
  p.seq.push_back(sequence); p.loop_index.push_back(loop_index);
  return PGS_OK;
}

// loadKeyFrame: a keyframe of sequence 0, poses as given
inline int pgs_load(PgsPlan& p, int loop_index, int& index) {
  if (loop_index < -1 || loop_index >= p.size()) return PGS_INVALID;
  if (p.size() >= p.cap) return PGS_CAPACITY;
  index = p.size();
  pgs_note_loop(p, index, loop_index);
  p.seq.push_back(0); p.loop_index.push_back(loop_index);
  return PGS_OK;
}

// one turn of optimize4DoF's loop: the range first .. cur and its loops (local node, local old node; ascending in the node), or
// PGS_CAPACITY with nothing changed.  -> 1 when there is something to optimise (the queue is emptied), 0 when nothing is queued
inline int pgs_take(PgsPlan& p, int& first, int& cur, std::vector<int>& loop_i, std::vector<int>& loop_a) {
  if (p.pending < 0) return 0;
  const int f = p.earliest_loop_index, c = p.pending;
  if (c - f + 1 > PG_MAX_NODES) return PGS_CAPACITY;
  std::vector<int> li, la;
  for (int k = f; k <= c; ++k)
    if (p.loop_index[k] >= 0) { li.push_back(k - f); la.push_back(p.loop_index[k] - f); }
  if ((int)li.size() > PG_MAX_LOOPS) return PGS_CAPACITY;
  first = f; cur = c; loop_i.swap(li); loop_a.swap(la);
  p.pending = -1;
  return 1;
}

}  // namespace vpl
