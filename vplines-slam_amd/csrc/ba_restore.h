// The pending state restore of a context (vpl_ba_reset_state), as a decision table without any device call.
// vpl_ba_reset_state enqueues nothing: it records that the states of the uploaded batch are to go back to their snapshots
// (pose_0, sb_0, ex_0, invd_0 and, RESTORE_LINES, plk_0).  The next vpl_ba_solve hands the record to k_prep, whose work-group
// copies its own window's snapshot before it reads the states; every other call that can observe or overwrite the states first
// issues the five device-to-device copies (flush).  Plain C++: tests/native/restore_fold_check.cpp drives it on the host.
#pragma once

enum RestoreMode { RESTORE_NONE = 0, RESTORE_STATES = 1, RESTORE_LINES = 2 };   // RESTORE_LINES: the states and the Pluecker vectors

// what a call does to the context, as far as the restore is concerned
enum RestoreEvent {
  RESTORE_EV_RESET,        // vpl_ba_reset_state
  RESTORE_EV_REUSE,        // the solve of vpl_ba_solve_odometry on the batch onlyLineOpt left (states only, the lines stay)
  RESTORE_EV_SOLVE,        // vpl_ba_solve
  RESTORE_EV_UPLOAD,       // an upload that has passed its refusals: it rewrites the snapshots
  RESTORE_EV_OBSERVE,      // download, pack_states_device, synchronize / collect, the session's calls, set_stream, set_prior_rule, ...
  RESTORE_EV_DESTROY       // vpl_ctx_destroy
};

struct RestoreStep {
  int flush;               // RestoreMode of the copies to issue now, before the call goes on
  int prep;                // RestoreMode handed to k_prep (RESTORE_EV_SOLVE only)
  int pending;             // the record after the call
};

// fold = false (VPL_BA_RESET_FOLD=0): a reset is the five copies at once, nothing is ever pending
inline RestoreStep restore_step(int pending, RestoreEvent ev, bool fold) {
  RestoreStep s = {RESTORE_NONE, RESTORE_NONE, pending};
  switch (ev) {
    case RESTORE_EV_RESET:      // two resets in a row are one restore
    case RESTORE_EV_REUSE: {
      const int want = ev == RESTORE_EV_RESET ? RESTORE_LINES : RESTORE_STATES;
      if (!fold) { s.flush = want; s.pending = RESTORE_NONE; }
      else s.pending = pending > want ? pending : want;
      break;
    }
    case RESTORE_EV_SOLVE:
      s.prep = pending;
      s.pending = RESTORE_NONE;
      break;
    case RESTORE_EV_UPLOAD:     // the snapshots themselves are replaced: nothing left to restore
    case RESTORE_EV_DESTROY:    // the arrays are freed, nobody can observe them (and the stream may be gone already)
      s.pending = RESTORE_NONE;
      break;
    case RESTORE_EV_OBSERVE:
      s.flush = pending;
      s.pending = RESTORE_NONE;
      break;
  }
  return s;
}
