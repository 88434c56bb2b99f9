// Host-only check of the pending-restore decision table (csrc/ba_restore.h; tests/test_restore_fold.py builds and runs it with
// g++ -fsanitize=address,undefined).  A model context -- the pending record and a log of what each call issued -- is driven
// through the call sequences of the library: which calls copy the snapshots (flush), which hand the restore to k_prep, which
// drop it, and that no sequence restores twice or not at all.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "ba_restore.h"

struct Model {
  bool fold;
  int pending = RESTORE_NONE;
  std::vector<std::string> log;     // "flush<mode>" / "prep<mode>" in the order they were issued
  // the states as a version number: 0 = the snapshot, anything else = moved by a solve / not restored
  int snapshot = 0, states = 0, next = 1;
  int start_from = -1;              // what the last solve started from
  explicit Model(bool f) : fold(f) {}
  RestoreStep call(RestoreEvent ev) {
    const RestoreStep s = restore_step(pending, ev, fold);
    pending = s.pending;
    if (s.flush) { log.push_back("flush" + std::to_string(s.flush)); states = snapshot; }
    if (ev == RESTORE_EV_SOLVE) {
      log.push_back("prep" + std::to_string(s.prep));
      if (s.prep) states = snapshot;
      start_from = states;
      states = next++;               // the solve moves them
    }
    if (ev == RESTORE_EV_UPLOAD) { snapshot = states = next++; }
    return s;
  }
};

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

static std::string joined(const Model& m) {
  std::string s;
  for (const std::string& e : m.log) s += (s.empty() ? "" : " ") + e;
  return s;
}

int main(int argc, char** argv) {
  // ---- the transitions of the issue, restore folded into k_prep
  { Model m(true);                    // reset then solve: nothing is copied, k_prep restores states and lines
    RestoreStep r = m.call(RESTORE_EV_RESET);
    CHECK(r.flush == RESTORE_NONE && m.pending == RESTORE_LINES && m.log.empty());
    r = m.call(RESTORE_EV_SOLVE);
    CHECK(r.flush == RESTORE_NONE && r.prep == RESTORE_LINES && m.pending == RESTORE_NONE);
    r = m.call(RESTORE_EV_SOLVE);     // a solve without a reset does not restore
    CHECK(r.prep == RESTORE_NONE && r.flush == RESTORE_NONE);
    CHECK(joined(m) == "prep2 prep0"); }
  { Model m(true);                    // reset then download: the download flushes, the solve after it does not restore again
    m.call(RESTORE_EV_RESET);
    RestoreStep r = m.call(RESTORE_EV_OBSERVE);
    CHECK(r.flush == RESTORE_LINES && m.pending == RESTORE_NONE && m.states == m.snapshot);
    r = m.call(RESTORE_EV_OBSERVE);   // ... and a second download has nothing left to flush
    CHECK(r.flush == RESTORE_NONE);
    r = m.call(RESTORE_EV_SOLVE);
    CHECK(r.prep == RESTORE_NONE);
    CHECK(joined(m) == "flush2 prep0"); }
  { Model m(true);                    // reset then reset: one restore
    m.call(RESTORE_EV_RESET);
    RestoreStep r = m.call(RESTORE_EV_RESET);
    CHECK(r.flush == RESTORE_NONE && m.pending == RESTORE_LINES);
    m.call(RESTORE_EV_SOLVE);
    CHECK(joined(m) == "prep2"); }
  { Model m(true);                    // reset then upload: the upload rewrites the snapshots, nothing is copied or pending
    m.call(RESTORE_EV_RESET);
    RestoreStep r = m.call(RESTORE_EV_UPLOAD);
    CHECK(r.flush == RESTORE_NONE && m.pending == RESTORE_NONE);
    r = m.call(RESTORE_EV_SOLVE);
    CHECK(r.prep == RESTORE_NONE);
    CHECK(joined(m) == "prep0"); }
  { Model m(true);                    // reset then set_stream: flushed (on the new stream, vpl_ctx_set_stream)
    m.call(RESTORE_EV_RESET);
    RestoreStep r = m.call(RESTORE_EV_OBSERVE);
    CHECK(r.flush == RESTORE_LINES && m.pending == RESTORE_NONE); }
  { Model m(true);                    // reset then destroy: dropped, no copy is enqueued on a context that is going away
    m.call(RESTORE_EV_RESET);
    RestoreStep r = m.call(RESTORE_EV_DESTROY);
    CHECK(r.flush == RESTORE_NONE && r.prep == RESTORE_NONE && m.pending == RESTORE_NONE && m.log.empty()); }
  { Model m(true);                    // solve_odometry on the batch onlyLineOpt left: states only, the optimised lines stay
    RestoreStep r = m.call(RESTORE_EV_REUSE);
    CHECK(r.flush == RESTORE_NONE && m.pending == RESTORE_STATES);
    r = m.call(RESTORE_EV_SOLVE);
    CHECK(r.prep == RESTORE_STATES); }
  { Model m(true);                    // the stronger request wins whatever the order
    m.call(RESTORE_EV_REUSE); m.call(RESTORE_EV_RESET);
    CHECK(m.pending == RESTORE_LINES);
    m.call(RESTORE_EV_REUSE);
    CHECK(m.pending == RESTORE_LINES); }
  // ---- VPL_BA_RESET_FOLD=0: the copies at once, never anything pending
  { Model m(false);
    RestoreStep r = m.call(RESTORE_EV_RESET);
    CHECK(r.flush == RESTORE_LINES && m.pending == RESTORE_NONE);
    r = m.call(RESTORE_EV_RESET);
    CHECK(r.flush == RESTORE_LINES);
    r = m.call(RESTORE_EV_SOLVE);
    CHECK(r.prep == RESTORE_NONE && r.flush == RESTORE_NONE);
    r = m.call(RESTORE_EV_REUSE);
    CHECK(r.flush == RESTORE_STATES && m.pending == RESTORE_NONE);
    CHECK(joined(m) == "flush2 flush2 prep0 flush1"); }
  // ---- random call sequences, both settings side by side: whenever the states can be observed (a flush point, the start of a
  // solve's arithmetic) the folded context holds what the unfolded one holds; restores are never issued twice for one reset
  std::mt19937 rng(argc > 1 ? std::atoi(argv[1]) : 7);
  const RestoreEvent evs[] = {RESTORE_EV_RESET, RESTORE_EV_REUSE, RESTORE_EV_SOLVE, RESTORE_EV_UPLOAD, RESTORE_EV_OBSERVE};
  int sequences = 0;
  for (int t = 0; t < 2000; ++t) {
    Model a(true), b(false);
    const int len = 1 + (int)(rng() % 12);
    for (int k = 0; k < len; ++k) {
      const RestoreEvent ev = evs[rng() % 5];
      const RestoreStep ra = a.call(ev), rb = b.call(ev);
      CHECK(rb.prep == RESTORE_NONE && b.pending == RESTORE_NONE);
      CHECK(ra.flush == RESTORE_NONE || ra.prep == RESTORE_NONE);        // never both in one call
      if (ev == RESTORE_EV_OBSERVE || ev == RESTORE_EV_SOLVE || ev == RESTORE_EV_UPLOAD) {
        CHECK(a.pending == RESTORE_NONE);
        CHECK((a.states == a.snapshot) == (b.states == b.snapshot));
        CHECK(a.states == b.states && a.snapshot == b.snapshot && a.start_from == b.start_from);
      }
    }
    a.call(RESTORE_EV_DESTROY);
    CHECK(a.pending == RESTORE_NONE);
    ++sequences;
  }
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("restore decision table ok: 9 scripted transitions, %d random sequences\n", sequences);
  return 0;
}
