"""The integer bookkeeping of a keyframe session (vpl_odo_*, include/vplines_ba.h) without a device: vpl_odo_debug_tracks
replays a script of frames, erase decisions and slide flags through the code vpl_odo_keyframe runs (csrc/odo_tracks.h) and
returns the track table after every step.  It is compared, integer for integer,
  (a) with a restatement of the feature manager of tests/test_gpu_sequence.py (Run._add_frame, the erasures, the slide's
      bookkeeping) on a dict in insertion order, and
  (b) the slide of every step with the ORACLE's slide_window (point_* and line_* of vpl_slide_tracks).
Also here: the argument checks of the session's entry points that need no device."""
import ctypes as C

import numpy as np

import oracle_api as o
import vplines_slam_amd as v
from vplines_slam_amd.capi import odo_debug_tracks

NF = 11
WS = NF - 1
E_INVALID, E_CAPACITY = -1, -4


def make_script(rng, n_slides=20):
    """11 frames that fill the window, then n_slides keyframes.  A pool of landmarks that come into view, stay a while and
    leave -- and some of them come back: tracks of every length and start frame, ids that reappear after a gap."""
    pool = int(rng.integers(8, 40))
    p_on, p_off = rng.uniform(0.05, 0.5), rng.uniform(0.05, 0.5)
    seen = rng.random(pool) < 0.5
    # a capacity some scripts run into -- after the window is full: while it fills only the first `cap` landmarks are in view
    # (a refused filling frame would leave the window short of a frame and the script without a meaning)
    cap = int(rng.choice([pool] * 5 + [max(2, 2 * pool // 3), max(2, pool // 2)]))
    frames = []
    for f in range(NF + n_slides):
        flip = rng.random(pool)
        seen = np.where(seen, flip >= p_off, flip < p_on)
        ids = [int(i) * 3 + 1 for i in np.nonzero(seen)[0] if f >= NF or i < cap]
        rng.shuffle(ids)
        frames.append(ids)
    flags = [v.MARGIN_NONE] * NF + [int(rng.choice([v.MARGIN_OLD, v.MARGIN_OLD, v.MARGIN_SECOND_NEW])) for _ in range(n_slides)]
    erase = (rng.random((NF + n_slides, cap)) < 0.06).astype(np.uint8)
    return cap, flags, frames, erase


def slide_one(flag, start, nobs):
    """Estimator::slideWindow on one track: (start, nobs, drop) afterwards; nobs 0 = erased.  removeBackShiftDepth
    (feature_manager.cpp:800-874) / removeFront (:915-956)"""
    if flag == v.MARGIN_OLD:
        if start != 0:
            return start - 1, nobs, -1
        return 0, (nobs - 1 if nobs - 1 >= 2 else 0), 0
    if start == WS:
        return WS - 1, nobs, -1
    if start + nobs - 1 < WS - 1:
        return start, nobs, -1
    return start, nobs - 1, WS - 1 - start


class Book:
    """the feature manager of tests/test_gpu_sequence.py reduced to its integers: a dict id -> [start, nobs] in insertion order"""

    def __init__(self, cap):
        self.cap, self.t, self.frames = cap, {}, 0

    def add_frame(self, slot, ids):
        ignored = 0
        for lm in ids:
            t = self.t.get(lm)
            if t is not None and t[0] + t[1] == slot:
                t[1] += 1
            elif t is None:
                self.t[lm] = [slot, 1]
            else:
                ignored += 1          # a landmark that was lost and comes back is not continued
        return ignored

    def step(self, flag, ids, erase):
        """returns (status, tracks that entered the slide [(start, nobs)], what the slide did to them, ignored)"""
        unknown = len({i for i in ids if i not in self.t})
        if len(self.t) + unknown > self.cap:
            return E_CAPACITY, [], [], 0
        if flag == v.MARGIN_NONE:
            ig = self.add_frame(self.frames, ids)
            self.frames += 1
            return 0, [], [], ig
        for i, lm in enumerate(list(self.t)):
            if erase[i]:
                del self.t[lm]
        entered = [tuple(t) for t in self.t.values()]
        slid = []
        for lm in list(self.t):
            s, n, d = slide_one(flag, *self.t[lm])
            slid.append((s, n, d))
            if n == 0:
                del self.t[lm]
            else:
                self.t[lm] = [s, n]
        return 0, entered, slid, self.add_frame(NF - 1, ids)

    def table(self):
        return [(lm, t[0], t[1]) for lm, t in self.t.items()]


def oracle_slide(flag, entered, opt):
    """the oracle's slide_window on a window whose point AND line tracks are `entered`"""
    n = len(entered)
    start, nobs = [s for s, _ in entered], [k for _, k in entered]
    tot = int(sum(nobs))
    pose = np.zeros((NF, 7))
    pose[:, 6] = 1.0
    pose[:, 0] = np.arange(NF) * 0.1
    ex = np.array([0, 0, 0, 0, 0, 0, 1.0])
    pobs = np.tile([0.1, -0.2, 1.0], (tot, 1))
    lobs = np.tile([0.1, 0.1, 0.3, -0.2, 0.0, 0.0, 1.0, 1.0], (tot, 1))
    plk = np.tile([0.0, 1.0, 0.0, 1.0, 0.0, 0.0], (n, 1))
    w = v.capi.Window(pose, np.zeros((NF, 9)), ex, start, nobs, pobs, np.full(n, 0.2), start, nobs, lobs, plk)
    st = o.slide_window(w, opt, flag, 5.0)
    return st


def test_track_bookkeeping_matches_the_restatement_and_the_oracles_slide():
    rng = np.random.default_rng(20261016)
    opt = v.default_options()
    n_scripts = 220
    lengths, starts, flags_seen = set(), set(), set()
    n_refused = n_ignored = n_erased_by_slide = n_steps = 0
    for _ in range(n_scripts):
        cap, flags, frames, erase = make_script(rng)
        rc, status, n_slide, slide, n_tracks, table, ignored = odo_debug_tracks(cap, flags, frames, erase)
        assert rc == 0
        book = Book(cap)
        for s, (flag, ids) in enumerate(zip(flags, frames)):
            before = book.table()
            st, entered, slid, ig = book.step(flag, ids, erase[s])
            assert status[s] == st, (s, status[s], st)
            assert ignored[s] == ig, s
            # (a) the whole table after the step, refused steps included (unchanged)
            got = [tuple(int(x) for x in table[s, i]) for i in range(n_tracks[s])]
            assert got == book.table(), (s, got, book.table())
            if st == E_CAPACITY:
                assert got == before
                n_refused += 1
                continue
            if flag == v.MARGIN_NONE:
                assert n_slide[s] == 0
                continue
            n_steps += 1
            flags_seen.add(flag)
            n_ignored += ig
            assert n_slide[s] == len(entered)
            got_slide = [tuple(int(x) for x in slide[s, i]) for i in range(n_slide[s])]
            assert got_slide == slid, (s, got_slide, slid)
            # (b) the oracle's slideWindow on the same tracks, as points and as lines
            if entered:
                ost = oracle_slide(flag, entered, opt)
                want = np.array(slid, np.int32).reshape(-1, 3)
                for a, b, c in ((ost.point_start, ost.point_nobs, ost.point_drop), (ost.line_start, ost.line_nobs, ost.line_drop)):
                    assert np.array_equal(a, want[:, 0]) and np.array_equal(b, want[:, 1]) and np.array_equal(c, want[:, 2]), s
            for (s0, k0), (_, k1, _) in zip(entered, slid):
                lengths.add(k0)
                starts.add(s0)
                n_erased_by_slide += k1 == 0
    print('accepted keyframes %d, refused steps %d, ignored observations %d, tracks the slide erased %d' % (n_steps, n_refused, n_ignored, n_erased_by_slide))
    assert n_steps >= 200 * 20 * 0.8
    assert lengths == set(range(1, NF + 1)), lengths
    assert starts == set(range(NF)), starts
    assert flags_seen == {v.MARGIN_OLD, v.MARGIN_SECOND_NEW}
    assert n_refused > 20 and n_ignored > 100 and n_erased_by_slide > 100, (n_refused, n_ignored, n_erased_by_slide)


def test_debug_tracks_refuses_bad_scripts():
    ids = [[1, 2]] * (NF + 1)
    er = np.zeros((NF + 1, 4), np.uint8)
    # a slide before the window is full, a twelfth filling frame, an unknown flag
    assert odo_debug_tracks(4, [v.MARGIN_OLD], [[1]], er[:1])[0] == E_INVALID
    assert odo_debug_tracks(4, [v.MARGIN_NONE] * (NF + 1), ids, er)[0] == E_INVALID
    assert odo_debug_tracks(4, [v.MARGIN_NONE] * NF + [7], ids, er)[0] == E_INVALID
    assert odo_debug_tracks(4, [v.MARGIN_NONE] * NF + [v.MARGIN_SECOND_NEW], ids, er)[0] == 0
    lib = v.load_hip_library()
    assert lib.vpl_odo_debug_tracks(4, 1, None, None, None, None, None, None, None, None, None, None) == E_INVALID


def test_session_argument_checks_need_no_device():
    lib = v.load_hip_library()
    h = C.c_void_p()
    opt = v.default_options()
    # no context, no sequences, no options: refused before anything touches a device
    assert lib.vpl_odo_create(C.byref(h), None, 1, C.byref(opt), 5.0, 5, 64, 64) == E_INVALID and not h.value
    assert lib.vpl_odo_create(None, None, 1, C.byref(opt), 5.0, 5, 64, 64) == E_INVALID
    assert lib.vpl_odo_create(C.byref(h), None, 0, C.byref(opt), 5.0, 5, 64, 64) == E_INVALID
    res = (v.capi.OdoResult * 1)()
    fr = (v.capi.OdoFrame * 1)()
    fl = (C.c_int * 1)(7)
    assert lib.vpl_odo_keyframe(None, fr, fl, res) == E_INVALID
    assert lib.vpl_odo_set_window(None, 0, None, None, None, None, None) == E_INVALID
    assert lib.vpl_odo_get_prior(None, 0, None) == E_INVALID
    assert lib.vpl_odo_get_tracks(None, 0, None, None, None, None, None, None, None, None, None, None, None) == E_INVALID
    assert lib.vpl_odo_stats(None, None, None, None) == E_INVALID
    lib.vpl_odo_destroy(None)
    assert C.sizeof(v.capi.OdoFrame) == 8 * (7 + 9) + C.sizeof(v.capi.Preintegration) + 3 * 16
    assert C.sizeof(v.capi.OdoResult) == 8 * (77 + 99 + 7) + 2 * C.sizeof(v.capi.SolveReport) + 5 * 4 + 4


def test_session_without_a_device_fails_loudly():
    """Without a GPU there is no context to borrow and none can be made: the constructor raises, nothing computes on the CPU."""
    import torch
    if torch.cuda.is_available():
        return
    import pytest
    with pytest.raises(RuntimeError):
        v.Session(n_seq=1, max_points=8, max_point_obs=64, max_lines=8, max_line_obs=64)
