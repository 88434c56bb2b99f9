"""The host side of the keyframe rule and of the failure check (include/vplines_ba.h, "the keyframe decision and the failure
check"), without a device:
  - vpl_odo_debug_parallax_list replays a script through the book vpl_odo_advance keeps (csrc/odo_tracks.h) and returns, per
    step, the list of qualifying tracks the device is told and last_track_num.  Both are held to a restatement of
    FeatureManager::addFeatureCheckParallax (feature_manager.cpp:115-136, 166-177) on the Book of tests/test_odo_tracks.py:
    last_track_num is COUNTED while the image is added, as the reference counts it, not read off the table afterwards;
  - vpl_failure_detection against a restatement of Estimator::failureDetection (estimator.cpp:909-936);
  - the argument checks of the new session calls, and the ctypes struct sizes."""
import ctypes as C

import numpy as np

import vplines_slam_amd as v
from vplines_slam_amd.capi import odo_debug_parallax_list
from test_odo_tracks import make_script, Book, NF, WS, E_INVALID, E_CAPACITY


class RuleBook(Book):
    """Book + what addFeatureCheckParallax(frame_count = WINDOW_SIZE) reads: last_track_num, counted image by image, and the
    tracks with start_frame <= frame_count - 2 && start_frame + size - 1 >= frame_count - 1, in the list's order"""

    last_track_num = 0

    def add_frame(self, slot, ids):
        self.last_track_num = sum(1 for lm in ids if lm in self.t and self.t[lm][0] + self.t[lm][1] == slot)
        return super().add_frame(slot, ids)

    def qualifying(self):
        return [(i, s, n) for i, (s, n) in enumerate(self.t.values()) if s <= WS - 2 and s + n - 1 >= WS - 1]


def test_parallax_list_matches_the_restatement_over_random_scripts():
    rng = np.random.default_rng(20261018)
    starts_all, starts_q, ends, flags_seen = set(), set(), set(), set()
    n_decisions = n_gap = n_refused = 0
    for _ in range(300):
        cap, flags, frames, erase = make_script(rng)
        rc, n_list, lst, last = odo_debug_parallax_list(cap, flags, frames, erase)
        assert rc == 0
        book = RuleBook(cap)
        for s, (flag, ids) in enumerate(zip(flags, frames)):
            st, _, _, ig = book.step(flag, ids, erase[s])
            if st == E_CAPACITY or book.frames < NF:
                assert n_list[s] == -1 and last[s] == 0, s
                n_refused += st == E_CAPACITY
                continue
            want = book.qualifying()
            assert n_list[s] == len(want), (s, n_list[s], len(want))
            assert [int(e) for e in lst[s, :n_list[s]]] == [i | (WS - 2 - st_) << 20 for i, st_, _ in want], s
            assert last[s] == book.last_track_num, (s, last[s], book.last_track_num)
            n_decisions += 1
            n_gap += ig
            flags_seen.add(flag)
            starts_q.update(st_ for _, st_, _ in want)
            for st_, n in book.t.values():
                starts_all.add(st_)
                ends.add(st_ + n - 1)
    print("decisions %d, ignored observations %d, refused steps %d" % (n_decisions, n_gap, n_refused))
    assert n_decisions + n_refused == 300 * 21 and n_decisions >= 300 * 10   # every step from the 11th frame on was looked at
    assert starts_all == set(range(NF)) and starts_q == set(range(WS - 1)), (starts_all, starts_q)
    assert {WS - 2, WS - 1} <= ends                      # tracks that end in frame 8 (not qualifying) and in frame 9 (qualifying)
    assert flags_seen == {v.MARGIN_NONE, v.MARGIN_OLD, v.MARGIN_SECOND_NEW}   # (MARGIN_NONE: the step that completes the window)
    assert n_gap > 100 and n_refused > 20


def test_parallax_list_by_hand_and_bad_scripts():
    """ids 1..4 from frame 0; 2 is lost after frame 8, 3 after frame 9, 4 after frame 7 and is back in frame 10; 5 starts in
    frame 9, 6 in frame 10"""
    frames = [[1, 2, 3, 4]] * 8 + [[1, 2, 3], [1, 3, 5], [1, 4, 5, 6]]
    er = np.zeros((NF, 8), np.uint8)
    rc, n_list, lst, last = odo_debug_parallax_list(8, [v.MARGIN_NONE] * NF, frames, er)
    assert rc == 0 and list(n_list[:NF - 1]) == [-1] * (NF - 1)
    # book order 1, 2, 3, 4, 5, 6: tracks 0 (id 1) and 2 (id 3, ends in 9) qualify, each with its frame-8 observation at index 8
    assert n_list[NF - 1] == 2 and list(lst[NF - 1, :2]) == [0 | 8 << 20, 2 | 8 << 20]
    assert last[NF - 1] == 2                             # ids 1 and 5 continued; 4 was ignored, 6 is new
    assert odo_debug_parallax_list(8, [v.MARGIN_OLD], [[1]], er[:1])[0] == E_INVALID
    lib = v.load_hip_library()
    assert lib.vpl_odo_debug_parallax_list(8, 1, None, None, None, None, None, None, None) == E_INVALID


def failure_restated(sb, pose, last, lim=(2.5, 1.0, 5.0, 1.0)):
    """estimator.cpp:909-936: Bas / Bgs [WINDOW_SIZE].norm(), (tmp_P - last_P).norm(), abs(tmp_P.z() - last_P.z())"""
    sb, pose, last = (np.asarray(a, float) for a in (sb, pose, last))
    d = pose[:3] - last[:3]
    mask = 0
    if np.sqrt(sb[3] * sb[3] + sb[4] * sb[4] + sb[5] * sb[5]) > lim[0]:
        mask |= 1
    if np.sqrt(sb[6] * sb[6] + sb[7] * sb[7] + sb[8] * sb[8]) > lim[1]:
        mask |= 2
    if np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) > lim[2]:
        mask |= 4
    if abs(d[2]) > lim[3]:
        mask |= 8
    return mask


def _state(ba=(0, 0, 0), bg=(0, 0, 0), p=(0, 0, 0), last=(0, 0, 0)):
    sb = np.concatenate([[0.3, -0.2, 0.1], ba, bg]).astype(float)
    pose = np.concatenate([p, [0, 0, 0, 1]]).astype(float)
    lp = np.concatenate([last, [0, 0, 0, 1]]).astype(float)
    return sb, pose, lp


def test_failure_detection_matches_the_restatement():
    cases = {
        0: _state(ba=(0.1, 0.2, -0.1), bg=(0.01, 0, 0.02), p=(1, 2, 0.5), last=(0.5, 1.5, 0.25)),
        1: _state(ba=(2.0, 1.5, 0.5)),
        2: _state(bg=(0.6, -0.6, 0.6)),
        4: _state(p=(4.0, 3.5, 0.5), last=(0, 0, 0)),
        8: _state(p=(1, 1, -0.2), last=(1, 1, 0.9)),
        15: _state(ba=(0, 0, -3), bg=(2, 0, 0), p=(10, 0, 5), last=(0, 0, 0)),
        12: _state(p=(0, 0, 6), last=(0, 0, 0)),
    }
    for want, (sb, pose, lp) in cases.items():
        assert failure_restated(sb, pose, lp) == want, want
        assert v.failure_detection(sb, pose, lp) == want, want
    # exactly on a limit: nothing fires (every value below is exact in binary: 1.5^2 + 2^2 = 2.5^2, 0.6^2 + 0.8^2 is NOT, so the
    # gyro bias sits on an axis), one ulp above: it fires
    on = _state(ba=(1.5, 2.0, 0.0), bg=(0, -1.0, 0), p=(3, 4, 0), last=(0, 0, 0))
    assert failure_restated(*on) == 0 and v.failure_detection(*on) == 0
    onz = _state(p=(0, 0, 2.0), last=(0, 0, 1.0))
    assert failure_restated(*onz) == 0 and v.failure_detection(*onz) == 0
    up = np.nextafter
    for want, st in ((1, _state(ba=(up(2.5, 3), 0, 0))), (2, _state(bg=(0, 0, up(1.0, 2)))), (4, _state(p=(up(5.0, 6), 0, 0))),
                     (8, _state(p=(0, 0, -up(1.0, 2))))):
        assert failure_restated(*st) == want and v.failure_detection(*st) == want, want
    # moved limits
    lim = v.default_failure_limits()
    assert (lim.max_acc_bias, lim.max_gyr_bias, lim.max_translation, lim.max_z) == (2.5, 1.0, 5.0, 1.0)
    lim.max_acc_bias, lim.max_gyr_bias, lim.max_translation, lim.max_z = 0.2, 0.01, 0.5, 0.2
    moved = (0.2, 0.01, 0.5, 0.2)
    sb, pose, lp = cases[0]
    assert failure_restated(sb, pose, lp, moved) == 1 | 2 | 4 | 8
    assert v.failure_detection(sb, pose, lp, lim) == 1 | 2 | 4 | 8
    lim.max_translation, lim.max_z = 50.0, 10.0
    sb, pose, lp = cases[15]
    assert v.failure_detection(sb, pose, lp, lim) == failure_restated(sb, pose, lp, (0.2, 0.01, 50.0, 10.0)) == 1 | 2
    # random states around the limits
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(400):
        st = _state(ba=rng.normal(0, 1.6, 3), bg=rng.normal(0, 0.6, 3), p=rng.normal(0, 2.5, 3), last=rng.normal(0, 0.5, 3))
        got = v.failure_detection(*st)
        assert got == failure_restated(*st)
        seen.add(got)
    assert len(seen) >= 8
    lib = v.load_hip_library()
    assert lib.vpl_failure_detection(None, None, None, None) == E_INVALID


def test_rule_calls_on_a_null_session_and_struct_sizes():
    lib = v.load_hip_library()
    rule = v.default_keyframe_rule()
    assert (rule.min_parallax, rule.min_track_num) == (10.0 / 460.0, 20)
    dec = v.OdoDecision()
    res = (v.capi.OdoResult * 1)()
    fr = (v.capi.OdoFrame * 1)()
    ifr = (v.capi.OdoImuFrame * 1)()
    imu = (v.capi.OdoImuOut * 1)()
    assert lib.vpl_odo_enable_keyframe_rule(None, C.byref(rule)) == E_INVALID
    assert lib.vpl_odo_get_decision(None, 0, C.byref(dec)) == E_INVALID
    assert lib.vpl_odo_solve_auto(None, res) == E_INVALID
    assert lib.vpl_odo_keyframe_auto(None, fr, res) == E_INVALID
    assert lib.vpl_odo_keyframe_imu_auto(None, ifr, res, imu) == E_INVALID
    lib.vpl_odo_default_keyframe_rule(None)
    lib.vpl_failure_default_limits(None)
    # the header's structs: a double and an int (padded to 16); four ints and two doubles; four doubles; the record the device
    # writes: four ints and a double
    assert C.sizeof(v.OdoKeyframeRule) == 16
    assert C.sizeof(v.OdoDecision) == 4 * 4 + 2 * 8
    assert C.sizeof(v.FailureLimits) == 4 * 8
    assert v.capi.ODO_DECISION_RECORD_BYTES == 4 * 4 + 8
    # OdoResult is as it was: the decision travels beside it, not in it
    assert C.sizeof(v.capi.OdoResult) == 8 * (77 + 99 + 7) + 2 * C.sizeof(v.capi.SolveReport) + 5 * 4 + 4
