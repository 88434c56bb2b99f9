"""Tracker session (vpl_trk_*) against the host mirror vplhost::LineFeatureTracker, bit for bit: tests/native/trk_session_check.cpp
runs both on the same frames in one process (two front-end contexts, the same VP seed per frame) and prints what each holds
after every call.  The mirror itself is held to the oracle by tests/test_line_tracker.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vplines_slam_amd as v

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VPL_E_INVALID, VPL_E_CAPACITY = -1, -4
FIELDS = ("img", "lines", "ids", "tcnt", "match", "vpids", "vps", "obs", "cnt")
BLANK = -1


def golden_frames():
    a, b = (np.load(os.path.join(ROOT, "tests", "golden", "mh04_%d.npy" % i)) for i in (1, 2))
    return a, b


def bar_frame(shape, shift=0):
    """a bright bar on black near the principal point: two long edges, the short ends stay below min_line_length"""
    f = np.zeros(shape, np.uint8)
    H, W = shape
    f[H // 2 - 7 + shift:H // 2 + 7 + shift, W // 2 - 60 + shift:W // 2 + 60 + shift] = 220
    return f


@pytest.fixture(scope="module")
def rig(tmp_path_factory):
    """the check program, and the frame file: 0..3 the frames of the mirror test (mh04_1, mh04_2, two rolled copies), 4 / 5 a bar
    and the bar moved by one pixel"""
    from test_preproc import euroc_maps
    tmp = tmp_path_factory.mktemp("trk")
    exe = str(tmp / "trk_session_check")
    libdir = os.path.join(ROOT, "vplines-slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "trk_session_check.cpp"),
                           "-L", libdir, "-lvplines_hip", "-Wl,-rpath," + libdir, "-o", exe])
    a, b = golden_frames()
    frames = np.stack([a, b, np.roll(b, (2, -3), (0, 1)), np.roll(b, (4, -7), (0, 1)), bar_frame(a.shape), bar_frame(a.shape, 1)])
    H, W = a.shape
    mx, my = euroc_maps(W, H)
    frames.tofile(str(tmp / "frames.raw"))
    mx.tofile(str(tmp / "mx.f32"))
    my.tofile(str(tmp / "my.f32"))

    def run(schedule, max_h, max_v, max_lines=1024, env=None):
        """schedule [call][seq] of frame indices -> {key: [values]}"""
        n_calls, n_seq = len(schedule), len(schedule[0])
        cmd = [exe, str(tmp / "frames.raw"), str(len(frames)), str(W), str(H), str(tmp / "mx.f32"), str(tmp / "my.f32"), str(max_h),
               str(max_v), str(max_lines), str(n_seq), str(n_calls)] + [str(f) for row in schedule for f in row]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        vals = {}
        for ln in r.stdout.strip().splitlines():
            parts = ln.split()
            vals[parts[0]] = parts[1:]
        return vals
    return run


def arr(vals, key):
    return np.array(vals[key], np.float64)


def assert_session_equals_mirror(vals, n_calls, n_seq):
    for k in range(n_calls):
        for s in range(n_seq):
            for f in FIELDS:
                m, d = vals["m%d_%d_%s" % (k, s, f)], vals["s%d_%d_%s" % (k, s, f)]
                if f == "img":
                    assert m == d, (k, s, f)                                           # 64-bit hashes: compared as text
                else:
                    assert np.array_equal(np.array(m, np.float64), np.array(d, np.float64), equal_nan=True), (k, s, f)


@pytest.fixture(scope="module")
def two_sequences(rig):
    """The two-sequence run, made once, in a fresh child process with VPL_DEBUG_GUARDS=1 (the pattern behind every device array
    changes no result).  Sequence 0 sees the four frames in order (and frame 0 once more in the fifth call, which sequence 1
    needs); sequence 1 a blank frame first, then frames 1, 0, a blank frame, 2."""
    schedule = [[0, BLANK], [1, 1], [2, 0], [3, BLANK], [0, 2]]
    return schedule, rig(schedule, 25, 40, env={"VPL_DEBUG_GUARDS": "1"})


def test_session_equals_the_mirror_bit_for_bit_on_two_sequences(two_sequences):
    """prepared image, kept line records, ids, t_cnt, match vector, VP ids, vps, observation rows (NaNs as NaNs), allfeature_cnt,
    lines_exist and the detection count: equal for every call and sequence; quota 25 / 40, so that it cuts"""
    schedule, vals = two_sequences
    n_calls = len(schedule)
    assert_session_equals_mirror(vals, n_calls, 2)
    # not vacuous: ids continue, the quota cut, the VP stage ran on every non-first frame of sequence 0 and classified lines
    n_tracked = sum(int(vals["s%d_0_res" % k][2]) for k in range(1, 4))
    assert n_tracked > 30
    for k in range(1, n_calls):
        ids, prev = arr(vals, "s%d_0_ids" % k), arr(vals, "s%d_0_ids" % (k - 1))
        assert int(vals["s%d_0_res" % k][2]) == np.isin(ids, prev).sum()
        assert int(vals["s%d_0_vps" % k][0]) == 1 and int(vals["s%d_0_res" % k][3]) == 0
        assert len(vals["s%d_0_ids" % k]) < int(vals["s%d_0_cnt" % k][2])               # fewer kept than detected
        assert len(vals["s%d_0_img" % k]) == 1
    assert sum(int((arr(vals, "s%d_0_vpids" % k) < 3).sum()) for k in range(1, n_calls)) > 10
    assert int(vals["s0_0_vps"][0]) == 0 and not arr(vals, "s0_0_obs").reshape(-1, 9)[:, 5:].any()
    assert not np.array_equal(arr(vals, "s1_0_obs"), arr(vals, "s1_1_obs"))
    # observation rows: normalised end points of the kept lines, every row with the VP entry of kept line 0
    fx, fy, cx, cy = np.float32(458.654), np.float32(457.296), np.float32(752 // 2), np.float32(480 // 2)
    for k in range(n_calls):
        obs = arr(vals, "s%d_0_obs" % k).reshape(-1, 9)
        l32 = arr(vals, "s%d_0_lines" % k).reshape(-1, 10)[:, :4].astype(np.float32)
        want = np.stack([(l32[:, 0] - cx) / fx, (l32[:, 1] - cy) / fy, (l32[:, 2] - cx) / fx, (l32[:, 3] - cy) / fy], 1)
        assert np.array_equal(obs[:, 1:5], want.astype(np.float64))
        assert np.array_equal(obs[:, 5:], np.repeat(obs[:1, 5:], len(obs), 0), equal_nan=True)
        assert np.array_equal(obs[:, 0], arr(vals, "s%d_0_ids" % k))


def test_frames_without_lines_and_the_minus_one_ids_of_sequence_1(two_sequences):
    """the quirks, stated directly (the equality with the mirror is checked above)"""
    _, vals = two_sequences
    # call 0, a blank first frame: nothing detected, nothing taken over, no rows
    assert vals["s0_1_cnt"] == ["0", "0", "0"] and vals["s0_1_obs"] == [] and vals["s0_1_lines"] == []
    # call 1: the first frame with lines is no first image any more: every line kept with id -1, no match, counter untouched
    ids = arr(vals, "s1_1_ids")
    n_det = int(vals["s1_1_cnt"][2])
    assert n_det > 50 and len(ids) == n_det and (ids == -1).all() and vals["s1_1_cnt"][:2] == ["0", "1"]
    assert vals["s1_1_match"] == [] and int(vals["s1_1_vps"][0]) == 0 and not arr(vals, "s1_1_tcnt").any()
    # call 2 matches against those lines: an inherited -1 reads as "no id", so all ids are fresh, but t_cnt counts
    assert int(vals["s2_1_res"][1]) == 1 and (arr(vals, "s2_1_ids") >= 0).all() and arr(vals, "s2_1_tcnt").any()
    # call 3, a blank frame in the middle of a run: not taken over -- the state is call 2's
    assert vals["s3_1_cnt"][1] == "0" and vals["s3_1_obs"] == []
    for f in ("img", "lines", "ids", "tcnt"):
        assert vals["s3_1_" + f] == vals["s2_1_" + f], f
    # call 4 is matched against the frame of call 2, ids continue across the gap
    assert int(vals["s4_1_res"][1]) == 1 and int(vals["s4_1_res"][2]) > 10
    assert np.isin(arr(vals, "s4_1_ids"), arr(vals, "s2_1_ids")).sum() == int(vals["s4_1_res"][2])


def test_no_guard_pad_is_overwritten_in_the_two_sequence_run(two_sequences):
    """VPL_DEBUG_GUARDS=1 in the child process: the 64 bytes behind every device array of both contexts, the session's store
    included, still hold their pattern at the end"""
    _, vals = two_sequences
    assert vals["guards"] == ["0", "0"]


def test_quota_zero_keeps_only_tracked_lines_and_two_kept_lines_skip_the_vp_stage(rig):
    """quota 0 / 0 on three frames: after the first image only lines that continue an id are kept.  Sequence 1 sees the bar: at
    most two lines are kept, so its VP stage never runs."""
    schedule = [[0, 4], [1, 5], [2, 4]]
    vals = rig(schedule, 0, 0)
    assert_session_equals_mirror(vals, 3, 2)
    for k in (1, 2):
        n_lines, _, n_tracked, _ = (int(x) for x in vals["s%d_0_res" % k])
        assert n_lines == n_tracked > 10 and int(vals["s%d_0_vps" % k][0]) == 1
        assert np.isin(arr(vals, "s%d_0_ids" % k), arr(vals, "s%d_0_ids" % (k - 1))).all()
        assert 1 <= int(vals["s%d_1_cnt" % k][2]) and int(vals["s%d_1_res" % k][0]) <= 2 and int(vals["s%d_1_vps" % k][0]) == 0
        assert not arr(vals, "s%d_1_obs" % k).reshape(-1, 9)[:, 5:].any()
    assert 1 <= int(vals["s0_1_res"][0]) <= 2


def test_a_skipped_vp_stage_does_not_advance_the_first_frame_counter(rig):
    """bar, bar moved (two or fewer lines kept: the VP stage is skipped), then two real frames: the first VP stage that runs is
    the sequence's first (first_frame = 1), as in the mirror, whose vps the session reproduces bit for bit"""
    vals = rig([[4], [5], [0], [1]], 25, 40)
    assert_session_equals_mirror(vals, 4, 1)
    assert [int(vals["s%d_0_vps" % k][0]) for k in range(4)] == [0, 0, 1, 1]
    assert int(vals["s1_0_res"][0]) <= 2 and int(vals["s1_0_cnt"][2]) >= 1
    assert arr(vals, "s2_0_vps")[1:].any() and arr(vals, "s3_0_vps")[1:].any()


@pytest.fixture
def make_context():
    """contexts of the golden frames' size; closed (an open session first) when the test ends, whether it passed or not"""
    made = []

    def make(max_images, n_seq, max_lines=1024, reserve=True, maps=False, **opt):
        a, _ = golden_frames()
        fe = v.frontend.FrontendContext(device=0, max_images=max_images, width=a.shape[1], height=a.shape[0], max_lines=max_lines)
        made.append(fe)
        if reserve:
            fe.match_reserve(n_seq, 8192)
        if maps:
            from test_preproc import euroc_maps
            fe.set_maps(*euroc_maps(a.shape[1], a.shape[0]))
        return fe, v.default_tracker_options(**opt)
    yield make
    for fe in made:
        fe.close()


K_ = dict(max_h_lines=25, max_v_lines=40, fx=458.654, fy=457.296, cx=376.0, cy=240.0)


def test_create_refusals(make_context):
    lib = v.load_hip_library()
    # a context with max_images = 2 cannot hold two sequences
    fe, opt = make_context(2, 2)
    h = C.c_void_p()
    assert lib.vpl_trk_create(C.byref(h), fe.h, 2, C.byref(opt)) == VPL_E_CAPACITY and not h.value
    assert lib.vpl_trk_create(C.byref(h), fe.h, 0, C.byref(opt)) == VPL_E_INVALID
    bad = v.default_tracker_options(fx=0.0)
    assert lib.vpl_trk_create(C.byref(h), fe.h, 1, C.byref(bad)) == VPL_E_INVALID
    # one sequence fits; a second session on the same context is refused
    t = v.TrackerSession(fe, 1, opt)
    assert lib.vpl_trk_create(C.byref(h), fe.h, 1, C.byref(opt)) == VPL_E_INVALID and not h.value
    t.close()
    t = v.TrackerSession(fe, 1, opt)      # free again after the first was destroyed
    t.close()
    # vpl_match_reserve has not been called
    fe, opt = make_context(2, 1, reserve=False)
    assert lib.vpl_trk_create(C.byref(h), fe.h, 1, C.byref(opt)) == VPL_E_CAPACITY and not h.value


def test_a_refused_frame_leaves_the_session_as_it_was(make_context):
    """max_lines_per_image = 8: the bar is accepted, a real frame yields more lines and is refused with VPL_E_CAPACITY; the state
    (image, kept lines, ids, t_cnt) is the same before and after, and the next bar frame goes on from that state.  (With the maps:
    the remap's interpolation gives the bar's edges the slope the detector follows.)"""
    a, _ = golden_frames()
    fe, opt = make_context(2, 1, max_lines=8, maps=True, **K_)
    t = v.TrackerSession(fe, 1, opt)
    r0 = t.frame(bar_frame(a.shape)[None], [7])[0]
    assert 1 <= r0["n_lines"] <= 8 and r0["lines_exist"] == 1 and r0["allfeature_cnt"] == r0["n_lines"]
    before = t.get_frame(0)
    assert before["img"].any()
    res = (v.TrackerResult * 1)()
    ids, obs = np.zeros((1, 8), np.int32), np.zeros((1, 8, 8))
    seed = np.array([8], np.uint32)
    raw = np.ascontiguousarray(a[None])
    rc = fe.lib.vpl_trk_frame(t.h, raw.ctypes.data_as(C.POINTER(C.c_uint8)), seed.ctypes.data_as(C.POINTER(C.c_uint32)), res,
                              ids.ctypes.data_as(C.POINTER(C.c_int)), obs.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == VPL_E_CAPACITY and b"lines found" in fe.lib.vpl_fe_last_error(fe.h)
    after = t.get_frame(0)
    n = r0["n_lines"]
    assert np.array_equal(before["img"], after["img"]) and np.array_equal(before["t_cnt"], after["t_cnt"])
    assert before["lines"][:n].tobytes() == after["lines"][:n].tobytes() and np.array_equal(before["ids"][:n], after["ids"][:n])
    r2 = t.frame(bar_frame(a.shape, 1)[None], [9])[0]
    # the next frame is matched against the bar's lines, and the counter goes on from where it stood (detection 0 never inherits)
    assert r2["matched"] == 1 and r2["allfeature_cnt"] == r0["allfeature_cnt"] + r2["n_detected"] - r2["n_tracked"]
    assert np.isin(r2["ids"], r0["ids"]).sum() == r2["n_tracked"] and (r2["ids"][r2["n_tracked"]:] >= r0["allfeature_cnt"]).all()


def test_reset_starts_the_sequence_again_and_keeps_the_counter(make_context):
    """no undistortion maps here: the frames are not remapped, as in the mirror without maps"""
    a, b = golden_frames()
    fe, opt = make_context(2, 1, **K_)
    t = v.TrackerSession(fe, 1, opt)
    r0 = t.frame(a[None], [1])[0]
    r1 = t.frame(b[None], [2])[0]
    assert r0["vp_ran"] == 0 and r1["vp_ran"] == 1 and r1["n_tracked"] > 10
    t.reset(0)
    r2 = t.frame(a[None], [3])[0]
    # a first image again: every line kept with fresh ids from where the counter stood, no match, no VP stage
    assert r2["n_lines"] == r2["n_detected"] == r0["n_lines"] and r2["matched"] == 0 and r2["vp_ran"] == 0
    assert np.array_equal(r2["ids"], r1["allfeature_cnt"] + np.arange(r2["n_lines"]))
    assert r2["allfeature_cnt"] == r1["allfeature_cnt"] + r2["n_lines"] and not r2["obs"][:, 4:].any()
    assert np.array_equal(r2["obs"][:, :4], r0["obs"][:, :4])
