"""The point tracker session (vpl_ptrk_*) against tests/pt_ref.py's tracker, n_seq = 2: sequence 0 sees the golden frames 1 .. 15
and publishes every image, sequence 1 sees them from frame 4 on and publishes every second image.  The reference runs on the
frames as the device's own CLAHE prepares them (that stage is held to the oracle by tests/test_preproc.py)."""
import functools

import numpy as np
import pytest

import vplines_slam_amd as v

import pt_inputs
import pt_ref

pytestmark = pytest.mark.gpu

VPL_E_CAPACITY = -4
N_CALLS = 15
DT = 0.05


def samples(seed, N):
    return v.relpose_debug_plan(seed, 0, N)["samples"]


def schedule(k):
    """call k -> (frame of sequence 0, frame of sequence 1, publish, seeds, times)"""
    f = pt_inputs.frames()
    return (f[k % 15], f[(k + 3) % 15]), (1, k % 2), (100 + k, 200 + k), (DT * (k + 1), 0.5 + 0.04 * (k + 1))


def make(max_candidates=8192):
    fe = v.frontend.FrontendContext(max_images=4, width=pt_inputs.W, height=pt_inputs.H, max_lines=64)
    fe.pt_reserve(max_candidates=max_candidates, max_corners=160, max_points=160)
    trk = v.PointTrackerSession(fe, 2, v.default_point_tracker_options(pt_inputs.CAM))
    return fe, trk


@functools.lru_cache(maxsize=None)
def equalised():
    """the 15 golden frames after the device's CLAHE(3.0, 8 x 8)"""
    fe = v.frontend.FrontendContext(max_images=15, width=pt_inputs.W, height=pt_inputs.H, max_lines=64)
    try:
        fe.pre_upload(pt_inputs.frames())
        fe.pre_run(True, 3.0, (8, 8))
        out = fe.pre_download()
    finally:
        fe.close()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def device_run():
    """the whole schedule on the device: per call (results of both sequences, get_frame of both), and the raw bytes of it all"""
    fe, trk = make()
    out = []
    try:
        for k in range(N_CALLS):
            frames, pub, seeds, times = schedule(k)
            r = trk.frame(np.stack(frames), times, pub, seeds)
            out.append((r, [trk.get_frame(0), trk.get_frame(1)]))
    finally:
        fe.close()
    return out


@functools.lru_cache(maxsize=None)
def reference_run():
    eq = equalised()
    trackers = [pt_ref.PointTracker(pt_inputs.CAM, pt_inputs.W, pt_inputs.H, samples) for _ in range(2)]
    out = []
    for k in range(N_CALLS):
        _, pub, seeds, times = schedule(k)
        idx = (k % 15, (k + 3) % 15)
        r = [trackers[s].read_image(eq[idx[s]], times[s], pub[s], seeds[s]) for s in range(2)]
        state = [dict(pts=t.pts.copy(), ids=t.ids.copy(), cnt=t.cnt.copy(), sc=t.sc.copy(), un=t.un.copy(), usc=t.usc.copy(), n_id=t.n_id)
                 for t in trackers]
        out.append((r, state))
    return out


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_session_matches_the_reference_after_every_call():
    dev, ref = device_run(), reference_run()
    seen = [set(), set()]
    for k in range(N_CALLS):
        _, pub, _, times = schedule(k)
        for s in range(2):
            d, g = dev[k][0][s], dev[k][1][s]
            r, st = ref[k][0][s], ref[k][1][s]
            got = {f: d[f] for f in r["res"]}
            print("call", k, "sequence", s, got)
            assert got == r["res"], (k, s, got, r["res"])
            assert g["n"] == len(st["pts"]) and g["next_id"] == st["n_id"]
            assert np.array_equal(g["ids"], st["ids"]) and np.array_equal(g["track_cnt"], st["cnt"])
            assert np.array_equal(g["pts"].view(np.uint32), st["pts"].view(np.uint32))
            assert np.array_equal(g["scores"].view(np.uint32), st["sc"].view(np.uint32))
            assert np.array_equal(g["un_scores"].view(np.uint32), st["usc"].view(np.uint32))
            assert (ulps(g["un_pts"], st["un"]) <= 1).all()
            # ids are never reused: a fresh point's id has not been seen in this sequence
            fresh = set(int(i) for i, c in zip(g["ids"], g["track_cnt"]) if c == 1)
            assert not (fresh & seen[s])
            seen[s] |= set(int(i) for i in g["ids"])
            # the rows
            assert np.array_equal(d["ids"], r["ids"])
            if not pub[s]:
                assert d["published"] == 0 and len(d["rows"]) == 0
                continue
            rows = d["rows"]
            assert rows.shape == r["rows"].shape
            assert np.array_equal(rows[:, 2:4], r["rows"][:, 2:4])                       # u, v
            assert (ulps(rows[:, 0:2], r["rows"][:, 0:2]) <= 1).all()                    # x, y: one float32 ulp
            assert np.array_equal(rows[:, 0:2], rows[:, 0:2].astype(np.float32).astype(np.float64))
            assert (rows[:, 6] == float(g["un_scores"][0])).all() if len(rows) else True   # prob: forw_un_scores[0] in every row
            # vx, vy from the device's own un-points of the two images, looked up by id (a point that was fresh in the
            # previous image had the key -1 there and is not found)
            sel = g["track_cnt"] > 1
            assert np.array_equal(g["ids"][sel], d["ids"])
            assert np.array_equal(rows[:, 0:2].astype(np.float32), g["un_pts"][sel])
            prev = dev[k - 1][1][s] if k else None
            pmap = {int(i): u for i, u, c in zip(prev["ids"], prev["un_pts"], prev["track_cnt"]) if c > 1} if prev else {}
            dt = times[s] - (schedule(k - 1)[3][s] if k else 0.0)
            for i, u, row in zip(d["ids"], g["un_pts"][sel], rows):
                want = (0.0, 0.0)
                if prev is not None and prev["n"] > 0 and int(i) in pmap:
                    p = pmap[int(i)]
                    want = (float(np.float32(float(u[0] - p[0]) / dt)), float(np.float32(float(u[1] - p[1]) / dt)))
                assert (row[4], row[5]) == want, (k, s, int(i), row[4:6], want)
    # the two sequences did not mix: they saw different frames and hold different lists
    assert not np.array_equal(dev[-1][1][0]["pts"][:20], dev[-1][1][1]["pts"][:20])
    assert ref[-1][0][0]["res"]["published"] > 50


def test_two_runs_give_the_same_bytes():
    a = device_run()
    device_run.cache_clear()
    b = device_run()
    for (ra, ga), (rb, gb) in zip(a, b):
        for s in range(2):
            assert all(np.array_equal(np.asarray(ra[s][f]), np.asarray(rb[s][f])) for f in ra[s])
            assert all(np.asarray(ga[s][f]).tobytes() == np.asarray(gb[s][f]).tobytes() for f in ga[s])


def test_reset_keeps_the_id_counter_and_the_neighbour():
    fe, trk = make()
    try:
        for k in range(3):
            frames, pub, seeds, times = schedule(k)
            trk.frame(np.stack(frames), times, (1, 1), seeds)
        before = trk.get_frame(1)
        trk.reset(1)
        assert trk.get_frame(1)["n"] == 0 and trk.get_frame(1)["next_id"] == before["next_id"]
        frames, pub, seeds, times = schedule(3)
        r = trk.frame(np.stack(frames), times, (1, 1), seeds)
        after = trk.get_frame(1)
        assert r[1]["tracked"] == 0 and r[1]["published"] == 0 and r[1]["detected"] == after["n"] > 0
        assert after["ids"].min() == before["next_id"] and (after["track_cnt"] == 1).all()
        # sequence 0 went on as in the undisturbed run (it publishes every image there too)
        want = device_run()[3]
        assert np.array_equal(r[0]["ids"], want[0][0]["ids"]) and np.array_equal(r[0]["rows"], want[0][0]["rows"])
    finally:
        fe.close()


def test_a_call_refused_for_capacity_leaves_both_sequences_as_they_were():
    """a fisheye mask that opens a 240 x 200 window keeps the candidate list short; without it the list overflows"""
    window = np.zeros((pt_inputs.H, pt_inputs.W), np.uint8)
    window[140:340, 250:490] = 255
    fe, trk = make(max_candidates=1200)
    eq = equalised()
    ref = [pt_ref.PointTracker(pt_inputs.CAM, pt_inputs.W, pt_inputs.H, samples) for _ in range(2)]
    for t in ref:
        t.base_mask = window
    try:
        trk.set_mask(window)
        frames, _, seeds, times = schedule(0)
        first = trk.frame(np.stack(frames), times, (1, 1), seeds)
        want = [ref[s].read_image(eq[(0, 3)[s]], times[s], 1, seeds[s]) for s in range(2)]
        assert [first[s]["detected"] for s in range(2)] == [want[s]["res"]["detected"] for s in range(2)] and first[0]["detected"] > 5
        held = [trk.get_frame(s) for s in range(2)]
        trk.set_mask(None)
        frames, _, seeds, times = schedule(1)
        with pytest.raises(RuntimeError, match="corner candidates"):
            trk.frame(np.stack(frames), times, (1, 0), seeds)
        for s in range(2):
            now = trk.get_frame(s)
            assert all(np.asarray(now[f]).tobytes() == np.asarray(held[s][f]).tobytes() for f in now)
        # the next good call matches the reference, which never saw the refused one
        trk.set_mask(window)
        got = trk.frame(np.stack(frames), times, (1, 1), seeds)
        for s in range(2):
            r = ref[s].read_image(eq[(1, 4)[s]], times[s], 1, seeds[s])
            assert {f: got[s][f] for f in r["res"]} == r["res"]
            assert np.array_equal(got[s]["ids"], r["ids"]) and np.array_equal(got[s]["rows"][:, 2:4], r["rows"][:, 2:4])
            assert got[s]["published"] > 0
    finally:
        fe.close()


def test_session_refusals():
    fe = v.frontend.FrontendContext(max_images=3, width=pt_inputs.W, height=pt_inputs.H, max_lines=64)
    try:
        opt = v.default_point_tracker_options(pt_inputs.CAM)
        with pytest.raises(RuntimeError, match="vpl_pt_reserve"):
            v.PointTrackerSession(fe, 1, opt)
        fe.pt_reserve(max_candidates=4096, max_corners=100, max_points=160)
        with pytest.raises(RuntimeError, match="max_cnt"):
            v.PointTrackerSession(fe, 1, opt)                      # 150 corners do not fit into rows of 100
        opt.max_cnt = 100
        with pytest.raises(RuntimeError, match="2 n_seq"):
            v.PointTrackerSession(fe, 2, opt)
        trk = v.PointTrackerSession(fe, 1, opt)
        with pytest.raises(RuntimeError, match="already"):
            v.PointTrackerSession(fe, 1, opt)
        trk.close()
        v.PointTrackerSession(fe, 1, opt).close()
    finally:
        fe.close()
