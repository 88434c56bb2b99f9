"""Wall time per frame of the line tracker's C calls over the 15 frames of tests/golden/mh04_frames.npz, two forms:
  parent   the calls vplhost::LineFeatureTracker::readImage makes, per camera and frame: vpl_pre_batch (prepared image down),
           vpl_edlines_detect + vpl_fe_synchronize + vpl_edlines_download, vpl_line_match_batch (both images and both line
           tables up again), vpl_line_track_ids on the host, vpl_vp_detect_batch;
  session  one vpl_trk_frame for all sequences (state resident on the device).
Only the C calls are timed (perf_counter around each; every one of them ends in a stream synchronise or is host code); the
numpy packing between the parent's calls, which a C++ caller does with a few memcpy, is not.  The two forms alternate --reps
times on one card, each pass from a fresh tracker; medians over frames 2..14.  Sequence s sees the frames rolled by 3 s pixels.
Prints one JSON line per n_seq with the medians, the bytes each way and the launches per frame (counted from the code), and
whether the ids and observation end points of the two forms were equal."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import vplines_slam_amd as v
from vplines_slam_amd import frontend as F
from test_preproc import euroc_maps

ML, MAX_KPS, MAX_H, MAX_V = 1024, 16384, 25, 40
FX, FY = 458.654, 457.296
u8p, ip, lp = C.POINTER(C.c_uint8), C.POINTER(C.c_int), C.POINTER(F.Line)


class Timer:
    def __init__(self):
        self.t = 0.0

    def __call__(self, fn, *a):
        t0 = time.perf_counter()
        rc = fn(*a)
        self.t += time.perf_counter() - t0
        return rc


class ParentTracker:
    """readImage of the host mirror, call for call (one camera)"""

    def __init__(self, fe, cx, cy):
        self.fe, self.lib, self.cx, self.cy = fe, fe.lib, cx, cy
        self.H, self.W = fe.H, fe.W
        self.img = np.zeros((self.H, self.W), np.uint8)
        self.prev_img = None
        self.prev = np.zeros(ML, F.LINE_DTYPE)
        self.n_prev, self.ids_prev, self.tc_prev = 0, np.zeros(0, np.int32), np.zeros(0, np.int32)
        self.started, self.cnt, self.vp_count = False, C.c_int(0), 0
        self.det = np.zeros(ML, F.LINE_DTYPE)
        self.ed, self.mp = F.default_param(), F.default_match_param()

    def frame(self, raw, seed, tm):
        lib, h = self.lib, self.fe.h
        chk = self.fe._check
        chk(tm(lib.vpl_pre_batch, h, 1, raw.ctypes.data_as(u8p), 1, 3.0, 8, 8, self.img.ctypes.data_as(u8p)), "pre")
        n_det = C.c_int(0)
        chk(tm(lib.vpl_edlines_detect, h, C.byref(self.ed)), "detect")
        chk(tm(lib.vpl_fe_synchronize, h), "sync")
        chk(tm(lib.vpl_edlines_download, h, 1, self.det.ctypes.data_as(lp), C.byref(n_det)), "download")
        n = n_det.value
        first = not self.started
        self.started = True
        if n == 0:
            return np.zeros(0, np.int32), np.zeros((0, 4), np.float32)
        if first or self.n_prev == 0:
            ids = (self.cnt.value + np.arange(n, dtype=np.int32)) if first else np.full(n, -1, np.int32)
            if first:
                self.cnt.value += n
            keep, tc = np.arange(n), np.zeros(n, np.int32)
        else:
            two = np.stack([self.prev_img, self.img])
            zero, one, nr, nc, matched = C.c_int(0), C.c_int(1), C.c_int(self.n_prev), C.c_int(n), C.c_int(0)
            r2c = np.full(ML, -1, np.int32)
            chk(tm(lib.vpl_line_match_batch, h, 2, two.ctypes.data_as(u8p), 1, C.byref(zero), C.byref(one), self.prev.ctypes.data_as(lp),
                   C.byref(nr), self.det.ctypes.data_as(lp), C.byref(nc), C.byref(self.mp), r2c.ctypes.data_as(ip), C.byref(matched)), "match")
            n_prev = self.n_prev if matched.value else 0
            ends = np.ascontiguousarray(self.det["line_endpoint"][:n])
            keep, ids, tc, vert = (np.zeros(n, np.int32) for _ in range(4))
            nv = C.c_int(0)
            nk = tm(lib.vpl_line_track_ids, n, ends.ctypes.data_as(C.POINTER(C.c_float)), n_prev, self.ids_prev.ctypes.data_as(ip),
                    self.tc_prev.ctypes.data_as(ip), len(self.tc_prev), r2c.ctypes.data_as(ip), MAX_H, MAX_V, C.byref(self.cnt),
                    keep.ctypes.data_as(ip), ids.ctypes.data_as(ip), tc.ctypes.data_as(ip), vert.ctypes.data_as(ip), C.byref(nv))
            assert nk >= 0
            keep, ids = keep[:nk], ids[:nk]
            if nk > 2:
                la, lh = np.zeros(ML, F.LINE_DTYPE), np.zeros(ML, F.LINE_DTYPE)
                la[:nk] = self.det[keep]
                hyp = vert[:nv.value] if nv.value > 2 else keep
                lh[:len(hyp)] = self.det[hyp]
                nh, na, sd, ff, st = C.c_int(len(hyp)), C.c_int(nk), C.c_uint32(seed), C.c_int(self.vp_count == 0), C.c_int(0)
                vps, vid = np.zeros(9), np.zeros(ML, np.int32)
                chk(tm(lib.vpl_vp_detect_batch, h, 1, lh.ctypes.data_as(lp), C.byref(nh), la.ctypes.data_as(lp), C.byref(na), FX, self.cx,
                       self.cy, C.byref(sd), C.byref(ff), vps.ctypes.data_as(C.POINTER(C.c_double)), vid.ctypes.data_as(ip), C.byref(st)), "vp")
                self.vp_count += 1
        kept = self.det[keep].copy()
        self.prev[:len(kept)] = kept
        self.n_prev, self.ids_prev, self.tc_prev = len(kept), np.ascontiguousarray(ids), np.ascontiguousarray(tc)
        self.prev_img = self.img.copy()
        return ids.copy(), kept["line_endpoint"].copy()


def measure(frames, n_seq, reps):
    T, H, W = frames.shape
    mx, my = euroc_maps(W, H)
    cx, cy = float(W // 2), float(H // 2)
    seqs = [np.ascontiguousarray(np.roll(frames, 3 * s, axis=2)) for s in range(n_seq)]
    fe_p = F.FrontendContext(device=0, max_images=2, width=W, height=H, max_lines=ML)
    fe_p.match_reserve(1, MAX_KPS)
    fe_p.set_maps(mx, my)
    fe_s = F.FrontendContext(device=0, max_images=2 * n_seq, width=W, height=H, max_lines=ML)
    fe_s.match_reserve(n_seq, MAX_KPS)
    fe_s.set_maps(mx, my)
    opt = F.default_tracker_options(MAX_H, MAX_V, FX, FY, cx, cy)
    med_p, med_s, equal = [], [], True
    for rep in range(reps):
        trackers = [ParentTracker(fe_p, cx, cy) for _ in range(n_seq)]
        tp, out_p = [], []
        for t in range(T):
            tm = Timer()
            out_p.append([trackers[s].frame(seqs[s][t], 1000 + t, tm) for s in range(n_seq)])
            tp.append(tm.t)
        ses = F.TrackerSession(fe_s, n_seq, opt)
        ts = []
        for t in range(T):
            raw = np.ascontiguousarray(np.stack([seqs[s][t] for s in range(n_seq)]))
            seed = np.full(n_seq, 1000 + t, np.uint32)
            rawp, seedp = raw.ctypes.data_as(u8p), seed.ctypes.data_as(C.POINTER(C.c_uint32))
            idp, obp = ses._ids.ctypes.data_as(ip), ses._obs.ctypes.data_as(C.POINTER(C.c_double))
            t0 = time.perf_counter()
            rc = ses.lib.vpl_trk_frame(ses.h, rawp, seedp, ses._res, idp, obp)
            ts.append(time.perf_counter() - t0)
            fe_s._check(rc, "vpl_trk_frame")
            for s in range(n_seq):
                n = ses._res[s].n_lines
                ids, ends = out_p[t][s]
                want = np.stack([(ends[:, 0] - np.float32(cx)) / np.float32(FX), (ends[:, 1] - np.float32(cy)) / np.float32(FY),
                                 (ends[:, 2] - np.float32(cx)) / np.float32(FX), (ends[:, 3] - np.float32(cy)) / np.float32(FY)], 1)
                equal &= n == len(ids) and np.array_equal(ses._ids[s, :n], ids) and np.array_equal(ses._obs[s, :n, :4], want.astype(np.float64))
        ses.close()
        med_p.append(float(np.median(tp[2:])) * 1e3)
        med_s.append(float(np.median(ts[2:])) * 1e3)
    fe_p.close()
    fe_s.close()
    PX, LB = W * H, 56 * ML
    rec = 16 * 4 + 72 + 4 * ML + 64 * ML
    return {
        "n_seq": n_seq, "frames": T, "reps": reps,
        "parent_ms_per_frame": med_p, "session_ms_per_frame": med_s,
        "parent_ms_median": float(np.median(med_p)), "session_ms_median": float(np.median(med_s)),
        "results_equal": bool(equal),
        # per frame, all sequences; the parent's figures are for a frame that matches and runs the VP stage
        "parent_bytes_down": n_seq * (PX + 2 * PX + 2 * LB + 16 + 2 * 16 * ML + 16), "parent_bytes_up": n_seq * (PX + LB + 8 + 4 * ML + 8 + 4 * ML + 76),
        "session_bytes_down": n_seq * (PX + 4), "session_bytes_up": n_seq * rec,
        "parent_kernels": 22 * n_seq, "parent_copies": 24 * n_seq, "parent_synchronisations": 8 * n_seq,
        "session_kernels": 26, "session_copies": 2, "session_synchronisations": 1,
    }


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seq", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    frames = np.load(os.path.join(ROOT, "tests", "golden", "mh04_frames.npz"))["frames"]
    for n in a.n_seq:
        print(json.dumps(measure(frames, n, a.reps)), flush=True)
