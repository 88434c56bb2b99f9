"""Secondary benchmark (bench.py is the flagship): the point tracker session, vpl_ptrk_frame, on the golden EuRoC frames at
n_seq = 1, 16 and 64 cameras per call.  Every camera sees the 15 frames in order (camera k starts at frame k mod 15) and
publishes every image, so each call runs CLAHE, LK, the border test, rejectWithF, setMask, detection, undistortedPoints and
updateID for n_seq images.  Reported: ms per call and per image and images/s from the wall clock around the whole call (packing,
both copies, the synchronisation), the median over the timed calls, with the spread; and the device time per kernel from
hipEvents around each launch (vpl_fe_kernel_times), taken in calls of their own because the events serialise the launches.
Prints one JSON line.

  python tools/bench_points.py [--calls 45] [--warmup 15]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import vplines_slam_amd as v  # noqa: E402

CAM = (458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)   # EuRoC cam0


def measure(frames, n_seq, calls, warmup):
    H, W = frames.shape[1:]
    fe = v.frontend.FrontendContext(max_images=2 * n_seq, width=W, height=H, max_lines=64)
    fe.pt_reserve(max_candidates=8192, max_corners=160, max_points=160)
    trk = v.PointTrackerSession(fe, n_seq, v.default_point_tracker_options(CAM))
    pub = np.ones(n_seq, np.int32)
    step = [0]

    def call():
        k = step[0]
        step[0] += 1
        raw = np.stack([frames[(k + s) % len(frames)] for s in range(n_seq)])
        t = time.perf_counter()
        r = trk.frame(raw, np.full(n_seq, 0.05 * (k + 1)), pub, np.arange(n_seq, dtype=np.uint64) + 1000 * k)
        return (time.perf_counter() - t) * 1e3, r

    for _ in range(warmup):
        call()
    wall, published = [], []
    for _ in range(calls):
        ms, r = call()
        wall.append(ms)
        published.append(statistics.mean(x["published"] for x in r))
    per = {}
    for _ in range(10):
        fe.enable_kernel_timing(True)      # clears the record
        call()
        for name, ms in fe.kernel_times().items():
            per.setdefault(name, []).append(ms)
    fe.enable_kernel_timing(False)
    fe.close()
    med = statistics.median(wall)
    kern = {k: round(statistics.median(x), 4) for k, x in per.items()}
    return dict(n_seq=n_seq, calls=calls, ms_per_call=round(med, 4), ms_per_call_min=round(min(wall), 4), ms_per_call_max=round(max(wall), 4),
                ms_per_image=round(med / n_seq, 4), images_per_s=round(1e3 * n_seq / med, 1),
                mean_points_published=round(statistics.mean(published), 1), kernels_ms=kern, device_ms_per_call=round(sum(kern.values()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=45)
    ap.add_argument("--warmup", type=int, default=15)
    a = ap.parse_args()
    frames = np.load(os.path.join(ROOT, "tests", "golden", "mh04_frames.npz"))["frames"]
    rows = [measure(frames, n, a.calls, a.warmup) for n in (1, 16, 64)]
    print(json.dumps(dict(bench="points", what="vpl_ptrk_frame", calls=a.calls, warmup=a.warmup, results=rows)))


if __name__ == "__main__":
    main()
