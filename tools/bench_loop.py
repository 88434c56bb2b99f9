"""Secondary benchmark (bench.py is the flagship): the loop-closure calls on the golden EuRoC frames (752 x 480).
  keyframe  vpl_lc_keyframe_batch on 16 frames per call, 150 window points each, FAST threshold 20: frames/s
  match     vpl_lc_match_batch on 16 pairs per call, 150 window descriptors against a frame's whole corner list: pairs/s
  verify    vpl_loop_verify_batch on 64 items per call, 60 points with 30 % outliers (about 25 RANSAC iterations each): items/s
Wall clock around the whole call (packing, both copies, the synchronisation), the median over the timed calls with the spread;
for the two front-end calls also the device time per kernel from hipEvents around each launch, taken in calls of their own.
Every step runs in a child process of its own under a time limit; a step that fails ends the run.  Prints one JSON line.

  python tools/bench_loop.py [--calls 30] [--warmup 5] [--limit 120]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CAM = (458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)   # EuRoC cam0
N_FRAMES, N_WINDOW, N_ITEMS = 16, 150, 64


def timed(call, calls, warmup):
    for _ in range(warmup):
        call()
    wall = []
    for _ in range(calls):
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
    return dict(ms_per_call=round(statistics.median(wall), 4), ms_per_call_min=round(min(wall), 4), ms_per_call_max=round(max(wall), 4))


def kernel_times(fe, call):
    per = {}
    for _ in range(10):
        fe.enable_kernel_timing(True)      # clears the record
        call()
        for name, ms in fe.kernel_times().items():
            per.setdefault(name, []).append(ms)
    fe.enable_kernel_timing(False)
    return {k: round(statistics.median(x), 4) for k, x in per.items()}


def frontend(np, v):
    frames = np.load(os.path.join(ROOT, "tests", "golden", "mh04_frames.npz"))["frames"]
    frames = np.ascontiguousarray(np.concatenate([frames, frames])[:N_FRAMES])
    pat = np.load(os.path.join(ROOT, "tests", "golden", "brief_pattern.npz"))
    fe = v.frontend.FrontendContext(max_images=N_FRAMES, width=frames.shape[2], height=frames.shape[1], max_lines=64)
    fe.lc_reserve(8192, 160)
    fe.lc_set_pattern(pat["x1"], pat["y1"], pat["x2"], pat["y2"])
    cam = v.frontend.PointCamera(*CAM)
    first = fe.lc_keyframe(frames, [np.zeros((0, 2))] * N_FRAMES, cam)
    win = [k["keypoints"][:: max(len(k["keypoints"]) // N_WINDOW, 1)][:N_WINDOW] for k in first]
    return fe, frames, cam, win


def step_keyframe(a):
    import numpy as np
    import vplines_slam_amd as v
    fe, frames, cam, win = frontend(np, v)
    call = lambda: fe.lc_keyframe(frames, win, cam)
    r = timed(call, a.calls, a.warmup)
    kern = kernel_times(fe, call)
    corners = [len(k["keypoints"]) for k in call()]
    fe.close()
    r.update(frames_per_call=N_FRAMES, frames_per_s=round(1e3 * N_FRAMES / r["ms_per_call"], 1), mean_corners=round(statistics.mean(corners), 1),
             kernels_ms=kern, device_ms_per_call=round(sum(kern.values()), 4))
    return r


def step_match(a):
    import numpy as np
    import vplines_slam_amd as v
    fe, frames, cam, win = frontend(np, v)
    kf = fe.lc_keyframe(frames, win, cam)
    old = [kf[(i + 1) % N_FRAMES] for i in range(N_FRAMES)]       # every frame against its successor
    args = ([k["window_brief"] for k in kf], [o["brief"] for o in old], [o["keypoints"] for o in old], [o["keypoints_norm"] for o in old])
    call = lambda: fe.lc_match(*args)
    r = timed(call, a.calls, a.warmup)
    kern = kernel_times(fe, call)
    accepted = [int(m["status"].sum()) for m in call()]
    fe.close()
    r.update(pairs_per_call=N_FRAMES, pairs_per_s=round(1e3 * N_FRAMES / r["ms_per_call"], 1), window_descriptors=N_WINDOW,
             mean_old_descriptors=round(statistics.mean(len(o["brief"]) for o in old), 1), mean_accepted=round(statistics.mean(accepted), 1),
             kernels_ms=kern)
    return r


def step_verify(a):
    import numpy as np
    import vplines_slam_amd as v
    import lc_inputs
    items = []
    for i in range(N_ITEMS):
        S = lc_inputs.loop_scene(60, 18, 1000 + i)
        items.append(v.LoopInput(S["pts3d"], S["old_norm"], S["origin_vio_T"], S["origin_vio_R"], lc_inputs.TIC, lc_inputs.QIC, 5000 + i))
    ctx = v.Context(device=0, max_windows=N_ITEMS)
    out = {}

    def call():
        out["r"] = ctx.loop_verify(items)

    r = timed(call, a.calls, a.warmup)
    res = out["r"][0]
    ctx.close()
    r.update(items_per_call=N_ITEMS, items_per_s=round(1e3 * N_ITEMS / r["ms_per_call"], 1),
             mean_ransac_iterations=round(statistics.mean(x.ransac_iterations for x in res), 1), loops_closed=sum(x.has_loop for x in res))
    return r


STEPS = dict(keyframe=step_keyframe, match=step_match, verify=step_verify)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--step", choices=sorted(STEPS))
    a = ap.parse_args()
    if a.step:                                   # the child: one step on the GPU
        print("RESULT " + json.dumps(STEPS[a.step](a)))
        return 0
    results = {}
    for name in ("keyframe", "match", "verify"):   # the parent never touches the GPU
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--calls", str(a.calls), "--warmup", str(a.warmup)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            results[name] = dict(error="time limit of %d s" % a.limit)
            break
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            results[name] = dict(error="exit status %d" % p.returncode, stderr=p.stderr[-2000:])
            break
        results[name] = json.loads(line[-1][len("RESULT "):])
    print(json.dumps(dict(bench="loop", calls=a.calls, warmup=a.warmup, results=results)))
    return 0 if all("error" not in r for r in results.values()) and len(results) == 3 else 1


if __name__ == "__main__":
    sys.exit(main())
