"""Secondary benchmark (bench.py is the flagship): the pose-graph session vpl_pgs_*, PoseGraph's keyframe list on the device.
  add        per-keyframe cost of vpl_pgs_add_keyframe with the record copied back (out) and without (out = NULL; the stream is
             synchronised once behind the last one), us per keyframe
  n256 / n1024 / n4096
             vpl_pgs_optimize with that many resident nodes in the range (one loop every 16 nodes), ms per call -- and the same
             graph through vpl_pg_optimize_batch from host arrays, which is what a caller has to do without the session: every
             pose uploaded, every pose read back
Wall clock around the whole call, the median over the timed calls with the spread.  A session's optimisation consumes its queue,
so every timed call runs on a session filled afresh (the filling is not timed).  The graphs are those of
tools/bench_posegraph.py: circles walked twice with a VIO drift and loop edges measured on the truth.  Every step runs in a child
process of its own under a time limit; a step that fails ends the run.  Prints one JSON line.

  python tools/bench_pgsession.py [--calls 10] [--warmup 2] [--limit 240]"""
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

STEPS = dict(add=2048, n256=256, n1024=1024, n4096=4096)


def graph(n):
    import numpy as np
    import pg_inputs
    import pg_ref
    n_loops = n // 16
    first = n - 2 * n_loops
    # the first loop onto node 0 and the last one at node n-1: the whole list is the range, as in the batch call beside it
    loops = [(first + 2 * k + 1, (k * (first - 2)) // n_loops) for k in range(n_loops)]
    g = pg_inputs.make_graph(n, loops, 100, turns=2.0, yaw_drift=20.0 / n, t_drift=(0.8 / n, -0.6 / n, 0.1 / n), noise=0.003, radius=0.05 * n)
    for i in range(n):
        g["loop_info"][i, 3:7] = pg_ref.mat2q(np.eye(3))
    return g


def fill(s, g):
    for k in range(len(g["vio_T"])):
        a = int(g["loop_local"][k])
        s.add(1, g["vio_T"][k], g["vio_R"][k], a, g["loop_info"][k] if a >= 0 else None, out=False)


def spread(x):
    return dict(median=round(statistics.median(x), 3), min=round(min(x), 3), max=round(max(x), 3))


def step(a):
    import vplines_slam_amd as v
    n = STEPS[a.step]
    g = graph(n)
    ctx = v.Context(device=0, max_windows=1)
    out = {}
    if a.step == "add":
        for mode in ("out", "null"):
            per = []
            for it in range(a.warmup + a.calls):
                with v.PoseGraphSession(ctx, v.default_pgs_options(max_keyframes=n)) as s:
                    t = time.perf_counter()
                    for k in range(n):
                        s.add(1, g["vio_T"][k], g["vio_R"][k], out=mode == "out")
                    s.drift()                                    # (one synchronisation behind the last launch)
                    per.append((time.perf_counter() - t) * 1e6 / n)
            out["us_per_keyframe_" + mode] = spread(per[a.warmup:])
        out["keyframes"] = n
    else:
        item = v.PoseGraphInput(g["vio_T"], g["vio_R"], g["loop_local"], g["loop_info"])
        sess, batch, res = [], [], None
        with v.PoseGraphSession(ctx, v.default_pgs_options(max_keyframes=n)) as s:
            for it in range(a.warmup + a.calls):
                s.reset()
                fill(s, g)
                s.drift()
                t = time.perf_counter()
                res = s.optimize()
                sess.append((time.perf_counter() - t) * 1e3)
                t = time.perf_counter()
                ref = ctx.pose_graph_optimize([item])[0]
                batch.append((time.perf_counter() - t) * 1e3)
            same = s.path()["T"].tobytes() == ref.T.tobytes()
        out = dict(nodes=n, loops=n // 16, iterations=res.iterations, session_ms=spread(sess[a.warmup:]), batch_from_host_ms=spread(batch[a.warmup:]),
                   same_poses=bool(same))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--step", choices=sorted(STEPS))
    a = ap.parse_args()
    if a.step:                                       # the child: one step on the GPU
        print("RESULT " + json.dumps(step(a)))
        return 0
    results = {}
    for name in ("add", "n256", "n1024", "n4096"):   # the parent never touches the GPU
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
    print(json.dumps(dict(bench="pgsession", **results)))
    return 1 if any("error" in r for r in results.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
