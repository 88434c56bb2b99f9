"""Secondary benchmark (bench.py is the flagship): vpl_pg_optimize_batch, PoseGraph::optimize4DoF on the device.
  single   one graph of 1000 nodes with 200 loops: ms per call
  batch    64 graphs of 200 nodes with 40 loops each in one call: ms per call, graphs/s
Wall clock around the whole call (planning, packing, both copies, the synchronisation), the median over the timed calls with the
spread; then the device time per kernel from hipEvents around each launch, taken in calls of their own (the events serialise the
launches, so their sum is not the call's time).  The graphs are circles walked twice with a VIO drift in yaw and position and loop
edges measured on the truth (tests/pg_inputs.py:make_graph).  Every step runs in a child process of its own under a time limit; a
step that fails ends the run.  Prints one JSON line.

  python tools/bench_posegraph.py [--calls 20] [--warmup 3] [--limit 240]"""
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

SHAPES = dict(single=(1, 1000, 200), batch=(64, 200, 40))


def graphs(count, n, n_loops):
    import vplines_slam_amd as v
    import pg_inputs
    out = []
    for s in range(count):
        first = n - 2 * n_loops                      # the last 2 L nodes hold the loops, every other one, onto spread-out old nodes
        loops = [(first + 2 * k, 1 + (k * (first - 2)) // n_loops) for k in range(n_loops)]
        g = pg_inputs.make_graph(n, loops, 100 + s, turns=2.0, yaw_drift=20.0 / n, t_drift=(0.8 / n, -0.6 / n, 0.1 / n), noise=0.003,
                                 radius=0.05 * n)
        out.append(v.PoseGraphInput(g["vio_T"], g["vio_R"], g["loop_local"], g["loop_info"]))
    return out


def step(a):
    import vplines_slam_amd as v
    count, n, n_loops = SHAPES[a.step]
    items = graphs(count, n, n_loops)
    ctx = v.Context(device=0, max_windows=count)
    out = {}

    def call():
        out["r"] = ctx.pose_graph_optimize(items)

    for _ in range(a.warmup):
        call()
    wall = []
    for _ in range(a.calls):
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
    per = {}
    for _ in range(5):
        ctx.enable_kernel_timing(True)               # clears the record
        call()
        for name, (ms, launches) in ctx.kernel_times().items():
            per.setdefault(name, []).append(ms)
    ctx.enable_kernel_timing(False)
    res = out["r"]
    ctx.close()
    ms = statistics.median(wall)
    return dict(graphs=count, nodes=n, loops=n_loops, ms_per_call=round(ms, 3), ms_per_call_min=round(min(wall), 3),
                ms_per_call_max=round(max(wall), 3), graphs_per_s=round(1e3 * count / ms, 1),
                mean_iterations=round(statistics.mean(r.iterations for r in res), 2),
                kernels_ms_per_call={k: round(statistics.median(x), 4) for k, x in per.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--step", choices=sorted(SHAPES))
    a = ap.parse_args()
    if a.step:                                       # the child: one step on the GPU
        print("RESULT " + json.dumps(step(a)))
        return 0
    results = {}
    for name in ("single", "batch"):                 # the parent never touches the GPU
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
    print(json.dumps(dict(bench="posegraph", **results)))
    return 1 if any("error" in r for r in results.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
