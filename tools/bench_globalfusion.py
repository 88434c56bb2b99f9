"""Secondary benchmark (bench.py is the flagship): vpl_gf_optimize_batch, GlobalOptimization::optimize on the device.
  long_S32 | long_S64 | long_S128   one chain of 16384 nodes with a fix every 10th node, 5 iterations, the substructured solve
  long_serial                        the same chain with S > n: one segment, the serial chain -- the yardstick
  batch                              64 chains of 512 nodes in one call (default S)
Wall clock around the whole call (planning, packing, both copies, the synchronisation), the median over the timed calls with the
spread; then the device time per timer name from hipEvents around each group of launches, taken in calls of their own (the events
serialise the launches, so their sum is not the call's time).  The chains are circles with a VIO drift in yaw and position and
fixes on the truth plus noise (tests/gf_inputs.py:make_chain).  Every step runs in a child process of its own under a time limit; a
step that fails ends the run.  Prints one JSON line.

  python tools/bench_globalfusion.py [--calls 10] [--warmup 2] [--limit 240] [--steps long_S64,batch]"""
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

LONG = 16384
SHAPES = dict(long_S32=(1, LONG, 32), long_S64=(1, LONG, 64), long_S128=(1, LONG, 128), long_serial=(1, LONG, LONG + 1), batch=(64, 512, 0))


def chains(count, n):
    import vplines_slam_amd as v
    import gf_inputs
    out = []
    for s in range(count):
        g = gf_inputs.make_chain(n, range(0, n, 10), 100 + s, turns=n / 400.0, radius=30.0, yaw_drift=0.5 / n, t_drift=(8.0 / n, -6.0 / n, 1.0 / n),
                                 noise=0.05, accuracy=0.5)
        out.append(v.GlobalFusionInput(g["local"], g["glob"], g["gps_node"], g["gps_xyz"], g["gps_accuracy"]))
    return out


def step(a):
    import vplines_slam_amd as v
    count, n, S = SHAPES[a.step]
    items = chains(count, n)
    opt = v.default_gf_options(segment=S)
    ctx = v.Context(device=0, max_windows=count)
    out = {}

    def call():
        out["r"] = ctx.global_fusion(items, opt)

    for _ in range(a.warmup):
        call()
    wall = []
    for _ in range(a.calls):
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
    per = {}
    for _ in range(3):
        ctx.enable_kernel_timing(True)               # clears the record
        call()
        for name, (ms, launches) in ctx.kernel_times().items():
            per.setdefault(name, []).append(ms)
    ctx.enable_kernel_timing(False)
    res = out["r"]
    ctx.close()
    ms = statistics.median(wall)
    return dict(chains=count, nodes=n, segment=S, ms_per_call=round(ms, 3), ms_per_call_min=round(min(wall), 3),
                ms_per_call_max=round(max(wall), 3), chains_per_s=round(1e3 * count / ms, 1),
                mean_iterations=round(statistics.mean(r.iterations for r in res), 2),
                final_cost_chain0=res[0].final_cost,
                kernels_ms_per_call={k: round(statistics.median(x), 4) for k, x in per.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--steps", default="long_S32,long_S64,long_S128,long_serial,batch")
    ap.add_argument("--step", choices=sorted(SHAPES))
    a = ap.parse_args()
    if a.step:                                       # the child: one step on the GPU
        print("RESULT " + json.dumps(step(a)))
        return 0
    results = {}
    for name in a.steps.split(","):                  # the parent never touches the GPU
        # the serial chain is some hundred times slower per call: fewer calls of it
        calls, warmup = (max(a.calls // 5, 2), 1) if name == "long_serial" else (a.calls, a.warmup)
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--calls", str(calls), "--warmup", str(warmup)]
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
    print(json.dumps(dict(bench="globalfusion", **results)))
    return 1 if any("error" in r for r in results.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
