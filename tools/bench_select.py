"""Secondary benchmark (bench.py is the flagship): device time of the feature selector, vpl_select_features_batch, per call and
per kernel, from hipEvents around each launch (vpl_ba_enable_kernel_timing), for
  64 sequences x 200 candidates x kappa 50   and   1 x 200 x 50
(100 used features and a cloud of 120 each).  Warm-up calls first, then the median over --reps calls; the wall clock of a whole
call (packing, allocation, the copies, the synchronisation) is reported next to it.  Prints one JSON line.

  python tools/bench_select.py [--reps 20] [--warmup 3]"""
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

import numpy as np  # noqa: E402

import select_inputs as si  # noqa: E402
import vplines_slam_amd as v  # noqa: E402

KERNELS = ("k_sel_prep", "k_sel_info", "k_sel_greedy")


def clocks():
    """the clocks as rocm-smi shows them, for the record (nothing is set)"""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:2]
    except Exception as e:  # noqa: BLE001
        return ["unavailable: %s" % type(e).__name__]


def scenes(n):
    """n sequences of the bench shape, each its own random scene"""
    out = []
    for k in range(n):
        s = si.random_scene(1000 + k, 200, 100, 120, 50)
        out.append(v.SelectInput.of(s))
    return out


def measure(ctx, par, inputs, reps, warmup):
    for _ in range(warmup):
        ctx.select_features(par, inputs)
    ctx.enable_kernel_timing(True)
    per = {k: [] for k in KERNELS}
    total = []
    for _ in range(reps):
        before = ctx.kernel_times()
        res = ctx.select_features(par, inputs)
        after = ctx.kernel_times()
        ms = {k: after[k][0] - before.get(k, (0.0, 0))[0] for k in KERNELS}
        for k in KERNELS:
            per[k].append(ms[k])
        total.append(sum(ms.values()))
    ctx.enable_kernel_timing(False)
    wall = []
    for _ in range(reps):
        t = time.perf_counter()
        ctx.select_features(par, inputs)
        wall.append((time.perf_counter() - t) * 1e3)
    return dict(sequences=len(inputs), candidates=200, kappa=50, selected=[int(len(r["ids"])) for r in res][:4],
                device_ms=round(statistics.median(total), 4), kernels_ms={k: round(statistics.median(per[k]), 4) for k in KERNELS},
                device_ms_min=round(min(total), 4), device_ms_max=round(max(total), 4), wall_ms=round(statistics.median(wall), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    par = si.params()
    ctx = v.Context(device=0, max_windows=64, max_points=8, max_point_obs=64, max_lines=8, max_line_obs=64)
    c0 = clocks()
    rows = [measure(ctx, par, scenes(n), a.reps, a.warmup) for n in (64, 1)]
    ctx.close()
    print(json.dumps(dict(bench="select", reps=a.reps, warmup=a.warmup, clocks_before=c0, clocks_after=clocks(), results=rows)))


if __name__ == "__main__":
    main()
