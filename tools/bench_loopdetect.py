"""Secondary benchmark (bench.py is the flagship): one LoopDetector.detect -- vpl_ld_detect, PoseGraph::detectLoop -- against a
database of 256, 1024 and 4096 stored keyframes of about 3000 descriptors each, on a generated k = 10, L = 6 vocabulary (10^6
words; the reference's brief_k10L6.bin is not available).  Wall clock around the whole call (packing, both copies, the
synchronisation), the median over the timed calls with the spread, and the device time per kernel from hipEvents around each
launch, taken in calls of their own.  Every timed call stores one more keyframe, so a size is the size at the first timed call.
Every size runs in a child process of its own under a time limit; a size that fails ends the run.  Prints one JSON line.
No figure is a pass mark.

  python tools/bench_loopdetect.py [--calls 20] [--warmup 3] [--limit 600]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, L = 10, 6
FLIPS = (0, 48, 32, 24, 16, 10)       # bits turned from a parent to its child, per level (level 1: random)
N_DESC, N_PLACES, NOISE_BITS = 3000, 600, 4
SIZES = (256, 1024, 4096)


def turn_bits(np, rng, d, n_bits):
    """d [n][4] uint64 with n_bits random bit positions of every row turned (a position drawn twice turns back)"""
    rows = np.arange(len(d))
    for _ in range(n_bits):
        pos = rng.integers(0, 256, len(d))
        d[rows, pos >> 6] ^= np.uint64(1) << (pos & 63).astype(np.uint64)
    return d


def vocabulary(np, v):
    """the k-ary tree numbered breadth first; a child's descriptor is its parent's with FLIPS[level] bits turned; leaf weights
    log-uniform in [0.01, 10] (the spread of an idf), inner weights 0"""
    rng = np.random.default_rng(1)
    desc, parent, first = [], [], 1
    level = rng.integers(0, 1 << 63, (K, 4)).astype(np.uint64) << np.uint64(1) | rng.integers(0, 2, (K, 4)).astype(np.uint64)
    ids = np.arange(first, first + K)
    desc.append(level); parent.append(np.zeros(K, np.int64))
    for lv in range(1, L):
        first += len(ids)
        level = turn_bits(np, rng, np.repeat(level, K, axis=0), FLIPS[lv])
        parent.append(np.repeat(ids, K))
        ids = np.arange(first, first + len(level))
        desc.append(level)
    desc, parent = np.concatenate(desc), np.concatenate(parent)
    n, n_words = len(desc), len(ids)
    weight = np.zeros(n)
    weight[-n_words:] = np.exp(rng.uniform(np.log(0.01), np.log(10.0), n_words))
    return v.Vocabulary(K, L, np.arange(1, n + 1), parent, weight, desc, ids, rng.permutation(n_words)), level


def step(size, a):
    import numpy as np
    import vplines_slam_amd as v
    voc, leaves = vocabulary(np, v)
    rng = np.random.default_rng(2)
    places = rng.integers(0, len(leaves), (N_PLACES, N_DESC))          # a place shows these leaves; a keyframe is a place seen with noise

    def keyframe():
        return turn_bits(np, rng, leaves[places[rng.integers(N_PLACES)]].copy(), NOISE_BITS)

    total = size + a.calls + a.warmup + 16
    fe = v.frontend.FrontendContext(max_images=1, width=64, height=48, max_lines=64)
    ld = v.LoopDetector(fe, 1, max_keyframes=total, max_keypoints=8192, max_words_total=total * N_DESC)
    t = time.perf_counter()
    ld.set_vocabulary(voc)
    set_ms = (time.perf_counter() - t) * 1e3
    for _ in range(size):
        ld.add([keyframe()])
    frames = [keyframe() for _ in range(a.calls + a.warmup + 10)]
    it = iter(frames)
    last = {}

    def call():
        last["r"] = ld.detect([next(it)], [ld.size(0)])[0]

    for _ in range(a.warmup):
        call()
    wall = []
    for _ in range(a.calls):
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
    per = {}
    for _ in range(10):
        fe.enable_kernel_timing(True)      # clears the record
        call()
        for name, ms in fe.kernel_times().items():
            per.setdefault(name, []).append(ms)
    fe.enable_kernel_timing(False)
    kern = {k: round(statistics.median(x), 4) for k, x in per.items()}
    r = dict(stored_keyframes=size, descriptors=N_DESC, words_in_bag=last["r"]["n_words"], results=len(last["r"]["ids"]),
             ms_per_call=round(statistics.median(wall), 4), ms_per_call_min=round(min(wall), 4), ms_per_call_max=round(max(wall), 4),
             kernels_ms=kern, device_ms_per_call=round(sum(kern.values()), 4), set_vocabulary_ms=round(set_ms, 1))
    fe.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=600, help="seconds a size may take")
    ap.add_argument("--size", type=int)
    a = ap.parse_args()
    if a.size:                                   # the child: one size on the GPU
        print("RESULT " + json.dumps(step(a.size, a)))
        return 0
    results = {}
    for size in SIZES:                           # the parent never touches the GPU
        cmd = [sys.executable, os.path.abspath(__file__), "--size", str(size), "--calls", str(a.calls), "--warmup", str(a.warmup)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            results[size] = dict(error="time limit of %d s" % a.limit)
            break
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            results[size] = dict(error="exit status %d" % p.returncode, stderr=p.stderr[-2000:])
            break
        results[size] = json.loads(line[-1][len("RESULT "):])
    print(json.dumps(dict(bench="loopdetect", k=K, L=L, calls=a.calls, warmup=a.warmup, results=results)))
    return 0 if all("error" not in r for r in results.values()) and len(results) == len(SIZES) else 1


if __name__ == "__main__":
    sys.exit(main())
