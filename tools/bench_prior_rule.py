"""Cost of the prior rule (vpl_ba_set_prior_rule): one context per batch, both rules on it, for
  bench    the benchmark batch: 512 windows of workload.config(200, 80) behind their primed priors (kept block n = 45)
  steady   workload.steady_batch of the same windows (a tenth of the point tracks over all 11 frames: n = 75)
Per rule: device time per batch of k_marg and k_prior_eigen (vpl_ba_enable_kernel_timing, events around every launch) and
whole-solve solves/s (reset_state + solve, graph replay on a stream of the context's own, no timing).

    python tools/bench_prior_rule.py [windows=512] [timed solves=20]
Prints one JSON line per (batch, rule)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import vplines_slam_amd as v

RULES = (("pivoted_cholesky", v.PRIOR_PIVOTED_CHOLESKY), ("eigen", v.PRIOR_EIGEN))


def measure(ctx, nw, steps, label, n_prior):
    for name, rule in RULES:
        ctx.set_prior_rule(rule)
        for _ in range(3):
            ctx.reset_state(); ctx.solve()
        ctx.synchronize()
        reps = 5
        ctx.enable_kernel_timing(True)
        for _ in range(reps):
            ctx.reset_state(); ctx.solve(); ctx.synchronize()
        kt = ctx.kernel_times()
        ctx.enable_kernel_timing(False)
        ctx.reset_state(); ctx.solve(); ctx.synchronize()   # the graph is captured again outside the timed region
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.reset_state(); ctx.solve()
        ctx.synchronize()
        dt = time.perf_counter() - t0
        ms = lambda k: round(kt[k][0] / reps, 4) if k in kt else 0.0
        print(json.dumps(dict(batch=label, windows=nw, n_prior=n_prior, rule=name, k_marg_ms=ms("k_marg"),
                              k_prior_eigen_ms=ms("k_prior_eigen"), k_lin_marg_ms=ms("k_lin_marg"),
                              solve_ms=round(1e3 * dt / steps, 3), solves_per_s=round(nw * steps / dt, 1))), flush=True)


def main():
    nw = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda", 0)
    opt = v.default_options()
    cfg = v.workload.config(200, 80)
    ids = list(range(nw))
    st = torch.cuda.Stream(dev)
    for label in ("bench", "steady"):
        pobs = v.workload.steady_point_obs(cfg) if label == "steady" else cfg.n_points * cfg.track_len
        ctx = v.Context(device=0, max_windows=nw, max_points=cfg.n_points, max_point_obs=pobs, max_lines=cfg.n_lines,
                        max_line_obs=cfg.n_lines * cfg.track_len, stream=st.cuda_stream)
        if label == "steady":
            B, n_prior = v.workload.steady_batch(ctx, ids, cfg, opt)
        else:
            B, keep = v.workload.primed_batch(ctx, ids, cfg, opt)
            ctx.upload(B, opt)
            n_prior = int(round(sum(keep[i].n for i in range(nw)) / nw))
        measure(ctx, nw, steps, label, n_prior)
        ctx.close()


if __name__ == "__main__":
    main()
