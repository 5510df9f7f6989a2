"""Cost of the finite-horizon soft value iteration (ops.soft_backward_horizon)
on one MI355X: the routing table.  Per model, in one process and one run,

  soft_horizon          the planner's shape
  soft_horizon/fused    forced fused (IRLMX_HORIZON_FUSED_BATCH=1: several states per thread at any batch)
  soft_horizon/sweep    forced per sweep (IRLMX_FUSED_MAX_STATES=0)
  soft_backward         ops.soft_backward with eps = 0 and max_iter = T on the same
                        model: time / T sweeps -- the stationary pass's sweep does
                        the same dots and softmax folds, without the T policy rows

at T = 128 on the models of the non-causal table (profiles/horizon.txt): 16x16 x
64, 32x32 x 1 / x 64, 45x45 x 1 / x 64, 64x64 x 1 / 16 / 64 / 256.  HIP events
around windows of back-to-back calls on the current stream, every shape warmed
up first, the passes alternating window by window; the median over the windows
is printed with each plan, and fused / per sweep per model.  A record, not a
threshold: compare only within one run.

usage: python tools/diag/soft_horizon_cost.py [--windows N] [--discount G] [--points size:instances:T:calls,...]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "irl-maxent_amd")]
import torch  # noqa: E402
from irlmx import DeviceMDP, ops  # noqa: E402

# size, instances, T, calls per window
POINTS = ((16, 64, 128, 4), (32, 1, 128, 4), (32, 64, 128, 4), (45, 1, 128, 4), (45, 64, 128, 2), (64, 1, 128, 4),
          (64, 16, 128, 2), (64, 64, 128, 2), (64, 256, 128, 1))
KEY = "IRLMX_FUSED_MAX_STATES"            # 0: per sweep
BATCH_KEY = "IRLMX_HORIZON_FUSED_BATCH"   # 1: fused also with several states per thread


def window_ms(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def plan_text(p):
    return f"{p['shape']} threads {p['threads']} spt {p['spt']} launches {p['launches']}"


def forced(fn, key, value):
    def run():
        os.environ[key] = value
        try:
            return fn()
        finally:
            del os.environ[key]
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--discount", type=float, default=0.9)
    ap.add_argument("--points", default=None, help="size:instances:T:calls,... instead of the points above")
    args = ap.parse_args()
    points = POINTS if args.points is None else [tuple(int(v) for v in p.split(":")) for p in args.points.split(",")]
    if not torch.cuda.is_available():
        sys.exit("soft_horizon_cost: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    g = args.discount
    print(f"device: {torch.cuda.get_device_name(dev)}; windows per pass: {args.windows}; discount {g}")
    table = []
    for size, B, T, calls in points:
        S = size * size
        mdp = DeviceMDP.icy_gridworld(size, [0.2] * B, device=dev)
        r = torch.as_tensor(np.random.default_rng(size).uniform(-1.0, 0.0, (B, S)), device=dev)
        phi = torch.full((B, S), -float("inf"), dtype=torch.float64, device=dev)
        phi[:, S - 1] = 0.0
        base = lambda: ops.soft_backward_horizon(mdp, r, g, T)          # noqa: E731
        passes = {"soft_horizon": (base, T),
                  "soft_horizon/fused": (forced(base, BATCH_KEY, "1"), T),
                  "soft_horizon/sweep": (forced(base, KEY, "0"), T),
                  "soft_backward": (lambda: ops.soft_backward(mdp, r, phi, g, eps=0.0, max_iter=T), T)}
        plans = {"soft_horizon": ops.execution_plan(mdp, "soft_backward_horizon"),
                 "soft_backward": ops.execution_plan(mdp, "soft_backward")}
        for fn, _ in passes.values():                      # warm-up (code objects, allocator)
            fn()
        torch.cuda.synchronize(dev)
        times = {k: [] for k in passes}
        for _ in range(args.windows):
            for k, (fn, _) in passes.items():
                times[k].append(window_ms(fn, calls))
        med = {k: statistics.median(v) for k, v in times.items()}
        us = {k: 1e3 * med[k] / passes[k][1] for k in passes}
        print(f"{size}x{size} x {B} (S = {S}, T = {T}, {calls} calls per window; pi_t {B * T * S * 4 * 8 / 2 ** 20:.0f} MiB)")
        for k in passes:
            plan = plan_text(plans[k]) if k in plans else "(forced)"
            print(f"  {k:20s} {med[k]:10.3f} ms per call (min {min(times[k]):.3f}, max {max(times[k]):.3f})  "
                  f"{us[k]:8.2f} us per step of {passes[k][1]}  plan: {plan}")
        ratio = med["soft_horizon/fused"] / med["soft_horizon/sweep"]
        print(f"  fused / per sweep {ratio:.2f}; soft_horizon step / soft_backward sweep "
              f"{us['soft_horizon'] / us['soft_backward']:.2f}", flush=True)
        table.append((f"{size}x{size} x {B}", us["soft_horizon/fused"], us["soft_horizon/sweep"], ratio,
                      plans["soft_horizon"]["shape"], us["soft_backward"]))
        torch.cuda.empty_cache()
    print("routing table (us per step):  model, fused, per sweep, fused / per sweep, the planner's shape, soft_backward sweep")
    for name, f, s, ratio, shape, sb in table:
        print(f"  {name:14s} {f:8.2f} {s:8.2f} {ratio:6.2f}  {shape:6s} {sb:8.2f}")


if __name__ == "__main__":
    main()
