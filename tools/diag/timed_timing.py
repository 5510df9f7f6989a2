"""Cost of the calls on time-indexed policies (ops.value_horizon,
ops.rollout_horizon) on one MI355X.  In one process and one run:

  value_horizon          the planner's shape
  value_horizon/fused    forced fused (IRLMX_HORIZON_FUSED_BATCH=1: several states per thread at any batch)
  value_horizon/sweep    forced per sweep (IRLMX_FUSED_MAX_STATES=0)

on 64x64 at T = 16 with 1 and with 256 instances, under the non-causal pi_t and
without a policy (the optimal value); and

  rollout_horizon        B = 64, N = 200, T = 256 on 16x16 under a stationary policy repeated T times
  rollout                ops.rollout on the same policy at max_len = T: the same trajectories

HIP events around windows of back-to-back calls on the current stream, every
shape warmed up first, the passes alternating window by window; the median over
the windows is printed.  A record, not a threshold: compare only within one run
(profiles/timed.txt is one).

usage: python tools/diag/timed_timing.py [--windows N] [--calls N]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "irl-maxent_amd")]
import torch  # noqa: E402
from irlmx import DeviceMDP, ops  # noqa: E402

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


def forced(fn, key, value):
    def run():
        os.environ[key] = value
        try:
            return fn()
        finally:
            del os.environ[key]
    return run


def measure(passes, windows, calls, dev):
    for fn in passes.values():                      # warm-up (code objects, allocator)
        fn()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in passes}
    for _ in range(windows):
        for k, fn in passes.items():
            times[k].append(window_ms(fn, calls))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("timed_timing: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(dev)}; windows per pass: {args.windows}; calls per window: {args.calls}")
    size, T = 64, 16
    S = size * size
    for B in (1, 256):
        mdp = DeviceMDP.icy_gridworld(size, [0.2] * B, device=dev)
        r = torch.as_tensor(np.random.default_rng(size).uniform(-1.0, 0.0, (B, S)), device=dev)
        pi = ops.backward_maxent_horizon(mdp, r, T)
        plan = ops.execution_plan(mdp, "value_horizon")
        print(f"value_horizon {size}x{size} x {B} (S = {S}, T = {T}); the planner's shape: {plan['shape']} "
              f"(threads {plan['threads']}, spt {plan['spt']})")
        for label, p in (("policy", pi), ("optimal", None)):
            base = lambda p=p: ops.value_horizon(mdp, r, T, p, 0.9)          # noqa: E731
            got = measure({"value_horizon": base, "value_horizon/fused": forced(base, BATCH_KEY, "1"),
                           "value_horizon/sweep": forced(base, KEY, "0")}, args.windows, args.calls, dev)
            for k, (med, lo, hi) in got.items():
                print(f"  {label:8s} {k:20s} {med:9.4f} ms per call (min {lo:.4f}, max {hi:.4f})  "
                      f"{1e3 * med / T:8.2f} us per step")
            print(f"  {label:8s} fused / per sweep {got['value_horizon/fused'][0] / got['value_horizon/sweep'][0]:.2f}",
                  flush=True)
        del pi
        torch.cuda.empty_cache()
    B, N, T, size = 64, 200, 256, 16
    S = size * size
    mdp = DeviceMDP.icy_gridworld(size, [0.2] * B, device=dev)
    r = torch.as_tensor(np.random.default_rng(1).uniform(-1.0, 0.0, (B, S)), device=dev)
    pi0 = ops.soft_backward_horizon(mdp, r, 0.9, 1)[:, 0].contiguous()
    tiled = pi0.unsqueeze(1).expand(B, T, S, 4).contiguous()
    none = torch.zeros((B, S), dtype=torch.uint8, device=dev)
    start = torch.as_tensor(np.random.default_rng(2).integers(0, S, (B, N)), device=dev)
    a = ops.rollout_horizon(mdp, tiled, start, N, 5)
    b = ops.rollout(mdp, pi0, none, start, N, T, 5)
    assert torch.equal(a.visits, b.visits) and torch.equal(a.lengths, b.lengths)
    got = measure({"rollout_horizon": lambda: ops.rollout_horizon(mdp, tiled, start, N, 5),
                   "rollout": lambda: ops.rollout(mdp, pi0, none, start, N, T, 5)}, args.windows, args.calls, dev)
    print(f"rollouts {size}x{size} x {B}, N = {N}, T = {T} ({B * N} trajectories; pi_t {B * T * S * 4 * 8 / 2 ** 20:.0f} MiB)")
    for k, (med, lo, hi) in got.items():
        print(f"  {k:20s} {med:9.4f} ms per call (min {lo:.4f}, max {hi:.4f})")
    print(f"  rollout_horizon / rollout {got['rollout_horizon'][0] / got['rollout'][0]:.2f}")


if __name__ == "__main__":
    main()
