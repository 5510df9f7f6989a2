"""Cost of policy evaluation (ops.policy_evaluation: policy-folded weights, K
fused multiply-adds per state and sweep) beside action-average value iteration
(ops.value_iteration(average=True): A * K per state and sweep) on one MI355X, on
the same inputs -- the uniform policy, so both run the same fixed point -- at
three points:

  16x16 x 64    fused both ways
  64x64 x 1     fused both ways (four states per lane)
  128x128 x 1   policy evaluation per sweep, value iteration on its persistent grid shape

HIP events around windows of back-to-back calls on the current stream; every
shape is warmed up first; the two passes alternate window by window and the
median, minimum and maximum over the windows are printed, with both plans and
sweep counts, and the time per sweep.  A record, not a threshold.

usage: python tools/diag/policy_eval_cost.py [--windows N] [--discount G]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "irl-maxent_amd")]
import torch  # noqa: E402
from irlmx import DeviceMDP, ops  # noqa: E402

POINTS = ((16, 64, 20), (64, 1, 10), (128, 1, 3))   # grid size, instances, calls per window


def window_ms(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def plan_text(p):
    return f"{p['shape']} threads {p['threads']} spt {p['spt']} launches {p['launches']} lds {p['lds_bytes']}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--discount", type=float, default=0.95)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("policy_eval_cost: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    g = args.discount
    print(f"device: {torch.cuda.get_device_name(dev)}; discount {g}, eps 1e-3; windows per pass: {args.windows}")
    for size, B, calls in POINTS:
        S = size * size
        mdp = DeviceMDP.icy_gridworld(size, [0.2] * B, device=dev)
        r = torch.as_tensor(np.random.default_rng(size).uniform(-1.0, 1.0, (B, S)), device=dev)
        pi = torch.full((B, S, 4), 0.25, dtype=torch.float64, device=dev)
        passes = {"policy_evaluation": lambda: ops.policy_evaluation(mdp, r, pi, g),
                  "value_iteration": lambda: ops.value_iteration(mdp, r, g, average=True)}
        plans = {k: ops.execution_plan(mdp, k) for k in passes}
        out = {k: fn() for k, fn in passes.items()}          # warm-up (code objects, allocator), and the check
        torch.cuda.synchronize(dev)
        sweeps = {k: int(v[1].max()) for k, v in out.items()}
        diff = float((out["policy_evaluation"][0] - out["value_iteration"][0]).abs().max())
        times = {k: [] for k in passes}
        for _ in range(args.windows):
            for k, fn in passes.items():
                times[k].append(window_ms(fn, calls))
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"{size}x{size} x {B} (S = {S}, {calls} calls per window), max |v_pe - v_vi| = {diff:.2e}")
        for k in passes:
            print(f"  {k:17s} {med[k]:9.3f} ms per call (min {min(times[k]):.3f}, max {max(times[k]):.3f})  "
                  f"{sweeps[k]} sweeps, {1e3 * med[k] / sweeps[k]:.2f} us per sweep  plan: {plan_text(plans[k])}")
        print(f"  policy_evaluation / value_iteration = {med['policy_evaluation'] / med['value_iteration']:.2f}",
              flush=True)


if __name__ == "__main__":
    main()
