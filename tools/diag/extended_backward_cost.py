"""Cost of the extended-range backward (ops.backward_maxent_extended: one int32
exponent per state, v_ldexp_f64 / v_frexp_* in the sweep) against the ordinary
rescaled backward (ops.backward_maxent) on one MI355X, at three points:

  16x16 x 64    fused both ways
  64x64 x 1     extended fused against the ordinary plan (cluster shape, solo)
  128x128 x 1   extended per sweep (32,767 launches) against the ordinary cluster plan

HIP events around windows of back-to-back calls on the current stream; every
shape is warmed up first; the two passes alternate window by window and the
median, minimum and maximum over the windows are printed, with both plans.
In-range rewards (uniform [-1, 0]): the two passes return the same bits there,
which is checked and printed before timing.  A record, not a threshold.

usage: python tools/diag/extended_backward_cost.py [--windows N]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "irl-maxent_amd")]
import torch  # noqa: E402
from irlmx import DeviceMDP, ops  # noqa: E402

POINTS = ((16, 64, 20), (64, 1, 10), (128, 1, 1))   # grid size, instances, calls per window


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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("extended_backward_cost: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(dev)}; windows per pass: {args.windows}")
    for size, B, calls in POINTS:
        S = size * size
        mdp = DeviceMDP.icy_gridworld(size, [0.2] * B, device=dev)
        r = torch.as_tensor(np.random.default_rng(size).uniform(-1.0, 0.0, (B, S)), device=dev)
        tm = ops.terminal_mask([S - 1], S, batch=B, device=dev)
        passes = {"ordinary": lambda: ops.backward_maxent(mdp, r, tm),
                  "extended": lambda: ops.backward_maxent_extended(mdp, r, tm)}
        plans = {"ordinary": ops.execution_plan(mdp, "backward"),
                 "extended": ops.execution_plan(mdp, "backward", extended_range=True)}
        out = {k: fn() for k, fn in passes.items()}          # warm-up (code objects, allocator), and the check
        torch.cuda.synchronize(dev)
        same = bool(torch.equal(out["ordinary"], out["extended"]))
        times = {k: [] for k in passes}
        for _ in range(args.windows):
            for k, fn in passes.items():
                times[k].append(window_ms(fn, calls))
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"{size}x{size} x {B} (S = {S}, {2 * S} sweeps, {calls} calls per window), same bits: {same}")
        for k in passes:
            print(f"  {k:9s} {med[k]:10.3f} ms per call (min {min(times[k]):.3f}, max {max(times[k]):.3f})  "
                  f"plan: {plan_text(plans[k])}")
        print(f"  extended / ordinary = {med['extended'] / med['ordinary']:.2f}", flush=True)


if __name__ == "__main__":
    main()
