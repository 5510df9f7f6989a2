"""Cost of the finite-horizon passes (ops.backward_maxent_horizon,
ops.forward_svf_horizon) on one MI355X, per step, beside the per-sweep cost of
the existing passes they resemble, in one process:

  16x16 x 64, 64x64 x 1     T = 128, on the planner's shape and, the routing check, forced fused
                            (IRLMX_HORIZON_FUSED_BATCH=1) and forced per sweep (IRLMX_FUSED_MAX_STATES=0);
                            --points adds sizes and batches (profiles/horizon.txt: 32x32, 45x45, 64x64 x 1..256)
  128x128 x 1, 128x128 x 64 per sweep (T = 256)

  ops.backward_maxent_extended   time / 2S sweeps: a horizon backward step does
                                 A times a collapsed sweep's multiply-adds, a
                                 division and an S * A store
  ops.forward_svf(max_iter=T+1)  time / (T + 1) sweeps: a horizon forward step
                                 also folds its weights from pi_t

HIP events around windows of back-to-back calls on the current stream, every
shape warmed up first, the passes alternating window by window; the median over
the windows is printed with each plan.  A record, not a threshold.

usage: python tools/diag/horizon_cost.py [--windows N] [--points size:instances:T:calls,...]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "irl-maxent_amd")]
import torch  # noqa: E402
from irlmx import DeviceMDP, ops  # noqa: E402

POINTS = ((16, 64, 128, 4), (64, 1, 128, 4), (128, 1, 256, 1), (128, 64, 256, 1))   # size, instances, T, calls per window
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--points", default=None, help="size:instances:T:calls,... instead of the four points above")
    args = ap.parse_args()
    points = POINTS if args.points is None else [tuple(int(v) for v in p.split(":")) for p in args.points.split(",")]
    if not torch.cuda.is_available():
        sys.exit("horizon_cost: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(dev)}; windows per pass: {args.windows}")
    for size, B, T, calls in points:
        S = size * size
        mdp = DeviceMDP.icy_gridworld(size, [0.2] * B, device=dev)
        r = torch.as_tensor(np.random.default_rng(size).uniform(-1.0, 0.0, (B, S)), device=dev)
        p0 = torch.full((B, S), 1.0 / S, dtype=torch.float64, device=dev)
        none = torch.zeros((B, S), dtype=torch.uint8, device=dev)
        term = ops.terminal_mask([S - 1], S, batch=B, device=dev)
        pi_t = ops.backward_maxent_horizon(mdp, r, T)
        pi0 = pi_t[:, 0].contiguous()
        passes = {"backward_horizon": (lambda: ops.backward_maxent_horizon(mdp, r, T), T),
                  "forward_horizon": (lambda: ops.forward_svf_horizon(mdp, p0, pi_t), T),
                  "backward_extended": (lambda: ops.backward_maxent_extended(mdp, r, term), 2 * S),
                  "forward_svf": (lambda: ops.forward_svf(mdp, p0, none, pi0, max_iter=T + 1), T + 1)}
        plans = {"backward_horizon": ops.execution_plan(mdp, "backward_horizon"),
                 "forward_horizon": ops.execution_plan(mdp, "forward_horizon"),
                 "backward_extended": ops.execution_plan(mdp, "backward", extended_range=True),
                 "forward_svf": ops.execution_plan(mdp, "forward")}
        small = S <= 4096              # both shapes exist: the same inputs forced fused and forced per sweep
        if small:
            def forced(fn, key, value):
                def run():
                    os.environ[key] = value
                    try:
                        return fn()
                    finally:
                        del os.environ[key]
                return run
            for k in ("backward_horizon", "forward_horizon"):
                passes[k + "/fused"] = (forced(passes[k][0], BATCH_KEY, "1"), T)
                passes[k + "/sweep"] = (forced(passes[k][0], KEY, "0"), T)
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
            print(f"  {k:23s} {med[k]:10.3f} ms per call (min {min(times[k]):.3f}, max {max(times[k]):.3f})  "
                  f"{us[k]:8.2f} us per step of {passes[k][1]}  plan: {plan}")
        print(f"  backward_horizon step / backward_extended sweep = {us['backward_horizon'] / us['backward_extended']:.2f}; "
              f"forward_horizon step / forward_svf sweep = {us['forward_horizon'] / us['forward_svf']:.2f}")
        if small:
            print(f"  fused / per sweep: backward {med['backward_horizon/fused'] / med['backward_horizon/sweep']:.2f}, "
                  f"forward {med['forward_horizon/fused'] / med['forward_horizon/sweep']:.2f}", flush=True)
        del pi_t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
