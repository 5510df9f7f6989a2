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

--grid: the extended pass's persistent grid shape (csrc/extended_grid.hip)
against its per-sweep shape (IRLMX_GRID=0) and the ordinary backward, at

  128x128 x 1, 8, 16, 64      256x256 x 1, 2, 4, 8, 32

one call per window, the routes alternating, --windows windows each (default
3: the spread is printed).  The grid route is timed as planned by default
(where the default route is the grid shape) and with the launch cap lifted
(IRLMX_EXT_GRID_MAX_LAUNCHES), so that every batch size shows what its
sequential launches cost; the default of the cap is set from these lines.

usage: python tools/diag/extended_backward_cost.py [--windows N] [--grid]"""
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


GRID_POINTS = ((128, 1), (128, 8), (128, 16), (128, 64), (256, 1), (256, 2), (256, 4), (256, 8), (256, 32))
ROUTES = {"grid": {}, "grid, cap lifted": {"IRLMX_EXT_GRID_MAX_LAUNCHES": "1000000"}, "per sweep": {"IRLMX_GRID": "0"}}


def with_keys(keys, fn):
    """fn() with these planner keys set (the library reads them at every call)."""
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update(keys)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def grid_points(dev, windows):
    for size, B in GRID_POINTS:
        S = size * size
        mdp = DeviceMDP.icy_gridworld(size, [0.2] * B, device=dev)
        r = torch.as_tensor(np.random.default_rng(size).uniform(-1.0, 0.0, (B, S)), device=dev)
        tm = ops.terminal_mask([S - 1], S, batch=B, device=dev)
        passes = {"ordinary": lambda: ops.backward_maxent(mdp, r, tm)}
        plans = {}
        for name, keys in ROUTES.items():
            plan = with_keys(keys, lambda: ops.execution_plan(mdp, "backward", extended_range=True))
            if name != "per sweep" and (plan["shape"] != "grid" or plan in plans.values()):
                continue                                     # not planned on the grid shape, or the same plan again
            plans[name] = plan
            passes[name] = lambda keys=keys: with_keys(keys, lambda: ops.backward_maxent_extended(mdp, r, tm))
        before = ops.counters()
        out = {k: fn() for k, fn in passes.items()}          # warm-up, and the check
        torch.cuda.synchronize(dev)
        after = ops.counters()
        same = all(bool(torch.equal(out["ordinary"], v)) for v in out.values())
        reruns = sum(after[k] - before[k] for k in ("rerun_not_resident", "rerun_timeout"))
        times = {k: [] for k in passes}
        for _ in range(windows):
            for k, fn in passes.items():
                times[k].append(window_ms(fn, 1))
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"{size}x{size} x {B} (S = {S}, {2 * S} sweeps), same bits: {same}, reruns in the warm-up: {reruns}")
        if "grid" not in plans:
            print("  default route: per sweep")
        for k in passes:
            g = plans.get(k)
            plan = "" if g is None or g["shape"] != "grid" else (
                f"  plan: spt {g['spt']}, {g['C']} workgroups per instance, {g['per_launch']} instances per launch, "
                f"xcd {g['G']}, {g['launches']} launches")
            ratio = "" if g is None or g["shape"] != "grid" else f"  per sweep / this = {med['per sweep'] / med[k]:.2f}"
            print(f"  {k:16s} {med[k]:10.3f} ms per call (min {min(times[k]):.3f}, max {max(times[k]):.3f}){ratio}{plan}",
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=None)
    ap.add_argument("--grid", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("extended_backward_cost: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    args.windows = args.windows or (3 if args.grid else 5)
    print(f"device: {torch.cuda.get_device_name(dev)}; windows per pass: {args.windows}")
    if args.grid:
        return grid_points(dev, args.windows)
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
