"""Cost of the one-call expected SVF (ops.expected_svf_horizon) beside the
two-call path it replaces (ops.backward_maxent_horizon or
ops.soft_backward_horizon, then ops.forward_svf_horizon) on one MI355X.  In one
process and one run, per input and model:

  two calls              the planner's shapes
  one call C=auto        segment 0: C = ceil(sqrt(T))
  one call C=T           every slice kept, nothing recomputed
  .../sweep              the same, forced per step (IRLMX_FUSED_MAX_STATES=0), where the planner's shape is fused

on `64x64` of tests/horizon_twin.py (T = 16), one 128x128 instance at T = 256,
and 16x16 x 3 at T = 40 and T = 4096 (the input whose one-call shape is fused);
with the workspace bytes beside the B * T * S * A * 8 bytes of pi_t.

HIP events around windows of back-to-back calls on the current stream, every
pass warmed up first, the passes alternating window by window; the median over
the windows is printed.  A record, not a threshold: the feature's claim is
memory (profiles/expected_svf_horizon.txt is one run).

usage: python tools/diag/expected_svf_timing.py [--windows N] [--calls N]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "irl-maxent_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"),
                os.path.join(ROOT, "tools", "diag")]
import torch  # noqa: E402
from irlmx import DeviceMDP, ops  # noqa: E402
from timed_timing import KEY, forced, measure  # noqa: E402


def inputs(dev):
    import horizon_twin as H
    c = H.case("64x64")
    yield "64x64 (tests/horizon_twin.py)", c.device_model(dev), np.array(c.reward), np.array(c.p0), c.T
    rng = np.random.default_rng(128)
    for size, B, T in ((128, 1, 256), (16, 3, 40), (16, 3, 4096)):
        S = size * size
        p0 = np.zeros((B, S))
        p0[:, 0] = 1.0
        yield (f"{size}x{size} x {B}", DeviceMDP.icy_gridworld(size, [0.2] * B, device=dev), rng.uniform(-1.0, 0.0, (B, S)),
               p0, T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("expected_svf_timing: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(dev)}; windows per pass: {args.windows}; calls per window: {args.calls}")
    for name, mdp, reward, p0, T in inputs(dev):
        B, S, A = mdp.batch, mdp.n_states, mdp.n_actions
        r, p = torch.as_tensor(reward, device=dev), torch.as_tensor(p0, device=dev)
        print(f"{name}: B = {B}, S = {S}, A = {A}, T = {T}; pi_t of the two-call path {B * T * S * A * 8} bytes")
        for model, discount in (("maxent", 1.0), ("causal", 0.9)):
            def two(model=model, discount=discount):
                pi = (ops.backward_maxent_horizon(mdp, r, T) if model == "maxent"
                      else ops.soft_backward_horizon(mdp, r, discount, T))
                return ops.forward_svf_horizon(mdp, p, pi)[0]

            def one(segment, model=model, discount=discount):
                return ops.expected_svf_horizon(mdp, r, p, T, model=model, discount=discount, segment=segment)[0]

            want = two()
            passes = {"two calls": two}
            plans = {}
            for label, seg in (("C=auto", 0), ("C=T", T)):
                plan = plans[label] = ops.expected_svf_horizon_plan(mdp, T, model, seg)
                assert torch.equal(one(seg).view(torch.int64), want.view(torch.int64)), (name, model, label)
                passes[f"one call {label}"] = lambda seg=seg: one(seg)
                if plan["shape"] == "fused":
                    passes[f"one call {label}/sweep"] = forced(lambda seg=seg: one(seg), KEY, "0")
            del want
            got = measure(passes, args.windows, args.calls, dev)
            for label, plan in plans.items():
                print(f"  {model:6s} plan {label:6s}: {plan['shape']}, C = {plan['segment']}, {plan['slices']} slices, "
                      f"workspace {plan['workspace_bytes']} bytes, LDS {plan['lds_bytes']}")
            for k, (med, lo, hi) in got.items():
                print(f"  {model:6s} {k:22s} {med:10.4f} ms per call (min {lo:.4f}, max {hi:.4f})  "
                      f"x {med / got['two calls'][0]:.2f} of two calls", flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
