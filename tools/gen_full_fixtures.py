#!/usr/bin/env python
"""Converged full-size fixtures for the GPU parity tests (tests/golden/full_*.npz).

The reference cannot reach these sizes (its unscaled backward is NaN beyond
12x12 and its dense sweeps take hours at 128x128), so the expected values come
from the CPU oracle's sparse-operand restatement (oracle/maxent_oracle.py
``*_csr``), which tests/test_oracle_golden.py pins to the dense restatement and
that one to the reference's own outputs.  Everything here runs in the build
container only; the GPU box reads the .npz files.

Workloads are exactly the bench's (bench.py CONFIGS, irlmx.shard.instance_slips,
irlmx.demos.sample with seed 1234 + b):

  full_c3.npz  128x128, B = 64: instances b = 0 and 63, the first 3 gradient
               steps of irl (maxent.py:240-252) from theta = 1 -- step 1's
               forward runs ~360k sweeps to convergence.
  full_c4.npz  256x256, 32 instances per GPU: b = 0 and 31, the first 7 steps
               (the bench's timed window at --steps 5 --warmup 2).
               Vectors of 65,536 states are stored on a fixed subset of 4,096
               states plus whole-vector sums (sum, sum |x|, max |x|); the SVF
               and theta of steps 1 and 7 also whole (svf0_full, theta6_full, ...).
  full_c5.npz  128x128 causal (config 5): the forward pass to convergence on the
               reference's own soft-VI policy (tests/golden/causal_128.npz), and
               the first 7 irl_causal steps (maxent.py:437-450) of the bench's
               c5 workload (one instance, discount 0.7).

  full_c2.npz  64x64, one instance (BASELINE config 2 as bench.py --config c2 runs
               it: p_slip 0.1, demonstrations seed 1234): the first 13 steps
               (the recorded c2 bench window, --warmup 3 --steps 10), full
               policy of step 1, SVF and theta of every step.
  run_c2.npz   the same instance run to the reference's stopping rule (as
               run_c3.npz below; a few minutes).

  run_c3.npz   128x128, B = 64: instances b = 0 and 63 run to the reference's own
               stopping rule (maxent.py:236-255, eps = 1e-4) -- step count,
               per-step forward sweeps and theta summaries, theta after steps
               6, 15 and 25 (the bench's timed window at W = 5, K = 20) and
               the final reward (theta, F = I).  ~2.5 h per instance.

  dense2048.npz  a seeded random dense MDP (S = 2048, A = 4, every entry
               nonzero; oracle random_dense_mdp() regenerates it bit for bit on any
               host), run through the dense oracle (the reference's own numpy
               statements, maxent.py:98-159, 279-341; solver.py:9-104):
               backward, forward, soft VI + causal forward, VI and its
               action-average form, with sweep counts.

Usage: python tools/gen_full_fixtures.py [c2 c2run c3 c4 c5 dense c3run]
       (~25 min on 8 cores without c3run)
"""

import os
import sys
import time
from multiprocessing import Pool

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = "1"

import numpy as np  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "irl-maxent_amd"))
OUT = os.path.join(ROOT, "tests", "golden")

import golden_parts          # noqa: E402  (tools/golden_parts.py: fixtures above 1 MiB are written in parts)
import maxent_oracle as O  # noqa: E402
from irlmx import demos    # noqa: E402  (the bench's own input generator: numpy only)

SUBSET_MAX_S = 16384   # larger vectors are stored on a subset of states


def subset(n_states, size, k=4096, seed=99):
    rng = np.random.default_rng(seed)
    pick = set(rng.choice(n_states, k - 8, replace=False).tolist())
    pick |= {0, size - 1, n_states - size, n_states - 1, size, 2 * size - 1, n_states // 2, n_states // 2 + 1}
    return np.array(sorted(pick))[:k]


def pack(prefix, vec, idx, out):
    vec = np.asarray(vec)
    out[prefix + "_sum"] = np.array([vec.sum(), np.abs(vec).sum(), np.abs(vec).max()])
    out[prefix] = vec if idx is None else vec[idx]


def bench_instance(size, b, n_total):
    slip = 0.1 + 0.2 * float(b) / n_total       # irlmx.shard.instance_slips
    mats = O.icy_gridworld_csr(size, slip)
    rv = O.stencil_row_val(mats, size)
    n = size * size
    e_f, p0, _ = demos.sample(rv, size, [n - 1], 0, n=200, seed=1234 + b, max_len=demos.safety_cap(size))
    return slip, mats, e_f, p0


FULL_STEPS = {"c4": (0, 6)}   # steps (0-based) whose whole vectors are kept although S > SUBSET_MAX_S


def job_irl(args):
    cfg, size, n_total, b, n_steps, causal = args
    t0 = time.time()
    n = size * size
    slip, mats, e_f, p0 = bench_instance(size, b, n_total)
    res = O.irl_steps_csr(mats, e_f, p0, [n - 1], n_steps, causal=causal, discount=0.7 if causal else None)
    idx = None if n <= SUBSET_MAX_S else subset(n, size)
    out = {"slip": np.array(slip), "e_f": e_f, "p0": p0,
           "k_f": np.array(res["k_f"]), "k_b": np.array(res["k_b"])}
    if idx is not None:
        out["idx"] = idx
    for i in range(n_steps):
        pack(f"svf{i}", res["svf"][i], idx, out)
        pack(f"theta{i}", res["theta"][i], idx, out)
        if idx is not None and i in FULL_STEPS.get(cfg, ()):
            out[f"svf{i}_full"] = res["svf"][i]
            out[f"theta{i}_full"] = res["theta"][i]
    pi0 = res["pi"][0]
    if idx is None:
        out["pi0"] = pi0
    else:
        out["pi0"] = pi0[idx]
        out["pi0_sum"] = np.array([pi0.sum(), np.abs(pi0).max()])
    print(f"[{cfg} b={b}] k_f={res['k_f']} k_b={res['k_b']} {time.time() - t0:.0f}s", flush=True)
    return cfg, b, out


RUN_KEEP = (1, 2, 3, 6, 13, 15, 25)


def job_run(args):
    """Whole irl run of one bench instance (run_c3.npz)."""
    cfg, size, n_total, b = args
    t0 = time.time()
    n = size * size
    slip, mats, e_f, p0 = bench_instance(size, b, n_total)

    def progress(k, theta, k_f, delta):
        if k <= 3 or k % 25 == 0:
            print(f"[run {cfg} b={b}] step {k} k_f={k_f} delta={delta:.3e} {time.time() - t0:.0f}s", flush=True)

    res = O.irl_run_csr(mats, e_f, p0, [n - 1], keep_steps=RUN_KEEP, on_step=progress)
    out = {"slip": np.array(slip), "steps": np.array(res["steps"]), "k_f": np.array(res["k_f"]),
           "delta": np.array(res["delta"]), "theta_sum": np.array(res["theta_sum"]), "theta": res["theta"]}
    for k, th in res["theta_at"].items():
        out[f"theta_at{k}"] = th
    print(f"[run {cfg} b={b}] steps={res['steps']} {time.time() - t0:.0f}s", flush=True)
    return "run_" + cfg, b, out


def job_dense(_):
    t0 = time.time()
    os.environ["OPENBLAS_NUM_THREADS"] = "4"
    P, r, term, p0 = O.random_dense_mdp()
    out = {"P_check": np.array([P.sum(), P[::7, ::5, :].sum(), P[-1, -1, -1]]), "reward": r}
    pi = O.backward_maxent(P, term, r, rescale=True)
    svf, k_f = O.forward_svf(P, p0, term, pi)
    cpi, cv, k_s = O.soft_backward(P, term, r, 0.7)
    csvf, k_cf = O.forward_svf(P, p0, term, cpi)
    v, k_v = O.value_iteration(P, r, 0.9)
    va, k_va = O.value_iteration(P, r, 0.9, average=True)
    out.update(pi=pi, svf=svf, k_f=np.array(k_f), cpi=cpi, cv=cv, k_s=np.array(k_s), csvf=csvf, k_cf=np.array(k_cf),
               v=v, k_v=np.array(k_v), va=va, k_va=np.array(k_va))
    print(f"[dense] k_f={k_f} k_s={k_s} k_cf={k_cf} k_v={k_v} k_va={k_va} {time.time() - t0:.0f}s", flush=True)
    return "dense2048", "dense", out


def job_c5_forward(_):
    t0 = time.time()
    z = np.load(os.path.join(OUT, "causal_128.npz"))
    size = int(z["size"])
    n = size * size
    p0 = np.zeros(n)
    p0[0] = 1.0
    svf, k = O.forward_svf_csr(O.icy_gridworld_csr(size, 0.2), p0, [n - 1], z["pi"])
    print(f"[c5 forward] k_f={k} {time.time() - t0:.0f}s", flush=True)
    return "c5", "fwd", {"svf": svf, "k_f": np.array(k)}


def main():
    which = sys.argv[1:] or ["c3", "c4", "c5", "dense"]
    jobs = []
    if "dense" in which:
        jobs.append((job_dense, None))
    if "c3" in which:
        jobs += [(job_irl, ("c3", 128, 64, b, 3, False)) for b in (0, 63)]
    if "c4" in which:   # 7 steps: the bench's --config c4 timed window (W = 2, K = 5) is steps 3-7
        jobs += [(job_irl, ("c4", 256, 32, b, 7, False)) for b in (0, 31)]
    if "c2" in which:   # 13 steps: the recorded c2 bench window (W = 3, K = 10)
        jobs.append((job_irl, ("c2", 64, 1, 0, 13, False)))
    if "c2run" in which:
        jobs.append((job_run, ("c2", 64, 1, 0)))
    if "c3run" in which:
        jobs += [(job_run, ("c3", 128, 64, b)) for b in (0, 63)]
    if "c5" in which:   # 7 steps, as config 4
        jobs += [(job_c5_forward, None), (job_irl, ("c5", 128, 1, 0, 7, True))]
    with Pool(len(jobs)) as pool:
        res = [pool.apply_async(f, (a,)) for f, a in jobs]
        res = [r.get() for r in res]
    files = {}
    for cfg, key, out in res:
        if key == "dense":
            for path in golden_parts.save(os.path.join(OUT, cfg), out):
                print("wrote", path, os.path.getsize(path), "bytes")
            continue
        d = files.setdefault(cfg, {})
        for k, v in out.items():
            d[f"{key}__{k}" if key != "fwd" else f"fwd__{k}"] = v
    for cfg, d in files.items():
        if cfg.startswith("run_"):
            d["instances"] = np.array(sorted({int(k.split("__")[0]) for k in d}))
            for path in golden_parts.save(os.path.join(OUT, cfg), d):
                print("wrote", path, os.path.getsize(path), "bytes")
            continue
        d["instances"] = np.array(sorted({int(k.split("__")[0]) for k in d if k.split("__")[0].isdigit()}))
        for path in golden_parts.save(os.path.join(OUT, f"full_{cfg}"), d):
            print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
