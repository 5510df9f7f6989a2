"""Config 3's backward (128x128, B = 64, the bench's slips, theta = 1) timed per
launch with HIP events, for A/B of library builds (IRLMX_LIB=<path>; run the
libraries alternately, one process each).  With IRLMX_STAMPS=1 the library
prints its per-block phase ticks to stderr.  pi= is a sha256 of the policy: equal
hashes, equal results.
usage: IRLMX_LIB=... python tools/diag/bwd_c3_events.py [tag] [launches [size B]]"""
import hashlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "irl-maxent_amd")]
import torch
from irlmx import DeviceMDP, ops
from irlmx.shard import instance_slips
dev = torch.device("cuda", 0)
tag = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IRLMX_LIB", "default")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
size = int(sys.argv[3]) if len(sys.argv) > 3 else 128
B = int(sys.argv[4]) if len(sys.argv) > 4 else 64
n = size * size
mdp = DeviceMDP.icy_gridworld(size, instance_slips(np.arange(B), B), device=dev)
tm = ops.terminal_mask([n - 1], n, batch=B, device=dev)
r = torch.ones((B, n), dtype=torch.float64, device=dev)
plan = ops.execution_plan(mdp, "backward")
pi = ops.backward_maxent(mdp, r, tm)
torch.cuda.synchronize()
h = hashlib.sha256(pi.cpu().numpy().tobytes()).hexdigest()[:12]
ms = []
for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ops.backward_maxent(mdp, r, tm)
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1))
print(f"[{tag}] {size}x{size} B={B} R={plan['R']} G={plan['G']} C={plan['C']} spt={plan['spt']} backward, HIP events over {reps} launches: "
      f"median {np.median(ms):.3f} ms  min {min(ms):.3f}  max {max(ms):.3f}  pi={h}", flush=True)
