"""Per-block phase cycles and polling passes of the cluster kernels
(IRLMX_STAMPS=1: the library prints, per launch, thread 0's cycles per block in
the sweeps, publish, wait and refresh phases and the mean and largest number of
polling passes its per-block ghost gather took -- per tile position too when an
instance has at most 8 tiles).  Config 3's backward under three forced plans,
config 3's forward capped at 3,000 sweeps, and one 128x128 instance's backward
and 20,000-sweep forward.  IRLMX_LIB=<path> loads another build.
usage: python tools/diag/cluster_stamps.py"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "irl-maxent_amd")]
import torch
from irlmx import DeviceMDP, ops
dev = torch.device("cuda", 0)
size, B = 128, 64
n = size * size


def case(B):
    mdp = DeviceMDP.icy_gridworld(size, np.linspace(0.1, 0.3, B) if B > 1 else 0.2, device=dev)
    tm = ops.terminal_mask([n - 1], n, batch=B, device=dev)
    r = torch.ones((B, n), dtype=torch.float64, device=dev)
    p0 = torch.zeros((B, n), dtype=torch.float64, device=dev)
    p0[:, 0] = 1.0
    return mdp, tm, r, p0


def timed(what, fn):
    t = time.perf_counter(); out = fn(); torch.cuda.synchronize(); dt = time.perf_counter() - t
    print(f"{what}: {dt*1e3:.2f} ms", flush=True)
    return out


mdp, tm, r, p0 = case(B)
pi = ops.backward_maxent(mdp, r, tm); torch.cuda.synchronize()
os.environ["IRLMX_STAMPS"] = "1"
for R, G in ((32, 8), (32, 4), (32, 1)):
    os.environ["IRLMX_CLUSTER_R"] = str(R); os.environ["IRLMX_CLUSTER_G"] = str(G)
    timed(f"backward B={B} R={R} G={G}", lambda: ops.backward_maxent(mdp, r, tm))
del os.environ["IRLMX_CLUSTER_R"], os.environ["IRLMX_CLUSTER_G"]
timed(f"forward B={B}, 3000 sweeps", lambda: ops.forward_svf(mdp, p0, tm, pi, max_iter=3000))
mdp, tm, r, p0 = case(1)
pi = timed("backward B=1", lambda: ops.backward_maxent(mdp, r, tm))
timed("forward B=1, 20000 sweeps", lambda: ops.forward_svf(mdp, p0, tm, pi, max_iter=20000))
