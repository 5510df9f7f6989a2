"""No VGPR spill in any kernel of csrc/rollout.hip: hipcc's kernel-resource-usage
remarks (tools/kernel_resources.py) for the rollout and the log-likelihood
kernel, each in its stationary and its time-indexed instantiation, the one sum
kernel both log-likelihood calls launch, and the statistics kernel.  CPU only
(hipcc cross-compiles gfx950)."""

import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "irl-maxent_amd", "csrc", "rollout.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TIMED = ("rollout_kernel", "demo_ll_traj_kernel")      # templates on bool TIMED
PLAIN = ("demo_ll_sum_kernel", "demo_statistics_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_trajectory_kernels_do_not_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), SRC],
                         capture_output=True, text=True, check=True, timeout=600,
                         env={**os.environ, "PATH": os.environ.get("PATH", "") + ":/opt/rocm/bin"}).stdout
    rows = [l for l in out.splitlines() if "vspill=" in l]
    for name in TIMED:
        for inst in ("<false>", "<true>"):
            assert sum(f"irlmx::{name}{inst}(" in l for l in rows) == 1, (name, inst, out)
    for name in PLAIN:
        assert sum(f"irlmx::{name}(" in l for l in rows) == 1, (name, out)
    # nothing else comes out of this file: no second sum kernel, none of the value pass's names
    assert len(rows) == 2 * len(TIMED) + len(PLAIN), out
    for l in rows:
        assert int(re.search(r"vspill=\s*(\d+)", l).group(1)) == 0, l
        assert int(re.search(r"vgpr=\s*(\d+)", l).group(1)) <= 128, l
