"""No VGPR spill in any kernel of csrc/horizon.hip: hipcc's
kernel-resource-usage remarks (tools/kernel_resources.py) for the four
per-sweep kernels, the three fused forward instantiations and the nine fused
backward ones -- the eight (states per thread, slot class) pairs reading their
table from memory and <1, 5> holding it in registers.  CPU only (hipcc
cross-compiles gfx950)."""

import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "irl-maxent_amd", "csrc", "horizon.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
BACKWARD = ("<1, 5, true>", "<1, 5, false>", "<2, 5, false>", "<4, 5, false>", "<1, 8, false>", "<2, 8, false>",
            "<1, 16, false>", "<2, 16, false>", "<1, 32, false>")
FORWARD = ("<1>", "<2>", "<4>")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_horizon_kernels_do_not_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), SRC],
                         capture_output=True, text=True, check=True, timeout=600,
                         env={**os.environ, "PATH": os.environ.get("PATH", "") + ":/opt/rocm/bin"}).stdout
    rows = [l for l in out.splitlines() if "irlmx::hz_" in l]
    for inst in BACKWARD:
        assert any(f"hz_bwd_fused_kernel{inst}" in l for l in rows), (inst, out)
    for inst in FORWARD:
        assert any(f"hz_fwd_fused_kernel{inst}" in l for l in rows), (inst, out)
    assert len(rows) == len(BACKWARD) + len(FORWARD) + 4, out
    for l in rows:
        assert int(re.search(r"vspill=\s*(\d+)", l).group(1)) == 0, l
        assert int(re.search(r"vgpr=\s*(\d+)", l).group(1)) <= 128, l    # 1024 threads per workgroup
