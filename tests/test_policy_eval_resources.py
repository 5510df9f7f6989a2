"""No VGPR spill in any kernel of csrc/policy_eval.hip: hipcc's
kernel-resource-usage remarks (tools/kernel_resources.py) for the weights,
sweep and finish kernels and all eight fused (states per thread, slot class)
instantiations.  CPU only (hipcc cross-compiles gfx950)."""

import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "irl-maxent_amd", "csrc", "policy_eval.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAIRS = ("<1, 5>", "<2, 5>", "<4, 5>", "<1, 8>", "<2, 8>", "<1, 16>", "<2, 16>", "<1, 32>")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_policy_eval_kernels_do_not_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), SRC],
                         capture_output=True, text=True, check=True, timeout=600,
                         env={**os.environ, "PATH": os.environ.get("PATH", "") + ":/opt/rocm/bin"}).stdout
    rows = [l for l in out.splitlines() if "irlmx::pe_" in l]
    for pair in PAIRS:
        assert any(f"pe_fused_kernel{pair}" in l for l in rows), (pair, out)
    assert len(rows) == len(PAIRS) + 3, out
    for l in rows:
        assert int(re.search(r"vspill=\s*(\d+)", l).group(1)) == 0, l
        assert int(re.search(r"vgpr=\s*(\d+)", l).group(1)) <= 128, l    # 1024 threads per workgroup
