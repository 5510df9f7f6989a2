"""No VGPR spill in any kernel of csrc/timed.hip: hipcc's kernel-resource-usage
remarks (tools/kernel_resources.py) for the three trajectory kernels, the two
per-sweep value kernels and the eight fused (states per thread, slot class)
instantiations -- the list fused_pair_ok(IRLMX_OP_VALUE_HORIZON, ..) admits, the
soft horizon pass's.  CPU only (hipcc cross-compiles gfx950)."""

import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "irl-maxent_amd", "csrc", "timed.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FUSED = ("<1, 5>", "<2, 5>", "<4, 5>", "<1, 8>", "<2, 8>", "<1, 16>", "<2, 16>", "<1, 32>")
PLAIN = ("tp_rollout_kernel", "tp_ll_traj_kernel", "tp_ll_sum_kernel", "tp_value_init_kernel", "tp_value_step_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_timed_kernels_do_not_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), SRC],
                         capture_output=True, text=True, check=True, timeout=600,
                         env={**os.environ, "PATH": os.environ.get("PATH", "") + ":/opt/rocm/bin"}).stdout
    rows = [l for l in out.splitlines() if "irlmx::tp_" in l]
    for inst in FUSED:
        assert sum(f"tp_value_fused_kernel{inst}" in l for l in rows) == 1, (inst, out)
    for name in PLAIN:
        assert sum(f"irlmx::{name}(" in l for l in rows) == 1, (name, out)
    assert len(rows) == len(FUSED) + len(PLAIN), out
    # nothing but tp_ kernels comes out of this file: none of rollout.hip's, horizon.hip's or soft_horizon.hip's names
    assert len([l for l in out.splitlines() if "vspill=" in l]) == len(rows), out
    for l in rows:
        assert int(re.search(r"vspill=\s*(\d+)", l).group(1)) == 0, l
        assert int(re.search(r"vgpr=\s*(\d+)", l).group(1)) <= 128, l    # 1024 threads per workgroup
