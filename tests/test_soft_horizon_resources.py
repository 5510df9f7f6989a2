"""No VGPR spill in any kernel of csrc/soft_horizon.hip: hipcc's
kernel-resource-usage remarks (tools/kernel_resources.py) for both passes of the
file's one skeleton -- SoftPass (irlmx_soft_backward_horizon) and ValuePass
(irlmx_value_horizon) -- each with its two per-sweep kernels and its eight fused
(states per thread, slot class) instantiations, the lists
fused_pair_ok(IRLMX_OP_SOFT_BACKWARD_HORIZON, ..) and
fused_pair_ok(IRLMX_OP_VALUE_HORIZON, ..) admit.  CPU only (hipcc cross-compiles
gfx950)."""

import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "irl-maxent_amd", "csrc", "soft_horizon.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PASSES = ("irlmx::SoftPass", "irlmx::ValuePass")
FUSED = ("1, 5", "2, 5", "4, 5", "1, 8", "2, 8", "1, 16", "2, 16", "1, 32")
SWEEP = ("value_hz_init_kernel", "value_hz_step_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_soft_horizon_kernels_do_not_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), SRC],
                         capture_output=True, text=True, check=True, timeout=600,
                         env={**os.environ, "PATH": os.environ.get("PATH", "") + ":/opt/rocm/bin"}).stdout
    rows = [l for l in out.splitlines() if "irlmx::value_hz_" in l]
    for p in PASSES:
        for inst in FUSED:
            assert sum(f"irlmx::value_hz_fused_kernel<{p}, {inst}>(" in l for l in rows) == 1, (p, inst, out)
        for name in SWEEP:
            assert sum(f"irlmx::{name}<{p}>(" in l for l in rows) == 1, (p, name, out)
    assert len(rows) == len(PASSES) * (len(FUSED) + len(SWEEP)), out
    # nothing else comes out of this file: none of horizon.hip's names, no trajectory kernel
    assert len([l for l in out.splitlines() if "vspill=" in l]) == len(rows), out
    for l in rows:
        assert int(re.search(r"vspill=\s*(\d+)", l).group(1)) == 0, l
        assert int(re.search(r"vgpr=\s*(\d+)", l).group(1)) <= 128, l    # 1024 threads per workgroup
