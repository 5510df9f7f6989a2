"""No VGPR spill in any kernel of csrc/expected_svf_horizon.hip: hipcc's
kernel-resource-usage remarks (tools/kernel_resources.py) for the per-step
kernels (init, value-only step and policy-row step per model, the forward step)
and the two fused kernels, which run 1024 threads per workgroup and so hold at
most 128 VGPRs.  Only names with the file's own prefix appear: the per-state
functions it shares with horizon.hip and soft_horizon.hip (horizon_rows.h) are
inlined.  CPU only (hipcc cross-compiles gfx950)."""

import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "irl-maxent_amd", "csrc", "expected_svf_horizon.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PER_MODEL = ("esh_init_kernel", "esh_value_kernel", "esh_policy_kernel", "esh_fused_kernel")
MODELS = ("<0>", "<1>")       # IRLMX_HORIZON_MODEL_MAXENT, _CAUSAL


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_expected_svf_kernels_do_not_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), SRC],
                         capture_output=True, text=True, check=True, timeout=600,
                         env={**os.environ, "PATH": os.environ.get("PATH", "") + ":/opt/rocm/bin"}).stdout
    rows = [l for l in out.splitlines() if "vspill=" in l]
    ours = [l for l in rows if "irlmx::esh_" in l]
    assert rows == ours, out                                               # only names with the new prefix
    assert not [l for l in out.splitlines() if "irlmx::hz_" in l or "irlmx::soft_hz_" in l], out
    for name in PER_MODEL:
        for inst in MODELS:
            assert sum(f"irlmx::{name}{inst}(" in l for l in ours) == 1, (name, inst, out)
    assert sum("irlmx::esh_fwd_kernel(" in l for l in ours) == 1, out
    assert len(ours) == len(PER_MODEL) * len(MODELS) + 1, out
    for l in ours:
        assert int(re.search(r"vspill=\s*(\d+)", l).group(1)) == 0, l
        if "esh_fused_kernel" in l:
            assert int(re.search(r"vgpr=\s*(\d+)", l).group(1)) <= 128, l    # 1024 threads per workgroup
