"""irlmx_soft_backward_horizon under the call contract of include/irlmx.h (needs
an MI355X): the entry point called directly on the guarded arena of
tests/abi_call.py (through tests/soft_horizon_call.py), on both shapes, with
value0 given and NULL.

The workspace is zeroed, filled with 0xFF or left as a donor call of other
rewards (a NaN among them) left it; every output is poisoned beforehand.  The
results must equal ``ops.soft_backward_horizon``'s bit for bit whatever the
workspace held, both guards must be intact and no output entry may keep its
sentinel -- the NONFINITE instance's included.

What the workspace holds (soft_hz_carve(), soft_horizon.hip):
  fused shape: no workspace at all (0 bytes: a NULL pointer is passed here)
  v[0]    soft_hz_init_kernel writes all of it
  v[1]    the first soft_hz_step_kernel, before the second reads it
"""

import numpy as np
import pytest

import horizon_twin as H
import soft_horizon_call as SC
from test_gpu_call_contract import contract, other_reward

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KEY = "IRLMX_FUSED_MAX_STATES"            # 0: every size per sweep


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    import irlmx
    return irlmx.require_device()


@pytest.mark.parametrize("shape", ["fused", "sweep"])
@pytest.mark.parametrize("name,discount", [("16x16", 1.0), ("37x23", 0.9), ("k8-s1029", 0.9)])
def test_soft_backward_horizon_contract(dev, monkeypatch, name, discount, shape):
    from irlmx import _lib, ops
    monkeypatch.delenv("IRLMX_HORIZON_FUSED_BATCH", raising=False)
    monkeypatch.delenv(KEY, raising=False)
    if shape == "sweep":
        monkeypatch.setenv(KEY, "0")
    else:
        monkeypatch.setenv("IRLMX_HORIZON_FUSED_BATCH", "1")   # several states per thread fused at any batch
    c = H.case(name)
    mdp = c.device_model(dev)
    plan = ops.execution_plan(mdp, "soft_backward_horizon")
    assert plan["shape"] == shape, plan
    need = int(_lib.load().irlmx_workspace_bytes(mdp.struct(), _lib.OP_SOFT_BACKWARD_HORIZON))
    assert need == (0 if shape == "fused" else 2 * (-(-c.B * c.S * 8 // 256) * 256)), need   # each buffer 256-aligned
    tm = ops.terminal_mask(c.terminal, c.S, batch=c.B, device=dev) if c.terminal else None
    reward = np.array(c.reward)
    pi, v0 = ops.soft_backward_horizon(mdp, reward, discount, c.T, tm, return_value0=True)
    donor = {"reward": other_reward(reward)}
    with_v0 = contract(f"{name}/{shape} soft horizon", lambda **kw: SC.soft_backward_horizon(
        mdp, reward, discount, c.T, tm, **kw), donor, {"p_action_t": pi, "value0": v0})
    assert with_v0["status"].tolist() == [_lib.OK] * c.B
    without = contract(f"{name}/{shape} soft horizon, value0 NULL", lambda **kw: SC.soft_backward_horizon(
        mdp, reward, discount, c.T, tm, value0=False, **kw), donor, {"p_action_t": pi})
    assert without["value0"] is None and without["status"].tolist() == [_lib.OK] * c.B
    # a NONFINITE instance: every entry written all the same, and the status computed without value0
    bad = donor["reward"]
    for value0 in (True, False):
        got = contract(f"{name}/{shape} soft horizon, NaN reward", lambda **kw: SC.soft_backward_horizon(
            mdp, bad, discount, c.T, tm, value0=value0, **kw), {"reward": reward}, {})
        assert got["status"].tolist() == [_lib.OK] * (c.B - 1) + [_lib.NONFINITE], got["status"]
