"""The call contract and the stream order of include/irlmx.h for the entry points
of include/irlmx_timed.h (needs an MI355X): tests/test_gpu_call_contract.py and
tests/test_gpu_stream_order.py for the three calls on time-indexed policies.
The wrappers, the claims and the rows are tests/timed_call.py's; the helpers
are those two suites' own, imported as they are.

* irlmx_value_horizon through ``abi_call.contract_call``: a guarded arena of
  exactly irlmx_workspace_bytes, filled with zeros, 0xFF bytes or what a donor
  call with other rewards and a NaN left there; every output poisoned,
  value_t included; on 16x16 (B = 3), fused and per sweep, under a policy and
  without one.
* all three entry points through ``abi_call.stream_call`` on a non-blocking
  side stream behind a device delay with inputs that land late, claim
  "asynchronous": the rows of test_gpu_stream_order, for this header.
"""

import numpy as np
import pytest

import abi_call as A
import horizon_twin as H
import test_gpu_call_contract as CC
import test_gpu_stream_order as SO
import timed_call as TC
from test_gpu_stream_order import cycles_per_ms, dev, streams  # noqa: F401  (module-scoped fixtures, instantiated here)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KEYS = ("IRLMX_FUSED_MAX_STATES", "IRLMX_HORIZON_FUSED_BATCH")


@pytest.fixture
def env(monkeypatch):
    def set_env(values):
        for k in KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in values.items():
            assert k in KEYS, k
            monkeypatch.setenv(k, str(v))
    set_env({})
    yield set_env
    set_env({})


@pytest.mark.parametrize("shape", ["fused", "sweep"])
@pytest.mark.parametrize("kind", ["policy", "optimal"])
def test_value_horizon_contract(dev, env, shape, kind):  # noqa: F811
    """``ops.value_horizon``'s bits whatever the workspace held -- the donor's
    rewards hold a NaN -- and no output entry keeps its sentinel, value_t and
    the NONFINITE instance's included; with value_t NULL the same value0."""
    from irlmx import _lib, ops
    env({"IRLMX_FUSED_MAX_STATES": 0} if shape == "sweep" else {})
    c = H.case("16x16")
    mdp = c.device_model(dev)
    assert ops.execution_plan(mdp, "value_horizon")["shape"] == shape
    need = int(_lib.load().irlmx_workspace_bytes(mdp.struct(), _lib.OP_VALUE_HORIZON))
    assert need == (0 if shape == "fused" else 2 * (-(-c.B * c.S * 8 // 256) * 256)), need
    reward = np.array(c.reward)
    pi = ops.backward_maxent_horizon(mdp, reward, c.T) if kind == "policy" else None
    v0, status, vt = ops.value_horizon(mdp, reward, c.T, pi, 0.9, return_values=True)
    donor = {"reward": CC.other_reward(reward)}
    full = CC.contract(f"16x16/{shape} value horizon {kind}", lambda **kw: TC.value_horizon(mdp, reward, c.T, pi, 0.9, **kw),
                       donor, {"value0": v0, "value_t": vt, "status": status})
    assert full["status"].tolist() == [_lib.OK] * c.B
    without = CC.contract(f"16x16/{shape} value horizon {kind}, value_t NULL",
                          lambda **kw: TC.value_horizon(mdp, reward, c.T, pi, 0.9, value_t=False, **kw), donor, {"value0": v0})
    assert without["value_t"] is None
    bad = donor["reward"]                                      # a NONFINITE instance: every entry written all the same
    for value_t in (True, False):
        got = CC.contract(f"16x16/{shape} value horizon {kind}, NaN reward",
                          lambda **kw: TC.value_horizon(mdp, bad, c.T, pi, 0.9, value_t=value_t, **kw), {"reward": reward}, {})
        assert got["status"].tolist() == [_lib.OK] * (c.B - 1) + [_lib.NONFINITE], got["status"]


@pytest.mark.parametrize("rid", [r.id for r in TC.ROWS])
def test_stream_order(dev, env, streams, cycles_per_ms, rid):  # noqa: F811
    """(r) on the default stream, (s) on a side stream, (d) behind a delay with late
    inputs: the same bits, and in (d) the call returns while the delay still runs."""
    r = TC.ROW[rid]
    env(r.keys)
    run = r.build(dev)
    claim = TC.CLAIMS[(r.entry, r.shape)]
    assert claim == SO.ASYNC
    ref = SO.three_runs(f"{r.id} {r.entry}", run, claim, streams, cycles_per_ms)
    for name, t in ref.items():                                  # (r) is what ops returns: judged in test_gpu_timed
        assert t is not None and t.numel() > 0, name
