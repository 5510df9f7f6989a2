"""The block hand-off compiled for config 3's plan (cluster.hip, trap_publish /
trap_gather: R 32, G 8, C 4, 12 states per lane, column pairs) gives the policy
of every other way to run the same backward, bit for bit.

The plan is forced on a 128x128 IcyGridWorld, the smallest shape it exists at,
for the full 2 S - 1 sweeps: 4,095 full blocks and a last block of 7 sweeps.
Each policy is compared, NaN positions included, with three references:

* the per-sweep shape (IRLMX_CLUSTER=0: no tiles, no hand-off at all);
* the same call with IRLMX_EAGER_SUMMARY=1: every block stores and polls the
  tiles' summary granules, which the compiled hand-off otherwise stores only
  in the rescale blocks;
* the same call with IRLMX_XCD_GROUP=0: the tiles of an instance are spread
  over the XCDs, so the publication takes its write-through store group.

A forced exchange timeout at this plan must rerun the call per sweep with the
same result.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZE = 128
S = SIZE * SIZE
PLAN = {"shape": "cluster", "R": 32, "G": 8, "C": 4, "spt": 12, "layout": 2}
KNOBS = ("IRLMX_CLUSTER", "IRLMX_CLUSTER_R", "IRLMX_CLUSTER_G", "IRLMX_EAGER_SUMMARY", "IRLMX_XCD_GROUP",
         "IRLMX_TRAP_NOSKIP", "IRLMX_TEST_DROP_TILE", "IRLMX_TEST_EXCHANGE_TIMEOUT_MS", "IRLMX_STRICT_EXCHANGE",
         "IRLMX_PLAN_CUS")


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    import irlmx
    return irlmx.require_device()


def reward(name, B):
    """[B, S] reward"""
    seeded = np.random.default_rng(128).uniform(-1.0, 0.5, (B, S))
    if name == "seeded":
        return seeded
    if name == "minus5":   # the vector decays: a rescale every block
        return np.full((B, S), -5.0)
    if name == "zero":     # the vector grows: a rescale every 32nd block
        return np.zeros((B, S))
    assert name == "nan"
    # tile 1 owns rows 32..63: row 27 is one of its upper ghost rows (owned by
    # tile 0), row 66 one of its lower ones (owned by tile 2)
    seeded[0, 27 * SIZE + 50] = np.nan
    seeded[B - 1, 66 * SIZE + 3] = np.nan
    return seeded


_cases = {}


def case(dev, name, B):
    """(mdp, reward tensor, terminal mask, per-sweep policy) of one case; the
    per-sweep reference is computed once and shared"""
    import os
    from irlmx import DeviceMDP, ops
    if (name, B) not in _cases:
        mdp = DeviceMDP.icy_gridworld(SIZE, np.linspace(0.1, 0.3, B), device=dev)
        rt = torch.as_tensor(reward(name, B), device=dev)
        tm = ops.terminal_mask([S - 1], S, batch=B, device=dev)
        saved = {k: os.environ.pop(k, None) for k in KNOBS}
        os.environ["IRLMX_CLUSTER"] = "0"
        try:
            assert ops.execution_plan(mdp, "backward")["shape"] != "cluster"
            per_sweep = ops.backward_maxent(mdp, rt, tm).cpu().numpy()
        finally:
            del os.environ["IRLMX_CLUSTER"]
            os.environ.update({k: v for k, v in saved.items() if v is not None})
        per_sweep.setflags(write=False)
        _cases[(name, B)] = (mdp, rt, tm, per_sweep)
    return _cases[(name, B)]


def force_plan(monkeypatch, mdp):
    from irlmx import ops
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("IRLMX_CLUSTER_R", "32")
    monkeypatch.setenv("IRLMX_CLUSTER_G", "8")
    plan = ops.execution_plan(mdp, "backward")
    assert {k: plan[k] for k in PLAN} == PLAN, plan


def same(got, ref, what):
    differ = int(np.sum(~((got == ref) | (np.isnan(got) & np.isnan(ref)))))
    assert np.array_equal(got, ref, equal_nan=True), (what, differ)


def check_three_references(dev, monkeypatch, name, B):
    from irlmx import ops
    mdp, rt, tm, per_sweep = case(dev, name, B)
    force_plan(monkeypatch, mdp)
    c0 = ops.counters()
    got = ops.backward_maxent(mdp, rt, tm).cpu().numpy()
    monkeypatch.setenv("IRLMX_EAGER_SUMMARY", "1")
    eager = ops.backward_maxent(mdp, rt, tm).cpu().numpy()
    monkeypatch.delenv("IRLMX_EAGER_SUMMARY")
    monkeypatch.setenv("IRLMX_XCD_GROUP", "0")
    spread = ops.backward_maxent(mdp, rt, tm).cpu().numpy()
    monkeypatch.delenv("IRLMX_XCD_GROUP")
    c1 = ops.counters()
    # three persistent launches, none handed back to the per-sweep shape
    assert c1["cluster_launches"] - c0["cluster_launches"] == 3
    assert c1["sweep_calls"] == c0["sweep_calls"] and c1["rerun_timeout"] == c0["rerun_timeout"]
    assert c1["rerun_not_resident"] == c0["rerun_not_resident"]
    if name == "nan":
        assert np.isnan(got).any()
    else:
        assert np.isfinite(got).all()
    same(got, per_sweep, (name, B, "differs from the per-sweep shape"))
    same(got, eager, (name, B, "differs from the call with every block's summaries exchanged"))
    same(got, spread, (name, B, "differs from the call with write-through publication"))


@pytest.mark.parametrize("name", ["seeded", "minus5", "zero", "nan"])
def test_handoff_edge_and_interior_tiles(dev, monkeypatch, name):
    """B = 2: rewards uniform in [-1, 0.5]; uniform -5 and 0 (a rescale every
    block, and every 32nd); a NaN in an interior tile's ghost rows."""
    check_three_references(dev, monkeypatch, name, 2)


def test_handoff_padded_grid(dev, monkeypatch):
    """B = 3: no multiple of 8, so the XCD-grouped grid is padded."""
    check_three_references(dev, monkeypatch, "seeded", 3)


def test_handoff_two_instances_per_xcd_group(dev, monkeypatch):
    """B = 9: instances 0 and 8 take their tiles from the same XCD group."""
    check_three_references(dev, monkeypatch, "seeded", 9)


def test_handoff_exchange_timeout_reruns(dev, monkeypatch):
    """An interior tile's workgroup leaves after the rendezvous: its neighbours'
    polls time out, the call is rerun per sweep and gives the same policy."""
    from irlmx import ops
    mdp, rt, tm, per_sweep = case(dev, "seeded", 2)
    force_plan(monkeypatch, mdp)
    ref = ops.backward_maxent(mdp, rt, tm)
    base = ops.counters()
    monkeypatch.setenv("IRLMX_TEST_DROP_TILE", "1")
    monkeypatch.setenv("IRLMX_TEST_EXCHANGE_TIMEOUT_MS", "50")
    got = ops.backward_maxent(mdp, rt, tm)
    after = ops.counters()
    assert after["rerun_timeout"] == base["rerun_timeout"] + 1
    assert after["sweep_calls"] == base["sweep_calls"] + 1
    assert torch.equal(got, ref)
    same(got.cpu().numpy(), per_sweep, "rerun differs from the per-sweep shape")
    torch.cuda.synchronize()
