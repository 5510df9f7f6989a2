"""The backward's trapezoid schedule (cluster.hip: unequal band heights, ghost
rows swept only while an owned row still depends on them) gives the policy of
the full sweep bit for bit.

Config 3's plan (R 32, G 8, C 4, 12 states per lane, column pairs) is forced on
a 128x128 IcyGridWorld with few instances: 4 tiles per instance, so top-edge,
interior and bottom-edge tiles all run, for the full 2 S - 1 sweeps (4095 full
blocks and a last block of 7 sweeps, which runs the layout with no row skipped).
Each policy is compared, NaN positions included, with the per-sweep shape
(IRLMX_CLUSTER=0: no tiles, no temporal blocking) and with the same layout
sweeping every row (IRLMX_TRAP_NOSKIP=1).
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZE = 128
S = SIZE * SIZE
PLAN = {"shape": "cluster", "R": 32, "G": 8, "C": 4, "spt": 12, "layout": 2}


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    import irlmx
    return irlmx.require_device()


def rewards(B):
    """name -> [B, S] reward"""
    seeded = np.random.default_rng(128).uniform(-1.0, 0.5, (B, S))
    nan = seeded.copy()
    # tile 1 owns rows 32..63: row 27 is one of its upper ghost rows (and owned by
    # tile 0), row 66 one of its lower ones
    nan[0, 27 * SIZE + 50] = np.nan
    nan[B - 1, 66 * SIZE + 3] = np.nan
    return {"seeded": seeded, "minus5": np.full((B, S), -5.0), "zero": np.zeros((B, S)), "nan": nan}


def three_ways(monkeypatch, dev, mdp, r):
    """the policy from the trapezoid schedule, from the same layout with nothing
    skipped, and from the per-sweep shape"""
    from irlmx import ops
    B = r.shape[0]
    rt = torch.as_tensor(r, device=dev)
    tm = ops.terminal_mask([S - 1], S, batch=B, device=dev)
    monkeypatch.setenv("IRLMX_CLUSTER_R", "32")
    monkeypatch.setenv("IRLMX_CLUSTER_G", "8")
    plan = ops.execution_plan(mdp, "backward")
    assert {k: plan[k] for k in PLAN} == PLAN, plan
    trap = ops.backward_maxent(mdp, rt, tm).cpu().numpy()
    monkeypatch.setenv("IRLMX_TRAP_NOSKIP", "1")
    noskip = ops.backward_maxent(mdp, rt, tm).cpu().numpy()
    monkeypatch.delenv("IRLMX_TRAP_NOSKIP")
    monkeypatch.setenv("IRLMX_CLUSTER", "0")
    assert ops.execution_plan(mdp, "backward")["shape"] != "cluster"
    per_sweep = ops.backward_maxent(mdp, rt, tm).cpu().numpy()
    return trap, noskip, per_sweep


def check(trap, noskip, per_sweep, what):
    assert np.array_equal(trap, noskip, equal_nan=True), (what, "differs from the layout with nothing skipped",
                                                          int(np.sum(~((trap == noskip) | (np.isnan(trap) & np.isnan(noskip))))))
    assert np.array_equal(trap, per_sweep, equal_nan=True), (what, "differs from the per-sweep shape",
                                                             int(np.sum(~((trap == per_sweep) | (np.isnan(trap) & np.isnan(per_sweep))))))


@pytest.mark.parametrize("name", ["seeded", "minus5", "zero", "nan"])
def test_trapezoid_bit_identical(dev, monkeypatch, name):
    """B = 2: rewards uniform in [-1, 0.5]; uniform -5 and 0 (the rescale
    extremes); NaNs in an interior tile's ghost rows."""
    from irlmx import DeviceMDP
    B = 2
    mdp = DeviceMDP.icy_gridworld(SIZE, np.linspace(0.1, 0.3, B), device=dev)
    trap, noskip, per_sweep = three_ways(monkeypatch, dev, mdp, rewards(B)[name])
    if name == "nan":
        assert np.isnan(trap).any()
    else:
        assert np.isfinite(trap).all()
    check(trap, noskip, per_sweep, name)


def test_trapezoid_padded_grid(dev, monkeypatch):
    """B = 3: the instance count is no multiple of 8, so the XCD-grouped grid is padded."""
    from irlmx import DeviceMDP
    B = 3
    mdp = DeviceMDP.icy_gridworld(SIZE, np.linspace(0.1, 0.3, B), device=dev)
    trap, noskip, per_sweep = three_ways(monkeypatch, dev, mdp, rewards(B)["seeded"])
    assert np.isfinite(trap).all()
    check(trap, noskip, per_sweep, "B = 3")


def test_trapezoid_with_stay(dev, monkeypatch):
    """A five-action table (DeviceMDP.with_stay()): self weights are nonzero
    inside the grid, so a row's own slot must never be treated as dead."""
    from irlmx import DeviceMDP
    B = 2
    mdp = DeviceMDP.icy_gridworld(SIZE, np.linspace(0.1, 0.3, B), device=dev).with_stay()
    trap, noskip, per_sweep = three_ways(monkeypatch, dev, mdp, rewards(B)["seeded"])
    assert np.isfinite(trap).all()
    check(trap, noskip, per_sweep, "with_stay")
