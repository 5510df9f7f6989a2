"""The cluster kernel's block end: the per-block ghost gather (cluster.h
gran_gather, which also counts its polling passes for the stamps) and the
backward's rescale behind one wave-uniform branch (cluster.hip).  Neither may
change a value -- the gather only decides when a neighbour's value is seen, and
the rescale left out is a multiplication by 2^0 -- so every case here compares
bit for bit with the per-sweep shape (IRLMX_CLUSTER=0), which exchanges
nothing: policies, and for the forward also state visitation frequencies,
sweep counts and status.

Shapes: the benchmarked trapezoid instantiation with edge and interior tiles
(128x128, R = 32, G = 8), ghosts wider than a tile with lanes holding fewer
than four wanted granules (64x64, R = 8, G = 12) stopped around block edges,
one 128x128 instance (the grid padded to the eight XCD groups), and the column
quads of width 256.  Nothing here times or depends on a hand-off delay.
"""

import numpy as np
import pytest

from conftest import icy_stencil_rect

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KEYS = ("IRLMX_FUSED_MAX_STATES", "IRLMX_CLUSTER", "IRLMX_CLUSTER_R", "IRLMX_CLUSTER_G", "IRLMX_GRID", "IRLMX_PAIR",
        "IRLMX_COMPACT")
SWEEP = {"IRLMX_FUSED_MAX_STATES": "0", "IRLMX_CLUSTER": "0", "IRLMX_GRID": "0"}


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    import irlmx
    return irlmx.require_device()


def use(monkeypatch, env):
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def square(size, B, dev):
    from irlmx import DeviceMDP, ops
    n = size * size
    mdp = DeviceMDP.icy_gridworld(size, np.linspace(0.1, 0.3, B) if B > 1 else 0.2, device=dev)
    tm = ops.terminal_mask([n - 1], n, batch=B, device=dev)
    p0 = np.zeros((B, n))
    p0[np.arange(B), np.arange(B) * 37] = 1.0
    return mdp, tm, p0


def cluster_plan(mdp, op, **want):
    from irlmx import ops
    plan = ops.execution_plan(mdp, op)
    assert plan["shape"] == "cluster", plan
    for k, v in want.items():
        assert plan[k] == v, (k, plan)


def backward_both(monkeypatch, mdp, tm, r, env, **want):
    from irlmx import ops
    use(monkeypatch, SWEEP)
    ref = ops.backward_maxent(mdp, r, tm)
    use(monkeypatch, env)
    cluster_plan(mdp, "backward", **want)
    got = ops.backward_maxent(mdp, r, tm)
    use(monkeypatch, {})
    assert torch.isfinite(ref).all()
    assert torch.equal(ref, got)
    return ref


TRAP = {"IRLMX_CLUSTER_R": "32", "IRLMX_CLUSTER_G": "8"}


def test_trapezoid_backward(dev, monkeypatch):
    """128x128, B = 2, R = 32, G = 8 (C = 4: two edge and two interior tiles per
    instance): seeded non-uniform rewards."""
    mdp, tm, _ = square(128, 2, dev)
    r = np.random.default_rng(11).uniform(0.0, 1.5, (2, 128 * 128))
    backward_both(monkeypatch, mdp, tm, r, TRAP, R=32, G=8, C=4)


@pytest.mark.parametrize("lo,hi", [(2.0, 4.0), (-4.0, -2.0)])
def test_trapezoid_backward_rescales(dev, monkeypatch, lo, hi):
    """The same plan with rewards that make the rescale exponent nonzero: a
    partition vector growing by more than 2^30 per block (rescaled in each of
    the first blocks, then at the period the growth bound allows) and one
    decaying as fast (rescaled in every block)."""
    mdp, tm, _ = square(128, 2, dev)
    r = np.random.default_rng(12).uniform(lo, hi, (2, 128 * 128))
    backward_both(monkeypatch, mdp, tm, r, TRAP, R=32, G=8, C=4)


WIDE = {"IRLMX_FUSED_MAX_STATES": "0", "IRLMX_CLUSTER_R": "8", "IRLMX_CLUSTER_G": "12"}


@pytest.fixture(scope="module")
def wide_case(dev):
    """64x64, B = 2: the instances, and the policy the forward cases share."""
    from irlmx import ops
    mdp, tm, p0 = square(64, 2, dev)
    r = np.random.default_rng(13).uniform(0.0, 1.0, (2, 64 * 64))
    with pytest.MonkeyPatch.context() as mp:
        use(mp, SWEEP)
        pi = ops.backward_maxent(mdp, r, tm)
    return mdp, tm, p0, r, pi


def test_wide_ghosts_backward(wide_case, monkeypatch):
    """64x64, R = 8, G = 12 (C = 8): ghost rows reach past the neighbouring tile."""
    mdp, tm, _, r, pi = wide_case
    use(monkeypatch, WIDE)
    cluster_plan(mdp, "backward", R=8, G=12, C=8)
    from irlmx import ops
    got = ops.backward_maxent(mdp, r, tm)
    use(monkeypatch, {})
    assert torch.equal(pi, got)


@pytest.mark.parametrize("cap", [11, 12, 13, 37])
def test_wide_ghosts_forward(wide_case, monkeypatch, cap):
    """The forward on the same tiles, stopped one sweep before a block's end, on
    it, one sweep past it and inside the fourth block (12 sweeps per block)."""
    from irlmx import ops
    mdp, tm, p0, _, pi = wide_case
    use(monkeypatch, SWEEP)
    ref = ops.forward_svf(mdp, p0, tm, pi, max_iter=cap)
    use(monkeypatch, WIDE)
    cluster_plan(mdp, "forward", R=8, G=12, C=8)
    got = ops.forward_svf(mdp, p0, tm, pi, max_iter=cap)
    use(monkeypatch, {})
    for i, what in enumerate(("svf", "sweeps", "status")):
        assert torch.equal(ref[i], got[i]), (cap, what)
    assert got[1].tolist() == [cap, cap]


def test_single_instance_128(dev, monkeypatch):
    """128x128, B = 1, 16 tiles per instance (the launch padded to the eight XCD
    groups): the backward with 8-row tiles and with the planner's own (32 tiles
    of 4 rows with 14 ghost rows), and the forward, whose own plan has 16 tiles,
    capped at 200 sweeps."""
    from irlmx import ops
    mdp, tm, p0 = square(128, 1, dev)
    r = np.random.default_rng(14).uniform(0.0, 1.5, (1, 128 * 128))
    pi = backward_both(monkeypatch, mdp, tm, r, {"IRLMX_CLUSTER_R": "8", "IRLMX_CLUSTER_G": "8"}, R=8, G=8, C=16)
    use(monkeypatch, {})
    cluster_plan(mdp, "backward")
    assert torch.equal(pi, ops.backward_maxent(mdp, r, tm))
    use(monkeypatch, SWEEP)
    ref = ops.forward_svf(mdp, p0, tm, pi, max_iter=200)
    use(monkeypatch, {})
    cluster_plan(mdp, "forward", C=16)
    got = ops.forward_svf(mdp, p0, tm, pi, max_iter=200)
    for i, what in enumerate(("svf", "sweeps", "status")):
        assert torch.equal(ref[i], got[i]), what


def test_width_256_backward(dev, monkeypatch):
    """256 wide, 32 high, B = 1: column quads (with compact weights where the
    planner takes that layout)."""
    from irlmx import DeviceMDP, _lib, ops
    W, H = 256, 32
    rv = icy_stencil_rect(W, H, 0.2)[None]
    mdp = DeviceMDP(_lib.LAYOUT_STENCIL5, W * H, 4, 1, False, torch.as_tensor(rv, device=dev), width=W, height=H,
                    device=dev)
    tm = ops.terminal_mask([W * H - 1], W * H, device=dev)
    r = np.random.default_rng(15).uniform(0.0, 1.5, (1, W * H))
    backward_both(monkeypatch, mdp, tm, r, {})
