"""The persistent grid shape of the extended-range backward on the device
(csrc/extended_grid.hip; needs an MI355X).

The shape applies from 8,192 states on; IRLMX_EXT_GRID_MIN_STATES=0 with
IRLMX_FUSED_MAX_STATES=0 brings it down to the small sizes used here.  Its
per-state arithmetic is the per-sweep shape's statement for statement, so every
result is compared bit for bit with the per-sweep extended pass (IRLMX_GRID=0).

Every test runs with IRLMX_STRICT_EXCHANGE=1 and a 2 s exchange timeout: a
healthy exchange takes microseconds and a whole launch here well under a
second, so working code cannot hit the limit, and a protocol error fails loudly
instead of waiting 20 s and passing through the per-sweep rerun.  For the same
reason every run that means to use the grid kernel asserts the plan first and
the counters afterwards: grid launches up by the planned count, no rerun.
"""

import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import elementwise_cases as C
import ell_cases as L
import extended_twin as T
import test_gpu_extended_range as G
from conftest import ORACLE_DIR, PKG_DIR, ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KEYS = ("IRLMX_FUSED_MAX_STATES", "IRLMX_CLUSTER", "IRLMX_GRID", "IRLMX_XCD_GROUP", "IRLMX_EXT_GRID_MIN_STATES",
        "IRLMX_EXT_GRID_MAX_LAUNCHES", "IRLMX_PLAN_CUS", "IRLMX_PLAN_GRID_PER_CU", "IRLMX_TEST_NOT_RESIDENT",
        "IRLMX_TEST_DROP_TILE")
ALWAYS = {"IRLMX_STRICT_EXCHANGE": "1", "IRLMX_TEST_EXCHANGE_TIMEOUT_MS": "2000"}
#: the grid shape at any size, up to three sequential launches
FORCED = {"IRLMX_EXT_GRID_MIN_STATES": 0, "IRLMX_FUSED_MAX_STATES": 0, "IRLMX_EXT_GRID_MAX_LAUNCHES": 3}
#: the per-sweep extended pass on the same inputs
PER_SWEEP = {"IRLMX_EXT_GRID_MIN_STATES": 0, "IRLMX_FUSED_MAX_STATES": 0, "IRLMX_GRID": 0}
TESTS_DIR = os.path.join(ROOT, "tests")


def capacity(workgroups):
    """Planner keys for a planned capacity of that many workgroups (the launch
    itself still checks co-residency on the device)."""
    return {"IRLMX_PLAN_CUS": workgroups, "IRLMX_PLAN_GRID_PER_CU": 1}


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    import irlmx
    return irlmx.require_device()


@pytest.fixture
def env(monkeypatch):
    """Set exactly the given planner keys (beside the strict exchange with its
    2 s limit); all of them are cleared afterwards."""
    def set_env(values):
        for k in KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in ALWAYS.items():
            monkeypatch.setenv(k, v)
        for k, v in values.items():
            assert k in KEYS, k
            monkeypatch.setenv(k, str(v))
    set_env({})
    yield set_env
    for k in KEYS + tuple(ALWAYS):
        monkeypatch.delenv(k, raising=False)


def grid_plan(mdp, **want):
    from irlmx import ops
    plan = ops.execution_plan(mdp, "backward", extended_range=True)
    assert plan["shape"] == "grid" and plan["threads"] == 256, plan
    assert plan["launches"] * plan["per_launch"] >= mdp.batch > (plan["launches"] - 1) * plan["per_launch"], plan
    assert plan["C"] == -(-mdp.n_states // (256 * plan["spt"])), plan
    for k, v in want.items():
        assert plan[k] == v, (k, plan)
    return plan


def run_grid(mdp, reward, term, **want):
    """(policy, status) on the grid shape: the plan asserted before the run, the counters after it."""
    from irlmx import ops
    plan = grid_plan(mdp, **want)
    before = ops.counters()
    pi, status = G.run_ext(mdp, reward, term)
    after = ops.counters()
    diff = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert diff == {"grid_launches": plan["launches"]}, (diff, plan)
    return pi, status


def run_sweep(mdp, reward, term):
    from irlmx import ops
    G.assert_sweep_plan(mdp)
    before = ops.counters()
    pi, status = G.run_ext(mdp, reward, term)
    after = ops.counters()
    assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {"sweep_calls": 1}
    return pi, status


def stencil_mdp(rv, W, H, dev):
    from irlmx import DeviceMDP, _lib
    rv = np.asarray(rv)
    return DeviceMDP(_lib.LAYOUT_STENCIL5, W * H, 4, rv.shape[0], False, torch.as_tensor(rv.copy(), device=dev),
                     width=W, height=H, device=dev)


_ref = {}


def per_sweep(key, env, mdp, reward, term):
    """The per-sweep extended pass on these inputs, computed once per key (the
    caller's keys are set again by the caller)."""
    if key not in _ref:
        env(PER_SWEEP)
        pi, status = run_sweep(mdp, reward, term)
        assert (status == 0).all(), (key, status)
        _ref[key] = pi
    return _ref[key]


def in_range(name, dev):
    W, H = (16, 16) if name == "16x16" else (37, 23)
    from irlmx import ops
    c = C.stencil(W, H)
    return c, stencil_mdp(c.rv, W, H, dev), c.reward.copy(), ops.terminal_mask(c.terminal, c.S, batch=c.B, device=dev)


# -- 1. forced small shapes -----------------------------------------------------------

def test_one_workgroup_per_instance(dev, env):
    cases = G.launches()[0]                                    # 64 x 4 x 3: S = 256
    mdp = G.wide_mdp(cases, dev)
    reward, tm = G.wide_inputs(cases, dev)
    ref = per_sweep("64x4", env, mdp, reward, tm)
    env(FORCED)
    pi, status = run_grid(mdp, reward, tm, C=1, spt=1, launches=1, per_launch=3)
    assert (status == 0).all() and torch.equal(pi, ref)


@pytest.mark.parametrize("name", ["16x16", "37x23"])
def test_in_range_equals_ordinary_pass(dev, env, name):
    from irlmx import ops
    c, mdp, reward, tm = in_range(name, dev)
    ref = per_sweep(name, env, mdp, reward, tm)
    env({})
    ordinary = ops.backward_maxent(mdp, reward, tm)
    env(FORCED)
    pi, status = run_grid(mdp, reward, tm, spt=1, launches=1, per_launch=3, C=1 if name == "16x16" else 4)
    assert (status == 0).all() and bool(torch.isfinite(ordinary).all())
    assert torch.equal(pi, ref) and torch.equal(pi, ordinary)


@pytest.mark.parametrize("cap,spt", [(3, 2), (1, 4)])
def test_states_per_thread(dev, env, cap, spt):
    """37 x 23 (851 states) x 3 with the planned capacity shrunk: two and four
    states per thread, one instance per launch."""
    c, mdp, reward, tm = in_range("37x23", dev)
    ref = per_sweep("37x23", env, mdp, reward, tm)
    env({**FORCED, **capacity(cap)})
    pi, status = run_grid(mdp, reward, tm, spt=spt, C=4 // spt, launches=3, per_launch=1)
    assert (status == 0).all() and torch.equal(pi, ref)


@pytest.mark.parametrize("name,form", [("k5-s1029", "sorted"), ("k8-s1029", "sorted"), ("k16-s1029", "sorted"),
                                       ("k5-s200", "scrambled")])
def test_ell(dev, env, name, form):
    """ELL models with one table per instance: 1,029 states on five workgroups
    (the last one holds 5 states) in the 5-, 8- and 16-slot classes, and 200
    states with scrambled slots (7 slots: the 8-slot class)."""
    from irlmx import ops
    c = L.case(name)
    mdp = L.device_model(c, dev, form)
    tm = ops.terminal_mask(c.terminal, c.S, batch=c.B, device=dev)
    reward = c.reward.copy()
    ref = per_sweep((name, form), env, mdp, reward, tm)
    env({})
    ordinary = ops.backward_maxent(mdp, reward, tm)
    env(FORCED)
    pi, status = run_grid(mdp, reward, tm, spt=1, C=-(-c.S // 256), launches=1, per_launch=c.B)
    assert (status == 0).all()
    assert torch.equal(pi, ref) and torch.equal(pi, ordinary)


# -- 2. wide range -------------------------------------------------------------------------

@pytest.mark.parametrize("i", [0, 1, 2], ids=["64x4x3", "128x4", "256x4"])
def test_wide_range(dev, env, i):
    from irlmx import ops
    cases = G.launches()[i]
    mdp = G.wide_mdp(cases, dev)
    reward, tm = G.wide_inputs(cases, dev)
    env(FORCED)
    pi, status = run_grid(mdp, reward, tm, spt=1, C=cases[0].S // 256, launches=1)
    assert (status == 0).all()
    G.assert_within_bound(pi, cases, "grid")
    env({})
    assert T.nan_rows(ops.backward_maxent(mdp, reward, tm).cpu().numpy()) > 0, "the ordinary pass no longer fails here"


# -- 3. the default route at the floor ---------------------------------------------------------

def test_default_route_at_the_floor(dev, env):
    """128 x 64, all keys at their defaults: the grid shape, one launch, 16,383
    collapsed sweeps.  (No longdouble comparison at this size.)"""
    from irlmx import ops
    case = T.wide(128, 64, -7.0)
    mdp = G.wide_mdp([case], dev)
    reward, tm = G.wide_inputs([case], dev)
    env({})
    assert 2 * case.S - 1 == 16383
    pi, status = run_grid(mdp, reward, tm, spt=1, C=32, launches=1, per_launch=1)
    assert (status == 0).all() and bool(torch.isfinite(pi).all())
    assert T.nan_rows(ops.backward_maxent(mdp, reward, tm).cpu().numpy()) > 0
    env({"IRLMX_GRID": 0})
    assert G.assert_sweep_plan(mdp)["launches"] == 16383
    swept, status = run_sweep(mdp, reward, tm)
    assert (status == 0).all() and torch.equal(pi, swept)


# -- 4. sequential launches ---------------------------------------------------------------------

@pytest.mark.parametrize("cap,ipl,launches", [(4, 1, 3), (8, 2, 2)])
def test_sequential_launches(dev, env, cap, ipl, launches):
    c, mdp, reward, tm = in_range("37x23", dev)
    ref = per_sweep("37x23", env, mdp, reward, tm)
    env({**FORCED, **capacity(cap)})
    pi, status = run_grid(mdp, reward, tm, spt=1, C=4, launches=launches, per_launch=ipl)
    assert (status == 0).all() and torch.equal(pi, ref)
    back = stencil_mdp(c.rv[::-1], 37, 23, dev)
    rpi, status = run_grid(back, reward[::-1].copy(), tm, spt=1, C=4, launches=launches, per_launch=ipl)
    assert (status == 0).all() and torch.equal(rpi, ref.flip(0))


# -- 5. the rerun path -----------------------------------------------------------------------------

def test_rendezvous_miss_reruns_per_sweep(dev, env):
    from irlmx import ops
    c, mdp, reward, tm = in_range("37x23", dev)
    ref = per_sweep("37x23", env, mdp, reward, tm)
    env({**FORCED, "IRLMX_TEST_NOT_RESIDENT": 1})
    grid_plan(mdp, launches=1)
    before = ops.counters()
    pi, status = G.run_ext(mdp, reward, tm)
    after = ops.counters()
    diff = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert diff == {"grid_launches": 1, "rerun_not_resident": 1, "sweep_calls": 1}, diff
    assert (status == 0).all() and torch.equal(pi, ref)


# -- 6. other behaviour ------------------------------------------------------------------------------

def test_nonfinite_reward(dev, env):
    cases = G.launches()[0]
    mdp = G.wide_mdp(cases, dev)
    reward, tm = G.wide_inputs(cases, dev)
    ref = per_sweep("64x4", env, mdp, reward, tm)
    bad = reward.copy()
    bad[1, 17] = 800.0                                         # exp(800) = inf
    env(FORCED)
    pi, status = run_grid(mdp, bad, tm, launches=1)
    assert (status == 0).all()
    assert bool(torch.isnan(pi[1]).all())
    assert torch.equal(pi[0], ref[0]) and torch.equal(pi[2], ref[2])
    bad[1, 17] = np.nan
    pi, status = run_grid(mdp, bad, tm, launches=1)
    assert bool(torch.isnan(pi[1]).all()) and torch.equal(pi[0], ref[0]) and torch.equal(pi[2], ref[2])


def test_unreachable_region(dev, env):
    """test_gpu_extended_range.test_unreachable_region's world on the grid shape:
    columns x <= 1 cannot be left, zs = 0 there and the policy rows are 0 / 0."""
    from irlmx import DeviceMDP, ops
    size = 8
    S = size * size
    rv = DeviceMDP.gridworld(size, device=dev).row_val.cpu().numpy()[0].copy()
    s = np.arange(S)
    edge = s % size == 1
    rv[:, 0, edge] += rv[:, 1, edge]
    rv[:, 1, edge] = 0.0
    mdp = stencil_mdp(rv[None], size, size, dev)
    reward = np.random.default_rng(S).uniform(-1.0, 0.0, S)
    tm = ops.terminal_mask([S - 1], S, device=dev)
    env(PER_SWEEP)
    swept, _ = run_sweep(mdp, reward, tm)
    env(FORCED)
    pi, status = run_grid(mdp, reward, tm, C=1, launches=1)
    got = pi[0].cpu().numpy()
    walled = s % size <= 1
    assert np.isnan(got[walled]).all() and np.isfinite(got[~walled]).all() and (status == 0).all()
    assert (got[s % size == 2, 1] == 0).all()
    assert np.array_equal(got, swept[0].cpu().numpy(), equal_nan=True)


CHECKS = textwrap.dedent("""
    import json, os, sys
    sys.path[:0] = [{root!r}, {pkg!r}, {oracle!r}, {tests!r}]
    import numpy as np, torch
    import test_gpu_extended_grid as E
    from irlmx import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    os.environ.update(E.ALWAYS)
    os.environ.update({{k: str(v) for k, v in E.FORCED.items()}})
    c, mdp, reward, tm = E.in_range("37x23", dev)
    pi, status = E.run_grid(mdp, reward, tm, spt=1, C=4, launches=1)
    out = {{"enabled": int(lib.irlmx_device_checks_enabled()), "fails": ops.device_check_failures(),
           "status": [int(x) for x in status]}}
    np.save({npy!r}, pi.cpu().numpy())
    json.dump(out, open({out!r}, "w"))
""")


def test_device_check_build(dev, env, tmp_path):
    """37 x 23 x 3 on the grid shape under libirlmx_checks.so: no failed bounds
    check and the same bits as the product build."""
    import __graft_entry__ as g
    c, mdp, reward, tm = in_range("37x23", dev)
    ref = per_sweep("37x23", env, mdp, reward, tm)
    res, npy = str(tmp_path / "checks.json"), str(tmp_path / "checks.npy")
    code = CHECKS.format(root=ROOT, pkg=PKG_DIR, oracle=ORACLE_DIR, tests=TESTS_DIR, out=res, npy=npy)
    e = {k: v for k, v in os.environ.items() if k not in KEYS}
    e["IRLMX_LIB"] = g.LIB_CHECKS
    subprocess.run([sys.executable, "-c", code], env=e, cwd=ROOT, check=True, timeout=300)
    out = json.load(open(res))
    assert out == {"enabled": 1, "fails": 0, "status": [0, 0, 0]}, out
    assert np.array_equal(np.load(npy), ref.cpu().numpy())


# -- 7. the batched driver ------------------------------------------------------------------------------

def test_batched_driver_auto(dev, env):
    """BatchedMaxEnt(extended_range="auto") on the 64 x 4 x 3 inputs: the two
    out-of-range instances are rerun on the grid shape every step; the same
    steps and the same theta, bit for bit, as with the per-sweep extended pass."""
    from irlmx import ops
    from irlmx.batch import BatchedMaxEnt
    cases = G.launches()[0]
    mdp = G.wide_mdp(cases, dev)
    reward, _ = G.wide_inputs(cases, dev)
    S = cases[0].S
    p0 = np.zeros((3, S))
    p0[:, S - 1] = 1.0                                         # starts in the terminal: the forward ends (two sweeps)
    e_features = np.full((3, S), 1.0 / S)
    n_steps = 2

    def run(keys):
        env(keys)
        d = BatchedMaxEnt(mdp, e_features, p0, cases[0].terminal, theta0=reward, extended_range="auto")
        before = ops.counters()
        pis = []
        for _ in range(n_steps):
            pis.append(d.backward().clone())
            d.step()
        after = ops.counters()
        return d, pis, {k: after[k] - before[k] for k in after}

    swept, pis_s, ds = run({**PER_SWEEP, "IRLMX_CLUSTER": 0})   # (the ordinary passes per sweep in both runs)
    env(FORCED)
    assert ops.execution_plan(mdp.take(torch.tensor([0, 1], device=dev)), "backward",
                              extended_range=True)["shape"] == "grid"
    grid, pis_g, dg = run({**FORCED, "IRLMX_CLUSTER": 0})
    assert ds["grid_launches"] == 0 and ds["rerun_not_resident"] == 0 and ds["rerun_timeout"] == 0, ds
    # a backward() and a step() per step, each rerunning its suspects in one persistent launch
    assert dg["grid_launches"] == 2 * n_steps and dg["rerun_not_resident"] == 0 and dg["rerun_timeout"] == 0, dg
    for a, b in zip(pis_g, pis_s):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    assert bool(torch.isfinite(pis_g[0]).all())
    assert torch.equal(grid.steps, swept.steps) and grid.k == swept.k == n_steps
    assert torch.equal(grid.theta, swept.theta) and bool(torch.isfinite(grid.theta).all())
