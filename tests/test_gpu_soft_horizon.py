"""The finite-horizon soft value iteration on the device (needs an MI355X).

ops.soft_backward_horizon (csrc/soft_horizon.hip) against
tests/soft_horizon_twin.py on tests/horizon_twin.py's cases, each at discount 1
and 0.9, each asserting its plan first:

* every entry of pi_t elementwise and V_0 normwise against the longdouble
  restatement, under 16 x max(e_twin, e_floor) -- the project's rule, e_twin
  the float64 twin's own error on the same input; the NaN / zero pattern and the
  status equal to the twin's;
* bit for bit: every fused instantiation against per sweep, the batch reversed,
  every instance of a per-instance-table launch alone, the device bounds-check
  build;
* on the deterministic GridWorld at discount 1 the non-causal horizon pass;
* the gradient identity d(p0 . V_0) / d r = D by central differences on the
  device; non-finite rewards; the batched driver and the drop-ins.

The measured ratios e_kernel / max(e_twin, e_floor) are printed per instance
(profiles/soft_horizon.txt records one run).
"""

import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import extended_ref as X
import horizon_twin as H
import soft_horizon_twin as SH
from conftest import ORACLE_DIR, PKG_DIR, ROOT, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LD = np.longdouble
KEY = "IRLMX_FUSED_MAX_STATES"            # 0: every size per sweep
BATCH_KEY = "IRLMX_HORIZON_FUSED_BATCH"   # 1: several states per thread run fused at any batch
TESTS_DIR = os.path.join(ROOT, "tests")
TABLES_LDS = 1536                         # the NpTables copy in front of V's two buffers


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    import irlmx
    return irlmx.require_device()


@pytest.fixture
def env(monkeypatch):
    """``env("sweep")``: every size through the per-sweep shape; ``env("fused")``:
    the fused shape wherever a kernel is instantiated, also with several states
    per thread below the batch the planner asks for; cleared afterwards."""
    def set_env(mode="default"):
        monkeypatch.delenv(KEY, raising=False)
        monkeypatch.delenv(BATCH_KEY, raising=False)
        if mode == "sweep":
            monkeypatch.setenv(KEY, "0")
        if mode == "fused":
            monkeypatch.setenv(BATCH_KEY, "1")
    set_env()
    yield set_env
    set_env()


def run_backward(mdp, reward, discount, T, terminal):
    """(pi_t, V_0, status) through the C ABI (ops.soft_backward_horizon does not return the status)."""
    from irlmx import _lib, ops
    lib = _lib.load()
    B, S, A = mdp.batch, mdp.n_states, mdp.n_actions
    r = torch.as_tensor(np.array(reward, dtype=np.float64), device=mdp.device).reshape(B, S).contiguous()
    pi = torch.full((B, T, S, A), -7.0, dtype=torch.float64, device=mdp.device)
    v0 = torch.full((B, S), -7.0, dtype=torch.float64, device=mdp.device)
    status = torch.full((B,), -7, dtype=torch.int32, device=mdp.device)
    ws, n = ops._workspace(mdp, _lib.OP_SOFT_BACKWARD_HORIZON)
    _lib.check(lib.irlmx_soft_backward_horizon(mdp.struct(), _lib.ptr(r), _lib.ptr(terminal), float(discount), T,
                                               _lib.ptr(pi), _lib.ptr(v0), _lib.ptr(status), _lib.ptr(ws), n,
                                               _lib.stream_ptr(mdp.device)), "soft_backward_horizon")
    return pi, v0, status


def run_case(c, dev, discount, tables=None, reward=None):
    """The pass on case c (of the instances ``tables``): numpy arrays pi, v0, status."""
    from irlmx import ops
    idx = list(range(c.B)) if tables is None else list(tables)
    mdp = c.device_model(dev, tables=tables)
    tm = ops.terminal_mask(c.terminal, c.S, batch=mdp.batch, device=mdp.device) if c.terminal else None
    r = (c.reward if reward is None else reward)[idx]
    pi, v0, st = run_backward(mdp, r, discount, c.T, tm)
    plain = ops.soft_backward_horizon(mdp, r, discount, c.T, tm)         # without V_0: the same policy
    assert torch.equal(plain.view(torch.int64), pi.view(torch.int64))
    return {"pi": pi.cpu().numpy(), "v0": v0.cpu().numpy(), "status": st.cpu().numpy()}


def assert_plan(c, dev, mode="default"):
    """Fused with the case's (states per thread, slot class) pair -- by default
    only at one state per thread (the cases' batches are far below one workgroup
    per CU), under env("fused") wherever the case names a pair; else per sweep."""
    from irlmx import _lib, ops
    mdp = c.device_model(dev)
    p = ops.execution_plan(mdp, "soft_backward_horizon")
    assert p == ops.execution_plan(mdp, _lib.OP_SOFT_BACKWARD_HORIZON)
    spt = None if c.bwd is None else c.bwd[0]
    if spt is not None and (mode == "fused" or (mode == "default" and spt == 1)):
        assert p["shape"] == "fused" and p["spt"] == spt and p["launches"] == 1, (c.name, p)
        assert p["lds_bytes"] == TABLES_LDS + 16 * c.S and p["spt"] * p["threads"] >= c.S, (c.name, p)
        per = -(-c.S // spt)
        assert p["threads"] == min(1024, -(-per // 64) * 64), (c.name, p)
    else:
        assert (p["shape"], p["spt"], p["threads"], p["launches"], p["lds_bytes"]) == ("sweep", 1, 256, 0, 0), p


_results = {}


def results(name, discount, dev):
    """The default-plan run of a case, computed once."""
    if (name, discount) not in _results:
        c = H.case(name)
        assert_plan(c, dev)
        _results[name, discount] = run_case(c, dev, discount)
    return _results[name, discount]


def same(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        same_bits = np.array_equal(x.view(np.int64), y.view(np.int64)) if x.dtype == np.float64 else np.array_equal(x, y)
        assert same_bits, f"{what}: {k} differs"


@pytest.mark.parametrize("discount", SH.DISCOUNTS)
@pytest.mark.parametrize("name", SH.CASES)
def test_accuracy(dev, env, name, discount):
    """pi_t elementwise and V_0 normwise of every instance under 16 x max(e_twin,
    e_floor); status and the NaN / zero pattern as the twin's (elementwise_err
    raises on either).  Measured ratios (one MI355X): profiles/soft_horizon.txt."""
    c = H.case(name)
    got = results(name, discount, dev)
    for b in range(c.B):
        e_pi, e_v0 = SH.errors(got["pi"][b], got["v0"][b], name, discount, b)
        t_pi, t_v0 = SH.e_twin(name, discount, b)
        b_pi, b_v0 = SH.bounds(name, discount, b)
        floor = X.e_floor(c.K, c.A)
        print(f"[soft horizon] {name}[{b}] g {discount} T {c.T} ratio pi {e_pi / max(t_pi, floor):.2f} "
              f"V0 {e_v0 / max(t_v0, floor):.2f} | e_kernel pi {e_pi:.2e} V0 {e_v0:.2e} | e_twin pi {t_pi:.2e} "
              f"V0 {t_v0:.2e}")
        assert e_pi <= b_pi, (name, b, e_pi, b_pi)
        assert e_v0 <= b_v0, (name, b, e_v0, b_v0)
        tpi, tv0, tstatus = SH.twin(name, discount, b)
        assert got["status"][b] == tstatus == SH.OK
        assert np.array_equal(np.isnan(got["pi"][b]), np.isnan(tpi)) and np.array_equal(got["pi"][b] == 0, tpi == 0)
        assert np.isfinite(got["pi"][b]).all() and np.isfinite(got["v0"][b]).all()
        if c.terminal:                                   # held: V_0 = r, bit for bit
            assert np.array_equal(got["v0"][b][c.terminal], c.reward[b][c.terminal])


@pytest.mark.parametrize("discount", SH.DISCOUNTS)
@pytest.mark.parametrize("name", H.FUSED)
def test_fused_equals_sweep(dev, env, name, discount):
    """Every fused instantiation -- those with several states per thread forced
    below their batch threshold -- and the per-sweep shape: the same bits."""
    c = H.case(name)
    default = results(name, discount, dev)
    for mode in ("fused", "sweep"):
        env(mode)
        assert_plan(c, dev, mode)
        same(run_case(c, dev, discount), default, f"{name} {mode}")


@pytest.mark.parametrize("name,discount", [("16x16", 1.0), ("16x16", 0.9), ("k5-s200", 0.9), ("128x40", 0.9)])
def test_batch_order_and_instances_alone(dev, env, name, discount):
    """Per-instance tables: the batch reversed gives reversed results, and every
    instance equals its table run alone."""
    c = H.case(name)
    whole = results(name, discount, dev)
    order = list(range(c.B))[::-1]
    same(run_case(c, dev, discount, tables=order), {k: v[order] for k, v in whole.items()}, name + " reversed")
    for b in range(c.B):
        same(run_case(c, dev, discount, tables=[b]), {k: v[[b]] for k, v in whole.items()}, f"{name}[{b}] alone")


@pytest.mark.parametrize("mode", ["fused", "sweep"])
def test_nan_reward_marks_its_instance_only(dev, env, mode):
    """A NaN reward in instance 1 of 3: NONFINITE for that instance alone, the
    twin's NaN pattern (one neighbourhood further per step), and the others
    bit-identical to their solo runs."""
    c = H.case("16x16")
    env(mode)
    r = c.reward.copy()
    r[1, 77] = np.nan
    got = run_case(c, dev, 0.9, reward=r)
    assert list(got["status"]) == [SH.OK, SH.NONFINITE, SH.OK]
    tpi, tv0, tstatus = SH.backward(c.model(1), c.terminal, r[1], 0.9, c.T)
    assert tstatus == SH.NONFINITE and np.isnan(tv0[77])
    assert np.array_equal(np.isnan(got["pi"][1]), np.isnan(tpi)) and np.array_equal(np.isnan(got["v0"][1]), np.isnan(tv0))
    assert np.isnan(got["pi"][1][c.T - 1]).sum() == 5 * 4 and not np.isnan(got["pi"][1][c.T - 1, 0]).any()
    for b in (0, 2):
        same({k: v[[b]] for k, v in got.items()}, run_case(c, dev, 0.9, tables=[b]), f"instance {b}")


CHECKS = textwrap.dedent("""
    import json, os, sys
    sys.path[:0] = [{root!r}, {pkg!r}, {oracle!r}, {tests!r}]
    import numpy as np
    import __graft_entry__ as g
    g.build()
    import irlmx
    from irlmx import _lib, ops
    import horizon_twin as H
    import test_gpu_soft_horizon as G
    dev = irlmx.require_device()
    out = {{"enabled": int(_lib.load().irlmx_device_checks_enabled()), "fails": []}}
    arrays = {{}}
    for sweep in (0, 1):
        os.environ[G.BATCH_KEY] = "1"
        if sweep:
            os.environ[G.KEY] = "0"
        for name in {names!r}:
            got = G.run_case(H.case(name), dev, 0.9)
            out["fails"].append(ops.device_check_failures())
            for k, v in got.items():
                arrays[f"{{name}}.{{sweep}}.{{k}}"] = v
    np.savez({npz!r}, **arrays)
    json.dump(out, open({out!r}, "w"))
""")


def test_device_check_build(dev, env, tmp_path):
    """ELL and stencil cases under libirlmx_checks.so, fused and per sweep, in a
    fresh process: no check bit set and the same bits as the product build."""
    import __graft_entry__ as g
    names = ("k5-s200", "k8-s1029", "k40-s300", "hub-s200", "37x23")
    res, npz = str(tmp_path / "checks.json"), str(tmp_path / "checks.npz")
    code = CHECKS.format(root=ROOT, pkg=PKG_DIR, oracle=ORACLE_DIR, tests=TESTS_DIR, out=res, npz=npz, names=names)
    e = {k: v for k, v in os.environ.items() if k not in (KEY, BATCH_KEY)}
    e["IRLMX_LIB"] = g.LIB_CHECKS
    subprocess.run([sys.executable, "-c", code], env=e, cwd=ROOT, check=True, timeout=300)
    out = json.load(open(res))
    assert out["enabled"] == 1 and out["fails"] == [0] * (2 * len(names)), out
    z = np.load(npz)
    for name in names:
        want = results(name, 0.9, dev)
        for sweep in (0, 1):
            same({k: z[f"{name}.{sweep}.{k}"] for k in want}, want, f"{name} checks {sweep}")


def test_deterministic_gridworld_is_the_non_causal_pass(dev, env):
    """DeviceMDP.gridworld(12) at discount 1, T = 20: pi_t agrees with
    ops.backward_maxent_horizon and V_0 with its log_z0, within the sum of the
    two passes' bounds (each 16 x max(e_twin, e_floor) of its own CPU twin
    against its own longdouble restatement on the same table and reward)."""
    from irlmx import DeviceMDP, ops
    from test_horizon_twin import deterministic_grid
    size, T = 12, 20
    S = size * size
    mod = H.stencil_model(deterministic_grid(size, size), size, size)
    reward = np.random.default_rng(22).uniform(-1.5, 0.0, S)
    mdp = DeviceMDP.gridworld(size, device=dev)
    P = mdp.to_dense()
    for a, m in enumerate(mod.mats):
        assert np.array_equal(P[:, :, a], m.toarray())                # the twin's table is the device's
    pi, v0 = ops.soft_backward_horizon(mdp, reward, 1.0, T, return_value0=True)
    hpi, hlz = ops.backward_maxent_horizon(mdp, reward, T, return_log_z0=True)
    tpi, tv0, _ = SH.backward(mod, [], reward, 1.0, T)
    rpi, rv0 = SH.backward_ref(mod.mats, [], reward, 1.0, T)
    htpi, htlz = H.backward(mod, [], reward, T)
    hrpi, hrlz = H.backward_ref(mod.mats, [], reward, T)
    b_pi = X.bound(X.elementwise_err(tpi, rpi), mod.K, mod.A) + X.bound(X.elementwise_err(htpi, hrpi), mod.K, mod.A)
    b_v0 = X.bound(X.normwise_err(tv0, rv0), mod.K, mod.A) + X.bound(X.normwise_err(htlz, hrlz), mod.K, mod.A)
    e_pi = X.elementwise_err(pi[0].cpu().numpy(), hpi[0].cpu().numpy())
    e_v0 = X.normwise_err(v0[0].cpu().numpy(), hlz[0].cpu().numpy())
    print(f"[soft horizon] gridworld(12) against the non-causal pass: pi {e_pi:.2e} (bound {b_pi:.2e}) "
          f"V0 {e_v0:.2e} (bound {b_v0:.2e})")
    assert e_pi <= b_pi and e_v0 <= b_v0, (e_pi, b_pi, e_v0, b_v0)


def test_gradient_identity_on_the_device(dev, env):
    """16x16 instance 0, T = 10, discount 1, h = 1e-3: the central difference of
    p0 . V_0 in r(s) against D(s) of ops.forward_svf_horizon under pi_t, at
    every 37th state.  |FD - D| <= 2 tau + 4 b_V max|V_0| / h: tau the
    longdouble truncation error at the same h (about 4.5e-7 by the h^2 law of
    tests/test_soft_horizon_twin.py), b_V the V_0 bound of the accuracy test
    on this input.  The 2 x 7 perturbed rewards run as one batch."""
    from irlmx import ops
    c = H.case("16x16")
    T, h, mod, r, p0 = 10, 1e-3, c.model(0), c.reward[0], c.p0[0]
    states = sorted(set(range(0, c.S, 37)))
    tau = float(np.max(np.abs(SH.fd_gradient(mod.mats, [], r, p0, T, h, states)
                              - SH.visitation_ref(mod.mats, [], r, p0, T)[states])))
    _, tv0, _ = SH.backward(mod, [], r, 1.0, T)
    b_v = X.bound(X.normwise_err(tv0, SH.backward_ref(mod.mats, [], r, 1.0, T, policy=False)[1]), c.K, c.A)
    rewards = np.tile(r, (2 * len(states), 1))
    for i, s in enumerate(states):
        rewards[2 * i, s] += h
        rewards[2 * i + 1, s] -= h
    mdp = c.device_model(dev, tables=[0] * len(rewards))
    _, v0 = ops.soft_backward_horizon(mdp, rewards, 1.0, T, return_value0=True)
    J = (v0.cpu().numpy().astype(LD) * p0.astype(LD)).sum(axis=1)
    hs = np.array([(LD(r[s] + h) - LD(r[s] - h)) for s in states])       # the step actually taken, in float64 rewards
    fd = (J[0::2] - J[1::2]) / hs
    one = c.device_model(dev, tables=[0])
    pi, v0_one = ops.soft_backward_horizon(one, r.copy(), 1.0, T, return_value0=True)
    D, _, _ = ops.forward_svf_horizon(one, p0.copy(), pi)
    err = float(np.max(np.abs(fd - D[0].cpu().numpy()[states].astype(LD))))
    allowed = 2 * tau + 4 * b_v * float(v0_one.abs().max()) / h
    print(f"[soft horizon] gradient identity: |FD - D| {err:.2e}, tau {tau:.2e}, allowed {allowed:.2e}")
    assert 1e-7 < tau < 1e-6 and err <= allowed, (err, tau, allowed)


# ---------------------------------------------------------------------------
# the batched driver
# ---------------------------------------------------------------------------

DRIVER_T = 12
DRIVER_G = 0.9


def driver_world(dev):
    from irlmx import DeviceMDP
    return DeviceMDP.icy_gridworld(12, [0.2, 0.1, 0.3], device=dev)


_demos = {}


def demonstrations(dev):
    """Rollouts of DRIVER_T steps without a terminal state under a policy of a
    planted reward: (mdp, states, lengths), computed once."""
    if not _demos:
        from irlmx import _lib, ops
        mdp = driver_world(dev)
        S = mdp.n_states
        theta = np.random.default_rng(3).uniform(0.2, 1.2, (3, S))
        pi = ops.soft_backward_horizon(mdp, theta, DRIVER_G, DRIVER_T)
        none = torch.zeros((3, S), dtype=torch.uint8, device=dev)
        ro = ops.rollout(mdp, pi[:, 0].contiguous(), none, [5, 70, 130], 64, DRIVER_T, seed=11,
                         return_trajectories=True)
        assert (ro.status == _lib.TRAJ_TRUNCATED).all() and (ro.lengths == DRIVER_T).all()
        _demos["v"] = (mdp, ro.states, ro.lengths)
    return _demos["v"]


def driver(dev, **kw):
    from irlmx.batch import BatchedCausalHorizon
    mdp, states, lengths = demonstrations(dev)
    return BatchedCausalHorizon.from_trajectories(mdp, states, lengths, [], horizon=DRIVER_T, discount=DRIVER_G, **kw)


def test_driver_step_is_the_three_ops(dev, env):
    from irlmx import ops
    from irlmx.batch import BatchedCausalHorizon, BatchedMaxEnt
    m = driver(dev)
    assert isinstance(m, BatchedCausalHorizon) and m.horizon == DRIVER_T and m.discount == DRIVER_G
    assert float(m.e_features.sum(dim=1).max()) == DRIVER_T + 1 == float(m.e_features.sum(dim=1).min())
    theta0 = m.theta.clone()
    pi = ops.soft_backward_horizon(m.mdp, theta0, DRIVER_G, DRIVER_T)
    svf, sweeps, _ = ops.forward_svf_horizon(m.mdp, m.p_initial, pi)
    want = m.optimizer.apply(theta0, m.e_features - svf, 0)
    back = m.backward()
    assert tuple(back.shape) == (3, DRIVER_T, m.mdp.n_states, 4) and torch.equal(back, pi)
    assert not torch.equal(pi, ops.backward_maxent_horizon(m.mdp, theta0, DRIVER_T))      # not the non-causal pass
    got_svf = m.step()
    assert torch.equal(got_svf, svf) and torch.equal(m.theta, want)
    assert m.last_forward_sweeps.tolist() == [DRIVER_T] * 3
    with pytest.raises(NotImplementedError, match="time-indexed"):
        m.log_likelihood(None, None, None)
    with pytest.raises(NotImplementedError, match="time-indexed"):
        m.expected_value_difference(theta0, 0.9)
    with pytest.raises(ValueError, match="non-causal"):
        BatchedMaxEnt(m.mdp, m.e_features, m.p_initial, [], horizon=DRIVER_T, causal=True, discount=0.9)
    with pytest.raises(ValueError, match="discount"):
        BatchedCausalHorizon(m.mdp, m.e_features, m.p_initial, [], DRIVER_T, discount=1.5)
    direct = BatchedCausalHorizon(m.mdp, m.e_features, m.p_initial, [], DRIVER_T, DRIVER_G)
    assert torch.equal(direct.step(), svf)


def test_driver_planted_statistics_and_compaction(dev, env):
    """With e_features = the device's own D(theta*), the first gradient is
    exactly 0 and theta stays theta*.  Planted in instance 0 alone, that
    instance stops after one step, so a compacted run works on fewer instances
    from step 2 on -- and ends with the same theta and steps as the uncompacted one."""
    from irlmx import ops
    ref = driver(dev)
    star = torch.as_tensor(np.random.default_rng(4).uniform(0.3, 1.1, tuple(ref.theta.shape)), device=dev)
    D, _, _ = ops.forward_svf_horizon(ref.mdp, ref.p_initial,
                                      ops.soft_backward_horizon(ref.mdp, star, DRIVER_G, DRIVER_T))
    m = driver(dev, theta0=star.cpu().numpy())
    m.e_features = D.clone()
    m.run(max_steps=3)
    assert torch.equal(m.theta, star) and m.steps.tolist() == [1, 1, 1] and float(m.last_delta.abs().max()) == 0.0

    runs = []
    for compact in (True, False):
        m = driver(dev, theta0=star.cpu().numpy())
        m.e_features[0] = D[0]
        seen = []
        m.run(eps=1e-3, max_steps=12, compact=compact, on_step=lambda o: seen.append(o.working_batch))
        runs.append((m.theta.clone(), m.steps.clone(), seen))
    assert runs[0][1].tolist()[0] == 1 and min(runs[0][1].tolist()[1:]) > 1, runs[0][1]
    assert runs[0][2][0] == 3 and runs[0][2][1] == 2 and set(runs[1][2]) == {3}, (runs[0][2], runs[1][2])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_dropins_and_driver_on_config1(dev, env):
    """maxent.irl_causal_horizon on BASELINE config 1's 5 x 5 world without a
    terminal state, its demonstrations cut after 10 steps: runs to its stopping
    rule and gives the driver's theta within 1e-9; the drop-ins equal ops bit
    for bit."""
    import maxent as M
    import maxent_oracle as O
    from conftest import unpack_trajectories
    from irlmx import DeviceMDP, ops
    from irlmx.batch import BatchedCausalHorizon
    z = load_golden("config1")
    T, g = 10, 0.9
    tjs = [O.Trajectory(t.transitions()[:T]) for t in unpack_trajectories(z["traj_flat"], z["traj_lens"])]
    opt = O.ExpSga(lr=O.linear_decay(0.2))
    P = z["p_transition"]
    reward = M.irl_causal_horizon(P, np.identity(25), [], tjs, opt, O.Constant(1.0), g, T)
    assert 10 < opt.k < 20000 and np.isfinite(reward).all(), opt.k
    p0 = M.initial_probabilities_from_trajectories(25, tjs)
    e = M.feature_expectation_from_trajectories(np.identity(25), tjs)
    mdp = DeviceMDP.resident(P)
    m = BatchedCausalHorizon(mdp, e, p0, [], T, discount=g)
    got, steps = m.run(eps=1e-4)
    assert int(steps[0]) == opt.k and np.max(np.abs(got[0].cpu().numpy() - reward)) <= 1e-9, (int(steps[0]), opt.k)
    svf = M.compute_expected_causal_svf_horizon(P, p0, [], reward, g, T)
    pi = M.local_causal_action_probabilities_horizon(P, [], reward, g, T)
    want_pi = ops.soft_backward_horizon(mdp, reward, g, T)
    want, _, _ = ops.forward_svf_horizon(mdp, p0, want_pi)
    assert pi.shape == (T, 25, 4) and np.array_equal(pi, want_pi[0].cpu().numpy())
    assert np.array_equal(svf, want[0].cpu().numpy()) and abs(svf.sum() - (T + 1)) < 1e-12
    # a terminal list: absorbing states, as ops with the mask
    svf_t = M.compute_expected_causal_svf_horizon(P, p0, [24], reward, g, T)
    tm = ops.terminal_mask([24], 25, device=dev)
    want_t, _, _ = ops.forward_svf_horizon(mdp, p0, ops.soft_backward_horizon(mdp, reward, g, T, tm), tm)
    assert np.array_equal(svf_t, want_t[0].cpu().numpy()) and svf_t.sum() < T + 1
    with pytest.raises(Exception, match="horizon 0 outside"):
        ops.soft_backward_horizon(mdp, reward, g, 0)
