"""The finite-horizon passes on the device (needs an MI355X).

ops.backward_maxent_horizon / ops.forward_svf_horizon (csrc/horizon.hip)
against tests/horizon_twin.py, each case asserting its plan first:

* every entry of pi_t against the longdouble backward, and of svf and svf_t
  against the longdouble forward fed the device's own float64 pi_t (the passes
  are judged separately), elementwise under 16 x max(e_twin, e_floor) -- the
  project's rule, e_twin the float64 twin's own error on the same input; exact
  zeros exact, NaN patterns and status equal to the twin's; log_z0 (signed,
  cancelling) normwise under the same rule;
* bit for bit: fused against per sweep, the batch reversed, every instance of a
  per-instance-table launch alone, the device bounds-check build; sum svf =
  T + 1 without terminals;
* non-finite inputs; the batched driver and the drop-ins.

The measured ratios e_kernel / max(e_twin, e_floor) are printed per instance
(profiles/horizon.txt records one run).
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
from conftest import ORACLE_DIR, PKG_DIR, ROOT, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LD = np.longdouble
KEY = "IRLMX_FUSED_MAX_STATES"            # 0: every size per sweep
BATCH_KEY = "IRLMX_HORIZON_FUSED_BATCH"   # 1: several states per thread run fused at any batch
TESTS_DIR = os.path.join(ROOT, "tests")


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


def run_backward(mdp, reward, T, terminal):
    """(pi_t, log_z0, status) through the C ABI (ops.backward_maxent_horizon does not return the status)."""
    from irlmx import _lib, ops
    lib = _lib.load()
    B, S, A = mdp.batch, mdp.n_states, mdp.n_actions
    r = torch.as_tensor(np.array(reward, dtype=np.float64), device=mdp.device).reshape(B, S).contiguous()
    pi = torch.full((B, T, S, A), -7.0, dtype=torch.float64, device=mdp.device)
    lz = torch.full((B, S), -7.0, dtype=torch.float64, device=mdp.device)
    status = torch.full((B,), -7, dtype=torch.int32, device=mdp.device)
    ws, n = ops._workspace(mdp, _lib.OP_BACKWARD_HORIZON)
    _lib.check(lib.irlmx_backward_maxent_horizon(mdp.struct(), _lib.ptr(r), _lib.ptr(terminal), T, _lib.ptr(pi),
                                                 _lib.ptr(lz), _lib.ptr(status), _lib.ptr(ws), n,
                                                 _lib.stream_ptr(mdp.device)), "backward_maxent_horizon")
    return pi, lz, status


def terminal_of(c, mdp):
    from irlmx import ops
    return ops.terminal_mask(c.terminal, c.S, batch=mdp.batch, device=mdp.device) if c.terminal else None


def run_case(c, dev, tables=None, reward=None, pi_t=None):
    """Both passes of case c (of the instances ``tables``): numpy arrays pi, lz,
    bstatus, svf, marg, fstatus.  ``pi_t``: the forward's input instead of the
    backward's own result."""
    from irlmx import ops
    idx = list(range(c.B)) if tables is None else list(tables)
    mdp = c.device_model(dev, tables=tables)
    tm = terminal_of(c, mdp)
    r = (c.reward if reward is None else reward)[idx]
    pi, lz, bst = run_backward(mdp, r, c.T, tm)
    feed = pi if pi_t is None else torch.as_tensor(pi_t, device=dev)
    svf, sweeps, fst, marg = ops.forward_svf_horizon(mdp, c.p0[idx].copy(), feed, tm, return_marginals=True)
    assert sweeps.tolist() == [c.T] * len(idx)
    plain = ops.backward_maxent_horizon(mdp, r, c.T, tm)           # without log_z0: the same policy
    assert torch.equal(plain.view(torch.int64), pi.view(torch.int64))
    return {"pi": pi.cpu().numpy(), "lz": lz.cpu().numpy(), "bstatus": bst.cpu().numpy(), "svf": svf.cpu().numpy(),
            "marg": marg.cpu().numpy(), "fstatus": fst.cpu().numpy()}


def assert_plan(c, dev, mode="default"):
    """The plan of both passes: fused with the case's states per thread -- by
    default only at one state per thread (the cases' batches are far below one
    workgroup per CU), under env("fused") wherever the case names a pair."""
    from irlmx import _lib, ops
    mdp = c.device_model(dev)
    pb, pf = ops.execution_plan(mdp, "backward_horizon"), ops.execution_plan(mdp, "forward_horizon")
    assert pb == ops.execution_plan(mdp, _lib.OP_BACKWARD_HORIZON)

    def fused(spt):
        return spt is not None and (mode == "fused" or (mode == "default" and spt == 1))

    for p, spt, lds in ((pb, None if c.bwd is None else c.bwd[0], 24), (pf, c.fwd, 16)):
        if not fused(spt):
            assert (p["shape"], p["spt"], p["threads"], p["launches"], p["lds_bytes"]) == ("sweep", 1, 256, 0, 0), p
        else:
            assert p["shape"] == "fused" and p["spt"] == spt and p["launches"] == 1, (c.name, p)
            assert p["lds_bytes"] == lds * c.S and p["spt"] * p["threads"] >= c.S, (c.name, p)
            per = -(-c.S // spt)
            assert p["threads"] == min(1024, -(-per // 64) * 64), (c.name, p)


_results = {}


def results(name, dev):
    """The default-plan run of a case, computed once."""
    if name not in _results:
        c = H.case(name)
        assert_plan(c, dev)
        _results[name] = run_case(c, dev)
    return _results[name]


def same(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        same_bits = np.array_equal(x.view(np.int64), y.view(np.int64)) if x.dtype == np.float64 else np.array_equal(x, y)
        assert same_bits, f"{what}: {k} differs"


def ratio(e, e_twin, k, a):
    return e / max(e_twin, X.e_floor(k, a))


@pytest.mark.parametrize("name", H.CASES)
def test_accuracy(dev, env, name):
    """pi_t, log_z0, svf and svf_t of every instance under 16 x max(e_twin,
    e_floor); status, exact zeros and NaN patterns as the twin's.  Measured
    ratios (one MI355X): profiles/horizon.txt; the largest is below 2."""
    c = H.case(name)
    got = results(name, dev)
    for b in range(c.B):
        rpi, rlz = c.ref_backward(b)
        e_twin_pi, e_twin_lz = c.e_twin_backward(b)
        e_pi = X.elementwise_err(got["pi"][b], rpi)
        e_lz = X.normwise_err(got["lz"][b], rlz)
        pi_dev = got["pi"][b]
        tD, tmarg, tstatus = H.forward(c.model(b), c.p0[b], c.terminal, pi_dev)
        rD, rmarg = H.forward_ref(c.model(b).mats, c.p0[b], c.terminal, pi_dev)
        e_twin_svf, e_twin_marg = X.elementwise_err(tD, rD), X.elementwise_err(tmarg, rmarg)
        e_svf, e_marg = X.elementwise_err(got["svf"][b], rD), X.elementwise_err(got["marg"][b], rmarg)
        print(f"[horizon] {name}[{b}] T {c.T} ratio pi {ratio(e_pi, e_twin_pi, c.K, c.A):.2f} "
              f"log_z0 {ratio(e_lz, e_twin_lz, c.K, c.A):.2f} svf {ratio(e_svf, e_twin_svf, c.Kc, c.A):.2f} "
              f"svf_t {ratio(e_marg, e_twin_marg, c.Kc, c.A):.2f} | e_kernel pi {e_pi:.2e} log_z0 {e_lz:.2e} "
              f"svf {e_svf:.2e} svf_t {e_marg:.2e} | e_twin pi {e_twin_pi:.2e} svf {e_twin_svf:.2e}")
        assert e_pi <= c.bound_pi(e_twin_pi), (name, b, e_pi, c.bound_pi(e_twin_pi))
        assert e_lz <= c.bound_pi(e_twin_lz), (name, b, e_lz, c.bound_pi(e_twin_lz))
        assert e_svf <= c.bound_svf(e_twin_svf), (name, b, e_svf, c.bound_svf(e_twin_svf))
        assert e_marg <= c.bound_svf(e_twin_marg), (name, b, e_marg, c.bound_svf(e_twin_marg))
        assert got["bstatus"][b] == H.OK and got["fstatus"][b] == tstatus == H.OK
        assert np.array_equal(np.isnan(got["pi"][b]), np.isnan(c.twin_backward(b)[0]))
        assert np.array_equal(got["marg"][b][0].view(np.int64), c.p0[b].view(np.int64))      # d_0 = p0
        if name.startswith("wide"):
            assert H.nan_rows(got["pi"][b]) == 0 and np.isfinite(got["lz"][b]).all()
        if c.T == 1:                                                                          # svf = p0 + d_1
            assert np.array_equal(got["svf"][b], c.p0[b] + got["marg"][b][1])
        if not c.terminal:
            tol = (c.T + 1) * (c.Kc + c.A + 2) * 2.0 ** -53                                   # include/irlmx.h
            assert abs(float(got["svf"][b].astype(LD).sum()) - (c.T + 1)) <= tol * (c.T + 1), name
    if c.ell is not None:
        import ell_cases as E
        for b, named in enumerate(E.case(c.ell).named):
            if named["empty"] is not None:            # an action with an empty row: an exact 0 at every step
                s, a = named["empty"]
                assert (got["pi"][b][:, s, a] == 0).all() and np.isfinite(got["pi"][b][:, s]).all()


@pytest.mark.parametrize("name", H.FUSED)
def test_fused_equals_sweep(dev, env, name):
    """Every fused instantiation -- those with several states per thread forced
    below their batch threshold -- and the per-sweep shape: the same bits."""
    c = H.case(name)
    default = results(name, dev)
    for mode in ("fused", "sweep"):
        env(mode)
        assert_plan(c, dev, mode)
        same(run_case(c, dev), default, f"{name} {mode}")


@pytest.mark.parametrize("name", ["16x16", "k5-s200", "128x40"])
def test_batch_order_and_instances_alone(dev, env, name):
    """Per-instance tables: the batch reversed gives reversed results, and every
    instance equals its table run alone."""
    c = H.case(name)
    whole = results(name, dev)
    order = list(range(c.B))[::-1]
    same(run_case(c, dev, tables=order), {k: v[order] for k, v in whole.items()}, name + " reversed")
    for b in range(c.B):
        same(run_case(c, dev, tables=[b]), {k: v[[b]] for k, v in whole.items()}, f"{name}[{b}] alone")


@pytest.mark.parametrize("mode", ["fused", "sweep"])
def test_nan_reward_poisons_its_instance_only(dev, env, mode):
    c = H.case("16x16")
    clean = results("16x16", dev)
    env(mode)
    r = c.reward.copy()
    r[1, 77] = np.nan
    got = run_case(c, dev, reward=r)
    assert np.isnan(got["pi"][1]).all() and np.isnan(got["lz"][1]).all()
    assert list(got["bstatus"]) == [H.OK] * 3                     # as the extended backward
    tpi, tlz = H.backward(c.model(1), c.terminal, r[1], c.T)
    assert np.isnan(tpi).all() and np.isnan(tlz).all()
    assert list(got["fstatus"]) == [H.OK, H.NONFINITE, H.OK]      # the forward, fed the NaN policy
    for b in (0, 2):
        same({k: v[[b]] for k, v in got.items()}, {k: v[[b]] for k, v in clean.items()}, f"instance {b}")


@pytest.mark.parametrize("name", ["16x16", "k5-s200"])
@pytest.mark.parametrize("mode", ["fused", "sweep"])
def test_nan_planted_in_one_policy_row(dev, env, name, mode):
    """A NaN row in pi_3 of instance 1: NaN spreads by IEEE rules from step 3
    on, in the slot order of the column form -- the twin's pattern exactly, in
    svf and in every marginal; status NONFINITE for that instance alone."""
    c = H.case(name)
    clean = results(name, dev)
    env(mode)
    pi = clean["pi"].copy()
    s = 40
    pi[1, 3, s, :] = np.nan
    got = run_case(c, dev, pi_t=pi)
    assert list(got["fstatus"]) == [H.OK, H.NONFINITE] + [H.OK] * (c.B - 2)
    tD, tmarg, tstatus = H.forward(c.model(1), c.p0[1], c.terminal, pi[1])
    assert tstatus == H.NONFINITE
    assert np.array_equal(np.isnan(got["svf"][1]), np.isnan(tD)) and np.isnan(tD).any()
    assert np.array_equal(np.isnan(got["marg"][1]), np.isnan(tmarg)) and not np.isnan(tmarg[:4]).any()
    assert np.isnan(tmarg[4]).any() and not np.isnan(tmarg[4]).all()      # the successors of s, one step later
    for b in set(range(c.B)) - {1}:
        for k in ("svf", "marg", "fstatus"):
            assert np.array_equal(got[k][b], clean[k][b]), (b, k)


CHECKS = textwrap.dedent("""
    import json, os, sys
    sys.path[:0] = [{root!r}, {pkg!r}, {oracle!r}, {tests!r}]
    import numpy as np
    import __graft_entry__ as g
    g.build()
    import irlmx
    from irlmx import _lib, ops
    import horizon_twin as H
    import test_gpu_horizon as G
    dev = irlmx.require_device()
    out = {{"enabled": int(_lib.load().irlmx_device_checks_enabled()), "fails": []}}
    arrays = {{}}
    for sweep in (0, 1):
        os.environ[G.BATCH_KEY] = "1"
        if sweep:
            os.environ[G.KEY] = "0"
        for name in {names!r}:
            got = G.run_case(H.case(name), dev)
            out["fails"].append(ops.device_check_failures())
            for k, v in got.items():
                arrays[f"{{name}}.{{sweep}}.{{k}}"] = v
    np.savez({npz!r}, **arrays)
    json.dump(out, open({out!r}, "w"))
""")


def test_device_check_build(dev, env, tmp_path):
    """ELL and stencil cases under libirlmx_checks.so, fused and per sweep: no
    check bit set and the same bits as the product build."""
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
        for sweep in (0, 1):
            same({k: z[f"{name}.{sweep}.{k}"] for k in results(name, dev)}, results(name, dev), f"{name} checks {sweep}")


# ---------------------------------------------------------------------------
# the batched driver
# ---------------------------------------------------------------------------

DRIVER_T = 12


def driver_world(dev):
    from irlmx import DeviceMDP
    return DeviceMDP.icy_gridworld(12, [0.2, 0.1, 0.3], device=dev)


_demos = {}


def demonstrations(dev):
    """Rollouts of DRIVER_T steps without a terminal state under the policy of a
    planted reward: (mdp, states, lengths), computed once."""
    if not _demos:
        from irlmx import _lib, ops
        mdp = driver_world(dev)
        S = mdp.n_states
        theta = np.random.default_rng(3).uniform(0.2, 1.2, (3, S))
        pi = ops.backward_maxent_horizon(mdp, theta, DRIVER_T)
        none = torch.zeros((3, S), dtype=torch.uint8, device=dev)
        ro = ops.rollout(mdp, pi[:, 0].contiguous(), none, [5, 70, 130], 64, DRIVER_T, seed=11,
                         return_trajectories=True)
        assert (ro.status == _lib.TRAJ_TRUNCATED).all() and (ro.lengths == DRIVER_T).all()
        _demos["v"] = (mdp, ro.states, ro.lengths)
    return _demos["v"]


def driver(dev, **kw):
    from irlmx.batch import BatchedMaxEnt
    mdp, states, lengths = demonstrations(dev)
    return BatchedMaxEnt.from_trajectories(mdp, states, lengths, [], horizon=DRIVER_T, **kw)


def test_driver_step_is_the_three_ops(dev, env):
    from irlmx import ops
    m = driver(dev)
    assert float(m.e_features.sum(dim=1).max()) == DRIVER_T + 1 == float(m.e_features.sum(dim=1).min())
    theta0 = m.theta.clone()
    pi = ops.backward_maxent_horizon(m.mdp, theta0, DRIVER_T)
    svf, sweeps, _ = ops.forward_svf_horizon(m.mdp, m.p_initial, pi)
    want = m.optimizer.apply(theta0, m.e_features - svf, 0)
    assert tuple(m.backward().shape) == (3, DRIVER_T, m.mdp.n_states, 4)
    got_svf = m.step()
    assert torch.equal(got_svf, svf) and torch.equal(m.theta, want)
    assert m.last_forward_sweeps.tolist() == [DRIVER_T] * 3
    with pytest.raises(NotImplementedError, match="time-indexed"):
        m.log_likelihood(None, None, None)
    with pytest.raises(NotImplementedError, match="time-indexed"):
        m.expected_value_difference(theta0, 0.9)
    from irlmx.batch import BatchedMaxEnt
    with pytest.raises(ValueError, match="non-causal"):
        BatchedMaxEnt(m.mdp, m.e_features, m.p_initial, [], horizon=DRIVER_T, causal=True, discount=0.9)
    ext = driver(dev, extended_range=True)           # ignored: the pass is always per state
    assert torch.equal(ext.step(), svf)


def test_driver_planted_statistics_and_compaction(dev, env):
    """With e_features = the device's own D(theta*), the first gradient is
    exactly 0 and theta stays theta*.  Planted in instance 0 alone, that
    instance stops after one step, so a compacted run works on fewer instances
    from step 2 on -- and ends with the same theta and steps as the uncompacted one."""
    from irlmx import ops
    ref = driver(dev)
    star = torch.as_tensor(np.random.default_rng(4).uniform(0.3, 1.1, tuple(ref.theta.shape)), device=dev)
    D, _, _ = ops.forward_svf_horizon(ref.mdp, ref.p_initial, ops.backward_maxent_horizon(ref.mdp, star, DRIVER_T))
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


def test_driver_gradient_shrinks_on_gridworld(dev, env):
    """The deterministic GridWorld, statistics planted from theta*, started at
    theta0 = 1: max|grad| after 20 steps is below its value at step 1 -- on the
    CPU twin first (the condition on theta*, T and the step count), then on the
    device."""
    from irlmx import DeviceMDP, ops
    from irlmx.batch import BatchedMaxEnt
    from irlmx.optim import ExpSga, linear_decay
    from test_horizon_twin import deterministic_grid
    size, T, steps = 5, 8, 20
    S = size * size
    star = np.random.default_rng(8).uniform(0.2, 1.5, S)
    p0 = np.full(S, 1.0 / S)
    mod = H.stencil_model(deterministic_grid(size, size), size, size)

    def twin_D(theta):
        return H.forward(mod, p0, [], H.backward(mod, [], theta, T)[0])[0]

    e = twin_D(star)
    theta, opt, grads = torch.ones(1, S, dtype=torch.float64), ExpSga(linear_decay(0.2)), []
    for k in range(steps + 1):
        g = torch.as_tensor(e - twin_D(theta[0].numpy())).unsqueeze(0)
        grads.append(float(g.abs().max()))
        theta = opt.apply(theta, g, k)
    assert grads[-1] < 0.5 * grads[0], grads                       # the twin: the inputs are fit for the test

    mdp = DeviceMDP.gridworld(size, device=dev)
    D_star, _, _ = ops.forward_svf_horizon(mdp, p0, ops.backward_maxent_horizon(mdp, star, T))
    m = BatchedMaxEnt(mdp, D_star, p0, [], horizon=T)
    got = []
    for _ in range(steps + 1):
        svf, _, _ = m.forward(m.backward())
        got.append(float(m.update(svf).abs().max()))
    assert got[-1] < got[0], got
    assert abs(got[0] - grads[0]) <= 1e-9 * grads[0]                # the same problem as the twin's


# ---------------------------------------------------------------------------
# the drop-ins
# ---------------------------------------------------------------------------

def test_dropins_on_config1(dev, env):
    """maxent.irl_horizon on BASELINE config 1's 5 x 5 world without a terminal
    state, its demonstrations cut after 10 steps: runs to its stopping rule
    (the CPU twin takes 959 steps), and the drop-ins equal ops bit for bit."""
    import maxent as M
    import maxent_oracle as O
    from conftest import unpack_trajectories
    from irlmx import DeviceMDP, ops
    z = load_golden("config1")
    T = 10
    tjs = [O.Trajectory(t.transitions()[:T]) for t in unpack_trajectories(z["traj_flat"], z["traj_lens"])]
    opt = O.ExpSga(lr=O.linear_decay(0.2))
    P = z["p_transition"]
    reward = M.irl_horizon(P, np.identity(25), [], tjs, opt, O.Constant(1.0), T)
    assert 100 < opt.k < 5000 and np.isfinite(reward).all(), opt.k
    p0 = M.initial_probabilities_from_trajectories(25, tjs)
    svf = M.compute_expected_svf_horizon(P, p0, [], reward, T)
    pi = M.local_action_probabilities_horizon(P, [], reward, T)
    mdp = DeviceMDP.resident(P)
    want_pi = ops.backward_maxent_horizon(mdp, reward, T)
    want, _, _ = ops.forward_svf_horizon(mdp, p0, want_pi)
    assert pi.shape == (T, 25, 4) and np.array_equal(pi, want_pi[0].cpu().numpy())
    assert np.array_equal(svf, want[0].cpu().numpy()) and abs(svf.sum() - (T + 1)) < 1e-12
    # a terminal list: absorbing states, as ops with the mask
    svf_t = M.compute_expected_svf_horizon(P, p0, [24], reward, T)
    tm = ops.terminal_mask([24], 25, device=dev)
    want_t, _, _ = ops.forward_svf_horizon(mdp, p0, ops.backward_maxent_horizon(mdp, reward, T, tm), tm)
    assert np.array_equal(svf_t, want_t[0].cpu().numpy()) and svf_t.sum() < T + 1
