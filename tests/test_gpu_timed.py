"""The calls on time-indexed policies on the device (needs an MI355X):
ops.rollout_horizon, ops.demo_log_likelihood_horizon, ops.value_horizon and
ops.expected_value_difference_horizon (include/irlmx_timed.h; csrc/rollout.hip, csrc/soft_horizon.hip)
against tests/timed_twin.py on tests/horizon_twin.py's cases, and the three
driver methods built on them.

* Rollouts and log-likelihoods equal the numpy twin bit for bit (integer
  counts, adds and one product per draw: no fused multiply-add to differ in),
  equal ops.rollout / ops.demo_log_likelihood under a stationary policy
  repeated T times, and are checked against two truths: exact visit counts on
  the deterministic GridWorld, and Hoeffding's bound on 20,000 trajectories.
* The value pass is measured normwise against the longdouble restatement under
  16 x max(e_twin, e_floor), bit for bit across its shapes, and against the
  forward pass through the duality p0 . v_0 = svf . r.

The measured figures are printed per case (profiles/timed_accuracy.txt records one run).
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
import rollout_twin as R
import test_timed_twin as TW
import timed_twin as TT
from conftest import ORACLE_DIR, PKG_DIR, ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LD = np.longdouble
KEY = "IRLMX_FUSED_MAX_STATES"            # 0: every size per sweep
BATCH_KEY = "IRLMX_HORIZON_FUSED_BATCH"   # 1: several states per thread run fused at any batch
TESTS_DIR = os.path.join(ROOT, "tests")
SEED = 4242


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    import irlmx
    return irlmx.require_device()


@pytest.fixture
def env(monkeypatch):
    """``env("sweep")``: every size per sweep; ``env("fused")``: the fused shape wherever a kernel is
    instantiated, also with several states per thread below the planner's batch; cleared afterwards."""
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


def mask(c, mdp):
    from irlmx import ops
    return ops.terminal_mask(c.terminal, c.S, batch=mdp.batch, device=mdp.device) if c.terminal else None


_policies = {}


def policies(name, dev):
    """The device's own pi_t of a case on its default plan, as numpy [B, T, S, A]: the non-causal pass's and the
    causal pass's at discount 1; computed once."""
    if name not in _policies:
        from irlmx import ops
        c = TT.case(name)
        mdp = c.device_model(dev)
        tm = mask(c, mdp)
        _policies[name] = {
            "noncausal": ops.backward_maxent_horizon(mdp, np.array(c.reward), c.T, tm).cpu().numpy(),
            "causal": ops.soft_backward_horizon(mdp, np.array(c.reward), 1.0, c.T, tm).cpu().numpy(),
            "optimal": None}
    return _policies[name]


def bits(x):
    return x.view(np.int64) if x.dtype == np.float64 else x


def same(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        if x is None or y is None:
            assert x is y, (what, k)
            continue
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        assert np.array_equal(bits(x), bits(y)), f"{what}: {k} differs"


# ---------------------------------------------------------------------------
# rollouts and their log-likelihood
# ---------------------------------------------------------------------------

#: case -> trajectories per instance (16x16: B * N = 900 crosses workgroups and instances)
ROLL = {"16x16": 300, "k5-s200": 40, "37x23": 60, "16x16-T1": 40}


def starts_of(c, N):
    st = np.random.default_rng(77).integers(0, c.S, (c.B, N))
    if c.terminal:
        st[:, 3] = c.terminal[0]          # a terminal start state: length 0, status OK
    return st


def as_np(out):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out._asdict().items()}


def roll_device(c, dev, pi, N, tables=None, trajectories=True, start=None):
    from irlmx import ops
    idx = list(range(c.B)) if tables is None else list(tables)
    mdp = c.device_model(dev, tables=tables)
    st = (starts_of(c, N) if start is None else start)[idx]
    seeds = [R.instance_seeds(SEED, c.B)[b] for b in idx]
    out = ops.rollout_horizon(mdp, pi[idx], st, N, seeds, terminal=mask(c, mdp), return_trajectories=trajectories)
    return as_np(out)


def roll_twin(c, pi, N, start=None):
    st = starts_of(c, N) if start is None else start
    tm = H._mask(c.terminal, c.S) if c.terminal else None
    per = [TT.rollout(c.model(b).nbr, c.model(b).rv, pi[b], tm, st[b], R.instance_seeds(SEED, c.B)[b]) for b in range(c.B)]
    out = {k: np.stack([p[k] for p in per]) for k in per[0]}
    return out


@pytest.mark.parametrize("kind", ["noncausal", "causal"])
@pytest.mark.parametrize("name", list(ROLL))
def test_rollout_and_log_likelihood_match_the_twin(dev, env, name, kind):
    """Status, lengths, states, actions, visits and starts, then ll_traj, ll and
    the status of the log-likelihood on those trajectories: the twin's bits."""
    from irlmx import _lib, ops
    c, N = H.case(name), ROLL[name]
    pi = policies(name, dev)[kind]
    got, want = roll_device(c, dev, pi, N), roll_twin(c, pi, N)
    same(got, want, f"{name} {kind} rollout")
    if not c.terminal:
        assert (got["status"] == _lib.TRAJ_TRUNCATED).all() and (got["lengths"] == c.T).all()
        assert (got["visits"].sum(axis=1) == N * (c.T + 1)).all()
    else:
        assert {_lib.TRAJ_OK, _lib.TRAJ_TRUNCATED} <= set(got["status"].ravel().tolist())
    same(roll_device(c, dev, pi, N, trajectories=False),
         {**want, "states": None, "actions": None}, f"{name} {kind} rollout without stored trajectories")
    ll, ll_traj, st = ops.demo_log_likelihood_horizon(pi, got["states"], got["actions"], got["lengths"])
    tw = [TT.log_likelihood(pi[b], want["states"][b], want["actions"][b], want["lengths"][b]) for b in range(c.B)]
    same({"ll": ll.cpu().numpy(), "ll_traj": ll_traj.cpu().numpy(), "status": st.cpu().numpy()},
         {"ll": np.array([t[0] for t in tw]), "ll_traj": np.stack([t[1] for t in tw]), "status": np.stack([t[2] for t in tw])},
         f"{name} {kind} log-likelihood")
    assert (st == _lib.TRAJ_OK).all() and np.isfinite(ll.cpu().numpy()).all()


@pytest.mark.parametrize("name", ["16x16", "37x23"])
def test_tiled_stationary_policy_is_the_stationary_call(dev, env, name):
    from irlmx import ops
    c, N = H.case(name), 64
    mdp = c.device_model(dev)
    pi0 = np.ascontiguousarray(policies(name, dev)["causal"][:, 0])
    tiled = np.ascontiguousarray(np.broadcast_to(pi0[:, None], (c.B, c.T) + pi0.shape[1:]))
    st = starts_of(c, N)
    tm = mask(c, mdp)
    zeros = torch.zeros((c.B, c.S), dtype=torch.uint8, device=dev)
    want = ops.rollout(mdp, pi0, tm if tm is not None else zeros, st, N, c.T, SEED, return_trajectories=True)
    got = ops.rollout_horizon(mdp, tiled, st, N, SEED, terminal=tm, return_trajectories=True)
    same(as_np(got), as_np(want), f"{name} tiled rollout")
    a = ops.demo_log_likelihood_horizon(tiled, got.states, got.actions, got.lengths)
    b = ops.demo_log_likelihood(pi0, want.states, want.actions, want.lengths)
    same({str(i): t.cpu().numpy() for i, t in enumerate(a)}, {str(i): t.cpu().numpy() for i, t in enumerate(b)},
         f"{name} tiled log-likelihood")


def test_rollout_instances_alone_and_batch_reversed(dev, env):
    c, N = H.case("16x16"), ROLL["16x16"]
    pi = policies("16x16", dev)["noncausal"]
    whole = roll_device(c, dev, pi, N)
    order = list(range(c.B))[::-1]
    same(roll_device(c, dev, pi, N, tables=order), {k: v[order] for k, v in whole.items()}, "reversed")
    for b in range(c.B):
        same(roll_device(c, dev, pi, N, tables=[b]), {k: v[[b]] for k, v in whole.items()}, f"instance {b} alone")


def test_nan_row_at_step_five(dev, env):
    """NaN in pi_t[1][5][s][:] for every third state: BAD_POLICY to exactly the
    trajectories of instance 1 the twin names, each at length 5, none earlier."""
    from irlmx import _lib
    c, N = H.case("16x16"), ROLL["16x16"]
    pi = policies("16x16", dev)["noncausal"].copy()
    pi[1, 5, ::3, :] = np.nan
    got, want = roll_device(c, dev, pi, N), roll_twin(c, pi, N)
    same(got, want, "NaN row")
    bad = got["status"] == _lib.TRAJ_BAD_POLICY
    assert bad[1].sum() > N // 6 and not bad[0].any() and not bad[2].any()
    assert (got["lengths"][bad] == 5).all() and (got["states"][bad][:, 5] % 3 == 0).all()
    assert (got["status"][~bad] == _lib.TRAJ_TRUNCATED).all()


def one_hot_policy(S, A, T, seed):
    a = np.random.default_rng(seed).integers(0, A, (T, S))
    pi = np.zeros((T, S, A))
    pi[np.arange(T)[:, None], np.arange(S)[None, :], a] = 1.0
    return pi


def test_exact_visits_on_the_deterministic_gridworld(dev, env):
    """DeviceMDP.gridworld(9), a one-hot time-indexed policy, T = 12, N = 64 with
    start masses 1/2, 1/4, 1/4: every trajectory is its start state's one path,
    so visits == N * svf of ops.forward_svf_horizon, exactly."""
    from irlmx import DeviceMDP, ops
    size, T, N = 9, 12, 64
    S = size * size
    mdp = DeviceMDP.gridworld(size, device=dev)
    pi = one_hot_policy(S, 4, T, 3)[None]
    start = np.array([[4] * 32 + [40] * 16 + [77] * 16])
    out = ops.rollout_horizon(mdp, pi, start, N, 9)
    p0 = out.starts.to(torch.float64) / N
    assert sorted(p0[0][p0[0] > 0].tolist()) == [0.25, 0.25, 0.5]
    svf, _, _ = ops.forward_svf_horizon(mdp, p0, pi)
    want = svf[0].cpu().numpy() * N
    assert np.array_equal(want, np.round(want)) and want.sum() == N * (T + 1)
    assert np.array_equal(out.visits[0].cpu().numpy(), want.astype(np.int64))


def test_visit_frequencies_within_hoeffding(dev, env):
    """16x16, N = 20,000, the CPU twin's non-causal pi_t uploaded as it is: the
    device draws the twin's trajectories bit for bit (tests/test_timed_twin.py
    decides the seed there), and max_s |visits / N - svf(s)| <= (T + 1)
    sqrt(ln(2 S / 1e-9) / (2 N)) with svf of ops.forward_svf_horizon."""
    from irlmx import ops
    c, pi, start = TW.statistical_input()
    N = TW.STAT_N
    twin = TT.rollout(c.model(0).nbr, c.model(0).rv, pi, None, start, R.instance_seeds(TW.STAT_SEED, 1)[0])
    mdp = c.device_model(dev, tables=[0])
    pi_b = np.array(pi[None])                      # (the twin's array is frozen)
    out = ops.rollout_horizon(mdp, pi_b, start[None], N, TW.STAT_SEED)
    assert np.array_equal(out.visits[0].cpu().numpy(), twin["visits"]) and np.array_equal(out.lengths[0].cpu().numpy(), twin["lengths"])
    p0 = out.starts.to(torch.float64) / N
    assert np.array_equal(p0[0].cpu().numpy(), c.p0[0])
    svf, _, _ = ops.forward_svf_horizon(mdp, p0, pi_b)
    dev_max = float((out.visits[0].to(torch.float64) / N - svf[0]).abs().max())
    bound = TW.hoeffding(c.T, c.S, N)
    print(f"[timed] statistical: max |visits / N - svf| {dev_max:.4f}, bound {bound:.4f}")
    assert dev_max <= bound


def test_bad_stored_trajectories_and_zero_probability(dev, env):
    """A length of T + 1, a state at S and an action at A: code 4 and NaN for that
    trajectory only; an action of probability 0: -inf."""
    from irlmx import _lib, ops
    c, N = H.case("16x16"), 16
    pi = policies("16x16", dev)["causal"].copy()
    got = roll_device(c, dev, pi, N)
    T = c.T
    states = np.concatenate([got["states"], got["states"][:, :, -1:]], axis=2)       # stride T + 2: a length of T + 1 fits the row
    actions = np.concatenate([got["actions"], got["actions"][:, :, -1:]], axis=2)
    lengths = got["lengths"].copy()
    lengths[0, 2] = T + 1
    states[1, 4, 7] = c.S
    actions[2, 6, 0] = c.A
    pi[0, 3, states[0, 9, 3], actions[0, 9, 3]] = 0.0
    ll, ll_traj, st = (t.cpu().numpy() for t in ops.demo_log_likelihood_horizon(pi, states, actions, lengths))
    tw = [TT.log_likelihood(pi[b], states[b], actions[b], lengths[b]) for b in range(c.B)]
    same({"ll": ll, "ll_traj": ll_traj, "status": st},
         {"ll": np.array([t[0] for t in tw]), "ll_traj": np.stack([t[1] for t in tw]), "status": np.stack([t[2] for t in tw])},
         "bad trajectories")
    bad = np.zeros((c.B, N), bool)
    bad[0, 2] = bad[1, 4] = bad[2, 6] = True
    assert np.array_equal(st == _lib.TRAJ_BAD_INDEX, bad) and (st[~bad] == _lib.TRAJ_OK).all()
    assert np.array_equal(np.isnan(ll_traj), bad) and np.isnan(ll).all()
    assert ll_traj[0, 9] == -np.inf and np.isfinite(np.delete(ll_traj[0], [2, 9])).all()


def test_telescoping_on_the_deterministic_gridworld(dev, env):
    """Full-length trajectories on DeviceMDP.gridworld(12) under the non-causal
    pi_t: ll_traj = sum_{t<=T} r(s_t) - log_z0(s_0) within the header's
    first-order bound (tests/timed_twin.py telescoping_bound; the twin is held
    to the same bound without a device).  Measured on one MI355X: worst error
    8.66e-15, 0.094 of the bound."""
    from irlmx import DeviceMDP, ops
    mod, reward, start = TW.telescoping_input()
    mdp = DeviceMDP.gridworld(TW.TELE_SIZE, device=dev)
    P = mdp.to_dense()
    for a, m in enumerate(mod.mats):
        assert np.array_equal(P[:, :, a], m.toarray())
    pi, lz = ops.backward_maxent_horizon(mdp, reward, TW.TELE_T, return_log_z0=True)
    out = ops.rollout_horizon(mdp, pi, start[None], TW.TELE_N, TW.TELE_SEED, return_trajectories=True)
    assert (out.lengths == TW.TELE_T).all()
    _, ll_traj, _ = ops.demo_log_likelihood_horizon(pi, out.states, out.actions, out.lengths)
    ratio, err = TW.telescoping_check(mod, reward, pi[0].cpu().numpy(), lz[0].cpu().numpy(), out.states[0].cpu().numpy(),
                                      out.actions[0].cpu().numpy(), ll_traj[0].cpu().numpy())
    print(f"[timed] telescoping: worst error {err:.2e}, worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


# ---------------------------------------------------------------------------
# the value pass
# ---------------------------------------------------------------------------

def run_value(mdp, reward, T, pi, discount, terminal, values=True):
    """(value0, value_t, status) through the C ABI, the outputs prefilled (ops.value_horizon takes torch.empty)."""
    from irlmx import _lib, ops
    lib = _lib.load()
    B, S, A = mdp.batch, mdp.n_states, mdp.n_actions
    r = torch.as_tensor(np.array(reward, dtype=np.float64), device=mdp.device).reshape(B, S).contiguous()
    p = None if pi is None else torch.as_tensor(np.array(pi), device=mdp.device).reshape(B, T, S, A).contiguous()
    v0 = torch.full((B, S), -7.0, dtype=torch.float64, device=mdp.device)
    vt = torch.full((B, T + 1, S), -7.0, dtype=torch.float64, device=mdp.device) if values else None
    status = torch.full((B,), -7, dtype=torch.int32, device=mdp.device)
    ws, n = ops._workspace(mdp, _lib.OP_VALUE_HORIZON)
    _lib.check(lib.irlmx_value_horizon(mdp.struct(), _lib.ptr(r), _lib.ptr(terminal), _lib.ptr(p), float(discount), T,
                                       _lib.ptr(v0), _lib.ptr(vt), _lib.ptr(status), _lib.ptr(ws), n,
                                       _lib.stream_ptr(mdp.device)), "value_horizon")
    return v0, vt, status


def run_case(c, dev, discount, tables=None, reward=None):
    """The three policies of case c (of the instances ``tables``): kind -> {"v0", "vt", "status"} as numpy."""
    from irlmx import ops
    idx = list(range(c.B)) if tables is None else list(tables)
    mdp = c.device_model(dev, tables=tables)
    tm = mask(c, mdp)
    r = (c.reward if reward is None else reward)[idx]
    out = {}
    for kind, pi in policies(c.name, dev).items():
        p = None if pi is None else pi[idx]
        v0, vt, st = run_value(mdp, r, c.T, p, discount, tm)
        plain, pst = ops.value_horizon(mdp, r, c.T, p, discount, tm)          # without value_t: the same value
        assert torch.equal(plain.view(torch.int64), v0.view(torch.int64)) and torch.equal(pst, st)
        out[kind] = {"v0": v0.cpu().numpy(), "vt": vt.cpu().numpy(), "status": st.cpu().numpy()}
    return out


def assert_plan(c, dev, mode="default"):
    """test_gpu_soft_horizon.assert_plan for "value_horizon": the same shapes, 16 * S bytes of LDS when fused."""
    from irlmx import _lib, ops
    mdp = c.device_model(dev)
    p = ops.execution_plan(mdp, "value_horizon")
    assert p == ops.execution_plan(mdp, _lib.OP_VALUE_HORIZON)
    spt = None if c.bwd is None else c.bwd[0]
    if spt is not None and (mode == "fused" or (mode == "default" and spt == 1)):
        assert p["shape"] == "fused" and p["spt"] == spt and p["launches"] == 1, (c.name, p)
        assert p["lds_bytes"] == 16 * c.S and p["spt"] * p["threads"] >= c.S, (c.name, p)
        per = -(-c.S // spt)
        assert p["threads"] == min(1024, -(-per // 64) * 64), (c.name, p)
        soft = ops.execution_plan(mdp, "soft_backward_horizon")
        assert {**soft, "lds_bytes": p["lds_bytes"]} == p, (soft, p)
    else:
        assert (p["shape"], p["spt"], p["threads"], p["launches"], p["lds_bytes"]) == ("sweep", 1, 256, 0, 0), p


_results = {}


def results(name, discount, dev):
    """The default-plan run of a case, computed once."""
    if (name, discount) not in _results:
        c = TT.case(name)
        assert_plan(c, dev)
        _results[name, discount] = run_case(c, dev, discount)
    return _results[name, discount]


def same_runs(a, b, what):
    for kind in a:
        same(a[kind], b[kind], f"{what} {kind}")


def take(run, idx):
    return {kind: {k: v[idx] for k, v in d.items()} for kind, d in run.items()}


@pytest.mark.parametrize("discount", TT.DISCOUNTS)
@pytest.mark.parametrize("name", TT.CASES)
def test_value_accuracy(dev, env, name, discount):
    """value0 of every instance and policy normwise under 16 x max(e_twin, e_floor),
    e_twin the float64 twin's own error on the same pi_t; status as the twin's;
    value_t[:, 0] == value0 and value_t[:, T] == reward.  Measured ratios (one
    MI355X): profiles/timed_accuracy.txt."""
    c = TT.case(name)
    got = results(name, discount, dev)
    floor = X.e_floor(c.K, c.A)
    for kind, pi in policies(name, dev).items():
        g = got[kind]
        assert np.array_equal(bits(g["vt"][:, 0]), bits(g["v0"])) and np.array_equal(bits(g["vt"][:, c.T]), bits(np.array(c.reward)))
        for b in range(c.B):
            p = None if pi is None else pi[b]
            tv0, _, tstatus = TT.value(c.model(b), c.terminal, c.reward[b], discount, c.T, p)
            ref = TT.value_ref(c.model(b).mats, c.terminal, c.reward[b], discount, c.T, p)[0]
            e_t, e_k = X.normwise_err(tv0, ref), X.normwise_err(g["v0"][b], ref)
            print(f"[timed] {name}[{b}] {kind} g {discount} T {c.T} ratio {e_k / max(e_t, floor):.2f} | e_kernel {e_k:.2e} "
                  f"e_twin {e_t:.2e}")
            assert e_k <= X.bound(e_t, c.K, c.A), (name, b, kind, e_k, e_t)
            assert g["status"][b] == tstatus == TT.OK and np.isfinite(g["vt"][b]).all()
            if c.terminal:
                assert np.array_equal(g["vt"][b][:, c.terminal], np.tile(c.reward[b][c.terminal], (c.T + 1, 1)))


@pytest.mark.parametrize("discount", TT.DISCOUNTS)
@pytest.mark.parametrize("name", TT.FUSED)
def test_value_fused_equals_sweep(dev, env, name, discount):
    """Every fused instantiation -- those with several states per thread forced
    below their batch threshold -- and the per-sweep shape: the same bits."""
    c = TT.case(name)
    default = results(name, discount, dev)
    for mode in ("fused", "sweep"):
        env(mode)
        assert_plan(c, dev, mode)
        same_runs(run_case(c, dev, discount), default, f"{name} {mode}")


@pytest.mark.parametrize("name,discount", [("16x16", 1.0), ("16x16", 0.9), ("k5-s200", 0.9), ("128x40", 0.9)])
def test_value_batch_order_and_instances_alone(dev, env, name, discount):
    c = TT.case(name)
    whole = results(name, discount, dev)
    order = list(range(c.B))[::-1]
    same_runs(run_case(c, dev, discount, tables=order), take(whole, order), name + " reversed")
    for b in range(c.B):
        same_runs(run_case(c, dev, discount, tables=[b]), take(whole, [b]), f"{name}[{b}] alone")


@pytest.mark.parametrize("mode", ["fused", "sweep"])
def test_nan_reward_marks_its_instance_only(dev, env, mode):
    c = TT.case("16x16")
    env(mode)
    r = c.reward.copy()
    r[1, 77] = np.nan
    got = run_case(c, dev, 0.9, reward=r)
    for kind, pi in policies("16x16", dev).items():
        g = got[kind]
        assert list(g["status"]) == [TT.OK, TT.NONFINITE, TT.OK], kind
        tv0, tvt, tstatus = TT.value(c.model(1), c.terminal, r[1], 0.9, c.T, None if pi is None else pi[1])
        assert tstatus == TT.NONFINITE and np.isnan(tv0[77])
        assert np.array_equal(np.isnan(g["vt"][1]), np.isnan(tvt)), kind
    clean = run_case(c, dev, 0.9)
    for b in (0, 2):
        same_runs(take(got, [b]), take(clean, [b]), f"instance {b}")


CHECKS = textwrap.dedent("""
    import json, os, sys
    sys.path[:0] = [{root!r}, {pkg!r}, {oracle!r}, {tests!r}]
    import numpy as np
    import __graft_entry__ as g
    g.build()
    import irlmx
    from irlmx import _lib, ops
    import timed_twin as TT
    import test_gpu_timed as G
    dev = irlmx.require_device()
    out = {{"enabled": int(_lib.load().irlmx_device_checks_enabled()), "fails": []}}
    arrays = {{}}
    for name in {names!r}:                    # the policies: on the default plan, as the product build's
        G.policies(name, dev)
    for sweep in (0, 1):
        os.environ[G.BATCH_KEY] = "1"
        if sweep:
            os.environ[G.KEY] = "0"
        for name in {names!r}:
            c = TT.case(name)
            got = G.run_case(c, dev, 0.9)
            roll = G.roll_device(c, dev, G.policies(name, dev)["noncausal"], 32)
            out["fails"].append(ops.device_check_failures())
            for kind, d in got.items():
                for k, v in d.items():
                    arrays[f"{{name}}.{{sweep}}.{{kind}}.{{k}}"] = v
            for k, v in roll.items():
                arrays[f"{{name}}.{{sweep}}.roll.{{k}}"] = v
    np.savez({npz!r}, **arrays)
    json.dump(out, open({out!r}, "w"))
""")


def test_device_check_build(dev, env, tmp_path):
    """ELL and stencil cases under libirlmx_checks.so, fused and per sweep, in a
    fresh process: no check bit set and the same bits as the product build."""
    import __graft_entry__ as g
    names = ("k5-s200", "hub-s200", "k16-s200", "k8-s1029", "k40-s300", "37x23")
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
        roll = roll_device(TT.case(name), dev, policies(name, dev)["noncausal"], 32)
        for sweep in (0, 1):
            for kind in want:
                same({k: z[f"{name}.{sweep}.{kind}.{k}"] for k in want[kind]}, want[kind], f"{name} checks {sweep} {kind}")
            same({k: z[f"{name}.{sweep}.roll.{k}"] for k in roll}, roll, f"{name} checks {sweep} rollout")


def ld_dot(a, b):
    return (np.asarray(a).astype(LD) * np.asarray(b).astype(LD)).sum(axis=-1)


@pytest.mark.parametrize("name", ["16x16", "37x23", "64x64", "k5-s200", "k8-s1029", "128x40"])
def test_duality_and_order(dev, env, name):
    """Discount 1.  Duality: p0 . value0 against svf . r of ops.forward_svf_horizon
    under the same pi_t, both dotted in longdouble, within the header's
    ((T + 1)(K_c + A + 2) + T (K + A + 2)) 2^-53 (T + 1) max|r|.  Order:
    V_soft_0 >= v*_0 >= v^pi_0 entrywise, each up to that bound; and so the
    expected value difference is >= -bound."""
    from irlmx import ops
    c = TT.case(name)
    got = results(name, 1.0, dev)
    mdp = c.device_model(dev)
    tm = mask(c, mdp)
    bound = TT.duality_bound(c)
    _, v_soft = ops.soft_backward_horizon(mdp, np.array(c.reward), 1.0, c.T, tm, return_value0=True)
    v_soft, v_opt = v_soft.cpu().numpy(), got["optimal"]["v0"]
    assert (v_soft >= v_opt - bound).all(), float((v_opt - v_soft).max())
    for kind in ("noncausal", "causal"):
        pi = policies(name, dev)[kind]
        svf, _, _ = ops.forward_svf_horizon(mdp, np.array(c.p0), pi, tm)
        lhs, rhs = ld_dot(c.p0, got[kind]["v0"]), ld_dot(svf.cpu().numpy(), c.reward)
        gap = float(np.max(np.abs(lhs - rhs)))
        print(f"[timed] {name} {kind} duality |p0 . v0 - svf . r| {gap:.2e}, bound {bound:.2e}")
        assert gap <= bound, (name, kind, gap, bound)
        assert (v_opt >= got[kind]["v0"] - bound).all(), (name, kind, float((got[kind]["v0"] - v_opt).max()))
        evd, vo, vp = ops.expected_value_difference_horizon(mdp, np.array(c.reward), pi, np.array(c.p0), 1.0, tm)
        assert np.array_equal(bits(vo.cpu().numpy()), bits(v_opt)) and np.array_equal(bits(vp.cpu().numpy()), bits(got[kind]["v0"]))
        assert torch.equal(evd, (torch.as_tensor(np.array(c.p0), device=dev) * (vo - vp)).sum(dim=1))
        assert (evd.cpu().numpy() >= -bound).all(), evd


def test_value_difference_of_the_greedy_policy_is_zero(dev, env):
    """16x16 instance 0: the longdouble recursion's greedy one-hot policy (the best
    action is more than 1e-9 ahead of every different action at every step and
    state; two moves into a corner's walls are one action, timed_twin.greedy_one_hot)
    has the optimal value, so its expected value difference is within the bound of 0."""
    from irlmx import ops
    c = TT.case("16x16")
    for discount in TT.DISCOUNTS:
        greedy, gap = TT.greedy_one_hot(c.model(0), c.terminal, c.reward[0], discount, c.T)
        assert gap > 1e-9, gap
        mdp = c.device_model(dev, tables=[0])
        evd, v_opt, v_pi = ops.expected_value_difference_horizon(mdp, c.reward[[0]], greedy[None], c.p0[[0]], discount)
        print(f"[timed] greedy policy: evd {float(evd[0]):.2e}, top-two gap {gap:.2e}")
        assert abs(float(evd[0])) <= TT.duality_bound(c)
        assert float((v_opt - v_pi).abs().max()) <= TT.duality_bound(c)


# ---------------------------------------------------------------------------
# the batched drivers
# ---------------------------------------------------------------------------

DRIVER_T = 12


def drivers(dev):
    """(non-causal horizon driver, causal horizon driver, states, actions, lengths) on three 12 x 12 icy worlds,
    from 48 demonstrations of DRIVER_T steps under a planted reward's causal policy."""
    from irlmx import DeviceMDP, ops
    from irlmx.batch import BatchedCausalHorizon, BatchedMaxEnt
    mdp = DeviceMDP.icy_gridworld(12, [0.2, 0.1, 0.3], device=dev)
    theta = np.random.default_rng(3).uniform(0.2, 1.2, (3, mdp.n_states))
    pi = ops.soft_backward_horizon(mdp, theta, 0.9, DRIVER_T)
    ro = ops.rollout_horizon(mdp, pi, [5, 70, 130], 48, 11, return_trajectories=True)
    assert (ro.lengths == DRIVER_T).all()
    a = BatchedMaxEnt.from_trajectories(mdp, ro.states, ro.lengths, [], horizon=DRIVER_T)
    b = BatchedCausalHorizon.from_trajectories(mdp, ro.states, ro.lengths, [], horizon=DRIVER_T, discount=0.9)
    return a, b, ro


def snapshot(m):
    work = None if m._work is None else m._work["idx"].clone()
    return m.theta.clone(), m.k, m.active.clone(), work, m.steps.clone()


def unchanged(m, snap):
    theta, k, active, work, steps = snap
    assert torch.equal(m.theta, theta) and m.k == k and torch.equal(m.active, active) and torch.equal(m.steps, steps)
    assert (m._work is None) == (work is None) and (work is None or torch.equal(m._work["idx"], work))


@pytest.mark.parametrize("which", ["noncausal", "causal"])
def test_driver_methods_are_the_ops(dev, env, which):
    from irlmx import ops
    a, b, ro = drivers(dev)
    m = a if which == "noncausal" else b
    m.step()
    true_r = torch.as_tensor(np.random.default_rng(6).uniform(-1.0, 0.0, (3, m.mdp.n_states)), device=dev)
    for compacted in (False, True):
        if compacted:
            m.active[1] = False
            assert m.compact() == 2 and m.working_batch == 2
        snap = snapshot(m)
        if which == "noncausal":
            pi = ops.backward_maxent_horizon(m.mdp, m.theta, DRIVER_T, m.terminal)
        else:
            pi = ops.soft_backward_horizon(m.mdp, m.theta, 0.9, DRIVER_T, m.terminal)
        ll, ll_traj, _ = ops.demo_log_likelihood_horizon(pi, ro.states, ro.actions, ro.lengths)
        assert torch.equal(m.log_likelihood_horizon(ro.states, ro.actions, ro.lengths), ll / ll_traj.shape[1])
        for discount in (1.0, 0.9):
            want = ops.expected_value_difference_horizon(m.mdp, true_r, pi, m.p_initial, discount, m.terminal)[0]
            assert torch.equal(m.expected_value_difference_horizon(true_r, discount), want) and want.shape == (3,)
        got = m.sample_horizon([5, 70, 130], 20, 13)
        want = ops.rollout_horizon(m.mdp, pi, [5, 70, 130], 20, 13, terminal=m.terminal, return_trajectories=True)
        same(as_np(got), as_np(want), f"{which} sample_horizon")
        unchanged(m, snap)
        with pytest.raises(NotImplementedError, match="time-indexed"):
            m.log_likelihood(ro.states, ro.actions, ro.lengths)
        with pytest.raises(NotImplementedError, match="time-indexed"):
            m.expected_value_difference(true_r, 0.9)


def test_stationary_driver_names_the_stationary_methods(dev, env):
    from irlmx import DeviceMDP
    from irlmx.batch import BatchedMaxEnt
    mdp = DeviceMDP.icy_gridworld(5, 0.2, device=dev)
    S = mdp.n_states
    m = BatchedMaxEnt(mdp, np.ones((1, S)), np.full((1, S), 1.0 / S), [S - 1])
    with pytest.raises(ValueError, match="log_likelihood"):
        m.log_likelihood_horizon(None, None, None)
    with pytest.raises(ValueError, match="expected_value_difference"):
        m.expected_value_difference_horizon(np.zeros(S))
    with pytest.raises(ValueError, match="rollout"):
        m.sample_horizon(0, 4, 0)


def test_sample_device_horizon(dev, env):
    from irlmx import demos, ops
    c = TT.case("16x16")
    mdp = c.device_model(dev)
    pi = policies("16x16", dev)["causal"]
    e, p0, lengths = demos.sample_device_horizon(mdp, pi, [0, 5, 200], n=50, seed=3)
    out = ops.rollout_horizon(mdp, pi, [0, 5, 200], 50, 3)
    assert torch.equal(e, out.visits.to(torch.float64) / 50) and torch.equal(p0, out.starts.to(torch.float64) / 50)
    assert (lengths == c.T).all() and out.visits.sum(dim=1).tolist() == [50 * (c.T + 1)] * 3
    assert float((e.sum(dim=1) - (c.T + 1)).abs().max()) < 1e-12        # (visits / 50 rounds entry by entry)
    bad = pi.copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="bad policy row"):
        demos.sample_device_horizon(mdp, bad, [0, 5, 200], n=50, seed=3)
