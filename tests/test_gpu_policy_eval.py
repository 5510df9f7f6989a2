"""Policy evaluation and the expected value difference on the device (needs an MI355X).

ops.policy_evaluation (csrc/policy_eval.hip) against tests/policy_eval_twin.py:
the plan each case means to run, fused and per-sweep shapes bit for bit, values
within the project's bound 16 x max(e_oracle, e_floor) of the longdouble
evaluation at the same sweep count (max-norm measure, rewards of both signs),
the converged value against the direct linear solve, the exact duality with the
forward pass <p0, v_k> = <d_k, r> (no oracle in between), the semantics the
header states, the device bounds-check build, and the public layers
(solver drop-in, BatchedMaxEnt).  tests/test_policy_eval_cases.py checks the
same inputs without a device.
"""

import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import ell_cases as L
import extended_ref as X
import maxent_oracle as O
import policy_eval_twin as T
from conftest import ORACLE_DIR, PKG_DIR, ROOT, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KEYS = ("IRLMX_FUSED_MAX_STATES", "IRLMX_CLUSTER", "IRLMX_GRID")
SWEEP = {"IRLMX_FUSED_MAX_STATES": 0}
FUSED_CASES = [n for n, p in T.FUSED.items() if p is not None]
TESTS_DIR = os.path.join(ROOT, "tests")


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    import irlmx
    return irlmx.require_device()


@pytest.fixture
def env(monkeypatch):
    """Set exactly the given planner keys; all of them are cleared afterwards."""
    def set_env(values):
        for k in KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in values.items():
            assert k in KEYS, k
            monkeypatch.setenv(k, str(v))
    set_env({})
    yield set_env
    set_env({})


def mask(mdp, terminal):
    from irlmx import ops
    return None if terminal is None else ops.terminal_mask(list(terminal), mdp.n_states, batch=mdp.batch,
                                                           device=mdp.device)


def run(mdp, r, pi, discount, terminal=None, eps=T.EPS, max_iter=0):
    """(value, iterations, status) as host tensors."""
    from irlmx import ops
    out = ops.policy_evaluation(mdp, np.array(r, order="C"), np.array(pi, order="C"), discount, mask(mdp, terminal),
                                eps, max_iter)
    return tuple(x.cpu() for x in out)


def same(got, ref, what):
    for i, (x, y) in enumerate(zip(got, ref)):
        assert L.same_bits(x, y), f"{what}: output {i} differs"


def plan_pair(mdp):
    """(shape, (states per lane, slot class)) of the policy-evaluation plan."""
    from irlmx import _lib, ops
    p = ops.execution_plan(mdp, _lib.OP_POLICY_EVALUATION)
    assert p == ops.execution_plan(mdp, "policy_evaluation")
    if p["shape"] != "fused":
        assert p["shape"] == "sweep" and p["threads"] == 256 and p["spt"] == 1 and p["lds_bytes"] == 0, p
        return "sweep", None
    S = mdp.n_states
    assert p["launches"] == 1 and p["spt"] * p["threads"] >= S and p["threads"] % 64 == 0, p
    assert p["lds_bytes"] == 3 * 8 * S + 32, p
    return "fused", (p["spt"], L.slot_class(5 if mdp.layout == _lib.LAYOUT_STENCIL5 else mdp.k_row))


# -- 1. plan -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(T.CASES))
def test_plan(dev, env, name):
    mdp = T.device_model(name, dev)
    want = T.FUSED[name]
    env({})
    assert plan_pair(mdp) == (("fused", want) if want else ("sweep", None)), name
    env(SWEEP)
    assert plan_pair(mdp) == ("sweep", None), name


# -- 2. shapes bit-identical ---------------------------------------------------------------------

@pytest.mark.parametrize("name", FUSED_CASES)
def test_fused_equals_per_sweep(dev, env, name):
    c = T.base(name)
    mdp = T.device_model(name, dev)
    r, pi, term = T.reward(name), T.policy(name, "dirichlet"), tuple(c.terminal)
    for discount, terminal, cap in ((0.95, None, 0), (0.7, term, 0), (0.95, term, 10), (1.0, term, 33)):
        env({})
        assert plan_pair(mdp)[0] == "fused"
        fused = run(mdp, r, pi, discount, terminal, max_iter=cap)
        env(SWEEP)
        assert plan_pair(mdp)[0] == "sweep"
        same(run(mdp, r, pi, discount, terminal, max_iter=cap), fused, f"{name} g={discount} cap={cap}")
        if cap:
            # every instance stopped by the cap, or converged on its own at or before it
            capped = (fused[1] == cap) & (fused[2] == T.MAXITER)
            assert (capped | ((fused[1] <= cap) & (fused[2] == T.OK))).all(), (name, cap, fused[1], fused[2])
            assert capped.any(), (name, cap, fused[1], fused[2])
        else:
            assert (fused[2] == T.OK).all(), (name, fused[2])
    # a NaN reward in the last instance, and a NaN policy entry in the first: NONFINITE after one sweep
    for what in ("reward", "policy"):
        bad_r, bad_pi = np.array(r), np.array(pi)
        if what == "reward":
            bad_r[-1, c.S // 2] = np.nan
        else:
            bad_pi[0, c.S // 3, 0] = np.nan
        b = c.B - 1 if what == "reward" else 0
        env({})
        fused = run(mdp, bad_r, bad_pi, 0.95, term)
        env(SWEEP)
        same(run(mdp, bad_r, bad_pi, 0.95, term), fused, f"{name} NaN {what}")
        assert int(fused[2][b]) == T.NONFINITE and int(fused[1][b]) == 1, (name, what, fused[1], fused[2])
        assert all(int(fused[2][i]) == T.OK for i in range(c.B) if i != b), (name, what, fused[2])


@pytest.mark.parametrize("name", ["k5-s200", "k8-s1029", "k16-s1029", "k32-s200"])
def test_ell_instance_alone_as_shared_model(dev, env, name):
    c = T.base(name)
    env({})
    r, pi = T.reward(name), T.policy(name, "dirichlet")
    batch = run(T.device_model(name, dev), r, pi, 0.95, tuple(c.terminal))
    for b in range(c.B):
        alone = T.device_model(name, dev, tables=[b], shared=True)
        got = run(alone, r[b:b + 1], pi[b:b + 1], 0.95, tuple(c.terminal))
        same(got, tuple(x[b:b + 1] for x in batch), f"{name}[{b}]")


# -- 3. accuracy ---------------------------------------------------------------------------------

RUNS = [(name, r) for name in T.CASES for r in T.runs(name)]


@pytest.mark.parametrize("name,spec", RUNS, ids=[f"{n}-{r[0]}-{r[1]}" for n, r in RUNS])
def test_accuracy_against_longdouble(dev, env, name, spec):
    """Sweep counts and status equal the twin's; the value is within
    16 x max(e_oracle, e_floor) of the longdouble evaluation at that sweep count
    (normwise).  Measured ratios e_kernel / e_floor: profiles/policy_evaluation.txt."""
    from irlmx import ops
    kind, discount, terminal = spec
    c = T.base(name)
    env({})
    mdp = T.device_model(name, dev)
    r = T.reward(name)
    if kind == "maxent":   # the device's own policy, as a user would pass it
        pi = ops.backward_maxent(mdp, np.array(c.reward), mask(mdp, c.terminal)).cpu().numpy()
        assert np.isfinite(pi).all()
    else:
        pi = T.policy(name, kind)
    v, k, st = (x.numpy() for x in run(mdp, r, pi, discount, terminal))
    for b in range(c.B):
        if kind == "maxent":
            tv, tk, tst, deltas = T.twin(c.mats[b], r[b], pi[b], discount, terminal=terminal)
            ref = T.longdouble(c.mats[b], r[b], pi[b], discount, tk, terminal)
            e_oracle = X.normwise_err(tv, ref)
            assert T.margin_ok(deltas), (name, b, deltas[-2:])
        else:
            tv, tk, tst, deltas, ref, e_oracle = T.reference(name, b, kind, discount, terminal)
        e = X.normwise_err(v[b], ref)
        allowed = X.bound(e_oracle, c.k_row, c.A)
        print(f"[policy-eval] {name}[{b}] {kind} g={discount} sweeps {int(k[b])} e_oracle {e_oracle:.3e} "
              f"e_kernel {e:.3e} e_kernel/e_floor {e / c.floor():.2f} allowed {allowed:.3e}")
        assert (int(k[b]), int(st[b])) == (tk, tst), (name, b, int(k[b]), tk, int(st[b]), tst)
        assert e <= allowed, (name, b, e, allowed)


# -- 4. direct solve -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["16x16", "k5-s200"])
def test_converged_value_against_direct_solve(dev, env, name):
    """eps = 1e-10: within eps g / (1 - g) (truncation) + bound x max|v| (rounding,
    the bound being normwise) of np.linalg.solve on (I - g P_pi)."""
    c = T.base(name)
    env({})
    eps, discount, term = 1e-10, 0.95, tuple(c.terminal)
    r, pi = T.reward(name), T.policy(name, "dirichlet")
    v, k, st = (x.numpy() for x in run(T.device_model(name, dev), r, pi, discount, term, eps=eps))
    assert (st == T.OK).all()
    for b in range(c.B):
        exact = T.direct_solve(c.mats[b], r[b], pi[b], discount, term)
        tv, tk, _, _ = T.twin(c.mats[b], r[b], pi[b], discount, eps=eps, terminal=term)
        e_oracle = X.normwise_err(tv, T.longdouble(c.mats[b], r[b], pi[b], discount, tk, term))
        allowed = T.truncation(eps, discount) + X.bound(e_oracle, c.k_row, c.A) * np.max(np.abs(exact))
        err = float(np.max(np.abs(v[b] - exact)))
        print(f"[policy-eval] direct {name}[{b}] sweeps {int(k[b])} (twin {tk}) err {err:.3e} allowed {allowed:.3e}")
        assert err <= allowed, (name, b, err, allowed)


# -- 5. duality with the forward pass ------------------------------------------------------------

@pytest.mark.parametrize("name", ["16x16", "k5-s200"])
def test_duality_with_forward_svf(dev, env, name):
    """<p0, v_k> = <d_k, r> after k capped sweeps each, gamma = 1, r >= 0, terminals
    set: both are sum_{j<k} p0^T W^j r for the same folded W.  First-order worst
    case of k sweeps with K slots and A-fold weights plus the two S-term dots
    (taken here in longdouble): (k (K + A + 2) + 2 S) 2^-53, relative -- every
    term is non-negative, nothing cancels."""
    from irlmx import ops
    c = T.base(name)
    env({})
    mdp = T.device_model(name, dev)
    r = np.abs(T.reward(name))
    pi, term, p0 = T.policy(name, "dirichlet"), tuple(c.terminal), np.array(c.p0)
    tm = mask(mdp, term)
    for cap in (1, 7, 200):
        def both(n):
            d = ops.forward_svf(mdp, p0, tm, np.array(pi), max_iter=n)
            v = ops.policy_evaluation(mdp, r, np.array(pi), 1.0, tm, 1e-5, n)
            return [x.cpu().numpy() for x in d], [x.cpu().numpy() for x in v]
        (d, kd, sd), (v, kv, sv) = both(cap)
        for b in range(c.B):
            n = cap
            db, vb = d[b], v[b]
            if int(kd[b]) < cap or int(kv[b]) < cap:   # one of them converged first: compare at that count
                assert T.OK in (int(sd[b]), int(sv[b]))
                n = min(int(kd[b]), int(kv[b]))
                (d2, kd2, _), (v2, kv2, _) = both(n)
                assert int(kd2[b]) == n and int(kv2[b]) == n
                db, vb = d2[b], v2[b]
            else:
                assert int(sd[b]) in (T.MAXITER, T.OK) and int(sv[b]) in (T.MAXITER, T.OK)
            lhs = np.sum(p0[b].astype(X.LD) * vb.astype(X.LD))
            rhs = np.sum(db.astype(X.LD) * r[b].astype(X.LD))
            allowed = (n * (c.k_row + c.A + 2) + 2 * c.S) * 2.0 ** -53 * rhs
            print(f"[policy-eval] duality {name}[{b}] k={n} rel {float(abs(lhs - rhs) / rhs):.3e} "
                  f"allowed {float(allowed / rhs):.3e}")
            assert rhs > 0 and abs(lhs - rhs) <= allowed, (name, b, n, lhs, rhs)
            if cap == 1:
                assert np.array_equal(vb, r[b]), (name, b)   # v_1 = r + 1 * 0


# -- 6. semantics --------------------------------------------------------------------------------

def test_terminal_zero_row_nan_and_reversal(dev, env):
    name = "16x16"
    c = T.base(name)
    env({})
    mdp = T.device_model(name, dev)
    r, term = T.reward(name), tuple(c.terminal)
    pi = np.array(T.policy(name, "dirichlet"))
    pi[:, 7, :] = 0.0                                   # an exact-0 row
    v, k, st = run(mdp, r, pi, 0.95, term)
    assert (st == T.OK).all()
    for s in term + (7,):
        assert np.array_equal(v[:, s].numpy(), r[:, s]), s
    # the batch reversed: the results reversed, bit for bit
    rev = T.device_model(name, dev, tables=[2, 1, 0])
    same(run(rev, r[::-1], pi[::-1], 0.95, term), tuple(x.flip(0) for x in (v, k, st)), "reversed batch")
    # a NaN reward stops instance 1 after one sweep; the others are untouched
    bad = np.array(r)
    bad[1, 3] = np.nan
    for values in ({}, SWEEP):
        env(values)
        v2, k2, st2 = run(mdp, bad, pi, 0.95, term)
        assert st2.tolist() == [T.OK, T.NONFINITE, T.OK] and int(k2[1]) == 1, (st2, k2)
        assert np.isnan(v2[1, 3].item())
        assert L.same_bits(v2[[0, 2]], v[[0, 2]]) and L.same_bits(k2[[0, 2]], k[[0, 2]])


def test_uniform_policy_agrees_with_average_value_iteration(dev, env):
    """Different statement orders (pi-folded weights here, the action mean of
    g P_a v there), so not bit-equal: within the bound of the accuracy test."""
    from irlmx import ops
    name = "16x16"
    c = T.base(name)
    env({})
    mdp = T.device_model(name, dev)
    r = T.reward(name)
    pi = np.full((c.B, c.S, c.A), 1.0 / c.A)
    v, k, st = (x.numpy() for x in run(mdp, r, pi, 0.95))
    vi, kvi, _ = (x.cpu().numpy() for x in ops.value_iteration(mdp, np.array(r), 0.95, T.EPS, average=True))
    for b in range(c.B):
        tv, tk, _, deltas = T.twin(c.mats[b], r[b], pi[b], 0.95)
        ref = T.longdouble(c.mats[b], r[b], pi[b], 0.95, tk)
        allowed = X.bound(X.normwise_err(tv, ref), c.k_row, c.A)
        assert T.margin_ok(deltas), (b, deltas[-2:])   # the input condition: no stop hinges on a last bit
        assert int(k[b]) == int(kvi[b]) == tk, (b, int(k[b]), int(kvi[b]), tk)
        assert X.normwise_err(v[b], vi[b]) <= allowed and X.normwise_err(v[b], ref) <= allowed, b


# -- 7. the bounds-check build ---------------------------------------------------------------------

WORKER = textwrap.dedent("""
    import sys
    sys.path[:0] = [{root!r}, {pkg!r}, {oracle!r}, {tests!r}]
    import numpy as np, torch
    import policy_eval_twin as T
    from irlmx import _lib, ops
    assert _lib.load().irlmx_device_checks_enabled() == 1
    dev = torch.device("cuda", 0)
    out = {{}}
    for name in ("16x16", "k5-s200"):
        c = T.base(name)
        mdp = T.device_model(name, dev)
        tm = ops.terminal_mask(list(c.terminal), c.S, batch=c.B, device=dev)
        v, k, st = ops.policy_evaluation(mdp, np.array(T.reward(name)), np.array(T.policy(name, "dirichlet")), 0.95, tm)
        out[name + "_v"], out[name + "_k"] = v.cpu().numpy(), k.cpu().numpy()
    out["failures"] = np.array(ops.device_check_failures())
    np.savez({out!r}, **out)
""")


def test_device_check_build_same_bits(dev, env, tmp_path):
    import __graft_entry__ as g
    env({})
    res = str(tmp_path / "pe_checks.npz")
    code = WORKER.format(root=ROOT, pkg=PKG_DIR, oracle=ORACLE_DIR, tests=TESTS_DIR, out=res)
    subprocess.run([sys.executable, "-c", code], env=dict(os.environ, IRLMX_LIB=g.LIB_CHECKS), cwd=ROOT, check=True,
                   timeout=300)
    z = np.load(res)
    assert int(z["failures"]) == 0
    for name in ("16x16", "k5-s200"):
        c = T.base(name)
        v, k, _ = run(T.device_model(name, dev), T.reward(name), T.policy(name, "dirichlet"), 0.95, tuple(c.terminal))
        assert np.array_equal(v.numpy().view(np.int64), z[name + "_v"].view(np.int64)), name
        assert np.array_equal(k.numpy(), z[name + "_k"]), name


# -- 8. public layers ----------------------------------------------------------------------------

class World5:
    """The part of the reference IcyGridWorld API solver.optimal_policy uses."""

    def __init__(self, p_transition):
        self.size, self.n_states, self.n_actions = 5, 25, 4
        self.actions = O.ACTIONS
        self.p_transition = p_transition

    def state_index_transition(self, s, a):
        return O.intended_successor(self.size, s, a)


def test_solver_drop_in_config1(dev, env):
    import solver as S
    env({})
    z = load_golden("config1")
    P, r, g = np.array(z["p_transition"], dtype=np.float64), np.array(z["reward"], dtype=np.float64), 0.7
    mats = X.mats_from_table(P)
    world = World5(P)
    opt = S.optimal_policy(world, r, g)
    assert opt.shape == (25,) and np.issubdtype(opt.dtype, np.integer)
    one_hot = np.zeros((25, 4))
    one_hot[np.arange(25), opt] = 1.0
    uniform = np.full((25, 4), 0.25)
    for policy, table in ((opt, one_hot), (one_hot, one_hot), (uniform, uniform)):
        v = S.policy_evaluation(P, r, policy, g)
        assert isinstance(v, np.ndarray) and v.shape == (25,) and v.dtype == np.float64
        tv, tk, _, _ = T.twin(mats, r, table, g)
        ref = T.longdouble(mats, r, table, g, tk)
        assert X.normwise_err(v, ref) <= X.bound(X.normwise_err(tv, ref), 5, 4)
    p0 = np.full(25, 1.0 / 25)
    evd_opt = S.expected_value_difference(P, r, opt, p0, g)
    assert isinstance(evd_opt, float) and abs(evd_opt) <= 2 * T.truncation(1e-3, g), evd_opt
    assert S.expected_value_difference(P, r, uniform, p0, g) > 0
    with pytest.raises(ValueError):
        S.policy_evaluation(P, r, np.zeros((25, 3)), g)


@pytest.mark.parametrize("name", ["16x16", "k5-s200"])
def test_expected_value_difference_with_terminals(dev, env, name):
    """The terminal branch of ops.expected_value_difference against references
    that share none of its code: the greedy policy of the device's value
    iteration is taken on the host from the CSR matrices, v* is the twin's /
    longdouble evaluation of it with the terminals, v_pi likewise, and the sum
    is taken in longdouble.  Input condition, asserted: wherever the two best
    actions of a state are closer than 1e-9 their rows are identical, so
    either choice folds to the same weights."""
    from irlmx import ops
    c = T.base(name)
    env({})
    mdp = T.device_model(name, dev)
    r, term, g = T.reward(name), tuple(c.terminal), 0.9
    pi, p0 = T.policy(name, "dirichlet"), np.array(c.p0)
    tm = mask(mdp, term)
    evd, v_opt, v_pi = (x.cpu().numpy() for x in
                        ops.expected_value_difference(mdp, np.array(r), np.array(pi), p0, g, tm))
    v_vi = ops.value_iteration(mdp, np.array(r), g, T.EPS)[0].cpu().numpy()
    for b in range(c.B):
        mats = c.mats[b]
        q = np.stack([m.dot(v_vi[b]) for m in mats], axis=1)
        order = np.argsort(-q, axis=1, kind="stable")
        best, second = (order[:, 0], order[:, 1]) if c.A > 1 else (order[:, 0], order[:, 0])
        for s in np.flatnonzero(q[np.arange(c.S), best] - q[np.arange(c.S), second] < 1e-9):
            assert (mats[best[s]][s] != mats[second[s]][s]).nnz == 0, (name, b, int(s))
        greedy = np.zeros((c.S, c.A))
        greedy[np.arange(c.S), q.argmax(axis=1)] = 1.0
        refs = []
        for got, policy in ((v_opt[b], greedy), (v_pi[b], pi[b])):
            tv, tk, tst, deltas = T.twin(mats, r[b], policy, g, terminal=term)
            ref = T.longdouble(mats, r[b], policy, g, tk, term)
            assert tst == T.OK and T.margin_ok(deltas), (name, b, deltas[-2:])
            allowed = X.bound(X.normwise_err(tv, ref), c.k_row, c.A)
            assert X.normwise_err(got, ref) <= allowed, (name, b, X.normwise_err(got, ref), allowed)
            refs.append((ref, allowed * float(np.max(np.abs(ref)))))
        (ref_opt, a_opt), (ref_pi, a_pi) = refs
        want = np.sum(p0[b].astype(X.LD) * (ref_opt - ref_pi))
        # p0 sums to 1: each value's absolute bound, plus the S-term float64 dot
        slack = a_opt + a_pi + c.S * 2.0 ** -53 * float(np.sum(p0[b] * np.abs(ref_opt - ref_pi).astype(np.float64)))
        assert abs(float(evd[b] - want)) <= slack, (name, b, float(evd[b]), float(want), slack)
        assert np.array_equal(v_opt[b][list(term)], r[b][list(term)])


def test_batched_expected_value_difference(dev, env):
    from irlmx import ops
    from irlmx.batch import BatchedMaxEnt
    name = "16x16"
    c = T.base(name)
    env({})
    mdp = T.device_model(name, dev)
    true_r = np.array(c.reward)
    e_features = np.stack([c.forward(b, 7)[0] for b in range(c.B)])   # any demonstration statistics do
    irl = BatchedMaxEnt(mdp, e_features, np.array(c.p0), c.terminal)
    for _ in range(3):
        irl.step()
    theta, k, steps = irl.theta.clone(), irl.k, irl.steps.clone()
    assert bool(torch.isfinite(theta).all())
    evd = irl.expected_value_difference(true_r, 0.9)
    assert evd.shape == (c.B,) and torch.equal(irl.theta, theta) and irl.k == k and torch.equal(irl.steps, steps)
    assert irl._work is None
    tm = mask(mdp, c.terminal)
    pi = ops.backward_maxent(mdp, theta, tm)
    by_hand = ops.expected_value_difference(mdp, true_r, pi, np.array(c.p0), 0.9, tm)[0]
    assert L.same_bits(evd.cpu(), by_hand.cpu())
    assert (evd > -2 * T.truncation(1e-3, 0.9)).all()
    # compacted: instance 1 stopped, the working set is {0, 2}; the result stays in original order
    irl.active[1] = False
    assert irl.compact() == 2
    work = irl._work
    evd2 = irl.expected_value_difference(true_r, 0.9)
    assert irl._work is work and L.same_bits(evd2.cpu(), by_hand.cpu())
    irl.step()                                           # the compacted run goes on as before
    assert torch.equal(irl.theta[1], theta[1]) and irl.k == k + 1
