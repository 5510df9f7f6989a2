"""tests/timed_twin.py against itself, against tests/rollout_twin.py and against
hand enumeration -- without a device:

(a) with a stationary policy repeated T times the rollout and log-likelihood
    twins equal rollout_twin's at max_len = T bit for bit;
(b) value_ref at T = 3 on a 3 x 3 world equals the enumeration of all paths;
(c) on every GPU input the float64 twin is within the header's first-order
    bound of value_ref per state, and the project's bound 16 x max(e_twin,
    e_floor) admits a second correct float64 evaluation: the input condition of
    the GPU accuracy test;
(d) duality at discount 1, p0 . v_0 = D . r, in longdouble;
(e) the inputs of the GPU tests' statistical and telescoping assertions stay
    inside their bounds on the twin.
"""

import itertools

import numpy as np
import pytest

import extended_ref as X
import horizon_twin as H
import rollout_twin as R
import timed_twin as TT
from conftest import icy_stencil_rect
from test_horizon_twin import deterministic_grid

LD = np.longdouble


def _same(a, b):
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["16x16", "37x23", "k5-s200"])
def test_tiled_policy_is_the_stationary_twin(name):
    """(a) terminals included; bad start states; a NaN row."""
    c = H.case(name)
    mod = c.model(0)
    rng = np.random.default_rng(5)
    pi = rng.uniform(0.0, 1.0, (c.S, c.A))
    pi[rng.integers(0, c.S, 6), rng.integers(0, c.A, 6)] = 0.0
    pi[3] = np.nan
    T = 9
    tm = H._mask(c.terminal + [c.S // 3], c.S)
    start = rng.integers(0, c.S, 120)
    start[[4, 9]] = (-1, c.S)
    start[10:14], start[14:18] = 3, c.S // 3              # the NaN row; a terminal start state
    want = R.rollout(mod.nbr, mod.rv, pi, tm, start, 0xDEADBEEF12345, T)
    got = TT.rollout(mod.nbr, mod.rv, np.tile(pi, (T, 1, 1)), tm, start, 0xDEADBEEF12345)
    _same(got, want)
    assert {R.OK, R.TRUNCATED, R.BAD_POLICY, R.BAD_INDEX} <= set(want["status"].tolist())
    ok = np.isin(want["status"], (R.OK, R.TRUNCATED))
    ll, ll_traj, st = TT.log_likelihood(np.tile(pi, (T, 1, 1)), want["states"][ok], want["actions"][ok], want["lengths"][ok])
    wll, wll_traj, wst = R.log_likelihood(pi, want["states"][ok], want["actions"][ok], want["lengths"][ok])
    assert np.array_equal(ll_traj, wll_traj, equal_nan=True) and np.array_equal(st, wst)
    assert np.array_equal(ll, wll, equal_nan=True)


def test_no_terminal_means_full_length():
    c = H.case("16x16")
    pi = c.twin_backward(0)[0]
    out = TT.rollout(c.model(0).nbr, c.model(0).rv, pi, None, np.arange(50), 7)
    assert (out["status"] == R.TRUNCATED).all() and (out["lengths"] == c.T).all()
    assert out["visits"].sum() == 50 * (c.T + 1) and (out["states"] >= 0).all()
    # a length above T has no policy row: code 4, as a length beyond the row
    lengths = out["lengths"].copy()
    lengths[3] = c.T + 1
    states = np.concatenate([out["states"], out["states"][:, -1:]], axis=1)
    actions = np.concatenate([out["actions"], out["actions"][:, -1:]], axis=1)
    ll, ll_traj, st = TT.log_likelihood(pi, states, actions, lengths)
    assert st[3] == R.BAD_INDEX and np.isnan(ll_traj[3]) and np.isnan(ll) and (np.delete(st, 3) == R.OK).all()
    assert np.isfinite(np.delete(ll_traj, 3)).all()


@pytest.mark.parametrize("discount", TT.DISCOUNTS)
def test_value_ref_is_the_sum_over_all_paths(discount):
    """(b) 3 x 3, slip 0.2, T = 3, a random time-indexed policy, state 8 terminal:
    v_0(s) = sum over every path prefix (s_0, a_0, .., s_t) of its weight times
    discount^t r(s_t) (the rows of pi_t need not sum to 1 exactly), a path that
    enters state 8 ending there."""
    rv = icy_stencil_rect(3, 3, 0.2)
    mod = H.stencil_model(rv, 3, 3)
    rng = np.random.default_rng(8)
    T, S, A = 3, 9, 4
    pi = rng.dirichlet(np.ones(A), (T, S))
    r = rng.uniform(-1.0, 1.0, S)
    P = np.stack([m.toarray() for m in mod.mats]).astype(LD)       # [A, S, S]
    g = LD(np.float64(discount))
    want = np.zeros(S, dtype=LD)
    for s0 in range(S):
        def walk(t, s, prob):
            here = prob * g ** t * LD(r[s])
            if t == T or s == 8:
                return here
            return here + sum(walk(t + 1, s2, prob * LD(pi[t, s, a]) * P[a, s, s2])
                              for a, s2 in itertools.product(range(A), range(S)) if P[a, s, s2] != 0)
        want[s0] = walk(0, s0, LD(1))
    got, vt = TT.value_ref(mod.mats, [8], r, discount, T, pi)
    assert np.max(np.abs(got - want)) <= 1e-17 and np.array_equal(vt[0], got) and np.array_equal(vt[T], r.astype(LD))
    # the optimal value dominates every policy's and is the greedy policy's own
    opt, _ = TT.value_ref(mod.mats, [8], r, discount, T)
    assert (opt >= got - 1e-18).all()
    greedy, gap = TT.greedy_one_hot(mod, [8], r, discount, T)
    assert gap > 0 and np.max(np.abs(TT.value_ref(mod.mats, [8], r, discount, T, greedy)[0] - opt)) <= 1e-18


@pytest.mark.parametrize("discount", TT.DISCOUNTS)
@pytest.mark.parametrize("name", TT.CASES)
def test_twin_value_within_the_bounds(name, discount):
    """(c) The issue words the input condition as "the twin's value is within
    X.bound of value_ref".  Read literally that is e_twin <= 16 x max(e_twin,
    e_floor), which holds of any number, so it is asserted in the two forms that
    can fail: the twin per state under the header's first-order bound
    T (K + A + 2) u w_0(s), and a second correct float64 evaluation (slots and
    actions reversed) under X.bound(e_twin) -- the bound the GPU test holds the
    kernels to admits another float64 evaluation of the same input, as
    tests/test_soft_horizon_twin.py shows for the soft pass."""
    c = TT.case(name)
    for b, kind in itertools.product(range(c.B), TT.POLICIES):
        pi = TT.twin_policy(name, kind, b)
        mod = c.model(b)
        v0, vt, status = TT.value(mod, c.terminal, c.reward[b], discount, c.T, pi)
        ref, rt = TT.value_ref(mod.mats, c.terminal, c.reward[b], discount, c.T, pi)
        assert status == TT.OK and np.array_equal(vt[0], v0) and np.array_equal(vt[c.T], c.reward[b])
        err = np.abs(v0.astype(LD) - ref).astype(np.float64)
        bound = TT.value_bound(mod, c.terminal, c.reward[b], discount, c.T, pi)
        assert (err <= bound).all(), (name, b, kind, float(np.max(err / bound)))
        e_t = X.normwise_err(v0, ref)
        e_2 = X.normwise_err(TT.value(mod, c.terminal, c.reward[b], discount, c.T, pi, second=True)[0], ref)
        print(f"[timed twin] {name}[{b}] {kind} g {discount} e_twin {e_t:.2e} second {e_2:.2e} worst err/bound "
              f"{float(np.max(err / bound)):.3f}")
        assert e_2 <= X.bound(e_t, c.K, c.A), (name, b, kind, e_2, e_t)
        if c.terminal:
            assert np.array_equal(v0[c.terminal], c.reward[b][c.terminal])


def test_cases_reach_every_fused_pair():
    """The (states per thread, slot class) pairs the cases name are the eight
    fused_pair_ok(IRLMX_OP_VALUE_HORIZON) admits (tests/test_timed_resources.py
    counts the instantiations); the GPU test asserts each case's plan."""
    pairs = {TT.case(n).bwd for n in TT.FUSED}
    assert pairs == {(1, 5), (2, 5), (4, 5), (1, 8), (2, 8), (1, 16), (2, 16), (1, 32)}
    assert all(TT.case(n).bwd is None for n in TT.CASES if n not in TT.FUSED)
    c = TT.case("k16-s200")
    assert (c.S, c.A, c.B, c.K) == (200, 3, 2, 16) and c.S <= 1024


@pytest.mark.parametrize("name", ["16x16", "37x23", "k5-s200", "k8-s1029"])
def test_duality_in_longdouble(name):
    """(d) p0 . v_0 = D . r at discount 1 with D of horizon_twin.forward_ref under
    the same pi_t, terminals included: to 1e-17 of D . |r|."""
    c = H.case(name)
    for b, kind in itertools.product(range(c.B), ("noncausal", "causal")):
        pi = TT.twin_policy(name, kind, b)
        v0, _ = TT.value_ref(c.model(b).mats, c.terminal, c.reward[b], 1.0, c.T, pi)
        D, _ = H.forward_ref(c.model(b).mats, c.p0[b], c.terminal, pi)
        lhs, rhs = (c.p0[b].astype(LD) * v0).sum(), (D * c.reward[b].astype(LD)).sum()
        scale = (D * np.abs(c.reward[b]).astype(LD)).sum()
        assert abs(lhs - rhs) <= 1e-17 * scale, (name, b, kind, float(abs(lhs - rhs) / scale))


# ---------------------------------------------------------------------------
# (e) the inputs of the GPU tests' statistical and telescoping assertions
# ---------------------------------------------------------------------------

STAT_N, STAT_SEED, STAT_DELTA = 20000, 2024, 1e-9


def statistical_input(b=0):
    """``(c, pi_t, start)``: case 16x16, the CPU twin's non-causal pi_t of
    instance b (uploaded as it is by the GPU test, so the device draws the
    twin's trajectories bit for bit) and start states that realise c.p0 exactly."""
    c = H.case("16x16")
    pi = c.twin_backward(b)[0]
    n1 = int(round(0.25 * STAT_N))
    start = np.concatenate([np.zeros(STAT_N - n1, dtype=np.int64), np.full(n1, c.S // 2 + 3, dtype=np.int64)])
    return c, pi, start


def hoeffding(T, S, N, delta=STAT_DELTA):
    """visits(s) / N is a mean of N independent counts in [0, T + 1]: Hoeffding,
    with a union bound over the S states at failure probability delta."""
    return (T + 1) * np.sqrt(np.log(2 * S / delta) / (2 * N))


def test_statistical_input_is_inside_its_bound():
    c, pi, start = statistical_input()
    out = TT.rollout(c.model(0).nbr, c.model(0).rv, pi, None, start, R.instance_seeds(STAT_SEED, 1)[0])
    assert np.array_equal(out["starts"] / STAT_N, c.p0[0])
    D, _ = H.forward_ref(c.model(0).mats, c.p0[0], [], pi)
    dev = float(np.max(np.abs(out["visits"] / STAT_N - D.astype(np.float64))))
    bound = hoeffding(c.T, c.S, STAT_N)
    print(f"[timed twin] statistical: max |visits / N - svf| {dev:.4f}, bound {bound:.4f}")
    assert dev <= bound


TELE_SIZE, TELE_T, TELE_N, TELE_SEED = 12, 20, 64, 5


def telescoping_input():
    """The deterministic 12 x 12 GridWorld, T = 20, a reward in (-1.5, 0)."""
    mod = H.stencil_model(deterministic_grid(TELE_SIZE, TELE_SIZE), TELE_SIZE, TELE_SIZE)
    reward = np.random.default_rng(23).uniform(-1.5, 0.0, TELE_SIZE * TELE_SIZE)
    start = np.random.default_rng(24).integers(0, TELE_SIZE * TELE_SIZE, TELE_N)
    return mod, reward, start


def telescoping_check(mod, reward, pi, log_z0, states, actions, ll_traj):
    """``(worst |ll_traj - truth| / bound, worst |ll_traj - truth|)`` over full-length trajectories."""
    worst = worst_abs = 0.0
    T = pi.shape[0]
    for n in range(states.shape[0]):
        st, ac = states[n], actions[n]
        truth = reward[st].astype(LD).sum() - LD(log_z0[st[0]])
        logs = np.log(pi[np.arange(T), st[:T], ac].astype(LD))
        bound = TT.telescoping_bound(mod.K, mod.A, logs.astype(np.float64), log_z0[st[0]])
        err = float(abs(LD(ll_traj[n]) - truth))
        worst, worst_abs = max(worst, err / bound), max(worst_abs, err)
    return worst, worst_abs


def test_telescoping_on_the_twin():
    mod, reward, start = telescoping_input()
    pi, lz = H.backward(mod, [], reward, TELE_T)
    out = TT.rollout(mod.nbr, mod.rv, pi, None, start, TELE_SEED)
    assert (out["lengths"] == TELE_T).all()
    _, ll_traj, st = TT.log_likelihood(pi, out["states"], out["actions"], out["lengths"])
    assert (st == R.OK).all()
    ratio, err = telescoping_check(mod, reward, pi, lz, out["states"], out["actions"], ll_traj)
    print(f"[timed twin] telescoping: worst error {err:.2e}, worst error / bound {ratio:.3f}")
    assert ratio <= 1.0
