"""The finite-horizon soft value iteration's twin and its longdouble
restatement, checked without a device (tests/soft_horizon_twin.py; the GPU
tests are tests/test_gpu_soft_horizon.py).

(a) the bound 16 x max(e_twin, e_floor) admits a second correct float64
    evaluation (slots reversed, one-shot log-sum-exp) on every GPU input;
(b) on a deterministic world at discount 1 the model is the non-causal one:
    pi_t and V_0 = log Z_0 of tests/horizon_twin.py;
(c) the gradient identity d(p0 . V_0) / d r(s) = D(s) in longdouble;
(d) T = 1 by hand; (e) the stay action; (f) non-finite rewards.
"""

import numpy as np
import pytest

import extended_ref as X
import horizon_twin as H
import soft_horizon_twin as SH
from conftest import icy_stencil_rect

LD = np.longdouble


@pytest.mark.parametrize("discount", SH.DISCOUNTS)
@pytest.mark.parametrize("name", SH.CASES)
def test_bound_admits_a_second_float64_evaluation(name, discount):
    """(a) pi_t elementwise, V_0 normwise.  Measured: the largest ratio e /
    max(e_twin, e_floor) is 1.21; e_twin of pi_t is 7e-16 .. 1.8e-14 on the short
    cases, 1.3e-12 on wide-64x4 (|V| about 1,226) and 6.4e-12 on wide-256x4."""
    c = H.case(name)
    for b in range(c.B):
        pi, v0, status = SH.twin(name, discount, b, second=True)
        assert status == SH.OK == SH.twin(name, discount, b)[2]
        e_pi, e_v0 = SH.errors(pi, v0, name, discount, b)
        t_pi, t_v0 = SH.e_twin(name, discount, b)
        floor = X.e_floor(c.K, c.A)
        print(f"[soft horizon twin] {name}[{b}] g {discount} T {c.T} e_twin pi {t_pi:.2e} V0 {t_v0:.2e} | second pi "
              f"{e_pi:.2e} V0 {e_v0:.2e} | ratio pi {e_pi / max(t_pi, floor):.2f} V0 {e_v0 / max(t_v0, floor):.2f}")
        assert e_pi <= X.bound(t_pi, c.K, c.A), (name, b, e_pi, t_pi)
        assert e_v0 <= X.bound(t_v0, c.K, c.A), (name, b, e_v0, t_v0)


@pytest.mark.parametrize("terminal", [[], [7, 50]], ids=["none", "terminals"])
def test_deterministic_world_is_the_non_causal_model(terminal):
    """(b) slip 0, discount 1: each action has one successor, so softmax_a(r +
    V(next)) = log sum_a er Z(next).  Agreement within the sum of the two
    passes' bounds, each from its own twin's error against its own longdouble
    restatement.  Measured: 5.8e-15 relative in pi_t, 3.6e-15 in V_0."""
    W, Hh, T = 12, 9, 20
    mod = H.stencil_model(icy_stencil_rect(W, Hh, 0.0), W, Hh)
    reward = np.random.default_rng(21).uniform(-1.5, 0.0, W * Hh)
    pi, v0, status = SH.backward(mod, terminal, reward, 1.0, T)
    hpi, hlz = H.backward(mod, terminal, reward, T)
    rpi, rv0 = SH.backward_ref(mod.mats, terminal, reward, 1.0, T)
    hrpi, hrlz = H.backward_ref(mod.mats, terminal, reward, T)
    assert status == SH.OK
    # the two longdouble restatements agree to longdouble's own rounding
    assert X.elementwise_err(rpi, hrpi) <= 1e-16 and X.normwise_err(rv0, hrlz) <= 1e-16
    b_pi = X.bound(X.elementwise_err(pi, rpi), mod.K, mod.A) + X.bound(X.elementwise_err(hpi, hrpi), mod.K, mod.A)
    b_v0 = X.bound(X.normwise_err(v0, rv0), mod.K, mod.A) + X.bound(X.normwise_err(hlz, hrlz), mod.K, mod.A)
    e_pi, e_v0 = X.elementwise_err(pi, hpi), X.normwise_err(v0, hlz)
    print(f"[soft horizon twin] deterministic {terminal}: pi {e_pi:.2e} (bound {b_pi:.2e}) V0 {e_v0:.2e} (bound {b_v0:.2e})")
    assert e_pi <= b_pi and e_v0 <= b_v0, (e_pi, b_pi, e_v0, b_v0)
    if terminal:
        assert np.array_equal(v0[terminal], reward[terminal])          # held: absorbing
        assert np.allclose(pi[:, terminal].sum(axis=2), 1.0, rtol=0, atol=1e-14)   # the row of step 3 all the same


@pytest.mark.parametrize("name,b", [("16x16", 0), ("37x23", 0)])
def test_gradient_identity(name, b):
    """(c) d(p0 . V_0) / d r(s) = D(s) at discount 1, T = 10, in longdouble: the
    central difference is off by a pure h^2 term -- at most 1e-7 at h = 1e-4
    (measured 4.5e-9) and at h = 1e-5 at most 1/50 of that figure."""
    c = H.case(name)
    terminal = [] if name == "16x16" else c.terminal
    assert name == "16x16" or terminal
    T, mats, r, p0 = 10, c.model(b).mats, c.reward[b], c.p0[b]
    states = sorted(set(range(0, c.S, 37)) | set(terminal))
    D = SH.visitation_ref(mats, terminal, r, p0, T)[states]
    err = {}
    for h in (1e-4, 1e-5):
        err[h] = float(np.max(np.abs(SH.fd_gradient(mats, terminal, r, p0, T, h, states) - D)))
    print(f"[soft horizon twin] gradient identity {name}: |FD - D| {err[1e-4]:.2e} at h = 1e-4, {err[1e-5]:.2e} at 1e-5")
    assert err[1e-4] <= 1e-7 and err[1e-5] <= err[1e-4] / 50, err


@pytest.mark.parametrize("discount", SH.DISCOUNTS)
def test_one_step_by_hand(discount):
    """(d) T = 1: V_0 = softmax_a (r + discount P_a r), pi_0 = exp(q - V_0)."""
    c = H.case("16x16-T1")
    mod, r = c.model(0), c.reward[0]
    q = np.stack([r + discount * np.asarray(m.dot(r)) for m in mod.mats], axis=1)
    want = np.log(np.exp(q).sum(axis=1))
    pi, v0, status = SH.twin("16x16-T1", discount, 0)
    assert status == SH.OK and pi.shape == (1, c.S, 4)
    assert np.max(np.abs(v0 - want)) <= 8 * 2.0 ** -52 * np.max(np.abs(want))
    assert np.max(np.abs(pi[0] - np.exp(q - want[:, None]))) <= 1e-14


def test_stay_action_rows_sum_to_one():
    """(e) A = 5: every entry is within the bound relatively, so a row's sum is within it absolutely."""
    for discount in SH.DISCOUNTS:
        pi, _, _ = SH.twin("64x12-stay", discount, 0)
        assert pi.shape[-1] == 5
        assert np.max(np.abs(pi.astype(LD).sum(axis=-1) - 1)) <= SH.bounds("64x12-stay", discount, 0)[0]


def test_single_action_rows_are_one():
    rv = np.zeros((1, 5, 6))
    rv[0, 1], rv[0, 0, [2, 5]], rv[0, 1, [2, 5]] = 1.0, 1.0, 0.0        # move +x, stay at the right edge
    mod = H.stencil_model(rv, 3, 2)
    pi, v0, status = SH.backward(mod, [], np.linspace(-1, 1, 6), 0.9, 4)
    assert status == SH.OK and np.array_equal(pi, np.ones((4, 6, 1)))


def test_nonfinite_rewards():
    """(f) A NaN reward spreads one neighbourhood per step, by IEEE rules, and
    always sits in V_0 at its own state; a -inf reward makes its own V NaN (-inf
    - -inf in the fold) and spreads the same way; a state whose zero-weight
    off-grid slot points at itself is reached too.  status NONFINITE."""
    c = H.case("16x16")
    mod, T = c.model(0), 3
    far = 15 * 16 + 15
    for bad in (np.nan, -np.inf, np.inf):
        r = c.reward[0].copy()
        r[0] = bad
        pi, v0, status = SH.backward(mod, [], r, 1.0, T)
        assert status == SH.NONFINITE and not np.isfinite(v0[0])
        s = np.arange(256)
        dist = s % 16 + s // 16                       # steps from state 0 on the grid: one more per step
        assert np.array_equal(~np.isfinite(v0), dist <= T), bad
        assert np.isfinite(pi[:, far]).all() and np.isnan(pi[:, 0]).all()
        assert np.array_equal(np.isnan(pi[0]).any(axis=1), dist <= T)
    clean = SH.backward(mod, [], c.reward[0], 1.0, T)
    assert clean[2] == SH.OK and np.isfinite(clean[0]).all() and np.isfinite(clean[1]).all()
    # a terminal state holds its non-finite reward
    r = c.reward[0].copy()
    r[40] = np.nan
    _, v0, status = SH.backward(mod, [40], r, 0.9, 2)
    assert status == SH.NONFINITE and np.isnan(v0[40])
