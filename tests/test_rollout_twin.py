"""The CPU twin of the demonstration kernels (tests/rollout_twin.py) against
what does not come from this project: Random123's known-answer vectors for
Philox4x32-10, the binomial law, and the reference's own statistics of its 200
trajectories in tests/golden/config1.npz.  No device."""

import numpy as np
import pytest

import rollout_twin as R
from conftest import icy_stencil_rect, load_golden

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = R.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert " ".join(f"{int(v):08x}" for v in got) == want


def test_philox_vectorised_equals_scalar():
    ctr = np.array([c for c, _, _ in KAT], dtype=np.uint64)
    key = np.array([k for _, k, _ in KAT], dtype=np.uint64)
    got = R.philox4x32_10(ctr, key)
    for i, (_, _, want) in enumerate(KAT):
        assert " ".join(f"{int(v):08x}" for v in got[i]) == want


def test_uniforms_in_unit_interval():
    lo, hi = R.uniforms(np.zeros(4, dtype=np.uint64)), R.uniforms(np.full(4, 0xffffffff, dtype=np.uint64))
    assert lo == (0.0, 0.0)
    assert hi[0] == hi[1] == 1.0 - 2.0 ** -53           # the largest value: still below 1
    n = np.arange(20000)
    ctr = np.stack([n % 7, n, 0 * n, 0 * n], axis=1)
    for u in R.uniforms(R.philox4x32_10(ctr, np.array(R.split_seed(99), dtype=np.uint64))):
        assert u.dtype == np.float64 and (u >= 0).all() and (u < 1).all()
        assert abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / u.size)
        assert (u * 2.0 ** 53 == np.floor(u * 2.0 ** 53)).all()     # 53-bit integers, exactly


def test_pick_rule():
    w = np.array([[0.0, 1.0, 0.0, 3.0, 0.0]])
    assert R.pick([0.0], w)[0] == 1                         # a zero-weight slot is never drawn, not even at u = 0
    assert R.pick([0.25 - 2.0 ** -54], w)[0] == 1
    assert R.pick([0.25], w)[0] == 3                        # strict compare: x = c_1 moves on
    assert R.pick([1.0 - 2.0 ** -53], w)[0] == 3
    # x rounds up to total: the last positive slot, not the trailing zero-weight one
    tiny = np.array([[2.0 ** -1074, 0.0]])
    assert R.pick([1.0 - 2.0 ** -53], tiny)[0] == 0
    for bad in ([0.0, 0.0], [1.0, -0.5], [1.0, np.nan], [np.inf, 1.0], [1e308, 1e308]):
        assert R.pick([0.5], np.array([bad]))[0] == -1, bad
    assert R.pick([0.5], np.array([[2.0, 6.0]]))[0] == 1    # rows need not be normalised


#: the committed seed of the unbiasedness test: key (12345, 7)
SEED = 12345 | (7 << 32)


def test_unbiased_first_step():
    """Step-0 action and successor frequencies on the 5x5 icy gridworld (p_slip
    0.2) from the centre state, N = 4096: each within five binomial standard
    deviations, 5 * sqrt(p (1 - p) / n), of its probability (n = N for the
    actions, the number of action-0 draws for the successors given action 0; a
    probability of 0 must give a count of 0).  Deterministic: one seed."""
    N, start = 4096, 12
    rv = icy_stencil_rect(5, 5, 0.2)
    pi = np.tile([0.4, 0.3, 0.2, 0.1], (25, 1))
    out = R.rollout(R.stencil_targets(5, 5), rv, pi, np.zeros(25, bool), np.full(N, start), SEED, 1)
    assert (out["lengths"] == 1).all() and (out["status"] == R.TRUNCATED).all()
    a, nxt = out["actions"][:, 0], out["states"][:, 1]
    worst = 0.0
    for j, p in enumerate(pi[start]):
        sigma = np.sqrt(p * (1 - p) / N)
        worst = max(worst, abs((a == j).mean() - p) / sigma)
    n0 = int((a == 0).sum())
    targets = R.stencil_targets(5, 5)[:, start]
    for k, p in enumerate(rv[0, :, start]):
        f = ((a == 0) & (nxt == targets[k])).sum() / n0
        if p == 0:
            assert f == 0
        else:
            worst = max(worst, abs(f - p) / np.sqrt(p * (1 - p) / n0))
    print(f"worst deviation {worst:.2f} sigma")
    assert worst <= 5.0, worst
    assert out["visits"].sum() == 2 * N and out["visits"][start] >= N and out["starts"][start] == N


def test_statistics_match_reference_fixture():
    """visits / n and starts / n of the reference's 200 trajectories equal its own
    feature expectation and initial distribution (maxent.py:15-60) exactly."""
    g = load_golden("config1")
    states, actions, lengths = R.pack(g["traj_flat"], g["traj_lens"])
    assert states.shape == (200, int(g["traj_lens"].max()) + 1) and actions.shape[1] == states.shape[1] - 1
    visits, starts, status = R.statistics(25, states, lengths)
    assert (status == R.OK).all()
    assert np.array_equal(visits / 200, g["e_features"]) and np.array_equal(starts / 200, g["p_initial"])
    assert visits.sum() == lengths.sum() + 200


def test_statistics_and_likelihood_guards():
    states = np.array([[0, 1, 2], [0, 3, -1], [0, 1, 1], [5, 0, 0]], dtype=np.int32)
    actions = np.array([[0, 1], [2, 0], [0, 0], [0, 0]], dtype=np.int32)
    lengths = np.array([2, 2, 3, 0])
    visits, starts, status = R.statistics(4, states, lengths)
    assert list(status) == [R.OK, R.BAD_INDEX, R.BAD_INDEX, R.BAD_INDEX]      # state -1, length > L, state 5
    assert list(visits) == [1, 1, 1, 0] and list(starts) == [1, 0, 0, 0]
    try:
        import maxent_oracle as O
        O.numpy_log_restated(np.ones(1))
    except OSError:
        pytest.skip("oracle/libblas_order.so not built")
    pi = np.full((4, 3), 0.25)
    pi[1, 1] = 0.0
    ll, ll_traj, status = R.log_likelihood(pi, states, actions, np.array([2, 1, 0, 0]))
    assert list(status) == [R.OK, R.OK, R.OK, R.BAD_INDEX]
    assert ll_traj[0] == -np.inf and ll_traj[2] == 0.0 and np.isnan(ll_traj[3]) and np.isnan(ll)
    assert ll_traj[1] == O.numpy_log_restated(np.array([0.25]))[0]
