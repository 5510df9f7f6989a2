"""The finite-horizon twin and its longdouble restatement, checked without a
device (tests/horizon_twin.py; the GPU tests are tests/test_gpu_horizon.py).

* Exact path enumeration on a deterministic 3 x 3 grid pins the conventions: a
  visited state contributes its reward, the final one included; a terminal
  state ends the path (absorbing, counted once); T + 1 marginals.
* A one-state world in closed form.
* The float64 twin against the longdouble restatement on every GPU input, under
  the project's CPU limit of 1e-12 on an unshared e_oracle.
* A float64 restatement with one common scale per step returns thousands of NaN
  rows on the wide inputs, where the twin returns none.
"""

import numpy as np
import pytest

import extended_ref as X
import horizon_twin as H

LD = np.longdouble
LIMIT = 1e-12


def deterministic_grid(W, Hh):
    """STENCIL5 row form [4, 5, S] of the deterministic GridWorld: action a moves
    in direction a, or stays where that leaves the grid."""
    S = W * Hh
    s = np.arange(S)
    x, y = s % W, s // W
    rv = np.zeros((4, 5, S))
    for a, (dx, dy) in enumerate([(1, 0), (-1, 0), (0, 1), (0, -1)]):
        ok = (x + dx >= 0) & (x + dx < W) & (y + dy >= 0) & (y + dy < Hh)
        rv[a, a + 1] = ok
        rv[a, 0] = ~ok
    return rv


def enumerate_paths(rv, nbr, reward, terminal, p0, T):
    """Exact ``(D, d_t, log_z0)`` under P(path) ~ exp(sum of the rewards of the
    visited states): every action sequence from every start state, a path
    ending where it enters a terminal state or after T steps."""
    A, K, S = rv.shape
    nxt = np.array([[nbr[int(np.flatnonzero(rv[a, :, s])[0]), s] for a in range(A)] for s in range(S)])
    er = np.exp(np.asarray(reward, dtype=LD))
    Z = np.zeros(S, dtype=LD)
    visits = np.zeros((S, T + 1, S), dtype=LD)       # [start, t, state], weighted, unnormalised

    def walk(start, path, weight):
        s = path[-1]
        if s in terminal or len(path) == T + 1:
            Z[start] += weight
            for t, u in enumerate(path):
                visits[start, t, u] += weight
            return
        for a in range(A):
            walk(start, path + [int(nxt[s, a])], weight * er[nxt[s, a]])

    for s0 in range(S):
        walk(s0, [s0], er[s0])
    d = np.einsum("s,stu->tu", np.asarray(p0, dtype=LD) / Z, visits)
    return d.sum(axis=0), d, np.log(Z)


@pytest.mark.parametrize("terminal", [[8], []], ids=["terminal8", "none"])
def test_exact_enumeration_3x3(terminal):
    W = Hh = 3
    T = 4
    mod = H.stencil_model(deterministic_grid(W, Hh), W, Hh)
    rng = np.random.default_rng(5)
    reward = rng.uniform(-1.0, 0.5, 9)
    p0 = np.zeros(9)
    p0[0], p0[4] = 0.6, 0.4
    D, d, lz = enumerate_paths(mod.rv, mod.nbr, reward, terminal, p0, T)
    rpi, rlz = H.backward_ref(mod.mats, terminal, reward, T)
    rD, rd = H.forward_ref(mod.mats, p0, terminal, rpi.astype(np.float64))
    # the reference against the enumeration: its own rounding.  Fewer than 100 longdouble operations feed any
    # entry, and the forward was fed pi rounded to float64 (2^-53 per factor, T factors)
    ld_tol = 100 * 2.0 ** -64 + (T + 1) * 2.0 ** -53
    assert X.elementwise_err(rlz, lz) <= 100 * 2.0 ** -64
    assert X.elementwise_err(rD, D) <= ld_tol and X.elementwise_err(rd, d) <= ld_tol
    # the twin against the enumeration
    pi, tlz = H.backward(mod, terminal, reward, T)
    tD, td, status = H.forward(mod, p0, terminal, pi)
    assert status == H.OK
    assert X.elementwise_err(tD, D) <= 1e-14 and X.elementwise_err(td, d) <= 1e-14, (X.elementwise_err(tD, D))
    assert X.normwise_err(tlz, lz) <= 1e-14
    if not terminal:
        assert abs(float(D.sum()) - (T + 1)) <= 1e-17 * (T + 1) * 10 and abs(tD.sum() - (T + 1)) <= 1e-14
        assert np.allclose(td.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    else:
        assert float(D.sum()) < T + 1            # paths end at the terminal
        assert (td[2:, 8] > 0).all() and (td[:2, 8] == 0).all()   # two steps from state 4: exact zeros before


def test_one_state_world_closed_form():
    """S = 1, every action stays: Z_t = er * A * Z_{t+1}, so pi = 1 / A,
    log Z_0 = (T + 1) r + T log A, d_t = 1 and D = T + 1."""
    rv = np.zeros((4, 5, 1))
    rv[:, 0, 0] = 1.0
    mod = H.stencil_model(rv, 1, 1)
    for T, r in ((1, -0.3), (7, 0.9), (300, -20.0), (300, 5.0)):
        pi, lz = H.backward(mod, [], [r], T)
        assert np.array_equal(pi, np.full((T, 1, 4), 0.25))
        want = (T + 1) * r + T * np.log(4.0)
        assert abs(lz[0] - want) <= 4 * np.spacing(abs(want)) * max(1, T // 50), (T, r, lz[0], want)
        D, d, status = H.forward(mod, [1.0], [], pi)
        assert status == H.OK and np.array_equal(d, np.ones((T + 1, 1))) and D[0] == T + 1
        rpi, rlz = H.backward_ref(mod.mats, [], [r], T)
        assert np.array_equal(rpi, np.full((T, 1, 4), LD(0.25)))
    # a terminal state holds Z = er: log Z_0 = r, and its mass does not move on
    pi, lz = H.backward(mod, [0], [0.7], 5)
    assert np.array_equal(pi, np.full((5, 1, 4), 0.25)) and abs(lz[0] - 0.7) <= 2 ** -52
    D, d, _ = H.forward(mod, [1.0], [0], pi)
    assert D[0] == 1.0 and np.array_equal(d[1:], np.zeros((5, 1)))


def test_nonfinite_reward_is_nan_everywhere():
    mod = H.stencil_model(deterministic_grid(3, 3), 3, 3)
    r = np.zeros(9)
    r[4] = np.nan
    pi, lz = H.backward(mod, [], r, 3)
    assert np.isnan(pi).all() and np.isnan(lz).all()
    r[4] = -np.inf                 # exp(-inf) = 0 is finite: Z(4) is an exact zero and its own row 0 / 0, no more
    pi, lz = H.backward(mod, [], r, 3)
    assert np.isnan(pi[:, 4]).all() and np.isfinite(np.delete(pi, 4, axis=1)).all()
    assert lz[4] == -np.inf and np.isfinite(np.delete(lz, 4)).all()


@pytest.mark.parametrize("name", H.CASES)
def test_twin_against_longdouble(name):
    """e_twin of every output on every GPU input stays below 1e-12, the limit
    on an unshared e_oracle; the forward is fed the twin's own float64 pi_t."""
    c = H.case(name)
    for b in range(c.B):
        e_pi, e_lz = c.e_twin_backward(b)
        e_svf, e_marg = c.forward_errors(b, c.twin_backward(b)[0])
        print(f"[horizon twin] {name}[{b}] T {c.T} e_pi {e_pi:.3e} e_logz0 {e_lz:.3e} e_svf {e_svf:.3e} "
              f"e_svf_t {e_marg:.3e}")
        assert max(e_pi, e_lz, e_svf, e_marg) <= LIMIT, (name, b, e_pi, e_lz, e_svf, e_marg)
        if not c.terminal:
            D = H.forward(c.model(b), c.p0[b], c.terminal, c.twin_backward(b)[0])[0]
            tol = (c.T + 1) * (c.Kc + c.A + 2) * 2.0 ** -53          # include/irlmx.h derives it
            assert abs(float(D.astype(LD).sum()) - (c.T + 1)) <= tol * (c.T + 1), name


@pytest.mark.parametrize("W,Hh,lo,T", H.WIDE)
def test_common_scale_returns_nan_rows(W, Hh, lo, T):
    """One power-of-two scale per step is not enough on the wide inputs: the
    restatement loses thousands of rows, the per-state exponent none."""
    c = H.case(f"wide-{W}x{Hh}")
    lost = H.nan_rows(H.backward_common_scale(c.model(0), c.reward[0], T))
    pi, lz = c.twin_backward(0)
    print(f"[horizon twin] wide {W}x{Hh} lo {lo} T {T}: common-scale NaN rows {lost}")
    assert lost >= 1000, lost
    assert H.nan_rows(pi) == 0 and np.isfinite(lz).all()
