"""CPU twin and longdouble restatement of the calls on time-indexed policies
(include/irlmx_timed.h; csrc/rollout.hip, csrc/soft_horizon.hip); not a test module.  Models and cases
come from tests/horizon_twin.py, the generator, ``pick`` and the log from
tests/rollout_twin.py.

* :func:`rollout` / :func:`log_likelihood` -- the header's statements in numpy:
  rollout_twin's with the policy row of step t.  Integer counts, adds and one
  product per draw: these two produce the device's bits, and the GPU tests
  compare bit for bit.
* :func:`value` -- the float64 twin of irlmx_value_horizon in the header's
  order.  numpy has no fused multiply-add, so it rounds each product and each
  sum separately where the kernels use ``fma``: two correct float64
  evaluations, never compared bit for bit.  ``second=True`` is another one
  (slots and actions in reverse order).
* :func:`value_ref` -- the same mathematics in ``np.longdouble`` on CSR
  matrices, with no attention to order.
* the header's first-order bounds: :func:`value_bound`, :func:`duality_bound`,
  :func:`telescoping_bound`.
"""

import functools

import numpy as np

import extended_ref as X
import horizon_twin as H
import rollout_twin as R

LD = np.longdouble
U = 2.0 ** -53
OK, NONFINITE = H.OK, H.NONFINITE
DISCOUNTS = (1.0, 0.9)
#: the launches of tests/test_gpu_timed.py's value tests: the smallest cases that reach every
#: fused pair -- <1,5> (16x16 with per-instance tables, 16x16-T1, 37x23 with terminals, k5-s200:
#: ELL with terminals), <2,5> (64x20), <4,5> (64x64), <1,8> (hub-s200), <2,8> (k8-s1029), <1,16>
#: (k16-s200, below), <2,16> (k16-s1029), <1,32> at A = 8 (k32-s200) -- and the two without a
#: fused kernel (128x40, k40-s300); tests/test_timed_twin.py holds the list to the eight pairs
CASES = ("16x16", "16x16-T1", "37x23", "64x20", "64x64", "k5-s200", "hub-s200", "k8-s1029", "k16-s200", "k16-s1029",
         "k32-s200", "128x40", "k40-s300")
#: those of CASES the fused shape runs
FUSED = tuple(n for n in CASES if n not in ("128x40", "k40-s300"))
POLICIES = ("noncausal", "causal", "optimal")


class EllCase(H.Case):
    """A horizon_twin.Case whose ELL tables are its own (horizon_twin's ELL cases
    are looked up by name in tests/ell_cases.py's fixed list)."""

    def device_model(self, dev, tables=None):
        import torch
        from irlmx import DeviceMDP, _lib
        mods = [self.models[b] for b in (range(self.B) if tables is None else tables)]
        t = lambda xs, dt: torch.as_tensor(np.stack(xs), dtype=dt, device=dev).contiguous()   # noqa: E731
        return DeviceMDP(_lib.LAYOUT_ELL, self.S, self.A, len(mods), False, t([m.rv for m in mods], torch.float64),
                         row_idx=t([m.nbr for m in mods], torch.int32), col_idx=t([m.src for m in mods], torch.int32),
                         col_val=t([m.cv for m in mods], torch.float64), k_row=self.K, k_col=self.Kc, device=dev)


def _k16_s200():
    """200 states, 3 actions, 2 tables of 2 .. 16 targets per state (k_row = 16), T = 12, terminals 199 and 2:
    ell_cases' generator at the one (states per thread, slot class) pair, <1,16>, no case of horizon_twin plans."""
    import ell_cases as E
    S, A, B, T = 200, 3, 2, 12
    tabs = [E.table(S, A, 2, 16, 16, 9990 + b) for b in range(B)]
    counts = {E.slot_counts(t.mats) for t in tabs}
    assert len(counts) == 1 and 9 <= next(iter(counts))[0] <= 16, counts
    (k_row, k_col), = counts
    rng = np.random.default_rng(9999)
    p0 = rng.dirichlet(np.ones(S), B)
    return EllCase("k16-s200", [H.ell_model(t.mats, k_row, k_col) for t in tabs], rng.uniform(-1.5, 0.0, (B, S)), p0,
                   [S - 1, 2], T, (1, 16), None)


@functools.lru_cache(maxsize=None)
def case(name):
    """horizon_twin's case of that name, or this module's own."""
    return _k16_s200() if name == "k16-s200" else H.case(name)


# ---------------------------------------------------------------------------
# trajectories
# ---------------------------------------------------------------------------

def rollout(targets, row_val, pi_t, terminal, start, seed):
    """One instance of irlmx_rollout_horizon: ``targets`` [K, S] ints,
    ``row_val`` [A, K, S], ``pi_t`` [T, S, A], ``terminal`` a bool [S] mask or
    None, ``start`` [N] ints, ``seed`` a 64-bit int.  Returns rollout_twin.rollout's
    dict with max_len = T."""
    targets, row_val = np.asarray(targets), np.asarray(row_val, dtype=np.float64)
    pi_t = np.asarray(pi_t, dtype=np.float64)
    T, S = pi_t.shape[0], pi_t.shape[1]
    terminal = np.zeros(S, bool) if terminal is None else np.asarray(terminal, dtype=bool)
    start = np.asarray(start, dtype=np.int64)
    N = start.size
    key = np.array(R.split_seed(seed), dtype=np.uint64)
    visits, starts = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    lengths, status = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    states = np.full((N, T + 1), -1, dtype=np.int32)
    actions = np.full((N, T), -1, dtype=np.int32)
    valid = (start >= 0) & (start < S)
    status[~valid] = R.BAD_INDEX
    state = np.where(valid, start, 0)
    np.add.at(starts, state[valid], 1)
    states[valid, 0] = state[valid]
    alive = valid & ~terminal[state]
    status[alive] = R.TRUNCATED
    for t in range(T):
        idx = np.flatnonzero(alive)
        if idx.size == 0:
            break
        s = state[idx]
        np.add.at(visits, s, 1)
        ctr = np.stack([np.full(idx.size, t), idx, np.zeros_like(idx), np.zeros_like(idx)], axis=1)
        u_action, u_next = R.uniforms(R.philox4x32_10(ctr, key))
        a = R.pick(u_action, pi_t[t][s])
        stop = a < 0
        status[idx[stop]], alive[idx[stop]] = R.BAD_POLICY, False
        idx, s, a, u_next = idx[~stop], s[~stop], a[~stop], u_next[~stop]
        k = R.pick(u_next, row_val[a, :, s])
        nxt = targets[np.maximum(k, 0), s]
        stop = (k < 0) | (nxt < 0) | (nxt >= S)
        status[idx[stop]], alive[idx[stop]] = R.BAD_TABLE, False
        idx, a, nxt = idx[~stop], a[~stop], nxt[~stop]
        actions[idx, t], states[idx, t + 1] = a, nxt
        lengths[idx] += 1
        state[idx] = nxt
        done = terminal[nxt]
        status[idx[done]], alive[idx[done]] = R.OK, False
    np.add.at(visits, state[valid], 1)
    return {"visits": visits, "starts": starts, "lengths": lengths, "status": status, "states": states,
            "actions": actions}


def log_likelihood(pi_t, states, actions, lengths):
    """``(ll, ll_traj [N], status [N])`` of one instance under ``pi_t`` [T, S, A]:
    numpy's log as maxent_oracle.numpy_log_restated computes it, every sum
    sequential from 0; a length above T is code 4 as every other bad length."""
    import maxent_oracle as O
    pi_t = np.asarray(pi_t, dtype=np.float64)
    T, S, A = pi_t.shape
    states, actions, lengths = np.asarray(states), np.asarray(actions), np.asarray(lengths)
    ll_traj = np.zeros(lengths.size)
    status = np.zeros(lengths.size, dtype=np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for n, length in enumerate(lengths):
            length = int(length)
            ac = actions[n] if actions.shape[1] else actions[n][:0]
            if length > T or not R._readable(states[n], ac, length, S, A):
                status[n], ll_traj[n] = R.BAD_INDEX, np.nan
                continue
            logs = O.numpy_log_restated(pi_t[np.arange(length), states[n, :length], actions[n, :length]])
            ll_traj[n] = np.add.accumulate(np.concatenate([[0.0], logs]))[-1]
        ll = np.add.accumulate(np.concatenate([[0.0], ll_traj]))[-1]
    return ll, ll_traj, status


def telescoping_bound(K, A, logs, log_z0):
    """The header's bound on |ll_traj - (sum_{t<=T} r(s_t) - log_z0(s_0))| of a
    full-length trajectory on a deterministic table: ``logs`` the T values log
    pi_t(s_t, a_t) (any precision), ``log_z0`` that of the start state."""
    logs = np.abs(np.asarray(logs, dtype=np.float64))
    T = logs.size
    partial = np.max(np.cumsum(logs)) if T else 0.0
    return U * (T * (K + A + 2) + 2 * logs.sum() + T * partial + 4 * abs(float(log_z0)))


# ---------------------------------------------------------------------------
# the value pass
# ---------------------------------------------------------------------------

def value(mod, terminal, reward, discount, T, pi_t=None, second=False):
    """``(v_0 [S], v_t [T + 1, S], status)`` in float64, in the header's order."""
    rv, nbr = mod.rv, mod.nbr
    A, K, S = rv.shape
    r = np.asarray(reward, dtype=np.float64)
    g = np.float64(discount)
    tm = H._mask(terminal, S)
    slots = range(K - 1, -1, -1) if second else range(K)
    acts = range(A - 1, -1, -1) if second else range(A)
    v = r.copy()
    out = np.empty((T + 1, S))
    out[T] = v
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            vn = v[nbr]
            e = np.zeros(S)
            best = None
            for a in acts:
                acc = np.zeros(S)
                for k in slots:
                    acc = rv[a, k] * vn[k] + acc
                if pi_t is not None:
                    e = pi_t[t][:, a] * acc + e
                else:
                    q = r + g * acc
                    best = q if best is None else np.where(np.isnan(best) | (q <= best), best, q)
            new = r + g * e if pi_t is not None else best
            v = np.where(tm, r, new)
            out[t] = v
    return v, out, (OK if np.isfinite(v).all() else NONFINITE)


def value_ref(mats, terminal, reward, discount, T, pi_t=None):
    """``(v_0 [S], v_t [T + 1, S])`` in longdouble from a float64 ``pi_t`` (None: the optimal value)."""
    p = X._ld_mats(mats)
    S = p[0].shape[0]
    r = np.asarray(reward, dtype=LD)
    g = LD(np.float64(discount))
    tm = H._mask(terminal, S)
    pi = None if pi_t is None else X._ld(pi_t)
    v = r.copy()
    out = [v]
    for t in range(T - 1, -1, -1):
        pv = [m.dot(v) for m in p]
        if pi is None:
            new = np.max(np.stack([r + g * x for x in pv]), axis=0)
        else:
            e = np.zeros(S, dtype=LD)
            for a, x in enumerate(pv):
                e = e + pi[t][:, a] * x
            new = r + g * e
        v = np.where(tm, r, new)
        out.append(v)
    return v, np.stack(out[::-1])


def value_bound(mod, terminal, reward, discount, T, pi_t=None):
    """The header's first-order bound per state: T (K + A + 2) u w_0(s), w the same recursion on |r|."""
    w0, _ = value_ref(mod.mats, terminal, np.abs(np.asarray(reward, dtype=np.float64)), discount, T, pi_t)
    return T * (mod.K + mod.A + 2) * U * w0.astype(np.float64)


def duality_bound(c):
    """The header's bound on |p0 . v_0 - D . r| at discount 1 for a distribution p0."""
    return ((c.T + 1) * (c.Kc + c.A + 2) + c.T * (c.K + c.A + 2)) * U * (c.T + 1) * float(np.max(np.abs(c.reward)))


def greedy_one_hot(mod, terminal, reward, discount, T):
    """``(pi_t [T, S, A] one-hot of the longdouble optimal recursion's first best
    action, smallest gap between the best q and the best q of a different
    action, over all steps and non-terminal states)``.  An action whose stored
    row at s equals the best action's row there is the same action at s (two
    moves into the walls of a corner): it ties exactly and is equally optimal;
    a terminal state holds v = r whatever its row says."""
    p = X._ld_mats(mod.mats)
    r = np.asarray(reward, dtype=LD)
    g = LD(np.float64(discount))
    _, vt = value_ref(mod.mats, terminal, reward, discount, T)
    tm = H._mask(terminal, mod.S)
    pi = np.zeros((T, mod.S, mod.A))
    gap = np.inf
    s = np.arange(mod.S)
    for t in range(T):
        q = np.stack([r + g * m.dot(vt[t + 1]) for m in p], axis=1)
        best = q.argmax(axis=1)
        pi[t][s, best] = 1.0
        same_row = (mod.rv == mod.rv[best, :, s].T[None]).all(axis=1).T          # [S, A]
        other = np.where(same_row, LD(-np.inf), q).max(axis=1)
        live = ~tm & np.isfinite(other)
        gap = min(gap, float(np.min((q[s, best] - other)[live])))
    return pi, gap


# ---------------------------------------------------------------------------
# per case: computed once, frozen
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def twin_policy(name, kind, b):
    """The CPU twins' pi_t of a case (tests without a device; the GPU tests take the device's own)."""
    import soft_horizon_twin as SH
    c = case(name)
    if kind == "optimal":
        return None
    if kind == "noncausal":
        return c.twin_backward(b)[0]
    return SH.backward(c.model(b), c.terminal, c.reward[b], 1.0, c.T)[0]


def errors(v0, c, b, discount, pi_t):
    """Normwise error of ``v0`` against the longdouble restatement under the same float64 ``pi_t``."""
    return X.normwise_err(v0, value_ref(c.model(b).mats, c.terminal, c.reward[b], discount, c.T, pi_t)[0])


def e_twin(c, b, discount, pi_t):
    return errors(value(c.model(b), c.terminal, c.reward[b], discount, c.T, pi_t)[0], c, b, discount, pi_t)
