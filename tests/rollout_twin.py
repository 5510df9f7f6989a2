"""CPU twin of the demonstration kernels (csrc/rollout.hip); not a test module.

A numpy restatement of everything include/irlmx.h states for irlmx_rollout,
irlmx_demo_statistics and irlmx_demo_log_likelihood: Philox4x32-10 in uint64
arithmetic, the two uniforms per step, the ``pick`` rule, the step rule and the
status codes, the visit / start statistics and the log-likelihood (numpy's log
as oracle/maxent_oracle.py restates it, sequential sums).  It is the checker of
tests/test_gpu_rollout.py, which compares bit for bit, and is itself pinned by
tests/test_rollout_twin.py (Random123's known-answer vectors, the reference's
statistics of tests/golden/config1.npz).  It does not import irlmx.

The trajectories of one instance advance in lock-step, one numpy operation per
step over the trajectories still alive; every floating-point sum is built by
elementwise adds in index order, so each trajectory sees exactly the scalar
sequence of operations the header states.
"""

import numpy as np

OK, TRUNCATED, BAD_POLICY, BAD_TABLE, BAD_INDEX = 0, 1, 2, 3, 4   # include/irlmx.h IRLMX_TRAJ_*

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
SH32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 of ``counter`` [..., 4] under ``key`` [..., 2] (any integer
    arrays of 32-bit values, broadcast against each other): uint64 [..., 4]
    holding the four 32-bit output words."""
    c = np.asarray(counter).astype(np.uint64) & MASK
    k = np.asarray(key).astype(np.uint64) & MASK
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                 # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> SH32) ^ c1 ^ k0, p1 & MASK, (p0 >> SH32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def uniforms(x):
    """``(u_action, u_next)`` of output words x [..., 4]: 53 bits each, in [0, 1)."""
    x = np.asarray(x, dtype=np.uint64)
    f = lambda lo, hi: ((hi >> np.uint64(5)).astype(np.float64) * 67108864.0
                        + (lo >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53
    return f(x[..., 0], x[..., 1]), f(x[..., 2], x[..., 3])


def split_seed(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def instance_seeds(seed, batch):
    """ops.rollout's rule for an int seed: ``(s & 0xffffffff) | (b << 32)``."""
    return [(int(seed) & 0xFFFFFFFF) | (b << 32) for b in range(batch)]


def pick(u, w):
    """The pick rule for m rows at once: u [m], w [m, n] -> index [m], -1 for an
    invalid row.  Running sums by elementwise adds in index order."""
    u, w = np.asarray(u, dtype=np.float64), np.asarray(w, dtype=np.float64)
    m, n = w.shape
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.zeros(m)
        sums = []
        for j in range(n):
            c = c + w[:, j]
            sums.append(c)
        total = c
        bad = (w < 0).any(axis=1) | np.isnan(w).any(axis=1) | ~(total > 0) | np.isinf(total)
        x = u * total
        below = x[:, None] < np.stack(sums, axis=1)
        first = below.argmax(axis=1)
        positive = w > 0
        last = n - 1 - positive[:, ::-1].argmax(axis=1)
    out = np.where(below.any(axis=1), first, last)
    out[bad] = -1
    return out


def stencil_targets(W, H):
    """[5, S] target of each stencil slot (self, +x, -x, +y, -y); an off-grid slot
    names the state itself (its weight is 0)."""
    s = np.arange(W * H)
    x, y = s % W, s // W
    return np.stack([s, np.where(x + 1 < W, s + 1, s), np.where(x > 0, s - 1, s),
                     np.where(y + 1 < H, s + W, s), np.where(y > 0, s - W, s)])


def rollout(targets, row_val, pi, terminal, start, seed, max_len):
    """One instance: ``targets`` [K, S] ints, ``row_val`` [A, K, S], ``pi`` [S, A],
    ``terminal`` a bool [S] mask, ``start`` [N] ints, ``seed`` a 64-bit int.
    Returns a dict: visits, starts [S] int64; lengths, status [N] int32; states
    [N, max_len + 1], actions [N, max_len] int32, -1 where nothing is written."""
    targets, row_val, pi = np.asarray(targets), np.asarray(row_val, dtype=np.float64), np.asarray(pi, dtype=np.float64)
    terminal = np.asarray(terminal, dtype=bool)
    start = np.asarray(start, dtype=np.int64)
    S, N = pi.shape[0], start.size
    key = np.array(split_seed(seed), dtype=np.uint64)
    visits, starts = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    lengths, status = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    states = np.full((N, max_len + 1), -1, dtype=np.int32)
    actions = np.full((N, max_len), -1, dtype=np.int32)
    valid = (start >= 0) & (start < S)
    status[~valid] = BAD_INDEX
    state = np.where(valid, start, 0)
    np.add.at(starts, state[valid], 1)
    states[valid, 0] = state[valid]
    alive = valid & ~terminal[state]
    status[alive] = TRUNCATED
    for t in range(max_len):
        idx = np.flatnonzero(alive)
        if idx.size == 0:
            break
        s = state[idx]
        np.add.at(visits, s, 1)
        ctr = np.stack([np.full(idx.size, t), idx, np.zeros_like(idx), np.zeros_like(idx)], axis=1)
        u_action, u_next = uniforms(philox4x32_10(ctr, key))
        a = pick(u_action, pi[s])
        stop = a < 0
        status[idx[stop]], alive[idx[stop]] = BAD_POLICY, False
        idx, s, a, u_next = idx[~stop], s[~stop], a[~stop], u_next[~stop]
        k = pick(u_next, row_val[a, :, s])                            # [m, K]
        nxt = targets[np.maximum(k, 0), s]
        stop = (k < 0) | (nxt < 0) | (nxt >= S)
        status[idx[stop]], alive[idx[stop]] = BAD_TABLE, False
        idx, a, nxt = idx[~stop], a[~stop], nxt[~stop]
        actions[idx, t], states[idx, t + 1] = a, nxt
        lengths[idx] += 1
        state[idx] = nxt
        done = terminal[nxt]
        status[idx[done]], alive[idx[done]] = OK, False
    np.add.at(visits, state[valid], 1)                                # final states (trajectory.py:43)
    return {"visits": visits, "starts": starts, "lengths": lengths, "status": status, "states": states,
            "actions": actions}


def _readable(states, actions, length, S, A):
    L = states.size - 1
    if not 0 <= length <= L:
        return False
    st = states[:length + 1]
    ok = bool(((st >= 0) & (st < S)).all())
    if actions is not None:
        ac = actions[:length]
        ok = ok and bool(((ac >= 0) & (ac < A)).all())
    return ok


def statistics(n_states, states, lengths):
    """``(visits [S], starts [S], status [N])`` of one instance's stored
    trajectories: states [N, L + 1] of which 0..lengths[n] count."""
    states, lengths = np.asarray(states), np.asarray(lengths)
    visits, starts = np.zeros(n_states, dtype=np.int64), np.zeros(n_states, dtype=np.int64)
    status = np.zeros(lengths.size, dtype=np.int32)
    for n, length in enumerate(lengths):
        if not _readable(states[n], None, int(length), n_states, 0):
            status[n] = BAD_INDEX
            continue
        starts[states[n, 0]] += 1
        np.add.at(visits, states[n, :length + 1], 1)
    return visits, starts, status


def log_likelihood(pi, states, actions, lengths):
    """``(ll, ll_traj [N], status [N])`` of one instance: numpy's log as
    maxent_oracle.numpy_log_restated computes it, every sum sequential from 0."""
    import maxent_oracle as O
    pi = np.asarray(pi, dtype=np.float64)
    S, A = pi.shape
    states, actions, lengths = np.asarray(states), np.asarray(actions), np.asarray(lengths)
    ll_traj = np.zeros(lengths.size)
    status = np.zeros(lengths.size, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for n, length in enumerate(lengths):
            length = int(length)
            if not _readable(states[n], actions[n] if actions.shape[1] else actions[n][:0], length, S, A):
                status[n], ll_traj[n] = BAD_INDEX, np.nan
                continue
            logs = O.numpy_log_restated(pi[states[n, :length], actions[n, :length]])
            ll_traj[n] = np.add.accumulate(np.concatenate([[0.0], logs]))[-1]
        ll = np.add.accumulate(np.concatenate([[0.0], ll_traj]))[-1]
    return ll, ll_traj, status


def pack(traj_flat, traj_lens):
    """The fixtures' packed trajectories (rows (s, a, s')) as ``(states [N, L + 1],
    actions [N, L], lengths [N])`` int32 with -1 padding, L the longest length."""
    traj_flat, traj_lens = np.asarray(traj_flat), np.asarray(traj_lens)
    N, L = traj_lens.size, int(traj_lens.max())
    states = np.full((N, L + 1), -1, dtype=np.int32)
    actions = np.full((N, L), -1, dtype=np.int32)
    o = 0
    for n, k in enumerate(traj_lens):
        rows = traj_flat[o:o + k]
        states[n, :k], states[n, k], actions[n, :k] = rows[:, 0], rows[-1, 2], rows[:, 1]
        o += k
    return states, actions, traj_lens.astype(np.int32)
