"""Inputs and CPU references of the elementwise-accuracy tests (not a test module).

tests/test_gpu_elementwise.py runs every kernel family on these inputs;
tests/test_extended_ref.py runs the extended reference (oracle/extended_ref.py)
on the same inputs without a GPU, so an input that leaves the reference's
guards (longdouble overflow of the unscaled backward, a surviving soft-VI start
value) fails in the CPU suite before a GPU run.  Everything is seeded; the
references are computed once per input and shared (functools.lru_cache; the
arrays are set read-only).
"""

import functools

import numpy as np

import extended_ref as X
import maxent_oracle as O
from conftest import icy_stencil_rect

SLIPS = (0.1, 0.2, 0.35)
#: reward ranges of the three instances of one launch: partition sums that grow
#: by ~7x, by ~e per sweep and one with a wide spread, so the instances of one
#: launch rescale by different amounts
RANGES = ((0.0, 1.0), (-6.0, 1.0), (-1.2, -0.4))
#: at width 256 (256 x 12: S = 3,072, 6,144 backward sweeps) the unscaled reference
#: must stay inside longdouble's exponent range, |ln(growth per sweep)| * 6,144 <
#: 11,356, i.e. a growth per sweep within e^(+-1.8): the ranges are shifted down
#: (growth ~e^1.0, a spread, and decay ~e^-0.8: one instance still rescales up and
#: another down).  The spread is [-4, 0]: at [-7, 0] with the stay action the
#: partition vector itself spans 1e328 along the 256 columns, more than float64
#: holds under any common scale -- the far states underflow to 0 and their policy
#: rows are 0 / 0 in the oracle and the kernels alike (DESIGN.md section 2,
#: "Elementwise accuracy"), which is a limit of float64, not an accuracy question
RANGES_W256 = ((-1.0, 0.0), (-4.0, 0.0), (-2.6, -1.8))

#: discount of the ELL and dense soft-VI / VI cases (converged in ~2,000 sweeps)
ELL_DISCOUNT = 0.8
#: of the dense cases (17 instances on the GEMM plan: ~700 sweeps each)
DENSE_DISCOUNT = 0.5

OK, MAXITER = 0, 2   # include/irlmx.h status codes


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


class Case:
    """One model with B instances: per-instance operands of the extended
    reference (``mats[b]``) and of the float64 oracle (CSR matrices or a dense
    table), rewards, initial distributions, terminals."""

    def __init__(self, name, mats, tables, reward, p0, terminal, k_row, n_actions):
        self.name, self.mats, self.tables = name, mats, tables
        self.reward, self.p0, self.terminal = reward, p0, list(terminal)
        self.k_row, self.A = int(k_row), int(n_actions)
        self.B, self.S = reward.shape
        self.phi = O.terminal_reward(self.terminal, self.S)
        _freeze(self.reward, self.p0, self.phi)
        self._cache = {}

    def floor(self):
        return X.e_floor(self.k_row, self.A)

    def _memo(self, key, fn):
        if key not in self._cache:
            out = fn()
            _freeze(*[a for a in out if isinstance(a, np.ndarray)])
            self._cache[key] = out
        return self._cache[key]

    # -- the float64 oracle (oracle/maxent_oracle.py) and the extended reference
    #    on the same input and sweep count -----------------------------------

    def backward(self, b):
        """(oracle pi, extended pi)"""
        def run():
            if self.tables is None:
                o = O.backward_maxent_csr(self.mats[b], self.terminal, self.reward[b])
            else:
                o = O.backward_maxent(self.tables[b], self.terminal, self.reward[b], rescale=True)
            return o, X.backward(self.mats[b], self.terminal, self.reward[b])
        return self._memo(("bwd", b), run)

    def _oracle_forward(self, b, pi, cap):
        if self.tables is None:
            return O.forward_svf_csr(self.mats[b], self.p0[b], self.terminal, pi, max_iter=cap)
        return O.forward_svf(self.tables[b], self.p0[b], self.terminal, pi, max_iter=cap)

    def forward(self, b, cap):
        """(oracle svf, sweeps, status, extended svf) on the oracle's policy"""
        def run():
            pi = self.backward(b)[0]
            d, k = self._oracle_forward(b, pi, cap)
            status = OK
            if k == cap:   # stopped by the cap unless that very sweep converged (maxent.py:108)
                prev = self._oracle_forward(b, pi, cap - 1)[0] if cap > 1 else np.zeros(self.S)
                status = OK if np.max(np.abs(d - prev)) <= 1e-5 else MAXITER
            return d, k, status, X.forward(self.mats[b], self.p0[b], self.terminal, pi, k)
        return self._memo(("fwd", b, cap), run)

    def soft(self, b, discount):
        """(oracle pi, oracle v, sweeps, extended pi, extended v), converged"""
        def run():
            if self.tables is None:
                pi, v, k = O.soft_backward_csr(self.mats[b], self.terminal, self.reward[b], discount)
            else:
                pi, v, k = O.soft_backward(self.tables[b], self.terminal, self.reward[b], discount)
            xpi, xv = X.soft_backward(self.mats[b], self.phi, self.reward[b], discount, k)
            return pi, v, k, xpi, xv
        return self._memo(("soft", b, discount), run)

    def vi(self, b, discount, average):
        """(oracle v, sweeps, extended v), converged"""
        def run():
            if self.tables is None:
                v, k = O.value_iteration_csr(self.mats[b], self.reward[b], discount, average=average)
            else:
                v, k = O.value_iteration(self.tables[b], self.reward[b], discount, average=average)
            return v, k, X.value_iteration(self.mats[b], self.reward[b], discount, k, average)
        return self._memo(("vi", b, discount, average), run)


def _p0(rng, B, S):
    """A delta at state 0 for the first instance, rand**8 normalised for the others."""
    p0 = rng.random((B, S)) ** 8
    p0[0] = 0.0
    p0[0, 0] = 1.0
    return p0 / p0.sum(axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def stencil(W, H, stay=False, B=3, ranges=None, seed=None):
    """B icy gridworlds (slips 0.1 / 0.2 / 0.35) on a W x H grid with two
    terminals; ``stay`` adds the fifth action of DeviceMDP.with_stay().  The
    STENCIL5 row tables are ``case.rv`` [B, 4, 5, S] (without the stay action:
    the device model adds its own)."""
    S = W * H
    rng = np.random.default_rng(1000 * W + H if seed is None else seed)
    if ranges is None:
        ranges = RANGES_W256 if W == 256 else RANGES
    rv = np.stack([icy_stencil_rect(W, H, p) for p in SLIPS[:B]])
    reward = np.stack([rng.uniform(lo, hi, S) for lo, hi in ranges[:B]])
    terminal = [S - 1, (H // 2) * W + W // 3]
    mats = []
    for b in range(B):
        t = rv[b]
        if stay:
            extra = np.zeros((1, 5, S))
            extra[0, 0] = 1.0                                   # P[s, s, 4] = 1
            t = np.concatenate([t, extra])
        mats.append(X.mats_from_stencil(t, W, H))
    case = Case(f"{W}x{H}" + ("+stay" if stay else ""), mats, None, reward, _p0(rng, B, S), terminal, 5,
                5 if stay else 4)
    case.rv, case.W, case.H = rv, W, H
    _freeze(rv)
    return case


@functools.lru_cache(maxsize=None)
def ell(S, B=2, A=3):
    """A seeded random sparse MDP: every state has 3-12 successors (the same set
    for every action, a random distribution per action), one table shared by B
    reward vectors; terminals S - 1 and 2."""
    rng = np.random.default_rng(7000 + S)
    P = np.zeros((S, S, A))
    for s in range(S):
        tg = rng.choice(S, size=int(rng.integers(3, 13)), replace=False)
        w = rng.random((tg.size, A)) + 0.05
        P[s, tg, :] = w / w.sum(axis=0, keepdims=True)
    nz = (P != 0.0).any(axis=2)
    reward = np.stack([rng.uniform(0.0, 1.0, S), rng.uniform(-2.0, 0.5, S)][:B])
    import scipy.sparse as sp
    mats = [[sp.csr_matrix(P[:, :, a]) for a in range(A)]] * B
    case = Case(f"ell{S}", mats, [P] * B, reward, _p0(rng, B, S), [S - 1, 2], int(nz.sum(axis=1).max()), A)
    case.P, case.k_col = P, int(nz.sum(axis=0).max())
    _freeze(P)
    return case


@functools.lru_cache(maxsize=None)
def dense(B=1):
    """O.random_dense_mdp(301, 3, seed=301): S odd, every entry nonzero; one
    table shared by B reward vectors (the first is the generator's own)."""
    P, r, terminal, p0 = O.random_dense_mdp(301, 3, seed=301)
    rng = np.random.default_rng(30100 + B)
    S = P.shape[0]
    reward = np.stack([r] + [rng.uniform(-1.0, 1.0, S) for _ in range(B - 1)])
    p0s = _p0(rng, B, S)
    p0s[0] = p0
    case = Case(f"dense301x{B}", [X.mats_from_table(P)] * B, [P] * B, reward, p0s, terminal, S, 3)
    case.P = P
    _freeze(P)
    return case
