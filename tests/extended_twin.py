"""CPU twin of the extended-range backward pass and the inputs of its tests (not
a test module).

:func:`backward` restates csrc/extended.hip in float64 numpy: every partition
value is ``m * 2**e`` with ``m`` in [0.5, 1) or exactly 0 (``np.frexp``'s form)
and an integer exponent ``e``; one collapsed sweep aligns a state's neighbours
to the largest exponent ``E`` among the slots with a nonzero weight,
accumulates in slot order and splits the sum again.  numpy has no fused
multiply-add, so the twin rounds each product and each sum separately where
the kernels use ``fma``: its policy may differ from theirs in the last bits
(two correct float64 evaluations; the tests bound both against the longdouble
reference, oracle/extended_ref.py, and never compare the twin's bits with the
device's).  The twin also records what makes "bit-identical to the rescaled
pass in range" a theorem: the largest alignment shift and the spread of the
exponents over all sweeps (:class:`Stats`).

Inputs (:func:`wide`): an icy gridworld (slip 0.2) on a W x H grid, terminal
``[S - 1]``, reward ``lo`` everywhere and 0 at state 0, optionally plus
``noise * rng.random(S)`` with ``np.random.default_rng(S)``: the partition
vector spans more than float64's exponent range along the W columns.
"""

import functools

import numpy as np

import extended_ref as X
import maxent_oracle as O
from conftest import icy_stencil_rect

ZERO = np.iinfo(np.int32).min   # exponent of an exact zero (kExtZero)
MIN_SHIFT = -1100               # kExtMinShift


class Stats:
    """Largest alignment shift ``E - e(nb_k)`` over the slots that contribute
    (nonzero weight, nonzero neighbour) and largest spread ``max e - min e``
    over the nonzero states, over all sweeps."""

    def __init__(self):
        self.max_shift = 0
        self.max_spread = 0

    def sweep(self, w, mn, en, E, e_new, m_new):
        live = (w != 0) & (mn != 0)
        if live.any():
            self.max_shift = max(self.max_shift, int((E[None, :] - en)[live].max()))
        nz = m_new != 0
        if nz.any():
            self.max_spread = max(self.max_spread, int(e_new[nz].max() - e_new[nz].min()))


def stencil_nbr(W, H):
    """Neighbour table [5, S] of the STENCIL5 layout (self, +x, -x, +y, -y; a
    slot that leaves the grid points at the state itself: csrc/common.h)."""
    s = np.arange(W * H)
    x, y = s % W, s // W
    return np.stack([s, np.where(x + 1 < W, s + 1, s), np.where(x > 0, s - 1, s),
                     np.where(y + 1 < H, s + W, s), np.where(y > 0, s - W, s)])


def ell_rows(P):
    """ELL row form of a dense [S, S, A] table as irlmx_dense_to_ell lays it out:
    the targets of each state (union over actions) ascending, unused slots at
    the state itself with value 0.  Returns (row_val [A, K, S], nbr [K, S])."""
    S, _, A = P.shape
    nz = (P != 0).any(axis=2)
    K = max(1, int(nz.sum(axis=1).max()))
    nbr = np.tile(np.arange(S), (K, 1))
    rv = np.zeros((A, K, S))
    for s in range(S):
        t = np.flatnonzero(nz[s])
        nbr[:t.size, s] = t
        rv[:, :t.size, s] = P[s, t, :].T
    return rv, nbr


def _aligned(mn, en, E):
    sh = np.clip(en.astype(np.int64) - E.astype(np.int64), MIN_SHIFT, 0).astype(np.int32)
    return np.ldexp(mn, sh)


def _split(acc, E):
    m, d = np.frexp(acc)
    e = np.where(acc == 0, ZERO, E.astype(np.int64) + d)
    return m, e


def backward(row_val, nbr, terminal, reward, stats=None):
    """Policy [S, A] of the extended-range pass: ``row_val`` [A, K, S],
    ``nbr`` [K, S] (target of slot k of state s), 2 * S sweeps."""
    rv = np.asarray(row_val, dtype=np.float64)
    A, K, S = rv.shape
    er = np.exp(np.asarray(reward, dtype=np.float64))
    tot = np.zeros((K, S))
    for a in range(A):                       # bwd_weights_kernel: the action sum in action order
        tot = tot + rv[a]
    w = er[None, :] * tot
    m = np.zeros(S)
    e = np.full(S, ZERO, dtype=np.int64)
    m[terminal] = 0.5                        # 1 = 0.5 * 2^1
    e[terminal] = 1
    with np.errstate(under="ignore"):
        for _ in range(2 * S - 1):
            mn, en = m[nbr], e[nbr]
            E = np.where(w != 0, en, ZERO).max(axis=0)
            z = _aligned(mn, en, E[None, :])
            acc = np.zeros(S)
            for k in range(K):
                acc = w[k] * z[k] + acc
            m_new, e_new = _split(acc, E)
            if stats is not None:
                stats.sweep(w, mn, en, E, e_new, m_new)
            m, e = m_new, e_new
        mn, en = m[nbr], e[nbr]
        E = np.where((rv != 0).any(axis=0), en, ZERO).max(axis=0)
        z = _aligned(mn, en, E[None, :])
        za = np.zeros((S, A))
        zsum = np.zeros(S)
        for a in range(A):
            acc = np.zeros(S)
            for k in range(K):
                acc = rv[a, k] * z[k] + acc
            za[:, a] = er * acc
            zsum = zsum + za[:, a]
    with np.errstate(invalid="ignore", divide="ignore"):
        return za / zsum[:, None]


class Wide:
    """One wide-range input with its references, each computed once."""

    def __init__(self, W, H, lo, noise=0.0):
        self.W, self.H, self.S = W, H, W * H
        self.rv = icy_stencil_rect(W, H, 0.2)
        self.nbr = stencil_nbr(W, H)
        r = np.full(self.S, float(lo))
        r[0] = 0.0
        if noise:
            r = r + noise * np.random.default_rng(self.S).random(self.S)
        self.reward = r
        self.terminal = [self.S - 1]
        self.mats = X.mats_from_stencil(self.rv, W, H)
        for a in (self.rv, self.nbr, self.reward):
            a.setflags(write=False)

    @functools.cached_property
    def ref(self):
        """The longdouble reference's policy (raises if it leaves its guards)."""
        out = X.backward(self.mats, self.terminal, self.reward)
        out.setflags(write=False)
        return out

    @functools.cached_property
    def oracle(self):
        """The rescaled float64 oracle: one common scale, as the ordinary kernels."""
        with np.errstate(all="ignore"):
            out = O.backward_maxent_csr(self.mats, self.terminal, self.reward)
        out.setflags(write=False)
        return out

    @functools.cached_property
    def twin(self):
        out = backward(self.rv, self.nbr, self.terminal, self.reward)
        out.setflags(write=False)
        return out

    @functools.cached_property
    def e_twin(self):
        return X.elementwise_err(self.twin, self.ref)

    def bound(self):
        """The project's rule with the twin in the oracle's place: 16 x max(e_twin, e_floor)."""
        return X.bound(self.e_twin, 5, 4)


@functools.lru_cache(maxsize=None)
def wide(W, H, lo, noise=0.0):
    return Wide(W, H, lo, noise)


#: (W, H, lo, noise) of the CPU test and of the GPU tests' launches
WIDE_INPUTS = ((64, 4, -15.0, 0.0), (64, 4, -12.0, 2.0), (128, 4, -7.0, 0.0), (256, 4, -4.0, 0.0))


def nan_rows(pi):
    return int(np.isnan(np.asarray(pi)).any(axis=-1).sum())
