"""CPU twin and longdouble restatement of the finite-horizon soft value
iteration (irlmx_soft_backward_horizon), and the inputs of its tests (not a
test module).  Models and cases come from tests/horizon_twin.py.

include/irlmx.h states the pass statement by statement; this module restates it
three times:

* :func:`backward` -- the float64 twin in that order: per action the slots
  accumulate in slot order over every stored slot (zero-weight ones included),
  ``q = r + discount * acc``, ``v = q_0`` then the pairwise ``softmax2`` fold,
  ``pi = exp(q - v)``, terminals hold ``V = r``.  numpy has no fused
  multiply-add, so the twin rounds each product and each sum separately where
  the kernels use ``fma``: two correct float64 evaluations, never compared bit
  for bit.  ``second=True`` is another correct float64 evaluation -- the slots
  in reverse order and a one-shot max-subtracted log-sum-exp -- that the bound
  must admit (tests/test_soft_horizon_twin.py).
* :func:`backward_ref` -- the same mathematics in ``np.longdouble`` on CSR
  matrices with a max-subtracted log-sum-exp and no attention to order.
* :func:`objective_ref` / :func:`fd_gradient` -- ``p0 . V_0`` in longdouble and
  its central differences in the reward: the gradient identity d(p0 . V_0) /
  d r(s) = D(s), D the visitation of horizon_twin.forward_ref under pi_t.

pi_t is ``exp(q - v)``, so its relative error is the ABSOLUTE error of
``q - v``: it grows with |V| (1e-12 at |V| of about 1,200 on the wide inputs).
"""

import functools

import numpy as np

import extended_ref as X
import horizon_twin as H

LD = np.longdouble
OK, NONFINITE = H.OK, H.NONFINITE
#: the discounts every case runs at
DISCOUNTS = (1.0, 0.9)
#: the launches of tests/test_gpu_soft_horizon.py (issue order)
CASES = ("16x16", "37x23", "64x20", "64x64", "128x40", "64x12-stay", "16x16-T1", "k5-s200", "k8-s1029", "k16-s1029",
         "k32-s200", "k40-s300", "hub-s200", "wide-64x4", "wide-256x4")


def _softmax2(x1, x2):
    hi = np.maximum(x1, x2)
    lo = np.minimum(x1, x2)
    return hi + np.log(1.0 + np.exp(lo - hi))               # maxent.py:274-276


def backward(mod, terminal, reward, discount, T, second=False):
    """``(pi_t [T, S, A], V_0 [S], status)`` in float64."""
    rv, nbr = mod.rv, mod.nbr
    A, K, S = rv.shape
    r = np.asarray(reward, dtype=np.float64)
    g = np.float64(discount)
    tm = H._mask(terminal, S)
    V = r.copy()
    pi = np.empty((T, S, A))
    slots = range(K - 1, -1, -1) if second else range(K)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            Vn = V[nbr]
            q = np.empty((S, A))
            for a in range(A):
                acc = np.zeros(S)
                for k in slots:
                    acc = rv[a, k] * Vn[k] + acc
                q[:, a] = r + g * acc
            if second:
                hi = q.max(axis=1)
                v = hi + np.log(np.exp(q - hi[:, None]).sum(axis=1))
            else:
                v = q[:, 0]
                for a in range(1, A):
                    v = _softmax2(v, q[:, a])
            pi[t] = np.exp(q - v[:, None])
            V = np.where(tm, r, v)
    return pi, V, (OK if np.isfinite(V).all() else NONFINITE)


def backward_ref(mats, terminal, reward, discount, T, policy=True):
    """``(pi_t [T, S, A] or None, V_0 [S])`` in longdouble; ``reward`` may be
    longdouble already (the central differences perturb it there)."""
    p = X._ld_mats(mats)
    S = p[0].shape[0]
    r = np.asarray(reward, dtype=LD)
    g = LD(np.float64(discount))
    tm = H._mask(terminal, S)
    V = r.copy()
    pi = np.empty((T, S, len(p)), dtype=LD) if policy else None
    for t in range(T - 1, -1, -1):
        q = np.stack([r + g * m.dot(V) for m in p], axis=1)
        hi = q.max(axis=1)
        v = hi + np.log(np.exp(q - hi[:, None]).sum(axis=1))
        if policy:
            pi[t] = np.exp(q - v[:, None])
        V = np.where(tm, r, v)
    return pi, V


def objective_ref(mats, terminal, reward, p0, T):
    """``p0 . V_0`` at discount 1 in longdouble."""
    return (np.asarray(p0, dtype=LD) * backward_ref(mats, terminal, reward, 1.0, T, policy=False)[1]).sum()


def fd_gradient(mats, terminal, reward, p0, T, h, states):
    """Central differences of :func:`objective_ref` in ``r(s)`` for ``s`` in ``states``, in longdouble."""
    out = np.empty(len(states), dtype=LD)
    r = np.asarray(reward, dtype=np.float64).astype(LD)
    for i, s in enumerate(states):
        up, dn = r.copy(), r.copy()
        up[s] += LD(h)
        dn[s] -= LD(h)
        out[i] = (objective_ref(mats, terminal, up, p0, T) - objective_ref(mats, terminal, dn, p0, T)) / (2 * LD(h))
    return out


def visitation_ref(mats, terminal, reward, p0, T):
    """D [S] in longdouble: horizon_twin.forward_ref under the longdouble pi_t at
    discount 1 (forward_ref takes pi_t rounded to float64: 2^-53 per factor)."""
    pi, _ = backward_ref(mats, terminal, reward, 1.0, T)
    return H.forward_ref(mats, p0, terminal, pi.astype(np.float64))[0]


def gradient_states(c):
    """The states the gradient identity is checked at: every 37th and the terminals."""
    return sorted(set(range(0, c.S, 37)) | set(c.terminal))


# ---------------------------------------------------------------------------
# per case, discount and instance: computed once, frozen
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def twin(name, discount, b, second=False):
    c = H.case(name)
    pi, v0, status = backward(c.model(b), c.terminal, c.reward[b], discount, c.T, second=second)
    H._frozen(pi, v0)
    return pi, v0, status


@functools.lru_cache(maxsize=None)
def ref(name, discount, b):
    c = H.case(name)
    out = backward_ref(c.model(b).mats, c.terminal, c.reward[b], discount, c.T)
    H._frozen(*out)
    return out


def errors(pi, v0, name, discount, b):
    """(elementwise error of pi_t, normwise error of V_0) against the longdouble restatement."""
    rpi, rv0 = ref(name, discount, b)
    return X.elementwise_err(pi, rpi), X.normwise_err(v0, rv0)


def e_twin(name, discount, b):
    pi, v0, _ = twin(name, discount, b)
    return errors(pi, v0, name, discount, b)


def bounds(name, discount, b):
    """(bound on pi_t elementwise, bound on V_0 normwise): 16 x max(e_twin, e_floor)."""
    c = H.case(name)
    e_pi, e_v0 = e_twin(name, discount, b)
    return X.bound(e_pi, c.K, c.A), X.bound(e_v0, c.K, c.A)
