"""MI355X drop-in for the reference module ``maxent`` (narendasan/irl-maxent, src/maxent.py).

Same public names, signatures, defaults and return types (float64 numpy
arrays) as the reference, so ``src/main.py`` runs unchanged with this
directory ahead of ``src/`` on ``sys.path``.  The fixed-point loops run on the
GPU through libirlmx.so (``irlmx.ops``); only the demonstration statistics,
the feature products and the user's optimizer stay on the host, as in the
reference's outer loop.

The backward passes run in numpy's own floating-point order when the model
allows it (S % 4 in {0, 1}: every square grid; by default up to 1024 states for
the backward and forward, 4096 for soft VI, 64 on a DENSE table --
ops.numpy_order_default): the non-causal
policy (local_action_probabilities, and the backward half of
compute_expected_svf / irl) is then bit-identical to the reference's on a
Haswell-family OpenBLAS host, and the soft VI's dot products follow numpy's
order (ops.*_numpy_order; IRLMX_NUMPY_ORDER=0 turns it off).
Above 625 states that is the reference run with one BLAS thread
(OPENBLAS_NUM_THREADS=1): numpy's multi-threaded OpenBLAS partitions the rows
differently there and its own last bits move with the thread count.

Deliberate differences (documented in DESIGN.md):
* Where the reference's backward pass overflows to NaN (about 13x13 at unit
  reward) the drop-in reruns it with its partition vector rescaled by powers
  of two (ratio-exact), so the policy stays finite.
  ``IRLMX_REFERENCE_OVERFLOW=1`` keeps the reference's NaN instead.
* ``p_transition`` may also be an ``irlmx.DeviceMDP`` already resident in HBM.
* ``IRLMX_EXTENDED_RANGE=1``: wherever the backward would take the rescaled
  tiled pass, it runs with one exponent per state instead
  (``ops.backward_maxent_extended``), so the policy stays finite and right
  where the partition vector spans more than float64's exponent range (the
  rescaled pass keeps one scale per instance: NaN rows, and wrong finite rows
  beside them).  The numpy-order attempt and ``IRLMX_REFERENCE_OVERFLOW=1``
  keep precedence; unset, nothing changes.  DENSE tables are not covered.
  One workgroup up to 4096 states, one persistent launch from 8192 states on
  (a 256 x 256 grid: 131,072 sweeps in one launch), one launch per sweep in
  between (``ops.backward_maxent_extended``).

Beyond the reference: ``local_action_probabilities_horizon``,
``compute_expected_svf_horizon`` and ``irl_horizon`` are the finite-horizon
form of the same model (``ops.backward_maxent_horizon``,
``ops.forward_svf_horizon``), for worlds without a terminal state
(``terminal=[]``) and demonstrations of a fixed length;
``local_causal_action_probabilities_horizon``,
``compute_expected_causal_svf_horizon`` and ``irl_causal_horizon`` are its
MaxCausalEnt counterpart for stochastic dynamics (``ops.soft_backward_horizon``:
the soft Bellman recursion over T steps, no terminal set or discount below 1
needed).
"""

import os
from itertools import chain

import numpy as np
import torch

from irlmx import DeviceMDP, ops

__all__ = ["feature_expectation_from_trajectories", "initial_probabilities_from_trajectories",
           "expected_svf_from_policy", "local_action_probabilities", "compute_expected_svf",
           "expected_svf", "irl", "softmax", "local_causal_action_probabilities",
           "compute_expected_causal_svf", "irl_causal", "local_action_probabilities_horizon",
           "compute_expected_svf_horizon", "irl_horizon", "local_causal_action_probabilities_horizon",
           "compute_expected_causal_svf_horizon", "irl_causal_horizon"]


def _rescale():
    return os.environ.get("IRLMX_REFERENCE_OVERFLOW", "0") != "1"


def _extended():
    return os.environ.get("IRLMX_EXTENDED_RANGE", "0") == "1"


def _model(p_transition):
    """The device model of ``p_transition`` (uploaded once per array, see
    DeviceMDP.resident; the reference re-copies it per call, maxent.py:98-102, 143, 320)."""
    if isinstance(p_transition, DeviceMDP):
        return p_transition
    return DeviceMDP.resident(p_transition)


def _host(t):
    return t[0].detach().cpu().numpy()


def _fdot(features, x, ident, transpose=False):
    # identity features: F.x == x bit for bit while x is finite (0 * finite adds
    # exact zeros); a non-finite x takes the real product so NaN spreads as in numpy
    if ident and np.isfinite(x).all():
        return x.copy()
    return features.T.dot(x) if transpose else features.dot(x)


def _is_identity(features):
    n, f = features.shape
    if n != f:
        return False
    return bool(np.all(np.diagonal(features) == 1.0)) and int(np.count_nonzero(features)) == n


# -- demonstration statistics (host, once per IRL run) -------------------------

def feature_expectation_from_trajectories(features, trajectories):
    """Average feature vector over all visited states, final states included (maxent.py:15-39)."""
    n_states, n_features = features.shape
    visited = np.fromiter(chain.from_iterable(t.states() for t in trajectories), dtype=np.int64)
    if np.array_equal(features, np.round(features)):
        # integer-valued features: visit counts times features is exact, so the
        # result equals the reference's sequential sum bit for bit
        counts = np.bincount(visited, minlength=n_states).astype(np.float64)
        fe = counts.dot(features)
    else:
        fe = np.zeros(n_features)
        for s in visited:
            fe += features[s, :]
    return fe / len(trajectories)


def initial_probabilities_from_trajectories(n_states, trajectories):
    """Fraction of trajectories starting in each state (maxent.py:42-60)."""
    p = np.zeros(n_states)
    for t in trajectories:
        p[t.transitions()[0][0]] += 1.0
    return p / len(trajectories)


# -- plain MaxEnt (Ziebart et al. 2008) -----------------------------------------

def expected_svf_from_policy(p_transition, p_initial, terminal, p_action, eps=1e-5):
    """Expected state visitation frequencies under ``p_action`` (maxent.py:63-114)."""
    mdp = _model(p_transition)
    term = ops.terminal_mask(terminal, mdp.n_states, device=mdp.device)
    svf, _, _ = _forward(mdp, p_initial, term, p_action, eps)
    return _host(svf)


def _np_order(mdp, op="backward"):
    """numpy's own summation order for this call: one instance of a model the
    numpy-order kernels cover, up to a per-op state count (backward / forward
    1024, soft VI 4096; 64 on a DENSE table) -- ops.numpy_order_default states
    the caps, their measured cost and the environment overrides
    (IRLMX_NUMPY_ORDER=0 turns it off)."""
    return ops.numpy_order_default(mdp, op)


def _forward(mdp, p_initial, term, pi, eps):
    return ops.forward_svf(mdp, p_initial, term, pi, eps, numpy_order=_np_order(mdp, "forward"))


def _backward(mdp, reward, term):
    """The backward policy on the device: numpy's order where the model allows it
    (bit-identical to the reference), the rescaled pass where that overflows
    (the numpy-order kernel stops at the overflow, so the detour costs the sweeps
    up to it: a few hundred at unit reward)."""
    reward = np.asarray(reward.cpu().numpy() if torch.is_tensor(reward) else reward, dtype=np.float64)
    if _np_order(mdp):
        pi = ops.backward_maxent_numpy_order(mdp, np.exp(reward), term)   # er = np.exp(reward), maxent.py:142
        if not _rescale() or bool(torch.isfinite(pi).all()):
            return pi
    if _extended() and _rescale():
        return ops.backward_maxent_extended(mdp, reward, term)
    return ops.backward_maxent(mdp, reward, term, rescale=_rescale())


def local_action_probabilities(p_transition, terminal, reward):
    """Backward pass of MaxEnt IRL, 2*S sweeps (maxent.py:119-159)."""
    mdp = _model(p_transition)
    term = ops.terminal_mask(terminal, mdp.n_states, device=mdp.device)
    return _host(_backward(mdp, reward, term))


def compute_expected_svf(p_transition, p_initial, terminal, reward, eps=1e-5):
    """Backward pass then forward pass (maxent.py:162-193)."""
    mdp = _model(p_transition)
    term = ops.terminal_mask(terminal, mdp.n_states, device=mdp.device)
    pi = _backward(mdp, reward, term)
    svf, _, _ = _forward(mdp, p_initial, term, pi, eps)
    return _host(svf)


expected_svf = compute_expected_svf


def _irl_loop(mdp, features, terminal, trajectories, optim, init, eps, svf_fn):
    n_states = mdp.n_states
    _, n_features = features.shape
    e_features = feature_expectation_from_trajectories(features, trajectories)
    p_initial = initial_probabilities_from_trajectories(n_states, trajectories)
    ident = _is_identity(features)
    term = ops.terminal_mask(terminal, n_states, device=mdp.device)
    p0 = torch.as_tensor(p_initial, device=mdp.device)

    theta = init(n_features)
    delta = np.inf
    optim.reset(theta)                       # theta is aliased and mutated by optim.step
    while delta > eps:
        theta_old = theta.copy()
        reward = _fdot(features, theta, ident)
        e_svf = svf_fn(mdp, reward, term, p0)
        grad = e_features - _fdot(features, e_svf, ident, transpose=True)
        optim.step(grad)
        delta = np.max(np.abs(theta_old - theta))
    return _fdot(features, theta, ident)


def irl(p_transition, features, terminal, trajectories, optim, init, eps=1e-4, eps_esvf=1e-5):
    """MaxEnt IRL by gradient ascent on the demonstration likelihood (maxent.py:196-255).

    The transition model is uploaded once; every gradient step runs the
    backward and forward passes on the device and moves only the reward (H2D)
    and the visitation frequencies (D2H) across PCIe.
    """
    mdp = _model(p_transition)

    def svf_fn(m, reward, term, p0):
        pi = _backward(m, reward, term)
        svf, _, _ = _forward(m, p0, term, pi, eps_esvf)
        return _host(svf)

    return _irl_loop(mdp, features, terminal, trajectories, optim, init, eps, svf_fn)


# -- finite horizon (no reference counterpart) ---------------------------------

def _streamed_svf(mdp, reward, p0, horizon, term, stream_policy, model, discount=1.0):
    """``stream_policy`` (True, or an int segment length) of the horizon drop-ins:
    ``ops.expected_svf_horizon``, the two passes in one call without the policy tensor."""
    segment = 0 if stream_policy is True else int(stream_policy)
    return ops.expected_svf_horizon(mdp, reward, p0, horizon, model=model, discount=discount, terminal=term,
                                    segment=segment)[0]


def _horizon_mask(mdp, terminal):
    """The terminal mask, or None for an empty ``terminal`` (no terminal state)."""
    return ops.terminal_mask(terminal, mdp.n_states, device=mdp.device) if np.size(terminal) else None


def local_action_probabilities_horizon(p_transition, terminal, reward, horizon):
    """Time-indexed local action probabilities [T, S, A] of the finite-horizon
    MaxEnt model with ``T = horizon`` steps (``ops.backward_maxent_horizon``):
    ``terminal`` may be ``[]``.  T * S * A * 8 bytes: 17 MB on a 64x64 grid at
    T = 128."""
    mdp = _model(p_transition)
    return _host(ops.backward_maxent_horizon(mdp, reward, horizon, _horizon_mask(mdp, terminal)))


def compute_expected_svf_horizon(p_transition, p_initial, terminal, reward, horizon, stream_policy=False):
    """Expected state visitation over the T + 1 states of a ``horizon``-step
    trajectory: the finite-horizon backward then forward pass
    (``ops.forward_svf_horizon``).  Sums to T + 1 without terminals.
    ``stream_policy`` (True, or an int segment length): the same bits from
    ``ops.expected_svf_horizon``, without the [T, S, A] policy in memory."""
    mdp = _model(p_transition)
    term = _horizon_mask(mdp, terminal)
    if stream_policy is not False:
        return _host(_streamed_svf(mdp, reward, p_initial, horizon, term, stream_policy, "maxent"))
    pi = ops.backward_maxent_horizon(mdp, reward, horizon, term)
    svf, _, _ = ops.forward_svf_horizon(mdp, p_initial, pi, term)
    return _host(svf)


def irl_horizon(p_transition, features, terminal, trajectories, optim, init, horizon, eps=1e-4, stream_policy=False):
    """MaxEnt IRL with the finite-horizon model: ``irl``'s gradient ascent, the
    expected visitation from ``compute_expected_svf_horizon`` (``stream_policy``
    as there).  For demonstrations of ``horizon`` steps each; ``terminal`` may
    be ``[]``."""
    mdp = _model(p_transition)
    term_h = _horizon_mask(mdp, terminal)

    def svf_fn(m, reward, term, p0):
        if stream_policy is not False:
            return _host(_streamed_svf(m, reward, p0, horizon, term_h, stream_policy, "maxent"))
        pi = ops.backward_maxent_horizon(m, reward, horizon, term_h)
        svf, _, _ = ops.forward_svf_horizon(m, p0, pi, term_h)
        return _host(svf)

    return _irl_loop(mdp, features, terminal, trajectories, optim, init, eps, svf_fn)


def local_causal_action_probabilities_horizon(p_transition, terminal, reward, discount, horizon):
    """Time-indexed policy exp(Q_t - V_t) [T, S, A] of the finite-horizon
    MaxCausalEnt model with ``T = horizon`` steps (``ops.soft_backward_horizon``):
    the model for stochastic dynamics; ``terminal`` may be ``[]`` and
    ``discount`` may be 1."""
    mdp = _model(p_transition)
    return _host(ops.soft_backward_horizon(mdp, reward, discount, horizon, _horizon_mask(mdp, terminal)))


def compute_expected_causal_svf_horizon(p_transition, p_initial, terminal, reward, discount, horizon,
                                        stream_policy=False):
    """Expected state visitation over the T + 1 states of a ``horizon``-step
    trajectory under the finite-horizon MaxCausalEnt policy: the soft Bellman
    recursion, then ``ops.forward_svf_horizon``.  ``stream_policy`` (True, or
    an int segment length): the same bits from ``ops.expected_svf_horizon``,
    without the [T, S, A] policy in memory."""
    mdp = _model(p_transition)
    term = _horizon_mask(mdp, terminal)
    if stream_policy is not False:
        return _host(_streamed_svf(mdp, reward, p_initial, horizon, term, stream_policy, "causal", discount))
    pi = ops.soft_backward_horizon(mdp, reward, discount, horizon, term)
    svf, _, _ = ops.forward_svf_horizon(mdp, p_initial, pi, term)
    return _host(svf)


def irl_causal_horizon(p_transition, features, terminal, trajectories, optim, init, discount, horizon, eps=1e-4,
                       stream_policy=False):
    """MaxCausalEnt IRL with the finite-horizon model: ``irl_causal``'s gradient
    ascent, the expected visitation from ``compute_expected_causal_svf_horizon``
    (the exact gradient of the demonstrations' likelihood; ``stream_policy`` as
    there).  For demonstrations of ``horizon`` steps each; ``terminal`` may be
    ``[]``."""
    mdp = _model(p_transition)
    term_h = _horizon_mask(mdp, terminal)

    def svf_fn(m, reward, term, p0):
        if stream_policy is not False:
            return _host(_streamed_svf(m, reward, p0, horizon, term_h, stream_policy, "causal", discount))
        pi = ops.soft_backward_horizon(m, reward, discount, horizon, term_h)
        svf, _, _ = ops.forward_svf_horizon(m, p0, pi, term_h)
        return _host(svf)

    return _irl_loop(mdp, features, terminal, trajectories, optim, init, eps, svf_fn)


# -- maximum causal entropy (Ziebart 2010) -------------------------------------

def softmax(x1, x2):
    """Elementwise soft maximum max + log(1 + exp(min - max)) (maxent.py:260-276)."""
    x_max = np.maximum(x1, x2)
    x_min = np.minimum(x1, x2)
    return x_max + np.log(1.0 + np.exp(x_min - x_max))


def _terminal_reward(terminal, n_states):
    # maxent.py:313-317: a full-length `terminal` is the terminal reward itself
    if len(terminal) == n_states:
        return np.array(terminal, dtype=float)
    phi = -np.inf * np.ones(n_states)
    phi[terminal] = 0.0
    return phi


def local_causal_action_probabilities(p_transition, terminal, reward, discount, eps=1e-5):
    """Soft value iteration of MaxCausalEnt IRL; returns exp(Q - V) (maxent.py:279-341)."""
    mdp = _model(p_transition)
    phi = _terminal_reward(terminal, mdp.n_states)
    pi, _, _, _ = ops.soft_backward(mdp, reward, phi, discount, eps, numpy_order=_np_order(mdp, "soft_backward"))
    return _host(pi)


def compute_expected_causal_svf(p_transition, p_initial, terminal, reward, discount,
                                eps_lap=1e-5, eps_svf=1e-5):
    """Soft value iteration then forward pass (maxent.py:344-380)."""
    mdp = _model(p_transition)
    phi = _terminal_reward(terminal, mdp.n_states)
    pi, _, _, _ = ops.soft_backward(mdp, reward, phi, discount, eps_lap, numpy_order=_np_order(mdp, "soft_backward"))
    term = ops.terminal_mask(terminal, mdp.n_states, device=mdp.device)
    svf, _, _ = _forward(mdp, p_initial, term, pi, eps_svf)
    return _host(svf)


def irl_causal(p_transition, features, terminal, trajectories, optim, init, discount,
               eps=1e-4, eps_svf=1e-5, eps_lap=1e-5):
    """MaxCausalEnt IRL by gradient ascent (maxent.py:383-453)."""
    mdp = _model(p_transition)
    phi = torch.as_tensor(_terminal_reward(terminal, mdp.n_states), device=mdp.device)

    def svf_fn(m, reward, term, p0):
        pi, _, _, _ = ops.soft_backward(m, reward, phi, discount, eps_lap, numpy_order=_np_order(m, "soft_backward"))
        svf, _, _ = _forward(m, p0, term, pi, eps_svf)
        return _host(svf)

    return _irl_loop(mdp, features, terminal, trajectories, optim, init, eps, svf_fn)
