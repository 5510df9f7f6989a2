"""Batched MaxEnt / MaxCausalEnt IRL: B independent gridworld instances per device call.

One ``step()`` is one gradient step of ``maxent.irl`` (maxent.py:240-252) or
``maxent.irl_causal`` (maxent.py:437-450) for every still-active instance at
once, entirely on the device:

    reward = F . theta                       (maxent.py:244 / 441)
    pi     = backward(reward)                (maxent.py:119-159, 2*S sweeps; causal:
                                              soft VI maxent.py:279-341)
    svf    = forward(p0, pi)                 (maxent.py:63-114, until max|dd| <= eps)
    grad   = e_features - F^T . svf          (maxent.py:248 / 445)
    theta  = optimizer(theta, grad, k)       (default ExpSga + linear_decay, optimizer.py:154-167,
                                              217-240; any of irlmx.optim's Sga, ExpSga,
                                              NormalizeGrad with the reference's schedules)

``F`` is the identity (``features=None``, the configs' case: reward = theta),
one ``[S, F]`` matrix shared by all instances, or ``[B, S, F]``.  ``run()``
repeats steps until every instance has met the reference's stopping rule
``max|theta_old - theta| <= eps`` (a NaN delta stops, as ``while NaN > eps``
does); a stopped instance's theta is frozen, so each instance ends exactly
where its own reference loop would.

Compaction (``run(compact=True)``, the default): once an instance has
stopped, the following steps run only the still-active instances -- their
tables, demonstration statistics and theta are gathered into a smaller batch
(``DeviceMDP.take``) and the kernels re-plan for it (fewer instances: more
CUs per instance) -- so a stopped instance no longer pays its 2*S backward
sweeps and its forward pass every step.  Per-instance results do not depend on
the batch they run in (every kernel shape and plan performs the same float64
operations in the same order per instance), so a compacted run equals an
uncompacted one bit for bit with identity features on the STENCIL5 and ELL
layouts (tests/test_gpu_full_run.py).  Two exceptions change rounding, not
results beyond it: with a feature matrix the F . theta / F^T . svf products are
torch GEMMs whose summation order may change with the batch size, and on the
DENSE layout the planner picks the GEMM or streaming kernel, the GEMM's
split-K waves and the dense-grid row blocking from the working batch, each with
its own per-row summation order (tested to 1e-9 against the uncompacted run).

No host round trip happens inside a step except the forward pass's own
convergence polling on the per-sweep shape -- and, with
``extended_range="auto"``, one device reduction and one host read per step
(which instances hold a NaN or an exact 0 in their policy).

Extended range (``extended_range``, non-causal only): the ordinary backward
keeps one power-of-two scale per instance, so a partition vector that spans
more than float64's exponent range (a reward contrast of 4 on a grid 256 wide)
comes back with NaN rows and, beside them, finite rows that are wrong.
``True`` runs every backward with one exponent per state
(``ops.backward_maxent_extended``); ``"auto"`` reruns only the instances that
show the symptom.  From 8192 states on the extended pass runs the instances
that can be co-resident in one persistent launch (and then synchronises the
stream); a rerun set that would need more sequential launches than
``IRLMX_EXT_GRID_MAX_LAUNCHES`` takes one launch per sweep, as every model
between 4096 and 8192 states does.

Finite horizon (``horizon=T``, non-causal only): for models without a terminal
state and demonstrations cut after T steps (``ops.rollout``'s truncated
trajectories).  ``backward()`` returns the time-indexed policy [n, T, S, A]
(``ops.backward_maxent_horizon``; n * T * S * A * 8 bytes: 17 MB for one 64x64
instance at T = 128) and ``forward()`` sums the T + 1 marginals
(``ops.forward_svf_horizon``), both fully asynchronous; ``terminal`` may be
empty; ``extended_range`` is ignored, the pass always keeps one exponent per
state.  ``BatchedCausalHorizon`` is the same driver with the finite-horizon
soft value iteration as its backward pass (``ops.soft_backward_horizon``): the
MaxCausalEnt model, for stochastic dynamics.  ``stream_policy=True`` (or a
segment length C) on either makes ``step()`` one call of
``ops.expected_svf_horizon``: the same bits without the policy tensor, memory
about 2 * sqrt(T) vectors of [n, S] instead of T * A.
"""

import numpy as np
import torch

from . import _lib, ops
from .mdp import DeviceMDP
from .optim import ExpSga, linear_decay


def terminal_reward(terminal, n_states, batch=1, device=None):
    """phi of the causal backward pass (maxent.py:313-317), as float64 [B, S]:
    0 at the terminal states and -inf elsewhere, or ``terminal`` itself when it
    has one entry per state."""
    if len(terminal) == n_states:
        phi = np.array(terminal, dtype=float)
    else:
        phi = -np.inf * np.ones(n_states)
        phi[terminal] = 0.0
    return torch.as_tensor(np.tile(phi, (batch, 1)), dtype=torch.float64, device=device)


class BatchedMaxEnt:
    def __init__(self, mdp: DeviceMDP, e_features, p_initial, terminal, features=None, lr0=0.2,
                 eps_esvf=1e-5, theta0=1.0, rescale=True, causal=False, discount=None, eps_lap=1e-5,
                 optimizer=None, extended_range=False, horizon=None, stream_policy=False):
        """``theta0``: a float (the reference's Constant init, optimizer.py:369-398) or
        an array [F] or [B, F] (e.g. drawn with the reference's Uniform init,
        optimizer.py:334-366).  ``optimizer``: an irlmx.optim optimiser (default
        ExpSga(linear_decay(lr0)), the reference main.py's choice).
        ``extended_range`` (ignored with ``causal=True``: soft VI works in the log
        domain already): ``False`` the ordinary backward; ``True`` every backward
        runs ``ops.backward_maxent_extended``; ``"auto"`` after the ordinary
        backward, the instances whose policy holds any NaN or any exact 0 are
        recomputed with the extended pass and spliced in.  In a gridworld a zero
        is either underflow or a state that cannot reach a terminal; in the
        second case the rerun returns the same zero.  The check costs one device
        reduction and one host read per step.
        ``horizon``: an int T >= 1 runs the finite-horizon passes (module
        docstring); ``terminal`` may then be empty; ValueError with
        ``causal=True``.
        ``stream_policy`` (horizon models only, ValueError without a horizon):
        ``True`` or an int C makes ``step()`` call ``ops.expected_svf_horizon``
        (``segment`` = 0 or C) instead of ``backward()`` plus ``forward()``: the
        same bits without the policy tensor.  ``backward()``, ``forward()`` and
        the consumers of the time-indexed policy stay as they are."""
        if horizon is not None:
            if causal:
                raise ValueError("horizon applies to the non-causal model only (the finite-horizon causal model "
                                 "is BatchedCausalHorizon)")
            if int(horizon) != horizon or not 1 <= int(horizon) <= _lib.HORIZON_MAX:
                raise ValueError(f"horizon must be an integer in [1, 2^20], got {horizon!r}")
            horizon = int(horizon)
        self.horizon = horizon
        if stream_policy is not False:
            if horizon is None:
                raise ValueError("stream_policy needs a horizon (it streams the time-indexed policy of a horizon model)")
            if stream_policy is not True and (int(stream_policy) != stream_policy or int(stream_policy) < 0):
                raise ValueError(f"stream_policy must be False, True or a segment length >= 0, got {stream_policy!r}")
        self.stream_policy = stream_policy
        if extended_range not in (False, True, "auto"):
            raise ValueError(f"extended_range must be False, True or 'auto', got {extended_range!r}")
        self.extended_range = extended_range
        self.mdp = mdp
        dev = mdp.device
        B, S = mdp.batch, mdp.n_states
        if features is None:
            self.features = None
            n_f = S
        else:
            f = torch.as_tensor(features, dtype=torch.float64, device=dev)
            if f.dim() == 2:
                assert f.shape[0] == S, f.shape
            else:
                assert f.dim() == 3 and f.shape[:2] == (B, S), f.shape
            self.features = f
            n_f = f.shape[-1]
        self.e_features = torch.as_tensor(e_features, dtype=torch.float64, device=dev).reshape(B, n_f)
        self.p_initial = torch.as_tensor(p_initial, dtype=torch.float64, device=dev).reshape(B, S)
        self.terminal = ops.terminal_mask(np.asarray(terminal, dtype=np.int64) if np.size(terminal) == 0 else terminal,
                                          S, batch=B, device=dev)
        self.causal = causal
        self.phi = None
        if causal:
            if discount is None:
                raise ValueError("causal IRL needs a discount (maxent.py:383)")
            self.phi = terminal_reward(terminal, S, batch=B, device=dev)
        self.discount = discount
        self.eps_lap = eps_lap
        if np.ndim(theta0) == 0:
            self.theta = torch.full((B, n_f), float(theta0), dtype=torch.float64, device=dev)
        else:
            t0 = torch.as_tensor(np.asarray(theta0, dtype=np.float64), device=dev)
            self.theta = t0.expand(B, n_f).clone() if t0.dim() == 1 else t0.reshape(B, n_f).clone()
        self.lr0 = lr0
        self.optimizer = optimizer if optimizer is not None else ExpSga(linear_decay(lr0))
        self.eps_esvf = eps_esvf
        self.rescale = rescale
        self.k = 0
        self.active = torch.ones(B, dtype=torch.bool, device=dev)
        self.steps = torch.zeros(B, dtype=torch.int64, device=dev)
        self.last_forward_sweeps = None    # [B] int64, 0 for instances not computed in the last step
        self.last_backward_sweeps = None   # causal: soft VI sweeps of the last backward() [B]
        self.last_delta = None
        self._work = None                  # compacted working set (compact()), None = all instances

    @property
    def batch(self):
        return self.mdp.batch

    @property
    def working_batch(self):
        """Instances the next step computes (all, or the active ones after compact())."""
        return self.batch if self._work is None else int(self._work["idx"].numel())

    # -- working set ----------------------------------------------------------

    def compact(self):
        """Restrict the following steps to the instances that are still active.

        Gathers their tables, demonstration statistics, masks and features into a
        smaller batch; theta stays full size (the working rows are gathered and
        scattered per step).  Returns the working batch size."""
        idx = torch.nonzero(self.active).squeeze(1)
        n = int(idx.numel())
        if n == self.working_batch:
            return n
        sel = lambda t: t.index_select(0, idx).contiguous() if t is not None else None
        feats = self.features
        if feats is not None and feats.dim() == 3:
            feats = sel(feats)
        self._work = {"idx": idx, "mdp": self.mdp.take(idx), "e_features": sel(self.e_features),
                      "p_initial": sel(self.p_initial), "terminal": sel(self.terminal), "phi": sel(self.phi),
                      "features": feats, "active": torch.ones(n, dtype=torch.bool, device=idx.device)}
        return n

    def _w(self, name):
        if self._work is None:
            return getattr(self, name)
        return self._work[name]

    def _theta_w(self):
        return self.theta if self._work is None else self.theta.index_select(0, self._work["idx"])

    def _active_w(self):
        return self.active if self._work is None else self.active.index_select(0, self._work["idx"])

    def _scatter(self, vec_w, fill=0):
        """A per-instance vector of the working set, expanded to all B instances."""
        if self._work is None:
            return vec_w
        out = torch.full((self.batch,) + tuple(vec_w.shape[1:]), fill, dtype=vec_w.dtype, device=vec_w.device)
        out[self._work["idx"]] = vec_w
        return out

    # -- one gradient step --------------------------------------------------

    def reward(self, theta=None, features=None):
        """F . theta (maxent.py:244): [B, S] for all instances by default."""
        if theta is None:
            theta, features = self.theta, self.features
        if features is None:
            return theta
        if features.dim() == 2:
            return theta @ features.T
        return torch.bmm(features, theta.unsqueeze(2)).squeeze(2)

    def features_t(self, svf, features=None):
        """F^T . svf, [n, F] (maxent.py:248)."""
        if features is None:
            features = self._w("features")
        if features is None:
            return svf
        if features.dim() == 2:
            return svf @ features
        return torch.bmm(svf.unsqueeze(1), features).squeeze(1)

    def backward(self):
        """Policy [n, S, A] of the working set (maxent.py:119-159 / 279-341); with
        ``horizon=T`` the time-indexed policy [n, T, S, A]."""
        r = self.reward(self._theta_w(), self._w("features"))
        mdp = self._w("mdp")
        if self.horizon is not None:
            return ops.backward_maxent_horizon(mdp, r, self.horizon, self._w("terminal"))
        if self.causal:
            pi, _, k, _ = ops.soft_backward(mdp, r, self._w("phi"), self.discount, self.eps_lap)
            self.last_backward_sweeps = self._scatter(k)
            return pi
        if self.extended_range is True:
            return ops.backward_maxent_extended(mdp, r, self._w("terminal"))
        pi = ops.backward_maxent(mdp, r, self._w("terminal"), rescale=self.rescale)
        if self.extended_range == "auto":
            suspect = (torch.isnan(pi) | (pi == 0)).flatten(1).any(dim=1)
            idx = torch.nonzero(suspect).squeeze(1)          # (the host read: the index count)
            if idx.numel():
                sub = mdp.take(idx)
                pi[idx] = ops.backward_maxent_extended(sub, r.index_select(0, idx),
                                                       self._w("terminal").index_select(0, idx))
        return pi

    def forward(self, pi):
        """``(svf [n, S], sweeps [n], status [n])`` of the working set (maxent.py:63-114);
        with ``horizon=T`` the sum of the T + 1 marginals, sweeps = T."""
        if self.horizon is not None:
            return ops.forward_svf_horizon(self._w("mdp"), self._w("p_initial"), pi, self._w("terminal"))
        return ops.forward_svf(self._w("mdp"), self._w("p_initial"), self._w("terminal"), pi, self.eps_esvf)

    def update(self, svf):
        """Optimiser step on the working set's theta (default ExpSga,
        optimizer.py:154-167); stopped instances stay frozen.  Returns the gradient [n, F]."""
        theta = self._theta_w()
        act = self._active_w()
        grad = self._w("e_features") - self.features_t(svf)
        new = self.optimizer.apply(theta, grad, self.k)
        delta = torch.where(act, (new - theta).abs().amax(dim=1),
                            torch.zeros((), dtype=torch.float64, device=theta.device))
        new = torch.where(act.unsqueeze(1), new, theta)
        if self._work is None:
            self.theta = new
        else:
            self.theta[self._work["idx"]] = new
        self.last_delta = self._scatter(delta)
        self.steps += self.active.to(torch.int64)
        self.k += 1
        return grad

    def _horizon_model(self):
        """``(model, discount)`` of ``ops.expected_svf_horizon`` for this driver's backward pass."""
        return "maxent", 1.0

    def expected_svf(self):
        """``(svf [n, S], sweeps [n], status [n])`` of the working set in one call,
        without the time-indexed policy (``ops.expected_svf_horizon``): what
        ``forward(backward())`` returns, bit for bit.  Horizon models only."""
        if self.horizon is None:
            raise ValueError("expected_svf runs the one-call pass of a horizon model; without a horizon use "
                             "forward(backward())")
        model, discount = self._horizon_model()
        auto = self.stream_policy is False or self.stream_policy is True      # (1 == True: identity, not equality)
        segment = 0 if auto else int(self.stream_policy)
        r = self.reward(self._theta_w(), self._w("features"))
        return ops.expected_svf_horizon(self._w("mdp"), r, self._w("p_initial"), self.horizon, model=model,
                                        discount=discount, terminal=self._w("terminal"), segment=segment)

    def step(self):
        if self.stream_policy is not False:
            svf, iters, _ = self.expected_svf()
        else:
            pi = self.backward()
            svf, iters, _ = self.forward(pi)
        self.last_forward_sweeps = self._scatter(iters)
        self.update(svf)
        return svf

    def expected_value_difference(self, true_reward, discount, eps=1e-3):
        """Expected value difference ``p0 . (v* - v_pi)`` of the current theta under
        ``true_reward`` ([S] or [B, S]), per instance: a [B] tensor in original
        instance order, also after compaction.  pi is the current theta's
        backward policy on all B instances (stopped ones included: their theta
        is their result); p0 and the terminals are this object's own
        (ops.expected_value_difference).  Reads theta only: theta, the step
        counter, the active set and the compaction state stay as they are."""
        self._stationary_only("expected_value_difference")
        work, sweeps = self._work, self.last_backward_sweeps
        self._work = None          # the full batch, in original order
        try:
            pi = self.backward()
        finally:
            self._work, self.last_backward_sweeps = work, sweeps
        B, S = self.batch, self.mdp.n_states
        r = torch.as_tensor(true_reward, dtype=torch.float64, device=self.theta.device)
        r = r.expand(B, S) if r.dim() == 1 else r.reshape(B, S)
        return ops.expected_value_difference(self.mdp, r.contiguous(), pi, self.p_initial, discount, self.terminal,
                                             eps)[0]

    def _stationary_only(self, what):
        if self.horizon is not None:
            raise NotImplementedError(f"{what} takes a stationary policy; with horizon={self.horizon} the policy is "
                                      "time-indexed [T, S, A]: use sample_horizon, log_likelihood_horizon and "
                                      "expected_value_difference_horizon")

    def log_likelihood(self, states, actions, lengths):
        """Mean per-trajectory log-likelihood of stored demonstrations (``states``
        [B, N, L + 1], ``actions`` [B, N, L], ``lengths`` [B, N], as
        ``ops.rollout`` returns them) under the current theta's backward policy,
        per instance: a [B] tensor in original instance order, also after
        compaction (``ops.demo_log_likelihood``'s sum over N).  The score that
        needs no true reward; -inf where a demonstration takes an action the
        policy gives probability 0.  Reads theta only: theta, the step counter,
        the active set and the compaction state stay as they are."""
        self._stationary_only("log_likelihood")
        work, sweeps = self._work, self.last_backward_sweeps
        self._work = None          # the full batch, in original order
        try:
            pi = self.backward()
        finally:
            self._work, self.last_backward_sweeps = work, sweeps
        ll, ll_traj, _ = ops.demo_log_likelihood(pi, torch.as_tensor(states, device=pi.device), actions, lengths)
        return ll / ll_traj.shape[1]

    # -- the time-indexed policy of a horizon model ------------------------------

    def _policy_t(self, what, stationary):
        """pi_t [B, T, S, A] of the current theta on all B instances in original
        order; theta, the step counter, the active set and the compaction state
        stay as they are."""
        if self.horizon is None:
            raise ValueError(f"{what} takes the time-indexed policy of a horizon model; without a horizon use "
                             f"{stationary}")
        work, sweeps = self._work, self.last_backward_sweeps
        self._work = None          # the full batch, in original order
        try:
            return self.backward()
        finally:
            self._work, self.last_backward_sweeps = work, sweeps

    def log_likelihood_horizon(self, states, actions, lengths):
        """:meth:`log_likelihood` for a horizon model: the mean per-trajectory
        log-likelihood of stored demonstrations (``states`` [B, N, L + 1],
        ``actions`` [B, N, L], ``lengths`` [B, N], as ``ops.rollout_horizon``
        returns them) under the current theta's time-indexed policy
        (``ops.demo_log_likelihood_horizon``'s sum over N), a [B] tensor in
        original instance order, also after compaction.  Reads theta only."""
        pi = self._policy_t("log_likelihood_horizon", "log_likelihood")
        ll, ll_traj, _ = ops.demo_log_likelihood_horizon(pi, torch.as_tensor(states, device=pi.device), actions,
                                                         lengths)
        return ll / ll_traj.shape[1]

    def expected_value_difference_horizon(self, true_reward, discount=1.0):
        """:meth:`expected_value_difference` for a horizon model: ``p0 . (v*_0 -
        v_pi_0)`` over the model's T steps under ``true_reward`` ([S] or
        [B, S]), pi the current theta's time-indexed policy, p0 and the
        terminals this object's own (``ops.expected_value_difference_horizon``):
        a [B] tensor in original instance order.  Reads theta only."""
        pi = self._policy_t("expected_value_difference_horizon", "expected_value_difference")
        B, S = self.batch, self.mdp.n_states
        r = torch.as_tensor(true_reward, dtype=torch.float64, device=self.theta.device)
        r = r.expand(B, S) if r.dim() == 1 else r.reshape(B, S)
        return ops.expected_value_difference_horizon(self.mdp, r.contiguous(), pi, self.p_initial, discount,
                                                     self.terminal)[0]

    def sample_horizon(self, start, n, seed):
        """``n`` trajectories of T steps per instance under the current theta's
        time-indexed policy (``ops.rollout_horizon`` with this object's
        terminals and ``return_trajectories=True``): its RolloutResult, in
        original instance order.  Reads theta only."""
        pi = self._policy_t("sample_horizon", "ops.rollout with backward()'s policy")
        return ops.rollout_horizon(self.mdp, pi, start, n, seed, terminal=self.terminal, return_trajectories=True)

    @classmethod
    def from_trajectories(cls, mdp, states, lengths, terminal, features=None, **kw):
        """A BatchedMaxEnt whose demonstration statistics come from stored
        trajectories (``states`` [B, N, L + 1], ``lengths`` [B, N]) through
        ``ops.demo_statistics``: ``p_initial = starts / N`` and ``e_features =
        visits / N`` (identity features), or ``(visits / N) @ F`` with a feature
        matrix ``features`` ([S, F] or [B, S, F]) -- maxent.py:15-60.  Raises
        ValueError if a trajectory holds a state off the model or a length
        beyond its row.  ``kw``: the constructor's other arguments."""
        visits, starts, status = ops.demo_statistics(mdp.n_states, torch.as_tensor(states, device=mdp.device), lengths)
        bad = int((status != 0).sum())
        if bad:
            raise ValueError(f"from_trajectories: {bad} of {status.numel()} trajectories hold a state outside "
                             f"[0, {mdp.n_states}) or a length outside their row")
        n = status.shape[1]
        e = visits.to(torch.float64) / n
        if features is not None:
            f = torch.as_tensor(features, dtype=torch.float64, device=e.device)
            e = e @ f if f.dim() == 2 else torch.bmm(e.unsqueeze(1), f).squeeze(1)
        return cls(mdp, e, starts.to(torch.float64) / n, terminal, features=features, **kw)

    def prime_compaction(self, eps=1e-4):
        """Run, once, every device operation of ``run()`` outside the passes --
        the stop test, ``compact()`` and ``update()`` on a working set, the
        scatter of its results -- on a scratch copy of this object (its state is
        left unchanged), for working sets of more and of at most 16 instances
        (torch's index_select switches kernels at 16 indices).  The first use of
        a device kernel in a process pays its code-object load: without this,
        bench.py's full run paid ~0.13 s at its first step and ~0.13 s at the
        first compaction to 15 instances (tools/diag/full_run_steps.py)."""
        import copy
        B = self.batch
        dev = self.theta.device
        for n in sorted({n for n in (B - 1, min(B - 1, 16), 1) if n >= 1}, reverse=True):
            sc = copy.copy(self)
            sc.theta, sc.steps, sc._work = self.theta.clone(), self.steps.clone(), None
            sc.active = torch.zeros(B, dtype=torch.bool, device=dev)
            sc.active[:n] = True
            sc.compact()
            svf = torch.zeros((n, self.mdp.n_states), dtype=torch.float64, device=dev)
            sc.last_forward_sweeps = sc._scatter(torch.zeros(n, dtype=torch.int64, device=dev))
            sc.update(svf)
            sc.active &= sc.last_delta > eps
            bool(sc.active.any())
            sc.reward()
        torch.cuda.synchronize(dev)

    def run(self, eps=1e-4, max_steps=None, compact=True, on_step=None):
        """Step until every instance meets ``max|dtheta| <= eps`` (maxent.py:240, 252).

        ``compact``: drop stopped instances from the working set before each
        step (module docstring).  ``on_step(self)`` is called after every step.
        Returns ``(reward [B, S], steps [B])`` -- ``features . theta`` and the
        number of gradient steps each instance took.
        """
        while bool(self.active.any()):
            if max_steps is not None and self.k >= max_steps:
                break
            if compact:
                self.compact()
            self.step()
            self.active &= self.last_delta > eps   # NaN > eps is False: a NaN step stops
            if on_step is not None:
                on_step(self)
        return self.reward(), self.steps


class BatchedCausalHorizon(BatchedMaxEnt):
    """Finite-horizon MaxCausalEnt IRL: ``BatchedMaxEnt(horizon=T)`` with the soft
    Bellman recursion over T steps as its backward pass
    (``ops.soft_backward_horizon``) -- the model for stochastic dynamics and
    demonstrations of a fixed length.  ``terminal`` may be empty and
    ``discount`` may be 1: the recursion needs neither to be well posed.  The
    forward pass, the update, compaction and ``from_trajectories`` (``horizon``
    and ``discount`` go through its ``**kw``) are the base class's;
    ``e_features - svf`` is the exact gradient of the demonstrations'
    likelihood.  ``log_likelihood`` and ``expected_value_difference`` raise
    NotImplementedError, as with any time-indexed policy: their twins are
    ``log_likelihood_horizon``, ``expected_value_difference_horizon`` and
    ``sample_horizon``."""

    def __init__(self, mdp, e_features, p_initial, terminal, horizon, discount=1.0, **kw):
        if kw.pop("causal", False):
            raise ValueError("BatchedCausalHorizon is the causal model already: causal= is not an argument")
        discount = float(discount)
        if not 0.0 <= discount <= 1.0:
            raise ValueError(f"discount must lie in [0, 1], got {discount!r}")
        super().__init__(mdp, e_features, p_initial, terminal, horizon=horizon, **kw)
        if self.horizon is None:
            raise ValueError("BatchedCausalHorizon needs a horizon")
        self.discount = discount

    def backward(self):
        """The time-indexed policy [n, T, S, A] of the working set."""
        r = self.reward(self._theta_w(), self._w("features"))
        return ops.soft_backward_horizon(self._w("mdp"), r, self.discount, self.horizon, self._w("terminal"))

    def _horizon_model(self):
        return "causal", self.discount
