"""Batched device operations of the MaxEnt-IRL inner loop (torch tensors in/out).

Every function runs on the HIP device through libirlmx.so; inputs are float64
(or uint8 masks) of shape [B, ...] and stay resident in HBM.  These are the
building blocks of the numpy drop-ins (``maxent``, ``solver``) and of the
batched IRL driver (``irlmx.batch``).
"""

import collections
import os

import numpy as np
import torch

from . import _lib
from .mdp import DeviceMDP

def _workspace(mdp, op):
    """Device workspace for one call, from torch's caching allocator.

    Allocated per call on the current stream: the allocator hands a freed block
    only to later work on the same stream (stream-ordered), so concurrent calls
    from other host threads or on other streams never share a workspace that an
    in-flight kernel still uses -- the stream / thread safety include/irlmx.h
    states for the C ABI."""
    lib = _lib.load()
    n = int(lib.irlmx_workspace_bytes(mdp.struct(), op))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=mdp.device), n


PLAN_FIELDS = ("shape", "R", "G", "C", "per_launch", "spt", "layout", "threads", "launches", "lds_bytes")
SHAPES = {0: "fused", 1: "cluster", 2: "sweep", 3: "dense", 4: "dense-gemm", 5: "grid", 6: "dense-grid"}
_OPS = {"backward": _lib.OP_BACKWARD, "forward": _lib.OP_FORWARD, "soft_backward": _lib.OP_SOFT_BACKWARD,
        "value_iteration": _lib.OP_VALUE_ITERATION, "policy_evaluation": _lib.OP_POLICY_EVALUATION,
        "backward_horizon": _lib.OP_BACKWARD_HORIZON, "forward_horizon": _lib.OP_FORWARD_HORIZON,
        "soft_backward_horizon": _lib.OP_SOFT_BACKWARD_HORIZON, "value_horizon": _lib.OP_VALUE_HORIZON}
_OPS.update({code: code for code in list(_OPS.values())})   # the _lib.OP_* codes themselves are accepted too


def execution_plan(mdp, op, rescale=True, extended_range=False):
    """The kernel plan a call of ``op`` ("backward", "forward", "soft_backward",
    "value_iteration", "policy_evaluation", "backward_horizon",
    "forward_horizon", "soft_backward_horizon", "value_horizon", or its ``_lib.OP_*`` code) on ``mdp``
    runs on the current device (irlmx_execution_plan):
    shape, tile rows R, ghost rows G, tiles per instance C, instances per launch,
    states per lane, in-tile layout, threads, sequential launches, LDS bytes.
    ``rescale=False``: the plan of ``backward_maxent(..., rescale=False)``.
    ``extended_range=True`` (``op="backward"`` only): the plan of
    ``backward_maxent_extended`` -- "fused", "grid" (G: 1 = each instance on one
    XCD, C workgroups per instance, instances per launch, sequential launches)
    or "sweep" with its 2*S - 1 launches."""
    import ctypes
    lib = _lib.load()
    buf = (ctypes.c_int64 * len(PLAN_FIELDS))()
    if extended_range:
        code = _OPS[op] | _lib.PLAN_EXTENDED_RANGE
    else:
        code = _OPS[op] | (0 if rescale or _OPS[op] != _lib.OP_BACKWARD else _lib.PLAN_NO_RESCALE)
    _lib.check(lib.irlmx_execution_plan(mdp.struct(), code, buf), "execution_plan")
    plan = dict(zip(PLAN_FIELDS, [int(v) for v in buf]))
    plan["shape"] = SHAPES[plan["shape"]]
    return plan


def counters():
    """Process-wide event counters of the library (irlmx_counters): persistent
    launches and per-sweep reruns, by name (``_lib.COUNTER_NAMES``)."""
    import ctypes
    lib = _lib.load()
    buf = (ctypes.c_int64 * len(_lib.COUNTER_NAMES))()
    n = lib.irlmx_counters(buf, len(_lib.COUNTER_NAMES))
    assert n == len(_lib.COUNTER_NAMES), n
    return dict(zip(_lib.COUNTER_NAMES, [int(v) for v in buf]))


def device_check_failures():
    """Bits of the in-kernel bounds checks that failed since the last call
    (irlmx_device_check_failures: 1 index, 2 granule, 4 tile); always 0 unless
    the library is the IRLMX_DEVICE_CHECKS build (libirlmx_checks.so)."""
    v = int(_lib.load().irlmx_device_check_failures())
    if v < 0:
        raise RuntimeError("irlmx_device_check_failures: HIP error")
    return v


def _f64(x, mdp, shape):
    t = torch.as_tensor(x, dtype=torch.float64, device=mdp.device)
    return t.reshape(shape).contiguous()


def terminal_mask(terminal, n_states, batch=1, device=None):
    """uint8 [B, S] mask with the reference's indexing semantics (maxent.py:99, 147).

    ``terminal`` is indexed into a numpy vector exactly as the reference indexes
    with it, so negative indices, duplicates and invalid index types behave (or
    raise) the same way.
    """
    m = np.zeros(n_states, dtype=np.uint8)
    m[terminal] = 1
    return torch.as_tensor(np.tile(m, (batch, 1)), device=device)


def backward_maxent(mdp, reward, terminal, rescale=True):
    """Local action probabilities [B, S, A] (maxent.py:119-159)."""
    lib = _lib.load()
    B, S, A = mdp.batch, mdp.n_states, mdp.n_actions
    r = _f64(reward, mdp, (B, S))
    term = terminal.to(device=mdp.device, dtype=torch.uint8).reshape(B, S).contiguous()
    pi = torch.empty((B, S, A), dtype=torch.float64, device=mdp.device)
    status = torch.empty(B, dtype=torch.int32, device=mdp.device)
    ws, n = _workspace(mdp, _lib.OP_BACKWARD)
    _lib.check(lib.irlmx_backward_maxent(mdp.struct(), _lib.ptr(r), _lib.ptr(term), 1 if rescale else 0,
                                         _lib.ptr(pi), _lib.ptr(status), _lib.ptr(ws), n,
                                         _lib.stream_ptr(mdp.device)), "backward_maxent")
    return pi


def backward_maxent_extended(mdp, reward, terminal):
    """Local action probabilities [B, S, A] (maxent.py:119-159) with one exponent
    per state (irlmx_backward_maxent_extended): finite, and right, where the
    partition vector spans more than float64's exponent range and
    ``backward_maxent`` returns NaN rows and wrong finite rows beside them;
    bit-identical to ``backward_maxent`` where that pass stays in range.
    STENCIL5 and ELL models.  Up to 4096 states one workgroup per instance;
    from 8192 states on (at most 16 slots per state, 2^18 states) one persistent
    launch for all sweeps of the instances that can be co-resident -- the call
    then synchronises the stream; whatever is in between, larger, or a batch
    that would need more sequential launches than
    ``IRLMX_EXT_GRID_MAX_LAUNCHES`` runs one launch per sweep (2*S - 1
    launches: slow at config-4 size).  ``execution_plan(...,
    extended_range=True)`` names the shape."""
    lib = _lib.load()
    B, S, A = mdp.batch, mdp.n_states, mdp.n_actions
    r = _f64(reward, mdp, (B, S))
    term = terminal.to(device=mdp.device, dtype=torch.uint8).reshape(B, S).contiguous()
    pi = torch.empty((B, S, A), dtype=torch.float64, device=mdp.device)
    status = torch.empty(B, dtype=torch.int32, device=mdp.device)
    ws, n = _workspace(mdp, _lib.OP_BACKWARD | _lib.PLAN_EXTENDED_RANGE)
    _lib.check(lib.irlmx_backward_maxent_extended(mdp.struct(), _lib.ptr(r), _lib.ptr(term), _lib.ptr(pi),
                                                  _lib.ptr(status), _lib.ptr(ws), n, _lib.stream_ptr(mdp.device)),
               "backward_maxent_extended")
    return pi


def numpy_order_supported(mdp, op="backward"):
    """Whether the numpy-order kernels cover this model (S <= 4096, S % 4 in
    {0, 1}; the forward's ELL column form at most 32 slots)."""
    S = mdp.n_states
    ok = S <= 4096 and S % 4 in (0, 1)
    if op == "forward" and mdp.layout == _lib.LAYOUT_ELL:
        ok = ok and mdp.k_col <= 32
    return ok


# Default numpy-order scope of the drop-ins per op: (states on STENCIL5 / ELL
# models, states on DENSE tables).  The kernels themselves cover 4096 states.
NUMPY_ORDER_CAPS = {"backward": (1024, 64), "forward": (1024, 64),
                    "soft_backward": (4096, 64), "value_iteration": (4096, 4096)}
_CAP_ENV = {"backward": "BWD", "forward": "FWD", "soft_backward": "SOFT", "value_iteration": "VI"}


def numpy_order_cap(mdp, op="backward"):
    """The largest state count at which the drop-ins run ``op`` in numpy's order
    on this model's layout (NUMPY_ORDER_CAPS; environment overrides: see
    numpy_order_default)."""
    sparse_cap, dense_cap = NUMPY_ORDER_CAPS[op]
    cap = int(os.environ.get("IRLMX_NUMPY_ORDER_MAX", sparse_cap))
    cap = int(os.environ.get(f"IRLMX_NUMPY_ORDER_{_CAP_ENV[op]}_MAX", cap))
    if mdp.layout == _lib.LAYOUT_DENSE:
        cap = min(cap, int(os.environ.get("IRLMX_NUMPY_ORDER_DENSE_MAX", dense_cap)))
    return cap


def numpy_order_default(mdp, op="backward"):
    """Whether the drop-ins (maxent.py, solver.py) run ``op`` ("backward",
    "forward", "soft_backward", "value_iteration") in numpy's order: one
    instance, a model the numpy-order kernels cover, and at most
    numpy_order_cap(mdp, op) states.

    Caps per op (NUMPY_ORDER_CAPS): value iteration and soft VI run in numpy's
    order on every model the kernels cover (4096 states; soft VI 64 on a DENSE
    table), so solver.value_iteration / optimal_policy and
    local_causal_action_probabilities reproduce the reference's values and argmax
    at config 2's 64x64 (tests/golden/c2_64.npz).  The backward and the forward
    stop at 1024 (64 on DENSE): beyond, their one-workgroup kernels re-read every
    entry each of thousands of sweeps -- measured on one MI355X
    (tools/diag/np_bwd_cost.py), the backward takes 31-435x the tiled shapes' time
    at 33x33-64x64 (1.26 s vs 2.9 ms at 64x64) and 132x / 1,650x on dense tables of
    256 / 1024 states; soft VI costs 4-16x on grids (milliseconds) but 75-950x on
    dense tables, value iteration (tens of sweeps) stays in milliseconds to a
    fraction of a second.  Above the caps the drop-ins take the tiled shapes
    (within 1e-9 of the oracle; argmax ties may fall differently).

    Environment: IRLMX_NUMPY_ORDER=0 turns numpy's order off;
    IRLMX_NUMPY_ORDER_MAX sets every op's grid cap, IRLMX_NUMPY_ORDER_{BWD,FWD,
    SOFT,VI}_MAX one op's, IRLMX_NUMPY_ORDER_DENSE_MAX the DENSE cap."""
    if mdp.batch != 1 or not numpy_order_supported(mdp, op) or os.environ.get("IRLMX_NUMPY_ORDER", "1") == "0":
        return False
    return mdp.n_states <= numpy_order_cap(mdp, op)


def backward_maxent_numpy_order(mdp, exp_reward, terminal):
    """Local action probabilities [B, S, A] (maxent.py:119-159) in numpy's own
    floating-point order (irlmx_backward_maxent_numpy_order): bit-identical to
    the reference's on a Haswell-family OpenBLAS host, NaN where it overflows.
    ``exp_reward`` is np.exp(reward) as the reference computes it (maxent.py:142)."""
    lib = _lib.load()
    B, S, A = mdp.batch, mdp.n_states, mdp.n_actions
    er = _f64(exp_reward, mdp, (B, S))
    term = terminal.to(device=mdp.device, dtype=torch.uint8).reshape(B, S).contiguous()
    pi = torch.empty((B, S, A), dtype=torch.float64, device=mdp.device)
    status = torch.empty(B, dtype=torch.int32, device=mdp.device)
    _lib.check(lib.irlmx_backward_maxent_numpy_order(mdp.struct(), _lib.ptr(er), _lib.ptr(term), _lib.ptr(pi),
                                                     _lib.ptr(status), _lib.stream_ptr(mdp.device)),
               "backward_maxent_numpy_order")
    return pi


def forward_svf(mdp, p_initial, terminal, p_action, eps=1e-5, max_iter=0, numpy_order=False):
    """Expected state-visitation frequencies (maxent.py:63-114).

    Returns ``(svf [B, S], iterations [B] int64, status [B] int32)``.
    ``numpy_order``: numpy's summation order (irlmx_forward_svf_numpy_order):
    SVF and sweep count bit-identical to the reference on a Haswell-family host.
    """
    lib = _lib.load()
    B, S, A = mdp.batch, mdp.n_states, mdp.n_actions
    p0 = _f64(p_initial, mdp, (B, S))
    pi = _f64(p_action, mdp, (B, S, A))
    term = terminal.to(device=mdp.device, dtype=torch.uint8).reshape(B, S).contiguous()
    svf = torch.empty((B, S), dtype=torch.float64, device=mdp.device)
    iters = torch.empty(B, dtype=torch.int64, device=mdp.device)
    status = torch.empty(B, dtype=torch.int32, device=mdp.device)
    if numpy_order:
        _lib.check(lib.irlmx_forward_svf_numpy_order(mdp.struct(), _lib.ptr(p0), _lib.ptr(term), _lib.ptr(pi),
                                                     float(eps), int(max_iter), _lib.ptr(svf), _lib.ptr(iters),
                                                     _lib.ptr(status), _lib.stream_ptr(mdp.device)),
                   "forward_svf_numpy_order")
        return svf, iters, status
    ws, n = _workspace(mdp, _lib.OP_FORWARD)
    _lib.check(lib.irlmx_forward_svf(mdp.struct(), _lib.ptr(p0), _lib.ptr(term), _lib.ptr(pi), float(eps),
                                     int(max_iter), _lib.ptr(svf), _lib.ptr(iters), _lib.ptr(status),
                                     _lib.ptr(ws), n, _lib.stream_ptr(mdp.device)), "forward_svf")
    return svf, iters, status


def soft_backward(mdp, reward, terminal_reward, discount, eps=1e-5, max_iter=0, numpy_order=False):
    """MaxCausalEnt soft value iteration (maxent.py:279-341).

    Returns ``(p_action [B, S, A], value [B, S], iterations [B], status [B])``.
    ``numpy_order``: every P_a . v summed in numpy's order
    (irlmx_soft_backward_numpy_order; numpy_order_supported(mdp) models only).
    """
    lib = _lib.load()
    B, S, A = mdp.batch, mdp.n_states, mdp.n_actions
    r = _f64(reward, mdp, (B, S))
    phi = _f64(terminal_reward, mdp, (B, S))
    pi = torch.empty((B, S, A), dtype=torch.float64, device=mdp.device)
    v = torch.empty((B, S), dtype=torch.float64, device=mdp.device)
    iters = torch.empty(B, dtype=torch.int64, device=mdp.device)
    status = torch.empty(B, dtype=torch.int32, device=mdp.device)
    if numpy_order:
        _lib.check(lib.irlmx_soft_backward_numpy_order(mdp.struct(), _lib.ptr(r), _lib.ptr(phi), float(discount),
                                                       float(eps), int(max_iter), _lib.ptr(pi), _lib.ptr(v),
                                                       _lib.ptr(iters), _lib.ptr(status), _lib.stream_ptr(mdp.device)),
                   "soft_backward_numpy_order")
        return pi, v, iters, status
    ws, n = _workspace(mdp, _lib.OP_SOFT_BACKWARD)
    _lib.check(lib.irlmx_soft_backward(mdp.struct(), _lib.ptr(r), _lib.ptr(phi), float(discount), float(eps),
                                       int(max_iter), _lib.ptr(pi), _lib.ptr(v), _lib.ptr(iters),
                                       _lib.ptr(status), _lib.ptr(ws), n, _lib.stream_ptr(mdp.device)),
               "soft_backward")
    return pi, v, iters, status


def value_iteration(mdp, reward, discount, eps=1e-3, average=False, max_iter=0, numpy_order=False):
    """Hard-max (solver.py:9-52) or action-average (solver.py:55-104) value iteration.

    Returns ``(value [B, S], iterations [B], status [B])``.  ``numpy_order``:
    numpy's summation order (irlmx_value_iteration_numpy_order), values
    bit-identical to the reference's on a Haswell-family OpenBLAS host.
    """
    lib = _lib.load()
    B, S = mdp.batch, mdp.n_states
    r = _f64(reward, mdp, (B, S))
    v = torch.empty((B, S), dtype=torch.float64, device=mdp.device)
    iters = torch.empty(B, dtype=torch.int64, device=mdp.device)
    status = torch.empty(B, dtype=torch.int32, device=mdp.device)
    if numpy_order:
        _lib.check(lib.irlmx_value_iteration_numpy_order(mdp.struct(), _lib.ptr(r), float(discount), float(eps),
                                                         1 if average else 0, int(max_iter), _lib.ptr(v),
                                                         _lib.ptr(iters), _lib.ptr(status),
                                                         _lib.stream_ptr(mdp.device)), "value_iteration_numpy_order")
        return v, iters, status
    ws, n = _workspace(mdp, _lib.OP_VALUE_ITERATION)
    _lib.check(lib.irlmx_value_iteration(mdp.struct(), _lib.ptr(r), float(discount), float(eps),
                                         1 if average else 0, int(max_iter), _lib.ptr(v), _lib.ptr(iters),
                                         _lib.ptr(status), _lib.ptr(ws), n, _lib.stream_ptr(mdp.device)),
               "value_iteration")
    return v, iters, status


def policy_evaluation(mdp, reward, p_action, discount, terminal=None, eps=1e-3, max_iter=0):
    """Value of the stochastic policy ``p_action`` [B, S, A] under ``reward``
    (irlmx_policy_evaluation): ``v <- r + discount * sum_a pi_a * (P_a v)`` from
    ``v = 0`` until ``max|dv| <= eps``.

    Returns ``(value [B, S], iterations [B], status [B])``.  ``terminal`` (a
    uint8 [B, S] mask, see :func:`terminal_mask`): those states get
    ``v(s) = r(s)``, their successors contribute nothing (the cleared rows of
    maxent.py:98-99); ``None``: no terminal handling, like ``value_iteration``.
    The rows of ``p_action`` need not be normalised: a MaxEnt policy with an
    exact-0 row is legal and gives ``v(s) = r(s)``.  STENCIL5 and ELL models.
    """
    lib = _lib.load()
    B, S, A = mdp.batch, mdp.n_states, mdp.n_actions
    r = _f64(reward, mdp, (B, S))
    pi = _f64(p_action, mdp, (B, S, A))
    term = None if terminal is None else terminal.to(device=mdp.device, dtype=torch.uint8).reshape(B, S).contiguous()
    v = torch.empty((B, S), dtype=torch.float64, device=mdp.device)
    iters = torch.empty(B, dtype=torch.int64, device=mdp.device)
    status = torch.empty(B, dtype=torch.int32, device=mdp.device)
    ws, n = _workspace(mdp, _lib.OP_POLICY_EVALUATION)
    _lib.check(lib.irlmx_policy_evaluation(mdp.struct(), _lib.ptr(r), _lib.ptr(pi), _lib.ptr(term), float(discount),
                                           float(eps), int(max_iter), _lib.ptr(v), _lib.ptr(iters), _lib.ptr(status),
                                           _lib.ptr(ws), n, _lib.stream_ptr(mdp.device)), "policy_evaluation")
    return v, iters, status


def _optional_mask(terminal, mdp):
    if terminal is None:
        return None
    return terminal.to(device=mdp.device, dtype=torch.uint8).reshape(mdp.batch, mdp.n_states).contiguous()


def _horizon_policy(mdp, horizon):
    """``(T, uninitialised pi_t [B, T, S, A])``; for a T outside [1, HORIZON_MAX] the call raises: one step is allocated."""
    T = int(horizon)
    shape = (mdp.batch, T if 1 <= T <= _lib.HORIZON_MAX else 1, mdp.n_states, mdp.n_actions)
    return T, torch.empty(shape, dtype=torch.float64, device=mdp.device)


def backward_maxent_horizon(mdp, reward, horizon, terminal=None, return_log_z0=False):
    """Time-indexed local action probabilities ``pi_t`` [B, T, S, A] of the
    finite-horizon MaxEnt model with ``T = horizon`` steps
    (irlmx_backward_maxent_horizon): from ``Z_T = exp(r)``, for t = T-1 .. 0,
    ``za_t = exp(r) * (P_a Z_{t+1})``, ``Z_t = sum_a za_t`` and ``pi_t = za_t /
    Z_t``.  No terminal state is needed (``terminal=None``); with a uint8
    [B, S] mask (:func:`terminal_mask`) those states are absorbing, ``Z_t =
    exp(r)``.  Every partition value carries its own exponent, as in
    :func:`backward_maxent_extended`, so the policy is finite wherever a
    successor has weight.  ``return_log_z0``: returns ``(pi_t, log_z0 [B, S])``,
    the log partition function of the T-step paths from each state.

    Memory: the result is ``B * T * S * A * 8`` bytes -- 17 MB for one 64x64
    instance at T = 128.  STENCIL5 and ELL models; ``execution_plan(mdp,
    "backward_horizon")`` names the shape."""
    lib = _lib.load()
    B, S = mdp.batch, mdp.n_states
    r = _f64(reward, mdp, (B, S))
    term = _optional_mask(terminal, mdp)
    T, pi = _horizon_policy(mdp, horizon)
    lz = torch.empty((B, S), dtype=torch.float64, device=mdp.device) if return_log_z0 else None
    status = torch.empty(B, dtype=torch.int32, device=mdp.device)
    ws, n = _workspace(mdp, _lib.OP_BACKWARD_HORIZON)
    _lib.check(lib.irlmx_backward_maxent_horizon(mdp.struct(), _lib.ptr(r), _lib.ptr(term), T, _lib.ptr(pi),
                                                 _lib.ptr(lz), _lib.ptr(status), _lib.ptr(ws), n,
                                                 _lib.stream_ptr(mdp.device)), "backward_maxent_horizon")
    return (pi, lz) if return_log_z0 else pi


def soft_backward_horizon(mdp, reward, discount, horizon, terminal=None, return_value0=False):
    """Time-indexed policy ``pi_t`` [B, T, S, A] of the finite-horizon
    MaxCausalEnt model with ``T = horizon`` steps (irlmx_soft_backward_horizon):
    from ``V_T = r``, for t = T-1 .. 0, ``q_a = r + discount * (P_a V_{t+1})``,
    ``V_t = softmax_a q_a`` (the reference's pairwise fold, numpy's exp / log)
    and ``pi_t = exp(q_a - V_t)``.  No terminal state, no discount below 1 and
    no convergence test are needed (``terminal=None``, ``discount`` in [0, 1]);
    with a uint8 [B, S] mask (:func:`terminal_mask`) those states are
    absorbing, ``V_t = r``.  ``return_value0``: returns ``(pi_t, V_0 [B, S])``.
    :func:`forward_svf_horizon` under ``pi_t`` gives the gradient of ``p0 . V_0``
    with respect to the reward.

    Memory: the result is ``B * T * S * A * 8`` bytes.  STENCIL5 and ELL models;
    ``execution_plan(mdp, "soft_backward_horizon")`` names the shape."""
    lib = _lib.load()
    B, S = mdp.batch, mdp.n_states
    r = _f64(reward, mdp, (B, S))
    term = _optional_mask(terminal, mdp)
    T, pi = _horizon_policy(mdp, horizon)
    v0 = torch.empty((B, S), dtype=torch.float64, device=mdp.device) if return_value0 else None
    status = torch.empty(B, dtype=torch.int32, device=mdp.device)
    ws, n = _workspace(mdp, _lib.OP_SOFT_BACKWARD_HORIZON)
    _lib.check(lib.irlmx_soft_backward_horizon(mdp.struct(), _lib.ptr(r), _lib.ptr(term), float(discount), T,
                                               _lib.ptr(pi), _lib.ptr(v0), _lib.ptr(status), _lib.ptr(ws), n,
                                               _lib.stream_ptr(mdp.device)), "soft_backward_horizon")
    return (pi, v0) if return_value0 else pi


def forward_svf_horizon(mdp, p_initial, p_action_t, terminal=None, return_marginals=False):
    """Expected state visitation of T steps under the time-indexed policy
    ``p_action_t`` [B, T, S, A] (irlmx_forward_svf_horizon): ``d_0 = p0``,
    ``d_{t+1} = sum_a P_a^T (pi_t[:, a] * d_t)`` with the rows of terminal
    states cleared, and ``svf = d_0 + .. + d_T``.

    Returns ``(svf [B, S], sweeps [B] int64 -- T for every instance --, status
    [B] int32)`` and with ``return_marginals`` a fourth entry ``svf_t`` [B, T + 1,
    S], the marginals (``B * (T + 1) * S * 8`` bytes).  Status is
    ``_lib.NONFINITE`` exactly where ``svf`` holds a non-finite entry.  Without
    terminals ``svf`` sums to T + 1."""
    lib = _lib.load()
    B, S, A = mdp.batch, mdp.n_states, mdp.n_actions
    pi = torch.as_tensor(p_action_t, dtype=torch.float64, device=mdp.device)
    if pi.dim() != 4 or pi.shape[0] != B or tuple(pi.shape[2:]) != (S, A):
        raise ValueError(f"p_action_t must be [B = {B}, T, S = {S}, A = {A}], got {tuple(pi.shape)}")
    pi = pi.contiguous()
    T = int(pi.shape[1])
    p0 = _f64(p_initial, mdp, (B, S))
    term = _optional_mask(terminal, mdp)
    svf = torch.empty((B, S), dtype=torch.float64, device=mdp.device)
    marg = torch.empty((B, T + 1, S), dtype=torch.float64, device=mdp.device) if return_marginals else None
    status = torch.empty(B, dtype=torch.int32, device=mdp.device)
    ws, n = _workspace(mdp, _lib.OP_FORWARD_HORIZON)
    _lib.check(lib.irlmx_forward_svf_horizon(mdp.struct(), _lib.ptr(p0), _lib.ptr(term), _lib.ptr(pi), T, _lib.ptr(svf),
                                             _lib.ptr(marg), _lib.ptr(status), _lib.ptr(ws), n,
                                             _lib.stream_ptr(mdp.device)), "forward_svf_horizon")
    sweeps = torch.full((B,), T, dtype=torch.int64, device=mdp.device)
    return (svf, sweeps, status, marg) if return_marginals else (svf, sweeps, status)


_HORIZON_MODELS = {"maxent": _lib.HORIZON_MODEL_MAXENT, "causal": _lib.HORIZON_MODEL_CAUSAL,
                   _lib.HORIZON_MODEL_MAXENT: _lib.HORIZON_MODEL_MAXENT,
                   _lib.HORIZON_MODEL_CAUSAL: _lib.HORIZON_MODEL_CAUSAL}
EXPECTED_SVF_PLAN_FIELDS = ("shape", "segment", "slices", "launches", "lds_bytes", "workspace_bytes")


def _horizon_model(model):
    if model not in _HORIZON_MODELS:
        raise ValueError(f'model must be "maxent" or "causal", got {model!r}')
    return _HORIZON_MODELS[model]


def expected_svf_horizon_plan(mdp, horizon, model="maxent", segment=0):
    """The plan of :func:`expected_svf_horizon` with these arguments
    (irlmx_expected_svf_horizon_plan): shape ("fused" or "sweep", one launch
    per step), the segment length C as resolved, the [B, S] slices held,
    launches (0: one per step), LDS bytes and workspace bytes."""
    import ctypes
    lib = _lib.load()
    buf = (ctypes.c_int64 * len(EXPECTED_SVF_PLAN_FIELDS))()
    _lib.check(lib.irlmx_expected_svf_horizon_plan(mdp.struct(), _horizon_model(model), int(horizon), int(segment), buf),
               "expected_svf_horizon_plan")
    plan = dict(zip(EXPECTED_SVF_PLAN_FIELDS, [int(v) for v in buf]))
    plan["shape"] = SHAPES[plan["shape"]]
    return plan


def expected_svf_horizon(mdp, reward, p_initial, horizon, model="maxent", discount=1.0, terminal=None, segment=0,
                         return_objective=False):
    """Expected state visitation of ``T = horizon`` steps straight from the
    reward (irlmx_expected_svf_horizon): what :func:`backward_maxent_horizon`
    (``model="maxent"``) or :func:`soft_backward_horizon` (``model="causal"``,
    with ``discount`` in [0, 1]) followed by :func:`forward_svf_horizon`
    returns, bit for bit, without the policy tensor ``pi_t`` [B, T, S, A].

    The backward's state is kept every ``segment`` = C steps and each segment
    is recomputed when the forward pass reaches it, so the workspace holds about
    ``T / C + C`` vectors of [B, S] instead of ``T * A``: ``segment=0`` takes
    C = ceil(sqrt(T)), a value above T keeps every step (no recomputation).

    Returns ``(svf [B, S], sweeps [B] int64 -- T for every instance --, status
    [B] int32)`` and with ``return_objective`` a fourth entry [B, S]: ``log_z0``
    for "maxent", ``V_0`` for "causal".  Status is ``_lib.NONFINITE`` exactly
    where either call of the two-call path reports it.  STENCIL5 and ELL
    models; :func:`expected_svf_horizon_plan` names the shape."""
    lib = _lib.load()
    B, S = mdp.batch, mdp.n_states
    code = _horizon_model(model)
    T, C = int(horizon), int(segment)
    r = _f64(reward, mdp, (B, S))
    p0 = _f64(p_initial, mdp, (B, S))
    term = _optional_mask(terminal, mdp)
    svf = torch.empty((B, S), dtype=torch.float64, device=mdp.device)
    obj = torch.empty((B, S), dtype=torch.float64, device=mdp.device) if return_objective else None
    status = torch.empty(B, dtype=torch.int32, device=mdp.device)
    # (from torch's allocator on the current stream, as _workspace: 0 bytes for arguments the call refuses)
    n = int(lib.irlmx_expected_svf_horizon_workspace_bytes(mdp.struct(), code, T, C))
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device=mdp.device)
    _lib.check(lib.irlmx_expected_svf_horizon(mdp.struct(), code, _lib.ptr(r), _lib.ptr(term), _lib.ptr(p0),
                                              float(discount), T, C, _lib.ptr(svf), _lib.ptr(obj), _lib.ptr(status),
                                              _lib.ptr(ws), n, _lib.stream_ptr(mdp.device)), "expected_svf_horizon")
    sweeps = torch.full((B,), T, dtype=torch.int64, device=mdp.device)
    return (svf, sweeps, status, obj) if return_objective else (svf, sweeps, status)


def _row_targets(mdp):
    """Target state of every stored slot, int64 [tables, K, S] on the device."""
    if mdp.layout == _lib.LAYOUT_ELL:
        return mdp.row_idx.to(torch.int64).clamp(0, mdp.n_states - 1)   # (a slot of value 0 may hold any index)
    if mdp.layout != _lib.LAYOUT_STENCIL5:
        raise ValueError("STENCIL5 and ELL models only")
    W, H = mdp.width, mdp.height
    s = torch.arange(mdp.n_states, dtype=torch.int64, device=mdp.device)
    x, y = s % W, s // W
    nb = torch.stack([s, torch.where(x + 1 < W, s + 1, s), torch.where(x > 0, s - 1, s),
                      torch.where(y + 1 < H, s + W, s), torch.where(y > 0, s - W, s)])
    return nb.unsqueeze(0)


def _greedy_one_hot(mdp, value):
    """One-hot [B, S, A] of ``argmax_a (P_a value)(s)``, first index on ties: the
    policy hard-max value iteration's last sweep follows.  One pass of torch
    tensor operations over the stored slots (not a fixed-point loop)."""
    B, S, A = mdp.batch, mdp.n_states, mdp.n_actions
    nb = _row_targets(mdp)                                           # [T, K, S]
    vn = value.unsqueeze(1).expand(B, nb.shape[1], S).gather(2, nb.expand(B, -1, -1))   # [B, K, S]
    q = (mdp.row_val.to(torch.float64) * vn.unsqueeze(1)).sum(dim=2)          # [B, A, S]
    return torch.nn.functional.one_hot(q.argmax(dim=1), A).to(torch.float64)  # [B, S, A]


def expected_value_difference(mdp, true_reward, p_action, p_initial, discount, terminal=None, eps=1e-3):
    """Expected value difference of a policy under the *true* reward:
    ``evd[b] = sum_s p0[b, s] * (v*[b, s] - v_pi[b, s])``, on the device.

    Returns ``(evd [B], v_opt [B, S], v_pi [B, S])``.  ``v_pi`` is
    :func:`policy_evaluation` of ``p_action``.  Without ``terminal``, ``v*`` is
    ``value_iteration(mdp, true_reward, discount, eps)``.  ``value_iteration``
    has no terminal argument, so with ``terminal`` ``v*`` is the evaluation
    (same ``terminal``, same ``eps``) of the greedy one-hot policy of that value
    iteration: the optimal policy's value in the model whose terminal states
    end the episode.  Both values are truncated fixed points (each within
    ``eps * discount / (1 - discount)`` of its limit), so the difference of an
    optimal policy can be slightly negative.
    """
    B, S = mdp.batch, mdp.n_states
    v_opt, _, _ = value_iteration(mdp, true_reward, discount, eps)
    if terminal is not None:
        v_opt, _, _ = policy_evaluation(mdp, true_reward, _greedy_one_hot(mdp, v_opt), discount, terminal, eps)
    v_pi, _, _ = policy_evaluation(mdp, true_reward, p_action, discount, terminal, eps)
    p0 = _f64(p_initial, mdp, (B, S))
    return (p0 * (v_opt - v_pi)).sum(dim=1), v_opt, v_pi


RolloutResult = collections.namedtuple("RolloutResult", "visits starts lengths status states actions")


def _i32(x, device, shape):
    t = torch.as_tensor(x, device=device)
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError(f"expected integers, got {t.dtype}")
    return t.to(torch.int32).reshape(shape).contiguous()


def rollout_seeds(seed, batch, device):
    """The per-instance 64-bit seeds of :func:`rollout` as an int64 [B] device
    tensor (the bits are what counts): an int s gives ``seed[b] = (s &
    0xffffffff) | (b << 32)``; a sequence of B ints is taken as is, modulo 2^64."""
    if np.ndim(seed) == 0 and not isinstance(seed, torch.Tensor):
        s = [(int(seed) & 0xffffffff) | (b << 32) for b in range(batch)]
    else:
        s = [int(v) & 0xffffffffffffffff for v in (seed.tolist() if hasattr(seed, "tolist") else seed)]
        if len(s) != batch:
            raise ValueError(f"seed has {len(s)} entries for {batch} instances")
    return torch.as_tensor(np.array(s, dtype=np.uint64).view(np.int64), device=device)


def _rollout_buffers(mdp, start, n, seed, steps, return_trajectories, what):
    """What :func:`rollout` and :func:`rollout_horizon` share: ``(start [B, n] int32, seeds [B], visits,
    starts, lengths, status, states, actions)`` -- ``states`` [B, n, steps + 1] and ``actions`` [B, n, steps]
    prefilled with -1, or None (also for a ``steps`` the call is going to refuse)."""
    B, S, dev = mdp.batch, mdp.n_states, mdp.device
    if n < 1:
        raise ValueError(f"{what}: n={n} < 1")
    st = torch.as_tensor(start if isinstance(start, torch.Tensor) else np.array(start), device=dev)
    if st.dim() < 2:
        st = st.reshape(-1, 1).expand(B, n)
    st = _i32(st, dev, (B, n))
    seeds = rollout_seeds(seed, B, dev)
    visits = torch.empty((B, S), dtype=torch.int64, device=dev)
    starts = torch.empty((B, S), dtype=torch.int64, device=dev)
    lengths = torch.empty((B, n), dtype=torch.int32, device=dev)
    status = torch.empty((B, n), dtype=torch.int32, device=dev)
    states = actions = None
    if return_trajectories and 1 <= steps <= _lib.ROLLOUT_MAX_LEN:
        states = torch.full((B, n, steps + 1), -1, dtype=torch.int32, device=dev)
        actions = torch.full((B, n, steps), -1, dtype=torch.int32, device=dev)
    return st, seeds, visits, starts, lengths, status, states, actions


def rollout(mdp, p_action, terminal, start, n, max_len, seed, return_trajectories=False):
    """Sample ``n`` trajectories per instance under the policy ``p_action``
    [B, S, A] on the device (irlmx_rollout), one thread per trajectory.

    ``terminal``: a uint8 [B, S] mask (:func:`terminal_mask`).  ``start``: an
    int, ``[B]`` or ``[B, n]`` start states.  ``max_len``: the step cap, 1 to
    2^20.  ``seed``: an int s (``seed[b] = (s & 0xffffffff) | (b << 32)``) or
    ``[B]`` 64-bit seeds; the random stream of trajectory i of an instance
    depends on that instance's seed, i and the step only, so a caller that
    shards or compacts a batch passes the seeds built from the original
    instance ids and gets the same trajectories.

    Returns ``RolloutResult(visits, starts, lengths, status, states, actions)``:
    int64 [B, S] state visits (final states included) and start counts, int32
    [B, n] lengths and ``_lib.TRAJ_*`` codes, and with ``return_trajectories``
    int32 ``states`` [B, n, max_len + 1] and ``actions`` [B, n, max_len] holding
    -1 beyond each trajectory's length (else None).  The same seeds give the
    same bits on every run.  STENCIL5 and ELL models.
    """
    lib = _lib.load()
    B, S, A, dev = mdp.batch, mdp.n_states, mdp.n_actions, mdp.device
    n, max_len = int(n), int(max_len)
    st, seeds, visits, starts, lengths, status, states, actions = _rollout_buffers(mdp, start, n, seed, max_len,
                                                                                   return_trajectories, "rollout")
    pi = _f64(p_action, mdp, (B, S, A))
    term = terminal.to(device=dev, dtype=torch.uint8).reshape(B, S).contiguous()
    _lib.check(lib.irlmx_rollout(mdp.struct(), _lib.ptr(pi), _lib.ptr(term), _lib.ptr(st), _lib.ptr(seeds), n, max_len,
                                 _lib.ptr(visits), _lib.ptr(starts), _lib.ptr(lengths), _lib.ptr(status),
                                 _lib.ptr(states), _lib.ptr(actions), _lib.stream_ptr(dev)), "rollout")
    return RolloutResult(visits, starts, lengths, status, states, actions)


def _stored(states, lengths):
    dev = _lib.require_device(states.device if isinstance(states, torch.Tensor) and states.is_cuda else None)
    states = torch.as_tensor(states, device=dev)
    if states.dim() != 3:
        raise ValueError(f"states must be [B, N, L + 1], got {tuple(states.shape)}")
    B, N, stride = states.shape
    return dev, B, N, stride, _i32(states, dev, (B, N, stride)), _i32(lengths, dev, (B, N))


def demo_statistics(n_states, states, lengths):
    """``(visits [B, S] int64, starts [B, S] int64, status [B, N] int32)`` of
    stored trajectories (irlmx_demo_statistics): ``states`` int [B, N, L + 1],
    of which entries 0..lengths[b, n] are read.  ``visits / N`` and ``starts /
    N`` are the reference's feature expectation with identity features and its
    initial state distribution (maxent.py:15-60).  A trajectory with a state
    outside [0, S) or a length outside [0, L] gets status ``_lib.TRAJ_BAD_INDEX``
    and counts nothing."""
    lib = _lib.load()
    dev, B, N, stride, st, ln = _stored(states, lengths)
    S = int(n_states)
    visits = torch.empty((B, S), dtype=torch.int64, device=dev)
    starts = torch.empty((B, S), dtype=torch.int64, device=dev)
    status = torch.empty((B, N), dtype=torch.int32, device=dev)
    _lib.check(lib.irlmx_demo_statistics(S, B, N, stride, _lib.ptr(st), _lib.ptr(ln), _lib.ptr(visits),
                                         _lib.ptr(starts), _lib.ptr(status), _lib.stream_ptr(dev)), "demo_statistics")
    return visits, starts, status


def _demo_ll(fn, name, dev, B, N, stride, horizon, pi, st, actions, ln):
    """What the two log-likelihood calls share once the policy is checked: the
    actions, the outputs and one checked call of ``fn`` (``horizon``: the sizes
    between ``stride`` and the policy, ``(T,)`` or none)."""
    S, A = int(pi.shape[-2]), int(pi.shape[-1])
    if stride > 1:
        ac = _i32(actions, dev, (B, N, stride - 1))
    else:
        ac = torch.zeros(1, dtype=torch.int32, device=dev)   # no trajectory has a step: never read
    ll = torch.empty(B, dtype=torch.float64, device=dev)
    ll_traj = torch.empty((B, N), dtype=torch.float64, device=dev)
    status = torch.empty((B, N), dtype=torch.int32, device=dev)
    _lib.check(fn(S, A, B, N, stride, *horizon, _lib.ptr(pi), _lib.ptr(st), _lib.ptr(ac), _lib.ptr(ln),
                  _lib.ptr(ll_traj), _lib.ptr(ll), _lib.ptr(status), _lib.stream_ptr(dev)), name)
    return ll, ll_traj, status


def demo_log_likelihood(p_action, states, actions, lengths):
    """Log-likelihood of stored demonstrations under the policy ``p_action``
    [B, S, A] (irlmx_demo_log_likelihood): ``(ll [B], ll_traj [B, N], status
    [B, N])`` with ``ll_traj[b, n] = sum_{t < len} log p_action[b, s_t, a_t]``
    (numpy's log, added in step order) and ``ll[b]`` their sum in trajectory
    order.  ``states`` [B, N, L + 1], ``actions`` [B, N, L], as :func:`rollout`
    returns them.  A zero-probability action gives -inf; a trajectory with an
    index out of range gets status ``_lib.TRAJ_BAD_INDEX`` and NaN."""
    lib = _lib.load()
    dev, B, N, stride, st, ln = _stored(states, lengths)
    pi = torch.as_tensor(p_action, dtype=torch.float64, device=dev)
    if pi.dim() != 3 or pi.shape[0] != B:
        raise ValueError(f"p_action must be [B = {B}, S, A], got {tuple(pi.shape)}")
    return _demo_ll(lib.irlmx_demo_log_likelihood, "demo_log_likelihood", dev, B, N, stride, (), pi.contiguous(), st,
                    actions, ln)


# ---------------------------------------------------------------------------
# time-indexed policies (include/irlmx_timed.h)
# ---------------------------------------------------------------------------

def _timed_policy(p_action_t, batch, device, sizes=None):
    """``p_action_t`` as a contiguous float64 [B, T, S, A] device tensor (``sizes``: the (S, A) it must have)."""
    pi = torch.as_tensor(p_action_t, dtype=torch.float64, device=device)
    if pi.dim() != 4 or pi.shape[0] != batch or (sizes is not None and tuple(pi.shape[2:]) != tuple(sizes)):
        want = "S, A" if sizes is None else f"S = {sizes[0]}, A = {sizes[1]}"
        raise ValueError(f"p_action_t must be [B = {batch}, T, {want}], got {tuple(pi.shape)}")
    return pi.contiguous()


def rollout_horizon(mdp, p_action_t, start, n, seed, terminal=None, return_trajectories=False):
    """Sample ``n`` trajectories of T steps per instance under the time-indexed
    policy ``p_action_t`` [B, T, S, A] on the device (irlmx_rollout_horizon):
    :func:`rollout` with ``max_len = T`` whose step t draws its action from
    ``p_action_t[b, t, s]`` -- the same generator, the same ``start`` and
    ``seed`` forms, the same result tuple.  ``terminal``: ``None`` (no state
    ends a trajectory) or a uint8 [B, S] mask.  Without a terminal state every
    trajectory has length T and status ``_lib.TRAJ_TRUNCATED``: "still alive
    after T steps" is the normal outcome here.  With ``return_trajectories``
    ``states`` is [B, n, T + 1] and ``actions`` [B, n, T].  A stationary policy
    repeated T times gives :func:`rollout`'s bits."""
    lib = _lib.load()
    B, S, A, dev = mdp.batch, mdp.n_states, mdp.n_actions, mdp.device
    n = int(n)
    pi = _timed_policy(p_action_t, B, dev, (S, A))
    T = int(pi.shape[1])
    st, seeds, visits, starts, lengths, status, states, actions = _rollout_buffers(mdp, start, n, seed, T,
                                                                                   return_trajectories, "rollout_horizon")
    term = _optional_mask(terminal, mdp)
    _lib.check(lib.irlmx_rollout_horizon(mdp.struct(), _lib.ptr(pi), _lib.ptr(term), _lib.ptr(st), _lib.ptr(seeds), n, T,
                                         _lib.ptr(visits), _lib.ptr(starts), _lib.ptr(lengths), _lib.ptr(status),
                                         _lib.ptr(states), _lib.ptr(actions), _lib.stream_ptr(dev)), "rollout_horizon")
    return RolloutResult(visits, starts, lengths, status, states, actions)


def demo_log_likelihood_horizon(p_action_t, states, actions, lengths):
    """Log-likelihood of stored demonstrations under the time-indexed policy
    ``p_action_t`` [B, T, S, A] (irlmx_demo_log_likelihood_horizon): ``(ll [B],
    ll_traj [B, N], status [B, N])`` with ``ll_traj[b, n] = sum_{t < len} log
    p_action_t[b, t, s_t, a_t]`` (numpy's log, added in step order) and
    ``ll[b]`` their sum in trajectory order.  ``states`` [B, N, L + 1],
    ``actions`` [B, N, L], as :func:`rollout_horizon` returns them (L = T) or
    any other L.  A zero-probability action gives -inf; a trajectory longer
    than T or with an index out of range gets status ``_lib.TRAJ_BAD_INDEX``
    and NaN."""
    lib = _lib.load()
    dev, B, N, stride, st, ln = _stored(states, lengths)
    pi = _timed_policy(p_action_t, B, dev)
    return _demo_ll(lib.irlmx_demo_log_likelihood_horizon, "demo_log_likelihood_horizon", dev, B, N, stride,
                    (int(pi.shape[1]),), pi, st, actions, ln)


def value_horizon(mdp, reward, horizon, p_action_t=None, discount=1.0, terminal=None, return_values=False):
    """Finite-horizon value of ``reward`` over ``T = horizon`` steps
    (irlmx_value_horizon): from ``v_T = r``, for t = T-1 .. 0, ``v_t = r +
    discount * sum_a p_action_t[:, t, :, a] * (P_a v_{t+1})`` under the
    time-indexed policy ``p_action_t`` [B, T, S, A], or with ``p_action_t=None``
    the optimal value ``v_t = max_a (r + discount * P_a v_{t+1})``.  A visited
    state contributes its reward, the final one included; with a uint8 [B, S]
    mask ``terminal`` those states are absorbing, ``v_t = r``.

    Returns ``(value0 [B, S], status [B])`` and with ``return_values`` a third
    entry ``value_t`` [B, T + 1, S], ``v_0 .. v_T``.  Status is
    ``_lib.NONFINITE`` exactly where ``value0`` holds a non-finite entry.  At
    discount 1, ``p0 . value0`` equals ``svf . r`` of
    :func:`forward_svf_horizon` under the same policy.  STENCIL5 and ELL
    models; ``execution_plan(mdp, "value_horizon")`` names the shape."""
    lib = _lib.load()
    B, S, A = mdp.batch, mdp.n_states, mdp.n_actions
    r = _f64(reward, mdp, (B, S))
    T = int(horizon)
    pi = None
    if p_action_t is not None:
        pi = _timed_policy(p_action_t, B, mdp.device, (S, A))
        if pi.shape[1] != T:
            raise ValueError(f"p_action_t holds {pi.shape[1]} steps for horizon {T}")
    term = _optional_mask(terminal, mdp)
    v0 = torch.empty((B, S), dtype=torch.float64, device=mdp.device)
    vt = None
    if return_values:
        vt = torch.empty((B, (T if 1 <= T <= _lib.HORIZON_MAX else 1) + 1, S), dtype=torch.float64, device=mdp.device)
    status = torch.empty(B, dtype=torch.int32, device=mdp.device)
    ws, n = _workspace(mdp, _lib.OP_VALUE_HORIZON)
    _lib.check(lib.irlmx_value_horizon(mdp.struct(), _lib.ptr(r), _lib.ptr(term), _lib.ptr(pi), float(discount), T,
                                       _lib.ptr(v0), _lib.ptr(vt), _lib.ptr(status), _lib.ptr(ws), n,
                                       _lib.stream_ptr(mdp.device)), "value_horizon")
    return (v0, status, vt) if return_values else (v0, status)


def expected_value_difference_horizon(mdp, true_reward, p_action_t, p_initial, discount=1.0, terminal=None):
    """Expected value difference of a time-indexed policy under the *true*
    reward over its T steps: ``evd[b] = sum_s p0[b, s] * (v*_0[b, s] -
    v_pi_0[b, s])``, two :func:`value_horizon` calls and a dot product.

    Returns ``(evd [B], v_opt [B, S], v_pi [B, S])``.  Both values are exact
    T-step recursions (no convergence test), so ``evd`` is non-negative up to
    rounding for rows that sum to at most 1."""
    B, S = mdp.batch, mdp.n_states
    pi = _timed_policy(p_action_t, B, mdp.device, (S, mdp.n_actions))
    T = int(pi.shape[1])
    v_opt, _ = value_horizon(mdp, true_reward, T, None, discount, terminal)
    v_pi, _ = value_horizon(mdp, true_reward, T, pi, discount, terminal)
    p0 = _f64(p_initial, mdp, (B, S))
    return (p0 * (v_opt - v_pi)).sum(dim=1), v_opt, v_pi


def dense_gemm(m, z):
    """``z @ m.T`` on the fp64 matrix cores (irlmx_dense_gemm): m [R, S], z [B, S]
    float64 device tensors -> [B, R].  The batched P . [v_1 .. v_B] contraction
    of the DENSE layout's shared-table sweeps."""
    lib = _lib.load()
    m = m.to(dtype=torch.float64).contiguous()
    z = z.to(dtype=torch.float64, device=m.device).contiguous()
    (R, S), (B, S2) = m.shape, z.shape
    if S2 != S:
        raise ValueError(f"dense_gemm: m is {tuple(m.shape)}, z is {tuple(z.shape)}")
    c = torch.empty((B, R), dtype=torch.float64, device=m.device)
    _lib.check(lib.irlmx_dense_gemm(_lib.ptr(m), _lib.ptr(z), _lib.ptr(c), R, S, B, _lib.stream_ptr(m.device)),
               "dense_gemm")
    return c


def dense_gemm_variant(rows, n, batch):
    """(row tiles, instance tiles, waves, 16-byte loads) of the MFMA kernel a
    dense_gemm of these sizes launches."""
    import ctypes
    lib = _lib.load()
    v = (ctypes.c_int32 * 4)()
    _lib.check(lib.irlmx_dense_gemm_variant(rows, n, batch, v), "dense_gemm_variant")
    return tuple(int(x) for x in v)


def optimal_policy(successor, value):
    """argmax_a value[successor[s, a]] per state, first index on ties (solver.py:107-124)."""
    lib = _lib.load()
    succ = successor.to(dtype=torch.int32).contiguous()
    S, A = succ.shape
    value = value.to(dtype=torch.float64).reshape(-1, S).contiguous()
    B = value.shape[0]
    out = torch.empty((B, S), dtype=torch.int64, device=value.device)
    _lib.check(lib.irlmx_optimal_policy(_lib.ptr(succ), S, A, B, _lib.ptr(value), _lib.ptr(out),
                                        _lib.stream_ptr(value.device)), "optimal_policy")
    return out


def stochastic_policy(successor, weighted_value):
    """w(value)[successor] normalised per state (solver.py:155-181)."""
    lib = _lib.load()
    succ = successor.to(dtype=torch.int32).contiguous()
    S, A = succ.shape
    wv = weighted_value.to(dtype=torch.float64).reshape(-1, S).contiguous()
    B = wv.shape[0]
    out = torch.empty((B, S, A), dtype=torch.float64, device=wv.device)
    _lib.check(lib.irlmx_stochastic_policy(_lib.ptr(succ), S, A, B, _lib.ptr(wv), _lib.ptr(out),
                                           _lib.stream_ptr(wv.device)), "stochastic_policy")
    return out


__all__ = ["DeviceMDP", "execution_plan", "numpy_order_default", "counters", "terminal_mask", "backward_maxent", "backward_maxent_extended", "backward_maxent_horizon", "forward_svf", "forward_svf_horizon", "soft_backward",
           "soft_backward_horizon", "expected_svf_horizon", "expected_svf_horizon_plan",
           "value_iteration", "policy_evaluation", "expected_value_difference", "rollout", "rollout_seeds",
           "demo_statistics", "demo_log_likelihood", "RolloutResult", "rollout_horizon", "demo_log_likelihood_horizon",
           "value_horizon", "expected_value_difference_horizon", "dense_gemm", "dense_gemm_variant", "optimal_policy", "stochastic_policy"]
