"""Calls of include/irlmx_timed.h's entry points under the call contract and the
stream order of include/irlmx.h (not a test module): what tests/abi_call.py's
``WRAPPED`` and tests/test_gpu_stream_order.py's ``CLAIMS`` / ``ROWS`` are to
irlmx.h, for the header of the time-indexed policies.

* ``WRAPPED``: C name -> wrapper, every entry point with a ``void* workspace``;
* ``CLAIMS``: (entry point, shape) -> whether the call may synchronise
  ``stream``, in the header's words ("asynchronous, both shapes");
* ``ROWS``: one row per (entry point, shape), run by
  tests/test_gpu_timed_contract.py through ``abi_call.stream_call`` exactly as
  test_gpu_stream_order runs its rows.

tests/test_abi_timed.py holds the three tables to the header without a device.
The builders import the GPU suites' helpers only when they run.
"""

import collections

import numpy as np
import torch

import abi_call as A
import horizon_twin as H

ASYNC = "async"


def value_horizon(mdp, reward, horizon, p_action_t=None, discount=1.0, terminal=None, value_t=True, fill="zero",
                  donor=None, side=None):
    """irlmx_value_horizon: {"value0" [B, S], "value_t" [B, T + 1, S] or None (``value_t=False``: NULL), "status"}.
    ``donor``: ``reward``, ``p_action_t`` (of the same horizon)."""
    from irlmx import _lib
    B, S, A_, T, dev = mdp.batch, mdp.n_states, mdp.n_actions, int(horizon), mdp.device
    out = {"value0": A._out(torch.float64, (B, S), dev), "value_t": A._out(torch.float64, (B, T + 1, S), dev, value_t),
           "status": A._out(torch.int32, (B,), dev)}

    def call(lib, ws, n, st, reward=reward, p_action_t=p_action_t, terminal=terminal):
        r, tm = A._in(reward, torch.float64, (B, S), dev), A._in(terminal, torch.uint8, (B, S), dev)
        pi = A._in(p_action_t, torch.float64, (B, T, S, A_), dev)
        return lib.irlmx_value_horizon(mdp.struct(), _lib.ptr(r), _lib.ptr(tm), _lib.ptr(pi), float(discount), T,
                                       _lib.ptr(out["value0"]), _lib.ptr(out["value_t"]), _lib.ptr(out["status"]), ws, n,
                                       st), (r, tm, pi)

    return A._run("irlmx_value_horizon", mdp, _lib.OP_VALUE_HORIZON, out, call, fill, donor, side)


#: C name -> the function above that calls it: every entry point of include/irlmx_timed.h with a ``void* workspace``
WRAPPED = {"irlmx_value_horizon": value_horizon}

#: (entry point, shape) -> the header's claim.  "-": the entry point has one shape.
CLAIMS = {
    ("irlmx_value_horizon", "fused"): ASYNC,
    ("irlmx_value_horizon", "sweep"): ASYNC,
    ("irlmx_rollout_horizon", "-"): ASYNC,
    ("irlmx_demo_log_likelihood_horizon", "-"): ASYNC,
}

Row = collections.namedtuple("Row", "id entry shape keys build")
ROWS = []


def row(id_, entry, shape, keys):
    assert (entry, shape) in CLAIMS, (entry, shape)

    def add(build):
        ROWS.append(Row(id_, entry, shape, keys, build))
        return build
    return add


ROLL_N = 24      # trajectories per instance of the two trajectory rows


def case_inputs(dev):
    """16x16 (B = 3, T = 40) on the device: (case, model, reward, the device's own non-causal pi_t)."""
    import test_gpu_stream_order as SO
    from irlmx import ops
    c = H.case("16x16")
    mdp = c.device_model(dev)
    r = SO.dv(c.reward, dev)
    return c, mdp, r, ops.backward_maxent_horizon(mdp, r, c.T, None)


for _shape, _keys in (("fused", {}), ("sweep", {"IRLMX_FUSED_MAX_STATES": 0})):
    @row(f"16x16/{_shape}/value-horizon", "irlmx_value_horizon", _shape, _keys)
    def _value(dev, shape=_shape):
        import test_gpu_call_contract as CC
        import test_gpu_stream_order as SO
        from irlmx import ops
        c, mdp, r, pi = case_inputs(dev)
        assert ops.execution_plan(mdp, "value_horizon")["shape"] == shape
        donor = {"reward": SO.dv(CC.other_reward(c.reward), dev),
                 "p_action_t": SO.dv(CC.uniform_policy(tuple(pi.shape)), dev)}
        return lambda side: value_horizon(mdp, r, c.T, pi, 0.9, None, donor=donor, side=side)


@row("16x16/rollout-horizon", "irlmx_rollout_horizon", "-", {})
def _rollout(dev):
    import test_gpu_call_contract as CC
    import test_gpu_stream_order as SO
    from irlmx import _lib, ops
    c, mdp, _, pi = case_inputs(dev)
    B, S, T, N = c.B, c.S, c.T, ROLL_N
    I32, I64 = torch.int32, torch.int64
    start = SO.dv(np.random.default_rng(31).integers(0, S, (B, N)), dev, dtype=I32)
    seeds = ops.rollout_seeds(77, B, dev)

    def fn(lib, st, out, extra, p_action_t, start, seed):
        extra["states"].fill_(-1)                  # (in stream order, as ops.rollout_horizon prefills them)
        extra["actions"].fill_(-1)
        return lib.irlmx_rollout_horizon(mdp.struct(), _lib.ptr(p_action_t), None, _lib.ptr(start), _lib.ptr(seed), N, T,
                                         _lib.ptr(out["visits"]), _lib.ptr(out["starts"]), _lib.ptr(out["lengths"]),
                                         _lib.ptr(out["traj_status"]), _lib.ptr(extra["states"]),
                                         _lib.ptr(extra["actions"]), st)

    return SO.free_call("irlmx_rollout_horizon", dev,
                        lambda: {"visits": SO.empty(dev, I64, B, S), "starts": SO.empty(dev, I64, B, S),
                                 "lengths": SO.empty(dev, I32, B, N), "traj_status": SO.empty(dev, I32, B, N)},
                        fn, {"p_action_t": pi, "start": start, "seed": seeds},
                        {"p_action_t": SO.dv(CC.uniform_policy(tuple(pi.shape)), dev), "start": SO.other_index(start, S),
                         "seed": seeds + 1},
                        lambda: {"states": SO.empty(dev, I32, B, N, T + 1), "actions": SO.empty(dev, I32, B, N, T)})


@row("16x16/demo-log-likelihood-horizon", "irlmx_demo_log_likelihood_horizon", "-", {})
def _log_likelihood(dev):
    import test_gpu_call_contract as CC
    import test_gpu_stream_order as SO
    from irlmx import _lib, ops
    c, mdp, _, pi = case_inputs(dev)
    B, S, A_, T, N = c.B, c.S, c.A, c.T, ROLL_N
    start = np.random.default_rng(31).integers(0, S, (B, N))
    got = ops.rollout_horizon(mdp, pi, start, N, 77, return_trajectories=True)
    real = {"p_action_t": pi, "states": got.states, "actions": got.actions, "lengths": got.lengths}
    donor = {"p_action_t": SO.dv(CC.uniform_policy(tuple(pi.shape)), dev), "states": SO.other_index(got.states, S),
             "actions": SO.other_index(got.actions, A_), "lengths": SO.other_index(got.lengths, T + 1)}
    F64, I32 = torch.float64, torch.int32
    return SO.free_call("irlmx_demo_log_likelihood_horizon", dev,
                        lambda: {"ll_traj": SO.empty(dev, F64, B, N), "ll": SO.empty(dev, F64, B),
                                 "traj_status": SO.empty(dev, I32, B, N)},
                        lambda lib, st, out, _, p_action_t, states, actions, lengths:
                        lib.irlmx_demo_log_likelihood_horizon(
                            S, A_, B, N, T + 1, T, _lib.ptr(p_action_t), _lib.ptr(states), _lib.ptr(actions),
                            _lib.ptr(lengths), _lib.ptr(out["ll_traj"]), _lib.ptr(out["ll"]),
                            _lib.ptr(out["traj_status"]), st),
                        real, donor)


ROW = {r.id: r for r in ROWS}
assert len(ROW) == len(ROWS)
#: every entry point the rows run: tests/test_abi_timed.py holds it equal to the header's set with a ``void* stream``
ENTRY_POINTS = sorted({r.entry for r in ROWS})
