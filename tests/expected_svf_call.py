"""Calls of include/irlmx_expected_svf.h's entry point under the call contract and
the stream order of include/irlmx.h (not a test module): what tests/timed_call.py
is to irlmx_timed.h, for the header of the one-call expected SVF.

* ``expected_svf_horizon``: the wrapper, as tests/abi_call.py's, with the
  workspace sized by irlmx_expected_svf_horizon_workspace_bytes (the size
  depends on T and C, which irlmx_workspace_bytes cannot express);
* ``CLAIMS``: (entry point, shape) -> the header's claim, "asynchronous, both shapes";
* ``ROWS``: one row per (model, shape), run by tests/test_gpu_expected_svf.py
  through ``abi_call.stream_call`` as test_gpu_stream_order runs its rows.
"""

import collections
import ctypes
import inspect

import torch

import abi_call as A
import horizon_twin as H

ASYNC = "async"
ENTRY = "irlmx_expected_svf_horizon"
MODELS = {"maxent": 0, "causal": 1}


def expected_svf_horizon(mdp, model, reward, p_initial, horizon, discount=1.0, terminal=None, segment=0, objective0=True,
                         fill="zero", donor=None, side=None):
    """irlmx_expected_svf_horizon: {"svf" [B, S], "objective0" [B, S] or None (``objective0=False``: NULL), "status"}.
    ``donor``: ``reward``, ``p_initial``."""
    from irlmx import _lib
    lib = _lib.load()
    B, S, T, C, dev, code = mdp.batch, mdp.n_states, int(horizon), int(segment), mdp.device, MODELS[model]
    out = {"svf": A._out(torch.float64, (B, S), dev), "objective0": A._out(torch.float64, (B, S), dev, objective0),
           "status": A._out(torch.int32, (B,), dev)}
    n = int(lib.irlmx_expected_svf_horizon_workspace_bytes(mdp.struct(), code, T, C))
    assert n > 0 and n % 256 == 0, n

    def call(ws, n_, st, reward=reward, p_initial=p_initial, terminal=terminal):
        r, p0 = A._in(reward, torch.float64, (B, S), dev), A._in(p_initial, torch.float64, (B, S), dev)
        tm = A._in(terminal, torch.uint8, (B, S), dev)
        rc = lib.irlmx_expected_svf_horizon(mdp.struct(), code, _lib.ptr(r), _lib.ptr(tm), _lib.ptr(p0), float(discount),
                                            T, C, _lib.ptr(out["svf"]), _lib.ptr(out["objective0"]),
                                            _lib.ptr(out["status"]), ctypes.c_void_p(ws), n_,
                                            st if st is not None else _lib.stream_ptr(dev))
        _lib.check(rc, ENTRY)
        return r, p0, tm

    if side is not None:              # (as abi_call._run: every tensor of ``donor`` names an input that lands late)
        late = {k: v for k, v in (donor or {}).items() if isinstance(v, torch.Tensor)}
        params = inspect.signature(call).parameters
        real = {k: params[k].default for k in late}
        return A.stream_call(ENTRY, dev, n, out, call, real, late, side)
    return A.contract_call(ENTRY, dev, n, out, lambda ws, n_, **inputs: call(ws, n_, None, **inputs), fill, donor)


#: (entry point, shape) -> the header's claim
CLAIMS = {(ENTRY, "fused"): ASYNC, (ENTRY, "sweep"): ASYNC}

Row = collections.namedtuple("Row", "id entry shape keys build")
ROWS = []


def _row(model, discount, shape, keys):
    def build(dev):
        import test_gpu_call_contract as CC
        import test_gpu_stream_order as SO
        from irlmx import ops
        c = H.case("16x16")
        mdp = c.device_model(dev)
        assert ops.expected_svf_horizon_plan(mdp, c.T, model)["shape"] == shape
        r, p0 = SO.dv(c.reward, dev), SO.dv(c.p0, dev)
        donor = {"reward": SO.dv(CC.other_reward(c.reward), dev), "p_initial": SO.dv(CC.other_p0(c.p0), dev)}
        return lambda side: expected_svf_horizon(mdp, model, r, p0, c.T, discount, donor=donor, side=side)
    ROWS.append(Row(f"16x16/{shape}/{model}", ENTRY, shape, keys, build))


for _shape, _keys in (("fused", {}), ("sweep", {"IRLMX_FUSED_MAX_STATES": 0})):
    _row("maxent", 1.0, _shape, _keys)
    _row("causal", 0.9, _shape, _keys)

ROW = {r.id: r for r in ROWS}
assert len(ROW) == len(ROWS) and {(r.entry, r.shape) for r in ROWS} == set(CLAIMS)
