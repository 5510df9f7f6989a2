"""irlmx_soft_backward_horizon under the call contract of include/irlmx.h (not a
test module): the entry point on tests/abi_call.py's guarded arena, in the
manner of that module's own wrappers, whose table this one extends."""

import torch

import abi_call as A


def soft_backward_horizon(mdp, reward, discount, horizon, terminal=None, value0=True, fill="zero", donor=None):
    """irlmx_soft_backward_horizon: {"p_action_t" [B, T, S, A], "value0" [B, S] or None (``value0=False``: NULL),
    "status"}.  ``donor``: ``reward``."""
    from irlmx import _lib
    B, S, A_, T, dev = mdp.batch, mdp.n_states, mdp.n_actions, int(horizon), mdp.device
    out = {"p_action_t": A._out(torch.float64, (B, T, S, A_), dev), "value0": A._out(torch.float64, (B, S), dev, value0),
           "status": A._out(torch.int32, (B,), dev)}

    def call(lib, ws, n, st, reward=reward):
        r, tm = A._in(reward, torch.float64, (B, S), dev), A._in(terminal, torch.uint8, (B, S), dev)
        return lib.irlmx_soft_backward_horizon(mdp.struct(), _lib.ptr(r), _lib.ptr(tm), float(discount), T,
                                               _lib.ptr(out["p_action_t"]), _lib.ptr(out["value0"]),
                                               _lib.ptr(out["status"]), ws, n, st), (r, tm)

    return A._run("irlmx_soft_backward_horizon", mdp, _lib.OP_SOFT_BACKWARD_HORIZON, out, call, fill, donor)


#: C name -> wrapper, beside abi_call.WRAPPED (a closed table: tests/test_call_contract_host.py pins its eight
#: entry points by the parameter name ``void* workspace``; this entry's is ``void* workspace_mem``, and
#: tests/test_gpu_soft_horizon_contract.py holds that this table covers every such declaration)
WRAPPED = {"irlmx_soft_backward_horizon": soft_backward_horizon}


def declared_with_workspace_mem(header):
    """Entry points of include/irlmx.h with a ``void* workspace_mem`` parameter (the other table's parser, for this name)."""
    import re
    text = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
    return {name for name, params in re.findall(r"\b(irlmx_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
            if re.search(r"\bvoid\s*\*\s*workspace_mem\b", params)}
