"""Failure paths of irlmx_backward_maxent_horizon / irlmx_forward_svf_horizon and
of IRLMX_OP_BACKWARD_HORIZON / IRLMX_OP_FORWARD_HORIZON in the model queries,
through ctypes, in the manner of tests/test_abi_policy_eval.py: every call
fails in the argument check, so the non-NULL array pointers are never
dereferenced and no GPU is needed.
"""

import ctypes

import pytest

EINVAL, EWORKSPACE = -1, -3
OP_B, OP_F = 8, 9   # IRLMX_OP_BACKWARD_HORIZON, IRLMX_OP_FORWARD_HORIZON (5 and 7 stay unknown ops)
PLAN_NO_RESCALE, PLAN_EXTENDED_RANGE = 0x100, 0x200
DENSE_MSG = "the finite-horizon passes do not run the DENSE layout (STENCIL5 and ELL only)"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from irlmx import _lib
    assert (_lib.OP_BACKWARD_HORIZON, _lib.OP_FORWARD_HORIZON) == (OP_B, OP_F)
    return _lib.load()


_keep = []
NULL = ctypes.c_void_p(0)


def fake():
    """A non-NULL address that the argument checks never dereference."""
    b = ctypes.create_string_buffer(64)
    _keep.append(b)
    return ctypes.cast(b, ctypes.c_void_p)


def model(layout=1, S=25, A=4, W=5, H=5, k_row=5, k_col=5, B=1, shared=1, row_idx=False, col=False):
    from irlmx import _lib
    m = _lib.MDPStruct()
    m.layout, m.n_states, m.n_actions, m.width, m.height = layout, S, A, W, H
    m.k_row, m.k_col, m.batch, m.shared = k_row, k_col, B, shared
    m.row_val = fake().value
    m.row_idx = fake().value if row_idx else None
    m.col_idx = fake().value if col and layout == 2 else None
    m.col_val = fake().value if col else None
    return m


def err(lib):
    return lib.irlmx_last_error().decode()


BIG = model(S=128 * 40, W=128, H=40, B=2, shared=0)


def backward(lib, m, horizon=10, **over):
    a = {k: fake() for k in ("reward", "terminal", "p_action_t", "log_z0", "status", "ws")}
    a["n"] = int(lib.irlmx_workspace_bytes(ctypes.byref(m), OP_B)) if m is not None else 0
    a.update(over)
    mp = ctypes.byref(m) if m is not None else None
    return lib.irlmx_backward_maxent_horizon(mp, a["reward"], a["terminal"], horizon, a["p_action_t"], a["log_z0"],
                                             a["status"], a["ws"], a["n"], NULL)


def forward(lib, m, horizon=10, **over):
    a = {k: fake() for k in ("p_initial", "terminal", "p_action_t", "svf", "svf_t", "status", "ws")}
    a["n"] = int(lib.irlmx_workspace_bytes(ctypes.byref(m), OP_F)) if m is not None else 0
    a.update(over)
    mp = ctypes.byref(m) if m is not None else None
    return lib.irlmx_forward_svf_horizon(mp, a["p_initial"], a["terminal"], a["p_action_t"], horizon, a["svf"],
                                         a["svf_t"], a["status"], a["ws"], a["n"], NULL)


def test_symbols_exported_and_bound(lib):
    from irlmx import _lib, ops
    import irlmx
    for name in ("irlmx_backward_maxent_horizon", "irlmx_forward_svf_horizon"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name in ("backward_maxent_horizon", "forward_svf_horizon"):
        assert callable(getattr(ops, name)) and name in ops.__all__ and getattr(irlmx, name) is getattr(ops, name)
    assert lib.irlmx_abi_version() == 1


def test_null_arguments(lib):
    assert backward(lib, None) == EINVAL and err(lib) == "mdp is NULL"
    assert forward(lib, None) == EINVAL and err(lib) == "mdp is NULL"
    for name in ("reward", "p_action_t", "status"):
        assert backward(lib, model(), **{name: NULL}) == EINVAL, name
        assert err(lib) == f"backward_maxent_horizon: {name} is NULL", (name, err(lib))
    for name in ("p_initial", "p_action_t", "svf", "status"):
        assert forward(lib, model(), **{name: NULL}) == EINVAL, name
        assert err(lib) == f"forward_svf_horizon: {name} is NULL", (name, err(lib))


def test_optional_arguments_may_be_null(lib):
    """terminal, log_z0 and svf_t: the call then gets as far as the workspace
    check (on the per-sweep model, whose workspace is not empty)."""
    assert backward(lib, BIG, terminal=NULL, log_z0=NULL, n=0, ws=NULL) == EWORKSPACE
    assert forward(lib, BIG, terminal=NULL, svf_t=NULL, n=0, ws=NULL) == EWORKSPACE


@pytest.mark.parametrize("horizon", [0, -1, 2 ** 20 + 1])
def test_horizon_out_of_range(lib, horizon):
    assert backward(lib, model(), horizon=horizon) == EINVAL
    assert err(lib) == f"backward_maxent_horizon: horizon {horizon} outside [1, 1048576]", err(lib)
    assert forward(lib, model(), horizon=horizon) == EINVAL
    assert err(lib) == f"forward_svf_horizon: horizon {horizon} outside [1, 1048576]", err(lib)


def test_bad_model(lib):
    assert backward(lib, model(S=0)) == EINVAL and "bad sizes S=0" in err(lib)
    assert backward(lib, model(layout=2, k_row=3)) == EINVAL and err(lib) == "ELL row form missing"
    assert forward(lib, model(layout=2, k_row=3, row_idx=True)) == EINVAL and err(lib) == "ELL column form missing"
    # more column slots than states: refused as irlmx_forward_svf refuses it (the kernels would index past the column form)
    wide = model(layout=2, k_row=3, k_col=30, row_idx=True, col=True)
    assert forward(lib, wide) == EINVAL and err(lib) == "ELL k_col=30 out of range (1..25)", err(lib)


def test_dense_layout_refused(lib):
    m = model(layout=3, k_row=25, k_col=25, col=True)
    assert backward(lib, m) == EINVAL and err(lib) == "backward_maxent_horizon: " + DENSE_MSG
    assert forward(lib, m) == EINVAL and err(lib) == "forward_svf_horizon: " + DENSE_MSG
    plan = (ctypes.c_int64 * 10)()
    for op in (OP_B, OP_F):
        assert lib.irlmx_workspace_bytes(ctypes.byref(m), op) == 0
        assert lib.irlmx_execution_plan(ctypes.byref(m), op, plan) == EINVAL
        assert err(lib) == "execution_plan: " + DENSE_MSG


def test_workspace(lib):
    """Fused models need none; a per-sweep model needs its ping-pong buffers
    (backward: mantissas, exponents and the flags; forward: d_t), whatever T."""
    small = model(B=4, shared=0)
    assert lib.irlmx_workspace_bytes(ctypes.byref(small), OP_B) == 0
    assert lib.irlmx_workspace_bytes(ctypes.byref(small), OP_F) == 0
    S, B = 128 * 40, 2
    need_b = int(lib.irlmx_workspace_bytes(ctypes.byref(BIG), OP_B))
    need_f = int(lib.irlmx_workspace_bytes(ctypes.byref(BIG), OP_F))
    assert need_b == 256 + 2 * B * S * 8 + 2 * B * S * 4 and need_f == 2 * B * S * 8, (need_b, need_f)
    for call, need in ((backward, need_b), (forward, need_f)):
        for got, ws in ((0, fake()), (need - 1, fake()), (need, NULL)):
            assert call(lib, BIG, n=got, ws=ws) == EWORKSPACE, got
            assert err(lib) == f"workspace too small: need {need} bytes, got {got}", err(lib)


def test_plan_and_flags(lib):
    plan = (ctypes.c_int64 * 10)()
    m = model()
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP_B, plan) == 0
    assert list(plan) == [0, 0, 0, 0, 0, 1, 0, 64, 1, 24 * 25], list(plan)     # fused: 25 states, one wave
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP_F, plan) == 0
    assert list(plan) == [0, 0, 0, 0, 0, 1, 0, 64, 1, 16 * 25], list(plan)
    for op in (OP_B, OP_F):
        assert lib.irlmx_execution_plan(ctypes.byref(BIG), op, plan) == 0
        assert list(plan) == [2, 0, 0, 0, 0, 1, 0, 256, 0, 0], list(plan)      # one launch per step
    wide = model(layout=2, S=300, k_row=40, k_col=3, row_idx=True, col=True)
    assert lib.irlmx_execution_plan(ctypes.byref(wide), OP_B, plan) == 0 and plan[0] == 2
    assert lib.irlmx_execution_plan(ctypes.byref(wide), OP_F, plan) == 0 and plan[0] == 0
    # the backward-only flags keep their messages
    for op in (OP_B, OP_F):
        assert lib.irlmx_execution_plan(ctypes.byref(m), op | PLAN_EXTENDED_RANGE, plan) == EINVAL
        assert "IRLMX_PLAN_EXTENDED_RANGE applies to IRLMX_OP_BACKWARD only" in err(lib)
        assert lib.irlmx_workspace_bytes(ctypes.byref(m), op | PLAN_EXTENDED_RANGE) == 0
        assert lib.irlmx_execution_plan(ctypes.byref(m), op | PLAN_NO_RESCALE, plan) == EINVAL
        assert "NO_RESCALE applies to IRLMX_OP_BACKWARD only" in err(lib)
    for op in (5, 7, 10):
        assert lib.irlmx_execution_plan(ctypes.byref(m), op, plan) == EINVAL and err(lib) == f"unknown op {op}"
