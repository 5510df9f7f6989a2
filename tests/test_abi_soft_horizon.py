"""Failure paths of irlmx_soft_backward_horizon and of
IRLMX_OP_SOFT_BACKWARD_HORIZON in the model queries, through ctypes, in the
manner of tests/test_abi_horizon.py: every call fails in the argument check, so
the non-NULL array pointers are never dereferenced and no GPU is needed.
"""

import ctypes

import pytest

EINVAL, EWORKSPACE = -1, -3
OP = 11   # IRLMX_OP_SOFT_BACKWARD_HORIZON (5, 7 and 10 stay unknown ops)
FN = "soft_backward_horizon"
DENSE_MSG = "the finite-horizon passes do not run the DENSE layout (STENCIL5 and ELL only)"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from irlmx import _lib
    assert _lib.OP_SOFT_BACKWARD_HORIZON == OP
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


def call(lib, m, horizon=10, discount=0.9, **over):
    a = {k: fake() for k in ("reward", "terminal", "p_action_t", "value0", "status", "ws")}
    a["n"] = int(lib.irlmx_workspace_bytes(ctypes.byref(m), OP)) if m is not None else 0
    a.update(over)
    mp = ctypes.byref(m) if m is not None else None
    return lib.irlmx_soft_backward_horizon(mp, a["reward"], a["terminal"], discount, horizon, a["p_action_t"],
                                           a["value0"], a["status"], a["ws"], a["n"], NULL)


def test_symbol_exported_and_bound(lib):
    from irlmx import _lib, ops
    import irlmx
    assert hasattr(lib, "irlmx_soft_backward_horizon") and "irlmx_soft_backward_horizon" in _lib.SIGNATURES
    assert callable(ops.soft_backward_horizon) and "soft_backward_horizon" in ops.__all__
    assert irlmx.soft_backward_horizon is ops.soft_backward_horizon
    assert lib.irlmx_abi_version() == 1


def test_null_arguments(lib):
    assert call(lib, None) == EINVAL and err(lib) == "mdp is NULL"
    for name in ("reward", "p_action_t", "status"):
        assert call(lib, model(), **{name: NULL}) == EINVAL, name
        assert err(lib) == f"{FN}: {name} is NULL", (name, err(lib))


def test_optional_arguments_may_be_null(lib):
    """terminal and value0: the call then gets as far as the workspace check (on
    the per-sweep model, whose workspace is not empty)."""
    assert call(lib, BIG, terminal=NULL, value0=NULL, n=0, ws=NULL) == EWORKSPACE


@pytest.mark.parametrize("horizon", [0, -1, 2 ** 20 + 1])
def test_horizon_out_of_range(lib, horizon):
    assert call(lib, model(), horizon=horizon) == EINVAL
    assert err(lib) == f"{FN}: horizon {horizon} outside [1, 1048576]", err(lib)
    assert call(lib, BIG, horizon=2 ** 20, n=0, ws=NULL) == EWORKSPACE      # the largest horizon passes the check


@pytest.mark.parametrize("discount,text", [(-0.1, "-0.1"), (1.5, "1.5"), (float("nan"), "nan"), (float("inf"), "inf")])
def test_discount_out_of_range(lib, discount, text):
    assert call(lib, model(), discount=discount) == EINVAL
    assert err(lib).replace("-nan", "nan") == f"{FN}: discount {text} outside [0, 1]", err(lib)
    for ok in (0.0, 1.0):
        assert call(lib, BIG, discount=ok, n=0, ws=NULL) == EWORKSPACE


def test_bad_model(lib):
    assert call(lib, model(S=0)) == EINVAL and "bad sizes S=0" in err(lib)
    assert call(lib, model(layout=2, k_row=3)) == EINVAL and err(lib) == "ELL row form missing"


def test_dense_layout_refused(lib):
    m = model(layout=3, k_row=25, k_col=25, col=True)
    assert call(lib, m) == EINVAL and err(lib) == f"{FN}: " + DENSE_MSG
    plan = (ctypes.c_int64 * 10)()
    assert lib.irlmx_workspace_bytes(ctypes.byref(m), OP) == 0
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP, plan) == EINVAL
    assert err(lib) == "execution_plan: " + DENSE_MSG


def test_workspace(lib):
    """Fused models need none; a per-sweep model needs V's two buffers, a
    multiple of 256 whatever T (the size query does not take it)."""
    small = model(B=4, shared=0)
    assert lib.irlmx_workspace_bytes(ctypes.byref(small), OP) == 0
    S, B = 128 * 40, 2
    need = int(lib.irlmx_workspace_bytes(ctypes.byref(BIG), OP))
    assert need == 2 * B * S * 8 and need % 256 == 0, need
    odd = model(S=127 * 41, W=127, H=41, B=3, shared=0)
    n_odd = int(lib.irlmx_workspace_bytes(ctypes.byref(odd), OP))
    assert n_odd % 256 == 0 and n_odd >= 2 * 3 * 127 * 41 * 8, n_odd
    for horizon in (1, 10, 2 ** 20):
        for got, ws in ((0, fake()), (need - 1, fake()), (need, NULL)):
            assert call(lib, BIG, horizon=horizon, n=got, ws=ws) == EWORKSPACE, got
            assert err(lib) == f"workspace too small: need {need} bytes, got {got}", err(lib)


def test_plan(lib):
    plan = (ctypes.c_int64 * 10)()
    m = model()
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP, plan) == 0
    assert list(plan) == [0, 0, 0, 0, 0, 1, 0, 64, 1, 1536 + 16 * 25], list(plan)   # fused: 25 states, one wave
    assert lib.irlmx_execution_plan(ctypes.byref(BIG), OP, plan) == 0
    assert list(plan) == [2, 0, 0, 0, 0, 1, 0, 256, 0, 0], list(plan)               # one launch per step
    wide = model(layout=2, S=300, k_row=40, k_col=3, row_idx=True, col=True)
    assert lib.irlmx_execution_plan(ctypes.byref(wide), OP, plan) == 0 and plan[0] == 2
    k32 = model(layout=2, S=200, k_row=32, k_col=32, row_idx=True, col=True)
    assert lib.irlmx_execution_plan(ctypes.byref(k32), OP, plan) == 0 and (plan[0], plan[5], plan[7]) == (0, 1, 256)
    # the backward-only flags keep their messages
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP | 0x200, plan) == EINVAL
    assert "IRLMX_PLAN_EXTENDED_RANGE applies to IRLMX_OP_BACKWARD only" in err(lib)
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP | 0x100, plan) == EINVAL
    assert "NO_RESCALE applies to IRLMX_OP_BACKWARD only" in err(lib)
    for op in (5, 7, 10, 99):
        assert lib.irlmx_execution_plan(ctypes.byref(m), op, plan) == EINVAL and err(lib) == f"unknown op {op}"
