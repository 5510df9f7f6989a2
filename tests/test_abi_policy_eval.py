"""Failure paths of irlmx_policy_evaluation and of IRLMX_OP_POLICY_EVALUATION in
the model queries, through ctypes, in the manner of tests/test_abi_errors.py:
every call fails in the argument check, so the non-NULL array pointers are
never dereferenced and no GPU is needed.
"""

import ctypes

import pytest

EINVAL, EWORKSPACE = -1, -3
OP = 6   # IRLMX_OP_POLICY_EVALUATION (5 stays the unknown op the earlier tests pin)
PLAN_NO_RESCALE, PLAN_EXTENDED_RANGE = 0x100, 0x200


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from irlmx import _lib
    assert _lib.OP_POLICY_EVALUATION == OP
    return _lib.load()


_keep = []
NULL = ctypes.c_void_p(0)


def fake():
    """A non-NULL address that the argument checks never dereference."""
    b = ctypes.create_string_buffer(64)
    _keep.append(b)
    return ctypes.cast(b, ctypes.c_void_p)


def model(layout=1, S=25, A=4, W=5, H=5, k_row=5, k_col=5, B=1, shared=1, row_idx=False, col_val=False):
    from irlmx import _lib
    m = _lib.MDPStruct()
    m.layout, m.n_states, m.n_actions, m.width, m.height = layout, S, A, W, H
    m.k_row, m.k_col, m.batch, m.shared = k_row, k_col, B, shared
    m.row_val = fake().value
    m.row_idx = fake().value if row_idx else None
    m.col_val = fake().value if col_val else None
    return m


def err(lib):
    return lib.irlmx_last_error().decode()


def call(lib, m, discount=0.9, **over):
    a = {k: fake() for k in ("reward", "p_action", "terminal", "value", "iterations", "status", "ws")}
    a["n"] = int(lib.irlmx_workspace_bytes(ctypes.byref(model()), OP))
    a.update(over)
    mp = ctypes.byref(m) if m is not None else None
    return lib.irlmx_policy_evaluation(mp, a["reward"], a["p_action"], a["terminal"], discount, 1e-3, 0, a["value"],
                                       a["iterations"], a["status"], a["ws"], a["n"], NULL)


def test_null_arguments(lib):
    assert call(lib, None) == EINVAL and err(lib) == "mdp is NULL"
    for name in ("reward", "p_action", "value", "iterations", "status"):
        assert call(lib, model(), **{name: NULL}) == EINVAL, name
        assert err(lib) == f"policy_evaluation: {name} is NULL", (name, err(lib))
    # terminal may be NULL: the call then gets as far as the workspace check
    assert call(lib, model(), terminal=NULL, n=0, ws=NULL) == EWORKSPACE


def test_bad_model(lib):
    assert call(lib, model(S=0)) == EINVAL and "bad sizes S=0" in err(lib)
    assert call(lib, model(layout=2, k_row=3)) == EINVAL and err(lib) == "ELL row form missing"


@pytest.mark.parametrize("layout", ["stencil", "ell"])
def test_workspace_too_small(lib, layout):
    kw = {"stencil": {}, "ell": dict(layout=2, k_row=3, k_col=3, row_idx=True)}[layout]
    m = model(B=4, shared=0, **kw)
    need = int(lib.irlmx_workspace_bytes(ctypes.byref(m), OP))
    K = 5 if layout == "stencil" else 3
    assert need >= 4 * K * 25 * 8 and need % 256 == 0, need        # at least the folded weights
    for got, ws in ((0, fake()), (need - 1, fake()), (need, NULL)):
        assert call(lib, m, n=got, ws=ws) == EWORKSPACE, (layout, got)
        assert err(lib) == f"workspace too small: need {need} bytes, got {got}", err(lib)


@pytest.mark.parametrize("discount", [1.5, -0.1, float("nan"), float("inf")])
def test_discount_outside_unit_interval(lib, discount):
    assert call(lib, model(), discount=discount) == EINVAL
    assert err(lib).startswith("policy_evaluation: discount") and "outside [0, 1]" in err(lib), err(lib)


def test_dense_layout_refused(lib):
    m = model(layout=3, k_row=25, k_col=25, col_val=True)
    assert call(lib, m) == EINVAL
    assert err(lib) == "policy_evaluation: policy evaluation does not run the DENSE layout (STENCIL5 and ELL only)"
    assert lib.irlmx_workspace_bytes(ctypes.byref(m), OP) == 0
    plan = (ctypes.c_int64 * 10)()
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP, plan) == EINVAL
    assert "does not run the DENSE layout" in err(lib)


def test_plan_and_flags(lib):
    plan = (ctypes.c_int64 * 10)()
    m = model()
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP, plan) == 0
    assert list(plan) == [0, 0, 0, 0, 0, 1, 0, 64, 1, 3 * 8 * 25 + 32], list(plan)    # fused: 25 states, one wave
    big = model(S=128 * 40, W=128, H=40)
    assert lib.irlmx_execution_plan(ctypes.byref(big), OP, plan) == 0
    assert list(plan) == [2, 0, 0, 0, 0, 1, 0, 256, 0, 0], list(plan)                 # one launch per sweep
    wide = model(layout=2, S=300, k_row=40, k_col=3, row_idx=True)
    assert lib.irlmx_execution_plan(ctypes.byref(wide), OP, plan) == 0 and plan[0] == 2
    # the backward-only flags keep their messages
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP | PLAN_EXTENDED_RANGE, plan) == EINVAL
    assert "IRLMX_PLAN_EXTENDED_RANGE applies to IRLMX_OP_BACKWARD only" in err(lib)
    assert lib.irlmx_workspace_bytes(ctypes.byref(m), OP | PLAN_EXTENDED_RANGE) == 0
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP | PLAN_NO_RESCALE, plan) == EINVAL
    assert "NO_RESCALE applies to IRLMX_OP_BACKWARD only" in err(lib)
    for op in (5, 7):
        assert lib.irlmx_execution_plan(ctypes.byref(m), op, plan) == EINVAL and err(lib) == f"unknown op {op}"
