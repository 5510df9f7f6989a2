"""include/irlmx_timed.h without a device: the coverage rules tests/test_abi.py and
tests/test_call_contract_host.py hold include/irlmx.h to, restated for the
header of the time-indexed policies -- a new entry point cannot stay out of the
binding, the contract wrappers or the stream-order rows -- and every failure
path of its three calls and of IRLMX_OP_VALUE_HORIZON through ctypes: each call
fails in the argument check, so the non-NULL pointers are never dereferenced.
"""

import ctypes
import os
import re

import pytest

from conftest import ROOT

EINVAL, EWORKSPACE = -1, -3
OP = 12   # IRLMX_OP_VALUE_HORIZON (5, 7 and 10 stay unknown ops)
HEADER = os.path.join(ROOT, "include", "irlmx_timed.h")
DENSE_MSG = "the finite-horizon passes do not run the DENSE layout (STENCIL5 and ELL only)"


def declared(param=None):
    """The functions include/irlmx_timed.h declares (``param``: those with a ``void* <param>``)."""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = set()
    for name, params in re.findall(r"\b(irlmx_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if param is None or re.search(r"\bvoid\s*\*\s*%s\b" % param, params):
            out.add(name)
    return out


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from irlmx import _lib
    assert _lib.OP_VALUE_HORIZON == OP
    return _lib.load()


# ---------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------

def test_header_symbols_exported_and_bound(lib):
    import irlmx
    from irlmx import _lib, ops
    names = declared()
    assert names == {"irlmx_rollout_horizon", "irlmx_demo_log_likelihood_horizon", "irlmx_value_horizon"}
    assert sorted(_lib.TIMED_SIGNATURES) == sorted(names)
    for n in names:
        assert hasattr(lib, n), n
        fn = getattr(lib, n)
        assert fn.argtypes == _lib.TIMED_SIGNATURES[n][1] and fn.restype is _lib.TIMED_SIGNATURES[n][0], n
        assert n not in _lib.SIGNATURES, n                      # irlmx.h's function list stays as it is
    assert lib.irlmx_abi_version() == 1
    for name in ("rollout_horizon", "demo_log_likelihood_horizon", "value_horizon", "expected_value_difference_horizon"):
        assert callable(getattr(ops, name)) and name in ops.__all__ and getattr(irlmx, name) is getattr(ops, name)
    assert ops._OPS["value_horizon"] == OP


def test_header_includes_the_main_header_and_declares_nothing_of_it():
    text = open(HEADER).read()
    assert '#include "irlmx.h"' in text
    main = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "irlmx.h")).read(), flags=re.S)
    assert "#define IRLMX_OP_VALUE_HORIZON 12" in main
    for n in declared():
        assert n not in main, n


def test_every_workspace_entry_point_has_a_contract_wrapper():
    import timed_call as TC
    assert declared("workspace") == set(TC.WRAPPED) == {"irlmx_value_horizon"}
    assert all(callable(f) for f in TC.WRAPPED.values())


def test_every_stream_entry_point_has_a_stream_order_row_with_a_claim():
    import timed_call as TC
    with_stream = declared("stream")
    assert with_stream == declared()                               # all three take a stream
    assert set(TC.ENTRY_POINTS) == with_stream
    assert {e for e, _ in TC.CLAIMS} == with_stream
    for r in TC.ROWS:
        assert TC.CLAIMS[(r.entry, r.shape)] == "async", r.id      # the header: "asynchronous, both shapes"
    assert {(r.entry, r.shape) for r in TC.ROWS} == set(TC.CLAIMS)  # every claim is run
    # the header says so, and irlmx.h's table lists the three calls
    assert "asynchronous" in open(HEADER).read()
    main = open(os.path.join(ROOT, "include", "irlmx.h")).read()
    for n in with_stream:
        assert n in main, n


# ---------------------------------------------------------------------------
# argument validation
# ---------------------------------------------------------------------------

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
DENSE = dict(layout=3, k_row=25, k_col=25, col=True)


def value(lib, m, horizon=10, discount=0.9, **over):
    a = {k: fake() for k in ("reward", "terminal", "p_action_t", "value0", "value_t", "status", "ws")}
    a["n"] = int(lib.irlmx_workspace_bytes(ctypes.byref(m), OP)) if m is not None else 0
    a.update(over)
    mp = ctypes.byref(m) if m is not None else None
    return lib.irlmx_value_horizon(mp, a["reward"], a["terminal"], a["p_action_t"], discount, horizon, a["value0"],
                                   a["value_t"], a["status"], a["ws"], a["n"], NULL)


def rollout(lib, m, n_traj=8, horizon=10, **over):
    a = {k: fake() for k in ("p_action_t", "terminal", "start", "seed", "visits", "starts", "lengths", "traj_status",
                             "states", "actions")}
    a.update(over)
    mp = ctypes.byref(m) if m is not None else None
    return lib.irlmx_rollout_horizon(mp, a["p_action_t"], a["terminal"], a["start"], a["seed"], n_traj, horizon,
                                     a["visits"], a["starts"], a["lengths"], a["traj_status"], a["states"], a["actions"],
                                     NULL)


def loglik(lib, S=25, A=4, B=1, N=8, stride=11, horizon=10, **over):
    a = {k: fake() for k in ("p_action_t", "states", "actions", "lengths", "ll_traj", "ll", "traj_status")}
    a.update(over)
    return lib.irlmx_demo_log_likelihood_horizon(S, A, B, N, stride, horizon, a["p_action_t"], a["states"], a["actions"],
                                                 a["lengths"], a["ll_traj"], a["ll"], a["traj_status"], NULL)


def test_value_null_arguments(lib):
    assert value(lib, None) == EINVAL and err(lib) == "mdp is NULL"
    for name in ("reward", "value0", "status"):
        assert value(lib, model(), **{name: NULL}) == EINVAL, name
        assert err(lib) == f"value_horizon: {name} is NULL", (name, err(lib))
    # terminal, p_action_t (the optimal value) and value_t may be NULL: the call gets as far as the workspace check
    assert value(lib, BIG, terminal=NULL, p_action_t=NULL, value_t=NULL, n=0, ws=NULL) == EWORKSPACE


def test_rollout_null_arguments(lib):
    assert rollout(lib, None) == EINVAL and err(lib) == "mdp is NULL"
    for name in ("p_action_t", "start", "seed", "visits", "starts", "lengths", "traj_status"):
        assert rollout(lib, model(), **{name: NULL}) == EINVAL, name
        assert err(lib) == f"rollout_horizon: {name} is NULL", (name, err(lib))
    for over in ({"states": NULL}, {"actions": NULL}):
        assert rollout(lib, model(), **over) == EINVAL
        assert err(lib) == "rollout_horizon: states and actions must both be NULL or both be set"
    assert rollout(lib, model(), n_traj=0) == EINVAL and err(lib) == "rollout_horizon: n_traj=0 < 1"


def test_log_likelihood_null_arguments_and_sizes(lib):
    for name in ("p_action_t", "states", "actions", "lengths", "ll_traj", "ll", "traj_status"):
        assert loglik(lib, **{name: NULL}) == EINVAL, name
        assert err(lib) == f"demo_log_likelihood_horizon: {name} is NULL", (name, err(lib))
    assert loglik(lib, S=0) == EINVAL and "bad sizes S=0" in err(lib)
    assert loglik(lib, N=0) == EINVAL and err(lib) == "demo_log_likelihood_horizon: n_traj=0 < 1"
    assert loglik(lib, stride=0) == EINVAL and err(lib) == "demo_log_likelihood_horizon: stride=0 < 1"


@pytest.mark.parametrize("horizon", [0, -1, 2 ** 20 + 1])
def test_horizon_out_of_range(lib, horizon):
    for fn, call in (("value_horizon", lambda: value(lib, model(), horizon=horizon)),
                     ("rollout_horizon", lambda: rollout(lib, model(), horizon=horizon)),
                     ("demo_log_likelihood_horizon", lambda: loglik(lib, horizon=horizon))):
        assert call() == EINVAL, fn
        assert err(lib) == f"{fn}: horizon {horizon} outside [1, 1048576]", err(lib)
    assert value(lib, BIG, horizon=2 ** 20, n=0, ws=NULL) == EWORKSPACE       # the largest horizon passes the check


@pytest.mark.parametrize("discount,text", [(-0.1, "-0.1"), (1.5, "1.5"), (float("nan"), "nan"), (float("inf"), "inf")])
def test_discount_out_of_range(lib, discount, text):
    assert value(lib, model(), discount=discount) == EINVAL
    assert err(lib).replace("-nan", "nan") == f"value_horizon: discount {text} outside [0, 1]", err(lib)
    for ok in (0.0, 1.0):
        assert value(lib, BIG, discount=ok, n=0, ws=NULL) == EWORKSPACE


def test_dense_layout_refused(lib):
    m = model(**DENSE)
    assert value(lib, m) == EINVAL and err(lib) == "value_horizon: " + DENSE_MSG
    assert rollout(lib, m) == EINVAL and err(lib) == "rollout_horizon: " + DENSE_MSG
    plan = (ctypes.c_int64 * 10)()
    assert lib.irlmx_workspace_bytes(ctypes.byref(m), OP) == 0
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP, plan) == EINVAL
    assert err(lib) == "execution_plan: " + DENSE_MSG


def test_bad_model(lib):
    assert value(lib, model(S=0)) == EINVAL and "bad sizes S=0" in err(lib)
    assert rollout(lib, model(layout=2, k_row=3)) == EINVAL and err(lib) == "ELL row form missing"


def test_workspace(lib):
    """Fused models need none; a per-sweep model needs v's two buffers, a multiple
    of 256 whatever T (the size query does not take it): the soft horizon pass's answer."""
    small = model(B=4, shared=0)
    assert lib.irlmx_workspace_bytes(ctypes.byref(small), OP) == 0
    S, B = 128 * 40, 2
    need = int(lib.irlmx_workspace_bytes(ctypes.byref(BIG), OP))
    assert need == 2 * B * S * 8 and need % 256 == 0, need
    for m in (small, BIG, model(S=127 * 41, W=127, H=41, B=3, shared=0),
              model(layout=2, S=300, k_row=40, k_col=3, row_idx=True, col=True)):
        n = int(lib.irlmx_workspace_bytes(ctypes.byref(m), OP))
        assert n % 256 == 0 and n == int(lib.irlmx_workspace_bytes(ctypes.byref(m), 11)), n
    for horizon in (1, 10, 2 ** 20):
        for got, ws in ((0, fake()), (need - 1, fake()), (need, NULL)):
            assert value(lib, BIG, horizon=horizon, n=got, ws=ws) == EWORKSPACE, got
            assert err(lib) == f"workspace too small: need {need} bytes, got {got}", err(lib)


def test_plan(lib):
    """As the soft horizon pass's, except that lds_bytes = 16 * S (no NpTables copy)."""
    plan, soft = (ctypes.c_int64 * 10)(), (ctypes.c_int64 * 10)()
    m = model()
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP, plan) == 0
    assert list(plan) == [0, 0, 0, 0, 0, 1, 0, 64, 1, 16 * 25], list(plan)          # fused: 25 states, one wave
    assert lib.irlmx_execution_plan(ctypes.byref(BIG), OP, plan) == 0
    assert list(plan) == [2, 0, 0, 0, 0, 1, 0, 256, 0, 0], list(plan)               # one launch per step
    wide = model(layout=2, S=300, k_row=40, k_col=3, row_idx=True, col=True)
    k32 = model(layout=2, S=200, k_row=32, k_col=32, row_idx=True, col=True)
    k8 = model(layout=2, S=1029, k_row=8, k_col=8, row_idx=True, col=True, B=3, shared=0)
    for mm in (m, BIG, wide, k32, k8, model(S=64 * 20, W=64, H=20), model(S=64 * 64, W=64, H=64)):
        assert lib.irlmx_execution_plan(ctypes.byref(mm), OP, plan) == 0
        assert lib.irlmx_execution_plan(ctypes.byref(mm), 11, soft) == 0
        want = list(soft)
        if want[0] == 0:
            want[9] = 16 * mm.n_states
        assert list(plan) == want, (list(plan), want)
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP | 0x200, plan) == EINVAL
    assert "IRLMX_PLAN_EXTENDED_RANGE applies to IRLMX_OP_BACKWARD only" in err(lib)
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP | 0x100, plan) == EINVAL
    assert "NO_RESCALE applies to IRLMX_OP_BACKWARD only" in err(lib)
    for op in (5, 7, 10, 99):
        assert lib.irlmx_execution_plan(ctypes.byref(m), op, plan) == EINVAL and err(lib) == f"unknown op {op}"
