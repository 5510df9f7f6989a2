"""Failure paths of irlmx_rollout, irlmx_demo_statistics and
irlmx_demo_log_likelihood through ctypes, in the manner of
tests/test_abi_policy_eval.py: every call fails in the argument check, so the
non-NULL array pointers are never dereferenced and no GPU is needed.
"""

import ctypes

import pytest

EINVAL = -1
MAX_LEN = 1 << 20


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from irlmx import _lib
    assert _lib.ROLLOUT_MAX_LEN == MAX_LEN
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


ROLLOUT_REQUIRED = ("p_action", "terminal", "start", "seed", "visits", "starts", "lengths", "traj_status")


def rollout(lib, m, n_traj=8, max_len=16, **over):
    a = {k: fake() for k in ROLLOUT_REQUIRED + ("states", "actions")}
    a.update(over)
    mp = ctypes.byref(m) if m is not None else None
    return lib.irlmx_rollout(mp, a["p_action"], a["terminal"], a["start"], a["seed"], n_traj, max_len, a["visits"],
                             a["starts"], a["lengths"], a["traj_status"], a["states"], a["actions"], NULL)


STATS_REQUIRED = ("states", "lengths", "visits", "starts", "traj_status")


def statistics(lib, S=25, B=1, N=8, stride=17, **over):
    a = {k: fake() for k in STATS_REQUIRED}
    a.update(over)
    return lib.irlmx_demo_statistics(S, B, N, stride, a["states"], a["lengths"], a["visits"], a["starts"],
                                     a["traj_status"], NULL)


LL_REQUIRED = ("p_action", "states", "actions", "lengths", "ll_traj", "ll", "traj_status")


def likelihood(lib, S=25, A=4, B=1, N=8, stride=17, **over):
    a = {k: fake() for k in LL_REQUIRED}
    a.update(over)
    return lib.irlmx_demo_log_likelihood(S, A, B, N, stride, a["p_action"], a["states"], a["actions"], a["lengths"],
                                         a["ll_traj"], a["ll"], a["traj_status"], NULL)


def test_abi_version_unchanged(lib):
    assert lib.irlmx_abi_version() == 1


def test_rollout_null_arguments(lib):
    assert rollout(lib, None) == EINVAL and err(lib) == "mdp is NULL"
    for name in ROLLOUT_REQUIRED:
        assert rollout(lib, model(), **{name: NULL}) == EINVAL, name
        assert err(lib) == f"rollout: {name} is NULL", (name, err(lib))
    assert rollout(lib, model(layout=2, k_row=3)) == EINVAL and err(lib) == "ELL row form missing"


def test_rollout_sizes(lib):
    for n in (0, -3):
        assert rollout(lib, model(), n_traj=n) == EINVAL
        assert err(lib) == f"rollout: n_traj={n} < 1", err(lib)
    for bad in (0, -1, MAX_LEN + 1):
        assert rollout(lib, model(), max_len=bad) == EINVAL
        assert err(lib) == f"rollout: max_len={bad} outside [1, {MAX_LEN}]", err(lib)


def test_rollout_states_and_actions_go_together(lib):
    for over in ({"states": NULL}, {"actions": NULL}):
        assert rollout(lib, model(), **over) == EINVAL
        assert err(lib) == "rollout: states and actions must both be NULL or both be set", err(lib)


def test_rollout_dense_layout_refused(lib):
    m = model(layout=3, k_row=25, k_col=25, col_val=True)
    assert rollout(lib, m) == EINVAL
    assert err(lib).startswith("rollout:") and "DENSE" in err(lib), err(lib)


def test_statistics_arguments(lib):
    for name in STATS_REQUIRED:
        assert statistics(lib, **{name: NULL}) == EINVAL, name
        assert err(lib) == f"demo_statistics: {name} is NULL", (name, err(lib))
    assert statistics(lib, N=0) == EINVAL and err(lib) == "demo_statistics: n_traj=0 < 1"
    assert statistics(lib, stride=0) == EINVAL and err(lib) == "demo_statistics: stride=0 < 1"
    assert statistics(lib, S=0) == EINVAL and err(lib).startswith("demo_statistics: bad sizes S=0")
    assert statistics(lib, B=0) == EINVAL and err(lib).startswith("demo_statistics: bad sizes")


def test_log_likelihood_arguments(lib):
    for name in LL_REQUIRED:
        assert likelihood(lib, **{name: NULL}) == EINVAL, name
        assert err(lib) == f"demo_log_likelihood: {name} is NULL", (name, err(lib))
    assert likelihood(lib, N=0) == EINVAL and err(lib) == "demo_log_likelihood: n_traj=0 < 1"
    assert likelihood(lib, stride=0) == EINVAL and err(lib) == "demo_log_likelihood: stride=0 < 1"
    assert likelihood(lib, A=0) == EINVAL and err(lib).startswith("demo_log_likelihood: bad sizes S=25 A=0")


def test_trajectory_codes_match_header(lib):
    import os
    import re
    from conftest import ROOT
    from irlmx import _lib
    src = open(os.path.join(ROOT, "include", "irlmx.h")).read()
    codes = dict(re.findall(r"#define IRLMX_TRAJ_(\w+) (\d+)", src))
    assert codes == {"OK": "0", "TRUNCATED": "1", "BAD_POLICY": "2", "BAD_TABLE": "3", "BAD_INDEX": "4"}
    assert (_lib.TRAJ_OK, _lib.TRAJ_TRUNCATED, _lib.TRAJ_BAD_POLICY, _lib.TRAJ_BAD_TABLE, _lib.TRAJ_BAD_INDEX) == \
        (0, 1, 2, 3, 4)
    assert len(_lib.TRAJ_NAMES) == 5
