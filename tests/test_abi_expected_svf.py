"""include/irlmx_expected_svf.h without a device: the header's coverage (its three
functions, exported and bound from a table of their own; the function lists of
irlmx.h and irlmx_timed.h as they were), every failure path of
irlmx_expected_svf_horizon through ctypes -- each call fails in the argument
check, so the non-NULL pointers are never dereferenced -- and the host
arithmetic of the size and plan queries: the memory bound the header states,
the resolved segment length and the routing rule.
"""

import ctypes
import math
import os
import re

import pytest

from conftest import ROOT
from test_abi_timed import DENSE, DENSE_MSG, NULL, err, fake, model

EINVAL, EWORKSPACE = -1, -3
MAXENT, CAUSAL = 0, 1
FUSED, SWEEP = 0, 2
HEADER = os.path.join(ROOT, "include", "irlmx_expected_svf.h")
NAMES = {"irlmx_expected_svf_horizon", "irlmx_expected_svf_horizon_workspace_bytes", "irlmx_expected_svf_horizon_plan"}
PRE = "expected_svf_horizon: "
NP_TABLES = 64 * 8 + 256 * 4          # sizeof(NpTables), csrc/common.h
LDS_MAX = 160 * 1024


def declared(path=HEADER):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return {name for name, _ in re.findall(r"\b(irlmx_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from irlmx import _lib
    return _lib.load()


@pytest.fixture
def fused_default(monkeypatch):
    for k in ("IRLMX_FUSED_MAX_STATES", "IRLMX_HORIZON_FUSED_BATCH", "IRLMX_PLAN_CUS"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# ---------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------

def test_header_symbols_exported_and_bound(lib):
    import irlmx
    from irlmx import _lib, ops
    assert declared() == NAMES
    assert set(_lib.EXPECTED_SVF_SIGNATURES) == NAMES
    for n in NAMES:
        assert hasattr(lib, n), n
        fn = getattr(lib, n)
        res, args = _lib.EXPECTED_SVF_SIGNATURES[n]
        assert fn.argtypes == args and fn.restype is res, n
        assert n not in _lib.SIGNATURES and n not in _lib.TIMED_SIGNATURES, n
    assert lib.irlmx_abi_version() == 1
    assert (_lib.HORIZON_MODEL_MAXENT, _lib.HORIZON_MODEL_CAUSAL) == (MAXENT, CAUSAL)
    for name in ("expected_svf_horizon", "expected_svf_horizon_plan"):
        assert callable(getattr(ops, name)) and name in ops.__all__ and getattr(irlmx, name) is getattr(ops, name)


def test_header_includes_the_main_header_and_the_others_declare_nothing_of_it():
    text = open(HEADER).read()
    assert '#include "irlmx.h"' in text
    assert "#define IRLMX_HORIZON_MODEL_MAXENT 0" in text and "#define IRLMX_HORIZON_MODEL_CAUSAL 1" in text
    assert "asynchronous" in text
    for other in ("irlmx.h", "irlmx_timed.h"):
        path = os.path.join(ROOT, "include", other)
        assert not (declared(path) & NAMES), other
        code = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
        for n in NAMES:
            assert n not in code, (other, n)
    assert "irlmx_expected_svf_horizon" in open(os.path.join(ROOT, "include", "irlmx.h")).read()   # the stream-order table


# ---------------------------------------------------------------------------
# argument validation
# ---------------------------------------------------------------------------

def nbytes(lib, m, mdl, horizon, segment):
    return int(lib.irlmx_expected_svf_horizon_workspace_bytes(ctypes.byref(m), mdl, horizon, segment))


def call(lib, m, mdl=MAXENT, discount=1.0, horizon=10, segment=0, **over):
    a = {k: fake() for k in ("reward", "terminal", "p_initial", "svf", "objective0", "status", "ws")}
    a["n"] = nbytes(lib, m, mdl, horizon, segment) if m is not None else 0
    a.update(over)
    mp = ctypes.byref(m) if m is not None else None
    return lib.irlmx_expected_svf_horizon(mp, mdl, a["reward"], a["terminal"], a["p_initial"], discount, horizon, segment,
                                          a["svf"], a["objective0"], a["status"], a["ws"], a["n"], NULL)


def test_null_arguments(lib):
    assert call(lib, None) == EINVAL and err(lib) == "mdp is NULL"
    for name in ("reward", "p_initial", "svf", "status"):
        assert call(lib, model(), **{name: NULL}) == EINVAL, name
        assert err(lib) == f"{PRE}{name} is NULL", (name, err(lib))
    # terminal and objective0 may be NULL: the call gets as far as the workspace check
    assert call(lib, model(), terminal=NULL, objective0=NULL, n=0) == EWORKSPACE


@pytest.mark.parametrize("mdl", [-1, 2, 7])
def test_model_outside(lib, mdl):
    m = model()
    assert call(lib, m, mdl=mdl, n=1 << 20) == EINVAL
    assert err(lib) == f"{PRE}model {mdl} is neither IRLMX_HORIZON_MODEL_MAXENT nor IRLMX_HORIZON_MODEL_CAUSAL"
    plan = (ctypes.c_int64 * 6)()
    assert nbytes(lib, m, mdl, 10, 0) == 0
    assert lib.irlmx_expected_svf_horizon_plan(ctypes.byref(m), mdl, 10, 0, plan) == EINVAL


@pytest.mark.parametrize("horizon", [0, -1, 2 ** 20 + 1])
def test_horizon_out_of_range(lib, horizon):
    m = model()
    for mdl in (MAXENT, CAUSAL):
        assert call(lib, m, mdl=mdl, horizon=horizon, n=1 << 20) == EINVAL
        assert err(lib) == f"{PRE}horizon {horizon} outside [1, 1048576]", err(lib)
        assert nbytes(lib, m, mdl, horizon, 0) == 0
    assert call(lib, m, horizon=2 ** 20, n=0) == EWORKSPACE             # the largest horizon passes the check


def test_segment_negative(lib):
    m = model()
    assert call(lib, m, segment=-1, n=1 << 20) == EINVAL and err(lib) == f"{PRE}segment -1 is negative"
    assert nbytes(lib, m, MAXENT, 10, -1) == 0
    plan = (ctypes.c_int64 * 6)()
    assert lib.irlmx_expected_svf_horizon_plan(ctypes.byref(m), MAXENT, 10, -1, plan) == EINVAL


@pytest.mark.parametrize("mdl,discount,text", [(CAUSAL, float("nan"), "nan outside [0, 1]"), (CAUSAL, 1.5, "1.5 outside [0, 1]"),
                                              (CAUSAL, -0.1, "-0.1 outside [0, 1]"), (MAXENT, 0.9, "0.9 outside {1} (MAXENT)"),
                                              (MAXENT, float("nan"), "nan outside {1} (MAXENT)")])
def test_discount_out_of_range(lib, mdl, discount, text):
    assert call(lib, model(), mdl=mdl, discount=discount) == EINVAL
    assert err(lib).replace("-nan", "nan") == f"{PRE}discount {text}", err(lib)


def test_discount_in_range(lib):
    for mdl, ok in ((CAUSAL, 0.0), (CAUSAL, 0.9), (CAUSAL, 1.0), (MAXENT, 1.0)):
        assert call(lib, model(), mdl=mdl, discount=ok, n=0) == EWORKSPACE, (mdl, ok)


def test_dense_layout_refused(lib):
    m = model(**DENSE)
    assert call(lib, m) == EINVAL and err(lib) == PRE + DENSE_MSG
    plan = (ctypes.c_int64 * 6)()
    assert nbytes(lib, m, MAXENT, 10, 0) == 0
    assert lib.irlmx_expected_svf_horizon_plan(ctypes.byref(m), MAXENT, 10, 0, plan) == EINVAL and err(lib) == PRE + DENSE_MSG


def test_bad_model(lib):
    assert call(lib, model(S=0)) == EINVAL and "bad sizes S=0" in err(lib)
    assert call(lib, model(layout=2, k_row=3)) == EINVAL and err(lib) == "ELL row form missing"
    assert call(lib, model(layout=2, k_row=3, row_idx=True)) == EINVAL and err(lib) == "ELL column form missing"


def test_workspace_too_small_or_null(lib):
    m = model()
    for mdl in (MAXENT, CAUSAL):
        need = nbytes(lib, m, mdl, 10, 0)
        assert need > 0 and need % 256 == 0
        for got, ws in ((0, fake()), (need - 1, fake()), (need, NULL)):
            assert call(lib, m, mdl=mdl, n=got, ws=ws) == EWORKSPACE, got
            assert err(lib) == f"{PRE}workspace too small: need {need} bytes, got {got}", err(lib)


# ---------------------------------------------------------------------------
# size and plan: host arithmetic only
# ---------------------------------------------------------------------------

def models():
    """The models of tests/test_abi_timed.py: 25, 1029 and 4096 states; ELL k = 8, 32 and 40."""
    return {"5x5": model(), "128x40": model(S=128 * 40, W=128, H=40, B=2, shared=0),
            "64x64": model(S=64 * 64, W=64, H=64), "64x20": model(S=64 * 20, W=64, H=20),
            "k40": model(layout=2, S=300, k_row=40, k_col=3, row_idx=True, col=True),
            "k40-col40": model(layout=2, S=300, k_row=40, k_col=40, row_idx=True, col=True, A=3, B=2, shared=0),
            "k32": model(layout=2, S=200, k_row=32, k_col=32, row_idx=True, col=True, A=8),
            "k8": model(layout=2, S=1029, k_row=8, k_col=8, row_idx=True, col=True, B=3, shared=0),
            "16x16x3": model(S=256, W=16, H=16, B=3, shared=0)}


def expect_fused(m, mdl):
    """The rule of the header: the forward's fused shape at one state per thread
    (at most 1,024 states, at most 32 column slots, at most 8 actions) and the LDS fit."""
    kc = 5 if m.layout == 1 else m.k_col
    lds = (NP_TABLES if mdl == CAUSAL else 0) + 8 * m.n_states * (m.n_actions + 2)
    return m.n_states <= 1024 and kc <= 32 and m.n_actions <= 8 and lds <= LDS_MAX, lds


HORIZONS = (1, 2, 40, 4096, 2 ** 20)


@pytest.mark.parametrize("name", sorted(models()))
def test_size_and_plan(lib, fused_default, name):
    m = models()[name]
    B, S, A = m.batch, m.n_states, m.n_actions
    plan = (ctypes.c_int64 * 6)()
    for mdl in (MAXENT, CAUSAL):
        fused, lds = expect_fused(m, mdl)
        for T in HORIZONS:
            auto = math.isqrt(T - 1) + 1                  # ceil(sqrt(T))
            assert (auto - 1) ** 2 < T <= auto ** 2
            for seg, C in ((0, auto), (1, 1), (3, min(3, T)), (T, T), (T + 5, T)):
                assert lib.irlmx_expected_svf_horizon_plan(ctypes.byref(m), mdl, T, seg, plan) == 0, err(lib)
                n = nbytes(lib, m, mdl, T, seg)
                nseg = -(-T // C)
                assert plan[1] == C, (name, T, seg, list(plan))
                assert plan[2] == nseg + C - 1 + (2 if nseg > 1 else 0), (name, T, seg, list(plan))
                assert plan[5] == n and n % 256 == 0 and n > 0
                assert n <= (nseg + C + A + 6) * B * S * 12 + 4096, (name, mdl, T, seg, n)
                per_state = 12 if mdl == MAXENT else 8
                assert n >= plan[2] * B * S * per_state                       # the slices are all there
                assert (plan[0], plan[3], plan[4]) == ((FUSED, 1, lds) if fused else (SWEEP, 0, 0)), (name, list(plan))
    # forced per step, as elsewhere
    fused_default.setenv("IRLMX_FUSED_MAX_STATES", "0")
    assert lib.irlmx_expected_svf_horizon_plan(ctypes.byref(m), MAXENT, 40, 0, plan) == 0
    assert (plan[0], plan[1], plan[3], plan[4]) == (SWEEP, 7, 0, 0), list(plan)


def test_named_figures(lib, fused_default):
    """C = 0 is 7 at T = 40 and 64 at T = 4096; at T = 4096, S = 256, A = 4, B = 3 the
    workspace is below 4 MB where the policy tensor is 100 MB; the routing of the named models."""
    plan = (ctypes.c_int64 * 6)()
    m = models()["16x16x3"]
    for T, C in ((40, 7), (4096, 64), (1, 1), (2, 2), (2 ** 20, 1024)):
        assert lib.irlmx_expected_svf_horizon_plan(ctypes.byref(m), MAXENT, T, 0, plan) == 0 and plan[1] == C, (T, list(plan))
    for mdl in (MAXENT, CAUSAL):
        for fused in (True, False):
            fused_default.setenv("IRLMX_FUSED_MAX_STATES", "4096" if fused else "0")
            n = nbytes(lib, m, mdl, 4096, 0)
            assert n < 4 * 2 ** 20 and 3 * 4096 * 256 * 4 * 8 > 100 * 10 ** 6, n
    fused_default.delenv("IRLMX_FUSED_MAX_STATES")
    shapes = {}
    for name, mm in models().items():
        assert lib.irlmx_expected_svf_horizon_plan(ctypes.byref(mm), CAUSAL, 40, 0, plan) == 0
        shapes[name] = plan[0]
    assert shapes == {"5x5": FUSED, "16x16x3": FUSED, "k32": FUSED, "k40": FUSED,      # k_col = 3: the forward's slots
                      "k40-col40": SWEEP, "k8": SWEEP, "64x20": SWEEP, "64x64": SWEEP, "128x40": SWEEP}, shapes
    # several states per thread stay per step whatever the batch rule says
    fused_default.setenv("IRLMX_HORIZON_FUSED_BATCH", "1")
    assert lib.irlmx_expected_svf_horizon_plan(ctypes.byref(models()["64x20"]), MAXENT, 40, 0, plan) == 0 and plan[0] == SWEEP
    assert lib.irlmx_expected_svf_horizon_plan(ctypes.byref(m), MAXENT, 40, 0, None) == EINVAL and err(lib) == PRE + "plan is NULL"
