"""The extended-range backward pass without a GPU: its CPU twin
(tests/extended_twin.py) on the inputs that leave float64's span under one
common scale, the condition under which the device pass is bit-identical to
the rescaled pass in range, and the C ABI's argument checks.

Measured (x86-64, numpy 2.2): twin against the longdouble reference 4.7e-16 ..
9.2e-16 on the four wide-range inputs; oracle rows with NaN 69 / 1 / 126 / 388.
"""

import ctypes

import numpy as np
import pytest

import elementwise_cases as C
import extended_ref as X
import extended_twin as T
from test_abi_errors import BAD_MODELS, EINVAL, EWORKSPACE, NULL, err, fake, model

OP_BACKWARD, EXTENDED = 1, 0x200


# -- 1. the twin on the wide-range inputs ---------------------------------------

@pytest.mark.parametrize("W,H,lo,noise", T.WIDE_INPUTS, ids=lambda v: str(v))
def test_twin_wide_range(W, H, lo, noise):
    case = T.wide(W, H, lo, noise)
    ref = case.ref                                   # raises outside the reference's guards
    assert np.isfinite(ref).all()
    n_nan = T.nan_rows(case.oracle)
    print(f"{W}x{H} lo={lo} noise={noise}: oracle rows with NaN {n_nan} of {case.S}")
    assert n_nan > 0, "the rescaled float64 oracle no longer fails on this input"
    twin = case.twin
    assert np.isfinite(twin).all()
    e = X.elementwise_err(twin, ref)
    print(f"twin vs longdouble {e:.3e}, bound {X.bound(0, 5, 4):.3e}, min pi {float(ref.min()):.3e}")
    assert e <= X.bound(0, 5, 4)


def test_finite_oracle_rows_can_be_wrong():
    """Beside the underflow front the common-scale pass returns finite rows with
    probability 0 for actions whose true probability is ~0.05: relative error 1."""
    case = T.wide(64, 4, -15.0)
    fin = np.isfinite(case.oracle).all(axis=1)
    rel = np.abs(case.oracle[fin] - case.ref[fin]) / np.abs(case.ref[fin])
    assert float(rel.max()) == 1.0
    assert X.elementwise_err(case.twin[fin], case.ref[fin]) <= X.bound(0, 5, 4)


# -- 2. the twin in range: alignment shifts and exponent spread ------------------

def _in_range_models():
    for W, H in ((16, 16), (37, 23)):
        c = C.stencil(W, H)
        for b in range(c.B):
            yield f"{c.name}[{b}]", c.rv[b], T.stencil_nbr(W, H), c.terminal, c.reward[b]
    c = C.ell(200)
    rv, nbr = T.ell_rows(c.P)
    assert rv.shape[1] == c.k_row
    for b in range(c.B):
        yield f"{c.name}[{b}]", rv, nbr, c.terminal, c.reward[b]


def test_twin_in_range_shifts():
    """Scaling every operand of an fma chain by one power of two commutes with
    rounding while nothing is subnormal: with every alignment shift and the
    whole exponent spread below 900 bits, neither the extended pass's aligned
    operands nor the rescaled pass's commonly scaled ones leave the normal
    range (1022 bits below the largest), so the two are bit-identical."""
    for name, rv, nbr, terminal, reward in _in_range_models():
        st = T.Stats()
        pi = T.backward(rv, nbr, terminal, reward, stats=st)
        print(f"{name}: max shift {st.max_shift} bits, max spread {st.max_spread} bits")
        assert np.isfinite(pi).all(), name
        assert st.max_shift < 900 and st.max_spread < 900, (name, st.max_shift, st.max_spread)


# -- 3. the C ABI ---------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from irlmx import _lib
    return _lib.load()


def _ext(lib, m, a):
    return lib.irlmx_backward_maxent_extended(m, a["reward"], a["terminal"], a["p_action"], a["status"], a["ws"],
                                              a["n"], NULL)


def _args(lib, m, **over):
    a = {k: fake() for k in ("reward", "terminal", "p_action", "status")}
    a["ws"], a["n"] = fake(), int(lib.irlmx_workspace_bytes(ctypes.byref(m), OP_BACKWARD | EXTENDED))
    a.update(over)
    return a


ELL = dict(layout=2, k_row=3, k_col=3, row_idx=True, col_idx=True, col_val=True)
DENSE = dict(layout=3, k_row=25, k_col=25, col_val=True)


def test_symbol_exported_and_bound(lib):
    from irlmx import _lib, ops
    import irlmx
    assert hasattr(lib, "irlmx_backward_maxent_extended")
    assert "irlmx_backward_maxent_extended" in _lib.SIGNATURES
    assert _lib.PLAN_EXTENDED_RANGE == EXTENDED
    assert callable(ops.backward_maxent_extended) and "backward_maxent_extended" in ops.__all__
    assert irlmx.backward_maxent_extended is ops.backward_maxent_extended
    assert lib.irlmx_abi_version() == 1


def test_flag_with_backward_only(lib):
    plan = (ctypes.c_int64 * 10)()
    for kw, K in (({}, 5), (ELL, 3)):
        m = model(B=3, shared=0, **kw)
        assert lib.irlmx_execution_plan(ctypes.byref(m), OP_BACKWARD | EXTENDED, plan) == 0, err(lib)
        # fused: one workgroup of 64 threads per instance, 24 B of LDS per state
        assert list(plan) == [0, 0, 0, 0, 0, 1, 0, 64, 1, 24 * 25]
        need = int(lib.irlmx_workspace_bytes(ctypes.byref(m), OP_BACKWARD | EXTENDED))
        assert need >= 3 * K * 25 * 8 + 3 * 4 and need % 256 == 0
        for op in (2, 3, 4):
            assert lib.irlmx_execution_plan(ctypes.byref(m), op | EXTENDED, plan) == EINVAL
            assert "IRLMX_PLAN_EXTENDED_RANGE applies to IRLMX_OP_BACKWARD only" in err(lib)
            assert lib.irlmx_workspace_bytes(ctypes.byref(m), op | EXTENDED) == 0
        assert lib.irlmx_execution_plan(ctypes.byref(m), OP_BACKWARD | EXTENDED | 0x100, plan) == EINVAL
    # every earlier op value keeps its answer
    m = model()
    for op in (0, 5, -1):
        assert lib.irlmx_execution_plan(ctypes.byref(m), op, plan) == EINVAL and err(lib) == f"unknown op {op}"
    assert lib.irlmx_execution_plan(ctypes.byref(m), 2 | 0x100, plan) == EINVAL
    assert "NO_RESCALE applies to IRLMX_OP_BACKWARD only" in err(lib)


def test_plan_sweep_above_fused_size(lib):
    plan = (ctypes.c_int64 * 10)()
    m = model(S=128 * 33, W=128, H=33)
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP_BACKWARD | EXTENDED, plan) == 0
    assert list(plan) == [2, 0, 0, 0, 0, 1, 0, 256, 2 * 128 * 33 - 1, 0]
    m = model(S=64 * 64, W=64, H=64)      # the ordinary backward leaves width 64 to the cluster shape
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP_BACKWARD | EXTENDED, plan) == 0
    assert list(plan) == [0, 0, 0, 0, 0, 4, 0, 1024, 1, 24 * 4096]
    m = model(layout=2, S=100, k_row=40, k_col=3, row_idx=True, col_idx=True, col_val=True)   # no 40-slot fused kernel
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP_BACKWARD | EXTENDED, plan) == 0 and plan[0] == 2
    m = model(S=(1 << 19) + 1, W=(1 << 19) + 1, H=1)
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP_BACKWARD | EXTENDED, plan) == EINVAL
    assert "at most 524288 states" in err(lib)
    a = _args(lib, model())
    assert _ext(lib, ctypes.byref(m), a) == EINVAL and "at most 524288 states" in err(lib)


def test_null_arrays_and_model(lib):
    m = model()
    assert _ext(lib, None, _args(lib, m)) == EINVAL and err(lib) == "mdp is NULL"
    for name in ("reward", "terminal", "p_action", "status"):
        assert _ext(lib, ctypes.byref(m), _args(lib, m, **{name: NULL})) == EINVAL, name
        assert err(lib) == f"backward_maxent_extended: {name} is NULL"


@pytest.mark.parametrize("case,kw,msg", BAD_MODELS, ids=[c[0] for c in BAD_MODELS])
def test_bad_model(lib, case, kw, msg):
    a = _args(lib, model())
    m = model(**kw)
    assert _ext(lib, ctypes.byref(m), a) == EINVAL
    assert msg in err(lib), (case, err(lib))
    assert lib.irlmx_workspace_bytes(ctypes.byref(m), OP_BACKWARD | EXTENDED) == 0
    plan = (ctypes.c_int64 * 10)()
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP_BACKWARD | EXTENDED, plan) == EINVAL and msg in err(lib)


@pytest.mark.parametrize("kw", [{}, ELL], ids=["stencil", "ell"])
def test_short_workspace(lib, kw):
    m = model(B=4, shared=0, **kw)
    need = int(lib.irlmx_workspace_bytes(ctypes.byref(m), OP_BACKWARD | EXTENDED))
    assert need > 0
    for got, ws in ((0, fake()), (need - 1, fake()), (need, NULL)):
        assert _ext(lib, ctypes.byref(m), _args(lib, m, n=got, ws=ws)) == EWORKSPACE, got
        assert err(lib) == f"workspace too small: need {need} bytes, got {got}"


def test_dense_refused(lib):
    m = model(**DENSE)
    a = _args(lib, model())
    assert _ext(lib, ctypes.byref(m), a) == EINVAL
    assert "DENSE" in err(lib) and err(lib).startswith("backward_maxent_extended:")
    plan = (ctypes.c_int64 * 10)()
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP_BACKWARD | EXTENDED, plan) == EINVAL and "DENSE" in err(lib)
    assert lib.irlmx_workspace_bytes(ctypes.byref(m), OP_BACKWARD | EXTENDED) == 0
