"""The inputs of tests/test_gpu_policy_eval.py, checked without a device.

Per accuracy run (tests/policy_eval_twin.py: case, instance, policy, discount):
the float64 twin after its own stopping sweep is within the contraction's
truncation bound of the direct solve; its last two deltas keep a relative
margin of 1e-9 from eps, so a last-bit difference on the device cannot move the
stopping sweep (a condition on the seeded inputs, asserted here); and the twin's
own error against the longdouble evaluation at that sweep count, e_oracle, is
printed -- it sets the GPU test's bound together with e_floor.
"""

import numpy as np
import pytest

import extended_ref as X
import policy_eval_twin as T


@pytest.fixture(scope="module", autouse=True)
def _extended():
    try:
        X.require_extended()
    except X.PrecisionUnavailable as e:
        pytest.skip(str(e))


RUNS = [(name, run) for name in T.CASES for run in T.runs(name)]


@pytest.mark.parametrize("name,run", RUNS, ids=[f"{n}-{r[0]}-{r[1]}" for n, r in RUNS])
def test_twin_against_direct_solve_and_margin(name, run):
    kind, discount, terminal = run
    c = T.base(name)
    for b in range(c.B):
        v, k, status, deltas, ref, e_oracle = T.reference(name, b, kind, discount, terminal)
        assert status == T.OK and k == len(deltas) and deltas[-1] <= T.EPS < deltas[-2], (name, b, deltas[-2:])
        assert T.margin_ok(deltas), (name, b, kind, discount, deltas[-2:])
        print(f"[policy-eval] {name}[{b}] {kind} g={discount} sweeps {k} e_oracle {e_oracle:.3e} "
              f"bound {X.bound(e_oracle, c.k_row, c.A):.3e}")
        exact = T.direct_solve(c.mats[b], T.reward(name)[b], T.policy(name, kind)[b], discount, terminal)
        err = float(np.max(np.abs(v - exact)))
        # the truncation bound holds in exact arithmetic; the twin's own rounding (e_oracle, normwise) comes on top
        assert err <= T.truncation(T.EPS, discount) + e_oracle * float(np.max(np.abs(exact))), (name, b, err)


def test_inputs_are_what_the_gpu_tests_assume():
    for name in T.CASES:
        c = T.base(name)
        r = T.reward(name)
        assert r.shape == (c.B, c.S) and (r.min(axis=1) < 0).all() and (r.max(axis=1) > 0).all(), name
        for kind in T.KINDS:
            pi = T.policy(name, kind)
            assert pi.shape == (c.B, c.S, c.A) and np.isfinite(pi).all() and (pi >= 0).all(), (name, kind)
        g = T.policy(name, "greedy")
        assert ((g == 0) | (g == 1)).all() and (g.sum(axis=2) == 1).all(), name
    # slot classes of the ELL cases: what FUSED names
    import ell_cases as L
    for name, pair in T.FUSED.items():
        if T.CASES[name][0] == "ell" and pair is not None:
            assert L.slot_class(T.base(name).k_row) == pair[1], name
    assert L.slot_class(T.base("k40-s300").k_row) == 0


def test_twin_semantics():
    """The stop rule, the cap, NaN, terminals and an exact-0 row in the twin itself."""
    c = T.base("16x16")
    r, pi, mats = T.reward("16x16")[0], T.policy("16x16", "dirichlet")[0], c.mats[0]
    v1, k1, st1, _ = T.twin(mats, r, pi, 0.9, max_iter=1)
    assert k1 == 1 and st1 == T.MAXITER and np.array_equal(v1, r)          # v_1 = r + g * 0
    term = tuple(c.terminal)
    v, k, st, _ = T.twin(mats, r, pi, 0.9, terminal=term)
    assert st == T.OK and np.array_equal(v[list(term)], r[list(term)])
    zero = pi.copy()
    zero[7] = 0.0
    vz, _, _, _ = T.twin(mats, r, zero, 0.9)
    assert vz[7] == r[7]
    bad = r.copy()
    bad[3] = np.nan
    _, kn, stn, _ = T.twin(mats, bad, pi, 0.9)
    assert kn == 1 and stn == T.NONFINITE
    assert np.allclose(T.longdouble(mats, r, pi, 0.9, k, term).astype(np.float64), v, rtol=0, atol=1e-13)
