"""The inputs of tests/test_gpu_ell_matrix.py (tests/ell_cases.py), without a GPU.

Per case: the generator is deterministic; k_row and k_col fall exactly in the
slot classes the case is named for, so the planner restated in ell_cases.plan
sends every pass to the instantiation the hand-written table lists (ell_cases.FUSED,
ell_cases.GRID); the named states have their properties; the CSR oracle's policy
is finite and exactly 0 at the empty action; the extended reference's guards
pass for every pass the GPU test runs (so a bad input fails here, before a GPU
run); and both slot layouts expand back to the matrices they were built from.
"""

import numpy as np
import pytest

import ell_cases as L
import extended_ref as X


@pytest.mark.parametrize("name", L.NAMES)
def test_generator(name):
    """Determinism, exact slot classes, the named states."""
    S, A, B, lo, hi, n_offsets, hub = L.SPECS[name]
    c = L.case(name)
    assert (c.S, c.A, c.B) == (S, A, B) and c.terminal == [S - 1, 2]
    assert (L.slot_class(c.k_row), L.slot_class(c.k_col)) == c.classes, (c.k_row, c.k_col)
    assert c.k_row == hi + (hub is not None) and c.k_col == (S if hub is not None else n_offsets)
    assert c.reward.min() >= L.REWARD_RANGE[0] and c.reward.max() <= L.REWARD_RANGE[1]
    seeds = set()
    for b in range(B):
        again = L.table(S, A, lo, hi, n_offsets, L._seed(name, b), hub)
        assert again.named == c.named[b]
        for m, m2 in zip(c.mats[b], again.mats):
            assert (m != m2).nnz == 0 and np.array_equal(m.data, m2.data)
        seeds.add(tuple(c.mats[b][0].indices[:50]))
        assert L.slot_counts(c.mats[b]) == (c.k_row, c.k_col)
        assert L.reaches_terminal(c.mats[b], c.terminal)
        u = L.union(c.mats[b])
        n_to, n_from = np.diff(u.indptr), np.diff(u.T.tocsr().indptr)
        assert n_to.min() >= 1 and u.diagonal().sum() == (u[hub, hub] if hub is not None else 0)
        named = c.named[b]
        assert not {named["single"], named["nosource"]} & set(c.terminal)
        assert n_to[named["full"]] == c.k_row and n_to[named["single"]] == 1
        assert n_from[named["nosource"]] == 0
        if hub is None:
            assert n_from[named["target"]] == c.k_col and n_to.min() < n_to.max() - 2   # unequal rows
        else:
            assert n_from[hub] == S
        for a, m in enumerate(c.mats[b]):
            sums = np.asarray(m.sum(axis=1)).reshape(-1)
            zero = sums == 0
            assert np.allclose(sums[~zero], 1.0, rtol=0, atol=1e-15) and (m.data > 0).all()
            if named["empty"] is None:
                assert A == 1 and not zero.any()
            else:
                s_e, a_e = named["empty"]
                assert s_e not in c.terminal
                assert np.flatnonzero(zero).tolist() == ([s_e] if a == a_e else [])
    assert len(seeds) == B    # the tables of one case differ


def test_plan_table_is_the_planner_restated():
    """ell_cases.FUSED / GRID (written out by hand) against ell_cases.plan (the
    planner restated from csrc): the same instantiation for every case and pass."""
    for name in L.NAMES:
        c = L.case(name)
        got = tuple(L.fused_pair(L.expected_plan(c, op), c.k_col if op == "forward" else c.k_row) for op in L.OPS)
        assert got == L.FUSED[name], (name, got)
        for op in L.OPS:
            p = L.expected_plan(c, op)
            assert p["shape"] in ("fused", "sweep")      # S <= 4096: never the grid shape
            if p["shape"] == "fused":
                per = -(-c.S // p["spt"])
                assert p["spt"] == (1 if c.S <= 1024 else 2 if c.S <= 2048 else 4) and per <= p["threads"] < per + 64
    for name, blocks in L.GRID.items():
        c = L.case(name)
        for op, n in zip(L.OPS, blocks):
            p = L.expected_plan(c, op, fused_max=0)
            assert p == ({"shape": "sweep"} if n is None else {"shape": "grid", "spt": 1, "threads": 256, "C": n}), (name, op)
    assert L.case("k8-s1029").S - 4 * 256 == 5


@pytest.mark.parametrize("name", L.NAMES)
def test_references_within_guards(name):
    """Every pass of the GPU test on the CPU: the oracle's policy is finite and
    exactly 0 at the empty action (and nowhere else), the no-source state's SVF
    is its p0 entry, and extended_ref's guards pass (the unscaled longdouble
    backward stays normal, converged soft VI leaves no start value).  Prints
    e_oracle per pass (the instance with the largest)."""
    c = L.case(name)
    e = {}
    worst = lambda key, val: e.__setitem__(key, max(e.get(key, 0.0), val))
    for b in range(c.B):
        named = c.named[b]
        o, ref = c.backward(b)                                  # raises if zs leaves longdouble's normal range
        assert np.isfinite(o).all() and np.isfinite(ref.astype(np.float64)).all()
        want_zero = np.zeros(o.shape, bool)
        if named["empty"] is not None:
            want_zero[named["empty"]] = True
        assert np.array_equal(o == 0, want_zero) and np.array_equal(ref == 0, want_zero)
        worst("backward", X.elementwise_err(o, ref))
        for cap in L.CAPS:
            d, k, status, dref = c.forward(b, cap)
            assert np.isfinite(d).all() and 1 <= k <= cap
            assert d[named["nosource"]] == c.p0[b, named["nosource"]] == dref[named["nosource"]]
            worst(f"forward{cap}", X.elementwise_err(d, dref))
        pi, v, k, xpi, xv = c.soft(b, L.DISCOUNT)               # raises if a start value survives
        assert np.isfinite(pi).all() and np.isfinite(v).all()
        assert (pi > 0).all()                                   # (an empty row is q = r there, not an exact 0)
        worst("soft_pi", X.elementwise_err(pi, xpi))
        worst("soft_v", X.normwise_err(v, xv))
        for average in (False, True):
            vv, k, xvv = c.vi(b, L.DISCOUNT, average)
            assert np.isfinite(vv).all() and k >= 1
            worst("vi_avg" if average else "vi_max", X.normwise_err(vv, xvv))
    floor = c.floor()
    print(f"\n[ell-cases] {name} e_floor={floor:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in e.items()))
    assert max(e.values()) < 1e-11                              # the oracle itself sits at rounding level


@pytest.mark.parametrize("name", L.NAMES)
def test_slot_layouts_expand_to_the_tables(name):
    """Both slot layouts, expanded on the host, are the generated matrices exactly
    (row form and column form); the sorted one is ascending with the unused slots
    last and on the state itself, the scrambled one differs from state to state,
    has two slots more and points its unused slots at other states."""
    c = L.case(name)
    forms = ("sorted", "scrambled") if name in ("k5-s200", "k8-s1029") else ("sorted",)
    s = np.arange(c.S)
    for b in range(c.B):
        for form in forms:
            ri, rv, ci, cv = L.host_arrays(c, b, form)
            pad = L.SCRAMBLE_PAD if form == "scrambled" else 0
            assert ri.shape == (c.k_row + pad, c.S) and rv.shape == (c.A, c.k_row + pad, c.S)
            assert ci.shape == (c.k_col + pad, c.S) and cv.shape == (c.A, c.k_col + pad, c.S)
            assert ri.dtype == ci.dtype == np.int32 and ri.min() >= 0 and ri.max() < c.S and 0 <= ci.min() <= ci.max() < c.S
            for idx, val, tr in ((ri, rv, False), (ci, cv, True)):
                for m, ref in zip(L.expand(idx, val, transpose=tr), c.mats[b]):
                    assert (m != ref).nnz == 0
                    if c.S <= 1029:
                        assert np.array_equal(m.toarray(), ref.toarray())    # the dense table, exactly
                used = (val != 0).any(axis=0)
                if form == "sorted":
                    assert (idx[~used] == np.broadcast_to(s, idx.shape)[~used]).all()
                    assert (used[:-1] >= used[1:]).all()                     # unused slots last
                    both = used[:-1] & used[1:]
                    assert (idx[:-1][both] < idx[1:][both]).all()            # ascending
                else:
                    assert (idx[~used] != np.broadcast_to(s, idx.shape)[~used]).all()
                    assert (~used).sum(axis=0).min() >= L.SCRAMBLE_PAD
                    first_unused = np.argmin(used, axis=0)
                    assert len(set(first_unused.tolist())) > 2               # padding at different positions
                    both = used[:-1] & used[1:]
                    assert (idx[:-1][both] > idx[1:][both]).any()            # not ascending
        if len(forms) == 2:
            assert not np.array_equal(L.host_arrays(c, 0, "scrambled")[0], L.host_arrays(c, 1, "scrambled")[0])


@pytest.mark.parametrize("name", ["k5-s200", "k5-s1029"])
def test_numpy_order_reward_keeps_the_unscaled_backward_finite(name):
    """ell_cases.numpy_order_reward: the oracle's restatement of the reference's
    unscaled float64 backward (numpy's order) is finite on it, and zero at the
    empty action only, so the GPU test compares every value.  On the case's own
    rewards it overflows at 1,029 states, which is why the shift exists."""
    import maxent_oracle as O
    c = L.case(name)
    r = L.numpy_order_reward(c)
    assert r.shape == c.reward.shape and np.allclose(np.exp(r).mean(axis=1) * c.A, 1.0)
    for b in range(c.B):
        pi = O.backward_maxent_blas_order_csr(c.mats[b], c.terminal, r[b])
        zero = np.zeros(pi.shape, bool)
        zero[c.named[b]["empty"]] = True
        assert np.isfinite(pi).all() and np.array_equal(pi == 0, zero)
        assert np.abs(pi.sum(axis=1) - 1.0).max() < 1e-12
        own = O.backward_maxent_blas_order_csr(c.mats[b], c.terminal, c.reward[b])
        assert np.isfinite(own).all() == (name == "k5-s200")
