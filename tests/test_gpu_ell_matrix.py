"""Generic sparse (ELL) models with per-instance tables across the planner's
matrix of kernel instantiations and both slot layouts (needs an MI355X).

The ELL kernels are compiled per (states per thread, slot class) pair and per
execution shape; the other suites enter that matrix at a handful of points,
always with one shared table in irlmx_dense_to_ell's slot layout.  The cases of
tests/ell_cases.py reach every fused pair fused_pair_ok admits for each pass, the
planner's fallbacks (a pair that is not instantiated, k_row or k_col above 32,
A above the grid shape's 5), A = 1 and A = 8, and the persistent grid shape
with 8, 16 and 32 slots -- each with B = 2 or 3 different tables in one launch
(``shared = 0``: the b' index of row_idx / col_idx / col_val), and two of them
in a hand-built slot layout that only keeps the header's promise ("unused
slots have value 0").

Per case and pass (backward; forward at caps 7 and 500; soft VI and both VIs
at discount 0.8):

1. the plan is asserted first (ell_cases.FUSED / GRID through ell_cases.plan);
2. sweep counts and status equal the CSR oracle's;
3. every entry of every instance is within 16 * max(e_oracle, e_floor) of the
   longdouble reference -- the run_* / judge helpers of tests/elementwise_run.py,
   shared with test_gpu_elementwise;
4. the policy entry of the empty action is exactly 0;
5. the SVF of the state nobody reaches is its p0 entry, bit for bit;
6. instance b of the batch equals the same table run alone as a shared B = 1
   model, bit for bit;
7. the per-sweep shape gives the same bits as the fused or grid shape;
8. ops.backward_maxent_extended equals ops.backward_maxent bit for bit, on its
   own asserted plan.

One line per case and pass is printed, ``[ell-matrix] case op plan e_oracle
e_kernel ratio allowed`` (profiles/ell_matrix.txt keeps a run's lines).
"""

import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import ell_cases as L
import maxent_oracle as O
import elementwise_run as E
import extended_ref as X
from conftest import ORACLE_DIR, PKG_DIR, ROOT
from elementwise_run import dev, env  # noqa: F401  (fixtures: build + device; the planner keys)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TAG = "ell-matrix"
DEFAULT, GRID = {}, {"IRLMX_FUSED_MAX_STATES": 0}


# ---------------------------------------------------------------------------
# the bounds-check build first: a wrong slot index shows there as a flag, not as a fault
# ---------------------------------------------------------------------------

#: (case, slot layout, planner keys) run on both builds
CHECKED = [("k5-s200", "sorted", DEFAULT), ("k5-s200", "scrambled", DEFAULT),
           ("k8-s1029", "sorted", GRID), ("k8-s1029", "scrambled", GRID)]

WORKER = textwrap.dedent("""
    import os, sys
    sys.path[:0] = [{root!r}, {pkg!r}, {oracle!r}, {tests!r}]
    import torch
    import ell_cases as L
    from irlmx import _lib, ops
    assert int(_lib.load().irlmx_device_checks_enabled()) == 1
    dev = torch.device("cuda", 0)
    out = {{}}
    for name, form, keys in {checked!r}:
        os.environ.pop("IRLMX_FUSED_MAX_STATES", None)
        os.environ.update({{k: str(v) for k, v in keys.items()}})
        c = L.case(name)
        mdp = L.device_model(c, dev, form)
        shapes = [ops.execution_plan(mdp, op)["shape"] for op in L.OPS]
        res = L.run_passes(c, mdp)
        out[name, form] = (shapes, res, ops.device_check_failures())
    torch.save(out, {out!r})
""")


def test_bounds_check_build(dev, env, tmp_path):
    """One subprocess on libirlmx_checks.so (every ELL index, granule offset and
    tile range checked in the kernels): k5-s200 and, on the grid shape, k8-s1029,
    each in both slot layouts with per-instance tables -- no check fails, and
    every result equals the product build's bit for bit."""
    import __graft_entry__ as g
    res = str(tmp_path / "checks.pt")
    code = WORKER.format(root=ROOT, pkg=PKG_DIR, oracle=ORACLE_DIR, tests=os.path.join(ROOT, "tests"), out=res,
                         checked=CHECKED)
    keep = {k: v for k, v in os.environ.items() if k not in E.KEYS}
    subprocess.run([sys.executable, "-c", code], env=dict(keep, IRLMX_LIB=g.LIB_CHECKS), cwd=ROOT, check=True,
                   timeout=600)
    out = torch.load(res, weights_only=False)
    assert set(out) == {(n, f) for n, f, _ in CHECKED}
    from irlmx import ops
    for name, form, keys in CHECKED:
        shapes, checked, fails = out[name, form]
        assert fails == 0, (name, form, fails)
        env(keys)
        c = L.case(name)
        mdp = L.device_model(c, dev, form)
        assert shapes == [ops.execution_plan(mdp, op)["shape"] for op in L.OPS]
        assert shapes == (["grid"] * 4 if keys else ["fused"] * 4), (name, form, shapes)
        L.assert_same(L.run_passes(c, mdp), checked, f"{name}/{form}: product build against the check build")
    assert ops.device_check_failures() == 0     # (always 0 on the product build)


# ---------------------------------------------------------------------------
# one case on one model: plans, the judged passes, the named states
# ---------------------------------------------------------------------------

def assert_plans(c, mdp, fused_max, pad=0):
    """The device's plan of every pass against ell_cases.plan; the plan strings of the printed lines."""
    from irlmx import ops
    out = {}
    for op in L.OPS:
        out[op] = E.expect_plan(mdp, op, **L.expected_plan(c, op, fused_max, pad))
    want = L.expected_plan(c, "extended", fused_max, pad)
    got = ops.execution_plan(mdp, "backward", extended_range=True)
    assert {k: got[k] for k in want} == want, ("extended", got)
    return out


def _t(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype)


def judged(c, mdp, label, plans):
    """Every pass through elementwise_run's run_* helpers (sweep counts and
    status against the CSR oracle, every entry against the longdouble reference
    at the existing factor of 16), the extended backward beside them; what the
    device returned, in the form of ell_cases.run_passes."""
    out = {"backward": (_t(E.run_backward(c, mdp, label, plans["backward"], tag=TAG)),)}
    out["extended"] = L.run_passes(c, mdp, passes=("extended",))["extended"]
    for cap in L.CAPS:
        svf, k, st = E.run_forward(c, mdp, label, plans["forward"], cap, tag=TAG)
        out[f"forward{cap}"] = (_t(svf), _t(k, torch.int64), _t(st, torch.int32))
    pi, v, k, st = E.run_soft(c, mdp, label, plans["soft_backward"], L.DISCOUNT, tag=TAG)
    out["soft"] = (_t(pi), _t(v), _t(k, torch.int64), _t(st, torch.int32))
    for average, (v, k, st) in E.run_vi(c, mdp, label, plans["value_iteration"], L.DISCOUNT, tag=TAG).items():
        out["vi_avg" if average else "vi_max"] = (_t(v), _t(k, torch.int64), _t(st, torch.int32))
    assert set(out) == set(L.PASSES)
    return out


def assert_named_states(c, res, tables=None):
    """The empty action's policy entry is exactly 0 (ordinary and extended
    backward); the SVF of the state without sources is its p0 entry, bit for bit,
    at both caps."""
    for i, b in enumerate(range(c.B) if tables is None else tables):
        named = c.named[b]
        if named["empty"] is not None:
            s, a = named["empty"]
            for p in ("backward", "extended"):
                assert res[p][0][i, s, a].item() == 0.0, (c.name, p, b)
                assert int((res[p][0][i] == 0).sum()) == 1, (c.name, p, b)
        u = named["nosource"]
        for cap in L.CAPS:
            assert L.same_bits(res[f"forward{cap}"][0][i, u], _t(c.p0[b, u])), (c.name, cap, b)


def check_model(c, dev, env, keys, form, label):
    """Checks 1-8 of the module docstring for one case, slot layout and set of planner keys."""
    fused_max = 0 if keys else L.FUSED_MAX_STATES
    pad = L.SCRAMBLE_PAD if form == "scrambled" else 0
    mdp = L.device_model(c, dev, form)
    assert (mdp.k_row, mdp.k_col, mdp.shared, mdp.batch) == (c.k_row + pad, c.k_col + pad, False, c.B)
    env(keys)
    res = judged(c, mdp, label, assert_plans(c, mdp, fused_max, pad))
    assert_named_states(c, res)
    assert L.same_bits(res["extended"][0], res["backward"][0]), f"{label}: extended backward differs"
    # every instance alone, as a shared single-table model: the same bits
    for b in range(c.B):
        solo = L.device_model(c, dev, form, tables=[b], shared=True)
        assert_plans(c, solo, fused_max, pad)
        L.assert_same(L.run_passes(c, solo, [b]), res, f"{label}: instance {b} alone against the batch", rows=[b])
    # the per-sweep shape: the same bits
    env(E.SWEEP)
    from irlmx import ops
    for op in L.OPS:
        E.expect_plan(mdp, op, shape="sweep")
    assert ops.execution_plan(mdp, "backward", extended_range=True)["shape"] == "sweep"
    L.assert_same(L.run_passes(c, mdp), res, f"{label}: per-sweep shape against {keys or 'the default plan'}")
    return mdp, res


@pytest.mark.parametrize("name", L.NAMES)
def test_fused_matrix(dev, env, name):
    """Every case on the default plan: the fused instantiation <SPT, KMAX> of
    ell_cases.FUSED for each pass, or the per-sweep shape where the pair is not
    instantiated (or a slot count is above 32)."""
    c = L.case(name)
    want = dict(zip(L.OPS, L.FUSED[name]))
    for op in L.OPS:   # the table itself, before the device is asked
        assert L.fused_pair(L.expected_plan(c, op), c.k_col if op == "forward" else c.k_row) == want[op], (name, op)
    check_model(c, dev, env, DEFAULT, "sorted", name)


@pytest.mark.parametrize("name", list(L.GRID))
def test_grid_shape(dev, env, name):
    """IRLMX_FUSED_MAX_STATES=0: k8-s1029 on the persistent grid shape for all
    four passes (KMAX 8, five workgroups per instance, the last one holding 5
    states), k32-s200 for the forward and backward only (A = 8 is above the
    Bellman grid kernels' 5 actions), k40-s300 on the per-sweep shape."""
    c = L.case(name)
    for op, blocks in zip(L.OPS, L.GRID[name]):
        p = L.expected_plan(c, op, fused_max=0)
        assert (p.get("C"), p["shape"]) == ((blocks, "grid") if blocks else (None, "sweep")), (name, op, p)
    check_model(c, dev, env, GRID, "sorted", f"{name}/grid-env")


@pytest.mark.parametrize("name,keys", [("k5-s200", DEFAULT), ("k8-s1029", GRID)], ids=["k5-s200", "k8-s1029-grid"])
def test_scrambled_slots(dev, env, name, keys):
    """The same matrices in a hand-built table: slots in a random order per
    state, k_row and k_col two above need (so the next slot class: 8 for k5-s200,
    16 for k8-s1029), unused slots at random positions pointing at other states
    with value 0; the column form likewise.  Same sweep counts, status and bound
    as the sorted form (not the same bits: the summation order differs), the same
    bit identities between batch compositions and shapes; the numpy-order
    backward refuses the table."""
    from irlmx import _lib, ops
    c = L.case(name)
    mdp, _ = check_model(c, dev, env, keys, "scrambled", f"{name}/scrambled" + ("/grid-env" if keys else ""))
    assert L.slot_class(mdp.k_row) == {"k5-s200": 8, "k8-s1029": 16}[name]
    tm = ops.terminal_mask(c.terminal, c.S, batch=c.B, device=dev)
    with pytest.raises(_lib.IrlmxError, match="ascending column order"):
        ops.backward_maxent_numpy_order(mdp, np.exp(c.reward), tm)


def test_take_gathers_per_instance_tables(dev, env):
    """DeviceMDP.take([2, 0]) on k5-s200's three tables (what
    BatchedMaxEnt.compact() calls): rows 2 and 0 of the full result, bit for bit."""
    c = L.case("k5-s200")
    mdp = L.device_model(c, dev)
    env(DEFAULT)
    full = L.run_passes(c, mdp)
    sub = mdp.take([2, 0])
    assert (sub.batch, sub.shared) == (2, False) and sub.row_idx.data_ptr() != mdp.row_idx.data_ptr()
    L.assert_same(L.run_passes(c, sub, [2, 0]), full, "take([2, 0]) against the full batch", rows=[2, 0])
    assert_named_states(c, L.run_passes(c, sub, [2, 0]), tables=[2, 0])


# ---------------------------------------------------------------------------
# numpy-order entry points on per-instance tables
# ---------------------------------------------------------------------------

def bits_equal(got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    return got.shape == ref.shape and np.array_equal(got.view(np.int64), ref.view(np.int64))


@pytest.mark.parametrize("name", ["k5-s200", "k5-s1029"])
def test_numpy_order_per_instance_tables(dev, env, name):
    """The numpy-order backward and VI on the sorted per-instance tables: per
    instance bit-identical to the oracle's restatement of numpy's order
    (O.backward_maxent_blas_order_csr, O.value_iteration_blas_order), and to the
    same entry point on that table alone.  The backward does not rescale (the
    reference does not), so it runs on ell_cases.numpy_order_reward -- the case's
    rewards shifted per instance to a growth of ~1 per sweep -- where every
    partition value stays finite over the 2 * S sweeps: the restatement's result
    is asserted finite, and zero at the empty action only, so all S * A values
    are compared.  The VI runs on the case's own rewards."""
    from irlmx import ops
    c = L.case(name)
    env(DEFAULT)
    mdp = L.device_model(c, dev)
    tm = ops.terminal_mask(c.terminal, c.S, batch=c.B, device=dev)
    r_np = L.numpy_order_reward(c)
    pi = ops.backward_maxent_numpy_order(mdp, np.exp(r_np), tm).cpu()
    vi = {avg: ops.value_iteration(mdp, c.reward.copy(), L.DISCOUNT, average=avg, numpy_order=True)
          for avg in (False, True)}
    for b in range(c.B):
        ref = O.backward_maxent_blas_order_csr(c.mats[b], c.terminal, r_np[b])
        zero = np.zeros(ref.shape, bool)
        zero[c.named[b]["empty"]] = True
        assert np.isfinite(ref).all() and np.array_equal(ref == 0, zero), (name, b)
        assert bits_equal(pi[b].numpy(), ref), (name, "backward", b)
        solo = L.device_model(c, dev, tables=[b], shared=True)
        pi_b = ops.backward_maxent_numpy_order(solo, np.exp(r_np[b]), tm[b:b + 1]).cpu()
        assert L.same_bits(pi_b[0], pi[b]), (name, "backward alone", b)
        P = np.stack([m.toarray() for m in c.mats[b]], axis=2)
        for avg, (v, k, st) in vi.items():
            v_ref, k_ref = O.value_iteration_blas_order(P, c.reward[b], L.DISCOUNT, average=avg)
            assert (int(k[b]), int(st[b])) == (k_ref, 0), (name, "vi", avg, b)
            assert np.isfinite(v_ref).all() and bits_equal(v[b].cpu().numpy(), v_ref), (name, "vi", avg, b)
            v_b, k_b, st_b = ops.value_iteration(solo, c.reward[b].copy(), L.DISCOUNT, average=avg, numpy_order=True)
            assert L.same_bits(v_b[0].cpu(), v[b].cpu()) and int(k_b[0]) == k_ref, (name, "vi alone", avg, b)


def test_numpy_order_forward_refuses_wide_columns(dev, env):
    """hub-s200 (k_col = 200): the numpy-order forward returns its documented
    IRLMX_EINVAL (k_col > 32) instead of reading 32 of 200 column slots."""
    from irlmx import _lib, ops
    c = L.case("hub-s200")
    env(DEFAULT)
    mdp = L.device_model(c, dev)
    assert mdp.k_col == c.S and not ops.numpy_order_supported(mdp, "forward") and ops.numpy_order_supported(mdp)
    tm = ops.terminal_mask(c.terminal, c.S, batch=c.B, device=dev)
    pi = np.stack([c.backward(b)[0] for b in range(c.B)])
    with pytest.raises(_lib.IrlmxError, match=rf"\({_lib.EINVAL}\).*k_col > 32"):
        ops.forward_svf(mdp, c.p0.copy(), tm, pi, max_iter=7, numpy_order=True)


# ---------------------------------------------------------------------------
# the grid shape at two states per thread
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("spt", [2, 4])
def test_grid_shape_more_states_per_thread(dev, env, spt):
    """grid_plan raises the states per thread only when bpi * B workgroups would
    not be co-resident, and only where the larger kernel's launch capacity then
    suffices.  Queried on an MI355X for every B up to 4,096 (ops.execution_plan
    under IRLMX_FUSED_MAX_STATES=0, one shared table): the tables of k5-s200 (one
    workgroup per instance at every SPT), k8-s1029 and k16-s1029 go from SPT 1
    straight to the per-sweep shape for every pass, and so does the VI of every
    case; the forward of k5-s2049 reaches SPT 2 (B = 143-153) and SPT 4
    (B = 154-170).  So: table 0 of k5-s2049, shared, at the smallest B whose
    forward plan has this SPT (looked up here, a host call), the forward at a cap
    of 50 on linear_grid_kernel<forward, SPT, 5> -- bit for bit the per-sweep
    shape for all instances, and for the first, middle and last instance the CSR
    oracle's sweep count and the elementwise bound against the longdouble
    reference."""
    from irlmx import ops
    c = L.case("k5-s2049")
    mats, pi0 = c.mats[0], c.backward(0)[0]
    base = L.device_model(c, dev, tables=[0], shared=True)
    env(GRID)
    B = next((B for B in range(1, 4097) if ops.execution_plan(base.with_batch(B), "forward")["spt"] == spt), None)
    assert B is not None and B > 1, spt
    mdp = base.with_batch(B)
    plan = E.expect_plan(mdp, "forward", shape="grid", spt=spt, threads=256, C=-(-c.S // (256 * spt)))
    assert ops.execution_plan(base.with_batch(B - 1), "forward")["spt"] == spt // 2
    rng = np.random.default_rng(4242 + spt)
    p0 = L.C._p0(rng, B, c.S)
    tm = ops.terminal_mask(c.terminal, c.S, batch=B, device=dev)
    run = lambda: tuple(x.cpu() for x in ops.forward_svf(mdp, p0, tm, np.tile(pi0, (B, 1, 1)), max_iter=50))
    got = run()
    env(E.SWEEP)
    E.expect_plan(mdp, "forward", shape="sweep")
    for i, (x, y) in enumerate(zip(got, run())):
        assert L.same_bits(x, y), f"forward B={B}: output {i} differs from the per-sweep shape"
    rows = []
    for b in (0, B // 2, B - 1):
        o, k_ref = O.forward_svf_csr(mats, p0[b], c.terminal, pi0, max_iter=50)
        ref = X.forward(mats, p0[b], c.terminal, pi0, k_ref)
        assert int(got[1][b]) == k_ref, (b, int(got[1][b]), k_ref)
        e_o = X.elementwise_err(o, ref)
        rows.append((f"svf[{b}]", e_o, X.elementwise_err(got[0][b].numpy(), ref), X.bound(e_o, c.k_row, c.A)))
    E.judge(c, f"k5-s2049/shared-x{B}/grid-env", "forward(cap=50)", plan, rows, TAG)
