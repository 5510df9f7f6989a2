"""The extended-range backward pass on the device (needs an MI355X).

ops.backward_maxent_extended holds every partition value as m * 2^e with its
own int32 exponent (csrc/extended.hip).  Checked here, each test asserting the
plan it means to run before it compares values:

* on inputs whose partition vector leaves float64's span under one common
  scale (tests/extended_twin.py: the ordinary pass returns NaN rows there), the
  policy is finite and every entry is within 16 x max(e_twin, e_floor) of the
  longdouble reference (oracle/extended_ref.py), e_twin the CPU twin's own error
  on that instance -- the project's rule with the twin in the oracle's place;
* in range it is bit-identical to the ordinary pass (tests/test_extended_range.py
  asserts the condition that makes this a theorem: shifts and spread < 900 bits);
* fused and per-sweep shapes agree bit for bit; ELL models; non-finite rewards
  and unreachable states; the batched driver, the drop-in switch and the device
  bounds-check build.
"""

import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import elementwise_cases as C
import extended_ref as X
import extended_twin as T
from conftest import ORACLE_DIR, PKG_DIR, ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KEYS = ("IRLMX_FUSED_MAX_STATES", "IRLMX_CLUSTER", "IRLMX_GRID")
SWEEP = {"IRLMX_FUSED_MAX_STATES": 0, "IRLMX_CLUSTER": 0, "IRLMX_GRID": 0}
TESTS_DIR = os.path.join(ROOT, "tests")


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    import irlmx
    return irlmx.require_device()


@pytest.fixture
def env(monkeypatch):
    """Set exactly the given planner keys; all of them are cleared afterwards."""
    def set_env(values):
        for k in KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in values.items():
            assert k in KEYS, k
            monkeypatch.setenv(k, str(v))
    set_env({})
    yield set_env
    set_env({})


def launches():
    """The wide-range launches: 64 x 4 with three rewards in one call, then 128 x 4 and 256 x 4."""
    return [[T.wide(64, 4, -15.0), T.wide(64, 4, -12.0, 2.0), T.wide(64, 4, -9.0)],
            [T.wide(128, 4, -7.0)], [T.wide(256, 4, -4.0)]]


def wide_mdp(cases, dev):
    from irlmx import DeviceMDP, _lib
    c = cases[0]
    rv = np.stack([x.rv for x in cases])
    return DeviceMDP(_lib.LAYOUT_STENCIL5, c.S, 4, len(cases), False, torch.as_tensor(rv, device=dev),
                     width=c.W, height=c.H, device=dev)


def wide_inputs(cases, dev):
    from irlmx import ops
    reward = np.stack([x.reward for x in cases])
    return reward, ops.terminal_mask(cases[0].terminal, cases[0].S, batch=len(cases), device=dev)


def run_ext(mdp, reward, term):
    """(policy, status) through the C ABI (ops.backward_maxent_extended returns the policy alone): the call
    of tests/abi_call.py, which also guards the workspace and requires every output entry written (the
    status is prefilled with -7, the policy with a sentinel NaN)."""
    import abi_call
    out = abi_call.backward_maxent_extended(mdp, np.array(reward, dtype=np.float64), term)
    return out["p_action"], out["status"].cpu().numpy()


def assert_fused_plan(mdp):
    from irlmx import ops
    plan = ops.execution_plan(mdp, "backward", extended_range=True)
    assert plan["shape"] == "fused" and plan["launches"] == 1, plan
    assert plan["lds_bytes"] == 24 * mdp.n_states and plan["spt"] * plan["threads"] >= mdp.n_states, plan
    return plan


def assert_sweep_plan(mdp):
    from irlmx import ops
    plan = ops.execution_plan(mdp, "backward", extended_range=True)
    assert plan["shape"] == "sweep" and plan["launches"] == 2 * mdp.n_states - 1 and plan["threads"] == 256, plan
    return plan


def assert_within_bound(pi, cases, tag):
    got = pi.cpu().numpy()
    assert np.isfinite(got).all(), tag
    for b, c in enumerate(cases):
        e = X.elementwise_err(got[b], c.ref)
        print(f"[extended] {tag} {c.W}x{c.H}[{b}] e_twin {c.e_twin:.3e} e_kernel {e:.3e} allowed {c.bound():.3e}")
        assert e <= c.bound(), (tag, b, e, c.bound())


_fused = {}


def fused_results(dev):
    """The fused pass on every wide-range launch, computed once: [(cases, mdp, pi, status)]."""
    if not _fused:
        out = []
        for cases in launches():
            mdp = wide_mdp(cases, dev)
            assert_fused_plan(mdp)
            reward, tm = wide_inputs(cases, dev)
            pi, status = run_ext(mdp, reward, tm)
            out.append((cases, mdp, pi, status))
        _fused["v"] = out
    return _fused["v"]


# -- 4. wide range, fused --------------------------------------------------------

def test_wide_range_fused(dev, env):
    from irlmx import ops
    for cases, mdp, pi, status in fused_results(dev):
        assert (status == 0).all(), status
        assert_within_bound(pi, cases, "fused")
        reward, tm = wide_inputs(cases, dev)
        ordinary = ops.backward_maxent(mdp, reward, tm)
        n = T.nan_rows(ordinary.cpu().numpy())
        print(f"[extended] ordinary pass {cases[0].W}x{cases[0].H} x {len(cases)}: rows with NaN {n}")
        assert n > 0, "the ordinary pass no longer fails on this input"


# -- 5. bit-identical in range -----------------------------------------------------

def in_range_models(dev):
    from irlmx import DeviceMDP, _lib
    for W, H in ((16, 16), (37, 23)):
        c = C.stencil(W, H)
        yield c, DeviceMDP(_lib.LAYOUT_STENCIL5, c.S, 4, c.B, False, torch.as_tensor(c.rv.copy(), device=dev),
                           width=W, height=H, device=dev)
    c = C.ell(200)
    mdp = DeviceMDP.from_dense(c.P.copy(), device=dev, layout="ell")
    assert mdp.layout == _lib.LAYOUT_ELL and mdp.k_row == c.k_row
    yield c, mdp.with_batch(c.B)


def test_bit_identical_in_range(dev, env):
    from irlmx import ops
    for c, mdp in in_range_models(dev):
        tm = ops.terminal_mask(c.terminal, c.S, batch=c.B, device=dev)
        env({})
        assert_fused_plan(mdp)
        fused = ops.backward_maxent_extended(mdp, c.reward.copy(), tm)
        env(SWEEP)
        assert ops.execution_plan(mdp, "backward")["shape"] == "sweep"
        assert_sweep_plan(mdp)
        ordinary = ops.backward_maxent(mdp, c.reward.copy(), tm)
        swept = ops.backward_maxent_extended(mdp, c.reward.copy(), tm)
        env({})
        assert bool(torch.isfinite(ordinary).all()), c.name
        assert torch.equal(fused, ordinary), c.name
        assert torch.equal(swept, ordinary), c.name


# -- 6. the per-sweep shape ----------------------------------------------------------

def test_per_sweep_shape(dev, env):
    from irlmx import ops
    cases, mdp, pi, _ = fused_results(dev)[0]
    reward, tm = wide_inputs(cases, dev)
    env({"IRLMX_FUSED_MAX_STATES": 0})
    assert_sweep_plan(mdp)
    swept, status = run_ext(mdp, reward, tm)
    env({})
    assert (status == 0).all() and torch.equal(swept, pi)
    big = [T.wide(128, 33, -7.0)]                     # S = 4,224: per sweep by size alone, 8,447 launches
    mdp = wide_mdp(big, dev)
    assert assert_sweep_plan(mdp)["launches"] == 8447
    reward, tm = wide_inputs(big, dev)
    pi, status = run_ext(mdp, reward, tm)
    assert (status == 0).all()
    assert_within_bound(pi, big, "sweep")


# -- 7. ELL ----------------------------------------------------------------------------

def test_ell_layout(dev, env):
    """The 64 x 4 table uploaded dense and forced to ELL.  Not bit-identical to
    the STENCIL5 result: irlmx_dense_to_ell orders a state's slots by ascending
    target (s - W, s - 1, s, s + 1, s + W; at most four of them are nonzero on a
    grid four rows high), the stencil by direction (s, s + 1, s - 1, s + W,
    s - W), so the fma chains add the same terms in another order.  The bound
    against the longdouble reference is asserted."""
    from irlmx import DeviceMDP, _lib, ops
    cases = launches()[0]
    c = cases[0]
    P = np.zeros((c.S, c.S, 4))
    s = np.arange(c.S)
    for a in range(4):
        for k in range(5):
            np.add.at(P, (s, c.nbr[k], a), c.rv[a, k])
    mdp = DeviceMDP.from_dense(P, device=dev, layout="ell")
    assert mdp.layout == _lib.LAYOUT_ELL and mdp.k_row == 4
    assert_fused_plan(mdp)
    tm = ops.terminal_mask(c.terminal, c.S, device=dev)
    for b, case in enumerate(cases):                  # the three rewards on the one (slip 0.2) table
        pi, status = run_ext(mdp, case.reward, tm)
        assert (status == 0).all()
        assert_within_bound(pi, [case], f"ell[{b}]")


# -- 8. non-finite rewards and unreachable states ------------------------------------

def test_nonfinite_reward(dev, env):
    from irlmx import _lib, ops
    cases = launches()[0][:2]
    mdp = wide_mdp(cases, dev)
    reward, tm = wide_inputs(cases, dev)
    reward = reward.copy()
    reward[0, 17] = 800.0                             # exp(800) = inf
    assert_fused_plan(mdp)
    pi, status = run_ext(mdp, reward, tm)
    assert bool(torch.isnan(pi[0]).all())
    assert torch.equal(pi[1], fused_results(dev)[0][2][1])
    # the ordinary pass: NaN everywhere too (bwd_nonfinite_rule), and its status
    lib = _lib.load()
    r = torch.as_tensor(reward, device=dev)
    opi = torch.empty_like(pi)
    ost = torch.full((2,), -7, dtype=torch.int32, device=dev)
    ws, n = ops._workspace(mdp, _lib.OP_BACKWARD)
    _lib.check(lib.irlmx_backward_maxent(mdp.struct(), _lib.ptr(r), _lib.ptr(tm), 1, _lib.ptr(opi), _lib.ptr(ost),
                                         _lib.ptr(ws), n, _lib.stream_ptr(dev)), "backward_maxent")
    assert bool(torch.isnan(opi[0]).all())
    assert np.array_equal(status, ost.cpu().numpy()), (status, ost)
    env({"IRLMX_FUSED_MAX_STATES": 0})
    assert_sweep_plan(mdp)
    swept, status2 = run_ext(mdp, reward, tm)
    env({})
    assert bool(torch.isnan(swept[0]).all()) and torch.equal(swept[1], pi[1]) and np.array_equal(status2, status)


def test_unreachable_region(dev, env):
    """A deterministic gridworld whose columns x <= 1 cannot be left: those
    states never reach the terminal, zs = 0 there and the policy is 0 / 0 = NaN,
    as in the reference (maxent.py:159); actions that lead into the region get
    probability exactly 0.  The NaN and zero patterns equal the twin's and the
    ordinary pass's; the values are bit-identical to the ordinary pass (in range)."""
    from irlmx import DeviceMDP, _lib, ops
    size = 8
    S = size * size
    base = DeviceMDP.gridworld(size, device=dev)
    rv = base.row_val.cpu().numpy()[0].copy()         # [4, 5, S]
    s = np.arange(S)
    edge = s % size == 1
    rv[:, 0, edge] += rv[:, 1, edge]                  # the step +x from x = 1 stays instead
    rv[:, 1, edge] = 0.0
    mdp = DeviceMDP(_lib.LAYOUT_STENCIL5, S, 4, 1, False, torch.as_tensor(rv[None], device=dev), width=size,
                    height=size, device=dev)
    reward = np.random.default_rng(S).uniform(-1.0, 0.0, S)
    tm = ops.terminal_mask([S - 1], S, device=dev)
    assert_fused_plan(mdp)
    pi, status = run_ext(mdp, reward, tm)
    got = pi[0].cpu().numpy()
    walled = s % size <= 1
    assert np.isnan(got[walled]).all() and np.isfinite(got[~walled]).all() and (status == 0).all()
    assert (got[s % size == 2, 1] == 0).all()         # action -x from x = 2 leads into the region
    twin = T.backward(rv, T.stencil_nbr(size, size), [S - 1], reward)
    e = X.elementwise_err(got, twin)                  # (NaN and zero patterns must match exactly)
    assert e <= X.bound(0, 5, 4), e
    env(SWEEP)
    ordinary = ops.backward_maxent(mdp, reward, tm)
    env({})
    assert np.array_equal(ordinary[0].cpu().numpy(), got, equal_nan=True)


# -- 9. driver and drop-in ---------------------------------------------------------------

def test_batched_driver(dev, env):
    from irlmx import ops
    from irlmx.batch import BatchedMaxEnt
    cases, mdp, pi_ext, _ = fused_results(dev)[0]
    reward, tm = wide_inputs(cases, dev)
    S = cases[0].S
    # The demonstrations start in the terminal state, so that step()'s forward pass
    # ends (two sweeps).  These rewards make state 0 a trap: its self-loop weight
    # exp(0) * sum_a P[0, 0, a] = 2 lets zs(0) outgrow every other state, the
    # MaxEnt policy points towards state 0 everywhere, and from any other start
    # the visitation frequencies grow by 0.757 per sweep without losing mass
    # (float64 oracle, 4,000 sweeps): `while delta > eps` (maxent.py:108) never
    # ends, in the reference as on the device.
    p0 = np.zeros((3, S))
    p0[:, S - 1] = 1.0
    e_features = np.full((3, S), 1.0 / S)

    def driver(mode):
        return BatchedMaxEnt(mdp, e_features, p0, cases[0].terminal, theta0=reward, extended_range=mode)

    assert_fused_plan(mdp)
    assert torch.equal(driver(True).backward(), pi_ext)
    off = driver(False).backward()
    assert np.array_equal(off.cpu().numpy(), ops.backward_maxent(mdp, reward, tm).cpu().numpy(), equal_nan=True)
    auto = driver("auto").backward()
    assert torch.equal(auto, pi_ext)
    # the third instance (lo = -9) is in range: auto leaves the ordinary pass's rows as they are
    assert bool(torch.isfinite(off[2]).all()) and bool((off[2] != 0).all())
    assert torch.equal(auto[2], off[2])
    assert not bool(torch.isfinite(off[0]).all())
    d = driver(True)
    d.step()
    assert bool(torch.isfinite(d.theta).all())
    with pytest.raises(ValueError):
        driver("always")
    causal = BatchedMaxEnt(mdp, e_features, p0, cases[0].terminal, theta0=reward, causal=True, discount=0.7,
                           extended_range=True)
    assert causal.causal and causal.extended_range is True   # accepted and ignored (soft VI: log domain)


DROPIN = textwrap.dedent("""
    import sys
    sys.path[:0] = [{root!r}, {pkg!r}, {oracle!r}, {tests!r}]
    import numpy as np, torch
    import __graft_entry__ as g
    g.build()
    import extended_twin as T
    import maxent
    from irlmx import DeviceMDP, _lib
    c = T.wide(64, 4, -15.0)
    dev = torch.device("cuda", 0)
    mdp = DeviceMDP(_lib.LAYOUT_STENCIL5, c.S, 4, 1, False, torch.as_tensor(c.rv[None].copy(), device=dev),
                    width=c.W, height=c.H, device=dev)
    np.save({out!r}, maxent.local_action_probabilities(mdp, c.terminal, c.reward))
""")


def test_dropin_switch(dev, env, tmp_path):
    """maxent.local_action_probabilities in a child process: with
    IRLMX_EXTENDED_RANGE=1 the extended pass's policy (after the numpy-order
    attempt, which underflows to NaN here), unset today's output."""
    from irlmx import ops
    cases, _, pi_ext, _ = fused_results(dev)[0]
    c = cases[0]
    got = {}
    for flag in ("1", None):
        out = str(tmp_path / f"pi_{flag}.npy")
        code = DROPIN.format(root=ROOT, pkg=PKG_DIR, oracle=ORACLE_DIR, tests=TESTS_DIR, out=out)
        e = {k: v for k, v in os.environ.items() if k not in KEYS + ("IRLMX_EXTENDED_RANGE",)}
        if flag:
            e["IRLMX_EXTENDED_RANGE"] = flag
        subprocess.run([sys.executable, "-c", code], env=e, cwd=ROOT, check=True, timeout=300)
        got[flag] = np.load(out)
    assert np.array_equal(got["1"], pi_ext[0].cpu().numpy())
    mdp1 = wide_mdp([c], dev)
    reward, tm = wide_inputs([c], dev)
    today = ops.backward_maxent(mdp1, reward, tm)[0].cpu().numpy()
    assert T.nan_rows(today) > 0
    assert np.array_equal(got[None], today, equal_nan=True)


# -- 10. the device bounds-check build ------------------------------------------------------

CHECKS = textwrap.dedent("""
    import json, os, sys
    sys.path[:0] = [{root!r}, {pkg!r}, {oracle!r}, {tests!r}]
    import numpy as np, torch
    import extended_twin as T
    import test_gpu_extended_range as G
    from irlmx import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    out = {{"enabled": int(lib.irlmx_device_checks_enabled()), "fails": []}}
    arrays = {{}}
    for i, cases in enumerate(G.launches()):
        mdp = G.wide_mdp(cases, dev)
        G.assert_fused_plan(mdp)
        reward, tm = G.wide_inputs(cases, dev)
        arrays[f"fused{{i}}"] = ops.backward_maxent_extended(mdp, reward, tm).cpu().numpy()
        out["fails"].append(ops.device_check_failures())
    os.environ["IRLMX_FUSED_MAX_STATES"] = "0"
    cases = G.launches()[0]
    mdp = G.wide_mdp(cases, dev)
    G.assert_sweep_plan(mdp)
    reward, tm = G.wide_inputs(cases, dev)
    arrays["sweep0"] = ops.backward_maxent_extended(mdp, reward, tm).cpu().numpy()
    out["fails"].append(ops.device_check_failures())
    del os.environ["IRLMX_FUSED_MAX_STATES"]
    big = [T.wide(128, 33, -7.0)]
    mdp = G.wide_mdp(big, dev)
    G.assert_sweep_plan(mdp)
    reward, tm = G.wide_inputs(big, dev)
    arrays["big"] = ops.backward_maxent_extended(mdp, reward, tm).cpu().numpy()
    out["fails"].append(ops.device_check_failures())
    np.savez({npz!r}, **arrays)
    json.dump(out, open({out!r}, "w"))
""")


def test_device_check_build(dev, env, tmp_path):
    """Tests 4 and 6 under libirlmx_checks.so: no failed bounds check, and the
    same bits as the product build (same arithmetic: the checks only guard indices)."""
    import __graft_entry__ as g
    res, npz = str(tmp_path / "checks.json"), str(tmp_path / "checks.npz")
    code = CHECKS.format(root=ROOT, pkg=PKG_DIR, oracle=ORACLE_DIR, tests=TESTS_DIR, out=res, npz=npz)
    e = {k: v for k, v in os.environ.items() if k not in KEYS}
    e["IRLMX_LIB"] = g.LIB_CHECKS
    subprocess.run([sys.executable, "-c", code], env=e, cwd=ROOT, check=True, timeout=300)
    out = json.load(open(res))
    assert out["enabled"] == 1
    assert out["fails"] == [0, 0, 0, 0, 0], out["fails"]
    z = np.load(npz)
    fused = fused_results(dev)
    for i, (_, _, pi, _) in enumerate(fused):
        assert np.array_equal(z[f"fused{i}"], pi.cpu().numpy()), i
    assert np.array_equal(z["sweep0"], fused[0][2].cpu().numpy())
    big = [T.wide(128, 33, -7.0)]
    assert np.isfinite(z["big"]).all()
    assert X.elementwise_err(z["big"][0], big[0].ref) <= big[0].bound()
