"""The finite-horizon expected SVF in one call on the device (needs an MI355X).

ops.expected_svf_horizon (csrc/expected_svf_horizon.hip) against the two-call
path it replaces -- ops.backward_maxent_horizon or ops.soft_backward_horizon,
then ops.forward_svf_horizon -- on cases of tests/horizon_twin.py, for both
models (the causal one at discounts 1.0 and 0.9), each case asserting its plan
first:

* bit for bit: svf, objective0 (log_z0 / V_0) and status equal the two-call
  path's as int64 patterns with NaN in the same places, for the segment lengths
  C in {0, 1, 3, T, T + 5} and in both shapes; the batch reversed, every
  instance of a per-instance-table launch alone, the device bounds-check build;
* non-finite inputs: a reward of +800 (exp(r) = inf) and a NaN reward in one
  instance give the two-call path's NaN pattern and status, the other
  instances untouched;
* an independent anchor: svf elementwise against the longdouble forward fed the
  longdouble backward, under 16 x max(e_twin, e_floor), the project's rule;
* memory: at T = 4096 the one-call path raises the peak by less than 4 MB where
  the two-call path raises it by more than 100 MB;
* the call contract (guarded dirty workspaces, poisoned outputs) and the stream
  order (side stream, behind a delay, claim "asynchronous") in both shapes;
* the batched drivers and the four drop-ins with ``stream_policy``.
"""

import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import abi_call as A
import expected_svf_call as EC
import extended_ref as X
import horizon_twin as H
import soft_horizon_twin as SH
import test_gpu_call_contract as CC
import test_gpu_stream_order as SO
from conftest import ORACLE_DIR, PKG_DIR, ROOT
from test_gpu_stream_order import cycles_per_ms, streams  # noqa: F401  (module-scoped fixtures, instantiated here)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KEY = "IRLMX_FUSED_MAX_STATES"            # 0: every size per step
BATCH_KEY = "IRLMX_HORIZON_FUSED_BATCH"
TESTS_DIR = os.path.join(ROOT, "tests")
NP_TABLES = 64 * 8 + 256 * 4              # sizeof(NpTables), csrc/common.h

CASES = ("16x16", "37x23", "64x12-stay", "16x16-T1", "128x40", "k8-s1029", "k40-s300")
#: the cases the fused shape runs: at most 1,024 states, at most 32 column slots
FUSED = ("16x16", "37x23", "64x12-stay", "16x16-T1")
MODELS = (("maxent", 1.0), ("causal", 1.0), ("causal", 0.9))
MODEL_IDS = ["maxent", "causal-1.0", "causal-0.9"]


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    import irlmx
    return irlmx.require_device()


@pytest.fixture
def env(monkeypatch):
    """``env("sweep")``: every size through the per-step shape; cleared afterwards."""
    def set_env(mode="default"):
        monkeypatch.delenv(KEY, raising=False)
        monkeypatch.delenv(BATCH_KEY, raising=False)
        if mode == "sweep":
            monkeypatch.setenv(KEY, "0")
    set_env()
    yield set_env
    set_env()


def segments(T):
    return (0, 1, 3, T, T + 5)


def terminal_of(c, mdp):
    from irlmx import ops
    return ops.terminal_mask(c.terminal, c.S, batch=mdp.batch, device=mdp.device) if c.terminal else None


def two_call(c, mdp, model, discount, reward, p0):
    """svf, objective0 and status of the two-call path through the C ABI (the ops do not
    return the backward's status): status is the OR of both calls'."""
    tm = terminal_of(c, mdp)
    if model == "maxent":
        bw = A.backward_maxent_horizon(mdp, reward, c.T, tm)
        obj = bw["log_z0"]
    else:
        bw = A.soft_backward_horizon(mdp, reward, discount, c.T, tm)
        obj = bw["value0"]
    fw = A.forward_svf_horizon(mdp, p0, bw["p_action_t"], tm, svf_t=False)
    return {"svf": fw["svf"].cpu().numpy(), "obj": obj.cpu().numpy(),
            "status": (bw["status"] | fw["status"]).cpu().numpy()}


def one_call(c, mdp, model, discount, reward, p0, segment):
    from irlmx import ops
    svf, sweeps, status, obj = ops.expected_svf_horizon(mdp, reward, p0, c.T, model=model, discount=discount,
                                                        terminal=terminal_of(c, mdp), segment=segment,
                                                        return_objective=True)
    assert sweeps.tolist() == [c.T] * mdp.batch
    return {"svf": svf.cpu().numpy(), "obj": obj.cpu().numpy(), "status": status.cpu().numpy()}


def same(got, ref, what):
    """int64 bit patterns equal, NaN in the same places (payload bits are not compared)."""
    for k in ref:
        x, y = got[k], ref[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        if x.dtype != np.float64:
            assert np.array_equal(x, y), f"{what}: {k} differs: {x} against {y}"
            continue
        nan = np.isnan(y)
        assert np.array_equal(np.isnan(x), nan), f"{what}: NaN pattern of {k} differs"
        diff = x[~nan].view(np.int64) != y[~nan].view(np.int64)
        assert not diff.any(), f"{what}: {int(diff.sum())} of {x.size} entries of {k} differ"


def assert_plan(c, mdp, model, mode, segment=0):
    from irlmx import ops
    p = ops.expected_svf_horizon_plan(mdp, c.T, model, segment)
    T = c.T
    C = min(segment, T) if segment else int(np.ceil(np.sqrt(T)))
    nseg = -(-T // C)
    fused = mode == "default" and c.name in FUSED
    lds = (NP_TABLES if model == "causal" else 0) + 8 * c.S * (c.A + 2)
    assert (p["shape"], p["launches"], p["lds_bytes"]) == (("fused", 1, lds) if fused else ("sweep", 0, 0)), (c.name, p)
    assert p["segment"] == C and p["slices"] == nseg + C - 1 + (2 if nseg > 1 else 0), (c.name, p)
    assert 0 < p["workspace_bytes"] <= (nseg + C + c.A + 6) * mdp.batch * c.S * 12 + 4096, (c.name, p)
    return p


_reference = {}


def reference(name, model, discount, dev):
    """The two-call path's result on the case's own inputs, computed once (default plan)."""
    key = (name, model, discount)
    if key not in _reference:
        c = H.case(name)
        _reference[key] = two_call(c, c.device_model(dev), model, discount, np.array(c.reward), np.array(c.p0))
    return _reference[key]


# ---------------------------------------------------------------------------
# bit identity
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("model,discount", MODELS, ids=MODEL_IDS)
@pytest.mark.parametrize("name", CASES)
def test_bits_of_the_two_call_path(dev, env, name, model, discount):
    """Every C, both shapes: the two-call path's bits."""
    from irlmx import _lib
    c = H.case(name)
    mdp = c.device_model(dev)
    ref = reference(name, model, discount, dev)
    assert ref["status"].tolist() == [_lib.OK] * c.B
    assert np.isfinite(ref["svf"]).all() and not np.isnan(ref["obj"]).any()
    if not c.terminal:
        np.testing.assert_allclose(ref["svf"].sum(axis=1), c.T + 1, rtol=1e-12)
    for mode in ("default", "sweep"):
        env(mode)
        for seg in segments(c.T):
            assert_plan(c, mdp, model, mode, seg)
            got = one_call(c, mdp, model, discount, np.array(c.reward), np.array(c.p0), seg)
            same(got, ref, f"{name} {model} {discount} {mode} C={seg}")
    # objective0 NULL: the same svf and status
    from irlmx import ops
    svf, _, status = ops.expected_svf_horizon(mdp, np.array(c.reward), np.array(c.p0), c.T, model=model, discount=discount,
                                              terminal=terminal_of(c, mdp), segment=3)
    same({"svf": svf.cpu().numpy(), "status": status.cpu().numpy()}, {"svf": ref["svf"], "status": ref["status"]},
         f"{name} without objective0")


@pytest.mark.parametrize("model,discount", MODELS, ids=MODEL_IDS)
@pytest.mark.parametrize("name", ["16x16", "128x40", "k8-s1029", "k40-s300"])
def test_batch_reversed_and_instances_alone(dev, env, name, model, discount):
    """Per-instance tables: the batch reversed gives the reversed result, each instance alone its own rows."""
    c = H.case(name)
    assert c.B > 1 and len(c.models) == c.B
    ref = reference(name, model, discount, dev)
    for mode in ("default", "sweep"):
        env(mode)
        for tables in (list(range(c.B))[::-1],) + tuple([b] for b in range(c.B)):
            mdp = c.device_model(dev, tables=tables)
            got = one_call(c, mdp, model, discount, c.reward[tables], c.p0[tables], 3)
            same(got, {k: v[tables] for k, v in ref.items()}, f"{name} {model} {mode} tables {tables}")


CHECKS = textwrap.dedent("""
    import json, os, sys
    sys.path[:0] = [{root!r}, {pkg!r}, {oracle!r}, {tests!r}]
    import numpy as np
    import __graft_entry__ as g
    import irlmx
    from irlmx import _lib, ops
    import horizon_twin as H
    import test_gpu_expected_svf as G
    dev = irlmx.require_device()
    out = {{"enabled": int(_lib.load().irlmx_device_checks_enabled()), "fails": []}}
    arrays = {{}}
    for sweep in (0, 1):
        if sweep:
            os.environ[G.KEY] = "0"
        for name in {names!r}:
            c = H.case(name)
            mdp = c.device_model(dev)
            for model, discount in G.MODELS:
                got = G.one_call(c, mdp, model, discount, np.array(c.reward), np.array(c.p0), 3)
                out["fails"].append(ops.device_check_failures())
                for k, v in got.items():
                    arrays[f"{{name}}.{{model}}.{{discount}}.{{sweep}}.{{k}}"] = v
    np.savez({npz!r}, **arrays)
    json.dump(out, open({out!r}, "w"))
""")


def test_device_check_build(dev, env, tmp_path):
    """ELL and stencil cases under libirlmx_checks.so, fused and per step: no
    check bit set and the two-call path's bits."""
    import __graft_entry__ as g
    names = ("16x16", "k8-s1029", "k40-s300", "37x23")
    res, npz = str(tmp_path / "checks.json"), str(tmp_path / "checks.npz")
    code = CHECKS.format(root=ROOT, pkg=PKG_DIR, oracle=ORACLE_DIR, tests=TESTS_DIR, out=res, npz=npz, names=names)
    e = {k: v for k, v in os.environ.items() if k not in (KEY, BATCH_KEY)}
    e["IRLMX_LIB"] = g.LIB_CHECKS
    subprocess.run([sys.executable, "-c", code], env=e, cwd=ROOT, check=True, timeout=300)
    out = json.load(open(res))
    assert out["enabled"] == 1 and out["fails"] == [0] * (2 * len(names) * len(MODELS)), out
    z = np.load(npz)
    for name in names:
        for model, discount in MODELS:
            ref = reference(name, model, discount, dev)
            for sweep in (0, 1):
                same({k: z[f"{name}.{model}.{discount}.{sweep}.{k}"] for k in ref}, ref, f"checks build {name} {model} {sweep}")


# ---------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("model,discount", MODELS, ids=MODEL_IDS)
@pytest.mark.parametrize("what,value", [("inf", 800.0), ("nan", float("nan"))])
def test_non_finite_reward(dev, env, what, value, model, discount):
    """exp(800) = inf and a NaN reward in instance 1 of 16x16: the two-call path's NaN
    pattern and status; instances 0 and 2 keep the bits of the clean input."""
    from irlmx import _lib
    c = H.case("16x16")
    mdp = c.device_model(dev)
    reward = np.array(c.reward)
    reward[1, 37] = value
    ref = two_call(c, mdp, model, discount, reward, np.array(c.p0))
    clean = reference("16x16", model, discount, dev)
    for b in (0, 2):
        same({k: v[b] for k, v in ref.items()}, {k: v[b] for k, v in clean.items()}, f"two-call path, instance {b}")
    if model == "maxent" or what == "nan":
        assert ref["status"].tolist() == [_lib.OK, _lib.NONFINITE, _lib.OK], ref["status"]
        assert np.isnan(ref["svf"][1]).any() and np.isnan(ref["obj"][1]).any()
    if model == "maxent":                                         # NaN rows everywhere, log_z0 NaN
        assert np.isnan(ref["obj"][1]).all()
    for mode in ("default", "sweep"):
        env(mode)
        for seg in segments(c.T):
            got = one_call(c, mdp, model, discount, reward, np.array(c.p0), seg)
            same(got, ref, f"16x16 {what} {model} {discount} {mode} C={seg}")


# ---------------------------------------------------------------------------
# an independent anchor: the longdouble forward fed the longdouble backward
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("model,discount", MODELS, ids=MODEL_IDS)
@pytest.mark.parametrize("name", ["16x16", "k8-s1029"])
def test_against_the_longdouble_passes(dev, env, name, model, discount):
    """svf elementwise under 16 x max(e_twin, e_floor): e_twin is the error of the
    float64 twins (backward, then forward on its own policy) against the same reference."""
    c = H.case(name)
    got = one_call(c, c.device_model(dev), model, discount, np.array(c.reward), np.array(c.p0), 0)
    for b in range(c.B):
        if model == "maxent":
            pi_ref, pi_twin = c.ref_backward(b)[0], c.twin_backward(b)[0]
        else:
            pi_ref, pi_twin = SH.ref(name, discount, b)[0], SH.twin(name, discount, b)[0]
        rD = H.forward_ref(c.model(b).mats, c.p0[b], c.terminal, pi_ref)[0]
        e_twin = X.elementwise_err(H.forward(c.model(b), c.p0[b], c.terminal, pi_twin)[0], rD)
        e = X.elementwise_err(got["svf"][b], rD)
        bound = c.bound_svf(e_twin)
        print(f"[expected-svf] {name}[{b}] {model} {discount}: e_kernel {e:.2e} e_twin {e_twin:.2e} bound {bound:.2e}")
        assert e <= bound, (name, b, model, e, bound)


# ---------------------------------------------------------------------------
# memory
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("model,discount", [("maxent", 1.0), ("causal", 0.9)], ids=["maxent", "causal-0.9"])
def test_peak_memory(dev, env, model, discount):
    """16x16, B = 3, T = 4096: the one-call path at C = 0 raises the peak of allocated
    bytes by less than 4 MB; the two-call path, run second, by more than 100 MB; same bits."""
    from irlmx import ops
    c = H.case("16x16")
    mdp = c.device_model(dev)
    T = 4096
    r, p0 = SO.dv(c.reward, dev), SO.dv(c.p0, dev)
    assert ops.expected_svf_horizon_plan(mdp, T, model)["segment"] == 64

    def peak_of(fn):
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = fn()
        torch.cuda.synchronize(dev)
        return torch.cuda.max_memory_allocated(dev) - base, out

    rise1, one = peak_of(lambda: ops.expected_svf_horizon(mdp, r, p0, T, model=model, discount=discount,
                                                          return_objective=True))

    def two():
        if model == "maxent":
            pi, obj = ops.backward_maxent_horizon(mdp, r, T, return_log_z0=True)
        else:
            pi, obj = ops.soft_backward_horizon(mdp, r, discount, T, return_value0=True)
        svf, _, status = ops.forward_svf_horizon(mdp, p0, pi)
        return svf, status, obj

    rise2, (svf, status, obj) = peak_of(two)
    print(f"[expected-svf] peak rise at T = {T}: one call {rise1} bytes, two calls {rise2} bytes")
    assert rise1 < 4 * 2 ** 20, rise1
    assert rise2 > 100 * 10 ** 6, rise2
    same({"svf": one[0].cpu().numpy(), "obj": one[3].cpu().numpy(), "status": one[2].cpu().numpy()},
         {"svf": svf.cpu().numpy(), "obj": obj.cpu().numpy(), "status": status.cpu().numpy()}, f"T = {T} {model}")


# ---------------------------------------------------------------------------
# call contract and stream order
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["fused", "sweep"])
@pytest.mark.parametrize("model,discount", [("maxent", 1.0), ("causal", 0.9)], ids=["maxent", "causal-0.9"])
def test_call_contract(dev, env, shape, model, discount):
    """ops.expected_svf_horizon's bits whatever the workspace held -- the donor's rewards
    hold a NaN -- no guard byte touched and no output entry left unwritten, the
    NONFINITE instance's included; with objective0 NULL the same svf."""
    from irlmx import _lib, ops
    env("sweep" if shape == "sweep" else "default")
    c = H.case("16x16")
    mdp = c.device_model(dev)
    reward, p0 = np.array(c.reward), np.array(c.p0)
    for seg in (0, 3, c.T):
        assert ops.expected_svf_horizon_plan(mdp, c.T, model, seg)["shape"] == shape
        svf, _, status, obj = ops.expected_svf_horizon(mdp, reward, p0, c.T, model=model, discount=discount, segment=seg,
                                                       return_objective=True)
        donor = {"reward": CC.other_reward(reward), "p_initial": CC.other_p0(p0)}
        what = f"16x16/{shape} expected svf {model} C={seg}"
        full = CC.contract(what, lambda **kw: EC.expected_svf_horizon(mdp, model, reward, p0, c.T, discount, segment=seg, **kw),
                           donor, {"svf": svf, "objective0": obj, "status": status})
        assert full["status"].tolist() == [_lib.OK] * c.B
        without = CC.contract(what + ", objective0 NULL",
                              lambda **kw: EC.expected_svf_horizon(mdp, model, reward, p0, c.T, discount, segment=seg,
                                                                   objective0=False, **kw), donor, {"svf": svf})
        assert without["objective0"] is None
    bad = CC.other_reward(reward)                                   # a NaN in the last instance
    got = CC.contract(f"16x16/{shape} expected svf {model}, NaN reward",
                      lambda **kw: EC.expected_svf_horizon(mdp, model, bad, p0, c.T, discount, **kw), {"reward": reward}, {})
    assert got["status"].tolist() == [_lib.OK] * (c.B - 1) + [_lib.NONFINITE], got["status"]


@pytest.mark.parametrize("rid", [r.id for r in EC.ROWS])
def test_stream_order(dev, env, streams, cycles_per_ms, rid):  # noqa: F811
    """(r) on the default stream, (s) on a side stream, (d) behind a delay with late
    inputs: the same bits, and in (d) the call returns while the delay still runs."""
    r = EC.ROW[rid]
    env("sweep" if r.keys else "default")
    run = r.build(dev)
    claim = EC.CLAIMS[(r.entry, r.shape)]
    assert claim == SO.ASYNC
    ref = SO.three_runs(f"{r.id} {r.entry}", run, claim, streams, cycles_per_ms)
    model = "maxent" if "maxent" in rid else "causal"
    want = reference("16x16", model, 1.0 if model == "maxent" else 0.9, dev)
    same({"svf": ref["svf"].cpu().numpy(), "obj": ref["objective0"].cpu().numpy(), "status": ref["status"].cpu().numpy()},
         want, rid)


# ---------------------------------------------------------------------------
# drivers and drop-ins
# ---------------------------------------------------------------------------

def _driver(cls, c, mdp, stream_policy, compact, **kw):
    """Six steps from theta = 0.5; instance 0's demonstrations are its own expected
    visitation there, so its gradient is an exact 0, it stops after one step and
    compaction has something to drop."""
    from irlmx import ops
    rng = np.random.default_rng(5)
    e = rng.uniform(0.0, 1.0, (c.B, c.S))
    e *= (12 + 1) / e.sum(axis=1, keepdims=True)                    # visit counts of 13 states
    r0 = np.full((c.B, c.S), 0.5)
    pi = ops.soft_backward_horizon(mdp, r0, kw["discount"], 12) if kw else ops.backward_maxent_horizon(mdp, r0, 12)
    e[0] = ops.forward_svf_horizon(mdp, np.array(c.p0), pi)[0][0].cpu().numpy()
    d = cls(mdp, e, np.array(c.p0), [], horizon=12, theta0=0.5, stream_policy=stream_policy, **kw)
    d.run(max_steps=6, compact=compact)
    assert d.k == 6 and d.steps.tolist() == [1, 6, 6], (d.k, d.steps)
    return d


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("kind", ["maxent", "causal"])
def test_drivers(dev, env, kind, compact):
    """BatchedMaxEnt(horizon=12, stream_policy=True) and BatchedCausalHorizon(stream_policy=5):
    theta, steps and last_forward_sweeps of stream_policy=False, bit for bit."""
    from irlmx.batch import BatchedCausalHorizon, BatchedMaxEnt
    c = H.case("16x16")
    mdp = c.device_model(dev)
    cls, kw, sp = (BatchedMaxEnt, {}, True) if kind == "maxent" else (BatchedCausalHorizon, {"discount": 0.9}, 5)
    base = _driver(cls, c, mdp, False, compact, **kw)
    got = _driver(cls, c, mdp, sp, compact, **kw)
    assert (got.working_batch == 2) == compact
    assert torch.equal(got.theta.view(torch.int64), base.theta.view(torch.int64))
    assert torch.equal(got.steps, base.steps) and torch.equal(got.last_forward_sweeps, base.last_forward_sweeps)
    assert torch.equal(got.active, base.active)
    svf, sweeps, status = got.expected_svf()                       # the working set's, against forward(backward())
    svf2, sweeps2, status2 = got.forward(got.backward())
    assert torch.equal(svf.view(torch.int64), svf2.view(torch.int64)) and torch.equal(sweeps, sweeps2)
    assert torch.equal(status, status2)


@pytest.mark.parametrize("stream_policy,segment", [(True, 0), (1, 1), (5, 5), (0, 0)])
def test_stream_policy_names_the_segment(dev, env, monkeypatch, stream_policy, segment):
    """True is C = ceil(sqrt(T)); an int is that segment length, 1 included (1 == True in Python)."""
    from irlmx import ops
    from irlmx.batch import BatchedMaxEnt
    c = H.case("16x16")
    seen = []
    real = ops.expected_svf_horizon

    def spy(*args, **kw):
        seen.append(kw["segment"])
        return real(*args, **kw)

    monkeypatch.setattr(ops, "expected_svf_horizon", spy)
    d = BatchedMaxEnt(c.device_model(dev), np.full((c.B, c.S), 13.0 / c.S), np.array(c.p0), [], horizon=12,
                      stream_policy=stream_policy)
    d.step()
    assert seen == [segment]


def test_stream_policy_needs_a_horizon(dev):
    from irlmx.batch import BatchedMaxEnt
    c = H.case("16x16")
    mdp = c.device_model(dev)
    with pytest.raises(ValueError, match="stream_policy needs a horizon"):
        BatchedMaxEnt(mdp, np.zeros((c.B, c.S)), np.array(c.p0), [0], stream_policy=True)
    with pytest.raises(ValueError, match="stream_policy must be"):
        BatchedMaxEnt(mdp, np.zeros((c.B, c.S)), np.array(c.p0), [], horizon=4, stream_policy=-2)


def test_drop_ins(dev, env):
    """The four drop-ins with stream_policy=True (and an int C): what they return without it, bit for bit."""
    import maxent as M
    import maxent_oracle as O
    from conftest import load_golden, unpack_trajectories
    z = load_golden("config1")
    T = 10
    tjs = [O.Trajectory(t.transitions()[:T]) for t in unpack_trajectories(z["traj_flat"], z["traj_lens"])]
    P = z["p_transition"]
    p0 = M.initial_probabilities_from_trajectories(25, tjs)
    reward = np.random.default_rng(9).uniform(-1.0, 0.0, 25)

    def bits(x):
        return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)

    for term in ([], [24]):
        want = M.compute_expected_svf_horizon(P, p0, term, reward, T)
        wantc = M.compute_expected_causal_svf_horizon(P, p0, term, reward, 0.9, T)
        for sp in (True, 4, 100):
            assert np.array_equal(bits(M.compute_expected_svf_horizon(P, p0, term, reward, T, stream_policy=sp)), bits(want))
            assert np.array_equal(bits(M.compute_expected_causal_svf_horizon(P, p0, term, reward, 0.9, T, stream_policy=sp)),
                                  bits(wantc))
    assert abs(want.sum() - (T + 1)) > 1e-6 and not np.array_equal(want, wantc)       # (the terminal absorbs; two models)

    def irl(fn, *args, **kw):                    # a loose stopping rule keeps the two runs short
        opt = O.ExpSga(lr=O.linear_decay(0.2))
        out = fn(P, np.identity(25), [], tjs, opt, O.Constant(1.0), *args, eps=5e-3, **kw)
        return out, opt.k

    for fn, args in ((M.irl_horizon, (T,)), (M.irl_causal_horizon, (0.9, T))):
        base, k = irl(fn, *args)
        got, k2 = irl(fn, *args, stream_policy=True)
        assert 3 < k == k2 < 2000 and np.isfinite(base).all(), (k, k2)
        assert np.array_equal(bits(got), bits(base)), fn.__name__
