"""The call contract of include/irlmx.h on the device (needs an MI355X): guarded
dirty workspaces and poisoned outputs, for every entry point that takes a
workspace and every execution shape.

Every numerical test of this project goes through ``irlmx.ops``, whose scratch
memory and outputs come from torch's caching allocator: a block that the
previous call of the same size just used, and that often still holds that
call's correct flags, counters, granules and answers.  Here each call goes
through tests/abi_call.py instead.  Per case, after the plan is asserted:

(a) the call on a zeroed workspace returns the bits ``ops.*`` returns on the
    same inputs -- and that ``ops`` result is first judged against the
    extended-precision reference or the family's twin, by the helpers of the
    suite the case comes from (elementwise_run.run_*, extended_twin,
    horizon_twin, policy_eval_twin);
(b) on a workspace of 0xFF bytes and on one exactly as a donor call left it
    (same entry point and model, other rewards with a NaN in the last
    instance, another p0 or policy, a sweep cap of 7) it returns the same bits
    again: policy or values, sweep counts and status;
(c) in all three runs the 64 KiB guards on both sides of the workspace are
    intact and no output entry keeps its sentinel (abi_call raises otherwise).

tests/test_call_contract_host.py shows on the CPU that these checks can fail.
No case invents inputs: each is the smallest one an existing suite runs on
that shape.  The one cluster case of the suite with more than one launch
(test_gpu_parity: 256 x 256 x 33) takes far longer than a few seconds and is
left out.

What initialises each carved piece, and what reads it first
-----------------------------------------------------------
Read from the entry points and their kernels before any of this ran.  No
persistent kernel polls a word the call has not written: every tagged
granule area is zeroed by a memset of the same call (tag 0 is never a valid
tag), so no fill can make a kernel wait for its exchange timeout.

Stationary families -- irlmx_forward_svf, irlmx_backward_maxent,
irlmx_soft_backward, irlmx_value_iteration (carve(), fixed_point.hip):
  the entry point's hipMemsetAsync(workspace, 0, total) covers every piece
  before the first kernel; what each piece holds when it is first read:
  wgt     forward: fwd_weights_kernel / dense_fwd_weights_launch write all of
          it, read by the fused, cluster, grid, dense-grid and sweep kernels;
          backward: bwd_weights_launch (dense GEMM: dense_gemm_launch writes
          the product each sweep before dense_bwd_gemm_epilogue reads it);
          soft VI / VI on a shared dense table: dense_bellman_gemm_sweep_launch
          writes the A products before its epilogue reads them
  bad     0 from the memset, set by atomicOr in the weights kernels; read by
          the loop kernels and bwd_nan_fill_kernel
  buf0/1  forward: d = 0 from the memset; backward: bwd_init_kernel /
          dense_bwd_init_launch; soft VI / VI: fill_kernel; each sweep writes
          the other buffer in full before the next reads it
  slots, done, iters, ndone
          0 from the memset; sweep_should_stop and run_until_done's host poll
          read them, the fused kernels keep them in LDS
  gran, sgran
          0 from the memset (untagged); cluster, grid and dense-grid kernels
          publish before they poll
  growth  bwd_growth_kernel writes [2][B] before cluster_run's kernel reads it
  err     0 from the memset; err[1..2] are the rendezvous counters (reset by
          cluster_run before each further launch), err[3] the compact-layout
          flag bwd_compact_check zeroes itself before its kernel
  Reruns: the cluster rerun memsets the whole workspace again and rebuilds the
  weights; the grid / dense-grid rerun (grid_launch_outcome) zeroes the four
  err words -- the abandoned launch left at its rendezvous and wrote nothing else.

irlmx_backward_maxent_extended (ext_carve(), extended.hip):
  wgt     bwd_weights_launch writes all of it; read by every shape's kernel
  bad     hipMemsetAsync(ws.bad) in the entry point, atomicOr in the weights kernel
  man[0], exp[0]   ext_init_kernel (per-sweep shape only; fused keeps them in LDS)
  man[1], exp[1]   ext_sweep_kernel's first sweep, before the second reads them
  gran, dgran, err (grid shape) ext_grid_run's three memsets before every launch

irlmx_backward_maxent_horizon / irlmx_forward_svf_horizon (hz_carve(), horizon.hip):
  fused shape: no workspace at all (0 bytes: a NULL pointer is passed here)
  bad     backward: hipMemsetAsync(ws.bad) in the entry point, atomicOr in hz_bwd_init_kernel
  man[0], exp[0]   hz_bwd_init_kernel / hz_fwd_init_kernel (the forward has no exp)
  man[1], exp[1]   the first hz_*_step_kernel, before the second reads them
  irlmx_soft_backward_horizon (the same hz_carve(): man[0..1] alone, as the forward; its kernels' v[0..1]):
  v[0]    value_hz_init_kernel<SoftPass> writes all of it
  v[1]    the first value_hz_step_kernel<SoftPass>, before the second reads it

irlmx_policy_evaluation (carve(), fixed_point.hip; policy_eval.hip):
  wgt     pe_weights_kernel writes all of it; read by pe_fused_kernel / pe_sweep_kernel
  everything after wgt (bad, buf0, buf1, slots, done, iters, ndone)
          fused shape: never read (v, the ring and the counters are in LDS);
          per-sweep shape: one hipMemsetAsync from ws.bad to the end before pe_sweep_kernel

The reading found no word that is read before it is written.
"""


import numpy as np
import pytest

import abi_call as A
import elementwise_cases as C
import elementwise_run as E
import ell_cases as L
import extended_ref as X
import horizon_twin as H
import policy_eval_twin as PT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TAG = "call-contract"
KEYS = E.KEYS + ("IRLMX_HORIZON_FUSED_BATCH", "IRLMX_EXT_GRID_MIN_STATES", "IRLMX_EXT_GRID_MAX_LAUNCHES",
                 "IRLMX_TEST_NOT_RESIDENT", "IRLMX_STRICT_EXCHANGE", "IRLMX_TEST_EXCHANGE_TIMEOUT_MS")
DEFAULT = {}
SWEEP = dict(E.SWEEP)
NO_FUSED = {"IRLMX_FUSED_MAX_STATES": 0}
BELLMAN_GRID = {"IRLMX_FUSED_MAX_STATES": 0, "IRLMX_CLUSTER": 0}
#: tests/test_gpu_extended_grid.py's keys: the grid shape at any size, a protocol error fails within 2 s
EXT_GRID = {"IRLMX_EXT_GRID_MIN_STATES": 0, "IRLMX_FUSED_MAX_STATES": 0, "IRLMX_EXT_GRID_MAX_LAUNCHES": 3,
            "IRLMX_STRICT_EXCHANGE": 1, "IRLMX_TEST_EXCHANGE_TIMEOUT_MS": 2000}
DENSE_ENV = {"dense": {"IRLMX_DENSE_GEMM_MIN": 1000000, "IRLMX_DENSE_GRID": 0},
             "dense-grid": {"IRLMX_DENSE_GEMM_MIN": 1000000},
             "dense-gemm": {"IRLMX_DENSE_GEMM_MIN": 2}}
CLUSTER_64x20 = {"IRLMX_FUSED_MAX_STATES": 0, "IRLMX_CLUSTER_R": 5, "IRLMX_CLUSTER_G": 3, "IRLMX_PAIR": 0}

STENCIL, ELL, DENSE = 1, 2, 3
#: The models of the matrix below, without a device: name -> (layout, S, A, W, H, k_row, k_col, B, shared) and
#: the planner keys each is run under.  tests/test_call_contract_host.py asks irlmx_workspace_bytes for every
#: op of every one of them; ``model()`` holds each device model to its row.
MODELS = {
    "16x16": ((STENCIL, 256, 4, 16, 16, 5, 5, 3, 0), (DEFAULT, SWEEP, NO_FUSED)),
    "16x16-T1": ((STENCIL, 256, 4, 16, 16, 5, 5, 1, 1), (DEFAULT, SWEEP)),
    "64x20": ((STENCIL, 1280, 4, 64, 20, 5, 5, 3, 0), (CLUSTER_64x20,)),
    "256x12": ((STENCIL, 3072, 4, 256, 12, 5, 5, 3, 0), (NO_FUSED,)),
    "37x23": ((STENCIL, 851, 4, 37, 23, 5, 5, 3, 0), (NO_FUSED, BELLMAN_GRID)),
    "64x4": ((STENCIL, 256, 4, 64, 4, 5, 5, 3, 0), (DEFAULT, NO_FUSED, EXT_GRID)),
    "k8-s1029": ((ELL, 1029, 3, 0, 0, 8, 8, 2, 0), (DEFAULT, NO_FUSED, {"IRLMX_HORIZON_FUSED_BATCH": 1})),
    "k32-s200": ((ELL, 200, 8, 0, 0, 32, 32, 2, 0), (DEFAULT,)),
    "k40-s300": ((ELL, 300, 3, 0, 0, 40, 40, 2, 0), (DEFAULT,)),
    "dense301x1": ((DENSE, 301, 3, 0, 0, 301, 301, 1, 1), (DENSE_ENV["dense"], DENSE_ENV["dense-grid"])),
    "dense301x17": ((DENSE, 301, 3, 0, 0, 301, 301, 17, 1), (DENSE_ENV["dense-gemm"],)),
}


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    import irlmx
    return irlmx.require_device()


@pytest.fixture
def env(monkeypatch):
    """Set exactly the given planner and launch keys; all of them are cleared afterwards."""
    def set_env(values):
        for k in KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in values.items():
            assert k in KEYS, k
            monkeypatch.setenv(k, str(v))
    set_env({})
    yield set_env
    set_env({})


def model(name, mdp):
    """``mdp`` is the model MODELS names (``shared`` matters to the workspace of a DENSE table only)."""
    from irlmx import _lib
    stencil = mdp.layout == _lib.LAYOUT_STENCIL5            # (the struct's slot counts of a stencil are 5)
    got = (mdp.layout, mdp.n_states, mdp.n_actions, mdp.width, mdp.height, 5 if stencil else mdp.k_row,
           5 if stencil else mdp.k_col, mdp.batch, int(mdp.shared))
    want = MODELS[name][0]
    n = 9 if want[0] == DENSE else 8
    assert got[:n] == want[:n], (name, got, want)
    return mdp


# ---------------------------------------------------------------------------
# (a), (b), (c) for one call
# ---------------------------------------------------------------------------

def contract(what, call, donor, ops_out):
    """``call(fill=, donor=)`` is one abi_call function on fixed inputs; ``ops_out``: name -> what ``ops`` returned."""
    zero = call(fill="zero")
    A.assert_same_bits(f"{what}: zeroed workspace against ops", {k: zero[k] for k in ops_out}, ops_out)
    for fill in ("ones", "stale"):
        got = call(fill=fill, donor=donor if fill == "stale" else None)
        A.assert_same_bits(f"{what}: {fill!r} workspace against a zeroed one", got, zero)
    return zero


def other_reward(reward):
    """The donor's rewards: every instance's reversed and halved (inside the range the case's
    references are guarded for), a NaN in the last instance."""
    r = np.array(reward, dtype=np.float64)[:, ::-1] * 0.5
    r[-1, r.shape[1] // 2] = np.nan
    return np.ascontiguousarray(r)


def other_p0(p0):
    return np.ascontiguousarray(np.roll(np.array(p0, dtype=np.float64), 1, axis=1))


def uniform_policy(shape):
    return np.full(shape, 1.0 / shape[-1])


def stationary(case, mdp, label, plans, caps, discount, passes=("backward", "forward", "soft", "vi")):
    """The four stationary passes of an elementwise_cases.Case, each ``ops`` result judged by elementwise_run."""
    from irlmx import ops
    tm = ops.terminal_mask(case.terminal, case.S, batch=case.B, device=mdp.device)
    reward = np.array(case.reward)
    if "backward" in passes:
        pi = E.run_backward(case, mdp, label, plans["backward"], tag=TAG)
        contract(f"{label} backward", lambda **kw: A.backward_maxent(mdp, reward, tm, **kw),
                 {"reward": other_reward(reward)}, {"p_action": pi})
    if "forward" in passes:
        policy = np.stack([case.backward(b)[0] for b in range(case.B)])
        for cap in caps:
            svf, k, st = E.run_forward(case, mdp, label, plans["forward"], cap, tag=TAG)
            assert cap != 7 or C.MAXITER in st, (label, cap, st)                # the cap of 7 does stop instances
            contract(f"{label} forward cap {cap}",
                     lambda **kw: A.forward_svf(mdp, np.array(case.p0), tm, policy, max_iter=cap, **kw),
                     {"p_initial": other_p0(case.p0), "max_iter": 7}, {"svf": svf, "iterations": k, "status": st})
    if "soft" in passes:
        phi = np.tile(case.phi, (case.B, 1))
        pi, v, k, st = E.run_soft(case, mdp, label, plans["soft_backward"], discount, tag=TAG)
        contract(f"{label} soft VI", lambda **kw: A.soft_backward(mdp, reward, phi, discount, **kw),
                 {"reward": other_reward(reward), "max_iter": 7},
                 {"p_action": pi, "value": v, "iterations": k, "status": st})
    if "vi" in passes:
        for average, (v, k, st) in E.run_vi(case, mdp, label, plans["value_iteration"], discount, tag=TAG).items():
            contract(f"{label} VI average={average}",
                     lambda **kw: A.value_iteration(mdp, reward, discount, average=average, **kw),
                     {"reward": other_reward(reward), "max_iter": 7}, {"value": v, "iterations": k, "status": st})


def shapes(mdp, shape, ops_=("backward", "forward", "soft_backward", "value_iteration")):
    return {op: E.expect_plan(mdp, op, shape=shape) for op in ops_}


def extended(label, mdp, reward, tm, pi_ops):
    """irlmx_backward_maxent_extended against ``ops.backward_maxent_extended``'s (judged) result."""
    contract(f"{label} extended backward", lambda **kw: A.backward_maxent_extended(mdp, reward, tm, **kw),
             {"reward": other_reward(reward)}, {"p_action": pi_ops})


def policy_eval(name, dev, shape, discount=0.7):
    """Policy evaluation of policy_eval_twin's case on its Dirichlet policy, judged as
    test_gpu_policy_eval.test_accuracy_against_longdouble judges it."""
    from irlmx import ops
    c, r, pi = PT.base(name), PT.reward(name), PT.policy(name, "dirichlet")
    mdp = model(name, PT.device_model(name, dev))
    assert ops.execution_plan(mdp, "policy_evaluation")["shape"] == shape, name
    v, k, st = ops.policy_evaluation(mdp, np.array(r), np.array(pi), discount, None, PT.EPS)
    for b in range(c.B):
        tv, tk, tst, deltas, ref, e_oracle = PT.reference(name, b, "dirichlet", discount, None)
        e, allowed = X.normwise_err(v[b].cpu().numpy(), ref), X.bound(e_oracle, c.k_row, c.A)
        print(f"[{TAG}] policy evaluation {name}[{b}] {shape} sweeps {int(k[b])} e_kernel {e:.3e} allowed {allowed:.3e}")
        assert (int(k[b]), int(st[b])) == (tk, tst) and e <= allowed, (name, b, int(k[b]), tk, e, allowed)
    contract(f"{name}/{shape} policy evaluation",
             lambda **kw: A.policy_evaluation(mdp, np.array(r), np.array(pi), discount, None, PT.EPS, **kw),
             {"reward": other_reward(r), "p_action": uniform_policy(pi.shape), "max_iter": 7},
             {"value": v, "iterations": k, "status": st})


def horizon(name, dev, shape_b, shape_f):
    """Both finite-horizon passes of horizon_twin's case, judged as test_gpu_horizon.test_accuracy
    judges them; each with its optional output given and NULL."""
    from irlmx import ops
    c = H.case(name)
    mdp = model(name, c.device_model(dev))
    assert ops.execution_plan(mdp, "backward_horizon")["shape"] == shape_b, name
    assert ops.execution_plan(mdp, "forward_horizon")["shape"] == shape_f, name
    tm = ops.terminal_mask(c.terminal, c.S, batch=mdp.batch, device=dev) if c.terminal else None
    reward, p0 = np.array(c.reward), np.array(c.p0)
    pi, lz = ops.backward_maxent_horizon(mdp, reward, c.T, tm, return_log_z0=True)
    svf, _, fst, marg = ops.forward_svf_horizon(mdp, p0, pi, tm, return_marginals=True)
    pi_h, lz_h, svf_h, marg_h = (x.cpu().numpy() for x in (pi, lz, svf, marg))
    for b in range(c.B):
        (rpi, rlz), (e_twin_pi, e_twin_lz) = c.ref_backward(b), c.e_twin_backward(b)
        assert X.elementwise_err(pi_h[b], rpi) <= c.bound_pi(e_twin_pi), (name, b)
        assert X.normwise_err(lz_h[b], rlz) <= c.bound_pi(e_twin_lz), (name, b)
        tD, tmarg, tstatus = H.forward(c.model(b), c.p0[b], c.terminal, pi_h[b])      # fed the device's own pi_t
        rD, rmarg = H.forward_ref(c.model(b).mats, c.p0[b], c.terminal, pi_h[b])
        e_svf, e_marg = X.elementwise_err(svf_h[b], rD), X.elementwise_err(marg_h[b], rmarg)
        assert e_svf <= c.bound_svf(X.elementwise_err(tD, rD)), (name, b, e_svf)
        assert e_marg <= c.bound_svf(X.elementwise_err(tmarg, rmarg)), (name, b, e_marg)
        assert int(fst[b]) == tstatus == H.OK
    label = f"{name} horizon"
    contract(f"{label} backward {shape_b}", lambda **kw: A.backward_maxent_horizon(mdp, reward, c.T, tm, **kw),
             {"reward": other_reward(reward)}, {"p_action_t": pi, "log_z0": lz})
    bare = contract(f"{label} backward {shape_b}, log_z0 NULL",
                    lambda **kw: A.backward_maxent_horizon(mdp, reward, c.T, tm, log_z0=False, **kw),
                    {"reward": other_reward(reward)}, {"p_action_t": pi})
    assert bare["log_z0"] is None
    donor = {"p_initial": other_p0(p0), "p_action_t": uniform_policy(tuple(pi.shape))}
    contract(f"{label} forward {shape_f}", lambda **kw: A.forward_svf_horizon(mdp, p0, pi, tm, **kw), donor,
             {"svf": svf, "svf_t": marg, "status": fst})
    bare = contract(f"{label} forward {shape_f}, svf_t NULL",
                    lambda **kw: A.forward_svf_horizon(mdp, p0, pi, tm, svf_t=False, **kw), donor,
                    {"svf": svf, "status": fst})
    assert bare["svf_t"] is None


# ---------------------------------------------------------------------------
# stencil, fused and per sweep: every entry point on 16 x 16 x 3
# ---------------------------------------------------------------------------

def stencil_mdp(case, dev):
    import test_gpu_elementwise as GE
    return GE.stencil_mdp(case, dev)


@pytest.mark.parametrize("family", ["stationary", "extended", "policy-evaluation", "horizon"])
@pytest.mark.parametrize("shape", ["fused", "sweep"])
def test_stencil_16x16(dev, env, shape, family):
    """C.stencil(16, 16), three instances, one workgroup per instance and one
    launch per sweep: the four stationary passes (forward at caps 7 and 3000),
    the extended backward (in range: the ordinary pass's bits), policy
    evaluation ("16x16" of policy_eval_twin) and both horizon passes ("16x16",
    T = 40, and "16x16-T1", whose svf_t has two rows)."""
    from irlmx import ops
    env(DEFAULT if shape == "fused" else SWEEP)
    case = C.stencil(16, 16)
    if family == "stationary":
        mdp = model("16x16", stencil_mdp(case, dev))
        stationary(case, mdp, f"stencil16x16/{shape}", shapes(mdp, shape), (7, 3000), 0.7)
    elif family == "extended":
        mdp = model("16x16", stencil_mdp(case, dev))
        assert ops.execution_plan(mdp, "backward", extended_range=True)["shape"] == shape
        tm = ops.terminal_mask(case.terminal, case.S, batch=case.B, device=dev)
        ordinary = E.run_backward(case, mdp, f"stencil16x16/{shape}", E.expect_plan(mdp, "backward", shape=shape), tag=TAG)
        pi = ops.backward_maxent_extended(mdp, np.array(case.reward), tm)
        A.assert_same_bits("extended backward in range against the ordinary pass", {"p_action": pi}, {"p_action": ordinary})
        extended(f"stencil16x16/{shape}", mdp, np.array(case.reward), tm, pi)
    elif family == "policy-evaluation":
        policy_eval("16x16", dev, shape)
    else:
        horizon("16x16", dev, shape, shape)
        horizon("16x16-T1", dev, shape, shape)


# ---------------------------------------------------------------------------
# cluster
# ---------------------------------------------------------------------------

#: (name, planner keys, backward layout, forward layout or None: backward only) -- rows of
#: test_gpu_elementwise.CLUSTER_CASES
CLUSTER = [("64x20", CLUSTER_64x20, 0, 0),
           ("256x12", {"IRLMX_FUSED_MAX_STATES": 0, "IRLMX_CLUSTER_R": 5, "IRLMX_CLUSTER_G": 3, "IRLMX_PAIR": 4}, 4, None),
           ("37x23", {"IRLMX_FUSED_MAX_STATES": 0, "IRLMX_CLUSTER_R": 5, "IRLMX_CLUSTER_G": 3}, 0, 0)]


@pytest.mark.parametrize("name,keys,lay_b,lay_f", CLUSTER, ids=[c[0] for c in CLUSTER])
def test_cluster(dev, env, name, keys, lay_b, lay_f):
    """The persistent tiled kernels on R = 5 owned and G = 3 ghost rows, three
    instances per launch: 64 x 20 (backward and forward), 256 x 12 on the
    compact-weight layout 4 (backward), 37 x 23 with its partial last tile
    (backward and forward)."""
    W, Hh = MODELS[name][0][3:5]
    case = C.stencil(W, Hh)
    mdp = model(name, stencil_mdp(case, dev))
    env(keys)
    tiles = (Hh + 4) // 5
    plans = {"backward": E.expect_plan(mdp, "backward", shape="cluster", R=5, G=3, C=tiles, per_launch=3, layout=lay_b)}
    passes = ("backward",)
    if lay_f is not None:
        plans["forward"] = E.expect_plan(mdp, "forward", shape="cluster", R=5, G=3, C=tiles, per_launch=3, layout=lay_f)
        passes = ("backward", "forward")
    stationary(case, mdp, f"stencil{name}/cluster", plans, (7, 3000), None, passes)


# ---------------------------------------------------------------------------
# grid
# ---------------------------------------------------------------------------

def ell_plans(c, mdp, fused_max):
    return {op: E.expect_plan(mdp, op, **L.expected_plan(c, op, fused_max)) for op in L.OPS}


def test_ell_grid(dev, env):
    """k8-s1029, the smallest case test_gpu_ell_matrix forces onto the persistent
    grid shape for all four passes (five workgroups per instance, the last one
    holding 5 states)."""
    c = L.case("k8-s1029")
    mdp = model("k8-s1029", L.device_model(c, dev))
    env(NO_FUSED)
    plans = ell_plans(c, mdp, 0)
    assert all(L.expected_plan(c, op, 0)["shape"] == "grid" for op in L.OPS)
    stationary(c, mdp, "k8-s1029/grid", plans, L.CAPS, L.DISCOUNT)


def test_stencil_bellman_grid(dev, env):
    """Soft VI and VI of 37 x 23 x 3 on the persistent grid shape: four workgroups per instance, the last partial."""
    case = C.stencil(37, 23)
    mdp = model("37x23", stencil_mdp(case, dev))
    env(BELLMAN_GRID)
    plans = {op: E.expect_plan(mdp, op, shape="grid", C=4, per_launch=3) for op in ("soft_backward", "value_iteration")}
    stationary(case, mdp, "stencil37x23/grid", plans, (), 0.7, ("soft", "vi"))


# ---------------------------------------------------------------------------
# ELL, fused
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["stationary", "policy-evaluation", "horizon"])
@pytest.mark.parametrize("name", ["k8-s1029", "k32-s200"])
def test_ell_fused(dev, env, name, family):
    """k8-s1029 (two states per thread; soft VI has no such pair and runs per
    sweep) and k32-s200 (the 32-slot class, A = 8) on the default plan; the
    horizon passes of k8-s1029 with IRLMX_HORIZON_FUSED_BATCH=1, as
    test_gpu_horizon forces several states per thread below the batch threshold."""
    c = L.case(name)
    if family == "stationary":
        env(DEFAULT)
        mdp = model(name, L.device_model(c, dev))
        plans = ell_plans(c, mdp, L.FUSED_MAX_STATES)
        assert [L.expected_plan(c, op)["shape"] for op in L.OPS] == ["fused", "fused", "sweep", "fused"]
        stationary(c, mdp, f"{name}/default", plans, L.CAPS, L.DISCOUNT)
    elif family == "policy-evaluation":
        env(DEFAULT)
        assert PT.FUSED[name] is not None
        policy_eval(name, dev, "fused")
    else:
        env({"IRLMX_HORIZON_FUSED_BATCH": 1} if name == "k8-s1029" else DEFAULT)
        horizon(name, dev, "fused", "fused")


@pytest.mark.parametrize("family", ["policy-evaluation", "horizon"])
def test_per_sweep_by_slot_count(dev, env, family):
    """k40-s300: 40 slots have no fused form, so policy evaluation and the
    horizon passes run per sweep on the default plan (16 x 16 forced per sweep
    is in test_stencil_16x16)."""
    env(DEFAULT)
    if family == "policy-evaluation":
        policy_eval("k40-s300", dev, "sweep")
    else:
        horizon("k40-s300", dev, "sweep", "sweep")


# ---------------------------------------------------------------------------
# finite-horizon soft value iteration, fused and per sweep
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["fused", "sweep"])
@pytest.mark.parametrize("name,discount", [("16x16", 1.0), ("37x23", 0.9), ("k8-s1029", 0.9)])
def test_soft_backward_horizon_contract(dev, env, name, discount, shape):
    """irlmx_soft_backward_horizon on both shapes, with value0 given and NULL:
    ``ops.soft_backward_horizon``'s bits whatever the workspace held -- the
    donor's rewards hold a NaN -- and no output entry keeps its sentinel, the
    NONFINITE instance's included."""
    from irlmx import _lib, ops
    env(NO_FUSED if shape == "sweep" else {"IRLMX_HORIZON_FUSED_BATCH": 1})    # several states per thread fused at any batch
    c = H.case(name)
    mdp = c.device_model(dev)
    plan = ops.execution_plan(mdp, "soft_backward_horizon")
    assert plan["shape"] == shape, plan
    need = int(_lib.load().irlmx_workspace_bytes(mdp.struct(), _lib.OP_SOFT_BACKWARD_HORIZON))
    assert need == (0 if shape == "fused" else 2 * (-(-c.B * c.S * 8 // 256) * 256)), need   # each buffer 256-aligned
    tm = ops.terminal_mask(c.terminal, c.S, batch=c.B, device=dev) if c.terminal else None
    reward = np.array(c.reward)
    pi, v0 = ops.soft_backward_horizon(mdp, reward, discount, c.T, tm, return_value0=True)
    donor = {"reward": other_reward(reward)}
    with_v0 = contract(f"{name}/{shape} soft horizon", lambda **kw: A.soft_backward_horizon(
        mdp, reward, discount, c.T, tm, **kw), donor, {"p_action_t": pi, "value0": v0})
    assert with_v0["status"].tolist() == [_lib.OK] * c.B
    without = contract(f"{name}/{shape} soft horizon, value0 NULL", lambda **kw: A.soft_backward_horizon(
        mdp, reward, discount, c.T, tm, value0=False, **kw), donor, {"p_action_t": pi})
    assert without["value0"] is None and without["status"].tolist() == [_lib.OK] * c.B
    # a NONFINITE instance: every entry written all the same, and the status computed without value0
    bad = donor["reward"]
    for value0 in (True, False):
        got = contract(f"{name}/{shape} soft horizon, NaN reward", lambda **kw: A.soft_backward_horizon(
            mdp, bad, discount, c.T, tm, value0=value0, **kw), {"reward": reward}, {})
        assert got["status"].tolist() == [_lib.OK] * (c.B - 1) + [_lib.NONFINITE], got["status"]


# ---------------------------------------------------------------------------
# dense
# ---------------------------------------------------------------------------

def dense_mdp(case, dev):
    import test_gpu_elementwise as GE
    return GE.dense_mdp(case, dev)


@pytest.mark.parametrize("plan", ["dense-grid", "dense"])
def test_dense_one_instance(dev, env, plan):
    """C.dense(1) on the persistent dense grid and, with IRLMX_DENSE_GRID=0, on the streaming kernels."""
    case = C.dense(1)
    mdp = model("dense301x1", dense_mdp(case, dev))
    env(DENSE_ENV[plan])
    stationary(case, mdp, f"dense301x1/{plan}", shapes(mdp, plan), (7, 3000), C.DENSE_DISCOUNT)


@pytest.mark.parametrize("what", ["backward", "soft", "vi"])
def test_dense_gemm(dev, env, what):
    """C.dense(17) on the GEMM plan: the backward's wgt holds the GEMM product, soft VI and VI take A * B * S doubles."""
    case = C.dense(17)
    mdp = model("dense301x17", dense_mdp(case, dev))
    env(DENSE_ENV["dense-gemm"])
    plans = shapes(mdp, "dense-gemm", ("backward", "soft_backward", "value_iteration"))
    stationary(case, mdp, "dense301x17/dense-gemm", plans, (), C.DENSE_DISCOUNT, (what,))


# ---------------------------------------------------------------------------
# extended backward, wide range
# ---------------------------------------------------------------------------

def wide_launch(dev):
    import test_gpu_extended_range as G
    cases = G.launches()[0]                               # 64 x 4, three rewards in one call
    mdp = model("64x4", G.wide_mdp(cases, dev))
    reward, tm = G.wide_inputs(cases, dev)
    return G, cases, mdp, reward, tm


@pytest.mark.parametrize("shape", ["fused", "sweep", "grid"])
def test_extended_wide(dev, env, shape):
    """The 64 x 4 x 3 wide-range launch of test_gpu_extended_range fused, forced
    per sweep, and on the persistent grid shape as test_gpu_extended_grid forces
    it (one workgroup per instance); every ``ops`` result inside the twin's bound."""
    from irlmx import ops
    G, cases, mdp, reward, tm = wide_launch(dev)
    env({"fused": DEFAULT, "sweep": NO_FUSED, "grid": EXT_GRID}[shape])
    plan = ops.execution_plan(mdp, "backward", extended_range=True)
    assert plan["shape"] == shape and (shape != "grid" or (plan["C"], plan["launches"], plan["per_launch"]) == (1, 1, 3)), plan
    pi = ops.backward_maxent_extended(mdp, reward, tm)
    G.assert_within_bound(pi, cases, f"{TAG} {shape}")
    extended(f"wide64x4/{shape}", mdp, reward, tm, pi)


# ---------------------------------------------------------------------------
# the rerun after an abandoned persistent launch
# ---------------------------------------------------------------------------

def rerun(what, env, keys, call, donor, ref):
    """``call`` with a stale workspace under IRLMX_TEST_NOT_RESIDENT=1: one more rerun counted per call
    (the donor reruns too), and ``ref``'s bits."""
    from irlmx import ops
    env({**keys, "IRLMX_TEST_NOT_RESIDENT": 1})
    before = ops.counters()
    got = call(fill="stale", donor=donor)
    after = ops.counters()
    assert after["rerun_not_resident"] - before["rerun_not_resident"] == 2, (what, before, after)
    A.assert_same_bits(f"{what}: rerun on a stale workspace", {k: got[k] for k in ref}, ref)


@pytest.mark.parametrize("shape", ["cluster", "grid", "dense-grid", "extended-grid"])
def test_rerun_on_a_dirtied_workspace(dev, env, shape):
    """IRLMX_TEST_NOT_RESIDENT=1: the persistent launch leaves at its rendezvous
    and the call reruns per sweep on the workspace it was given -- stale from a
    donor that went the same way.  The bits of the undisturbed call (dense: of
    the streaming kernels, which are the rerun's)."""
    from irlmx import ops
    if shape == "cluster":
        case = C.stencil(64, 20)
        mdp = model("64x20", stencil_mdp(case, dev))
        env(CLUSTER_64x20)
        tm = ops.terminal_mask(case.terminal, case.S, batch=case.B, device=dev)
        reward = np.array(case.reward)
        pi = E.run_backward(case, mdp, "stencil64x20/cluster", E.expect_plan(mdp, "backward", shape="cluster"), tag=TAG)
        rerun("cluster backward", env, CLUSTER_64x20, lambda **kw: A.backward_maxent(mdp, reward, tm, **kw),
              {"reward": other_reward(reward)}, {"p_action": pi})
        env(CLUSTER_64x20)
        policy = np.stack([case.backward(b)[0] for b in range(case.B)])
        svf, k, st = E.run_forward(case, mdp, "stencil64x20/cluster", E.expect_plan(mdp, "forward", shape="cluster"), 7, tag=TAG)
        rerun("cluster forward", env, CLUSTER_64x20,
              lambda **kw: A.forward_svf(mdp, np.array(case.p0), tm, policy, max_iter=7, **kw),
              {"p_initial": other_p0(case.p0), "max_iter": 7}, {"svf": svf, "iterations": k, "status": st})
    elif shape == "grid":
        c = L.case("k8-s1029")
        mdp = model("k8-s1029", L.device_model(c, dev))
        env(NO_FUSED)
        reward, phi = np.array(c.reward), np.tile(c.phi, (c.B, 1))
        pi, v, k, st = E.run_soft(c, mdp, "k8-s1029/grid", E.expect_plan(mdp, "soft_backward", shape="grid"), L.DISCOUNT,
                                  tag=TAG)
        rerun("grid soft VI", env, NO_FUSED, lambda **kw: A.soft_backward(mdp, reward, phi, L.DISCOUNT, **kw),
              {"reward": other_reward(reward), "max_iter": 7}, {"p_action": pi, "value": v, "iterations": k, "status": st})
    elif shape == "dense-grid":
        case = C.dense(1)
        mdp = model("dense301x1", dense_mdp(case, dev))
        tm = ops.terminal_mask(case.terminal, case.S, batch=case.B, device=dev)
        reward = np.array(case.reward)
        env(DENSE_ENV["dense"])
        pi = E.run_backward(case, mdp, "dense301x1/dense", E.expect_plan(mdp, "backward", shape="dense"), tag=TAG)
        env(DENSE_ENV["dense-grid"])
        E.expect_plan(mdp, "backward", shape="dense-grid")
        rerun("dense grid backward", env, DENSE_ENV["dense-grid"], lambda **kw: A.backward_maxent(mdp, reward, tm, **kw),
              {"reward": other_reward(reward)}, {"p_action": pi})
    else:
        G, cases, mdp, reward, tm = wide_launch(dev)
        env(EXT_GRID)
        assert ops.execution_plan(mdp, "backward", extended_range=True)["shape"] == "grid"
        pi = ops.backward_maxent_extended(mdp, reward, tm)
        G.assert_within_bound(pi, cases, f"{TAG} grid")
        rerun("extended grid backward", env, EXT_GRID, lambda **kw: A.backward_maxent_extended(mdp, reward, tm, **kw),
              {"reward": other_reward(reward)}, {"p_action": pi})


# ---------------------------------------------------------------------------
# entry points without a workspace: every output entry written
# ---------------------------------------------------------------------------

def outputs_only(what, dev, outputs, invoke):
    """The sentinel check alone (no workspace: ``invoke`` gets a NULL pointer and 0 bytes and ignores both)."""
    from irlmx import _lib
    return A.contract_call(what, dev, 0, outputs, lambda ws, n: _lib.check(invoke(), what))


def test_numpy_order_outputs(dev, env):
    """The numpy-order entry points at their smallest golden cases: dense12 of
    tests/golden/generic.npz (12 states, ELL layout) for the backward, soft VI
    and VI, s5_ones of maxent_small.npz for the forward (its own p0 and policy)."""
    from conftest import load_golden
    import maxent_oracle as O
    from irlmx import DeviceMDP, _lib, ops
    lib = _lib.load()
    env(DEFAULT)
    g = load_golden("generic")
    P, r, term = g["dense12__P"], g["dense12__reward"], [int(t) for t in g["dense12__terminal"]]
    S, _, A_ = P.shape
    mdp = DeviceMDP.from_dense(P, device=dev, layout="ell")
    st = _lib.stream_ptr(dev)
    tm = ops.terminal_mask(term, S, device=dev)
    er = torch.as_tensor(np.exp(r), device=dev).reshape(1, S).contiguous()
    rr = torch.as_tensor(np.array(r), device=dev).reshape(1, S).contiguous()
    phi = torch.as_tensor(O.terminal_reward(term, S), device=dev).reshape(1, S).contiguous()
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    i64, i32 = torch.empty(1, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    out = {"p_action": f64(1, S, A_), "status": i32}
    outputs_only("irlmx_backward_maxent_numpy_order", dev, out, lambda: lib.irlmx_backward_maxent_numpy_order(
        mdp.struct(), _lib.ptr(er), _lib.ptr(tm), _lib.ptr(out["p_action"]), _lib.ptr(i32), st))
    out = {"p_action": f64(1, S, A_), "value": f64(1, S), "iterations": i64, "status": i32}
    outputs_only("irlmx_soft_backward_numpy_order", dev, out, lambda: lib.irlmx_soft_backward_numpy_order(
        mdp.struct(), _lib.ptr(rr), _lib.ptr(phi), 0.9, 1e-5, 0, _lib.ptr(out["p_action"]), _lib.ptr(out["value"]),
        _lib.ptr(i64), _lib.ptr(i32), st))
    out = {"value": f64(1, S), "iterations": i64, "status": i32}
    for average in (0, 1):
        outputs_only("irlmx_value_iteration_numpy_order", dev, out, lambda: lib.irlmx_value_iteration_numpy_order(
            mdp.struct(), _lib.ptr(rr), 0.9, 1e-3, average, 0, _lib.ptr(out["value"]), _lib.ptr(i64), _lib.ptr(i32), st))
    z = load_golden("maxent_small")
    size = int(z["s5_ones__size"])
    n = size * size
    world = DeviceMDP.from_dense(O.icy_gridworld_table(size, float(z["s5_ones__p_slip"])), device=dev, layout="stencil")
    tm = ops.terminal_mask([int(t) for t in z["s5_ones__terminal"]], n, device=dev)
    p0 = torch.as_tensor(np.array(z["s5_ones__p0"]), device=dev).reshape(1, n).contiguous()
    pi = torch.as_tensor(np.array(z["s5_ones__pi"]), device=dev).reshape(1, n, 4).contiguous()
    out = {"svf": f64(1, n), "iterations": i64, "status": i32}
    outputs_only("irlmx_forward_svf_numpy_order", dev, out, lambda: lib.irlmx_forward_svf_numpy_order(
        world.struct(), _lib.ptr(p0), _lib.ptr(tm), _lib.ptr(pi), 1e-5, 0, _lib.ptr(out["svf"]), _lib.ptr(i64),
        _lib.ptr(i32), st))
    assert int(i64[0]) == int(z["s5_ones__k_f"])


def test_rollout_and_demonstration_outputs(dev, env):
    """irlmx_rollout, irlmx_demo_statistics and irlmx_demo_log_likelihood on
    test_gpu_rollout's 5 x 5 model: visits, starts, lengths, the status codes,
    ll_traj and ll are written in full.  ``states`` and ``actions`` past a
    trajectory's end are left unspecified by the header: nothing is asserted
    about them (they are prefilled with -1, as ops.rollout does)."""
    import test_gpu_rollout as R
    from irlmx import _lib, ops
    lib = _lib.load()
    env(DEFAULT)
    c, _, _ = R.host("5x5")
    mdp = R.device_model("5x5", dev)
    B, S, A_, N, max_len = mdp.batch, mdp.n_states, mdp.n_actions, R.N, 40
    st = _lib.stream_ptr(dev)
    pi = torch.as_tensor(np.array(R.policy("5x5", "dirichlet")), device=dev).contiguous()
    tm = ops.terminal_mask(list(c.terminal), S, batch=B, device=dev)
    start = torch.as_tensor(np.array(R.starts("5x5")), device=dev).to(torch.int32).contiguous()
    seeds = ops.rollout_seeds(R.SEED, B, dev)
    states = torch.full((B, N, max_len + 1), -1, dtype=torch.int32, device=dev)
    actions = torch.full((B, N, max_len), -1, dtype=torch.int32, device=dev)
    i64 = lambda: torch.empty((B, S), dtype=torch.int64, device=dev)
    i32 = lambda: torch.empty((B, N), dtype=torch.int32, device=dev)
    out = {"visits": i64(), "starts": i64(), "lengths": i32(), "traj_status": i32()}
    for traj in (True, False):
        outputs_only("irlmx_rollout", dev, out, lambda: lib.irlmx_rollout(
            mdp.struct(), _lib.ptr(pi), _lib.ptr(tm), _lib.ptr(start), _lib.ptr(seeds), N, max_len,
            _lib.ptr(out["visits"]), _lib.ptr(out["starts"]), _lib.ptr(out["lengths"]), _lib.ptr(out["traj_status"]),
            _lib.ptr(states if traj else None), _lib.ptr(actions if traj else None), st))
    lengths = out["lengths"].clone()
    stats = {"visits": i64(), "starts": i64(), "traj_status": i32()}
    outputs_only("irlmx_demo_statistics", dev, stats, lambda: lib.irlmx_demo_statistics(
        S, B, N, max_len + 1, _lib.ptr(states), _lib.ptr(lengths), _lib.ptr(stats["visits"]), _lib.ptr(stats["starts"]),
        _lib.ptr(stats["traj_status"]), st))
    A.assert_same_bits("demo statistics against the rollout", {k: stats[k] for k in ("visits", "starts")}, out)
    ll = {"ll_traj": torch.empty((B, N), dtype=torch.float64, device=dev),
          "ll": torch.empty(B, dtype=torch.float64, device=dev), "traj_status": i32()}
    outputs_only("irlmx_demo_log_likelihood", dev, ll, lambda: lib.irlmx_demo_log_likelihood(
        S, A_, B, N, max_len + 1, _lib.ptr(pi), _lib.ptr(states), _lib.ptr(actions), _lib.ptr(lengths),
        _lib.ptr(ll["ll_traj"]), _lib.ptr(ll["ll"]), _lib.ptr(ll["traj_status"]), st))
