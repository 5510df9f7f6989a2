"""Stream order and asynchrony of every entry point of include/irlmx.h that takes
a ``stream`` (needs an MI355X).

Every other numerical test runs on torch's current stream, the legacy default
stream, where everything serialises: a helper kernel, memset or copy that the
library issued on stream 0 instead of ``stream``, a host read without a
synchronise of ``stream`` before it, or a stray synchronise or allocation in a
path documented as asynchronous all give the right bits there.  Here each call
runs three times (tests/abi_call.py, ``stream_call``):

(r) on the default stream with the device idle -- the result an existing test
    already judges against the extended reference, a twin or a fixture (the
    row's ``judged`` names it; nothing is derived again here);
(s) on a non-blocking side stream, no delay;
(d) on that stream behind a ``torch.cuda._sleep`` of max(50 ms, 10 x the host
    time of (s)'s call), at most 1 s, with every array input landing late:
    the input buffers hold a donor's legal but different values until, in
    stream order after the delay, the real ones are copied over them, the
    workspace is filled with 0xFF and the outputs with their sentinels; right
    after the call the donor's values are copied back.

(s) and (d) must equal (r) bit for bit -- outputs, sweep counts, status -- and in
(d) a row whose claim is "async" (CLAIMS, taken from the header) must have
returned while the delay was still running.  A piece of the library that ran on
another stream runs during the delay: it reads the donor's inputs, or its
memset is overwritten by the fill, or its output by the sentinel.

No row invents inputs: the builders are those of test_gpu_call_contract and of
the suites it takes its cases from.  tests/test_call_contract_host.py holds
ENTRY_POINTS equal to the header's functions with a ``void* stream`` parameter.
The last tests show, on stand-in "entry points" written in torch, that the
three checks can fail.

Each (d) run prints one ``[stream-order]`` line; with IRLMX_STREAM_ORDER_LOG
set the lines are appended to that file (profiles/stream_order.txt is one run).
"""

import collections
import ctypes
import functools
import os

import numpy as np
import pytest

import abi_call as A
import elementwise_cases as C
import elementwise_run as E
import ell_cases as L
import horizon_twin as H
import maxent_oracle as O
import policy_eval_twin as PT
import test_gpu_call_contract as CC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TAG = "stream-order"
ASYNC, SYNC = "async", "may synchronise"

#: (entry point, shape) -> whether the call may synchronise ``stream``, in the words of include/irlmx.h
#: (its call-contract block lists the same rows).  "-": the entry point has one shape.
CLAIMS = {
    # one workgroup per instance: every pass is one launch
    **{(e, "fused"): ASYNC for e in (
        "irlmx_backward_maxent", "irlmx_forward_svf", "irlmx_soft_backward", "irlmx_value_iteration",
        "irlmx_backward_maxent_extended", "irlmx_policy_evaluation", "irlmx_backward_maxent_horizon",
        "irlmx_forward_svf_horizon", "irlmx_soft_backward_horizon")},
    # a fixed sweep count, one launch per sweep: nothing is read on the host
    ("irlmx_backward_maxent", "sweep"): ASYNC,
    ("irlmx_backward_maxent", "dense"): ASYNC,
    ("irlmx_backward_maxent", "dense-gemm"): ASYNC,
    ("irlmx_backward_maxent_extended", "sweep"): ASYNC,
    ("irlmx_backward_maxent_horizon", "sweep"): ASYNC,
    ("irlmx_forward_svf_horizon", "sweep"): ASYNC,
    ("irlmx_soft_backward_horizon", "sweep"): ASYNC,
    # a data-dependent sweep count, one launch per sweep: the host polls the done counter
    **{(e, s): SYNC for e in ("irlmx_forward_svf", "irlmx_soft_backward", "irlmx_value_iteration")
       for s in ("sweep", "dense")},
    ("irlmx_soft_backward", "dense-gemm"): SYNC,
    ("irlmx_value_iteration", "dense-gemm"): SYNC,
    ("irlmx_policy_evaluation", "sweep"): SYNC,
    # persistent launches: the outcome of each launch is read on the host
    **{(e, s): SYNC for e in ("irlmx_backward_maxent", "irlmx_forward_svf", "irlmx_soft_backward",
                              "irlmx_value_iteration") for s in ("grid", "dense-grid")},
    ("irlmx_backward_maxent", "cluster"): SYNC,
    ("irlmx_forward_svf", "cluster"): SYNC,
    ("irlmx_backward_maxent_extended", "grid"): SYNC,
    # one shape each
    ("irlmx_rollout", "-"): ASYNC,
    ("irlmx_demo_statistics", "-"): ASYNC,
    ("irlmx_demo_log_likelihood", "-"): ASYNC,
    ("irlmx_numpy_math", "-"): ASYNC,
    **{(e, "props known"): ASYNC for e in (
        "irlmx_backward_maxent_numpy_order", "irlmx_forward_svf_numpy_order", "irlmx_soft_backward_numpy_order",
        "irlmx_value_iteration_numpy_order")},
    ("irlmx_optimal_policy", "-"): ASYNC,
    ("irlmx_stochastic_policy", "-"): ASYNC,
    ("irlmx_build_icy_gridworld", "-"): ASYNC,
    ("irlmx_build_gridworld", "-"): ASYNC,
    ("irlmx_dense_to_stencil", "-"): ASYNC,
    ("irlmx_dense_to_rows", "-"): ASYNC,
    ("irlmx_dense_ell_sizes", "-"): ASYNC,
    ("irlmx_dense_to_ell", "-"): ASYNC,
    ("irlmx_dense_gemm", "-"): ASYNC,
    ("irlmx_mdp_properties", "-"): SYNC,
}

Row = collections.namedtuple("Row", "id entry shape keys judged build")
ROWS = []


def row(id_, entry, shape, keys, judged):
    """Decorator: ``build(dev)`` -> ``run(side)`` of one row.  ``build`` makes the model, asserts the plan and
    puts every input on the device; ``run(None)`` is (r), ``run(A.Side(...))`` (s) and (d)."""
    assert (entry, shape) in CLAIMS, (entry, shape)

    def add(build):
        ROWS.append(Row(id_, entry, shape, keys, judged, build))
        return build
    return add


# ---------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------

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
        for k in CC.KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in values.items():
            assert k in CC.KEYS, k
            monkeypatch.setenv(k, str(v))
    set_env({})
    yield set_env
    set_env({})


@pytest.fixture(scope="module")
def streams(dev):
    """The two side streams of this module (with the default stream: three in the process)."""
    return torch.cuda.Stream(dev), torch.cuda.Stream(dev)


@pytest.fixture(scope="module")
def cycles_per_ms(dev):
    """``torch.cuda._sleep`` cycles per millisecond, from one timed sleep."""
    n = 20_000_000
    torch.cuda._sleep(1_000_000)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    t0.record()
    torch.cuda._sleep(n)
    t1.record()
    t1.synchronize()
    ms = t0.elapsed_time(t1)
    assert 1.0 < ms < 2000.0, ms
    record(f"calibration: torch.cuda._sleep({n}) took {ms:.2f} ms: {n / ms:.0f} cycles per ms")
    return n / ms


def record(line):
    print(f"\n[{TAG}] {line}", flush=True)
    path = os.environ.get("IRLMX_STREAM_ORDER_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def delay_ms_for(host_ms):
    """max(50 ms, 10 x the host time of the call on an undelayed stream), at most 1 s: ten times covers host
    jitter on a shared machine, the cap keeps the file within minutes."""
    return min(1000.0, max(50.0, 10.0 * host_ms))


def three_runs(what, run, claim, streams, cycles_per_ms):
    """(r), (s), (d) of one row; returns (r)'s outputs."""
    ref = run(None)
    plain = A.Side(streams[0])
    A.assert_same_bits(f"{what}: side stream, no delay, against the default stream", run(plain), ref)
    delay = delay_ms_for(plain.host_ms)
    late = A.Side(streams[0], cycles=int(delay * cycles_per_ms), claim=claim)
    try:
        got = run(late)
    finally:
        record(f"{what}: host {plain.host_ms:.2f} ms, delay {delay:.0f} ms, behind the delay host "
               f"{-1.0 if late.host_ms is None else late.host_ms:.2f} ms, returned_early {late.returned_early}, "
               f"claim {claim}")
    A.assert_same_bits(f"{what}: behind a delay of {delay:.0f} ms against the default stream", got, ref)
    return ref


# ---------------------------------------------------------------------------
# inputs on the device, and their donors
# ---------------------------------------------------------------------------

def dv(x, dev, dtype=None, shape=None):
    t = torch.as_tensor(np.array(x), dtype=dtype or torch.float64, device=dev)
    return (t if shape is None else t.reshape(shape)).contiguous()


def rolled(t, dim=-1):
    """A legal but different mask, distribution or phi: the same entries one state further."""
    return torch.roll(t, 1, dims=dim).contiguous()


def other_index(t, n):
    """In-range integers that differ: (x + 1) mod n, entries below 0 (unused padding) taken as 0."""
    return ((t.clamp(min=0).to(torch.int64) + 1) % n).to(t.dtype).contiguous()


@functools.lru_cache(maxsize=None)
def oracle_policy(case):
    """The float64 oracle's backward policy [B, S, A]: elementwise_run.run_forward's input (Case.backward(b)[0]),
    without the extended reference that Case.backward computes beside it."""
    if case.tables is None:
        pi = [O.backward_maxent_csr(case.mats[b], case.terminal, case.reward[b]) for b in range(case.B)]
    else:
        pi = [O.backward_maxent(case.tables[b], case.terminal, case.reward[b], rescale=True) for b in range(case.B)]
    return np.ascontiguousarray(np.stack(pi))


PASS_OP = {"backward": "backward", "forward": "forward", "soft": "soft_backward", "vi": "value_iteration",
           "vi-avg": "value_iteration"}
PASS_ENTRY = {"backward": "irlmx_backward_maxent", "forward": "irlmx_forward_svf", "soft": "irlmx_soft_backward",
              "vi": "irlmx_value_iteration", "vi-avg": "irlmx_value_iteration"}


def stationary_run(case, mdp, what, discount, cap, dev):
    """``run(side)`` of one stationary pass of an elementwise_cases.Case, as test_gpu_call_contract.stationary calls it."""
    from irlmx import ops
    B, S, A_ = case.B, case.S, case.A
    tm = ops.terminal_mask(case.terminal, S, batch=B, device=dev)
    r, dr = dv(case.reward, dev), dv(CC.other_reward(case.reward), dev)
    if what == "backward":
        return lambda side: A.backward_maxent(mdp, r, tm, donor={"reward": dr, "terminal": rolled(tm)}, side=side)
    if what == "forward":
        p0, pi = dv(case.p0, dev), dv(oracle_policy(case), dev)
        donor = {"p_initial": dv(CC.other_p0(case.p0), dev), "terminal": rolled(tm),
                 "p_action": dv(CC.uniform_policy((B, S, A_)), dev)}
        return lambda side: A.forward_svf(mdp, p0, tm, pi, max_iter=cap, donor=donor, side=side)
    if what == "soft":
        phi = dv(np.tile(case.phi, (B, 1)), dev)
        donor = {"reward": dr, "terminal_reward": rolled(phi)}
        return lambda side: A.soft_backward(mdp, r, phi, discount, donor=donor, side=side)
    average = what == "vi-avg"
    return lambda side: A.value_iteration(mdp, r, discount, average=average, donor={"reward": dr}, side=side)


def stationary_rows(name, keys, shape, passes, get, discount, caps, judged, plan=None):
    """One row per pass (the forward once per cap).  ``get(dev)`` -> (case, device model); ``plan(case, mdp, op)``
    asserts the plan (default: its shape)."""
    for what in passes:
        for cap in (caps if what == "forward" else (None,)):
            sh = shape(what) if callable(shape) else shape
            rid = f"{name}/{sh}/{what}" + (f"-cap{cap}" if cap is not None else "")

            @row(rid, PASS_ENTRY[what], sh, keys, judged)
            def build(dev, what=what, cap=cap, sh=sh):
                case, mdp = get(dev)
                mdp = CC.model(name, mdp)
                if plan is None:
                    E.expect_plan(mdp, PASS_OP[what], shape=sh)
                else:
                    plan(case, mdp, PASS_OP[what])
                return stationary_run(case, mdp, what, discount, cap, dev)


ALL = ("backward", "forward", "soft", "vi", "vi-avg")

# -- 16 x 16 x 3, fused and per sweep: every entry point with a workspace ------------------------------------

for _shape, _keys in (("fused", CC.DEFAULT), ("sweep", CC.SWEEP)):
    stationary_rows("16x16", _keys, _shape, ALL, lambda dev: (C.stencil(16, 16), CC.stencil_mdp(C.stencil(16, 16), dev)),
                    0.7, (7, 3000), f"test_gpu_call_contract.test_stencil_16x16[{_shape}-stationary]")

    @row(f"16x16/{_shape}/extended", "irlmx_backward_maxent_extended", _shape, _keys,
         f"test_gpu_call_contract.test_stencil_16x16[{_shape}-extended]")
    def _extended(dev, shape=_shape):
        from irlmx import ops
        case = C.stencil(16, 16)
        mdp = CC.model("16x16", CC.stencil_mdp(case, dev))
        assert ops.execution_plan(mdp, "backward", extended_range=True)["shape"] == shape
        tm = ops.terminal_mask(case.terminal, case.S, batch=case.B, device=dev)
        r, donor = dv(case.reward, dev), {"reward": dv(CC.other_reward(case.reward), dev), "terminal": rolled(tm)}
        return lambda side: A.backward_maxent_extended(mdp, r, tm, donor=donor, side=side)

    @row(f"16x16/{_shape}/policy-evaluation", "irlmx_policy_evaluation", _shape, _keys,
         f"test_gpu_call_contract.test_stencil_16x16[{_shape}-policy-evaluation]")
    def _policy_eval(dev, shape=_shape):
        from irlmx import ops
        mdp = CC.model("16x16", PT.device_model("16x16", dev))
        assert ops.execution_plan(mdp, "policy_evaluation")["shape"] == shape
        r, pi = dv(PT.reward("16x16"), dev), dv(PT.policy("16x16", "dirichlet"), dev)
        donor = {"reward": dv(CC.other_reward(PT.reward("16x16")), dev),
                 "p_action": dv(CC.uniform_policy(tuple(pi.shape)), dev)}
        return lambda side: A.policy_evaluation(mdp, r, pi, 0.7, None, PT.EPS, donor=donor, side=side)

    @row(f"16x16/{_shape}/horizon-backward", "irlmx_backward_maxent_horizon", _shape, _keys,
         f"test_gpu_call_contract.test_stencil_16x16[{_shape}-horizon]")
    def _hz_backward(dev, shape=_shape):
        from irlmx import ops
        c = H.case("16x16")
        mdp = CC.model("16x16", c.device_model(dev))
        assert ops.execution_plan(mdp, "backward_horizon")["shape"] == shape and not c.terminal
        r, donor = dv(c.reward, dev), {"reward": dv(CC.other_reward(c.reward), dev)}
        return lambda side: A.backward_maxent_horizon(mdp, r, c.T, None, donor=donor, side=side)

    @row(f"16x16/{_shape}/horizon-forward", "irlmx_forward_svf_horizon", _shape, _keys,
         f"test_gpu_call_contract.test_stencil_16x16[{_shape}-horizon]")
    def _hz_forward(dev, shape=_shape):
        from irlmx import ops
        c = H.case("16x16")
        mdp = CC.model("16x16", c.device_model(dev))
        assert ops.execution_plan(mdp, "forward_horizon")["shape"] == shape
        pi = ops.backward_maxent_horizon(mdp, np.array(c.reward), c.T, None)      # the device's own pi_t, as there
        p0 = dv(c.p0, dev)
        donor = {"p_initial": dv(CC.other_p0(c.p0), dev), "p_action_t": dv(CC.uniform_policy(tuple(pi.shape)), dev)}
        return lambda side: A.forward_svf_horizon(mdp, p0, pi, None, donor=donor, side=side)

    @row(f"16x16/{_shape}/soft-horizon", "irlmx_soft_backward_horizon", _shape, _keys,
         f"test_gpu_call_contract.test_soft_backward_horizon_contract[16x16-1.0-{_shape}]")
    def _soft_hz(dev, shape=_shape):
        from irlmx import ops
        c = H.case("16x16")
        mdp = CC.model("16x16", c.device_model(dev))
        assert ops.execution_plan(mdp, "soft_backward_horizon")["shape"] == shape and c.T == 40
        r, donor = dv(c.reward, dev), {"reward": dv(CC.other_reward(c.reward), dev)}
        return lambda side: A.soft_backward_horizon(mdp, r, 1.0, c.T, None, donor=donor, side=side)

# -- the persistent shapes -----------------------------------------------------------------------------------

stationary_rows("64x20", CC.CLUSTER_64x20, "cluster", ("backward", "forward"),
                lambda dev: (C.stencil(64, 20), CC.stencil_mdp(C.stencil(64, 20), dev)), None, (7, 3000),
                "test_gpu_call_contract.test_cluster[64x20]")
stationary_rows("37x23", CC.BELLMAN_GRID, "grid", ("soft", "vi", "vi-avg"),
                lambda dev: (C.stencil(37, 23), CC.stencil_mdp(C.stencil(37, 23), dev)), 0.7, (),
                "test_gpu_call_contract.test_stencil_bellman_grid")
stationary_rows("k8-s1029", CC.NO_FUSED, "grid", ALL,
                lambda dev: (L.case("k8-s1029"), L.device_model(L.case("k8-s1029"), dev)), L.DISCOUNT, L.CAPS,
                "test_gpu_call_contract.test_ell_grid",
                plan=lambda c, mdp, op: E.expect_plan(mdp, op, **L.expected_plan(c, op, 0)))
# k32-s200 on the default plan: fused, but soft VI, which has no 32-slot pair and runs per sweep
stationary_rows("k32-s200", CC.DEFAULT, lambda what: "sweep" if what == "soft" else "fused", ALL,
                lambda dev: (L.case("k32-s200"), L.device_model(L.case("k32-s200"), dev)), L.DISCOUNT, L.CAPS,
                "test_gpu_call_contract.test_ell_fused[k32-s200-stationary]",
                plan=lambda c, mdp, op: E.expect_plan(mdp, op, **L.expected_plan(c, op, L.FUSED_MAX_STATES)))
for _plan in ("dense", "dense-grid"):
    stationary_rows("dense301x1", CC.DENSE_ENV[_plan], _plan, ALL, lambda dev: (C.dense(1), CC.dense_mdp(C.dense(1), dev)),
                    C.DENSE_DISCOUNT, (7, 3000), f"test_gpu_call_contract.test_dense_one_instance[{_plan}]")
stationary_rows("dense301x17", CC.DENSE_ENV["dense-gemm"], "dense-gemm", ("backward", "soft", "vi", "vi-avg"),
                lambda dev: (C.dense(17), CC.dense_mdp(C.dense(17), dev)), C.DENSE_DISCOUNT, (),
                "test_gpu_call_contract.test_dense_gemm")


@row("64x4/grid/extended", "irlmx_backward_maxent_extended", "grid", CC.EXT_GRID,
     "test_gpu_call_contract.test_extended_wide[grid]")
def _extended_grid(dev):
    from irlmx import ops
    _, _, mdp, reward, tm = CC.wide_launch(dev)
    plan = ops.execution_plan(mdp, "backward", extended_range=True)
    assert plan["shape"] == "grid" and (plan["C"], plan["launches"], plan["per_launch"]) == (1, 1, 3), plan
    r, donor = dv(reward, dev), {"reward": dv(CC.other_reward(reward), dev), "terminal": rolled(tm)}
    return lambda side: A.backward_maxent_extended(mdp, r, tm, donor=donor, side=side)


# ---------------------------------------------------------------------------
# entry points without a workspace
# ---------------------------------------------------------------------------

def free_call(name, dev, make_out, fn, real, donor, make_extra=None):
    """``run(side)`` of an entry point without a workspace: ``fn(lib, stream, out, extra, **inputs)`` returns its
    result code.  ``make_extra``: arrays the call writes only in part (a trajectory's unused tail), which ``fn``
    prefills in stream order; they are returned beside the outputs and compared, but carry no sentinel."""
    from irlmx import _lib
    lib = _lib.load()

    def run(side):
        out, extra = make_out(), (make_extra() if make_extra else {})

        def invoke(ws, n, st, **inputs):
            _lib.check(fn(lib, st, out, extra, **inputs), name)

        A.stream_call(name, dev, 0, out, invoke, real, donor, side)
        return {**out, **extra}
    return run


def empty(dev, dtype, *shape):
    return torch.empty(shape, dtype=dtype, device=dev)


F64, I64, I32 = torch.float64, torch.int64, torch.int32


def dense12(dev):
    """dense12 of tests/golden/generic.npz as an ELL model whose props are known, and its inputs on the device."""
    from conftest import load_golden
    from irlmx import DeviceMDP, ops
    g = load_golden("generic")
    P, r, term = g["dense12__P"], np.array(g["dense12__reward"]), [int(t) for t in g["dense12__terminal"]]
    S, _, A_ = P.shape
    mdp = DeviceMDP.from_dense(P, device=dev, layout="ell")
    mdp.struct()                                   # irlmx_mdp_properties: the row order is known from here on
    assert mdp._struct.props & 0x40000000
    other = CC.other_reward(r.reshape(1, S))
    tm = ops.terminal_mask(term, S, device=dev)
    phi = dv(O.terminal_reward(term, S), dev, shape=(1, S))
    return mdp, S, A_, dv(r, dev, shape=(1, S)), dv(other, dev), tm, phi


NP_JUDGED = "test_gpu_call_contract.test_numpy_order_outputs (bits: test_gpu_parity.test_generic_ell_path)"


@row("dense12/numpy-order/backward", "irlmx_backward_maxent_numpy_order", "props known", CC.DEFAULT, NP_JUDGED)
def _np_backward(dev):
    from irlmx import _lib
    mdp, S, A_, r, dr, tm, _ = dense12(dev)
    return free_call("irlmx_backward_maxent_numpy_order", dev,
                     lambda: {"p_action": empty(dev, F64, 1, S, A_), "status": empty(dev, I32, 1)},
                     lambda lib, st, out, _, exp_reward, terminal: lib.irlmx_backward_maxent_numpy_order(
                         mdp.struct(), _lib.ptr(exp_reward), _lib.ptr(terminal), _lib.ptr(out["p_action"]),
                         _lib.ptr(out["status"]), st),
                     {"exp_reward": torch.exp(r), "terminal": tm}, {"exp_reward": torch.exp(dr), "terminal": rolled(tm)})


@row("dense12/numpy-order/soft", "irlmx_soft_backward_numpy_order", "props known", CC.DEFAULT, NP_JUDGED)
def _np_soft(dev):
    from irlmx import _lib
    mdp, S, A_, r, dr, _, phi = dense12(dev)
    return free_call("irlmx_soft_backward_numpy_order", dev,
                     lambda: {"p_action": empty(dev, F64, 1, S, A_), "value": empty(dev, F64, 1, S),
                              "iterations": empty(dev, I64, 1), "status": empty(dev, I32, 1)},
                     lambda lib, st, out, _, reward, terminal_reward: lib.irlmx_soft_backward_numpy_order(
                         mdp.struct(), _lib.ptr(reward), _lib.ptr(terminal_reward), 0.9, 1e-5, 0, _lib.ptr(out["p_action"]),
                         _lib.ptr(out["value"]), _lib.ptr(out["iterations"]), _lib.ptr(out["status"]), st),
                     {"reward": r, "terminal_reward": phi}, {"reward": dr, "terminal_reward": rolled(phi)})


for _average in (0, 1):
    @row(f"dense12/numpy-order/vi-average{_average}", "irlmx_value_iteration_numpy_order", "props known", CC.DEFAULT,
         NP_JUDGED)
    def _np_vi(dev, average=_average):
        from irlmx import _lib
        mdp, S, _, r, dr, _, _ = dense12(dev)
        return free_call("irlmx_value_iteration_numpy_order", dev,
                         lambda: {"value": empty(dev, F64, 1, S), "iterations": empty(dev, I64, 1),
                                  "status": empty(dev, I32, 1)},
                         lambda lib, st, out, _, reward: lib.irlmx_value_iteration_numpy_order(
                             mdp.struct(), _lib.ptr(reward), 0.9, 1e-3, average, 0, _lib.ptr(out["value"]),
                             _lib.ptr(out["iterations"]), _lib.ptr(out["status"]), st),
                         {"reward": r}, {"reward": dr})


@row("s5_ones/numpy-order/forward", "irlmx_forward_svf_numpy_order", "props known", CC.DEFAULT,
     "test_gpu_call_contract.test_numpy_order_outputs (bits: test_gpu_parity.test_maxent_small_cases)")
def _np_forward(dev):
    from conftest import load_golden
    from irlmx import DeviceMDP, _lib, ops
    z = load_golden("maxent_small")
    size = int(z["s5_ones__size"])
    n = size * size
    world = DeviceMDP.from_dense(O.icy_gridworld_table(size, float(z["s5_ones__p_slip"])), device=dev, layout="stencil")
    world.struct()
    tm = ops.terminal_mask([int(t) for t in z["s5_ones__terminal"]], n, device=dev)
    p0, pi = dv(z["s5_ones__p0"], dev, shape=(1, n)), dv(z["s5_ones__pi"], dev, shape=(1, n, 4))
    return free_call("irlmx_forward_svf_numpy_order", dev,
                     lambda: {"svf": empty(dev, F64, 1, n), "iterations": empty(dev, I64, 1), "status": empty(dev, I32, 1)},
                     lambda lib, st, out, _, p_initial, terminal, p_action: lib.irlmx_forward_svf_numpy_order(
                         world.struct(), _lib.ptr(p_initial), _lib.ptr(terminal), _lib.ptr(p_action), 1e-5, 0,
                         _lib.ptr(out["svf"]), _lib.ptr(out["iterations"]), _lib.ptr(out["status"]), st),
                     {"p_initial": p0, "terminal": tm, "p_action": pi},
                     {"p_initial": rolled(p0), "terminal": rolled(tm), "p_action": dv(CC.uniform_policy((1, n, 4)), dev)})


# -- demonstrations: the 5 x 5 model of test_gpu_rollout, max_len 40 ---------------------------------------

MAX_LEN = 40


def rollout_inputs(dev):
    import test_gpu_rollout as R
    from irlmx import ops
    c, _, _ = R.host("5x5")
    mdp = R.device_model("5x5", dev)
    mdp.struct()
    pi = dv(R.policy("5x5", "dirichlet"), dev)
    tm = ops.terminal_mask(list(c.terminal), mdp.n_states, batch=mdp.batch, device=dev)
    start = dv(R.starts("5x5"), dev, dtype=I32)
    seeds = ops.rollout_seeds(R.SEED, mdp.batch, dev)
    return R, mdp, pi, tm, start, seeds


@row("5x5/rollout", "irlmx_rollout", "-", CC.DEFAULT,
     "test_gpu_rollout.test_matches_twin[5x5-...-dirichlet], "
     "test_gpu_call_contract.test_rollout_and_demonstration_outputs")
def _rollout(dev):
    from irlmx import _lib
    R, mdp, pi, tm, start, seeds = rollout_inputs(dev)
    B, S, A_, N = mdp.batch, mdp.n_states, mdp.n_actions, R.N

    def fn(lib, st, out, extra, p_action, terminal, start, seed):
        extra["states"].fill_(-1)                  # (in stream order, as ops.rollout prefills them)
        extra["actions"].fill_(-1)
        return lib.irlmx_rollout(mdp.struct(), _lib.ptr(p_action), _lib.ptr(terminal), _lib.ptr(start), _lib.ptr(seed), N,
                                 MAX_LEN, _lib.ptr(out["visits"]), _lib.ptr(out["starts"]), _lib.ptr(out["lengths"]),
                                 _lib.ptr(out["traj_status"]), _lib.ptr(extra["states"]), _lib.ptr(extra["actions"]), st)

    return free_call("irlmx_rollout", dev,
                     lambda: {"visits": empty(dev, I64, B, S), "starts": empty(dev, I64, B, S),
                              "lengths": empty(dev, I32, B, N), "traj_status": empty(dev, I32, B, N)},
                     fn, {"p_action": pi, "terminal": tm, "start": start, "seed": seeds},
                     {"p_action": dv(CC.uniform_policy((B, S, A_)), dev), "terminal": rolled(tm),
                      "start": other_index(start, S), "seed": seeds + 1},
                     lambda: {"states": empty(dev, I32, B, N, MAX_LEN + 1), "actions": empty(dev, I32, B, N, MAX_LEN)})


def stored(dev):
    """The trajectories ops.rollout stores for the row above, and donors: every state and action one further
    (mod S, mod A; the -1 padding as 0), every length one longer (mod max_len + 1) -- all in range."""
    from irlmx import ops
    R, mdp, pi, tm, start, _ = rollout_inputs(dev)
    got = ops.rollout(mdp, pi, tm, start, R.N, MAX_LEN, R.SEED, return_trajectories=True)
    S, A_ = mdp.n_states, mdp.n_actions
    real = {"states": got.states, "actions": got.actions, "lengths": got.lengths}
    donor = {"states": other_index(got.states, S), "actions": other_index(got.actions, A_),
             "lengths": other_index(got.lengths, MAX_LEN + 1)}
    assert int(donor["states"].min()) >= 0 and int(donor["states"].max()) < S and int(donor["actions"].max()) < A_
    assert int(donor["lengths"].min()) >= 0 and int(donor["lengths"].max()) <= MAX_LEN
    return R, mdp, pi, real, donor


@row("5x5/demo-statistics", "irlmx_demo_statistics", "-", CC.DEFAULT,
     "test_gpu_rollout.test_statistics_round_trip and test_gpu_call_contract.test_rollout_and_demonstration_outputs")
def _demo_statistics(dev):
    from irlmx import _lib
    R, mdp, _, real, donor = stored(dev)
    B, S, N = mdp.batch, mdp.n_states, R.N
    keys = ("states", "lengths")
    return free_call("irlmx_demo_statistics", dev,
                     lambda: {"visits": empty(dev, I64, B, S), "starts": empty(dev, I64, B, S),
                              "traj_status": empty(dev, I32, B, N)},
                     lambda lib, st, out, _, states, lengths: lib.irlmx_demo_statistics(
                         S, B, N, MAX_LEN + 1, _lib.ptr(states), _lib.ptr(lengths), _lib.ptr(out["visits"]),
                         _lib.ptr(out["starts"]), _lib.ptr(out["traj_status"]), st),
                     {k: real[k] for k in keys}, {k: donor[k] for k in keys})


@row("5x5/demo-log-likelihood", "irlmx_demo_log_likelihood", "-", CC.DEFAULT,
     "test_gpu_rollout.test_log_likelihood_matches_twin and test_gpu_call_contract.test_rollout_and_demonstration_outputs")
def _demo_log_likelihood(dev):
    from irlmx import _lib
    R, mdp, pi, real, donor = stored(dev)
    B, S, A_, N = mdp.batch, mdp.n_states, mdp.n_actions, R.N
    return free_call("irlmx_demo_log_likelihood", dev,
                     lambda: {"ll_traj": empty(dev, F64, B, N), "ll": empty(dev, F64, B),
                              "traj_status": empty(dev, I32, B, N)},
                     lambda lib, st, out, _, p_action, states, actions, lengths: lib.irlmx_demo_log_likelihood(
                         S, A_, B, N, MAX_LEN + 1, _lib.ptr(p_action), _lib.ptr(states), _lib.ptr(actions),
                         _lib.ptr(lengths), _lib.ptr(out["ll_traj"]), _lib.ptr(out["ll"]), _lib.ptr(out["traj_status"]), st),
                     {"p_action": pi, **real}, {"p_action": dv(CC.uniform_policy((B, S, A_)), dev), **donor})


# -- elementwise, policies, builders, converters, GEMM, properties -----------------------------------------

for _op, _key in ((0, "exp"), (1, "log")):
    @row(f"npmath/{_key}", "irlmx_numpy_math", "-", CC.DEFAULT,
         f"test_gpu_npmath.test_device_numpy_math_bit_exact[{_op}-{_key}]")
    def _numpy_math(dev, op=_op, key=_key):
        from conftest import load_golden
        from irlmx import _lib
        x = dv(np.ascontiguousarray(load_golden("npmath")["x_" + key], dtype=np.float64), dev)
        return free_call("irlmx_numpy_math", dev, lambda: {"y": torch.empty_like(x)},
                         lambda lib, st, out, _, x: lib.irlmx_numpy_math(op, _lib.ptr(x), _lib.ptr(out["y"]), x.numel(), st),
                         {"x": x}, {"x": torch.flip(x, (0,)).contiguous()})


def successors(dev):
    """The intended successors of the 5 x 5 gridworld and three value vectors (elementwise_cases.stencil(5, 5)'s rewards)."""
    succ = np.array([[O.intended_successor(5, s, a) for a in range(4)] for s in range(25)])
    return dv(succ, dev, dtype=I32), dv(C.stencil(5, 5).reward, dev)


@row("5x5/optimal-policy", "irlmx_optimal_policy", "-", CC.DEFAULT, "test_gpu_argmax (ops.optimal_policy against np.argmax)")
def _optimal_policy(dev):
    from irlmx import _lib
    succ, v = successors(dev)
    return free_call("irlmx_optimal_policy", dev, lambda: {"policy": empty(dev, I64, 3, 25)},
                     lambda lib, st, out, _, successor, value: lib.irlmx_optimal_policy(
                         _lib.ptr(successor), 25, 4, 3, _lib.ptr(value), _lib.ptr(out["policy"]), st),
                     {"successor": succ, "value": v}, {"successor": other_index(succ, 25), "value": rolled(v)})


@row("5x5/stochastic-policy", "irlmx_stochastic_policy", "-", CC.DEFAULT,
     "test_gpu_parity.test_value_iteration_cases (solver.stochastic_policy_from_value)")
def _stochastic_policy(dev):
    from irlmx import _lib
    succ, v = successors(dev)
    w = torch.exp(v)
    return free_call("irlmx_stochastic_policy", dev, lambda: {"p_policy": empty(dev, F64, 3, 25, 4)},
                     lambda lib, st, out, _, successor, weighted_value: lib.irlmx_stochastic_policy(
                         _lib.ptr(successor), 25, 4, 3, _lib.ptr(weighted_value), _lib.ptr(out["p_policy"]), st),
                     {"successor": succ, "weighted_value": w},
                     {"successor": other_index(succ, 25), "weighted_value": rolled(w)})


@row("5x5/build-icy", "irlmx_build_icy_gridworld", "-", CC.DEFAULT, "test_gpu_parity.test_world_builders_bit_exact")
def _build_icy(dev):
    from irlmx import _lib
    slip = dv([0.2, 0.1], dev)
    return free_call("irlmx_build_icy_gridworld", dev, lambda: {"row_val": empty(dev, F64, 2, 4, 5, 25)},
                     lambda lib, st, out, _, p_slip: lib.irlmx_build_icy_gridworld(5, _lib.ptr(p_slip), 2,
                                                                                   _lib.ptr(out["row_val"]), st),
                     {"p_slip": slip}, {"p_slip": dv([0.35, 0.3], dev)})


@row("5x5/build-gridworld", "irlmx_build_gridworld", "-", CC.DEFAULT, "test_gpu_parity.test_world_builders_bit_exact")
def _build_gridworld(dev):
    from irlmx import _lib
    return free_call("irlmx_build_gridworld", dev, lambda: {"row_val": empty(dev, F64, 2, 4, 5, 25)},
                     lambda lib, st, out, _: lib.irlmx_build_gridworld(5, 2, _lib.ptr(out["row_val"]), st), {}, {})


def dense_tables(which, dev):
    """(table [S, S, A] on the device, a donor with the same nonzero pattern and other values, S, A, grid)."""
    from conftest import load_golden
    if which == "icy5":
        P, D, grid = O.icy_gridworld_table(5, 0.2), O.icy_gridworld_table(5, 0.35), (5, 5)
        assert np.array_equal(P != 0, D != 0)
    else:
        P, grid = load_golden("generic")["dense12__P"], (4, 3)
        D = P * 0.5
    S, _, A_ = P.shape
    return dv(np.ascontiguousarray(P), dev), dv(np.ascontiguousarray(D), dev), S, A_, grid


CONVERT_JUDGED = "test_gpu_parity.test_dense_upload_layouts / test_dense_to_ell_device (DeviceMDP.from_dense)"

for _which in ("icy5", "dense12"):
    @row(f"{_which}/dense-to-stencil", "irlmx_dense_to_stencil", "-", CC.DEFAULT, CONVERT_JUDGED)
    def _to_stencil(dev, which=_which):
        from irlmx import _lib
        P, D, S, A_, (W, Hh) = dense_tables(which, dev)
        return free_call("irlmx_dense_to_stencil", dev,
                         lambda: {"row_val": empty(dev, F64, 1, A_, 5, S), "off_stencil": empty(dev, I32, 1)},
                         lambda lib, st, out, _, dense: lib.irlmx_dense_to_stencil(
                             _lib.ptr(dense), W, Hh, A_, _lib.ptr(out["row_val"]), _lib.ptr(out["off_stencil"]), st),
                         {"dense": P}, {"dense": D})

    @row(f"{_which}/dense-to-rows", "irlmx_dense_to_rows", "-", CC.DEFAULT, CONVERT_JUDGED)
    def _to_rows(dev, which=_which):
        from irlmx import _lib
        P, D, S, A_, _ = dense_tables(which, dev)
        return free_call("irlmx_dense_to_rows", dev,
                         lambda: {"p_rows": empty(dev, F64, 1, A_, S, S), "m_rows": empty(dev, F64, 1, S, S)},
                         lambda lib, st, out, _, dense: lib.irlmx_dense_to_rows(
                             _lib.ptr(dense), S, A_, _lib.ptr(out["p_rows"]), _lib.ptr(out["m_rows"]), st),
                         {"dense": P}, {"dense": D})

    @row(f"{_which}/dense-ell-sizes", "irlmx_dense_ell_sizes", "-", CC.DEFAULT, CONVERT_JUDGED)
    def _ell_sizes(dev, which=_which):
        from irlmx import _lib
        P, D, S, A_, _ = dense_tables(which, dev)
        return free_call("irlmx_dense_ell_sizes", dev,
                         lambda: {"k_out": empty(dev, I32, 2), "col_count": empty(dev, I32, S)},
                         lambda lib, st, out, _, dense: lib.irlmx_dense_ell_sizes(
                             _lib.ptr(dense), S, A_, _lib.ptr(out["k_out"]), _lib.ptr(out["col_count"]), st),
                         {"dense": P}, {"dense": D})

    @row(f"{_which}/dense-to-ell", "irlmx_dense_to_ell", "-", CC.DEFAULT, CONVERT_JUDGED)
    def _to_ell(dev, which=_which):
        from irlmx import DeviceMDP, _lib
        P, D, S, A_, _ = dense_tables(which, dev)
        sized = DeviceMDP.from_dense(P.cpu().numpy(), device=dev, layout="ell")     # the sizes of the real table: the
        kr, kc = sized.k_row, sized.k_col                                            # donor has the same pattern
        return free_call("irlmx_dense_to_ell", dev,
                         lambda: {"row_idx": empty(dev, I32, 1, kr, S), "row_val": empty(dev, F64, 1, A_, kr, S),
                                  "col_idx": empty(dev, I32, 1, kc, S), "col_val": empty(dev, F64, 1, A_, kc, S)},
                         lambda lib, st, out, _, dense: lib.irlmx_dense_to_ell(
                             _lib.ptr(dense), S, A_, kr, kc, _lib.ptr(out["row_idx"]), _lib.ptr(out["row_val"]),
                             _lib.ptr(out["col_idx"]), _lib.ptr(out["col_val"]), st),
                         {"dense": P}, {"dense": D})

for _rows, _n, _batch in ((300, 300, 5), (301, 301, 3)):
    @row(f"gemm/{_rows}x{_n}x{_batch}", "irlmx_dense_gemm", "-", CC.DEFAULT,
         f"test_gpu_dense.test_dense_gemm_kernel_vs_torch[{_rows}-{_n}-{_batch}-...]")
    def _gemm(dev, rows=_rows, n=_n, batch=_batch):
        from irlmx import _lib
        g = torch.Generator(device=dev).manual_seed(rows + n + batch)
        rand = lambda *shape: torch.rand(shape, dtype=F64, device=dev, generator=g)
        m, z, dm, dz = rand(rows, n), rand(batch, n), rand(rows, n), rand(batch, n)
        return free_call("irlmx_dense_gemm", dev, lambda: {"c": empty(dev, F64, batch, rows)},
                         lambda lib, st, out, _, m, z: lib.irlmx_dense_gemm(_lib.ptr(m), _lib.ptr(z), _lib.ptr(out["c"]),
                                                                            rows, n, batch, st),
                         {"m": m, "z": z}, {"m": dm, "z": dz})


def properties_run(dev, mdp, donor):
    """irlmx_mdp_properties on a struct whose table pointers are the late-landing buffers; ``props`` is host memory."""
    from irlmx import _lib
    names = [k for k in ("row_val", "row_idx", "col_idx", "col_val") if getattr(mdp, k) is not None]
    real = {k: getattr(mdp, k) for k in names}
    donor = {**real, **donor}
    donor = {k: (v.clone() if v is real[k] else v) for k, v in donor.items()}

    def fn(lib, st, out, _, **tables):
        s = _lib.MDPStruct()
        s.layout, s.n_states, s.n_actions, s.width, s.height = mdp.layout, mdp.n_states, mdp.n_actions, mdp.width, mdp.height
        stencil = mdp.layout == _lib.LAYOUT_STENCIL5
        s.k_row, s.k_col = (5, 5) if stencil else (mdp.k_row, mdp.k_col)
        s.batch, s.shared = mdp.batch, int(mdp.shared)
        for k, t in tables.items():
            setattr(s, k, t.data_ptr())
        props = ctypes.c_int32(0)
        rc = lib.irlmx_mdp_properties(ctypes.byref(s), ctypes.byref(props), st)
        out["props"][0] = props.value
        return rc

    return free_call("irlmx_mdp_properties", dev, lambda: {"props": torch.empty(1, dtype=I32)}, fn, real, donor)


@row("256x12/properties", "irlmx_mdp_properties", "-", CC.DEFAULT,
     "test_gpu_call_contract.test_cluster[256x12] (the compact layout is planned from these props)")
def _props_stencil(dev):
    case = C.stencil(256, 12)
    mdp = CC.model("256x12", CC.stencil_mdp(case, dev))
    scale = torch.arange(1, 6, dtype=F64, device=dev).reshape(1, 1, 5, 1)      # +x and -x coefficients differ: not compact
    run = properties_run(dev, mdp, {"row_val": (mdp.row_val * scale).contiguous()})
    return run


@row("k32-s200/properties", "irlmx_mdp_properties", "-", CC.DEFAULT,
     "test_gpu_ell_matrix (sorted and scrambled forms: the numpy-order calls accept or refuse by these props)")
def _props_ell(dev):
    mdp = CC.model("k32-s200", L.device_model(L.case("k32-s200"), dev))
    donor = {"row_val": torch.flip(mdp.row_val, (2,)).contiguous(), "row_idx": torch.flip(mdp.row_idx, (1,)).contiguous()}
    return properties_run(dev, mdp, donor)                                      # descending rows: not sorted


ROW = {r.id: r for r in ROWS}
assert len(ROW) == len(ROWS)
#: every entry point the rows run: tests/test_call_contract_host.py holds it equal to the header's set
ENTRY_POINTS = sorted({r.entry for r in ROWS})


# ---------------------------------------------------------------------------
# sections 2 and 3: (r), (s), (d) of every row
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("rid", [r.id for r in ROWS])
def test_stream_order(dev, env, streams, cycles_per_ms, rid):
    r = ROW[rid]
    env(r.keys)
    run = r.build(dev)
    three_runs(f"{r.id} {r.entry}", run, CLAIMS[(r.entry, r.shape)], streams, cycles_per_ms)


def test_properties_tell_the_donor_apart(dev, env):
    """The donors of the two irlmx_mdp_properties rows do have other properties than the real tables, so a
    check that ran early would have changed ``props``."""
    from irlmx import _lib
    env(CC.DEFAULT)
    for rid, bit in (("256x12/properties", _lib.PROP_COMPACT), ("k32-s200/properties", _lib.PROP_ELL_SORTED)):
        got = int(ROW[rid].build(dev)(None)["props"][0])
        assert got & _lib.PROPS_KNOWN and got & bit, (rid, hex(got))


# ---------------------------------------------------------------------------
# section 4: two calls in flight
# ---------------------------------------------------------------------------

#: (first, second): the first is an "async" row, enqueued behind its delay on one stream; the second goes behind
#: an equal delay on the other stream and may synchronise.  Shapes and the process-wide salts are mixed.
PAIRS = [
    ("16x16/fused/forward-cap3000", "k8-s1029/grid/soft"),
    ("16x16/fused/policy-evaluation", "64x20/cluster/backward"),
    ("16x16/sweep/horizon-backward", "64x4/grid/extended"),
    ("dense301x17/dense-gemm/backward", "5x5/rollout"),
    ("16x16/fused/backward", "16x16/fused/backward"),
]
PAIR_DELAY_MS = 300.0


@pytest.mark.parametrize("first,second", PAIRS, ids=[f"{a}+{b}" for a, b in PAIRS])
def test_two_calls_in_flight(dev, env, streams, cycles_per_ms, first, second):
    """Each call has its own arena and late-landing inputs; each result equals its solo (r) bits.  The counters
    are not asserted: a persistent launch that loses the co-residency rendezvous reruns per sweep, same bits."""
    ra, rb = ROW[first], ROW[second]
    assert CLAIMS[(ra.entry, ra.shape)] == ASYNC
    env(ra.keys)
    run_a = ra.build(dev)
    ref_a = run_a(None)
    env(rb.keys)
    run_b = rb.build(dev)
    ref_b = run_b(None)
    cycles = int(PAIR_DELAY_MS * cycles_per_ms)
    env(ra.keys)
    sa = A.Side(streams[0], cycles=cycles, claim=ASYNC, defer=True)
    run_a(sa)                                                  # enqueued, still behind its delay
    env(rb.keys)
    sb = A.Side(streams[1], cycles=cycles)
    try:
        got_b = run_b(sb)
    finally:
        got_a = sa.finish()
    record(f"pair {first} + {second}: first returned_early {sa.returned_early} (host {sa.host_ms:.2f} ms), second "
           f"returned_early {sb.returned_early} (host {sb.host_ms:.2f} ms)")
    A.assert_same_bits(f"{first} beside {second}", got_a, ref_a)
    A.assert_same_bits(f"{second} beside {first}", got_b, ref_b)


# ---------------------------------------------------------------------------
# section 5: the Python layer on a side stream
# ---------------------------------------------------------------------------

def as_dict(x):
    return {str(i): t for i, t in enumerate(x if isinstance(x, (tuple, list)) else (x,)) if t is not None}


def late_python(what, fn, real, donor, stream, cycles):
    """``fn(**buffers)`` under ``torch.cuda.stream(stream)`` behind the delay, the buffers holding ``donor`` until
    ``real`` lands in stream order.  Returns (fn's result, returned_early)."""
    bufs = {k: d.clone() for k, d in donor.items()}
    torch.cuda.current_stream().synchronize()
    ev = torch.cuda.Event()
    try:
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)
            ev.record(stream)
            for k, b in bufs.items():
                b.copy_(real[k])
            if cycles > 1 and ev.query():                     # (cycles = 1: the warming run, no delay to speak of)
                raise A.HarnessDrained(f"{what}: the set-up drained the stream")
            out = fn(**bufs)
            early = not ev.query()
            for k, b in bufs.items():
                b.copy_(donor[k])
    finally:
        stream.synchronize()
    return out, early


def ops_cases(dev):
    """name -> (fn(**inputs), real inputs, donors): every ops wrapper irlmx.batch uses, on 16 x 16 x 3 (the
    demonstration statistics on the 5 x 5 rollout), device tensors in."""
    from irlmx import ops
    case, c = C.stencil(16, 16), H.case("16x16")
    mdp, hmdp = CC.stencil_mdp(case, dev), c.device_model(dev)
    B, S, A_ = case.B, case.S, case.A
    tm = ops.terminal_mask(case.terminal, S, batch=B, device=dev)
    r, dr = dv(case.reward, dev), dv(CC.other_reward(case.reward), dev)
    p0, dp0 = dv(case.p0, dev), dv(CC.other_p0(case.p0), dev)
    pi, dpi = dv(oracle_policy(case), dev), dv(CC.uniform_policy((B, S, A_)), dev)
    phi = dv(np.tile(case.phi, (B, 1)), dev)
    hr, hdr, hp0 = dv(c.reward, dev), dv(CC.other_reward(c.reward), dev), dv(c.p0, dev)
    hpi = ops.backward_maxent_horizon(hmdp, hr, 8, None)
    R, rmdp, rpi, real, donor = stored(dev)
    rS = rmdp.n_states
    return {
        "backward_maxent": (lambda reward, terminal: ops.backward_maxent(mdp, reward, terminal),
                            {"reward": r, "terminal": tm}, {"reward": dr, "terminal": rolled(tm)}),
        "backward_maxent_extended": (lambda reward, terminal: ops.backward_maxent_extended(mdp, reward, terminal),
                                     {"reward": r, "terminal": tm}, {"reward": dr, "terminal": rolled(tm)}),
        "soft_backward": (lambda reward, phi: ops.soft_backward(mdp, reward, phi, 0.7),
                          {"reward": r, "phi": phi}, {"reward": dr, "phi": rolled(phi)}),
        "forward_svf": (lambda p0, terminal, pi: ops.forward_svf(mdp, p0, terminal, pi, max_iter=3000),   # (the case's cap)
                        {"p0": p0, "terminal": tm, "pi": pi}, {"p0": dp0, "terminal": rolled(tm), "pi": dpi}),
        "value_iteration": (lambda reward: ops.value_iteration(mdp, reward, 0.7), {"reward": r}, {"reward": dr}),
        "policy_evaluation": (lambda reward, pi, terminal: ops.policy_evaluation(mdp, reward, pi, 0.7, terminal),
                              {"reward": r, "pi": pi, "terminal": tm}, {"reward": dr, "pi": dpi, "terminal": rolled(tm)}),
        "expected_value_difference": (
            lambda reward, pi, p0, terminal: ops.expected_value_difference(mdp, reward, pi, p0, 0.7, terminal),
            {"reward": r, "pi": pi, "p0": p0, "terminal": tm}, {"reward": dr, "pi": dpi, "p0": dp0, "terminal": rolled(tm)}),
        "backward_maxent_horizon": (lambda reward: ops.backward_maxent_horizon(hmdp, reward, 8, None, return_log_z0=True),
                                    {"reward": hr}, {"reward": hdr}),
        "soft_backward_horizon": (lambda reward: ops.soft_backward_horizon(hmdp, reward, 1.0, 8, None, return_value0=True),
                                  {"reward": hr}, {"reward": hdr}),
        "forward_svf_horizon": (lambda p0, pi: ops.forward_svf_horizon(hmdp, p0, pi, None, return_marginals=True),
                                {"p0": hp0, "pi": hpi},
                                {"p0": rolled(hp0), "pi": dv(CC.uniform_policy(tuple(hpi.shape)), dev)}),
        "demo_statistics": (lambda states, lengths: ops.demo_statistics(rS, states, lengths),
                            {k: real[k] for k in ("states", "lengths")}, {k: donor[k] for k in ("states", "lengths")}),
        "demo_log_likelihood": (
            lambda pi, states, actions, lengths: ops.demo_log_likelihood(pi, states, actions, lengths),
            {"pi": rpi, **real}, {"pi": dv(CC.uniform_policy(tuple(rpi.shape)), dev), **donor}),
    }


OPS_USED_BY_BATCH = ("backward_maxent", "backward_maxent_extended", "soft_backward", "forward_svf", "value_iteration",
                     "policy_evaluation", "expected_value_difference", "backward_maxent_horizon", "soft_backward_horizon",
                     "forward_svf_horizon", "demo_statistics", "demo_log_likelihood")
PYTHON_DELAY_MS = 100.0


@pytest.mark.parametrize("name", OPS_USED_BY_BATCH)
def test_ops_wrapper_on_a_side_stream(dev, env, streams, cycles_per_ms, name):
    """``_lib.stream_ptr``, the per-call ``torch.empty`` workspace and outputs and the torch operations of each
    wrapper follow torch's current stream: the default-stream bits with inputs that land late."""
    env(CC.DEFAULT)
    fn, real, donor = ops_cases(dev)[name]
    ref = as_dict(fn(**real))
    torch.cuda.current_stream().synchronize()
    as_dict(late_python(name, fn, real, donor, streams[0], 1)[0])            # warms the allocator on that stream
    got, early = late_python(name, fn, real, donor, streams[0], int(PYTHON_DELAY_MS * cycles_per_ms))
    record(f"ops.{name} under torch.cuda.stream: returned_early {early}")
    A.assert_same_bits(f"ops.{name} on a side stream", as_dict(got), ref)
    assert early, f"ops.{name} on the fused shape waited for the stream"   # (every pass here is one fused launch)


def step_bits(make, real, donor, stream=None, cycles=0):
    """theta, svf and last_delta after one ``step()`` of ``make()``; on ``stream``, behind the delay, with theta,
    e_features and p_initial landing late."""
    bm = make()
    if stream is None:
        svf = bm.step()
        torch.cuda.current_stream().synchronize()
        return {"theta": bm.theta, "svf": svf, "last_delta": bm.last_delta}, None
    bufs = {k: getattr(bm, k) for k in real}
    for k, b in bufs.items():
        b.copy_(donor[k])
    torch.cuda.current_stream().synchronize()
    ev = torch.cuda.Event()
    try:
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)
            ev.record(stream)
            for k, b in bufs.items():
                b.copy_(real[k])
            if cycles > 1 and ev.query():
                raise A.HarnessDrained("step(): the set-up drained the stream")
            svf = bm.step()
            early = not ev.query()
            for k in ("e_features", "p_initial"):
                bufs[k].copy_(donor[k])
    finally:
        stream.synchronize()
    return {"theta": bm.theta, "svf": svf, "last_delta": bm.last_delta}, early


@pytest.mark.parametrize("driver", ["BatchedMaxEnt", "BatchedCausalHorizon"])
def test_gradient_step_on_a_side_stream(dev, env, streams, cycles_per_ms, driver):
    """One full ``step()`` on 16 x 16 x 3 with identity features from theta = 1 (BatchedCausalHorizon: T = 8):
    theta, svf and last_delta equal the default-stream step's bits, and the step returns while the delay still
    runs -- irlmx.batch: "no host round trip happens inside a step" on the fused shape."""
    from irlmx import batch
    env(CC.DEFAULT)
    case = C.stencil(16, 16)
    e_features = np.roll(np.array(case.p0), 5, axis=1) * 10.0          # visit counts of a kind: only the bits matter here
    real = {"theta": torch.ones((case.B, case.S), dtype=F64, device=dev), "e_features": dv(e_features, dev),
            "p_initial": dv(case.p0, dev)}
    donor = {"theta": dv(np.array(case.reward)[:, ::-1] * 0.5, dev), "e_features": rolled(real["e_features"]),
             "p_initial": dv(CC.other_p0(case.p0), dev)}

    def make():
        mdp = CC.stencil_mdp(case, dev)
        if driver == "BatchedMaxEnt":
            return batch.BatchedMaxEnt(mdp, real["e_features"].clone(), real["p_initial"].clone(), case.terminal)
        return batch.BatchedCausalHorizon(mdp, real["e_features"].clone(), real["p_initial"].clone(), [], horizon=8)

    ref, _ = step_bits(make, real, donor)
    step_bits(make, real, donor, streams[0], 1)
    got, early = step_bits(make, real, donor, streams[0], int(PYTHON_DELAY_MS * cycles_per_ms))
    record(f"{driver}.step() under torch.cuda.stream: returned_early {early}")
    A.assert_same_bits(f"{driver}.step() on a side stream", got, ref)
    assert early, f"{driver}.step() waited for the stream"


# ---------------------------------------------------------------------------
# section 6: the harness can fail
# ---------------------------------------------------------------------------

def stand_in(dev, fault):
    """A torch "entry point" y = 2 x + (the sum of its zeroed workspace) with 256 bytes of workspace."""
    x = torch.arange(64, dtype=F64, device=dev)
    real, donor = {"x": x}, {"x": x + 100.0}

    def run(side):
        side = side or A.Side(None, fill="zero")
        out = {"y": empty(dev, F64, 64)}

        def invoke(ws, n, st, x):
            w = side.arena.workspace().view(F64)
            default = torch.cuda.default_stream(dev)
            if fault == "zeroes its workspace on the default stream":
                with torch.cuda.stream(default):
                    w.zero_()
            else:
                w.zero_()
            if fault == "reads its input on the default stream":
                with torch.cuda.stream(default):
                    out["y"].copy_(2.0 * x + w.sum())
            else:
                out["y"].copy_(2.0 * x + w.sum())
            if fault == "synchronises":
                torch.cuda.current_stream().synchronize()

        return A.stream_call(f"stand-in ({fault})", dev, 256, out, invoke, real, donor, side)
    return run


def test_clean_stand_in_passes(dev, streams, cycles_per_ms):
    ref = three_runs("stand-in (clean)", stand_in(dev, None), ASYNC, streams, cycles_per_ms)
    assert ref["y"][3].item() == 6.0


@pytest.mark.parametrize("fault,message", [("reads its input on the default stream", "entries of y .* were not written"),
                                           ("zeroes its workspace on the default stream", "entries of y differ")])
def test_work_on_another_stream_is_flagged(dev, streams, cycles_per_ms, fault, message):
    """The first leaves the sentinel (its output, written during the delay from the donor's input, is poisoned
    afterwards); the second reads the 0xFF fill that landed after its memset."""
    with pytest.raises(A.ContractViolation, match=message):
        three_runs(f"stand-in ({fault})", stand_in(dev, fault), SYNC, streams, cycles_per_ms)
    torch.cuda.synchronize(dev)


def test_a_synchronise_in_an_async_call_is_flagged(dev, streams, cycles_per_ms):
    with pytest.raises(A.AsynchronyViolation, match="declared asynchronous"):
        three_runs("stand-in (synchronises)", stand_in(dev, "synchronises"), ASYNC, streams, cycles_per_ms)
    three_runs("stand-in (synchronises)", stand_in(dev, "synchronises"), SYNC, streams, cycles_per_ms)   # bits are right
