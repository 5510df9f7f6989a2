"""A call runs the shape its plan reports.

irlmx_execution_plan and the entry points read one route (csrc/fixed_point.hip
route()).  For the smallest model that reaches each branch of it, every pass
must move exactly the event counters of the planned shape (the count_event call
sites: a fused launch counts nothing, the cluster shape one cluster_launches
per launch, the grid and dense grid shapes one grid_launches, every per-sweep
shape -- sparse, dense rows, dense GEMM -- one sweep_calls), no rerun counter,
and return the bits of the same call with the fused, cluster and grid shapes
switched off (IRLMX_FUSED_MAX_STATES=0 IRLMX_CLUSTER=0 IRLMX_GRID=0; a DENSE
table knows none of the three, so there the second run repeats the first).

The compact-weight probe of a width-256 backward is left to
test_gpu_parity.test_compact_weights_rectangular_and_multi_launch: its
per-sweep twin takes 2 * S launches at S >= 6144.
"""

import numpy as np
import pytest

import ell_cases as L
import maxent_oracle as O
from conftest import icy_stencil_rect

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OPS = L.OPS
SWITCHES = ("IRLMX_FUSED_MAX_STATES", "IRLMX_CLUSTER", "IRLMX_GRID", "IRLMX_DENSE_GRID", "IRLMX_DENSE_GEMM_MIN",
            "IRLMX_COMPACT")
PER_SWEEP = {"IRLMX_FUSED_MAX_STATES": "0", "IRLMX_CLUSTER": "0", "IRLMX_GRID": "0"}
DISCOUNT = 0.7
MAX_ITER = 300


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    import irlmx
    return irlmx.require_device()


def stencil_model(dev, W, H, B):
    from irlmx import DeviceMDP, _lib
    rv = np.stack([icy_stencil_rect(W, H, p) for p in np.linspace(0.1, 0.3, B)])
    return DeviceMDP(_lib.LAYOUT_STENCIL5, W * H, 4, B, False, torch.as_tensor(rv, device=dev), width=W, height=H,
                     device=dev)


def ell_model(dev, name):
    return L.device_model(L.case(name), dev)


def dense_model(dev, S, A, B):
    """B instances over one shared random DENSE table."""
    from irlmx import DeviceMDP
    P = O.random_dense_mdp(S, A, seed=S + B)[0]
    return DeviceMDP.from_dense(P, device=dev, layout="dense").with_batch(B)


def all_ops(shape):
    return dict.fromkeys(OPS, shape)


def linear(shape, bellman):
    return {"backward": shape, "forward": shape, "soft_backward": bellman, "value_iteration": bellman}


#: name -> (model builder, environment of the call, {op: planned shape}, also the backward without rescaling?)
CASES = {
    "stencil-6x6": (lambda d: stencil_model(d, 6, 6, 2), {}, all_ops("fused"), False),
    # width 64: forward and backward on the cluster shape although the grid fits one CU
    "stencil-64x8": (lambda d: stencil_model(d, 64, 8, 2), {}, linear("cluster", "fused"), False),
    "stencil-24x24": (lambda d: stencil_model(d, 24, 24, 2), {"IRLMX_FUSED_MAX_STATES": "0"},
                      linear("cluster", "grid"), True),
    "ell-k8-s1029": (lambda d: ell_model(d, "k8-s1029"), {"IRLMX_FUSED_MAX_STATES": "0"}, all_ops("grid"), False),
    "ell-k40-s300": (lambda d: ell_model(d, "k40-s300"), {}, all_ops("sweep"), False),
    "dense-s64-b2": (lambda d: dense_model(d, 64, 4, 2), {}, all_ops("dense-grid"), False),
    # 16 instances of a shared table: the GEMM planner takes the three non-forward ops
    "dense-s64-b16": (lambda d: dense_model(d, 64, 4, 16), {},
                      {"backward": "dense-gemm", "forward": "dense-grid", "soft_backward": "dense-gemm",
                       "value_iteration": "dense-gemm"}, False),
    "dense-s64-b2-grid-off": (lambda d: dense_model(d, 64, 4, 2), {"IRLMX_DENSE_GRID": "0"}, all_ops("dense"), False),
}


def moved(plan):
    """The counters a call on this plan moves, and by how much."""
    shape = plan["shape"]
    if shape == "fused":
        return {}
    if shape == "cluster":
        return {"cluster_launches": plan["launches"]}
    if shape in ("grid", "dense-grid"):
        return {"grid_launches": 1}
    assert shape in ("sweep", "dense", "dense-gemm"), plan
    return {"sweep_calls": 1}


def inputs(mdp, seed):
    from irlmx import ops
    B, S, A = mdp.batch, mdp.n_states, mdp.n_actions
    rng = np.random.default_rng(seed)
    pi = rng.uniform(0.1, 1.0, (B, S, A))
    p0 = np.zeros((B, S))
    p0[:, 0] = 1.0
    phi = np.full((B, S), -1e3)
    phi[:, S - 1] = 0.0
    return {"reward": rng.uniform(-1.2, -0.2, (B, S)), "terminal": ops.terminal_mask([S - 1], S, batch=B, device=mdp.device),
            "p0": p0, "pi": pi / pi.sum(axis=2, keepdims=True), "phi": phi}


def run(mdp, op, x, rescale=True):
    from irlmx import ops
    if op == "backward":
        res = (ops.backward_maxent(mdp, x["reward"], x["terminal"], rescale=rescale),)
    elif op == "forward":
        res = ops.forward_svf(mdp, x["p0"], x["terminal"], x["pi"], max_iter=MAX_ITER)
    elif op == "soft_backward":
        res = ops.soft_backward(mdp, x["reward"], x["phi"], DISCOUNT, max_iter=MAX_ITER)
    else:
        res = ops.value_iteration(mdp, x["reward"], DISCOUNT, max_iter=MAX_ITER)
    out = tuple(t.cpu() for t in res)
    torch.cuda.synchronize(mdp.device)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_dispatch_follows_the_plan(dev, monkeypatch, name):
    from irlmx import ops
    build, env, shapes, no_rescale = CASES[name]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    mdp = build(dev)
    x = inputs(mdp, len(name))
    calls = [(op, True) for op in OPS] + ([("backward", False)] if no_rescale else [])
    for op, rescale in calls:
        what = f"{name} {op}" + ("" if rescale else " rescale=0")
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        plan = ops.execution_plan(mdp, op, rescale=rescale)
        # (without rescaling the backward leaves the cluster shape to the per-sweep one)
        want = shapes[op] if rescale else "sweep"
        assert plan["shape"] == want, (what, plan)
        before = ops.counters()
        got = run(mdp, op, x, rescale)
        after = ops.counters()
        delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
        print(what, plan["shape"], delta)
        assert delta == moved(plan), (what, plan, delta)
        for k, v in PER_SWEEP.items():
            monkeypatch.setenv(k, v)
        ref = run(mdp, op, x, rescale)
        for k in PER_SWEEP:
            monkeypatch.delenv(k)
        assert len(got) == len(ref)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert L.same_bits(a, b), f"{what}: output {i} differs from the per-sweep shape's"
