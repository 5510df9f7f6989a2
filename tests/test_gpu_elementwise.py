"""Every kernel family, entry by entry, against the extended-precision reference (needs an MI355X).

The other GPU suites compare with the float64 oracle in a max-norm at 1e-9:
entries a million times smaller than the largest may be wrong by any factor
there, and where the reference program overflows the oracle's rescaled
restatement is its own witness.  Here each family runs small inputs that still
have all its parts (several tiles, ghost rows, partial tiles, several instances
per launch) and every output entry is compared with oracle/extended_ref.py:
the same statements in np.longdouble, unscaled, checked against mpmath in
tests/test_extended_ref.py.

Per case and pass: the plan that was meant to run is asserted first; the sweep
count and status equal the oracle's; then, for every instance,

    e_kernel <= 16 * max(e_oracle, e_floor)

with e_oracle the float64 oracle's own error against the reference on the same
input and sweep count and e_floor = (k_row * A + A + 2) * 2**-53
(extended_ref.bound).  Policies and SVFs are measured elementwise (exact zeros
must be exact zeros: nothing is left out), signed value vectors relative to
their largest entry (extended_ref's docstring says why).  One line per case and
pass is printed: ``[elementwise] case op plan e_oracle e_kernel ratio allowed``
with the instance of the largest ratio = e_kernel / max(e_oracle, e_floor)
(profiles/elementwise_accuracy.txt keeps a run's lines).

One case has a factor of its own, written beside it with its reason
(FORWARD_FACTOR_128x16): every other pass of every case holds the 16.
"""

import numpy as np
import pytest

import elementwise_cases as C
import extended_ref as X
from elementwise_run import (SWEEP, dev, env, expect_plan, run_backward, run_forward,  # noqa: F401 (fixtures)
                             run_soft, run_vi)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# ---------------------------------------------------------------------------
# device models of the shared inputs (tests/elementwise_cases.py)
# ---------------------------------------------------------------------------

def stencil_mdp(case, dev, stay=False):
    from irlmx import DeviceMDP, _lib
    mdp = DeviceMDP(_lib.LAYOUT_STENCIL5, case.S, 4, case.B, False, torch.as_tensor(case.rv.copy(), device=dev),
                    width=case.W, height=case.H, device=dev)
    return mdp.with_stay() if stay else mdp


def built_mdp(case, dev):
    """The device's own world builder on a square grid: its tables must be the
    ones the references were computed on, bit for bit."""
    from irlmx import DeviceMDP
    assert case.W == case.H
    mdp = DeviceMDP.icy_gridworld(case.W, list(C.SLIPS[:case.B]), device=dev)
    assert np.array_equal(mdp.row_val.cpu().numpy(), case.rv), "device world builder differs from the row tables"
    return mdp


def ell_mdp(case, dev):
    from irlmx import DeviceMDP, _lib
    mdp = DeviceMDP.from_dense(case.P.copy(), device=dev, layout="ell")
    assert mdp.layout == _lib.LAYOUT_ELL and (mdp.k_row, mdp.k_col) == (case.k_row, case.k_col)
    return mdp.with_batch(case.B)


def dense_mdp(case, dev):
    from irlmx import DeviceMDP, _lib
    mdp = DeviceMDP.from_dense(case.P.copy(), device=dev, layout="dense")
    assert mdp.layout == _lib.LAYOUT_DENSE
    return mdp.with_batch(case.B)


# ---------------------------------------------------------------------------
# stencil grids
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["fused", "sweep"])
def test_stencil_fused_and_per_sweep(dev, env, shape):
    """16 x 16, three instances (slips 0.1 / 0.2 / 0.35; rewards in [0, 1], [-6, 1]
    and [-1.2, -0.4] in one launch; two terminals; a delta and two spread initial
    distributions) on the device-built tables: one workgroup per instance, and
    one launch per sweep.  All four passes."""
    case = C.stencil(16, 16)
    mdp = built_mdp(case, dev)
    env({} if shape == "fused" else SWEEP)
    label = f"stencil16x16/{shape}"
    for op in ("backward", "forward", "soft_backward", "value_iteration"):
        expect_plan(mdp, op, shape=shape)
    run_backward(case, mdp, label, shape)
    for cap in (7, 3000):
        run_forward(case, mdp, label, shape, cap)
    for discount in (0.7, 0.95):
        run_soft(case, mdp, label, shape, discount)
        run_vi(case, mdp, label, shape, discount)


#: The one case that needs more than 16: the forward at 128 x 16 stopped by the cap of 3,000
#: sweeps.  Every shape folds the actions into one weight per edge before the sweeps
#: (fwd_weights_kernel: w = sum_a P_a pi_a, rounded once) and reuses it in every sweep, so that
#: rounding is a fixed perturbation of the input which the sweeps carry coherently, amplified by
#: the mean sweep at which an entry's mass arrived (extended_ref.forward: ~1,600 here, where mass
#: still lingers beside the start state after 3,000 sweeps).  The oracle rounds pi_a * d afresh
#: each sweep, so e_oracle does not hold that term.  Its size does not come from the kernels:
#: exact longdouble sweeps on float64-rounded folded weights, on the CPU, are off by 15.8 x
#: max(e_oracle, e_floor) on this input (tests/test_extended_ref.py::
#: test_folded_forward_weights_explain_128x16, which asserts 16 + that <= 32).  So: 16 for what
#: two correct float64 evaluations may differ by anyway, plus 16 for the folded weights.
#: DESIGN.md section 2, "Elementwise accuracy", has the derivation.
FORWARD_FACTOR_128x16 = 32.0

#: (W, H, forced R, forced G, IRLMX_PAIR or None, IRLMX_COMPACT or None, backward layout, forward layout)
CLUSTER_CASES = [
    (64, 20, 5, 3, 0, None, 0, 0), (64, 20, 5, 3, 1, None, 1, 1), (64, 20, 5, 3, 2, None, 2, 2),
    (64, 20, 3, 5, None, None, 2, 2),
    (128, 16, 5, 3, 0, None, 0, 0), (128, 16, 5, 3, 1, None, 1, 1), (128, 16, 5, 3, 2, None, 2, 2),
    (128, 16, 5, 3, 3, None, 3, 3), (128, 16, 3, 5, None, None, 2, 2),
    (256, 12, 5, 3, 0, None, 0, 0), (256, 12, 5, 3, 3, None, 3, 3), (256, 12, 5, 3, 4, None, 4, 3),
    (256, 12, 5, 3, None, 0, 3, 0), (256, 12, 3, 5, None, None, 4, 0),
    (37, 23, 5, 3, None, None, 0, 0), (37, 23, 3, 5, None, None, 0, 0),
]


@pytest.mark.parametrize("W,H,R,G,pair,compact,lay_b,lay_f", CLUSTER_CASES,
                         ids=[f"{c[0]}x{c[1]}-R{c[2]}G{c[3]}-pair{c[4]}-compact{c[5]}" for c in CLUSTER_CASES])
def test_cluster_forced_small_plans(dev, env, W, H, R, G, pair, compact, lay_b, lay_f):
    """The persistent tiled kernels on forced small tiles (R = 5 owned rows with
    G = 3 ghost rows, and ghosts wider than tiles: R = 3, G = 5; 3-8 tiles per
    instance, the last one partial, three instances per launch) in every in-tile
    layout of each width: per state (0), pair rows (1), column pairs (2), column
    quads (3), column quads with compact weights (4: the width-256 backward;
    IRLMX_COMPACT=0 puts it back on the five-weight quads), and a generic width.
    Backward: all 2 * S sweeps.  Forward: a cap of 7 (inside the first block) and
    a cap of 3,000 or convergence."""
    case = C.stencil(W, H)
    mdp = stencil_mdp(case, dev)
    e = {"IRLMX_FUSED_MAX_STATES": 0, "IRLMX_CLUSTER_R": R, "IRLMX_CLUSTER_G": G}
    if pair is not None:
        e["IRLMX_PAIR"] = pair
    if compact is not None:
        e["IRLMX_COMPACT"] = compact
    env(e)
    label = f"stencil{W}x{H}/cluster"
    C_tiles = (H + R - 1) // R
    plan_b = expect_plan(mdp, "backward", shape="cluster", R=R, G=G, C=C_tiles, per_launch=3, layout=lay_b)
    plan_f = expect_plan(mdp, "forward", shape="cluster", R=R, G=G, C=C_tiles, per_launch=3, layout=lay_f)
    run_backward(case, mdp, label, plan_b)
    run_forward(case, mdp, label, plan_f, 7)
    run_forward(case, mdp, label, plan_f, 3000, FORWARD_FACTOR_128x16 if (W, H) == (128, 16) else X.FACTOR)


@pytest.mark.parametrize("solo_t", [None, 16])
def test_cluster_solo_tile(dev, env, solo_t):
    """One 64 x 64 instance on one tile (C = 1, no ghost rows), rewards in
    [-1.2, -0.4]: 8,192 backward sweeps in blocks of kSoloBwdT = 256 between
    rescales (and of 16, IRLMX_SOLO_T), on the device-built table; the forward
    on the planner's own plan for one 64 x 64 instance (eight tiles of 8 rows
    with 12 ghost rows: ghosts wider than tiles)."""
    case = C.stencil(64, 64, B=1, ranges=((-1.2, -0.4),))
    mdp = built_mdp(case, dev)
    e = {"IRLMX_FUSED_MAX_STATES": 0}
    if solo_t is not None:
        e["IRLMX_SOLO_T"] = solo_t
    env(e)
    label = f"stencil64x64/solo(T={solo_t or 256})"
    plan_b = expect_plan(mdp, "backward", shape="cluster", R=64, C=1, per_launch=1, layout=2)
    plan_f = expect_plan(mdp, "forward", shape="cluster", R=8, G=12, C=8, per_launch=1, layout=2)
    run_backward(case, mdp, label, plan_b)
    run_forward(case, mdp, label, plan_f, 3000)


@pytest.mark.parametrize("discount", [0.7, 0.95])
def test_grid_shape_soft_vi_and_vi(dev, env, discount):
    """Soft VI and VI (max and average) as one persistent launch exchanging values
    every sweep, at the smallest input that has all of it: 37 x 23 = 851 states
    are four workgroups of 256 per instance, the last one partial, three
    instances (rewards of both signs in the second), to convergence."""
    case = C.stencil(37, 23)
    mdp = stencil_mdp(case, dev)
    env({"IRLMX_FUSED_MAX_STATES": 0})
    label = "stencil37x23/grid"
    plan_s = expect_plan(mdp, "soft_backward", shape="grid", C=4, per_launch=3)
    plan_v = expect_plan(mdp, "value_iteration", shape="grid", C=4, per_launch=3)
    run_soft(case, mdp, label, plan_s, discount)
    run_vi(case, mdp, label, plan_v, discount)


@pytest.mark.parametrize("W,H", [(64, 12), (256, 8)])
def test_stay_action_five_action_table(dev, env, W, H):
    """DeviceMDP.with_stay(): the five-action table (self weights inside the grid)
    on forced three-row tiles.  At width 256 the planner must keep it off the
    compact-weight layout, which cannot hold such a table."""
    case = C.stencil(W, H, stay=True)
    mdp = stencil_mdp(case, dev, stay=True)
    assert mdp.n_actions == 5
    env({"IRLMX_FUSED_MAX_STATES": 0, "IRLMX_CLUSTER_R": 3, "IRLMX_CLUSTER_G": 2})
    label = f"stencil{W}x{H}+stay/cluster"
    tiles = (H + 2) // 3
    plan_b = expect_plan(mdp, "backward", shape="cluster", R=3, G=2, C=tiles, per_launch=3,
                         layout=2 if W == 64 else 3)
    plan_f = expect_plan(mdp, "forward", shape="cluster", R=3, G=2, C=tiles, per_launch=3,
                         layout=2 if W == 64 else 0)
    run_backward(case, mdp, label, plan_b)
    for cap in (7, 3000):
        run_forward(case, mdp, label, plan_f, cap)
    env({"IRLMX_FUSED_MAX_STATES": 0})
    blocks = (case.S + 255) // 256     # workgroups of 256 states per instance
    run_soft(case, mdp, label, expect_plan(mdp, "soft_backward", shape="grid", C=blocks, per_launch=3), 0.7)
    run_vi(case, mdp, label, expect_plan(mdp, "value_iteration", shape="grid", C=blocks, per_launch=3), 0.7)


# ---------------------------------------------------------------------------
# general sparsity (ELL) and dense tables
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("S,shape", [(200, "fused"), (513, "sweep"), (513, "grid")])
def test_ell(dev, env, S, shape):
    """A seeded random sparse MDP (3-12 successors per state, three actions) in
    the ELL layout, one table shared by two reward vectors: 200 states in one
    workgroup; 513 states (odd, no multiple of the wave size) one launch per
    sweep and on the persistent ELL grid (three workgroups per instance, the
    last holding one state).  All four passes."""
    case = C.ell(S)
    mdp = ell_mdp(case, dev)
    env({"fused": {}, "sweep": SWEEP, "grid": {"IRLMX_FUSED_MAX_STATES": 0}}[shape])
    label = f"ell{S}/{shape}"
    for op in ("backward", "forward", "soft_backward", "value_iteration"):
        expect_plan(mdp, op, shape=shape)
    run_backward(case, mdp, label, shape)
    for cap in (7, 3000):
        run_forward(case, mdp, label, shape, cap)
    run_soft(case, mdp, label, shape, C.ELL_DISCOUNT)
    run_vi(case, mdp, label, shape, C.ELL_DISCOUNT)


@pytest.mark.parametrize("plan", ["dense", "dense-grid", "dense-gemm"])
def test_dense(dev, env, plan):
    """O.random_dense_mdp(301, 3, seed=301) (S odd: the K tail of every row
    product): the streaming kernels, the persistent dense shape (two instances)
    and the fp64 MFMA GEMM shape (17 instances of the shared table: one full
    16-instance tile and a tail; the forward has no GEMM form and stays on its
    own shape).  All four passes."""
    B = 17 if plan == "dense-gemm" else 2
    case = C.dense(B)
    mdp = dense_mdp(case, dev)
    env({"dense": {"IRLMX_DENSE_GEMM_MIN": 1000000, "IRLMX_DENSE_GRID": 0},
         "dense-grid": {"IRLMX_DENSE_GEMM_MIN": 1000000},
         "dense-gemm": {"IRLMX_DENSE_GEMM_MIN": 2}}[plan])
    label = f"dense301x{B}/{plan}"
    for op in ("backward", "soft_backward", "value_iteration"):
        expect_plan(mdp, op, shape=plan)
    plan_f = expect_plan(mdp, "forward", shape="dense" if plan == "dense" else "dense-grid")
    run_backward(case, mdp, label, plan)
    # (17 instances: the capped forward only, to keep the longdouble reference to seconds)
    for cap in ((7, 200) if B == 17 else (7, 3000)):
        run_forward(case, mdp, label, plan_f, cap)
    run_soft(case, mdp, label, plan, C.DENSE_DISCOUNT)
    run_vi(case, mdp, label, plan, C.DENSE_DISCOUNT)
