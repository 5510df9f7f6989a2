"""Fixtures and per-pass helpers of the elementwise-accuracy GPU tests (not a test module).

tests/test_gpu_elementwise.py and tests/test_gpu_ell_matrix.py share them: the
``dev`` / ``env`` fixtures (build and device; the planner's environment keys),
``expect_plan``, and one ``run_*`` helper per pass, which runs the pass on the
device, asserts sweep counts and status against the oracle and every entry
against the extended reference (``judge``: e_kernel <= factor * max(e_oracle,
e_floor), oracle/extended_ref.py), prints one line tagged ``[tag]`` and
returns what the device computed.
"""

import numpy as np
import pytest

import elementwise_cases as C
import extended_ref as X

# the planner keys the suite already uses (IRLMX_DENSE_GRID=0, as in test_gpu_dense_grid.py: the only
# way to the streaming dense kernels at a size the persistent dense shape holds)
KEYS = ("IRLMX_FUSED_MAX_STATES", "IRLMX_CLUSTER", "IRLMX_CLUSTER_R", "IRLMX_CLUSTER_G", "IRLMX_PAIR",
        "IRLMX_COMPACT", "IRLMX_SOLO_T", "IRLMX_GRID", "IRLMX_DENSE_GEMM_MIN", "IRLMX_DENSE_GRID")
SWEEP = {"IRLMX_FUSED_MAX_STATES": 0, "IRLMX_CLUSTER": 0, "IRLMX_GRID": 0}


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


# ---------------------------------------------------------------------------
# one pass on the device against oracle and reference
# ---------------------------------------------------------------------------

def expect_plan(mdp, op, **fields):
    from irlmx import ops
    plan = ops.execution_plan(mdp, op)
    got = {k: plan[k] for k in fields}
    assert got == fields, (op, plan)
    return ",".join(f"{k}={v}" for k, v in fields.items())


def judge(case, label, op, plan, rows, tag="elementwise"):
    """rows: per instance (what, e_oracle, e_kernel, bound).  Prints the instance
    of the largest ratio = e_kernel / max(e_oracle, e_floor) with the ratio its
    bound allows, then asserts the bound for every instance.  ``tag``: the
    line's prefix."""
    floor = case.floor()
    worst = max(rows, key=lambda r: r[2] / max(r[1], floor))
    base = max(worst[1], floor)
    print(f"\n[{tag}] {label} {op} {plan} e_oracle={worst[1]:.2e} e_kernel={worst[2]:.2e} "
          f"ratio={worst[2] / base:.3g} allowed={worst[3] / base:.3g}", flush=True)
    for what, e_o, e_k, lim in rows:
        assert e_k <= lim, (f"{label} {op} {what}: e_kernel {e_k:.3e} > {lim:.3e} "
                            f"(e_oracle {e_o:.3e}, e_floor {floor:.3e}, {lim / max(e_o, floor):.1f} x the larger)")


def run_backward(case, mdp, label, plan, tag="elementwise"):
    from irlmx import ops
    tm = ops.terminal_mask(case.terminal, case.S, batch=case.B, device=mdp.device)
    pi = ops.backward_maxent(mdp, case.reward.copy(), tm).cpu().numpy()
    rows = []
    for b in range(case.B):
        o, ref = case.backward(b)
        e_o = X.elementwise_err(o, ref)
        rows.append((f"pi[{b}]", e_o, X.elementwise_err(pi[b], ref), X.bound(e_o, case.k_row, case.A)))
    judge(case, label, "backward", plan, rows, tag)
    return pi


def run_forward(case, mdp, label, plan, cap, factor=X.FACTOR, tag="elementwise"):
    """The forward pass on the oracle's float64 policy (the same input for the
    kernel, the oracle and the reference), stopped by eps or by ``cap``."""
    from irlmx import ops
    tm = ops.terminal_mask(case.terminal, case.S, batch=case.B, device=mdp.device)
    pi = np.stack([case.backward(b)[0] for b in range(case.B)])
    svf, k, st = ops.forward_svf(mdp, case.p0.copy(), tm, pi, max_iter=cap)
    svf, k, st = svf.cpu().numpy(), k.tolist(), st.tolist()
    rows = []
    for b in range(case.B):
        d, k_ref, st_ref, ref = case.forward(b, cap)
        assert (k[b], st[b]) == (k_ref, st_ref), (label, "forward", cap, b, k[b], st[b], k_ref, st_ref)
        e_o = X.elementwise_err(d, ref)
        rows.append((f"svf[{b}]", e_o, X.elementwise_err(svf[b], ref), X.bound(e_o, case.k_row, case.A, factor)))
    judge(case, label, f"forward(cap={cap},k={max(k)})", plan, rows, tag)
    return svf, k, st


def run_soft(case, mdp, label, plan, discount, tag="elementwise"):
    from irlmx import ops
    phi = np.tile(case.phi, (case.B, 1))
    pi, v, k, st = ops.soft_backward(mdp, case.reward.copy(), phi, discount)
    pi, v, k, st = pi.cpu().numpy(), v.cpu().numpy(), k.tolist(), st.tolist()
    rows_pi, rows_v = [], []
    for b in range(case.B):
        o_pi, o_v, k_ref, ref_pi, ref_v = case.soft(b, discount)
        assert (k[b], st[b]) == (k_ref, C.OK), (label, "soft", discount, b, k[b], st[b], k_ref)
        e_pi, e_v = X.elementwise_err(o_pi, ref_pi), X.normwise_err(o_v, ref_v)
        rows_pi.append((f"pi[{b}]", e_pi, X.elementwise_err(pi[b], ref_pi), X.bound(e_pi, case.k_row, case.A)))
        rows_v.append((f"v[{b}]", e_v, X.normwise_err(v[b], ref_v), X.bound(e_v, case.k_row, case.A)))
    judge(case, label, f"soft_pi(g={discount},k={max(k)})", plan, rows_pi, tag)
    judge(case, label, f"soft_v(g={discount})", plan, rows_v, tag)
    return pi, v, k, st


def run_vi(case, mdp, label, plan, discount, tag="elementwise"):
    from irlmx import ops
    out = {}
    for average in (False, True):
        v, k, st = ops.value_iteration(mdp, case.reward.copy(), discount, average=average)
        v, k, st = v.cpu().numpy(), k.tolist(), st.tolist()
        rows = []
        for b in range(case.B):
            o_v, k_ref, ref_v = case.vi(b, discount, average)
            assert (k[b], st[b]) == (k_ref, C.OK), (label, "vi", discount, average, b, k[b], st[b], k_ref)
            e_o = X.normwise_err(o_v, ref_v)
            rows.append((f"v[{b}]", e_o, X.normwise_err(v[b], ref_v), X.bound(e_o, case.k_row, case.A)))
        judge(case, label, f"vi_{'avg' if average else 'max'}(g={discount},k={max(k)})", plan, rows, tag)
        out[average] = (v, k, st)
    return out
