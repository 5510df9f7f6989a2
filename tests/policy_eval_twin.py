"""CPU twin, references and inputs of the policy-evaluation tests (not a test module).

ops.policy_evaluation folds the policy into one weight per stored edge and then
sweeps K fused multiply-adds per state (csrc/policy_eval.hip).  Nothing here
folds anything:

* :func:`twin` -- float64 numpy, per action: ``v <- r + g * sum_a pi_a * (P_a v)``
  on CSR matrices from ``v = 0`` with the kernels' stop rule; returns the sweep
  count and every delta.  It plays the oracle's role (there is no reference
  function to restate: the reference evaluates the uniform policy only).
* :func:`longdouble` -- the same statements in np.longdouble for a given sweep
  count, on oracle/extended_ref.py's operands.  It plays the reference's role.
* :func:`direct_solve` -- ``np.linalg.solve`` on ``(I - g P_pi) v = r``.

tests/test_policy_eval_cases.py checks the inputs below without a device;
tests/test_gpu_policy_eval.py runs them on one.  Everything is seeded and
cached; cached arrays are read-only.
"""

import functools

import numpy as np

import elementwise_cases as C
import ell_cases as L
import extended_ref as X
import maxent_oracle as O

OK, NONFINITE, MAXITER = 0, 1, 2   # include/irlmx.h status codes
EPS = 1e-3
DISCOUNTS = (0.7, 0.95)
#: the stop must not hinge on a last bit: every one of the twin's last two deltas
#: is at least this far (relative) from eps -- a condition on the inputs
MARGIN = 1e-9

#: name -> (kind, spec, B); stencil spec = (W, H, stay)
CASES = {
    "16x16": ("stencil", (16, 16, False), 3),
    "37x23": ("stencil", (37, 23, False), 1),
    "64x20": ("stencil", (64, 20, False), 1),
    "64x64": ("stencil", (64, 64, False), 1),
    "64x12+stay": ("stencil", (64, 12, True), 1),
    "k5-s200": ("ell", "k5-s200", 3),
    "k8-s1029": ("ell", "k8-s1029", 2),
    "k8-s200": ("ell", "k8-s200", 2),        # A = 1
    "k16-s1029": ("ell", "k16-s1029", 2),
    "k32-s200": ("ell", "k32-s200", 2),      # A = 8
    "128x40": ("stencil", (128, 40, False), 1),
    "k40-s300": ("ell", "k40-s300", 2),
}
#: the fused instantiation (states per lane, slot class) of each case, None: one launch per sweep
FUSED = {"16x16": (1, 5), "37x23": (1, 5), "64x20": (2, 5), "64x64": (4, 5), "64x12+stay": (1, 5),
         "k5-s200": (1, 5), "k8-s1029": (2, 8), "k8-s200": (1, 8), "k16-s1029": (2, 16), "k32-s200": (1, 32),
         "128x40": None, "k40-s300": None}
KINDS = ("dirichlet", "greedy", "maxent")


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def base(name):
    """The elementwise_cases.Case the model comes from (tables, terminals, k_row, A)."""
    kind, spec, B = CASES[name]
    if kind == "stencil":
        W, H, stay = spec
        return C.stencil(W, H, stay, B)
    c = L.case(spec)
    assert c.B == B, (name, c.B)
    return c


@functools.lru_cache(maxsize=None)
def reward(name):
    """[B, S] rewards of both signs."""
    c = base(name)
    r = np.random.default_rng(4200 + list(CASES).index(name)).uniform(-1.0, 1.0, (c.B, c.S))
    _freeze(r)
    return r


def greedy_policy(mats, r):
    """One-hot of argmax_a (P_a r)(s), first index on ties."""
    q = np.stack([m.dot(r) for m in mats], axis=1)
    pi = np.zeros_like(q)
    pi[np.arange(q.shape[0]), q.argmax(axis=1)] = 1.0
    return pi


@functools.lru_cache(maxsize=None)
def policy(name, kind):
    """[B, S, A] float64: "dirichlet" (seeded), "greedy" (one-hot), or "maxent"
    (the float64 oracle's rescaled backward policy of the base case's reward
    and terminals; the GPU tests take the device's own instead)."""
    c = base(name)
    if kind == "dirichlet":
        rng = np.random.default_rng(5200 + list(CASES).index(name))
        pi = rng.dirichlet(np.ones(c.A), size=(c.B, c.S))
    elif kind == "greedy":
        pi = np.stack([greedy_policy(c.mats[b], reward(name)[b]) for b in range(c.B)])
    else:
        assert kind == "maxent", (name, kind)
        pi = np.stack([O.backward_maxent_csr(c.mats[b], c.terminal, c.reward[b]) for b in range(c.B)])
        assert np.isfinite(pi).all(), name
    pi = np.ascontiguousarray(pi, dtype=np.float64)
    _freeze(pi)
    return pi


def runs(name):
    """(policy kind, discount, terminal or None) of every accuracy run of a case:
    the full product of the three policy kinds and both discounts.  The MaxEnt
    policy runs with the case's terminals (it is the policy of that episodic
    model), the other two without."""
    term = tuple(base(name).terminal)
    return [(kind, g, term if kind == "maxent" else None) for kind in KINDS for g in DISCOUNTS]


# ---------------------------------------------------------------------------
# the twin, the longdouble evaluation, the direct solve
# ---------------------------------------------------------------------------

def _keep(n, terminal, dtype):
    keep = np.ones(n, dtype=dtype)
    if terminal is not None:
        keep[list(terminal)] = 0.0
    return keep


def twin(mats, r, pi, discount, eps=EPS, terminal=None, max_iter=0):
    """``(v, sweeps, status, deltas)``: float64, per action, nothing folded."""
    r = np.asarray(r, dtype=np.float64)
    pi = np.asarray(pi, dtype=np.float64) * _keep(r.size, terminal, np.float64)[:, None]
    v = np.zeros_like(r)
    deltas = []
    with np.errstate(invalid="ignore"):
        while True:
            acc = np.zeros_like(r)
            for a, m in enumerate(mats):
                acc = acc + pi[:, a] * m.dot(v)
            nv = r + discount * acc
            d = np.abs(nv - v)
            delta = np.nan if np.isnan(d).any() else d.max()
            v = nv
            deltas.append(float(delta))
            if not delta > eps:
                break
            if max_iter > 0 and len(deltas) >= max_iter:
                break
    status = NONFINITE if delta != delta else (MAXITER if delta > eps else OK)
    return v, len(deltas), status, deltas


def longdouble(mats, r, pi, discount, k, terminal=None):
    """The same statements in np.longdouble, exactly ``k`` sweeps."""
    p = X._ld_mats(mats)
    r, g = X._ld(r), X.LD(np.float64(discount))
    pi = X._ld(pi) * _keep(r.size, terminal, X.LD)[:, None]
    v = np.zeros_like(r)
    for _ in range(int(k)):
        acc = np.zeros_like(r)
        for a, m in enumerate(p):
            acc = acc + pi[:, a] * m.dot(v)
        v = r + g * acc
    return v


def direct_solve(mats, r, pi, discount, terminal=None):
    """The fixed point itself: ``(I - g P_pi) v = r``, terminal rows of P_pi cleared."""
    r = np.asarray(r, dtype=np.float64)
    pi = np.asarray(pi, dtype=np.float64) * _keep(r.size, terminal, np.float64)[:, None]
    p_pi = np.zeros((r.size, r.size))
    for a, m in enumerate(mats):
        p_pi += pi[:, a][:, None] * (m.toarray() if hasattr(m, "toarray") else np.asarray(m))
    return np.linalg.solve(np.eye(r.size) - discount * p_pi, r)


def truncation(eps, discount):
    """The contraction's bound on |v_k - v_inf| after a sweep with delta <= eps."""
    return eps * discount / (1.0 - discount)


def margin_ok(deltas, eps=EPS):
    return all(abs(d - eps) >= MARGIN * eps for d in deltas[-2:])


@functools.lru_cache(maxsize=None)
def reference(name, b, kind, discount, terminal):
    """``(twin v, sweeps, status, deltas, longdouble v, e_oracle)`` of one
    accuracy run on the CPU policy (``policy(name, kind)``)."""
    c = base(name)
    pi = policy(name, kind)[b]
    v, k, status, deltas = twin(c.mats[b], reward(name)[b], pi, discount, terminal=terminal)
    ref = longdouble(c.mats[b], reward(name)[b], pi, discount, k, terminal)
    _freeze(v, ref)
    return v, k, status, tuple(deltas), ref, X.normwise_err(v, ref)


# ---------------------------------------------------------------------------
# device side (torch and irlmx are imported here only)
# ---------------------------------------------------------------------------

def device_model(name, dev, tables=None, shared=False):
    """The DeviceMDP of a case (all its tables, or the given ones)."""
    import torch
    from irlmx import DeviceMDP, _lib
    kind, spec, B = CASES[name]
    c = base(name)
    if kind == "ell":
        return L.device_model(c, dev, tables=tables, shared=shared)
    idx = list(range(B)) if tables is None else list(tables)
    rv = torch.as_tensor(np.ascontiguousarray(c.rv[idx]), dtype=torch.float64, device=dev)
    mdp = DeviceMDP(_lib.LAYOUT_STENCIL5, c.S, 4, len(idx), shared, rv, width=c.W, height=c.H, device=dev)
    return mdp.with_stay() if spec[2] else mdp
