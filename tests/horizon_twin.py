"""CPU twin and longdouble restatement of the finite-horizon passes, and the
inputs of their tests (not a test module).

include/irlmx.h states the two passes (irlmx_backward_maxent_horizon,
irlmx_forward_svf_horizon) statement by statement; this module restates them
three times:

* :func:`backward` / :func:`forward` -- the float64 twin, in the kernels'
  statement order: every partition value is ``m * 2**e`` (``np.frexp``'s form)
  with an integer exponent, a state's neighbours are aligned to the largest
  exponent over the slots where some action has a nonzero entry, the actions
  accumulate in slot order, ``za = er * acc``, the sequential action sum, ``pi =
  za / zsum``; the forward folds its weights from ``pi_t`` every step over every
  slot of the column form.  numpy has no fused multiply-add, so the twin rounds
  each product and each sum separately where the kernels use ``fma`` (as
  tests/extended_twin.py does): two correct float64 evaluations, never compared
  bit for bit; both are bounded against
* :func:`backward_ref` / :func:`forward_ref` -- the same mathematics in
  ``np.longdouble`` on CSR matrices, unscaled, with no attention to order.
  Raises if a partition value leaves longdouble's normal range.
* :func:`backward_common_scale` -- float64 with ONE power-of-two scale per
  instance and step (what a rescaled pass would do): it returns NaN rows on the
  wide inputs, which is why the kernels keep an exponent per state.

Inputs: :data:`CASES`, the list the GPU tests run (tests/test_gpu_horizon.py)
and tests/test_horizon_twin.py checks without a device.
"""

import functools

import numpy as np

import extended_ref as X
import extended_twin as ET
from conftest import icy_stencil_rect

LD = np.longdouble
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
ZERO = ET.ZERO
OK, NONFINITE = 0, 1


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


class Model:
    """One table on the host in the forms the passes read: the row form
    (``rv`` [A, K, S], ``nbr`` [K, S]), the column form (``cv`` [A, Kc, S] =
    P[src_k(t), t, a], ``src`` [Kc, S], ``valid`` [Kc, S]: False for an off-grid
    stencil slot, whose weight is an exact 0 whatever the policy holds) and the
    per-action CSR matrices ``mats`` of the longdouble restatement."""

    def __init__(self, rv, nbr, cv, src, valid, mats):
        self.rv, self.nbr, self.cv, self.src, self.valid, self.mats = rv, nbr, cv, src, valid, mats
        self.A, self.K, self.S = rv.shape
        self.Kc = cv.shape[1]
        _frozen(rv, nbr, cv, src, valid)


def stencil_model(rv, W, H):
    rv = np.ascontiguousarray(rv, dtype=np.float64)
    nbr = ET.stencil_nbr(W, H)
    valid = nbr != np.arange(W * H)[None, :]
    valid[0] = True
    opposite = [0, 2, 1, 4, 3]
    cv = np.stack([np.stack([np.where(valid[k], rv[a, opposite[k]][nbr[k]], 0.0) for k in range(5)])
                   for a in range(rv.shape[0])])
    return Model(rv, nbr, cv, nbr.copy(), valid, X.mats_from_stencil(rv, W, H))


def ell_model(mats, k_row, k_col):
    import ell_cases as E
    ri, rv, ci, cv = E.ell_arrays(mats, k_row, k_col)
    return Model(rv, ri.astype(np.int64), cv, ci.astype(np.int64), np.ones(ci.shape, bool), mats)


def _mask(terminal, S):
    tm = np.zeros(S, bool)
    tm[np.asarray(terminal, dtype=np.int64)] = True
    return tm


# ---------------------------------------------------------------------------
# the float64 twin
# ---------------------------------------------------------------------------

def backward(mod, terminal, reward, T):
    """``(pi_t [T, S, A], log_z0 [S])`` of the finite-horizon backward pass."""
    rv, nbr = mod.rv, mod.nbr
    A, K, S = rv.shape
    with np.errstate(all="ignore"):
        er = np.exp(np.asarray(reward, dtype=np.float64))
    if not np.isfinite(er).all():           # bwd_nonfinite_rule: NaN at every row of every step
        return np.full((T, S, A), np.nan), np.full(S, np.nan)
    tm = _mask(terminal, S)
    m_T, e_T = ET._split(er, np.zeros(S, dtype=np.int64))
    m, e = m_T, e_T
    anyk = (rv != 0).any(axis=0)
    pi = np.empty((T, S, A))
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            mn, en = m[nbr], e[nbr]
            E = np.where(anyk, en, ZERO).max(axis=0)
            z = ET._aligned(mn, en, E[None, :])
            za = np.zeros((S, A))
            zsum = np.zeros(S)
            for a in range(A):
                acc = np.zeros(S)
                for k in range(K):
                    acc = rv[a, k] * z[k] + acc
                za[:, a] = er * acc
                zsum = zsum + za[:, a]
            pi[t] = za / zsum[:, None]
            m_new, e_new = ET._split(zsum, E)
            m, e = np.where(tm, m_T, m_new), np.where(tm, e_T, e_new)
        log_z0 = np.where(e == ZERO, -np.inf, e.astype(np.float64) * LN2 + np.log(np.where(m == 0, 1.0, m)))
    return pi, log_z0


def forward(mod, p0, terminal, pi_t):
    """``(svf [S], svf_t [T + 1, S], status)`` of the finite-horizon forward pass."""
    cv, src = mod.cv, mod.src
    A, Kc, S = cv.shape
    pi_t = np.asarray(pi_t, dtype=np.float64)
    T = pi_t.shape[0]
    live = mod.valid & ~_mask(terminal, S)[src]
    d = np.array(p0, dtype=np.float64)
    D = d.copy()
    marg = np.empty((T + 1, S))
    marg[0] = d
    with np.errstate(all="ignore"):
        for t in range(T):
            w = np.zeros((Kc, S))
            for a in range(A):
                w = cv[a] * pi_t[t][:, a][src] + w
            w = np.where(live, w, 0.0)
            acc = np.zeros(S)
            for k in range(Kc):
                acc = w[k] * d[src[k]] + acc
            d = acc
            D = D + d
            marg[t + 1] = d
    return D, marg, (OK if np.isfinite(D).all() else NONFINITE)


# ---------------------------------------------------------------------------
# the longdouble restatement
# ---------------------------------------------------------------------------

def backward_ref(mats, terminal, reward, T):
    """``(pi_t [T, S, A], log_z0 [S])`` in longdouble, unscaled.  ``exp(r)`` is
    evaluated in longdouble: its float64 rounding belongs to the evaluation
    under test.  Raises if a nonzero Z leaves longdouble's normal range."""
    p = X._ld_mats(mats)
    S = p[0].shape[0]
    er = np.exp(X._ld(reward))
    tm = _mask(terminal, S)
    tiny = np.finfo(LD).smallest_normal
    Z = er.copy()
    pi = np.empty((T, S, len(p)), dtype=LD)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for t in range(T - 1, -1, -1):
            za = np.stack([er * m.dot(Z) for m in p], axis=1)
            zs = za.sum(axis=1)
            pi[t] = za / zs[:, None]
            Z = np.where(tm, er, zs)
            nz = Z != 0
            if not np.isfinite(Z).all() or (nz.any() and not Z[nz].min() > tiny):
                raise FloatingPointError(f"horizon reference: Z_{t} leaves longdouble's normal range; choose another input")
        log_z0 = np.where(Z == 0, LD(-np.inf), np.log(np.where(Z == 0, LD(1), Z)))
    return pi, log_z0


def forward_ref(mats, p0, terminal, pi_t):
    """``(svf [S], svf_t [T + 1, S])`` in longdouble from a float64 ``pi_t``."""
    p = [X._clear_rows(m, np.asarray(terminal, dtype=np.int64)) for m in X._ld_mats(mats)]
    pt = [m.T.tocsr() if hasattr(m, "tocsr") else np.ascontiguousarray(m.T) for m in p]
    pi = X._ld(pi_t)
    d = X._ld(p0)
    D = d.copy()
    marg = [d]
    for t in range(pi.shape[0]):
        acc = np.zeros_like(d)
        for a, m in enumerate(pt):
            acc = acc + m.dot(pi[t][:, a] * d)
        d = acc
        D = D + d
        marg.append(d)
    return D, np.stack(marg)


# ---------------------------------------------------------------------------
# one common scale per step (why the kernels keep an exponent per state)
# ---------------------------------------------------------------------------

def backward_common_scale(mod, reward, T):
    """pi_t [T, S, A] in float64 with the whole partition vector rescaled by one
    power of two per step (no terminal): entries further than float64's span
    below the largest flush to 0 and their rows come back 0 / 0."""
    rv, nbr = mod.rv, mod.nbr
    A, K, S = rv.shape
    er = np.exp(np.asarray(reward, dtype=np.float64))
    Z = er.copy()
    pi = np.empty((T, S, A))
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            z = Z[nbr]
            za = np.stack([er * sum(rv[a, k] * z[k] for k in range(K)) for a in range(A)], axis=1)
            zs = za.sum(axis=1)
            pi[t] = za / zs[:, None]
            Z = np.ldexp(zs, -int(np.frexp(zs.max())[1]))
    return pi


def nan_rows(pi):
    return int(np.isnan(np.asarray(pi)).any(axis=-1).sum())


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

#: (W, H, lo, T): icy slip 0.2, reward lo everywhere and 0 at state 0, no terminal
WIDE = ((64, 4, -15.0, 96), (128, 4, -7.0, 200), (256, 4, -4.0, 400))


class Case:
    """One launch: B instances with their tables, rewards, initial
    distributions, the terminal list, the horizon and the plan the device must
    report -- ``bwd``: (states per thread, slot class) of the fused backward or
    None where only the per-sweep shape applies; ``fwd``: states per thread or
    None (with several states per thread the planner takes the fused shape only
    from one workgroup per CU on: IRLMX_HORIZON_FUSED_BATCH).  The
    twin's and the reference's results are computed once per instance."""

    def __init__(self, name, models, reward, p0, terminal, T, bwd, fwd, grid=None, ell=None):
        self.name, self.models, self.T, self.bwd, self.fwd = name, models, int(T), bwd, fwd
        self.reward, self.p0, self.terminal = np.asarray(reward, float), np.asarray(p0, float), list(terminal)
        self.grid, self.ell = grid, ell          # (W, H) of a stencil case / the ell_cases name
        self.B, self.S = self.reward.shape
        self.A, self.K, self.Kc = models[0].A, models[0].K, models[0].Kc
        _frozen(self.reward, self.p0)

    def model(self, b):
        return self.models[b if len(self.models) > 1 else 0]

    @functools.lru_cache(maxsize=None)
    def twin_backward(self, b):
        out = backward(self.model(b), self.terminal, self.reward[b], self.T)
        _frozen(*out)
        return out

    @functools.lru_cache(maxsize=None)
    def ref_backward(self, b):
        out = backward_ref(self.model(b).mats, self.terminal, self.reward[b], self.T)
        _frozen(*out)
        return out

    def e_twin_backward(self, b):
        """(elementwise error of the twin's pi_t, normwise error of its log_z0)"""
        (pi, lz), (rpi, rlz) = self.twin_backward(b), self.ref_backward(b)
        return X.elementwise_err(pi, rpi), X.normwise_err(lz, rlz)

    def forward_errors(self, b, pi_t, got=None):
        """``(e_svf, e_svf_t)`` against the longdouble forward fed ``pi_t``
        (float64 [T, S, A]) of the twin's forward on the same ``pi_t``, or of
        ``got = (svf, svf_t)``."""
        rD, rm = forward_ref(self.model(b).mats, self.p0[b], self.terminal, pi_t)
        if got is None:
            got = forward(self.model(b), self.p0[b], self.terminal, pi_t)[:2]
        return X.elementwise_err(got[0], rD), X.elementwise_err(got[1], rm)

    def bound_pi(self, e_twin):
        return X.bound(e_twin, self.K, self.A)

    def bound_svf(self, e_twin):
        return X.bound(e_twin, self.Kc, self.A)

    def device_model(self, dev, tables=None):
        """The DeviceMDP of this case (``tables``: of these instances alone)."""
        import torch
        from irlmx import DeviceMDP, _lib
        if self.ell is not None:
            import ell_cases as E
            return E.device_model(E.case(self.ell), dev, tables=tables)
        idx = list(range(self.B)) if tables is None else list(tables)
        if len(self.models) == 1:
            rv, shared, n = self.models[0].rv[None], True, len(idx)
        else:
            rv, shared, n = np.stack([self.models[b].rv for b in idx]), False, len(idx)
        W, H = self.grid
        return DeviceMDP(_lib.LAYOUT_STENCIL5, self.S, self.A, n, shared,
                         torch.as_tensor(np.array(rv), device=dev), width=W, height=H, device=dev)


def _two_deltas(B, S):
    p0 = np.zeros((B, S))
    p0[:, 0] = 0.75
    p0[:, S // 2 + 3] = 0.25
    return p0


def _stencil_case(name, W, H, slips, T, terminal, bwd, fwd, stay=False, seed=0, p0=None):
    S = W * H
    rng = np.random.default_rng(1000 + seed)
    models = []
    for slip in slips:
        rv = icy_stencil_rect(W, H, slip)
        if stay:                                  # DeviceMDP.with_stay: a fifth action that stays
            extra = np.zeros((1, 5, S))
            extra[0, 0] = 1.0
            rv = np.concatenate([rv, extra])
        models.append(stencil_model(rv, W, H))
    B = len(slips)
    reward = rng.uniform(-1.5, 0.0, (B, S))
    return Case(name, models, reward, _two_deltas(B, S) if p0 is None else p0, terminal, T, bwd, fwd, grid=(W, H))


def _wide_case(W, H, lo, T):
    S = W * H
    reward = np.full((1, S), float(lo))
    reward[0, 0] = 0.0
    spt = 1 if S <= 1024 else 2
    return Case(f"wide-{W}x{H}", [stencil_model(icy_stencil_rect(W, H, 0.2), W, H)], reward, np.full((1, S), 1.0 / S),
                [], T, (spt, 5), spt, grid=(W, H))


#: ELL cases of tests/ell_cases.py: (name, horizon, with the case's terminals)
ELL = (("k5-s200", 12, True), ("k8-s1029", 8, True), ("k16-s1029", 8, False), ("k32-s200", 12, False),
       ("k40-s300", 10, True), ("hub-s200", 12, True))


def _ell_case(name, T, with_terminal):
    import ell_cases as E
    c = E.case(name)
    models = [ell_model(c.mats[b], c.k_row, c.k_col) for b in range(c.B)]
    bwd, fwd = E.FUSED[name][0], E.FUSED[name][1]
    return Case(name, models, c.reward, c.p0, c.terminal if with_terminal else [], T, bwd,
                None if fwd is None else fwd[0], ell=name)


@functools.lru_cache(maxsize=None)
def case(name):
    S3723 = 37 * 23
    builders = {
        "16x16": lambda: _stencil_case("16x16", 16, 16, (0.2, 0.1, 0.35), 40, [], (1, 5), 1, seed=1),
        "37x23": lambda: _stencil_case("37x23", 37, 23, (0.2,), 30, [S3723 - 1, 17], (1, 5), 1, seed=2),
        "64x20": lambda: _stencil_case("64x20", 64, 20, (0.2,), 24, [], (2, 5), 2, seed=3),
        "64x64": lambda: _stencil_case("64x64", 64, 64, (0.2,), 16, [], (4, 5), 4, seed=4),
        "128x40": lambda: _stencil_case("128x40", 128, 40, (0.2, 0.3), 12, [], None, None, seed=5),
        "64x12-stay": lambda: _stencil_case("64x12-stay", 64, 12, (0.2,), 20, [], (1, 5), 1, stay=True, seed=6),
        "16x16-T1": lambda: _stencil_case("16x16-T1", 16, 16, (0.2,), 1, [], (1, 5), 1, seed=7),
    }
    for W, H, lo, T in WIDE:
        builders[f"wide-{W}x{H}"] = functools.partial(_wide_case, W, H, lo, T)
    for n, T, wt in ELL:
        builders[n] = functools.partial(_ell_case, n, T, wt)
    return builders[name]()


#: the launches of tests/test_gpu_horizon.py
CASES = ("16x16", "37x23", "64x20", "64x64", "128x40", "64x12-stay", "k5-s200", "k8-s1029", "k16-s1029", "k32-s200",
         "k40-s300", "hub-s200", "wide-64x4", "wide-256x4", "16x16-T1")
#: those of CASES the fused shape runs in at least one pass
FUSED = tuple(n for n in CASES if n not in ("128x40", "k40-s300"))
