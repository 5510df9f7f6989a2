"""Plain extended-precision reference of the four hot loops -- TEST INFRASTRUCTURE ONLY.

``maxent_oracle.py`` is a float64 restatement that follows numpy's operation
order and, where the reference overflows, rescales by powers of two.  This
module is the independent yardstick for it and for the HIP kernels: the same
statements (maxent.py:105-114, 142-159, 320-341; solver.py:40-50, 95-100)
in ``np.longdouble`` (x87: 64-bit mantissa, 15-bit exponent), with **no
rescaling** and no attention to summation order.  It is deliberately the
simplest code that can be right; tests/test_extended_ref.py checks it against
50-digit ``mpmath`` arithmetic.

Every pass takes the per-action matrices ``P_a[from, to]`` as a list of scipy
CSR matrices or dense ndarrays (see :func:`mats_from_table`,
:func:`mats_from_stencil`), so stencil, ELL and dense models all run through
the same few lines, and every fixed-point pass runs exactly the ``k`` sweeps the
caller passes: the reference has no stopping rule of its own (a threshold
evaluated in another precision can stop one sweep earlier or later, which is
not what an accuracy test is about).

Error measures (do not swap one for the other to quieten a failure):

* :func:`elementwise_err` -- ``max |got - ref| / |ref|`` over the entries with
  ``ref != 0``; exact zeros and the non-finite pattern must match exactly.  For
  policies, state-visitation frequencies and soft-VI policies: sums, products
  and ratios of non-negative terms, well conditioned entry by entry, so correct
  float64 code holds ~1e-15 on *every* entry, however small.
* :func:`normwise_err` -- ``max |got - ref| / max |ref|``.  For signed value
  vectors (soft-VI ``v``, VI ``v`` with rewards of both signs) only: there
  ``r + gamma * P v`` cancels, a single entry near zero is ill conditioned (the
  float64 oracle itself reaches 3e-13 elementwise at rewards in [-6, 1]), and an
  elementwise bound would raise false alarms that somebody would later "fix" by
  loosening the measure the other outputs rely on.

Bound: :func:`bound` -- a float64 evaluation under test must stay within
``FACTOR = 16`` times the larger of the oracle's own error against this
reference (same input, same sweep count) and :func:`e_floor`, the worst-case
rounding of one final sweep.
"""

import numpy as np

LD = np.longdouble

#: what may legitimately differ between two correct float64 evaluations
#: (summation order, FMA contraction, collapsed action-sum coefficients, ghost-row
#: recomputation), as a multiple of the oracle's own error
FACTOR = 16.0


class PrecisionUnavailable(RuntimeError):
    """The host's ``np.longdouble`` is not the x87 80-bit format."""


def require_extended():
    """Raise unless np.longdouble has >= 63 mantissa bits and a 15-bit exponent."""
    fi = np.finfo(LD)
    if fi.nmant < 63 or fi.maxexp != 16384:
        raise PrecisionUnavailable(f"np.longdouble has {fi.nmant} mantissa bits, maxexp {fi.maxexp}: "
                                   "the extended reference needs the x87 format (>= 63 bits, maxexp 16384)")


# ---------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------

def _ld_mats(mats):
    """The per-action matrices as longdouble operands (CSR stays CSR)."""
    require_extended()
    out = []
    for m in mats:
        if hasattr(m, "tocsr"):
            out.append(m.tocsr().astype(LD))
        else:
            m = np.asarray(m)
            if m.ndim != 2 or m.shape[0] != m.shape[1]:
                raise ValueError(f"per-action matrix must be square, got {m.shape}")
            out.append(m.astype(LD))
    return out


def _ld(x):
    return np.asarray(x, dtype=np.float64).astype(LD)


def mats_from_table(p_transition):
    """Dense per-action matrices of a ``[S, S, A]`` table (the reference's slices
    ``P[:, :, a]``, maxent.py:102)."""
    p = np.asarray(p_transition, dtype=np.float64)
    return [np.ascontiguousarray(p[:, :, a]) for a in range(p.shape[2])]


def mats_from_stencil(row_val, width, height):
    """Per-action CSR matrices of a STENCIL5 row table ``[A, 5, S]`` on a
    width x height grid: slot 0 is the state itself, slots 1-4 its neighbours
    (+x, -x, +y, -y).  A nonzero weight on a slot that leaves the grid raises."""
    import scipy.sparse as sp
    rv = np.asarray(row_val, dtype=np.float64)
    n = width * height
    if rv.ndim != 3 or rv.shape[1] != 5 or rv.shape[2] != n:
        raise ValueError(f"row table must be [A, 5, {n}], got {rv.shape}")
    s = np.arange(n)
    x, y = s % width, s // width
    on_grid = [np.ones(n, bool), x + 1 < width, x > 0, y + 1 < height, y > 0]
    offset = [0, 1, -1, width, -width]
    mats = []
    for a in range(rv.shape[0]):
        rows, cols, vals = [], [], []
        for k in range(5):
            nz = rv[a, k] != 0.0
            if np.any(nz & ~on_grid[k]):
                raise ValueError(f"action {a}, slot {k}: nonzero weight off the grid")
            rows.append(s[nz])
            cols.append(s[nz] + offset[k])
            vals.append(rv[a, k][nz])
        mats.append(sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                                  shape=(n, n)))
    return mats


def _clear_rows(m, rows):
    """``m`` with the given rows set to zero (maxent.py:98-99)."""
    keep = np.ones(m.shape[0], dtype=LD)
    keep[rows] = 0.0
    if hasattr(m, "tocsr"):
        import scipy.sparse as sp
        return (sp.diags(keep) @ m).tocsr()
    return m * keep[:, None]


# ---------------------------------------------------------------------------
# the four passes
# ---------------------------------------------------------------------------

def backward(mats, terminal, reward, exp_reward=None):
    """Local action probabilities ``[S, A]`` (maxent.py:142-159): ``2 * S`` sweeps
    of ``za[:, a] = exp(r) * (P_a zs)``, ``zs = sum_a za`` from the terminal
    indicator, unscaled.  Raises if ``zs`` leaves longdouble's normal range (a
    condition on the caller's inputs: roughly ``2 S |ln(A e^r)| < 11,000``).

    ``exp(r)`` is evaluated in longdouble: its float64 rounding is part of the
    error of the evaluation under test (the device's exp and numpy's differ in
    the last bit).  ``exp_reward`` replaces it by the caller's float64 values,
    to compare the sweeps alone on a shared ``np.exp(reward)``."""
    p = _ld_mats(mats)
    n = p[0].shape[0]
    er = np.exp(_ld(reward)) if exp_reward is None else _ld(exp_reward)   # maxent.py:142
    zs = np.zeros(n, dtype=LD)
    zs[terminal] = 1.0                                          # maxent.py:147
    za = None
    with np.errstate(over="ignore", invalid="ignore"):          # (overflow is reported below)
        for _ in range(2 * n):                                  # maxent.py:154
            za = np.stack([er * m.dot(zs) for m in p], axis=1)  # maxent.py:155
            zs = za.sum(axis=1)                                 # maxent.py:156
    if not np.isfinite(zs).all():
        raise FloatingPointError("extended backward: zs overflowed longdouble; choose a smaller input")
    if not zs.min() > np.finfo(LD).smallest_normal:
        raise FloatingPointError(f"extended backward: zs reaches {zs.min()!r}, at or below longdouble's "
                                 "smallest normal number; choose another input")
    return za / zs[:, None]                                     # maxent.py:159


def forward(mats, p_initial, terminal, p_action, k, with_condition=False):
    """State-visitation frequencies ``[S]`` after exactly ``k`` sweeps of
    ``d <- p0 + sum_a P_a^T (pi_a * d)`` from ``d = 0``, terminal rows cleared
    (maxent.py:98-112).

    ``with_condition``: also the condition number of the result with respect to
    the edge weights ``W[s, t] = sum_a pi[s, a] P_a[s, t]``.  ``d_k = sum_{j<k}
    (W^T)^j p0``, and a relative change of at most ``eps`` in every weight changes
    the term ``j`` by at most ``j * eps``, so to first order

        |delta d_k[t]| / d_k[t]  <=  eps * c[t],   c[t] = sum_j j ((W^T)^j p0)[t] / d_k[t]

    -- the mean sweep at which the mass at ``t`` arrived (at most ``k``; small
    where the pass has converged quickly, near ``k / 2`` where mass still lingers
    at the cap).  Returns ``(d, max_t c[t])``.  An evaluation that rounds the
    weights once and reuses them every sweep (the kernels' forward pass) carries
    this term coherently; one that rounds ``pi_a * d`` afresh each sweep (the
    oracle) does not.  It explains, and does not set, the one case-specific
    factor of tests/test_gpu_elementwise.py."""
    p = [_clear_rows(m, terminal) for m in _ld_mats(mats)]
    pt = [m.T.tocsr() if hasattr(m, "tocsr") else np.ascontiguousarray(m.T) for m in p]
    p0 = _ld(p_initial)
    pi = _ld(p_action)

    def step(x):
        acc = np.zeros_like(x)
        for a, m in enumerate(pt):
            acc = acc + m.dot(pi[:, a] * x)
        return acc

    d = np.zeros(p0.shape[0], dtype=LD)
    g = np.zeros_like(d)                                        # sum_j j (W^T)^j p0
    for _ in range(int(k)):
        if with_condition:
            g = step(g + d)
        d = p0 + step(d)                                        # maxent.py:110
    if not with_condition:
        return d
    nz = d > 0
    return d, (float(np.max(g[nz] / d[nz])) if nz.any() else 0.0)


def _softmax2(x1, x2):
    hi = np.maximum(x1, x2)
    lo = np.minimum(x1, x2)
    return hi + np.log(LD(1.0) + np.exp(lo - hi))               # maxent.py:274-276


def soft_backward(mats, phi, reward, discount, k):
    """``(pi [S, A], v [S])`` after exactly ``k`` sweeps of discounted soft value
    iteration from ``v = -1e200`` (maxent.py:320-341); ``phi`` is the full
    terminal-reward vector (-inf off the terminals).  Raises if a start sentinel
    survives: with fewer sweeps than the model's diameter ``exp(q - v)`` is
    discontinuous in the last bit of ``q`` there, and two correct evaluations
    may differ by 0 versus 1."""
    p = _ld_mats(mats)
    n = p[0].shape[0]
    phi, r, g = _ld(phi), _ld(reward), LD(np.float64(discount))
    if int(k) < 1:
        raise ValueError("soft_backward needs at least one sweep")
    v = np.full(n, LD(-1e200))                                  # maxent.py:323
    q = None
    with np.errstate(over="ignore", invalid="raise"):
        for _ in range(int(k)):
            q = np.stack([r + g * m.dot(v) for m in p], axis=1)     # maxent.py:329
            v = phi
            for a in range(len(p)):
                v = _softmax2(v, q[:, a])                       # maxent.py:332-333
        if not (v > LD(-1e100)).all():
            raise FloatingPointError(f"extended soft VI: {int((v <= LD(-1e100)).sum())} states still hold the "
                                     f"-1e200 start value after {k} sweeps; run more sweeps")
        return np.exp(q - v[:, None]), v                        # maxent.py:341


def value_iteration(mats, reward, discount, k, average=False):
    """``v [S]`` after exactly ``k`` sweeps of ``v <- r + max_a gamma P_a v``
    (solver.py:40-50) or the action average (solver.py:95-100), from ``v = 0``."""
    p = _ld_mats(mats)
    r, g = _ld(reward), LD(np.float64(discount))
    v = np.zeros(p[0].shape[0], dtype=LD)
    for _ in range(int(k)):
        q = g * np.stack([m.dot(v) for m in p], axis=0)         # solver.py:44
        v = r + (q.sum(axis=0) / LD(len(p)) if average else q.max(axis=0))   # solver.py:47 / :99
    return v


# ---------------------------------------------------------------------------
# error measures and the bound
# ---------------------------------------------------------------------------

def _pair(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        raise AssertionError(f"shape {got.shape} against {ref.shape}")
    return got.astype(LD), ref.astype(LD)


def elementwise_err(got, ref):
    """``max |got - ref| / |ref|`` over the entries with ``ref != 0``.  Raises
    AssertionError unless ``got`` is exactly 0 where ``ref`` is, and NaN / +inf /
    -inf in the same places.  No entry is left out."""
    got, ref = _pair(got, ref)
    for name, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        if not np.array_equal(f(got), f(ref)):
            raise AssertionError(f"{name} pattern differs at {int(np.count_nonzero(f(got) != f(ref)))} entries")
    fin = np.isfinite(ref)
    zero = fin & (ref == 0)
    if np.any(got[zero] != 0):
        raise AssertionError(f"{int(np.count_nonzero(got[zero] != 0))} entries are nonzero where the reference is "
                             f"exactly 0 (largest {float(np.max(np.abs(got[zero]))):.3e})")
    nz = fin & ~zero
    if not nz.any():
        return 0.0
    return float(np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])))


def normwise_err(got, ref):
    """``max |got - ref| / max |ref|`` -- signed value vectors only (module
    docstring).  The non-finite pattern must match."""
    got, ref = _pair(got, ref)
    fin = np.isfinite(ref)
    if not np.array_equal(fin, np.isfinite(got)) or not np.array_equal(got[~fin], ref[~fin], equal_nan=True):
        raise AssertionError("non-finite pattern differs")
    if not fin.any():
        return 0.0
    scale = np.max(np.abs(ref[fin]))
    if scale == 0:
        if np.any(got[fin] != 0):
            raise AssertionError("nonzero entries against an all-zero reference")
        return 0.0
    return float(np.max(np.abs(got[fin] - ref[fin])) / scale)


def e_floor(k_row, n_actions):
    """Worst-case relative rounding of one final float64 sweep: ``k_row * A``
    products and sums, ``A`` action sums, one scaling and one division or
    addition -- ``(k_row * A + A + 2) * 2**-53``.  Keeps a case where the oracle
    happens to be exact from demanding zero."""
    return (k_row * n_actions + n_actions + 2) * 2.0 ** -53


def bound(e_oracle, k_row, n_actions, factor=FACTOR):
    """The most a float64 evaluation may differ from the extended reference."""
    return factor * max(e_oracle, e_floor(k_row, n_actions))
