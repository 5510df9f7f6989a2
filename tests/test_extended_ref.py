"""The extended-precision reference (oracle/extended_ref.py) and its measures, on the CPU.

* the reference against 50-digit mpmath arithmetic: longdouble is precise
  enough to judge float64 (1e-17 elementwise, all four passes);
* the reference against the reference program's own recorded outputs
  (tests/golden/), by the rule the GPU tests use;
* the oracle's ``rescale=True`` backward against the unrescaled extended
  evaluation: the first check of the rescaling that does not share its idea;
* the inputs of tests/test_gpu_elementwise.py stay inside the reference's guards;
* the elementwise measure sees an error the suite's max-norm ``close()`` does not.

Most of the file's time is the unscaled longdouble backward of 3,072-4,096
states (6,144-8,192 sweeps in x87 arithmetic: 2-4 s per instance); the cases
that need it are the point of the file.
"""

import mpmath as mp
import numpy as np
import pytest

import elementwise_cases as C
import extended_ref as X
import maxent_oracle as O
from conftest import load_golden

try:
    X.require_extended()
except X.PrecisionUnavailable as e:   # a host without x87 long double
    pytest.skip(str(e), allow_module_level=True)

#: forward sweeps in longdouble this file spends on one fixture case
SWEEP_BUDGET = 6_000


# ---------------------------------------------------------------------------
# against mpmath (50 digits)
# ---------------------------------------------------------------------------

def _mpf(x):
    """A longdouble as an exact mpf (two float64 pieces hold its 64 bits)."""
    x = np.longdouble(x)
    if not np.isfinite(x):
        return mp.mpf(float(x))
    hi = np.float64(x)
    lo = np.float64(x - np.longdouble(hi))
    assert np.longdouble(hi) + np.longdouble(lo) == x
    return mp.mpf(float(hi)) + mp.mpf(float(lo))


def _rows(P):
    """[A][S] lists of (target, mpf weight) of a dense [S, S, A] table."""
    S, _, A = P.shape
    return [[[(t, mp.mpf(float(P[s, t, a]))) for t in np.flatnonzero(P[s, :, a])] for s in range(S)]
            for a in range(A)]


def _mp_dot(rows_a, v):
    return [mp.fsum(w * v[t] for t, w in row) for row in rows_a]


def _mp_backward(P, terminal, reward):
    S, _, A = P.shape
    rows = _rows(P)
    er = [mp.exp(mp.mpf(float(r))) for r in reward]
    zs = [mp.mpf(0)] * S
    for t in np.arange(S)[terminal]:
        zs[t] = mp.mpf(1)
    for _ in range(2 * S):
        za = [[er[s] * x for s, x in enumerate(_mp_dot(rows[a], zs))] for a in range(A)]
        zs = [mp.fsum(za[a][s] for a in range(A)) for s in range(S)]
    return [[za[a][s] / zs[s] for a in range(A)] for s in range(S)]


def _mp_forward(P, p0, terminal, pi, k):
    S, _, A = P.shape
    Pc = np.array(P)
    Pc[terminal, :, :] = 0.0
    cols = _rows(np.transpose(Pc, (1, 0, 2)))        # [A][to] lists of (from, weight)
    p0 = [mp.mpf(float(x)) for x in p0]
    pi = [[mp.mpf(float(x)) for x in row] for row in pi]
    d = [mp.mpf(0)] * S
    for _ in range(k):
        d = [p0[t] + mp.fsum(w * pi[s][a] * d[s] for a in range(A) for s, w in cols[a][t]) for t in range(S)]
    return d


def _mp_softmax2(x1, x2):
    hi, lo = max(x1, x2), min(x1, x2)
    return hi + mp.log(1 + mp.exp(lo - hi))


def _mp_soft(P, phi, reward, discount, k):
    S, _, A = P.shape
    rows = _rows(P)
    r = [mp.mpf(float(x)) for x in reward]
    phi = [mp.mpf(float(x)) for x in phi]
    g = mp.mpf(float(discount))
    v = [mp.mpf(-1e200)] * S
    for _ in range(k):
        q = [[r[s] + g * x for s, x in enumerate(_mp_dot(rows[a], v))] for a in range(A)]
        v = list(phi)
        for a in range(A):
            v = [_mp_softmax2(v[s], q[a][s]) for s in range(S)]
    return [[mp.exp(q[a][s] - v[s]) for a in range(A)] for s in range(S)], v


def _mp_vi(P, reward, discount, k, average):
    S, _, A = P.shape
    rows = _rows(P)
    r = [mp.mpf(float(x)) for x in reward]
    g = mp.mpf(float(discount))
    v = [mp.mpf(0)] * S
    for _ in range(k):
        q = [[g * x for x in _mp_dot(rows[a], v)] for a in range(A)]
        v = [r[s] + (mp.fsum(q[a][s] for a in range(A)) / A if average else max(q[a][s] for a in range(A)))
             for s in range(S)]
    return v


def _mp_elementwise(got, ref):
    """max |got - ref| / |ref| of a longdouble array against nested mpf lists."""
    got = np.asarray(got)
    ref = np.array(ref, dtype=object).reshape(got.shape)
    worst = mp.mpf(0)
    for g, r in zip(got.ravel(), ref.ravel()):
        if r == 0:
            assert g == 0
            continue
        worst = max(worst, abs(_mpf(g) - r) / abs(r))
    return float(worst)


def _mp_normwise(got, ref):
    got = np.asarray(got)
    scale = max(abs(r) for r in ref)
    return float(max(abs(_mpf(g) - r) for g, r in zip(got, ref)) / scale)


def _mp_models():
    rng = np.random.default_rng(55)
    yield "icy5", O.icy_gridworld_table(5, 0.2), [24], rng.uniform(-1.0, 1.0, 25), np.full(25, 1.0 / 25)
    z = load_golden("generic")
    yield "sparse20", z["sparse20__P"], [int(t) for t in z["sparse20__terminal"]], z["sparse20__reward"], \
        z["sparse20__p0"]


@pytest.mark.parametrize("model", ["icy5", "sparse20"])
def test_reference_against_mpmath(model):
    """All four passes on a 5x5 icy gridworld (rewards of both signs) and on the
    ``sparse20`` MDP of tests/golden/generic.npz: the longdouble reference agrees
    with 50-digit arithmetic to 1e-17 on every entry (values: relative to the
    largest), two orders of magnitude below float64's rounding."""
    name, P, terminal, reward, p0 = next(m for m in _mp_models() if m[0] == model)
    S = P.shape[0]
    mats = X.mats_from_table(P)
    phi = O.terminal_reward(terminal, S)
    with mp.workdps(50):
        pi = X.backward(mats, terminal, reward)
        assert _mp_elementwise(pi, _mp_backward(P, terminal, reward)) <= 1e-17
        pi64 = np.asarray(pi, dtype=np.float64)
        for k in (1, 80):
            svf = X.forward(mats, p0, terminal, pi64, k)
            assert _mp_elementwise(svf, _mp_forward(P, p0, terminal, pi64, k)) <= 1e-17, k
        for discount in (0.7,):
            # the converged count: the -1e200 start value decays by `discount` per sweep
            # and the reference refuses to run while it is still there
            k = O.soft_backward(P, terminal, reward, discount)[2]
            spi, v = X.soft_backward(mats, phi, reward, discount, k)
            ref_pi, ref_v = _mp_soft(P, phi, reward, discount, k)
            assert _mp_elementwise(spi, ref_pi) <= 1e-17, discount
            assert _mp_normwise(v, ref_v) <= 1e-17, discount
        for discount in (0.7, 0.95):
            for average in (False, True):
                vv = X.value_iteration(mats, reward, discount, 40, average)
                assert _mp_normwise(vv, _mp_vi(P, reward, discount, 40, average)) <= 1e-17, (discount, average)


# ---------------------------------------------------------------------------
# against the reference program's recorded outputs
# ---------------------------------------------------------------------------

def _rule(e_got, e_oracle, k_row, n_actions, what):
    lim = X.bound(e_oracle, k_row, n_actions)
    assert e_got <= lim, f"{what}: {e_got:.3e} > 16 * max({e_oracle:.3e}, {X.e_floor(k_row, n_actions):.3e})"


def _xmats(P):
    """Operands of the extended reference: CSR for the (sparse) fixture tables."""
    import scipy.sparse as sp
    return [sp.csr_matrix(P[:, :, a]) for a in range(P.shape[2])]


def _check_backward(P, terminal, reward, recorded, what):
    mats = _xmats(P)
    S, _, A = P.shape
    ref = X.backward(mats, terminal, reward)
    e_o = X.elementwise_err(O.backward_maxent(P, terminal, reward, rescale=True), ref)
    _rule(X.elementwise_err(recorded, ref), e_o, S, A, what + " pi")


def _check_forward(P, p0, terminal, pi, k, recorded, what):
    S, _, A = P.shape
    ref = X.forward(_xmats(P), p0, terminal, pi, k)
    d, ko = O.forward_svf(P, p0, terminal, pi, max_iter=k)
    assert ko == k, (what, ko, k)
    _rule(X.elementwise_err(recorded, ref), X.elementwise_err(d, ref), S, A, what + " svf")


def _check_soft(P, terminal, reward, discount, k, recorded_pi, what):
    S, _, A = P.shape
    phi = O.terminal_reward(terminal, S)
    ref_pi, ref_v = X.soft_backward(_xmats(P), phi, reward, discount, k)
    pi, v, ko = O.soft_backward(P, terminal, reward, discount, max_iter=k)
    assert ko == k, (what, ko, k)
    _rule(X.elementwise_err(recorded_pi, ref_pi), X.elementwise_err(pi, ref_pi), S, A, what + " soft pi")


def _check_vi(P, reward, discount, k, average, recorded, what):
    S, _, A = P.shape
    ref = X.value_iteration(_xmats(P), reward, discount, k, average)
    v, ko = O.value_iteration(P, reward, discount, average=average, max_iter=k)
    assert ko == k, (what, ko, k)
    _rule(X.normwise_err(recorded, ref), X.normwise_err(v, ref), S, A, what + " v")


def test_reference_against_recorded_outputs():
    """config1, maxent_small, causal_small, vi and generic fixtures (the reference
    program's own float64 outputs), wherever the reference stayed finite: the
    extended reference run for the recorded sweep count agrees with them within
    16 * max(e_oracle, e_floor), elementwise for policies and SVFs, relative to
    the largest entry for values.  (The dense tables make k_row = S in e_floor:
    numpy's dgemv sums all S products of a row.)  Forward passes of more than
    6,000 sweeps (s8_unif: 11.9M; s16_unif: 16k; s32_unif: 53k) are left to the suites that
    run them on the device; their backward / soft passes are checked."""
    z = load_golden("config1")
    P, term, ones = z["p_transition"], [int(t) for t in z["terminal"]], np.ones(25)
    _check_backward(P, term, ones, z["pi1"], "config1")
    _check_forward(P, z["p_initial"], term, z["pi1"], int(z["k_f1"]), z["svf1"], "config1")
    _check_soft(P, term, ones, 0.7, int(z["k_s1"]), z["cpi1"], "config1")
    _check_forward(P, z["p_initial"], term, z["cpi1"], int(z["k_cf1"]), z["csvf1"], "config1 causal")
    _check_vi(P, z["reward"], 0.7, int(z["vi_sweeps"]), False, z["value"], "config1")

    z = load_golden("maxent_small")
    checked = 0
    for c in [str(n) for n in z["names"]]:
        if not np.isfinite(z[c + "__pi"]).all():
            continue                                   # the reference overflowed, or had no terminal
        P = O.icy_gridworld_table(int(z[c + "__size"]), float(z[c + "__p_slip"]))
        term = [int(t) for t in z[c + "__terminal"]]
        _check_backward(P, term, z[c + "__reward"], z[c + "__pi"], c)
        checked += 1
        if int(z[c + "__k_f"]) <= SWEEP_BUDGET:
            _check_forward(P, z[c + "__p0"], term, z[c + "__pi"], int(z[c + "__k_f"]), z[c + "__svf"], c)
    assert checked >= 5, checked

    z = load_golden("causal_small")
    for c in [str(n) for n in z["names"]]:
        P = O.icy_gridworld_table(int(z[c + "__size"]), 0.2)
        term = [int(t) for t in z[c + "__terminal"]]
        _check_soft(P, term, z[c + "__reward"], float(z[c + "__discount"]), int(z[c + "__k_s"]), z[c + "__pi"], c)
        if int(z[c + "__k_f"]) <= SWEEP_BUDGET:
            _check_forward(P, z[c + "__p0"], term, z[c + "__pi"], int(z[c + "__k_f"]), z[c + "__svf"], c + " causal")

    z = load_golden("vi")
    for c in sorted({k.split("__")[0] for k in z.files if k.startswith("s")}):
        P = O.icy_gridworld_table(int(z[c + "__size"]), 0.2)
        _check_vi(P, z[c + "__reward"], float(z[c + "__discount"]), int(z[c + "__k"]), bool(z[c + "__average"]),
                  z[c + "__value"], c)
    _check_vi(O.gridworld_table(4), z["det4__reward"], 0.5, int(z["det4__k"]), False, z["det4__value"], "det4")

    z = load_golden("generic")
    for c in [str(n) for n in z["names"]]:
        P, term = z[c + "__P"], [int(t) for t in z[c + "__terminal"]]
        r, p0 = z[c + "__reward"], z[c + "__p0"]
        _check_backward(P, term, r, z[c + "__pi"], c)
        _check_forward(P, p0, term, z[c + "__pi"], int(z[c + "__k_f"]), z[c + "__svf"], c)
        _check_soft(P, term, r, 0.8, int(z[c + "__k_s"]), z[c + "__cpi"], c)
        _check_forward(P, p0, term, z[c + "__cpi"], int(z[c + "__k_cf"]), z[c + "__csvf"], c + " causal")
        _check_vi(P, r, 0.9, int(z[c + "__k_v"]), False, z[c + "__v"], c)
        _check_vi(P, r, 0.9, int(z[c + "__k_va"]), True, z[c + "__va"], c + " average")


# ---------------------------------------------------------------------------
# the oracle's rescaling against the unrescaled evaluation
# ---------------------------------------------------------------------------

#: (size, reward range, seed, forward sweeps); the forward runs the same count in both
RESCALE_CASES = [(32, (0.0, 1.0), 321, 1000), (32, (-6.0, 1.0), 322, 1000), (48, (-3.0, 0.5), 481, 1000),
                 (64, (-1.2, -0.4), 641, 1000)]
_rescale_cache = {}


def _rescale_case(size, rng_range, seed, k_f):
    key = (size, rng_range, seed)
    if key not in _rescale_cache:
        S = size * size
        r = np.random.default_rng(seed).uniform(*rng_range, S)
        mats = O.icy_gridworld_csr(size, 0.2)
        term = [S - 1]
        pi = O.backward_maxent_csr(mats, term, r)                       # rescale=True
        p0 = np.zeros(S)
        p0[0] = 1.0
        svf, k = O.forward_svf_csr(mats, p0, term, pi, max_iter=k_f)
        _rescale_cache[key] = dict(mats=mats, term=term, r=r, pi=pi, svf=svf,
                                   svf_ref=X.forward(mats, p0, term, pi, k))
    return _rescale_cache[key]


@pytest.mark.parametrize("size,rng_range,seed,k_f", RESCALE_CASES)
def test_oracle_rescale_against_unrescaled_reference(size, rng_range, seed, k_f):
    """The oracle's power-of-two rescaled backward (the only "truth" of the
    non-causal backward above ~13x13, where the reference program overflows)
    against the extended reference, which does not rescale at all (zs reaches
    1e1800-1e2800 here): every policy entry within 1e-14, relative to itself.

    The sweeps are isolated from the one input rounding both sides would
    otherwise not share: the reference is given the oracle's float64
    ``np.exp(reward)`` (maxent.py:142 as the reference program evaluates it).
    With the exactly rounded exponential instead, the rounding of exp(r) -- half
    an ulp per state, a perturbation of the input, not of the sweeps -- is
    amplified by the conditioning of the dominant eigenvector, up to ~1e-13 at
    rewards in [-6, 1]; that full error is what the GPU tests compare, as
    ``e_oracle``, because the device's exp differs from numpy's in the last bit,
    and it dominates their backward bounds.  So that it cannot drift unnoticed
    it is limited too, at the 32 x 32 cases here and at the GPU inputs
    (test_gpu_case_inputs_within_guards): below 1e-12, which is 2**-53 times an
    amplification of 1e4, three orders inside the suite's 1e-9.
    The forward pass (same sweep count, the oracle's policy) likewise."""
    c = _rescale_case(size, rng_range, seed, k_f)
    ref = X.backward(c["mats"], c["term"], c["r"], exp_reward=np.exp(c["r"]))
    e = X.elementwise_err(c["pi"], ref)
    e_svf = X.elementwise_err(c["svf"], c["svf_ref"])
    print(f"rescale {size}x{size} r in {rng_range}: e_oracle {e:.2e}, svf {e_svf:.2e}")
    assert e < 1e-14, e
    assert e_svf < 1e-13, e_svf
    if size == 32:
        e_unshared = X.elementwise_err(c["pi"], X.backward(c["mats"], c["term"], c["r"]))
        print(f"rescale {size}x{size} r in {rng_range}: e_oracle with the exact exp(r) {e_unshared:.2e}")
        assert e_unshared < 1e-12, e_unshared


def test_oracle_rescale_dense():
    """The same at a dense table (S = 300, A = 3: zs reaches 1e420)."""
    P, r, term, _ = O.random_dense_mdp(300, 3, seed=300)
    ref = X.backward(X.mats_from_table(P), term, r, exp_reward=np.exp(r))
    e = X.elementwise_err(O.backward_maxent(P, term, r, rescale=True), ref)
    print(f"rescale dense 300: e_oracle {e:.2e}")
    assert e < 1e-14, e


# ---------------------------------------------------------------------------
# the GPU tests' inputs stay inside the reference's guards
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["256x12", "256x8+stay", "ell200", "ell513"])
def test_gpu_case_inputs_within_guards(which):
    """The width-256 and ELL inputs of tests/test_gpu_elementwise.py: the
    unscaled backward stays normal in longdouble, converged soft VI leaves no
    start value, no SVF entry is exactly zero (nothing drops out of the
    elementwise comparison), and the oracle itself sits at rounding level."""
    if which.startswith("256"):
        case = C.stencil(256, int(which.split("+")[0][4:]), stay=which.endswith("stay"))
    else:
        case = C.ell(int(which[3:]))
        assert 3 <= case.k_row <= 12 and case.k_col <= 32, (case.k_row, case.k_col)
    for b in range(case.B):
        o, ref = case.backward(b)                       # raises if zs leaves the normal range
        assert (ref > 0).all()
        assert X.elementwise_err(o, ref) < 1e-12        # (exact exp(r): the unshared e_oracle)
        if which == "ell200" or (which == "ell513" and b == 0):   # (513: the same table for both instances)
            d, k, status, dref = case.forward(b, 3000)
            assert (dref > 0).all()
            assert X.elementwise_err(d, dref) < 1e-12
            pi, v, k, xpi, xv = case.soft(b, C.ELL_DISCOUNT)   # raises if a start value survives
            assert X.elementwise_err(pi, xpi) < 1e-12 and X.normwise_err(v, xv) < 1e-13


# ---------------------------------------------------------------------------
# the measure itself
# ---------------------------------------------------------------------------

def test_elementwise_measure_sees_what_max_norm_misses():
    """One small SVF entry (below 1e-9 of the largest) of the 32x32, r in [-6, 1]
    case off by a factor 1 + 1e-6: the max-norm ``close()`` of
    tests/test_gpu_parity.py passes it, ``elementwise_err`` reports 1e-6."""
    try:
        import test_gpu_parity
    except BaseException as e:   # (its own importorskip("torch") must not turn this test into a skip)
        pytest.fail(f"tests/test_gpu_parity.py does not import: {e!r}")
    c = _rescale_case(*RESCALE_CASES[1])
    ref = np.asarray(c["svf_ref"], dtype=np.float64)
    small = np.flatnonzero((ref > 0) & (ref < 1e-9 * ref.max()))
    assert small.size > 0
    bad = c["svf"].copy()
    bad[small[small.size // 2]] *= 1.0 + 1e-6
    test_gpu_parity.close(bad, ref, rtol=1e-9, what="perturbed svf")      # does not notice
    assert X.elementwise_err(c["svf"], c["svf_ref"]) < 1e-13
    assert 0.9e-6 < X.elementwise_err(bad, c["svf_ref"]) < 1.1e-6


def test_forward_condition_number():
    """extended_ref.forward's condition number is the first-order sensitivity to
    the edge weights: scaling every weight by 1 + eps (all errors of one sign,
    the worst case) changes the worst entry by eps * c, at a cap inside the
    first sweeps and where mass still lingers after 3,000."""
    case = C.stencil(16, 16)
    b, eps = 1, 2.0 ** -30
    pi = case.backward(b)[0]
    for k in (7, 3000):
        d, cond = X.forward(case.mats[b], case.p0[b], case.terminal, pi, k, with_condition=True)
        assert np.array_equal(d, X.forward(case.mats[b], case.p0[b], case.terminal, pi, k))
        moved = X.forward(case.mats[b], case.p0[b], case.terminal, pi * (1.0 + eps), k)
        assert 1.0 <= cond <= k
        assert abs(X.elementwise_err(moved, d) / (eps * cond) - 1.0) < 1e-5, k


def test_folded_forward_weights_explain_128x16():
    """Why the 3,000-sweep forward at 128 x 16 has a factor of its own in
    tests/test_gpu_elementwise.py (FORWARD_FACTOR_128x16 = 32).  The kernels
    fold the actions into one weight per edge, W[s, t] = sum_a pi[s, a] P_a[s, t],
    round it to float64 once and reuse it every sweep.  Here the sweeps are
    exact (longdouble) and only the folded weights are rounded to float64: the
    SVF of the point-start instance is then off by ~4.6e-14, 16 times the
    error of the oracle's float64 sweeps on unfolded operands, largest at a
    state beside the start that holds hundreds of visits -- the coherent term
    the condition number of extended_ref.forward predicts (far inside its
    worst case).  Folded weights plus the ordinary factor stay within 32."""
    import scipy.sparse as sp
    case = C.stencil(128, 16)
    b, k = 0, 3000
    d_oracle, k_ref, _, ref = case.forward(b, k)
    assert k_ref == k
    pi = case.backward(b)[0]
    keep = np.ones(case.S)
    keep[case.terminal] = 0.0                                       # maxent.py:98-99
    folded = None
    for a, m in enumerate(case.mats[b]):                            # float64 products, float64 action sum
        t = (sp.diags(keep * pi[:, a]) @ m).tocsr()
        folded = t if folded is None else folded + t
    wt = folded.T.tocsr().astype(np.longdouble)
    p0 = case.p0[b].astype(np.longdouble)
    d = np.zeros(case.S, dtype=np.longdouble)
    for _ in range(k):
        d = p0 + wt.dot(d)
    rel = np.abs(d - ref) / ref
    e_weights, at = float(rel.max()), int(rel.argmax())
    base = max(X.elementwise_err(d_oracle, ref), case.floor())
    cond = X.forward(case.mats[b], case.p0[b], case.terminal, pi, k, with_condition=True)[1]
    print(f"folded weights 128x16: e_weights {e_weights:.2e} = {e_weights / base:.1f} x max(e_oracle, e_floor), "
          f"at state {at} (svf {float(ref[at]):.0f}), condition {cond:.0f}")
    assert e_weights > 10 * base                                    # the oracle does not hold this term
    assert ref[at] > 100                                            # a large entry, not a small one
    assert e_weights <= case.A * 2.0 ** -53 * cond                  # inside the first-order worst case
    assert X.FACTOR + e_weights / base <= 32.0


def test_measures_reject_pattern_mismatch():
    ref = np.array([0.0, 1.0, 2.0], dtype=np.longdouble)
    assert X.elementwise_err(np.array([0.0, 1.0, 2.0]), ref) == 0.0
    with pytest.raises(AssertionError):
        X.elementwise_err(np.array([1e-300, 1.0, 2.0]), ref)              # nonzero where the reference is 0
    with pytest.raises(AssertionError):
        X.elementwise_err(np.array([0.0, np.nan, 2.0]), ref)
    with pytest.raises(AssertionError):
        X.normwise_err(np.array([0.0, np.inf, 2.0]), ref)
    assert X.normwise_err(np.array([0.0, 1.0, 2.5]), ref) == 0.25
    assert X.e_floor(5, 4) == 26 * 2.0 ** -53 and X.bound(0.0, 5, 4) == 16 * 26 * 2.0 ** -53


def test_guards_raise():
    mats = O.icy_gridworld_csr(16, 0.2)
    with pytest.raises(FloatingPointError):                               # e^(2 * 256 * (ln 4 + 30)) overflows
        X.backward(mats, [255], np.full(256, 30.0))
    with pytest.raises(FloatingPointError):                               # start values survive 3 sweeps
        X.soft_backward(mats, O.terminal_reward([255], 256), np.zeros(256), 0.9, 3)
