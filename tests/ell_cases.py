"""Inputs of the ELL instantiation-matrix tests (not a test module).

tests/test_gpu_ell_matrix.py runs generic sparse (ELL) models with per-instance
tables through every fused (states per thread, slot class) instantiation the
planner admits, its fallbacks and the persistent grid shape;
tests/test_ell_cases.py checks, without a GPU, that these inputs are what they
claim to be and stay inside the extended reference's guards.

One generator (``table``) in the spirit of test_gpu_full_size.random_sparse_mats:
state s reaches targets (s + o) mod S with o from one fixed set of ``n_offsets``
offsets (so no state has more than ``n_offsets`` sources), the row length drawn
per state from lo..hi; one state has every offset (k_row is exactly hi) and one
target has every source (k_col is exactly n_offsets).  Each action is a random
distribution over a random subset of the row's targets.  Every table also
holds, by name (``Table.named``):

* ``single``    a state with one successor;
* ``empty``     (state, action): a non-terminal state where that action's row is
                entirely zero and the other actions' rows are not -- the policy
                entry is an exact 0 in the reference (None at A = 1, where an
                empty row would be a 0 / 0 policy row);
* ``nosource``  a state no state transitions into: its SVF is its p0 entry, bit
                for bit, at every cap.

No state is absorbing and every state reaches a terminal.  Everything is
seeded; the cases are elementwise_cases.Case objects on the CSR oracle
(``tables=None``) and share its cached references.

Two slot layouts of the same matrices (``ell_arrays``): the one
irlmx_dense_to_ell produces (targets / sources ascending, unused slots at the
end pointing at the state itself), and a scrambled one that uses what
include/irlmx.h leaves open ("unused slots have value 0"): slots in a random
order per state, two slots more than needed, the unused ones at random
positions pointing at some other valid state.
"""

import functools

import numpy as np

import elementwise_cases as C

DISCOUNT = C.ELL_DISCOUNT        # soft VI and VI: converged in ~2,000 / ~30 sweeps
CAPS = (7, 500)                  # forward caps: too few sweeps for the folded-weight term to build up
REWARD_RANGE = (-1.2, -0.2)
SCRAMBLE_PAD = 2

#: name -> (S, A, B, lo, hi, n_offsets, hub).  ``hub``: every state also reaches
#: that state (itself included), so k_col = S beside a small k_row.
SPECS = {
    "k5-s200": (200, 4, 3, 2, 5, 5, None),
    "k8-s200": (200, 1, 2, 2, 8, 8, None),
    "k32-s200": (200, 8, 2, 2, 32, 32, None),
    "k40-s300": (300, 3, 2, 2, 40, 40, None),
    "hub-s200": (200, 3, 2, 2, 7, 7, 7),
    "k5-s1029": (1029, 3, 2, 2, 5, 5, None),
    "k8-s1029": (1029, 3, 2, 2, 8, 8, None),
    "k16-s1029": (1029, 3, 2, 2, 16, 16, None),
    "k5-s2049": (2049, 2, 2, 2, 5, 5, None),
    "k8-s2049": (2049, 2, 2, 2, 8, 8, None),
}
NAMES = tuple(SPECS)


def slot_class(k):
    return 5 if k <= 5 else 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 0


#: the slot classes (k_row, k_col) each case must fall in exactly, from its spec: 5 is 1..5, 8
#: is 6..8, 16 is 9..16, 32 is 17..32, 0 is above 32 (no register-resident form)
CLASSES = {name: (slot_class(hi + (hub is not None)), slot_class(S if hub is not None else n_offsets))
           for name, (S, A, B, lo, hi, n_offsets, hub) in SPECS.items()}

OPS = ("backward", "forward", "soft_backward", "value_iteration")
_ = None   # one launch per sweep
#: The fused instantiation <SPT, KMAX> each pass of each case reaches on the
#: default plan, None for the per-sweep shape: written out by hand, derived
#: from fused_shape / fused_pair_ok (csrc/fixed_point.hip, .h).  plan() below restates
#: the planner; tests/test_ell_cases.py holds the two against each other, the GPU
#: test holds the device's plan against this table.
FUSED = {
    #              backward  forward   soft_backward  value_iteration
    "k5-s200":   ((1, 5),   (1, 5),   (1, 5),        (1, 5)),
    "k8-s200":   ((1, 8),   (1, 8),   (1, 8),        (1, 8)),
    "k32-s200":  ((1, 32),  (1, 32),  _,             (1, 32)),
    "k40-s300":  (_,        _,        _,             _),
    "hub-s200":  ((1, 8),   _,        (1, 8),        (1, 8)),
    "k5-s1029":  ((2, 5),   (2, 5),   (2, 5),        (2, 5)),
    "k8-s1029":  ((2, 8),   (2, 8),   _,             (2, 8)),
    "k16-s1029": ((2, 16),  (2, 16),  _,             _),
    "k5-s2049":  ((4, 5),   (4, 5),   _,             (4, 5)),
    "k8-s2049":  (_,        _,        _,             (4, 8)),
}
#: under IRLMX_FUSED_MAX_STATES=0: workgroups per instance on the persistent grid
#: shape (256 states each), None for the per-sweep shape
GRID = {
    "k8-s1029": (5, 5, 5, 5),        # the last workgroup holds 5 states
    "k32-s200": (1, 1, _, _),        # A = 8 > kGridMaxActions: soft VI and VI per sweep
    "k40-s300": (_, _, _, _),
}

# -- the planner, restated (csrc/fixed_point.h: slot_class, fused_pair_ok; csrc/fixed_point.hip: fused_shape;
#    csrc/grid.hip: grid_plan; csrc/extended.hip takes the backward's list) -------------------

FUSED_MAX_STATES, MAX_ACTIONS, GRID_MAX_ACTIONS, GRID_THREADS, WAVE = 4096, 8, 5, 256, 64
_LINEAR = {5: (1, 2, 4), 8: (1, 2), 16: (1, 2), 32: (1,)}
PAIRS = {"backward": _LINEAR, "forward": _LINEAR,
         "soft_backward": {5: (1, 2), 8: (1,), 16: (1,)},
         "value_iteration": {5: (1, 2, 4), 8: (1, 2, 4), 16: (1,), 32: (1,)}}


def plan(S, A, k_row, k_col, op, fused_max=FUSED_MAX_STATES):
    """The plan fields the device must report for ``op``: shape, and for the
    fused shape spt and threads, for the grid shape spt, threads and C (with the
    whole batch co-resident, which every case here is)."""
    kmax = slot_class(k_col if op == "forward" else k_row)
    if S <= fused_max and A <= MAX_ACTIONS:
        spt = 1
        while (S + spt - 1) // spt > 1024:
            spt *= 2
        if spt in PAIRS[op].get(kmax, ()):
            per = (S + spt - 1) // spt
            return {"shape": "fused", "spt": spt, "threads": min(1024, (per + WAVE - 1) // WAVE * WAVE)}
    elif S > fused_max:
        bellman = op in ("soft_backward", "value_iteration")
        if kmax and (kmax <= 16 and A <= GRID_MAX_ACTIONS if bellman else A <= MAX_ACTIONS):
            return {"shape": "grid", "spt": 1, "threads": GRID_THREADS, "C": (S + GRID_THREADS - 1) // GRID_THREADS}
    return {"shape": "sweep"}


def fused_pair(p, k):
    """(SPT, KMAX) of a fused plan, None otherwise -- the form of FUSED."""
    return (p["spt"], slot_class(k)) if p["shape"] == "fused" else None


# -- the generator ---------------------------------------------------------------------------

class Table:
    """Per-action CSR matrices of one table and its named states."""

    def __init__(self, mats, named):
        self.mats, self.named = mats, named


def table(S, A, lo, hi, n_offsets, seed, hub=None):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    offsets = rng.choice(np.arange(1, S), n_offsets, replace=False)
    empty_action = None
    avoid = {0, 2, S - 1} | ({hub} if hub is not None else set())   # the delta of p0, the terminals, the hub
    while True:
        full, single, empty, nosource, target = (int(x) for x in rng.choice(S, 5, replace=False))
        into_nosource = {int((nosource - o) % S) for o in offsets}
        into_target = {int((target - o) % S) for o in offsets}
        if {full, single, empty, nosource, target} & avoid:
            continue
        if full in into_nosource or single in into_target:
            continue
        if hub is not None and hub in {int((full + o) % S) for o in offsets}:
            continue   # (the hub is the row's hi + 1-th target)
        break
    must = [set() for _ in range(S)]   # offsets a state must / must not use
    never = [set() for _ in range(S)]
    for j, o in enumerate(offsets):
        must[(target - o) % S].add(j)       # every possible source of `target` is one
        never[(nosource - o) % S].add(j)    # nobody reaches `nosource`
    must[full] = set(range(n_offsets))
    rows, cols = [], []
    vals = [[] for _ in range(A)]
    rows_a = [[] for _ in range(A)]
    cols_a = [[] for _ in range(A)]
    for s in range(S):
        n = int(rng.integers(lo, hi + 1))
        if s == single:
            n = 0 if hub is not None else 1
        free = [j for j in rng.permutation(n_offsets) if j not in must[s] and j not in never[s]]
        use = sorted(must[s]) + free[:max(0, n - len(must[s]))]
        tg = {int((s + offsets[j]) % S) for j in use}
        if hub is not None:
            tg.add(hub)
        tg = np.array(sorted(tg))
        n = tg.size
        m = rng.random((A, n)) < 0.5
        m[np.arange(A), rng.integers(0, n, A)] = True        # at least one target per action
        live = np.arange(A)
        if A > 1 and s == empty:
            empty_action = int(rng.integers(0, A))
            m[empty_action] = False
            live = np.delete(live, empty_action)
        for j in np.flatnonzero(~m.any(axis=0)):             # the row is the union over the actions
            m[rng.choice(live), j] = True
        w = (rng.random((A, n)) + 0.05) * m
        tot = w.sum(axis=1, keepdims=True)
        w = np.divide(w, tot, out=np.zeros_like(w), where=tot > 0)
        for a in range(A):
            nz = m[a]
            rows_a[a].append(np.full(int(nz.sum()), s))
            cols_a[a].append(tg[nz])
            vals[a].append(w[a][nz])
    mats = []
    for a in range(A):
        mat = sp.csr_matrix((np.concatenate(vals[a]), (np.concatenate(rows_a[a]), np.concatenate(cols_a[a]))),
                            shape=(S, S))
        mat.sort_indices()
        mats.append(mat)
    return Table(mats, {"full": full, "single": single, "empty": (empty, empty_action) if A > 1 else None,
                        "nosource": nosource, "target": target})


def union(mats):
    u = sum(abs(m) for m in mats).tocsr()
    u.sort_indices()
    return u


def slot_counts(mats):
    """(k_row, k_col): the largest number of targets of a state and of sources of
    a state, over the union of the actions."""
    u = union(mats)
    return int(np.diff(u.indptr).max()), int(np.diff(u.T.tocsr().indptr).max())


def reaches_terminal(mats, terminal):
    """Whether every state reaches a terminal (and so no state is absorbing)."""
    ut = union(mats).T.tocsr()
    seen = np.zeros(ut.shape[0], bool)
    seen[terminal] = True
    front = np.array(terminal)
    while front.size:
        nxt = np.unique(np.concatenate([ut.indices[ut.indptr[t]:ut.indptr[t + 1]] for t in front]))
        front = nxt[~seen[nxt]]
        seen[front] = True
    return bool(seen.all())


def _seed(name, b):
    return 9000 + 100 * NAMES.index(name) + b


@functools.lru_cache(maxsize=None)
def case(name):
    """The named case: a elementwise_cases.Case with B per-instance tables
    (different seeds), ``case.k_col``, ``case.named[b]`` and ``case.classes``."""
    S, A, B, lo, hi, n_offsets, hub = SPECS[name]
    tabs = [table(S, A, lo, hi, n_offsets, _seed(name, b), hub) for b in range(B)]
    counts = {slot_counts(t.mats) for t in tabs}
    assert len(counts) == 1, (name, counts)           # every table is exact, so they agree
    (k_row, k_col), = counts
    rng = np.random.default_rng(_seed(name, 99))
    reward = rng.uniform(*REWARD_RANGE, (B, S))
    c = C.Case(name, [t.mats for t in tabs], None, reward, C._p0(rng, B, S), [S - 1, 2], k_row, A)
    c.k_col, c.named, c.classes = k_col, [t.named for t in tabs], CLASSES[name]
    return c


def numpy_order_reward(c):
    """The case's rewards shifted per instance by -log(A * mean(exp(r))), so that
    the partition values of the *unscaled* backward (the numpy-order entry point
    does not rescale, like the reference) neither grow nor decay on average per
    sweep and stay finite and nonzero in float64 over all 2 * S sweeps.  (With
    the case's own rewards A * exp(r) is ~1.55 per sweep at A = 3: float64
    overflows within the 2,058 sweeps of 1,029 states.)"""
    return c.reward - np.log(c.A * np.exp(c.reward).mean(axis=1, keepdims=True))


def expected_plan(c, op, fused_max=FUSED_MAX_STATES, pad=0):
    """plan() of case c with ``pad`` slots more than needed (the scrambled form).
    ``op="extended"`` (ops.backward_maxent_extended): fused wherever the
    backward's pair is (it takes the backward's list; 24 B of LDS per state
    fit at every size here), else one launch per sweep -- it has no grid form."""
    p = plan(c.S, c.A, c.k_row + pad, c.k_col + pad, "backward" if op == "extended" else op, fused_max)
    return {"shape": "sweep"} if op == "extended" and p["shape"] != "fused" else p


# -- slot layouts ----------------------------------------------------------------------------

def ell_arrays(mats, k_row, k_col, scramble=None):
    """Host ELL arrays of one table: (row_idx [k_row, S] int32, row_val
    [A, k_row, S], col_idx [k_col, S] int32, col_val [A, k_col, S]).

    ``scramble=None``: irlmx_dense_to_ell's layout (ascending, unused slots last,
    pointing at the state itself).  A seed: every state's slots in a random order
    of their own, unused slots anywhere, each pointing at a random state other
    than the row's own (value 0)."""
    n, A = mats[0].shape[0], len(mats)
    rng = None if scramble is None else np.random.default_rng(scramble)

    def form(u, ms, k):
        cnt = np.diff(u.indptr)
        assert cnt.max() <= k, (int(cnt.max()), k)
        rows = np.repeat(np.arange(n), cnt)
        nth = np.arange(u.indices.size) - np.repeat(u.indptr[:-1], cnt)     # entry number within its row
        if rng is None:
            slot = nth
            idx = np.tile(np.arange(n), (k, 1))
        else:
            order = np.argsort(rng.random((n, k)), axis=1)                   # a permutation of the slots per state
            slot = order[rows, nth]
            idx = (np.arange(n)[None, :] + rng.integers(1, n, (k, n))) % n   # never the state itself
        idx[slot, rows] = u.indices
        val = np.zeros((A, k, n))
        for a, m in enumerate(ms):
            val[a, slot, rows] = np.asarray(m[rows, u.indices]).reshape(-1)
        return idx.astype(np.int32), val

    u = union(mats)
    ri, rv = form(u, mats, k_row)
    ut = u.T.tocsr()
    ut.sort_indices()
    ci, cv = form(ut, [m.T.tocsr() for m in mats], k_col)
    return ri, rv, ci, cv


def expand(idx, val, transpose=False):
    """The per-action CSR matrices a slot form describes (slots naming the same
    state add up; ``transpose``: a column form)."""
    import scipy.sparse as sp
    k, n = idx.shape
    rows = np.tile(np.arange(n), k)
    out = []
    for a in range(val.shape[0]):
        m = sp.coo_matrix((val[a].reshape(-1), (rows, idx.reshape(-1).astype(np.int64))), shape=(n, n)).tocsr()
        m.eliminate_zeros()
        out.append(m.T.tocsr() if transpose else m)
    return out


def scramble_seed(name, b):
    return _seed(name, 50 + b)


def host_arrays(c, b, form):
    """ell_arrays of table b of case c in the "sorted" or the "scrambled" form."""
    if form == "sorted":
        return ell_arrays(c.mats[b], c.k_row, c.k_col)
    assert form == "scrambled", form
    return ell_arrays(c.mats[b], c.k_row + SCRAMBLE_PAD, c.k_col + SCRAMBLE_PAD, scramble=scramble_seed(c.name, b))


# -- device side (torch and irlmx are imported here only) ------------------------------------------

def device_model(c, dev, form="sorted", tables=None, shared=False):
    """A DeviceMDP(LAYOUT_ELL) holding the given tables of case c (all of them by
    default) as per-instance tables, or one table shared (``shared=True``)."""
    import torch
    from irlmx import DeviceMDP, _lib
    tables = list(range(c.B)) if tables is None else list(tables)
    assert not shared or len(tables) == 1
    ri, rv, ci, cv = (np.stack(x) for x in zip(*[host_arrays(c, b, form) for b in tables]))
    t = lambda x, dt: torch.as_tensor(x, dtype=dt, device=dev).contiguous()
    return DeviceMDP(_lib.LAYOUT_ELL, c.S, c.A, len(tables), shared, t(rv, torch.float64),
                     row_idx=t(ri, torch.int32), col_idx=t(ci, torch.int32), col_val=t(cv, torch.float64),
                     k_row=ri.shape[1], k_col=ci.shape[1], device=dev)


PASSES = ("backward", "extended", "forward7", "forward500", "soft", "vi_max", "vi_avg")


def run_passes(c, mdp, tables=None, passes=PASSES):
    """Every pass on ``mdp`` with the inputs of the given instances of case c (the
    forward on the oracle's float64 policy): {pass: tuple of host tensors}."""
    import torch
    from irlmx import ops
    idx = list(range(c.B)) if tables is None else list(tables)
    n = len(idx)
    assert mdp.batch == n
    tm = ops.terminal_mask(c.terminal, c.S, batch=n, device=mdp.device)
    r = c.reward[idx].copy()
    out = {}
    for p in passes:
        if p == "backward":
            res = (ops.backward_maxent(mdp, r, tm),)
        elif p == "extended":
            res = (ops.backward_maxent_extended(mdp, r, tm),)
        elif p.startswith("forward"):
            pi = np.stack([c.backward(b)[0] for b in idx])
            res = ops.forward_svf(mdp, c.p0[idx].copy(), tm, pi, max_iter=int(p[7:]))
        elif p == "soft":
            res = ops.soft_backward(mdp, r, np.tile(c.phi, (n, 1)), DISCOUNT)
        else:
            res = ops.value_iteration(mdp, r, DISCOUNT, average=p == "vi_avg")
        out[p] = tuple(x.cpu() for x in res)
    torch.cuda.synchronize(mdp.device)
    return out


def same_bits(x, y):
    import torch
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
    return x.shape == y.shape and x.dtype == y.dtype and bool(torch.equal(bits(x), bits(y)))


def assert_same(got, ref, what, rows=None):
    """Every tensor of every pass of ``got`` equals ``ref``'s (rows ``rows`` of it), bit for bit."""
    assert got.keys() <= ref.keys(), (got.keys(), ref.keys())
    for p, res in got.items():
        for i, (x, y) in enumerate(zip(res, ref[p])):
            y = y if rows is None else y[list(rows)]
            assert same_bits(x, y), f"{what}: {p}[{i}] differs"
