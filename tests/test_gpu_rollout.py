"""Demonstrations on the device (csrc/rollout.hip; needs an MI355X):
ops.rollout, ops.demo_statistics and ops.demo_log_likelihood bit for bit against
tests/rollout_twin.py, every trajectory status code on its guarded path, batch
independence, the round trip through stored trajectories, and the public layers
(demos.sample_device, BatchedMaxEnt.from_trajectories / log_likelihood).
tests/test_rollout_twin.py pins the twin itself without a device.

Shapes: B = 3 instances of N = 130 trajectories, so B * N = 390 crosses a
256-thread workgroup and ends in a partial wave; grids of 25, 21 and 36 states
and a 200-state ELL model.
"""

import functools

import numpy as np
import pytest

import elementwise_cases as C
import ell_cases as L
import maxent_oracle as O
import policy_eval_twin as T
import rollout_twin as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, N, SEED = 3, 130, 2024
ELL = "k5-s200"
#: model -> (W, H, stay) or the ELL slot form; step cap per model
STENCILS = {"5x5": (5, 5, False), "7x3": (7, 3, False), "6x6+stay": (6, 6, True)}
MODELS = tuple(STENCILS) + ("ell-sorted", "ell-scrambled")
MAX_LEN = {"5x5": 40, "7x3": 40, "6x6+stay": 48, "ell-sorted": 64, "ell-scrambled": 64}
KINDS = T.KINDS


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    import irlmx
    return irlmx.require_device()


def need_log():
    try:
        O.numpy_log_restated(np.ones(1))
    except OSError:
        pytest.skip("oracle/libblas_order.so not built: no restated numpy log to compare with")


# -- host inputs (shared, read-only) ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def host(model):
    """``(case, targets, row_val)``: per table the [K, S] slot targets and the
    [A, K, S] weights exactly as the device model holds them."""
    if model in STENCILS:
        W, H, stay = STENCILS[model]
        c = C.stencil(W, H, stay, B)
        rv = c.rv
        if stay:
            extra = np.zeros((B, 1, 5, c.S))
            extra[:, 0, 0] = 1.0
            rv = np.concatenate([rv, extra], axis=1)
        targets = [R.stencil_targets(W, H)] * B
        rvs = list(rv)
    else:
        c = L.case(ELL)
        assert c.B == B
        arrs = [L.host_arrays(c, b, model[4:]) for b in range(B)]
        targets, rvs = [a[0] for a in arrs], [a[1] for a in arrs]
    for a in list(targets) + list(rvs):
        a.setflags(write=False)
    return c, targets, rvs


def device_model(model, dev, tables=None, shared=False):
    from irlmx import DeviceMDP, _lib
    c, _, _ = host(model)
    if model not in STENCILS:
        return L.device_model(c, dev, form=model[4:], tables=tables, shared=shared)
    idx = list(range(B)) if tables is None else list(tables)
    rv = torch.as_tensor(np.ascontiguousarray(c.rv[idx]), dtype=torch.float64, device=dev)
    mdp = DeviceMDP(_lib.LAYOUT_STENCIL5, c.S, 4, len(idx), shared, rv, width=c.W, height=c.H, device=dev)
    return mdp.with_stay() if STENCILS[model][2] else mdp


@functools.lru_cache(maxsize=None)
def policy(model, kind):
    """[B, S, A]: policy_eval_twin's three kinds on this model's case."""
    c, _, _ = host(model)
    seed = 6100 + MODELS.index(model)
    if kind == "dirichlet":
        pi = np.random.default_rng(seed).dirichlet(np.ones(c.A), size=(B, c.S))
    elif kind == "greedy":
        r = np.random.default_rng(seed + 50).uniform(-1.0, 1.0, (B, c.S))
        pi = np.stack([T.greedy_policy(c.mats[b], r[b]) for b in range(B)])
    else:
        pi = np.stack([O.backward_maxent_csr(c.mats[b], c.terminal, c.reward[b]) for b in range(B)])
        assert np.isfinite(pi).all() and not np.array_equal(pi.sum(axis=2), np.ones((B, c.S)))   # not normalised, exactly
    pi = np.ascontiguousarray(pi, dtype=np.float64)
    pi.setflags(write=False)
    return pi


@functools.lru_cache(maxsize=None)
def starts(model):
    c, _, _ = host(model)
    st = np.random.default_rng(6300 + MODELS.index(model)).integers(0, c.S, (B, N))
    st[:, 0] = c.terminal[0]          # one start on a terminal in every instance
    st.setflags(write=False)
    return st


def term_mask(c):
    m = np.zeros(c.S, dtype=bool)
    m[c.terminal] = True
    return m


def run(mdp, pi, terminal, start, n, max_len, seed, trajectories=True):
    """ops.rollout as a dict of host numpy arrays; the device checks stay clean."""
    from irlmx import ops
    tm = ops.terminal_mask(list(terminal), mdp.n_states, batch=mdp.batch, device=mdp.device)
    out = ops.rollout(mdp, np.array(pi, order="C"), tm, start, n, max_len, seed, return_trajectories=trajectories)
    got = {k: (v.cpu().numpy() if v is not None else None) for k, v in out._asdict().items()}
    assert ops.device_check_failures() == 0
    return got


def twin(model, tables, pi, terminal, start, seeds, max_len):
    _, targets, rvs = host(model)
    mask = np.zeros(pi.shape[1], dtype=bool)
    mask[list(terminal)] = True
    return [R.rollout(targets[t], rvs[t], pi[b], mask, start[b], seeds[b], max_len) for b, t in enumerate(tables)]


def assert_equal(got, refs, what):
    for b, ref in enumerate(refs):
        for k, v in ref.items():
            assert got[k][b].dtype == v.dtype and np.array_equal(got[k][b], v), f"{what}: {k}[{b}] differs"


# -- 1. bit for bit against the twin --------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tables", ["own", "shared"])
@pytest.mark.parametrize("model", MODELS)
def test_matches_twin(dev, model, tables, kind):
    c, _, _ = host(model)
    if tables == "own":
        mdp, tabs = device_model(model, dev), list(range(B))
    else:
        mdp, tabs = device_model(model, dev, tables=[0], shared=True).with_batch(B), [0] * B
    pi, st, max_len = policy(model, kind), starts(model), MAX_LEN[model]
    got = run(mdp, pi, c.terminal, st, N, max_len, SEED)
    refs = twin(model, tabs, pi, c.terminal, st, R.instance_seeds(SEED, B), max_len)
    assert_equal(got, refs, f"{model} {tables} {kind}")
    assert got["states"].shape == (B, N, max_len + 1) and got["actions"].shape == (B, N, max_len)
    assert (got["lengths"][:, 0] == 0).all() and (got["status"][:, 0] == R.OK).all()      # the terminal starts
    assert got["lengths"].max() > 1
    if kind != "greedy":
        assert (got["status"] == R.OK).sum() > B                      # some trajectories reach a terminal
    total = got["visits"].sum(axis=1)
    assert np.array_equal(total, got["lengths"].sum(axis=1) + N + (got["status"] >= R.BAD_POLICY).sum(axis=1))


def test_without_trajectories(dev):
    c, _, _ = host("5x5")
    mdp = device_model("5x5", dev)
    pi, st = policy("5x5", "dirichlet"), starts("5x5")
    full = run(mdp, pi, c.terminal, st, N, 40, SEED)
    bare = run(mdp, pi, c.terminal, st, N, 40, SEED, trajectories=False)
    assert bare["states"] is None and bare["actions"] is None
    for k in ("visits", "starts", "lengths", "status"):
        assert np.array_equal(bare[k], full[k]), k
    again = run(mdp, pi, c.terminal, st, N, 40, SEED)                 # the same bits on every run
    for k in full:
        assert np.array_equal(again[k], full[k]), k
    other = run(mdp, pi, c.terminal, st, N, 40, SEED + 1)
    assert not np.array_equal(other["lengths"], full["lengths"])


# -- 2. every status code, each on its guarded path -----------------------------------------------

def test_truncated(dev):
    c, _, _ = host("5x5")
    mdp = device_model("5x5", dev, tables=[0])
    pi = policy("5x5", "dirichlet")[:1]
    st = np.zeros((1, N), dtype=np.int64)                             # 8 moves from the only terminal
    got = run(mdp, pi, [24], st, N, 3, SEED)
    assert (got["status"] == R.TRUNCATED).all() and (got["lengths"] == 3).all()
    assert (got["states"] >= 0).all() and (got["actions"] >= 0).all()
    assert got["visits"].sum() == 4 * N
    assert_equal(got, twin("5x5", [0], pi, [24], st, R.instance_seeds(SEED, 1), 3), "max_len 3")


def test_terminal_start(dev):
    c, _, _ = host("7x3")
    mdp = device_model("7x3", dev, tables=[1])
    t = c.terminal[1]
    got = run(mdp, policy("7x3", "maxent")[1:2], c.terminal, t, N, 40, 5)
    assert (got["status"] == R.OK).all() and (got["lengths"] == 0).all()
    assert got["visits"][0, t] == N and got["visits"].sum() == N and got["starts"][0, t] == N
    assert (got["states"][0, :, 0] == t).all() and (got["states"][0, :, 1:] == -1).all() and (got["actions"] == -1).all()


@pytest.mark.parametrize("fill", [0.0, float("nan"), -0.25])
def test_bad_policy_row(dev, fill):
    c, _, _ = host("5x5")
    mdp = device_model("5x5", dev, tables=[0])
    pi = policy("5x5", "dirichlet")[:1].copy()
    if fill == 0.0:
        pi[0, 0, :] = 0.0                                             # the whole row of the start state
    else:
        pi[0, 0, 2] = fill                                            # one NaN / negative entry in it
    st = np.zeros((1, N), dtype=np.int64)
    st[0, N // 2:] = 5                                                # (0, 1): some of these walk into state 0
    got = run(mdp, pi, c.terminal, st, N, 40, SEED)
    assert (got["status"][0, :N // 2] == R.BAD_POLICY).all() and (got["lengths"][0, :N // 2] == 0).all()
    assert (got["status"][0, N // 2:] == R.BAD_POLICY).any()
    assert got["visits"][0, 0] >= 2 * (N // 2)                        # counted at the step and as the final state
    assert_equal(got, twin("5x5", [0], pi, c.terminal, st, R.instance_seeds(SEED, 1), 40), f"policy row {fill}")


def test_bad_table_row(dev):
    from irlmx import DeviceMDP, _lib
    c, _, _ = host("ell-sorted")
    ri, rv, ci, cv = (np.array(x) for x in L.host_arrays(c, 0, "sorted"))
    s0 = 7
    assert s0 not in c.terminal
    rv[:, :, s0] = 0.0                                                # every action's row of the start state
    t = lambda x, dt: torch.as_tensor(x[None], dtype=dt, device=dev).contiguous()
    mdp = DeviceMDP(_lib.LAYOUT_ELL, c.S, c.A, 1, True, t(rv, torch.float64), row_idx=t(ri, torch.int32),
                    col_idx=t(ci, torch.int32), col_val=t(cv, torch.float64), k_row=ri.shape[0], k_col=ci.shape[0],
                    device=dev)
    pi = policy("ell-sorted", "dirichlet")[:1]
    got = run(mdp, pi, c.terminal, s0, N, 64, SEED)
    assert (got["status"] == R.BAD_TABLE).all() and (got["lengths"] == 0).all()
    assert got["visits"][0, s0] == 2 * N and got["visits"].sum() == 2 * N
    mask = term_mask(c)
    ref = R.rollout(ri, rv, pi[0], mask, np.full(N, s0), R.instance_seeds(SEED, 1)[0], 64)
    assert_equal(got, [ref], "zeroed table row")


def test_bad_start(dev):
    c, _, _ = host("5x5")
    mdp = device_model("5x5", dev)
    pi = policy("5x5", "dirichlet")
    st = np.array(starts("5x5"))
    st[0, :] = -1                                                     # a whole instance: nothing counted
    st[1, :] = c.S
    st[2, ::2] = np.where(np.arange(N)[::2] % 4 == 0, -1, c.S)        # mixed with good starts
    got = run(mdp, pi, c.terminal, st, N, 40, SEED)
    assert (got["status"][:2] == R.BAD_INDEX).all() and (got["lengths"][:2] == 0).all()
    assert got["visits"][:2].sum() == 0 and got["starts"][:2].sum() == 0
    assert (got["states"][:2] == -1).all() and (got["actions"][:2] == -1).all()
    assert (got["status"][2, ::2] == R.BAD_INDEX).all() and (got["status"][2, 1::2] <= R.TRUNCATED).all()
    assert got["starts"][2].sum() == N // 2
    assert_equal(got, twin("5x5", range(B), pi, c.terminal, st, R.instance_seeds(SEED, B), 40), "bad starts")
    good = run(mdp, pi, c.terminal, starts("5x5"), N, 40, SEED)       # the process goes on
    assert (good["status"] <= R.TRUNCATED).all()


# -- 3. batch independence ------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["7x3", "ell-scrambled"])
def test_batch_independence(dev, model):
    c, _, _ = host(model)
    pi, st, max_len = policy(model, "dirichlet"), starts(model), MAX_LEN[model]
    seeds = R.instance_seeds(SEED, B)
    full = run(device_model(model, dev), pi, c.terminal, st, N, max_len, SEED)
    one = run(device_model(model, dev, tables=[2]), pi[2:], c.terminal, st[2:], N, max_len, [seeds[2]])
    for k in full:
        assert np.array_equal(one[k][0], full[k][2]), k
    order = [2, 0]
    taken = run(device_model(model, dev).take(order), pi[order], c.terminal, st[order], N, max_len,
                [seeds[i] for i in order])
    for k in full:
        assert np.array_equal(taken[k], full[k][order]), k


# -- 4. round trip through stored trajectories ----------------------------------------------------

def test_statistics_round_trip(dev):
    from irlmx import ops
    for model in ("5x5", "ell-sorted"):
        c, _, _ = host(model)
        got = run(device_model(model, dev), policy(model, "maxent"), c.terminal, starts(model), N, MAX_LEN[model], SEED)
        assert (got["status"] <= R.TRUNCATED).all()
        visits, st, status = ops.demo_statistics(c.S, torch.as_tensor(got["states"], device=dev), got["lengths"])
        assert visits.dtype == torch.int64 and status.dtype == torch.int32
        assert (status.cpu().numpy() == R.OK).all()
        assert np.array_equal(visits.cpu().numpy(), got["visits"]) and np.array_equal(st.cpu().numpy(), got["starts"])
        assert ops.device_check_failures() == 0


def test_statistics_reference_fixture(dev):
    from irlmx import ops
    g = load_golden("config1")
    states, _, lengths = R.pack(g["traj_flat"], g["traj_lens"])
    visits, st, status = ops.demo_statistics(25, torch.as_tensor(states[None], device=dev), lengths[None])
    assert (status.cpu().numpy() == R.OK).all()
    v = visits.cpu().numpy()[0]
    assert np.array_equal(v / 200, g["e_features"]) and np.array_equal(v, np.rint(g["e_features"] * 200))
    assert np.array_equal(st.cpu().numpy()[0] / 200, g["p_initial"])


def test_statistics_guards(dev):
    from irlmx import ops
    states = np.array([[[0, 1, 2], [0, 3, -1], [0, 1, 1], [5, 0, 0], [2, -7, 9]]], dtype=np.int32)
    lengths = np.array([[2, 2, 3, 0, 0]])
    visits, st, status = ops.demo_statistics(4, torch.as_tensor(states, device=dev), lengths)
    ref = R.statistics(4, states[0], lengths[0])
    assert list(ref[2]) == [R.OK, R.BAD_INDEX, R.BAD_INDEX, R.BAD_INDEX, R.OK]
    for x, y in zip((visits, st, status), ref):
        assert np.array_equal(x.cpu().numpy()[0], y)
    assert ops.device_check_failures() == 0


# -- 5. log-likelihood ----------------------------------------------------------------------------

def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def test_log_likelihood_matches_twin(dev):
    from irlmx import ops
    need_log()
    c, _, _ = host("5x5")
    got = run(device_model("5x5", dev), policy("5x5", "dirichlet"), c.terminal, starts("5x5"), N, 40, SEED)
    pi = policy("5x5", "maxent").copy()                  # judged under another, unnormalised policy
    b0 = int(np.argmax(got["lengths"][0] > 0))
    pi[0, got["states"][0, b0, 0], got["actions"][0, b0, 0]] = 0.0     # a demonstrated action of probability 0
    ll, ll_traj, status = (x.cpu().numpy() for x in ops.demo_log_likelihood(
        pi, torch.as_tensor(got["states"], device=dev), got["actions"], got["lengths"]))
    assert (status == R.OK).all() and ll_traj[0, b0] == -np.inf and ll[0] == -np.inf
    assert np.isfinite(ll[1:]).all() and (ll_traj[:, 0] == 0.0).all()  # the terminal starts: empty sums
    for b in range(B):
        r_ll, r_traj, r_status = R.log_likelihood(pi[b], got["states"][b], got["actions"][b], got["lengths"][b])
        assert np.array_equal(bits(ll_traj[b]), bits(r_traj)) and bits(ll[b]) == bits(r_ll), b
        assert np.array_equal(status[b], r_status)
    assert ops.device_check_failures() == 0


def test_log_likelihood_reference_fixture(dev):
    from irlmx import ops
    need_log()
    g = load_golden("config1")
    states, actions, lengths = R.pack(g["traj_flat"], g["traj_lens"])
    for name in ("pi1", "cpi1"):                         # the MaxEnt and the causal policy of the first step
        pi = np.ascontiguousarray(g[name], dtype=np.float64)
        ll, ll_traj, status = (x.cpu().numpy() for x in ops.demo_log_likelihood(
            pi[None], torch.as_tensor(states[None], device=dev), actions[None], lengths[None]))
        r_ll, r_traj, r_status = R.log_likelihood(pi, states, actions, lengths)
        assert np.array_equal(bits(ll_traj[0]), bits(r_traj)) and bits(ll[0]) == bits(r_ll), name
        assert np.array_equal(status[0], r_status) and (status == R.OK).all()


def test_log_likelihood_guards(dev):
    from irlmx import ops
    states = np.array([[[0, 1, 2], [0, 3, -1], [0, 1, 1], [5, 0, 0], [0, 1, 2]]], dtype=np.int32)
    actions = np.array([[[0, 1], [2, 0], [0, 0], [0, 0], [0, 3]]], dtype=np.int32)
    lengths = np.array([[2, 1, 3, 0, 2]])
    pi = np.full((1, 4, 3), 0.25)
    ll, ll_traj, status = (x.cpu().numpy() for x in ops.demo_log_likelihood(
        pi, torch.as_tensor(states, device=dev), actions, lengths))
    assert list(status[0]) == [R.OK, R.OK, R.BAD_INDEX, R.BAD_INDEX, R.BAD_INDEX]   # length 3 > L, state 5, action 3
    assert np.isfinite(ll_traj[0, :2]).all() and np.isnan(ll_traj[0, 2:]).all() and np.isnan(ll[0])
    assert ops.device_check_failures() == 0


# -- 6. the public layers -------------------------------------------------------------------------

SIZE, NB, ND = 8, 4, 64
SLIPS = (0.1, 0.2, 0.3, 0.15)


def test_sample_device(dev):
    from irlmx import DeviceMDP, demos
    mdp = DeviceMDP.icy_gridworld(SIZE, SLIPS, device=dev)
    S = SIZE * SIZE
    e, p0, lengths = demos.sample_device(mdp, [S - 1], 0, n=ND, seed=11)
    assert e.shape == (NB, S) and e.dtype == torch.float64 and lengths.shape == (NB, ND)
    counts = (e * ND).cpu().numpy()
    assert np.array_equal(counts, np.rint(counts))
    assert np.array_equal(counts.sum(axis=1), lengths.cpu().numpy().sum(axis=1) + ND)
    assert np.array_equal(p0.cpu().numpy()[:, 0], np.ones(NB)) and float(p0.sum()) == NB
    rv = mdp.row_val.cpu().numpy()
    mask = np.zeros(S, dtype=bool)
    mask[S - 1] = True
    pol = demos.expert_policy(SIZE, S - 1)
    for b, seed in enumerate(R.instance_seeds(11, NB)):
        ref = R.rollout(R.stencil_targets(SIZE, SIZE), rv[b], pol, mask, np.zeros(ND, dtype=np.int64), seed,
                        demos.safety_cap(SIZE))
        assert np.array_equal(counts[b], ref["visits"]) and np.array_equal(lengths[b].cpu().numpy(), ref["lengths"])
    with pytest.raises(demos.TruncatedDemonstrations):
        demos.sample_device(mdp, [S - 1], 0, n=ND, seed=11, max_len=5)
    cut = demos.sample_device(mdp, [S - 1], 0, n=ND, seed=11, max_len=5, on_truncate="allow")
    assert int(cut[2].max()) == 5
    with pytest.raises(ValueError, match="status 4"):
        demos.sample_device(mdp, [S - 1], S, n=ND, seed=11)


@pytest.fixture(scope="module")
def stored(dev):
    """The 8x8 model, its expert demonstrations with stored trajectories, the terminal list."""
    from irlmx import DeviceMDP, demos, ops
    mdp = DeviceMDP.icy_gridworld(SIZE, SLIPS, device=dev)
    S = SIZE * SIZE
    pol = torch.as_tensor(demos.expert_policy(SIZE, S - 1), device=dev).unsqueeze(0).expand(NB, S, 4)
    out = ops.rollout(mdp, pol, ops.terminal_mask([S - 1], S, batch=NB, device=dev), 0, ND, demos.safety_cap(SIZE), 11,
                      return_trajectories=True)
    assert int(out.status.max()) == R.OK
    return mdp, out, [S - 1]


def test_from_trajectories(dev, stored):
    from irlmx.batch import BatchedMaxEnt
    mdp, out, terminal = stored
    a = BatchedMaxEnt.from_trajectories(mdp, out.states, out.lengths, terminal)
    e, p0 = out.visits.to(torch.float64) / ND, out.starts.to(torch.float64) / ND
    assert torch.equal(a.e_features, e) and torch.equal(a.p_initial, p0)
    b = BatchedMaxEnt(mdp, e, p0, terminal)
    a.run(max_steps=6)
    b.run(max_steps=6)
    assert a.k == b.k == 6 and L.same_bits(a.theta, b.theta)
    f = torch.as_tensor(np.random.default_rng(3).uniform(0, 1, (SIZE * SIZE, 5)), device=dev)
    withf = BatchedMaxEnt.from_trajectories(mdp, out.states, out.lengths, terminal, features=f, lr0=0.1)
    assert withf.e_features.shape == (NB, 5) and torch.equal(withf.e_features, e @ f) and withf.lr0 == 0.1
    bad = out.states.clone()
    bad[1, 3, 0] = SIZE * SIZE
    with pytest.raises(ValueError, match="1 of 256"):
        BatchedMaxEnt.from_trajectories(mdp, bad, out.lengths, terminal)


def test_batched_log_likelihood(dev, stored):
    from irlmx import ops
    from irlmx.batch import BatchedMaxEnt
    mdp, out, terminal = stored
    m = BatchedMaxEnt.from_trajectories(mdp, out.states, out.lengths, terminal)
    m.run(max_steps=3)
    m.active[1] = False
    assert m.compact() == NB - 1                                      # a compacted working set
    before = (m.theta.clone(), m.k, m.active.clone(), m._work, m.steps.clone())
    ll = m.log_likelihood(out.states, out.actions, out.lengths)
    assert L.same_bits(m.theta, before[0]) and m.k == before[1] and torch.equal(m.active, before[2])
    assert m._work is before[3] and torch.equal(m.steps, before[4]) and m.working_batch == NB - 1
    pi = ops.backward_maxent(mdp, m.reward(), m.terminal)             # all instances, original order
    ref, ref_traj, status = ops.demo_log_likelihood(pi, out.states, out.actions, out.lengths)
    assert int(status.max()) == R.OK and ll.shape == (NB,) and L.same_bits(ll, ref / ND)
    assert bool(torch.isfinite(ll).all()) and bool((ll < 0).all())
