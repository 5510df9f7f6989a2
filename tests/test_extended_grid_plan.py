"""The planner of the extended-range backward's persistent grid shape
(csrc/extended.hip: ext_grid_plan), without a GPU: the plan and the workspace
are queried through the C ABI with IRLMX_PLAN_CUS x IRLMX_PLAN_GRID_PER_CU
standing in for the device's capacity, so no HIP call is made.

Order of the shapes: fused, grid (from 8,192 states on, an absolute floor;
IRLMX_EXT_GRID_MIN_STATES), per sweep.  Plan fields of the grid shape:
[0] 5, [2] XCD grouping, [3] workgroups per instance, [4] instances per launch,
[5] states per thread, [7] 256 threads, [8] sequential launches.
"""

import ctypes

import pytest

from test_abi_errors import err, model

OP_BACKWARD, EXTENDED = 1, 0x200
KEYS = ("IRLMX_GRID", "IRLMX_FUSED_MAX_STATES", "IRLMX_EXT_GRID_MIN_STATES", "IRLMX_EXT_GRID_MAX_LAUNCHES",
        "IRLMX_PLAN_CUS", "IRLMX_PLAN_GRID_PER_CU", "IRLMX_XCD_GROUP")
SMALL = {"IRLMX_EXT_GRID_MIN_STATES": 0, "IRLMX_FUSED_MAX_STATES": 0}
ELL = dict(layout=2, k_col=3, row_idx=True, col_idx=True, col_val=True)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from irlmx import _lib
    return _lib.load()


@pytest.fixture
def env(monkeypatch):
    """Exactly the given keys, on a planned capacity of `cap` workgroups."""
    def set_env(cap=256, **values):
        for k in KEYS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("IRLMX_PLAN_CUS", str(cap))
        monkeypatch.setenv("IRLMX_PLAN_GRID_PER_CU", "1")
        for k, v in values.items():
            assert k in KEYS, k
            monkeypatch.setenv(k, str(v))
    set_env()
    return set_env


def plan_of(lib, m):
    plan = (ctypes.c_int64 * 10)()
    assert lib.irlmx_execution_plan(ctypes.byref(m), OP_BACKWARD | EXTENDED, plan) == 0, err(lib)
    return list(plan)


def grid(bpi, spt=1, ipl=1, launches=1, xcd=0):
    return [5, 0, xcd, bpi, ipl, spt, 0, 256, launches, 0]


def sweep(S):
    return [2, 0, 0, 0, 0, 1, 0, 256, 2 * S - 1, 0]


def stencil(W, H, **kw):
    return model(S=W * H, W=W, H=H, **kw)


def test_floor_at_default_keys(lib, env):
    assert plan_of(lib, stencil(128, 64)) == grid(bpi=32)              # S = 8,192: one launch
    assert plan_of(lib, stencil(127, 64)) == sweep(127 * 64)           # S = 8,128
    assert plan_of(lib, stencil(128, 33)) == [2, 0, 0, 0, 0, 1, 0, 256, 8447, 0]
    assert plan_of(lib, stencil(64, 64)) == [0, 0, 0, 0, 0, 4, 0, 1024, 1, 24 * 4096]   # fused comes first


def test_floor_does_not_follow_the_fused_limit(lib, env):
    env(IRLMX_FUSED_MAX_STATES=0)
    assert plan_of(lib, stencil(128, 33)) == sweep(128 * 33)
    assert plan_of(lib, stencil(64, 4)) == sweep(256)
    assert plan_of(lib, stencil(128, 64)) == grid(bpi=32)


def test_grid_key_off(lib, env):
    env(IRLMX_GRID=0)
    assert plan_of(lib, stencil(128, 64)) == sweep(8192)
    env(IRLMX_GRID=0, **SMALL)
    assert plan_of(lib, stencil(37, 23)) == sweep(851)


def test_small_sizes_through_the_keys(lib, env):
    env(**SMALL)
    assert plan_of(lib, stencil(64, 4)) == grid(bpi=1)                 # S = 256: one full workgroup
    assert plan_of(lib, stencil(37, 23)) == grid(bpi=4)                # S = 851
    env(IRLMX_EXT_GRID_MIN_STATES=0)                                   # the fused shape still comes first
    assert plan_of(lib, stencil(37, 23))[0] == 0


def test_capacity_moves_states_per_thread(lib, env):
    for cap, want in ((4, grid(bpi=4)), (3, grid(bpi=2, spt=2)), (2, grid(bpi=2, spt=2)), (1, grid(bpi=1, spt=4))):
        env(cap, **SMALL)
        assert plan_of(lib, stencil(37, 23)) == want, cap
    env(1, **SMALL)
    assert plan_of(lib, stencil(41, 25)) == sweep(1025)                # 1,025 states: two workgroups even at spt 4


def test_ell_slot_classes(lib, env):
    env(1, **SMALL)                                                    # S = 512 on one workgroup: two states per thread
    for k in (40, 32, 16):
        assert plan_of(lib, model(S=512, k_row=k, **ELL)) == sweep(512), k
    for k in (8, 6):
        assert plan_of(lib, model(S=512, k_row=k, **ELL)) == grid(bpi=1, spt=2), k
    env(2, **SMALL)
    assert plan_of(lib, model(S=512, k_row=16, **ELL)) == grid(bpi=2)
    assert plan_of(lib, model(S=512, k_row=9, **ELL)) == grid(bpi=2)
    for k in (17, 32, 40):
        assert plan_of(lib, model(S=512, k_row=k, **ELL)) == sweep(512), k
    env(1, **SMALL)                                                    # four states per thread: the 5-slot class only
    assert plan_of(lib, model(S=1024, k_row=5, **ELL)) == grid(bpi=1, spt=4)
    assert plan_of(lib, model(S=1024, k_row=8, **ELL)) == sweep(1024)


def test_sequential_launches_and_cap(lib, env):
    m = stencil(37, 23, B=3, shared=0)
    for cap, ipl, launches in ((4, 1, 3), (7, 1, 3), (8, 2, 2), (11, 2, 2), (12, 3, 1)):
        env(cap, IRLMX_EXT_GRID_MAX_LAUNCHES=3, **SMALL)
        assert plan_of(lib, m) == grid(bpi=4, ipl=ipl, launches=launches), cap
    # above the cap: more states per thread (fewer workgroups per instance), and per sweep when nothing fits
    env(4, IRLMX_EXT_GRID_MAX_LAUNCHES=2, **SMALL)
    assert plan_of(lib, m) == grid(bpi=2, spt=2, ipl=2, launches=2)
    env(8, IRLMX_EXT_GRID_MAX_LAUNCHES=1, **SMALL)
    assert plan_of(lib, m) == grid(bpi=2, spt=2, ipl=3, launches=1)
    env(4, IRLMX_EXT_GRID_MAX_LAUNCHES=1, **SMALL)
    assert plan_of(lib, m) == grid(bpi=1, spt=4, ipl=3, launches=1)
    env(2, IRLMX_EXT_GRID_MAX_LAUNCHES=1, **SMALL)
    assert plan_of(lib, m) == sweep(851)
    env(1, IRLMX_EXT_GRID_MAX_LAUNCHES=2, **SMALL)
    assert plan_of(lib, m) == sweep(851)
    env(1, IRLMX_EXT_GRID_MAX_LAUNCHES=3, **SMALL)
    assert plan_of(lib, m) == grid(bpi=1, spt=4, ipl=1, launches=3)
    env(12, IRLMX_EXT_GRID_MAX_LAUNCHES=0, **SMALL)                    # the shape switched off by its cap
    assert plan_of(lib, stencil(37, 23)) == sweep(851)


def test_default_cap_is_one_launch(lib, env):
    env(4, **SMALL)
    assert plan_of(lib, stencil(37, 23, B=2, shared=0)) == grid(bpi=2, spt=2, ipl=2)
    env(1, **SMALL)
    assert plan_of(lib, stencil(37, 23, B=2, shared=0)) == sweep(851)


def test_two_workgroups_per_cu_without_xcd_groups(lib, env, monkeypatch):
    """A device of 256 CUs with room for 4 workgroups each: launches whose
    instances are not grouped by XCD are planned for 2 per CU."""
    def device():
        env(256)
        monkeypatch.setenv("IRLMX_PLAN_GRID_PER_CU", "4")
    device()
    assert plan_of(lib, stencil(256, 256)) == grid(bpi=256)
    assert plan_of(lib, stencil(256, 256, B=2, shared=0)) == grid(bpi=256, ipl=2)
    assert plan_of(lib, stencil(256, 256, B=3, shared=0)) == grid(bpi=128, spt=2, ipl=3)
    assert plan_of(lib, stencil(256, 256, B=4, shared=0)) == grid(bpi=128, spt=2, ipl=4)
    assert plan_of(lib, stencil(256, 256, B=5, shared=0)) == grid(bpi=64, spt=4, ipl=5)
    assert plan_of(lib, stencil(128, 128, B=7, shared=0)) == grid(bpi=64, ipl=7)
    assert plan_of(lib, stencil(128, 128, B=16, shared=0)) == grid(bpi=64, ipl=16, xcd=1)   # grouped: all 4 per CU
    monkeypatch.setenv("IRLMX_XCD_GROUP", "0")
    assert plan_of(lib, stencil(128, 128, B=16, shared=0)) == grid(bpi=32, spt=2, ipl=16)
    monkeypatch.setenv("IRLMX_PLAN_GRID_PER_CU", "1")                  # one instance may take the whole capacity
    monkeypatch.setenv("IRLMX_PLAN_CUS", "64")
    assert plan_of(lib, stencil(128, 128)) == grid(bpi=64)


def test_xcd_groups_from_eight_instances(lib, env):
    m = stencil(37, 23, B=8, shared=0)
    env(32, **SMALL)                                                   # 4 workgroups per XCD share: one instance each
    assert plan_of(lib, m) == grid(bpi=4, ipl=8, xcd=1)
    env(32, IRLMX_XCD_GROUP=0, **SMALL)
    assert plan_of(lib, m) == grid(bpi=4, ipl=8)
    env(32, **SMALL)
    assert plan_of(lib, stencil(37, 23, B=7, shared=0)) == grid(bpi=4, ipl=7)
    # grouping never costs a launch: 9 instances fit ungrouped (36 workgroups), grouped only 8 of them
    env(36, **SMALL)
    assert plan_of(lib, stencil(37, 23, B=9, shared=0)) == grid(bpi=4, ipl=9)


def test_too_many_states_for_the_block_words(lib, env):
    env(1 << 20)
    S = (1 << 18) + 256
    assert plan_of(lib, stencil(S, 1)) == sweep(S)                     # 257 workgroups at four states per thread
    assert plan_of(lib, stencil(1 << 18, 1)) == grid(bpi=256, spt=4)
    assert plan_of(lib, stencil(1 << 16, 1)) == grid(bpi=256)


def test_workspace_holds_one_launch_of_granules(lib, env):
    m = stencil(37, 23, B=3, shared=0)
    sizes = {}
    for cap in (4, 8, 12):
        env(cap, IRLMX_EXT_GRID_MAX_LAUNCHES=3, **SMALL)
        ipl = plan_of(lib, m)[4]
        need = int(lib.irlmx_workspace_bytes(ctypes.byref(m), OP_BACKWARD | EXTENDED))
        sizes[ipl] = need
        # weights, the per-sweep ping-pong (the rerun's), value granules (3 sweeps x S x 2 x 16 B), block words
        floor = 3 * 5 * 851 * 8 + 2 * 3 * 851 * 12 + ipl * (96 * 851 + 4 * 4 * 16) + 16
        assert need >= floor and need % 256 == 0, (cap, need, floor)
    assert sizes[1] < sizes[2] < sizes[3]
    env(4, IRLMX_GRID=0, **SMALL)
    assert int(lib.irlmx_workspace_bytes(ctypes.byref(m), OP_BACKWARD | EXTENDED)) < sizes[1]
