"""The call-contract harness (tests/abi_call.py) without a device.

* Coverage: the entry points of include/irlmx.h with a ``void* workspace``
  parameter are exactly the ones abi_call wraps, so a new one cannot stay out
  of tests/test_gpu_call_contract.py's matrix.
  Likewise the entry points with a ``void* stream`` parameter are exactly the
  ones tests/test_gpu_stream_order.py has a row for, each with a stated claim
  about asynchrony.
* Self-test: on CPU tensors, against stand-in "calls" that write their
  workspace and outputs through host pointers, the checker flags a byte written
  at ``workspace + n``, a byte written just before the workspace, an unwritten
  float64, int32 and int64 output entry and an output that depends on the
  workspace's contents on entry -- and nothing on a stand-in that keeps the
  contract.  This is the evidence that the GPU assertions can fail; no kernel
  is broken to produce it.
* irlmx_workspace_bytes is a multiple of 256 for every model and op of the GPU
  matrix (models without a device, as tests/test_abi_*.py build them).
"""

import ctypes
import os
import re

import pytest

torch = pytest.importorskip("torch")

import abi_call as A  # noqa: E402
from conftest import ROOT  # noqa: E402

HEADER = os.path.join(ROOT, "include", "irlmx.h")


# -- coverage ----------------------------------------------------------------------------------

def declared_with_workspace():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    names = set()
    for name, params in re.findall(r"\b(irlmx_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*workspace\b", params):
            names.add(name)
    return names


def test_every_entry_point_with_a_workspace_is_wrapped():
    declared = declared_with_workspace()
    assert len(declared) == 9 and "irlmx_forward_svf_horizon" in declared, declared   # the parser sees them
    assert "irlmx_soft_backward_horizon" in declared, declared
    assert declared == set(A.WRAPPED), (declared - set(A.WRAPPED), set(A.WRAPPED) - declared)
    from irlmx import _lib
    for name, fn in A.WRAPPED.items():
        assert name in _lib.SIGNATURES and callable(fn) and "irlmx_" + fn.__name__ == name, name


def declared_with_stream():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {name for name, params in re.findall(r"\b(irlmx_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
            if re.search(r"\bvoid\s*\*\s*stream\b", params)}


def test_every_entry_point_with_a_stream_has_a_stream_order_row():
    import test_gpu_stream_order as SO
    from irlmx import _lib
    declared = declared_with_stream()
    assert len(declared) == 27 and {"irlmx_mdp_properties", "irlmx_dense_gemm", "irlmx_rollout"} <= declared, declared
    assert declared_with_workspace() <= declared                 # every call with a workspace enqueues work
    assert declared == set(SO.ENTRY_POINTS), (declared - set(SO.ENTRY_POINTS), set(SO.ENTRY_POINTS) - declared)
    assert declared <= set(_lib.SIGNATURES)
    for r in SO.ROWS:                                            # every row states its claim and who judges its bits
        assert SO.CLAIMS[(r.entry, r.shape)] in (SO.ASYNC, SO.SYNC) and r.judged, r.id
        assert set(r.keys) <= set(SO.CC.KEYS), r.id
    ran = {(r.entry, r.shape) for r in SO.ROWS}
    assert set(SO.CLAIMS) == ran, (set(SO.CLAIMS) - ran, ran - set(SO.CLAIMS))     # no claim without a row that checks it
    for first, second in SO.PAIRS:
        assert first in SO.ROW and second in SO.ROW, (first, second)
    assert len(SO.PAIRS) <= 6


# -- the harness against stand-in calls --------------------------------------------------------------

N = 1024


class StandIn:
    """A host "entry point" with a float64, an int64 and an int32 output.  ``fault`` names the promise it breaks."""

    def __init__(self, fault=None, n=N):
        self.fault, self.n = fault, n

    def __call__(self, fill="zero", donor=None):
        out = {"value": torch.empty((2, 5), dtype=torch.float64), "iterations": torch.empty(2, dtype=torch.int64),
               "status": torch.empty(2, dtype=torch.int32)}

        def invoke(ws, n, scale=1.0):
            assert (ws is None) == (n == 0) and n == self.n
            first = ctypes.string_at(ws, 1)[0] if ws else 0        # what the workspace held on entry
            if ws:
                assert ws % A.ALIGN == 0
                ctypes.memset(ws, 0x3C, n)                          # scratch, all of it, to the last byte
            if self.fault == "byte at n":
                ctypes.memset(ws + n, 0, 1)
            if self.fault == "byte before":
                ctypes.memset(ws - 1, 0, 1)
            out["value"].copy_(torch.arange(10, dtype=torch.float64).reshape(2, 5) * scale)
            out["value"][1, 2] = float("nan")                       # an honest NaN is not the sentinel
            out["iterations"].copy_(torch.tensor([3, 0]))
            out["status"].copy_(torch.tensor([0, 1], dtype=torch.int32))
            if self.fault == "reads the workspace":
                out["value"][0, 0] = float(first)
            for name, at in (("value", (1, 4)), ("iterations", (1,)), ("status", (0,))):
                if self.fault == f"{name} unwritten":
                    A.poison(out[name][at].reshape(1))
            return None

        return A.contract_call(f"stand-in ({self.fault})", "cpu", self.n, out, invoke, fill, donor)


def all_fills(call):
    zero = call(fill="zero")
    for fill in ("ones", "stale"):
        A.assert_same_bits(f"{fill} against zero", call(fill=fill, donor={"scale": -2.0} if fill == "stale" else None), zero)
    return zero


@pytest.mark.parametrize("n", [N, 256, 0])
def test_clean_stand_in_passes(n):
    zero = all_fills(StandIn(n=n))
    assert zero["iterations"].tolist() == [3, 0] and zero["status"].tolist() == [0, 1]
    assert zero["value"][0, 3].item() == 3.0 and bool(torch.isnan(zero["value"][1, 2]))


@pytest.mark.parametrize("fill", ["zero", "ones", "stale"])
@pytest.mark.parametrize("fault,message", [
    ("byte at n", rf"1 guard bytes at or beyond workspace \+ workspace_bytes changed, the first at workspace offset {N} "),
    ("byte before", r"1 guard bytes before the workspace changed, the first at workspace offset -1 "),
    ("value unwritten", r"1 of 10 entries of value \(2, 5\) were not written, the first at flat index 9"),
    ("iterations unwritten", r"1 of 2 entries of iterations \(2,\) were not written, the first at flat index 1"),
    ("status unwritten", r"1 of 2 entries of status \(2,\) were not written, the first at flat index 0"),
])
def test_guard_and_sentinel_faults_are_flagged(fault, message, fill):
    with pytest.raises(A.ContractViolation, match=message):
        StandIn(fault)(fill=fill, donor={"scale": -2.0})


def test_side_stream_mode_degrades_on_the_cpu():
    """``stream_call`` with a Side on a CPU device is the plain call: the same checks, the same bits."""
    def run(side, fault=None):
        out = {"value": torch.empty(4, dtype=torch.float64), "status": torch.empty(1, dtype=torch.int32)}

        def invoke(ws, n, stream, x):
            assert stream is None and ws % A.ALIGN == 0 and n == 256
            ctypes.memset(ws, 0x3C, n + (fault == "byte at n"))
            out["value"].copy_(2.0 * x)
            if fault != "status unwritten":
                out["status"].fill_(0)

        x = torch.arange(4, dtype=torch.float64)
        return A.stream_call("stand-in", "cpu", 256, out, invoke, {"x": x}, {"x": x + 1.0}, side)

    side = A.Side(None, cycles=1000, claim="async")
    A.assert_same_bits("side against plain", run(side), run(None))
    assert side.returned_early is None and run(side)["value"].tolist() == [0.0, 2.0, 4.0, 6.0]
    for fault, message in (("byte at n", "guard bytes at or beyond"), ("status unwritten", "entries of status")):
        with pytest.raises(A.ContractViolation, match=message):
            run(side, fault)


def test_dependence_on_the_fill_is_flagged():
    call = StandIn("reads the workspace")
    zero = call(fill="zero")                                   # each run alone keeps (c): only the comparison can tell
    assert zero["value"][0, 0].item() == 0.0
    with pytest.raises(A.ContractViolation, match="ones against zero: 1 of 10 entries of value differ.*flat index 0"):
        A.assert_same_bits("ones against zero", call(fill="ones"), zero)
    stale = call(fill="stale", donor={"scale": -2.0})          # the donor left 0x3C bytes behind
    assert stale["value"][0, 0].item() == float(0x3C)
    with pytest.raises(A.ContractViolation, match="value differ"):
        all_fills(call)


def test_same_bits_tells_nan_payloads_and_signed_zeros_apart():
    a = torch.tensor([0.0, float("nan")], dtype=torch.float64)
    A.assert_same_bits("same", {"x": a, "k": torch.tensor([1, 2])}, {"x": a.clone().numpy(), "k": [1, 2]})
    A.assert_same_bits("NULL", {"x": None}, {"x": None})
    for other in (torch.tensor([-0.0, float("nan")], dtype=torch.float64), A.poison(a.clone())):
        with pytest.raises(A.ContractViolation):
            A.assert_same_bits("differs", {"x": a}, {"x": other})
    with pytest.raises(A.ContractViolation, match="NULL"):
        A.assert_same_bits("optional", {"x": a}, {"x": None})


def test_sentinels():
    t = A.poison(torch.zeros(3, dtype=torch.float64))
    assert bool(torch.isnan(t).all()) and t.view(torch.int64).tolist() == [0x7FF8DEADBEEF0001] * 3
    assert A.poison(torch.zeros(2, dtype=torch.int32)).tolist() == [-7, -7]
    assert A.unwritten(torch.tensor([float("nan"), 1.0], dtype=torch.float64)).numel() == 0
    arena = A.Arena(100, "cpu")
    assert arena.pointer() % 256 == 0 and arena.lo >= A.GUARD == 65536
    assert arena.buf.numel() - arena.lo - arena.n >= A.GUARD and arena.workspace().numel() == 100
    with pytest.raises(ValueError):
        StandIn()(fill="stale")
    with pytest.raises(ValueError):
        StandIn()(fill="dirty")


# -- workspace sizes --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from irlmx import _lib
    return _lib.load()


_keep = []


def fake():
    """A non-NULL address that the size query never dereferences."""
    b = ctypes.create_string_buffer(64)
    _keep.append(b)
    return ctypes.cast(b, ctypes.c_void_p).value


def test_workspace_bytes_are_multiples_of_256(lib, monkeypatch):
    import test_gpu_call_contract as G
    from irlmx import _lib
    ops = {"backward": _lib.OP_BACKWARD, "extended": _lib.OP_BACKWARD | _lib.PLAN_EXTENDED_RANGE,
           "forward": _lib.OP_FORWARD, "soft": _lib.OP_SOFT_BACKWARD, "vi": _lib.OP_VALUE_ITERATION,
           "policy evaluation": _lib.OP_POLICY_EVALUATION, "backward horizon": _lib.OP_BACKWARD_HORIZON,
           "forward horizon": _lib.OP_FORWARD_HORIZON, "soft backward horizon": _lib.OP_SOFT_BACKWARD_HORIZON}
    positive = 0
    for name, (dims, envs) in G.MODELS.items():
        m = _lib.MDPStruct()
        (m.layout, m.n_states, m.n_actions, m.width, m.height, m.k_row, m.k_col, m.batch, m.shared) = dims
        m.row_val, m.col_val = fake(), fake()
        if dims[0] == G.ELL:
            m.row_idx, m.col_idx = fake(), fake()
        # (without a device nothing is co-resident: the planned capacity of the persistent shapes is given)
        for keys in envs + tuple({**e, "IRLMX_PLAN_CUS": 256, "IRLMX_PLAN_GRID_PER_CU": 4} for e in envs):
            for k in G.KEYS + ("IRLMX_PLAN_CUS", "IRLMX_PLAN_GRID_PER_CU"):
                monkeypatch.delenv(k, raising=False)
            for k, v in keys.items():
                monkeypatch.setenv(k, str(v))
            for what, op in ops.items():
                n = int(lib.irlmx_workspace_bytes(ctypes.byref(m), op))
                assert n % 256 == 0, (name, keys, what, n)
                if dims[0] == G.DENSE and what in ("extended", "policy evaluation", "backward horizon", "forward horizon",
                                                    "soft backward horizon"):
                    assert n == 0, (name, what, n)             # not run on the DENSE layout
                elif "horizon" not in what:
                    assert n > 0, (name, keys, what, n)        # (the fused horizon shapes need none)
                positive += n > 0
    assert positive > 100
