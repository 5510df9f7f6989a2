"""Calls of the C ABI under the call contract of include/irlmx.h (not a test module).

``irlmx.ops`` takes every workspace and every output from ``torch.empty``, so a
test that goes through it sees the block torch's caching allocator last handed
out: usually the same case's correct intermediate state and the previous
shape's correct answer.  The functions here call the entry points that take a
``void* workspace`` directly, one function per entry point (``WRAPPED``), and
hold each call to what include/irlmx.h states beside irlmx_workspace_bytes:

* the workspace is one arena ``[guard | n bytes | guard]`` with ``n =
  irlmx_workspace_bytes(...)`` and exactly ``n`` passed as ``workspace_bytes``;
  both guards (64 KiB each, filled with 0xA5) must be unchanged after a stream
  synchronise; ``n == 0`` passes a NULL workspace;
* the ``n`` bytes hold, on entry, zeros (``fill="zero"``), 0xFF bytes
  (``"ones"``: doubles read as NaN, counters and flags as -1, tags as all ones)
  or exactly what a donor call left there (``"stale"``: the same entry point on
  the same model, hence the same layout, with the inputs given in ``donor``);
* every float64 output is prefilled with a quiet NaN of a payload no kernel
  produces and every integer output with -7; no entry may hold its sentinel
  afterwards (compared as integers: NaN != NaN).

A broken promise raises ContractViolation.  ``contract_call`` and the classes
below do not care which device their tensors are on:
tests/test_call_contract_host.py runs them against stand-in calls on the CPU.

Stream order (``stream_call``, and ``side=`` of every function below): the same
call on a non-blocking side stream, behind a device delay, with inputs that
land late -- see ``Side``.  tests/test_gpu_stream_order.py runs every entry
point of the header that takes a ``stream`` through it.
"""

import ctypes
import inspect
import time

import numpy as np
import torch

GUARD = 64 * 1024
GUARD_BYTE = 0xA5
ALIGN = 256                          # hipMalloc's and torch's alignment, which include/irlmx.h asks for
F64_SENTINEL = 0x7FF8DEADBEEF0001    # a quiet NaN (as an int64 it is positive)
INT_SENTINEL = -7
FILLS = ("zero", "ones", "stale")


class ContractViolation(AssertionError):
    """A call touched a guard or left an output entry unwritten."""


def poison(t):
    """Fill an output tensor with its sentinel."""
    if t.dtype == torch.float64:
        t.view(torch.int64).fill_(F64_SENTINEL)
    else:
        assert t.dtype in (torch.int32, torch.int64), t.dtype
        t.fill_(INT_SENTINEL)
    return t


def unwritten(t):
    """Flat indices of the entries of ``t`` that still hold the sentinel bits."""
    hit = (t.view(torch.int64) == F64_SENTINEL) if t.dtype == torch.float64 else (t == INT_SENTINEL)
    return hit.reshape(-1).nonzero().reshape(-1)


def assert_written(what, outputs):
    for name, t in outputs.items():
        if t is None:
            continue
        left = unwritten(t)
        if left.numel():
            raise ContractViolation(f"{what}: {left.numel()} of {t.numel()} entries of {name} {tuple(t.shape)} were "
                                    f"not written, the first at flat index {int(left[0])}")


def _bits(x, like=None):
    """A host tensor of ``x`` (a tensor, an array or a list; integers in ``like``'s dtype), doubles as int64."""
    t = x.detach().cpu() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if like is not None and not t.dtype.is_floating_point and not like.dtype.is_floating_point:
        t = t.to(like.dtype)
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def assert_same_bits(what, got, ref):
    """Every output of ``got`` (name -> tensor or None) equals ``ref``'s entry of that name bit for bit."""
    for name, g in got.items():
        r = ref[name]
        if g is None or r is None:
            if g is not r:
                raise ContractViolation(f"{what}: {name} is given in one call and NULL in the other")
            continue
        gb = _bits(g)
        rb = _bits(r, gb)
        if gb.dtype != rb.dtype or gb.shape != rb.shape:
            raise ContractViolation(f"{what}: {name} is {gb.dtype} {tuple(gb.shape)} against {rb.dtype} {tuple(rb.shape)}")
        diff = (gb != rb).reshape(-1).nonzero().reshape(-1)
        if diff.numel():
            raise ContractViolation(f"{what}: {diff.numel()} of {gb.numel()} entries of {name} differ, the first at "
                                    f"flat index {int(diff[0])}")


class Arena:
    """``[guard | n bytes | guard]`` of uint8 on ``device``, the ``n`` bytes 256-byte aligned."""

    def __init__(self, n, device):
        self.n = int(n)
        self.buf = torch.empty(2 * GUARD + self.n + ALIGN, dtype=torch.uint8, device=device)
        self.buf.fill_(GUARD_BYTE)
        # (a device allocation is aligned already; host memory need not be: the front guard grows by the difference)
        self.lo = GUARD + (-(self.buf.data_ptr() + GUARD)) % ALIGN
        assert self.pointer() % ALIGN == 0 and self.lo >= GUARD and self.buf.numel() - self.lo - self.n >= GUARD

    def pointer(self):
        return self.buf.data_ptr() + self.lo

    def workspace(self):
        return self.buf[self.lo:self.lo + self.n]

    def fill(self, mode):
        assert mode in ("zero", "ones"), mode
        self.workspace().fill_(0 if mode == "zero" else 0xFF)

    def check_guards(self, what):
        for name, g, first in (("before the workspace", self.buf[:self.lo], -self.lo),
                               ("at or beyond workspace + workspace_bytes", self.buf[self.lo + self.n:], self.n)):
            bad = (g != GUARD_BYTE).nonzero().reshape(-1)
            if bad.numel():
                raise ContractViolation(f"{what}: {bad.numel()} guard bytes {name} changed, the first at workspace "
                                        f"offset {first + int(bad[0])} (workspace_bytes = {self.n})")


def _synchronize(device):
    device = torch.device(device)
    if device.type == "cuda":
        torch.cuda.current_stream(device).synchronize()


def contract_call(what, device, n, outputs, invoke, fill="zero", donor=None):
    """Run ``invoke(workspace address or None, n, **inputs)`` under the contract.

    ``outputs``: name -> preallocated output tensor (None: an optional output
    passed as NULL).  ``fill``: see the module docstring; for ``"stale"`` the
    donor call ``invoke(ws, n, **donor)`` runs first on the zeroed arena, under
    the same checks, and the real call finds the arena as the donor left it.
    ``invoke`` returns whatever must stay alive until the stream is
    synchronised.  Returns ``outputs``."""
    if fill not in FILLS:
        raise ValueError(f"fill {fill!r} not in {FILLS}")
    if fill == "stale" and donor is None:
        raise ValueError("fill='stale' needs the donor call's inputs")
    arena = Arena(n, device)

    def once(tag, **inputs):
        for t in outputs.values():
            if t is not None:
                poison(t)
        keep = invoke(arena.pointer() if arena.n else None, arena.n, **inputs)
        _synchronize(device)
        del keep
        arena.check_guards(f"{what} [{tag}]")
        assert_written(f"{what} [{tag}]", outputs)

    if fill == "stale":
        arena.fill("zero")
        once("donor of stale", **donor)
    else:
        arena.fill(fill)
    once(fill)
    return outputs


# ---------------------------------------------------------------------------
# the same call on a side stream, behind a delay
# ---------------------------------------------------------------------------

class HarnessDrained(AssertionError):
    """The delay had run out before the entry point was called: the set-up blocked
    the host or the delay is too short.  A defect of the test, not of the library."""


class AsynchronyViolation(AssertionError):
    """A call declared asynchronous returned only after the work queued before it had run."""


class Side:
    """How ``stream_call`` runs one call: on ``stream`` (a torch.cuda.Stream, which
    is non-blocking: it does not wait for the legacy default stream; None: the
    current stream), behind
    ``cycles`` of ``torch.cuda._sleep`` (0: no delay), the workspace filled with
    ``fill`` in stream order.  ``claim`` "async": the call must return while the
    delay still runs (AsynchronyViolation otherwise); anything else asserts
    nothing about it.  ``defer``: ``stream_call`` returns once everything is
    enqueued and ``finish()`` synchronises, checks and returns the outputs -- so
    that a second call can be put in flight on another stream in between.

    After the call: ``returned_early`` (None without a delay), ``host_ms`` (the
    wall time of the entry point on the host), ``arena``."""

    def __init__(self, stream, cycles=0, claim=None, fill="ones", defer=False):
        self.stream, self.cycles, self.claim, self.fill, self.defer = stream, int(cycles), claim, fill, defer
        self.returned_early = self.host_ms = self.arena = self.finish = None


def stream_call(what, device, n, outputs, invoke, real, donor, side=None):
    """Run ``invoke(workspace address or None, n, stream handle, **inputs)`` under the
    contract, on the current stream (``side=None``: the device otherwise idle,
    the workspace zeroed) or as ``side`` says.

    ``real``: name -> device tensor of every array input; ``donor``: the same
    names -> legal inputs of the same type and shape with other values.  The
    entry point is handed buffers that hold the donor's values until, in stream
    order after the delay, the real ones are copied over them, and that take
    the donor's values again right after the call.  In stream order after the
    delay as well: the workspace fill and the outputs' sentinels.  So whatever
    part of a call runs on another stream runs during the delay: it reads the
    donor's inputs, or its memset is overwritten by the fill, or its output by
    the sentinel; and a read deferred past the call finds the donor's values
    again.  Nothing between the delay and the return of ``invoke`` may block
    the host (HarnessDrained).  On a CPU device ``side`` degrades to the plain
    call.  Returns ``outputs``."""
    device = torch.device(device)
    if device.type != "cuda" or side is None:
        handle = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == "cuda" else None
        return contract_call(what, device, n, outputs, lambda ws, n_: invoke(ws, n_, handle, **real),
                             "zero" if side is None else side.fill)
    assert set(real) == set(donor), (what, sorted(real), sorted(donor))
    for k, t in real.items():
        d = donor[k]
        assert t.is_cuda and d.is_cuda and t.dtype == d.dtype and t.shape == d.shape and t.data_ptr() != d.data_ptr(), (what, k)
    # before the delay: every allocation, the guards, the donor's values in the input buffers
    arena = side.arena = Arena(n, device)
    bufs = {k: d.clone() for k, d in donor.items()}
    given = [t for t in outputs.values() if t is not None]
    for t in given:
        poison(t)
    _synchronize(device)                  # (the set-up ran on the current stream; a side stream does not wait for it)
    s = side.stream if side.stream is not None else torch.cuda.current_stream(device)
    handle = ctypes.c_void_p(s.cuda_stream)
    ev = torch.cuda.Event()
    keep = None
    try:
        with torch.cuda.stream(s):
            if side.cycles:
                torch.cuda._sleep(side.cycles)
            ev.record(s)
            for k, b in bufs.items():
                b.copy_(real[k])
            if arena.n:
                arena.fill(side.fill)
            for t in given:
                poison(t)
            if side.cycles and ev.query():
                raise HarnessDrained(f"{what}: the set-up drained the stream: the delay of {side.cycles} cycles was over "
                                     f"before the entry point was called (a defect of the test, not of the library)")
            t0 = time.perf_counter()
            keep = invoke(arena.pointer() if arena.n else None, arena.n, handle, **bufs)
            side.host_ms = (time.perf_counter() - t0) * 1e3
            side.returned_early = (not ev.query()) if side.cycles else None
            for k, b in bufs.items():
                b.copy_(donor[k])
    except BaseException:
        s.synchronize()                   # nothing of this call is freed while the stream still uses it
        raise

    def finish():
        s.synchronize()
        nonlocal keep
        keep = None
        arena.check_guards(f"{what} [side stream]")
        assert_written(f"{what} [side stream]", outputs)
        if side.cycles and side.claim == "async" and not side.returned_early:
            raise AsynchronyViolation(f"{what}: declared asynchronous, but the call returned after {side.host_ms:.1f} ms "
                                      f"with the delay queued before it already over: it waited for the stream")
        return outputs

    side.finish = finish
    return outputs if side.defer else finish()


# ---------------------------------------------------------------------------
# the entry points of include/irlmx.h that take a workspace
# ---------------------------------------------------------------------------

def _in(x, dtype, shape, dev):
    """A fresh contiguous device tensor of an input (None stays None: an optional pointer)."""
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype).reshape(shape).contiguous()
    return torch.tensor(np.array(x), dtype=dtype, device=dev).reshape(shape).contiguous()


def _out(dtype, shape, dev, given=True):
    return torch.empty(shape, dtype=dtype, device=dev) if given else None


def _run(name, mdp, op, outputs, call, fill, donor, side=None):
    """``call(lib, ws, n, stream, **inputs)`` is the ctypes call; its result code is checked.

    ``side`` (a Side): the call goes through ``stream_call`` instead.  Every
    tensor of ``donor`` then names an input that lands late, and the wrapper's
    own argument of that name must be a device tensor of the same type and
    shape (``_in`` passes both through untouched); every other array input
    must be a device tensor as well -- a host array would be uploaded inside
    the call and block the host.  ``fill`` and the scalars of ``donor`` are not
    used (``side.fill`` is)."""
    from irlmx import _lib
    lib = _lib.load()
    n = int(lib.irlmx_workspace_bytes(mdp.struct(), op))

    if side is not None:
        late = {k: v for k, v in (donor or {}).items() if isinstance(v, torch.Tensor)}
        params = inspect.signature(call).parameters
        real = {k: params[k].default for k in late}

        def invoke_on(ws, n, st, **inputs):
            rc, keep = call(lib, ctypes.c_void_p(ws), n, st if st is not None else _lib.stream_ptr(mdp.device), **inputs)
            _lib.check(rc, name)
            return keep

        return stream_call(name, mdp.device, n, outputs, invoke_on, real, late, side)

    def invoke(ws, n, **inputs):
        rc, keep = call(lib, ctypes.c_void_p(ws), n, _lib.stream_ptr(mdp.device), **inputs)
        _lib.check(rc, name)
        return keep

    return contract_call(name, mdp.device, n, outputs, invoke, fill, donor)


def backward_maxent(mdp, reward, terminal, rescale=True, fill="zero", donor=None, side=None):
    """irlmx_backward_maxent: {"p_action" [B, S, A], "status" [B]}.  ``donor``: a dict of ``reward``, ``terminal``."""
    from irlmx import _lib
    B, S, A, dev = mdp.batch, mdp.n_states, mdp.n_actions, mdp.device
    out = {"p_action": _out(torch.float64, (B, S, A), dev), "status": _out(torch.int32, (B,), dev)}

    def call(lib, ws, n, st, reward=reward, terminal=terminal):
        r, tm = _in(reward, torch.float64, (B, S), dev), _in(terminal, torch.uint8, (B, S), dev)
        return lib.irlmx_backward_maxent(mdp.struct(), _lib.ptr(r), _lib.ptr(tm), 1 if rescale else 0,
                                         _lib.ptr(out["p_action"]), _lib.ptr(out["status"]), ws, n, st), (r, tm)

    return _run("irlmx_backward_maxent", mdp, _lib.OP_BACKWARD, out, call, fill, donor, side)


def backward_maxent_extended(mdp, reward, terminal, fill="zero", donor=None, side=None):
    """irlmx_backward_maxent_extended: {"p_action", "status"}.  ``donor``: ``reward``, ``terminal``."""
    from irlmx import _lib
    B, S, A, dev = mdp.batch, mdp.n_states, mdp.n_actions, mdp.device
    out = {"p_action": _out(torch.float64, (B, S, A), dev), "status": _out(torch.int32, (B,), dev)}

    def call(lib, ws, n, st, reward=reward, terminal=terminal):
        r, tm = _in(reward, torch.float64, (B, S), dev), _in(terminal, torch.uint8, (B, S), dev)
        return lib.irlmx_backward_maxent_extended(mdp.struct(), _lib.ptr(r), _lib.ptr(tm), _lib.ptr(out["p_action"]),
                                                  _lib.ptr(out["status"]), ws, n, st), (r, tm)

    return _run("irlmx_backward_maxent_extended", mdp, _lib.OP_BACKWARD | _lib.PLAN_EXTENDED_RANGE, out, call, fill,
                donor, side)


def forward_svf(mdp, p_initial, terminal, p_action, eps=1e-5, max_iter=0, fill="zero", donor=None, side=None):
    """irlmx_forward_svf: {"svf" [B, S], "iterations" [B], "status" [B]}.
    ``donor``: ``p_initial``, ``terminal``, ``p_action``, ``max_iter``."""
    from irlmx import _lib
    B, S, A, dev = mdp.batch, mdp.n_states, mdp.n_actions, mdp.device
    out = {"svf": _out(torch.float64, (B, S), dev), "iterations": _out(torch.int64, (B,), dev),
           "status": _out(torch.int32, (B,), dev)}

    def call(lib, ws, n, st, p_initial=p_initial, terminal=terminal, p_action=p_action, max_iter=max_iter):
        p0, tm = _in(p_initial, torch.float64, (B, S), dev), _in(terminal, torch.uint8, (B, S), dev)
        pi = _in(p_action, torch.float64, (B, S, A), dev)
        return lib.irlmx_forward_svf(mdp.struct(), _lib.ptr(p0), _lib.ptr(tm), _lib.ptr(pi), float(eps), int(max_iter),
                                     _lib.ptr(out["svf"]), _lib.ptr(out["iterations"]), _lib.ptr(out["status"]), ws, n,
                                     st), (p0, tm, pi)

    return _run("irlmx_forward_svf", mdp, _lib.OP_FORWARD, out, call, fill, donor, side)


def soft_backward(mdp, reward, terminal_reward, discount, eps=1e-5, max_iter=0, fill="zero", donor=None, side=None):
    """irlmx_soft_backward: {"p_action", "value", "iterations", "status"}.  ``donor``: ``reward``, ``max_iter``."""
    from irlmx import _lib
    B, S, A, dev = mdp.batch, mdp.n_states, mdp.n_actions, mdp.device
    out = {"p_action": _out(torch.float64, (B, S, A), dev), "value": _out(torch.float64, (B, S), dev),
           "iterations": _out(torch.int64, (B,), dev), "status": _out(torch.int32, (B,), dev)}

    def call(lib, ws, n, st, reward=reward, max_iter=max_iter, terminal_reward=terminal_reward):
        r, phi = _in(reward, torch.float64, (B, S), dev), _in(terminal_reward, torch.float64, (B, S), dev)
        return lib.irlmx_soft_backward(mdp.struct(), _lib.ptr(r), _lib.ptr(phi), float(discount), float(eps),
                                       int(max_iter), _lib.ptr(out["p_action"]), _lib.ptr(out["value"]),
                                       _lib.ptr(out["iterations"]), _lib.ptr(out["status"]), ws, n, st), (r, phi)

    return _run("irlmx_soft_backward", mdp, _lib.OP_SOFT_BACKWARD, out, call, fill, donor, side)


def value_iteration(mdp, reward, discount, eps=1e-3, average=False, max_iter=0, fill="zero", donor=None, side=None):
    """irlmx_value_iteration: {"value", "iterations", "status"}.  ``donor``: ``reward``, ``max_iter``."""
    from irlmx import _lib
    B, S, dev = mdp.batch, mdp.n_states, mdp.device
    out = {"value": _out(torch.float64, (B, S), dev), "iterations": _out(torch.int64, (B,), dev),
           "status": _out(torch.int32, (B,), dev)}

    def call(lib, ws, n, st, reward=reward, max_iter=max_iter):
        r = _in(reward, torch.float64, (B, S), dev)
        return lib.irlmx_value_iteration(mdp.struct(), _lib.ptr(r), float(discount), float(eps), 1 if average else 0,
                                         int(max_iter), _lib.ptr(out["value"]), _lib.ptr(out["iterations"]),
                                         _lib.ptr(out["status"]), ws, n, st), (r,)

    return _run("irlmx_value_iteration", mdp, _lib.OP_VALUE_ITERATION, out, call, fill, donor, side)


def policy_evaluation(mdp, reward, p_action, discount, terminal=None, eps=1e-3, max_iter=0, fill="zero", donor=None,
                      side=None):
    """irlmx_policy_evaluation: {"value", "iterations", "status"}.  ``donor``: ``reward``, ``p_action``, ``max_iter``."""
    from irlmx import _lib
    B, S, A, dev = mdp.batch, mdp.n_states, mdp.n_actions, mdp.device
    out = {"value": _out(torch.float64, (B, S), dev), "iterations": _out(torch.int64, (B,), dev),
           "status": _out(torch.int32, (B,), dev)}

    def call(lib, ws, n, st, reward=reward, p_action=p_action, max_iter=max_iter, terminal=terminal):
        r, pi = _in(reward, torch.float64, (B, S), dev), _in(p_action, torch.float64, (B, S, A), dev)
        tm = _in(terminal, torch.uint8, (B, S), dev)
        return lib.irlmx_policy_evaluation(mdp.struct(), _lib.ptr(r), _lib.ptr(pi), _lib.ptr(tm), float(discount),
                                           float(eps), int(max_iter), _lib.ptr(out["value"]),
                                           _lib.ptr(out["iterations"]), _lib.ptr(out["status"]), ws, n, st), (r, pi, tm)

    return _run("irlmx_policy_evaluation", mdp, _lib.OP_POLICY_EVALUATION, out, call, fill, donor, side)


def backward_maxent_horizon(mdp, reward, horizon, terminal=None, log_z0=True, fill="zero", donor=None, side=None):
    """irlmx_backward_maxent_horizon: {"p_action_t" [B, T, S, A], "log_z0" [B, S] or None (``log_z0=False``: NULL),
    "status"}.  ``donor``: ``reward``."""
    from irlmx import _lib
    B, S, A, T, dev = mdp.batch, mdp.n_states, mdp.n_actions, int(horizon), mdp.device
    out = {"p_action_t": _out(torch.float64, (B, T, S, A), dev), "log_z0": _out(torch.float64, (B, S), dev, log_z0),
           "status": _out(torch.int32, (B,), dev)}

    def call(lib, ws, n, st, reward=reward, terminal=terminal):
        r, tm = _in(reward, torch.float64, (B, S), dev), _in(terminal, torch.uint8, (B, S), dev)
        return lib.irlmx_backward_maxent_horizon(mdp.struct(), _lib.ptr(r), _lib.ptr(tm), T, _lib.ptr(out["p_action_t"]),
                                                 _lib.ptr(out["log_z0"]), _lib.ptr(out["status"]), ws, n, st), (r, tm)

    return _run("irlmx_backward_maxent_horizon", mdp, _lib.OP_BACKWARD_HORIZON, out, call, fill, donor, side)


def forward_svf_horizon(mdp, p_initial, p_action_t, terminal=None, svf_t=True, fill="zero", donor=None, side=None):
    """irlmx_forward_svf_horizon: {"svf" [B, S], "svf_t" [B, T + 1, S] or None (``svf_t=False``: NULL), "status"}.
    ``donor``: ``p_initial``, ``p_action_t`` (of the same horizon)."""
    from irlmx import _lib
    B, S, A, dev = mdp.batch, mdp.n_states, mdp.n_actions, mdp.device
    T = int(p_action_t.shape[1])
    out = {"svf": _out(torch.float64, (B, S), dev), "svf_t": _out(torch.float64, (B, T + 1, S), dev, svf_t),
           "status": _out(torch.int32, (B,), dev)}

    def call(lib, ws, n, st, p_initial=p_initial, p_action_t=p_action_t, terminal=terminal):
        p0, tm = _in(p_initial, torch.float64, (B, S), dev), _in(terminal, torch.uint8, (B, S), dev)
        pi = _in(p_action_t, torch.float64, (B, T, S, A), dev)
        return lib.irlmx_forward_svf_horizon(mdp.struct(), _lib.ptr(p0), _lib.ptr(tm), _lib.ptr(pi), T,
                                             _lib.ptr(out["svf"]), _lib.ptr(out["svf_t"]), _lib.ptr(out["status"]), ws,
                                             n, st), (p0, tm, pi)

    return _run("irlmx_forward_svf_horizon", mdp, _lib.OP_FORWARD_HORIZON, out, call, fill, donor, side)


def soft_backward_horizon(mdp, reward, discount, horizon, terminal=None, value0=True, fill="zero", donor=None,
                          side=None):
    """irlmx_soft_backward_horizon: {"p_action_t" [B, T, S, A], "value0" [B, S] or None (``value0=False``: NULL),
    "status"}.  ``donor``: ``reward``."""
    from irlmx import _lib
    B, S, A, T, dev = mdp.batch, mdp.n_states, mdp.n_actions, int(horizon), mdp.device
    out = {"p_action_t": _out(torch.float64, (B, T, S, A), dev), "value0": _out(torch.float64, (B, S), dev, value0),
           "status": _out(torch.int32, (B,), dev)}

    def call(lib, ws, n, st, reward=reward, terminal=terminal):
        r, tm = _in(reward, torch.float64, (B, S), dev), _in(terminal, torch.uint8, (B, S), dev)
        return lib.irlmx_soft_backward_horizon(mdp.struct(), _lib.ptr(r), _lib.ptr(tm), float(discount), T,
                                               _lib.ptr(out["p_action_t"]), _lib.ptr(out["value0"]),
                                               _lib.ptr(out["status"]), ws, n, st), (r, tm)

    return _run("irlmx_soft_backward_horizon", mdp, _lib.OP_SOFT_BACKWARD_HORIZON, out, call, fill, donor, side)


#: C name -> the function above that calls it: every entry point of include/irlmx.h with a
#: ``void* workspace`` parameter (tests/test_call_contract_host.py holds the two sets equal)
WRAPPED = {
    "irlmx_backward_maxent": backward_maxent,
    "irlmx_backward_maxent_extended": backward_maxent_extended,
    "irlmx_forward_svf": forward_svf,
    "irlmx_soft_backward": soft_backward,
    "irlmx_value_iteration": value_iteration,
    "irlmx_policy_evaluation": policy_evaluation,
    "irlmx_backward_maxent_horizon": backward_maxent_horizon,
    "irlmx_forward_svf_horizon": forward_svf_horizon,
    "irlmx_soft_backward_horizon": soft_backward_horizon,
}
