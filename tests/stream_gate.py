"""The gate pattern of tests/test_streams_gpu.py: one C-ABI call made with late inputs behind long-running GPU work.

A `Case` names an entry point and its argument list (without the ctx in front and the on_device flag behind).  In the list
  In(real, poison)   is an input buffer: a host array with on_device = 0, a device buffer with on_device = 1.  `poison` is a
                     different, equally valid input of the same shape and type;
  Out(shape, dtype)  is an output buffer of the same kind, filled with a sentinel before the call;
  HostOut(...)       is an output that include/kocr.h keeps on the host in both forms (counts, label rows);
  Ptrs([In, ...])    is an array of pointers to input buffers (kocr_pipeline's images);
a numpy array is a host argument in both forms, None a null pointer, anything else a scalar.

`host_call` makes the call with host arrays.  `gated_call` makes it with device buffers on the current context stream `S`:
the device inputs hold the poison, and on `S`, with no host synchronisation in between, are queued a gate (GPU work of
GATE_MS), device-to-device copies of the real inputs over the poison, the call, and copies of the outputs into snapshots.
The last call on the context before the gated one is the same call on the POISON (the arenas are bump allocators reset by
every call, so each intermediate buffer of the gated call then starts out holding poison-derived values at the same address).
A launch or copy of the call that is not on `S`, or is there in the wrong order, then reads the poison, a value derived from
it, or a sentinel.
"""
import ctypes
import time

import numpy as np

GATE_MS = 150.0   # tens to low hundreds of milliseconds; the tests assert that it was at least 4x the call it shields
SENTINEL = 0xA5


class In:
    def __init__(self, real, poison):
        self.real, self.poison = np.ascontiguousarray(real), np.ascontiguousarray(poison)
        assert self.real.shape == self.poison.shape and self.real.dtype == self.poison.dtype
        assert self.real.tobytes() != self.poison.tobytes(), "the poison must differ from the real input"


class Out:
    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(int(v) for v in np.atleast_1d(shape)), np.dtype(dtype)

    def host(self):
        a = np.empty(self.shape, self.dtype)
        a.view(np.uint8).reshape(-1)[:] = SENTINEL
        return a


class HostOut(Out):
    pass


class Ptrs:
    def __init__(self, items):
        self.items = list(items)


class Case:
    """fn: the entry point; args: see the module docstring; asynchronous: the on_device form returns nothing on the host and
    include/kocr.h does not document it as synchronising; view(outs) -> the comparable part of the outputs, as a list of
    arrays (default: everything); ok: the return codes the call may give (the device form must give the host form's)."""

    def __init__(self, fn, args, asynchronous, view=None, ok=(0,), flag=True):
        self.fn, self.args, self.asynchronous, self.view, self.ok = fn, list(args), asynchronous, view or (lambda outs: outs), ok
        self.flag = flag  # False: a host-pointer entry point without the on_device parameter

    def inputs(self):
        for a in self.args:
            for b in (a.items if isinstance(a, Ptrs) else [a]):
                if isinstance(b, In):
                    yield b


def same_bits(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes()
                                         for g, w in zip(got, want))


def _call(lib, ctx, case, pointer_of, on_device):
    """pointer_of(In | Out | HostOut) -> address.  Returns the return code and the wall time of the call in ms."""
    fn = getattr(lib, case.fn)
    keep, cargs = [], []
    for i, a in enumerate(case.args):
        as_arg = lambda address: ctypes.cast(ctypes.c_void_p(address), fn.argtypes[i + 1])  # noqa: E731
        if isinstance(a, Ptrs):
            arr = (ctypes.c_void_p * len(a.items))(*[pointer_of(b) for b in a.items])
            keep.append(arr)
            cargs.append(as_arg(ctypes.addressof(arr)))
        elif isinstance(a, (In, Out)):
            cargs.append(as_arg(pointer_of(a)))
        elif isinstance(a, np.ndarray):
            cargs.append(as_arg(a.ctypes.data))
        else:
            cargs.append(a)
    if case.flag:
        cargs.append(on_device)
    assert len(cargs) + 1 == len(fn.argtypes), case.fn
    t0 = time.perf_counter()
    rc = fn(ctx._h, *cargs)
    return rc, (time.perf_counter() - t0) * 1e3


def host_call(lib, ctx, case, which="real"):
    """The call with host arrays (on_device = 0) on whatever stream the context is on.  Returns (rc, outputs, ms)."""
    bufs = {}
    for a in case.args:
        if isinstance(a, Out):
            bufs[id(a)] = a.host()
    rc, ms = _call(lib, ctx, case, lambda a: (getattr(a, which) if isinstance(a, In) else bufs[id(a)]).ctypes.data, 0)
    return rc, [bufs[id(a)] for a in case.args if isinstance(a, Out)], ms


def _to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _from_dev(t, spec):
    return t.cpu().numpy().view(spec.dtype).reshape(spec.shape)


class Gate:
    """GPU work of about `ms` milliseconds on the current torch stream: torch.cuda._sleep, calibrated once, or a chain of
    large matmuls where the installed torch has none."""

    def __init__(self, ms=GATE_MS):
        import torch

        self.ms = ms
        self.sleep = getattr(torch.cuda, "_sleep", None)
        if self.sleep is None:
            self.a = torch.rand(4096, 4096, device="cuda")
        self.units = 1
        self.units = max(1, int(np.ceil(self._measure(1_000_000 if self.sleep else 4))))

    def _measure(self, trial):
        import torch

        self.units = trial
        self.run()  # once unmeasured: the first launch loads the kernel
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run()
        e1.record()
        torch.cuda.synchronize()
        return trial * self.ms / max(e0.elapsed_time(e1), 1e-3)

    def run(self):
        if self.sleep is not None:
            self.sleep(self.units)
        else:
            for _ in range(self.units):
                self.a @ self.a


class Gated:
    """What gated_call observed: rc, outs (the snapshots; host outputs as they stood when the call returned), call_ms (host
    wall time of the call), gate_ms (GPU time of the gate), gate_running (the gate had not finished when the call returned)"""


def device_call(lib, ctx, case, stream, which="real"):
    """The device-pointer call on the real or the poison inputs, ungated, synchronised: the warm-up.  Returns (rc, ms to
    completion)."""
    import torch

    dev = {id(a): _to_dev(getattr(a, which)) for a in case.inputs()}
    host = {}
    for a in case.args:
        if isinstance(a, HostOut):
            host[id(a)] = a.host()
        elif isinstance(a, Out):
            dev[id(a)] = _to_dev(a.host())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        rc, _ = _call(lib, ctx, case, lambda a: host[id(a)].ctypes.data if isinstance(a, HostOut) else dev[id(a)].data_ptr(), 1)
    stream.synchronize()
    return rc, (time.perf_counter() - t0) * 1e3


def gated_call(lib, ctx, case, stream, gate, on_device=1):
    """See the module docstring.  With on_device = 0 the arguments are host arrays (the real inputs) and only the gate is
    queued ahead of the call."""
    import torch

    g = Gated()
    live, real, snap, host = {}, {}, {}, {}
    for a in case.inputs():
        live[id(a)], real[id(a)] = (_to_dev(a.poison), _to_dev(a.real)) if on_device else (None, a.real)
    for a in case.args:
        if isinstance(a, HostOut) or (isinstance(a, Out) and not on_device):
            host[id(a)] = a.host()
        elif isinstance(a, Out):
            live[id(a)], snap[id(a)] = _to_dev(a.host()), _to_dev(np.full(a.shape, 0, a.dtype))

    def pointer_of(a):
        if id(a) in host:
            return host[id(a)].ctypes.data
        return live[id(a)].data_ptr() if on_device else real[id(a)].ctypes.data

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):   # from here to the snapshots nothing synchronises the host with the device
        e0.record()
        gate.run()
        e1.record()
        if on_device:
            for a in case.inputs():
                live[id(a)].copy_(real[id(a)], non_blocking=True)
        g.rc, g.call_ms = _call(lib, ctx, case, pointer_of, on_device)
        g.gate_running = not e1.query()
        host_now = {k: v.copy() for k, v in host.items()}
        for k in snap:
            snap[k].copy_(live[k], non_blocking=True)
    stream.synchronize()
    g.gate_ms = e0.elapsed_time(e1)
    g.outs = [host_now[id(a)] if id(a) in host_now else _from_dev(snap[id(a)], a) for a in case.args if isinstance(a, Out)]
    return g
