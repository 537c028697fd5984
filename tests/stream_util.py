"""The stream contract of the kernel boundary, made visible: a gate in front of every call.

include/chiara.h promises that chr_reduce_local, chr_reduce_multi(_ex), chr_reduce_tree(_batch), chr_fill, every
user-op launcher and the binary16 ops are "enqueued on `stream`" and "return at once".  On the legacy NULL stream with
a device synchronise behind every call (the rest of the suite) neither half of that can fail.  Here a case runs as

    before   every operand buffer holds STALE contents (valid data of the same type from another seed), every output
             0xA5 bytes; the case has run once on the NULL stream with the same arguments (module load, lazy
             initialisation) and the device is idle
    gate     on a non-blocking stream S only: event, one asynchronous copy of GATE_BYTES from page-locked host memory
             into a device pad, event
    upload   on S only: asynchronous copies of the TRUE operands from page-locked memory
    call     the library call(s) under test, given S's handle
    read     on S only: asynchronous copies of the results into page-locked memory
    wait     S.synchronize() -- never a device synchronise, nothing on the NULL stream since the gate

A launch that went anywhere but S runs while the gate is still copying: it reads stale operands, or writes its output
before the true ones arrive, and the result differs from the reference of the true operands.  Two facts per case,
both asserted by Outcome.check():

    ordered           the results equal the references, bit for bit
    returned at once  right after the last library call returned the gate's end event had not completed

and a case whose gate lasted less than twice its own host time (gate enqueue to call return) fails as inconclusive.

S is checked to be non-blocking (hipStreamGetFlags on the HIP runtime this process already loaded, bit
hipStreamNonBlocking): a blocking stream would order against the NULL stream and hide a launch that strayed there.

The gate's size: tests/test_gpu_streams.py::test_control_a_strayed_call_shows hands the call a second non-blocking
stream that nothing orders against S, requires that the result is then NOT the reference, and requires the gate to
last at least 20 times the largest host time any case of the run recorded -- the forced-shapes child included, whose
16 MiB cases are 512 launch pieces each and set that largest time.  Chosen size: GATE_BYTES = 3 GiB.  Measured on an
MI355X (that test's printed line, three runs): gate 56.19 ms; largest host enqueue time 1.38 ms, 1.54 ms and 1.36 ms
(the child's in-place 16 MiB f32 SUM fold).  At 1 GiB the gate lasted 18.74 ms against 1.36 ms: 13.7 times, too short.
Every other case enqueues in 0.03 - 0.2 ms.  In the control the strayed fold and the strayed 8-leaf tree both gave
exactly the reference of the stale operands."""
import ctypes
import time

import numpy as np
import torch

import gpu_util as gu

GATE_BYTES = 3 << 30
# test_control_a_strayed_call_shows on an MI355X at this size (its printed line): the gate's duration from its events
# and the largest host enqueue time (gate enqueue to call return) of any case, the child's included.
GATE_MEASURED = {"gate_ms": 56.19, "largest_enqueue_ms": 1.54}

HIP_STREAM_NON_BLOCKING = 0x01  # hip_runtime_api.h hipStreamNonBlocking

_hip = None


def hip():
    """The HIP runtime this process already runs on (torch's copy, which libchiara.so resolved to as well)."""
    global _hip
    if _hip is None:
        torch.cuda.init()
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        assert path, "no HIP runtime is loaded in this process"
        L = ctypes.CDLL(path)
        L.hipStreamGetFlags.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)]
        L.hipStreamGetFlags.restype = ctypes.c_int
        L.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
        L.hipStreamCreateWithFlags.restype = ctypes.c_int
        _hip = L
    return _hip


def stream_flags(handle):
    flags = ctypes.c_uint(0xFFFFFFFF)
    rc = hip().hipStreamGetFlags(ctypes.c_void_p(handle), ctypes.byref(flags))
    assert rc == 0, f"hipStreamGetFlags: {rc}"
    return flags.value


def is_nonblocking(handle):
    return handle != 0 and bool(stream_flags(handle) & HIP_STREAM_NON_BLOCKING)


def nonblocking_stream():
    """A torch stream that is a non-blocking HIP stream, asserted, and already used once (its queue exists)."""
    s = torch.cuda.Stream(device=gu.DEV)
    if not is_nonblocking(s.cuda_stream):  # torch's pool is blocking on this build: make one
        h = ctypes.c_void_p()
        rc = hip().hipStreamCreateWithFlags(ctypes.byref(h), HIP_STREAM_NON_BLOCKING)
        assert rc == 0, f"hipStreamCreateWithFlags: {rc}"
        s = torch.cuda.ExternalStream(h.value, device=gu.DEV)
    assert is_nonblocking(s.cuda_stream), f"stream flags {stream_flags(s.cuda_stream):#x}: not non-blocking"
    with torch.cuda.stream(s):
        torch.zeros(16, dtype=torch.uint8, device=gu.DEV).add_(1)
    s.synchronize()
    return s


def pinned(nbytes):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8).pin_memory()


def pinned_copy(a):
    """A page-locked uint8 tensor holding a's bytes (padding bytes of structured elements included)."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = pinned(raw.size)
    t[:raw.size].numpy()[:] = raw
    return t


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


_gate = None


def shared_gate():
    """The one gate of this process: its pads are allocated on first use and kept."""
    global _gate
    if _gate is None:
        _gate = Gate()
    return _gate


class Gate:
    """The page-locked pad and the device pad."""

    def __init__(self, nbytes=GATE_BYTES):
        self.nbytes = nbytes
        self.host = pinned(nbytes)
        self.host.fill_(0x3C)
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=gu.DEV)
        torch.cuda.synchronize(gu.DEV)

    def enqueue(self, stream):
        """event, copy, event on `stream` (the caller has made it current); returns the two events."""
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        self.dev.copy_(self.host, non_blocking=True)
        ev1.record(stream)
        return ev0, ev1


class Slot:
    """nbytes of device memory `off` bytes into a 16-byte aligned allocation."""

    def __init__(self, nbytes, off=0, true=None, stale=None):
        self.nbytes, self.off = int(nbytes), off
        self.t = gu.empty_dev(self.nbytes + 32)
        assert self.t.data_ptr() % 16 == 0
        self.view = self.t[off:off + self.nbytes]
        self.ptr = self.t.data_ptr() + off
        self.true = None if true is None else pinned_copy(true)
        self.stale = None if stale is None else torch.from_numpy(bits(stale).copy())
        self.result = None
        self.ref = None

    def reset(self):
        if self.stale is not None:
            self.view.copy_(self.stale)
        else:
            self.view.fill_(0xA5)


class Case:
    """The buffers of one gated call: operands (true and stale contents), outputs (0xA5), and which of them are read
    back and compared with which reference."""

    def __init__(self, what):
        self.what = what
        self.slots = []
        self.reads = []

    def operand(self, true, stale, off=0):
        assert true.dtype == stale.dtype and true.shape == stale.shape
        s = Slot(true.nbytes, off, true, stale)
        self.slots.append(s)
        return s

    def stale_only(self, stale, off=0):
        """A buffer the gated sequence itself fills (chr_fill): stale before, nothing uploaded."""
        s = Slot(stale.nbytes, off, None, stale)
        self.slots.append(s)
        return s

    def output(self, nbytes, off=0):
        s = Slot(nbytes, off)
        self.slots.append(s)
        return s

    def expect(self, slot, ref):
        slot.ref = bits(ref).copy()
        assert slot.ref.size == slot.nbytes, (self.what, slot.ref.size, slot.nbytes)
        slot.result = pinned(slot.nbytes)
        self.reads.append(slot)
        return slot


class Outcome:
    def __init__(self, what, got, refs, at_once, enqueue_s, gate_ms, rc):
        self.what, self.got, self.refs = what, got, refs
        self.at_once, self.enqueue_s, self.gate_ms, self.rc = at_once, enqueue_s, gate_ms, rc

    @property
    def ordered(self):
        return all(g.size == r.size and np.array_equal(g, r) for g, r in zip(self.got, self.refs))

    def differing(self):
        return [int(np.count_nonzero(g != r)) for g, r in zip(self.got, self.refs)]

    def times(self):
        return f"host time from gate enqueue to call return {self.enqueue_s * 1e3:.3f} ms, gate {self.gate_ms:.3f} ms"

    def verdict(self):
        """None if the case passed, else what failed."""
        if self.rc != 0:
            return f"{self.what}: the call returned {self.rc}"
        if not self.at_once:
            return f"{self.what}: the gate had completed when the call returned ({self.times()})"
        if self.gate_ms * 1e-3 < 2 * self.enqueue_s:
            return f"{self.what}: inconclusive, the gate was shorter than twice the enqueue time ({self.times()})"
        if not self.ordered:
            return (f"{self.what}: not ordered on its stream: {self.differing()} bytes differ from the reference of "
                    f"the true operands ({self.times()})")
        return None

    def check(self):
        v = self.verdict()
        assert v is None, v


LARGEST_ENQUEUE = {"s": 0.0, "what": None}  # over every case this process ran or was told of (the child's)


def note_enqueue(seconds, what):
    if seconds > LARGEST_ENQUEUE["s"]:
        LARGEST_ENQUEUE.update(s=seconds, what=what)


def run_gated(case, call, gate, stream, call_stream=None, warm=True):
    """The sequence of the module docstring.  call(handle) makes the library call(s) and returns their status (the
    first nonzero one).  call_stream: the stream handed to the call when it is not `stream` (the control); it is
    synchronised too before the results are read."""
    handle = (call_stream or stream).cuda_stream
    rc = 0
    if warm:  # module load and lazy initialisation: once on the NULL stream, same arguments
        for s in case.slots:
            s.reset()
        rc = call(0)
        torch.cuda.synchronize(gu.DEV)
    for s in case.slots:
        s.reset()
    torch.cuda.synchronize(gu.DEV)
    with torch.cuda.stream(stream):
        t0 = time.perf_counter()
        ev0, ev1 = gate.enqueue(stream)
        for s in case.slots:
            if s.true is not None:
                s.view.copy_(s.true[:s.nbytes], non_blocking=True)
        rc = call(handle) or rc
        t1 = time.perf_counter()
        at_once = not ev1.query()
        if call_stream is not None:  # the control: what the strayed call left is read after both streams
            call_stream.synchronize()
        for s in case.reads:
            s.result[:s.nbytes].copy_(s.view, non_blocking=True)
    stream.synchronize()
    out = Outcome(case.what, [s.result[:s.nbytes].numpy().copy() for s in case.reads], [s.ref for s in case.reads],
                  at_once, t1 - t0, ev0.elapsed_time(ev1), rc)
    note_enqueue(out.enqueue_s, case.what)
    return out
