"""First-party device ops on the user-op interface: libchiara_ops.so (include/chiara_ops.h).

    from chiara_amd import ops
    op = ops.float16_op(ca.SUM)                # IEEE binary16 SUM; also PROD, MAX, MIN
    g.all_reduce_radix_batch(sends, recvs, count, ops.F16_DTYPE, op, k, b)
    ops.release()                               # the codes go back to the 64 user-op codes

The elements are 2-byte binary16 values (numpy float16, torch.float16) and travel as UINT16; the op gives them their
meaning.  The op codes are valid wherever a user-defined op is: every reduce_* entry point, the collectives on
communicators and local groups, the MPICH baselines (the ops are commutative).  Any other dtype is refused
(ERR_UNSUPPORTED, nothing enqueued).  The library is loaded on first use and registers nothing until asked; there is
no fallback: a missing libchiara_ops.so is an error."""
import ctypes
import os

from ._lib import HERE, PKG_ROOT, ChiaraError, lib
from .collectives import SUCCESS, UINT16

F16_DTYPE = UINT16
OPS_LIB_PATH = os.path.join(HERE, "libchiara_ops.so")

_ops_lib = None


def ops_lib():
    """libchiara_ops.so, loaded on first use (libchiara.so, its dependency, is this process's copy)."""
    global _ops_lib
    if _ops_lib is None:
        lib()
        if not os.path.exists(OPS_LIB_PATH):
            raise ImportError(f"libchiara_ops.so not found at {OPS_LIB_PATH}; build it with `make -C {PKG_ROOT}` "
                              f"(hipcc --offload-arch=gfx950) or __graft_entry__.build()")
        L = ctypes.CDLL(OPS_LIB_PATH)
        L.chr_ops_float16.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.chr_ops_float16.restype = ctypes.c_int
        L.chr_ops_release.argtypes = []
        L.chr_ops_release.restype = ctypes.c_int
        L.chr_ops_stats.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_int]
        L.chr_ops_stats.restype = None
        _ops_lib = L
    return _ops_lib


def float16_op(kind):
    """The op code of binary16 `kind` (SUM, PROD, MAX or MIN), registered on the first call for that kind
    (chr_ops_float16); the same code until release()."""
    op = ctypes.c_int(0)
    rc = ops_lib().chr_ops_float16(int(kind), ctypes.byref(op))
    if rc != SUCCESS:
        raise ChiaraError(rc, "chr_ops_float16")
    return op.value


def release():
    """Free every op this library registered (chr_ops_release); returns the status code."""
    return ops_lib().chr_ops_release()


def stats(reset=False):
    """(fold-launcher calls, tree-launcher calls, trees handed over) since the last reset (chr_ops_stats)."""
    c = (ctypes.c_long * 3)()
    ops_lib().chr_ops_stats(c, 1 if reset else 0)
    return tuple(c)
