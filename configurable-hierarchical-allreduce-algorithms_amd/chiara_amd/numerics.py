"""First-party struct ops on derived element types: libchiara_numerics.so (include/chiara_numerics.h).

    from chiara_amd import numerics as num
    t, op = num.sum2_type(ca.FLOAT32), num.sum2_op()        # {hi, lo} pairs, a double-word SUM
    num.sum2_pack(pairs, values, count, ca.FLOAT32, stream)  # pairs[i] = {values[i], +0}
    g.all_reduce_radix_batch(sends, recvs, count, t, op, k, b)
    num.sum2_unpack(values, pairs, count, ca.FLOAT32, stream)
    num.release()                                            # the op and type codes go back

sum2 carries about twice the base type's precision through whatever expression tree the geometry and schedule fix, so
on well-conditioned data the unpacked sum is the correctly rounded one for every (n, k, b).  moments merges
{n, mean, M2} records with Chan's formula: moments_pack makes one record per sample, the allreduce merges them, the
variance is M2 / n.  The base type is FLOAT32 or FLOAT64.  The op codes are valid wherever a user-defined op is; the
ops take any live type of the right content (your own type_contiguous(2, FLOAT32) as well) and refuse every other
dtype (ERR_UNSUPPORTED, nothing enqueued).  The library is loaded on first use and registers nothing until asked;
there is no fallback: a missing libchiara_numerics.so is an error."""
import ctypes
import os

from ._lib import HERE, PKG_ROOT, ChiaraError, lib
from .collectives import SUCCESS, _addr, _stream

NUM_LIB_PATH = os.path.join(HERE, "libchiara_numerics.so")

_num_lib = None


def num_lib():
    """libchiara_numerics.so, loaded on first use (libchiara.so, its dependency, is this process's copy)."""
    global _num_lib
    if _num_lib is None:
        lib()
        if not os.path.exists(NUM_LIB_PATH):
            raise ImportError(f"libchiara_numerics.so not found at {NUM_LIB_PATH}; build it with `make -C {PKG_ROOT}` "
                              f"(hipcc --offload-arch=gfx950) or __graft_entry__.build()")
        L = ctypes.CDLL(NUM_LIB_PATH)
        vp, ip, sz, i = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_size_t, ctypes.c_int
        for name, args in (("chr_num_sum2", [ip]), ("chr_num_moments", [ip]),
                           ("chr_num_sum2_type", [i, ip]), ("chr_num_moments_type", [i, ip]),
                           ("chr_num_sum2_pack", [vp, vp, sz, i, vp]), ("chr_num_sum2_unpack", [vp, vp, sz, i, vp]),
                           ("chr_num_moments_pack", [vp, vp, sz, i, vp]),
                           ("chr_num_moments_unpack", [vp, vp, vp, vp, sz, i, vp]), ("chr_num_release", [])):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = ctypes.c_int
        L.chr_num_stats.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_int]
        L.chr_num_stats.restype = None
        _num_lib = L
    return _num_lib


def _code(fn, what, *args):
    out = ctypes.c_int(0)
    rc = fn(*args, ctypes.byref(out))
    if rc != SUCCESS:
        raise ChiaraError(rc, what)
    return out.value


def sum2_op():
    """The op code of the double-word SUM (chr_num_sum2), registered on the first call; the same until release()."""
    return _code(num_lib().chr_num_sum2, "chr_num_sum2")


def moments_op():
    """The op code of the {n, mean, M2} merge (chr_num_moments)."""
    return _code(num_lib().chr_num_moments, "chr_num_moments")


def sum2_type(base):
    """The {hi, lo} element type over `base` (FLOAT32 or FLOAT64): type_contiguous(2, base), cached until release()."""
    return _code(num_lib().chr_num_sum2_type, "chr_num_sum2_type", int(base))


def moments_type(base):
    """The {n, mean, M2} element type over `base`: type_contiguous(3, base), cached until release()."""
    return _code(num_lib().chr_num_moments_type, "chr_num_moments_type", int(base))


def sum2_pack(pairs, values, count, base, stream=None):
    """pairs[i] = {values[i], +0} for `count` device elements, enqueued on `stream`; returns the status code."""
    return num_lib().chr_num_sum2_pack(_addr(pairs), _addr(values), count, int(base), _stream(stream))


def sum2_unpack(values, pairs, count, base, stream=None):
    """values[i] = pairs[i].hi."""
    return num_lib().chr_num_sum2_unpack(_addr(values), _addr(pairs), count, int(base), _stream(stream))


def moments_pack(recs, samples, count, base, stream=None):
    """recs[i] = {1, samples[i], +0}."""
    return num_lib().chr_num_moments_pack(_addr(recs), _addr(samples), count, int(base), _stream(stream))


def moments_unpack(n, mean, m2, recs, count, base, stream=None):
    """De-interleaves `count` records into the three arrays; any of them may be None."""
    return num_lib().chr_num_moments_unpack(_addr(n), _addr(mean), _addr(m2), _addr(recs), count, int(base),
                                            _stream(stream))


def release():
    """Free the ops and the cached types this library registered (chr_num_release); returns the status code."""
    return num_lib().chr_num_release()


def stats(reset=False):
    """(fold-launcher calls, tree-launcher calls, trees handed over) since the last reset (chr_num_stats)."""
    c = (ctypes.c_long * 3)()
    num_lib().chr_num_stats(c, 1 if reset else 0)
    return tuple(c)
