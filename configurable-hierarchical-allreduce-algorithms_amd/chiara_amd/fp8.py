"""OCP FP8 (E4M3 / E5M2) ops and scaled casts on the user-op interface: libchiara_fp8.so (include/chiara_fp8.h).

    from chiara_amd import fp8
    op = fp8.fp8_op(fp8.E4M3, ca.SUM, fp8.SATURATE)          # also PROD, MAX, MIN; E5M2; IEEE
    fp8.quantize(codes, x, n, ca.FLOAT32, fp8.E4M3, 1 / amax * 448, fp8.SATURATE, stream)
    g.all_reduce_radix_batch(sends, recvs, count, fp8.F8_DTYPE, op, k, b)
    fp8.dequantize(y, codes, n, ca.BFLOAT16, fp8.E4M3, amax / 448, stream)
    fp8.release()                                             # the codes go back to the 64 user-op codes

The elements are 1-byte codes (torch.float8_e4m3fn / torch.float8_e5m2, or uint8) and travel as UINT8; the op gives
them their meaning: one round-to-nearest-even per combine, subnormals kept, overflow to NaN (E4M3) / inf (E5M2) under
IEEE and to +-max under SATURATE, one canonical NaN (0x7F / 0x7E).  The op codes are valid wherever a user-defined op
is: every reduce_* entry point, the collectives on communicators and local groups, the MPICH baselines (the ops are
commutative).  Any other dtype is refused (ERR_UNSUPPORTED, nothing enqueued).  The library is loaded on first use and
registers nothing until asked; there is no fallback: a missing libchiara_fp8.so is an error."""
import ctypes
import os

from ._lib import HERE, PKG_ROOT, ChiaraError, lib
from .collectives import SUCCESS, UINT8, _addr, _stream

E4M3, E5M2 = 0, 1
IEEE, SATURATE = 0, 1
F8_DTYPE = UINT8
FP8_LIB_PATH = os.path.join(HERE, "libchiara_fp8.so")

_fp8_lib = None


def fp8_lib():
    """libchiara_fp8.so, loaded on first use (libchiara.so, its dependency, is this process's copy)."""
    global _fp8_lib
    if _fp8_lib is None:
        lib()
        if not os.path.exists(FP8_LIB_PATH):
            raise ImportError(f"libchiara_fp8.so not found at {FP8_LIB_PATH}; build it with `make -C {PKG_ROOT}` "
                              f"(hipcc --offload-arch=gfx950) or __graft_entry__.build()")
        L = ctypes.CDLL(FP8_LIB_PATH)
        L.chr_fp8_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.chr_fp8_op.restype = ctypes.c_int
        L.chr_fp8_quantize.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
        L.chr_fp8_quantize.restype = ctypes.c_int
        L.chr_fp8_dequantize.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_float, ctypes.c_void_p]
        L.chr_fp8_dequantize.restype = ctypes.c_int
        L.chr_fp8_release.argtypes = []
        L.chr_fp8_release.restype = ctypes.c_int
        L.chr_fp8_stats.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_int]
        L.chr_fp8_stats.restype = None
        _fp8_lib = L
    return _fp8_lib


def fp8_op(fmt, kind, overflow=IEEE):
    """The op code of `kind` (SUM, PROD, MAX or MIN) on format `fmt` under `overflow`, registered on the first call
    for that combination (chr_fp8_op); the same code until release().  MAX and MIN have one code for both policies."""
    op = ctypes.c_int(0)
    rc = fp8_lib().chr_fp8_op(int(fmt), int(kind), int(overflow), ctypes.byref(op))
    if rc != SUCCESS:
        raise ChiaraError(rc, "chr_fp8_op")
    return op.value


def quantize(dst, src, n, src_type, fmt, scale=1.0, overflow=IEEE, stream=None):
    """dst[i] = enc(f32(src[i]) * scale) for i < n (chr_fp8_quantize): src of FLOAT32 or BFLOAT16, dst n bytes;
    tensors or addresses.  Enqueued on `stream`; returns the status code."""
    return fp8_lib().chr_fp8_quantize(_addr(dst), _addr(src), n, int(src_type), int(fmt), float(scale), int(overflow),
                                      _stream(stream))


def dequantize(dst, src, n, dst_type, fmt, scale=1.0, stream=None):
    """dst[i] = round(dec(src[i]) * scale) for i < n (chr_fp8_dequantize): dst of FLOAT32 or BFLOAT16; tensors or
    addresses.  Enqueued on `stream`; returns the status code."""
    return fp8_lib().chr_fp8_dequantize(_addr(dst), _addr(src), n, int(dst_type), int(fmt), float(scale),
                                        _stream(stream))


def release():
    """Free every op this library registered (chr_fp8_release); returns the status code."""
    return fp8_lib().chr_fp8_release()


def stats(reset=False):
    """(fold-launcher calls, tree-launcher calls, trees handed over) since the last reset (chr_fp8_stats)."""
    c = (ctypes.c_long * 3)()
    fp8_lib().chr_fp8_stats(c, 1 if reset else 0)
    return tuple(c)
