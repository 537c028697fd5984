"""MXFP6 block-scaled SUM and casts on the user-op interface: libchiara_mx6.so (include/chiara_mx6.h).

    from chiara_amd import mx6
    t, op = mx6.mx6_type(), mx6.mx6_sum(mx6.E2M3)              # the 400-byte tile type; also mx6.E3M2
    tiles = torch.empty(mx6.tiles_for(n) * mx6.TILE_BYTES, dtype=torch.uint8, device="cuda")
    mx6.quantize(tiles, x, n, ca.FLOAT32, mx6.E2M3, stream)    # 32 six-bit values share one E8M0 scale
    g.all_reduce_radix_batch(sends, recvs, mx6.tiles_for(n), t, op, k, b)
    mx6.dequantize(y, tiles, n, ca.BFLOAT16, mx6.E2M3, stream)
    mx6.release()                                              # the op and type codes go back

One element is a tile: 16 scale bytes, then 16 blocks of 32 six-bit codes, 24 bytes each with code i in bits 6i .. 6i+5,
512 values in 400 bytes, so every count is in tiles: 0.76 of chiara_amd.mx's bytes on the wire under the same rule, with
three (E2M3) or two (E3M2) mantissa bits where chiara_amd.mx4 keeps one.  Neither format has a NaN code: a NaN is a
block whose scale is 0xFF.  The op codes are valid wherever a user-defined op is; any dtype but a live
type_contiguous(100, UINT32) and any pointer that is not 4-byte aligned is refused (ERR_UNSUPPORTED, nothing enqueued).
The library is loaded on first use and registers nothing until asked; there is no fallback: a missing
libchiara_mx6.so is an error.

mx6_sum's ops carry the fold launcher alone, so the flat schedules' expression trees run fold by fold.
mx6_sum_tree(fmt) is the same SUM with the tree kernel of libchiara_mx6_tree.so (include/chiara_mx6_tree.h): one HBM
pass per tree (single-fold chains stay with the folds), the same bytes; tree_stats() counts its launchers' calls and
tree_release() frees its ops."""
import ctypes
import os

from ._lib import HERE, PKG_ROOT, ChiaraError, lib
from .collectives import SUCCESS, _addr, _stream

E2M3, E3M2 = 0, 1
TILE_VALUES, TILE_BYTES = 512, 400
MX6_LIB_PATH = os.path.join(HERE, "libchiara_mx6.so")

_mx6_lib = None


def mx6_lib():
    """libchiara_mx6.so, loaded on first use (libchiara.so, its dependency, is this process's copy)."""
    global _mx6_lib
    if _mx6_lib is None:
        lib()
        if not os.path.exists(MX6_LIB_PATH):
            raise ImportError(f"libchiara_mx6.so not found at {MX6_LIB_PATH}; build it with `make -C {PKG_ROOT}` "
                              f"(hipcc --offload-arch=gfx950) or __graft_entry__.build()")
        L = ctypes.CDLL(MX6_LIB_PATH)
        vp, ip, sz, i = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_size_t, ctypes.c_int
        for name, args in (("chr_mx6_type", [ip]), ("chr_mx6_sum", [i, ip]), ("chr_mx6_quantize", [vp, vp, sz, i, i, vp]),
                           ("chr_mx6_dequantize", [vp, vp, sz, i, i, vp]), ("chr_mx6_release", [])):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = ctypes.c_int
        L.chr_mx6_stats.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_int]
        L.chr_mx6_stats.restype = None
        _mx6_lib = L
    return _mx6_lib


def _code(fn, what, *args):
    out = ctypes.c_int(0)
    rc = fn(*args, ctypes.byref(out))
    if rc != SUCCESS:
        raise ChiaraError(rc, what)
    return out.value


def mx6_type():
    """The tile type, type_contiguous(100, UINT32), shared by both formats (chr_mx6_type): created on the first call,
    cached until release()."""
    return _code(mx6_lib().chr_mx6_type, "chr_mx6_type")


def mx6_sum(fmt):
    """The op code of the block-scaled SUM on tiles of format `fmt` (E2M3 or E3M2), registered on the first call for
    that format (chr_mx6_sum); the same code until release()."""
    return _code(mx6_lib().chr_mx6_sum, "chr_mx6_sum", int(fmt))


def tiles_for(n):
    """The tiles that hold n values: ceil(n / 512)."""
    return (int(n) + TILE_VALUES - 1) // TILE_VALUES


def quantize(tiles, src, n, src_type, fmt, stream=None):
    """tiles = Q(src) (chr_mx6_quantize): the n values of src, FLOAT32 or BFLOAT16, into tiles_for(n) whole tiles;
    tensors or addresses.  Enqueued on `stream`; returns the status code."""
    return mx6_lib().chr_mx6_quantize(_addr(tiles), _addr(src), n, int(src_type), int(fmt), _stream(stream))


def dequantize(dst, tiles, n, dst_type, fmt, stream=None):
    """dst[i] = dec(code i) * 2^(scale - 127) for i < n (chr_mx6_dequantize): dst of FLOAT32 or BFLOAT16; tensors or
    addresses.  Enqueued on `stream`; returns the status code."""
    return mx6_lib().chr_mx6_dequantize(_addr(dst), _addr(tiles), n, int(dst_type), int(fmt), _stream(stream))


def release():
    """Free the ops and the cached type this library registered (chr_mx6_release); returns the status code."""
    return mx6_lib().chr_mx6_release()


def stats(reset=False):
    """(fold-launcher calls, calls they declined, kernels they enqueued) since the last reset (chr_mx6_stats)."""
    c = (ctypes.c_long * 3)()
    mx6_lib().chr_mx6_stats(c, 1 if reset else 0)
    return tuple(c)


# ---- one-pass expression trees: libchiara_mx6_tree.so (include/chiara_mx6_tree.h) -----------------------------------

MX6_TREE_LIB_PATH = os.path.join(HERE, "libchiara_mx6_tree.so")

_mx6_tree_lib = None


def mx6_tree_lib():
    """libchiara_mx6_tree.so, loaded on first use (libchiara_mx6.so and libchiara.so, its dependencies, are this
    process's copies)."""
    global _mx6_tree_lib
    if _mx6_tree_lib is None:
        mx6_lib()
        if not os.path.exists(MX6_TREE_LIB_PATH):
            raise ImportError(f"libchiara_mx6_tree.so not found at {MX6_TREE_LIB_PATH}; build it with "
                              f"`make -C {PKG_ROOT}` (hipcc --offload-arch=gfx950) or __graft_entry__.build()")
        L = ctypes.CDLL(MX6_TREE_LIB_PATH)
        L.chr_mx6_sum_tree.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.chr_mx6_sum_tree.restype = ctypes.c_int
        L.chr_mx6_tree_release.argtypes = []
        L.chr_mx6_tree_release.restype = ctypes.c_int
        L.chr_mx6_tree_stats.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_int]
        L.chr_mx6_tree_stats.restype = None
        _mx6_tree_lib = L
    return _mx6_tree_lib


def mx6_sum_tree(fmt):
    """The op code of the same SUM on tiles of format `fmt` registered with its tree launcher (chr_mx6_sum_tree): the
    flat schedules' expression trees and reduce_tree(_batch) run in one HBM pass, the bytes are mx6_sum(fmt)'s.
    Another code than mx6_sum(fmt)'s, the same until tree_release()."""
    return _code(mx6_tree_lib().chr_mx6_sum_tree, "chr_mx6_sum_tree", int(fmt))


def tree_release():
    """Free the ops libchiara_mx6_tree.so registered (chr_mx6_tree_release); returns the status code."""
    return mx6_tree_lib().chr_mx6_tree_release()


def tree_stats(reset=False):
    """(tree-launcher calls, calls declined, trees handed over, kernels enqueued) since the last reset, both formats
    together (chr_mx6_tree_stats)."""
    c = (ctypes.c_long * 4)()
    mx6_tree_lib().chr_mx6_tree_stats(c, 1 if reset else 0)
    return tuple(c)
