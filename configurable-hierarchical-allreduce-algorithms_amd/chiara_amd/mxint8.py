"""MXINT8 block-scaled SUM and casts on the user-op interface: libchiara_mxint8.so (include/chiara_mxint8.h).

    from chiara_amd import mxint8
    t, op = mxint8.mxint8_type(), mxint8.mxint8_sum()          # the 528-byte tile type and the SUM
    tiles = torch.empty(mxint8.tiles_for(n) * mxint8.TILE_BYTES, dtype=torch.uint8, device="cuda")
    mxint8.quantize(tiles, x, n, ca.FLOAT32, stream)           # 32 int8 codes share one E8M0 scale
    g.all_reduce_radix_batch(sends, recvs, mxint8.tiles_for(n), t, op, k, b)
    mxint8.dequantize(y, tiles, n, ca.BFLOAT16, stream)
    mxint8.release()                                           # the op and type codes go back

One element is a tile, chiara_amd.mx's layout: 16 scale bytes, then 16 blocks of 32 two's-complement codes, a code's
value being code / 64; 512 values in 528 bytes, so every count is in tiles.  A uniform grid with seven magnitude bits
where MXFP8 E4M3 keeps three mantissa bits.  There is no NaN code: a NaN is a block whose scale is 0xFF.  The op code
is valid wherever a user-defined op is; any dtype but a live type_contiguous(132, UINT32) and any pointer that is not
4-byte aligned is refused (ERR_UNSUPPORTED, nothing enqueued).  The library is loaded on first use and registers
nothing until asked; there is no fallback: a missing libchiara_mxint8.so is an error.

mxint8_sum's op carries the fold launcher alone, so the flat schedules' expression trees run fold by fold.
mxint8_sum_tree() is the same SUM with the tree kernel of libchiara_mxint8_tree.so (include/chiara_mxint8_tree.h): one
HBM pass per tree (single-fold chains stay with the folds), the same bytes; tree_stats() counts its launcher's calls
and tree_release() frees its op."""
import ctypes
import os

from ._lib import HERE, PKG_ROOT, ChiaraError, lib
from .collectives import SUCCESS, _addr, _stream

TILE_VALUES, TILE_BYTES = 512, 528
MXINT8_LIB_PATH = os.path.join(HERE, "libchiara_mxint8.so")

_mxint8_lib = None


def mxint8_lib():
    """libchiara_mxint8.so, loaded on first use (libchiara.so, its dependency, is this process's copy)."""
    global _mxint8_lib
    if _mxint8_lib is None:
        lib()
        if not os.path.exists(MXINT8_LIB_PATH):
            raise ImportError(f"libchiara_mxint8.so not found at {MXINT8_LIB_PATH}; build it with `make -C {PKG_ROOT}` "
                              f"(hipcc --offload-arch=gfx950) or __graft_entry__.build()")
        L = ctypes.CDLL(MXINT8_LIB_PATH)
        vp, ip, sz, i = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_size_t, ctypes.c_int
        for name, args in (("chr_mxi8_type", [ip]), ("chr_mxi8_sum", [ip]), ("chr_mxi8_quantize", [vp, vp, sz, i, vp]),
                           ("chr_mxi8_dequantize", [vp, vp, sz, i, vp]), ("chr_mxi8_release", [])):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = ctypes.c_int
        L.chr_mxi8_stats.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_int]
        L.chr_mxi8_stats.restype = None
        _mxint8_lib = L
    return _mxint8_lib


def _code(fn, what):
    out = ctypes.c_int(0)
    rc = fn(ctypes.byref(out))
    if rc != SUCCESS:
        raise ChiaraError(rc, what)
    return out.value


def mxint8_type():
    """The tile type, type_contiguous(132, UINT32) (chr_mxi8_type): created on the first call, cached until release()."""
    return _code(mxint8_lib().chr_mxi8_type, "chr_mxi8_type")


def mxint8_sum():
    """The op code of the block-scaled SUM, registered on the first call (chr_mxi8_sum); the same code until release()."""
    return _code(mxint8_lib().chr_mxi8_sum, "chr_mxi8_sum")


def tiles_for(n):
    """The tiles that hold n values: ceil(n / 512)."""
    return (int(n) + TILE_VALUES - 1) // TILE_VALUES


def quantize(tiles, src, n, src_type, stream=None):
    """tiles = Q(src) (chr_mxi8_quantize): the n values of src, FLOAT32 or BFLOAT16, into tiles_for(n) whole tiles;
    tensors or addresses.  Enqueued on `stream`; returns the status code."""
    return mxint8_lib().chr_mxi8_quantize(_addr(tiles), _addr(src), n, int(src_type), _stream(stream))


def dequantize(dst, tiles, n, dst_type, stream=None):
    """dst[i] = code i / 64 * 2^(scale - 127) for i < n (chr_mxi8_dequantize): dst of FLOAT32 or BFLOAT16; tensors or
    addresses.  Enqueued on `stream`; returns the status code."""
    return mxint8_lib().chr_mxi8_dequantize(_addr(dst), _addr(tiles), n, int(dst_type), _stream(stream))


def release():
    """Free the op and the cached type this library registered (chr_mxi8_release); returns the status code."""
    return mxint8_lib().chr_mxi8_release()


def stats(reset=False):
    """(fold-launcher calls, calls it declined, kernels it enqueued) since the last reset (chr_mxi8_stats)."""
    c = (ctypes.c_long * 3)()
    mxint8_lib().chr_mxi8_stats(c, 1 if reset else 0)
    return tuple(c)


# ---- one-pass expression trees: libchiara_mxint8_tree.so (include/chiara_mxint8_tree.h) -----------------------------

MXINT8_TREE_LIB_PATH = os.path.join(HERE, "libchiara_mxint8_tree.so")

_mxint8_tree_lib = None


def mxint8_tree_lib():
    """libchiara_mxint8_tree.so, loaded on first use (libchiara_mxint8.so and libchiara.so, its dependencies, are this
    process's copies)."""
    global _mxint8_tree_lib
    if _mxint8_tree_lib is None:
        mxint8_lib()
        if not os.path.exists(MXINT8_TREE_LIB_PATH):
            raise ImportError(f"libchiara_mxint8_tree.so not found at {MXINT8_TREE_LIB_PATH}; build it with "
                              f"`make -C {PKG_ROOT}` (hipcc --offload-arch=gfx950) or __graft_entry__.build()")
        L = ctypes.CDLL(MXINT8_TREE_LIB_PATH)
        L.chr_mxi8_sum_tree.argtypes = [ctypes.POINTER(ctypes.c_int)]
        L.chr_mxi8_sum_tree.restype = ctypes.c_int
        L.chr_mxi8_tree_release.argtypes = []
        L.chr_mxi8_tree_release.restype = ctypes.c_int
        L.chr_mxi8_tree_stats.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_int]
        L.chr_mxi8_tree_stats.restype = None
        _mxint8_tree_lib = L
    return _mxint8_tree_lib


def mxint8_sum_tree():
    """The op code of the same SUM registered with its tree launcher (chr_mxi8_sum_tree): the flat schedules'
    expression trees and reduce_tree(_batch) run in one HBM pass, the bytes are mxint8_sum's.  Another code than
    mxint8_sum()'s, the same until tree_release()."""
    return _code(mxint8_tree_lib().chr_mxi8_sum_tree, "chr_mxi8_sum_tree")


def tree_release():
    """Free the op libchiara_mxint8_tree.so registered (chr_mxi8_tree_release); returns the status code."""
    return mxint8_tree_lib().chr_mxi8_tree_release()


def tree_stats(reset=False):
    """(tree-launcher calls, calls declined, trees handed over, kernels enqueued) since the last reset
    (chr_mxi8_tree_stats)."""
    c = (ctypes.c_long * 4)()
    mxint8_tree_lib().chr_mxi8_tree_stats(c, 1 if reset else 0)
    return tuple(c)
