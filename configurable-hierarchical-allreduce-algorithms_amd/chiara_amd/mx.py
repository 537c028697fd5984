"""MXFP8 block-scaled SUM and casts on the user-op interface: libchiara_mx.so (include/chiara_mx.h).

    from chiara_amd import mx, fp8
    t, op = mx.mx_type(), mx.mx_sum(fp8.E4M3)                 # the 528-byte tile type; also fp8.E5M2
    tiles = torch.empty(mx.tiles_for(n) * mx.TILE_BYTES, dtype=torch.uint8, device="cuda")
    mx.quantize(tiles, x, n, ca.FLOAT32, fp8.E4M3, stream)    # 32 values share one E8M0 scale
    g.all_reduce_radix_batch(sends, recvs, mx.tiles_for(n), t, op, k, b)
    mx.dequantize(y, tiles, n, ca.BFLOAT16, fp8.E4M3, stream)
    mx.release()                                              # the op and type codes go back

One element is a tile: 16 scale bytes, then 16 blocks of 32 FP8 codes, 512 values in 528 bytes, so every count is in
tiles.  A combine aligns the two scales of a block, adds in f32, and re-encodes under the smallest scale that fits the
block's new amax: partial sums never leave the format's range the way they do under one scale per tensor.  The op
codes are valid wherever a user-defined op is; any dtype but a live type_contiguous(132, UINT32) and any pointer that
is not 4-byte aligned is refused (ERR_UNSUPPORTED, nothing enqueued).  The library is loaded on first use and
registers nothing until asked; there is no fallback: a missing libchiara_mx.so is an error.

mx_sum's op carries the fold launcher alone, so the flat schedules' expression trees run fold by fold.
mx_sum_tree(fmt) is the same SUM with the tree kernel of libchiara_mx_tree.so (include/chiara_mx_tree.h): one HBM
pass per tree, the same bytes; tree_stats() counts its launcher's calls and tree_release() frees its ops."""
import ctypes
import os

from ._lib import HERE, PKG_ROOT, ChiaraError, lib
from .collectives import SUCCESS, _addr, _stream

TILE_VALUES, TILE_BYTES = 512, 528
MX_LIB_PATH = os.path.join(HERE, "libchiara_mx.so")

_mx_lib = None


def mx_lib():
    """libchiara_mx.so, loaded on first use (libchiara.so, its dependency, is this process's copy)."""
    global _mx_lib
    if _mx_lib is None:
        lib()
        if not os.path.exists(MX_LIB_PATH):
            raise ImportError(f"libchiara_mx.so not found at {MX_LIB_PATH}; build it with `make -C {PKG_ROOT}` "
                              f"(hipcc --offload-arch=gfx950) or __graft_entry__.build()")
        L = ctypes.CDLL(MX_LIB_PATH)
        vp, ip, sz, i = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_size_t, ctypes.c_int
        for name, args in (("chr_mx_type", [ip]), ("chr_mx_sum", [i, ip]), ("chr_mx_quantize", [vp, vp, sz, i, i, vp]),
                           ("chr_mx_dequantize", [vp, vp, sz, i, i, vp]), ("chr_mx_release", [])):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = ctypes.c_int
        L.chr_mx_stats.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_int]
        L.chr_mx_stats.restype = None
        _mx_lib = L
    return _mx_lib


def _code(fn, what, *args):
    out = ctypes.c_int(0)
    rc = fn(*args, ctypes.byref(out))
    if rc != SUCCESS:
        raise ChiaraError(rc, what)
    return out.value


def mx_type():
    """The tile type, type_contiguous(132, UINT32) (chr_mx_type): created on the first call, cached until release()."""
    return _code(mx_lib().chr_mx_type, "chr_mx_type")


def mx_sum(fmt):
    """The op code of the block-scaled SUM on tiles of format `fmt` (fp8.E4M3 or fp8.E5M2), registered on the first
    call for that format (chr_mx_sum); the same code until release()."""
    return _code(mx_lib().chr_mx_sum, "chr_mx_sum", int(fmt))


def tiles_for(n):
    """The tiles that hold n values: ceil(n / 512)."""
    return (int(n) + TILE_VALUES - 1) // TILE_VALUES


def quantize(tiles, src, n, src_type, fmt, stream=None):
    """tiles = Q(src) (chr_mx_quantize): the n values of src, FLOAT32 or BFLOAT16, into tiles_for(n) whole tiles;
    tensors or addresses.  Enqueued on `stream`; returns the status code."""
    return mx_lib().chr_mx_quantize(_addr(tiles), _addr(src), n, int(src_type), int(fmt), _stream(stream))


def dequantize(dst, tiles, n, dst_type, fmt, stream=None):
    """dst[i] = dec(code i) * 2^(scale - 127) for i < n (chr_mx_dequantize): dst of FLOAT32 or BFLOAT16; tensors or
    addresses.  Enqueued on `stream`; returns the status code."""
    return mx_lib().chr_mx_dequantize(_addr(dst), _addr(tiles), n, int(dst_type), int(fmt), _stream(stream))


def release():
    """Free the ops and the cached type this library registered (chr_mx_release); returns the status code."""
    return mx_lib().chr_mx_release()


def stats(reset=False):
    """(fold-launcher calls, calls it declined, kernels it enqueued) since the last reset (chr_mx_stats)."""
    c = (ctypes.c_long * 3)()
    mx_lib().chr_mx_stats(c, 1 if reset else 0)
    return tuple(c)


# ---- one-pass expression trees: libchiara_mx_tree.so (include/chiara_mx_tree.h) -------------------------------------

MX_TREE_LIB_PATH = os.path.join(HERE, "libchiara_mx_tree.so")

_mx_tree_lib = None


def mx_tree_lib():
    """libchiara_mx_tree.so, loaded on first use (libchiara_mx.so and libchiara.so, its dependencies, are this
    process's copies)."""
    global _mx_tree_lib
    if _mx_tree_lib is None:
        mx_lib()
        if not os.path.exists(MX_TREE_LIB_PATH):
            raise ImportError(f"libchiara_mx_tree.so not found at {MX_TREE_LIB_PATH}; build it with `make -C {PKG_ROOT}` "
                              f"(hipcc --offload-arch=gfx950) or __graft_entry__.build()")
        L = ctypes.CDLL(MX_TREE_LIB_PATH)
        L.chr_mx_sum_tree.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.chr_mx_sum_tree.restype = ctypes.c_int
        L.chr_mx_tree_release.argtypes = []
        L.chr_mx_tree_release.restype = ctypes.c_int
        L.chr_mx_tree_stats.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_int]
        L.chr_mx_tree_stats.restype = None
        _mx_tree_lib = L
    return _mx_tree_lib


def mx_sum_tree(fmt):
    """The op code of the same SUM registered with its tree launcher (chr_mx_sum_tree): the flat schedules' expression
    trees and reduce_tree(_batch) run in one HBM pass, the bytes are mx_sum's.  Another code than mx_sum(fmt)'s, the
    same until tree_release()."""
    return _code(mx_tree_lib().chr_mx_sum_tree, "chr_mx_sum_tree", int(fmt))


def tree_release():
    """Free the ops libchiara_mx_tree.so registered (chr_mx_tree_release); returns the status code."""
    return mx_tree_lib().chr_mx_tree_release()


def tree_stats(reset=False):
    """(tree-launcher calls, calls declined, trees handed over, kernels enqueued) since the last reset
    (chr_mx_tree_stats)."""
    c = (ctypes.c_long * 4)()
    mx_tree_lib().chr_mx_tree_stats(c, 1 if reset else 0)
    return tuple(c)
