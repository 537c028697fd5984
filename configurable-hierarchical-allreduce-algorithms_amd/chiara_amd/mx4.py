"""MXFP4 block-scaled SUM and casts on the user-op interface: libchiara_mx4.so (include/chiara_mx4.h).

    from chiara_amd import mx4
    t, op = mx4.mx4_type(), mx4.mx4_sum()                      # the 272-byte tile type and the SUM on it
    tiles = torch.empty(mx4.tiles_for(n) * mx4.TILE_BYTES, dtype=torch.uint8, device="cuda")
    mx4.quantize(tiles, x, n, ca.FLOAT32, stream)              # 32 E2M1 values share one E8M0 scale
    g.all_reduce_radix_batch(sends, recvs, mx4.tiles_for(n), t, op, k, b)
    mx4.dequantize(y, tiles, n, ca.BFLOAT16, stream)
    mx4.release()                                              # the op and type codes go back

One element is a tile: 16 scale bytes, then 16 blocks of 32 four-bit codes, two to a byte, 512 values in 272 bytes, so
every count is in tiles: half of chiara_amd.mx's bytes on the wire under the same rule.  E2M1 has no NaN code: a NaN is
a block whose scale is 0xFF.  The op code is valid wherever a user-defined op is; any dtype but a live
type_contiguous(68, UINT32) and any pointer that is not 4-byte aligned is refused (ERR_UNSUPPORTED, nothing enqueued).
The library is loaded on first use and registers nothing until asked; there is no fallback: a missing
libchiara_mx4.so is an error.

mx4_sum's op carries the fold launcher alone, so the flat schedules' expression trees run fold by fold.
mx4_sum_tree() is the same SUM with the tree kernel of libchiara_mx4_tree.so (include/chiara_mx4_tree.h): one HBM
pass per tree of up to 31 775 tiles (larger ones and single-fold chains stay with the folds, which measured faster
there), the same bytes; tree_stats() counts its launcher's calls and tree_release() frees its op.

mx4_sum_sr() and quantize_sr() are the SUM and the quantize with stochastic rounding of libchiara_mx4_sr.so
(include/chiara_mx4_sr.h) on the same tiles, for gradients: sr_set_seed(step) on every rank before each collective,
dequantize() as before, sr_stats() and sr_release() like their namesakes."""
import ctypes
import os

from ._lib import HERE, PKG_ROOT, ChiaraError, lib
from .collectives import SUCCESS, _addr, _stream

TILE_VALUES, TILE_BYTES = 512, 272
MX4_LIB_PATH = os.path.join(HERE, "libchiara_mx4.so")

_mx4_lib = None


def mx4_lib():
    """libchiara_mx4.so, loaded on first use (libchiara.so, its dependency, is this process's copy)."""
    global _mx4_lib
    if _mx4_lib is None:
        lib()
        if not os.path.exists(MX4_LIB_PATH):
            raise ImportError(f"libchiara_mx4.so not found at {MX4_LIB_PATH}; build it with `make -C {PKG_ROOT}` "
                              f"(hipcc --offload-arch=gfx950) or __graft_entry__.build()")
        L = ctypes.CDLL(MX4_LIB_PATH)
        vp, ip, sz, i = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_size_t, ctypes.c_int
        for name, args in (("chr_mx4_type", [ip]), ("chr_mx4_sum", [ip]), ("chr_mx4_quantize", [vp, vp, sz, i, vp]),
                           ("chr_mx4_dequantize", [vp, vp, sz, i, vp]), ("chr_mx4_release", [])):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = ctypes.c_int
        L.chr_mx4_stats.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_int]
        L.chr_mx4_stats.restype = None
        _mx4_lib = L
    return _mx4_lib


def _code(fn, what):
    out = ctypes.c_int(0)
    rc = fn(ctypes.byref(out))
    if rc != SUCCESS:
        raise ChiaraError(rc, what)
    return out.value


def mx4_type():
    """The tile type, type_contiguous(68, UINT32) (chr_mx4_type): created on the first call, cached until release()."""
    return _code(mx4_lib().chr_mx4_type, "chr_mx4_type")


def mx4_sum():
    """The op code of the block-scaled SUM on MX4 tiles, registered on the first call (chr_mx4_sum); the same code
    until release()."""
    return _code(mx4_lib().chr_mx4_sum, "chr_mx4_sum")


def tiles_for(n):
    """The tiles that hold n values: ceil(n / 512)."""
    return (int(n) + TILE_VALUES - 1) // TILE_VALUES


def quantize(tiles, src, n, src_type, stream=None):
    """tiles = Q(src) (chr_mx4_quantize): the n values of src, FLOAT32 or BFLOAT16, into tiles_for(n) whole tiles;
    tensors or addresses.  Enqueued on `stream`; returns the status code."""
    return mx4_lib().chr_mx4_quantize(_addr(tiles), _addr(src), n, int(src_type), _stream(stream))


def dequantize(dst, tiles, n, dst_type, stream=None):
    """dst[i] = dec(code i) * 2^(scale - 127) for i < n (chr_mx4_dequantize): dst of FLOAT32 or BFLOAT16; tensors or
    addresses.  Enqueued on `stream`; returns the status code."""
    return mx4_lib().chr_mx4_dequantize(_addr(dst), _addr(tiles), n, int(dst_type), _stream(stream))


def release():
    """Free the op and the cached type this library registered (chr_mx4_release); returns the status code."""
    return mx4_lib().chr_mx4_release()


def stats(reset=False):
    """(fold-launcher calls, calls it declined, kernels it enqueued) since the last reset (chr_mx4_stats)."""
    c = (ctypes.c_long * 3)()
    mx4_lib().chr_mx4_stats(c, 1 if reset else 0)
    return tuple(c)


# ---- one-pass expression trees: libchiara_mx4_tree.so (include/chiara_mx4_tree.h) -----------------------------------

MX4_TREE_LIB_PATH = os.path.join(HERE, "libchiara_mx4_tree.so")

_mx4_tree_lib = None


def mx4_tree_lib():
    """libchiara_mx4_tree.so, loaded on first use (libchiara_mx4.so and libchiara.so, its dependencies, are this
    process's copies)."""
    global _mx4_tree_lib
    if _mx4_tree_lib is None:
        mx4_lib()
        if not os.path.exists(MX4_TREE_LIB_PATH):
            raise ImportError(f"libchiara_mx4_tree.so not found at {MX4_TREE_LIB_PATH}; build it with `make -C {PKG_ROOT}` "
                              f"(hipcc --offload-arch=gfx950) or __graft_entry__.build()")
        L = ctypes.CDLL(MX4_TREE_LIB_PATH)
        L.chr_mx4_sum_tree.argtypes = [ctypes.POINTER(ctypes.c_int)]
        L.chr_mx4_sum_tree.restype = ctypes.c_int
        L.chr_mx4_tree_release.argtypes = []
        L.chr_mx4_tree_release.restype = ctypes.c_int
        L.chr_mx4_tree_stats.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_int]
        L.chr_mx4_tree_stats.restype = None
        _mx4_tree_lib = L
    return _mx4_tree_lib


def mx4_sum_tree():
    """The op code of the same SUM registered with its tree launcher (chr_mx4_sum_tree): the flat schedules' expression
    trees and reduce_tree(_batch) run in one HBM pass, the bytes are mx4_sum's.  Another code than mx4_sum()'s, the
    same until tree_release()."""
    return _code(mx4_tree_lib().chr_mx4_sum_tree, "chr_mx4_sum_tree")


def tree_release():
    """Free the op libchiara_mx4_tree.so registered (chr_mx4_tree_release); returns the status code."""
    return mx4_tree_lib().chr_mx4_tree_release()


def tree_stats(reset=False):
    """(tree-launcher calls, calls declined, trees handed over, kernels enqueued) since the last reset
    (chr_mx4_tree_stats)."""
    c = (ctypes.c_long * 4)()
    mx4_tree_lib().chr_mx4_tree_stats(c, 1 if reset else 0)
    return tuple(c)


# ---- stochastic rounding: libchiara_mx4_sr.so (include/chiara_mx4_sr.h) ----------------------------------------------

MX4_SR_LIB_PATH = os.path.join(HERE, "libchiara_mx4_sr.so")

_mx4_sr_lib = None


def mx4_sr_lib():
    """libchiara_mx4_sr.so, loaded on first use (libchiara_mx4.so and libchiara.so, its dependencies, are this
    process's copies)."""
    global _mx4_sr_lib
    if _mx4_sr_lib is None:
        mx4_lib()
        if not os.path.exists(MX4_SR_LIB_PATH):
            raise ImportError(f"libchiara_mx4_sr.so not found at {MX4_SR_LIB_PATH}; build it with `make -C {PKG_ROOT}` "
                              f"(hipcc --offload-arch=gfx950) or __graft_entry__.build()")
        L = ctypes.CDLL(MX4_SR_LIB_PATH)
        vp, sz, i, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
        L.chr_mx4_sr_sum.argtypes = [ctypes.POINTER(ctypes.c_int)]
        L.chr_mx4_sr_sum.restype = ctypes.c_int
        L.chr_mx4_sr_set_seed.argtypes = [u32]
        L.chr_mx4_sr_set_seed.restype = None
        L.chr_mx4_sr_quantize.argtypes = [vp, vp, sz, i, u32, vp]
        L.chr_mx4_sr_quantize.restype = ctypes.c_int
        L.chr_mx4_sr_release.argtypes = []
        L.chr_mx4_sr_release.restype = ctypes.c_int
        L.chr_mx4_sr_stats.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_int]
        L.chr_mx4_sr_stats.restype = None
        _mx4_sr_lib = L
    return _mx4_sr_lib


def mx4_sum_sr():
    """The op code of the SUM that rounds stochastically (chr_mx4_sr_sum) on mx4_type()'s tiles: the fold launcher
    alone, so trees run fold by fold.  The random bits are a function of the seed, the place in the tile and the
    operands' bits: the same bytes on every rank and under every slicing.  The same code until sr_release()."""
    return _code(mx4_sr_lib().chr_mx4_sr_sum, "chr_mx4_sr_sum")


def sr_set_seed(seed):
    """The seed of every later SR SUM of this process (chr_mx4_sr_set_seed; default 0), read at enqueue time.  Every
    rank sets the same value before the same collective, and a new one every step: unbiasedness is over seeds."""
    mx4_sr_lib().chr_mx4_sr_set_seed(int(seed) & 0xFFFFFFFF)


def quantize_sr(tiles, src, n, src_type, seed, stream=None):
    """tiles = Q_sr(src) (chr_mx4_sr_quantize): quantize() with stochastic rounding under `seed`, keyed on the tile's
    index as well.  Enqueued on `stream`; returns the status code.  dequantize() reads the result."""
    return mx4_sr_lib().chr_mx4_sr_quantize(_addr(tiles), _addr(src), n, int(src_type), int(seed) & 0xFFFFFFFF, _stream(stream))


def sr_release():
    """Free the op libchiara_mx4_sr.so registered (chr_mx4_sr_release); returns the status code."""
    return mx4_sr_lib().chr_mx4_sr_release()


def sr_stats(reset=False):
    """(fold-launcher calls, calls it declined, kernels it enqueued) since the last reset (chr_mx4_sr_stats)."""
    c = (ctypes.c_long * 3)()
    mx4_sr_lib().chr_mx4_sr_stats(c, 1 if reset else 0)
    return tuple(c)
