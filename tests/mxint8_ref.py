"""Reference for libchiara_mxint8.so: include/chiara_mxint8.h's rule in numpy, host only.  Tiles are uint8 arrays of
whole 528-byte tiles, tests/mx_ref.py's layout.  Every ldexp is mx_ref.ldexp32; the sum is one float32 add; the encode
is np.rint (half to even) of the value times 64, clipped to +-127.  expected() evaluates the library's own plans under
tests/plan_sim.py, as mx6_ref.py does."""
import functools

import numpy as np
import pytest

import pyoracle as po
from fp8_ref import f32_to_bf16
from mx_ref import join, ldexp32, split

DTYPE, TILE = "mxint8", np.dtype("V528")  # the name and the element the plan evaluator sees
TILE_BYTES, TILE_VALUES = 528, 512
THRESHOLD, MAX_EXP = 127 / 128, 1  # max = 127/64 = THRESHOLD * 2^MAX_EXP


def decode(codes):
    return np.asarray(codes, dtype=np.uint8).view(np.int8) / 64.0


def encode(r):
    """enc_sat: the nearest multiple of 1/64, ties to the even code, clipped to +-127/64; no 0x80 and no -0."""
    return np.clip(np.rint(np.asarray(r, dtype=np.float64) * 64), -127, 127).astype(np.int8).view(np.uint8)


def requantise(s, e, e_zero):
    """Steps 4 - 7 on finite float32 sums s (n, 16, 32) relative to scales e (n, 16): (new scales, codes)."""
    amax = np.abs(s).max(axis=-1)
    mant, x = np.frexp(amax.astype(np.float64))
    e2 = np.where(amax == 0, e_zero, np.clip(e + x - MAX_EXP + (mant > THRESHOLD), 0, 254))
    return e2, encode(ldexp32(s, (e - e2)[..., None]))


def combine(x, y):
    """x o y = f(in = x, inout = y) on whole tiles; returns new tiles."""
    ex, px = split(x)
    ey, py = split(y)
    e = np.maximum(ex, ey)
    s = ldexp32(decode(py), (ey - e)[..., None]) + ldexp32(decode(px), (ex - e)[..., None])
    e2, codes = requantise(s, e, e)
    nan = (ex == 0xFF) | (ey == 0xFF)
    return join(np.where(nan, 0xFF, e2), np.where(nan[..., None], 0, codes).astype(np.uint8))


def quantize_ref(src):
    """The tiles of the float32 values src: beyond len(src) the last tile holds +0; a non-finite value: a NaN block."""
    s = np.zeros(((src.size + TILE_VALUES - 1) // TILE_VALUES, 16, 32), dtype=np.float32)
    s.reshape(-1)[:src.size] = src
    nan = ~np.isfinite(s).all(axis=-1)
    e2, codes = requantise(np.where(nan[..., None], np.float32(0), s), np.full(s.shape[:2], 127, dtype=np.int64), 0)
    return join(np.where(nan, 0xFF, e2), np.where(nan[..., None], 0, codes).astype(np.uint8))


def dequantize_ref(tiles, n, bf16=False):
    """The first n values as uint32 bits of float32, or uint16 bits of bf16; a NaN is 0x7FC00000 / 0x7FC0."""
    e, p = split(tiles)
    v = np.where((e == 0xFF)[..., None], np.uint32(0x7FC00000).view(np.float32), ldexp32(decode(p), (e - 127)[..., None]))
    v = v.astype(np.float32).reshape(-1)[:n]
    return f32_to_bf16(v) if bf16 else v.view(np.uint32)


def expected(mode, sends, k, b, schedule):
    """Every rank's output tiles of a collective: the library's plan under the plan evaluator over this rule."""
    import plan_sim

    def reduce_local(inp, inout, dtype, op):  # pyoracle.reduce_local's contract: inout = inp o inout, in place
        assert dtype == DTYPE and op == "sum" and inp.size == inout.size
        inout[:] = combine(inp, inout).view(TILE)
        return inout

    def reduce_multi(acc, ins, dtype, op):
        return functools.reduce(lambda a, x: reduce_local(x, a, dtype, op), ins, acc)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(po, "reduce_local", reduce_local)
        mp.setattr(po, "reduce_multi", reduce_multi)
        mp.setitem(po.NP_DTYPES, DTYPE, TILE)
        outs = plan_sim.simulate(mode, [np.array(s, dtype=np.uint8).view(TILE) for s in sends], k, b, DTYPE, "sum",
                                 schedule=schedule)
    return [np.ascontiguousarray(o).view(np.uint8) for o in outs]
