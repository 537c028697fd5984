"""Reference for libchiara_mx4.so: include/chiara_mx4.h's rule in numpy, host only.  Tiles are uint8 arrays of whole
272-byte tiles; codes travel unpacked, one E2M1 code (0 .. 15) per value.  Every ldexp is tests/mx_ref.py's ldexp32
(float64 ldexp, one rounding to float32); the sum is one float32 add.  expected() evaluates the library's own plans
under tests/plan_sim.py with this rule on elements of dtype V272, as tests/mx_ref.py does it."""
import numpy as np
import pytest

import pyoracle as po
from fp8_ref import f32_to_bf16
from mx_ref import ldexp32

DTYPE, TILE = "mx4", np.dtype("V272")  # the name and the element the plan evaluator sees
TILE_BYTES, TILE_VALUES = 272, 512
MAGS = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6])  # code s eem: sign, then these in code order
TABLE = np.concatenate([MAGS, -MAGS])


def split(tiles):
    """(scales (n, 16) int64, codes (n, 16, 32) uint8 in 0 .. 15) of n whole tiles: value 2i is byte i's low nibble."""
    t = np.ascontiguousarray(tiles).view(np.uint8).reshape(-1, TILE_BYTES)
    b = t[:, 16:].reshape(-1, 16, 16)
    return t[:, :16].astype(np.int64), np.stack([b & 15, b >> 4], axis=-1).reshape(-1, 16, 32)


def join(scales, codes):
    c = np.asarray(codes, dtype=np.uint8).reshape(-1, 16, 16, 2)
    t = np.empty((c.shape[0], TILE_BYTES), dtype=np.uint8)
    t[:, :16] = scales
    t[:, 16:] = (c[..., 0] | c[..., 1] << 4).reshape(-1, 256)
    return t.reshape(-1)


def encode(r):
    """enc_sat: nearest of MAGS after the clamp to 6, ties to the even code, the sign kept whatever the magnitude."""
    a = np.minimum(np.abs(np.asarray(r, dtype=np.float64)), 6.0)
    hi = np.minimum(np.searchsorted(MAGS, a, side="left"), 7)  # first entry >= a
    lo = np.maximum(hi - 1, 0)
    d_lo, d_hi = a - MAGS[lo], MAGS[hi] - a
    pick = np.where(d_hi < d_lo, hi, np.where(d_lo < d_hi, lo, np.where(hi % 2 == 0, hi, lo)))
    return (np.where(np.signbit(r), 8, 0) | pick).astype(np.uint8)


def requantise(s, e, e_zero):
    """Steps 4 - 7 on finite float32 sums s (n, 16, 32) relative to scales e (n, 16): (new scales, codes)."""
    amax = np.abs(s).max(axis=-1)
    mant, x = np.frexp(amax.astype(np.float64))
    e2 = np.where(amax == 0, e_zero, np.clip(e + x - 3 + (mant > 0.75), 0, 254))
    return e2, encode(ldexp32(s, (e - e2)[..., None]))


def combine(x, y):
    """x o y = f(in = x, inout = y) on whole tiles; returns new tiles."""
    ex, px = split(x)
    ey, py = split(y)
    e = np.maximum(ex, ey)
    s = ldexp32(TABLE[py], (ey - e)[..., None]) + ldexp32(TABLE[px], (ex - e)[..., None])
    e2, codes = requantise(s, e, e)
    nan = (ex == 0xFF) | (ey == 0xFF)
    return join(np.where(nan, 0xFF, e2), np.where(nan[..., None], 0, codes))


def quantize_ref(src):
    """The tiles of the float32 values src: beyond len(src) the last tile holds +0; a non-finite value: a NaN block."""
    s = np.zeros((src.size + TILE_VALUES - 1) // TILE_VALUES * TILE_VALUES, dtype=np.float32)
    s[:src.size] = src
    s = s.reshape(-1, 16, 32)
    nan = ~np.isfinite(s).all(axis=-1)
    e2, codes = requantise(np.where(nan[..., None], np.float32(0), s), np.full(s.shape[:2], 127, dtype=np.int64), 0)
    return join(np.where(nan, 0xFF, e2), np.where(nan[..., None], 0, codes))


def dequantize_ref(tiles, n, bf16=False):
    """The first n values as uint32 bits of float32, or uint16 bits of bf16; a NaN is 0x7FC00000 / 0x7FC0."""
    e, p = split(tiles)
    v = np.where((e == 0xFF)[..., None], np.uint32(0x7FC00000).view(np.float32), ldexp32(TABLE[p], (e - 127)[..., None]))
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
        for x in ins:
            reduce_local(x, acc, dtype, op)
        return acc

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(po, "reduce_local", reduce_local)
        mp.setattr(po, "reduce_multi", reduce_multi)
        mp.setitem(po.NP_DTYPES, DTYPE, TILE)
        outs = plan_sim.simulate(mode, [np.array(s, dtype=np.uint8).view(TILE) for s in sends], k, b, DTYPE, "sum",
                                 schedule=schedule)
    return [np.ascontiguousarray(o).view(np.uint8) for o in outs]
