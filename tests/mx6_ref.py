"""Reference for libchiara_mx6.so: include/chiara_mx6.h's rule in numpy, host only.  Tiles are uint8 arrays of whole
400-byte tiles; codes travel unpacked, one six-bit code (0 .. 63) per value.  Every ldexp is tests/mx_ref.py's ldexp32;
the sum is one float32 add.  expected() evaluates the library's own plans under tests/plan_sim.py, as mx4_ref.py does."""
import functools

import numpy as np
import pytest

import pyoracle as po
from fp8_ref import f32_to_bf16
from mx_ref import ldexp32

E2M3, E3M2 = 0, 1
DTYPE, TILE = "mx6", np.dtype("V400")  # the name and the element the plan evaluator sees
TILE_BYTES, TILE_VALUES = 400, 512
MAN_BITS, EXP_BIAS, MAX_EXP = {E2M3: 3, E3M2: 2}, {E2M3: 1, E3M2: 3}, {E2M3: 3, E3M2: 5}


def _mags(fmt):
    """The 32 magnitudes in code order, from the bit fields: subnormals m * 2^(1 - bias - M), else (1 + m/2^M) * 2^(e - bias)."""
    m_bits, bias = MAN_BITS[fmt], EXP_BIAS[fmt]
    e, m = np.divmod(np.arange(32), 1 << m_bits)
    return np.where(e == 0, np.ldexp(m.astype(np.float64), 1 - bias - m_bits), np.ldexp(1 + m / (1 << m_bits), e - bias))


MAGS = {f: _mags(f) for f in (E2M3, E3M2)}
TABLE = {f: np.concatenate([MAGS[f], -MAGS[f]]) for f in MAGS}  # the value of every code; -0 is code 0x20
THRESHOLD = {f: MAGS[f][31] / 2.0 ** MAX_EXP[f] for f in MAGS}  # max = THRESHOLD * 2^MAX_EXP: 0.9375 and 0.875


def split(tiles):
    """(scales (n, 16) int64, codes (n, 16, 32) uint8 in 0 .. 63): code i is bits 6i .. 6i+5 of its block's 24 bytes."""
    t = np.ascontiguousarray(tiles).view(np.uint8).reshape(-1, TILE_BYTES)
    bits = np.unpackbits(t[:, 16:].reshape(-1, 16, 24), axis=-1, bitorder="little").reshape(-1, 16, 32, 6)
    return t[:, :16].astype(np.int64), np.packbits(bits, axis=-1, bitorder="little")[..., 0]


def join(scales, codes):
    c = np.asarray(codes, dtype=np.uint8).reshape(-1, 16, 32, 1)
    bits = np.unpackbits(c, axis=-1, bitorder="little")[..., :6].reshape(-1, 16, 192)
    t = np.empty((c.shape[0], TILE_BYTES), dtype=np.uint8)
    t[:, :16] = scales
    t[:, 16:] = np.packbits(bits, axis=-1, bitorder="little").reshape(-1, 384)
    return t.reshape(-1)


def encode(fmt, r):
    """enc_sat: nearest magnitude after the clamp to max, ties to the even code, the sign kept whatever the magnitude."""
    mags = MAGS[fmt]
    a = np.minimum(np.abs(np.asarray(r, dtype=np.float64)), mags[31])
    hi = np.minimum(np.searchsorted(mags, a, side="left"), 31)  # first entry >= a
    lo = np.maximum(hi - 1, 0)
    d_lo, d_hi = a - mags[lo], mags[hi] - a
    pick = np.where(d_hi < d_lo, hi, np.where(d_lo < d_hi, lo, np.where(hi % 2 == 0, hi, lo)))
    return (np.where(np.signbit(r), 32, 0) | pick).astype(np.uint8)


def requantise(fmt, s, e, e_zero):
    """Steps 4 - 7 on finite float32 sums s (n, 16, 32) relative to scales e (n, 16): (new scales, codes)."""
    amax = np.abs(s).max(axis=-1)
    mant, x = np.frexp(amax.astype(np.float64))
    e2 = np.where(amax == 0, e_zero, np.clip(e + x - MAX_EXP[fmt] + (mant > THRESHOLD[fmt]), 0, 254))
    return e2, encode(fmt, ldexp32(s, (e - e2)[..., None]))


def combine(x, y, fmt):
    """x o y = f(in = x, inout = y) on whole tiles; returns new tiles."""
    ex, px = split(x)
    ey, py = split(y)
    e = np.maximum(ex, ey)
    s = ldexp32(TABLE[fmt][py], (ey - e)[..., None]) + ldexp32(TABLE[fmt][px], (ex - e)[..., None])
    e2, codes = requantise(fmt, s, e, e)
    nan = (ex == 0xFF) | (ey == 0xFF)
    return join(np.where(nan, 0xFF, e2), np.where(nan[..., None], 0, codes))


def quantize_ref(src, fmt):
    """The tiles of the float32 values src: beyond len(src) the last tile holds +0; a non-finite value: a NaN block."""
    s = np.zeros(((src.size + TILE_VALUES - 1) // TILE_VALUES, 16, 32), dtype=np.float32)
    s.reshape(-1)[:src.size] = src
    nan = ~np.isfinite(s).all(axis=-1)
    e2, codes = requantise(fmt, np.where(nan[..., None], np.float32(0), s), np.full(s.shape[:2], 127, dtype=np.int64), 0)
    return join(np.where(nan, 0xFF, e2), np.where(nan[..., None], 0, codes))


def dequantize_ref(tiles, n, fmt, bf16=False):
    """The first n values as uint32 bits of float32, or uint16 bits of bf16; a NaN is 0x7FC00000 / 0x7FC0."""
    e, p = split(tiles)
    v = np.where((e == 0xFF)[..., None], np.uint32(0x7FC00000).view(np.float32), ldexp32(TABLE[fmt][p], (e - 127)[..., None]))
    v = v.astype(np.float32).reshape(-1)[:n]
    return f32_to_bf16(v) if bf16 else v.view(np.uint32)


def expected(fmt, mode, sends, k, b, schedule):
    """Every rank's output tiles of a collective: the library's plan under the plan evaluator over this rule."""
    import plan_sim

    def reduce_local(inp, inout, dtype, op):  # pyoracle.reduce_local's contract: inout = inp o inout, in place
        assert dtype == DTYPE and op == "sum" and inp.size == inout.size
        inout[:] = combine(inp, inout, fmt).view(TILE)
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
