"""Reference for the MXFP8 SUM and casts of libchiara_mx.so: include/chiara_mx.h's rule in numpy, host only.  Tiles are
uint8 arrays of whole 528-byte tiles.  Decode and encode are tests/fp8_ref.py's; every ldexp is numpy's float64 ldexp
-- exact on these operands -- followed by one rounding to float32; the sum is one numpy float32 add.  A collective's
expected bytes come from the library's own plans under tests/plan_sim.py with the oracle's MPI_Reduce_local
restatement replaced by this rule on elements of dtype V528 (expected(), as tests/fp8_ref.py does it)."""
import numpy as np
import pytest

import fp8_ref
import pyoracle as po

DTYPE, TILE = "mx", np.dtype("V528")  # the name and the element the plan evaluator sees
TILE_BYTES, TILE_VALUES = 528, 512
MAX_EXP = {fp8_ref.E4M3: 9, fp8_ref.E5M2: 16}  # max = 0.875 * 2^MAX_EXP


def split(tiles):
    """(scales (n, 16) int64, codes (n, 16, 32) uint8) of n whole tiles."""
    t = np.ascontiguousarray(tiles).view(np.uint8).reshape(-1, TILE_BYTES)
    return t[:, :16].astype(np.int64), t[:, 16:].reshape(-1, 16, 32)


def join(scales, codes):
    t = np.empty((scales.shape[0], TILE_BYTES), dtype=np.uint8)
    t[:, :16] = scales
    t[:, 16:] = codes.reshape(-1, TILE_VALUES)
    return t.reshape(-1)


def ldexp32(v, k):
    with np.errstate(all="ignore"):
        return np.ldexp(np.asarray(v, dtype=np.float64), k).astype(np.float32)


def requantise(fmt, s, e, e_zero):
    """Steps 4 - 7 on float32 sums s (n, 16, 32) relative to scales e (n, 16): (new scales, codes)."""
    fin = np.isfinite(s)
    amax = np.where(fin, np.abs(s), np.float32(0)).max(axis=-1)
    mant, x = np.frexp(amax.astype(np.float64))
    e2 = np.clip(e + x - MAX_EXP[fmt] + (mant > 0.875), 0, 254)
    e2 = np.where(amax == 0, e_zero, e2)
    t = ldexp32(s, (e - e2)[..., None])
    codes = fp8_ref.encode(fmt, fp8_ref.SATURATE, np.where(fin, t, 0).astype(np.float64))
    return e2, np.where(fin, codes, fp8_ref.CANONICAL_NAN[fmt]).astype(np.uint8)


def combine(fmt, x, y):
    """x o y = f(in = x, inout = y) on whole tiles; returns new tiles."""
    ex, px = split(x)
    ey, py = split(y)
    e = np.maximum(ex, ey)
    a = ldexp32(fp8_ref.decode(fmt, px), (ex - e)[..., None])
    b = ldexp32(fp8_ref.decode(fmt, py), (ey - e)[..., None])
    with np.errstate(all="ignore"):
        s = b + a
    e2, codes = requantise(fmt, s, e, e)
    nan = (ex == 0xFF) | (ey == 0xFF)
    return join(np.where(nan, 0xFF, e2), np.where(nan[..., None], fp8_ref.CANONICAL_NAN[fmt], codes))


def quantize_ref(fmt, src):
    """The tiles of the float32 values src: beyond len(src) the last tile holds +0."""
    s = np.zeros((src.size + TILE_VALUES - 1) // TILE_VALUES * TILE_VALUES, dtype=np.float32)
    s[:src.size] = src
    s = s.reshape(-1, 16, 32)
    return join(*requantise(fmt, s, np.full(s.shape[:2], 127, dtype=np.int64), 0))


def dequantize_ref(fmt, tiles, n, bf16=False):
    """The first n values as uint32 bits of float32, or uint16 bits of bf16; a NaN is 0x7FC00000 / 0x7FC0."""
    e, p = split(tiles)
    v = ldexp32(fp8_ref.decode(fmt, p), (e - 127)[..., None])
    v = np.where((e == 0xFF)[..., None] | np.isnan(v), np.uint32(0x7FC00000).view(np.float32), v).astype(np.float32)
    v = v.reshape(-1)[:n]
    return fp8_ref.f32_to_bf16(v) if bf16 else v.view(np.uint32)


def expected(fmt, mode, sends, k, b, schedule):
    """Every rank's output tiles of a collective: the library's plan under the plan evaluator over this rule."""
    import plan_sim

    def reduce_local(inp, inout, dtype, op):  # pyoracle.reduce_local's contract: inout = inp o inout, in place
        assert dtype == DTYPE and op == "sum" and inp.size == inout.size
        inout[:] = combine(fmt, inp, inout).view(TILE)
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
