"""Reference for libchiara_mx4_sr.so: include/chiara_mx4_sr.h's rule in numpy, host only, on tests/mx4_ref.py's tiles,
ldexp32 and scale choice.  Everything about the rounding is float64, where floor(f * 2^16) is exact."""
import numpy as np
import pytest

import mx4_ref
from mx4_ref import MAGS, TABLE, TILE_VALUES, join, ldexp32, split

M32 = 0xFFFFFFFF


def mix32(x):
    """lowbias32 on uint64 arrays holding 32-bit values."""
    x = x ^ x >> 16
    x = x * 0x7feb352d & M32
    x = x ^ x >> 15
    x = x * 0x846ca68b & M32
    return x ^ x >> 16


def enc_sr(t, u):
    """Codes of the clamped float32 t (..., 32) under the 16-bit integers u: up iff floor(f * 2^16) + u >= 2^16."""
    a = np.abs(t.astype(np.float64))
    lo = np.searchsorted(MAGS, a, side="right") - 1  # the largest member <= |t|
    hi = np.minimum(lo + 1, 7)
    f = np.where(a == MAGS[lo], 0.0, (a - MAGS[lo]) / np.maximum(MAGS[hi] - MAGS[lo], 0.5))
    up = np.floor(f * 65536).astype(np.int64) + u >= 65536
    return (np.where(np.signbit(t), 8, 0) | np.where(up, hi, lo)).astype(np.uint8)


def requantise_sr(s, e, e_zero, seed, tile):
    """Steps 4 - 7 on finite float32 sums s (n, 16, 32) relative to scales e (n, 16); tile (n,) is T: (scales, codes)."""
    amax = np.abs(s).max(axis=-1)
    mant, x = np.frexp(amax.astype(np.float64))
    e2 = np.where(amax == 0, e_zero, np.clip(e + x - 3 + (mant > 0.75), 0, 254))
    t = np.clip(ldexp32(s, (e - e2)[..., None]), np.float32(-6), np.float32(6)).astype(np.float32)
    b = t.view(np.uint32).astype(np.uint64).reshape(t.shape[:2] + (16, 2))
    ks = mix32(np.uint64(seed) ^ (tile.astype(np.uint64) & M32))[:, None]
    kb = mix32(ks ^ (np.arange(16, dtype=np.uint64) | e2.astype(np.uint64) << 8))[..., None]
    c = np.arange(1, 17, dtype=np.uint64) * 0x9E3779B9 & M32
    w = mix32(b[..., 0] ^ ((b[..., 1] << 16 | b[..., 1] >> 16) & M32) ^ (kb + c & M32))
    u = np.stack([w & 0xFFFF, w >> 16], axis=-1).reshape(t.shape).astype(np.int64)
    return e2, enc_sr(t, u)


def combine(x, y, seed):
    """x o y on whole tiles under the SR rule (T = 0); returns new tiles."""
    ex, px = split(x)
    ey, py = split(y)
    e = np.maximum(ex, ey)
    s = ldexp32(TABLE[py], (ey - e)[..., None]) + ldexp32(TABLE[px], (ex - e)[..., None])
    e2, codes = requantise_sr(s, e, e, seed, np.zeros(e.shape[0], dtype=np.int64))
    nan = (ex == 0xFF) | (ey == 0xFF)
    return join(np.where(nan, 0xFF, e2), np.where(nan[..., None], 0, codes))


def quantize_ref(src, seed):
    """The tiles of the float32 values src, T = the tile's index; the rest is mx4_ref.quantize_ref."""
    s = np.zeros((src.size + TILE_VALUES - 1) // TILE_VALUES * TILE_VALUES, dtype=np.float32)
    s[:src.size] = src
    s = s.reshape(-1, 16, 32)
    nan = ~np.isfinite(s).all(axis=-1)
    e2, codes = requantise_sr(np.where(nan[..., None], np.float32(0), s), np.full(s.shape[:2], 127, dtype=np.int64), 0,
                              seed, np.arange(s.shape[0]))
    return join(np.where(nan, 0xFF, e2), np.where(nan[..., None], 0, codes))


def expected(mode, sends, k, b, schedule, seed):
    """Every rank's output tiles of a collective: mx4_ref.expected's plan evaluation with this rule for its combine."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(mx4_ref, "combine", lambda x, y: combine(x, y, seed))
        return mx4_ref.expected(mode, sends, k, b, schedule)
