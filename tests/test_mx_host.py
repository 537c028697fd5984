"""tests/mx_ref.py and tests/mx4_ref.py -- the only judges of every MX GPU test -- against the prose of
include/chiara_mx.h and include/chiara_mx4.h, host only.  Nothing of the code under check is reused: tiles are taken
apart here from the headers' byte layout, the FP8 decode tables are torch's float8 casts and E2M1's is the header's list,
and the rule's outcome is not recomputed but checked property by property -- the scale by trying the next smaller one,
a code by brute force over every code of the format.

Arithmetic: float64.  A decoded value times a power of two is exact there, and so is the sum of two of them wherever
the scales are at most 20 apart (E5M2 spans 2^-16 .. 1.75 * 2^15: 52 bits with the gap); one astype(float32) is then
the rule's one rounding.  The f32 sum times 2^(e - e') is exact too (24 bits, an exponent within +-420), and a
difference to a code's value is exact wherever two codes are anywhere near a tie.

Operands: those of test_operand_domain in tests/test_gpu_mx.py and tests/test_gpu_mx4.py -- all code pairs (65 536 per
FP8 format, 256 for E2M1) under every scale pair of GAPS, 32 pairs to a block and one pair beside block-mates."""
import types

import numpy as np
import pytest
import torch

import mx4_ref
import mx_ref
from test_gpu_mx import domain_operands as fp8_operands
from test_gpu_mx4 import domain_operands as fp4_operands


def _f8_table(dtype):
    return torch.arange(256, dtype=torch.uint8).view(dtype).to(torch.float64).numpy()


_E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6])  # chiara_mx4.h: `s eem` decodes to +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}


def _fmt(name, table, mbits, emin, nan_code, tile_bytes, **fns):
    """table: code -> float64; mbits and emin (the smallest normal's exponent) give a code's step; max: largest finite."""
    return types.SimpleNamespace(name=name, table=table, mbits=mbits, emin=emin, nan_code=nan_code, tile_bytes=tile_bytes,
                                 max=float(table[np.isfinite(table)].max()), sign=table.size >> 1, **fns)


E4M3 = _fmt("e4m3", _f8_table(torch.float8_e4m3fn), 3, -6, 0x7F, 528, operands=lambda m: fp8_operands(0, m),
            combine=lambda x, y: mx_ref.combine(0, x, y), quantize=lambda v: mx_ref.quantize_ref(0, v),
            dequantize=lambda t, n, bf16=False: mx_ref.dequantize_ref(0, t, n, bf16))
E5M2 = _fmt("e5m2", _f8_table(torch.float8_e5m2), 2, -14, 0x7E, 528, operands=lambda m: fp8_operands(1, m),
            combine=lambda x, y: mx_ref.combine(1, x, y), quantize=lambda v: mx_ref.quantize_ref(1, v),
            dequantize=lambda t, n, bf16=False: mx_ref.dequantize_ref(1, t, n, bf16))
E2M1 = _fmt("e2m1", np.concatenate([_E2M1, -_E2M1]), 1, 0, None, 272, operands=fp4_operands,
            combine=mx4_ref.combine, quantize=mx4_ref.quantize_ref, dequantize=mx4_ref.dequantize_ref)
FMT = pytest.mark.parametrize("F", [E4M3, E5M2, E2M1], ids=lambda F: F.name)
MATES = pytest.mark.parametrize("mates", [False, True], ids=["pairs", "with block-mates"])


def test_tables_are_the_headers():
    """The independent decode: max 448 / 57344 / 6, the canonical NaN codes are NaNs, E5M2 has infinities, E2M1 has
    neither, -0 is the sign bit alone."""
    assert (E4M3.max, E5M2.max, E2M1.max) == (448.0, 57344.0, 6.0)
    assert np.isnan(E4M3.table[0x7F]) and np.isnan(E5M2.table[0x7E]) and np.isinf(E5M2.table[0x7C])
    assert np.isfinite(E2M1.table).all() and not np.isinf(E4M3.table).any()
    for F in (E4M3, E5M2, E2M1):
        assert F.table[F.sign] == 0 and np.signbit(F.table[F.sign]) and not np.signbit(F.table[0])


def _unpack(F, tiles):
    """(scales (B,), codes (B, 32)) per block, from the headers' layout: 16 scale bytes, then block b's codes in order;
    MX4 packs value 2i into the low nibble of byte i and value 2i + 1 into the high one."""
    t = np.ascontiguousarray(tiles).view(np.uint8).reshape(-1, F.tile_bytes)
    body = t[:, 16:].reshape(t.shape[0] * 16, -1)
    if F is E2M1:
        body = np.stack([body & 15, body >> 4], axis=-1).reshape(-1, 32)
    return t[:, :16].reshape(-1).astype(np.int64), body


def _sums(F, x, y):
    """Steps 2 - 3: (e, s) with s the f32 sums as float64, for operands whose scales are at most 20 apart."""
    (ex, px), (ey, py) = _unpack(F, x), _unpack(F, y)
    e = np.maximum(ex, ey)
    assert (np.abs(ex - ey)[(ex != 0xFF) & (ey != 0xFF)] <= 20).all()
    with np.errstate(all="ignore"):
        a = F.table[px] * np.exp2((ex - e).astype(np.float64))[:, None]
        b = F.table[py] * np.exp2((ey - e).astype(np.float64))[:, None]
        return e, (b + a).astype(np.float32).astype(np.float64)


def _check_blocks(F, s, e, e2, codes, zero_scale, what):
    """The rule's steps 4 - 7 on blocks (B, 32): sums s relative to scales e gave scales e2 and `codes`."""
    fin = np.isfinite(s)
    amax = np.where(fin, np.abs(s), 0.0).max(axis=-1)
    fits = lambda k: amax * np.exp2((e - k).astype(np.float64)) <= F.max
    # scale: the smallest of 0 .. 254 that fits, found by trying the next smaller one; 254 where none does
    nz = amax > 0
    assert ((e2 >= 0) & (e2 <= 254)).all(), what
    smallest = np.where(fits(e2), (e2 == 0) | ~fits(e2 - 1), e2 == 254)
    bad = np.flatnonzero(nz & ~smallest)
    assert bad.size == 0, f"{what}: scale not the smallest that fits in {bad.size} blocks, e.g. amax={amax[bad[0]]!r} " \
                          f"e={e[bad[0]]} e'={e2[bad[0]]}"
    assert (e2[~nz] == zero_scale[~nz]).all(), f"{what}: the scale of an all-zero block"
    # codes
    if F.nan_code is None:
        assert fin.all(), what
    else:
        assert (codes[~fin] == F.nan_code).all(), f"{what}: a non-finite sum is the canonical NaN code"
    with np.errstate(all="ignore"):
        t = np.where(fin, s, 0.0) * np.exp2((e - e2).astype(np.float64))[:, None]
    assert (e2[(np.abs(t) > F.max).any(axis=-1)] == 254).all(), f"{what}: saturation below the clamp at 254"
    assert ((codes[fin] & F.sign != 0) == np.signbit(s[fin])).all(), f"{what}: the sum's sign is kept, on zeros too"
    tc = np.clip(t, -F.max, F.max)[fin]
    assert (tc.view(np.uint64) & np.uint64(0xFF) == 0).all()  # 24 significant bits: the low byte carries the code
    key = np.unique(tc.view(np.uint64) | codes[fin].astype(np.uint64))
    tu, cu = (key & ~np.uint64(0xFF)).view(np.float64), (key & np.uint64(0xFF)).astype(np.int64)
    value = np.where(np.isfinite(F.table), F.table, np.inf)
    assert np.isfinite(value[cu]).all(), f"{what}: a finite sum encoded as a non-finite code"
    for lo in range(0, tu.size, 1 << 15):
        v, c = tu[lo:lo + (1 << 15)], cu[lo:lo + (1 << 15)]
        dist = np.abs(value[None, :] - v[:, None])
        best = dist.min(axis=1)
        mine = dist[np.arange(v.size), c]
        bad = np.flatnonzero(mine != best)
        assert bad.size == 0, f"{what}: {v[bad[0]]!r} encoded as {c[bad[0]]:#x}, not a nearest code"
        tie = ((dist == best[:, None]) & (value[None, :] != value[c][:, None])).any(axis=1)
        bad = np.flatnonzero(tie & (c % 2 != 0))
        assert bad.size == 0, f"{what}: the tie at {v[bad[0]]!r} went to the odd code {c[bad[0]]:#x}"
    return amax


@FMT
@MATES
def test_combine_scale_and_codes(F, mates):
    """Scale choice and codes of combine over the whole operand domain: the smallest scale that fits (e' - 1 does not,
    or e' is 0; 254 where nothing fits), max(ex, ey) for an all-zero block; every code a nearest one of the rescaled
    f32 sum, ties to the even code, the sum's sign on zeros, saturation only at e' = 254, the canonical NaN code for a
    non-finite sum, which takes no part in the amax.  The domain holds sums of exactly max * 2^k (the scale one step
    too large would pass every GPU test) and the clamp at 254; the clamp at 0 is test_lower_clamp's."""
    x, y = F.operands(mates)
    e, s = _sums(F, x, y)
    e2, codes = _unpack(F, F.combine(x, y))
    amax = _check_blocks(F, s, e, e2, codes, e, f"{F.name} combine")
    mant = np.frexp(amax / F.max)[0]
    assert (mant[amax > 0] == 0.5).any() and (e2 == 254).any()  # amax = max * 2^k; the upper clamp


@FMT
def test_lower_clamp(F):
    """The operand domain's MX4 blocks never reach e' = 0 (their amax is 6 at least), so: every code alone in a block
    of zeros under scales 0 .. 3 on both sides.  The smallest fitting scale would be negative for most; e' is 0 and
    the codes are the nearest ones there, nothing saturating."""
    ncodes = F.table.size
    pairs = [(a, b) for a in range(4) for b in range(4)]
    body = np.zeros((len(pairs) * ncodes, 32), dtype=np.uint8)
    body[:, 5] = np.tile(np.arange(ncodes), len(pairs))
    blocks = -(-body.shape[0] // 16) * 16
    body = np.resize(body, (blocks, 32))
    scales = np.resize(np.repeat(np.array(pairs), ncodes, axis=0), (blocks, 2))
    join = mx4_ref.join if F is E2M1 else mx_ref.join
    x, y = join(scales[:, 0].reshape(-1, 16), body), join(scales[:, 1].reshape(-1, 16), np.zeros_like(body))
    e, s = _sums(F, x, y)
    e2, codes = _unpack(F, F.combine(x, y))
    amax = _check_blocks(F, s, e, e2, codes, e, f"{F.name} lower clamp")
    with np.errstate(divide="ignore"):
        unclamped = e + np.ceil(np.log2(amax / F.max))
    assert ((amax > 0) & (unclamped < 0)).sum() > ncodes and (e2[(amax > 0) & (unclamped < 0)] == 0).all()


@FMT
@MATES
def test_combine_commutes(F, mates):
    """combine(x, y) == combine(y, x) byte for byte: the fold launchers ignore running_first on the strength of it."""
    x, y = F.operands(mates)
    assert np.array_equal(F.combine(x, y), F.combine(y, x))


@FMT
def test_nan_blocks(F):
    """Scale 0xFF on either side or both: scale 0xFF and canonical codes (FP8: the format's NaN code; MX4: 0x00 bytes),
    whatever the other side holds, NaN and inf codes included; the blocks beside them follow the rule."""
    rng = np.random.default_rng(7)
    nt = 64
    tiles = []
    for side in range(2):
        t = rng.integers(0, 256, (nt, F.tile_bytes)).astype(np.uint8)
        t[:, :16] = rng.integers(117, 138, (nt, 16))  # at most 20 apart
        tiles.append(t)
    which = rng.integers(0, 4, (nt, 16))  # 0: neither, 1: x, 2: y, 3: both
    tiles[0][:, :16][(which & 1) != 0] = 0xFF
    tiles[1][:, :16][(which & 2) != 0] = 0xFF
    x, y = tiles[0].reshape(-1), tiles[1].reshape(-1)
    out = F.combine(x, y)
    e2, codes = _unpack(F, out)
    nan = which.reshape(-1) != 0
    assert (e2[nan] == 0xFF).all() and (e2[~nan] != 0xFF).all()
    assert (codes[nan] == (0 if F.nan_code is None else F.nan_code)).all()
    assert np.array_equal(out, F.combine(y, x))
    e, s = _sums(F, x, y)
    _check_blocks(F, s[~nan], e[~nan], e2[~nan], codes[~nan], e[~nan], f"{F.name} beside NaN blocks")


def _bf16_values(order):
    return (np.asarray(order, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


ORDERS = {"sorted": np.arange(1 << 16, dtype=np.uint16),
          "permuted": np.random.default_rng(5).permutation(np.arange(1 << 16, dtype=np.uint16))}


def _step(F, mag):
    """The format's spacing at the binade of the code value `mag` (>= 0): 2^(max(exponent, emin) - mbits)."""
    ex = np.frexp(mag)[1] - 1  # mag = 1.x * 2^ex; frexp(0) = (0, 0) falls to emin below
    return np.exp2((np.maximum(np.where(mag > 0, ex, F.emin), F.emin) - F.mbits).astype(np.float64))


@FMT
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_quantize_every_bf16(F, order):
    """quantize_ref on all 65 536 bf16 patterns, as homogeneous blocks and permuted: the rule's steps with e = 127 and
    scale 0 for an all-zero block (the same scale and code checks as combine); for MX4 a block with a non-finite value
    is the canonical NaN block.  Then dequantize_ref of those tiles: ldexp(dec(code), scale - 127) rounded to f32,
    overflow to inf, 0x7FC00000 for a NaN; its bf16 output is torch's round-to-nearest-even of the f32 one; and every
    finite x lies within half a step of its dequantized value, the step being the format's spacing in the code's
    binade times 2^(scale - 127) -- which also pins the order of values inside a tile."""
    src = _bf16_values(ORDERS[order])
    tiles = F.quantize(src)
    e2, codes = _unpack(F, tiles)
    with np.errstate(invalid="ignore"):  # signalling NaN patterns
        s = src.astype(np.float64).reshape(-1, 32)
    live = np.ones(s.shape[0], dtype=bool)
    if F.nan_code is None:
        live = np.isfinite(s).all(axis=-1)
        assert (e2[~live] == 0xFF).all() and (codes[~live] == 0).all() and (e2[live] != 0xFF).all()
    e = np.full(s.shape[0], 127, dtype=np.int64)
    _check_blocks(F, s[live], e[live], e2[live], codes[live], np.zeros_like(e)[live], f"{F.name} quantize {order}")
    # dequantize: exact values from the independent table
    with np.errstate(all="ignore"):
        exact = np.where((e2 == 0xFF)[:, None], np.nan, F.table[codes] * np.exp2((e2 - 127).astype(np.float64))[:, None])
        want = exact.astype(np.float32).reshape(-1)
    got = F.dequantize(tiles, src.size)
    assert np.array_equal(got, np.where(np.isnan(want), np.uint32(0x7FC00000), want.view(np.uint32)))
    bf = torch.from_numpy(got.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got_bf = F.dequantize(tiles, src.size, bf16=True)
    nan = np.isnan(want)
    assert np.array_equal(got_bf[~nan], bf[~nan]) and (got_bf[nan] == 0x7FC0).all()
    ok = np.isfinite(s) & live[:, None]
    half = _step(F, np.abs(F.table[codes])) * np.exp2((e2 - 127).astype(np.float64))[:, None] / 2
    assert (e2[live] < 254).all()  # no bf16 value reaches the clamp: nothing saturates
    bad = np.flatnonzero((np.abs(exact - s) > half)[ok])
    assert bad.size == 0, f"{bad.size} values further than half a step from their source"


@FMT
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_quantize_of_dequantize_is_the_tile(F, order):
    """quantize_ref(dequantize_ref(t)) == t for the tiles t of every bf16 pattern.  Two kinds of block cannot come
    back under the headers' own rule, and are pinned for what they do instead.  A block whose dequantized values
    overflow f32 (dec(code) * 2^(scale - 127) >= 2^128, "overflow to +-inf as ldexp gives it") comes back with NaN
    codes (FP8) or as the NaN block (MX4).  A block whose largest code rounded down to exactly max / 2 now fits the
    next smaller scale ("the smallest fitting scale"): it comes back one scale lower, with the same values.  Every
    other block, NaN blocks and NaN codes included, is byte-identical."""
    t = F.quantize(_bf16_values(ORDERS[order]))
    n = t.size // F.tile_bytes * 512
    back = F.quantize(F.dequantize(t, n).view(np.float32))
    (e0, c0), (e1, c1) = _unpack(F, t), _unpack(F, back)
    with np.errstate(all="ignore"):
        v0 = np.where((e0 == 0xFF)[:, None], np.nan, F.table[c0] * np.exp2((e0 - 127).astype(np.float64))[:, None])
        v1 = np.where((e1 == 0xFF)[:, None], np.nan, F.table[c1] * np.exp2((e1 - 127).astype(np.float64))[:, None])
    over = (np.abs(np.nan_to_num(v0)) >= 2.0 ** 128).any(axis=-1)
    top = np.where(np.isfinite(v0), np.abs(F.table[c0]), 0.0).max(axis=-1)
    lower = ~over & (top == F.max / 2) & (e0 > 0) & (e0 != 0xFF)
    same = ~over & ~lower
    assert np.array_equal(e0[same], e1[same]) and np.array_equal(c0[same], c1[same])
    assert (e1[lower] == e0[lower] - 1).all() and np.array_equal(v0[lower], v1[lower], equal_nan=True)
    o0, o1 = np.abs(np.nan_to_num(v0[over])) >= 2.0 ** 128, v1[over]
    assert np.isnan(o1[o0]).all()
    assert same.any()


@FMT
@pytest.mark.parametrize("n", [1, 31, 33, 511, 513])
def test_quantize_tails_are_plus_zero(F, n):
    """Values beyond n count as +0: code 0 in a block that n cuts, scale 0 and codes 0 in the blocks wholly beyond."""
    src = _bf16_values(ORDERS["permuted"][:n])
    src = np.where(np.isfinite(src), src, np.float32(1.5))  # a non-finite value would make an MX4 NaN block
    e2, codes = _unpack(F, F.quantize(src))
    assert e2.size == -(-n // 512) * 16
    assert (codes.reshape(-1)[n:] == 0).all() and (e2[-(-n // 32):] == 0).all()
    full = np.zeros(e2.size * 32, dtype=np.float32)
    full[:n] = src
    assert np.array_equal(F.quantize(full), F.quantize(src))
