"""libchiara_mx6.so (include/chiara_mx6.h, chiara_amd/mx6.py) on the device, bit for bit against tests/mx6_ref.py."""
import functools

import numpy as np
import pytest

import chiara_amd as ca
import fp8_ref
import gpu_util as gu
import mx6_ref
from chiara_amd import mx6
from footprint_util import Guarded
from test_gpu_mx import GAPS  # (ex, ey): gaps 0, +-1, +-4, +-20 at base scales 1, 127 and 253

pytestmark = pytest.mark.gpu

TB = mx6.TILE_BYTES
BIG = 4 * 4096 + 3  # tiles: more trips than the fold's grid holds workgroups, so workgroups stride
FORMATS = pytest.mark.parametrize("fmt", [mx6.E2M3, mx6.E3M2], ids=["e2m3", "e3m2"])


@pytest.fixture(scope="module", autouse=True)
def env():  # (tile type, {format: op code}); released when the module is done
    yield mx6.mx6_type(), {f: mx6.mx6_sum(f) for f in (mx6.E2M3, mx6.E3M2)}
    assert mx6.release() == 0


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    rows = [f"[{i}] got={int(got[i]):#x} want={int(want[i]):#x}" for i in bad[:8]]
    assert got.shape == want.shape and bad.size == 0, f"{what}: {bad.size} of {got.size} differ: {rows}"


def _fold(env, fmt, out, acc, ins, n, rf=0, dt=None):
    rc = ca.reduce_multi_ex(out, acc, ins, n, env[0] if dt is None else dt, env[1][fmt], rf, gu.stream())
    gu.sync()
    return rc


@FORMATS
@pytest.mark.parametrize("mates", [False, True], ids=["pairs", "with block-mates"])
def test_operand_domain(env, fmt, mates):
    """All 4 096 code pairs through one fold, m = 1, under every scale pair of GAPS: 32 pairs to a block, or one pair
    per block beside a max code, a subnormal and zeros, which fix the amax so that the pair is renormalised both ways."""
    x, y = np.divmod(np.arange(4096, dtype=np.int64), 64)
    if mates:
        px, py = np.zeros((2, 4096 * len(GAPS), 32), dtype=np.uint8)
        px[:, 0], py[:, 0] = np.tile(x, len(GAPS)), np.tile(y, len(GAPS))
        px[:, 1], py[:, 2] = 0x1F, 0x01  # the max code and the smallest subnormal
        scales = np.repeat(np.array(GAPS), 4096, axis=0)
    else:
        px, py = np.tile(x.reshape(-1, 32), (len(GAPS), 1)), np.tile(y.reshape(-1, 32), (len(GAPS), 1))
        scales = np.repeat(np.array(GAPS), 128, axis=0)
    blocks = -(-scales.shape[0] // 16) * 16  # whole tiles: the first blocks again
    px, py, scales = (np.resize(a, (blocks,) + a.shape[1:]) for a in (px, py, scales))
    inp, acc = (mx6_ref.join(scales[:, k].reshape(-1, 16), p) for k, p in ((0, px), (1, py)))
    out = gu.empty_dev(acc.size).fill_(0xA5)
    assert _fold(env, fmt, out, gu.to_dev(acc), [gu.to_dev(inp)], acc.size // TB) == 0
    _same(gu.from_dev(out, np.uint8), mx6_ref.combine(inp, acc, fmt), "operand domain")


@FORMATS
def test_positions(fmt):
    """Block r of 64 holds code (i + r) % 64 at value i: every code at every position, decoded and encoded again."""
    codes = ((np.arange(32)[None, :] + np.arange(64)[:, None]) % 64).astype(np.uint8)
    tiles, n = mx6_ref.join(np.full((4, 16), 127), codes), 4 * mx6.TILE_VALUES
    wide, back = gu.empty_dev(4 * n).fill_(0xA5), gu.empty_dev(tiles.size).fill_(0xA5)
    assert mx6.dequantize(wide, gu.to_dev(tiles), n, ca.FLOAT32, fmt, gu.stream()) == 0
    assert mx6.quantize(back, wide, n, ca.FLOAT32, fmt, gu.stream()) == 0
    gu.sync()
    table = mx6_ref.TABLE[fmt][codes].astype(np.float32).reshape(-1)
    _same(gu.from_dev(wide, np.uint32), table.view(np.uint32), "decode positions")
    _same(gu.from_dev(back, np.uint8), mx6_ref.quantize_ref(table, fmt), "encode positions")


def _wild(ntiles, seed):
    """Random codes; scales 0, 1, 253, 254 (both clamps), near 127, 0xFF; 1/8 zero blocks."""
    rng = np.random.default_rng(seed)
    pool = np.array([0, 0, 1, 254, 254, 253, 0xFF] + list(range(118, 137)))
    codes = rng.integers(0, 64, (ntiles, 16, 32)).astype(np.uint8)
    codes[rng.integers(0, 8, (ntiles, 16)) == 0] = 0
    return mx6_ref.join(pool[rng.integers(0, pool.size, (ntiles, 16))], codes)


@FORMATS
@pytest.mark.parametrize("n", [1, 3, 4, 5, BIG])
def test_fold_shapes(env, fmt, n):
    """Partial, nearly full, full and one-and-a-bit wave trips, and more trips than workgroups; m = 0, 1, 2, 7, both
    operand orders, `out` aliased or apart, 16-B aligned or 4 or 8 bytes in, between guard bands.  BIG repeats 7 tiles."""
    xs = [_wild(min(n, 7), [61, r]) for r in range(8)]
    rep = lambda a: np.resize(a.reshape(-1, TB), (n, TB)).reshape(-1)
    for phase in (0, 4, 8):
        d = [Guarded(n * TB, phase, key=r).load(rep(x)) for r, x in enumerate(xs)]
        out = Guarded(n * TB, phase, key=99)
        for m in (0, 1, 2, 7):
            for rf in (0, 1):
                op = lambda r, x: mx6_ref.combine(r, x, fmt) if rf else mx6_ref.combine(x, r, fmt)
                want = rep(functools.reduce(op, xs[1:1 + m], xs[0]))
                for alias in (False, True):
                    out.reset()
                    acc = out.load(rep(xs[0])).ptr if alias else d[0].ptr
                    assert _fold(env, fmt, out.ptr, acc, [g.ptr for g in d[1:1 + m]], n, rf) == 0
                    _same(out.read(np.uint8), want, f"n={n} phase={phase} m={m} running_first={rf} alias={alias}")
                    assert out.guards_intact(), out.guards_intact()


WIDE = {"f32": (ca.FLOAT32, np.uint32), "bf16": (ca.BFLOAT16, np.uint16)}


@FORMATS
@pytest.mark.parametrize("src_type", sorted(WIDE))
def test_casts(fmt, src_type):
    """Every bf16 pattern (the non-finite ones make NaN blocks), sorted and permuted, and tails: exact footprints."""
    bits = np.arange(1 << 16, dtype=np.uint16)
    perm = np.random.default_rng(5).permutation(bits)
    for order, n in [(bits, bits.size)] + [(perm, n) for n in (bits.size, 1, 31, 33, 511, 513)]:
        src, f32 = order[:n], fp8_ref.bf16_to_f32(order[:n])
        tiles, d_src = Guarded(mx6.tiles_for(n) * TB, key=1), gu.to_dev(src if src_type == "bf16" else f32)
        assert mx6.quantize(tiles.ptr, d_src, n, WIDE[src_type][0], fmt, gu.stream()) == 0
        gu.sync()
        want = mx6_ref.quantize_ref(f32, fmt)
        _same(tiles.read(np.uint8), want, f"quantize n={n}")
        assert tiles.guards_intact(), tiles.guards_intact()
        for dst_type, (dt, npdt) in WIDE.items():
            dst = Guarded(n * np.dtype(npdt).itemsize, key=2)
            assert mx6.dequantize(dst.ptr, tiles.ptr, n, dt, fmt, gu.stream()) == 0
            gu.sync()
            _same(dst.read(npdt), mx6_ref.dequantize_ref(want, n, fmt, bf16=dst_type == "bf16"), f"dequantize n={n} {dst_type}")
            assert dst.guards_intact(), dst.guards_intact()


@FORMATS
@pytest.mark.parametrize("n,geometries", [(2, [(2, 1), (2, 2)]), (4, [(4, 4), (2, 2)])])
def test_local_group_collectives(env, fmt, n, geometries):
    """8 tiles per rank, FLAT and EXACT, against the same plan under the plan evaluator; data: quantized normals."""
    rng = np.random.default_rng([n, 6])
    sends = [mx6_ref.quantize_ref((rng.standard_normal((128, 32)) * np.exp2(rng.integers(-20, 21, (128, 1))))
                                  .astype(np.float32).reshape(-1), fmt) for _ in range(n)]
    g, d_send = ca.LocalGroup(n, 0), [gu.to_dev(s) for s in sends]
    try:
        for k, b in geometries:
            for sched in (ca.SCHEDULE_FLAT, ca.SCHEDULE_EXACT):
                g.set_schedule(sched)
                for mode, fn, count in ((ca.MODE_ALLREDUCE, g.all_reduce_radix_batch, 8),
                                        (ca.MODE_REDUCE_SCATTER, g.reduce_scatter_radix_batch, 8 // n)):
                    want = mx6_ref.expected(fmt, mode, sends, k, b, sched)
                    recv = [gu.empty_dev(count * TB).fill_(0xA5) for _ in range(n)]
                    assert fn(d_send, recv, count, env[0], env[1][fmt], k, b) == 0
                    gu.sync()
                    for r in range(n):
                        _same(gu.from_dev(recv[r], np.uint8), want[r], f"mode {mode} ({n}, {k}, {b}) schedule {sched} rank {r}")
    finally:
        g.destroy()


@FORMATS
def test_refusals(env, fmt):
    """CHR_UINT8, chr_type_contiguous(99, CHR_UINT32), a pointer one byte in: ERR_UNSUPPORTED, nothing enqueued."""
    x = gu.to_dev(_wild(4, 1))
    out = gu.empty_dev(4 * TB + 16).fill_(0xA5)
    other = ca.type_contiguous(99, ca.UINT32)
    for dt, n, o in ((ca.UINT8, 4 * TB, 0), (other, 4, 0), (env[0], 3, 1)):
        mx6.stats(reset=True)
        assert _fold(env, fmt, out.data_ptr() + o, x, [x], n, dt=dt) == ca.ERR_UNSUPPORTED
        assert mx6.stats() == (1, 1, 0), mx6.stats()
    assert ca.type_free(other) == 0
    gu.sync()
    assert bool((out == 0xA5).all())
