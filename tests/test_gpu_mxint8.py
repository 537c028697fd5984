"""libchiara_mxint8.so (include/chiara_mxint8.h, chiara_amd/mxint8.py) on the device, bit for bit against
tests/mxint8_ref.py."""
import functools

import numpy as np
import pytest

import chiara_amd as ca
import fp8_ref
import gpu_util as gu
import mxint8_ref as ref
from chiara_amd import mxint8
from footprint_util import Guarded
from mx_ref import join

pytestmark = pytest.mark.gpu

TB = mxint8.TILE_BYTES
BIG = 2 * 4096 + 3  # tiles: more trips than the fold's grid holds workgroups, so workgroups stride
GAPS = [0, 1, 7, 8, 15, 16, 17, 24, 25, 40]  # 7 | 8: the 16-bit combine ends; 16 | 17, 24 | 25: f32 sums begin to round


@pytest.fixture(scope="module", autouse=True)
def env():  # (tile type, op code); released when the module is done
    yield mxint8.mxint8_type(), mxint8.mxint8_sum()
    assert mxint8.release() == 0


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    rows = [f"[{i}] got={int(got[i]):#x} want={int(want[i]):#x}" for i in bad[:8]]
    assert got.shape == want.shape and bad.size == 0, f"{what}: {bad.size} of {got.size} differ: {rows}"


def _fold(env, out, acc, ins, n, rf=0, dt=None):
    rc = ca.reduce_multi_ex(out, acc, ins, n, env[0] if dt is None else dt, env[1], rf, gu.stream())
    gu.sync()
    return rc


@pytest.mark.parametrize("d", GAPS)
@pytest.mark.parametrize("mates", [False, True], ids=["pairs", "with block-mates"])
def test_operand_domain(env, mates, d):
    """All 65 536 code pairs (0x80 on both sides) through one fold, m = 1, at gap d in both orders from the base scales
    1, 127 and 253: 32 pairs to a block, or one pair per block beside a +-127 code in the block's other lane, a -+1 code
    and zeros, which pin the amax so that the pair is renormalised both ways and, where it cancels, by them alone."""
    scale_pairs = sorted({(lo, lo + d) for lo in (1, 127, 253 - d)} | {(lo + d, lo) for lo in (1, 127, 253 - d)})
    x, y = np.divmod(np.arange(65536, dtype=np.int64), 256)
    if mates:
        px, py = np.zeros((2, 65536, 32), dtype=np.uint8)
        px[:, 0], py[:, 0] = x, y
        px[:, 17], py[:, 2] = np.where((x + y) % 2, 0x7F, 0x81), np.where((x + y) % 2, 0xFF, 0x01)
    else:
        px, py = x.reshape(-1, 32).astype(np.uint8), y.reshape(-1, 32).astype(np.uint8)
    per = px.shape[0]
    scales = np.repeat(np.array(scale_pairs), per, axis=0).reshape(-1, 16, 2)
    px, py = np.tile(px, (len(scale_pairs), 1)), np.tile(py, (len(scale_pairs), 1))
    inp, acc = join(scales[..., 0], px), join(scales[..., 1], py)
    out = gu.empty_dev(acc.size).fill_(0xA5)
    assert _fold(env, out, gu.to_dev(acc), [gu.to_dev(inp)], acc.size // TB) == 0
    _same(gu.from_dev(out, np.uint8), ref.combine(inp, acc), f"operand domain, scales {scale_pairs}")


def test_positions():
    """Block r of 256 holds code (i + r) % 256 at value i: every code at every position, decoded and encoded again
    (0x80, -2.0, comes back as 0x81 under the next scale, halved with its block)."""
    codes = ((np.arange(32)[None, :] + np.arange(256)[:, None]) % 256).astype(np.uint8)
    tiles, n = join(np.full((16, 16), 127), codes), 16 * mxint8.TILE_VALUES
    wide, back = gu.empty_dev(4 * n).fill_(0xA5), gu.empty_dev(tiles.size).fill_(0xA5)
    assert mxint8.dequantize(wide, gu.to_dev(tiles), n, ca.FLOAT32, gu.stream()) == 0
    assert mxint8.quantize(back, wide, n, ca.FLOAT32, gu.stream()) == 0
    gu.sync()
    table = ref.decode(codes).astype(np.float32).reshape(-1)
    _same(gu.from_dev(wide, np.uint32), table.view(np.uint32), "decode positions")
    _same(gu.from_dev(back, np.uint8), ref.quantize_ref(table), "encode positions")


def _wild(ntiles, seed, close=False):
    """Random codes; scales 0, 1, 253, 254 (both clamps), near 127, 0xFF -- or, close, 120 .. 127 alone, where whole
    waves stay on the integer combine; 1/8 zero blocks."""
    rng = np.random.default_rng(seed)
    pool = np.arange(120, 128) if close else np.array([0, 0, 1, 254, 254, 253, 0xFF] + list(range(118, 137)))
    codes = rng.integers(0, 256, (ntiles, 16, 32)).astype(np.uint8)
    codes[rng.integers(0, 8, (ntiles, 16)) == 0] = 0
    return join(pool[rng.integers(0, pool.size, (ntiles, 16))], codes)


@pytest.mark.parametrize("close", [False, True], ids=["wild", "close"])
@pytest.mark.parametrize("n", [1, 2, 3, BIG])
def test_fold_shapes(env, n, close):
    """Half a wave trip (one tile: one less than a trip), a trip, a trip and a tile, and more trips than workgroups;
    m = 0, 1, 2, 7, 17 (past one launch), both operand orders, `out` aliased or apart, 16-B aligned or 4 or 8 bytes in,
    between guard bands.  BIG repeats 7 tiles."""
    xs = [_wild(min(n, 7), [62, r], close) for r in range(18)]
    rep = lambda a: np.resize(a.reshape(-1, TB), (n, TB)).reshape(-1)
    for phase in (0, 4, 8):
        d = [Guarded(n * TB, phase, key=r).load(rep(x)) for r, x in enumerate(xs)]
        out = Guarded(n * TB, phase, key=99)
        for m in (0, 1, 2, 7, 17):
            for rf in (0, 1):
                op = lambda r, x: ref.combine(r, x) if rf else ref.combine(x, r)
                want = rep(functools.reduce(op, xs[1:1 + m], xs[0]))
                for alias in (False, True):
                    out.reset()
                    acc = out.load(rep(xs[0])).ptr if alias else d[0].ptr
                    assert _fold(env, out.ptr, acc, [g.ptr for g in d[1:1 + m]], n, rf) == 0
                    _same(out.read(np.uint8), want, f"n={n} phase={phase} m={m} running_first={rf} alias={alias}")
                    assert out.guards_intact(), out.guards_intact()


WIDE = {"f32": (ca.FLOAT32, np.uint32), "bf16": (ca.BFLOAT16, np.uint16)}


@pytest.mark.parametrize("src_type", sorted(WIDE))
def test_casts(src_type):
    """Every bf16 pattern (the non-finite ones make NaN blocks), sorted and permuted, and tails: exact footprints."""
    bits = np.arange(1 << 16, dtype=np.uint16)
    perm = np.random.default_rng(5).permutation(bits)
    for order, n in [(bits, bits.size)] + [(perm, n) for n in (bits.size, 1, 31, 33, 511, 513)]:
        src, f32 = order[:n], fp8_ref.bf16_to_f32(order[:n])
        tiles, d_src = Guarded(mxint8.tiles_for(n) * TB, key=1), gu.to_dev(src if src_type == "bf16" else f32)
        assert mxint8.quantize(tiles.ptr, d_src, n, WIDE[src_type][0], gu.stream()) == 0
        gu.sync()
        want = ref.quantize_ref(f32)
        _same(tiles.read(np.uint8), want, f"quantize n={n}")
        assert tiles.guards_intact(), tiles.guards_intact()
        for dst_type, (dt, npdt) in WIDE.items():
            dst = Guarded(n * np.dtype(npdt).itemsize, key=2)
            assert mxint8.dequantize(dst.ptr, tiles.ptr, n, dt, gu.stream()) == 0
            gu.sync()
            _same(dst.read(npdt), ref.dequantize_ref(want, n, bf16=dst_type == "bf16"), f"dequantize n={n} {dst_type}")
            assert dst.guards_intact(), dst.guards_intact()


@pytest.mark.parametrize("n,geometries", [(2, [(2, 1), (2, 2)]), (4, [(4, 4), (2, 2)])])
def test_local_group_collectives(env, n, geometries):
    """8 tiles per rank, FLAT and EXACT, against the same plan under the plan evaluator; data: quantized normals."""
    rng = np.random.default_rng([n, 6])
    sends = [ref.quantize_ref((rng.standard_normal((128, 32)) * np.exp2(rng.integers(-20, 21, (128, 1))))
                              .astype(np.float32).reshape(-1)) for _ in range(n)]
    g, d_send = ca.LocalGroup(n, 0), [gu.to_dev(s) for s in sends]
    try:
        for k, b in geometries:
            for sched in (ca.SCHEDULE_FLAT, ca.SCHEDULE_EXACT):
                g.set_schedule(sched)
                for mode, fn, count in ((ca.MODE_ALLREDUCE, g.all_reduce_radix_batch, 8),
                                        (ca.MODE_REDUCE_SCATTER, g.reduce_scatter_radix_batch, 8 // n)):
                    want = ref.expected(mode, sends, k, b, sched)
                    recv = [gu.empty_dev(count * TB).fill_(0xA5) for _ in range(n)]
                    assert fn(d_send, recv, count, env[0], env[1], k, b) == 0
                    gu.sync()
                    for r in range(n):
                        _same(gu.from_dev(recv[r], np.uint8), want[r], f"mode {mode} ({n}, {k}, {b}) schedule {sched} rank {r}")
    finally:
        g.destroy()


def test_refusals(env):
    """CHR_UINT8, chr_type_contiguous(131, CHR_UINT32), a pointer one byte in: ERR_UNSUPPORTED, nothing enqueued."""
    x = gu.to_dev(_wild(4, 1))
    out = gu.empty_dev(4 * TB + 16).fill_(0xA5)
    other = ca.type_contiguous(131, ca.UINT32)
    for dt, n, o in ((ca.UINT8, 4 * TB, 0), (other, 4, 0), (env[0], 3, 1)):
        mxint8.stats(reset=True)
        assert _fold(env, out.data_ptr() + o, x, [x], n, dt=dt) == ca.ERR_UNSUPPORTED
        assert mxint8.stats() == (1, 1, 0), mxint8.stats()
    assert ca.type_free(other) == 0
    gu.sync()
    assert bool((out == 0xA5).all())
