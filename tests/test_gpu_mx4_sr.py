"""libchiara_mx4_sr.so (include/chiara_mx4_sr.h, chiara_amd/mx4.py) on the device, bit for bit against
tests/mx4_sr_ref.py."""
import functools

import numpy as np
import pytest

import chiara_amd as ca
import fp8_ref
import gpu_util as gu
import mx4_ref
import mx4_sr_ref as sr
from chiara_amd import mx4
from footprint_util import Guarded
from test_gpu_mx4 import BIG, TB, WIDE, _fold, _same, _wild, domain_operands

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 0xDEADBEEF)


@pytest.fixture(scope="module", autouse=True)
def env():  # (tile type, op code); the seed back to its default and the codes released when the module is done
    yield mx4.mx4_type(), mx4.mx4_sum_sr()
    mx4.sr_set_seed(0)
    assert mx4.sr_release() == 0 and mx4.release() == 0


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("mates", [False, True], ids=["pairs", "with block-mates"])
def test_operand_domain(env, mates, seed):
    """test_gpu_mx4's operands: all 256 code pairs under every scale pair of GAPS, alone and beside block-mates.  The
    reference's bytes differ from the RNE rule's and from the next seed's, so neither rounding nor seed is idle."""
    inp, acc = domain_operands(mates)
    want = sr.combine(inp, acc, seed)
    assert (want != mx4_ref.combine(inp, acc)).any()
    assert (want != sr.combine(inp, acc, SEEDS[(SEEDS.index(seed) + 1) % 3])).any()
    mx4.sr_set_seed(seed)
    out = gu.empty_dev(acc.size).fill_(0xA5)
    assert _fold(env, out, gu.to_dev(acc), [gu.to_dev(inp)], acc.size // TB) == 0
    _same(gu.from_dev(out, np.uint8), want, "operand domain")


@pytest.mark.parametrize("n", [1, 3, 4, 5, BIG])
def test_fold_shapes(env, n):
    """test_gpu_mx4.test_fold_shapes under seed 5: trips partial to striding, m = 0, 1, 2, 7, both operand orders,
    `out` aliased or apart, 16-B aligned or 4 bytes in, between guard bands.  BIG repeats 7 tiles."""
    mx4.sr_set_seed(5)
    xs = [_wild(min(n, 7), [43, r]) for r in range(8)]
    rep = lambda a: np.resize(a.reshape(-1, TB), (n, TB)).reshape(-1)
    for phase in (0, 4):
        d = [Guarded(n * TB, phase, key=r).load(rep(x)) for r, x in enumerate(xs)]
        out = Guarded(n * TB, phase, key=99)
        for m in (0, 1, 2, 7):
            for rf in (0, 1):
                op = lambda r, x: sr.combine(r, x, 5) if rf else sr.combine(x, r, 5)
                want = rep(functools.reduce(op, xs[1:1 + m], xs[0]))
                for alias in (False, True):
                    out.reset()
                    acc = out.load(rep(xs[0])).ptr if alias else d[0].ptr
                    assert _fold(env, out.ptr, acc, [g.ptr for g in d[1:1 + m]], n, rf) == 0
                    _same(out.read(np.uint8), want, f"n={n} phase={phase} m={m} running_first={rf} alias={alias}")
                    assert out.guards_intact(), out.guards_intact()


def test_fold_continuation(env):
    """m = 17 at n = 5: the second launch, continuing from `out`, rounds under the call's seed."""
    mx4.sr_set_seed(0x1234)
    xs = [_wild(5, [47, r]) for r in range(18)]
    out = gu.empty_dev(5 * TB).fill_(0xA5)
    assert _fold(env, out, gu.to_dev(xs[0]), [gu.to_dev(x) for x in xs[1:]], 5) == 0
    _same(gu.from_dev(out, np.uint8), functools.reduce(lambda r, x: sr.combine(x, r, 0x1234), xs[1:], xs[0]), "m=17")


def test_seed_change(env):
    """The same call under seeds 1, 2, 1: the bytes differ as the reference's differ, then are the first again."""
    inp, acc = domain_operands(True)
    want = {s: sr.combine(inp, acc, s) for s in (1, 2)}
    assert (want[1] != want[2]).any()
    d_inp, d_acc, out = gu.to_dev(inp), gu.to_dev(acc), gu.empty_dev(acc.size)
    for s in (1, 2, 1):
        mx4.sr_set_seed(s)
        assert _fold(env, out.fill_(0xA5), d_acc, [d_inp], acc.size // TB) == 0
        _same(gu.from_dev(out, np.uint8), want[s], f"seed {s}")


@pytest.mark.parametrize("seed", [0, 0xC0FFEE])
@pytest.mark.parametrize("src_type", sorted(WIDE))
def test_quantize(src_type, seed):
    """Normals at block magnitudes 2^-20 .. 2^20, their second tile a copy of the first (the tile key tells them
    apart); every bf16 pattern, permuted, and tails.  Exact footprints; mx4.dequantize reads the result."""
    rng = np.random.default_rng(9)
    x = (rng.standard_normal((128, 32)) * np.exp2(rng.integers(-20, 21, (128, 1)))).astype(np.float32).reshape(-1)
    x[512:1024] = x[:512]
    x = fp8_ref.bf16_to_f32(fp8_ref.f32_to_bf16(x)) if src_type == "bf16" else x
    perm = fp8_ref.bf16_to_f32(rng.permutation(np.arange(1 << 16, dtype=np.uint16)))
    for f32, n in [(x, x.size)] + [(perm, n) for n in (perm.size, 1, 31, 33, 511, 513)]:
        twins, f32 = f32 is x, f32[:n]
        want = sr.quantize_ref(f32, seed)
        assert not twins or (want[:TB] != want[TB:2 * TB]).any()
        tiles, d_src = Guarded(mx4.tiles_for(n) * TB, key=1), gu.to_dev(fp8_ref.f32_to_bf16(f32) if src_type == "bf16" else f32)
        assert mx4.quantize_sr(tiles.ptr, d_src, n, WIDE[src_type][0], seed, gu.stream()) == 0
        gu.sync()
        _same(tiles.read(np.uint8), want, f"quantize_sr n={n}")
        assert tiles.guards_intact(), tiles.guards_intact()
        dst = Guarded(n * 4, key=2)
        assert mx4.dequantize(dst.ptr, tiles.ptr, n, ca.FLOAT32, gu.stream()) == 0
        gu.sync()
        _same(dst.read(np.uint32), mx4_ref.dequantize_ref(want, n), f"dequantize n={n}")


@pytest.mark.parametrize("n,k,b", [(2, 2, 1), (4, 4, 4), (4, 2, 2), (8, 4, 4), (8, 2, 2)])
def test_local_group_collectives(env, n, k, b):
    """8 tiles per rank, FLAT and EXACT, against the same plan under the plan evaluator; data: quantized normals."""
    mx4.sr_set_seed(77)
    rng = np.random.default_rng([n, 4])
    sends = [mx4_ref.quantize_ref((rng.standard_normal((128, 32)) * np.exp2(rng.integers(-20, 21, (128, 1))))
                                  .astype(np.float32).reshape(-1)) for _ in range(n)]
    g, d_send = ca.LocalGroup(n, 0), [gu.to_dev(s) for s in sends]
    try:
        for sched in (ca.SCHEDULE_FLAT, ca.SCHEDULE_EXACT):
            g.set_schedule(sched)
            for mode, fn, count in ((ca.MODE_ALLREDUCE, g.all_reduce_radix_batch, 8),
                                    (ca.MODE_REDUCE_SCATTER, g.reduce_scatter_radix_batch, 8 // n)):
                want = sr.expected(mode, sends, k, b, sched, 77)
                recv = [gu.empty_dev(count * TB).fill_(0xA5) for _ in range(n)]
                assert fn(d_send, recv, count, env[0], env[1], k, b) == 0
                gu.sync()
                for r in range(n):
                    _same(gu.from_dev(recv[r], np.uint8), want[r], f"mode {mode} ({n}, {k}, {b}) schedule {sched} rank {r}")
    finally:
        g.destroy()


def test_refusals(env):
    """CHR_UINT8, chr_type_contiguous(67, CHR_UINT32), a pointer one byte in: ERR_UNSUPPORTED, nothing enqueued."""
    x = gu.to_dev(_wild(4, 1))
    out = gu.empty_dev(4 * TB + 16).fill_(0xA5)
    other = ca.type_contiguous(67, ca.UINT32)
    for dt, n, o in ((ca.UINT8, 4 * TB, 0), (other, 4, 0), (env[0], 3, 1)):
        mx4.sr_stats(reset=True)
        assert _fold(env, out.data_ptr() + o, x, [x], n, dt=dt) == ca.ERR_UNSUPPORTED
        assert mx4.sr_stats() == (1, 1, 0), mx4.sr_stats()
    assert ca.type_free(other) == 0
    gu.sync()
    assert bool((out == 0xA5).all())
