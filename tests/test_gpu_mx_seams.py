"""The launcher seams of the four tile libraries (libchiara_mx.so, libchiara_mx_tree.so, libchiara_mx4.so,
libchiara_mx4_tree.so) that tests/test_gpu_mx*.py leave alone: fan-in beyond one fold launch, alignment residues 8 and
12, the tree launchers called directly with a residency cap and a mixed batch, MXFP4's size gate, and uneven pipeline
slices through a LocalGroup.  Bit for bit against tests/mx_ref.py and tests/mx4_ref.py (themselves held to the headers
by tests/test_mx_host.py); every test also reads the launchers' counters, so that a result alone never stands for the
path it was meant to take."""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest

import chiara_amd as ca
import fp8_ref
import gpu_util as gu
import mx4_ref
import mx_ref
import test_gpu_mx as t8
import test_gpu_mx4 as t4
import test_gpu_mx4_tree as t4t
import test_gpu_mx_tree as t8t
from chiara_amd import mx, mx4
from footprint_util import Guarded
from test_gpu_mx_tree import C4, DEEP
from test_gpu_user_tree import UserTree
from tree_util import random_program

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MX4_TREE_SRC = os.path.join(REPO, "configurable-hierarchical-allreduce-algorithms_amd", "csrc", "ops", "mx4_tree_ops.hip")


def _kind(name):
    """One tile library under test: its Python module, reference and the constants of its launchers."""
    if name == "mx4":
        return types.SimpleNamespace(
            name=name, lib=mx4, TB=t4.TB, BIG=t4.BIG, wild=t4._wild, combine=mx4_ref.combine, eval=t4t._eval,
            quantize=mx4_ref.quantize_ref, expected=mx4_ref.expected, vec_mask=7,  # mx4_tree_ops.hip tree_vec: & 7
            launcher=lambda: mx4.mx4_tree_lib().chr_mx4_sum_tree_launch)
    f = fp8_ref.FORMATS[name]
    return types.SimpleNamespace(
        name=name, lib=mx, TB=t8.TB, BIG=t8.BIG, wild=t8._wild, combine=functools.partial(mx_ref.combine, f),
        eval=functools.partial(t8t._eval, f), quantize=functools.partial(mx_ref.quantize_ref, f),
        expected=functools.partial(mx_ref.expected, f), vec_mask=15,  # mx_tree_ops.hip tree_vec: & 15
        launcher=lambda: getattr(mx.mx_tree_lib(), f"chr_mx_{name}_sum_tree"))


KINDS = [_kind(n) for n in ("e4m3", "e5m2", "mx4")]
KIND = pytest.mark.parametrize("K", KINDS, ids=lambda K: K.name)
MX4 = KINDS[2]


@pytest.fixture(scope="module")
def env():  # {kind: (tile type, fold-only op, one-pass op)}; released when the module is done
    e = {"mx4": (mx4.mx4_type(), mx4.mx4_sum(), mx4.mx4_sum_tree())}
    for name, f in t8.FORMATS:
        e[name] = (mx.mx_type(), mx.mx_sum(f), mx.mx_sum_tree(f))
    yield e
    assert mx4.tree_release() == 0 and mx4.release() == 0 and mx.tree_release() == 0 and mx.release() == 0


_same = t8._same


def _rep(K, a, n):
    return np.resize(a.reshape(-1, K.TB), (n, K.TB)).reshape(-1)


def _reset(K):
    K.lib.stats(reset=True), K.lib.tree_stats(reset=True)


# ---- fan-in beyond one fold launch ---------------------------------------------------------------------------------

@KIND
@pytest.mark.parametrize("n", [3, "BIG"])
def test_fan_in_beyond_one_launch(env, K, n):
    """m = 17 and 33 through chr_reduce_multi_ex, which has no fan-in limit of its own: the fold launcher splits at
    kMaxIns = 16 and each later launch continues from `out` (`cur = out`, a second FoldArgs) -- with `out` apart from
    `acc` the only place where the two differ.  3 tiles and BIG (workgroups stride), `out` aliasing `acc` or not,
    pointers 16-B aligned or 4 bytes in, both running_first, the output between guard bands; the operands repeat 8
    buffers of 7 distinct tiles.  Expected: the left fold of the reference's combine.  The path is known by the
    launcher's counters: one call, nothing declined, ceil(m / 16) kernels."""
    n = K.BIG if n == "BIG" else n
    dt, op, _ = env[K.name]
    xs = [K.wild(min(n, 7), [43, r]) for r in range(8)]
    for phase in (0, 4):
        d = [Guarded(n * K.TB, phase, key=r).load(_rep(K, x, n)) for r, x in enumerate(xs)]
        out = Guarded(n * K.TB, phase, key=99)
        for m in (17, 33):
            which = [1 + j % 7 for j in range(m)]
            for rf in (0, 1):
                fold = lambda r, x: K.combine(r, x) if rf else K.combine(x, r)
                want = _rep(K, functools.reduce(fold, [xs[w] for w in which], xs[0]), n)
                for alias in (False, True):
                    out.reset()
                    acc = out.load(_rep(K, xs[0], n)).ptr if alias else d[0].ptr
                    _reset(K)
                    assert ca.reduce_multi_ex(out.ptr, acc, [d[w].ptr for w in which], n, dt, op, rf, gu.stream()) == 0
                    gu.sync()
                    assert K.lib.stats() == (1, 0, -(-m // 16)), K.lib.stats()
                    _same(out.read(np.uint8), want, f"n={n} phase={phase} m={m} running_first={rf} alias={alias}")
                    assert out.guards_intact(), out.guards_intact()


# ---- alignment residues 8 and 12 -----------------------------------------------------------------------------------

@KIND
@pytest.mark.parametrize("phase", [8, 12])
def test_residues_8_and_12(env, K, phase):
    """Every pointer 8 or 12 bytes past a 16-byte boundary: the fold at m = 2 (its 4-B instantiation: the fold tests
    `& 15`) and the tree on C4 and DEEP, n = 1, 3, 5 tiles, bytes and guard bands.  At 8 the MX4 tree alone keeps its
    wide (8-B) instantiation (its tree_vec tests `& 7`, MXFP8's `& 15`); the bytes cannot show which one ran, the
    launch count of a mixed batch does: two C4 trees in one reduce_tree_batch, one 16-B aligned and one at this
    residue, share a grid (one kernel) exactly when both take the same instantiation -- MX4 at residue 8 -- and take
    two kernels everywhere else."""
    dt, fold_op, tree_op = env[K.name]
    for n in (1, 3, 5):
        xs = [K.wild(n, [47, r]) for r in range(8)]
        d = [Guarded(n * K.TB, phase, key=r).load(x) for r, x in enumerate(xs)]
        out = Guarded(n * K.TB, phase, key=99)
        assert out.ptr % 16 == phase
        _reset(K)
        assert ca.reduce_multi_ex(out.ptr, d[0].ptr, [d[1].ptr, d[2].ptr], n, dt, fold_op, 0, gu.stream()) == 0
        gu.sync()
        assert K.lib.stats() == (1, 0, 1), K.lib.stats()
        _same(out.read(np.uint8), K.combine(xs[2], K.combine(xs[1], xs[0])), f"fold n={n}")
        assert out.guards_intact(), out.guards_intact()
        for comb, swaps in (C4, DEEP):
            nl = len(comb)
            out.reset()
            _reset(K)
            assert ca.reduce_tree(out.ptr, [g.ptr for g in d[:nl]], comb, swaps, n, dt, tree_op, gu.stream()) == 0
            gu.sync()
            assert (K.lib.tree_stats(), K.lib.stats()) == ((1, 0, 1, 1), (0, 0, 0)), (K.lib.tree_stats(), K.lib.stats())
            _same(out.read(np.uint8), K.eval(xs[:nl], comb, swaps), f"tree n={n} comb={comb}")
            assert out.guards_intact(), out.guards_intact()
        # the mixed batch: tree 0 at residue 0, tree 1 at this residue
        d0 = [Guarded(n * K.TB, 0, key=20 + r).load(x) for r, x in enumerate(xs)]
        outs = [Guarded(n * K.TB, 0, key=98), out.reset()]
        _reset(K)
        assert ca.reduce_tree_batch([o.ptr for o in outs], [[g.ptr for g in d0], [g.ptr for g in d]], [C4[0]] * 2,
                                    [C4[1]] * 2, n, dt, tree_op, gu.stream()) == 0
        gu.sync()
        kernels = 1 if phase & K.vec_mask == 0 else 2
        assert K.lib.tree_stats() == (1, 0, 2, kernels), (K.lib.tree_stats(), kernels)
        for o in outs:
            _same(o.read(np.uint8), K.eval(xs, *C4), f"mixed batch n={n}")
            assert o.guards_intact(), o.guards_intact()


# ---- the tree launchers called directly ----------------------------------------------------------------------------

def _launcher(K):
    fn = K.launcher()
    fn.argtypes = [ctypes.POINTER(UserTree), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def _user_tree(out, leaves, comb, swaps, n):
    t = UserTree()
    t.out, t.nleaves, t.n = out, len(leaves), n
    for j, p in enumerate(leaves):
        t.leaves[j], t.comb[j] = p, comb[j]
    for c, s in enumerate(swaps):
        t.swaps[c] = s
    return t


@KIND
@pytest.mark.parametrize("phases", [[0, 4] * 4 + [0], [0] * 3 + [4, 0, 0, 4, 0, 0, 4, 0, 0, 0]], ids=["5+4", "10+3"])
def test_launcher_direct_cap_and_mixed_batch(env, K, phases):
    """The tree launcher itself, as the library calls it from inside a comm call with overlap on: wg_per_cu = 12
    (kCoresidentWgPerCu), beside 0 (the launcher's own 16) and 32 -- the value sizes the launch's dynamic LDS, which
    no test through chr_reduce_tree* or a LocalGroup ever passes.  One call holds trees of both instantiations
    interleaved, 3 tiles each: random programs of 2 .. 8 leaves, C4 and DEEP; the 2-leaf one is a single-fold chain
    and rides along because the others pay.  `5+4`: five trees 16-B aligned and four 4 bytes in, one grid per
    instantiation.  `10+3`: the wide pass flushes at kMaxTreesPerLaunch = 8 and its second grid holds two trees, so
    block0 is filled a second time after a flush.  Every cap gives the bytes of the Python stack evaluation, between
    guard bands, and tree_stats() the launches the code implies: per instantiation ceil(trees / 8)."""
    dt = env[K.name][0]
    fn = _launcher(K)
    rng = np.random.default_rng(3)
    progs = ([random_program(rng, nl) for nl in range(2, 9)] + [C4, DEEP]) * 2
    n, trees = 3, []
    for t, phase in enumerate(phases):
        comb, swaps = progs[t]
        xs = [K.wild(n, [53, t, r]) for r in range(len(comb))]
        d = [Guarded(n * K.TB, phase, key=16 * t + r).load(x) for r, x in enumerate(xs)]
        trees.append((Guarded(n * K.TB, phase, key=1000 + t), d, comb, swaps, K.eval(xs, comb, swaps)))
    wide = sum(1 for p in phases if p == 0)
    kernels = -(-wide // 8) + -(-(len(phases) - wide) // 8)
    for cap in (0, 12, 32):
        arr = (UserTree * len(trees))(*[_user_tree(o.reset().ptr, [g.ptr for g in d], comb, swaps, n)
                                        for o, d, comb, swaps, _ in trees])
        _reset(K)
        assert fn(arr, len(trees), dt, cap, gu.stream().cuda_stream, None) == 0
        gu.sync()
        assert (K.lib.tree_stats(), K.lib.stats()) == ((1, 0, len(trees), kernels), (0, 0, 0)), K.lib.tree_stats()
        for t, (o, _, comb, _, want) in enumerate(trees):
            _same(o.read(np.uint8), want, f"cap {cap} tree {t} comb={comb}")
            assert o.guards_intact(), o.guards_intact()


# ---- MXFP4's size gate ---------------------------------------------------------------------------------------------

def _gate():
    """kOnePassMaxTiles, from its one definition (csrc/ops/mx4_tree_ops.hip: `constexpr size_t kOnePassMaxTiles = ...;`)."""
    with open(MX4_TREE_SRC) as f:
        (v,) = re.findall(r"^constexpr size_t kOnePassMaxTiles = (\d+);", f.read(), re.M)
    return int(v)


def test_mx4_size_gate(env):
    """Both sides of kOnePassMaxTiles (MXFP8's launcher has no such gate): a 3-leaf program with an inner node at
    exactly the gate is taken -- tree_stats() == (1, 0, 1, 1), no fold call -- and one tile more is declined whole and
    evaluated by the folds -- (1, 1, 0, 0), fold calls, none declined; both give the reference's bytes, the leaves
    repeating 7 tiles.  reduce_tree_batch serves one count to all its trees, so "any tree larger declines the call"
    goes through the launcher itself: a 3-tile tree beside one over the gate returns nonzero and both outputs keep
    their 0xA5 fill."""
    K, (dt, _, tree_op) = MX4, env["mx4"]
    gate = _gate()
    assert gate > t4.BIG
    comb, swaps = [0, 0, 2], [0, 1]
    xs = [K.wild(7, [59, r]) for r in range(3)]
    want7 = K.eval(xs, comb, swaps)
    d = [gu.to_dev(_rep(K, x, gate + 1)) for x in xs]
    out = gu.empty_dev((gate + 1) * K.TB)
    for n in (gate, gate + 1):
        out.fill_(0xA5)
        _reset(K)
        assert ca.reduce_tree(out, d, comb, swaps, n, dt, tree_op, gu.stream()) == 0
        gu.sync()
        got = K.lib.tree_stats(), K.lib.stats()
        if n == gate:
            assert got == ((1, 0, 1, 1), (0, 0, 0)), got
        else:
            assert got[0] == (1, 1, 0, 0) and got[1][0] >= 1 and got[1][1] == 0 and got[1][2] >= 1, got
        res = gu.from_dev(out, np.uint8)
        _same(res[:n * K.TB], _rep(K, want7, n), f"n={n}")
        assert (res[n * K.TB:] == 0xA5).all()
    small = [gu.to_dev(x[:3 * K.TB]) for x in xs]
    small_out = gu.empty_dev(3 * K.TB).fill_(0xA5)
    out.fill_(0xA5)
    arr = (UserTree * 2)(_user_tree(small_out.data_ptr(), [g.data_ptr() for g in small], comb, swaps, 3),
                         _user_tree(out.data_ptr(), [g.data_ptr() for g in d], comb, swaps, gate + 1))
    _reset(K)
    assert _launcher(K)(arr, 2, dt, 0, gu.stream().cuda_stream, None) != 0
    gu.sync()
    assert (K.lib.tree_stats(), K.lib.stats()) == ((1, 1, 0, 0), (0, 0, 0))
    assert bool((small_out == 0xA5).all()) and bool((out == 0xA5).all())


# ---- uneven pipeline slices ----------------------------------------------------------------------------------------

def marked_sends(K, world, tiles, seed):
    """Every rank's send: quantized normals over 40 binades, then one NaN block (scale 0xFF) and one all-zero block
    (scale 0, codes 0) at positions that depend on the rank, so that propagation across ranks shows in the bytes."""
    sends = []
    for r in range(world):
        rng = np.random.default_rng([seed, r])
        v = rng.standard_normal((tiles * 16, 32)) * np.exp2(rng.integers(-20, 21, (tiles * 16, 1)))
        t = K.quantize(v.astype(np.float32).reshape(-1)).reshape(tiles, K.TB).copy()
        codes = (K.TB - 16) // 16
        for blk, scale in (((37 * r + 5) % (tiles * 16), 0xFF), ((53 * r + 11) % (tiles * 16), 0)):
            t[blk // 16, blk % 16] = scale
            if scale == 0:
                t[blk // 16, 16 + blk % 16 * codes:16 + (blk % 16 + 1) * codes] = 0
        sends.append(t.reshape(-1))
    return sends


def planned(mode, world, rank, k, b, count, slices):
    """(slices, tree steps, the trees' distinct tile counts) of a rank's flat plan: what the planner made of the call."""
    text = ca.describe_plan(mode, world, rank, k, b, count, slices=slices, schedule=ca.SCHEDULE_FLAT)
    return (int(re.search(r" slices=(\d+)", text).group(1)), text.count("\ntree "),
            sorted({int(x) for x in re.findall(r"\ntree \w+ \d+ \w+ \d+ (\d+)", text)}))


@KIND
@pytest.mark.parametrize("tiles", [40, 8, 1552])
def test_uneven_slices_local_group(env, K, tiles):
    """8 virtual ranks, SCHEDULE_FLAT, set_slices(3), allreduce and reduce-scatter, the fold-only op and the one-pass
    op, against the plan evaluator (which knows no slices).  Each rank's send holds a NaN block and an all-zero block.
    40 and 8 tiles, (k, b) = (4, 4) and (2, 2): the planner cuts slices at 256-element and pieces at 64-element bounds
    (csrc/schedule.cpp build_plan_flat), so these counts run as one slice (asserted from the plan) -- but they do
    give ranks whose piece is empty beside one rank that holds the whole chunk, and the virtual ranks' jobs of a step
    share one launcher call: user_trees filters the n == 0 jobs before the launcher sees them, which takes n == 0 for
    a tree it cannot evaluate and would decline the call, so declined == 0 pins the filter.
    1552 tiles, allreduce at (4, 4): chunks of 776 tiles, which three slices do cut, into 256, 256 and 264, and the
    pieces into trees of 64 and 72 tiles beside empty ones -- trees of different tile counts in one launcher call (both
    asserted from the plan).  The fold-only op's calls never touch the tree launcher; the one-pass op's all did."""
    dt, fold_op, tree_op = env[K.name]
    sends = marked_sends(K, 8, tiles, 61)
    g, d_send = ca.LocalGroup(8, 0), [gu.to_dev(s) for s in sends]
    cases = [(k, b, mode) for k, b in ((4, 4), (2, 2)) for mode in (ca.MODE_ALLREDUCE, ca.MODE_REDUCE_SCATTER)]
    try:
        g.set_schedule(ca.SCHEDULE_FLAT)
        g.set_slices(3)
        for k, b, mode in cases if tiles != 1552 else cases[:1]:
            fn, count = ((g.all_reduce_radix_batch, tiles) if mode == ca.MODE_ALLREDUCE else
                         (g.reduce_scatter_radix_batch, tiles // 8))
            plans = [planned(mode, 8, r, k, b, count, 3) for r in range(8)]
            if tiles == 1552:
                assert all(p[0] == 3 for p in plans) and {x for p in plans for x in p[2]} == {64, 72}, plans
                assert any(p[1] == 0 for p in plans)
            else:
                assert all(p[0] == 1 for p in plans), plans
            want = K.expected(mode, sends, k, b, ca.SCHEDULE_FLAT)
            assert any((w.reshape(-1, K.TB)[:, :16] == 0xFF).any() for w in want)  # a NaN block came through
            for op in (fold_op, tree_op):
                recv = [gu.empty_dev(count * K.TB).fill_(0xA5) for _ in range(8)]
                _reset(K)
                assert fn(d_send, recv, count, dt, op, k, b) == 0
                gu.sync()
                calls, declined, trees, kernels = K.lib.tree_stats()
                if op == fold_op:
                    assert (calls, K.lib.stats()[1]) == (0, 0) and K.lib.stats()[0] >= 1, (K.lib.tree_stats(), K.lib.stats())
                else:
                    assert declined == 0 and trees >= calls >= 1 and kernels >= 1, K.lib.tree_stats()
                for r in range(8):
                    _same(gu.from_dev(recv[r], np.uint8), want[r], f"mode {mode} ({k}, {b}) op {op} rank {r}")
    finally:
        g.destroy()
