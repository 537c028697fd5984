"""libchiara_mx6_tree.so (include/chiara_mx6_tree.h, chiara_amd/mx6.py) on the device: whole expression trees of the MXFP6
SUMs in one pass, bit for bit against the program evaluated on a Python stack with tests/mx6_ref.py's combine."""
import ctypes

import numpy as np
import pytest

import chiara_amd as ca
import gpu_util as gu
import mx6_ref
from chiara_amd import mx6
from footprint_util import Guarded
from test_gpu_mx6 import BIG, FORMATS, TB, _same, _wild
from tree_util import random_program

pytestmark = pytest.mark.gpu

C4 = ([0, 1, 1, 1, 0, 1, 1, 2], [0] * 7)  # the flat schedule's k = 4, b = 4 tree
DEEP = ([0, 0, 0, 3], [1, 0, 1])          # stack depth 4: all three park slots live
PROGS = [C4, DEEP] + [random_program(np.random.default_rng([3, nl]), nl) for nl in range(2, 9)]


class UserTree(ctypes.Structure):  # chiara.h chr_user_tree
    _fields_ = [("out", ctypes.c_void_p), ("leaves", ctypes.c_void_p * 8), ("nleaves", ctypes.c_int),
                ("comb", ctypes.c_ubyte * 8), ("swaps", ctypes.c_ubyte * 8), ("n", ctypes.c_size_t)]


@pytest.fixture(scope="module", autouse=True)
def env():  # (tile type, {format: op code of the one-pass op}); released when the module is done
    yield mx6.mx6_type(), {f: mx6.mx6_sum_tree(f) for f in (mx6.E2M3, mx6.E3M2)}
    assert mx6.tree_release() == 0 and mx6.release() == 0


def _eval(leaves, comb, swaps, fmt):
    """push leaf j, then comb[j] combines: run = top o run, or with the swap bit run o top."""
    st, ci = [], 0
    for x, c in zip(leaves, comb):
        st.append(x)
        for _ in range(c):
            top, run = st.pop(), st.pop()
            st.append(mx6_ref.combine(run, top, fmt) if swaps[ci] else mx6_ref.combine(top, run, fmt))
            ci += 1
    assert len(st) == 1
    return st[0]


@FORMATS
@pytest.mark.parametrize("n", [1, 3, 4, 5, BIG])
def test_tree_shapes(env, fmt, n):
    """A quarter of a four-tile wave trip, a trip whose last row is missing, one trip, one and a bit, and more trips
    than a tree has workgroups; wild data (NaN blocks, both clamps, zero blocks); every program of PROGS, DEEP's depth
    4 included; `out` out of place, over leaf 0 and over the last leaf; pointers 16-B aligned or 8 bytes in (8-B
    accesses) or 4 and 12 bytes in (4-B accesses), the output between guard bands.  One launcher call, one tree, one
    kernel, nothing declined, no fold -- except for a program that one fold launch evaluates with the same traffic
    (every leaf straight into one running value, one operand order: here the 2-leaf one), which is declined to that
    one fold.  The BIG leaves repeat 7 tiles."""
    xs = [_wild(min(n, 7), [37, r]) for r in range(8)]
    rep = lambda a: np.resize(a.reshape(-1, TB), (n, TB)).reshape(-1)
    wants = [rep(_eval(xs[:len(comb)], comb, swaps, fmt)) for comb, swaps in PROGS]
    for phase in (0, 4, 8, 12):
        d = [Guarded(n * TB, phase, key=r).load(rep(x)) for r, x in enumerate(xs)]
        spare = Guarded(n * TB, phase, key=99)
        for (comb, swaps), want in zip(PROGS, wants):
            nl = len(comb)
            chain = all(c == 1 for c in comb[1:]) and len(set(swaps)) == 1
            for where in (None, 0, nl - 1):
                out = spare.reset() if where is None else d[where]
                mx6.tree_stats(reset=True), mx6.stats(reset=True)
                assert ca.reduce_tree(out.ptr, [g.ptr for g in d[:nl]], comb, swaps, n, env[0], env[1][fmt], gu.stream()) == 0
                gu.sync()
                got = mx6.tree_stats(), mx6.stats()
                assert got == (((1, 1, 0, 0), (1, 0, 1)) if chain else ((1, 0, 1, 1), (0, 0, 0))), got
                _same(out.read(np.uint8), want, f"n={n} phase={phase} comb={comb} swaps={swaps} out over {where}")
                assert out.guards_intact(), out.guards_intact()
                if where is not None:
                    out.load(rep(xs[where]))


@FORMATS
def test_batch_beyond_one_launch(env, fmt):
    """9 trees of 5 leaves in one reduce_tree_batch, 3 tiles each, tree 4 four bytes in: one launcher call, one launch
    of 8-B accesses that is full at its 8 trees and one of 4-B accesses, every tree's bytes between guard bands."""
    rng = np.random.default_rng(11)
    progs = [random_program(rng, 5) for _ in range(9)]
    leaves = [[_wild(3, [41, t, r]) for r in range(5)] for t in range(9)]
    d = [[Guarded(3 * TB, 4 if t == 4 else 0, key=r).load(x) for r, x in enumerate(lv)] for t, lv in enumerate(leaves)]
    outs = [Guarded(3 * TB, 4 if t == 4 else 0, key=99) for t in range(9)]
    mx6.tree_stats(reset=True), mx6.stats(reset=True)
    assert ca.reduce_tree_batch([o.ptr for o in outs], [[g.ptr for g in lv] for lv in d], [c for c, _ in progs],
                                [s for _, s in progs], 3, env[0], env[1][fmt], gu.stream()) == 0
    gu.sync()
    assert mx6.tree_stats() == (1, 0, 9, 2) and mx6.stats()[0] == 0, (mx6.tree_stats(), mx6.stats())
    for t, (comb, swaps) in enumerate(progs):
        _same(outs[t].read(np.uint8), _eval(leaves[t], comb, swaps, fmt), f"tree {t}")
        assert outs[t].guards_intact(), outs[t].guards_intact()


@FORMATS
@pytest.mark.parametrize("n", [2, 4, 8])
def test_local_group_collectives(env, fmt, n):
    """8 tiles per rank under SCHEDULE_FLAT, geometries (4, 4) and (2, 2) -- 2 ranks have no plan under (4, 4) and run
    (2, 2) alone -- against the same plan under the plan evaluator (what the fold-only op gives); where trees occur
    they went to the tree launcher and none was declined (4 ranks under (4, 4) reduce in one fold chain, no tree: the
    counters are read over a case's calls; 2 ranks have nothing but 2-leaf chains, the folds' by the launcher's rule,
    and only their bytes are checked)."""
    rng = np.random.default_rng([n, 7])
    sends = [mx6_ref.quantize_ref((rng.standard_normal((128, 32)) * np.exp2(rng.integers(-20, 21, (128, 1))))
                                  .astype(np.float32).reshape(-1), fmt) for _ in range(n)]
    g, d_send = ca.LocalGroup(n, 0), [gu.to_dev(s) for s in sends]
    try:
        g.set_schedule(ca.SCHEDULE_FLAT)
        mx6.tree_stats(reset=True)
        for k, b in ((4, 4), (2, 2))[n == 2:]:
            for mode, fn, count in ((ca.MODE_ALLREDUCE, g.all_reduce_radix_batch, 8),
                                    (ca.MODE_REDUCE_SCATTER, g.reduce_scatter_radix_batch, 8 // n)):
                want = mx6_ref.expected(fmt, mode, sends, k, b, ca.SCHEDULE_FLAT)
                recv = [gu.empty_dev(count * TB).fill_(0xA5) for _ in range(n)]
                assert fn(d_send, recv, count, env[0], env[1][fmt], k, b) == 0
                gu.sync()
                for r in range(n):
                    _same(gu.from_dev(recv[r], np.uint8), want[r], f"mode {mode} ({n}, {k}, {b}) rank {r}")
        calls, declined, trees, kernels = mx6.tree_stats()
        assert n == 2 or (declined == 0 and trees >= calls >= 2 and kernels >= 2), mx6.tree_stats()
    finally:
        g.destroy()


@FORMATS
def test_declines(env, fmt):
    """CHR_UINT8 and chr_type_contiguous(99, CHR_UINT32): the tree launcher declines, nothing enqueued, and the fold
    launcher's refusal becomes ERR_UNSUPPORTED.  9 leaves and a depth-5 program never reach a launcher through
    chr_reduce_tree (the library refuses them itself, tests/test_tree_program.py), so the exported launcher is called
    directly: nonzero, counted as declined, nothing enqueued.  The output unchanged throughout."""
    x = gu.to_dev(_wild(4, 1))
    out = gu.empty_dev(4 * TB).fill_(0xA5)
    other = ca.type_contiguous(99, ca.UINT32)
    for dt, n in ((ca.UINT8, 4 * TB), (other, 4)):
        mx6.tree_stats(reset=True)
        assert ca.reduce_tree(out, [x, x, x], [0, 0, 2], [0, 0], n, dt, env[1][fmt], gu.stream()) == ca.ERR_UNSUPPORTED
        assert mx6.tree_stats() == (1, 1, 0, 0), mx6.tree_stats()
    assert ca.type_free(other) == 0
    launch = getattr(mx6.mx6_tree_lib(), f"chr_mx6_{('e2m3', 'e3m2')[fmt]}_sum_tree_launch")
    launch.argtypes = [ctypes.POINTER(UserTree), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    for nl, comb in ((9, [0] + [1] * 7), (7, [0, 0, 0, 0, 0, 3, 1])):  # 9 leaves; depth 5
        t = UserTree(out=out.data_ptr(), nleaves=nl, n=4)
        for j in range(8):
            t.leaves[j] = x.data_ptr()
        for j, c in enumerate(comb):
            t.comb[j] = c
        mx6.tree_stats(reset=True)
        assert launch(ctypes.byref(t), 1, env[0], 0, gu.stream().cuda_stream, None) != 0
        assert mx6.tree_stats() == (1, 1, 0, 0), mx6.tree_stats()
    gu.sync()
    assert bool((out == 0xA5).all())
