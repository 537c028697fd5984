"""libchiara_mx4_tree.so (include/chiara_mx4_tree.h, chiara_amd/mx4.py) on the device: whole expression trees of the MX4
SUM in one pass, bit for bit against the program evaluated on a Python stack with tests/mx4_ref.py's combine."""
import numpy as np
import pytest

import chiara_amd as ca
import gpu_util as gu
import mx4_ref
from chiara_amd import mx4
from footprint_util import Guarded
from test_gpu_mx4 import BIG, TB, _same, _wild
from tree_util import random_program

pytestmark = pytest.mark.gpu

C4 = ([0, 1, 1, 1, 0, 1, 1, 2], [0] * 7)  # the flat schedule's k = 4, b = 4 tree
DEEP = ([0, 0, 0, 3], [1, 0, 1])          # stack depth 4
PROGS = [C4, DEEP] + [random_program(np.random.default_rng([3, nl]), nl) for nl in range(2, 9)]


@pytest.fixture(scope="module", autouse=True)
def env():  # (tile type, op code of the one-pass op); released when the module is done
    yield mx4.mx4_type(), mx4.mx4_sum_tree()
    assert mx4.tree_release() == 0 and mx4.release() == 0


def _eval(leaves, comb, swaps):
    """push leaf j, then comb[j] combines: run = top o run, or with the swap bit run o top."""
    st, ci = [], 0
    for x, c in zip(leaves, comb):
        st.append(x)
        for _ in range(c):
            top, run = st.pop(), st.pop()
            st.append(mx4_ref.combine(run, top) if swaps[ci] else mx4_ref.combine(top, run))
            ci += 1
    assert len(st) == 1
    return st[0]


@pytest.mark.parametrize("n", [1, 2, 3, BIG])
def test_tree_shapes(env, n):
    """Half a two-tile wave trip, one, one and a half, and more trips than a tree has workgroups; every program of
    PROGS, DEEP's depth 4 included (the kernel holds four slots, nothing is declined for depth); `out` out of place,
    over leaf 0 and over the last leaf; pointers 16-B aligned (8-B accesses) or 4 bytes in (4-B accesses), the output
    between guard bands.  One launcher call, one tree, one kernel, nothing declined, no fold -- except for a program
    that one fold launch evaluates with the same traffic (every leaf straight into one running value, one operand
    order: here the 2-leaf one), which is declined to that one fold.  The BIG leaves repeat 7 tiles; BIG lies below the
    31 775 tiles beyond which the launcher leaves a call to the folds for speed."""
    xs = [_wild(min(n, 7), [37, r]) for r in range(8)]
    rep = lambda a: np.resize(a.reshape(-1, TB), (n, TB)).reshape(-1)
    for phase in (0, 4):
        d = [Guarded(n * TB, phase, key=r).load(rep(x)) for r, x in enumerate(xs)]
        spare = Guarded(n * TB, phase, key=99)
        for comb, swaps in PROGS:
            nl = len(comb)
            want = rep(_eval(xs[:nl], comb, swaps))
            chain = all(c == 1 for c in comb[1:]) and len(set(swaps)) == 1
            for where in (None, 0, nl - 1):
                out = spare.reset() if where is None else d[where]
                mx4.tree_stats(reset=True), mx4.stats(reset=True)
                assert ca.reduce_tree(out.ptr, [g.ptr for g in d[:nl]], comb, swaps, n, env[0], env[1], gu.stream()) == 0
                gu.sync()
                got = mx4.tree_stats(), mx4.stats()
                assert got == (((1, 1, 0, 0), (1, 0, 1)) if chain else ((1, 0, 1, 1), (0, 0, 0))), got
                _same(out.read(np.uint8), want, f"n={n} phase={phase} comb={comb} swaps={swaps} out over {where}")
                assert out.guards_intact(), out.guards_intact()
                if where is not None:
                    out.load(rep(xs[where]))


def test_batch_beyond_one_launch(env):
    """9 trees of 5 leaves in one reduce_tree_batch, 3 tiles each: one launcher call, two launches, every tree's bytes."""
    rng = np.random.default_rng(11)
    progs = [random_program(rng, 5) for _ in range(9)]
    leaves = [[_wild(3, [41, t, r]) for r in range(5)] for t in range(9)]
    d = [[gu.to_dev(x) for x in lv] for lv in leaves]
    outs = [gu.empty_dev(3 * TB) for _ in range(9)]
    mx4.tree_stats(reset=True), mx4.stats(reset=True)
    assert ca.reduce_tree_batch(outs, d, [c for c, _ in progs], [s for _, s in progs], 3, env[0], env[1], gu.stream()) == 0
    gu.sync()
    assert mx4.tree_stats() == (1, 0, 9, 2) and mx4.stats()[0] == 0, (mx4.tree_stats(), mx4.stats())
    for t, (comb, swaps) in enumerate(progs):
        _same(gu.from_dev(outs[t], np.uint8), _eval(leaves[t], comb, swaps), f"tree {t}")


@pytest.mark.parametrize("n", [4, 8])
def test_local_group_collectives(env, n):
    """8 tiles per rank under SCHEDULE_FLAT, geometries (4, 4) and (2, 2), against the same plan under the plan
    evaluator (what the fold-only op gives); the trees went to the tree launcher and none was declined (4 ranks under
    (4, 4) reduce in one fold chain, no tree: the counters are read over a case's calls)."""
    rng = np.random.default_rng([n, 4])
    sends = [mx4_ref.quantize_ref((rng.standard_normal((128, 32)) * np.exp2(rng.integers(-20, 21, (128, 1))))
                                  .astype(np.float32).reshape(-1)) for _ in range(n)]
    g, d_send = ca.LocalGroup(n, 0), [gu.to_dev(s) for s in sends]
    try:
        g.set_schedule(ca.SCHEDULE_FLAT)
        mx4.tree_stats(reset=True)
        for k, b in ((4, 4), (2, 2)):
            for mode, fn, count in ((ca.MODE_ALLREDUCE, g.all_reduce_radix_batch, 8),
                                    (ca.MODE_REDUCE_SCATTER, g.reduce_scatter_radix_batch, 8 // n)):
                want = mx4_ref.expected(mode, sends, k, b, ca.SCHEDULE_FLAT)
                recv = [gu.empty_dev(count * TB).fill_(0xA5) for _ in range(n)]
                assert fn(d_send, recv, count, env[0], env[1], k, b) == 0
                gu.sync()
                for r in range(n):
                    _same(gu.from_dev(recv[r], np.uint8), want[r], f"mode {mode} ({n}, {k}, {b}) rank {r}")
        calls, declined, trees, kernels = mx4.tree_stats()
        assert declined == 0 and trees >= calls >= 2 and kernels >= 2, mx4.tree_stats()
    finally:
        g.destroy()


def test_declines(env):
    """CHR_UINT8 and chr_type_contiguous(67, CHR_UINT32): the tree launcher declines, nothing enqueued, and the fold
    launcher's refusal becomes ERR_UNSUPPORTED; the output unchanged."""
    x = gu.to_dev(_wild(4, 1))
    out = gu.empty_dev(4 * TB).fill_(0xA5)
    other = ca.type_contiguous(67, ca.UINT32)
    for dt, n in ((ca.UINT8, 4 * TB), (other, 4)):
        mx4.tree_stats(reset=True)
        assert ca.reduce_tree(out, [x, x, x], [0, 0, 2], [0, 0], n, dt, env[1], gu.stream()) == ca.ERR_UNSUPPORTED
        assert mx4.tree_stats() == (1, 1, 0, 0), mx4.tree_stats()
    assert ca.type_free(other) == 0
    gu.sync()
    assert bool((out == 0xA5).all())
