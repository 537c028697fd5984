"""The binary16 ops of libchiara_ops.so (include/chiara_ops.h, chiara_amd/ops.py) on the device, bit for bit against
tests/f16_ref.py: the whole operand domain, every path of the fold and tree kernels the public header compiles for a
2-byte element, what a call touches besides its result, the collectives on a local group under every schedule, the
MPICH baselines and the refusals.  The module's teardown releases the ops."""
import functools

import numpy as np
import pytest

import chiara_amd as ca
import f16_ref
import pyoracle as po
from chiara_amd import ops
from footprint_util import Guarded
from streaming_cases import STATIC_PROGS, _nonzero_swaps, batch_programs
from tree_util import random_program

pytestmark = pytest.mark.gpu

F16 = ops.F16_DTYPE
OPS = f16_ref.OPS


@pytest.fixture(scope="module")
def gu():
    import gpu_util

    return gpu_util


@pytest.fixture(scope="module", autouse=True)
def code():
    """op name -> op code; released when the module is done."""
    codes = {name: ops.float16_op(f16_ref.KIND[name]) for name in OPS}
    yield codes
    assert ops.release() == 0


@pytest.fixture(scope="module")
def groups():
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = ca.LocalGroup(n, 0)
        return cache[n]

    yield get
    for g in cache.values():
        g.destroy()


def _report(got, want, x=None, y=None):
    """How many elements differ and the first of them, operands included where given."""
    bad = np.flatnonzero(got != want)
    rows = []
    for i in bad[:8]:
        ops_ = f"in={int(x[i]):#06x} inout={int(y[i]):#06x} " if x is not None else ""
        rows.append(f"[{i}] {ops_}got={int(got[i]):#06x} want={int(want[i]):#06x}")
    return f"{bad.size} of {got.size} elements differ: " + "; ".join(rows)


def _same(got, want, what, x=None, y=None):
    assert got.dtype == np.uint16 and got.shape == want.shape, what
    assert np.array_equal(got, want), f"{what}: {_report(got, want, x, y)}"


def _data(op, n, seed, rank):
    """Operands on which the op's operand order and association show: SUM and MAX on TIES-like data (+-0, NaNs of
    every kind, infinities) and on U[-1, 1); PROD and MIN on random bits and, so that long products stay finite, on
    factors near one."""
    h = n // 2
    if op in ("sum", "max"):
        return np.concatenate([f16_ref.ties(h, seed, rank), f16_ref.uniform(n - h, seed, rank)])
    rng = np.random.default_rng([seed, rank, 9])
    near_one = rng.uniform(0.8, 1.25, n - h).astype(np.float16).view(np.uint16)
    return np.concatenate([f16_ref.random_bits(h, seed, rank), near_one])


class Dev:
    """n elements at `off` bytes into a 16-byte aligned device allocation."""

    def __init__(self, gu, n, off=0, host=None):
        self.gu, self.n, self.off = gu, n, off
        self.t = gu.empty_dev(2 * n + 32)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + off
        if host is not None:
            self.load(host)

    def load(self, host):
        self.t[self.off:self.off + 2 * self.n] = self.gu.to_dev(host)
        return self

    def fill(self, byte):
        self.t.fill_(byte)
        return self

    def read(self):
        return self.t[self.off:self.off + 2 * self.n].cpu().numpy().view(np.uint16)


# ---- the operand domain ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def domain(gu):
    """All 65 536 bit patterns against each of the 64 partners: 4 Mi elements."""
    acc = np.tile(np.arange(1 << 16, dtype=np.uint16), 64)
    inp = np.repeat(f16_ref.partners(), 1 << 16)
    return acc, inp, gu.to_dev(acc), gu.to_dev(inp)


@pytest.mark.parametrize("op", OPS)
def test_operand_domain(gu, code, domain, op):
    """Every bit pattern as `inout` against 64 partners as `in` (+-0, +-smallest and +-largest subnormal, +-smallest
    normal, +-1, +-65504, +-inf, quiet / signalling / negative NaNs, random fill), both operand orders, one fold
    each: bit for bit.  This is what decides whether gfx950's half add and multiply keep subnormals and round as IEEE
    under the package's flags, and whether MAX / MIN move the chosen operand's bits untouched."""
    acc, inp, d_acc, d_in = domain
    n = acc.size
    for rf in (0, 1):
        out = gu.empty_dev(2 * n).fill_(0xA5)
        assert ca.reduce_multi_ex(out, d_acc, [d_in], n, F16, code[op], rf, gu.stream()) == 0
        gu.sync()
        got = gu.from_dev(out, np.uint16, n)
        x, y = (acc, inp) if rf else (inp, acc)  # running first: acc o in = f(in = acc, inout = in)
        want = f16_ref.combine(op, x, y)
        print(f"operand domain {op} running_first={rf}: {int(np.count_nonzero(got != want))} of {n} elements differ")
        _same(got, want, f"{op} running_first={rf}", x, y)


# ---- fold shapes ---------------------------------------------------------------------------------------------------

FOLD_N = 8 * (2 * 1024 + 300) + 5  # two whole chunks of 4 vectors x 256 lanes, 300 grid-stride vectors, a tail of 5
FOLD_M = (1, 2, 3, 8, 16, 17)      # 17: two launches past kMaxIns
# bytes into the allocation of (acc, every in, out): all aligned; all one element in (element-wise); only out shifted
LAYOUTS = {"aligned": (0, 0, 0), "all one element in": (2, 2, 2), "out one element in": (0, 0, 2)}


@functools.lru_cache(maxsize=None)
def _fold_operands(op):
    xs = [_data(op, FOLD_N, 77, r) for r in range(18)]
    for x in xs:
        x.flags.writeable = False
    return xs


@pytest.mark.parametrize("op", OPS)
def test_fold_shapes(gu, code, op):
    xs = _fold_operands(op)
    for layout, (o_acc, o_in, o_out) in LAYOUTS.items():
        d = [Dev(gu, FOLD_N, o_acc if j == 0 else o_in, x) for j, x in enumerate(xs)]
        work = Dev(gu, FOLD_N, o_out)
        for m in FOLD_M:
            ins = [b.ptr for b in d[1:1 + m]]
            for rf in (0, 1):
                want = f16_ref.fold_ref(xs[0], xs[1:1 + m], op, bool(rf))
                for inplace in (False, True):
                    if inplace:  # out == acc: a copy of the accumulator at the output's place
                        work.fill(0xA5).load(xs[0])
                        acc = work.ptr
                    else:
                        work.fill(0xA5)
                        acc = d[0].ptr
                    rc = ca.reduce_multi_ex(work.ptr, acc, ins, FOLD_N, F16, code[op], rf, gu.stream())
                    assert rc == 0
                    gu.sync()
                    _same(work.read(), want, f"{op} {layout} m={m} running_first={rf} inplace={inplace}")


# ---- tree shapes ---------------------------------------------------------------------------------------------------

TREE_N = 8 * (3 * 256 + 70) + 5  # whole and partial trips at U = 4, 2 and 1 (256 / 128 / 64 vectors), a tail of 5


@functools.lru_cache(maxsize=None)
def _tree_operands(op):
    xs = [_data(op, TREE_N, 91, r) for r in range(9)]
    for x in xs:
        x.flags.writeable = False
    return xs


def _tree_cases():
    """(comb, swaps, what): every static program unswapped and swapped, one non-static program per leaf count."""
    rng = np.random.default_rng(1609)
    out = []
    for nl, progs in STATIC_PROGS.items():
        for comb in progs:
            out.append((comb, [0] * (nl - 1), "static"))
            out.append((comb, _nonzero_swaps(rng, nl), "static swapped"))
    for nl in range(3, 9):
        while True:
            comb, swaps = random_program(rng, nl)
            if comb not in STATIC_PROGS.get(nl, []):
                break
        out.append((comb, swaps, "non-static"))
    return out


TREE_CASES = _tree_cases()


@pytest.mark.parametrize("op", OPS)
def test_tree_shapes(gu, code, op):
    """Every static program of the library's streaming trees, unswapped and with a nonzero swap word, and a random
    non-static program per leaf count 3..8, each in one pass (one tree-launcher call, no fold call); the root over
    leaf 0 and over the last leaf; a tree with a misaligned leaf, and one with a misaligned root, element-wise."""
    xs = _tree_operands(op)
    d = [Dev(gu, TREE_N, 0, x) for x in xs]
    out = Dev(gu, TREE_N)

    def run(comb, swaps, leaves, dst, what):
        ops.stats(reset=True)
        rc = ca.reduce_tree(dst.ptr, [b.ptr for b in leaves], comb, swaps, TREE_N, F16, code[op], gu.stream())
        assert rc == 0, what
        gu.sync()
        assert ops.stats() == (0, 1, 1), (what, ops.stats())
        _same(dst.read(), f16_ref.tree_ref(xs[:len(comb)], comb, swaps, op), f"{op} {what} {comb} {swaps}")

    for comb, swaps, what in TREE_CASES:
        run(comb, swaps, d[:len(comb)], out.fill(0xA5), what)
    for nl, progs in STATIC_PROGS.items():
        comb, swaps = progs[-1], _nonzero_swaps(np.random.default_rng(nl), nl)
        for alias in (0, nl - 1):
            leaves = list(d[:nl])
            leaves[alias] = out.fill(0xA5).load(xs[alias])
            run(comb, swaps, leaves, out, f"out = leaf {alias}")
    comb, swaps = STATIC_PROGS[8][0], [1, 0, 0, 1, 0, 1, 0]
    shifted_leaf = Dev(gu, TREE_N, 2, xs[3])
    run(comb, swaps, d[:3] + [shifted_leaf] + d[4:8], out.fill(0xA5), "leaf 3 one element in")
    run(comb, swaps, d[:8], Dev(gu, TREE_N, 2).fill(0xA5), "out one element in")


def test_tree_batch_of_nine(gu, code):
    """chr_reduce_tree_batch of 9 eight-leaf trees (two launches: 8 segments and 1), SUM: one tree-launcher call."""
    op = "sum"
    xs = _tree_operands(op)
    d = [Dev(gu, TREE_N, 0, x) for x in xs]
    progs = batch_programs()
    outs = [Dev(gu, TREE_N).fill(0xA5) for _ in progs]
    rows = [[d[(t + j) % 9] for j in range(8)] for t in range(len(progs))]
    ops.stats(reset=True)
    rc = ca.reduce_tree_batch([o.ptr for o in outs], [[b.ptr for b in row] for row in rows], [p[0] for p in progs],
                              [p[1] for p in progs], TREE_N, F16, code[op], gu.stream())
    assert rc == 0
    gu.sync()
    assert ops.stats() == (0, 1, len(progs))
    for t, (comb, swaps) in enumerate(progs):
        want = f16_ref.tree_ref([xs[(t + j) % 9] for j in range(8)], comb, swaps, op)
        _same(outs[t].read(), want, f"batch tree {t} {comb} {swaps}")


# ---- footprint -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("phase", [0, 2])
def test_footprint_fold_and_tree(gu, code, phase):
    """One fold (m = 3) and one 8-leaf tree, every operand between stamped guard bands, aligned (the vector paths)
    and one element in (element-wise): the result is right, the output's guards are intact and no input changed."""
    op, n = "sum", FOLD_N
    xs = _fold_operands(op)[:8]
    ins = [Guarded(2 * n, phase, key=10 + j).load(x) for j, x in enumerate(xs)]
    snaps = [g.snapshot() for g in ins]
    out = Guarded(2 * n, phase, key=99)
    assert ca.reduce_multi_ex(out.ptr, ins[0].ptr, [g.ptr for g in ins[1:4]], n, F16, code[op], 0, gu.stream()) == 0
    gu.sync()
    _same(out.read(np.uint16), f16_ref.fold_ref(xs[0], xs[1:4], op), f"fold phase {phase}")
    assert out.guards_intact(), out.guards_intact()
    comb, swaps = STATIC_PROGS[8][1], [0, 1, 0, 0, 1, 0, 0]
    out.reset()
    assert ca.reduce_tree(out.ptr, [g.ptr for g in ins], comb, swaps, n, F16, code[op], gu.stream()) == 0
    gu.sync()
    _same(out.read(np.uint16), f16_ref.tree_ref(xs, comb, swaps, op), f"tree phase {phase}")
    assert out.guards_intact(), out.guards_intact()
    for g, s in zip(ins, snaps):
        assert g.unchanged_since(s), g.unchanged_since(s)


# ---- collectives on a local group ----------------------------------------------------------------------------------

BLOCK = 1029  # elements per rank block
GEOMETRIES = [(8, 4, 4), (8, 2, 2), (6, 4, 6), (4, 4, 4), (2, 2, 1)]
SCHEDULES = {"flat": ca.SCHEDULE_FLAT, "flat_1shot": ca.SCHEDULE_FLAT_1SHOT, "reference": ca.SCHEDULE_REFERENCE,
             "exact": ca.SCHEDULE_EXACT, "balanced": ca.SCHEDULE_BALANCED}
MODE = {"ar": ca.MODE_ALLREDUCE, "rs": ca.MODE_REDUCE_SCATTER}


def _balanced_valid(mode, n, k, b):
    hdr = ca.parse_plan(ca.describe_plan(MODE[mode], n, 0, k, b, BLOCK * n if mode == "ar" else BLOCK, 1,
                                         ca.SCHEDULE_BALANCED))["header"]
    return hdr["error"] == 0 and hdr["balanced"] == 1


def _run_group(gu, g, mode, sends, k, b, op_code, inplace=False):
    n = len(sends)
    count = sends[0].size // n if mode == "rs" else sends[0].size
    d_send = [gu.to_dev(s) for s in sends]
    if inplace:
        d_recv, d_sendp = d_send, [ca.IN_PLACE] * n
    else:
        d_recv, d_sendp = [gu.empty_dev(2 * count).fill_(0xA5) for _ in range(n)], d_send
    fn = g.all_reduce_radix_batch if mode == "ar" else g.reduce_scatter_radix_batch
    rc = fn(d_sendp, d_recv, count, F16, op_code, k, b)
    assert rc == 0, f"rc={rc}"
    return [gu.from_dev(t, np.uint16, count) for t in d_recv]


def _widen(bits, npdt):
    return bits.view(np.float16).astype(npdt)


def _narrow(a):
    return a.astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("n,k,b", GEOMETRIES)
def test_local_group_collectives(gu, code, groups, n, k, b):
    """Allreduce and reduce-scatter under FLAT, FLAT_1SHOT, REFERENCE, EXACT and (where the plan balances) BALANCED,
    pipeline depths 0 and 3, one allreduce in place.  Three references per case:
      SUM on U[-1, 1) against the SCHEDULE_REFERENCE plan under the plan evaluator (tests/f16_ref.py), bit-exact;
      SUM on integers in [-16, 16], every partial sum exact, against the oracle's int32 result converted to half --
        independent of plan_sim;
      MAX on finite nonzero halves against the oracle's float MAX of the widened inputs, narrowed."""
    g = groups(n)
    try:
        for mode in ("ar", "rs"):
            in_n = BLOCK * n  # ar: count = n * BLOCK; rs: recvcount = BLOCK, send = n * BLOCK
            fo = po.allreduce_radix_batch if mode == "ar" else po.reduce_scatter_radix_batch
            uni = [f16_ref.uniform(in_n, 5, r) for r in range(n)]
            want_uni = f16_ref.expected(MODE[mode], uni, k, b, "sum")
            ints = [f16_ref.small_ints(in_n, 6, r) for r in range(n)]
            want_int = [_narrow(w) for w in fo([v for _, v in ints], k, b, "i32", "sum")]
            fin = [f16_ref.finite_nonzero(in_n, 7, r) for r in range(n)]
            want_max = [_narrow(w) for w in fo([_widen(x, np.float32) for x in fin], k, b, "f32", "max")]
            first = True
            for name, sch in SCHEDULES.items():
                if name == "balanced" and not _balanced_valid(mode, n, k, b):
                    continue
                g.set_schedule(sch)
                for slices in (0, 3):
                    g.set_slices(slices)
                    what = f"{mode} n={n} k={k} b={b} {name} slices={slices}"
                    inplace = mode == "ar" and name == "flat" and slices == 3
                    got = _run_group(gu, g, mode, uni, k, b, code["sum"], inplace)
                    for r in range(n):
                        _same(got[r], want_uni[r], f"{what} SUM U[-1,1) rank {r}")
                    got = _run_group(gu, g, mode, [x for x, _ in ints], k, b, code["sum"])
                    for r in range(n):
                        _same(got[r], want_int[r], f"{what} SUM integers rank {r}")
                    got = _run_group(gu, g, mode, fin, k, b, code["max"])
                    for r in range(n):
                        _same(got[r], want_max[r], f"{what} MAX rank {r}")
                    if first and n == 8 and name == "flat" and mode == "ar":
                        first = False
                        ops.stats(reset=True)
                        _run_group(gu, g, mode, uni, k, b, code["sum"])
                        folds, tree_calls, trees = ops.stats()
                        assert tree_calls > 0 and trees >= tree_calls and folds == 0, ops.stats()
    finally:
        g.set_schedule(ca.SCHEDULE_FLAT)
        g.set_slices(0)


@pytest.mark.parametrize("algo,n", [("ring", 8), ("rd", 6), ("rsag", 8)])
def test_mpich_baselines(gu, code, groups, algo, n):
    """Ring, recursive doubling (6 ranks: the fold and unfold of a non-power-of-two) and reduce-scatter-allgather
    with f16 SUM, the ops being commutative: against the baseline's own plan under the plan evaluator."""
    mode = {"ring": ca.MODE_MPICH_RING, "rd": ca.MODE_MPICH_RD, "rsag": ca.MODE_MPICH_RSAG}[algo]
    count = BLOCK * n + 3
    sends = [f16_ref.uniform(count, 8, r) for r in range(n)]
    want = f16_ref.expected(mode, sends, 2, 0, "sum", schedule=ca.SCHEDULE_FLAT)
    d_send = [gu.to_dev(s) for s in sends]
    d_recv = [gu.empty_dev(2 * count).fill_(0xA5) for _ in range(n)]
    assert groups(n).allreduce_mpich(mode, d_send, d_recv, count, F16, code["sum"]) == 0
    for r in range(n):
        _same(gu.from_dev(d_recv[r], np.uint16, count), want[r], f"{algo} rank {r}")


# ---- refusals --------------------------------------------------------------------------------------------------------

def test_other_dtypes_are_refused(gu, code):
    """float16_op(SUM) with FLOAT32, and with derived types (of 2 and of 6 bytes), in a fold and in a tree:
    ERR_UNSUPPORTED, nothing enqueued, the output untouched."""
    n = 1024
    derived = [ca.type_contiguous(1, ca.UINT16), ca.type_contiguous(3, ca.UINT16)]
    try:
        for dt in [ca.FLOAT32] + derived:
            es = ca.type_size(dt)
            src = [gu.to_dev(np.full(n * es, 0x3C, np.uint8)) for _ in range(4)]
            out = gu.empty_dev(n * es).fill_(0xA5)
            assert ca.reduce_multi(out, src[0], src[1:2], n, dt, code["sum"], gu.stream()) == ca.ERR_UNSUPPORTED
            assert ca.reduce_tree(out, src, [0, 1, 0, 2], [0, 0, 0], n, dt, code["sum"],
                                  gu.stream()) == ca.ERR_UNSUPPORTED
            gu.sync()
            assert bool((out == 0xA5).all()), f"dtype {dt}: the output was written"
            assert bool((src[0] == 0x3C).all())
    finally:
        for t in derived:
            assert ca.type_free(t) == 0
