"""The OCP FP8 ops and casts of libchiara_fp8.so (include/chiara_fp8.h, chiara_amd/fp8.py) on the device, bit for bit
against tests/fp8_ref.py: the whole operand domain of every op on both paths, every path of the fold and tree kernels
the public header compiles for a 1-byte element, what a call touches besides its result, the collectives on a local
group under every schedule, one MPICH baseline, the casts and the refusals.  The module's teardown releases the ops."""
import functools

import numpy as np
import pytest

import chiara_amd as ca
import fp8_ref
import pyoracle as po
from chiara_amd import fp8
from footprint_util import Guarded
from streaming_cases import STATIC_PROGS, _nonzero_swaps, batch_programs
from tree_util import random_program

pytestmark = pytest.mark.gpu

F8 = fp8.F8_DTYPE
COMBOS = fp8_ref.COMBOS  # (format name, op name, policy name): the 12 ops
# the ops whose shapes are swept: SUM of each policy plus MAX, in both formats
SHAPE_COMBOS = [(f, op, p) for f, op, p in COMBOS if op == "sum" or op == "max"]


def _id(c):
    return "-".join(c)


def _ref(c):
    return fp8_ref.Ref(fp8_ref.FORMATS[c[0]], c[1], fp8_ref.POLICIES[c[2]])


@pytest.fixture(scope="module")
def gu():
    import gpu_util

    return gpu_util


@pytest.fixture(scope="module", autouse=True)
def code():
    """(format, op, policy) names -> op code; released when the module is done."""
    codes = {c: fp8.fp8_op(fp8_ref.FORMATS[c[0]], fp8_ref.KIND[c[1]], fp8_ref.POLICIES[c[2]]) for c in COMBOS}
    assert len(set(codes.values())) == 12
    yield codes
    assert fp8.release() == 0


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
        ops_ = f"in={int(x[i]):#04x} inout={int(y[i]):#04x} " if x is not None else ""
        rows.append(f"[{i}] {ops_}got={int(got[i]):#x} want={int(want[i]):#x}")
    return f"{bad.size} of {got.size} elements differ: " + "; ".join(rows)


def _same(got, want, what, x=None, y=None):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), f"{what}: {_report(got, want, x, y)}"


def _data(c, n, seed, rank):
    """Operands on which the op's operand order and association show: half TIES-like data (+-0, NaN codes, the largest
    magnitudes), half U[-1, 1)."""
    fmt, h = fp8_ref.FORMATS[c[0]], n // 2
    return np.concatenate([fp8_ref.ties(fmt, h, seed, rank), fp8_ref.uniform(fmt, n - h, seed, rank)])


class Dev:
    """nbytes at `off` bytes into a 16-byte aligned device allocation."""

    def __init__(self, gu, nbytes, off=0, host=None):
        self.gu, self.n, self.off = gu, nbytes, off
        self.t = gu.empty_dev(nbytes + 32)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + off
        if host is not None:
            self.load(host)

    def load(self, host):
        self.t[self.off:self.off + self.n] = self.gu.to_dev(host)
        return self

    def fill(self, byte):
        self.t.fill_(byte)
        return self

    def read(self, npdt=np.uint8):
        return self.t[self.off:self.off + self.n].cpu().numpy().view(npdt)


# ---- the operand domain ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", COMBOS, ids=_id)
def test_operand_domain(gu, code, c):
    """All 65 536 (inout, in) pairs -- eight whole 8 KiB chunks (2 vectors x 256 lanes) of the vector path, where SUM
    and PROD run their packed combine -- both operand orders, with every
    buffer 16-B aligned and again with every buffer one byte into its allocation (the element-wise path): bit for bit.
    This is what decides what gfx950's conversions do at the subnormal boundary, on NaN codes and on signed zeros, and
    whether MAX / MIN move the chosen operand's byte untouched."""
    ref = _ref(c)
    acc = np.tile(np.arange(256, dtype=np.uint8), 256)
    inp = np.repeat(np.arange(256, dtype=np.uint8), 256)
    n = acc.size
    for off in (0, 1):
        d_acc, d_in = Dev(gu, n, off, acc), Dev(gu, n, off, inp)
        for rf in (0, 1):
            out = Dev(gu, n, off).fill(0xA5)
            assert ca.reduce_multi_ex(out.ptr, d_acc.ptr, [d_in.ptr], n, F8, code[c], rf, gu.stream()) == 0
            gu.sync()
            got = out.read()
            x, y = (acc, inp) if rf else (inp, acc)  # running first: acc o in = f(in = acc, inout = in)
            want = ref.combine(x, y)
            print(f"operand domain {_id(c)} offset={off} running_first={rf}: "
                  f"{int(np.count_nonzero(got != want))} of {n} elements differ")
            _same(got, want, f"{_id(c)} offset={off} running_first={rf}", x, y)


# ---- fold shapes ---------------------------------------------------------------------------------------------------

FOLD_N = 16 * (2 * 1024 + 300) + 5  # whole chunks of 2 vectors x 256 lanes, 300 grid-stride vectors, a tail of 5
FOLD_M = (1, 2, 3, 8, 16, 17)       # 17: two launches past kMaxIns
# bytes into the allocation of (acc, every in, out): all aligned; all one byte in (element-wise); only out shifted
LAYOUTS = {"aligned": (0, 0, 0), "all one byte in": (1, 1, 1), "out one byte in": (0, 0, 1)}


@functools.lru_cache(maxsize=None)
def _fold_operands(c):
    xs = [_data(c, FOLD_N, 77, r) for r in range(18)]
    for x in xs:
        x.flags.writeable = False
    return xs


@pytest.mark.parametrize("c", SHAPE_COMBOS, ids=_id)
def test_fold_shapes(gu, code, c):
    ref, xs = _ref(c), _fold_operands(c)
    want = {(m, rf): ref.fold_ref(xs[0], xs[1:1 + m], bool(rf)) for m in FOLD_M for rf in (0, 1)}
    for layout, (o_acc, o_in, o_out) in LAYOUTS.items():
        d = [Dev(gu, FOLD_N, o_acc if j == 0 else o_in, x) for j, x in enumerate(xs)]
        work = Dev(gu, FOLD_N, o_out)
        for m in FOLD_M:
            ins = [b.ptr for b in d[1:1 + m]]
            for rf in (0, 1):
                for inplace in (False, True):
                    if inplace:  # out == acc: a copy of the accumulator at the output's place
                        work.fill(0xA5).load(xs[0])
                        acc = work.ptr
                    else:
                        work.fill(0xA5)
                        acc = d[0].ptr
                    rc = ca.reduce_multi_ex(work.ptr, acc, ins, FOLD_N, F8, code[c], rf, gu.stream())
                    assert rc == 0
                    gu.sync()
                    _same(work.read(), want[m, rf], f"{_id(c)} {layout} m={m} running_first={rf} inplace={inplace}")


# ---- tree shapes ---------------------------------------------------------------------------------------------------

TREE_N = 16 * (3 * 256 + 70) + 5  # whole and partial trips at U = 4, 2 and 1 (256 / 128 / 64 vectors), a tail of 5


@functools.lru_cache(maxsize=None)
def _tree_operands(c):
    xs = [_data(c, TREE_N, 91, r) for r in range(9)]
    for x in xs:
        x.flags.writeable = False
    return xs


def _tree_cases():
    """(comb, swaps, what): every static program unswapped and swapped, one non-static program per leaf count."""
    rng = np.random.default_rng(1608)
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


@pytest.mark.parametrize("c", SHAPE_COMBOS, ids=_id)
def test_tree_shapes(gu, code, c):
    """Every static program of the library's streaming trees, unswapped and with a nonzero swap word, and a random
    non-static program per leaf count 3..8, each in one pass (one tree-launcher call, no fold call); the root over
    leaf 0 and over the last leaf; a tree with a misaligned leaf, and one with a misaligned root, element-wise."""
    ref, xs = _ref(c), _tree_operands(c)
    d = [Dev(gu, TREE_N, 0, x) for x in xs]
    out = Dev(gu, TREE_N)

    def run(comb, swaps, leaves, dst, what):
        fp8.stats(reset=True)
        rc = ca.reduce_tree(dst.ptr, [b.ptr for b in leaves], comb, swaps, TREE_N, F8, code[c], gu.stream())
        assert rc == 0, what
        gu.sync()
        assert fp8.stats() == (0, 1, 1), (what, fp8.stats())
        _same(dst.read(), ref.tree_ref(xs[:len(comb)], comb, swaps), f"{_id(c)} {what} {comb} {swaps}")

    for comb, swaps, what in TREE_CASES:
        run(comb, swaps, d[:len(comb)], out.fill(0xA5), what)
    for nl, progs in STATIC_PROGS.items():
        comb, swaps = progs[-1], _nonzero_swaps(np.random.default_rng(nl), nl)
        for alias in (0, nl - 1):
            leaves = list(d[:nl])
            leaves[alias] = out.fill(0xA5).load(xs[alias])
            run(comb, swaps, leaves, out, f"out = leaf {alias}")
    comb, swaps = STATIC_PROGS[8][0], [1, 0, 0, 1, 0, 1, 0]
    shifted_leaf = Dev(gu, TREE_N, 1, xs[3])
    run(comb, swaps, d[:3] + [shifted_leaf] + d[4:8], out.fill(0xA5), "leaf 3 one byte in")
    run(comb, swaps, d[:8], Dev(gu, TREE_N, 1).fill(0xA5), "out one byte in")


def test_tree_batch_of_nine(gu, code):
    """chr_reduce_tree_batch of 9 eight-leaf trees (two launches: 8 segments and 1), E4M3 SATURATE SUM: one
    tree-launcher call."""
    c = ("e4m3", "sum", "sat")
    ref, xs = _ref(c), _tree_operands(c)
    d = [Dev(gu, TREE_N, 0, x) for x in xs]
    progs = batch_programs()
    outs = [Dev(gu, TREE_N).fill(0xA5) for _ in progs]
    rows = [[d[(t + j) % 9] for j in range(8)] for t in range(len(progs))]
    fp8.stats(reset=True)
    rc = ca.reduce_tree_batch([o.ptr for o in outs], [[b.ptr for b in row] for row in rows], [p[0] for p in progs],
                              [p[1] for p in progs], TREE_N, F8, code[c], gu.stream())
    assert rc == 0
    gu.sync()
    assert fp8.stats() == (0, 1, len(progs))
    for t, (comb, swaps) in enumerate(progs):
        want = ref.tree_ref([xs[(t + j) % 9] for j in range(8)], comb, swaps)
        _same(outs[t].read(), want, f"batch tree {t} {comb} {swaps}")


# ---- footprint -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("phase", [0, 2])
def test_footprint_fold_and_tree(gu, code, phase):
    """One fold (m = 3) and one 8-leaf tree, every operand between stamped guard bands, aligned (the vector paths)
    and two bytes in (element-wise): the result is right, the output's guards are intact and no input changed."""
    c, n = ("e5m2", "sum", "ieee"), FOLD_N
    ref, xs = _ref(c), _fold_operands(c)[:8]
    ins = [Guarded(n, phase, key=10 + j).load(x) for j, x in enumerate(xs)]
    snaps = [g.snapshot() for g in ins]
    out = Guarded(n, phase, key=99)
    assert ca.reduce_multi_ex(out.ptr, ins[0].ptr, [g.ptr for g in ins[1:4]], n, F8, code[c], 0, gu.stream()) == 0
    gu.sync()
    _same(out.read(np.uint8), ref.fold_ref(xs[0], xs[1:4]), f"fold phase {phase}")
    assert out.guards_intact(), out.guards_intact()
    comb, swaps = STATIC_PROGS[8][1], [0, 1, 0, 0, 1, 0, 0]
    out.reset()
    assert ca.reduce_tree(out.ptr, [g.ptr for g in ins], comb, swaps, n, F8, code[c], gu.stream()) == 0
    gu.sync()
    _same(out.read(np.uint8), ref.tree_ref(xs, comb, swaps), f"tree phase {phase}")
    assert out.guards_intact(), out.guards_intact()
    for g, s in zip(ins, snaps):
        assert g.unchanged_since(s), g.unchanged_since(s)


# ---- collectives on a local group ----------------------------------------------------------------------------------

BLOCK = 1029  # elements (bytes) per rank block: no chunk boundary is 16-B aligned
GEOMETRIES = [(8, 4, 4), (8, 2, 2), (6, 4, 6), (4, 4, 4), (2, 2, 1)]
SCHEDULES = {"flat": ca.SCHEDULE_FLAT, "flat_1shot": ca.SCHEDULE_FLAT_1SHOT, "reference": ca.SCHEDULE_REFERENCE,
             "exact": ca.SCHEDULE_EXACT, "balanced": ca.SCHEDULE_BALANCED}
MODE = {"ar": ca.MODE_ALLREDUCE, "rs": ca.MODE_REDUCE_SCATTER}
GROUP_FORMATS = [("e4m3", "sat"), ("e5m2", "ieee")]


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
        d_recv, d_sendp = [gu.empty_dev(count).fill_(0xA5) for _ in range(n)], d_send
    fn = g.all_reduce_radix_batch if mode == "ar" else g.reduce_scatter_radix_batch
    rc = fn(d_sendp, d_recv, count, F8, op_code, k, b)
    assert rc == 0, f"rc={rc}"
    return [gu.from_dev(t, np.uint8, count) for t in d_recv]


@pytest.mark.parametrize("fmt,policy", GROUP_FORMATS, ids=["e4m3-sat", "e5m2-ieee"])
@pytest.mark.parametrize("n,k,b", GEOMETRIES)
def test_local_group_collectives(gu, code, groups, n, k, b, fmt, policy):
    """Allreduce and reduce-scatter under FLAT, FLAT_1SHOT, REFERENCE, EXACT and (where the plan balances) BALANCED,
    pipeline depths 0 and 3, one allreduce in place.  Three references per case:
      SUM on U[-1, 1) against the SCHEDULE_REFERENCE plan under the plan evaluator (tests/fp8_ref.py), bit-exact;
      SUM on integers in {-1, 0, 1}, every partial sum exact, against the oracle's int32 result converted to the
        format -- independent of plan_sim;
      MAX on finite nonzero codes against the oracle's float MAX of the decoded inputs, re-encoded."""
    f = fp8_ref.FORMATS[fmt]
    c_sum, c_max = (fmt, "sum", policy), (fmt, "max", "ieee")
    ref = _ref(c_sum)
    g = groups(n)
    try:
        for mode in ("ar", "rs"):
            in_n = BLOCK * n  # ar: count = n * BLOCK; rs: recvcount = BLOCK, send = n * BLOCK
            fo = po.allreduce_radix_batch if mode == "ar" else po.reduce_scatter_radix_batch
            uni = [fp8_ref.uniform(f, in_n, 5, r) for r in range(n)]
            want_uni = ref.expected(MODE[mode], uni, k, b)
            ints = [fp8_ref.small_ints(f, in_n, 6, r) for r in range(n)]
            want_int = [fp8_ref.encode(f, fp8_ref.IEEE, w.astype(np.float64))
                        for w in fo([v for _, v in ints], k, b, "i32", "sum")]
            fin = [fp8_ref.finite_nonzero(f, in_n, 7, r) for r in range(n)]
            want_max = [fp8_ref.encode(f, fp8_ref.IEEE, w.astype(np.float64))
                        for w in fo([fp8_ref.decode(f, x).astype(np.float32) for x in fin], k, b, "f32", "max")]
            first = True
            for name, sch in SCHEDULES.items():
                if name == "balanced" and not _balanced_valid(mode, n, k, b):
                    continue
                g.set_schedule(sch)
                for slices in (0, 3):
                    g.set_slices(slices)
                    what = f"{fmt} {policy} {mode} n={n} k={k} b={b} {name} slices={slices}"
                    inplace = mode == "ar" and name == "flat" and slices == 3
                    got = _run_group(gu, g, mode, uni, k, b, code[c_sum], inplace)
                    for r in range(n):
                        _same(got[r], want_uni[r], f"{what} SUM U[-1,1) rank {r}")
                    got = _run_group(gu, g, mode, [x for x, _ in ints], k, b, code[c_sum])
                    for r in range(n):
                        _same(got[r], want_int[r], f"{what} SUM integers rank {r}")
                    got = _run_group(gu, g, mode, fin, k, b, code[c_max])
                    for r in range(n):
                        _same(got[r], want_max[r], f"{what} MAX rank {r}")
                    if first and n == 8 and name == "flat" and mode == "ar":
                        first = False
                        fp8.stats(reset=True)
                        _run_group(gu, g, mode, uni, k, b, code[c_sum])
                        folds, tree_calls, trees = fp8.stats()
                        assert tree_calls > 0 and trees >= tree_calls and folds == 0, fp8.stats()
    finally:
        g.set_schedule(ca.SCHEDULE_FLAT)
        g.set_slices(0)


def test_mpich_ring_baseline(gu, code, groups):
    """The ring allreduce of 8 ranks with E4M3 SATURATE SUM, the ops being commutative: against the baseline's own
    plan under the plan evaluator."""
    c, n = ("e4m3", "sum", "sat"), 8
    count = BLOCK * n + 3
    sends = [fp8_ref.uniform(fp8_ref.E4M3, count, 8, r) for r in range(n)]
    want = _ref(c).expected(ca.MODE_MPICH_RING, sends, 2, 0, schedule=ca.SCHEDULE_FLAT)
    d_send = [gu.to_dev(s) for s in sends]
    d_recv = [gu.empty_dev(count).fill_(0xA5) for _ in range(n)]
    assert groups(n).allreduce_mpich(ca.MODE_MPICH_RING, d_send, d_recv, count, F8, code[c]) == 0
    for r in range(n):
        _same(gu.from_dev(d_recv[r], np.uint8, count), want[r], f"ring rank {r}")


# ---- the casts -------------------------------------------------------------------------------------------------------

THIRD = float(np.float32(1) / np.float32(3))
WIDE = {"f32": (ca.FLOAT32, 4), "bf16": (ca.BFLOAT16, 2)}


def _cast_pair(gu, src_host, src_es, dst_nbytes, dst_es, shifted):
    """The source at 0 or one source element into its allocation, the destination between guard bands at phase 0 or
    one destination element."""
    src = Dev(gu, src_host.nbytes, src_es if shifted else 0, src_host)
    return src, src.t.clone(), Guarded(dst_nbytes, dst_es if shifted else 0, key=41)


def _quantize_and_check(gu, src_bits, src_f32, wide, scales, what):
    dt, es = WIDE[wide]
    n = src_bits.size
    for shifted in (False, True):
        src, snap, dst = _cast_pair(gu, src_bits, es, n, 1, shifted)
        for fmt, f in fp8_ref.FORMATS.items():
            for policy, o in fp8_ref.POLICIES.items():
                for scale in scales:
                    dst.reset()
                    assert fp8.quantize(dst.ptr, src.ptr, n, dt, f, scale, o, gu.stream()) == 0
                    gu.sync()
                    got, want = dst.read(np.uint8), fp8_ref.quantize_ref(f, o, src_f32, scale)
                    bad = np.flatnonzero(got != want)
                    rows = [f"[{i}] src={int(src_bits[i]):#x} got={int(got[i]):#04x} want={int(want[i]):#04x}" for i in bad[:8]]
                    assert bad.size == 0, f"{what} {fmt} {policy} scale={scale!r} shifted={shifted}: {bad.size} differ: {rows}"
                    assert dst.guards_intact(), dst.guards_intact()
        assert bool((src.t == snap).all()), f"{what}: the source changed"


def test_quantize_from_bf16(gu):
    """All 65 536 bf16 bit patterns (and 5 more elements, so that the aligned call has a tail), both formats, both
    policies, scales 1, 0.5, 3, f32(1/3), 2^-120 and 2^100."""
    bits = np.concatenate([np.arange(1 << 16, dtype=np.uint16), np.array([0x3F80, 0x7F80, 0xFFFF, 0x0001, 0x8000], np.uint16)])
    _quantize_and_check(gu, bits, fp8_ref.bf16_to_f32(bits), "bf16", (1.0, 0.5, 3.0, THIRD, 2.0 ** -120, 2.0 ** 100),
                        "quantize bf16")


def _f32_edge_inputs():
    """For every finite code of both formats its value, the two midpoints to its neighbours and the f32 values just
    above and below each midpoint; the same beyond max (the value an unbounded exponent would put there and the
    midpoint to it); f32 subnormals, +-0, +-inf and NaNs; 64 Ki random bit patterns."""
    vals = []
    for f in (fp8_ref.E4M3, fp8_ref.E5M2):
        mags = fp8_ref._MAGS[f].astype(np.float32)  # the finite magnitudes and the entry past max: all exact in f32
        mids = ((mags[:-1].astype(np.float64) + mags[1:].astype(np.float64)) / 2).astype(np.float32)  # exact
        edge = np.concatenate([mags, mids, np.nextafter(mids, np.float32(np.inf)), np.nextafter(mids, np.float32(0)),
                               np.nextafter(mags, np.float32(np.inf)), mags[-1:] * np.float32(1.5)])
        vals += [edge, -edge]
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000,
                        0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001,
                        0xFFFFFFFF, 0x7FA00000], dtype=np.uint32).view(np.float32)
    rng = np.random.default_rng(832)
    rand = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return np.concatenate(vals + [special, rand]).astype(np.float32)


def test_quantize_from_f32(gu):
    src = _f32_edge_inputs()
    _quantize_and_check(gu, src.view(np.uint32), src, "f32", (1.0, 3.0), "quantize f32")


DEQ_N = 16 * (1024 + 300) + 5


@pytest.mark.parametrize("wide", sorted(WIDE))
def test_dequantize(gu, wide):
    """All 256 codes tiled to n = 16 * (1024 + 300) + 5, to float32 and to bf16, scales 1, 2^-7, 3, f32(1/3), 2^100
    and 2^-140 (an f32 subnormal: products underflow), aligned and one element in."""
    dt, es = WIDE[wide]
    codes = np.resize(np.arange(256, dtype=np.uint8), DEQ_N)
    npdt = np.uint32 if wide == "f32" else np.uint16
    for shifted in (False, True):
        src, snap, dst = _cast_pair(gu, codes, 1, DEQ_N * es, es, shifted)
        for fmt, f in fp8_ref.FORMATS.items():
            for scale in (1.0, 2.0 ** -7, 3.0, THIRD, 2.0 ** 100, 2.0 ** -140):
                dst.reset()
                assert fp8.dequantize(dst.ptr, src.ptr, DEQ_N, dt, f, scale, gu.stream()) == 0
                gu.sync()
                got, want = dst.read(npdt), fp8_ref.dequantize_ref(f, codes, scale, bf16=wide == "bf16")
                bad = np.flatnonzero(got != want)
                rows = [f"[{i}] code={int(codes[i]):#04x} got={int(got[i]):#x} want={int(want[i]):#x}" for i in bad[:8]]
                assert bad.size == 0, f"dequantize {wide} {fmt} scale={scale!r} shifted={shifted}: {bad.size} differ: {rows}"
                assert dst.guards_intact(), dst.guards_intact()
        assert bool((src.t == snap).all()), "the source changed"


def test_cast_refusals(gu):
    """NULL pointers, other dtypes, values outside the enums: the status code and nothing written; n = 0: success and
    nothing written."""
    n = 1024
    src = gu.to_dev(np.full(n, 1.0, np.float32))
    cod = gu.to_dev(np.full(n, 0x38, np.uint8))
    q = gu.empty_dev(n).fill_(0xA5)
    w = gu.empty_dev(4 * n).fill_(0xA5)
    s = gu.stream()
    assert fp8.quantize(None, src, n, ca.FLOAT32, fp8.E4M3, 1.0, fp8.IEEE, s) == ca.ERR_INVALID_ARG
    assert fp8.quantize(q, None, n, ca.FLOAT32, fp8.E4M3, 1.0, fp8.IEEE, s) == ca.ERR_INVALID_ARG
    assert fp8.dequantize(None, cod, n, ca.FLOAT32, fp8.E4M3, 1.0, s) == ca.ERR_INVALID_ARG
    assert fp8.dequantize(w, None, n, ca.FLOAT32, fp8.E4M3, 1.0, s) == ca.ERR_INVALID_ARG
    for dt in (ca.FLOAT64, ca.UINT16, ca.UINT8, ca.INT32):
        assert fp8.quantize(q, src, n, dt, fp8.E4M3, 1.0, fp8.IEEE, s) == ca.ERR_UNSUPPORTED
        assert fp8.dequantize(w, cod, n, dt, fp8.E4M3, 1.0, s) == ca.ERR_UNSUPPORTED
    for fmt in (2, -1):
        assert fp8.quantize(q, src, n, ca.FLOAT32, fmt, 1.0, fp8.IEEE, s) == ca.ERR_UNSUPPORTED
        assert fp8.dequantize(w, cod, n, ca.FLOAT32, fmt, 1.0, s) == ca.ERR_UNSUPPORTED
    for o in (2, -1):
        assert fp8.quantize(q, src, n, ca.FLOAT32, fp8.E5M2, 1.0, o, s) == ca.ERR_UNSUPPORTED
    assert fp8.quantize(q, src, 0, ca.FLOAT32, fp8.E4M3, 1.0, fp8.IEEE, s) == 0
    assert fp8.dequantize(w, cod, 0, ca.BFLOAT16, fp8.E5M2, 1.0, s) == 0
    gu.sync()
    assert bool((q == 0xA5).all()) and bool((w == 0xA5).all())


# ---- refusals --------------------------------------------------------------------------------------------------------

def test_other_dtypes_are_refused(gu, code):
    """fp8_op(E4M3, SUM) with FLOAT32, UINT16 and derived types (of 1 and of 3 bytes), in a fold and in a tree:
    ERR_UNSUPPORTED, nothing enqueued, output and inputs untouched."""
    n, c = 1024, ("e4m3", "sum", "ieee")
    derived = [ca.type_contiguous(1, ca.UINT8), ca.type_contiguous(3, ca.UINT8)]
    try:
        for dt in [ca.FLOAT32, ca.UINT16] + derived:
            es = ca.type_size(dt)
            src = [gu.to_dev(np.full(n * es, 0x38, np.uint8)) for _ in range(4)]
            out = gu.empty_dev(n * es).fill_(0xA5)
            assert ca.reduce_multi(out, src[0], src[1:2], n, dt, code[c], gu.stream()) == ca.ERR_UNSUPPORTED
            assert ca.reduce_tree(out, src, [0, 1, 0, 2], [0, 0, 0], n, dt, code[c], gu.stream()) == ca.ERR_UNSUPPORTED
            gu.sync()
            assert bool((out == 0xA5).all()), f"dtype {dt}: the output was written"
            for t in src:
                assert bool((t == 0x38).all())
    finally:
        for t in derived:
            assert ca.type_free(t) == 0
