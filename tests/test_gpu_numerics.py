"""The struct ops of libchiara_numerics.so (include/chiara_numerics.h, chiara_amd/numerics.py) on the device, bit for
bit against tests/numerics_ref.py: the operand domain of both functors on both bases, every path of the fold and tree
kernels the public header compiles for 8-, 16-, 12- and 24-byte elements, the library's own pack / unpack kernels, what
each call touches besides its result, the collectives on a local group, the MPICH baselines and the refusals.  Every
comparison is on the bits.  The module's teardown releases the ops and types."""
import functools
import itertools

import numpy as np
import pytest

import chiara_amd as ca
import numerics_ref as nr
import struct_ref as sr
from chiara_amd import numerics as num
from footprint_util import Guarded
from streaming_cases import STATIC_PROGS, _nonzero_swaps, batch_programs
from tree_util import random_program

pytestmark = pytest.mark.gpu

BASE = {np.float32: ca.FLOAT32, np.float64: ca.FLOAT64}
KINDS = [("sum2", np.float32), ("sum2", np.float64), ("moments", np.float32), ("moments", np.float64)]
IDS = [f"{f}-{np.dtype(T).name}" for f, T in KINDS]


@pytest.fixture(scope="module")
def gu():
    import gpu_util

    return gpu_util


@pytest.fixture(scope="module", autouse=True)
def env():
    """(functor, base) -> (op code, type code); released when the module is done."""
    codes = {}
    for f, T in KINDS:
        op = num.sum2_op() if f == "sum2" else num.moments_op()
        t = (num.sum2_type if f == "sum2" else num.moments_type)(BASE[T])
        codes[(f, T)] = (op, t)
    yield codes
    assert num.release() == 0


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


def _fk(f):
    return nr.FUNCTORS[f]


def _report(got, want, k, x=None, y=None):
    """How many elements differ and the first eight of them, operands included where given."""
    g, w = nr.bits(got).reshape(-1, k), nr.bits(want).reshape(-1, k)
    bad = np.flatnonzero((g != w).any(axis=1))
    rows = []
    for i in bad[:8]:
        ops_ = ""
        if x is not None:
            ops_ = (f"in={[hex(int(v)) for v in nr.bits(x).reshape(-1, k)[i]]} "
                    f"inout={[hex(int(v)) for v in nr.bits(y).reshape(-1, k)[i]]} ")
        rows.append(f"[{i}] {ops_}got={[hex(int(v)) for v in g[i]]} want={[hex(int(v)) for v in w[i]]}")
    return f"{bad.size} of {g.shape[0]} elements differ: " + "; ".join(rows)


def _same(got, want, k, what, x=None, y=None):
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(nr.bits(got), nr.bits(want)), f"{what}: {_report(got, want, k, x, y)}"


def _data(f, T, n, seed, rank):
    """n elements (flat base array) on which association and operand order show: one element in eight from the
    operand-domain partners (zeros, subnormals, infinities, NaNs, random bits), the rest plausible values --
    normalised pairs of well-scaled sums; records of small counts, means near 1000 and small M2."""
    rng = np.random.default_rng([seed, rank, 2 if f == "sum2" else 3, np.dtype(T).itemsize])
    if f == "sum2":
        part = nr.sum2_partners(T)
        hi = (rng.uniform(-1, 1, n) * np.exp2(rng.integers(-8, 9, n))).astype(T)
        mag = np.abs(hi)
        ulp = (mag - np.nextafter(mag, T(0))).astype(np.float64)
        rows = np.stack([hi, (rng.uniform(-1, 1, n) * 0.5 * ulp).astype(T)], axis=1)
    else:
        part = nr.moments_partners(T)
        cnt = rng.integers(0, 6, n)
        mean = np.where(cnt > 0, rng.standard_normal(n) * 3 + 1000, 0.0)
        m2 = np.where(cnt > 1, rng.uniform(0, 10, n) * cnt, 0.0)
        rows = np.stack([cnt.astype(T), mean.astype(T), m2.astype(T)], axis=1)
    special = rng.integers(0, 8, n) == 0
    rows[special] = part[rng.integers(0, part.shape[0], int(special.sum()))]
    return np.ascontiguousarray(rows).reshape(-1)


class Dev:
    """nbytes at `off` bytes into a 16-byte aligned device allocation."""

    def __init__(self, gu, nbytes, off=0, host=None):
        self.gu, self.nbytes, self.off = gu, nbytes, off
        self.t = gu.empty_dev(nbytes + 64)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + off
        if host is not None:
            self.load(host)

    def load(self, host):
        self.t[self.off:self.off + self.nbytes] = self.gu.to_dev(host)
        return self

    def fill(self, byte):
        self.t.fill_(byte)
        return self

    def read(self, npdt):
        return self.t[self.off:self.off + self.nbytes].cpu().numpy().view(npdt)


# ---- the operand domain ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f,T", KINDS, ids=IDS)
def test_operand_domain(gu, env, f, T):
    """Every ordered pair of the partner list (sum2: 2 020^2; moments: 1 456^2) in one fold per operand order, bit for
    bit.  This is what decides whether the device's add, multiply and divide round as IEEE under the package's flags,
    subnormal quotients included, and whether the compiler kept every operation of two_sum as written."""
    fn, k = _fk(f)
    part = nr.sum2_partners(T) if f == "sum2" else nr.moments_partners(T)
    acc, inp = nr.cross(part)
    n = acc.shape[0]
    assert n == (2020 ** 2 if f == "sum2" else 1456 ** 2)
    op, dt = env[(f, T)]
    d_acc, d_in = gu.to_dev(acc), gu.to_dev(inp)
    nbytes = acc.nbytes
    for rf in (0, 1):
        out = gu.empty_dev(nbytes).fill_(0xA5)
        assert ca.reduce_multi_ex(out, d_acc, [d_in], n, dt, op, rf, gu.stream()) == 0
        gu.sync()
        got = gu.from_dev(out, T, n * k)
        x, y = (acc, inp) if rf else (inp, acc)  # running first: acc o in = f(in = acc, inout = in)
        want = fn(x, y)
        differ = int(np.count_nonzero((nr.bits(got).reshape(-1, k) != nr.bits(want)).any(axis=1)))
        print(f"operand domain {f} {np.dtype(T).name} running_first={rf}: {differ} of {n} elements differ")
        _same(got, want, k, f"{f} {np.dtype(T).name} running_first={rf}", x, y)


# ---- fold shapes ---------------------------------------------------------------------------------------------------

def _fold_n(es):
    """8-byte pairs: two whole fold chunks (4 vectors x 256 lanes), 300 further vectors and a tail shorter than a
    vector; 16-byte pairs: the same in vectors of one element; the 12- and 24-byte records run element-wise: whole
    waves plus a partial one."""
    return {8: 2 * (2 * 1024 + 300) + 1, 16: 2 * 1024 + 300, 12: 19 * 64 + 37, 24: 19 * 64 + 37}[es]


FOLD_M = (1, 3, 8, 17)  # 17: two launches past kMaxIns


@functools.lru_cache(maxsize=None)
def _fold_operands(f, T):
    k = _fk(f)[1]
    xs = [_data(f, T, _fold_n(k * np.dtype(T).itemsize), 77, r) for r in range(18)]
    for x in xs:
        x.flags.writeable = False
    return xs


@pytest.mark.parametrize("f,T", KINDS, ids=IDS)
def test_fold_shapes(gu, env, f, T):
    """m = 1, 3, 8, 17 in both operand orders; every operand aligned, every operand one element in, only `out` one
    element in, and `out` aliasing `acc`."""
    fn, k = _fk(f)
    es = k * np.dtype(T).itemsize
    n = _fold_n(es)
    xs = _fold_operands(f, T)
    op, dt = env[(f, T)]
    layouts = {"aligned": (0, 0, 0), "all one element in": (es, es, es), "out one element in": (0, 0, es)}
    for layout, (o_acc, o_in, o_out) in layouts.items():
        d = [Dev(gu, n * es, o_acc if j == 0 else o_in, x) for j, x in enumerate(xs)]
        work = Dev(gu, n * es, o_out)
        for m in FOLD_M:
            ins = [b.ptr for b in d[1:1 + m]]
            for rf in (0, 1):
                want = sr.fold_ref(xs[0], xs[1:1 + m], k, fn, bool(rf))
                for inplace in (False, True):
                    if inplace:  # out == acc: a copy of the accumulator at the output's place
                        work.fill(0xA5).load(xs[0])
                        acc = work.ptr
                    else:
                        work.fill(0xA5)
                        acc = d[0].ptr
                    assert ca.reduce_multi_ex(work.ptr, acc, ins, n, dt, op, rf, gu.stream()) == 0
                    gu.sync()
                    _same(work.read(T), want, k, f"{f} {layout} m={m} running_first={rf} inplace={inplace}")


# ---- tree shapes ---------------------------------------------------------------------------------------------------

def _tree_n(es):
    """Whole and partial trips at U = 4, 2 and 1 (256 / 128 / 64 vectors) and, for 8-byte pairs, a tail element;
    the records: whole one-wave workgroups plus a partial one."""
    return {8: 2 * (3 * 256 + 70) + 1, 16: 3 * 256 + 70, 12: 5 * 64 + 37, 24: 5 * 64 + 37}[es]


@functools.lru_cache(maxsize=None)
def _tree_operands(f, T):
    k = _fk(f)[1]
    xs = [_data(f, T, _tree_n(k * np.dtype(T).itemsize), 91, r) for r in range(9)]
    for x in xs:
        x.flags.writeable = False
    return xs


def _tree_cases():
    """(comb, swaps, what): every static program of the library's streaming trees with a nonzero swap word, and one
    random program per leaf count 2..8, its swap bits nonzero too."""
    rng = np.random.default_rng(1610)
    out = []
    for nl, progs in STATIC_PROGS.items():
        for comb in progs:
            out.append((comb, _nonzero_swaps(rng, nl), "static"))
    for nl in range(2, 9):
        comb, _ = random_program(rng, nl)
        out.append((comb, _nonzero_swaps(rng, nl), "random"))
    return out


TREE_CASES = _tree_cases()


@pytest.mark.parametrize("f,T", KINDS, ids=IDS)
def test_tree_shapes(gu, env, f, T):
    """Each program in one pass (one tree-launcher call, no fold call), aligned and with every operand one element in;
    the root over leaf 0 and over the last leaf."""
    fn, k = _fk(f)
    es = k * np.dtype(T).itemsize
    n = _tree_n(es)
    xs = _tree_operands(f, T)
    op, dt = env[(f, T)]

    def run(comb, swaps, leaves, dst, what):
        num.stats(reset=True)
        rc = ca.reduce_tree(dst.ptr, [b.ptr for b in leaves], comb, swaps, n, dt, op, gu.stream())
        assert rc == 0, what
        gu.sync()
        assert num.stats() == (0, 1, 1), (what, num.stats())
        _same(dst.read(T), sr.tree_ref(xs[:len(comb)], comb, swaps, k, fn), k, f"{f} {what} {comb} {swaps}")

    for off in (0, es):
        d = [Dev(gu, n * es, off, x) for x in xs]
        out = Dev(gu, n * es, off)
        for comb, swaps, what in TREE_CASES:
            run(comb, swaps, d[:len(comb)], out.fill(0xA5), f"{what} offset {off}")
        for nl, progs in STATIC_PROGS.items():
            comb, swaps = progs[-1], _nonzero_swaps(np.random.default_rng(nl), nl)
            for alias in (0, nl - 1):
                leaves = list(d[:nl])
                leaves[alias] = out.fill(0xA5).load(xs[alias])
                run(comb, swaps, leaves, out, f"out = leaf {alias} offset {off}")


def test_tree_batch_of_nine(gu, env):
    """chr_reduce_tree_batch of 9 eight-leaf trees (two launches: 8 segments and 1), sum2 f32: one tree-launcher
    call."""
    f, T = "sum2", np.float32
    fn, k = _fk(f)
    n = _tree_n(8)
    xs = _tree_operands(f, T)
    op, dt = env[(f, T)]
    d = [Dev(gu, n * 8, 0, x) for x in xs]
    progs = batch_programs()
    outs = [Dev(gu, n * 8).fill(0xA5) for _ in progs]
    rows = [[d[(t + j) % 9] for j in range(8)] for t in range(len(progs))]
    num.stats(reset=True)
    rc = ca.reduce_tree_batch([o.ptr for o in outs], [[b.ptr for b in row] for row in rows], [p[0] for p in progs],
                              [p[1] for p in progs], n, dt, op, gu.stream())
    assert rc == 0
    gu.sync()
    assert num.stats() == (0, 1, len(progs))
    for t, (comb, swaps) in enumerate(progs):
        want = sr.tree_ref([xs[(t + j) % 9] for j in range(8)], comb, swaps, k, fn)
        _same(outs[t].read(T), want, k, f"batch tree {t} {comb} {swaps}")


def test_moments_f64_tree_is_one_pass(gu, env):
    """An 8-leaf tree of 24-byte records takes the header's element-wise one-pass kernel: one tree-launcher call, no
    fold call."""
    f, T = "moments", np.float64
    fn, k = _fk(f)
    n = 4099
    xs = [_data(f, T, n, 93, r) for r in range(8)]
    op, dt = env[(f, T)]
    d = [gu.to_dev(x) for x in xs]
    out = gu.empty_dev(n * 24).fill_(0xA5)
    comb, swaps = [0, 1, 1, 1, 0, 1, 1, 2], [0, 1, 0, 0, 1, 0, 1]
    num.stats(reset=True)
    assert ca.reduce_tree(out, d, comb, swaps, n, dt, op, gu.stream()) == 0
    gu.sync()
    assert num.stats() == (0, 1, 1), num.stats()
    _same(gu.from_dev(out, T, n * k), sr.tree_ref(xs, comb, swaps, k, fn), k, "moments f64 8-leaf tree")


# ---- footprint -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f,T", [("sum2", np.float32), ("moments", np.float64)], ids=["sum2-float32", "moments-float64"])
@pytest.mark.parametrize("phase_elems", [0, 1])
def test_footprint_fold_and_tree(gu, env, f, T, phase_elems):
    """One fold (m = 3) and one 8-leaf tree, every operand between stamped guard bands, aligned and one element in:
    the result is right, the output's guards are intact and no input changed."""
    fn, k = _fk(f)
    es = k * np.dtype(T).itemsize
    n = _fold_n(es)
    phase = phase_elems * es % 16
    xs = _fold_operands(f, T)[:8]
    op, dt = env[(f, T)]
    ins = [Guarded(n * es, phase, key=10 + j).load(x) for j, x in enumerate(xs)]
    snaps = [g.snapshot() for g in ins]
    out = Guarded(n * es, phase, key=99)
    assert ca.reduce_multi_ex(out.ptr, ins[0].ptr, [g.ptr for g in ins[1:4]], n, dt, op, 0, gu.stream()) == 0
    gu.sync()
    _same(out.read(T), sr.fold_ref(xs[0], xs[1:4], k, fn, False), k, f"fold phase {phase}")
    assert out.guards_intact(), out.guards_intact()
    comb, swaps = STATIC_PROGS[8][1], [0, 1, 0, 0, 1, 0, 0]
    out.reset()
    assert ca.reduce_tree(out.ptr, [g.ptr for g in ins], comb, swaps, n, dt, op, gu.stream()) == 0
    gu.sync()
    _same(out.read(T), sr.tree_ref(xs, comb, swaps, k, fn), k, f"tree phase {phase}")
    assert out.guards_intact(), out.guards_intact()
    for g, s in zip(ins, snaps):
        assert g.unchanged_since(s), g.unchanged_since(s)


def _random_bits(T, n, seed):
    """Random bit patterns (NaNs of every payload among them) with a few -0 and +0."""
    rng = np.random.default_rng([seed, np.dtype(T).itemsize])
    nbits = 8 * np.dtype(T).itemsize
    v = rng.integers(0, 1 << nbits, n, dtype=np.uint64).astype(nr.UINT[np.dtype(T)]).view(T)
    v[::7] = T(-0.0)
    v[3::11] = T(0.0)
    return v


@pytest.mark.parametrize("T", nr.BASES)
@pytest.mark.parametrize("phase_elems", [0, 1])
def test_footprint_pack_and_unpack(gu, T, phase_elems):
    """Each of the four conversions writes exactly its n output elements: guards intact on every output, every input
    unchanged; moments_unpack with every subset of its outputs left out."""
    isz = np.dtype(T).itemsize
    n = 4 * 256 * 3 + 5
    v = _random_bits(T, n, 41)
    base = BASE[T]
    for k, pack, ref_pack in ((2, num.sum2_pack, nr.sum2_pack), (3, num.moments_pack, nr.moments_pack)):
        src = Guarded(n * isz, phase_elems * isz % 16, key=1).load(v)
        snap = src.snapshot()
        out = Guarded(n * isz * k, phase_elems * isz * k % 16, key=2)
        assert pack(out.ptr, src.ptr, n, base, gu.stream()) == 0
        gu.sync()
        _same(out.read(T), ref_pack(v), k, f"pack K={k}")
        assert out.guards_intact(), out.guards_intact()
        assert src.unchanged_since(snap), src.unchanged_since(snap)
    pairs = _random_bits(T, 2 * n, 42)
    src = Guarded(2 * n * isz, phase_elems * 2 * isz % 16, key=3).load(pairs)
    snap = src.snapshot()
    out = Guarded(n * isz, phase_elems * isz % 16, key=4)
    assert num.sum2_unpack(out.ptr, src.ptr, n, base, gu.stream()) == 0
    gu.sync()
    _same(out.read(T), pairs.reshape(-1, 2)[:, 0], 1, "sum2_unpack")
    assert out.guards_intact() and src.unchanged_since(snap)
    recs = _random_bits(T, 3 * n, 43)
    src = Guarded(3 * n * isz, phase_elems * 3 * isz % 16, key=5).load(recs)
    snap = src.snapshot()
    for keep in itertools.product((False, True), repeat=3):
        if not any(keep):
            continue
        outs = [Guarded(n * isz, phase_elems * isz % 16, key=6 + j) for j in range(3)]
        ptrs = [o.ptr if kp else None for o, kp in zip(outs, keep)]
        assert num.moments_unpack(*ptrs, src.ptr, n, base, gu.stream()) == 0
        gu.sync()
        for j, (o, kp) in enumerate(zip(outs, keep)):
            assert o.guards_intact(), (keep, j, o.guards_intact())
            if kp:
                _same(o.read(T), recs.reshape(-1, 3)[:, j], 1, f"moments_unpack {keep} output {j}")
        assert src.unchanged_since(snap), src.unchanged_since(snap)


# ---- round trips -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", nr.BASES)
def test_round_trips(gu, T):
    """unpack(pack(v)) == v bitwise on random bits, NaNs and -0 included: n = 0, 1, 5, one vector, 4 099; aligned, and
    with source and destination both one element past a 16-byte boundary."""
    isz = np.dtype(T).itemsize
    base = BASE[T]
    for n, off in itertools.product((0, 1, 5, 16 // isz, 4099), (0, 1)):
        v = _random_bits(T, n, 50 + n)
        src = Dev(gu, n * isz, off * isz, v)
        what = f"n={n} offset {off}"
        mid = Dev(gu, 2 * n * isz, off * 2 * isz % 16).fill(0xA5)
        back = Dev(gu, n * isz, off * isz).fill(0xA5)
        assert num.sum2_pack(mid.ptr, src.ptr, n, base, gu.stream()) == 0
        assert num.sum2_unpack(back.ptr, mid.ptr, n, base, gu.stream()) == 0
        gu.sync()
        _same(mid.read(T), nr.sum2_pack(v), 2, f"sum2_pack {what}")
        _same(back.read(T), v, 1, f"sum2 round trip {what}")
        mid = Dev(gu, 3 * n * isz, off * 3 * isz % 16).fill(0xA5)
        outs = [Dev(gu, n * isz, off * isz).fill(0xA5) for _ in range(3)]
        assert num.moments_pack(mid.ptr, src.ptr, n, base, gu.stream()) == 0
        assert num.moments_unpack(outs[0].ptr, outs[1].ptr, outs[2].ptr, mid.ptr, n, base, gu.stream()) == 0
        gu.sync()
        _same(mid.read(T), nr.moments_pack(v), 3, f"moments_pack {what}")
        _same(outs[0].read(T), np.ones(n, dtype=T), 1, f"moments count {what}")
        _same(outs[1].read(T), v, 1, f"moments round trip {what}")
        _same(outs[2].read(T), np.zeros(n, dtype=T), 1, f"moments M2 {what}")
        for b in [src, mid, back] + outs:  # nothing past the payload was written (the allocation's spare bytes)
            used = b.off + b.nbytes
            assert bool((b.t[used:] == (0 if b is src else 0xA5)).all()), f"{what}: bytes past the payload changed"


# ---- collectives on a local group ----------------------------------------------------------------------------------

BLOCK = 257
COLLECTIVE_KINDS = [("sum2", np.float32), ("moments", np.float64)]
SCHED = {"flat": ca.SCHEDULE_FLAT, "exact": ca.SCHEDULE_EXACT, "reference": ca.SCHEDULE_REFERENCE}


def _run_group(gu, g, mode, sends, T, k, b, op, dt, es):
    n = len(sends)
    elems = sends[0].nbytes // es
    count = elems // n if mode == "rs" else elems
    d_send = [gu.to_dev(s) for s in sends]
    d_recv = [gu.empty_dev(count * es).fill_(0xA5) for _ in range(n)]
    fn = g.all_reduce_radix_batch if mode == "ar" else g.reduce_scatter_radix_batch
    rc = fn(d_send, d_recv, count, dt, op, k, b)
    gu.sync()
    assert rc == 0, f"rc={rc}"
    return [gu.from_dev(t, T, count * es // np.dtype(T).itemsize) for t in d_recv]


@pytest.mark.parametrize("f,T", COLLECTIVE_KINDS, ids=["sum2-float32", "moments-float64"])
def test_local_group_collectives(gu, env, groups, f, T):
    """Allreduce at (8, 4, 4) flat with 1 and 3 slices, (6, 3, 2) exact and (4, 2, 2) reference, reduce-scatter at
    (8, 2, 8), n x 257 elements: every rank bit for bit against the same plan under struct_ref's interpreter."""
    fn, kk = _fk(f)
    es = kk * np.dtype(T).itemsize
    op, dt = env[(f, T)]
    cases = [("ar", 8, 4, 4, "flat", 1), ("ar", 8, 4, 4, "flat", 3), ("ar", 6, 3, 2, "exact", 1),
             ("ar", 4, 2, 2, "reference", 1), ("rs", 8, 2, 8, "flat", 1)]
    for mode, n, k, b, sched, slices in cases:
        g = groups(n)
        g.set_schedule(SCHED[sched])
        g.set_slices(slices)
        try:
            in_n = BLOCK * n * (n if mode == "rs" else 1)
            sends = [_data(f, T, in_n, 5, r) for r in range(n)]
            cmode = ca.MODE_ALLREDUCE if mode == "ar" else ca.MODE_REDUCE_SCATTER
            want = sr.simulate(cmode, sends, k, b, kk, fn, slices=slices, schedule=SCHED[sched], commutative=True)
            got = _run_group(gu, g, mode, sends, T, k, b, op, dt, es)
            for r in range(n):
                _same(got[r], want[r], kk, f"{f} {mode} ({n}, {k}, {b}) {sched} slices={slices} rank {r}")
        finally:
            g.set_schedule(ca.SCHEDULE_FLAT)
            g.set_slices(1)


@pytest.mark.parametrize("f,T", COLLECTIVE_KINDS, ids=["sum2-float32", "moments-float64"])
def test_mpich_baselines(gu, env, groups, f, T):
    """Recursive exchange, k-reduce-scatter-allgather (taken because the ops are commutative) and the pairwise
    reduce-scatter, against the baseline's own plan under the interpreter."""
    fn, kk = _fk(f)
    es = kk * np.dtype(T).itemsize
    op, dt = env[(f, T)]
    for algo, mode, n, k in (("recexch", ca.MODE_MPICH_RECEXCH, 6, 2), ("krsag", ca.MODE_MPICH_KRSAG, 8, 2)):
        count = BLOCK * n
        sends = [_data(f, T, count, 8, r) for r in range(n)]
        want = sr.simulate(mode, sends, k, 0, kk, fn, schedule=ca.SCHEDULE_FLAT, commutative=True)
        d_send = [gu.to_dev(s) for s in sends]
        d_recv = [gu.empty_dev(count * es).fill_(0xA5) for _ in range(n)]
        assert groups(n).allreduce_mpich(mode, d_send, d_recv, count, dt, op, k, 0) == 0, algo
        gu.sync()
        for r in range(n):
            _same(gu.from_dev(d_recv[r], T, count * kk), want[r], kk, f"{f} {algo} rank {r}")
    n, count = 8, BLOCK
    sends = [_data(f, T, count * n, 9, r) for r in range(n)]
    want = sr.simulate(ca.MODE_MPICH_RS_PAIRWISE, sends, 2, 0, kk, fn, schedule=ca.SCHEDULE_FLAT, commutative=True)
    d_send = [gu.to_dev(s) for s in sends]
    d_recv = [gu.empty_dev(count * es).fill_(0xA5) for _ in range(n)]
    assert groups(n).reduce_scatter_mpich(ca.MODE_MPICH_RS_PAIRWISE, d_send, d_recv, count, dt, op) == 0
    gu.sync()
    for r in range(n):
        _same(gu.from_dev(d_recv[r], T, count * kk), want[r], kk, f"{f} pairwise reduce-scatter rank {r}")


@pytest.mark.parametrize("T", nr.BASES)
def test_sum2_allreduce_does_not_depend_on_the_geometry(gu, env, groups, T):
    """The host test's data on the device: pack, allreduce at (8, 4, 4) and at (8, 2, 2) under the default schedule,
    unpack.  The unpacked bits are equal across the geometries and equal to T(math.fsum(...)) on every rank."""
    values = nr.independence_data(T)
    exact = nr.exact_sum(values)
    n, cnt, isz = 8, nr.INDEP_COUNT, np.dtype(T).itemsize
    op, dt = env[("sum2", T)]
    g = groups(n)
    d_val = [gu.to_dev(v) for v in values]
    d_send = [gu.empty_dev(cnt * 2 * isz) for _ in range(n)]
    for r in range(n):
        assert num.sum2_pack(d_send[r], d_val[r], cnt, BASE[T], gu.stream()) == 0
    gu.sync()
    results = []
    for k, b in ((4, 4), (2, 2)):
        d_recv = [gu.empty_dev(cnt * 2 * isz).fill_(0xA5) for _ in range(n)]
        assert g.all_reduce_radix_batch(d_send, d_recv, cnt, dt, op, k, b) == 0
        gu.sync()
        outs = []
        for r in range(n):
            d_out = gu.empty_dev(cnt * isz).fill_(0xA5)
            assert num.sum2_unpack(d_out, d_recv[r], cnt, BASE[T], gu.stream()) == 0
            gu.sync()
            outs.append(gu.from_dev(d_out, T, cnt))
            _same(outs[-1], exact, 1, f"(8, {k}, {b}) rank {r} against the exact sum")
        results.append(outs)
    for r in range(n):
        _same(results[0][r], results[1][r], 1, f"rank {r} across the geometries")


# ---- refusals --------------------------------------------------------------------------------------------------------

def test_other_dtypes_are_refused(gu, env, groups):
    """sum2 on FLOAT32, on contiguous(3, f32) and contiguous(2, INT32); moments on contiguous(2, f64): ERR_UNSUPPORTED
    from a fold and from a tree, nothing enqueued, the output keeps its fill byte.  A freed type code is refused
    before the op is asked.  The caller's own contiguous(2, FLOAT32) is taken.  A predefined SUM on the sum2 type
    stays ERR_UNSUPPORTED."""
    n = 1024
    sum2, _ = env[("sum2", np.float32)]
    mom, _ = env[("moments", np.float64)]
    derived = {"f32x3": ca.type_contiguous(3, ca.FLOAT32), "i32x2": ca.type_contiguous(2, ca.INT32),
               "f64x2": ca.type_contiguous(2, ca.FLOAT64), "own": ca.type_contiguous(2, ca.FLOAT32)}
    dead = ca.type_contiguous(2, ca.FLOAT32)
    assert ca.type_free(dead) == 0
    try:
        for op, dt in ((sum2, ca.FLOAT32), (sum2, derived["f32x3"]), (sum2, derived["i32x2"]), (mom, derived["f64x2"])):
            es = ca.type_size(dt)
            src = [gu.to_dev(np.full(n * es, 0x3C, np.uint8)) for _ in range(4)]
            out = gu.empty_dev(n * es).fill_(0xA5)
            assert ca.reduce_multi(out, src[0], src[1:2], n, dt, op, gu.stream()) == ca.ERR_UNSUPPORTED
            assert ca.reduce_tree(out, src, [0, 1, 0, 2], [0, 0, 0], n, dt, op, gu.stream()) == ca.ERR_UNSUPPORTED
            gu.sync()
            assert bool((out == 0xA5).all()), f"dtype {dt}: the output was written"
            assert bool((src[0] == 0x3C).all())
        src = [gu.to_dev(np.full(n * 8, 0x3C, np.uint8)) for _ in range(2)]
        out = gu.empty_dev(n * 8).fill_(0xA5)
        assert ca.reduce_multi(out, src[0], src[1:2], n, dead, sum2, gu.stream()) != 0
        gu.sync()
        assert bool((out == 0xA5).all()), "a freed type: the output was written"
        # the caller's own type of the same content: taken, and the same bits as with the library's type
        x, y = _data("sum2", np.float32, n, 3, 0), _data("sum2", np.float32, n, 3, 1)
        dx, dy = gu.to_dev(x), gu.to_dev(y)
        out = gu.empty_dev(n * 8).fill_(0xA5)
        assert ca.reduce_multi(out, dy, [dx], n, derived["own"], sum2, gu.stream()) == 0
        gu.sync()
        _same(gu.from_dev(out, np.float32, 2 * n), sr.fold_ref(y, [x], 2, nr.sum2, False), 2, "the caller's own type")
        # a predefined op on the sum2 type
        g = groups(4)
        t = env[("sum2", np.float32)][1]
        d = [gu.empty_dev(4 * BLOCK * 8) for _ in range(4)]
        dr = [gu.empty_dev(4 * BLOCK * 8).fill_(0xA5) for _ in range(4)]
        assert g.all_reduce_radix_batch(d, dr, 4 * BLOCK, t, ca.SUM, 2, 2) == ca.ERR_UNSUPPORTED
        gu.sync()
        assert all(bool((x == 0xA5).all()) for x in dr)
    finally:
        for t in derived.values():
            assert ca.type_free(t) == 0
