"""Derived element types (chr_type_contiguous) with user-defined ops on the device, bit for bit.

The ops are tests/userop/struct_op.hip: one element is Blk<B, K>, K consecutive B, and the launchers come from
include/chiara_user_op.hpp -- whose kernels run an element size S that does not divide 16 element-wise or in groups
of lcm(S, 16) bytes.  Every test that reaches those kernels runs twice: through libstruct_op.so, the header as shipped
(groups at the sizes where they measured faster, every tree taken), and through libstruct_op_all.so (groups at every
size that has them, and the trees the register rule keeps from the vector kernel declined to the folds).  Expected
values are numpy's (tests/struct_ref.py; its HalfAdd is the oracle's user_halfadd, tests/test_type_contiguous_host.py),
and for HalfAdd collectives the oracle's own on 3N base elements: the chunk boundaries coincide.  Every output sits
between guard bands and every input is compared with a snapshot (tests/footprint_util.py): the call writes exactly
n * S bytes."""
import ctypes
import itertools
import os
from math import gcd

import numpy as np
import pytest

import chiara_amd as ca
import pyoracle as po
import struct_ref as sr
from footprint_util import Guarded
from tree_util import random_program

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BUILDS = {"shipped": "libstruct_op.so", "all": "libstruct_op_all.so"}
KNOBS = {"shipped": (1, 1), "all": (2, 0)}  # CHR_USER_GROUP_VEC, CHR_USER_TREE_WIDE_ELEMENTWISE
# shape -> (numpy base type, K, the library's base type)
SH = {"u8x3": (np.uint8, 3, ca.UINT8), "i16x3": (np.int16, 3, ca.INT16), "f32x2": (np.float32, 2, ca.FLOAT32),
      "f32x3": (np.float32, 3, ca.FLOAT32), "f32x4": (np.float32, 4, ca.FLOAT32), "f32x5": (np.float32, 5, ca.FLOAT32),
      "f64x3": (np.float64, 3, ca.FLOAT64), "f64x4": (np.float64, 4, ca.FLOAT64), "f64x6": (np.float64, 6, ca.FLOAT64),
      "f64x8": (np.float64, 8, ca.FLOAT64), "f64x9": (np.float64, 9, ca.FLOAT64), "i32x3": (np.int32, 3, ca.INT32)}
ROTMIX_SHAPES = [s for s in SH if s != "i32x3"]
HALFADD = {"f32": "f32x3", "f64": "f64x3", "i32": "i32x3"}
C4_TREE = ([0, 1, 1, 1, 0, 1, 1, 2], [0] * 7)
SWAP_TREE = ([0, 1, 1, 1, 0, 1, 1, 2], [1, 0, 1, 0, 1, 0, 1])  # test_gpu_user_op.py's, with its swap bits


class UserTree(ctypes.Structure):  # chiara.h chr_user_tree
    _fields_ = [("out", ctypes.c_void_p), ("leaves", ctypes.c_void_p * 8), ("nleaves", ctypes.c_int),
                ("comb", ctypes.c_ubyte * 8), ("swaps", ctypes.c_ubyte * 8), ("n", ctypes.c_size_t)]


def _size(shape):
    npdt, k, _ = SH[shape]
    return np.dtype(npdt).itemsize * k


def _geom(s):
    """(elements per group E, vectors per group V, groups per lane of a fold trip U) of the header's kernels for an
    element of s bytes; a size with no vector path counts as groups of one element."""
    if 16 % s == 0:
        return 16 // s, 1, 4
    v = s // gcd(s, 16)
    return (16 * v // s, v, min(4, 8 // v)) if v <= 8 else (1, v, 1)


def _tree_taken(shape, nl, knobs):
    """The tree launcher takes an nl-leaf tree of this shape, in its vector kernel or element-wise; else it declines:
    a shape whose trees take groups (include/chiara_user_op.hpp Grp<T>::kTree) with NL x V > 8, in a build that
    declines those."""
    s, (group_vec, wide_elementwise) = _size(shape), knobs
    v = _geom(s)[1]
    groups = 16 % s != 0 and v <= 8 and s % 4 == 0 and (group_vec == 2 or (group_vec == 1 and s == 32))
    return not groups or nl * v <= 8 or bool(wide_elementwise)


def _data(rng, npdt, count):
    if np.dtype(npdt).kind == "f":
        return rng.uniform(-2, 2, count).astype(npdt)
    ii = np.iinfo(npdt)
    return rng.integers(ii.min, ii.max, count, dtype=npdt, endpoint=True)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def gu():
    import gpu_util

    return gpu_util


class Ops:
    """The derived types and the ops of libstruct_op.so, created on first use, freed at the end of the module."""

    def __init__(self, build):
        path = os.path.join(HERE, "userop", BUILDS[build])
        assert os.path.exists(path), f"{path} missing: make -C tests/userop -f struct_op.mk (build())"
        self.build = build
        self.lib = ctypes.CDLL(path)
        self.lib.chr_struct_counters.argtypes = [ctypes.POINTER(ctypes.c_long)]
        self.lib.chr_struct_counters.restype = None
        self.lib.chr_struct_counters_reset.restype = None
        self.lib.chr_struct_knobs.argtypes = [ctypes.POINTER(ctypes.c_int)]
        self.lib.chr_struct_knobs.restype = None
        self._types, self._ops = {}, {}

    def addr(self, name):
        return ctypes.cast(getattr(self.lib, name), ctypes.c_void_p).value

    def type(self, shape):
        if shape not in self._types:
            _, k, base = SH[shape]
            self._types[shape] = ca.type_contiguous(k, base)
            assert ca.type_size(self._types[shape]) == _size(shape)
        return self._types[shape]

    def op(self, functor, shape, tree=True, commute=False):
        key = (functor, shape, tree, commute)
        if key not in self._ops:
            fold = self.addr(f"chr_struct_{functor}_{shape}")
            self._ops[key] = ca.op_create(fold, commute=commute,
                                          tree=self.addr(f"chr_struct_{functor}_{shape}_tree") if tree else None)
        return self._ops[key]

    def counting_op(self):
        if "counting" not in self._ops:
            self._ops["counting"] = ca.op_create(self.addr("chr_struct_counting_fold"),
                                                 tree=self.addr("chr_struct_counting_tree"))
        return self._ops["counting"]

    def counters(self):
        """(fold-launcher calls, tree-launcher calls, of those declined, trees handed over)"""
        c = (ctypes.c_long * 4)()
        self.lib.chr_struct_counters(c)
        return tuple(c)

    def knobs(self):
        k = (ctypes.c_int * 2)()
        self.lib.chr_struct_knobs(k)
        return tuple(k)

    def close(self):
        for o in self._ops.values():
            assert ca.op_free(o) == 0
        for t in self._types.values():
            assert ca.type_free(t) == 0


@pytest.fixture(scope="module", params=list(BUILDS))
def so(request):
    o = Ops(request.param)
    yield o
    o.close()


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


def test_build_knobs(so):
    assert so.knobs() == KNOBS[so.build]


# ---- folds --------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ROTMIX_SHAPES)
def test_folds_every_layout(gu, so, shape):
    """chr_reduce_multi_ex with RotMix: m = 0, 1, 3, 17 (past kMaxIns: a second launch continuing from `out`), both
    operand orders; n = one full trip + a partial trip + a partial group, and n = 1 and G/S - 1 (below one group).
    Layouts: A all operands 16-byte aligned; B all at S mod 16 (element offset 1 of an aligned buffer: the peeled
    head); C one operand at S mod 16 and the rest aligned (incongruent: element-wise); D `out` aliasing `acc`."""
    npdt, k, _ = SH[shape]
    s = _size(shape)
    e, _, u = _geom(s)
    n_big = 256 * u * e + 37 * e + (e - 1 if e > 1 else 0)
    sizes = sorted({n_big, 1, max(e - 1, 1)})
    rng = np.random.default_rng(100 + s)
    acc = _data(rng, npdt, n_big * k)
    ins = [_data(rng, npdt, n_big * k) for _ in range(17)]
    phases = sorted({0, s % 16})
    d_acc = {p: Guarded(n_big * s, phase=p, key=1).load(acc) for p in phases}
    d_ins = {p: [Guarded(n_big * s, phase=p, key=2 + j).load(x) for j, x in enumerate(ins)] for p in phases}
    snap = {id(g): g.snapshot() for p in phases for g in [d_acc[p]] + d_ins[p]}
    d_out = {p: Guarded(n_big * s, phase=p, key=40, capacity=n_big * s) for p in phases}
    dt, op = so.type(shape), so.op("RotMixK", shape, tree=False)
    layouts = "ABCD" if s % 16 else "AD"
    for m, rf in itertools.product((0, 1, 3, 17), (0, 1)):
        want = sr.fold_ref(acc, ins[:m], k, sr.rotmix, bool(rf))
        for n, layout in itertools.product(sizes, layouts):
            if n != n_big and (layout in "CD" or m in (0, 3)):
                continue
            p_all = s % 16 if layout == "B" else 0
            a = d_acc[s % 16 if layout == "C" and m == 0 else p_all]
            xs = [d_ins[s % 16 if layout == "C" and j == 0 else p_all][j] for j in range(m)]
            out = a if layout == "D" else d_out[p_all].reset(n * s)
            what = f"{shape} m={m} rf={rf} n={n} layout {layout}"
            assert ca.reduce_multi_ex(out.ptr, a.ptr, [x.ptr for x in xs], n, dt, op, rf, gu.stream()) == 0, what
            gu.sync()
            assert out.guards_intact(), f"{what}: {out.guards_intact()}"
            np.testing.assert_array_equal(_bits(out.read(npdt)[:n * k]), _bits(want[:n * k]), err_msg=what)
            if layout == "D":
                np.testing.assert_array_equal(_bits(out.read(npdt)[n * k:]), _bits(acc[n * k:]), err_msg=what)
                a.load(acc)
            for g in [a] + xs:
                assert g.unchanged_since(snap[id(g)]), f"{what}: {g.unchanged_since(snap[id(g)])}"


def test_reduce_local_on_a_derived_type(gu, so):
    npdt, k, _ = SH["f64x3"]
    n = 1000
    rng = np.random.default_rng(7)
    x, y = _data(rng, npdt, n * k), _data(rng, npdt, n * k)
    dx, dy = gu.to_dev(x), gu.to_dev(y)
    assert ca.reduce_local(dx, dy, n, so.type("f64x3"), so.op("RotMixK", "f64x3"), gu.stream()) == 0
    gu.sync()
    np.testing.assert_array_equal(_bits(gu.from_dev(dy, npdt, n * k)), _bits(sr.fold_ref(y, [x], k, sr.rotmix, False)))


# ---- trees --------------------------------------------------------------------------------------

def _programs():
    rng = np.random.default_rng(2024)
    progs = [C4_TREE, SWAP_TREE]
    for nl in (2, 3, 4, 8):
        progs += [random_program(rng, nl), random_program(rng, nl)]
    return progs


PROGS = _programs()


@pytest.mark.parametrize("shape", ROTMIX_SHAPES)
def test_trees_every_layout(gu, so, shape):
    """chr_reduce_tree with RotMix registered with its tree launcher: 2, 3, 4 and 8 leaves, the C4 program, the one
    with swap bits and two random ones per leaf count; `out` apart, over leaf 0 and over the last leaf; layouts A
    (aligned), B (all at S mod 16) and C (one leaf at S mod 16: element-wise); n = several trips + a partial trip + a
    partial group, and 1 and G/S - 1.  A tree the launcher declines (libstruct_op_all.so: tree_u_for) runs fold by
    fold: the same bits."""
    npdt, k, _ = SH[shape]
    s = _size(shape)
    e = _geom(s)[0]
    n_big = 256 * e + 21 * e + (e - 1 if e > 1 else 0)
    rng = np.random.default_rng(200 + s)
    leaves = [_data(rng, npdt, n_big * k) for _ in range(8)]
    phases = sorted({0, s % 16})
    d_leaf = {p: [Guarded(n_big * s, phase=p, key=60 + j).load(x) for j, x in enumerate(leaves)] for p in phases}
    snap = {id(g): g.snapshot() for p in phases for g in d_leaf[p]}
    d_out = {p: Guarded(n_big * s, phase=p, key=90, capacity=n_big * s) for p in phases}
    dt, op = so.type(shape), so.op("RotMixK", shape)
    combos = [("A", None), ("A", 0), ("A", -1)]
    if s % 16:
        combos += [("B", None), ("B", 0), ("B", -1), ("C", None), ("C", 0)]
    for comb, swaps in PROGS:
        nl = len(comb)
        want = sr.tree_ref(leaves[:nl], comb, swaps, k, sr.rotmix)
        for n, (layout, into) in itertools.product(sorted({n_big, 1, max(e - 1, 1)}), combos):
            if n != n_big and (layout, into) != ("A", None) and (layout, into) != ("B", None):
                continue
            p_all = s % 16 if layout == "B" else 0
            lv = [d_leaf[s % 16 if layout == "C" and j == nl // 2 else p_all][j] for j in range(nl)]
            out = d_out[p_all].reset(n * s) if into is None else lv[into % nl]
            what = f"{shape} {comb} {swaps} n={n} layout {layout} into={into}"
            assert ca.reduce_tree(out.ptr, [g.ptr for g in lv], comb, swaps, n, dt, op, gu.stream()) == 0, what
            gu.sync()
            assert out.guards_intact(), f"{what}: {out.guards_intact()}"
            np.testing.assert_array_equal(_bits(out.read(npdt)[:n * k]), _bits(want[:n * k]), err_msg=what)
            if into is not None:
                np.testing.assert_array_equal(_bits(out.read(npdt)[n * k:]), _bits(leaves[into % nl][n * k:]))
                out.load(leaves[into % nl])
            for g in lv:
                assert g.unchanged_since(snap[id(g)]), f"{what}: {g.unchanged_since(snap[id(g)])}"


def _user_tree(out, leaf_ptrs, comb, swaps, n):
    t = UserTree()
    t.out = out
    for j, p in enumerate(leaf_ptrs):
        t.leaves[j] = p
        t.comb[j] = comb[j]
    for c, sw in enumerate(swaps):
        t.swaps[c] = sw
    t.nleaves, t.n = len(leaf_ptrs), n
    return t


@pytest.mark.parametrize("shape", ["f32x3", "f32x4", "f64x3", "f64x4", "f64x8", "u8x3", "f64x9"])
def test_tree_launcher_caps_and_mixed_batch(gu, so, shape):
    """The tree launcher called directly with wg_per_cu = 0 and 12 (the cap beside RCCL): 9 trees in one call -- past
    kMaxTreesPerLaunch, of every leaf count among 2, 3, 4 that the launcher takes -- give identical bits; where the
    build declines a leaf count (libstruct_op_all.so, the register rule), the same call with one more tree of that
    leaf count (or, when it takes none, that tree alone) returns nonzero and writes nothing."""
    npdt, k, _ = SH[shape]
    s = _size(shape)
    e = _geom(s)[0]
    n = 256 * e + 21 * e + (e - 1 if e > 1 else 0)
    rng = np.random.default_rng(300 + s)
    prng = np.random.default_rng(11)
    fn = getattr(so.lib, f"chr_struct_RotMixK_{shape}_tree")
    fn.argtypes = [ctypes.POINTER(UserTree), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    taken = [nl for nl in (2, 3, 4) if _tree_taken(shape, nl, so.knobs())]
    refused = [nl for nl in (2, 3, 4, 8) if not _tree_taken(shape, nl, so.knobs())]
    nls = [taken[t % len(taken)] for t in range(9)] if taken else []
    calls = [(nls, True)] if taken else []
    if refused:
        calls.append((nls + refused[:1], False))
    nls = nls + refused[:1]
    progs = [random_program(prng, nl) for nl in nls]
    leaves = [[_data(rng, npdt, n * k) for _ in range(nl)] for nl in nls]
    d_leaf = [[gu.to_dev(x) for x in lv] for lv in leaves]
    for cap, (call, takes) in itertools.product((0, 12), calls):
        outs = [Guarded(n * s, key=120 + t) for t in range(len(call))]
        before = [o.snapshot() for o in outs]
        arr = (UserTree * len(call))(*[_user_tree(outs[t].ptr, [d.data_ptr() for d in d_leaf[t]], *progs[t], n)
                                       for t in range(len(call))])
        rc = fn(arr, len(call), so.type(shape), cap, gu.stream().cuda_stream, None)
        gu.sync()
        assert (rc == 0) == takes, (shape, cap, call, rc)
        for t, (comb, swaps) in enumerate(progs[:len(call)]):
            if rc:
                assert outs[t].unchanged_since(before[t]), f"{shape} cap {cap}: a declined call wrote tree {t}'s output"
                continue
            assert outs[t].guards_intact(), f"{shape} cap {cap} tree {t}: {outs[t].guards_intact()}"
            np.testing.assert_array_equal(_bits(outs[t].read(npdt)), _bits(sr.tree_ref(leaves[t], comb, swaps, k, sr.rotmix)),
                                          err_msg=f"{shape} cap {cap} tree {t}")


@pytest.mark.parametrize("shape,nl", [("f64x3", 2), ("f64x3", 3), ("f32x3", 2), ("f64x4", 4)])
def test_tree_batch_of_nine(gu, so, shape, nl):
    """chr_reduce_tree_batch with 9 trees (past kMaxTreesPerLaunch); libstruct_op_all.so declines f64 x 3 with 3
    leaves: the folds."""
    npdt, k, _ = SH[shape]
    s = _size(shape)
    e = _geom(s)[0]
    n = 64 * e + 5 * e + 1
    rng = np.random.default_rng(400 + s + nl)
    progs = [random_program(rng, nl) for _ in range(9)]
    leaves = [[_data(rng, npdt, n * k) for _ in range(nl)] for _ in range(9)]
    d_leaf = [[gu.to_dev(x) for x in lv] for lv in leaves]
    outs = [Guarded(n * s, key=150 + t) for t in range(9)]
    assert ca.reduce_tree_batch([o.ptr for o in outs], d_leaf, [c for c, _ in progs], [w for _, w in progs], n,
                                so.type(shape), so.op("RotMixK", shape), gu.stream()) == 0
    gu.sync()
    for t, (comb, swaps) in enumerate(progs):
        assert outs[t].guards_intact(), f"tree {t}: {outs[t].guards_intact()}"
        np.testing.assert_array_equal(_bits(outs[t].read(npdt)), _bits(sr.tree_ref(leaves[t], comb, swaps, k, sr.rotmix)),
                                      err_msg=f"{shape} {nl} leaves, tree {t}")


def test_wide_tree_runs_element_wise_or_is_declined_to_the_folds(gu, so):
    """8 leaves of 24-byte elements: in groups NL x V = 24 loads of 16 B per lane would be in flight.  Measured on that
    tree at 16 MiB per leaf (tools/userop_bench.py --struct, fraction of 8 TB/s at 9 units, 2 rounds): declined to the
    folds 0.332-0.334, the element-wise one-pass tree 0.608.  The shipped header keeps the one-pass tree: one
    tree-launcher call, none declined, no fold call.  libstruct_op_all.so declines: the launcher returns nonzero with
    nothing enqueued and the library evaluates C4's tree in three fold-launcher calls.  The bits are the fold-by-fold
    value either way.  A 2-leaf tree of the same type is taken by both."""
    npdt, k, _ = SH["f64x3"]
    n = 4099
    rng = np.random.default_rng(5)
    leaves = [_data(rng, npdt, n * k) for _ in range(8)]
    d = [gu.to_dev(x) for x in leaves]
    dt, op = so.type("f64x3"), so.counting_op()
    comb, swaps = C4_TREE
    out = Guarded(n * 24, key=170)
    so.lib.chr_struct_counters_reset()
    assert ca.reduce_tree(out.ptr, d, comb, swaps, n, dt, op, gu.stream()) == 0
    gu.sync()
    assert so.counters() == ((0, 1, 0, 1) if so.build == "shipped" else (3, 1, 1, 1)), so.counters()
    assert out.guards_intact(), out.guards_intact()
    # fold by fold: ((l0 l1 l2 l3) (l4 l5 l6 l7)) as three chains
    left = sr.fold_ref(leaves[0], leaves[1:4], k, sr.rotmix, False)
    right = sr.fold_ref(leaves[4], leaves[5:8], k, sr.rotmix, False)
    want = sr.fold_ref(left, [right], k, sr.rotmix, False)
    np.testing.assert_array_equal(_bits(want), _bits(sr.tree_ref(leaves, comb, swaps, k, sr.rotmix)))
    np.testing.assert_array_equal(_bits(out.read(npdt)), _bits(want))
    out2 = Guarded(n * 24, key=171)
    so.lib.chr_struct_counters_reset()
    assert ca.reduce_tree(out2.ptr, d[:2], [0, 1], [1], n, dt, op, gu.stream()) == 0
    gu.sync()
    assert so.counters() == (0, 1, 0, 1), so.counters()
    np.testing.assert_array_equal(_bits(out2.read(npdt)), _bits(sr.tree_ref(leaves[:2], [0, 1], [1], k, sr.rotmix)))


# ---- collectives: HalfAdd, pinned by the reference through the oracle -----------------------------

CASES = [(8, 4, 4), (8, 2, 8), (6, 3, 2), (4, 2, 2), (2, 2, 1)]
SCHEDS = {"flat": ca.SCHEDULE_FLAT, "exact": ca.SCHEDULE_EXACT, "reference": ca.SCHEDULE_REFERENCE}


def _collective(gu, g, mode, sends, count, dt, npdt, op, k, b, inplace):
    """Every rank's output (base elements) of an allreduce ("ar": count per rank) or reduce-scatter ("rs": recvcount)."""
    n = len(sends)
    out_bytes = count * ca.type_size(dt)
    if inplace:
        d_recv, d_send = [gu.to_dev(x) for x in sends], [ca.IN_PLACE] * n
    else:
        d_recv, d_send = [gu.empty_dev(out_bytes) for _ in range(n)], [gu.to_dev(x) for x in sends]
    fn = g.all_reduce_radix_batch if mode == "ar" else g.reduce_scatter_radix_batch
    rc = fn(d_send, d_recv, count, dt, op, k, b)
    gu.sync()
    assert rc == 0, rc
    return [gu.from_dev(d, npdt, out_bytes // np.dtype(npdt).itemsize) for d in d_recv]


def _halfadd_runs():
    """(n, k, b) x N per rank in {n, 5n, 341n} x base type, each with a schedule, a pipeline depth, a collective, in
    place or not, with the tree launcher or folds only: the second factor cycles so that all its 72 combinations run
    twice and every first one at least three times."""
    first = list(itertools.product(CASES, (1, 5, 341), ("f32", "f64", "i32")))
    second = list(itertools.product(SCHEDS, (1, 2, 3), ("ar", "rs"), (False, True), (True, False)))
    return [(first[i % len(first)], second[i % len(second)]) for i in range(2 * len(second))]


def test_halfadd_collectives_match_the_oracle_on_the_base_type(gu, so, groups):
    """A derived-type call with count N equals, byte for byte, the oracle's user_halfadd collective on the base type
    with count 3N.  341 x 24 bytes is no multiple of 16: chunks alternate between aligned and 8 mod 16."""
    bad = []
    for ((n, k, b), mult, base), (sched, slices, mode, inplace, tree) in _halfadd_runs():
        shape = HALFADD[base]
        npdt = SH[shape][0]
        count = mult * n if mode == "ar" else mult  # rs: recvcount; every rank sends n * recvcount
        sends = [po.fill(3 * mult * n, base, po.PAT_UNIFORM, 31 + mult, r) for r in range(n)]
        want = (po.allreduce_radix_batch if mode == "ar" else po.reduce_scatter_radix_batch)(
            sends, k, b, base, "user_halfadd", inplace)
        g = groups(n)
        g.set_schedule(SCHEDS[sched])
        g.set_slices(slices)
        try:
            got = _collective(gu, g, mode, sends, count, so.type(shape), npdt, so.op("HalfAddK", shape, tree=tree), k, b,
                              inplace)
        finally:
            g.set_schedule(ca.SCHEDULE_FLAT)
            g.set_slices(1)
        if not all(np.array_equal(_bits(x), _bits(w)) for x, w in zip(got, want)):
            bad.append(((n, k, b), mult, base, sched, slices, mode, inplace, tree))
    assert not bad, f"{len(bad)} device/oracle mismatches, e.g. {bad[:5]}"


@pytest.mark.parametrize("tree", [True, False])
def test_halfadd_phases_and_baselines(gu, so, groups, tree):
    """One call of each stand-alone reduction phase and one MPICH baseline per branch -- recursive doubling with a
    non-commutative op (rank-ordered operands), the ring, and k-reduce-scatter-allgather's refusal -- on f64 x 3."""
    shape, base, npdt = "f64x3", "f64", np.float64
    dt, op = so.type(shape), so.op("HalfAddK", shape, tree=tree)
    n, k, b, rc = 8, 2, 2, 341
    g = groups(n)
    for algo, mode in (("irs", ca.MODE_INTRA_REDUCE_SCATTER), ("ilr", ca.MODE_INTER_REDUCE_LINEAR)):
        in_n, out_n = po.phase_sizes(algo, n, b, rc)
        sends = [po.fill(3 * in_n, base, po.PAT_UNIFORM, 5, r) for r in range(n)]
        want = po.phase_collective(algo, sends, base, "user_halfadd", k, b, 3 * rc)
        d_send, d_recv = [gu.to_dev(x) for x in sends], [gu.empty_dev(out_n * 24) for _ in range(n)]
        assert g.phase_collective(mode, d_send, d_recv, rc, dt, op, k, b) == 0
        gu.sync()
        for r in range(n):
            np.testing.assert_array_equal(_bits(gu.from_dev(d_recv[r], npdt, 3 * out_n)), _bits(want[r][:3 * out_n]),
                                          err_msg=f"{algo} rank {r}")
    count = 341 * n
    sends = [po.fill(3 * count, base, po.PAT_UNIFORM, 9, r) for r in range(n)]
    for algo, mode in (("rd", ca.MODE_MPICH_RD), ("ring", ca.MODE_MPICH_RING)):
        want = po.mpich_allreduce(algo, sends, base, "user_halfadd")
        d_send, d_recv = [gu.to_dev(x) for x in sends], [gu.empty_dev(count * 24) for _ in range(n)]
        assert g.allreduce_mpich(mode, d_send, d_recv, count, dt, op) == 0
        gu.sync()
        for r in range(n):
            np.testing.assert_array_equal(_bits(gu.from_dev(d_recv[r], npdt, 3 * count)), _bits(want[r]),
                                          err_msg=f"{algo} rank {r}")
    d_send, d_recv = [gu.to_dev(x) for x in sends], [gu.empty_dev(count * 24) for _ in range(n)]
    assert g.allreduce_mpich(ca.MODE_MPICH_KRSAG, d_send, d_recv, count, dt, op, 2, 0) == ca.ERR_UNSUPPORTED
    # a predefined op on the derived type: refused before anything is enqueued
    assert g.all_reduce_radix_batch(d_send, d_recv, count, dt, ca.SUM, 2, 2) == ca.ERR_UNSUPPORTED
    gu.sync()


def test_host_buffers_through_the_pipelined_windows(gu, so):
    """Host buffers on a single-rank communicator with chr_comm_set_host_pipeline: 2.4 MB of 24-byte elements in 1 MiB
    windows (a window holds whole elements), out of place and in place: the allreduce of one rank is its input."""
    comm = ca.Comm(1, ca.get_unique_id(), 0, 0)
    try:
        comm.set_host_pipeline(1)
        n = 100001
        x = po.fill(3 * n, "f64", po.PAT_UNIFORM, 3, 0)
        y = np.zeros_like(x)
        dt, op = so.type("f64x3"), so.op("HalfAddK", "f64x3")
        assert ca.all_reduce_radix_batch(x, y, n, dt, op, comm, 2, 1) == 0
        np.testing.assert_array_equal(_bits(y), _bits(x))
        z = x.copy()
        assert ca.all_reduce_radix_batch(ca.IN_PLACE, z, n, dt, op, comm, 2, 1) == 0
        np.testing.assert_array_equal(_bits(z), _bits(x))
        assert ca.all_reduce_radix_batch(x, y, n, dt, ca.SUM, comm, 2, 1) == ca.ERR_UNSUPPORTED
    finally:
        comm.set_host_pipeline(0)
        comm.destroy()


# ---- collectives: RotMix, pinned by the plan interpreter ------------------------------------------

@pytest.mark.parametrize("n,k,b,sched,slices", [(8, 4, 4, "flat", 1), (8, 4, 4, "flat", 3), (6, 3, 2, "exact", 1)])
@pytest.mark.parametrize("tree", [True, False])
def test_rotmix_collectives_match_the_plan_interpreter(gu, so, groups, n, k, b, sched, slices, tree):
    """RotMix mixes the components of an element, so a collective that cut elements anywhere else than the plans do
    would show: f64 x 3 allreduce and reduce-scatter against struct_ref's interpreter of the same plans."""
    npdt, kk, _ = SH["f64x3"]
    count = 341 * n
    rng = np.random.default_rng(n * 100 + slices)
    g = groups(n)
    g.set_schedule(SCHEDS[sched])
    g.set_slices(slices)
    try:
        for mode, cmode in (("ar", ca.MODE_ALLREDUCE), ("rs", ca.MODE_REDUCE_SCATTER)):
            per = count if mode == "ar" else count // n
            sends = [_data(rng, npdt, count * kk) for _ in range(n)]
            want = sr.simulate(cmode, sends, k, b, kk, sr.rotmix, slices=slices, schedule=SCHEDS[sched])
            got = _collective(gu, g, mode, sends, per, so.type("f64x3"), npdt, so.op("RotMixK", "f64x3", tree=tree), k, b,
                              False)
            for r in range(n):
                np.testing.assert_array_equal(_bits(got[r]), _bits(want[r]), err_msg=f"{mode} rank {r}")
    finally:
        g.set_schedule(ca.SCHEDULE_FLAT)
        g.set_slices(1)


# ---- data movement with no op, and a freed type ---------------------------------------------------

def test_data_movement_and_a_dead_type(gu, groups):
    """chr_local_allgather_radix_batch and the stand-alone intra scatter move 24-byte elements with no op; once the
    type is freed the same call is CHR_ERR_INVALID_ARG."""
    n, k, b, cnt = 8, 2, 4, 341
    dt = ca.type_contiguous(3, ca.FLOAT64)
    g = groups(n)
    try:
        sends = [po.fill(3 * cnt, "f64", po.PAT_UNIFORM, 21, r) for r in range(n)]
        d_send, d_recv = [gu.to_dev(x) for x in sends], [gu.empty_dev(n * cnt * 24) for _ in range(n)]
        assert g.allgather_radix_batch(d_send, cnt, dt, d_recv, k, b) == 0
        gu.sync()
        for r in range(n):
            np.testing.assert_array_equal(_bits(gu.from_dev(d_recv[r], np.float64, 3 * n * cnt)),
                                          _bits(np.concatenate(sends)), err_msg=f"allgather rank {r}")
        in_n, out_n = po.phase_sizes("isc", n, b, cnt)
        ssend = [po.fill(3 * in_n, "f64", po.PAT_UNIFORM, 23, r) for r in range(n)]
        want = po.phase_collective("isc", ssend, "f64", "sum", k, b, 3 * cnt)
        d_s, d_r = [gu.to_dev(x) for x in ssend], [gu.empty_dev(out_n * 24) for _ in range(n)]
        assert g.phase_collective(ca.MODE_INTRA_SCATTER, d_s, d_r, cnt, dt, ca.SUM, k, b) == 0
        gu.sync()
        for r in range(n):
            np.testing.assert_array_equal(_bits(gu.from_dev(d_r[r], np.float64, 3 * out_n)), _bits(want[r][:3 * out_n]),
                                          err_msg=f"intra scatter rank {r}")
    finally:
        assert ca.type_free(dt) == 0
    assert g.allgather_radix_batch(d_send, cnt, dt, d_recv, k, b) == ca.ERR_INVALID_ARG
    assert g.phase_collective(ca.MODE_INTRA_SCATTER, d_s, d_r, cnt, dt, ca.SUM, k, b) == ca.ERR_INVALID_ARG
