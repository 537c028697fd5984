"""The memory footprint of every kernel and collective entry point.

The rest of the GPU suite pins what a call computes inside [out, out + n).  This file pins what else it touches:
every output lies between guard bands of position-dependent bytes and every input is snapshotted, guards and
payload, before the call (tests/footprint_util.py).  Every case asserts
  (a) rc == 0 and the output payload bit-equal to the oracle (or to the reference's golden hash),
  (b) the output's guards intact,
  (c) every input byte-identical to its snapshot: each ins[j], each leaf that is not the output, `acc` when
      out != acc, every rank's send buffer.
The sizes sit on the launchers' own edges: the scalar head align_split cuts (one element short of it, exactly it,
one more), a body of less than one vector, one element either side of a whole trip, two trips and a partial one
with a ragged tail; the phases put the operands on every path (vector body with and without a head, the scalar
kernel throughout).  The streaming shapes (XCD map, odd-XCD handover, launch pieces) run in child processes with
the tuning variables set, their outputs under a guard as large as the payload, which covers every address a
surplus workgroup of the remapped grid could form.  A mismatch names the region and the byte offset of the first
differing byte from the payload's start, which says which trip or segment strayed."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import chiara_amd as ca
import footprint_util as fu
import pyoracle as po
from test_gpu_kernels import DT, OP, _bits, _bytes_copy
from test_gpu_tree import C4_TREE, K2B8_TREE
from test_gpu_xcd_map import XCD_CONFIGS
from tree_util import random_program, tree_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def gu():
    import gpu_util

    return gpu_util


def _es(dtype):
    return np.dtype(po.NP_DTYPES[dtype]).itemsize


class Pool:
    """Guarded buffers by (slot, phase), each with room for `cap` payload bytes: a sweep re-stamps and resizes them
    (Guarded.reset) instead of allocating a dozen buffers per case.  The upper guard only grows with the room a
    smaller payload leaves."""

    def __init__(self, cap, hi_guard=fu.GUARD_BYTES):
        self.cap, self.hi, self.bufs = cap, hi_guard, {}

    def get(self, slot, phase, nbytes):
        g = self.bufs.get((slot, phase))
        if g is None:
            g = self.bufs[(slot, phase)] = fu.Guarded(nbytes, phase, hi_guard=self.hi, capacity=self.cap,
                                                      key=zlib.crc32(f"{slot}@{phase}".encode()))
            return g
        return g.reset(nbytes)


def _verdict(rc, out, got, ref, watched):
    """The problems of one case: (a) rc and result, (b) the output's guards, (c) every watched input."""
    bad = []
    if rc != 0:
        bad.append(f"rc = {rc}")
    if got is not None and not np.array_equal(_bits(got), _bits(ref)):
        bad.append("result != oracle")
    chk = out.guards_intact()
    if not chk:
        bad.append(f"out {chk!r}")
    for name, g, snap in watched:
        chk = g.unchanged_since(snap)
        if not chk:
            bad.append(f"{name} {chk!r}")
    return bad


def _edges(head, E, T):
    """Element counts on the launch edges for a scalar head of `head` elements, E elements per vector and T vectors
    per trip."""
    ns = [1, head - 1, head, head + 1, head + E - 1, head + T * E - 1, head + T * E, head + T * E + 1,
          head + (2 * T + 1) * E + (E - 1)]
    return sorted({n for n in ns if n > 0})


def _layouts(es):
    """(output phase, input phase): everything at phase 0, at one element, at one element below the boundary (a
    16-byte element: at 8, which no vector can serve), and the inputs off the output by one element (8 bytes for a
    16-byte element, its own alignment): the scalar kernel throughout."""
    lay = [(0, 0), (es % 16, es % 16), ((16 - es) % 16, (16 - es) % 16)]
    if es == 16:
        lay.append((8, 8))
    lay.append((0, 8 if es == 16 else es))
    return sorted(set(lay), key=lay.index)


def _head(phase, es):
    return (16 - phase) // es if phase and phase % es == 0 else 0


def test_the_checks_fail_on_the_device_when_a_call_strays(gu):
    """The checks themselves, on device memory: the bucket kernel asked for one element more than the payload holds
    writes that element into the upper guard (memory the buffer owns), and is reported at offset n * es with at most
    es differing bytes; asked to write into an input's payload, it is reported by that input's snapshot."""
    n = 1024 * 4 + 3
    acc, x = po.fill(n + 1, "f32", 0, 3, 0), po.fill(n + 1, "f32", 0, 3, 1)
    out, d_acc, d_x = fu.Guarded(n * 4, 0, key=1), fu.Guarded((n + 1) * 4, 0, key=2), fu.Guarded((n + 1) * 4, 0, key=3)
    d_acc.load(acc), d_x.load(x)
    assert ca.reduce_multi(out.ptr, d_acc.ptr, [d_x.ptr], n + 1, ca.FLOAT32, ca.SUM, gu.stream()) == 0
    gu.sync()
    chk = out.guards_intact()
    assert not chk and len(chk.diffs) == 1, repr(chk)
    d = chk.diffs[0]
    assert d.region == "upper" and n * 4 <= d.offset < (n + 1) * 4 and 1 <= d.count <= 4, repr(chk)
    ref = po.reduce_multi(acc.copy(), [x], "f32", "sum")
    assert np.array_equal(out.read(np.uint32), ref[:n].view(np.uint32))
    snap = d_x.snapshot()
    assert ca.reduce_multi(d_x.ptr + 64, d_acc.ptr, [d_acc.ptr], 5, ca.FLOAT32, ca.SUM, gu.stream()) == 0
    gu.sync()
    chk = d_x.unchanged_since(snap)
    assert not chk and chk.diffs[0].region == "payload", repr(chk)
    assert 64 <= chk.diffs[0].offset < 84 and chk.diffs[0].count <= 20, repr(chk)
    assert d_x.guards_intact()


# ---- bucket kernel --------------------------------------------------------------------------------------------

BUCKET = [("u8", "sum"), ("bf16", "sum"), ("f32", "sum"), ("f64", "sum"), ("fi", "maxloc"), ("di", "maxloc"),
          ("cd", "sum"), ("cd", "prod")]
BUCKET_M = (1, 3, 8, 9)
# cases per sweep = 2 (out == acc, out separate) x 4 fan-ins x the distinct counts of every layout.  With a head of
# h elements the nine counts of _edges are distinct unless small ones coincide or vanish:
#   es 1, 2, 4 (E = 16, 8, 4): phase 0 / 0 and the inputs-off layout, h = 0: {1, E - 1} and four around the trips = 6
#               each; one element in, h = E - 1: all 9; one below the boundary, h = 1: {1, 2, E} and four = 7: 28 x 8
#   es 8 (E = 2): one element in IS one below the boundary, so three layouts: h = 0: {1} and four = 5 (twice);
#               h = 1: {1, 2} and four = 6: 16 x 8
#   es 16 (E = 1): no head; {1, T - 1, T, T + 1, 2 T + 1} at 0 / 0, at 8 / 8 (no vector can serve it) and with the
#               inputs 8 bytes off: 15 x 8
BUCKET_CASES = {"u8": 224, "bf16": 224, "f32": 224, "f64": 128, "fi": 128, "di": 120, "cd": 120}


def _bucket_u(dtype, op, m):
    """Vectors per lane of the plain shape (reduce_vec.hpp vec_u_dt; m = 9 runs a group of 8 first)."""
    return 1 if dtype == "cd" and op == "prod" else 4 if min(m, 8) <= 2 else 2


def _bucket_sweep(dtype, op):
    es = _es(dtype)
    E = 16 // es
    for alias in (True, False):
        for m in BUCKET_M:
            T = 256 * _bucket_u(dtype, op, m)
            for po_, pi_ in _layouts(es):
                for n in _edges(_head(po_, es) if po_ == pi_ else 0, E, T):
                    yield alias, m, po_, pi_, n


def _bucket_data(dtype, op, nmax, pattern):
    data = [po.fill(nmax, dtype, pattern, 31, r) for r in range(10)]
    if dtype == "di":  # the struct's padding bytes carry a marker per operand: a whole-element copy moves them
        for r, x in enumerate(data):
            x.view(np.uint8).reshape(-1, 16)[:, 12:] = 0xA0 + r
    return data


def _chain_running_first(acc, ins, dtype, op):
    run = _bytes_copy(acc)
    for x in ins:
        nxt = _bytes_copy(x)
        po.reduce_local(run, nxt, dtype, op)  # MPI_Reduce_local(in = running, inout = next)
        run = nxt
    return run


def _run_bucket(gu, dtype, op, flags=0, pattern=po.PAT_UNIFORM):
    es, npdt = _es(dtype), po.NP_DTYPES[dtype]
    cases = list(_bucket_sweep(dtype, op))
    nmax = max(c[4] for c in cases)
    pool = Pool(nmax * es)
    data = _bucket_data(dtype, op, nmax, pattern)
    refs, bad = {}, []
    for alias, m, po_, pi_, n in cases:
        acc_np, ins_np = data[0][:n], [x[:n] for x in data[1:m + 1]]
        if (m, n) not in refs:
            refs[(m, n)] = (_chain_running_first(acc_np, ins_np, dtype, op) if flags else
                            po.reduce_multi(_bytes_copy(acc_np), ins_np, dtype, op))
        out = pool.get("out", po_, n * es)
        acc = out if alias else pool.get("acc", po_, n * es)
        acc.load(acc_np)
        ins = [pool.get(f"in{j}", pi_, n * es).load(x) for j, x in enumerate(ins_np)]
        watched = [(f"ins[{j}]", g, g.snapshot()) for j, g in enumerate(ins)]
        if not alias:
            watched.append(("acc", acc, acc.snapshot()))
        ptrs = [g.ptr for g in ins]
        if flags:
            rc = ca.reduce_multi_ex(out.ptr, acc.ptr, ptrs, n, DT[dtype], OP[op], flags, gu.stream())
        else:
            rc = ca.reduce_multi(out.ptr, acc.ptr, ptrs, n, DT[dtype], OP[op], gu.stream())
        gu.sync()
        for p in _verdict(rc, out, out.read(npdt), refs[(m, n)], watched):
            bad.append(f"{'in place' if alias else 'out of place'} m={m} phases={po_}/{pi_} n={n}: {p}")
    return len(cases), bad


@pytest.mark.parametrize("dtype,op", BUCKET, ids=[f"{d}-{o}" for d, o in BUCKET])
def test_bucket_kernel_footprint(gu, dtype, op):
    """chr_reduce_multi, one type per element class (1, 2, 4, 8 bytes, the 8-byte pair, the 16-byte pair with padding
    bytes, the 16-byte complex whose PROD runs one vector per lane): out == acc and out separate, m = 1, 3, 8 and 9 (at
    9 the second group of launch_reduce continues from `out`: the caller's acc must still be untouched), every layout
    of _layouts, every count of _edges."""
    ran, bad = _run_bucket(gu, dtype, op)
    assert ran == BUCKET_CASES[dtype], ran
    assert not bad, f"{len(bad)} problems, e.g. {bad[:4]}"


def test_bucket_kernel_footprint_running_first(gu):
    """chr_reduce_multi_ex(CHR_REDUCE_RUNNING_FIRST), f32 MAX on TIES data (the swapped op codes are kernels of
    their own; -0 / +0 and NaN make the order visible): the same sweep against MPICH_do_reduce's chain."""
    ran, bad = _run_bucket(gu, "f32", "max", ca.REDUCE_RUNNING_FIRST, po.PAT_TIES)
    assert ran == BUCKET_CASES["f32"], ran
    assert not bad, f"{len(bad)} problems, e.g. {bad[:4]}"


def test_the_sweeps_cover_their_edges():
    """What the counts asserted above stand for: every sweep holds both aliasings, all four fan-ins, a layout on the
    scalar kernel, a head, and counts one element either side of a whole trip."""
    for dtype, op in BUCKET:
        cases = list(_bucket_sweep(dtype, op))
        es = _es(dtype)
        assert len(cases) == BUCKET_CASES[dtype] and len(set(cases)) == len(cases), (dtype, len(cases))
        assert {c[0] for c in cases} == {True, False} and {c[1] for c in cases} == set(BUCKET_M)
        assert any(c[2] != c[3] for c in cases) and (es == 16 or any(_head(c[2], es) for c in cases))
        for m in BUCKET_M:
            TE = 256 * _bucket_u(dtype, op, m) * (16 // es)
            ns = {c[4] for c in cases if c[1] == m and c[2] == c[3] == 0}
            assert {1, TE - 1, TE, TE + 1, 2 * TE + 2 * (16 // es) - 1} <= ns, (dtype, m, sorted(ns))
    assert [(p, _head(p, 4)) for p in (0, 4, 12)] == [(0, 0), (4, 3), (12, 1)]
    for dtype, op in TREE:
        assert len(list(_tree_sweep(dtype))) == TREE_CASES[dtype], (dtype, len(list(_tree_sweep(dtype))))


@pytest.mark.parametrize("dtype,op", BUCKET[:7], ids=[d for d, _ in BUCKET[:7]])
def test_bucket_kernel_n0_touches_nothing(gu, dtype, op):
    es = _es(dtype)
    bufs = [fu.Guarded(64 * es, 0, key=j).load(po.fill(64, dtype, 0, 3, j)) for j in range(3)]
    snaps = [g.snapshot() for g in bufs]
    out, acc, x = bufs
    assert ca.reduce_multi(out.ptr, acc.ptr, [x.ptr], 0, DT[dtype], OP[op], gu.stream()) == 0
    assert ca.reduce_multi(out.ptr, out.ptr, [x.ptr], 0, DT[dtype], OP[op], gu.stream()) == 0
    assert ca.reduce_tree(out.ptr, [acc.ptr, x.ptr], [0, 1], [0], 0, DT[dtype], OP[op], gu.stream()) == 0
    gu.sync()
    for g, s in zip(bufs, snaps):
        assert g.unchanged_since(s), repr(g.unchanged_since(s))


# ---- tree kernel, plain shape -----------------------------------------------------------------------------------

TREE = [("f32", "sum"), ("bf16", "sum"), ("i16", "sum"), ("di", "maxloc"), ("cf", "sum")]
# (program, output) pairs: the two 8-leaf programs with out separate and over leaf 0, 3, 7, the 4-leaf one with out
# separate and over leaf 0, 3 = 11; times the distinct counts of the three layouts (as for the bucket kernel): es 2
# and 4: 6 + 9 + 6 = 21; es 8: 5 + 6 + 5 = 16; es 16 (phase es is phase 0, so 8 / 8 instead): 3 x 5 = 15
TREE_CASES = {"f32": 231, "bf16": 231, "i16": 231, "di": 165, "cf": 176}


def _tree_programs():
    rng = np.random.default_rng(5)
    while True:
        comb, swaps = random_program(rng, 4)
        if any(swaps):
            return [C4_TREE, K2B8_TREE, (comb, swaps)]


TREE_PROGS = _tree_programs()


def _tree_layouts(es):
    lay = [(0, 0), (es % 16, es % 16)] + ([(8, 8)] if es == 16 else [])
    lay.append((0, 8 if es == 16 else es))  # the leaves off the output: not congruent, the scalar tree kernel
    return sorted(set(lay), key=lay.index)


def _tree_sweep(dtype):
    es = _es(dtype)
    E = 16 // es
    for pi, (comb, swaps) in enumerate(TREE_PROGS):
        nl = len(comb)
        T = 256 * (4 if nl <= 4 else 2)  # reduce_tree.hpp tree_u<NL, false>
        for into in [None] + sorted({min(j, nl - 1) for j in (0, 3, 7)}):
            for po_, pl_ in _tree_layouts(es):
                for n in _edges(_head(po_, es) if po_ == pl_ else 0, E, T):
                    yield pi, into, po_, pl_, n


@pytest.mark.parametrize("dtype,op", TREE, ids=[d for d, _ in TREE])
def test_tree_kernel_footprint(gu, dtype, op):
    """chr_reduce_tree at the plain shape: C4's and the k = 2, b = 8 tree and a random 4-leaf program with swapped
    combines (U = 2 and U = 4 trips), out separate and over leaf 0, 3 and 7 -- the other leaves must stay as they
    were -- at phase 0, at one element, and with the leaves off the output (the scalar tree kernel); counts on the
    head, partial-trip and tail edges of that leaf count's trip."""
    es, npdt = _es(dtype), po.NP_DTYPES[dtype]
    cases = list(_tree_sweep(dtype))
    nmax = max(c[4] for c in cases)
    pool = Pool(nmax * es)
    pat = po.PAT_TIES if dtype == "di" else po.PAT_UNIFORM
    data = [po.fill(nmax, dtype, pat, 41, r) for r in range(8)]
    refs, bad = {}, []
    for pi, into, po_, pl_, n in cases:
        comb, swaps = TREE_PROGS[pi]
        nl = len(comb)
        lv_np = [x[:n] for x in data[:nl]]
        if (pi, n) not in refs:
            refs[(pi, n)] = tree_ref(lv_np, comb, swaps, dtype, op)
        leaves = [pool.get("out" if j == into else f"leaf{j}", po_ if j == into else pl_, n * es).load(x)
                  for j, x in enumerate(lv_np)]
        out = pool.get("out", po_, n * es) if into is None else leaves[into]
        watched = [(f"leaf {j}", g, g.snapshot()) for j, g in enumerate(leaves) if j != into]
        rc = ca.reduce_tree(out.ptr, [g.ptr for g in leaves], comb, swaps, n, DT[dtype], OP[op], gu.stream())
        gu.sync()
        for p in _verdict(rc, out, out.read(npdt), refs[(pi, n)], watched):
            where = "separate" if into is None else f"leaf {into}"
            bad.append(f"program {pi} out={where} phases={po_}/{pl_} n={n}: {p}")
    assert len(cases) == TREE_CASES[dtype], len(cases)
    assert not bad, f"{len(bad)} problems, e.g. {bad[:4]}"


def test_tree_batch_of_nine_footprint(gu):
    """chr_reduce_tree_batch, 9 trees of 8 leaves, n = 2053 f32 one element off a boundary (a head of 3, a ragged
    tail): two launches, 8 segments then 1.  Every output guarded, all 72 leaves snapshotted."""
    rng = np.random.default_rng(19)
    n, nt, off = 2053, 9, 4
    progs = [random_program(rng, 8) for _ in range(nt)]
    data = [[po.fill(n, "f32", 0, 7, 8 * t + j) for j in range(8)] for t in range(nt)]
    leaves = [[fu.Guarded(n * 4, off, key=100 + 8 * t + j).load(x) for j, x in enumerate(row)]
              for t, row in enumerate(data)]
    outs = [fu.Guarded(n * 4, off, key=900 + t) for t in range(nt)]
    snaps = [[g.snapshot() for g in row] for row in leaves]
    rc = ca.reduce_tree_batch([o.ptr for o in outs], [[g.ptr for g in row] for row in leaves], [p[0] for p in progs],
                              [p[1] for p in progs], n, ca.FLOAT32, ca.SUM, gu.stream())
    gu.sync()
    bad = []
    for t in range(nt):
        watched = [(f"leaf {j}", g, snaps[t][j]) for j, g in enumerate(leaves[t])]
        ref = tree_ref(data[t], progs[t][0], progs[t][1], "f32", "sum")
        bad += [f"tree {t}: {p}" for p in _verdict(rc, outs[t], outs[t].read(np.float32), ref, watched)]
    assert not bad, bad[:4]


def test_trees_packed_back_to_back_footprint(gu):
    """The executor's layout: a slice's chunks lie back to back, so one tree's overrun is the next chunk's data.
    Three trees of n = 4099 f32 share one allocation for their outputs and one per leaf index for their leaves:
    their 16-byte phases are 0, 12 and 8, each with its own head and tail.  All three results bit-exact (nothing
    rewrites a neighbour's overrun here), the outer guards intact, every leaf unchanged."""
    rng = np.random.default_rng(23)
    n, nt = 4099, 3
    assert [(t * n * 4) % 16 for t in range(nt)] == [0, 12, 8]
    progs = [C4_TREE, K2B8_TREE, random_program(rng, 8)]
    data = [[po.fill(n, "f32", 0, 9, 8 * t + j) for j in range(8)] for t in range(nt)]
    leaves = [fu.Guarded(nt * n * 4, 0, key=200 + j).load(np.concatenate([data[t][j] for t in range(nt)]))
              for j in range(8)]
    out = fu.Guarded(nt * n * 4, 0, key=299)
    stamp = out.read(np.uint8).copy()
    snaps = [g.snapshot() for g in leaves]
    rc = ca.reduce_tree_batch([out.ptr + t * n * 4 for t in range(nt)],
                              [[g.ptr + t * n * 4 for g in leaves] for t in range(nt)], [p[0] for p in progs],
                              [p[1] for p in progs], n, ca.FLOAT32, ca.SUM, gu.stream())
    gu.sync()
    ref = np.concatenate([tree_ref(data[t], progs[t][0], progs[t][1], "f32", "sum") for t in range(nt)])
    bad = _verdict(rc, out, out.read(np.float32), ref, [(f"leaves {j}", g, snaps[j]) for j, g in enumerate(leaves)])
    assert not bad, bad[:4]
    # and one tree alone writes its own chunk only: the neighbours' bytes keep the stamp
    out.reset()
    rc = ca.reduce_tree(out.ptr + n * 4, [g.ptr + n * 4 for g in leaves], progs[1][0], progs[1][1], n, ca.FLOAT32,
                        ca.SUM, gu.stream())
    gu.sync()
    got = out.read(np.uint8)
    assert rc == 0 and out.guards_intact(), repr(out.guards_intact())
    assert np.array_equal(got[:n * 4], stamp[:n * 4]) and np.array_equal(got[2 * n * 4:], stamp[2 * n * 4:])
    assert np.array_equal(got[n * 4:2 * n * 4].view(np.uint32), ref[n:2 * n].view(np.uint32))


# ---- user-op launchers (include/chiara_user_op.hpp) ---------------------------------------------------------------

USER_DT = {"f32": ca.FLOAT32, "f64": ca.FLOAT64, "i32": ca.INT32}
OPN = "user_halfadd"


@pytest.fixture(scope="module")
def fold_op():
    so = os.path.join(HERE, "userop", "libhalfadd_op.so")
    assert os.path.exists(so), f"{so} missing: make -C tests/userop (__graft_entry__.build())"
    lib = ctypes.CDLL(so)
    op = ca.op_create(ctypes.cast(lib.chr_test_halfadd, ctypes.c_void_p).value)
    yield op
    assert ca.op_free(op) == 0


@pytest.fixture(scope="module")
def tree_op():
    from test_gpu_user_tree import Op

    o = Op()
    yield o
    assert ca.op_free(o.tree) == 0 and ca.op_free(o.decline) == 0


@pytest.mark.parametrize("dt", ["f32", "f64", "i32"])
def test_user_fold_launcher_footprint(gu, fold_op, dt):
    """k_fold through chr_reduce_multi with a user op: its chunks of kU x 256 = 1024 vectors (one element either side
    of one, two whole ones, two and a partial one with an element tail), fewer elements than a vector, and calls
    whose operands are off a 16-byte boundary -- all of them, or one input only -- which run element by element;
    m = 1 and 3, out separate and out == acc."""
    es, npdt = _es(dt), po.NP_DTYPES[dt]
    E, C = 16 // es, 1024 * (16 // es)
    aligned = [1, E - 1, E, C - 1, C, C + 1, 2 * C, 2 * C + 5 * E + (E - 1)]
    cases = [(alias, m, 0, 0, n) for alias in (True, False) for m in (1, 3) for n in aligned]
    cases += [(alias, m, es, es, n) for alias in (True, False) for m in (1, 3) for n in (257, C + 1)]
    cases += [(alias, 3, 0, es, n) for alias in (True, False) for n in (257, C + 1)]
    nmax = max(c[4] for c in cases)
    pool = Pool(nmax * es)
    data = [po.fill(nmax, dt, po.PAT_UNIFORM, 51, r) for r in range(4)]
    refs, bad = {}, []
    for alias, m, po_, pi_, n in cases:
        acc_np, ins_np = data[0][:n], [x[:n] for x in data[1:m + 1]]
        if (m, n) not in refs:
            refs[(m, n)] = po.reduce_multi(acc_np.copy(), ins_np, dt, OPN)
        out = pool.get("out", po_, n * es)
        acc = (out if alias else pool.get("acc", po_, n * es)).load(acc_np)
        ins = [pool.get(f"in{j}", pi_ if j == 0 else po_, n * es).load(x) for j, x in enumerate(ins_np)]
        watched = [(f"ins[{j}]", g, g.snapshot()) for j, g in enumerate(ins)]
        if not alias:
            watched.append(("acc", acc, acc.snapshot()))
        rc = ca.reduce_multi(out.ptr, acc.ptr, [g.ptr for g in ins], n, USER_DT[dt], fold_op, gu.stream())
        gu.sync()
        for p in _verdict(rc, out, out.read(npdt), refs[(m, n)], watched):
            bad.append(f"{'in place' if alias else 'out of place'} m={m} phases={po_}/{pi_} n={n}: {p}")
    assert len(cases) == 2 * 2 * 8 + 2 * 2 * 2 + 2 * 2
    assert not bad, f"{len(bad)} problems, e.g. {bad[:4]}"


@pytest.mark.parametrize("dt", ["f32", "f64", "i32"])
def test_user_tree_launcher_footprint(gu, tree_op, dt):
    """k_tree through chr_reduce_tree with a tree op: trips of 64 x U vectors for 8 leaves (U = 1) and 2 leaves
    (U = 4) -- whole trips, one element either side, the partial trip, the element tail, more than one span of XCD
    runs (8 x 256 KiB per leaf) with a ragged end -- and a tree with one leaf off a boundary, element by element, at
    257 elements and past the 4096 workgroups an element-wise tree strides over; out separate, over leaf 0 and over
    the last leaf.  The host-side counters show that the tree launcher took every case (one call, one tree, no fold)."""
    es, npdt = _es(dt), po.NP_DTYPES[dt]
    E = 16 // es
    swap8 = ([0, 1, 1, 1, 0, 1, 1, 2], [1, 0, 1, 0, 1, 0, 1])
    progs = [(C4_TREE, 64), (swap8, 64), (([0, 1], [1]), 256)]
    cases = []
    for pi, (_, tv) in enumerate(progs):
        TE = tv * E
        for n in (1, E - 1, TE - 1, TE, TE + 1, (2 * tv + 1) * E + 5 * E + (E - 1)):
            cases += [(pi, into, 0, n) for into in (None, 0, -1)]
    span = 8 * (256 << 10) // 16  # vectors per leaf in one span of 8 XCD runs
    cases += [(0, into, 0, (span + 64 * 37 + 5) * E + (E - 1)) for into in (None, 0)]
    cases += [(pi, into, es, n) for pi in (0, 2) for into in (None, 0) for n in (257, 4096 * 64 + 77)]
    nmax = max(c[3] for c in cases)
    pool = Pool(nmax * es)
    data = [po.fill(nmax, dt, po.PAT_UNIFORM, 61, r) for r in range(8)]
    refs, bad = {}, []
    for pi, into, shift, n in cases:
        comb, swaps = progs[pi][0]
        nl = len(comb)
        into = nl - 1 if into == -1 else into
        lv_np = [x[:n] for x in data[:nl]]
        if (pi, n) not in refs:
            refs[(pi, n)] = tree_ref(lv_np, comb, swaps, dt, OPN)
        off_leaf = nl // 2 if shift else None  # this leaf alone sits one element off a 16-byte boundary
        leaves = [pool.get("out" if j == into else f"leaf{j}", shift if j == off_leaf else 0, n * es).load(x)
                  for j, x in enumerate(lv_np)]
        out = pool.get("out", 0, n * es) if into is None else leaves[into]
        watched = [(f"leaf {j}", g, g.snapshot()) for j, g in enumerate(leaves) if j != into]
        tree_op.reset()
        rc = ca.reduce_tree(out.ptr, [g.ptr for g in leaves], comb, swaps, n, USER_DT[dt], tree_op.tree, gu.stream())
        gu.sync()
        what = f"program {pi} out={'separate' if into is None else f'leaf {into}'} shift={shift} n={n}"
        if tree_op.counters()[:3] != (0, 1, 1):
            bad.append(f"{what}: launcher calls {tree_op.counters()}")
        bad += [f"{what}: {p}" for p in _verdict(rc, out, out.read(npdt), refs[(pi, n)], watched)]
    assert len(cases) == 3 * 6 * 3 + 2 + 2 * 2 * 2
    assert not bad, f"{len(bad)} problems, e.g. {bad[:4]}"


# ---- chr_fill ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["u8", "bf16", "f64", "di"])
def test_fill_footprint(gu, dtype):
    """k_fill is grid-stride over at most 8192 workgroups of 256: one element, one either side of a workgroup, and
    one element past the capped grid's first round."""
    es, npdt = _es(dtype), po.NP_DTYPES[dtype]
    ns = (1, 255, 256, 257, 8192 * 256 + 1)
    g = fu.Guarded(0, 0, capacity=ns[-1] * es, key=77)
    for n in ns:
        g.reset(n * es)
        rc = ca.fill(g.ptr, n, DT[dtype], po.PAT_UNIFORM, 0xC41A5EED, 5, stream=gu.stream())
        gu.sync()
        bad = _verdict(rc, g, g.read(npdt), po.fill(n, dtype, po.PAT_UNIFORM, 0xC41A5EED, 5), [])
        assert not bad, (n, bad)


# ---- streaming shapes: XCD map, handover, launch pieces --------------------------------------------------------------

CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [{here!r}, {oracle!r}, {pkg!r}]
import chiara_amd as ca
import footprint_util as fu
import gpu_util as gu
import pyoracle as po
from tree_util import tree_ref

bad, ran = [], 0
def verdict(what, rc, out, ref, watched):
    global ran
    ran += 1
    if rc:
        bad.append(f"{{what}}: rc = {{rc}}")
    if not np.array_equal(out.read(np.uint32), ref.view(np.uint32)):
        bad.append(f"{{what}}: result != oracle")
    chk = out.guards_intact()
    if not chk:
        bad.append(f"{{what}}: out {{chk!r}}")
    for name, g, snap in watched:
        chk = g.unchanged_since(snap)
        if not chk:
            bad.append(f"{{what}}: {{name}} {{chk!r}}")

NS = (4096 * 8 * 3 + 17, 100003, (1 << 20) + 4 * 64 * 3 + 4, 1 << 21)
CAP = max(NS) * 4
# the outputs take a guard as large as the payload (fu.stream_guard): all that the grid's surplus workgroups reach
outs = [fu.Guarded(0, 0, hi_guard=CAP, capacity=CAP, key=1000 + j) for j in range(3)]
ins = [fu.Guarded(0, 0, capacity=CAP, key=2000 + j) for j in range(8)]

# bucket kernel: m = 1 (U = 4, 4 KiB trips), 3 (U = 2) and 7 (U = 1), in place and out of place
data = [po.fill(max(NS), "f32", 0, 11, r) for r in range(8)]
for m in (1, 3, 7):
    for n in NS:
        ref = po.reduce_multi(data[0][:n].copy(), [x[:n] for x in data[1:m + 1]], "f32", "sum")
        for alias in (True, False):
            out = outs[0].reset(n * 4)
            acc = (out if alias else ins[7].reset(n * 4)).load(data[0][:n])
            xs = [ins[j].reset(n * 4).load(data[j + 1][:n]) for j in range(m)]
            watched = [(f"ins[{{j}}]", g, g.snapshot()) for j, g in enumerate(xs)]
            if not alias:
                watched.append(("acc", acc, acc.snapshot()))
            rc = ca.reduce_multi(out.ptr, acc.ptr, [g.ptr for g in xs], n, ca.FLOAT32, ca.SUM, gu.stream())
            gu.sync()
            verdict(f"bucket m={{m}} n={{n}} {{'in place' if alias else 'out of place'}}", rc, out, ref, watched)

# batched trees: 3 trees of 8 leaves (left folds) and of 3 leaves, ragged lengths
for nl in (3, 8):
    for n in (100003, (1 << 19) + 7):
        trees = [[po.fill(n, "f32", 0, 23 + t, j) for j in range(nl)] for t in range(3)]
        lv = [[fu.Guarded(n * 4, 0, key=3000 + 8 * t + j).load(x) for j, x in enumerate(tr)]
              for t, tr in enumerate(trees)]
        snaps = [[g.snapshot() for g in row] for row in lv]
        for o in outs:
            o.reset(n * 4)
        comb = [[0] + [1] * (nl - 1)] * 3
        rc = ca.reduce_tree_batch([o.ptr for o in outs], [[g.ptr for g in row] for row in lv], comb, None, n,
                                  ca.FLOAT32, ca.SUM, gu.stream())
        gu.sync()
        for t, tr in enumerate(trees):
            ref = po.reduce_multi(tr[0].copy(), tr[1:], "f32", "sum")
            verdict(f"trees nl={{nl}} n={{n}} tree {{t}}", rc, outs[t], ref,
                    [(f"leaf {{j}}", g, snaps[t][j]) for j, g in enumerate(lv[t])])
        del lv, snaps

# the 2-leaf tree: a streaming one is the bucket kernel out of place (reduce_tree.hip), both operand orders, unless
# out is the fold's input (the tree kernel); TIES data and MAX, so the order shows
for n in (100003, (1 << 20) + 4 * 64 * 3 + 4):
    a, b = po.fill(n, "f32", 2, 31, 0), po.fill(n, "f32", 2, 31, 1)
    for sw in (0, 1):
        ref = tree_ref([a, b], [0, 1], [sw], "f32", "max")
        for into in (None, 0, 1):
            lv = [(outs[0] if into == j else ins[j]).reset(n * 4).load(x) for j, x in enumerate((a, b))]
            out = outs[0].reset(n * 4) if into is None else lv[into]
            watched = [(f"leaf {{j}}", g, g.snapshot()) for j, g in enumerate(lv) if j != into]
            rc = ca.reduce_tree(out.ptr, [g.ptr for g in lv], [0, 1], [sw], n, ca.FLOAT32, ca.MAX, gu.stream())
            gu.sync()
            verdict(f"2-leaf n={{n}} swap={{sw}} out={{into}}", rc, out, ref, watched)
print(json.dumps({{"bad": bad[:20], "nbad": len(bad), "ran": ran}}))
"""
CHILD_CASES = 3 * 4 * 2 + 2 * 2 * 3 + 2 * 2 * 3


def test_streaming_shapes_footprint():
    """The streaming (nt) shapes under every XCD configuration of test_gpu_xcd_map.py -- run lengths, launch pieces of
    3000 vectors with a partial trip in each, handovers of up to half an odd XCD's share -- each in a fresh child
    process (the tuning variables are read once per process), the seven children at once.  The grid of such a launch
    holds `trips + 8 * hand` workgroups and the surplus ones must idle: the outputs' upper guards are as large as
    the payload.  Bucket kernel f32, m = 1, 3, 7, in place and out of place at that file's four counts; its batched
    trees with every leaf snapshotted; the 2-leaf tree with both swap bits into a separate buffer and into either
    leaf.  CHR_REDUCE_NT_MIN_BYTES = 1 makes the 2-leaf tree of these sizes the streaming one that takes the bucket
    kernel out of place (CHR_REDUCE_NT alone forces the nt shapes but leaves that threshold at 40 MiB)."""
    assert len(XCD_CONFIGS) <= 7 and {(4, 0, -1), (8, 3000, -1), (0, 0, 2), (4, 3000, 3)} <= set(XCD_CONFIGS)
    code = CHILD.format(here=HERE, oracle=os.path.join(REPO, "oracle"),
                        pkg=os.path.join(REPO, "configurable-hierarchical-allreduce-algorithms_amd"))
    procs = []
    for run_kib, max_vec, hand_shift in XCD_CONFIGS:
        env = dict(os.environ, CHR_REDUCE_NT="1", CHR_REDUCE_NT_MIN_BYTES="1", CHR_XCD_RUN_KIB=str(run_kib),
                   CHR_REDUCE_MAX_LAUNCH_VEC=str(max_vec))
        if hand_shift >= 0:
            env["CHR_XCD_HAND_SHIFT"] = str(hand_shift)
        procs.append(subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    failures = []
    for cfg, p in zip(XCD_CONFIGS, procs):
        try:
            out, err = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            out, err = p.communicate()
            failures.append((cfg, "timeout"))
            continue
        if p.returncode != 0:
            failures.append((cfg, err[-3000:]))
            continue
        res = json.loads(out.strip().splitlines()[-1])
        if res["bad"] or res["ran"] != CHILD_CASES:
            failures.append((cfg, res["ran"], res["nbad"], res["bad"][:10]))
    assert not failures, failures


# ---- collectives through LocalGroup ---------------------------------------------------------------------------

SCHED = {"flat": ca.SCHEDULE_FLAT, "exact": ca.SCHEDULE_EXACT, "flat_1shot": ca.SCHEDULE_FLAT_1SHOT}
MPICH_MODE = {"ring": ca.MODE_MPICH_RING, "rd": ca.MODE_MPICH_RD, "rsag": ca.MODE_MPICH_RSAG,
              "rx": ca.MODE_MPICH_RECEXCH, "krsag": ca.MODE_MPICH_KRSAG, "rm": ca.MODE_MPICH_RMULT}
RS_MODE = {"rs_radix": ca.MODE_MPICH_RS_RADIX, "rs_halving": ca.MODE_MPICH_RS_HALVING,
           "rs_doubling": ca.MODE_MPICH_RS_DOUBLING, "rs_pairwise": ca.MODE_MPICH_RS_PAIRWISE}
PHASE_MODE = {"irs": ca.MODE_INTRA_REDUCE_SCATTER, "ilr": ca.MODE_INTER_REDUCE_LINEAR, "isc": ca.MODE_INTRA_SCATTER}


def _manifest(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)["cases"]


def _radix_cases():
    """The first case of every distinct (mode, n, k, b) with n <= 8, and its first in-place case where it has one."""
    first, inplace = {}, {}
    for c in _manifest("manifest.json"):
        key = (c["mode"], c["n"], c["k"], c["b"])
        if c["n"] > 8:
            continue
        first.setdefault(key, c)
        if c["inplace"]:
            inplace.setdefault(key, c)
    return list(first.values()) + [c for k, c in inplace.items() if first[k] is not c]


def _baseline_cases(name):
    """Per algorithm (phase function) of a baseline manifest: its 8-rank out-of-place case with the most elements,
    and its first 8-rank in-place case where it has one."""
    by = {}
    for c in _manifest(name):
        if c["n"] == 8:
            by.setdefault(c["mode"], []).append(c)
    out = []
    for mode, cs in by.items():
        oop = [c for c in cs if not c["inplace"]]
        out.append(max(oop, key=lambda c: c["count"]))
        out += [c for c in cs if c["inplace"]][:1]
    return out


RADIX = _radix_cases()


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


@pytest.fixture(scope="module")
def rank_pool():
    return Pool(64 << 10)


def _collective_case(gu, g, c, pool):
    """One golden case with every rank's buffers guarded: the problems found."""
    mode, n, cnt, dtype = c["mode"], c["n"], c["count"], c["dtype"]
    es = _es(dtype)
    k, b = c["k"], c["b"]
    if mode in PHASE_MODE:
        send_n, recv_n = po.phase_sizes(mode, n, b, cnt)
    elif mode == "rs" or mode in RS_MODE:
        send_n, recv_n = cnt * n, cnt
    elif mode == "ag":
        send_n, recv_n = cnt, cnt * n
    else:
        send_n = recv_n = cnt
    sends = [po.fill(send_n, dtype, c["pattern"], c["seed"], r) for r in range(n)]
    inplace = bool(c["inplace"])
    recv, watched = [], []
    for r in range(n):
        if not inplace:
            recv.append(pool.get(f"recv{r}", 0, recv_n * es).load(np.zeros(recv_n * es, np.uint8)))
        elif mode == "ag":  # the own block already in place, the others to be received
            own = np.zeros((n, cnt * es), np.uint8)
            own[r] = sends[r].view(np.uint8)
            recv.append(pool.get(f"recv{r}", 0, recv_n * es).load(own))
        else:  # recv holds the input: for a reduce-scatter all n * recvcount elements of it
            recv.append(pool.get(f"recv{r}", 0, send_n * es).load(sends[r]))
    if inplace:
        S = [ca.IN_PLACE] * n
    else:
        send = [pool.get(f"send{r}", 0, send_n * es).load(sends[r]) for r in range(n)]
        watched = [(f"rank {r} send", s, s.snapshot()) for r, s in enumerate(send)]
        S = [s.ptr for s in send]
    R = [x.ptr for x in recv]
    gu.sync()
    if mode == "ar":
        rc = g.all_reduce_radix_batch(S, R, cnt, DT[dtype], OP[c["op"]], k, b)
    elif mode == "rs":
        rc = g.reduce_scatter_radix_batch(S, R, cnt, DT[dtype], OP[c["op"]], k, b)
    elif mode == "ag":
        rc = g.allgather_radix_batch(S, cnt, DT[dtype], R, k, b)
    elif mode in MPICH_MODE:
        rc = g.allreduce_mpich(MPICH_MODE[mode], S, R, cnt, DT[dtype], OP[c["op"]], k, b)
    elif mode in RS_MODE:
        rc = g.reduce_scatter_mpich(RS_MODE[mode], S, R, cnt, DT[dtype], OP[c["op"]], k)
    else:
        rc = g.phase_collective(PHASE_MODE[mode], S, R, cnt, DT[dtype], OP[c["op"]], k or 2, b)
    gu.sync()
    bad = [] if rc == 0 else [f"rc = {rc}"]
    # an in-place reduce-scatter leaves recv[recvcount, n * recvcount) unspecified (MPI): only the result is hashed
    # and only the guards around the whole input are checked
    outs = [x.read(np.uint8)[:recv_n * es] for x in recv]
    if hashlib.sha256(b"".join(o.tobytes() for o in outs)).hexdigest() != c["sha256"]:
        bad.append("result != the reference's golden hash")
    for r, x in enumerate(recv):
        chk = x.guards_intact()
        if not chk:
            bad.append(f"rank {r} recv {chk!r}")
    for name, s, snap in watched:
        chk = s.unchanged_since(snap)
        if not chk:
            bad.append(f"{name} {chk!r}")
    return [f"{c['id']}: {p}" for p in bad]


def test_collective_case_selection():
    keys = {(c["mode"], c["n"], c["k"], c["b"]) for c in RADIX}
    assert len(keys) == 147 and sum(not c["inplace"] for c in RADIX) == 147 and sum(c["inplace"] for c in RADIX) == 72
    assert {c["mode"] for c in RADIX} == {"ar", "rs", "ag"} and max(c["n"] for c in RADIX) == 8
    assert sorted(c["mode"] for c in _baseline_cases("mpich_manifest.json") if not c["inplace"]) == sorted(MPICH_MODE)
    assert sorted(c["mode"] for c in _baseline_cases("rsmpich_manifest.json") if not c["inplace"]) == sorted(RS_MODE)
    assert sorted(c["mode"] for c in _baseline_cases("phases_manifest.json") if not c["inplace"]) == sorted(PHASE_MODE)


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("schedule", ["flat", "exact", "flat_1shot"])
def test_radix_batch_collectives_footprint(gu, groups, rank_pool, schedule, slices):
    """The allreduce and the reduce-scatter on the reference's golden cases (the first of every (mode, n, k, b) with
    n <= 8, and the first in-place one), under the flat, exact and one-shot schedules at pipeline depths 1 and 3: out
    of place every rank's send buffer is byte-identical afterwards and its recv buffer hashes to the reference's
    value between intact guards; in place the guards around recv are intact and the hash matches."""
    bad, ran = [], 0
    for c in RADIX:
        if c["mode"] == "ag":
            continue
        g = groups(c["n"])
        g.set_schedule(SCHED[schedule])
        g.set_slices(slices)
        try:
            bad += _collective_case(gu, g, c, rank_pool)
            ran += 1
        finally:
            g.set_schedule(ca.SCHEDULE_FLAT)
            g.set_slices(1)
    assert ran == 2 * 49 + sum(c["inplace"] and c["mode"] != "ag" for c in RADIX)
    assert not bad, f"{len(bad)} problems, e.g. {bad[:4]}"


def test_allgather_and_baseline_collectives_footprint(gu, groups, rank_pool):
    """The allgather on its golden cases (pure data movement: one plan), and one 8-rank case -- the largest -- plus an
    in-place one per MPICH allreduce baseline, per MPICH reduce-scatter baseline and per stand-alone phase."""
    cases = [c for c in RADIX if c["mode"] == "ag"]
    cases += _baseline_cases("mpich_manifest.json") + _baseline_cases("rsmpich_manifest.json")
    cases += _baseline_cases("phases_manifest.json")
    bad = []
    for c in cases:
        bad += _collective_case(gu, groups(c["n"]), c, rank_pool)
    assert len(cases) >= 49 + 6 + 4 + 3
    assert not bad, f"{len(bad)} problems, e.g. {bad[:4]}"
