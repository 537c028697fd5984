"""Every launch path of the kernel boundary behind the gate of tests/stream_util.py: the call is handed a non-blocking
stream S whose queue is still busy with the gate's copy, the true operands arrive on S after the gate, and the host
waits for S alone.  A launch (or hipMemcpyAsync, or stream-ordered allocation) that left S shows as wrong bits, a call
that waited as a completed gate.  Expected bits: pyoracle, tree_util.tree_ref, struct_ref, f16_ref -- bit for bit.

Shapes, the smallest that split into every kind of launch:
  bucket  n = 4 * (2 * 1024 + 300) + 8 with every operand SHIFT bytes into a 16-byte aligned allocation (congruent: a
          scalar head, a vector body, a scalar tail), and the same n with `out` alone shifted (the scalar kernel);
          m = 0 (out of place: hipMemcpyAsync), 1, 8, 17 (three chained groups that continue from `out`); in place
          and out of place; one (type, op) per translation unit.  SHIFT is 4 bytes, and 8 for the types of 8 and 16
          bytes, whose elements cannot start 4 bytes in (reduce_common.hpp align_split: an offset that is no multiple
          of the element size is not congruent, and MPI's types are naturally aligned).
  tree    n = 8 * (3 * 256 + 70) + 5 with every leaf and the root SHIFT bytes in (scalar head and tail launched before
          the vector body is flushed), one type per tree unit.
  batch   chr_reduce_tree_batch takes one leaf count per call, so "9 eight-leaf trees mixed with 3-leaf ones" is two
          calls back to back in one gated sequence: streaming_cases.batch_programs() (two flushes: 8 segments and 1)
          and three 3-leaf trees whose leaves are the nine roots just written.  (Mixed leaf counts inside one launch
          list happen in the executors: the local-group tests below.)
The forced shapes (several launch pieces and tree segments per call at these n) run in one child process: this
module's own __main__, with test_gpu_fuzz.py's environment."""
import collections
import ctypes
import functools
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if __name__ == "__main__":  # the child: the paths conftest.py gives the parent
    for _p in (HERE, os.path.join(REPO, "oracle"), os.path.join(REPO, "configurable-hierarchical-allreduce-algorithms_amd")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import pytest  # noqa: E402

import chiara_amd as ca  # noqa: E402
import pyoracle as po  # noqa: E402
from streaming_cases import STATIC_PROGS, batch_programs  # noqa: E402
from test_gpu_dispatch_sweep import pattern_for  # noqa: E402
from test_gpu_kernels import DT, OP, _bytes_copy  # noqa: E402
from tree_util import random_program, tree_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SEED_TRUE, SEED_STALE = 5, 905
N_BUCKET = 4 * (2 * 1024 + 300) + 8
N_TREE = 8 * (3 * 256 + 70) + 5
STREAM_BYTES = 16 << 20  # per operand: m = 1 is 48 MiB per call, above nt_min_bytes (40 MiB)
FORCED_ENV = {"CHR_REDUCE_NT": "1", "CHR_REDUCE_MAX_LAUNCH_VEC": "2048", "CHR_XCD_RUN_KIB": "4"}  # test_gpu_fuzz.py's
C4 = [0, 1, 1, 1, 0, 1, 1, 2]
C4_SWAPS = [1, 0, 1, 0, 1, 0, 1]


def esize(dtype):
    return np.dtype(po.NP_DTYPES[dtype]).itemsize


def shift(dtype):
    """4 bytes in; the types of 8 and 16 bytes (aligned to 8) cannot start there: 8."""
    return max(4, min(esize(dtype), 8))


@functools.lru_cache(maxsize=None)
def operands(dtype, pattern, n, seed, count=18):
    xs = [po.fill(n, dtype, pattern, seed, r) for r in range(count)]
    for x in xs:
        x.flags.writeable = False
    return xs


def fold_ref(dtype, op, acc, ins, running_first):
    if not running_first:
        return po.reduce_multi(_bytes_copy(acc), [_bytes_copy(x) for x in ins], dtype, op)
    run = _bytes_copy(acc)  # test_gpu_kernels.test_reduce_multi_running_first's chain
    for x in ins:
        nxt = _bytes_copy(x)
        po.reduce_local(run, nxt, dtype, op)
        run = nxt
    return run


# ---- the case lists -----------------------------------------------------------------------------------------------

# layout: "in" every operand and the output SHIFT bytes in; "out" the output alone; "aligned" none
Fold = collections.namedtuple("Fold", "dtype op m layout inplace running_first n entry")
Tree = collections.namedtuple("Tree", "dtype op comb swaps n layout alias")

FOLD_PAIRS = [("f32", "sum"), ("bf16", "max"),   # reduce_kernels.hip (core)
              ("u8", "bxor"), ("i64", "prod"),   # reduce_int.hip
              ("fi", "maxloc"), ("cf", "prod")]  # reduce_pair.hip
TREE_PAIRS = [("f32", "sum"), ("i16", "min"), ("u64", "sum"), ("di", "maxloc"), ("cd", "sum")]  # one per tree unit


def fold_cases(dtype, op):
    return [Fold(dtype, op, m, layout, inplace, False, N_BUCKET, "multi")
            for layout in ("in", "out") for m in (0, 1, 8, 17) for inplace in (True, False)]


def extra_fold_cases():
    nstream = STREAM_BYTES // 4
    return [Fold("f32", "max", 3, "in", False, True, N_BUCKET, "multi"),       # CHR_REDUCE_RUNNING_FIRST
            Fold("f32", "sum", 1, "aligned", False, False, nstream, "multi"),  # the streaming shape at its threshold
            Fold("f32", "sum", 1, "aligned", True, False, nstream, "multi"),
            Fold("f32", "sum", 1, "in", True, False, N_BUCKET, "local")]       # chr_reduce_local


def _non_static(nl, seed):
    rng = np.random.default_rng(seed)
    while True:
        comb, swaps = random_program(rng, nl)
        if comb not in STATIC_PROGS.get(nl, []):
            return comb, swaps


def tree_cases(dtype, op):
    comb, swaps = _non_static(8, 31)  # runs on the interpreter kernel
    return [Tree(dtype, op, C4, C4_SWAPS, N_TREE, "in", None),
            Tree(dtype, op, comb, swaps, N_TREE, "in", None),
            Tree(dtype, op, C4, C4_SWAPS, N_TREE, "in", 0),   # the root over leaf 0
            Tree(dtype, op, C4, C4_SWAPS, N_TREE, "in", 7),   # the root over the last leaf
            Tree(dtype, op, [0], [], N_TREE, "in", None)]     # one leaf: a copy


def extra_tree_cases():
    return [Tree("f32", "sum", [0, 1], [0], STREAM_BYTES // 4, "aligned", None)]  # folds on the bucket kernel


def what_of(c):
    d = c._asdict()
    return type(c).__name__ + " " + " ".join(f"{k}={v}" for k, v in d.items())


# ---- building a gated case ------------------------------------------------------------------------------------------

def build_fold(su, c):
    pat = pattern_for(c.op)
    cnt = 18 if c.n <= N_BUCKET else c.m + 1  # the 16 MiB operands: only those the case reads
    true, stale = operands(c.dtype, pat, c.n, SEED_TRUE, cnt), operands(c.dtype, pat, c.n, SEED_STALE, cnt)
    case = su.Case(what_of(c))
    sh = shift(c.dtype)
    o_ops = sh if c.layout == "in" else 0
    o_out = 0 if c.layout == "aligned" else sh
    if c.inplace:
        acc = out = case.operand(true[0], stale[0], o_out)
    else:
        acc = case.operand(true[0], stale[0], o_ops)
        out = case.output(true[0].nbytes, o_out)
    ins = [case.operand(true[j + 1], stale[j + 1], o_ops) for j in range(c.m)]
    case.expect(out, fold_ref(c.dtype, c.op, true[0], true[1:1 + c.m], c.running_first))
    ptrs = [x.ptr for x in ins]
    if c.entry == "local":
        assert c.m == 1 and c.inplace
        return case, lambda h: ca.reduce_local(ptrs[0], acc.ptr, c.n, DT[c.dtype], OP[c.op], h)
    if c.running_first:
        return case, lambda h: ca.reduce_multi_ex(out.ptr, acc.ptr, ptrs, c.n, DT[c.dtype], OP[c.op],
                                                  ca.REDUCE_RUNNING_FIRST, h)
    return case, lambda h: ca.reduce_multi(out.ptr, acc.ptr, ptrs, c.n, DT[c.dtype], OP[c.op], h)


def build_tree(su, c):
    pat = pattern_for(c.op)
    nl = len(c.comb)
    cnt = 18 if c.n <= N_BUCKET else nl
    true, stale = operands(c.dtype, pat, c.n, SEED_TRUE, cnt)[:nl], operands(c.dtype, pat, c.n, SEED_STALE, cnt)[:nl]
    case = su.Case(what_of(c))
    off = shift(c.dtype) if c.layout == "in" else 0
    leaves = [case.operand(true[j], stale[j], off) for j in range(nl)]
    out = case.output(true[0].nbytes, off) if c.alias is None else leaves[c.alias]
    case.expect(out, tree_ref(list(true), c.comb, c.swaps, c.dtype, c.op))
    ptrs = [x.ptr for x in leaves]
    return case, lambda h: ca.reduce_tree(out.ptr, ptrs, c.comb, c.swaps, c.n, DT[c.dtype], OP[c.op], h)


def build_batch(su):
    """batch_programs()'s nine 8-leaf trees, then three 3-leaf trees over the nine roots: two calls, one sequence."""
    dtype, op, n = "f32", "sum", N_TREE
    true, stale = operands(dtype, 0, n, SEED_TRUE)[:9], operands(dtype, 0, n, SEED_STALE)[:9]
    case = su.Case("batch of 9 eight-leaf trees, then 3 three-leaf trees over their roots")
    off = shift(dtype)
    d = [case.operand(true[j], stale[j], off) for j in range(9)]
    progs = batch_programs()
    roots = [case.output(true[0].nbytes, off) for _ in progs]
    tops = [case.output(true[0].nbytes, off) for _ in range(3)]
    rows = [[d[(t + j) % 9].ptr for j in range(8)] for t in range(9)]
    root_ref = [tree_ref([true[(t + j) % 9] for j in range(8)], comb, swaps, dtype, op)
                for t, (comb, swaps) in enumerate(progs)]
    prog3 = [([0, 1, 1], [0, 1]), ([0, 0, 2], [1, 0]), ([0, 1, 1], [1, 1])]
    for t in range(9):
        case.expect(roots[t], root_ref[t])
    for u, (comb, swaps) in enumerate(prog3):
        case.expect(tops[u], tree_ref(root_ref[3 * u:3 * u + 3], comb, swaps, dtype, op))

    def call(h):
        rc = ca.reduce_tree_batch([r.ptr for r in roots], rows, [p[0] for p in progs], [p[1] for p in progs], n,
                                  DT[dtype], OP[op], h)
        return rc or ca.reduce_tree_batch([x.ptr for x in tops], [[r.ptr for r in roots[3 * u:3 * u + 3]] for u in range(3)],
                                          [p[0] for p in prog3], [p[1] for p in prog3], n, DT[dtype], OP[op], h)

    return case, call


def run_case(su, gate, stream, c):
    case, call = build_batch(su) if c == "batch" else (build_fold if isinstance(c, Fold) else build_tree)(su, c)
    return su.run_gated(case, call, gate, stream)


def all_builtin_cases():
    out = []
    for dtype, op in FOLD_PAIRS:
        out += fold_cases(dtype, op)
    out += extra_fold_cases()
    for dtype, op in TREE_PAIRS:
        out += tree_cases(dtype, op)
    return out + extra_tree_cases() + ["batch"]


# ---- fixtures -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def su():
    import stream_util

    return stream_util


@pytest.fixture(scope="module")
def gate(su):
    return su.shared_gate()


@pytest.fixture(scope="module")
def S(su):
    return su.nonblocking_stream()


def _check_all(su, gate, S, cases):
    bad = []
    for c in cases:
        v = run_case(su, gate, S, c).verdict()
        if v is not None:
            bad.append(v)
    assert not bad, f"{len(bad)} of {len(cases)} cases: " + " | ".join(bad[:4])


# ---- the bucket kernel ------------------------------------------------------------------------------------------------

def test_the_stream_is_non_blocking_and_the_null_stream_is_not(su, S):
    assert su.is_nonblocking(S.cuda_stream)
    assert not su.is_nonblocking(0)


@pytest.mark.parametrize("dtype,op", FOLD_PAIRS)
def test_bucket_folds_are_ordered_on_their_stream(su, gate, S, dtype, op):
    """Head / body / tail and the scalar kernel alone, m = 0, 1, 8, 17, in place and out of place."""
    _check_all(su, gate, S, fold_cases(dtype, op))


def test_running_first_streaming_and_reduce_local(su, gate, S):
    _check_all(su, gate, S, extra_fold_cases())


# ---- the tree kernel ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,op", TREE_PAIRS)
def test_trees_are_ordered_on_their_stream(su, gate, S, dtype, op):
    """C4 with a nonzero swap word, a non-static program, the root over leaf 0 and over the last leaf, one leaf."""
    _check_all(su, gate, S, tree_cases(dtype, op))


def test_streaming_two_leaf_tree_and_the_batches(su, gate, S):
    _check_all(su, gate, S, extra_tree_cases() + ["batch"])


# ---- chr_fill -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,op,pattern", [("f32", "sum", 0), ("li", "maxloc", 2)])
def test_fill_then_fold_on_one_stream(su, gate, S, dtype, op, pattern):
    """stale accumulator; chr_fill(acc) on S; a fold on S reading it; read back: the reference on po.fill's data."""
    n, seed, m = N_BUCKET, 0xC41A5EED, 3
    filled = po.fill(n, dtype, pattern, seed, 7)
    true, stale = operands(dtype, pattern, n, SEED_TRUE), operands(dtype, pattern, n, SEED_STALE)
    case = su.Case(f"chr_fill {dtype} pattern {pattern}, then a fold")
    acc = case.stale_only(stale[0])
    ins = [case.operand(true[j + 1], stale[j + 1]) for j in range(m)]
    out = case.output(filled.nbytes)
    case.expect(out, fold_ref(dtype, op, filled, true[1:1 + m], False))
    case.expect(acc, filled)

    def call(h):
        rc = ca.fill(acc.ptr, n, DT[dtype], pattern, seed, 7, stream=h)
        return rc or ca.reduce_multi(out.ptr, acc.ptr, [x.ptr for x in ins], n, DT[dtype], OP[op], h)

    su.run_gated(case, call, gate, S).check()


# ---- user ops ---------------------------------------------------------------------------------------------------------------

OPN = "user_halfadd"


@pytest.fixture(scope="module")
def user():
    """halfadd with the fold launcher alone (trees run fold by fold through stream-ordered scratch), with its tree
    launcher, and with a tree launcher that declines; freed at the end."""
    path = os.path.join(HERE, "userop", "libhalfadd_tree_op.so")
    assert os.path.exists(path), f"{path} missing: make -C tests/userop -f tree_op.mk (__graft_entry__.build())"
    lib = ctypes.CDLL(path)
    fold = ctypes.cast(lib.chr_test_halfadd, ctypes.c_void_p).value
    codes = {"fold": ca.op_create(fold),
             "tree": ca.op_create(fold, tree=ctypes.cast(lib.chr_test_halfadd_tree, ctypes.c_void_p).value),
             "decline": ca.op_create(fold, tree=ctypes.cast(lib.chr_test_decline_tree, ctypes.c_void_p).value)}
    yield codes
    for code in codes.values():
        assert ca.op_free(code) == 0


@pytest.mark.parametrize("m", [1, 17])
def test_user_fold_launcher_on_its_stream(su, gate, S, user, m):
    n = N_BUCKET
    true, stale = operands("f32", 0, n, SEED_TRUE), operands("f32", 0, n, SEED_STALE)
    case = su.Case(f"halfadd fold m={m}")
    acc = case.operand(true[0], stale[0], 4)
    ins = [case.operand(true[j + 1], stale[j + 1], 4) for j in range(m)]
    out = case.output(true[0].nbytes, 4)
    case.expect(out, po.reduce_multi(true[0].copy(), [x.copy() for x in true[1:1 + m]], "f32", OPN))
    su.run_gated(case, lambda h: ca.reduce_multi(out.ptr, acc.ptr, [x.ptr for x in ins], n, ca.FLOAT32, user["fold"], h),
                 gate, S).check()


@pytest.mark.parametrize("which", ["tree", "fold", "decline"])
def test_user_trees_on_their_stream(su, gate, S, user, which):
    """The 8-leaf C4 tree with swap bits: in one pass (the tree launcher); fold by fold with its inner nodes in
    hipMallocAsync scratch (no tree launcher); and through a tree launcher that declines."""
    n = N_TREE
    true, stale = operands("f32", 0, n, SEED_TRUE)[:8], operands("f32", 0, n, SEED_STALE)[:8]
    case = su.Case(f"halfadd tree, op registered as {which!r}")
    leaves = [case.operand(true[j], stale[j], 4) for j in range(8)]
    out = case.output(true[0].nbytes, 4)
    case.expect(out, tree_ref(list(true), C4, C4_SWAPS, "f32", OPN))
    su.run_gated(case, lambda h: ca.reduce_tree(out.ptr, [x.ptr for x in leaves], C4, C4_SWAPS, n, ca.FLOAT32,
                                                user[which], h), gate, S).check()


@pytest.mark.parametrize("which", ["fold", "decline"])
def test_two_user_trees_through_folds_behind_one_gate(su, gate, S, user, which):
    """Two fold-by-fold trees back to back on the busy stream, the second reading the first's root.  With a
    hipMallocAsync / hipFreeAsync pair per call the second call's hipFreeAsync waited on the host until the stream
    had drained (the pool had handed it the block whose free was still pending): 56.8 ms in eight such calls behind a
    56.6 ms gate.  The scratch is kept per stream now (user_ops.cpp TreeScratch): both calls return at once."""
    n = N_TREE
    true, stale = operands("f32", 0, n, SEED_TRUE)[:8], operands("f32", 0, n, SEED_STALE)[:8]
    case = su.Case(f"two halfadd trees through folds, op registered as {which!r}")
    leaves = [case.operand(true[j], stale[j], 4) for j in range(8)]
    first, second = case.output(true[0].nbytes, 4), case.output(true[0].nbytes, 4)
    ref1 = tree_ref(list(true), C4, C4_SWAPS, "f32", OPN)
    case.expect(first, ref1)
    case.expect(second, tree_ref([ref1] + list(true[1:]), C4, C4_SWAPS, "f32", OPN))

    def call(h):
        rc = ca.reduce_tree(first.ptr, [x.ptr for x in leaves], C4, C4_SWAPS, n, ca.FLOAT32, user[which], h)
        return rc or ca.reduce_tree(second.ptr, [first.ptr] + [x.ptr for x in leaves[1:]], C4, C4_SWAPS, n, ca.FLOAT32,
                                    user[which], h)

    su.run_gated(case, call, gate, S).check()


def test_rotmix_on_a_derived_type_off_alignment(su, gate, S):
    """f64 x 3 (24 bytes) with every buffer 8 bytes into its allocation: one fold (m = 3) and one 8-leaf tree fold by
    fold, whose scratch slots start at the residue of `out` (user_ops.cpp user_tree, `skew`)."""
    import struct_ref as sr

    path = os.path.join(HERE, "userop", "libstruct_op.so")
    assert os.path.exists(path), f"{path} missing: make -C tests/userop -f struct_op.mk (__graft_entry__.build())"
    lib = ctypes.CDLL(path)
    dt = ca.type_contiguous(3, ca.FLOAT64)
    op = ca.op_create(ctypes.cast(lib.chr_struct_RotMixK_f64x3, ctypes.c_void_p).value)
    try:
        n, k = 256 * 2 + 21 * 2 + 1, 3
        true, stale = operands("f64", 0, n * k, SEED_TRUE)[:8], operands("f64", 0, n * k, SEED_STALE)[:8]
        case = su.Case("rotmix f64x3 fold m=3, 8 bytes in")
        acc = case.operand(true[0], stale[0], 8)
        ins = [case.operand(true[j + 1], stale[j + 1], 8) for j in range(3)]
        out = case.output(true[0].nbytes, 8)
        assert out.ptr % 16 == 8
        case.expect(out, sr.fold_ref(true[0], true[1:4], k, sr.rotmix, False))
        su.run_gated(case, lambda h: ca.reduce_multi(out.ptr, acc.ptr, [x.ptr for x in ins], n, dt, op, h), gate, S).check()
        case = su.Case("rotmix f64x3 tree fold by fold, 8 bytes in")
        leaves = [case.operand(true[j], stale[j], 8) for j in range(8)]
        out = case.output(true[0].nbytes, 8)
        case.expect(out, sr.tree_ref(list(true), C4, C4_SWAPS, k, sr.rotmix))
        su.run_gated(case, lambda h: ca.reduce_tree(out.ptr, [x.ptr for x in leaves], C4, C4_SWAPS, n, dt, op, h),
                     gate, S).check()
    finally:
        assert ca.op_free(op) == 0 and ca.type_free(dt) == 0


def test_binary16_sum_fold_and_tree(su, gate, S):
    import f16_ref
    from chiara_amd import ops

    code = ops.float16_op(ca.SUM)
    try:
        n = N_TREE
        true = [f16_ref.uniform(n, SEED_TRUE, r) for r in range(8)]
        stale = [f16_ref.uniform(n, SEED_STALE, r) for r in range(8)]
        case = su.Case("binary16 SUM fold m=3")
        acc = case.operand(true[0], stale[0])
        ins = [case.operand(true[j + 1], stale[j + 1]) for j in range(3)]
        out = case.output(true[0].nbytes)
        case.expect(out, f16_ref.fold_ref(true[0], true[1:4], "sum"))
        su.run_gated(case, lambda h: ca.reduce_multi(out.ptr, acc.ptr, [x.ptr for x in ins], n, ops.F16_DTYPE, code, h),
                     gate, S).check()
        case = su.Case("binary16 SUM 8-leaf tree")
        leaves = [case.operand(true[j], stale[j]) for j in range(8)]
        out = case.output(true[0].nbytes)
        case.expect(out, f16_ref.tree_ref(true, C4, C4_SWAPS, "sum"))
        su.run_gated(case, lambda h: ca.reduce_tree(out.ptr, [x.ptr for x in leaves], C4, C4_SWAPS, n, ops.F16_DTYPE,
                                                    code, h), gate, S).check()
    finally:
        assert ops.release() == 0


# ---- the forced shapes, in one child ---------------------------------------------------------------------------------------

def test_forced_shapes_in_a_child(su):
    """The fold and tree cases above with CHR_REDUCE_NT=1, CHR_REDUCE_MAX_LAUNCH_VEC=2048 and CHR_XCD_RUN_KIB=4 (read
    once per process): several launch pieces and tree segments per call.  One JSON line per case."""
    env = dict(os.environ, **FORCED_ENV)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    rows = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(rows) == len(all_builtin_cases()), (len(rows), p.stderr[-2000:])
    for r in rows:
        su.note_enqueue(r["enqueue_ms"] * 1e-3, "child: " + r["what"])
    bad = [r["verdict"] for r in rows if r["verdict"] is not None]
    assert not bad, f"{len(bad)} of {len(rows)} cases: " + " | ".join(bad[:4])


# ---- the executors' streams ---------------------------------------------------------------------------------------------

def _group_operands(su, case, count, nranks):
    true = [po.fill(count, "f32", 0, 17, r) for r in range(nranks)]
    stale = [po.fill(count, "f32", 0, 917, r) for r in range(nranks)]
    sends = [case.operand(true[r], stale[r]) for r in range(nranks)]
    recvs = [case.output(true[0].nbytes) for _ in range(nranks)]
    return true, sends, recvs


def _same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


@pytest.mark.parametrize("schedule", ["flat", "exact"])
def test_local_group_after_a_producer_on_another_stream(su, gate, schedule):
    """chiara.h's recipe: `sends` produced behind a gate on a non-blocking stream P, an event recorded on P, the
    group's stream made to wait for it; then the blocking call."""
    import torch

    import gpu_util as gu

    nranks, k, b, count = 8, 4, 4, 4096
    g = ca.LocalGroup(nranks, 0)
    try:
        g.set_schedule(ca.SCHEDULE_EXACT if schedule == "exact" else ca.SCHEDULE_FLAT)
        assert not su.is_nonblocking(g.stream), "chiara.h: the group's stream is a blocking stream"
        P = su.nonblocking_stream()
        case = su.Case(f"local group {schedule}")
        true, sends, recvs = _group_operands(su, case, count, nranks)
        want = po.allreduce_radix_batch(true, k, b, "f32", "sum")
        for s in case.slots:
            s.reset()
        assert g.all_reduce_radix_batch([s.ptr for s in sends], [r.ptr for r in recvs], count, ca.FLOAT32, ca.SUM, k, b) == 0
        for s in case.slots:
            s.reset()
        torch.cuda.synchronize(gu.DEV)
        with torch.cuda.stream(P):
            _, ev1 = gate.enqueue(P)
            for s in sends:
                s.view.copy_(s.true[:s.nbytes], non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(P)
        torch.cuda.ExternalStream(g.stream, device=gu.DEV).wait_event(ready)
        gate_pending = not ev1.query()
        assert g.all_reduce_radix_batch([s.ptr for s in sends], [r.ptr for r in recvs], count, ca.FLOAT32, ca.SUM, k, b) == 0
        assert gate_pending, "inconclusive: the gate had completed before the call was made"
        bad = [r for r in range(nranks) if not _same_bits(gu.from_dev(recvs[r].view, np.float32), want[r])]
        assert not bad, f"ranks {bad} differ from the oracle"
    finally:
        g.destroy()


def test_local_group_after_a_producer_on_the_null_stream(su, gate):
    """"It orders after work on the legacy NULL stream": the sends are filled by chr_fill on stream 0, behind a gate
    on stream 0, and the call follows with no synchronise."""
    import torch

    import gpu_util as gu

    nranks, k, b, count = 8, 4, 4, 4096
    g = ca.LocalGroup(nranks, 0)
    try:
        case = su.Case("local group, NULL-stream producer")
        _, sends, recvs = _group_operands(su, case, count, nranks)
        filled = [po.fill(count, "f32", 0, 23, r) for r in range(nranks)]
        want = po.allreduce_radix_batch(filled, k, b, "f32", "sum")
        args = ([s.ptr for s in sends], [r.ptr for r in recvs], count, ca.FLOAT32, ca.SUM, k, b)
        for s in case.slots:
            s.reset()
        assert ca.fill(sends[0].ptr, count, ca.FLOAT32, 0, 23, 0, stream=0) == 0
        assert g.all_reduce_radix_batch(*args) == 0
        for s in case.slots:
            s.reset()
        torch.cuda.synchronize(gu.DEV)
        _, ev1 = gate.enqueue(torch.cuda.default_stream(gu.DEV))
        for r in range(nranks):
            assert ca.fill(sends[r].ptr, count, ca.FLOAT32, 0, 23, r, stream=0) == 0
        gate_pending = not ev1.query()
        assert g.all_reduce_radix_batch(*args) == 0
        assert gate_pending, "inconclusive: the gate had completed before the call was made"
        bad = [r for r in range(nranks) if not _same_bits(gu.from_dev(recvs[r].view, np.float32), want[r])]
        assert not bad, f"ranks {bad} differ from the oracle"
    finally:
        g.destroy()


def test_single_rank_comm_streams(su, gate):
    """The communicator's stream (test_rccl_comm_single_rank's use of it): blocking, so a NULL-stream producer is
    ordered before the call; and the event recipe with the _async call and chr_comm_synchronize."""
    import torch

    import gpu_util as gu

    count = 4096
    comm = ca.Comm(1, ca.get_unique_id(), 0, 0)
    try:
        assert not su.is_nonblocking(comm.stream), "chiara.h: the communicator's stream is a blocking stream"
        case = su.Case("single-rank comm")
        true, sends, recvs = _group_operands(su, case, count, 1)
        send, recv = sends[0], recvs[0]
        filled = po.fill(count, "f32", 0, 29, 0)
        for s in case.slots:
            s.reset()
        assert ca.all_reduce_radix_batch(send.ptr, recv.ptr, count, ca.FLOAT32, ca.SUM, comm, 2, 1) == 0
        # the NULL-stream producer
        for s in case.slots:
            s.reset()
        torch.cuda.synchronize(gu.DEV)
        _, ev1 = gate.enqueue(torch.cuda.default_stream(gu.DEV))
        assert ca.fill(send.ptr, count, ca.FLOAT32, 0, 29, 0, stream=0) == 0
        gate_pending = not ev1.query()
        assert ca.all_reduce_radix_batch(send.ptr, recv.ptr, count, ca.FLOAT32, ca.SUM, comm, 2, 1) == 0
        assert gate_pending, "inconclusive: the gate had completed before the call was made"
        assert _same_bits(gu.from_dev(recv.view, np.float32), filled)
        # the event recipe, asynchronous
        P = su.nonblocking_stream()
        for s in case.slots:
            s.reset()
        torch.cuda.synchronize(gu.DEV)
        with torch.cuda.stream(P):
            _, ev1 = gate.enqueue(P)
            send.view.copy_(send.true[:send.nbytes], non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(P)
        torch.cuda.ExternalStream(comm.stream, device=gu.DEV).wait_event(ready)
        assert ca.all_reduce_radix_batch(send.ptr, recv.ptr, count, ca.FLOAT32, ca.SUM, comm, 2, 1, async_op=True) == 0
        assert not ev1.query(), "the _async call waited for the gate (or the gate was too short)"
        assert comm.synchronize() == 0
        assert _same_bits(gu.from_dev(recv.view, np.float32), true[0])
    finally:
        comm.destroy()
        torch.cuda.synchronize(gu.DEV)


# ---- the control: the check must bite (last, so that it sees every case's enqueue time) ---------------------------------------

def test_control_a_strayed_call_shows(su, gate, S):
    """The same sequence with the call handed a second non-blocking stream that nothing orders against S -- what a
    launcher that dropped its stream argument amounts to: the result must NOT be the reference.  It races a read
    against a copy on valid buffers, as test_the_checks_fail_on_the_device_when_a_call_strays writes into memory the
    buffer owns.  And the gate must have lasted 20 times the largest host enqueue time of any case."""
    S2 = su.nonblocking_stream()
    assert S2.cuda_stream != S.cuda_stream
    gates = []
    for c in (Fold("f32", "sum", 1, "in", False, False, N_BUCKET, "multi"), Tree("f32", "sum", C4, C4_SWAPS, N_TREE, "in", None)):
        nops = 2 if isinstance(c, Fold) else 8
        true, stale = operands("f32", 0, c.n, SEED_TRUE)[:nops], operands("f32", 0, c.n, SEED_STALE)[:nops]
        if isinstance(c, Fold):
            ref_true, ref_stale = fold_ref("f32", "sum", true[0], true[1:], False), fold_ref("f32", "sum", stale[0], stale[1:], False)
            case, call = build_fold(su, c)
        else:
            ref_true = tree_ref(list(true), c.comb, c.swaps, "f32", "sum")
            ref_stale = tree_ref(list(stale), c.comb, c.swaps, "f32", "sum")
            case, call = build_tree(su, c)
        differ = np.count_nonzero(ref_true.view(np.uint32) != ref_stale.view(np.uint32)) / ref_true.size
        assert differ >= 0.99, f"stale and true references differ in only {differ:.4f} of the elements"
        good = su.run_gated(case, call, gate, S)
        good.check()
        out = su.run_gated(case, call, gate, S, call_stream=S2)
        is_stale = np.array_equal(out.got[0], su.bits(ref_stale))
        print(f"control {type(c).__name__}: strayed call equals the reference: {out.ordered}; equals the reference of "
              f"the stale operands: {is_stale}; {out.differing()[0]} of {out.refs[0].size} bytes differ; {out.times()}")
        assert out.rc == 0 and out.at_once, out.times()
        assert not out.ordered, "a call on a stream that nothing orders against S still gave the reference: the gate does not bite"
        gates += [good.gate_ms, out.gate_ms]
    largest = su.LARGEST_ENQUEUE
    print(f"control: GATE_BYTES {su.GATE_BYTES >> 20} MiB, gate {min(gates):.3f} ms (shortest of {len(gates)}), largest host "
          f"enqueue time {largest['s'] * 1e3:.3f} ms ({largest['what']})")
    assert min(gates) * 1e-3 >= 20 * largest["s"], (min(gates), largest)


# ---- the child ------------------------------------------------------------------------------------------------------------------

def main():
    import stream_util as su_

    for k, v in FORCED_ENV.items():  # the configuration is the parent's to set: refuse to run without it
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    gate_, stream = su_.shared_gate(), su_.nonblocking_stream()
    for c in all_builtin_cases():
        o = run_case(su_, gate_, stream, c)
        print(json.dumps({"what": o.what, "verdict": o.verdict(), "enqueue_ms": round(o.enqueue_s * 1e3, 4),
                          "gate_ms": round(o.gate_ms, 3)}), flush=True)


if __name__ == "__main__":
    main()
