"""Every (dtype, op) code through the public API: the host-side dispatch (csrc/kernel_table.hpp) must hand each of
the 18 x 12 pairs to the kernel that computes it -- vector kernel, scalar kernel and tree kernel, in both operand
orders where the order picks another kernel -- or reject it untouched.  Bit-exact against the oracle.

Two layouts per pair:
  (a) every operand 16-byte congruent, n = (256 * 4 + 3) * E + 1 elements with E = 16 / element size: one full
      trip of the plain vector kernel (256 threads x 4 vectors), one partial trip and a scalar tail (for 16-byte
      elements the + 1 is one more vector and there is no tail);
  (b) the inputs one element off the output's alignment, n = 257: the whole call runs on the scalar kernel.
      16-byte elements cannot be made incongruent by element offsets (their scalar path: test_gpu_tree.py's
      test_tree_scalar_path_pair_and_complex_every_program and the pair fixtures of test_gpu_kernels.py)."""
import functools

import numpy as np
import pytest

import chiara_amd as ca
import pyoracle as po
from test_gpu_kernels import DT, OP, _bits, _bytes_copy
from tree_util import tree_ref

pytestmark = pytest.mark.gpu

DTYPES, OPS = list(DT), list(OP)
FLOATS, PAIRS, CPLX = ("f32", "f64", "bf16"), ("fi", "di", "li", "2i", "si"), ("cf", "cd")
M = 3
COMB, SWAPS = [0, 1, 1], [0, 1]


def valid(dtype, op):
    """MPICH 3.3.2's (type, op) table (include/chiara.h)."""
    if dtype in PAIRS:
        return op in ("maxloc", "minloc")
    if dtype in CPLX:
        return op in ("sum", "prod")
    if op in ("sum", "prod", "max", "min"):
        return True
    if op in ("land", "lor", "lxor"):
        return dtype != "bf16"
    return op in ("band", "bor", "bxor") and dtype not in FLOATS


def test_the_sweep_covers_the_whole_table():
    assert [DT[d] for d in DTYPES] == list(range(18)) and [OP[o] for o in OPS] == list(range(12))
    assert sum(valid(d, o) for d in DTYPES for o in OPS) == 2 * 7 + 4 + 8 * 10 + 5 * 2 + 2 * 2


def layouts(dtype):
    """(name, n, element offset of the inputs) per layout."""
    es = np.dtype(po.NP_DTYPES[dtype]).itemsize
    a = ("congruent", (256 * 4 + 3) * (16 // es) + 1, 0)
    return [a] if es == 16 else [a, ("inputs off by one", 257, 1)]


def pattern_for(op):
    if op in ("max", "min", "maxloc", "minloc", "lor", "lxor"):
        return po.PAT_TIES
    return po.PAT_SPARSE if op == "land" else po.PAT_UNIFORM


@functools.lru_cache(maxsize=None)
def operands(dtype, pattern, n, i32_prod):
    """acc and M inputs; shared by the tests and never written (every user copies)."""
    acc = po.fill(n, dtype, pattern, 5, 0)
    ins = [po.fill(n, dtype, pattern, 5, r + 1) for r in range(M)]
    if i32_prod:  # as test_gpu_kernels._check_multi
        ins = [(x % 7).astype(np.int32) for x in ins]
    for x in [acc] + ins:
        x.flags.writeable = False
    return acc, ins


def dev_at(gu, x, off):
    """x's bytes on the device, `off` elements into a 16-byte aligned buffer: (tensor, address of x[0])."""
    t = gu.empty_dev(x.nbytes + off * x.itemsize)
    t[off * x.itemsize:off * x.itemsize + x.nbytes] = gu.to_dev(x)
    return t, t.data_ptr() + off * x.itemsize


@pytest.fixture(scope="module")
def gu():
    import gpu_util

    return gpu_util


@pytest.mark.parametrize("dtype", DTYPES)
def test_bucket_every_op(gu, dtype):
    npdt = po.NP_DTYPES[dtype]
    for op in OPS:
        for name, n, in_off in layouts(dtype):
            acc, ins = operands(dtype, pattern_for(op), n, op == "prod" and dtype == "i32")
            d_acc, p_acc = dev_at(gu, acc, 0)
            d_ins = [dev_at(gu, x, in_off) for x in ins]
            rc = ca.reduce_multi(p_acc, p_acc, [p for _, p in d_ins], n, DT[dtype], OP[op], gu.stream())
            gu.sync()
            got = gu.from_dev(d_acc, npdt, n)
            if not valid(dtype, op):
                assert rc == 1, (dtype, op, name)
                assert np.array_equal(got.view(np.uint8), acc.view(np.uint8)), (dtype, op, name)
                continue
            assert rc == 0, (dtype, op, name)
            ref = po.reduce_multi(_bytes_copy(acc), [_bytes_copy(x) for x in ins], dtype, op)
            np.testing.assert_array_equal(_bits(got), _bits(ref), err_msg=f"{dtype} {op} {name}")


RUNNING_FIRST = ([(d, o) for d in FLOATS for o in ("sum", "prod", "max", "min")] +
                 [(d, o) for d in ("fi", "di") for o in ("maxloc", "minloc")] +
                 [(d, o) for d in CPLX for o in ("sum", "prod")])


@pytest.mark.parametrize("dtype,op", RUNNING_FIRST)
def test_bucket_running_first(gu, dtype, op):
    """CHR_REDUCE_RUNNING_FIRST on every pair whose running-first order has a kernel of its own: each step is
    MPI_Reduce_local(running, next), as test_gpu_kernels.test_reduce_multi_running_first evaluates it."""
    npdt = po.NP_DTYPES[dtype]
    for name, n, in_off in layouts(dtype):
        acc, ins = operands(dtype, po.PAT_TIES, n, False)
        run = _bytes_copy(acc)
        for x in ins:
            nxt = _bytes_copy(x)
            po.reduce_local(run, nxt, dtype, op)
            run = nxt
        d_acc, p_acc = dev_at(gu, acc, 0)
        d_ins = [dev_at(gu, x, in_off) for x in ins]
        rc = ca.reduce_multi_ex(p_acc, p_acc, [p for _, p in d_ins], n, DT[dtype], OP[op], ca.REDUCE_RUNNING_FIRST,
                                gu.stream())
        assert rc == 0, (dtype, op, name)
        gu.sync()
        np.testing.assert_array_equal(_bits(gu.from_dev(d_acc, npdt, n)), _bits(run), err_msg=f"{dtype} {op} {name}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_tree_every_valid_op(gu, dtype):
    """A 3-leaf program with one combine in each operand order, on the vector and on the scalar tree kernel."""
    npdt = po.NP_DTYPES[dtype]
    for op in OPS:
        if not valid(dtype, op):
            continue
        for name, n, in_off in layouts(dtype):
            acc, ins = operands(dtype, pattern_for(op), n, op == "prod" and dtype == "i32")
            leaves = [acc] + ins[:2]
            d_leaves = [dev_at(gu, x, in_off) for x in leaves]
            d_out = gu.empty_dev(acc.nbytes)
            rc = ca.reduce_tree(d_out, [p for _, p in d_leaves], COMB, SWAPS, n, DT[dtype], OP[op], gu.stream())
            assert rc == 0, (dtype, op, name)
            gu.sync()
            ref = tree_ref(leaves, COMB, SWAPS, dtype, op)
            np.testing.assert_array_equal(_bits(gu.from_dev(d_out, npdt, n)), _bits(ref), err_msg=f"{dtype} {op} {name}")
