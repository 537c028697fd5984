"""The kernels' element arithmetic over the operand-domain tables (tests/domain_util.py): every 8-bit operand pair,
every 16-bit value against a partner set, sign boundaries of the wider integers, subnormal operands and results,
overflow to +-inf, underflow to subnormals and +-0, invalid operations, bf16 results the packed RNE convert rounds to
inf or to a subnormal, padding bytes of the pair types.  Bit-exact against the oracle (which
tests/test_operand_domain.py pins on the CPU), nothing excluded, through every path that has arithmetic of its own:

  vector      chr_reduce_multi, m = 1, operands 16-byte congruent, cut into calls below the streaming threshold
  streaming   one call at or above it (u8, i8, bf16, f32; the small tables tiled)
  scalar      inputs off the output's alignment: apply<> instead of apply_vec<>
  running     CHR_REDUCE_RUNNING_FIRST, where that order has kernels of its own
  tree        the tree kernel's 2-leaf program, plain and swapped, and a 3-leaf program with one swapped combine
  fold        m = 3 on i8 / u8, so the SWAR code meets intermediate values as inputs

The vector-shaped paths run the table in both cell orders (domain_util.table): in the in-major order `in` is constant
along a 16-byte vector, so SWAR or packed code that reads `in` from the neighbouring lane (the i8 MAX path without its
`<< 8`, say) gives the right answer there and shows only where `in` varies."""
import functools

import numpy as np
import pytest

import chiara_amd as ca
import domain_util as du
import pyoracle as po
from test_gpu_dispatch_sweep import RUNNING_FIRST, dev_at
from test_gpu_kernels import DT, OP, _bits, _bytes_copy
from tree_util import tree_ref

pytestmark = pytest.mark.gpu

NT_MIN_BYTES = 40 << 20  # nt_min_bytes (csrc/reduce_kernels.hip): (m + 2) * n * es from which a call streams
STREAMING = ("u8", "i8", "bf16", "f32")
# the dispatch sweep's list, and the integer pairs: a MAXLOC / MINLOC tie keeps inout's padding bytes, which the
# tables fill, so the order shows on li and si as well (2i has no padding: both orders give the same bits)
RF_CASES = RUNNING_FIRST + [(d, o) for d in ("li", "2i", "si") for o in du.LOC]
RF_DTYPES = tuple(dict.fromkeys(d for d, _ in RF_CASES))


@pytest.fixture(scope="module")
def gu():
    import gpu_util

    return gpu_util


def esize(dtype):
    return np.dtype(po.NP_DTYPES[dtype]).itemsize


@functools.lru_cache(maxsize=None)
def ref_local(dtype, op, order=du.IN_MAJOR):
    """MPI_Reduce_local(in = x, inout = y) over the table, by the oracle; shared and read-only."""
    if order == du.IN_MAJOR:
        x, y = du.table(dtype)
        r = po.reduce_local(x, _bytes_copy(y), dtype, op)
    else:
        r = du.reorder(ref_local(dtype, op), dtype, order)
    r.flags.writeable = False
    return r


both_orders = pytest.mark.parametrize("order", du.ORDERS)


class Report:
    """Every op of a test is run and compared before the test fails, so one wrong op does not hide the next."""

    def __init__(self):
        self.failures = []

    def check(self, got, want, x, y, dtype, op, path):
        if np.array_equal(_bits(got), _bits(want)):
            return
        try:
            du.assert_cells_equal(got, want, x, y, dtype, op, path)
            self.failures.append(f"{dtype} {op} {path}: results differ")  # not reached: the cells differ
        except AssertionError as e:
            self.failures.append(str(e))

    def done(self):
        assert not self.failures, "\n".join(self.failures)


def pieces(n, es, nops=3):
    """[start, stop) ranges of at most the largest multiple of 4096 elements that keeps nops * count * es under the
    streaming threshold (and every piece as congruent as the whole)."""
    step = (NT_MIN_BYTES - 1) // (nops * es) // 4096 * 4096
    return [(a, min(a + step, n)) for a in range(0, n, step)]


def fold_in_pieces(gu, p_out, p_acc, p_ins, n, dtype, op, flags=0):
    es = esize(dtype)
    for a, b in pieces(n, es, len(p_ins) + 2):
        o = a * es
        rc = ca.reduce_multi_ex(p_out + o, p_acc + o, [p + o for p in p_ins], b - a, DT[dtype], OP[op], flags, gu.stream())
        assert rc == 0, (dtype, op, a, b)
    gu.sync()


@both_orders
@pytest.mark.parametrize("dtype", du.DTYPES)
def test_vector_kernel(gu, dtype, order):
    x, y = du.table(dtype, order)
    (d_x, p_x), (d_y, p_y) = dev_at(gu, x, 0), dev_at(gu, y, 0)
    d_out, rep = gu.empty_dev(x.nbytes), Report()
    for op in du.valid_ops(dtype):
        d_out.zero_()
        fold_in_pieces(gu, d_out.data_ptr(), p_y, [p_x], x.size, dtype, op)
        want = ref_local(dtype, op, order)
        rep.check(gu.from_dev(d_out, x.dtype, x.size), want, x, y, dtype, op, f"vector kernel, {order}")
    rep.done()


@both_orders
@pytest.mark.parametrize("dtype", STREAMING)
def test_streaming_shape(gu, dtype, order):
    x, y = du.table(dtype, order)
    reps = -(-NT_MIN_BYTES // (3 * x.nbytes))
    xs, ys = (x, y) if reps == 1 else (np.tile(x, reps), np.tile(y, reps))
    n = xs.size
    assert 3 * (n // (16 // x.itemsize)) * 16 >= NT_MIN_BYTES
    (d_x, p_x), (d_y, p_y) = dev_at(gu, xs, 0), dev_at(gu, ys, 0)
    d_out, rep = gu.empty_dev(xs.nbytes), Report()
    for op in du.valid_ops(dtype):
        d_out.zero_()
        assert ca.reduce_multi(d_out.data_ptr(), p_y, [p_x], n, DT[dtype], OP[op], gu.stream()) == 0
        gu.sync()
        want = ref_local(dtype, op, order) if reps == 1 else np.tile(ref_local(dtype, op, order), reps)
        rep.check(gu.from_dev(d_out, x.dtype, n), want, xs, ys, dtype, op, f"streaming shape, {order}")
    rep.done()


@pytest.mark.parametrize("dtype", du.DTYPES)
def test_scalar_kernel(gu, dtype):
    """Inputs one element off the output's alignment (16-byte elements: off by their own alignment, 8 bytes, since
    whole elements keep them congruent).  bf16: a 1-in-8 sub-table, skewed so that every partner keeps meeting
    an eighth of the values."""
    x, y = du.table(dtype)
    sel = None
    if dtype == "bf16":
        i = np.arange(x.size, dtype=np.int64)
        sel = np.flatnonzero((i + i // 512) % 8 == 0)
        x, y = x[sel], y[sel]
    es = x.itemsize

    def shifted(a):  # one element, or one 8-byte word of a 16-byte element
        if es < 16:
            return dev_at(gu, a, 1)
        return dev_at(gu, np.ascontiguousarray(a).view(np.uint8).view(np.uint64), 1)

    (d_x, p_x), (d_y, p_y) = shifted(x), shifted(y)
    assert (p_x - d_x.data_ptr()) % 16 == min(es, 8) and p_x + x.nbytes <= d_x.data_ptr() + d_x.numel()
    d_out, rep = gu.empty_dev(x.nbytes), Report()
    for op in du.valid_ops(dtype):
        d_out.zero_()
        assert ca.reduce_multi(d_out.data_ptr(), p_y, [p_x], x.size, DT[dtype], OP[op], gu.stream()) == 0
        gu.sync()
        want = ref_local(dtype, op) if sel is None else ref_local(dtype, op)[sel]
        rep.check(gu.from_dev(d_out, x.dtype, x.size), want, x, y, dtype, op, "scalar kernel")
    rep.done()


@both_orders
@pytest.mark.parametrize("dtype", RF_DTYPES)
def test_running_first(gu, dtype, order):
    """acc = x is the running value: MPI_Reduce_local(in = running, inout = next), the result taking next's place
    (as test_gpu_dispatch_sweep.test_bucket_running_first evaluates it)."""
    x, y = du.table(dtype, order)
    (d_x, p_x), (d_y, p_y) = dev_at(gu, x, 0), dev_at(gu, y, 0)
    d_out, rep = gu.empty_dev(x.nbytes), Report()
    for op in [o for d, o in RF_CASES if d == dtype]:
        run = _bytes_copy(x)
        for nxt in [_bytes_copy(y)]:
            po.reduce_local(run, nxt, dtype, op)
            run = nxt
        d_out.zero_()
        fold_in_pieces(gu, d_out.data_ptr(), p_x, [p_y], x.size, dtype, op, ca.REDUCE_RUNNING_FIRST)
        rep.check(gu.from_dev(d_out, x.dtype, x.size), run, x, y, dtype, op, f"REDUCE_RUNNING_FIRST, {order}")
    rep.done()


# leaves as (x, y, z = x rotated by one element), the program; every first combine is MPI_Reduce_local(in = x,
# inout = y)
TREES = {"2-leaf": ("yx", [0, 1], [0]), "2-leaf swapped": ("xy", [0, 1], [1]),
         "3-leaf, one swapped": ("yxz", [0, 1, 1], [0, 1])}


@pytest.mark.parametrize("prog", list(TREES), ids=[p.replace(" ", "_").replace(",", "") for p in TREES])
@both_orders
@pytest.mark.parametrize("dtype", du.DTYPES)
def test_tree_kernel(gu, dtype, prog, order):
    """Cut like the vector kernel's calls: a 2-leaf tree of 40 MiB or more is handed to the bucket kernel."""
    names, comb, swaps = TREES[prog]
    x, y = du.table(dtype, order)
    host = {"x": x, "y": y}
    if "z" in names:
        host["z"] = du.rotate(x, 1)
    leaves = [host[c] for c in names]
    dev = [dev_at(gu, a, 0) for a in leaves]
    d_out, rep = gu.empty_dev(x.nbytes), Report()
    es = x.itemsize
    for op in du.valid_ops(dtype):
        d_out.zero_()
        for a, b in pieces(x.size, es):
            rc = ca.reduce_tree(d_out.data_ptr() + a * es, [p + a * es for _, p in dev], comb, swaps, b - a, DT[dtype],
                                OP[op], gu.stream())
            assert rc == 0, (dtype, op, prog)
        gu.sync()
        want = tree_ref(leaves, comb, swaps, dtype, op)
        rep.check(gu.from_dev(d_out, x.dtype, x.size), want, x, y, dtype, op, f"tree kernel, {prog}, {order}")
    rep.done()


@pytest.mark.parametrize("dtype", ["i8", "u8"])
def test_m3_fold(gu, dtype):
    """y op x op (x rotated by 1) op (x rotated by 257): the second and third steps take results as their inout."""
    x, y = du.table(dtype)
    ins = [x, du.rotate(x, 1), du.rotate(x, 257)]
    (d_y, p_y), dev = dev_at(gu, y, 0), [dev_at(gu, a, 0) for a in ins]
    d_out, rep = gu.empty_dev(x.nbytes), Report()
    for op in du.valid_ops(dtype):
        d_out.zero_()
        assert ca.reduce_multi(d_out.data_ptr(), p_y, [p for _, p in dev], x.size, DT[dtype], OP[op], gu.stream()) == 0
        gu.sync()
        want = po.reduce_multi(_bytes_copy(y), ins, dtype, op)
        rep.check(gu.from_dev(d_out, x.dtype, x.size), want, x, y, dtype, op, "m = 3 fold (in, in rotated by 1 and by 257)")
    rep.done()
