"""Reference for the binary16 ops of libchiara_ops.so (include/chiara_ops.h): a numpy restatement of the four
functors, and the test-side evaluators over it.  Host only.

Elements are uint16 arrays holding binary16 bits.  With MPI's convention x o y = f(in = x, inout = y):
  SUM / PROD  r = y + x (y * x) on np.float16, any NaN result the canonical 0x7E00.  numpy computes half arithmetic
              through float32 and rounds once more; that is a correct single rounding to nearest even, because a
              float32 significand (24 bits) holds 2 * 11 + 2 bits (the product of two halves is exact in float32, and
              the double rounding of a sum is innocuous at p >= 2q + 2), subnormal results included.
  MAX / MIN   where(y > x, y, x) / where(y < x, y, x), selecting on the uint16 views: the chosen operand's bits
              untouched; a tie or an unordered compare returns x, the library's float rule.

The oracle has no binary16 (MPICH 3.3.2 has none), so the expected bits of a collective come from the library's own
plans, executed by tests/plan_sim.py over these functions: patched() swaps pyoracle's reduce_local / reduce_multi and
adds the dtype name "f16" for the duration of a with block, and expected() runs the SCHEDULE_REFERENCE plan, whose
order the goldens pin to the reference.  Neither plan_sim.py nor pyoracle.py is edited."""
import contextlib

import numpy as np
import pytest

import chiara_amd as ca
import pyoracle as po

DTYPE = "f16"  # the name the plan evaluator sees; the elements are uint16
OPS = ("sum", "prod", "max", "min")
KIND = {"sum": ca.SUM, "prod": ca.PROD, "max": ca.MAX, "min": ca.MIN}
CANONICAL_NAN = np.uint16(0x7E00)


def combine(op, x, y):
    """x o y = f(in = x, inout = y) elementwise on uint16 arrays of binary16 bits; returns new uint16 bits."""
    x = np.ascontiguousarray(x, dtype=np.uint16)
    y = np.ascontiguousarray(y, dtype=np.uint16)
    xf, yf = x.view(np.float16), y.view(np.float16)
    with np.errstate(all="ignore"):
        if op in ("sum", "prod"):
            r = yf + xf if op == "sum" else yf * xf
            return np.where(np.isnan(r), CANONICAL_NAN, r.view(np.uint16)).astype(np.uint16)
        if op == "max":
            return np.where(yf > xf, y, x)
        if op == "min":
            return np.where(yf < xf, y, x)
    raise ValueError(op)


def reduce_local(inp, inout, dtype, op):
    """pyoracle.reduce_local's contract: inout = inp o inout, in place."""
    assert dtype == DTYPE and inp.size == inout.size
    inout[:] = combine(op, inp, inout)
    return inout


def reduce_multi(acc, ins, dtype, op):
    """pyoracle.reduce_multi's contract: acc = ins[m-1] o (... (ins[0] o acc)), in place."""
    for x in ins:
        reduce_local(x, acc, dtype, op)
    return acc


def fold_ref(acc, ins, op, running_first=False):
    """chr_reduce_multi(_ex): out = ins[m-1] o (... (ins[0] o acc)), or running first (((acc o ins[0]) o ins[1]) ...)."""
    r = np.array(acc, dtype=np.uint16)
    for x in ins:
        r = combine(op, r, x) if running_first else combine(op, x, r)
    return r


def tree_ref(leaves, comb, swaps, op):
    """The stack program of tests/tree_util.tree_ref over combine(): push leaf j, then comb[j] combines, each popping
    `top` and folding it into the running value below: run = top o run, or with the swap bit run = run o top."""
    stack, ci = [], 0
    for j, leaf in enumerate(leaves):
        stack.append(np.array(leaf, dtype=np.uint16))
        for _ in range(comb[j]):
            top = stack.pop()
            run = stack.pop()
            stack.append(combine(op, run, top) if swaps[ci] else combine(op, top, run))
            ci += 1
    assert len(stack) == 1
    return stack[0]


@contextlib.contextmanager
def patched():
    """pyoracle's MPI_Reduce_local restatement replaced by the binary16 one, for tests/plan_sim.py and
    tests/tree_util.py, which look both up in the module at every call."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(po, "reduce_local", reduce_local)
        mp.setattr(po, "reduce_multi", reduce_multi)
        mp.setitem(po.NP_DTYPES, DTYPE, np.uint16)
        yield


def expected(mode, sends, k, b, op, schedule=None, inplace=False):
    """Every rank's output bits of a collective: the library's plan (default: SCHEDULE_REFERENCE) under the plan
    evaluator over the binary16 functions."""
    import plan_sim

    with patched():
        return plan_sim.simulate(mode, [np.array(s, dtype=np.uint16) for s in sends], k, b, DTYPE, op, inplace,
                                 schedule=ca.SCHEDULE_REFERENCE if schedule is None else schedule)


def left_fold(sends, op):
    """The plain rank-order fold ((s0 o s1) o s2) ...: what a schedule-blind reduction would give."""
    r = np.array(sends[0], dtype=np.uint16)
    for s in sends[1:]:
        r = combine(op, r, s)
    return r


def uniform(n, seed, rank):
    """U[-1, 1) rounded to binary16, as uint16 bits."""
    rng = np.random.default_rng([seed, rank])
    return rng.uniform(-1.0, 1.0, n).astype(np.float16).view(np.uint16)


def small_ints(n, seed, rank):
    """Integers in [-16, 16] as (binary16 bits, int32 values): sums of up to 8 ranks stay exact in binary16."""
    rng = np.random.default_rng([seed, rank, 1])
    v = rng.integers(-16, 17, n).astype(np.int32)
    return v.astype(np.float16).view(np.uint16), v


def finite_nonzero(n, seed, rank):
    """Random finite nonzero halves (normals and subnormals of both signs), as uint16 bits."""
    rng = np.random.default_rng([seed, rank, 2])
    mag = rng.integers(1, 0x7C00, n).astype(np.uint16)  # 0x0001 .. 0x7BFF
    return mag | (rng.integers(0, 2, n).astype(np.uint16) << np.uint16(15))


def random_bits(n, seed, rank):
    rng = np.random.default_rng([seed, rank, 3])
    return rng.integers(0, 1 << 16, n).astype(np.uint16)


def ties(n, seed, rank):
    """TIES-like data: +-0, quiet / signalling / negative NaNs, +-inf and a few small values, so that operand order
    shows in MAX / MIN (which zero, which NaN payload) and NaNs meet in SUM."""
    pool = np.array([0x0000, 0x8000, 0x7E00, 0xFE00, 0x7D01, 0xFC01, 0x7E55, 0x7C00, 0xFC00, 0x3C00, 0xBC00, 0x3C00,
                     0x0001, 0x8001, 0x4000, 0xC000], dtype=np.uint16)
    rng = np.random.default_rng([seed, rank, 4])
    return pool[rng.integers(0, pool.size, n)]


# 64 partners for the operand-domain sweep: the special values, then random fill
def partners():
    special = []
    for v in (0x0000, 0x0001, 0x03FF, 0x0400, 0x3C00, 0x7BFF, 0x7C00):  # 0, subnormals, min normal, 1, 65504, inf
        special += [v, v | 0x8000]
    special += [0x7E00, 0xFE00, 0x7D00, 0xFD00, 0x7C01, 0xFC01, 0x7FFF, 0xFFFF, 0x7E01]  # quiet / signalling / negative
    rng = np.random.default_rng(1616)
    fill = rng.integers(0, 1 << 16, 64 - len(special)).astype(np.uint16)
    out = np.concatenate([np.array(special, dtype=np.uint16), fill])
    assert out.size == 64
    return out
