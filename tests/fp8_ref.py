"""Reference for the OCP FP8 ops and casts of libchiara_fp8.so (include/chiara_fp8.h): the formats from their
definition, the arithmetic in float64 with a nearest-even search of the 256-entry value table, and the test-side
evaluators over it.  Host only, and independent of the code under test.

Elements are uint8 arrays of codes.  With MPI's convention x o y = f(in = x, inout = y):
  SUM / PROD  r = dec(y) + dec(x) (dec(y) * dec(x)) in float64 -- exact: the sums need at most 34 bits, the products
              8 -- then encode(): the nearest finite magnitude of the table, ties to the even code, with one more
              entry past max standing for the value the format would have there were its exponent unbounded (E4M3
              480, E5M2 65536).  A magnitude that rounds to that entry has overflowed: the canonical NaN (E4M3) or
              +-inf (E5M2) under IEEE.  SATURATE clamps r to [-max, +max] first.  Any NaN is the canonical 0x7F / 0x7E.
  MAX / MIN   where(dec(y) > dec(x), y, x) / where(dec(y) < dec(x), y, x) on the codes: the chosen operand's byte
              untouched; a tie or an unordered compare returns x, the library's float rule.

The oracle has no 8-bit float, so the expected bits of a collective come from the library's own plans, executed by
tests/plan_sim.py over these functions (patched(), expected(), as tests/f16_ref.py does it)."""
import contextlib

import numpy as np
import pytest

import chiara_amd as ca
import pyoracle as po

DTYPE = "f8"  # the name the plan evaluator sees; the elements are uint8
E4M3, E5M2 = 0, 1
IEEE, SATURATE = 0, 1
FORMATS = {"e4m3": E4M3, "e5m2": E5M2}
POLICIES = {"ieee": IEEE, "sat": SATURATE}
OPS = ("sum", "prod", "max", "min")
KIND = {"sum": ca.SUM, "prod": ca.PROD, "max": ca.MAX, "min": ca.MIN}
CANONICAL_NAN = {E4M3: 0x7F, E5M2: 0x7E}
MAX_CODE = {E4M3: 0x7E, E5M2: 0x7B}
MAX_VALUE = {E4M3: 448.0, E5M2: 57344.0}
# every (format, op, policy) the library registers: MAX and MIN once per format
COMBOS = [(f, op, p) for f in FORMATS for op in OPS for p in (("ieee", "sat") if op in ("sum", "prod") else ("ieee",))]


def _decode_table(fmt):
    """code -> float64 value, from the format definition: sign, E exponent bits (bias 2^(E-1) - 1), M mantissa bits,
    subnormals at exponent 0; E4M3 (fn) has no infinities and one NaN mantissa at the top exponent, E5M2 is IEEE."""
    ebits, mbits = (4, 3) if fmt == E4M3 else (5, 2)
    bias = (1 << (ebits - 1)) - 1
    out = np.empty(256, dtype=np.float64)
    for c in range(256):
        s = -1.0 if c & 0x80 else 1.0
        e = (c >> mbits) & ((1 << ebits) - 1)
        m = c & ((1 << mbits) - 1)
        if fmt == E5M2 and e == 31:
            v = np.inf if m == 0 else np.nan
        elif fmt == E4M3 and e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m / (1 << mbits) * 2.0 ** (1 - bias)
        else:
            v = (1 + m / (1 << mbits)) * 2.0 ** (e - bias)
        out[c] = s * v
    return out


TABLE = {f: _decode_table(f) for f in (E4M3, E5M2)}
# the finite magnitudes in code order (codes 0 .. max are monotonic), and the entry past max
_MAGS = {f: np.append(TABLE[f][:MAX_CODE[f] + 1], 2 * TABLE[f][MAX_CODE[f]] - TABLE[f][MAX_CODE[f] - 1]) for f in TABLE}


def decode(fmt, codes):
    return TABLE[fmt][np.asarray(codes, dtype=np.uint8)]


def encode(fmt, overflow, r):
    """The code of each float64 value of r: one round-to-nearest-even with the exponent unbounded, then the policy."""
    r = np.asarray(r, dtype=np.float64)
    nan = np.isnan(r)
    a = np.abs(np.where(nan, 0.0, r))
    if overflow == SATURATE:
        a = np.minimum(a, MAX_VALUE[fmt])
    mags = _MAGS[fmt]
    top = mags.size - 1  # the entry past max: overflow
    hi = np.minimum(np.searchsorted(mags, a, side="left"), top)  # first entry >= a
    lo = np.maximum(hi - 1, 0)
    with np.errstate(invalid="ignore"):
        d_lo, d_hi = a - mags[lo], mags[hi] - a  # a beyond the last entry: d_hi < 0, the last entry wins
    pick = np.where(d_hi < d_lo, hi, np.where(d_lo < d_hi, lo, np.where(hi % 2 == 0, hi, lo)))
    sign = np.where(np.signbit(r), 0x80, 0).astype(np.uint8)
    over = CANONICAL_NAN[fmt] if fmt == E4M3 else (sign | 0x7C)
    out = np.where(pick == top, over, sign | pick.astype(np.uint8))
    return np.where(nan, CANONICAL_NAN[fmt], out).astype(np.uint8)


def combine(fmt, op, overflow, x, y):
    """x o y = f(in = x, inout = y) elementwise on uint8 arrays of codes; returns new uint8 codes."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    y = np.ascontiguousarray(y, dtype=np.uint8)
    xf, yf = decode(fmt, x), decode(fmt, y)
    with np.errstate(all="ignore"):
        if op == "sum":
            return encode(fmt, overflow, yf + xf)
        if op == "prod":
            return encode(fmt, overflow, yf * xf)
        if op == "max":
            return np.where(yf > xf, y, x)
        if op == "min":
            return np.where(yf < xf, y, x)
    raise ValueError(op)


def quantize_ref(fmt, overflow, src, scale):
    """enc(f32(src) * scale): src a float32 array (a bf16 source widened exactly), one numpy float32 multiply."""
    with np.errstate(all="ignore"):
        p = np.asarray(src, dtype=np.float32) * np.float32(scale)
    return encode(fmt, overflow, p.astype(np.float64))


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16(x):
    """Round to nearest even on the bits; NaN is 0x7FC0 (the only NaN a dequantize hands it is the canonical one)."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r).astype(np.uint16)


def dequantize_ref(fmt, codes, scale, bf16=False):
    """round(dec(codes) * scale) as uint32 bits of float32, or uint16 bits of bf16; a NaN is 0x7FC00000 / 0x7FC0."""
    with np.errstate(all="ignore"):
        p = decode(fmt, codes).astype(np.float32) * np.float32(scale)
    p = np.where(np.isnan(p), np.uint32(0x7FC00000).view(np.float32), p).astype(np.float32)
    return f32_to_bf16(p) if bf16 else p.view(np.uint32)


class Ref:
    """The evaluators of one (format, op, policy): what tests/f16_ref.py has at module level."""

    def __init__(self, fmt, op, overflow=IEEE):
        self.fmt, self.op, self.overflow = fmt, op, overflow

    def combine(self, x, y):
        return combine(self.fmt, self.op, self.overflow, x, y)

    def reduce_local(self, inp, inout, dtype, op):
        """pyoracle.reduce_local's contract: inout = inp o inout, in place."""
        assert dtype == DTYPE and op == self.op and inp.size == inout.size
        inout[:] = self.combine(inp, inout)
        return inout

    def reduce_multi(self, acc, ins, dtype, op):
        """pyoracle.reduce_multi's contract: acc = ins[m-1] o (... (ins[0] o acc)), in place."""
        for x in ins:
            self.reduce_local(x, acc, dtype, op)
        return acc

    def fold_ref(self, acc, ins, running_first=False):
        """chr_reduce_multi(_ex): out = ins[m-1] o (... (ins[0] o acc)), or running first (((acc o ins[0]) o ...)."""
        r = np.array(acc, dtype=np.uint8)
        for x in ins:
            r = self.combine(r, x) if running_first else self.combine(x, r)
        return r

    def tree_ref(self, leaves, comb, swaps):
        """The stack program of tests/tree_util.tree_ref over combine(): push leaf j, then comb[j] combines, each
        popping `top` and folding it into the running value below: run = top o run, or swapped run = run o top."""
        stack, ci = [], 0
        for j, leaf in enumerate(leaves):
            stack.append(np.array(leaf, dtype=np.uint8))
            for _ in range(comb[j]):
                top = stack.pop()
                run = stack.pop()
                stack.append(self.combine(run, top) if swaps[ci] else self.combine(top, run))
                ci += 1
        assert len(stack) == 1
        return stack[0]

    @contextlib.contextmanager
    def patched(self):
        """pyoracle's MPI_Reduce_local restatement replaced by this one, for tests/plan_sim.py and
        tests/tree_util.py, which look both up in the module at every call."""
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(po, "reduce_local", self.reduce_local)
            mp.setattr(po, "reduce_multi", self.reduce_multi)
            mp.setitem(po.NP_DTYPES, DTYPE, np.uint8)
            yield

    def expected(self, mode, sends, k, b, schedule=None, inplace=False):
        """Every rank's output codes of a collective: the library's plan (default: SCHEDULE_REFERENCE) under the plan
        evaluator over these functions."""
        import plan_sim

        with self.patched():
            return plan_sim.simulate(mode, [np.array(s, dtype=np.uint8) for s in sends], k, b, DTYPE, self.op, inplace,
                                     schedule=ca.SCHEDULE_REFERENCE if schedule is None else schedule)

    def left_fold(self, sends):
        """The plain rank-order fold ((s0 o s1) o s2) ...: what a schedule-blind reduction would give."""
        r = np.array(sends[0], dtype=np.uint8)
        for s in sends[1:]:
            r = self.combine(r, s)
        return r


# The same evaluators as functions of (format, op, policy), the layout of tests/f16_ref.py.
def fold_ref(fmt, op, overflow, acc, ins, running_first=False):
    return Ref(fmt, op, overflow).fold_ref(acc, ins, running_first)


def tree_ref(fmt, op, overflow, leaves, comb, swaps):
    return Ref(fmt, op, overflow).tree_ref(leaves, comb, swaps)


def patched(fmt, op, overflow=IEEE):
    return Ref(fmt, op, overflow).patched()


def expected(fmt, op, overflow, mode, sends, k, b, schedule=None, inplace=False):
    return Ref(fmt, op, overflow).expected(mode, sends, k, b, schedule, inplace)


# ---- data ------------------------------------------------------------------------------------------------------------

def uniform(fmt, n, seed, rank):
    """U[-1, 1) rounded to the format, as codes."""
    rng = np.random.default_rng([seed, rank])
    return encode(fmt, IEEE, rng.uniform(-1.0, 1.0, n))


def small_ints(fmt, n, seed, rank):
    """Integers in {-1, 0, 1} as (codes, int32 values): every partial sum of up to 8 ranks is at most 8 in magnitude
    and exact in both formats."""
    rng = np.random.default_rng([seed, rank, 1])
    v = rng.integers(-1, 2, n).astype(np.int32)
    return encode(fmt, IEEE, v.astype(np.float64)), v


def finite_nonzero(fmt, n, seed, rank):
    """Random finite nonzero codes (normals and subnormals of both signs)."""
    rng = np.random.default_rng([seed, rank, 2])
    mag = rng.integers(1, MAX_CODE[fmt] + 1, n).astype(np.uint8)
    return mag | (rng.integers(0, 2, n).astype(np.uint8) << np.uint8(7))


def random_bits(n, seed, rank):
    rng = np.random.default_rng([seed, rank, 3])
    return rng.integers(0, 256, n).astype(np.uint8)


def ties(fmt, n, seed, rank):
    """TIES-like data: +-0, NaN codes of both signs, the largest magnitudes (+-inf for E5M2) and a few small values,
    so that operand order shows in MAX / MIN (which zero, which NaN code) and NaNs and overflows meet in SUM."""
    one = 0x38 if fmt == E4M3 else 0x3C
    top = [0x7F, 0xFF, 0x7E, 0xFE, 0x7D, 0xFD] if fmt == E4M3 else [0x7F, 0xFF, 0x7D, 0xFE, 0x7C, 0xFC, 0x7B, 0xFB]
    pool = np.array([0x00, 0x80, one, one | 0x80, one, 0x01, 0x81, 0x40, 0xC0] + top, dtype=np.uint8)
    rng = np.random.default_rng([seed, rank, 4])
    return pool[rng.integers(0, pool.size, n)]
