"""Operand-domain tables for the reduction kernels' element arithmetic, and a numpy restatement of that arithmetic
written independently of oracle/chiara_oracle.c (tests/test_operand_domain.py holds the oracle to it on the CPU,
tests/test_gpu_operand_domain.py holds every kernel path to the oracle on the device).

A table is a pair of flat arrays (x, y) = (in, inout) of MPI_Reduce_local holding every combination of an operand set
with a partner set (x = np.repeat, y = np.tile; table(dtype, INOUT_MAJOR) lists the same cells the other way round, so
that `in` too varies from lane to lane).  Everything is deterministic; arrays are built from bit patterns, so
signalling NaNs and padding bytes are what the table says, and are handed out read-only.

  i8 / u8    all 256 x 256 pairs
  i16 / u16  all 65 536 values x 64 partners (sign, byte and power-of-two boundaries, a fixed-seed remainder)
  i32 .. u64 an edge set (0, +-1, both signednesses' limits, 2^k, 2^k +- 1 and their negations, 0x80 / 0xFF at each byte)
             squared
  bf16       all 65 536 bit patterns x 512 partners: every 4th of the sorted {sign} x {exponent 0..255} x
             {mantissa 0, 1, 0x40, 0x7F}, i.e. +-0, every power of two and +-inf
  f32        {sign} x {exponent 0..255} x {mantissa 0, 1, 1 << 22, all ones} squared
  f64        the same with exponents 0..63, 960..1089, 1984..2047
  cf / cd    each part from 32 values (+-0, +-1, subnormal / normal / finite limits, +-inf, a quiet and a signalling
             NaN, numbers whose squares overflow and underflow); 1 024 complex values squared
  pairs      64 edge values x 5 indices (INT32_MIN, -1, 0, 1, INT32_MAX) = 320 elements, squared; the padding bytes of
             di / li / si hold a non-zero pattern per element, another one on either side
"""
import functools

import numpy as np

import pyoracle as po

ARITH, LOGIC, BITWISE = ("sum", "prod", "max", "min"), ("land", "lor", "lxor"), ("band", "bor", "bxor")
LOC = ("maxloc", "minloc")
INTS = ("i8", "u8", "i16", "u16", "i32", "u32", "i64", "u64")
PAIRS, CPLX = ("fi", "di", "li", "2i", "si"), ("cf", "cd")
DTYPES = ("f32", "f64", "i32", "bf16", "i8", "u8", "i16", "u16", "u32", "i64", "u64") + PAIRS + CPLX

# (unsigned type of the bit pattern, exponent bits, mantissa bits)
FMT = {"f32": (np.uint32, 8, 23), "f64": (np.uint64, 11, 52), "bf16": (np.uint16, 8, 7)}
PART = {"cf": "f32", "cd": "f64", "fi": "f32", "di": "f64"}  # the floating format inside a complex / pair element


def valid_ops(dtype):
    """MPICH 3.3.2's (type, op) table (include/chiara.h), restated."""
    if dtype in PAIRS:
        return LOC
    if dtype in CPLX:
        return ("sum", "prod")
    if dtype == "bf16":
        return ARITH
    return ARITH + LOGIC + (BITWISE if dtype in INTS else ())


def _uint(bits):
    return {8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}[bits]


def _raw(a):
    """One opaque item per element, whatever the type: what repeat / tile / roll move without looking inside."""
    es = a.dtype.itemsize
    a = np.ascontiguousarray(a)
    if es in (1, 2, 4, 8):
        return a.view(np.uint8).view(_uint(8 * es))
    return a.view(np.uint8).view(np.dtype((np.void, es)))


def _cross(a, b):
    """(x, y): every element of a as `in` against every element of b as `inout`."""
    x = np.repeat(_raw(a), b.size).view(np.uint8).view(a.dtype)
    y = np.tile(_raw(b), a.size).view(np.uint8).view(b.dtype)
    x.flags.writeable = y.flags.writeable = False
    return x, y


def rotate(a, k):
    """a rotated by k elements (element i of the result is a[i - k]), padding bytes kept."""
    return np.roll(_raw(a), k).view(np.uint8).view(a.dtype)


def _fill_to(vals, count, bits, seed):
    """vals without repeats, then fixed-seed random `bits`-bit values up to `count` entries."""
    out = list(dict.fromkeys(int(v) & ((1 << bits) - 1) for v in vals))
    assert len(out) <= count, (len(out), count)
    rng = np.random.default_rng(seed)
    while len(out) < count:
        v = int(rng.integers(0, 1 << 62)) & ((1 << bits) - 1)
        if v not in out:
            out.append(v)
    return np.array(out, dtype=np.uint64).astype(_uint(bits))


def partners16():
    vals = [0, 1, 2, 0xFFFF, 0x7FFF, 0x8000, 0x8001, 0x00FF, 0x0100, 0xFF00, 0x0080]
    vals += [1 << k for k in range(16)] + [(1 << k) - 1 for k in range(1, 17)]
    return _fill_to(vals, 64, 16, 16)


def int_edges(bits):
    top, ones = 1 << (bits - 1), (1 << bits) - 1
    v = {0, 1, ones, top, top + 1, top - 1, top - 2, ones - 1}  # 0, +-1; min, min + 1, max, max - 1 of either sign
    for k in range(bits):
        for e in ((1 << k), (1 << k) + 1, (1 << k) - 1):  # 2^k - 1: all ones below bit k
            v |= {e & ones, -e & ones}
    for j in range(bits // 8):
        v |= {0x80 << (8 * j), 0xFF << (8 * j)}
    assert len(v) <= 1024
    return np.array(sorted(v), dtype=np.uint64).astype(_uint(bits))


def float_edges(fmt, exps, mants):
    """{sign} x exps x mants as bit patterns, sorted."""
    udt, ebits, mbits = FMT[fmt]
    s, e, m = np.meshgrid(np.arange(2, dtype=np.uint64), np.asarray(exps, dtype=np.uint64),
                          np.asarray(mants, dtype=np.uint64), indexing="ij")
    return np.sort(((s << np.uint64(ebits + mbits)) | (e << np.uint64(mbits)) | m).ravel()).astype(udt)


def _bits_of(values, fmt):
    fdt = np.float32 if fmt == "f32" else np.float64
    a = np.array(values, dtype=np.float64).astype(fdt)
    assert np.array_equal(a.astype(np.float64), np.array(values, dtype=np.float64))  # exactly representable
    return [int(b) for b in a.view(FMT[fmt][0])]


QNAN = {"f32": 0x7FC12345, "f64": 0x7FF8000012345678}
SNAN = {"f32": 0xFFA54321, "f64": 0xFFF4000087654321}  # quiet bit clear, sign set


def complex_parts(fmt):
    """The 32 part values of the complex tables, as bit patterns."""
    _, ebits, mbits = FMT[fmt]
    emin, emax = 2 - (1 << (ebits - 1)), (1 << (ebits - 1)) - 1  # -126 / 127, -1022 / 1023
    mags = [0.0, 1.0, 2.0 ** (emin - mbits), 2.0 ** emin - 2.0 ** (emin - mbits), 2.0 ** emin,
            (2.0 - 2.0 ** -mbits) * 2.0 ** emax, np.inf]
    if fmt == "f32":  # squares: overflow, underflow to 0, just overflow, subnormal, overflow after rounding, ties to 0
        mags += [2.0 ** 100, 2.0 ** -100, 2.0 ** 64, 2.0 ** -70, 1.5 * 2.0 ** 63, 2.0 ** -75, 3.0, 1.0 + 2.0 ** -23]
    else:
        mags += [2.0 ** 600, 2.0 ** -600, 2.0 ** 512, 2.0 ** -520, 1.5 * 2.0 ** 511, 2.0 ** -538, 3.0, 1.0 + 2.0 ** -52]
    vals = _bits_of(mags, fmt) + _bits_of([-m for m in mags], fmt) + [QNAN[fmt], SNAN[fmt]]
    assert len(set(vals)) == 32
    return np.array(vals, dtype=np.uint64).astype(FMT[fmt][0])


def pair_values(dtype):
    """The 64 values of a pair table, as bit patterns of the value type."""
    if dtype in ("fi", "di"):
        fmt = PART[dtype]
        _, ebits, mbits = FMT[fmt]
        emin, emax = 2 - (1 << (ebits - 1)), (1 << (ebits - 1)) - 1
        mags = [0.0, 2.0 ** (emin - mbits), 2.0 ** emin - 2.0 ** (emin - mbits), 2.0 ** emin, 1.0,
                (2.0 - 2.0 ** -mbits) * 2.0 ** emax, np.inf, 1.0 + 2.0 ** -mbits, 2.0, 0.5, 3.0, 1.5,
                2.0 ** 10, 2.0 ** -10, 2.0 ** 50, 2.0 ** -50, 2.0 ** 100, 2.0 ** -100]
        vals = _bits_of(mags, fmt) + _bits_of([-m for m in mags], fmt) + [QNAN[fmt]]
        return _fill_to(vals, 64, 8 * FMT[fmt][0]().itemsize, 64)
    bits = {"li": 64, "2i": 32, "si": 16}[dtype]
    top = 1 << (bits - 1)
    vals = [0, 1, -1, 2, -2, 7, -7, top, top + 1, top - 1, top - 2, 0x7F, 0x80, 0xFF, 0x100, -0x80, -0x81, -0x100]
    for k in range(2, bits - 1, max(1, bits // 16)):
        vals += [1 << k, -(1 << k)]
    return _fill_to(vals, 64, bits, 64)


PAIR_INDICES = (-(2 ** 31), -1, 0, 1, 2 ** 31 - 1)


def pair_elements(dtype, side):
    """The 320 elements of a pair table; `side` (0: in, 1: inout) picks the padding pattern."""
    npdt = po.NP_DTYPES[dtype]
    v = np.repeat(pair_values(dtype), len(PAIR_INDICES))
    n, es = v.size, npdt.itemsize
    raw = ((np.arange(n)[:, None] * (7 + 6 * side) + np.arange(es)[None, :] + 100 * side) % 255 + 1).astype(np.uint8)
    a = raw.reshape(-1).view(npdt)
    a["v"] = v.view(npdt.fields["v"][0])
    a["i"] = np.tile(np.array(PAIR_INDICES, dtype=np.int32), n // len(PAIR_INDICES))
    return a


def operand_sets(dtype):
    """(a, b): the values `in` takes and the values `inout` takes."""
    npdt = np.dtype(po.NP_DTYPES[dtype])
    if dtype in ("i8", "u8"):
        v = np.arange(256, dtype=np.uint8).view(npdt)
        return (v, v)
    if dtype in ("i16", "u16"):
        return (np.arange(65536, dtype=np.uint16).view(npdt), partners16().view(npdt))
    if dtype in INTS:
        v = int_edges(8 * npdt.itemsize).view(npdt)
        return (v, v)
    if dtype == "bf16":
        return (np.arange(65536, dtype=np.uint16), float_edges("bf16", range(256), (0, 1, 0x40, 0x7F))[::4])
    if dtype == "f32":
        v = float_edges("f32", range(256), (0, 1, 1 << 22, 0x7FFFFF)).view(npdt)
        return (v, v)
    if dtype == "f64":
        exps = list(range(64)) + list(range(960, 1090)) + list(range(1984, 2048))
        v = float_edges("f64", exps, (0, 1, 1 << 51, (1 << 52) - 1)).view(npdt)
        return (v, v)
    if dtype in CPLX:
        p = complex_parts(PART[dtype])
        v = np.stack([np.repeat(p, p.size), np.tile(p, p.size)], axis=1).reshape(-1).view(npdt)  # (re, im)
        return (v, v)
    return (pair_elements(dtype, 0), pair_elements(dtype, 1))


IN_MAJOR, INOUT_MAJOR = "in-major", "inout-major"
ORDERS = (IN_MAJOR, INOUT_MAJOR)


@functools.lru_cache(maxsize=None)
def table(dtype, order=IN_MAJOR):
    """(x, y) = (in, inout), read-only: every combination of operand_sets(dtype), once.  In the in-major order `in` is
    repeated and `inout` tiled, so `in` is constant along a 16-byte vector and only `inout` varies from lane to lane; the
    inout-major order lists the same cells the other way round (`in` tiled, `inout` repeated).  Code that takes a
    neighbouring lane's operand by mistake shows only in the order in which that operand varies."""
    a, b = operand_sets(dtype)
    if order == IN_MAJOR:
        return _cross(a, b)
    y, x = _cross(b, a)
    return x, y


def reorder(r, dtype, order):
    """Per-cell results r of the in-major table, in `order`."""
    if order == IN_MAJOR:
        return r
    a, b = operand_sets(dtype)
    return np.ascontiguousarray(_raw(r).reshape(a.size, b.size).T).reshape(-1).view(np.uint8).view(r.dtype)


# ---- classes of floating bit patterns ------------------------------------------------------------------------------

def fbits(a, fmt):
    """The bit patterns of a's floating parts (a complex array gives two per element)."""
    return np.ascontiguousarray(a).view(np.uint8).view(FMT[fmt][0])


def fclass(u, fmt):
    """dict of boolean arrays over bit patterns u: nan, inf, sub (subnormal), negzero, finite, default_nan."""
    udt, ebits, mbits = FMT[fmt]
    sign = udt(1 << (ebits + mbits))
    expm = udt(((1 << ebits) - 1) << mbits)
    mant = udt((1 << mbits) - 1)
    e, m = u & expm, u & mant
    return {"nan": (e == expm) & (m != 0), "inf": (e == expm) & (m == 0), "sub": (e == 0) & (m != 0),
            "negzero": u == sign, "finite": e != expm,
            "default_nan": u == (sign | expm | udt(1 << (mbits - 1)))}  # x86's: sign set, quiet bit only


# ---- the numpy restatement -----------------------------------------------------------------------------------------

def _f_arith(op, a, b):
    """a op b in the host's IEEE arithmetic, a written first."""
    with np.errstate(all="ignore"):
        return a + b if op == "sum" else a * b


def np_reduce_local(x, y, dtype, op):
    """(r, undefined): r = inout after MPI_Reduce_local(in = x, inout = y), MPICH's loop inout = OP(inout, in);
    `undefined` marks the cells this restatement leaves open (SUM / PROD of two NaNs on f32 / f64 / bf16: which payload
    survives is up to the host's code generation), None where there are none.  None for the operations that have no
    numpy restatement (complex PROD, the pair types)."""
    npdt = np.dtype(po.NP_DTYPES[dtype])
    if dtype in PAIRS or (dtype in CPLX and op == "prod"):
        return None
    if dtype in CPLX:  # SUM by parts, in + inout; of two NaNs in a part in's survives, quieted
        fmt = PART[dtype]
        udt, _, mbits = FMT[fmt]
        fdt = np.float32 if fmt == "f32" else np.float64
        xf, yf = x.view(fdt), y.view(fdt)
        r = _f_arith("sum", xf, yf)
        both = np.isnan(xf) & np.isnan(yf)
        r.view(udt)[both] = xf.view(udt)[both] | udt(1 << (mbits - 1))
        return r.view(npdt), None
    if dtype in INTS:
        udt = _uint(8 * npdt.itemsize)
        ux, uy = x.view(udt), y.view(udt)
        if op == "sum":
            return (uy + ux).view(npdt), None  # unsigned arrays wrap at the element width
        if op == "prod":
            return (uy * ux).view(npdt), None
        if op in ("max", "min"):
            return np.where(y > x if op == "max" else y < x, y, x), None
        if op in LOGIC:
            tx, ty = x != 0, y != 0
            t = tx & ty if op == "land" else tx | ty if op == "lor" else tx ^ ty
            return t.astype(npdt), None
        return (uy & ux if op == "band" else uy | ux if op == "bor" else uy ^ ux).view(npdt), None
    if dtype == "bf16":  # widen, f32 op, RNE; a NaN result is quieted as (u >> 16) | 0x40
        fx = (x.astype(np.uint32) << np.uint32(16)).view(np.float32)
        fy = (y.astype(np.uint32) << np.uint32(16)).view(np.float32)
        if op in ("max", "min"):
            return np.where(fy > fx if op == "max" else fy < fx, y, x), None
        r = _f_arith(op, fy, fx)
        u = r.view(np.uint32).astype(np.uint64)
        rne = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
        out = np.where(np.isnan(r), (u >> np.uint64(16)) | np.uint64(0x40), rne).astype(np.uint16)
        return out, np.isnan(fx) & np.isnan(fy)
    if op in ("sum", "prod"):
        return _f_arith(op, y, x), np.isnan(x) & np.isnan(y)
    if op in ("max", "min"):
        return np.where(y > x if op == "max" else y < x, y, x), None
    tx, ty = x != 0, y != 0  # C truth: NaN is true, -0 false
    t = tx & ty if op == "land" else tx | ty if op == "lor" else tx ^ ty
    return t.astype(npdt), None


# ---- reporting -----------------------------------------------------------------------------------------------------

def cells(a):
    """Per-element bit patterns: unsigned integers, or for pair / 16-byte elements one row of bytes each."""
    es = a.dtype.itemsize
    a = np.ascontiguousarray(a)
    if a.dtype.names is None and es in (1, 2, 4, 8):
        return a.view(_uint(8 * es))
    return a.view(np.uint8).reshape(-1, es)


def _hex(c, i):
    return f"0x{int(c[i]):0{2 * c.dtype.itemsize}x}" if c.ndim == 1 else "bytes:" + c[i].tobytes().hex()


def assert_cells_equal(got, want, x, y, dtype, op, path, keep=None):
    """got == want bit for bit (where `keep`, if given); the failure names dtype, op, path, the number of wrong cells
    and the first 8 as hex (in, inout, got, want)."""
    g, w = cells(got), cells(want)
    assert g.shape == w.shape, f"{dtype} {op} {path}: {g.shape} results for {w.shape} cells"
    bad = g != w
    if bad.ndim == 2:
        bad = bad.any(axis=1)
    if keep is not None:
        bad &= keep
    if not bad.any():
        return
    idx = np.flatnonzero(bad)
    cx, cy = cells(x), cells(y)
    first = ", ".join(f"[{i}] ({_hex(cx, i)}, {_hex(cy, i)}, {_hex(g, i)}, {_hex(w, i)})" for i in idx[:8])
    raise AssertionError(f"{dtype} {op} {path}: {idx.size} of {bad.size} cells wrong; "
                         f"first [cell] (in, inout, got, want): {first}")
