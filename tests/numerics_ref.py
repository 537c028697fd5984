"""Reference for the struct ops of libchiara_numerics.so (include/chiara_numerics.h): a numpy restatement of the two
functors over (n, K) row views, as tests/struct_ref.py's halfadd / rotmix are written, and the partner lists of the
operand-domain tests.  Host only.  Folds, trees and whole collectives come from struct_ref.fold_ref, tree_ref and
simulate with these functors passed in.

Every operation is one numpy operation on arrays of the base type (float32 or float64): numpy rounds each once, to
nearest even, keeps subnormals and contracts nothing, which is the contract the device code is built to
(-fno-fast-math -ffp-contract=off).  NaN results are written as bits, so the canonical quiet NaN is exact."""
import math

import numpy as np

QNAN_BITS = {np.dtype(np.float32): np.uint32(0x7FC00000), np.dtype(np.float64): np.uint64(0x7FF8000000000000)}
UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}
BASES = (np.float32, np.float64)


def bits(a):
    """The elements' bit patterns (uint32 / uint64 view)."""
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype])


def _canon(r):
    """NaN -> the canonical quiet NaN, every other value's bits untouched."""
    return np.where(np.isnan(r), QNAN_BITS[r.dtype], bits(r)).astype(UINT[r.dtype]).view(r.dtype)


def _fast(a, b):
    s = a + b
    return s, b - (s - a)


def _two_sum(a, b):
    sw = np.abs(a) < np.abs(b)
    return _fast(np.where(sw, b, a), np.where(sw, a, b))


def sum2(x, y):
    """x o y = f(in = x, inout = y) on {hi, lo} rows: the double-word sum of include/chiara_numerics.h."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.dtype == y.dtype and x.shape == y.shape and x.shape[1] == 2
    xh, xl, yh, yl = x[:, 0], x[:, 1], y[:, 0], y[:, 1]
    with np.errstate(all="ignore"):
        s = xh + yh
        sh, sl = _two_sum(xh, yh)
        th, tl = _two_sum(xl, yl)
        c = sl + th
        vh, vl = _fast(sh, c)
        w = tl + vl
        zh, zl = _fast(vh, w)
    early, late = ~np.isfinite(s), ~np.isfinite(zh)
    zero = np.zeros_like(s)
    out = np.empty_like(x)
    out[:, 0] = np.where(early, _canon(s), np.where(late, _canon(zh), zh))
    out[:, 1] = np.where(early | late, zero, zl)
    # np.where moves NaNs as values; write their bits again so that the canonical NaN stays exact
    out[:, 0] = _canon(out[:, 0])
    return out


def moments(x, y):
    """x o y on {n, mean, M2} rows: Chan's merge of include/chiara_numerics.h."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.dtype == y.dtype and x.shape == y.shape and x.shape[1] == 3
    zero = np.zeros(x.shape[0], dtype=x.dtype)
    with np.errstate(all="ignore"):
        y_first = (y[:, 0] > x[:, 0]) | ((y[:, 0] == x[:, 0]) & (y[:, 1] < x[:, 1]))
        an, am = np.where(y_first, y[:, 0], x[:, 0]), np.where(y_first, y[:, 1], x[:, 1])
        bn, bm = np.where(y_first, x[:, 0], y[:, 0]), np.where(y_first, x[:, 1], y[:, 1])
        n = an + bn
        z = bn == 0
        w = np.where(z, zero, bn / n)
        t = np.where(z, zero, (an * bn) / n)
        d = bm - am
        mean = am + d * w
        m2 = (x[:, 2] + y[:, 2]) + (d * d) * t
    nan = np.isnan(n)
    q = QNAN_BITS[x.dtype]
    out = np.empty(x.shape, dtype=UINT[x.dtype])
    out[:, 0] = np.where(nan, q, bits(n))
    out[:, 1] = np.where(nan, q, bits(_canon(mean)))
    out[:, 2] = np.where(nan, q, bits(_canon(m2)))
    return out.view(x.dtype)


FUNCTORS = {"sum2": (sum2, 2), "moments": (moments, 3)}


# ---- packing, as the library's pack kernels do it -----------------------------------------------------------------

def sum2_pack(v):
    out = np.zeros((v.size, 2), dtype=v.dtype)
    out[:, 0] = v
    return out.reshape(-1)


def moments_pack(v):
    out = np.zeros((v.size, 3), dtype=v.dtype)
    out[:, 0] = 1
    out[:, 1] = v
    return out.reshape(-1)


# ---- the partner lists of the operand-domain tests ------------------------------------------------------------------

def _from_bits(T, b):
    return np.array(b, dtype=UINT[np.dtype(T)]).view(T)


def sum2_partners(T):
    """2 020 {hi, lo} pairs as a (2020, 2) array.  hi: +-0, +- smallest and largest subnormal, +- smallest normal, +-1,
    1 + eps, +-eps/2, 3, +-max, +-max/2, max (1 - eps), +-inf, a quiet, a signalling and a negative NaN -- 24 values --
    then random bit patterns up to 2 020.  lo: 0 with probability 1/4, else uniform within half the distance from |hi|
    to the next value towards zero (so |lo| <= ulp(hi) / 2, a normalised pair), and 0 where hi is 0 or not finite."""
    T = np.dtype(T).type
    fi = np.finfo(T)
    U = UINT[np.dtype(T)]
    nbits = 8 * np.dtype(T).itemsize
    sub_lo, sub_hi = _from_bits(T, [1])[0], _from_bits(T, [(1 << fi.nmant) - 1])[0]
    exp_all = ((1 << (nbits - 1 - fi.nmant)) - 1) << fi.nmant
    nans = _from_bits(T, [exp_all | (1 << (fi.nmant - 1)), exp_all | 1, (1 << (nbits - 1)) | exp_all | (1 << (fi.nmant - 1)) | 5])
    special = [T(0), -T(0), sub_lo, -sub_lo, sub_hi, -sub_hi, fi.tiny, -fi.tiny, T(1), T(-1), T(1) + fi.eps,
               fi.eps / T(2), -fi.eps / T(2), T(3), fi.max, -fi.max, fi.max / T(2), -fi.max / T(2),
               fi.max * (T(1) - fi.eps), T(np.inf), T(-np.inf)]
    special = np.concatenate([np.array(special, dtype=T), nans])
    assert special.size == 24
    rng = np.random.default_rng([2020, nbits])
    fill = rng.integers(0, 1 << nbits, 2020 - special.size, dtype=np.uint64).astype(U).view(T)
    hi = np.concatenate([special, fill])
    with np.errstate(all="ignore"):
        mag = np.abs(hi)
        ulp = np.where(np.isfinite(hi), mag - np.nextafter(mag, T(0)), T(0)).astype(np.float64)
        u = rng.uniform(-1.0, 1.0, hi.size)
        lo = np.where(rng.integers(0, 4, hi.size) == 0, 0.0, u * 0.5 * ulp).astype(T)
    out = np.empty((hi.size, 2), dtype=T)
    out[:, 0], out[:, 1] = hi, lo
    assert out.shape == (2020, 2)
    return out


def moments_partners(T):
    """The 13 x 14 x 8 = 1 456 records n x mean x M2 as a (1456, 3) array."""
    T = np.dtype(T).type
    fi = np.finfo(T)
    sub = _from_bits(T, [1])[0]
    ns = [0.0, -0.0, 1, 2, 3, 7, 1e6, 2.0 ** 24, np.inf, -np.inf, np.nan, -1, 0.5]
    means = [T(0), -T(0), T(1), T(-1), T(100), T(100) * (T(1) + fi.eps), fi.max, -fi.max, fi.tiny, sub, T(np.inf),
             T(-np.inf), T(np.nan), T(1e-3)]
    m2s = [T(0), -T(0), T(1), T(2.5), fi.max, T(np.inf), T(np.nan), sub]
    out = np.array([(T(n), m, q) for n in ns for m in means for q in m2s], dtype=T)
    assert out.shape == (1456, 3)
    return out


def cross(p):
    """Every ordered pair of the rows of p: (x, y), each (len(p)^2, K); x varies slowest."""
    n = p.shape[0]
    return np.repeat(p, n, axis=0), np.tile(p, (n, 1))


# ---- the data of the geometry-independence and moments statements ----------------------------------------------------

GEOMETRIES = [(8, 4, 4), (8, 2, 2), (8, 2, 8), (8, 8, 1)]
INDEP_COUNT = 8 * 257


def independence_data(T, seed=31):
    """Eight ranks of well-conditioned values: uniform in (-1, 1) scaled by 2^-8 .. 2^8, one generator, rank order."""
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-1, 1, INDEP_COUNT) * np.exp2(rng.integers(-8, 9, INDEP_COUNT))).astype(T) for _ in range(8)]


def exact_sum(values):
    """T(math.fsum(...)) per element: the exact sum of the ranks' values rounded to float64 by fsum, then to T.  For
    float32 the exact sum of eight 24-bit values of comparable scale fits a float64's 53 bits, so the conversion is
    in practice the only rounding."""
    T = values[0].dtype.type
    cols = np.stack([v.astype(np.float64) for v in values])
    return np.array([T(math.fsum(cols[:, i])) for i in range(cols.shape[1])], dtype=T)


def moments_data(T):
    """Eight ranks of one sample each: mean 1000, sigma 3."""
    rng = np.random.default_rng(7)
    return [(rng.standard_normal(2056) * 3 + 1000).astype(T) for _ in range(8)]
