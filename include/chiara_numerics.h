/*
 * chiara_numerics.h -- first-party struct ops on the derived-type interface (libchiara_numerics.so).
 *
 * chr_type_contiguous describes an element that is a struct of K base values; the two reductions callers ask an
 * allreduce library for on such elements ship here, built through include/chiara_user_op.hpp exactly as a caller's
 * own op would be and registered with chr_op_create_tree.  A C caller without hipcc, or a Python caller
 * (chiara_amd/numerics.py), links or loads libchiara_numerics.so beside libchiara.so.  libchiara.so and
 * libchiara_ops.so gain no kernel and no symbol.
 *
 * The base type B is CHR_FLOAT32 or CHR_FLOAT64.  With MPI's convention x o y = f(in = x, inout = y), every operation
 * in B, each rounded once, no contraction; qNaN is 0x7FC00000 / 0x7FF8000000000000.
 *
 * sum2 -- a double-word SUM, element {hi, lo} = chr_type_contiguous(2, B).  `hi` carries the sum, `lo` its rounding
 * error, about twice B's precision through any expression tree, so that on well-conditioned data `hi` is the correctly
 * rounded exact sum whatever the geometry (n, k, b) or schedule:
 *
 *   two_sum(a, b):  if |a| < |b| swap(a, b);  s = a + b;  e = b - (s - a);  return (s, e)
 *   fast(a, b):     s = a + b;  e = b - (s - a);  return (s, e)
 *
 *   s = x.hi + y.hi
 *   if s is not finite:            return { s is NaN ? qNaN : s, +0 }
 *   (sh, sl) = two_sum(x.hi, y.hi);   (th, tl) = two_sum(x.lo, y.lo)
 *   c = sl + th;  (vh, vl) = fast(sh, c);  w = tl + vl;  (zh, zl) = fast(vh, w)
 *   if zh is not finite:           return { zh is NaN ? qNaN : zh, +0 }
 *   return { zh, zl }
 *
 * two_sum orders its operands by magnitude: the branch-free form computes s - b first, which overflows next to the
 * largest finite values and made the result depend on the operand order.  As written, f(x, y) and f(y, x) are
 * bit-identical on normalised operands (|lo| <= ulp(hi) / 2), and every finite result is normalised.
 *
 * moments -- mean / variance records {n, mean, M2} = chr_type_contiguous(3, B), n a count held in B, merged with Chan's
 * formula:
 *
 *   y_first = (y.n > x.n) or (y.n == x.n and y.mean < x.mean)
 *   (a, b) = y_first ? (y, x) : (x, y)                       -- a: the record with more samples
 *   n = a.n + b.n
 *   if n is NaN:  return { qNaN, qNaN, qNaN }
 *   z = (b.n == 0);  w = z ? +0 : b.n / n;  t = z ? +0 : (a.n * b.n) / n;  d = b.mean - a.mean
 *   return { n, canon(a.mean + d * w), canon((x.M2 + y.M2) + (d * d) * t) }     -- canon: NaN -> qNaN
 *
 * {0, 0, 0} is the identity up to the sign of zero components; `/` is the correctly rounded IEEE quotient, subnormal
 * results included.  The variance of the merged samples is M2 / n (or / (n - 1)).
 *
 * Both ops are created commutative with both launchers: folds through k_fold, the flat schedules' expression trees in
 * one pass through k_tree (the 12- and 24-byte records element-wise).  The launchers read a call's dtype at run time
 * (chr_type_get_contiguous) and take any live type of the right content -- the caller's own
 * chr_type_contiguous(2, CHR_FLOAT32) as well as chr_num_sum2_type's; every other dtype (predefined types, another
 * count, another base) is declined with nothing enqueued and the library returns CHR_ERR_UNSUPPORTED.
 */
#ifndef CHIARA_NUMERICS_H
#define CHIARA_NUMERICS_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>

#include "chiara.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The op (one op serves both bases).  The first call registers it (chr_op_create_tree: one of the 64 user-op codes; a
 * full registry returns the registry's own error), later calls return the same code until chr_num_release.  Loading
 * the library registers nothing.  Thread-safe.  op == NULL: CHR_ERR_INVALID_ARG. */
int chr_num_sum2(chr_op* op);
int chr_num_moments(chr_op* op);

/* The element type for `base` (CHR_FLOAT32 or CHR_FLOAT64; any other: CHR_ERR_UNSUPPORTED): chr_type_contiguous(2,
 * base) and (3, base), created on the first call (one of the 64 type codes) and cached until chr_num_release.
 * type == NULL: CHR_ERR_INVALID_ARG. */
int chr_num_sum2_type(chr_dtype base, chr_dtype* type);
int chr_num_moments_type(chr_dtype base, chr_dtype* type);

/* Streaming conversions on device buffers, enqueued on `s`; the call returns at once.  n == 0 enqueues nothing.
 * Source and destination may not overlap.  Each call writes exactly its n output elements.  A NULL pointer where one
 * is required: CHR_ERR_INVALID_ARG; a base other than the two: CHR_ERR_UNSUPPORTED; a failed launch: CHR_ERR_HIP.
 *   sum2_pack       pairs[i] = {values[i], +0}
 *   sum2_unpack     values[i] = pairs[i].hi
 *   moments_pack    recs[i] = {1, samples[i], +0}
 *   moments_unpack  count[i], mean[i], m2[i] = recs[i]; any of the three outputs may be NULL (not all) */
int chr_num_sum2_pack(void* pairs, const void* values, size_t n, chr_dtype base, hipStream_t s);
int chr_num_sum2_unpack(void* values, const void* pairs, size_t n, chr_dtype base, hipStream_t s);
int chr_num_moments_pack(void* recs, const void* samples, size_t n, chr_dtype base, hipStream_t s);
int chr_num_moments_unpack(void* count, void* mean, void* m2, const void* recs, size_t n, chr_dtype base,
                           hipStream_t s);

/* Frees the ops (chr_op_free) and the cached types (chr_type_free): their codes go back to the 64 + 64.  A later
 * request registers again, possibly under another code.  No call using them may be in flight. */
int chr_num_release(void);

/* What the library asked of the launchers since the last reset: out[0] fold-launcher calls, out[1] tree-launcher
 * calls, out[2] trees handed over (declined calls included).  reset != 0 zeroes the counters after reading. */
void chr_num_stats(long out[3], int reset);

#ifdef __cplusplus
}
#endif

#endif /* CHIARA_NUMERICS_H */
