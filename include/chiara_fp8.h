/*
 * chiara_fp8.h -- OCP FP8 (E4M3 / E5M2) ops and scaled casts on the user-op interface (libchiara_fp8.so).
 *
 * libchiara.so's kernel set and type table are closed; like the binary16 ops (chiara_ops.h) and the struct ops
 * (chiara_numerics.h), the 8-bit floats ship in a shared object of their own, built through
 * include/chiara_user_op.hpp exactly as a caller's op would be and registered with chr_op_create_tree.
 *
 * Formats.  OCP 8-bit floating point, not the fnuz variants:
 *   CHR_FP8_E4M3  e4m3fn: bias 7, subnormals, max 448 (0x7E), no infinities, NaN 0x7F / 0xFF
 *   CHR_FP8_E5M2  e5m2:   bias 15, subnormals, max 57344 (0x7B), +-inf 0x7C / 0xFC, NaN 0x7D..0x7F / 0xFD..0xFF
 * Elements are 1 byte and travel as CHR_UINT8 (CHR_FP8_DTYPE): the library moves them, the op gives them their
 * meaning.  The canonical NaN is 0x7F (E4M3) and 0x7E (E5M2): positive, whatever produced it.
 *
 * Arithmetic, with MPI's convention x o y = f(in = x, inout = y):
 *   SUM   the real-number inout + in of the decoded values, rounded once to the format, round-to-nearest-even
 *         (computed in f32 and converted once: 24 >= 2 * 4 + 2 bits, so the double rounding is innocuous).  Subnormal
 *         operands and results kept, signed zeros as IEEE, any NaN result canonical.
 *   PROD  inout * in, the same rules (every product of two 8-bit floats is exact in f32).
 *   Overflow of SUM and PROD is decided as if the exponent were unbounded: a magnitude up to max plus half an ulp,
 *   tie to even, rounds to max (E4M3 464 -> 448: the tie's even side is max; E5M2 61440 -> inf: the even side is up).
 *   Beyond that
 *     CHR_FP8_IEEE      E4M3 gives the canonical NaN, E5M2 gives +-inf;
 *     CHR_FP8_SATURATE  the f32 result is clamped to [-max, +max] before the conversion when it is not NaN, so
 *                       overflow and E5M2 infinities give +-max; inf - inf, 0 * inf and NaN operands still give the
 *                       canonical NaN.
 *   MAX   dec(inout) > dec(in) ? inout : in -- the library's float rule (a tie, +-0, or an unordered compare returns
 *         `in`); the chosen operand's byte passes through untouched, NaN codes included.  Independent of the policy.
 *   MIN   dec(inout) < dec(in) ? inout : in, likewise.
 * All ops are created commutative and carry both launchers (folds through k_fold, the flat schedules' expression
 * trees in one pass through k_tree).  A call with any dtype other than CHR_UINT8, derived types included, is declined
 * by both launchers: CHR_ERR_UNSUPPORTED, nothing enqueued.
 */
#ifndef CHIARA_FP8_H
#define CHIARA_FP8_H

#include "chiara.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHR_FP8_DTYPE CHR_UINT8 /* elements travel as bytes; the op gives them meaning */
typedef enum { CHR_FP8_E4M3 = 0, CHR_FP8_E5M2 = 1 } chr_fp8_format; /* OCP e4m3fn / e5m2, not fnuz */
typedef enum { CHR_FP8_IEEE = 0, CHR_FP8_SATURATE = 1 } chr_fp8_overflow;

/* The op of `kind` (CHR_SUM, CHR_PROD, CHR_MAX or CHR_MIN) on format `f` under overflow policy `o`.  Any other kind,
 * or a format or policy outside the enums: CHR_ERR_UNSUPPORTED, nothing registered.  MAX and MIN do not depend on `o`:
 * both values return the same code, so at most 12 of the 64 user-op codes are taken.  The first call for a
 * combination registers it (chr_op_create_tree; a full registry returns the registry's own error), later calls return
 * the same code.  Loading the library registers nothing.  Thread-safe.  op == NULL: CHR_ERR_INVALID_ARG. */
int chr_fp8_op(chr_fp8_format f, chr_op kind, chr_fp8_overflow o, chr_op* op);

/* dst[i] = enc_f,o(f32(src[i]) * scale), i < n: one f32 multiply (round-to-nearest-even, f32 subnormals kept, never
 * contracted), then the conversion rule of SUM above with policy `o`, infinite products included; NaN gives the
 * canonical NaN.  src_type is CHR_FLOAT32 or CHR_BFLOAT16; dst holds n bytes. */
int chr_fp8_quantize(void* dst, const void* src, size_t n, chr_dtype src_type, chr_fp8_format f, float scale,
                     chr_fp8_overflow o, hipStream_t s);

/* dst[i] = round_dst(dec_f(src[i]) * scale), i < n: one f32 multiply; for CHR_BFLOAT16 one more round-to-nearest-even
 * (the library's f32 -> bf16).  A NaN result is 0x7FC00000 / 0x7FC0.  dst_type is CHR_FLOAT32 or CHR_BFLOAT16.
 *
 * Both casts are streaming kernels of this library (16-B vectors where both pointers are 16-B aligned, element-wise
 * otherwise and for the tail), enqueued on `s`, returning at once.  n == 0 enqueues nothing.  Source and destination
 * may not overlap; a call writes exactly its n output elements.  A NULL pointer: CHR_ERR_INVALID_ARG; another dtype
 * or a value outside the enums: CHR_ERR_UNSUPPORTED; a failed launch: CHR_ERR_HIP. */
int chr_fp8_dequantize(void* dst, const void* src, size_t n, chr_dtype dst_type, chr_fp8_format f, float scale,
                       hipStream_t s);

/* Frees every op this library holds (chr_op_free): their codes go back to the 64.  A later chr_fp8_op registers
 * again, possibly under another code.  No call using one of the ops may be in flight. */
int chr_fp8_release(void);

/* What the library asked of the launchers since the last reset: out[0] fold-launcher calls, out[1] tree-launcher
 * calls, out[2] trees handed over (declined calls included).  reset != 0 zeroes the counters after reading. */
void chr_fp8_stats(long out[3], int reset);

#ifdef __cplusplus
}
#endif

#endif /* CHIARA_FP8_H */
