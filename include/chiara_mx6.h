/*
 * chiara_mx6.h -- MXFP6 block-scaled SUM and casts on the user-op interface (libchiara_mx6.so).
 *
 * The 6-bit members of the OCP Microscaling family beside chiara_mx.h's MXFP8 and chiara_mx4.h's MXFP4: the same E8M0
 * block scales, the same rule, 400 bytes per 512 values on the wire against 528 and 272.  Three or two mantissa bits
 * survive a sum that is requantised at every node of a tree where MXFP4's single bit does not.  Like every first-party
 * op it ships in a shared object of its own, registered with chr_op_create; its kernels are hand-written
 * (csrc/ops/mx6_ops.hip, csrc/ops/mx6_tile.hpp).
 *
 * Formats (chr_mx6_format), a code being six bits:
 *                      CHR_MX6_E2M3  `s ee mmm`            CHR_MX6_E3M2  `s eee mm`
 *   bias               1                                   3
 *   ee / eee == 0      the subnormals m / 8                the subnormals m / 4 * 2^-2 (the smallest is 0.0625)
 *   otherwise          (1 + m / 8) * 2^(ee - 1)            (1 + m / 4) * 2^(eee - 3)
 *   max                7.5 = 0.9375 * 2^3                  28 = 0.875 * 2^5
 * Neither format has a NaN code or an infinity.  -0 is code 0x20.
 *
 * Element: the MX6 tile, CHR_MX6_TILE_VALUES = 512 values in CHR_MX6_TILE_BYTES = 400 bytes (16 + 16 x 24), shared by
 * both formats:
 *   bytes 0 .. 15                         the E8M0 scales of blocks 0 .. 15: bias 127, value 2^(scale - 127); 0xFF is
 *                                         the NaN scale
 *   bytes 16 + 24 b .. 16 + 24 b + 23     the 32 codes of block b, a 192-bit little-endian string: code i occupies
 *                                         bits 6 i .. 6 i + 5 of it (bit k of the string is bit k % 8 of byte k / 8)
 * The type is chr_type_contiguous(100, CHR_UINT32) (chr_mx6_type): every count is in tiles, and no message, slice or
 * fold begins inside a block.  A NaN exists only as a block whose scale is 0xFF, and the canonical NaN block is scale
 * 0xFF with twenty-four 0x00 code bytes.  Value i of a block is dec(code i) * 2^(scale - 127).
 *
 * SUM, with MPI's convention x o y = f(in = x, inout = y), per block with scales ex, ey and codes px[i], py[i].  Every
 * operation is in f32, rounded once to nearest even, f32 subnormals kept, nothing contracted -- chiara_mx4.h's steps,
 * changed only where the format forces it:
 *   1. ex == 0xFF or ey == 0xFF: the result is the canonical NaN block.
 *   2. e = max(ex, ey).
 *   3. s[i] = ldexp(dec(py[i]), ey - e) + ldexp(dec(px[i]), ex - e), dec being the format's own.  (One of the two
 *      shifts is 0; the other ldexp is exact or, below 2^-126, rounded once.  Relative to e no magnitude exceeds
 *      2 * max, so every s[i] is finite.)
 *   4. amax = max |s[i]|.  amax == 0: e' = e, and the codes are the encoded signed zeros.
 *   5. Otherwise E is the smallest integer with amax * 2^-E <= max: with amax = f * 2^x, f in [0.5, 1), that is
 *      x - 3 + (f > 0.9375) for E2M3 and x - 5 + (f > 0.875) for E3M2.
 *   6. e' = clamp(e + E, 0, 254).
 *   7. p'[i] = enc_sat(ldexp(s[i], e - e')): one round-to-nearest to the format, ties to the even code, subnormals
 *      kept, clamped to +-max, the sign of a zero (and of a value that rounds to zero) kept.
 * The rule commutes bit for bit (f32 addition does, and the NaN block is canonical), so both operand orders of a fold
 * give the same bytes.  It is not associative: a result depends on the schedule's expression tree.
 *
 * The ops are created commutative and carry the fold launcher alone: the flat schedules' expression trees run fold by
 * fold through the library's scratch (chiara.h); chiara_mx6_tree.h has the same SUMs with one-pass trees.  Any dtype other than a live chr_type_contiguous(100, CHR_UINT32), and
 * any call with a pointer that is not 4-byte aligned, is declined: CHR_ERR_UNSUPPORTED, nothing enqueued.  A block
 * lies at byte 16 + 24 b of its tile, 8-byte aligned whenever the buffer is: pointers that are all 8-byte aligned take
 * 8-byte accesses, any others 4-byte ones; the bytes are the same.
 */
#ifndef CHIARA_MX6_H
#define CHIARA_MX6_H

#include "chiara.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHR_MX6_TILE_VALUES 512
#define CHR_MX6_TILE_BYTES 400

typedef enum { CHR_MX6_E2M3 = 0, CHR_MX6_E3M2 = 1 } chr_mx6_format;

/* The tile type, chr_type_contiguous(100, CHR_UINT32), shared by both formats: created on the first call (a full type
 * registry returns the registry's own error), the same code until chr_mx6_release.  The ops take any live type of that
 * content, the caller's own included.  type == NULL: CHR_ERR_INVALID_ARG.  Thread-safe. */
int chr_mx6_type(chr_dtype* type);

/* The SUM above on tiles of format `f`: one op per format, registered on the first call for it (chr_op_create,
 * commutative; a full registry returns the registry's own error), the same code until chr_mx6_release.  Loading the
 * library registers nothing.  A format outside the enum or op == NULL: CHR_ERR_INVALID_ARG.  Thread-safe. */
int chr_mx6_sum(chr_mx6_format f, chr_op* op);

/* The fold launchers those ops are registered with (chr_user_reduce_fn; running_first is not looked at), for a caller
 * that registers them itself. */
int chr_mx6_e2m3_sum_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dtype,
                          int running_first, hipStream_t stream, void* ctx);
int chr_mx6_e3m2_sum_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dtype,
                          int running_first, hipStream_t stream, void* ctx);

/* tiles = Q(src): the n values of src (CHR_FLOAT32 or CHR_BFLOAT16, widened exactly) become ceil(n / 512) whole
 * tiles.  Per block, steps 4 - 7 of SUM with s[i] = src[i] (the sign of a zero is kept) and e = 127: the scale is the
 * smallest that fits the block's amax, and an all-zero block gets scale 0.  A block with any non-finite source value
 * becomes the canonical NaN block, the OCP convention for a format without a NaN code.  Values beyond n count as +0,
 * so the blocks of the last tile that lie wholly beyond n are +0 codes under scale 0. */
int chr_mx6_quantize(void* tiles, const void* src, size_t n, chr_dtype src_type, chr_mx6_format f, hipStream_t s);

/* dst[i] = ldexp(dec(code i), scale - 127) in f32 for i < n, overflow to +-inf as ldexp gives it; for CHR_BFLOAT16
 * one more round-to-nearest-even (the library's f32 -> bf16).  A scale of 0xFF gives 0x7FC00000 / 0x7FC0.  Exactly n
 * values are written and nothing else; `tiles` holds ceil(n / 512) tiles.
 *
 * Both casts are streaming kernels of this library, enqueued on `s`, returning at once.  n == 0 enqueues nothing.
 * Source and destination may not overlap.  `tiles` is at least 4-byte aligned and the wide buffer aligned to its
 * element (anything else: CHR_ERR_UNSUPPORTED); 8-byte aligned tiles take 8-byte accesses and a 16-byte aligned wide
 * buffer 16-byte ones.  A NULL pointer or a format outside the enum: CHR_ERR_INVALID_ARG; another dtype:
 * CHR_ERR_UNSUPPORTED; a failed launch: CHR_ERR_HIP. */
int chr_mx6_dequantize(void* dst, const void* tiles, size_t n, chr_dtype dst_type, chr_mx6_format f, hipStream_t s);

/* Frees the ops and the cached type this library holds (chr_op_free, chr_type_free): their codes go back.  A later
 * chr_mx6_sum / chr_mx6_type registers again, possibly under another code.  No call using them may be in flight. */
int chr_mx6_release(void);

/* What the library asked of the fold launchers since the last reset: out[0] calls, out[1] calls they declined
 * (nothing enqueued), out[2] kernels they enqueued.  reset != 0 zeroes the counters after reading. */
void chr_mx6_stats(long out[3], int reset);

#ifdef __cplusplus
}
#endif

#endif /* CHIARA_MX6_H */
