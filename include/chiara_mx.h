/*
 * chiara_mx.h -- MXFP8 block-scaled SUM and casts on the user-op interface (libchiara_mx.so).
 *
 * libchiara.so's kernel set and type table are closed; like the binary16 ops (chiara_ops.h), the struct ops
 * (chiara_numerics.h) and the per-tensor-scaled FP8 ops (chiara_fp8.h), the block-scaled 8-bit floats ship in a shared
 * object of their own, registered with chr_op_create.  Unlike those, the op is no element-wise functor: a combine is
 * a cooperative operation on a block of 32 values, so the launcher's kernel is hand-written (csrc/ops/mx_ops.hip).
 *
 * Element: the MX tile.  The OCP Microscaling layout -- 32 FP8 codes sharing one E8M0 power-of-two scale -- with
 * scales and codes interleaved, so that one buffer per rank travels and every split falls between whole blocks.  One
 * element is a tile of CHR_MX_TILE_VALUES = 512 values in CHR_MX_TILE_BYTES = 528 bytes (33 x 16 B):
 *   bytes 0 .. 15                         the E8M0 scales of blocks 0 .. 15: bias 127, value 2^(scale - 127); 0xFF is
 *                                         the NaN scale
 *   bytes 16 + 32 b .. 16 + 32 b + 31     the 32 codes of block b, in order
 * The type is chr_type_contiguous(132, CHR_UINT32) (chr_mx_type): every count is in tiles, and no message, slice or
 * fold begins inside a block.  The codes are OCP e4m3fn or e5m2 with the canonical NaNs of chiara_fp8.h (0x7F / 0x7E);
 * value i of a block is dec(code i) * 2^(scale - 127).
 *
 * SUM, with MPI's convention x o y = f(in = x, inout = y), per block with scales ex, ey and codes px[i], py[i].  Every
 * operation is in f32, rounded once to nearest even, f32 subnormals kept, nothing contracted:
 *   1. ex == 0xFF or ey == 0xFF: the result scale is 0xFF and all 32 codes are the canonical NaN.
 *   2. e = max(ex, ey).
 *   3. a[i] = ldexp(dec(px[i]), ex - e), b[i] = ldexp(dec(py[i]), ey - e), s[i] = b[i] + a[i].  (One of the two shifts
 *      is 0; the other ldexp is exact or, below 2^-126, rounded once.  Relative to e no magnitude exceeds 2 * 57344.)
 *   4. A non-finite s[i] -- a NaN code, an E5M2 infinity, inf - inf -- gives the canonical NaN code and takes no part
 *      in the amax.
 *   5. amax = max |s[i]| over the finite s[i].
 *   6. amax == 0: e' = e, and the codes are the encoded signed zeros (and the NaN codes of step 4).
 *   7. Otherwise E is the smallest integer with amax * 2^-E <= max (448 for E4M3, 57344 for E5M2),
 *      e' = clamp(e + E, 0, 254), and p'[i] = enc_sat(ldexp(s[i], e - e')), enc_sat being chiara_fp8.h's SATURATE
 *      conversion: one round-to-nearest-even to the format, subnormals kept, clamped to +-max.
 * The smallest fitting scale, not OCP's floor(log2 amax) - emax, which lets the largest value of a block saturate by
 * up to 12 % at every combine: here a value saturates only at the e' = 254 clamp.  The rule commutes bit for bit (f32
 * addition does, and every NaN is canonical), so both operand orders of a fold give the same bytes.  It is not
 * associative: a result depends on the schedule's expression tree.
 *
 * The op is created commutative and carries the fold launcher alone: the flat schedules' expression trees run fold by
 * fold through the library's scratch (chiara.h).  chiara_mx_tree.h (libchiara_mx_tree.so) registers the same SUM with a
 * tree launcher, one HBM pass per tree and the same bytes.  Any dtype other than a live chr_type_contiguous(132, CHR_UINT32),
 * and any call with a pointer that is not 4-byte aligned, is declined: CHR_ERR_UNSUPPORTED, nothing enqueued.
 * Pointers that are all 16-byte aligned take 16-byte accesses, any others 4-byte ones; the bytes are the same.
 */
#ifndef CHIARA_MX_H
#define CHIARA_MX_H

#include "chiara_fp8.h" /* chr_fp8_format alone: nothing of libchiara_fp8.so is linked */

#ifdef __cplusplus
extern "C" {
#endif

#define CHR_MX_TILE_VALUES 512
#define CHR_MX_TILE_BYTES 528

/* The tile type, chr_type_contiguous(132, CHR_UINT32): created on the first call (a full type registry returns the
 * registry's own error), the same code until chr_mx_release.  The op takes any live type of that content, the
 * caller's own included.  type == NULL: CHR_ERR_INVALID_ARG.  Thread-safe. */
int chr_mx_type(chr_dtype* type);

/* The SUM above on tiles of format `f`: one op per format, registered on the first call for it (chr_op_create,
 * commutative; a full registry returns the registry's own error), the same code until chr_mx_release.  Loading the
 * library registers nothing.  A format outside the enum: CHR_ERR_UNSUPPORTED; op == NULL: CHR_ERR_INVALID_ARG.
 * Thread-safe. */
int chr_mx_sum(chr_fp8_format f, chr_op* op);

/* The fold launchers those ops are registered with (chr_user_reduce_fn; running_first is not looked at), for a caller
 * that registers them itself: chiara_mx_tree.h pairs them with its tree launchers. */
int chr_mx_e4m3_sum_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dtype,
                         int running_first, hipStream_t stream, void* ctx);
int chr_mx_e5m2_sum_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dtype,
                         int running_first, hipStream_t stream, void* ctx);

/* tiles = Q(src): the n values of src (CHR_FLOAT32 or CHR_BFLOAT16, widened exactly) become ceil(n / 512) whole
 * tiles.  Per block, steps 4 - 7 of SUM with s[i] = src[i] (the sign of a zero is kept) and e = 127: a non-finite
 * source value gives the canonical NaN code and takes no part in the amax, the scale is the smallest that fits the
 * block's amax, and a block whose finite values are all zero gets scale 0.  Values beyond n count as +0, so the blocks
 * of the last tile that lie wholly beyond n are +0 codes under scale 0. */
int chr_mx_quantize(void* tiles, const void* src, size_t n, chr_dtype src_type, chr_fp8_format f, hipStream_t s);

/* dst[i] = ldexp(dec(code i), scale - 127) in f32 for i < n, overflow to +-inf as ldexp gives it; for CHR_BFLOAT16
 * one more round-to-nearest-even (the library's f32 -> bf16).  A scale of 0xFF or a NaN code gives 0x7FC00000 /
 * 0x7FC0.  Exactly n values are written and nothing else; `tiles` holds ceil(n / 512) tiles.
 *
 * Both casts are streaming kernels of this library, enqueued on `s`, returning at once.  n == 0 enqueues nothing.
 * Source and destination may not overlap.  `tiles` is at least 4-byte aligned and the wide buffer aligned to its
 * element (anything else: CHR_ERR_UNSUPPORTED); 16-byte aligned buffers take 16-byte accesses.  A NULL pointer:
 * CHR_ERR_INVALID_ARG; another dtype or a format outside the enum: CHR_ERR_UNSUPPORTED; a failed launch: CHR_ERR_HIP. */
int chr_mx_dequantize(void* dst, const void* tiles, size_t n, chr_dtype dst_type, chr_fp8_format f, hipStream_t s);

/* Frees the ops and the cached type this library holds (chr_op_free, chr_type_free): their codes go back.  A later
 * chr_mx_sum / chr_mx_type registers again, possibly under another code.  No call using them may be in flight. */
int chr_mx_release(void);

/* What the library asked of the fold launcher since the last reset: out[0] calls, out[1] calls it declined (nothing
 * enqueued), out[2] kernels it enqueued.  reset != 0 zeroes the counters after reading. */
void chr_mx_stats(long out[3], int reset);

#ifdef __cplusplus
}
#endif

#endif /* CHIARA_MX_H */
