/*
 * chiara_mxint8.h -- MXINT8 block-scaled SUM and casts on the user-op interface (libchiara_mxint8.so).
 *
 * The fourth concrete format of the OCP Microscaling v1.0 specification beside chiara_mx.h's MXFP8, chiara_mx4.h's
 * MXFP4 and chiara_mx6.h's MXFP6: the same E8M0 block scales and the same rule, over two's-complement int8 codes on a
 * uniform grid, seven magnitude bits and no exponent field -- what a quantized-gradient collective carries at 8 bits.
 * Like every first-party op it ships in a shared object of its own, registered with chr_op_create; its kernels are
 * hand-written (csrc/ops/mxint8_ops.hip, csrc/ops/mxint8_tile.hpp).
 *
 * Element: the MX tile of chiara_mx.h, CHR_MXI8_TILE_VALUES = 512 values in CHR_MXI8_TILE_BYTES = 528 bytes:
 *   bytes 0 .. 15                         the E8M0 scales of blocks 0 .. 15: bias 127, value 2^(scale - 127); 0xFF is
 *                                         the NaN scale
 *   bytes 16 + 32 b .. 16 + 32 b + 31     the 32 codes of block b, one two's-complement byte each
 * Value i of a block is dec(code i) * 2^(scale - 127) with dec(c) = (int8)c / 64.  All 256 codes decode; 0x80 is -2.0.
 * The encoder is symmetric, as OCP recommends: it never emits 0x80, and max = 127/64 = 1.984375 = 0.9921875 * 2^1.
 * There is no -0: a value that rounds to zero is 0x00.  A NaN exists only as a block whose scale is 0xFF, and the
 * canonical NaN block is scale 0xFF with thirty-two 0x00 codes.  The type is chr_type_contiguous(132, CHR_UINT32)
 * (chr_mxi8_type): every count is in tiles, and no message, slice or fold begins inside a block.
 *
 * SUM, with MPI's convention x o y = f(in = x, inout = y), per block with scales ex, ey and codes px[i], py[i].  Every
 * operation is in f32, rounded once to nearest even, f32 subnormals kept, nothing contracted -- chiara_mx6.h's steps,
 * changed only where the format forces it:
 *   1. ex == 0xFF or ey == 0xFF: the result is the canonical NaN block.
 *   2. e = max(ex, ey).
 *   3. s[i] = ldexp(dec(py[i]), ey - e) + ldexp(dec(px[i]), ex - e).
 *   4. amax = max |s[i]|.  amax == 0: e' = e, and all codes are 0x00.
 *   5. Otherwise E is the smallest integer with amax * 2^-E <= 127/64: with amax = f * 2^x, f in [0.5, 1), that is
 *      x - 1 + (f > 0.9921875).
 *   6. e' = clamp(e + E, 0, 254).
 *   7. p'[i] = enc_sat(ldexp(s[i], e - e')): round to the nearest multiple of 1/64, ties to the even code, clamped to
 *      +-127/64.
 * The rule commutes bit for bit (f32 addition does, and the NaN block is canonical), so both operand orders of a fold
 * give the same bytes.  It is not associative: a result depends on the schedule's expression tree.
 *
 * The op is created commutative and carries the fold launcher alone: the flat schedules' expression trees run fold by
 * fold through the library's scratch (chiara.h).  Any dtype other than a live chr_type_contiguous(132, CHR_UINT32) --
 * chr_mx_type's code is one -- and any call with a pointer that is not 4-byte aligned is declined:
 * CHR_ERR_UNSUPPORTED, nothing enqueued.  Pointers that are all 16-byte aligned take 16-byte accesses, any others
 * 4-byte ones; the bytes are the same.
 */
#ifndef CHIARA_MXINT8_H
#define CHIARA_MXINT8_H

#include "chiara.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHR_MXI8_TILE_VALUES 512
#define CHR_MXI8_TILE_BYTES 528

/* The tile type, chr_type_contiguous(132, CHR_UINT32): created on the first call (a full type registry returns the
 * registry's own error), the same code until chr_mxi8_release.  The op takes any live type of that content, the
 * caller's own included.  type == NULL: CHR_ERR_INVALID_ARG.  Thread-safe. */
int chr_mxi8_type(chr_dtype* type);

/* The SUM above: registered on the first call (chr_op_create, commutative; a full registry returns the registry's own
 * error), the same code until chr_mxi8_release.  Loading the library registers nothing.  op == NULL:
 * CHR_ERR_INVALID_ARG.  Thread-safe. */
int chr_mxi8_sum(chr_op* op);

/* The fold launcher that op is registered with (chr_user_reduce_fn; running_first is not looked at), for a caller that
 * registers it itself. */
int chr_mxi8_sum_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dtype,
                      int running_first, hipStream_t stream, void* ctx);

/* tiles = Q(src): the n values of src (CHR_FLOAT32 or CHR_BFLOAT16, widened exactly) become ceil(n / 512) whole
 * tiles.  Per block, steps 4 - 7 of SUM with s[i] = src[i] and e = 127: the scale is the smallest that fits the
 * block's amax, and an all-zero block gets scale 0.  A block with any non-finite source value becomes the canonical
 * NaN block.  Values beyond n count as +0, so the blocks of the last tile that lie wholly beyond n are 0x00 codes under
 * scale 0. */
int chr_mxi8_quantize(void* tiles, const void* src, size_t n, chr_dtype src_type, hipStream_t s);

/* dst[i] = ldexp(dec(code i), scale - 127) in f32 for i < n, overflow to +-inf as ldexp gives it; for CHR_BFLOAT16
 * one more round-to-nearest-even (the library's f32 -> bf16).  A scale of 0xFF gives 0x7FC00000 / 0x7FC0.  Exactly n
 * values are written and nothing else; `tiles` holds ceil(n / 512) tiles.
 *
 * Both casts are streaming kernels of this library, enqueued on `s`, returning at once.  n == 0 enqueues nothing.
 * Source and destination may not overlap.  `tiles` is at least 4-byte aligned and the wide buffer aligned to its
 * element (anything else: CHR_ERR_UNSUPPORTED); 16-byte aligned buffers take 16-byte accesses.  A NULL pointer:
 * CHR_ERR_INVALID_ARG; another dtype: CHR_ERR_UNSUPPORTED; a failed launch: CHR_ERR_HIP. */
int chr_mxi8_dequantize(void* dst, const void* tiles, size_t n, chr_dtype dst_type, hipStream_t s);

/* Frees the op and the cached type this library holds (chr_op_free, chr_type_free): their codes go back.  A later
 * chr_mxi8_sum / chr_mxi8_type registers again, possibly under another code.  No call using them may be in flight. */
int chr_mxi8_release(void);

/* What the library asked of the fold launcher since the last reset: out[0] calls, out[1] calls it declined (nothing
 * enqueued), out[2] kernels it enqueued.  reset != 0 zeroes the counters after reading. */
void chr_mxi8_stats(long out[3], int reset);

#ifdef __cplusplus
}
#endif

#endif /* CHIARA_MXINT8_H */
