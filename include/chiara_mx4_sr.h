/*
 * chiara_mx4_sr.h -- the MXFP4 block-scaled SUM and quantize with stochastic rounding (libchiara_mx4_sr.so).
 *
 * chiara_mx4.h's SUM ends every combine in one round-to-nearest-even.  E2M1 keeps one mantissa bit, so in a gradient
 * allreduce an addend below half a step of the running block is dropped at every level of the tree, in the same
 * direction on every rank and every step.  This library is the same tile (chr_mx4_type, no second type), the same
 * rule up to the last step, and a last step that rounds up with a probability equal to the value's place between its
 * two neighbours.  Dequantize is chr_mx4_dequantize.  The kernels are hand-written (csrc/ops/mx4_sr_ops.hip).
 *
 * SUM.  Steps 1 - 6 of chiara_mx4.h stand as written: NaN blocks, e = max(ex, ey), the aligned f32 sums s[i], amax,
 * the smallest fitting scale e', clamped to 0 .. 254.  Step 7 becomes
 *   7. p'[i] = enc_sr(t[i], u[i]),  t[i] = clamp(ldexp(s[i], e - e'), -6, 6) in f32, exactly as in chiara_mx4.h.
 * enc_sr, on the grid G = {0, 0.5, 1, 1.5, 2, 3, 4, 6}: lo is the largest member of G that is <= |t|.  If |t| == lo
 * the magnitude is lo (so |t| = 6 needs no upper neighbour, and a representable value is never moved).  Otherwise hi
 * is the next member above lo, f = (|t| - lo) / (hi - lo) is a real in (0, 1), and the magnitude is hi iff
 * floor(f * 2^16) + u >= 2^16, else lo: u is a 16-bit integer, so P(up) = floor(f * 2^16) / 2^16.  The sign bit of t
 * is kept, also on a result of magnitude 0.  Nothing overflows: |t| <= 6.
 *
 * The random halves u[i].  mix32 is lowbias32, all mod 2^32:
 *   x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 * Per block:  kb = mix32(mix32(seed ^ T) ^ (blk | e' << 8)), blk the block's index in its tile (0 .. 15), e' the
 * block's new scale, T = 0 for SUM and the low 32 bits of the tile's index in the buffer for quantize.
 * Per pair j = 0 .. 15 (values 2j and 2j + 1, the two nibbles of code byte j), with C_j = (j + 1) * 0x9E3779B9 mod 2^32:
 *   w = mix32(bits(t[2j]) ^ rotl32(bits(t[2j + 1]), 16) ^ (kb + C_j)),  u[2j] = w & 0xFFFF,  u[2j + 1] = w >> 16,
 * where bits is the f32 pattern of the clamped t, sign included.  One hash serves a pair: a 32-bit integer multiply is
 * not a full-rate instruction, and 16 random bits resolve P(up) to 2^-16 of a step, far below what one mantissa bit
 * can show.
 *
 * Why the bits come from there.  A fold launcher sees (out, acc, ins, m, n), never where its slice lies in the
 * caller's buffer; the executor slices at tile granularity, differently per schedule and pipeline depth, and the
 * EXACT schedules let two ranks compute the same partial sum and rely on identical bytes.  So the random bits are a
 * pure function of the seed, the value's place inside its own tile and the operands' bits: the SR SUM is a
 * deterministic, bit-commutative function of its two operand tiles, and both operand orders, `out` aliasing, fan-in
 * continuation, slicing and plan evaluation work as they do for chr_mx4_sum.  It is not associative either.
 *
 * Known property.  In a SUM, equal (t pair, blk, e', j) in different tiles round alike: the rounding is unbiased over
 * seeds, not over tiles.  Callers change the seed every step (chr_mx4_sr_set_seed), and every rank sets the same
 * value before the same collective.
 *
 * Not here: an SR tree launcher (flat-schedule trees run fold by fold), SR for MXFP8, MXFP6 and MXINT8, and a
 * per-call seed through the collectives' signatures.
 */
#ifndef CHIARA_MX4_SR_H
#define CHIARA_MX4_SR_H

#include <stdint.h>

#include "chiara_mx4.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The SR SUM above on chr_mx4_type's tiles: one op, registered on the first call (chr_op_create, commutative, the fold
 * launcher alone; a full registry returns the registry's own error), the same code until chr_mx4_sr_release.  Loading
 * the library registers nothing.  op == NULL: CHR_ERR_INVALID_ARG.  Thread-safe. */
int chr_mx4_sr_sum(chr_op* op);

/* The seed of every later SR SUM of this process (default 0): atomic, read by the fold launcher once per call at
 * enqueue time, so every launch of a call -- a fan-in beyond 16 continues from `out` -- rounds under one seed. */
void chr_mx4_sr_set_seed(uint32_t seed);

/* The fold launcher that op is registered with (chr_user_reduce_fn; running_first is not looked at), for a caller
 * that registers it itself.  It declines what chr_mx4_sum_fold declines: any dtype but a live
 * chr_type_contiguous(68, CHR_UINT32), any pointer that is not 4-byte aligned -- nonzero, nothing enqueued. */
int chr_mx4_sr_sum_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dtype,
                        int running_first, hipStream_t stream, void* ctx);

/* tiles = Q_sr(src): chr_mx4_quantize with step 7 above on s[i] = src[i], e = 127 and T = the tile's index in
 * `tiles`, so that identical tiles of one buffer round apart.  Scale 0 for an all-zero block, the canonical NaN block
 * for a block with a non-finite value, +0 beyond n: as in chr_mx4_quantize, and so are the alignment rules and the
 * error codes. */
int chr_mx4_sr_quantize(void* tiles, const void* src, size_t n, chr_dtype src_type, uint32_t seed, hipStream_t s);

/* Frees the op this library registered (chr_op_free); the tile type is libchiara_mx4.so's.  No call using the op may
 * be in flight. */
int chr_mx4_sr_release(void);

/* What the library asked of the fold launcher since the last reset: out[0] calls, out[1] calls it declined (nothing
 * enqueued), out[2] kernels it enqueued.  reset != 0 zeroes the counters after reading. */
void chr_mx4_sr_stats(long out[3], int reset);

#ifdef __cplusplus
}
#endif

#endif /* CHIARA_MX4_SR_H */
