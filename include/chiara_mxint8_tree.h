/*
 * chiara_mxint8_tree.h -- the MXINT8 block-scaled SUM with one-pass expression trees (libchiara_mxint8_tree.so).
 *
 * chr_mxi8_sum (chiara_mxint8.h, libchiara_mxint8.so) carries the fold launcher alone, so under the flat schedules
 * each chunk's expression tree runs fold by fold through the library's scratch: C4's 8-leaf tree is three launcher
 * calls and 13 units of HBM traffic.  The op of this header is the same SUM -- the same tile, the same rule, the same
 * bytes in every call -- registered with chr_op_create_tree: `fn` is libchiara_mxint8.so's fold launcher, `tree_fn` a
 * launcher whose kernel (csrc/ops/mxint8_tree_ops.hip, chr_mxi8::k_mxi8_tree) evaluates a whole tree in one HBM pass
 * and one launch, 9 units for the 8-leaf tree, every inner node requantised to the format in registers exactly as a
 * fold would have stored it: on packed 16-bit integers where every block of the wave has close scales at that node, in
 * f32 otherwise, chosen per combine.  The kernels live in a shared object of their own, which links
 * libchiara_mxint8.so and libchiara.so; libchiara_mxint8.so's kernel set stays as it is.
 *
 * The tree launcher takes a call when its dtype is a live chr_type_contiguous(132, CHR_UINT32), every tree has 2..8
 * leaves, n > 0 tiles and a program within stack depth 4, and `out` and every leaf are non-null and 4-byte aligned.
 * Any other call it declines whole, nothing enqueued, and the library evaluates those trees fold by fold through
 * `fn`, whose verdict alone can become CHR_ERR_UNSUPPORTED (chiara.h).  It also declines, for speed alone, a call made
 * of nothing but trees that one fold launch evaluates with the same traffic -- each leaf folded straight into one
 * running value, in one operand order; every 2-leaf tree is one -- where the fold kernel measured faster
 * (csrc/ops/mxint8_tree_ops.hip has the rows).  Pointers of a tree that are all 16-byte aligned take 16-byte accesses,
 * any others 4-byte ones; the bytes are the same.  `out` may alias any leaf at the same element offset.  A program's
 * swap bits are accepted and ignored: the rule commutes bit for bit (chiara_mxint8.h), so both operand orders of a
 * combine give the same bytes.  wg_per_cu > 0 is honoured the library's way, dynamic LDS of (LDS per CU) / wg_per_cu
 * bytes per workgroup, none of it touched; 0 takes the launcher's own 16 per CU.
 */
#ifndef CHIARA_MXINT8_TREE_H
#define CHIARA_MXINT8_TREE_H

#include "chiara_mxint8.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The SUM of chiara_mxint8.h with the tree launcher: one op, registered on the first call (chr_op_create_tree,
 * commutative; a full registry returns the registry's own error), the same code until chr_mxi8_tree_release.  A
 * different op code from chr_mxi8_sum's.  Loading the library registers nothing.  op == NULL: CHR_ERR_INVALID_ARG.
 * Thread-safe. */
int chr_mxi8_sum_tree(chr_op* op);

/* The tree launcher that op is registered with (chr_user_tree_fn), for a caller that registers or times it itself. */
int chr_mxi8_sum_tree_launch(const chr_user_tree* trees, int ntrees, chr_dtype dtype, int wg_per_cu, hipStream_t stream,
                             void* ctx);

/* Frees the op this library holds (chr_op_free): its code goes back.  The tile type is libchiara_mxint8.so's
 * (chr_mxi8_type, chr_mxi8_release).  No call using the op may be in flight. */
int chr_mxi8_tree_release(void);

/* What the library asked of the tree launcher since the last reset: out[0] calls, out[1] calls declined (nothing
 * enqueued), out[2] trees handed over by the calls taken, out[3] kernels enqueued.  reset != 0 zeroes the counters
 * after reading.  The folds of this op -- 1-leaf trees, chr_reduce_multi, declined calls -- count in chr_mxi8_stats. */
void chr_mxi8_tree_stats(long out[4], int reset);

#ifdef __cplusplus
}
#endif

#endif /* CHIARA_MXINT8_TREE_H */
