/*
 * chiara_mx6_tree.h -- the MXFP6 block-scaled SUMs with one-pass expression trees (libchiara_mx6_tree.so).
 *
 * chr_mx6_sum (chiara_mx6.h, libchiara_mx6.so) carries the fold launcher alone, so under the flat schedules each
 * chunk's expression tree runs fold by fold through the library's scratch: C4's 8-leaf tree is three launcher calls
 * and 13 units of HBM traffic.  The ops of this header are the same SUMs -- the same tile, the same rule, the same
 * bytes in every call -- registered with chr_op_create_tree: `fn` is libchiara_mx6.so's fold launcher of the format,
 * `tree_fn` a launcher whose kernel (csrc/ops/mx6_tree_ops.hip, chr_mx6::k_mx6_tree) evaluates a whole tree in one HBM
 * pass and one launch, 9 units for the 8-leaf tree, every inner node requantised to the format in registers exactly as
 * a fold would have stored it.  A lane owns a whole block, so only the top of the program's stack stays in registers;
 * the values below it wait in LDS private to the lane.  The kernels live in a shared object of their own, which links
 * libchiara_mx6.so and libchiara.so; libchiara_mx6.so's kernel set stays as it is.
 *
 * A tree launcher takes a call when its dtype is a live chr_type_contiguous(100, CHR_UINT32), every tree has 2..8
 * leaves, n > 0 tiles and a program within stack depth 4, and `out` and every leaf are non-null and 4-byte aligned.
 * Any other call it declines whole, nothing enqueued, and the library evaluates those trees fold by fold through
 * `fn`, whose verdict alone can become CHR_ERR_UNSUPPORTED (chiara.h).  It also declines, for speed alone, a call made
 * of nothing but trees that one fold launch evaluates with the same traffic -- each leaf folded straight into one
 * running value, in one operand order; every 2-leaf tree is one -- where the fold kernel runs the same combines
 * without the LDS round trips (csrc/ops/mx6_tree_ops.hip has the rows).  Pointers of a tree that are all 8-byte
 * aligned take 8-byte accesses, any others 4-byte ones; the bytes are the same.  `out` may alias any leaf at the same
 * element offset.  A program's swap bits are accepted and ignored: the rule commutes bit for bit (chiara_mx6.h), so
 * both operand orders of a combine give the same bytes.  wg_per_cu > 0 is honoured the library's way, dynamic LDS of
 * (LDS per CU) / wg_per_cu bytes per workgroup, of which the kernel uses the first 6 144 for its stack; 0 takes the
 * launcher's own 16 per CU, and no launch asks for less than those 6 144 bytes, 26 workgroups per CU.
 */
#ifndef CHIARA_MX6_TREE_H
#define CHIARA_MX6_TREE_H

#include "chiara_mx6.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The SUM of chiara_mx6.h on tiles of format `f` with the tree launcher: one op per format, registered on the first
 * call for it (chr_op_create_tree, commutative; a full registry returns the registry's own error), the same code until
 * chr_mx6_tree_release.  A different op code from chr_mx6_sum's.  Loading the library registers nothing.  A format
 * outside the enum or op == NULL: CHR_ERR_INVALID_ARG.  Thread-safe. */
int chr_mx6_sum_tree(chr_mx6_format f, chr_op* op);

/* The tree launchers those ops are registered with (chr_user_tree_fn), for a caller that registers or times them
 * itself. */
int chr_mx6_e2m3_sum_tree_launch(const chr_user_tree* trees, int ntrees, chr_dtype dtype, int wg_per_cu,
                                 hipStream_t stream, void* ctx);
int chr_mx6_e3m2_sum_tree_launch(const chr_user_tree* trees, int ntrees, chr_dtype dtype, int wg_per_cu,
                                 hipStream_t stream, void* ctx);

/* Frees the ops this library holds (chr_op_free): their codes go back.  The tile type is libchiara_mx6.so's
 * (chr_mx6_type, chr_mx6_release).  No call using the ops may be in flight. */
int chr_mx6_tree_release(void);

/* What the library asked of the tree launchers since the last reset, both formats together: out[0] calls, out[1] calls
 * declined (nothing enqueued), out[2] trees handed over by the calls taken, out[3] kernels enqueued.  reset != 0
 * zeroes the counters after reading.  The folds of these ops -- 1-leaf trees, chr_reduce_multi, declined calls -- count
 * in chr_mx6_stats. */
void chr_mx6_tree_stats(long out[4], int reset);

#ifdef __cplusplus
}
#endif

#endif /* CHIARA_MX6_TREE_H */
