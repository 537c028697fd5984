/*
 * chiara_ops.h -- first-party device ops on the user-op interface (libchiara_ops.so).
 *
 * libchiara.so's kernel set and type table are closed; what they lack ships here, built through
 * include/chiara_user_op.hpp exactly as a caller's own op would be and registered with chr_op_create_tree.  A C caller
 * without hipcc, or a Python caller, links (or loads) libchiara_ops.so beside libchiara.so and gets the op code.
 *
 * IEEE binary16 SUM / PROD / MAX / MIN.  Elements are 2 bytes and travel as CHR_UINT16 (CHR_OPS_F16_DTYPE): the
 * library moves them, the op gives them their meaning.  With MPI's convention x o y = f(in = x, inout = y):
 *   SUM   inout + in in binary16: one round-to-nearest-even, subnormal operands and results kept, any NaN result the
 *         canonical 0x7E00
 *   PROD  inout * in, the same rules
 *   MAX   inout > in ? inout : in -- the library's float rule (a tie or an unordered compare returns `in`); the chosen
 *         operand's bits pass through untouched, NaN payloads and signalling NaNs included
 *   MIN   inout < in ? inout : in, likewise
 * All four are created commutative, as the predefined ops are (the MPICH baselines take their commutative paths), and
 * carry both launchers: folds through k_fold, the flat schedules' expression trees in one pass through k_tree.  A
 * call with any other dtype, derived types included, is declined by both launchers: CHR_ERR_UNSUPPORTED, nothing
 * enqueued.
 */
#ifndef CHIARA_OPS_H
#define CHIARA_OPS_H

#include "chiara.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHR_OPS_F16_DTYPE CHR_UINT16

/* The binary16 op of `kind` (CHR_SUM, CHR_PROD, CHR_MAX or CHR_MIN; any other: CHR_ERR_UNSUPPORTED).  The first call
 * for a kind registers it (chr_op_create_tree: one of the 64 user-op codes; a full registry returns the registry's
 * own error), later calls return the same code.  Loading the library registers nothing.  Thread-safe.
 * op == NULL: CHR_ERR_INVALID_ARG. */
int chr_ops_float16(chr_op kind, chr_op* op);

/* Frees every op this library holds (chr_op_free): their codes go back to the 64.  A later chr_ops_float16 registers
 * again, possibly under another code.  No call using one of the ops may be in flight. */
int chr_ops_release(void);

/* What the library asked of the launchers since the last reset: out[0] fold-launcher calls, out[1] tree-launcher
 * calls, out[2] trees handed over (declined calls included).  reset != 0 zeroes the counters after reading. */
void chr_ops_stats(long out[3], int reset);

#ifdef __cplusplus
}
#endif

#endif /* CHIARA_OPS_H */
