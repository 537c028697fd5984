// kernel_table.hpp -- the one description of the reduction-kernel set: which (type, op) pairs are legal, which kernel
// instantiation computes each, and which translation unit compiles it.  constexpr functions of plain ints, for host
// and device code; every dispatcher (dispatch_kernel in reduce_common.hpp) and every predicate derives from these.
#pragma once

#include "chiara.h"

namespace chr {

constexpr int kNumDtypes = CHR_C_DOUBLE_COMPLEX + 1;  // 18
constexpr int kNumOps = CHR_MINLOC + 1;               // 12

// Internal op codes for the running-value-first order of MPICH_do_reduce
// (allreduce_recexch.cpp:147-186): each step is MPI_Reduce_local(running, next).  Integer SUM
// and PROD are bitwise commutative (wrapping); MAX/MIN differ on ties such as -0/+0 and on NaN
// compares, so they have their own codes.
constexpr int kMaxSw = 16, kMinSw = 17;
// SUM / PROD on the floating types are bitwise commutative except for one thing: when both operands are NaN, IEEE
// 754 leaves open whose payload survives.  The reference's loop (inout = inout + in, MPICH on x86) keeps inout's;
// gfx950 keeps the FIRST SOURCE OPERAND's (tools/nan_rule_probe.hip), and the compiler may commute a plain + or *
// (`a + b` and `b + a` both compiled to a-first there).  So the kernels pin the order in the instruction
// (add_keep / mul_keep in reduce_common.hpp: the first argument's NaN survives), and the running-value-first order
// gets its own codes, as MAX / MIN do: kSumSw / kProdSw keep the incoming operand's NaN
// (tests/test_gpu_nan_payloads.py).
constexpr int kSumSw = 20, kProdSw = 21;
// The same for MAXLOC / MINLOC on every pair type but 2INT: a tie keeps inout's words and takes only the lower
// index, so the operand order shows in the value bits of the floating pairs (-0 vs +0; a NaN compare keeps inout
// too) and in the padding bytes of DOUBLE_INT, LONG_INT and SHORT_INT (MPICH's loop never touches a.value's
// padding on a tie; tests/domain_util.py fills it).  2INT has no padding and ties are bitwise equal.
constexpr int kMaxLocSw = 18, kMinLocSw = 19;
// every op code a kernel is instantiated for: chr_op's, then the running-first codes
constexpr int kKernelOps[] = {CHR_SUM,  CHR_PROD,   CHR_MAX,    CHR_MIN, CHR_LAND, CHR_LOR,   CHR_LXOR,  CHR_BAND, CHR_BOR,
                              CHR_BXOR, CHR_MAXLOC, CHR_MINLOC, kMaxSw,  kMinSw,   kMaxLocSw, kMinLocSw, kSumSw,   kProdSw};
constexpr int kNumKernelOps = sizeof(kKernelOps) / sizeof(kKernelOps[0]);
constexpr int kMaxKernelOp = kProdSw;

constexpr size_t dtype_size(int dtype) {
    switch (dtype) {
    case CHR_FLOAT32: return 4;
    case CHR_FLOAT64: return 8;
    case CHR_INT32: return 4;
    case CHR_BFLOAT16: return 2;
    case CHR_INT8: case CHR_UINT8: return 1;
    case CHR_INT16: case CHR_UINT16: return 2;
    case CHR_UINT32: return 4;
    case CHR_INT64: case CHR_UINT64: return 8;
    // the pair and complex types: the C struct, i.e. MPI's extent (the element stride of a buffer)
    case CHR_FLOAT_INT: case CHR_2INT: case CHR_SHORT_INT: case CHR_C_FLOAT_COMPLEX: return 8;
    case CHR_DOUBLE_INT: case CHR_LONG_INT: case CHR_C_DOUBLE_COMPLEX: return 16;
    default: return 0;
    }
}

constexpr bool is_pair_dtype(int dtype) { return dtype >= CHR_FLOAT_INT && dtype <= CHR_SHORT_INT; }
constexpr bool pair_order_shows(int dtype) { return is_pair_dtype(dtype) && dtype != CHR_2INT; }  // kMaxLocSw
constexpr bool is_complex_dtype(int dtype) { return dtype == CHR_C_FLOAT_COMPLEX || dtype == CHR_C_DOUBLE_COMPLEX; }
constexpr bool is_float_dtype(int dtype) {
    return dtype == CHR_FLOAT32 || dtype == CHR_FLOAT64 || dtype == CHR_BFLOAT16;
}

constexpr bool is_arith_op(int op) { return op >= CHR_SUM && op <= CHR_MIN; }
constexpr bool is_logic_op(int op) { return op >= CHR_LAND && op <= CHR_LXOR; }
constexpr bool is_bitwise_op(int op) { return op >= CHR_BAND && op <= CHR_BXOR; }
constexpr bool is_arith_sw_op(int op) { return op == kMaxSw || op == kMinSw || op == kSumSw || op == kProdSw; }

// MPI's predefined-op/type table as MPICH 3.3.2's MPI_Reduce_local applies it (probed): SUM/PROD/
// MAX/MIN on every type, the logical ops on the integer types and on float/double (an MPICH
// extension of the standard's table), the bitwise ops on the integer types.  bf16 is this
// library's own type: arithmetic and MAX/MIN only.
constexpr bool valid_dtype_op(int dtype, int op) {
    if (!dtype_size(dtype)) return false;
    // MPICH 3.3.2's table for the pair and complex types (oracle/ref_pairs_probe table,
    // tests/golden/pairs_manifest.json): MAXLOC / MINLOC on the pairs only, SUM / PROD on complex only
    if (is_pair_dtype(dtype)) return op == CHR_MAXLOC || op == CHR_MINLOC;
    if (is_complex_dtype(dtype)) return op == CHR_SUM || op == CHR_PROD;
    if (op == CHR_MAXLOC || op == CHR_MINLOC) return false;
    if (is_arith_op(op)) return true;
    if (is_logic_op(op)) return dtype != CHR_BFLOAT16;
    return is_bitwise_op(op) && !is_float_dtype(dtype);
}

// A kernel instantiation: k_reduce_vec / k_reduce_scalar / k_reduce_tree / k_reduce_tree_scalar <dt, op, ...>.
struct KernelId {
    int dt, op;
};

// The kernel instantiation that computes (dtype, op).  Signedness only matters to MAX/MIN:
// wrapping SUM/PROD, the logical and the bitwise ops give the same bits on the unsigned type of
// the same width (int32's kernels serve uint32 there).  running_first (MPICH_do_reduce order)
// changes results only for floating types -- MAX/MIN on ties of -0/+0 and NaN compares, SUM/PROD on
// which NaN survives when two meet (kSumSw / kProdSw) -- and for MAXLOC/MINLOC ties (kMaxLocSw).
constexpr KernelId canon_op(int dtype, int op, bool running_first) {
    if (is_pair_dtype(dtype) || is_complex_dtype(dtype)) {
        if (running_first && pair_order_shows(dtype))  // ties: -0/+0, NaN compares, padding bytes
            return {dtype, op == CHR_MAXLOC ? kMaxLocSw : op == CHR_MINLOC ? kMinLocSw : op};
        if (running_first && is_complex_dtype(dtype))  // which NaN survives, per part (reduce_common.hpp apply)
            return {dtype, op == CHR_SUM ? kSumSw : op == CHR_PROD ? kProdSw : op};
        return {dtype, op};
    }
    if (is_float_dtype(dtype)) {
        if (running_first && (op == CHR_MAX || op == CHR_MIN)) return {dtype, op == CHR_MAX ? kMaxSw : kMinSw};
        if (running_first && (op == CHR_SUM || op == CHR_PROD)) return {dtype, op == CHR_SUM ? kSumSw : kProdSw};
        return {dtype, op};
    }
    if (op == CHR_MAX || op == CHR_MIN) return {dtype, op};
    switch (dtype_size(dtype)) {
    case 1: return {CHR_UINT8, op};
    case 2: return {CHR_UINT16, op};
    case 4: return {CHR_INT32, op};
    default: return {CHR_UINT64, op};
    }
}

// The bucket kernels that exist (canon_op's image, proved below).
constexpr bool kernel_exists(int kdt, int kop) {
    if (is_pair_dtype(kdt))
        return kop == CHR_MAXLOC || kop == CHR_MINLOC ||
               (pair_order_shows(kdt) && (kop == kMaxLocSw || kop == kMinLocSw));
    if (is_complex_dtype(kdt)) return kop == CHR_SUM || kop == CHR_PROD || kop == kSumSw || kop == kProdSw;
    if (is_float_dtype(kdt)) return is_arith_op(kop) || is_arith_sw_op(kop) || (is_logic_op(kop) && kdt != CHR_BFLOAT16);
    switch (kdt) {
    case CHR_INT32: case CHR_UINT8: case CHR_UINT16: case CHR_UINT64:
        return is_arith_op(kop) || is_logic_op(kop) || is_bitwise_op(kop);
    case CHR_INT8: case CHR_INT16: case CHR_UINT32: case CHR_INT64: return kop == CHR_MAX || kop == CHR_MIN;
    default: return false;
    }
}
// The tree kernels: a program's swap bits carry the operand order of every combine, so no running-first codes.
constexpr bool tree_kernel_exists(int kdt, int kop) { return kernel_exists(kdt, kop) && kop < kNumOps; }

// The type whose 16-byte vector kernel computes (kdt, kop): the bitwise ops see no element boundaries (apply_vec
// works on whole dwords), so int32's vector kernels serve every width.  The scalar kernels (unaligned calls, heads
// and tails) keep the element width.
constexpr int vec_kernel_dt(int kdt, int kop) { return is_bitwise_op(kop) ? CHR_INT32 : kdt; }

// The translation units that compile the kernels (one code object each, built in parallel): the bucket kernels of
// reduce_kernels.hip / reduce_int.hip / reduce_pair.hip, the tree kernels of reduce_tree.hip /
// reduce_tree_int_narrow.hip / reduce_tree_int_wide.hip / reduce_tree_pair.hip.
enum KernelTu { kTuNone = -1, kTuCore, kTuInt, kTuPair, kTuTree, kTuTreeIntNarrow, kTuTreeIntWide, kTuTreePair, kNumTus };
constexpr bool is_tree_tu(int tu) { return tu >= kTuTree; }

// Which translation unit owns the bucket (tree = false) or tree kernels of (kdt, kop): the arithmetic of the
// floating types and int32 in the core units, the pair and complex types in theirs, everything else (the other
// integer types, the logical and bitwise ops) in the integer units -- the trees' split by element width.
constexpr int kernel_tu(bool tree, int kdt, int kop) {
    if (!(tree ? tree_kernel_exists(kdt, kop) : kernel_exists(kdt, kop))) return kTuNone;
    if (is_pair_dtype(kdt) || is_complex_dtype(kdt)) return tree ? kTuTreePair : kTuPair;
    if ((is_float_dtype(kdt) || kdt == CHR_INT32) && (is_arith_op(kop) || is_arith_sw_op(kop)))
        return tree ? kTuTree : kTuCore;
    if (!tree) return kTuInt;
    return dtype_size(kdt) <= 2 ? kTuTreeIntNarrow : kTuTreeIntWide;
}

// ---- the table is consistent: checked over every (dtype, op, operand order) at compile time ----

constexpr bool every_valid_input_has_a_kernel() {
    for (int dt = 0; dt < kNumDtypes; ++dt)
        for (int op = 0; op < kNumOps; ++op)
            for (int rf = 0; rf < 2; ++rf) {
                if (!valid_dtype_op(dt, op)) continue;
                const KernelId k = canon_op(dt, op, rf != 0);
                if (!kernel_exists(k.dt, k.op) || (!rf && !tree_kernel_exists(k.dt, k.op))) return false;
            }
    return true;
}

constexpr bool every_kernel_has_one_owner() {
    for (int kdt = 0; kdt < kNumDtypes; ++kdt)
        for (int kop = 0; kop <= kMaxKernelOp; ++kop) {
            const int btu = kernel_tu(false, kdt, kop), ttu = kernel_tu(true, kdt, kop);
            int bucket = 0, tree = 0;
            for (int tu = 0; tu < kNumTus; ++tu) {
                bucket += !is_tree_tu(tu) && btu == tu;
                tree += is_tree_tu(tu) && ttu == tu;
            }
            if (bucket != (kernel_exists(kdt, kop) ? 1 : 0) || tree != (tree_kernel_exists(kdt, kop) ? 1 : 0))
                return false;
        }
    return true;
}

constexpr bool no_dead_kernels() {
    // reached by some valid (dtype, op): a bucket kernel in either operand order, a tree kernel in MPI_Reduce_local's
    bool bucket[kNumDtypes][kMaxKernelOp + 1] = {}, tree[kNumDtypes][kMaxKernelOp + 1] = {};
    for (int dt = 0; dt < kNumDtypes; ++dt)
        for (int op = 0; op < kNumOps; ++op)
            for (int rf = 0; rf < 2; ++rf) {
                if (!valid_dtype_op(dt, op)) continue;
                const KernelId k = canon_op(dt, op, rf != 0);
                bucket[k.dt][k.op] = true;
                if (!rf) tree[k.dt][k.op] = true;
            }
    for (int kdt = 0; kdt < kNumDtypes; ++kdt)
        for (int kop = 0; kop <= kMaxKernelOp; ++kop)
            if ((kernel_exists(kdt, kop) && !bucket[kdt][kop]) || (tree_kernel_exists(kdt, kop) && !tree[kdt][kop]))
                return false;
    return true;
}

static_assert(every_valid_input_has_a_kernel(), "canon_op maps a valid (dtype, op) to a kernel that does not exist");
static_assert(every_kernel_has_one_owner(), "a kernel is owned by no translation unit, or by more than one");
static_assert(no_dead_kernels(), "a kernel exists that no valid (dtype, op) reaches");

}  // namespace chr
