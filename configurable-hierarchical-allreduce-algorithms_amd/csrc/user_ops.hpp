// user_ops.hpp -- user-defined reduction ops (chr_op_create) and the dispatchers every reduction of the library goes
// through: a user op runs the caller's own device launcher, a predefined op the library's kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "chr_internal.hpp"

namespace chr {

// The library's one mapping of a HIP status to a chr_result; CHR_DEBUG prints what was lost in it.
__attribute__((visibility("hidden"))) inline int hip_code(hipError_t e) {
    if (e == hipSuccess) return CHR_SUCCESS;
    if (e == hipErrorOutOfMemory) return CHR_ERR_OUT_OF_MEMORY;
    if (std::getenv("CHR_DEBUG")) std::fprintf(stderr, "[chiara] HIP error: %s\n", hipGetErrorString(e));
    return CHR_ERR_HIP;
}

// User ops take the chr_op codes [kUserOpBase, kUserOpBase + kMaxUserOps): above every predefined op and every
// internal kernel code (kMaxSw ... kProdSw).
constexpr int kUserOpBase = 64;
constexpr int kMaxUserOps = 64;

// Derived element types (chr_type_contiguous) take the chr_dtype codes [kUserTypeBase, kUserTypeBase + kMaxUserTypes),
// above every predefined type.  One element is `count` consecutive base elements, kMaxElemBytes at most.
constexpr int kUserTypeBase = 64;
constexpr int kMaxUserTypes = 64;
constexpr size_t kMaxElemBytes = 65536;

bool is_user_op(int op);
bool is_derived_type(int dtype);
// MPI_Type_size: dtype_size for a predefined code, the registry for a live derived one, 0 for anything else.  Every
// host-side byte count goes through this; dtype_size stays the kernels' constexpr table of the predefined types.
size_t elem_size(int dtype);
// MPI_Op_commutative: every predefined op is commutative; a user op as chr_op_create recorded it.
bool op_commutative(int op);
// CHR_SUCCESS for a live user op on a type with a size (derived types included) and for a (type, op) pair MPICH's
// table accepts (valid_dtype_op); CHR_ERR_UNSUPPORTED for a predefined op on a live derived type (MPI's predefined
// ops take no derived type: MPICH answers MPI_ERR_OP); CHR_ERR_INVALID_ARG otherwise.  valid_any: the first of these.
int check_any(int dtype, int op);
bool valid_any(int dtype, int op);

// The reductions: chr_result codes.  reduce_any is MPI_Reduce_local chained over ins (launch_reduce's contract);
// reduce_tree_any evaluates one post-order program (launch_reduce_tree's); reduce_tree_multi_any a batch of them.  A
// user op's trees go to its tree launcher in one call per batch (chr_op_create_tree), fold by fold through its fold
// launcher when it has none or the launcher declines.
int reduce_any(void* out, const void* acc, const void* const* ins, int m, size_t n, int dtype, int op, hipStream_t s,
               bool running_first = false);
int reduce_tree_any(void* out, const void* const* leaves, int nl, const uint8_t* comb, const uint8_t* swaps, size_t n,
                    int dtype, int op, hipStream_t s);
int reduce_tree_multi_any(const TreeJob* jobs, int njobs, int dtype, int op, hipStream_t s);

}  // namespace chr
