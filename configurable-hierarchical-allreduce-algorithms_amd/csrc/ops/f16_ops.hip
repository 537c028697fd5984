// f16_ops.hip -- libchiara_ops.so: IEEE binary16 SUM / PROD / MAX / MIN as first-party ops on the user-op interface
// (include/chiara_ops.h has the contract).  The arithmetic is four functors over _Float16; the kernels are the public
// header's own (include/chiara_user_op.hpp k_fold, k_tree), compiled into this code object as they would be into any
// caller's, so libchiara.so gains no kernel and no symbol.  Built with the package's HIPFLAGS: -fno-fast-math keeps the
// NaN tests and the compare-and-select of MAX / MIN as written, and gfx950's half add and multiply keep subnormals
// (the f16 denormal mode of a HIP kernel is IEEE; only f32 has a flush switch).
#include <atomic>
#include <mutex>

#include "chiara_ops.h"
#include "chiara_user_op.hpp"

namespace chr_ops {  // named: the functors are template arguments of the kernels, whose symbols the resource test reads

using f16 = _Float16;

// One canonical NaN: the result does not depend on operand order or on which payload the hardware propagates.
__device__ __forceinline__ f16 canonical(f16 r) {
    return r != r ? __builtin_bit_cast(f16, (uint16_t)0x7E00) : r;
}

struct F16Sum {
    __device__ f16 operator()(f16 in, f16 inout) const { return canonical(inout + in); }
};
struct F16Prod {
    __device__ f16 operator()(f16 in, f16 inout) const { return canonical(inout * in); }
};
// csrc/reduce_common.hpp apply()'s float rule: a tie or an unordered compare returns `in`; a select moves bits.
struct F16Max {
    __device__ f16 operator()(f16 in, f16 inout) const { return inout > in ? inout : in; }
};
struct F16Min {
    __device__ f16 operator()(f16 in, f16 inout) const { return inout < in ? inout : in; }
};

}  // namespace chr_ops

using namespace chr_ops;

// Both launchers of each op, for CHR_UINT16 alone: any other dtype is declined before anything is enqueued.
CHR_DEFINE_USER_OP_FOR(chr_ops_f16_sum_fold, f16, F16Sum, CHR_OPS_F16_DTYPE)
CHR_DEFINE_USER_OP_FOR(chr_ops_f16_prod_fold, f16, F16Prod, CHR_OPS_F16_DTYPE)
CHR_DEFINE_USER_OP_FOR(chr_ops_f16_max_fold, f16, F16Max, CHR_OPS_F16_DTYPE)
CHR_DEFINE_USER_OP_FOR(chr_ops_f16_min_fold, f16, F16Min, CHR_OPS_F16_DTYPE)
CHR_DEFINE_USER_TREE_FOR(chr_ops_f16_sum_tree, f16, F16Sum, CHR_OPS_F16_DTYPE)
CHR_DEFINE_USER_TREE_FOR(chr_ops_f16_prod_tree, f16, F16Prod, CHR_OPS_F16_DTYPE)
CHR_DEFINE_USER_TREE_FOR(chr_ops_f16_max_tree, f16, F16Max, CHR_OPS_F16_DTYPE)
CHR_DEFINE_USER_TREE_FOR(chr_ops_f16_min_tree, f16, F16Min, CHR_OPS_F16_DTYPE)

namespace {

std::atomic<long> g_fold_calls{0}, g_tree_calls{0}, g_trees{0};

// What is registered: the launchers above behind the counters of chr_ops_stats.  The op's ctx is its Kind.
struct Kind {
    chr_user_reduce_fn fold;
    chr_user_tree_fn tree;
};
const Kind kKinds[4] = {
    {chr_ops_f16_sum_fold, chr_ops_f16_sum_tree},
    {chr_ops_f16_prod_fold, chr_ops_f16_prod_tree},
    {chr_ops_f16_max_fold, chr_ops_f16_max_tree},
    {chr_ops_f16_min_fold, chr_ops_f16_min_tree},
};

int counted_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dt, int running_first,
                 hipStream_t stream, void* ctx) {
    ++g_fold_calls;
    return static_cast<const Kind*>(ctx)->fold(out, acc, ins, m, n, dt, running_first, stream, nullptr);
}

int counted_tree(const chr_user_tree* trees, int ntrees, chr_dtype dt, int wg_per_cu, hipStream_t stream, void* ctx) {
    ++g_tree_calls;
    g_trees += ntrees;
    return static_cast<const Kind*>(ctx)->tree(trees, ntrees, dt, wg_per_cu, stream, nullptr);
}

std::mutex g_mu;
int g_code[4] = {-1, -1, -1, -1};  // the live op of each kind; -1: not registered

}  // namespace

extern "C" {

int chr_ops_float16(chr_op kind, chr_op* op) {
    if (!op) return CHR_ERR_INVALID_ARG;
    const int k = (int)kind;
    if (k != CHR_SUM && k != CHR_PROD && k != CHR_MAX && k != CHR_MIN) return CHR_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_code[k] < 0) {
        chr_op code;
        if (int rc = chr_op_create_tree(counted_fold, counted_tree, const_cast<Kind*>(&kKinds[k]), 1, &code)) return rc;
        g_code[k] = (int)code;
    }
    *op = (chr_op)g_code[k];
    return CHR_SUCCESS;
}

int chr_ops_release(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = CHR_SUCCESS;
    for (int& c : g_code) {
        if (c < 0) continue;
        const int e = chr_op_free((chr_op)c);
        if (!rc) rc = e;
        c = -1;
    }
    return rc;
}

void chr_ops_stats(long out[3], int reset) {
    if (out) {
        out[0] = g_fold_calls;
        out[1] = g_tree_calls;
        out[2] = g_trees;
    }
    if (reset) {
        g_fold_calls = 0;
        g_tree_calls = 0;
        g_trees = 0;
    }
}

}  // extern "C"
