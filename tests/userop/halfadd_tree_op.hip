// halfadd_tree_op.hip -- TEST INFRASTRUCTURE: the device side of the one-pass user-op tree tests
// (tests/test_gpu_user_tree.py, tests/test_gpu_user_tree_rccl.py, tests/test_user_tree_resources.py).
// The op of halfadd_op.hip restated -- in o inout = in * 0.5 + inout on float and double, rounded after the multiply
// (built with -ffp-contract=off), 3 * in + inout (wrapping) on int32; non-commutative, the oracle's ORC_USER_HALFADD
// -- with both launchers of chr_op_create_tree built from the same functors through include/chiara_user_op.hpp, and
// host-side counters of what the library asked of them.
#include <atomic>

#include "chiara_user_op.hpp"

struct HalfAdd {
    __device__ float operator()(float in, float inout) const {
        const float h = in * 0.5f;
        return h + inout;
    }
};
struct HalfAddD {
    __device__ double operator()(double in, double inout) const {
        const double h = in * 0.5;
        return h + inout;
    }
};
struct Mix3 {  // the same MPI function on MPI_INT: 3 * in + inout, wrapping
    __device__ int32_t operator()(int32_t in, int32_t inout) const {
        return (int32_t)((uint32_t)in * 3u + (uint32_t)inout);
    }
};

namespace {
std::atomic<long> g_fold_calls{0}, g_tree_calls{0}, g_trees{0};
std::atomic<int> g_last_wg{-1};
}  // namespace

// One op over three types, as an MPI user function switches on its datatype argument.
extern "C" int chr_test_halfadd(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dt,
                                int running_first, hipStream_t stream, void*) {
    ++g_fold_calls;
    switch (dt) {
    case CHR_FLOAT32: return chr_user::launch_fold<float, HalfAdd>(out, acc, ins, m, n, running_first, stream);
    case CHR_FLOAT64: return chr_user::launch_fold<double, HalfAddD>(out, acc, ins, m, n, running_first, stream);
    case CHR_INT32: return chr_user::launch_fold<int32_t, Mix3>(out, acc, ins, m, n, running_first, stream);
    default: return 1;
    }
}

// The tree launcher for the same three types; any other type is declined (the library then asks the fold launcher,
// which refuses it).
extern "C" int chr_test_halfadd_tree(const chr_user_tree* trees, int ntrees, chr_dtype dt, int wg_per_cu,
                                     hipStream_t stream, void*) {
    ++g_tree_calls;
    g_trees += ntrees;
    g_last_wg = wg_per_cu;
    switch (dt) {
    case CHR_FLOAT32: return chr_user::launch_tree<float, HalfAdd>(trees, ntrees, wg_per_cu, stream);
    case CHR_FLOAT64: return chr_user::launch_tree<double, HalfAddD>(trees, ntrees, wg_per_cu, stream);
    case CHR_INT32: return chr_user::launch_tree<int32_t, Mix3>(trees, ntrees, wg_per_cu, stream);
    default: return 1;
    }
}

// A tree launcher that declines every call and enqueues nothing: the library must fall back to the folds.
extern "C" int chr_test_decline_tree(const chr_user_tree*, int ntrees, chr_dtype, int wg_per_cu, hipStream_t, void*) {
    ++g_tree_calls;
    g_trees += ntrees;
    g_last_wg = wg_per_cu;
    return 1;
}

// counters: out[0] fold-launcher calls, [1] tree-launcher calls, [2] trees handed over, [3] the last wg_per_cu
extern "C" void chr_test_counters(long* out) {
    out[0] = g_fold_calls;
    out[1] = g_tree_calls;
    out[2] = g_trees;
    out[3] = g_last_wg;
}
extern "C" void chr_test_counters_reset() {
    g_fold_calls = 0;
    g_tree_calls = 0;
    g_trees = 0;
    g_last_wg = -1;
}
