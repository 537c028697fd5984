// struct_op.hip -- TEST INFRASTRUCTURE: the device ops of the derived-type tests (tests/test_gpu_struct_op.py,
// tests/test_gpu_struct_op_rccl.py, tests/test_struct_op_resources.py).  One element is Blk<B, K>, K consecutive B --
// what chr_type_contiguous(K, B) describes -- and every launcher comes from include/chiara_user_op.hpp.
//   HalfAddK  halfadd_op.hip's arithmetic per component: in * 0.5 + inout on float and double, rounded after the
//             multiply (built with -ffp-contract=off), 3 * in + inout (wrapping) on int32.  On count N of B x 3 it is
//             the oracle's ORC_USER_HALFADD on 3N of B.
//   RotMixK   mixes components, non-commutative: r.v[i] = in.v[(i + 1) % K] * 0.5 + inout.v[i], on the integer bases
//             3 * in.v[(i + 1) % K] + inout.v[i] computed unsigned and wrapping at the base width.  A launcher that
//             cut an element in two, or took components for elements, shows in the bits.
#include <atomic>
#include <type_traits>

#include "chiara_user_op.hpp"

template <typename B, int K>
struct Blk {
    B v[K];
};

template <typename B>
__device__ __forceinline__ B mix1(B in, B inout) {
    if constexpr (std::is_floating_point<B>::value) {
        const B h = in * (B)0.5;
        return h + inout;
    } else {
        using U = typename std::make_unsigned<B>::type;
        return (B)(U)((U)in * (U)3 + (U)inout);
    }
}

template <typename B, int K>
struct HalfAddK {
    __device__ Blk<B, K> operator()(const Blk<B, K>& in, const Blk<B, K>& inout) const {
        Blk<B, K> r;
#pragma unroll
        for (int i = 0; i < K; ++i) r.v[i] = mix1<B>(in.v[i], inout.v[i]);
        return r;
    }
};
template <typename B, int K>
struct RotMixK {
    __device__ Blk<B, K> operator()(const Blk<B, K>& in, const Blk<B, K>& inout) const {
        Blk<B, K> r;
#pragma unroll
        for (int i = 0; i < K; ++i) r.v[i] = mix1<B>(in.v[(i + 1) % K], inout.v[i]);
        return r;
    }
};

#define STRUCT_OP(F, tag, B, K)                                                                                      \
    using F##_##tag = F<B, K>;                                                                                       \
    using Blk_##F##_##tag = Blk<B, K>;                                                                               \
    CHR_DEFINE_USER_OP(chr_struct_##F##_##tag, Blk_##F##_##tag, F##_##tag)                                           \
    CHR_DEFINE_USER_TREE(chr_struct_##F##_##tag##_tree, Blk_##F##_##tag, F##_##tag)

STRUCT_OP(RotMixK, u8x3, uint8_t, 3)
STRUCT_OP(RotMixK, i16x3, int16_t, 3)
STRUCT_OP(RotMixK, f32x2, float, 2)
STRUCT_OP(RotMixK, f32x3, float, 3)
STRUCT_OP(RotMixK, f32x4, float, 4)
STRUCT_OP(RotMixK, f32x5, float, 5)
STRUCT_OP(RotMixK, f64x3, double, 3)
STRUCT_OP(RotMixK, f64x4, double, 4)
STRUCT_OP(RotMixK, f64x6, double, 6)
STRUCT_OP(RotMixK, f64x8, double, 8)
STRUCT_OP(RotMixK, f64x9, double, 9)
STRUCT_OP(HalfAddK, f32x3, float, 3)
STRUCT_OP(HalfAddK, f64x3, double, 3)
STRUCT_OP(HalfAddK, i32x3, int32_t, 3)

// The f64 x 3 RotMix launchers again, counting on the host what the library asked of them and what the tree launcher
// answered: a declined call must have enqueued nothing, and the folds then compute the same bits.
namespace {
std::atomic<long> g_fold_calls{0}, g_tree_calls{0}, g_tree_declined{0}, g_trees{0};
}  // namespace

extern "C" int chr_struct_counting_fold(void* out, const void* acc, const void* const* ins, int m, size_t n,
                                        chr_dtype dt, int running_first, hipStream_t stream, void* ctx) {
    ++g_fold_calls;
    return chr_struct_RotMixK_f64x3(out, acc, ins, m, n, dt, running_first, stream, ctx);
}
extern "C" int chr_struct_counting_tree(const chr_user_tree* trees, int ntrees, chr_dtype dt, int wg_per_cu,
                                        hipStream_t stream, void* ctx) {
    ++g_tree_calls;
    g_trees += ntrees;
    const int rc = chr_struct_RotMixK_f64x3_tree(trees, ntrees, dt, wg_per_cu, stream, ctx);
    if (rc != 0) ++g_tree_declined;
    return rc;
}
// counters: out[0] fold-launcher calls, [1] tree-launcher calls, [2] of those declined, [3] trees handed over
extern "C" void chr_struct_counters(long* out) {
    out[0] = g_fold_calls;
    out[1] = g_tree_calls;
    out[2] = g_tree_declined;
    out[3] = g_trees;
}
extern "C" void chr_struct_counters_reset() {
    g_fold_calls = 0;
    g_tree_calls = 0;
    g_tree_declined = 0;
    g_trees = 0;
}
// The build's knobs, for the tests and the benchmark rows: [0] CHR_USER_GROUP_VEC, [1] CHR_USER_TREE_WIDE_ELEMENTWISE
extern "C" void chr_struct_knobs(int* out) {
    out[0] = CHR_USER_GROUP_VEC;
    out[1] = CHR_USER_TREE_WIDE_ELEMENTWISE;
}
