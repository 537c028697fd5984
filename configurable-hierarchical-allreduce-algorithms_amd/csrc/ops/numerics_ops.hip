// numerics_ops.hip -- libchiara_numerics.so: a double-word SUM and Welford / Chan moments as first-party ops on derived
// element types (include/chiara_numerics.h has the contract).  The arithmetic is two functor templates over
// chr_type_contiguous(2, B) and (3, B), B float or double; the reduction kernels are the public header's own
// (include/chiara_user_op.hpp k_fold, k_tree), compiled into this code object as they would be into any caller's, so
// libchiara.so and libchiara_ops.so gain no kernel and no symbol.  Pack and unpack are this file's own streaming
// kernels.  Built with the package's HIPFLAGS: -fno-fast-math keeps the NaN and infinity tests as written,
// -ffp-contract=off keeps every operation rounded once (an fma would change the error terms of two_sum), and `/` is
// hipcc's default correctly rounded division.
#include <atomic>
#include <mutex>

#include "chiara_numerics.h"
#include "chiara_user_op.hpp"

namespace chr_num {  // named: the functors are template arguments of the kernels, whose symbols the resource test reads

template <typename B> struct Bits;
template <> struct Bits<float> { using U = uint32_t; static constexpr U kQNaN = 0x7FC00000u; };
template <> struct Bits<double> { using U = uint64_t; static constexpr U kQNaN = 0x7FF8000000000000ull; };

template <typename B>
__device__ __forceinline__ B qnan() {
    return __builtin_bit_cast(B, Bits<B>::kQNaN);
}
// One canonical NaN: the result does not depend on operand order or on which payload the hardware propagates.
template <typename B>
__device__ __forceinline__ B canon(B r) {
    return r != r ? qnan<B>() : r;
}
template <typename B>
__device__ __forceinline__ bool finite(B r) {
    return r - r == (B)0;  // inf - inf and NaN - NaN are NaN
}
__device__ __forceinline__ float mag(float r) { return __builtin_fabsf(r); }
__device__ __forceinline__ double mag(double r) { return __builtin_fabs(r); }

template <typename B> struct Pair { B hi, lo; };        // chr_type_contiguous(2, B)
template <typename B> struct Rec { B n, mean, m2; };    // chr_type_contiguous(3, B)

// s = a + b and its rounding error, valid for |a| >= |b|
template <typename B>
__device__ __forceinline__ void fast_two_sum(B a, B b, B& s, B& e) {
    s = a + b;
    e = b - (s - a);
}
// the same for any order: the larger magnitude first (an unordered compare keeps the order; the result is NaN anyway)
template <typename B>
__device__ __forceinline__ void two_sum(B a, B b, B& s, B& e) {
    const bool sw = mag(a) < mag(b);
    fast_two_sum<B>(sw ? b : a, sw ? a : b, s, e);
}

template <typename B>
struct Sum2 {
    __device__ Pair<B> operator()(const Pair<B>& x, const Pair<B>& y) const {
        const B s = x.hi + y.hi;
        if (!finite(s)) return {canon(s), (B)0};
        B sh, sl, th, tl, vh, vl, zh, zl;
        two_sum<B>(x.hi, y.hi, sh, sl);
        two_sum<B>(x.lo, y.lo, th, tl);
        const B c = sl + th;
        fast_two_sum<B>(sh, c, vh, vl);
        const B w = tl + vl;
        fast_two_sum<B>(vh, w, zh, zl);
        if (!finite(zh)) return {canon(zh), (B)0};
        return {zh, zl};
    }
};

template <typename B>
struct Moments {
    __device__ Rec<B> operator()(const Rec<B>& x, const Rec<B>& y) const {
        const bool y_first = y.n > x.n || (y.n == x.n && y.mean < x.mean);
        const B an = y_first ? y.n : x.n, am = y_first ? y.mean : x.mean;  // a: the record with more samples
        const B bn = y_first ? x.n : y.n, bm = y_first ? x.mean : y.mean;
        const B n = an + bn;
        if (n != n) return {qnan<B>(), qnan<B>(), qnan<B>()};
        const bool z = bn == (B)0;
        const B w = z ? (B)0 : bn / n;
        const B t = z ? (B)0 : (an * bn) / n;
        const B d = bm - am;
        return {n, canon(am + d * w), canon((x.m2 + y.m2) + (d * d) * t)};
    }
};

// ---- pack / unpack: one 16-B vector of base values <-> K 16-B vectors of records ------------------------------------
//
// A lane's unit is VN = 16 / sizeof(B) consecutive base values and their VN records, K * 16 consecutive bytes: every
// access 16 bytes when the call's pointers are all 16-B aligned (vec), grid-stride, then the elements past the last
// whole vector (or, unaligned, every element) one per lane.  Each index is read and written by one lane.
constexpr unsigned kConvBlock = 256;
constexpr unsigned kConvMaxBlocks = 4096;

template <typename B, int K> struct Elem { B v[K]; };
template <typename B> struct BaseVec { B e[16 / sizeof(B)]; };
template <typename B, int K> struct ElemVec { Elem<B, K> e[16 / sizeof(B)]; };
template <int K> struct Words { chr_user::tree_w4 w[K]; };
template <int K> struct Outs { void* p[K]; };

// The record of one packed value: sum2 {x, +0}, moments {1, x, +0}.
template <typename B, int K>
__device__ __forceinline__ Elem<B, K> make_elem(B x) {
    Elem<B, K> r;
    if constexpr (K == 2) {
        r.v[0] = x;
        r.v[1] = (B)0;
    } else {
        r.v[0] = (B)1;
        r.v[1] = x;
        r.v[2] = (B)0;
    }
    return r;
}

template <typename B, int K>
__global__ __launch_bounds__(kConvBlock) void k_pack(void* out, const void* in, size_t n, int vec) {
    constexpr int VN = 16 / sizeof(B);
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t done = 0;
    if (vec) {
        const size_t nv = n / VN;
        const chr_user::tree_w4* inv = static_cast<const chr_user::tree_w4*>(in);
        chr_user::tree_w4* outv = static_cast<chr_user::tree_w4*>(out);
        for (size_t v = tid; v < nv; v += stride) {
            const BaseVec<B> x = __builtin_bit_cast(BaseVec<B>, inv[v]);
            ElemVec<B, K> r;
#pragma unroll
            for (int e = 0; e < VN; ++e) r.e[e] = make_elem<B, K>(x.e[e]);
            const Words<K> w = __builtin_bit_cast(Words<K>, r);
#pragma unroll
            for (int k = 0; k < K; ++k) outv[v * K + k] = w.w[k];
        }
        done = nv * VN;
    }
    for (size_t i = done + tid; i < n; i += stride)
        static_cast<Elem<B, K>*>(out)[i] = make_elem<B, K>(static_cast<const B*>(in)[i]);
}

// outs.p[k] receives component k of every record; a NULL output is skipped.
template <typename B, int K>
__global__ __launch_bounds__(kConvBlock) void k_unpack(Outs<K> outs, const void* in, size_t n, int vec) {
    constexpr int VN = 16 / sizeof(B);
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t done = 0;
    if (vec) {
        const size_t nv = n / VN;
        const chr_user::tree_w4* inv = static_cast<const chr_user::tree_w4*>(in);
        for (size_t v = tid; v < nv; v += stride) {
            Words<K> w;
#pragma unroll
            for (int k = 0; k < K; ++k) w.w[k] = inv[v * K + k];
            const ElemVec<B, K> r = __builtin_bit_cast(ElemVec<B, K>, w);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (!outs.p[k]) continue;
                BaseVec<B> x;
#pragma unroll
                for (int e = 0; e < VN; ++e) x.e[e] = r.e[e].v[k];
                static_cast<chr_user::tree_w4*>(outs.p[k])[v] = __builtin_bit_cast(chr_user::tree_w4, x);
            }
        }
        done = nv * VN;
    }
    for (size_t i = done + tid; i < n; i += stride) {
        const Elem<B, K> r = static_cast<const Elem<B, K>*>(in)[i];
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (outs.p[k]) static_cast<B*>(outs.p[k])[i] = r.v[k];
    }
}

}  // namespace chr_num

using namespace chr_num;

namespace {

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned conv_grid(size_t n, int vn, bool vec) {
    const size_t lanes = vec ? n / vn + n % vn : n;
    const size_t blocks = (lanes + kConvBlock - 1) / kConvBlock;
    return (unsigned)(blocks < kConvMaxBlocks ? (blocks ? blocks : 1) : kConvMaxBlocks);
}

template <typename B, int K>
int launch_pack(void* out, const void* in, size_t n, hipStream_t s) {
    const bool vec = aligned16(out) && aligned16(in);
    hipLaunchKernelGGL((k_pack<B, K>), dim3(conv_grid(n, 16 / sizeof(B), vec)), dim3(kConvBlock), 0, s, out, in, n,
                       vec ? 1 : 0);
    return hipGetLastError() == hipSuccess ? CHR_SUCCESS : CHR_ERR_HIP;
}

template <typename B, int K>
int launch_unpack(const Outs<K>& outs, const void* in, size_t n, hipStream_t s) {
    bool vec = aligned16(in);
    for (int k = 0; k < K; ++k) vec = vec && aligned16(outs.p[k]);  // NULL counts as aligned: it is never written
    hipLaunchKernelGGL((k_unpack<B, K>), dim3(conv_grid(n, 16 / sizeof(B), vec)), dim3(kConvBlock), 0, s, outs, in, n,
                       vec ? 1 : 0);
    return hipGetLastError() == hipSuccess ? CHR_SUCCESS : CHR_ERR_HIP;
}

bool base_ok(chr_dtype base) { return base == CHR_FLOAT32 || base == CHR_FLOAT64; }

// The content of a call's dtype, read at run time: a derived code means nothing at compile time.  A predefined type
// answers count 1; a dead or unknown code is an error.  Either way the call is declined.
bool content(chr_dtype dt, int want_count, chr_dtype* base) {
    int count = 0;
    return chr_type_get_contiguous(dt, base, &count) == CHR_SUCCESS && count == want_count && base_ok(*base);
}

std::atomic<long> g_fold_calls{0}, g_tree_calls{0}, g_trees{0};

}  // namespace

// The launchers the ops are registered with: any live chr_type_contiguous(2, f32 / f64) for sum2, (3, f32 / f64) for
// moments; every other dtype is declined before anything is enqueued.
extern "C" int chr_num_sum2_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dt,
                                 int running_first, hipStream_t stream, void*) {
    ++g_fold_calls;
    chr_dtype base;
    if (!content(dt, 2, &base)) return 1;
    return base == CHR_FLOAT32
               ? chr_user::launch_fold<Pair<float>, Sum2<float>>(out, acc, ins, m, n, running_first, stream)
               : chr_user::launch_fold<Pair<double>, Sum2<double>>(out, acc, ins, m, n, running_first, stream);
}
extern "C" int chr_num_sum2_tree(const chr_user_tree* trees, int ntrees, chr_dtype dt, int wg_per_cu,
                                 hipStream_t stream, void*) {
    ++g_tree_calls;
    g_trees += ntrees;
    chr_dtype base;
    if (!content(dt, 2, &base)) return 1;
    return base == CHR_FLOAT32 ? chr_user::launch_tree<Pair<float>, Sum2<float>>(trees, ntrees, wg_per_cu, stream)
                               : chr_user::launch_tree<Pair<double>, Sum2<double>>(trees, ntrees, wg_per_cu, stream);
}
extern "C" int chr_num_moments_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dt,
                                    int running_first, hipStream_t stream, void*) {
    ++g_fold_calls;
    chr_dtype base;
    if (!content(dt, 3, &base)) return 1;
    return base == CHR_FLOAT32
               ? chr_user::launch_fold<Rec<float>, Moments<float>>(out, acc, ins, m, n, running_first, stream)
               : chr_user::launch_fold<Rec<double>, Moments<double>>(out, acc, ins, m, n, running_first, stream);
}
extern "C" int chr_num_moments_tree(const chr_user_tree* trees, int ntrees, chr_dtype dt, int wg_per_cu,
                                    hipStream_t stream, void*) {
    ++g_tree_calls;
    g_trees += ntrees;
    chr_dtype base;
    if (!content(dt, 3, &base)) return 1;
    return base == CHR_FLOAT32
               ? chr_user::launch_tree<Rec<float>, Moments<float>>(trees, ntrees, wg_per_cu, stream)
               : chr_user::launch_tree<Rec<double>, Moments<double>>(trees, ntrees, wg_per_cu, stream);
}

namespace {

std::mutex g_mu;
int g_op[2] = {-1, -1};                      // sum2, moments; -1: not registered
int g_type[2][2] = {{-1, -1}, {-1, -1}};     // [sum2, moments][f32, f64]

int get_op(int which, chr_op* op) {
    if (!op) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_op[which] < 0) {
        chr_op code;
        const int rc = which == 0 ? chr_op_create_tree(chr_num_sum2_fold, chr_num_sum2_tree, nullptr, 1, &code)
                                  : chr_op_create_tree(chr_num_moments_fold, chr_num_moments_tree, nullptr, 1, &code);
        if (rc) return rc;
        g_op[which] = (int)code;
    }
    *op = (chr_op)g_op[which];
    return CHR_SUCCESS;
}

int get_type(int which, chr_dtype base, chr_dtype* type) {
    if (!type) return CHR_ERR_INVALID_ARG;
    if (!base_ok(base)) return CHR_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(g_mu);
    int& slot = g_type[which][base == CHR_FLOAT64];
    if (slot < 0) {
        chr_dtype code;
        if (int rc = chr_type_contiguous(which == 0 ? 2 : 3, base, &code)) return rc;
        slot = (int)code;
    }
    *type = (chr_dtype)slot;
    return CHR_SUCCESS;
}

}  // namespace

extern "C" {

int chr_num_sum2(chr_op* op) { return get_op(0, op); }
int chr_num_moments(chr_op* op) { return get_op(1, op); }
int chr_num_sum2_type(chr_dtype base, chr_dtype* type) { return get_type(0, base, type); }
int chr_num_moments_type(chr_dtype base, chr_dtype* type) { return get_type(1, base, type); }

int chr_num_sum2_pack(void* pairs, const void* values, size_t n, chr_dtype base, hipStream_t s) {
    if (!pairs || !values) return CHR_ERR_INVALID_ARG;
    if (!base_ok(base)) return CHR_ERR_UNSUPPORTED;
    if (n == 0) return CHR_SUCCESS;
    return base == CHR_FLOAT32 ? launch_pack<float, 2>(pairs, values, n, s) : launch_pack<double, 2>(pairs, values, n, s);
}

int chr_num_sum2_unpack(void* values, const void* pairs, size_t n, chr_dtype base, hipStream_t s) {
    if (!pairs || !values) return CHR_ERR_INVALID_ARG;
    if (!base_ok(base)) return CHR_ERR_UNSUPPORTED;
    if (n == 0) return CHR_SUCCESS;
    const Outs<2> outs{{values, nullptr}};
    return base == CHR_FLOAT32 ? launch_unpack<float, 2>(outs, pairs, n, s) : launch_unpack<double, 2>(outs, pairs, n, s);
}

int chr_num_moments_pack(void* recs, const void* samples, size_t n, chr_dtype base, hipStream_t s) {
    if (!recs || !samples) return CHR_ERR_INVALID_ARG;
    if (!base_ok(base)) return CHR_ERR_UNSUPPORTED;
    if (n == 0) return CHR_SUCCESS;
    return base == CHR_FLOAT32 ? launch_pack<float, 3>(recs, samples, n, s) : launch_pack<double, 3>(recs, samples, n, s);
}

int chr_num_moments_unpack(void* count, void* mean, void* m2, const void* recs, size_t n, chr_dtype base,
                           hipStream_t s) {
    if (!recs || (!count && !mean && !m2)) return CHR_ERR_INVALID_ARG;
    if (!base_ok(base)) return CHR_ERR_UNSUPPORTED;
    if (n == 0) return CHR_SUCCESS;
    const Outs<3> outs{{count, mean, m2}};
    return base == CHR_FLOAT32 ? launch_unpack<float, 3>(outs, recs, n, s) : launch_unpack<double, 3>(outs, recs, n, s);
}

int chr_num_release(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = CHR_SUCCESS;
    for (int& c : g_op) {
        if (c < 0) continue;
        const int e = chr_op_free((chr_op)c);
        if (!rc) rc = e;
        c = -1;
    }
    for (auto& row : g_type)
        for (int& c : row) {
            if (c < 0) continue;
            const int e = chr_type_free((chr_dtype)c);
            if (!rc) rc = e;
            c = -1;
        }
    return rc;
}

void chr_num_stats(long out[3], int reset) {
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
