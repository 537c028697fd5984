// fp8_ops.hip -- libchiara_fp8.so: OCP FP8 (E4M3 / E5M2) SUM / PROD / MAX / MIN as first-party ops on the user-op
// interface, and the scaled casts into and out of the formats (include/chiara_fp8.h has the contract).  The arithmetic
// is four functor templates over a 1-byte element; the reduction kernels are the public header's own
// (include/chiara_user_op.hpp k_fold, k_tree: 16 elements per 16-B vector per lane), compiled into this code object as
// they would be into any caller's, so the other three libraries gain no kernel and no symbol.  The casts are this
// file's own streaming kernels.  Built with the package's HIPFLAGS: -fno-fast-math keeps the NaN tests and the
// compare-and-select of MAX / MIN as written, -ffp-contract=off keeps the one f32 multiply of a cast a multiply.
//
// Decode and encode are gfx950's conversions (v_cvt_f32_fp8 / v_cvt_f32_bf8, v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32).
// The encode instruction only ever sees finite values of magnitude <= max: NaN and overflow are decided in code
// before it (enc below), so what the instruction does with them -- which depends on the wave's FP16_OVFL mode bit --
// never shows.  In range it rounds to nearest even and keeps subnormals and the sign of zero: all 65 536 operand pairs
// of all 12 ops are bit-exact against the float64 reference on an MI355X, on the vector and the element-wise path
// (tests/test_gpu_fp8_ops.py), and so are the casts over every bf16 pattern and every f32 rounding boundary.
//
// Measured (tools/userop_bench.py --fp8 --fp8-perbyte, HBM-cold, 2 alternating rounds in one process; the binary16 SUM
// of libchiara_ops.so on the same bytes is the HBM-bound reference; "per byte" is this file built with
// -DCHR_FP8_PACKED=0, make fp8_ab).  First the per-byte functors alone (profiles/r11/fp8/userop_bench.json):
//                              f16 SUM        E4M3 SUM IEEE   E4M3 SUM SAT    E5M2 SUM IEEE
//   fold m = 1, 64 MiB, GB/s   5360 / 5459    4705 / 4822     4679 / 4973     4258 / 4546
//   fold m = 3, 64 MiB, GB/s   5485 / 5474    4112 / 4070     4551 / 4507     3475 / 3485
//   8-leaf tree, 16 MiB leaves 0.710 / 0.711  0.299 / 0.299   0.328 / 0.328   0.265 / 0.265   (of 8 TB/s, 9 units)
//   8-leaf tree, 64 MiB leaves 0.765 / 0.770  0.351 / 0.352   0.397 / 0.398   0.310 / 0.311
// Both rounds of every FP8 figure lie below both rounds of binary16 in every row: a per-byte functor (extract, two
// decodes, the operation, the NaN and overflow tests, one encode, insert -- sixteen times per vector) is
// arithmetic-bound through these kernels.  So SUM and PROD offer the header's packed combine (below), and the same
// rows again, packed against per byte in one process (profiles/r11/fp8/userop_bench_packed_ab.json):
//                              f16 SUM        E4M3 IEEE packed | per byte    E4M3 SAT packed | per byte     E5M2 IEEE packed | per byte
//   fold m = 1, GB/s           5306 / 5392    5221 / 5251 | 4713 / 4802      5199 / 5256 | 4803 / 4923      5090 / 5112 | 4343 / 4553
//   fold m = 3, GB/s           5315 / 5297    5047 / 5031 | 4166 / 4158      5023 / 5044 | 4514 / 4516      4475 / 4495 | 3481 / 3484
//   tree, 16 MiB leaves        0.705 / 0.706  0.506 / 0.506 | 0.299 / 0.299  0.515 / 0.516 | 0.328 / 0.328  0.367 / 0.367 | 0.264 / 0.264
//   tree, 64 MiB leaves        0.767 / 0.772  0.591 / 0.607 | 0.352 / 0.352  0.620 / 0.619 | 0.396 / 0.397  0.439 / 0.439 | 0.311 / 0.310
// The ranges separate in the packed path's favour in every row for all three ops, so all of SUM and PROD keep it
// (PROD and E5M2 SATURATE, which the rows do not time, are the same code but for one instruction, or the guard of
// E4M3 SATURATE).  The folds come within 1-6 % of binary16 (E5M2 m = 3: 16 %); the trees, seven combines per element,
// stay arithmetic-bound at 0.72-0.81 of it (E5M2 IEEE, whose guard builds a signed infinity: 0.52-0.57).  MAX and MIN
// have no packed form: they were not timed.
//
// Two 16-B vectors per lane per fold trip, not the header's four: a vector is 16 elements here, and at four the
// compiler held 91-93 VGPRs for the per-byte SUM / PROD and spills MAX / MIN at 128; at two the packed SUM / PROD take
// 63-64 and MAX / MIN 71, inside the 72 a wave may hold beside RCCL (tests/test_fp8_host.py).
#define CHR_USER_FOLD_U 2

#include <atomic>
#include <mutex>

#include "chiara_fp8.h"
#include "chiara_user_op.hpp"

namespace chr_fp8 {  // named: the functors are template arguments of the kernels, whose symbols the resource test reads

using f8 = uint8_t;  // a code of either format; the functor's template arguments say which

constexpr int kE4M3 = CHR_FP8_E4M3, kE5M2 = CHR_FP8_E5M2, kIEEE = CHR_FP8_IEEE, kSat = CHR_FP8_SATURATE;

template <int FMT>
__device__ __forceinline__ float dec(f8 b) {
    if constexpr (FMT == kE4M3) return __builtin_amdgcn_cvt_f32_fp8((int)b, 0);
    else return __builtin_amdgcn_cvt_f32_bf8((int)b, 0);
}

// The format's code of the f32 value r under policy OVF: one round-to-nearest-even with the exponent unbounded.
//   NaN                    the canonical NaN, positive
//   |r| past the last magnitude that rounds to max (E4M3: 464, the tie, goes to the even 448; E5M2: 61440, the tie,
//   goes to the even side above max, so it is already past)
//                          IEEE: E4M3 the canonical NaN, E5M2 +-inf;  SATURATE: +-max
//   max < |r| otherwise    +-max
//   anything else          the instruction
template <int FMT, int OVF>
__device__ __forceinline__ f8 enc(float r) {
    constexpr float kMax = FMT == kE4M3 ? 448.0f : 57344.0f;
    constexpr f8 kNaN = FMT == kE4M3 ? 0x7F : 0x7E;
    if (r != r) return kNaN;
    const float a = __builtin_fabsf(r);
    if constexpr (OVF == kIEEE) {
        const bool over = FMT == kE4M3 ? a > 464.0f : a >= 61440.0f;
        if (over) return FMT == kE4M3 ? kNaN : (f8)(((__builtin_bit_cast(uint32_t, r) >> 24) & 0x80u) | 0x7Cu);
    }
    const float c = a > kMax ? __builtin_copysignf(kMax, r) : r;
    int w;
    if constexpr (FMT == kE4M3) w = __builtin_amdgcn_cvt_pk_fp8_f32(c, c, 0, false);
    else w = __builtin_amdgcn_cvt_pk_bf8_f32(c, c, 0, false);
    return (f8)(w & 0xFF);
}

// ---- the packed combine: the four elements of a word (include/chiara_user_op.hpp, packed combines) ------------------
//
// Two packed decodes per operand word, four f32 operations, the guard of enc() per value, two packed encodes.  A value
// the guard decides itself (NaN, and under IEEE overflow) goes to the instruction as +0, whose code is 0x00, and its
// code is OR-ed into the word afterwards; every other value is clamped to [-max, +max] by a median, which keeps the
// sign of zero.  Which ops take it is a measurement (the table above): CHR_FP8_PACKED 1 -- those that pay; 0 -- none
// (the per-byte side of the A/B: make fp8_ab); 2 -- all.
#ifndef CHR_FP8_PACKED
#define CHR_FP8_PACKED 1
#endif
constexpr bool packed_pays(int /*fmt*/, int /*ovf*/) { return true; }  // every timed (format, policy) separated
constexpr bool packs(int fmt, int ovf) { return CHR_FP8_PACKED == 2 || (CHR_FP8_PACKED == 1 && packed_pays(fmt, ovf)); }

typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int FMT, bool HI>
__device__ __forceinline__ f32x2 dec2(uint32_t w) {
    if constexpr (FMT == kE4M3) return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
    else return __builtin_amdgcn_cvt_pk_f32_bf8((int)w, HI);
}

// enc()'s decisions for byte K of a word: c is what the instruction converts, o collects the codes decided here.
template <int FMT, int OVF, int K>
__device__ __forceinline__ void guard(float r, float& c, uint32_t& o) {
    constexpr float kMax = FMT == kE4M3 ? 448.0f : 57344.0f;
    constexpr uint32_t kNaN = FMT == kE4M3 ? 0x7Fu : 0x7Eu;
    const float a = __builtin_fabsf(r);
    bool own;       // NaN, or overflow under IEEE (the negated compares are true for NaN)
    uint32_t code;
    if constexpr (OVF == kSat) {
        own = r != r;
        code = kNaN;
    } else if constexpr (FMT == kE4M3) {
        own = !(a <= 464.0f);
        code = kNaN;
    } else {
        own = !(a < 61440.0f);
        code = r != r ? kNaN : (((__builtin_bit_cast(uint32_t, r) >> 24) & 0x80u) | 0x7Cu);
    }
    c = own ? 0.0f : __builtin_amdgcn_fmed3f(r, -kMax, kMax);
    o |= own ? code << (8 * K) : 0u;
}

template <int FMT, int OVF, bool MUL>
__device__ __forceinline__ uint32_t packed_arith(uint32_t in, uint32_t inout) {
    const f32x2 xl = dec2<FMT, false>(in), xh = dec2<FMT, true>(in);
    const f32x2 yl = dec2<FMT, false>(inout), yh = dec2<FMT, true>(inout);
    const f32x2 rl = MUL ? yl * xl : yl + xl, rh = MUL ? yh * xh : yh + xh;
    float c0, c1, c2, c3;
    uint32_t o = 0;
    guard<FMT, OVF, 0>(rl[0], c0, o);
    guard<FMT, OVF, 1>(rl[1], c1, o);
    guard<FMT, OVF, 2>(rh[0], c2, o);
    guard<FMT, OVF, 3>(rh[1], c3, o);
    int w;
    if constexpr (FMT == kE4M3) {
        w = __builtin_amdgcn_cvt_pk_fp8_f32(c0, c1, 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(c2, c3, w, true);
    } else {
        w = __builtin_amdgcn_cvt_pk_bf8_f32(c0, c1, 0, false);
        w = __builtin_amdgcn_cvt_pk_bf8_f32(c2, c3, w, true);
    }
    return (uint32_t)w | o;
}

template <int FMT, int OVF, bool MUL, bool PACKED>
struct Arith {
    __device__ f8 operator()(f8 in, f8 inout) const {
        return enc<FMT, OVF>(MUL ? dec<FMT>(inout) * dec<FMT>(in) : dec<FMT>(inout) + dec<FMT>(in));
    }
};
template <int FMT, int OVF, bool MUL>
struct Arith<FMT, OVF, MUL, true> : Arith<FMT, OVF, MUL, false> {
    static __device__ __forceinline__ uint32_t packed(uint32_t in, uint32_t inout) {
        return packed_arith<FMT, OVF, MUL>(in, inout);
    }
};
template <int FMT, int OVF> struct Sum : Arith<FMT, OVF, false, packs(FMT, OVF)> {};
template <int FMT, int OVF> struct Prod : Arith<FMT, OVF, true, packs(FMT, OVF)> {};
// csrc/reduce_common.hpp apply()'s float rule: a tie or an unordered compare returns `in`; a select moves the byte.
template <int FMT>
struct Max {
    __device__ f8 operator()(f8 in, f8 inout) const { return dec<FMT>(inout) > dec<FMT>(in) ? inout : in; }
};
template <int FMT>
struct Min {
    __device__ f8 operator()(f8 in, f8 inout) const { return dec<FMT>(inout) < dec<FMT>(in) ? inout : in; }
};

// ---- the casts: 16 codes <-> 16 f32 (four 16-B vectors) or 16 bf16 (two) per lane ---------------------------------
//
// A lane's unit is 16 consecutive elements: every access 16 bytes when both pointers are 16-B aligned (vec),
// grid-stride, then the elements past the last whole unit (or, unaligned, every element) one per lane.  Each index is
// read and written by one lane.
constexpr unsigned kCastBlock = 256;
constexpr unsigned kCastMaxBlocks = 4096;

using w4 = chr_user::tree_w4;
using bf16_bits = uint16_t;

__device__ __forceinline__ float widen(float x) { return x; }
__device__ __forceinline__ float widen(bf16_bits x) { return __builtin_bit_cast(float, (uint32_t)x << 16); }
// One canonical NaN out of a dequantize; the f32 -> bf16 rounding is the library's (csrc/reduce_common.hpp f2bf).
__device__ __forceinline__ void narrow(float r, float& o) { o = r != r ? __builtin_bit_cast(float, 0x7FC00000u) : r; }
__device__ __forceinline__ void narrow(float r, bf16_bits& o) {
    o = r != r ? (bf16_bits)0x7FC0 : __builtin_bit_cast(bf16_bits, (__bf16)r);
}

template <typename W> struct Wide16 { W e[16]; };
template <typename W> struct WideWords { w4 w[sizeof(W)]; };  // 16 W: sizeof(W) vectors of 16 bytes
struct Codes16 { f8 e[16]; };

template <typename S, int FMT, int OVF>
__global__ __launch_bounds__(kCastBlock) void k_quantize(void* dst, const void* src, size_t n, float scale, int vec) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t done = 0;
    if (vec) {
        constexpr int K = (int)sizeof(S);
        const size_t nv = n / 16;
        const w4* inv = static_cast<const w4*>(src);
        w4* outv = static_cast<w4*>(dst);
        for (size_t v = tid; v < nv; v += stride) {
            WideWords<S> w;
#pragma unroll
            for (int k = 0; k < K; ++k) w.w[k] = inv[v * K + k];
            const Wide16<S> x = __builtin_bit_cast(Wide16<S>, w);
            Codes16 r;
#pragma unroll
            for (int e = 0; e < 16; ++e) r.e[e] = enc<FMT, OVF>(widen(x.e[e]) * scale);
            outv[v] = __builtin_bit_cast(w4, r);
        }
        done = nv * 16;
    }
    for (size_t i = done + tid; i < n; i += stride)
        static_cast<f8*>(dst)[i] = enc<FMT, OVF>(widen(static_cast<const S*>(src)[i]) * scale);
}

template <typename D, int FMT>
__global__ __launch_bounds__(kCastBlock) void k_dequantize(void* dst, const void* src, size_t n, float scale, int vec) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t done = 0;
    if (vec) {
        constexpr int K = (int)sizeof(D);
        const size_t nv = n / 16;
        const w4* inv = static_cast<const w4*>(src);
        w4* outv = static_cast<w4*>(dst);
        for (size_t v = tid; v < nv; v += stride) {
            const Codes16 x = __builtin_bit_cast(Codes16, inv[v]);
            Wide16<D> r;
#pragma unroll
            for (int e = 0; e < 16; ++e) narrow(dec<FMT>(x.e[e]) * scale, r.e[e]);
            const WideWords<D> w = __builtin_bit_cast(WideWords<D>, r);
#pragma unroll
            for (int k = 0; k < K; ++k) outv[v * K + k] = w.w[k];
        }
        done = nv * 16;
    }
    for (size_t i = done + tid; i < n; i += stride)
        narrow(dec<FMT>(static_cast<const f8*>(src)[i]) * scale, static_cast<D*>(dst)[i]);
}

}  // namespace chr_fp8

using namespace chr_fp8;

// Both launchers of each op, for CHR_UINT8 alone: any other dtype is declined before anything is enqueued.
#define CHR_FP8_OP(name, ...)                                                                                        \
    CHR_DEFINE_USER_OP_FOR(chr_fp8_##name##_fold, f8, __VA_ARGS__, CHR_FP8_DTYPE)                                    \
    CHR_DEFINE_USER_TREE_FOR(chr_fp8_##name##_tree, f8, __VA_ARGS__, CHR_FP8_DTYPE)
namespace {
using SumE4I = Sum<kE4M3, kIEEE>;
using SumE4S = Sum<kE4M3, kSat>;
using ProdE4I = Prod<kE4M3, kIEEE>;
using ProdE4S = Prod<kE4M3, kSat>;
using SumE5I = Sum<kE5M2, kIEEE>;
using SumE5S = Sum<kE5M2, kSat>;
using ProdE5I = Prod<kE5M2, kIEEE>;
using ProdE5S = Prod<kE5M2, kSat>;
}  // namespace
CHR_FP8_OP(e4m3_sum_ieee, SumE4I)
CHR_FP8_OP(e4m3_sum_sat, SumE4S)
CHR_FP8_OP(e4m3_prod_ieee, ProdE4I)
CHR_FP8_OP(e4m3_prod_sat, ProdE4S)
CHR_FP8_OP(e4m3_max, Max<kE4M3>)
CHR_FP8_OP(e4m3_min, Min<kE4M3>)
CHR_FP8_OP(e5m2_sum_ieee, SumE5I)
CHR_FP8_OP(e5m2_sum_sat, SumE5S)
CHR_FP8_OP(e5m2_prod_ieee, ProdE5I)
CHR_FP8_OP(e5m2_prod_sat, ProdE5S)
CHR_FP8_OP(e5m2_max, Max<kE5M2>)
CHR_FP8_OP(e5m2_min, Min<kE5M2>)

namespace {

std::atomic<long> g_fold_calls{0}, g_tree_calls{0}, g_trees{0};

static_assert(CHR_SUM == 0 && CHR_PROD == 1 && CHR_MAX == 2 && CHR_MIN == 3 && kE4M3 == 0 && kE5M2 == 1 && kIEEE == 0 &&
                  kSat == 1,
              "kKinds and g_code are indexed by these values");

// What is registered: the launchers above behind the counters of chr_fp8_stats.  The op's ctx is its Kind.
struct Kind {
    chr_user_reduce_fn fold;
    chr_user_tree_fn tree;
};
#define CHR_FP8_KIND(name) {chr_fp8_##name##_fold, chr_fp8_##name##_tree}
// [format][kind][policy]; MAX and MIN have one op, under policy 0
const Kind kKinds[2][4][2] = {
    {{CHR_FP8_KIND(e4m3_sum_ieee), CHR_FP8_KIND(e4m3_sum_sat)},
     {CHR_FP8_KIND(e4m3_prod_ieee), CHR_FP8_KIND(e4m3_prod_sat)},
     {CHR_FP8_KIND(e4m3_max), {nullptr, nullptr}},
     {CHR_FP8_KIND(e4m3_min), {nullptr, nullptr}}},
    {{CHR_FP8_KIND(e5m2_sum_ieee), CHR_FP8_KIND(e5m2_sum_sat)},
     {CHR_FP8_KIND(e5m2_prod_ieee), CHR_FP8_KIND(e5m2_prod_sat)},
     {CHR_FP8_KIND(e5m2_max), {nullptr, nullptr}},
     {CHR_FP8_KIND(e5m2_min), {nullptr, nullptr}}},
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
int g_code[2][4][2] = {{{-1, -1}, {-1, -1}, {-1, -1}, {-1, -1}},  // the live op of each combination; -1: not registered
                       {{-1, -1}, {-1, -1}, {-1, -1}, {-1, -1}}};

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned cast_grid(size_t n, bool vec) {
    const size_t lanes = vec ? n / 16 + n % 16 : n;
    const size_t blocks = (lanes + kCastBlock - 1) / kCastBlock;
    return (unsigned)(blocks < kCastMaxBlocks ? (blocks ? blocks : 1) : kCastMaxBlocks);
}

template <typename S, int FMT, int OVF>
int launch_quantize(void* dst, const void* src, size_t n, float scale, hipStream_t s) {
    const bool vec = aligned16(dst) && aligned16(src);
    hipLaunchKernelGGL((k_quantize<S, FMT, OVF>), dim3(cast_grid(n, vec)), dim3(kCastBlock), 0, s, dst, src, n, scale,
                       vec ? 1 : 0);
    return hipGetLastError() == hipSuccess ? CHR_SUCCESS : CHR_ERR_HIP;
}

template <typename S>
int quantize_of(void* dst, const void* src, size_t n, int f, float scale, int o, hipStream_t s) {
    if (f == kE4M3)
        return o == kIEEE ? launch_quantize<S, kE4M3, kIEEE>(dst, src, n, scale, s)
                          : launch_quantize<S, kE4M3, kSat>(dst, src, n, scale, s);
    return o == kIEEE ? launch_quantize<S, kE5M2, kIEEE>(dst, src, n, scale, s)
                      : launch_quantize<S, kE5M2, kSat>(dst, src, n, scale, s);
}

template <typename D, int FMT>
int launch_dequantize(void* dst, const void* src, size_t n, float scale, hipStream_t s) {
    const bool vec = aligned16(dst) && aligned16(src);
    hipLaunchKernelGGL((k_dequantize<D, FMT>), dim3(cast_grid(n, vec)), dim3(kCastBlock), 0, s, dst, src, n, scale,
                       vec ? 1 : 0);
    return hipGetLastError() == hipSuccess ? CHR_SUCCESS : CHR_ERR_HIP;
}

bool format_ok(int f) { return f == kE4M3 || f == kE5M2; }
bool policy_ok(int o) { return o == kIEEE || o == kSat; }
bool wide_ok(chr_dtype t) { return t == CHR_FLOAT32 || t == CHR_BFLOAT16; }

}  // namespace

extern "C" {

int chr_fp8_op(chr_fp8_format f, chr_op kind, chr_fp8_overflow o, chr_op* op) {
    if (!op) return CHR_ERR_INVALID_ARG;
    const int k = (int)kind;
    if (k != CHR_SUM && k != CHR_PROD && k != CHR_MAX && k != CHR_MIN) return CHR_ERR_UNSUPPORTED;
    if (!format_ok((int)f) || !policy_ok((int)o)) return CHR_ERR_UNSUPPORTED;
    const int p = (k == CHR_MAX || k == CHR_MIN) ? 0 : (int)o;
    std::lock_guard<std::mutex> lk(g_mu);
    int& slot = g_code[(int)f][k][p];
    if (slot < 0) {
        chr_op code;
        if (int rc = chr_op_create_tree(counted_fold, counted_tree, const_cast<Kind*>(&kKinds[(int)f][k][p]), 1, &code))
            return rc;
        slot = (int)code;
    }
    *op = (chr_op)slot;
    return CHR_SUCCESS;
}

int chr_fp8_quantize(void* dst, const void* src, size_t n, chr_dtype src_type, chr_fp8_format f, float scale,
                     chr_fp8_overflow o, hipStream_t s) {
    if (!dst || !src) return CHR_ERR_INVALID_ARG;
    if (!wide_ok(src_type) || !format_ok((int)f) || !policy_ok((int)o)) return CHR_ERR_UNSUPPORTED;
    if (n == 0) return CHR_SUCCESS;
    return src_type == CHR_FLOAT32 ? quantize_of<float>(dst, src, n, (int)f, scale, (int)o, s)
                                   : quantize_of<bf16_bits>(dst, src, n, (int)f, scale, (int)o, s);
}

int chr_fp8_dequantize(void* dst, const void* src, size_t n, chr_dtype dst_type, chr_fp8_format f, float scale,
                       hipStream_t s) {
    if (!dst || !src) return CHR_ERR_INVALID_ARG;
    if (!wide_ok(dst_type) || !format_ok((int)f)) return CHR_ERR_UNSUPPORTED;
    if (n == 0) return CHR_SUCCESS;
    if (dst_type == CHR_FLOAT32)
        return f == CHR_FP8_E4M3 ? launch_dequantize<float, kE4M3>(dst, src, n, scale, s)
                                 : launch_dequantize<float, kE5M2>(dst, src, n, scale, s);
    return f == CHR_FP8_E4M3 ? launch_dequantize<bf16_bits, kE4M3>(dst, src, n, scale, s)
                             : launch_dequantize<bf16_bits, kE5M2>(dst, src, n, scale, s);
}

int chr_fp8_release(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = CHR_SUCCESS;
    for (auto& fmt : g_code)
        for (auto& kind : fmt)
            for (int& c : kind) {
                if (c < 0) continue;
                const int e = chr_op_free((chr_op)c);
                if (!rc) rc = e;
                c = -1;
            }
    return rc;
}

void chr_fp8_stats(long out[3], int reset) {
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
