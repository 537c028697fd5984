// mx6_ops.hip -- libchiara_mx6.so: the MXFP6 block-scaled SUM (E2M3 and E3M2) on the user-op interface, and the casts
// into and out of the MX6 tile (include/chiara_mx6.h has the contract: the 400-byte tile, the SUM rule, the error
// codes).  The rule is libchiara_mx4.so's with six-bit codes; the kernels are not k_mx4_fold with another constant,
// because a block of 32 six-bit codes is 24 bytes -- neither one 16-B access nor a whole number of bytes per value --
// and gfx950 converts FP6 a whole block at a time.  Every kernel is templated on the format.  Built with the package's
// HIPFLAGS (-fno-fast-math, -ffp-contract=off) and with packed f32 arithmetic disabled for this code object, so that
// the 32 sums of a lane stay 32 v_add_f32.
//
// How the work is split.  One-wave workgroups.  A lane owns a whole block, the unit of the converts; the 16 lanes of
// a DPP row are a tile, and a wave trip covers four tiles, 1 600 consecutive bytes.  Each lane loads its block's scale
// as a byte of the tile's 16-B header.  The amax and the scale choice are the lane's own, nothing is exchanged.  The
// only traffic between lanes is the assembly of a tile's 16 new scale bytes into four header words: two DPP row
// shifts (row_shl:1, row_shl:2) after which lanes 0, 4, 8 and 12 of the row store one word each.  No LDS.  The grid is
// capped at kMaxGrid workgroups and a launch takes 16 operands; a wider fan-in continues from `out`.
//
// Data movement.  A block lies at byte 16 + 24 b of its tile: 8-B aligned whenever the buffer is, 16-B aligned only
// for even b.  The wide path (every pointer 8-B aligned) is written as three 8-B non-temporal accesses, the other as
// six 4-B ones.  What shipped in the ISA is the same for both: gfx950 asks only word alignment of a multi-word global
// access and the backend merges neighbours, so a block moves as one global_load_dwordx4 and one global_load_dwordx2
// (and the same two stores), 4 bytes in as well as 16-B aligned (tests/test_gpu_mx6.py runs both).  The other wide
// shape, two 12-B accesses, was not measured: written in C++ it is merged into the same 16 + 8 pair, and nothing here
// is inline assembly.
//
// Registers.  72 VGPRs for the folds, 60 - 67 (64 - 72 allocated) for the casts, no scratch, no LDS
// (tests/test_mx6_resources.py).  A combine that decoded both operands to f32 would hold 64 values and 12 code words.
// Here the operand of the larger scale, which needs no shift, is decoded by v_cvt_scalef32_pk32_bf16_{fp6,bf6} into 16
// VGPRs -- every E2M3 and E3M2 value is exact in bf16 -- and only then the other one by v_cvt_scalef32_pk32_f32_{fp6,
// bf6} into 32, when both operands' code words are dead.  Each sum widens its bf16 half (one v_lshlrev_b32 or
// v_and_b32) as it is added, and the sums, the renormalised values and the encode's operands share the same 32
// registers.  Two scheduling barriers keep the decodes in that order: without them the scheduler begins the shifts of
// the f32 operand while the other's code words are alive and the fold takes 86 VGPRs.  Both decodes run at a literal
// scale of 1.0 and the operand of the smaller scale is aligned with v_ldexp_f32: a relative scale reaches 2^-254,
// below what the converts' scale operand holds (mx4_ops.hip has the argument).  Encode is
// v_cvt_scalef32_2xpk16_{fp6,bf6}_f32 at scale 1.0 on values already clamped to +-max with v_med3_f32.
//
// What the converts do, found on the device and pinned by tests/test_gpu_mx6.py (every code at every position, all
// 4 096 code pairs, every bf16 pattern): pk32 decodes value i from bits 6 i .. 6 i + 5, the tile's order, and the
// bf16 form puts value 2 k in the low half of VGPR k; 2xpk16 interleaves its operands, code 2 k from the first
// 16-vector's element k and code 2 k + 1 from the second's, so the even and the odd values of a block are its two
// operands; the encode rounds to nearest with ties to the even code, keeps subnormals, saturates, and keeps the sign
// of a zero and of a value that rounds to zero.  Nothing is corrected in VALU.
//
// Per lane and combine the ISA holds 1 v_cvt_scalef32_pk32_bf16, 1 v_cvt_scalef32_pk32_f32, 1 v_cvt_scalef32_2xpk16,
// 64 v_ldexp_f32 (32 aligning, 32 renormalising), 32 v_add_f32, 32 v_lshlrev_b32 / v_and_b32 (the widening), 16
// v_max3_f32, 32 v_med3_f32 and 20 v_cndmask_b32; per trip two v_mov_b32_dpp.  Against k_mx4_fold that is 3 converts
// for 48 and 32 widening instructions more.
//
// Measured (tools/userop_bench.py --mx6, folds in place at 127 100 tiles per operand -- 50.8 MB here, 67.1 MB for
// MXFP8, 34.6 MB for MXFP4 -- each over an HBM-cold rotation of its own, the four variants alternating within each
// round of one process, the command run twice: the range over the four rounds; profiles/r16/mx6/userop_bench.json and
// userop_bench_run2.json):
//                              MX E4M3 SUM    MX4 SUM        MX6 E2M3 SUM   MX6 E3M2 SUM   MX6 / MX E4M3
//   fold m = 1, GB/s           4449 - 4482    4514 - 4550    3849 - 3861    3846 - 3860
//   fold m = 1, 10^9 values/s  1438 - 1449    2832 - 2855    1642 - 1648    1641 - 1647    1.13 - 1.14
//   fold m = 3, GB/s           3345 - 3376    3204 - 3264    4044 - 4084    4014 - 4074
//   fold m = 3, 10^9 values/s   649 -  655    1206 - 1229    1035 - 1046    1027 - 1043    1.58 - 1.61
// GB/s is of the (m + 2) x bytes traffic.  The expectation was values per second not below the MXFP8 E4M3 fold's in
// the same process; it holds in both rows and for both formats.  At m = 1 the gain is less than the 1.32 the bytes
// alone would give (GB/s is 0.86 of MXFP8's); at m = 3, where the combines per byte weigh more, GB/s is 1.21 of
// MXFP8's: a combine here is three converts where k_mx_fold's decodes and encodes value by value.
#include <atomic>
#include <mutex>

#include <hip/hip_runtime.h>

#include "mx6_tile.hpp"  // the tile and the rule on the device: Place .. combine

namespace chr_mx6 {

constexpr int kMaxIns = 16;          // operands per launch; a wider fan-in continues from `out`
constexpr unsigned kMaxGrid = 4096;  // one-wave workgroups a launch strides over
using bf16_bits = uint16_t;

struct FoldArgs {
    void* out;
    const void* acc;
    const void* ins[kMaxIns];
    int m;
    size_t n;  // tiles
};

// out = ins[m-1] o (... (ins[0] o acc)) on n tiles, one HBM pass.  A tile is read and written by one row of a wave,
// all its loads before its stores: `out` may alias `acc`.  m == 0 copies.  The lanes of a trip's missing tiles carry
// zeros through the same instructions (the row shifts stay wave-wide) and neither load nor store.
template <int F, bool VEC>
__global__ __launch_bounds__(kWave) void k_mx6_fold(FoldArgs a) {
    const size_t trips = (a.n + kTripTiles - 1) / kTripTiles;
    const char* const acc = static_cast<const char*>(a.acc);
    char* const out = static_cast<char*>(a.out);
    for (size_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const Place at(trip);
        const bool live = at.tile < a.n;
        w6 r = {0u, 0u, 0u, 0u, 0u, 0u};
        int er = 0;
        if (live) {
            r = ld24<VEC>(acc + at.codes());
            er = ld_scale(acc + at.scale());
        }
        for (int j = 0; j < a.m; ++j) {
            const char* const in = static_cast<const char*>(a.ins[j]);
            w6 x = {0u, 0u, 0u, 0u, 0u, 0u};
            int ex = 0;
            if (live) {
                x = ld24<VEC>(in + at.codes());
                ex = ld_scale(in + at.scale());
            }
            combine<F>(r, er, x, ex);
        }
        const uint32_t word = header_word(er);
        if (live) st_tile<VEC>(out, at, r, word);
    }
}

__device__ __forceinline__ float widen(float x) { return x; }
__device__ __forceinline__ float widen(bf16_bits x) { return __builtin_bit_cast(float, (uint32_t)x << 16); }
// One canonical NaN out of a dequantize; the f32 -> bf16 rounding is the library's (csrc/reduce_common.hpp f2bf).
__device__ __forceinline__ void narrow(float r, float& o) { o = r != r ? __builtin_bit_cast(float, 0x7FC00000u) : r; }
__device__ __forceinline__ void narrow(float r, bf16_bits& o) {
    o = r != r ? (bf16_bits)0x7FC0 : __builtin_bit_cast(bf16_bits, (__bf16)r);
}

template <typename W> struct Wide32 { W e[kBlockValues]; };
template <typename W> struct WideWords { w4 w[2 * sizeof(W)]; };  // 32 W: 2 * sizeof(W) vectors of 16 bytes

// tiles = Q(src): a lane reads its block's 32 source values (128 B of f32, 64 B of bf16) as 16-B vectors where src is
// 16-B aligned (wide_vec) and all 32 lie below n, one by one and +0 beyond n otherwise.  A non-finite value makes the
// block the canonical NaN block; its own bits take no part in the arithmetic.
template <int F, typename S, bool VEC>
__global__ __launch_bounds__(kWave) void k_mx6_quantize(void* tiles, const void* src, size_t n, int wide_vec) {
    const size_t ntiles = (n + kTileValues - 1) / kTileValues, trips = (ntiles + kTripTiles - 1) / kTripTiles;
    const S* const in = static_cast<const S*>(src);
    for (size_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const Place at(trip);
        const bool live = at.tile < ntiles;
        const size_t i0 = at.value0();
        float s[kBlockValues];
        if (live && wide_vec && i0 + kBlockValues <= n) {
            WideWords<S> w;
#pragma unroll
            for (int k = 0; k < 2 * (int)sizeof(S); ++k)
                w.w[k] = __builtin_nontemporal_load(reinterpret_cast<const w4*>(in + i0) + k);
            const Wide32<S> x = __builtin_bit_cast(Wide32<S>, w);
#pragma unroll
            for (int i = 0; i < kBlockValues; ++i) s[i] = widen(x.e[i]);
        } else {
#pragma unroll
            for (int i = 0; i < kBlockValues; ++i) s[i] = live && i0 + i < n ? widen(in[i0 + i]) : 0.0f;
        }
        bool nan = false;
#pragma unroll
        for (int i = 0; i < kBlockValues; ++i) {
            const bool fin = __builtin_fabsf(s[i]) < __builtin_inff();
            nan |= !fin;
            s[i] = fin ? s[i] : 0.0f;
        }
        int e2;
        w6 codes = requantise<F>(s, kBias, 0, e2);
#pragma unroll
        for (int k = 0; k < kBlockWords; ++k) codes[k] = nan ? 0u : codes[k];
        const uint32_t word = header_word(nan ? kNaNScale : e2);
        if (live) st_tile<VEC>(static_cast<char*>(tiles), at, codes, word);
    }
}

// dst[i] = ldexp(dec(code i), scale - 127), i < n: a lane's 32 values as 16-B vectors where dst is 16-B aligned
// (wide_vec) and all 32 lie below n, one by one below n otherwise; a lane wholly beyond n touches nothing.
template <int F, typename D, bool VEC>
__global__ __launch_bounds__(kWave) void k_mx6_dequantize(void* dst, const void* tiles, size_t n, int wide_vec) {
    const size_t ntiles = (n + kTileValues - 1) / kTileValues, trips = (ntiles + kTripTiles - 1) / kTripTiles;
    const char* const in = static_cast<const char*>(tiles);
    D* const out = static_cast<D*>(dst);
    for (size_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const Place at(trip);
        const size_t i0 = at.value0();
        if (i0 >= n) continue;
        const f32x32 v = dec32<F>(ld24<VEC>(in + at.codes()));
        const int e = ld_scale(in + at.scale());
        const bool nan = e == kNaNScale;
        Wide32<D> r;
#pragma unroll
        for (int i = 0; i < kBlockValues; ++i) narrow(nan ? __builtin_nanf("") : __builtin_ldexpf(v[i], e - kBias), r.e[i]);
        if (wide_vec && i0 + kBlockValues <= n) {
            const WideWords<D> w = __builtin_bit_cast(WideWords<D>, r);
#pragma unroll
            for (int k = 0; k < 2 * (int)sizeof(D); ++k)
                __builtin_nontemporal_store(w.w[k], reinterpret_cast<w4*>(out + i0) + k);
        } else {
#pragma unroll
            for (int i = 0; i < kBlockValues; ++i)
                if (i0 + i < n) out[i0 + i] = r.e[i];
        }
    }
}

}  // namespace chr_mx6

using namespace chr_mx6;

namespace {

std::atomic<long> g_fold_calls{0}, g_declined{0}, g_kernels{0};

unsigned grid_for(size_t tiles) {
    const size_t trips = (tiles + kTripTiles - 1) / kTripTiles;
    return (unsigned)(trips < kMaxGrid ? (trips ? trips : 1) : kMaxGrid);
}

// The chr_user_reduce_fn of format F.  Declines -- nonzero, nothing enqueued -- any dtype but a live tile type and any
// pointer that is not 4-B aligned.  Fan-in beyond kMaxIns runs as consecutive launches, each continuing from `out`.
// running_first is not looked at: the rule commutes bit for bit.
template <int F>
int sum_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dt, hipStream_t stream) {
    ++g_fold_calls;
    uintptr_t al = bits_of(out) | bits_of(acc);
    bool ok = out && acc && m >= 0 && (m == 0 || ins) && is_tile_type(dt);
    for (int j = 0; ok && j < m; ++j) {
        ok = ins[j] != nullptr;
        al |= bits_of(ins[j]);
    }
    if (!ok || (al & 3)) {
        ++g_declined;
        return 1;
    }
    if (n == 0) return 0;
    const bool vec = (al & 7) == 0;
    const unsigned grid = grid_for(n);
    int done = 0;
    const void* cur = acc;
    do {
        FoldArgs a{};
        a.out = out;
        a.acc = cur;
        a.m = m - done < kMaxIns ? m - done : kMaxIns;
        for (int j = 0; j < a.m; ++j) a.ins[j] = ins[done + j];
        a.n = n;
        if (vec) hipLaunchKernelGGL((k_mx6_fold<F, true>), dim3(grid), dim3(kWave), 0, stream, a);
        else hipLaunchKernelGGL((k_mx6_fold<F, false>), dim3(grid), dim3(kWave), 0, stream, a);
        if (hipGetLastError() != hipSuccess) return 1;
        ++g_kernels;
        done += a.m;
        cur = out;
    } while (done < m);
    return 0;
}

}  // namespace

extern "C" int chr_mx6_e2m3_sum_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dt,
                                     int, hipStream_t stream, void*) {
    return sum_fold<CHR_MX6_E2M3>(out, acc, ins, m, n, dt, stream);
}
extern "C" int chr_mx6_e3m2_sum_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dt,
                                     int, hipStream_t stream, void*) {
    return sum_fold<CHR_MX6_E3M2>(out, acc, ins, m, n, dt, stream);
}

namespace {

std::mutex g_mu;
int g_op[2] = {-1, -1};  // the live op of each format; -1: not registered
int g_type = -1;         // the cached tile type

bool wide_ok(chr_dtype t) { return t == CHR_FLOAT32 || t == CHR_BFLOAT16; }
bool format_ok(chr_mx6_format f) { return f == CHR_MX6_E2M3 || f == CHR_MX6_E3M2; }

template <int F, typename S>
int launch_quantize(void* tiles, const void* src, size_t n, hipStream_t s) {
    const unsigned grid = grid_for((n + CHR_MX6_TILE_VALUES - 1) / CHR_MX6_TILE_VALUES);
    const int wide_vec = (bits_of(src) & 15) == 0;
    if ((bits_of(tiles) & 7) == 0)
        hipLaunchKernelGGL((k_mx6_quantize<F, S, true>), dim3(grid), dim3(kWave), 0, s, tiles, src, n, wide_vec);
    else
        hipLaunchKernelGGL((k_mx6_quantize<F, S, false>), dim3(grid), dim3(kWave), 0, s, tiles, src, n, wide_vec);
    return hipGetLastError() == hipSuccess ? CHR_SUCCESS : CHR_ERR_HIP;
}

template <int F, typename D>
int launch_dequantize(void* dst, const void* tiles, size_t n, hipStream_t s) {
    const unsigned grid = grid_for((n + CHR_MX6_TILE_VALUES - 1) / CHR_MX6_TILE_VALUES);
    const int wide_vec = (bits_of(dst) & 15) == 0;
    if ((bits_of(tiles) & 7) == 0)
        hipLaunchKernelGGL((k_mx6_dequantize<F, D, true>), dim3(grid), dim3(kWave), 0, s, dst, tiles, n, wide_vec);
    else
        hipLaunchKernelGGL((k_mx6_dequantize<F, D, false>), dim3(grid), dim3(kWave), 0, s, dst, tiles, n, wide_vec);
    return hipGetLastError() == hipSuccess ? CHR_SUCCESS : CHR_ERR_HIP;
}

// What both casts check before anything is enqueued; CHR_SUCCESS: launch.
int cast_args(const void* tiles, const void* wide, chr_dtype wide_type, chr_mx6_format f) {
    if (!tiles || !wide || !format_ok(f)) return CHR_ERR_INVALID_ARG;
    if (!wide_ok(wide_type)) return CHR_ERR_UNSUPPORTED;
    if ((bits_of(tiles) & 3) || (bits_of(wide) & (wide_type == CHR_FLOAT32 ? 3 : 1))) return CHR_ERR_UNSUPPORTED;
    return CHR_SUCCESS;
}

}  // namespace

extern "C" {

int chr_mx6_type(chr_dtype* type) {
    if (!type) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_type < 0) {
        chr_dtype code;
        if (int rc = chr_type_contiguous(CHR_MX6_TILE_BYTES / 4, CHR_UINT32, &code)) return rc;
        g_type = (int)code;
    }
    *type = (chr_dtype)g_type;
    return CHR_SUCCESS;
}

int chr_mx6_sum(chr_mx6_format f, chr_op* op) {
    if (!op || !format_ok(f)) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_op[f] < 0) {
        chr_op code;
        if (int rc = chr_op_create(f == CHR_MX6_E2M3 ? chr_mx6_e2m3_sum_fold : chr_mx6_e3m2_sum_fold, nullptr, 1, &code))
            return rc;
        g_op[f] = (int)code;
    }
    *op = (chr_op)g_op[f];
    return CHR_SUCCESS;
}

int chr_mx6_quantize(void* tiles, const void* src, size_t n, chr_dtype src_type, chr_mx6_format f, hipStream_t s) {
    if (int rc = cast_args(tiles, src, src_type, f)) return rc;
    if (n == 0) return CHR_SUCCESS;
    if (f == CHR_MX6_E2M3)
        return src_type == CHR_FLOAT32 ? launch_quantize<CHR_MX6_E2M3, float>(tiles, src, n, s)
                                       : launch_quantize<CHR_MX6_E2M3, bf16_bits>(tiles, src, n, s);
    return src_type == CHR_FLOAT32 ? launch_quantize<CHR_MX6_E3M2, float>(tiles, src, n, s)
                                   : launch_quantize<CHR_MX6_E3M2, bf16_bits>(tiles, src, n, s);
}

int chr_mx6_dequantize(void* dst, const void* tiles, size_t n, chr_dtype dst_type, chr_mx6_format f, hipStream_t s) {
    if (int rc = cast_args(tiles, dst, dst_type, f)) return rc;
    if (n == 0) return CHR_SUCCESS;
    if (f == CHR_MX6_E2M3)
        return dst_type == CHR_FLOAT32 ? launch_dequantize<CHR_MX6_E2M3, float>(dst, tiles, n, s)
                                       : launch_dequantize<CHR_MX6_E2M3, bf16_bits>(dst, tiles, n, s);
    return dst_type == CHR_FLOAT32 ? launch_dequantize<CHR_MX6_E3M2, float>(dst, tiles, n, s)
                                   : launch_dequantize<CHR_MX6_E3M2, bf16_bits>(dst, tiles, n, s);
}

int chr_mx6_release(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = CHR_SUCCESS;
    for (int& op : g_op) {
        if (op < 0) continue;
        const int e = chr_op_free((chr_op)op);
        if (!rc) rc = e;
        op = -1;
    }
    if (g_type >= 0) {
        const int e = chr_type_free((chr_dtype)g_type);
        if (!rc) rc = e;
        g_type = -1;
    }
    return rc;
}

void chr_mx6_stats(long out[3], int reset) {
    if (out) {
        out[0] = g_fold_calls;
        out[1] = g_declined;
        out[2] = g_kernels;
    }
    if (reset) {
        g_fold_calls = 0;
        g_declined = 0;
        g_kernels = 0;
    }
}

}  // extern "C"
