// mx4_ops.hip -- libchiara_mx4.so: the MXFP4 block-scaled SUM on the user-op interface, and the casts into and out of
// the MX4 tile (include/chiara_mx4.h has the contract: the 272-byte tile, the SUM rule, the error codes).  The rule is
// libchiara_mx.so's with E2M1 codes; the kernels are not k_mx_fold with another constant, because a block of 32
// four-bit codes is 16 bytes: a single 16-B access holds a whole block.  Built with the package's HIPFLAGS
// (-fno-fast-math, -ffp-contract=off) and with packed f32 arithmetic disabled for this code object, so that the 32
// sums of a lane stay 32 v_add_f32.
//
// How the work is split.  One-wave workgroups.  A lane owns a whole block: its 32 codes are one 16-B access, the 16
// lanes of a DPP row are a tile, and a wave trip covers four tiles, 1 088 consecutive bytes.  Each lane loads its
// block's scale as a byte of the tile's 16-B header.  The block's amax and its scale choice are then the lane's own
// business -- where k_mx_fold's lane pair exchanges its amax by DPP and both lanes choose the same scale, here nothing
// is exchanged and nothing is computed twice.  The only traffic between lanes is the assembly of a tile's 16 new scale
// bytes into four header words: two DPP row shifts (row_shl:1, row_shl:2) after which lanes 0, 4, 8 and 12 of the
// row store one word each.  No LDS is allocated and no ds_bpermute is issued.
//
// One sweep.  The 32 sums of a block stay in registers as f32 from decode to encode: the amax needs all of them
// before the first can be encoded, and they fit -- the fold takes 59 VGPRs (64 allocated), the casts 52 - 58, no
// scratch (tests/test_mx4_resources.py).  The other shape, an amax sweep followed by a second sweep that re-derives
// the sums for the encode, would hold 8 sums at a time and pay for it with every decode, aligning v_ldexp_f32 and
// v_add_f32 issued twice, 96 more VALU instructions per combine beside the 192 listed below, in a kernel whose rate falls
// with the combines per byte; it was not needed and is not shipped.
//
// Decode is gfx950's v_cvt_scalef32_pk_f32_fp4 at a literal scale 1.0 with op_sel picking the byte, followed by one
// v_ldexp_f32 on the operand of the smaller scale (the other shift of the rule is 0, and f32 addition commutes bit for
// bit, so the kernel does not branch on running_first).  The convert's own scale operand could fold that ldexp into
// the decode, but a relative scale reaches 2^-254, below what an f32 scale operand holds, and no test has shown the
// same bits for the shifts in between: the plain decode and v_ldexp_f32 are the rule as written.  Encode is
// v_cvt_scalef32_pk_fp4_f32 at scale 1.0 on values already clamped to [-6, 6] with v_med3_f32.  On the device both
// converts are the rule as it stands: the low nibble is element 0 on both sides, the encode rounds to nearest with
// ties to the even code, keeps the subnormal 0.5, and keeps the sign of a zero and of a value that rounds to zero, so
// nothing is corrected in VALU.  tests/test_gpu_mx4.py pins that on all 256 code pairs and on every bf16 pattern.
// The scale choice is one v_frexp_exp / v_frexp_mant pair and one compare: max = 6 = 0.75 * 2^3, so with
// amax = f * 2^x, f in [0.5, 1), the smallest E with amax * 2^-E <= 6 is x - 3, plus 1 when f > 0.75.
//
// k_mx4_fold requantises every intermediate block in registers: each `o` rounds to the format, and the bits equal the
// fold-by-fold result, with m + 1 reads and one write per tile.  Loads and stores are non-temporal; the grid is capped
// at kMaxGrid one-wave workgroups.  The casts keep the split: a lane reads or writes its block's 32 wide values, 128 B
// of f32 or 64 B of bf16, as 16-B vectors where the wide buffer is 16-B aligned and the block lies wholly below n,
// one by one at the tail.
//
// Per lane and combine the ISA holds 32 v_cvt_scalef32_pk_f32_fp4, 64 v_ldexp_f32 (32 aligning, 32 renormalising), 32
// v_add_f32, 16 v_max3_f32 (the amax, two sums at a time), 32 v_med3_f32 and 16 v_cvt_scalef32_pk_fp4_f32; per trip
// two v_mov_b32_dpp.
//
// Measured (tools/userop_bench.py --mx4, folds in place at 127 100 tiles per operand -- 34.6 MB here, 67.1 MB for
// MXFP8 -- each over an HBM-cold rotation of its own, alternating rounds with libchiara_mx.so's E4M3 fold in one
// process, the command run twice: the range over the four rounds; profiles/r14/mx4/userop_bench.json):
//                              MX E4M3 SUM      MX4 SUM          MX4 / MX E4M3
//   fold m = 1, GB/s           4472 - 4491      4529 - 4576      1.010 - 1.019
//   fold m = 1, 10^9 values/s  1445 - 1452      2841 - 2871      1.96 - 1.98
//   fold m = 3, GB/s           3373 - 3385      3261 - 3279      0.965 - 0.972
//   fold m = 3, 10^9 values/s   654 -  656      1228 - 1234      1.87 - 1.89
// GB/s is of the (m + 2) x bytes traffic.  The expectation was MXFP8's arithmetic per value on half the bytes: GB/s
// lower, values per second not lower.  Values per second bear it out in both rows.  GB/s is lower at m = 3 and is not
// at m = 1, where the ranges lie clear of each other the other way round: twice the values per byte at the same
// bytes per second, which says the MXFP8 fold at m = 1 is not held by its arithmetic alone.
#include <atomic>
#include <mutex>

#include <hip/hip_runtime.h>

#include "mx4_tile.hpp"  // the tile and the rule on the device: Place .. combine

namespace chr_mx4 {

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
template <bool VEC>
__global__ __launch_bounds__(kWave) void k_mx4_fold(FoldArgs a) {
    const size_t trips = (a.n + kTripTiles - 1) / kTripTiles;
    const char* const acc = static_cast<const char*>(a.acc);
    char* const out = static_cast<char*>(a.out);
    for (size_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const Place at(trip);
        const bool live = at.tile < a.n;
        w4 r = {0u, 0u, 0u, 0u};
        int er = 0;
        if (live) {
            r = ld16<VEC>(acc + at.codes());
            er = ld_scale(acc + at.scale());
        }
        for (int j = 0; j < a.m; ++j) {
            const char* const in = static_cast<const char*>(a.ins[j]);
            w4 x = {0u, 0u, 0u, 0u};
            int ex = 0;
            if (live) {
                x = ld16<VEC>(in + at.codes());
                ex = ld_scale(in + at.scale());
            }
            combine(r, er, x, ex);
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
template <typename S, bool VEC>
__global__ __launch_bounds__(kWave) void k_mx4_quantize(void* tiles, const void* src, size_t n, int wide_vec) {
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
        w4 codes = requantise(s, kBias, 0, e2);
#pragma unroll
        for (int k = 0; k < 4; ++k) codes[k] = nan ? 0u : codes[k];
        const uint32_t word = header_word(nan ? kNaNScale : e2);
        if (live) st_tile<VEC>(static_cast<char*>(tiles), at, codes, word);
    }
}

// dst[i] = ldexp(dec(code i), scale - 127), i < n: a lane's 32 values as 16-B vectors where dst is 16-B aligned
// (wide_vec) and all 32 lie below n, one by one below n otherwise; a lane wholly beyond n touches nothing.
template <typename D, bool VEC>
__global__ __launch_bounds__(kWave) void k_mx4_dequantize(void* dst, const void* tiles, size_t n, int wide_vec) {
    const size_t ntiles = (n + kTileValues - 1) / kTileValues, trips = (ntiles + kTripTiles - 1) / kTripTiles;
    const char* const in = static_cast<const char*>(tiles);
    D* const out = static_cast<D*>(dst);
    for (size_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const Place at(trip);
        const size_t i0 = at.value0();
        if (i0 >= n) continue;
        const w4 codes = ld16<VEC>(in + at.codes());
        const int e = ld_scale(in + at.scale());
        const bool nan = e == kNaNScale;
        Wide32<D> r;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float v[8];
            dec8<true>(codes[k], e - kBias, v);
#pragma unroll
            for (int b = 0; b < 8; ++b) narrow(nan ? __builtin_nanf("") : v[b], r.e[8 * k + b]);
        }
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

}  // namespace chr_mx4

using namespace chr_mx4;

namespace {

std::atomic<long> g_fold_calls{0}, g_declined{0}, g_kernels{0};

unsigned grid_for(size_t tiles) {
    const size_t trips = (tiles + kTripTiles - 1) / kTripTiles;
    return (unsigned)(trips < kMaxGrid ? (trips ? trips : 1) : kMaxGrid);
}

}  // namespace

// The chr_user_reduce_fn the op is registered with.  Declines -- nonzero, nothing enqueued -- any dtype but a live tile
// type and any pointer that is not 4-B aligned.  Fan-in beyond kMaxIns runs as consecutive launches, each continuing
// from `out`.  running_first is not looked at: the rule commutes bit for bit.
extern "C" int chr_mx4_sum_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dt, int,
                                hipStream_t stream, void*) {
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
    const bool vec = (al & 15) == 0;
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
        if (vec) hipLaunchKernelGGL((k_mx4_fold<true>), dim3(grid), dim3(kWave), 0, stream, a);
        else hipLaunchKernelGGL((k_mx4_fold<false>), dim3(grid), dim3(kWave), 0, stream, a);
        if (hipGetLastError() != hipSuccess) return 1;
        ++g_kernels;
        done += a.m;
        cur = out;
    } while (done < m);
    return 0;
}

namespace {

std::mutex g_mu;
int g_op = -1;    // the live op; -1: not registered
int g_type = -1;  // the cached tile type

bool wide_ok(chr_dtype t) { return t == CHR_FLOAT32 || t == CHR_BFLOAT16; }

template <typename S>
int launch_quantize(void* tiles, const void* src, size_t n, hipStream_t s) {
    const unsigned grid = grid_for((n + CHR_MX4_TILE_VALUES - 1) / CHR_MX4_TILE_VALUES);
    const int wide_vec = (bits_of(src) & 15) == 0;
    if ((bits_of(tiles) & 15) == 0)
        hipLaunchKernelGGL((k_mx4_quantize<S, true>), dim3(grid), dim3(kWave), 0, s, tiles, src, n, wide_vec);
    else
        hipLaunchKernelGGL((k_mx4_quantize<S, false>), dim3(grid), dim3(kWave), 0, s, tiles, src, n, wide_vec);
    return hipGetLastError() == hipSuccess ? CHR_SUCCESS : CHR_ERR_HIP;
}

template <typename D>
int launch_dequantize(void* dst, const void* tiles, size_t n, hipStream_t s) {
    const unsigned grid = grid_for((n + CHR_MX4_TILE_VALUES - 1) / CHR_MX4_TILE_VALUES);
    const int wide_vec = (bits_of(dst) & 15) == 0;
    if ((bits_of(tiles) & 15) == 0)
        hipLaunchKernelGGL((k_mx4_dequantize<D, true>), dim3(grid), dim3(kWave), 0, s, dst, tiles, n, wide_vec);
    else
        hipLaunchKernelGGL((k_mx4_dequantize<D, false>), dim3(grid), dim3(kWave), 0, s, dst, tiles, n, wide_vec);
    return hipGetLastError() == hipSuccess ? CHR_SUCCESS : CHR_ERR_HIP;
}

// What both casts check before anything is enqueued; CHR_SUCCESS: launch.
int cast_args(const void* tiles, const void* wide, chr_dtype wide_type) {
    if (!tiles || !wide) return CHR_ERR_INVALID_ARG;
    if (!wide_ok(wide_type)) return CHR_ERR_UNSUPPORTED;
    if ((bits_of(tiles) & 3) || (bits_of(wide) & (wide_type == CHR_FLOAT32 ? 3 : 1))) return CHR_ERR_UNSUPPORTED;
    return CHR_SUCCESS;
}

}  // namespace

extern "C" {

int chr_mx4_type(chr_dtype* type) {
    if (!type) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_type < 0) {
        chr_dtype code;
        if (int rc = chr_type_contiguous(CHR_MX4_TILE_BYTES / 4, CHR_UINT32, &code)) return rc;
        g_type = (int)code;
    }
    *type = (chr_dtype)g_type;
    return CHR_SUCCESS;
}

int chr_mx4_sum(chr_op* op) {
    if (!op) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_op < 0) {
        chr_op code;
        if (int rc = chr_op_create(chr_mx4_sum_fold, nullptr, 1, &code)) return rc;
        g_op = (int)code;
    }
    *op = (chr_op)g_op;
    return CHR_SUCCESS;
}

int chr_mx4_quantize(void* tiles, const void* src, size_t n, chr_dtype src_type, hipStream_t s) {
    if (int rc = cast_args(tiles, src, src_type)) return rc;
    if (n == 0) return CHR_SUCCESS;
    return src_type == CHR_FLOAT32 ? launch_quantize<float>(tiles, src, n, s) : launch_quantize<bf16_bits>(tiles, src, n, s);
}

int chr_mx4_dequantize(void* dst, const void* tiles, size_t n, chr_dtype dst_type, hipStream_t s) {
    if (int rc = cast_args(tiles, dst, dst_type)) return rc;
    if (n == 0) return CHR_SUCCESS;
    return dst_type == CHR_FLOAT32 ? launch_dequantize<float>(dst, tiles, n, s) : launch_dequantize<bf16_bits>(dst, tiles, n, s);
}

int chr_mx4_release(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = CHR_SUCCESS;
    if (g_op >= 0) {
        rc = chr_op_free((chr_op)g_op);
        g_op = -1;
    }
    if (g_type >= 0) {
        const int e = chr_type_free((chr_dtype)g_type);
        if (!rc) rc = e;
        g_type = -1;
    }
    return rc;
}

void chr_mx4_stats(long out[3], int reset) {
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
