// mxint8_ops.hip -- libchiara_mxint8.so: the MXINT8 block-scaled SUM on the user-op interface, and the casts into and
// out of the tile (include/chiara_mxint8.h has the contract: the 528-byte tile, the SUM rule, the error codes).  The
// tile is MXFP8's and the rule is the family's; the kernels are not k_mx_fold with another table, because on int8
// codes the whole combine is exact in integers whenever the two block scales are close, and gfx950's packed 16-bit
// VALU then does two values per instruction.  Built with the package's HIPFLAGS (-fno-fast-math, -ffp-contract=off)
// and with packed f32 arithmetic disabled for this code object, as every MX library is.
//
// How the work is split.  One-wave workgroups.  A lane owns 16 consecutive codes, one 16-B access, the widest there
// is; lanes 2j and 2j + 1 of a half-wave form block j, so a half-wave is a tile and a wave trip covers two tiles,
// 1 056 consecutive bytes.  A lane per block would need two accesses per operand and twice the registers per lane for
// nothing: the only thing the pair exchanges is the block's amax, one DPP quad_perm:[1,0,3,2] and a max.  Each lane
// loads its block's scale as a byte of the tile's header.  A tile's 16 new scale bytes become four header words by
// two DPP row shifts (row_shl:2, row_shl:4), after which lanes 0, 8, 16 and 24 of the half-wave store one word each.
// No LDS.  The grid is capped at kMaxGrid workgroups and a launch takes 16 operands; a wider fan-in continues from
// `out`.  Loads and stores are non-temporal.
//
// The integer combine (mxint8_tile.hpp combine_i16).  For a gap d = |ex - ey| <= 7 every sum of step 3 is an integer
// of at most 128 * 128 + 128 < 2^15 units of the smaller scale: exact in f32, so integer arithmetic gives the rule's
// bits.  A code word's four bytes are unpacked into two registers of two 16-bit values (v_pk_lshlrev_b16 and
// v_pk_ashrrev_i16; the a << d is folded into the right shift), added (v_pk_add_u16), reduced to an amax
// (v_pk_max_i16, v_pk_min_i16), renormalised by a round-half-even arithmetic shift or an exact left shift, and
// repacked by mask, shift and or.  The new scale comes from a leading-zero count.  With the smaller scale in 6 .. 246
// step 6 cannot clamp and nothing saturates.  Every other case -- larger gaps, where the f32 sum may round and the
// rule's two roundings are observable; scales at which step 6 may clamp; the NaN scale -- takes combine_f32, the rule
// as written.  A middle tier on 32-bit integers (d <= 16 is still exact) is not built: one value per instruction is
// what combine_f32 issues too.  The choice is wave-uniform, by one ballot: a wave of close scales never executes the
// f32 path, and any other wave takes it for all its blocks.
//
// Registers: 48 VGPRs for the folds, 35 - 39 for the casts, no scratch, no LDS (tests/test_mxint8_resources.py).
//
// Per lane and combine of 16 values the ISA holds, on the integer path, 24 v_pk_ashrrev_i16, 24 v_pk_add_u16, 16
// v_pk_lshlrev_b16, 8 v_pk_lshrrev_b16, 7 v_pk_max_i16, 7 v_pk_min_i16, about 20 v_and_b32 and 8 v_perm_b32 /
// v_lshl_or_b32, some 115 VALU instructions; on the f32 path 48 v_ldexp_f32, 32 v_cvt_f32_i32 (SDWA byte selects), 16
// v_add_f32, 16 v_rndne_f32, 16 v_med3_f32, 16 v_cvt_i32_f32 and 8 v_max3_f32, some 170 with the packing.
//
// Measured (tools/userop_bench.py --mxint8 --mxint8-f32 build/libchiara_mxint8_f32.so: folds in place at 127 100 tiles
// = 67.1 MB per operand, each variant over an HBM-cold rotation of its own, the three variants alternating within each
// round of one process, the command run twice: the range over the four rounds; profiles/r17/mxint8/userop_bench.json
// and userop_bench_run2.json).  `close` is tiles quantized from normals of one variance, `wild` random codes under
// mixed scales with clamps and NaN blocks; the f32-only build is the A/B object (make mxint8_ab); GB/s is of the
// (m + 2) x bytes traffic, and the ratio is also that of values per second, the tiles being the same size:
//                              MX E4M3 SUM    MXINT8 SUM     MXINT8 f32-only   MXINT8 / MX E4M3   f32-only / MX E4M3
//   close, fold m = 1, GB/s    4447 - 4457    4649 - 4669    4549 - 4564       1.04 - 1.05        1.02 - 1.03
//   close, fold m = 3, GB/s    3364 - 3373    4294 - 4334    3707 - 3740       1.28 - 1.29        1.10 - 1.11
//   wild,  fold m = 1, GB/s    4422 - 4466    4493 - 4548    4528 - 4564       1.01 - 1.02        1.02 - 1.03
//   wild,  fold m = 3, GB/s    3341 - 3362    3652 - 3673    3733 - 3749       1.09               1.11 - 1.12
// The expectation was at least the MXFP8 E4M3 fold's values per second at m = 3 on close scales: it holds, 1.28 - 1.29.
// The integer combine earns its place there, 1.16 of the f32-only build; on wild data, where nearly every wave holds
// a block that needs the f32 path, the ballot and the branch cost 2 % against the f32-only build.
#include <atomic>
#include <mutex>

#include <hip/hip_runtime.h>

#include "mxint8_tile.hpp"  // the tile and the rule on the device: Place .. combine

namespace chr_mxi8 {

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

// out = ins[m-1] o (... (ins[0] o acc)) on n tiles, one HBM pass.  A tile is read and written by one half-wave, all
// its loads before its stores: `out` may alias `acc`.  m == 0 copies.  The lanes of a trip's missing second tile
// carry zeros under scale 127 through the same instructions (the exchanges between lanes stay wave-wide, and they do
// not push the wave onto the f32 path) and neither load nor store.
template <bool VEC>
__global__ __launch_bounds__(kWave) void k_mxi8_fold(FoldArgs a) {
    const size_t trips = (a.n + 1) / 2;
    const char* const acc = static_cast<const char*>(a.acc);
    char* const out = static_cast<char*>(a.out);
    for (size_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const Place at(trip);
        const bool live = at.tile < a.n;
        w4 r = {0u, 0u, 0u, 0u};
        int er = kBias;
        if (live) {
            r = ld16<VEC>(acc + at.codes());
            er = ld_scale(acc + at.scale());
        }
        for (int j = 0; j < a.m; ++j) {
            const char* const in = static_cast<const char*>(a.ins[j]);
            w4 x = {0u, 0u, 0u, 0u};
            int ex = kBias;
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

template <typename W> struct Wide16 { W e[kLaneValues]; };
template <typename W> struct WideWords { w4 w[sizeof(W)]; };  // 16 W: sizeof(W) vectors of 16 bytes

// tiles = Q(src): the same lane-pair layout, a lane reading its 16 source values (64 B of f32, 32 B of bf16) as 16-B
// vectors where src is 16-B aligned (wide_vec) and all 16 lie below n, one by one and +0 beyond n otherwise.  A
// non-finite value in either lane of a block makes it the canonical NaN block; its own bits take no part in the
// arithmetic.
template <typename S, bool VEC>
__global__ __launch_bounds__(kWave) void k_mxi8_quantize(void* tiles, const void* src, size_t n, int wide_vec) {
    const size_t ntiles = (n + kTileValues - 1) / kTileValues, trips = (ntiles + 1) / 2;
    const S* const in = static_cast<const S*>(src);
    for (size_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const Place at(trip);
        const bool live = at.tile < ntiles;
        const size_t i0 = at.value0();
        float s[kLaneValues];
        if (live && wide_vec && i0 + kLaneValues <= n) {
            WideWords<S> w;
#pragma unroll
            for (int k = 0; k < (int)sizeof(S); ++k)
                w.w[k] = __builtin_nontemporal_load(reinterpret_cast<const w4*>(in + i0) + k);
            const Wide16<S> x = __builtin_bit_cast(Wide16<S>, w);
#pragma unroll
            for (int i = 0; i < kLaneValues; ++i) s[i] = widen(x.e[i]);
        } else {
#pragma unroll
            for (int i = 0; i < kLaneValues; ++i) s[i] = live && i0 + i < n ? widen(in[i0 + i]) : 0.0f;
        }
        int bad = 0;
#pragma unroll
        for (int i = 0; i < kLaneValues; ++i) {
            const bool fin = __builtin_fabsf(s[i]) < __builtin_inff();
            bad |= fin ? 0 : 1;
            s[i] = fin ? s[i] : 0.0f;
        }
        const bool nan = (bad | of_partner(bad)) != 0;
        int e2;
        w4 codes = requantise(s, kBias, 0, e2);
#pragma unroll
        for (int k = 0; k < 4; ++k) codes[k] = nan ? 0u : codes[k];
        const uint32_t word = header_word(nan ? kNaNScale : e2);
        if (live) st_tile<VEC>(static_cast<char*>(tiles), at, codes, word);
    }
}

// dst[i] = ldexp(dec(code i), scale - 127), i < n, as one v_ldexp_f32 of the code's integer by scale - 133 (one
// rounding, the rule's): a lane's 16 values as 16-B vectors where dst is 16-B aligned (wide_vec) and all 16 lie below
// n, one by one below n otherwise; a lane wholly beyond n touches nothing.
template <typename D, bool VEC>
__global__ __launch_bounds__(kWave) void k_mxi8_dequantize(void* dst, const void* tiles, size_t n, int wide_vec) {
    const size_t ntiles = (n + kTileValues - 1) / kTileValues, trips = (ntiles + 1) / 2;
    const char* const in = static_cast<const char*>(tiles);
    D* const out = static_cast<D*>(dst);
    for (size_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const Place at(trip);
        const size_t i0 = at.value0();
        if (i0 >= n) continue;
        const w4 codes = ld16<VEC>(in + at.codes());
        const int e = ld_scale(in + at.scale());
        const int shift = e - kBias - kFrac;
        const bool nan = e == kNaNScale;
        Wide16<D> r;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                narrow(nan ? __builtin_nanf("") : __builtin_ldexpf(code_f32(codes[k], b), shift), r.e[4 * k + b]);
        }
        if (wide_vec && i0 + kLaneValues <= n) {
            const WideWords<D> w = __builtin_bit_cast(WideWords<D>, r);
#pragma unroll
            for (int k = 0; k < (int)sizeof(D); ++k)
                __builtin_nontemporal_store(w.w[k], reinterpret_cast<w4*>(out + i0) + k);
        } else {
#pragma unroll
            for (int i = 0; i < kLaneValues; ++i)
                if (i0 + i < n) out[i0 + i] = r.e[i];
        }
    }
}

}  // namespace chr_mxi8

using namespace chr_mxi8;

namespace {

std::atomic<long> g_fold_calls{0}, g_declined{0}, g_kernels{0};

unsigned grid_for(size_t tiles) {
    const size_t trips = (tiles + 1) / 2;
    return (unsigned)(trips < kMaxGrid ? (trips ? trips : 1) : kMaxGrid);
}

}  // namespace

// The chr_user_reduce_fn the op is registered with.  Declines -- nonzero, nothing enqueued -- any dtype but a live tile
// type and any pointer that is not 4-B aligned.  Fan-in beyond kMaxIns runs as consecutive launches, each continuing
// from `out`.  running_first is not looked at: the rule commutes bit for bit.
extern "C" int chr_mxi8_sum_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dt, int,
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
        if (vec) hipLaunchKernelGGL((k_mxi8_fold<true>), dim3(grid), dim3(kWave), 0, stream, a);
        else hipLaunchKernelGGL((k_mxi8_fold<false>), dim3(grid), dim3(kWave), 0, stream, a);
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
    const unsigned grid = grid_for((n + CHR_MXI8_TILE_VALUES - 1) / CHR_MXI8_TILE_VALUES);
    const int wide_vec = (bits_of(src) & 15) == 0;
    if ((bits_of(tiles) & 15) == 0)
        hipLaunchKernelGGL((k_mxi8_quantize<S, true>), dim3(grid), dim3(kWave), 0, s, tiles, src, n, wide_vec);
    else
        hipLaunchKernelGGL((k_mxi8_quantize<S, false>), dim3(grid), dim3(kWave), 0, s, tiles, src, n, wide_vec);
    return hipGetLastError() == hipSuccess ? CHR_SUCCESS : CHR_ERR_HIP;
}

template <typename D>
int launch_dequantize(void* dst, const void* tiles, size_t n, hipStream_t s) {
    const unsigned grid = grid_for((n + CHR_MXI8_TILE_VALUES - 1) / CHR_MXI8_TILE_VALUES);
    const int wide_vec = (bits_of(dst) & 15) == 0;
    if ((bits_of(tiles) & 15) == 0)
        hipLaunchKernelGGL((k_mxi8_dequantize<D, true>), dim3(grid), dim3(kWave), 0, s, dst, tiles, n, wide_vec);
    else
        hipLaunchKernelGGL((k_mxi8_dequantize<D, false>), dim3(grid), dim3(kWave), 0, s, dst, tiles, n, wide_vec);
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

int chr_mxi8_type(chr_dtype* type) {
    if (!type) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_type < 0) {
        chr_dtype code;
        if (int rc = chr_type_contiguous(CHR_MXI8_TILE_BYTES / 4, CHR_UINT32, &code)) return rc;
        g_type = (int)code;
    }
    *type = (chr_dtype)g_type;
    return CHR_SUCCESS;
}

int chr_mxi8_sum(chr_op* op) {
    if (!op) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_op < 0) {
        chr_op code;
        if (int rc = chr_op_create(chr_mxi8_sum_fold, nullptr, 1, &code)) return rc;
        g_op = (int)code;
    }
    *op = (chr_op)g_op;
    return CHR_SUCCESS;
}

int chr_mxi8_quantize(void* tiles, const void* src, size_t n, chr_dtype src_type, hipStream_t s) {
    if (int rc = cast_args(tiles, src, src_type)) return rc;
    if (n == 0) return CHR_SUCCESS;
    return src_type == CHR_FLOAT32 ? launch_quantize<float>(tiles, src, n, s) : launch_quantize<bf16_bits>(tiles, src, n, s);
}

int chr_mxi8_dequantize(void* dst, const void* tiles, size_t n, chr_dtype dst_type, hipStream_t s) {
    if (int rc = cast_args(tiles, dst, dst_type)) return rc;
    if (n == 0) return CHR_SUCCESS;
    return dst_type == CHR_FLOAT32 ? launch_dequantize<float>(dst, tiles, n, s) : launch_dequantize<bf16_bits>(dst, tiles, n, s);
}

int chr_mxi8_release(void) {
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

void chr_mxi8_stats(long out[3], int reset) {
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
