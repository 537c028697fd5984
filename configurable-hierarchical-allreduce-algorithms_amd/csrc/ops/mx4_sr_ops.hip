// mx4_sr_ops.hip -- libchiara_mx4_sr.so: the MXFP4 block-scaled SUM and quantize with stochastic rounding on the
// user-op interface (include/chiara_mx4_sr.h has the contract: the rule's last step enc_sr, the random halves, and why
// they are a pure function of the seed, the place in the tile and the operands' bits).  The tile, its loads and
// stores, the decode and the header assembly are csrc/ops/mx4_tile.hpp's, unedited; the type is chr_mx4_type's.
// Built with the package's HIPFLAGS and MXFLAGS like libchiara_mx4.so.
//
// How the work is split.  As in mx4_ops.hip: one-wave workgroups, a lane owns a whole block (one 16-B access), the 16
// lanes of a DPP row are a tile, a wave trip covers four tiles, the header words are assembled by two DPP row shifts.
// That split is what makes the random source cheap: the block's amax, its new scale e' and the block key
// kb = mix32(ks ^ (blk | e' << 8)) are lane-private and computed once per block, with no exchange and no LDS.
// ks = mix32(seed ^ T) is wave-uniform in the fold (T = 0: computed once per kernel, on the scalar unit) and one hash
// per lane and trip in the quantize (T = the tile's index).  The seed is a kernel argument.
//
// One hash per pair.  The 32 sums of a block stay in registers as f32 from decode to encode, as in k_mx4_fold.  Two
// neighbouring values, the two nibbles of a code byte, are renormalised and clamped together, hashed once
// (v_alignbit_b32 for the rotate, two v_xor, and lowbias32: two v_mul_lo_u32 and three shift-xor pairs), and the
// hash's halves are their u.  v_mul_lo_u32 is a quarter-rate instruction, hence a pair and not a value per hash.
//
// Encode: VALU, not v_cvt_scalef32_sr_pk_fp4_f32.  The rule is P(up) = floor(f * 2^16) / 2^16 with an exact value
// never moved; how the hardware convert aligns its random operand against the discarded bits -- in particular below
// 1.0, where the grid's step is 0.5 and not a mantissa bit -- is not something this library could pin on the whole
// operand domain without shipping both paths, so the rule is written out in integer arithmetic, which leaves nothing
// to pin.  With a = bits(|t|):
//   |t| >= 1: the grid keeps one mantissa bit, so ((a >> 6) + u) >> 16 is the rounded pattern >> 22 -- the carry walks
//             into the exponent at 1.5 -> 2, 3 -> 4 and (4, 6) -> 6 -- and the code is that minus 0xFC (1.0 is
//             0x3F800000 >> 22 = 0xFE, code 2);
//   |t| <  1: the step is 0.5, and X = trunc(|t| * 2^17) (exact: a power of two, v_cvt_u32_f32 truncates) is
//             q * 2^16 + floor(f * 2^16) with q = (|t| >= 0.5), so (X + u) >> 16 is the code 0, 1 or 2 itself.
// Then the sign bit is ORed in as bit 3.  Per value that is 2 shifts, an add and a subtract, or a multiply, a convert,
// an add and a shift, the compare and select between them, and the sign; per pair the hash above and the packing.
// tests/test_gpu_mx4_sr.py holds it to tests/mx4_sr_ref.py bit for bit on all 256 code pairs under every scale gap.
//
// Resources (tests/test_mx4_sr_resources.py): at most 72 allocated VGPRs, no scratch, no static LDS.
//
// Measured (tools/userop_bench.py --mx4, the sr_ rows: folds in place at 127 100 tiles per operand over an HBM-cold
// rotation, alternating with libchiara_mx4.so's RNE fold in one process, the command run twice: the range over the
// four rounds of both runs; profiles/r20/mx4_sr/userop_bench.json and userop_bench_run2.json):
//                                      MX4 SUM (RNE)    MX4 SR SUM       SR / RNE
//   fold m = 1, GB/s                   4568 - 4597      2022 - 2044      0.440 - 0.446
//   fold m = 3, GB/s                   3220 - 3277      1221 - 1229      0.373 - 0.379
//   quantize from f32, GB/s            2371 - 2380      2360 - 2370      0.993 - 0.999
// GB/s is of the (m + 2) x bytes traffic, for the quantize of the 4 bytes read and 17 / 32 written per value.  The
// fold was ALU-bound before and pays for the hash and the integer encode in full; the quantize is held by its f32
// reads and hides nearly all of it.  No ratio was a target: the rows are on record for whoever chooses between the ops
// and for a later SR tree kernel.
#include <atomic>
#include <mutex>

#include <hip/hip_runtime.h>

#include "chiara_mx4_sr.h"
#include "mx4_tile.hpp"  // the tile on the device: Place, ld16 / st_tile, dec8, header_word, the constants

namespace chr_mx4_sr {

using namespace chr_mx4;

constexpr int kMaxIns = 16;          // operands per launch; a wider fan-in continues from `out`
constexpr unsigned kMaxGrid = 4096;  // one-wave workgroups a launch strides over
constexpr uint32_t kGolden = 0x9E3779B9u;
using bf16_bits = uint16_t;

__device__ __forceinline__ uint32_t mix32(uint32_t x) {  // lowbias32
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint32_t bits(float t) { return __builtin_bit_cast(uint32_t, t); }

// enc_sr(t, u) for |t| <= 6 and u < 2^16: the E2M1 code, sign in bit 3 (the file's header comment derives both arms).
__device__ __forceinline__ uint32_t enc_sr(float t, uint32_t u) {
    const uint32_t b = bits(t), a = b & 0x7FFFFFFFu;
    const uint32_t big = (((a >> 6) + u) >> 16) - 0xFCu;
    const uint32_t small = ((uint32_t)(__builtin_fabsf(t) * 131072.0f) + u) >> 16;
    return (a >= 0x3F800000u ? big : small) | ((b >> 28) & 8u);
}

// Steps 4 - 7 of the rule on a lane's block, the last one enc_sr: s holds the 32 finite sums relative to scale e, ks
// is mix32(seed ^ T) and blk the block's index in its tile.  The scale choice is mx4_tile.hpp's requantise's, word
// for word; e_zero is the scale of an all-zero block (e for SUM, 0 for quantize).
__device__ __forceinline__ w4 requantise_sr(const float (&s)[kBlockValues], int e, int e_zero, uint32_t ks, unsigned blk,
                                            int& e_out) {
    float am = 0.0f;
#pragma unroll
    for (int i = 0; i < kBlockValues; ++i) am = __builtin_fmaxf(am, __builtin_fabsf(s[i]));
    const int E = __builtin_amdgcn_frexp_expf(am) - kMaxExp + (__builtin_amdgcn_frexp_mantf(am) > 0.75f ? 1 : 0);
    int e2 = e + E;
    e2 = e2 < 0 ? 0 : e2 > kMaxScale ? kMaxScale : e2;
    e2 = am == 0.0f ? e_zero : e2;
    const int shift = e - e2;
    const uint32_t kb = mix32(ks ^ (blk | (uint32_t)e2 << 8));
    w4 codes;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t w = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {  // pair j = 4 k + p: code byte p of word k
            const int j = 4 * k + p;
            const float t0 = __builtin_amdgcn_fmed3f(__builtin_ldexpf(s[2 * j], shift), -kMax, kMax);
            const float t1 = __builtin_amdgcn_fmed3f(__builtin_ldexpf(s[2 * j + 1], shift), -kMax, kMax);
            const uint32_t h = mix32(bits(t0) ^ __builtin_rotateleft32(bits(t1), 16) ^ (kb + (uint32_t)(j + 1) * kGolden));
            w |= (enc_sr(t0, h & 0xFFFFu) | enc_sr(t1, h >> 16) << 4) << (8 * p);
        }
        codes[k] = w;
    }
    e_out = e2;
    return codes;
}

// (r, er) = (x, ex) o (r, er) on a lane's block under the SR rule -- and equally (r, er) o (x, ex): f32 addition
// commutes bit for bit, and the random halves are a function of the sums.  Steps 1 - 3 are mx4_tile.hpp's combine's.
__device__ __forceinline__ void combine_sr(w4& r, int& er, const w4& x, int ex, uint32_t ks, unsigned blk) {
    const bool nan = er == kNaNScale || ex == kNaNScale;
    const bool r_low = er < ex;
    const int e = r_low ? ex : er, d = (r_low ? er : ex) - e;  // d <= 0: the shift of the smaller scale's operand
    float s[kBlockValues];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float lo[8], hi[8];
        dec8<true>(r_low ? r[k] : x[k], d, lo);
        dec8<false>(r_low ? x[k] : r[k], 0, hi);
#pragma unroll
        for (int i = 0; i < 8; ++i) s[8 * k + i] = hi[i] + lo[i];
    }
    int e2;
    const w4 codes = requantise_sr(s, e, e, ks, blk, e2);
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = nan ? 0u : codes[k];  // the canonical NaN block: sixteen 0x00 code bytes
    er = nan ? kNaNScale : e2;
}

struct FoldArgs {
    void* out;
    const void* acc;
    const void* ins[kMaxIns];
    int m;
    uint32_t seed;
    size_t n;  // tiles
};

// out = ins[m-1] o (... (ins[0] o acc)) on n tiles under the SR rule, one HBM pass, every intermediate block rounded
// in registers as the fold-by-fold result is.  A tile is read and written by one row of a wave, all its loads before
// its stores: `out` may alias `acc`.  m == 0 copies.  The lanes of a trip's missing tiles carry zeros through the
// same instructions (the row shifts stay wave-wide) and neither load nor store.
template <bool VEC>
__global__ __launch_bounds__(kWave) void k_mx4_sr_fold(FoldArgs a) {
    const size_t trips = (a.n + kTripTiles - 1) / kTripTiles;
    const char* const acc = static_cast<const char*>(a.acc);
    char* const out = static_cast<char*>(a.out);
    const uint32_t ks = mix32(a.seed);  // T = 0: wave-uniform, once per kernel
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
            combine_sr(r, er, x, ex, ks, at.b);
        }
        const uint32_t word = header_word(er);
        if (live) st_tile<VEC>(out, at, r, word);
    }
}

__device__ __forceinline__ float widen(float x) { return x; }
__device__ __forceinline__ float widen(bf16_bits x) { return __builtin_bit_cast(float, (uint32_t)x << 16); }

template <typename W> struct Wide32 { W e[kBlockValues]; };
template <typename W> struct WideWords { w4 w[2 * sizeof(W)]; };  // 32 W: 2 * sizeof(W) vectors of 16 bytes

// tiles = Q_sr(src): k_mx4_quantize's reads (a lane's 32 source values as 16-B vectors where src is 16-B aligned and
// all 32 lie below n, one by one and +0 beyond n otherwise) and NaN blocks, with enc_sr keyed on the tile's index.
template <typename S, bool VEC>
__global__ __launch_bounds__(kWave) void k_mx4_sr_quantize(void* tiles, const void* src, size_t n, int wide_vec, uint32_t seed) {
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
        w4 codes = requantise_sr(s, kBias, 0, mix32(seed ^ (uint32_t)at.tile), at.b, e2);
#pragma unroll
        for (int k = 0; k < 4; ++k) codes[k] = nan ? 0u : codes[k];
        const uint32_t word = header_word(nan ? kNaNScale : e2);
        if (live) st_tile<VEC>(static_cast<char*>(tiles), at, codes, word);
    }
}

}  // namespace chr_mx4_sr

using namespace chr_mx4_sr;

namespace {

std::atomic<long> g_fold_calls{0}, g_declined{0}, g_kernels{0};
std::atomic<uint32_t> g_seed{0};

unsigned grid_for(size_t tiles) {
    const size_t trips = (tiles + kTripTiles - 1) / kTripTiles;
    return (unsigned)(trips < kMaxGrid ? (trips ? trips : 1) : kMaxGrid);
}

}  // namespace

// The chr_user_reduce_fn the op is registered with.  Declines -- nonzero, nothing enqueued -- any dtype but a live tile
// type and any pointer that is not 4-B aligned.  The seed is read once: every launch of a fan-in beyond kMaxIns, each
// continuing from `out`, rounds under it.  running_first is not looked at: the rule commutes bit for bit.
extern "C" int chr_mx4_sr_sum_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dt, int,
                                   hipStream_t stream, void*) {
    ++g_fold_calls;
    const uint32_t seed = g_seed.load();
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
        a.seed = seed;
        a.n = n;
        if (vec) hipLaunchKernelGGL((k_mx4_sr_fold<true>), dim3(grid), dim3(kWave), 0, stream, a);
        else hipLaunchKernelGGL((k_mx4_sr_fold<false>), dim3(grid), dim3(kWave), 0, stream, a);
        if (hipGetLastError() != hipSuccess) return 1;
        ++g_kernels;
        done += a.m;
        cur = out;
    } while (done < m);
    return 0;
}

namespace {

std::mutex g_mu;
int g_op = -1;  // the live op; -1: not registered

template <typename S>
int launch_quantize(void* tiles, const void* src, size_t n, uint32_t seed, hipStream_t s) {
    const unsigned grid = grid_for((n + CHR_MX4_TILE_VALUES - 1) / CHR_MX4_TILE_VALUES);
    const int wide_vec = (bits_of(src) & 15) == 0;
    if ((bits_of(tiles) & 15) == 0)
        hipLaunchKernelGGL((k_mx4_sr_quantize<S, true>), dim3(grid), dim3(kWave), 0, s, tiles, src, n, wide_vec, seed);
    else
        hipLaunchKernelGGL((k_mx4_sr_quantize<S, false>), dim3(grid), dim3(kWave), 0, s, tiles, src, n, wide_vec, seed);
    return hipGetLastError() == hipSuccess ? CHR_SUCCESS : CHR_ERR_HIP;
}

}  // namespace

extern "C" {

int chr_mx4_sr_sum(chr_op* op) {
    if (!op) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_op < 0) {
        chr_op code;
        if (int rc = chr_op_create(chr_mx4_sr_sum_fold, nullptr, 1, &code)) return rc;
        g_op = (int)code;
    }
    *op = (chr_op)g_op;
    return CHR_SUCCESS;
}

void chr_mx4_sr_set_seed(uint32_t seed) { g_seed.store(seed); }

int chr_mx4_sr_quantize(void* tiles, const void* src, size_t n, chr_dtype src_type, uint32_t seed, hipStream_t s) {
    if (!tiles || !src) return CHR_ERR_INVALID_ARG;
    if (src_type != CHR_FLOAT32 && src_type != CHR_BFLOAT16) return CHR_ERR_UNSUPPORTED;
    if ((bits_of(tiles) & 3) || (bits_of(src) & (src_type == CHR_FLOAT32 ? 3 : 1))) return CHR_ERR_UNSUPPORTED;
    if (n == 0) return CHR_SUCCESS;
    return src_type == CHR_FLOAT32 ? launch_quantize<float>(tiles, src, n, seed, s)
                                   : launch_quantize<bf16_bits>(tiles, src, n, seed, s);
}

int chr_mx4_sr_release(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = CHR_SUCCESS;
    if (g_op >= 0) {
        rc = chr_op_free((chr_op)g_op);
        g_op = -1;
    }
    return rc;
}

void chr_mx4_sr_stats(long out[3], int reset) {
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
