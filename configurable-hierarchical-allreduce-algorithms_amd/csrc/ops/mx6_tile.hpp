// mx6_tile.hpp -- the MX6 tile and the SUM rule on the device (include/chiara_mx6.h has the contract), the text of
// csrc/ops/mx6_ops.hip (libchiara_mx6.so: the folds and the casts) and of any later kernel that combines MX6 tiles.
// Built with the package's HIPFLAGS and with packed f32 arithmetic disabled (the Makefile's MXFLAGS), so that the 32
// sums of a lane stay 32 v_add_f32; mx6_ops.hip's header comment says how the work is split over lanes, how a block's
// 24 bytes move and how a combine stays inside the register budget.
#pragma once

#include <hip/hip_runtime.h>

#include "chiara_mx6.h"

namespace chr_mx6 {  // named: the resource test reads the kernels' symbols

constexpr int kTileBytes = CHR_MX6_TILE_BYTES, kTileValues = CHR_MX6_TILE_VALUES;
constexpr int kHeader = 16;       // the scale bytes in front of a tile's codes
constexpr int kBlockValues = 32;  // codes per lane: a whole block, what one convert decodes or encodes
constexpr int kBlockBytes = 24;   // 192 bits: six words, three 8-B accesses
constexpr int kBlockWords = kBlockBytes / 4;
constexpr int kRow = 16;          // lanes per tile: one DPP row
constexpr int kWave = 64;         // one-wave workgroups
constexpr int kTripTiles = kWave / kRow;  // four tiles, 1 600 consecutive bytes, per wave trip
constexpr int kNaNScale = 0xFF, kBias = 127, kMaxScale = 254;

static_assert(kTileBytes == kHeader + kRow * kBlockBytes && kTileValues == kRow * kBlockValues, "a DPP row is a tile");

// What the format forces: max = kThreshold * 2^kMaxExp, the largest magnitude of a code.
template <int F> struct Format;
template <> struct Format<CHR_MX6_E2M3> {
    static constexpr float kMax = 7.5f, kThreshold = 0.9375f;
    static constexpr int kMaxExp = 3;
};
template <> struct Format<CHR_MX6_E3M2> {
    static constexpr float kMax = 28.0f, kThreshold = 0.875f;
    static constexpr int kMaxExp = 5;
};

typedef unsigned int w2 __attribute__((ext_vector_type(2)));
typedef unsigned int w4 __attribute__((ext_vector_type(4)));
typedef unsigned int w6 __attribute__((ext_vector_type(6)));    // a block's codes: code i in bits 6 i .. 6 i + 5
typedef unsigned int w16 __attribute__((ext_vector_type(16)));  // a block decoded to bf16, value 2 k in word k's low half
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x32 __attribute__((ext_vector_type(32)));

inline uintptr_t bits_of(const void* p) { return (uintptr_t)p; }

// The content of a call's dtype, read at run time: a derived code means nothing at compile time.
inline bool is_tile_type(chr_dtype dt) {
    chr_dtype base;
    int count = 0;
    return chr_type_get_contiguous(dt, &base, &count) == CHR_SUCCESS && base == CHR_UINT32 &&
           count == CHR_MX6_TILE_BYTES / 4;
}

// v_cvt_scalef32_pk32_f32_{fp6,bf6} at scale 1.0: six VGPRs of codes to 32 f32, value i from bits 6 i .. 6 i + 5, the
// tile's own order.  Exact on all 64 codes, -0 included.
template <int F>
__device__ __forceinline__ f32x32 dec32(w6 w) {
    if constexpr (F == CHR_MX6_E2M3) return __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(w, 1.0f);
    else return __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(w, 1.0f);
}
// v_cvt_scalef32_pk32_bf16_{fp6,bf6} at scale 1.0: the same 32 values in 16 VGPRs.  Every E2M3 and E3M2 value has at
// most four significant bits and an exponent in -4 .. 4: exact in bf16.
template <int F>
__device__ __forceinline__ w16 dec32_bf16(w6 w) {
    if constexpr (F == CHR_MX6_E2M3) return __builtin_bit_cast(w16, __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(w, 1.0f));
    else return __builtin_bit_cast(w16, __builtin_amdgcn_cvt_scalef32_pk32_bf16_bf6(w, 1.0f));
}
// Value i of a block decoded to bf16, widened: its 16 bits are the upper half of the f32.
__device__ __forceinline__ float bf16_at(const w16& h, int i) {
    return __builtin_bit_cast(float, (i & 1) ? h[i >> 1] & 0xFFFF0000u : h[i >> 1] << 16);
}
// v_cvt_scalef32_2xpk16_{fp6,bf6}_f32 at scale 1.0: the instruction takes two 16-vectors and interleaves them, code
// 2 k from its first operand's element k and code 2 k + 1 from its second's, so the even values of a block go in as
// one operand and the odd ones as the other and the tile's order holds.  c is already clamped to +-max.
template <int F>
__device__ __forceinline__ w6 enc32(const float (&c)[kBlockValues]) {
    f32x16 even, odd;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        even[k] = c[2 * k];
        odd[k] = c[2 * k + 1];
    }
    if constexpr (F == CHR_MX6_E2M3) return __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(even, odd, 1.0f);
    else return __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(even, odd, 1.0f);
}

// A block's 24 bytes at p: three 8-B accesses where every pointer of the call is 8-B aligned (16 + 24 b keeps that
// alignment, and no more for odd b), six words otherwise.  gfx950 needs only word alignment for a multi-word global
// access, and the backend merges adjacent ones: both forms reach the ISA as one 16-B and one 8-B access.
template <bool VEC>
__device__ __forceinline__ w6 ld24(const char* p) {
    w6 r;
    if constexpr (VEC) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const w2 v = __builtin_nontemporal_load(reinterpret_cast<const w2*>(p) + k);
            r[2 * k] = v[0];
            r[2 * k + 1] = v[1];
        }
    } else {
#pragma unroll
        for (int k = 0; k < kBlockWords; ++k) r[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p) + k);
    }
    return r;
}
template <bool VEC>
__device__ __forceinline__ void st24(char* p, w6 v) {
    if constexpr (VEC) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const w2 t = {v[2 * k], v[2 * k + 1]};
            __builtin_nontemporal_store(t, reinterpret_cast<w2*>(p) + k);
        }
    } else {
#pragma unroll
        for (int k = 0; k < kBlockWords; ++k) __builtin_nontemporal_store(v[k], reinterpret_cast<uint32_t*>(p) + k);
    }
}
__device__ __forceinline__ int ld_scale(const char* p) {
    return (int)__builtin_nontemporal_load(reinterpret_cast<const uint8_t*>(p));
}

// Where a lane stands in a trip: tile 4 * trip + row, block b of that tile -- its 24 code bytes and its scale byte.
struct Place {
    size_t tile;
    unsigned b;  // lane of the row: the block
    __device__ __forceinline__ Place(size_t trip) : tile(kTripTiles * trip + (threadIdx.x >> 4)), b(threadIdx.x & 15u) {}
    __device__ __forceinline__ size_t codes() const { return tile * kTileBytes + kHeader + (size_t)kBlockBytes * b; }
    __device__ __forceinline__ size_t scale() const { return tile * kTileBytes + b; }
    __device__ __forceinline__ size_t value0() const { return tile * kTileValues + (size_t)kBlockValues * b; }
};

// Lane b of a row holds block b's scale: word w of the tile's header, the bytes of blocks 4w .. 4w + 3, assembled in
// lane 4w with two DPP row shifts (row_shl:n hands lane i the value of lane i + n of its row; a lane that would read
// past the row's end gets 0, and lanes 0, 4, 8, 12 never do).  Every lane computes a word; those four hold the header.
__device__ __forceinline__ uint32_t header_word(int scale) {
    const uint32_t s = (uint32_t)scale;
    const uint32_t two = s | ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x101 /* row_shl:1 */, 0xF, 0xF, true) << 8);
    return two | ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)two, 0x102 /* row_shl:2 */, 0xF, 0xF, true) << 16);
}
template <bool VEC>
__device__ __forceinline__ void st_tile(char* out, const Place& at, w6 codes, uint32_t word) {
    st24<VEC>(out + at.codes(), codes);
    if ((at.b & 3u) == 0)  // lane 4w: header bytes 4w .. 4w + 3
        __builtin_nontemporal_store(word, reinterpret_cast<uint32_t*>(out + at.tile * kTileBytes + at.b));
}

// Steps 4 - 7 of the rule on a lane's block: s holds the 32 finite sums relative to scale e.  Returns the codes and the
// new scale; e_zero is the scale of an all-zero block (e for SUM, 0 for quantize).  The amax is the lane's own: no
// exchange, and one scale choice per block.  s is renormalised in place: the encode reads it, and nothing else does.
template <int F>
__device__ __forceinline__ w6 requantise(float (&s)[kBlockValues], int e, int e_zero, int& e_out) {
    using Fm = Format<F>;
    float am = 0.0f;
#pragma unroll
    for (int i = 0; i < kBlockValues; ++i) am = __builtin_fmaxf(am, __builtin_fabsf(s[i]));
    const int E = __builtin_amdgcn_frexp_expf(am) - Fm::kMaxExp + (__builtin_amdgcn_frexp_mantf(am) > Fm::kThreshold ? 1 : 0);
    int e2 = e + E;
    e2 = e2 < 0 ? 0 : e2 > kMaxScale ? kMaxScale : e2;
    e2 = am == 0.0f ? e_zero : e2;
    const int shift = e - e2;
#pragma unroll
    for (int i = 0; i < kBlockValues; ++i)  // the clamp keeps the sign of zero
        s[i] = __builtin_amdgcn_fmed3f(__builtin_ldexpf(s[i], shift), -Fm::kMax, Fm::kMax);
    e_out = e2;
    return enc32<F>(s);
}

// (r, er) = (x, ex) o (r, er) on a lane's block -- and equally (r, er) o (x, ex): the rule commutes.  The operand of
// the smaller scale is decoded to f32 and shifted down; the other one is decoded to bf16, 16 VGPRs, and each value is
// widened as it is added, so a combine never holds two blocks of f32.
template <int F>
__device__ __forceinline__ void combine(w6& r, int& er, const w6& x, int ex) {
    const bool nan = er == kNaNScale || ex == kNaNScale;
    const bool r_low = er < ex;
    const int e = r_low ? ex : er, d = (r_low ? er : ex) - e;  // d <= 0: the shift of the smaller scale's operand
    w6 lo, hi;
#pragma unroll
    for (int k = 0; k < kBlockWords; ++k) {
        lo[k] = r_low ? r[k] : x[k];
        hi[k] = r_low ? x[k] : r[k];
    }
    const w16 h = dec32_bf16<F>(hi);
    __builtin_amdgcn_sched_barrier(0);  // nothing crosses: left alone, the scheduler starts on the shifts of l before h
    const f32x32 l = dec32<F>(lo);      // is decoded and holds 86 VGPRs
    __builtin_amdgcn_sched_barrier(0);
    float s[kBlockValues];
#pragma unroll
    for (int i = 0; i < kBlockValues; ++i) s[i] = bf16_at(h, i) + __builtin_ldexpf(l[i], d);
    int e2;
    const w6 codes = requantise<F>(s, e, e, e2);
#pragma unroll
    for (int k = 0; k < kBlockWords; ++k) r[k] = nan ? 0u : codes[k];  // the canonical NaN block: 24 zero code bytes
    er = nan ? kNaNScale : e2;
}

}  // namespace chr_mx6
