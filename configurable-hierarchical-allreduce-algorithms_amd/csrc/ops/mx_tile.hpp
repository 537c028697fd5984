// mx_tile.hpp -- the MX tile and the SUM rule on the device (include/chiara_mx.h has the contract), one text for the
// code objects that combine tiles: csrc/ops/mx_ops.hip (libchiara_mx.so: the fold and the casts) and
// csrc/ops/mx_tree_ops.hip (libchiara_mx_tree.so: whole expression trees).  Both build with the package's HIPFLAGS and
// with packed f32 arithmetic disabled (the Makefile's MXFLAGS), so that the sixteen sums of a lane stay sixteen
// v_add_f32; mx_ops.hip's header comment says how the work is split over lanes and why decode and encode are the
// instructions they are.
#pragma once

#include <hip/hip_runtime.h>

#include "chiara_mx.h"

namespace chr_mx {  // named: the resource tests read the kernels' symbols

constexpr int kE4M3 = CHR_FP8_E4M3, kE5M2 = CHR_FP8_E5M2;
constexpr int kTileBytes = CHR_MX_TILE_BYTES, kTileValues = CHR_MX_TILE_VALUES;
constexpr int kHeader = 16;      // the scale bytes in front of a tile's codes
constexpr int kLaneValues = 16;  // codes per lane: one 16-B access
constexpr int kWave = 64;        // one-wave workgroups: two tiles per trip
constexpr int kNaNScale = 0xFF, kBias = 127, kMaxScale = 254;

static_assert(kTileBytes == kHeader + kTileValues && kTileValues == 32 * kLaneValues, "a half-wave is a tile");

typedef unsigned int w4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

inline uintptr_t bits_of(const void* p) { return (uintptr_t)p; }

// The content of a call's dtype, read at run time: a derived code means nothing at compile time.
inline bool is_tile_type(chr_dtype dt) {
    chr_dtype base;
    int count = 0;
    return chr_type_get_contiguous(dt, &base, &count) == CHR_SUCCESS && base == CHR_UINT32 &&
           count == CHR_MX_TILE_BYTES / 4;
}

// The element format.  FP4 (a 272-byte tile) is not a third specialisation: a lane owns a whole block there (mx4_tile.hpp).
template <int FMT> struct Fmt;
template <> struct Fmt<kE4M3> {
    static constexpr float kMax = 448.0f;  // 0.875 * 2^9
    static constexpr int kMaxExp = 9;
    static constexpr uint32_t kNaN = 0x7Fu;
};
template <> struct Fmt<kE5M2> {
    static constexpr float kMax = 57344.0f;  // 0.875 * 2^16
    static constexpr int kMaxExp = 16;
    static constexpr uint32_t kNaN = 0x7Eu;
};

template <int FMT, bool HI>
__device__ __forceinline__ f32x2 dec2(uint32_t w) {
    if constexpr (FMT == kE4M3) return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
    else return __builtin_amdgcn_cvt_pk_f32_bf8((int)w, HI);
}
template <int FMT>
__device__ __forceinline__ uint32_t enc4(float c0, float c1, float c2, float c3) {
    int w;
    if constexpr (FMT == kE4M3) {
        w = __builtin_amdgcn_cvt_pk_fp8_f32(c0, c1, 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(c2, c3, w, true);
    } else {
        w = __builtin_amdgcn_cvt_pk_bf8_f32(c0, c1, 0, false);
        w = __builtin_amdgcn_cvt_pk_bf8_f32(c2, c3, w, true);
    }
    return (uint32_t)w;
}

// 16 bytes at p: one 16-B access, or four words where the call's pointers are only 4-B aligned.
template <bool VEC>
__device__ __forceinline__ w4 ld16(const char* p) {
    if constexpr (VEC) {
        return __builtin_nontemporal_load(reinterpret_cast<const w4*>(p));
    } else {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        w4 r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = __builtin_nontemporal_load(q + k);
        return r;
    }
}
template <bool VEC>
__device__ __forceinline__ void st16(char* p, w4 v) {
    if constexpr (VEC) {
        __builtin_nontemporal_store(v, reinterpret_cast<w4*>(p));
    } else {
        uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) __builtin_nontemporal_store(v[k], q + k);
    }
}
__device__ __forceinline__ int ld_scale(const char* p) {
    return (int)__builtin_nontemporal_load(reinterpret_cast<const uint8_t*>(p));
}

// Where a lane stands in a trip: tile 2 * trip + half, block j of that tile, the lane's 16 codes and its scale byte.
struct Place {
    size_t tile;
    unsigned q;  // lane of the half-wave: 16 * q is the offset of its codes, q / 2 its block
    __device__ __forceinline__ Place(size_t trip) : tile(2 * trip + (threadIdx.x >> 5)), q(threadIdx.x & 31u) {}
    __device__ __forceinline__ size_t codes() const { return tile * kTileBytes + kHeader + (size_t)kLaneValues * q; }
    __device__ __forceinline__ size_t scale() const { return tile * kTileBytes + (q >> 1); }
    __device__ __forceinline__ size_t value0() const { return tile * kTileValues + (size_t)kLaneValues * q; }
};

// The even lanes of a half-wave hold their blocks' scales: word w of the tile's header, bytes of blocks 4w .. 4w + 3,
// assembled in lane w of the half-wave (every lane computes a word; lanes 0 .. 3 hold the header).
__device__ __forceinline__ uint32_t header_word(int scale) {
    const unsigned first = (threadIdx.x & 32u) + 8u * (threadIdx.x & 3u);
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        word |= ((uint32_t)__builtin_amdgcn_ds_bpermute((int)(4u * (first + 2u * k)), scale) & 0xFFu) << (8 * k);
    return word;
}
template <bool VEC>
__device__ __forceinline__ void st_tile(char* out, const Place& at, w4 codes, uint32_t word) {
    st16<VEC>(out + at.codes(), codes);
    if (at.q < 4)
        __builtin_nontemporal_store(word, reinterpret_cast<uint32_t*>(out + at.tile * kTileBytes + 4u * at.q));
}

// Steps 4 - 7 of the rule on a lane's half of a block: s holds the 16 sums relative to scale e.  Returns the codes and
// the new scale; e_zero is the scale of a block whose finite values are all zero (e for SUM, 0 for quantize).  Both
// lanes of a block compute the same amax and so the same scale.
template <int FMT>
__device__ __forceinline__ w4 requantise(const float (&s)[kLaneValues], int e, int e_zero, int& e_out) {
    constexpr uint32_t kInf = 0x7F800000u;
    // |s| of the finite values as bits: for non-negative floats the order of the bits is the order of the values
    uint32_t amax = 0;
#pragma unroll
    for (int i = 0; i < kLaneValues; ++i) {
        const uint32_t a = __builtin_bit_cast(uint32_t, s[i]) & 0x7FFFFFFFu;
        const uint32_t f = a < kInf ? a : 0u;
        amax = f > amax ? f : amax;
    }
    const uint32_t other = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)amax, 0xB1 /* quad_perm:[1,0,3,2] */, 0xF, 0xF, false);
    amax = other > amax ? other : amax;
    const float am = __builtin_bit_cast(float, amax);
    const int E = __builtin_amdgcn_frexp_expf(am) - Fmt<FMT>::kMaxExp + (__builtin_amdgcn_frexp_mantf(am) > 0.875f ? 1 : 0);
    int e2 = e + E;
    e2 = e2 < 0 ? 0 : e2 > kMaxScale ? kMaxScale : e2;
    e2 = amax == 0 ? e_zero : e2;
    const int shift = e - e2;
    w4 codes;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float c[4];
        uint32_t nan = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float v = s[4 * k + b];
            const bool own = !(__builtin_fabsf(v) < __builtin_inff());  // NaN or infinite: the canonical NaN code
            const float t = __builtin_ldexpf(v, shift);
            c[b] = own ? 0.0f : __builtin_amdgcn_fmed3f(t, -Fmt<FMT>::kMax, Fmt<FMT>::kMax);  // keeps the sign of zero
            nan |= own ? Fmt<FMT>::kNaN << (8 * b) : 0u;
        }
        codes[k] = enc4<FMT>(c[0], c[1], c[2], c[3]) | nan;  // the instruction's code of +0 is 0x00
    }
    e_out = e2;
    return codes;
}

// (r, er) = (x, ex) o (r, er) on a lane's half of a block -- and equally (r, er) o (x, ex): the rule commutes.
template <int FMT>
__device__ __forceinline__ void combine(w4& r, int& er, const w4& x, int ex) {
    const bool nan = er == kNaNScale || ex == kNaNScale;
    const bool r_low = er < ex;
    const int e = r_low ? ex : er, d = (r_low ? er : ex) - e;  // d <= 0: the shift of the smaller scale's operand
    float s[kLaneValues];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t lo = r_low ? r[k] : x[k], hi = r_low ? x[k] : r[k];
        const f32x2 l0 = dec2<FMT, false>(lo), l1 = dec2<FMT, true>(lo);
        const f32x2 h0 = dec2<FMT, false>(hi), h1 = dec2<FMT, true>(hi);
        s[4 * k + 0] = h0[0] + __builtin_ldexpf(l0[0], d);
        s[4 * k + 1] = h0[1] + __builtin_ldexpf(l0[1], d);
        s[4 * k + 2] = h1[0] + __builtin_ldexpf(l1[0], d);
        s[4 * k + 3] = h1[1] + __builtin_ldexpf(l1[1], d);
    }
    int e2;
    const w4 codes = requantise<FMT>(s, e, e, e2);
    constexpr uint32_t kNaN4 = Fmt<FMT>::kNaN * 0x01010101u;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = nan ? kNaN4 : codes[k];
    er = nan ? kNaNScale : e2;
}

}  // namespace chr_mx
