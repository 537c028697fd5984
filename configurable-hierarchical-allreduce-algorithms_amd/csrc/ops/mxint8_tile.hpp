// mxint8_tile.hpp -- the MXINT8 tile and the SUM rule on the device (include/chiara_mxint8.h has the contract), the
// text of csrc/ops/mxint8_ops.hip (libchiara_mxint8.so: the fold and the casts) and of any later kernel that combines
// MXINT8 tiles.  Built with the package's HIPFLAGS and with packed f32 arithmetic disabled (the Makefile's MXFLAGS);
// mxint8_ops.hip's header comment says how the work is split over lanes and when a combine runs on packed 16-bit
// integers instead of f32.
#pragma once

#include <hip/hip_runtime.h>

#include "chiara_mxint8.h"

// 1: a wave whose blocks all have close scales combines them on packed 16-bit integers (combine_i16); 0: every
// combine is the f32 one, the other side of the A/B (make mxint8_ab)
#ifndef CHR_MXI8_INT
#define CHR_MXI8_INT 1
#endif

namespace chr_mxi8 {  // named: the resource test reads the kernels' symbols

constexpr int kTileBytes = CHR_MXI8_TILE_BYTES, kTileValues = CHR_MXI8_TILE_VALUES;
constexpr int kHeader = 16;      // the scale bytes in front of a tile's codes
constexpr int kLaneValues = 16;  // codes per lane: one 16-B access, half a block
constexpr int kWave = 64;        // one-wave workgroups: two tiles per trip
constexpr int kNaNScale = 0xFF, kBias = 127, kMaxScale = 254;
constexpr int kFrac = 6;          // a code is an integer count of 2^-6
constexpr float kMaxCode = 127.0f, kThreshold = 0.9921875f;  // max = 127/64 = kThreshold * 2^kMaxExp
constexpr int kMaxExp = 1;
// The integer combine's domain.  |a| 2^d + |b| <= 128 * 128 + 128 < 2^15 for a gap d <= 7: the sums fit 16 bits.  The
// new scale lies between lo - 6 (the amax is one unit) and lo + 8 (it is 16 512 units), so with lo in 6 .. 246 step 6
// of the rule cannot clamp, and neither scale is 0xFF.
constexpr int kGap16 = 7, kLoMin = 6, kLoMax = kMaxScale - 8;

static_assert(kTileBytes == kHeader + kTileValues && kTileValues == 32 * kLaneValues, "a half-wave is a tile");

typedef unsigned int w4 __attribute__((ext_vector_type(4)));
typedef short h2 __attribute__((ext_vector_type(2)));            // two values: the operands of the v_pk_*16
typedef unsigned short u2 __attribute__((ext_vector_type(2)));  // the same, where a shift may push bits out

inline uintptr_t bits_of(const void* p) { return (uintptr_t)p; }

// The content of a call's dtype, read at run time: a derived code means nothing at compile time.
inline bool is_tile_type(chr_dtype dt) {
    chr_dtype base;
    int count = 0;
    return chr_type_get_contiguous(dt, &base, &count) == CHR_SUCCESS && base == CHR_UINT32 &&
           count == CHR_MXI8_TILE_BYTES / 4;
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

// Where a lane stands in a trip: tile 2 * trip + half, block q / 2 of that tile, the lane's 16 codes and its scale byte.
struct Place {
    size_t tile;
    unsigned q;  // lane of the half-wave: 16 * q is the offset of its codes
    __device__ __forceinline__ Place(size_t trip) : tile(2 * trip + (threadIdx.x >> 5)), q(threadIdx.x & 31u) {}
    __device__ __forceinline__ size_t codes() const { return tile * kTileBytes + kHeader + (size_t)kLaneValues * q; }
    __device__ __forceinline__ size_t scale() const { return tile * kTileBytes + (q >> 1); }
    __device__ __forceinline__ size_t value0() const { return tile * kTileValues + (size_t)kLaneValues * q; }
};

// What the other lane of the block holds: quad_perm:[1,0,3,2].
__device__ __forceinline__ int of_partner(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false); }

// Both lanes of a block hold its scale: word w of the tile's header, the bytes of blocks 4w .. 4w + 3, which lanes
// 8w, 8w + 2, 8w + 4 and 8w + 6 of the half-wave hold -- all in one DPP row of 16 -- is assembled in lane 8w with two
// row shifts (row_shl:n hands lane i the value of lane i + n of its row, 0 past the row's end, which lanes 0 and 8 of
// a row never reach).  Every lane computes a word; lanes 0, 8, 16 and 24 of the half-wave hold the header.
__device__ __forceinline__ uint32_t header_word(int scale) {
    const uint32_t s = (uint32_t)scale;
    const uint32_t two = s | ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x102 /* row_shl:2 */, 0xF, 0xF, true) << 8);
    return two | ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)two, 0x104 /* row_shl:4 */, 0xF, 0xF, true) << 16);
}
template <bool VEC>
__device__ __forceinline__ void st_tile(char* out, const Place& at, w4 codes, uint32_t word) {
    st16<VEC>(out + at.codes(), codes);
    if ((at.q & 7u) == 0)  // lane 8w: header bytes 4w .. 4w + 3
        __builtin_nontemporal_store(word, reinterpret_cast<uint32_t*>(out + at.tile * kTileBytes + (at.q >> 1)));
}

// Byte b of w as the code's integer: dec is this times 2^-6.
__device__ __forceinline__ float code_f32(uint32_t w, int b) { return (float)(int)(int8_t)(w >> (8 * b)); }

// Steps 4 - 7 of the rule on a lane's half of a block: s holds the 16 finite sums relative to scale e.  Returns the
// codes and the new scale; e_zero is the scale of an all-zero block (e for SUM, 0 for quantize).  Both lanes of a block
// compute the same amax and so the same scale.  The encode is one v_ldexp_f32 by (e - e') + 6 -- exact unless the
// rule's own ldexp rounds below 2^-126, where both ways give the code 0x00 -- then v_rndne_f32, the clamp and v_cvt_i32.
__device__ __forceinline__ w4 requantise(const float (&s)[kLaneValues], int e, int e_zero, int& e_out) {
    float am = 0.0f;
#pragma unroll
    for (int i = 0; i < kLaneValues; ++i) am = __builtin_fmaxf(am, __builtin_fabsf(s[i]));
    am = __builtin_fmaxf(am, __builtin_bit_cast(float, of_partner(__builtin_bit_cast(int, am))));
    const int E = __builtin_amdgcn_frexp_expf(am) - kMaxExp + (__builtin_amdgcn_frexp_mantf(am) > kThreshold ? 1 : 0);
    int e2 = e + E;
    e2 = e2 < 0 ? 0 : e2 > kMaxScale ? kMaxScale : e2;
    e2 = am == 0.0f ? e_zero : e2;
    const int shift = e - e2 + kFrac;
    w4 codes;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float t = __builtin_rintf(__builtin_ldexpf(s[4 * k + b], shift));
            w |= ((uint32_t)(int)__builtin_amdgcn_fmed3f(t, -kMaxCode, kMaxCode) & 0xFFu) << (8 * b);
        }
        codes[k] = w;
    }
    e_out = e2;
    return codes;
}

// (r, er) = (x, ex) o (r, er) on a lane's half of a block, the rule as written -- and equally (r, er) o (x, ex): the
// rule commutes.  Any scales, the NaN scale and those at which step 6 clamps included.
__device__ __forceinline__ void combine_f32(w4& r, int& er, const w4& x, int ex) {
    const bool nan = er == kNaNScale || ex == kNaNScale;
    const bool r_low = er < ex;
    const int e = r_low ? ex : er, d = (r_low ? er : ex) - e;  // d <= 0: the shift of the smaller scale's operand
    float s[kLaneValues];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t lo = r_low ? r[k] : x[k], hi = r_low ? x[k] : r[k];
#pragma unroll
        for (int b = 0; b < 4; ++b)
            s[4 * k + b] = __builtin_ldexpf(code_f32(hi, b), -kFrac) + __builtin_ldexpf(code_f32(lo, b), d - kFrac);
    }
    int e2;
    const w4 codes = requantise(s, e, e, e2);
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = nan ? 0u : codes[k];  // the canonical NaN block: 0x00 codes
    er = nan ? kNaNScale : e2;
}

// Whether combine_i16 may take this lane's pair of scales.
__device__ __forceinline__ bool close_scales(int er, int ex) {
    const int lo = er < ex ? er : ex, hi = er < ex ? ex : er;
    return lo >= kLoMin && lo <= kLoMax && hi - lo <= kGap16;
}

__device__ __forceinline__ h2 splat(int v) { return h2{(short)v, (short)v}; }
__device__ __forceinline__ h2 as_h2(uint32_t w) { return __builtin_bit_cast(h2, w); }
__device__ __forceinline__ h2 shl(h2 v, h2 n) { return (h2)((u2)v << (u2)n); }

// The same combine for close_scales(er, ex), on integers in units of 2^(lo - 127 - 6), two values to an instruction.
// With a the code under the larger scale, b the other and d the gap, S = (a << d) + b is the rule's s[i] exactly (f32
// holds it: |S| < 2^15).  A word's even bytes are sign-extended in place by a left and an arithmetic right shift of
// both halves, its odd bytes by the right shift alone, and the a << d is folded into those right shifts: shift by
// 8 - d.  The amax is a max and a min over the lane's eight registers and one exchange with the partner; the new
// scale comes from its leading-zero count: with L the index of its top bit, E' = L - 6, one more when the amax
// exceeds 127 * 2^E' -- the rule's f > 0.9921875.  E' > 0: every S is shifted right, round half to even (add half - 1
// and the bit that will become the lowest, then shift).  E' <= 0: S << -E' is exact.  No result exceeds 127 in
// magnitude, so nothing saturates and 0x80 is never written.
__device__ __forceinline__ void combine_i16(w4& r, int& er, const w4& x, int ex) {
    const bool r_low = er < ex;
    const int lo_e = r_low ? er : ex, hi_e = r_low ? ex : er;
    const h2 up = splat(8 - (hi_e - lo_e)), eight = splat(8);
    h2 S[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t lo = r_low ? r[k] : x[k], hi = r_low ? x[k] : r[k];
        S[2 * k] = (shl(as_h2(hi), eight) >> up) + (shl(as_h2(lo), eight) >> eight);  // bytes 0 and 2
        S[2 * k + 1] = (as_h2(hi & 0xFF00FF00u) >> up) + (as_h2(lo) >> eight);         // bytes 1 and 3
    }
    h2 mx = S[0], mn = S[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        mx = __builtin_elementwise_max(mx, S[i]);
        mn = __builtin_elementwise_min(mn, S[i]);
    }
    const int top = mx[0] > mx[1] ? mx[0] : mx[1], bottom = mn[0] < mn[1] ? mn[0] : mn[1];
    int amax = top > -bottom ? top : -bottom;  // >= 0: bottom <= top
    const int other = of_partner(amax);
    amax = other > amax ? other : amax;
    const int lz = __builtin_clz((unsigned)amax | 1u);  // 17 .. 31: amax <= 16 512
    const int E = 25 - lz + (((unsigned)amax << (lz - 17)) > (127u << 8) ? 1 : 0);
    const int down = E > 0 ? E : 0;
    const h2 vup = splat(E < 0 ? -E : 0), vdown = splat(down);
    const h2 low_bit = splat(down ? 1 : 0), half_less_1 = splat(down ? (1 << (down - 1)) - 1 : 0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t byte[2];
#pragma unroll
        for (int odd = 0; odd < 2; ++odd) {
            const h2 t = shl(S[2 * k + odd], vup);
            const h2 c = (t + half_less_1 + ((t >> vdown) & low_bit)) >> vdown;
            byte[odd] = __builtin_bit_cast(uint32_t, c) & 0x00FF00FFu;
        }
        r[k] = byte[0] | (byte[1] << 8);
    }
    er = amax == 0 ? hi_e : lo_e + E;
}

// (r, er) = (x, ex) o (r, er).  The choice of path is the wave's, not the lane's: one ballot, and a wave whose 32
// blocks all have close scales -- ranks' gradients -- never executes the f32 combine; any other wave takes it whole,
// which is the rule for every block.
__device__ __forceinline__ void combine(w4& r, int& er, const w4& x, int ex) {
#if CHR_MXI8_INT
    if (__builtin_amdgcn_ballot_w64(!close_scales(er, ex)) == 0) {
        combine_i16(r, er, x, ex);
        return;
    }
#endif
    combine_f32(r, er, x, ex);
}

}  // namespace chr_mxi8
