// mx4_tile.hpp -- the MX4 tile and the SUM rule on the device (include/chiara_mx4.h has the contract), the text of
// csrc/ops/mx4_ops.hip (libchiara_mx4.so: the fold and the casts) and of any later kernel that combines MX4 tiles.
// Built with the package's HIPFLAGS and with packed f32 arithmetic disabled (the Makefile's MXFLAGS), so that the 32
// sums of a lane stay 32 v_add_f32; mx4_ops.hip's header comment says how the work is split over lanes and why decode
// and encode are the instructions they are.
#pragma once

#include <hip/hip_runtime.h>

#include "chiara_mx4.h"

namespace chr_mx4 {  // named: the resource test reads the kernels' symbols

constexpr int kTileBytes = CHR_MX4_TILE_BYTES, kTileValues = CHR_MX4_TILE_VALUES;
constexpr int kHeader = 16;       // the scale bytes in front of a tile's codes
constexpr int kBlockValues = 32;  // codes per lane: a whole block, one 16-B access
constexpr int kBlockBytes = 16;
constexpr int kRow = 16;          // lanes per tile: one DPP row
constexpr int kWave = 64;         // one-wave workgroups
constexpr int kTripTiles = kWave / kRow;  // four tiles, 1 088 consecutive bytes, per wave trip
constexpr int kNaNScale = 0xFF, kBias = 127, kMaxScale = 254;
constexpr float kMax = 6.0f;  // 0.75 * 2^3
constexpr int kMaxExp = 3;

static_assert(kTileBytes == kHeader + kRow * kBlockBytes && kTileValues == kRow * kBlockValues, "a DPP row is a tile");

typedef unsigned int w4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

inline uintptr_t bits_of(const void* p) { return (uintptr_t)p; }

// The content of a call's dtype, read at run time: a derived code means nothing at compile time.
inline bool is_tile_type(chr_dtype dt) {
    chr_dtype base;
    int count = 0;
    return chr_type_get_contiguous(dt, &base, &count) == CHR_SUCCESS && base == CHR_UINT32 &&
           count == CHR_MX4_TILE_BYTES / 4;
}

// v_cvt_scalef32_pk_f32_fp4 at scale 1.0: byte B of w, the low nibble in [0] and the high nibble in [1], the tile's
// own order.  Exact on all 16 codes, -0 included.
template <int B>
__device__ __forceinline__ f32x2 dec2(uint32_t w) {
    return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, B);
}
// v_cvt_scalef32_pk_fp4_f32 at scale 1.0 into byte B of w: c0 in the low nibble, c1 in the high one.  On the device
// it is the rule's enc_sat as it stands -- nearest, ties to the even code, the subnormal kept, the sign of a zero and
// of a value that rounds to zero kept -- so nothing is corrected in VALU (tests/test_gpu_mx4.py pins it).
template <int B>
__device__ __forceinline__ uint32_t enc2(uint32_t w, float c0, float c1) {
    return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, c0, c1, 1.0f, B);
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

// Where a lane stands in a trip: tile 4 * trip + row, block b of that tile -- its 16 code bytes and its scale byte.
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
__device__ __forceinline__ void st_tile(char* out, const Place& at, w4 codes, uint32_t word) {
    st16<VEC>(out + at.codes(), codes);
    if ((at.b & 3u) == 0)  // lane 4w: header bytes 4w .. 4w + 3
        __builtin_nontemporal_store(word, reinterpret_cast<uint32_t*>(out + at.tile * kTileBytes + at.b));
}

// Steps 4 - 7 of the rule on a lane's block: s holds the 32 finite sums relative to scale e.  Returns the codes and the
// new scale; e_zero is the scale of an all-zero block (e for SUM, 0 for quantize).  The amax is the lane's own: no
// exchange, and one scale choice per block.
__device__ __forceinline__ w4 requantise(const float (&s)[kBlockValues], int e, int e_zero, int& e_out) {
    float am = 0.0f;
#pragma unroll
    for (int i = 0; i < kBlockValues; ++i) am = __builtin_fmaxf(am, __builtin_fabsf(s[i]));
    const int E = __builtin_amdgcn_frexp_expf(am) - kMaxExp + (__builtin_amdgcn_frexp_mantf(am) > 0.75f ? 1 : 0);
    int e2 = e + E;
    e2 = e2 < 0 ? 0 : e2 > kMaxScale ? kMaxScale : e2;
    e2 = am == 0.0f ? e_zero : e2;
    const int shift = e - e2;
    w4 codes;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float c[8];
#pragma unroll
        for (int b = 0; b < 8; ++b)  // the clamp keeps the sign of zero
            c[b] = __builtin_amdgcn_fmed3f(__builtin_ldexpf(s[8 * k + b], shift), -kMax, kMax);
        uint32_t w = 0;
        w = enc2<0>(w, c[0], c[1]);
        w = enc2<1>(w, c[2], c[3]);
        w = enc2<2>(w, c[4], c[5]);
        w = enc2<3>(w, c[6], c[7]);
        codes[k] = w;
    }
    e_out = e2;
    return codes;
}

// The eight values of word w, the operand of the smaller scale shifted down by -d.
template <bool SHIFT>
__device__ __forceinline__ void dec8(uint32_t w, int d, float (&v)[8]) {
    const f32x2 p0 = dec2<0>(w), p1 = dec2<1>(w), p2 = dec2<2>(w), p3 = dec2<3>(w);
    const float t[8] = {p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = SHIFT ? __builtin_ldexpf(t[i], d) : t[i];
}

// (r, er) = (x, ex) o (r, er) on a lane's block -- and equally (r, er) o (x, ex): the rule commutes.
__device__ __forceinline__ void combine(w4& r, int& er, const w4& x, int ex) {
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
    const w4 codes = requantise(s, e, e, e2);
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = nan ? 0u : codes[k];  // the canonical NaN block: sixteen 0x00 code bytes
    er = nan ? kNaNScale : e2;
}

}  // namespace chr_mx4
