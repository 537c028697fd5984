// mx4_pair.hpp -- the MX4 SUM rule on half a block: the device text of csrc/ops/mx4_tree_ops.hip
// (libchiara_mx4_tree.so).  mx4_tile.hpp's split gives a lane a whole block, 32 f32 sums live inside a combine; that
// leaves no registers for an expression stack (mx4_tree_ops.hip's header comment has the counts).  Here a lane pair
// owns a block: lane q of a half-wave holds bytes 8 q .. 8 q + 7 of the tile's codes, 16 values of block q / 2, and
// both lanes of the pair hold the block's scale.  The rule is mx4_tile.hpp's instruction for instruction -- the same
// converts at scale 1.0 (dec2, enc2, dec8), the same v_ldexp_f32, v_add_f32 and v_med3_f32 on every value -- so the
// bytes are the fold's; only the amax crosses lanes, by one DPP exchange, and max is exact.  Built with the package's
// HIPFLAGS and MXFLAGS like every text that combines tiles.
#pragma once

#include "mx4_tile.hpp"

namespace chr_mx4 {

constexpr int kHalfValues = 16;  // codes per lane: half a block, two words
constexpr int kHalfBytes = 8;
constexpr int kHalfWave = 32;    // lanes per tile
constexpr int kPairTripTiles = kWave / kHalfWave;  // two tiles, 544 consecutive bytes, per wave trip

static_assert(kTileBytes == kHeader + kHalfWave * kHalfBytes && kTileValues == kHalfWave * kHalfValues,
              "a half-wave is a tile");

typedef unsigned int w2 __attribute__((ext_vector_type(2)));

// 8 bytes at p: one 8-B access, or two words where the call's pointers are only 4-B aligned.
template <bool VEC>
__device__ __forceinline__ w2 ld8(const char* p) {
    if constexpr (VEC) {
        return __builtin_nontemporal_load(reinterpret_cast<const w2*>(p));
    } else {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        w2 r;
        r[0] = __builtin_nontemporal_load(q);
        r[1] = __builtin_nontemporal_load(q + 1);
        return r;
    }
}
template <bool VEC>
__device__ __forceinline__ void st8(char* p, w2 v) {
    if constexpr (VEC) {
        __builtin_nontemporal_store(v, reinterpret_cast<w2*>(p));
    } else {
        uint32_t* q = reinterpret_cast<uint32_t*>(p);
        __builtin_nontemporal_store(v[0], q);
        __builtin_nontemporal_store(v[1], q + 1);
    }
}

// Where a lane stands in a trip: tile 2 * trip + half, lane q of that half-wave -- its 8 code bytes and the scale byte
// of its block, q / 2.
struct PairPlace {
    size_t tile;
    unsigned q;
    __device__ __forceinline__ PairPlace(size_t trip) : tile(kPairTripTiles * trip + (threadIdx.x >> 5)), q(threadIdx.x & 31u) {}
    __device__ __forceinline__ size_t codes() const { return tile * kTileBytes + kHeader + (size_t)kHalfBytes * q; }
    __device__ __forceinline__ size_t scale() const { return tile * kTileBytes + (q >> 1); }
};

// Lanes 2 b and 2 b + 1 of a half-wave hold block b's scale: word w of the tile's header, the bytes of blocks 4w ..
// 4w + 3, sits in lanes 8w, 8w + 2, 8w + 4 and 8w + 6, all of one DPP row, and is assembled in lane 8w with two row
// shifts (row_shl:n hands lane i the value of lane i + n of its row; a lane that would read past the row's end gets
// 0, and lanes 0 and 8 of a row never do).  Every lane computes a word; lanes 0, 8, 16 and 24 hold the header.
__device__ __forceinline__ uint32_t pair_header_word(int scale) {
    const uint32_t s = (uint32_t)scale;
    const uint32_t two = s | ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x102 /* row_shl:2 */, 0xF, 0xF, true) << 8);
    return two | ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)two, 0x104 /* row_shl:4 */, 0xF, 0xF, true) << 16);
}
template <bool VEC>
__device__ __forceinline__ void st_pair_tile(char* out, const PairPlace& at, w2 codes, uint32_t word) {
    st8<VEC>(out + at.codes(), codes);
    if ((at.q & 7u) == 0)  // lane 8w: header bytes 4w .. 4w + 3, which is where its own scale byte begins
        __builtin_nontemporal_store(word, reinterpret_cast<uint32_t*>(out + at.scale()));
}

// Steps 4 - 7 of the SUM on a lane's half of a block: s holds its 16 finite sums relative to scale e; an all-zero block
// keeps e.  The amax is the lane's own fmax completed by the partner's (quad_perm:[1,0,3,2] swaps the lanes of a
// pair), so both lanes choose the same scale and an inner node needs no further exchange.
__device__ __forceinline__ w2 requantise_half(const float (&s)[kHalfValues], int e, int& e_out) {
    float am = 0.0f;
#pragma unroll
    for (int i = 0; i < kHalfValues; ++i) am = __builtin_fmaxf(am, __builtin_fabsf(s[i]));
    const float other = __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, am), 0xB1 /* quad_perm:[1,0,3,2] */, 0xF, 0xF, false));
    am = __builtin_fmaxf(am, other);
    const int E = __builtin_amdgcn_frexp_expf(am) - kMaxExp + (__builtin_amdgcn_frexp_mantf(am) > 0.75f ? 1 : 0);
    int e2 = e + E;
    e2 = e2 < 0 ? 0 : e2 > kMaxScale ? kMaxScale : e2;
    e2 = am == 0.0f ? e : e2;
    const int shift = e - e2;
    w2 codes;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
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

// (r, er) = (x, ex) o (r, er) on a lane's half of a block -- and equally (r, er) o (x, ex): the rule commutes.  Wave-
// wide: the exchange in requantise_half reads the partner lane, so both lanes of a pair run it together.
__device__ __forceinline__ void combine_half(w2& r, int& er, const w2& x, int ex) {
    const bool nan = er == kNaNScale || ex == kNaNScale;
    const bool r_low = er < ex;
    const int e = r_low ? ex : er, d = (r_low ? er : ex) - e;  // d <= 0: the shift of the smaller scale's operand
    float s[kHalfValues];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float lo[8], hi[8];
        dec8<true>(r_low ? r[k] : x[k], d, lo);
        dec8<false>(r_low ? x[k] : r[k], 0, hi);
#pragma unroll
        for (int i = 0; i < 8; ++i) s[8 * k + i] = hi[i] + lo[i];
    }
    int e2;
    const w2 codes = requantise_half(s, e, e2);
    r[0] = nan ? 0u : codes[0];  // the canonical NaN block: sixteen 0x00 code bytes
    r[1] = nan ? 0u : codes[1];
    er = nan ? kNaNScale : e2;
}

}  // namespace chr_mx4
