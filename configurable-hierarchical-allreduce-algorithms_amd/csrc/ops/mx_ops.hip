// mx_ops.hip -- libchiara_mx.so: the MXFP8 block-scaled SUM on the user-op interface, and the casts into and out of
// the MX tile (include/chiara_mx.h has the contract: the 528-byte tile, the SUM rule, the error codes).  A combine is
// a cooperative operation on a block of 32 values -- align two scales, add, find the new amax, choose the new scale,
// re-encode -- which an element-wise functor cannot express, so none of the three kernels comes through
// include/chiara_user_op.hpp: they are this file's own.  Built with the package's HIPFLAGS (-fno-fast-math keeps the
// finiteness tests as written, -ffp-contract=off keeps every add an add) and with packed f32 arithmetic disabled for
// this code object, so that the sixteen sums of a lane stay sixteen v_add_f32.
//
// How the work is split.  One-wave workgroups.  A lane owns 16 consecutive codes, one 16-B access; lanes 2j and 2j + 1
// of a half-wave form block j, so a half-wave is a tile and a wave trip covers two tiles, 1 056 consecutive bytes.
// Each lane loads its block's scale as a byte of the tile's 16-B header (the 32 lanes of a half-wave share that line).
// The 16 values of a lane live in registers as f32 from decode to encode; the only exchange between lanes is the
// block's amax, one DPP quad_perm:[1,0,3,2] and a max, and the assembly of a tile's 16 new scale bytes, four
// ds_bpermute per trip after which lanes 0 .. 3 of the half-wave store one word each.  No LDS is allocated.
//
// Decode is gfx950's v_cvt_pk_f32_fp8 / _bf8 followed by one v_ldexp_f32 on the operand of the smaller scale (the
// other shift of the rule is 0, and f32 addition commutes bit for bit, so which operand is `in` does not matter and
// the kernel does not branch on running_first).  The scaled converts (v_cvt_scalef32_pk_f32_fp8 / _bf8 with 2^(ex - e)
// as the scale operand) would fold the ldexp into the decode, but a relative scale reaches 2^-254, below what an f32
// scale operand can hold, and what the instruction does with a result below 2^-126 is not established: the plain
// decode and v_ldexp_f32 are the rule as written.  Encode is v_cvt_pk_fp8_f32 / _bf8_f32 on values already clamped
// to [-max, +max], as csrc/ops/fp8_ops.hip does it; NaN codes are OR-ed in afterwards.  The scale choice is one
// v_frexp_exp / v_frexp_mant pair and one compare: max = 0.875 * 2^9 (E4M3) or 0.875 * 2^16 (E5M2), so with
// amax = f * 2^x, f in [0.5, 1), the smallest E with amax * 2^-E <= max is x - 9 (x - 16), plus 1 when f > 0.875.
//
// The tile and the rule on the device (decode, combine, requantise, a tile's loads and stores) are csrc/ops/mx_tile.hpp,
// shared with the one-pass trees of libchiara_mx_tree.so (csrc/ops/mx_tree_ops.hip).
//
// k_mx_fold requantises every intermediate block in registers: each `o` rounds to the format, and the bits equal the
// fold-by-fold result, with m + 1 reads and one write per tile.  Loads and stores are non-temporal; the grid is
// capped at kMaxGrid one-wave workgroups, 16 per CU, which leaves room beside RCCL.
//
// Measured (tools/userop_bench.py --mx, folds in place at 127 100 tiles = 64 MiB per operand, HBM-cold, 2 alternating
// rounds in one process, GB/s of the (m + 2) x bytes traffic; libchiara_fp8.so's E4M3 SATURATE SUM on the same bytes
// is the yardstick; profiles/r12/mx/userop_bench.json):
//                      FP8 E4M3 SUM SAT   MX E4M3 SUM     MX E5M2 SUM     MX / FP8
//   fold m = 1, GB/s   5210 / 5209        4306 / 4450     4328 / 4461     0.83-0.86
//   fold m = 3, GB/s   5042 / 5057        3364 / 3372     3374 / 3372     0.67
// The kernel is ALU-bound: its rate falls as the combines per byte moved rise, where the FP8 SUM stays level.  Per
// lane and combine the ISA holds 16 v_cvt_pk_f32, 32 v_ldexp_f32 (16 aligning, 16 renormalising), 16 v_add_f32, 16
// v_med3_f32, 8 v_cvt_pk encodes and one DPP; 52 VGPRs (56 allocated), no scratch (tests/test_mx_resources.py).
#include <atomic>
#include <mutex>

#include <hip/hip_runtime.h>

#include "mx_tile.hpp"  // the tile and the rule on the device: Fmt .. combine, shared with csrc/ops/mx_tree_ops.hip

namespace chr_mx {

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
// carry zeros through the same instructions (the exchanges between lanes stay wave-wide) and neither load nor store.
template <int FMT, bool VEC>
__global__ __launch_bounds__(kWave) void k_mx_fold(FoldArgs a) {
    const size_t trips = (a.n + 1) / 2;
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
            combine<FMT>(r, er, x, ex);
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
// vectors where src is 16-B aligned (wide_vec) and all 16 lie below n, one by one and +0 beyond n otherwise.
template <typename S, int FMT, bool VEC>
__global__ __launch_bounds__(kWave) void k_mx_quantize(void* tiles, const void* src, size_t n, int wide_vec) {
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
        int e2;
        const w4 codes = requantise<FMT>(s, kBias, 0, e2);
        const uint32_t word = header_word(e2);
        if (live) st_tile<VEC>(static_cast<char*>(tiles), at, codes, word);
    }
}

// dst[i] = ldexp(dec(code i), scale - 127), i < n: a lane's 16 values as 16-B vectors where dst is 16-B aligned
// (wide_vec) and all 16 lie below n, one by one below n otherwise; a lane wholly beyond n touches nothing.
template <typename D, int FMT, bool VEC>
__global__ __launch_bounds__(kWave) void k_mx_dequantize(void* dst, const void* tiles, size_t n, int wide_vec) {
    const size_t ntiles = (n + kTileValues - 1) / kTileValues, trips = (ntiles + 1) / 2;
    const char* const in = static_cast<const char*>(tiles);
    D* const out = static_cast<D*>(dst);
    for (size_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const Place at(trip);
        const size_t i0 = at.value0();
        if (i0 >= n) continue;
        const w4 codes = ld16<VEC>(in + at.codes());
        const int e = ld_scale(in + at.scale());
        const int shift = e - kBias;
        const bool nan = e == kNaNScale;
        Wide16<D> r;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const f32x2 lo = dec2<FMT, false>(codes[k]), hi = dec2<FMT, true>(codes[k]);
            const float v[4] = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
            for (int b = 0; b < 4; ++b)
                narrow(nan ? __builtin_nanf("") : __builtin_ldexpf(v[b], shift), r.e[4 * k + b]);
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

}  // namespace chr_mx

using namespace chr_mx;

namespace {

std::atomic<long> g_fold_calls{0}, g_declined{0}, g_kernels{0};

unsigned grid_for(size_t tiles) {
    const size_t trips = (tiles + 1) / 2;
    return (unsigned)(trips < kMaxGrid ? (trips ? trips : 1) : kMaxGrid);
}

// The chr_user_reduce_fn of format FMT.  Declines -- nonzero, nothing enqueued -- any dtype but a live tile type and
// any pointer that is not 4-B aligned.  Fan-in beyond kMaxIns runs as consecutive launches, each continuing from `out`.
template <int FMT>
int fold_launcher(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dt, hipStream_t stream) {
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
        if (vec) hipLaunchKernelGGL((k_mx_fold<FMT, true>), dim3(grid), dim3(kWave), 0, stream, a);
        else hipLaunchKernelGGL((k_mx_fold<FMT, false>), dim3(grid), dim3(kWave), 0, stream, a);
        if (hipGetLastError() != hipSuccess) return 1;
        ++g_kernels;
        done += a.m;
        cur = out;
    } while (done < m);
    return 0;
}

}  // namespace

// The launchers the ops are registered with.  running_first is not looked at: the rule commutes bit for bit.
extern "C" int chr_mx_e4m3_sum_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dt,
                                    int, hipStream_t stream, void*) {
    return fold_launcher<kE4M3>(out, acc, ins, m, n, dt, stream);
}
extern "C" int chr_mx_e5m2_sum_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dt,
                                    int, hipStream_t stream, void*) {
    return fold_launcher<kE5M2>(out, acc, ins, m, n, dt, stream);
}

namespace {

std::mutex g_mu;
int g_op[2] = {-1, -1};  // the live op of each format; -1: not registered
int g_type = -1;         // the cached tile type

bool format_ok(int f) { return f == kE4M3 || f == kE5M2; }
bool wide_ok(chr_dtype t) { return t == CHR_FLOAT32 || t == CHR_BFLOAT16; }

template <typename S, int FMT>
int launch_quantize(void* tiles, const void* src, size_t n, hipStream_t s) {
    const unsigned grid = grid_for((n + CHR_MX_TILE_VALUES - 1) / CHR_MX_TILE_VALUES);
    const int wide_vec = (bits_of(src) & 15) == 0;
    if ((bits_of(tiles) & 15) == 0)
        hipLaunchKernelGGL((k_mx_quantize<S, FMT, true>), dim3(grid), dim3(kWave), 0, s, tiles, src, n, wide_vec);
    else
        hipLaunchKernelGGL((k_mx_quantize<S, FMT, false>), dim3(grid), dim3(kWave), 0, s, tiles, src, n, wide_vec);
    return hipGetLastError() == hipSuccess ? CHR_SUCCESS : CHR_ERR_HIP;
}

template <typename D, int FMT>
int launch_dequantize(void* dst, const void* tiles, size_t n, hipStream_t s) {
    const unsigned grid = grid_for((n + CHR_MX_TILE_VALUES - 1) / CHR_MX_TILE_VALUES);
    const int wide_vec = (bits_of(dst) & 15) == 0;
    if ((bits_of(tiles) & 15) == 0)
        hipLaunchKernelGGL((k_mx_dequantize<D, FMT, true>), dim3(grid), dim3(kWave), 0, s, dst, tiles, n, wide_vec);
    else
        hipLaunchKernelGGL((k_mx_dequantize<D, FMT, false>), dim3(grid), dim3(kWave), 0, s, dst, tiles, n, wide_vec);
    return hipGetLastError() == hipSuccess ? CHR_SUCCESS : CHR_ERR_HIP;
}

// What both casts check before anything is enqueued; CHR_SUCCESS: launch.
int cast_args(const void* tiles, const void* wide, chr_dtype wide_type, int f) {
    if (!tiles || !wide) return CHR_ERR_INVALID_ARG;
    if (!wide_ok(wide_type) || !format_ok(f)) return CHR_ERR_UNSUPPORTED;
    if ((bits_of(tiles) & 3) || (bits_of(wide) & (wide_type == CHR_FLOAT32 ? 3 : 1))) return CHR_ERR_UNSUPPORTED;
    return CHR_SUCCESS;
}

}  // namespace

extern "C" {

int chr_mx_type(chr_dtype* type) {
    if (!type) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_type < 0) {
        chr_dtype code;
        if (int rc = chr_type_contiguous(CHR_MX_TILE_BYTES / 4, CHR_UINT32, &code)) return rc;
        g_type = (int)code;
    }
    *type = (chr_dtype)g_type;
    return CHR_SUCCESS;
}

int chr_mx_sum(chr_fp8_format f, chr_op* op) {
    if (!op) return CHR_ERR_INVALID_ARG;
    if (!format_ok((int)f)) return CHR_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(g_mu);
    int& slot = g_op[(int)f];
    if (slot < 0) {
        chr_op code;
        if (int rc = chr_op_create(f == CHR_FP8_E4M3 ? chr_mx_e4m3_sum_fold : chr_mx_e5m2_sum_fold, nullptr, 1, &code))
            return rc;
        slot = (int)code;
    }
    *op = (chr_op)slot;
    return CHR_SUCCESS;
}

int chr_mx_quantize(void* tiles, const void* src, size_t n, chr_dtype src_type, chr_fp8_format f, hipStream_t s) {
    if (int rc = cast_args(tiles, src, src_type, (int)f)) return rc;
    if (n == 0) return CHR_SUCCESS;
    if (src_type == CHR_FLOAT32)
        return f == CHR_FP8_E4M3 ? launch_quantize<float, kE4M3>(tiles, src, n, s)
                                 : launch_quantize<float, kE5M2>(tiles, src, n, s);
    return f == CHR_FP8_E4M3 ? launch_quantize<bf16_bits, kE4M3>(tiles, src, n, s)
                             : launch_quantize<bf16_bits, kE5M2>(tiles, src, n, s);
}

int chr_mx_dequantize(void* dst, const void* tiles, size_t n, chr_dtype dst_type, chr_fp8_format f, hipStream_t s) {
    if (int rc = cast_args(tiles, dst, dst_type, (int)f)) return rc;
    if (n == 0) return CHR_SUCCESS;
    if (dst_type == CHR_FLOAT32)
        return f == CHR_FP8_E4M3 ? launch_dequantize<float, kE4M3>(dst, tiles, n, s)
                                 : launch_dequantize<float, kE5M2>(dst, tiles, n, s);
    return f == CHR_FP8_E4M3 ? launch_dequantize<bf16_bits, kE4M3>(dst, tiles, n, s)
                             : launch_dequantize<bf16_bits, kE5M2>(dst, tiles, n, s);
}

int chr_mx_release(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = CHR_SUCCESS;
    for (int& c : g_op) {
        if (c < 0) continue;
        const int e = chr_op_free((chr_op)c);
        if (!rc) rc = e;
        c = -1;
    }
    if (g_type >= 0) {
        const int e = chr_type_free((chr_dtype)g_type);
        if (!rc) rc = e;
        g_type = -1;
    }
    return rc;
}

void chr_mx_stats(long out[3], int reset) {
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
