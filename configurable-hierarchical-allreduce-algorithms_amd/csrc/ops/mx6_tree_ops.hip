// mx6_tree_ops.hip -- libchiara_mx6_tree.so: the MXFP6 block-scaled SUMs (E2M3 and E3M2) registered with tree launchers
// of their own (include/chiara_mx6_tree.h), so that the flat schedules' expression trees run in one HBM pass: every leaf
// read once, the root written once, every inner node requantised in registers to the bytes chr_mx6_<f>_sum_fold would
// have stored.  The rule is csrc/ops/mx6_tile.hpp's own text (Place, ld24, combine<F>, header_word, st_tile), the text
// libchiara_mx6.so's fold runs.  Built with the package's HIPFLAGS and MXFLAGS: no packed f32 arithmetic in this code
// object either.
//
// How the work is split: as k_mx6_fold.  One-wave workgroups; a lane owns a whole block, six code words and a scale,
// the unit of gfx950's FP6 converts; the 16 lanes of a DPP row are a tile; a trip covers four tiles, 1 600 consecutive
// bytes of every leaf; a tree's workgroups stride over its trips, at most kMaxTreeBlocks of them, and trees of one
// instantiation share a grid, eight to a launch, each tree's workgroups contiguous.  The lanes of a trip's missing
// tiles carry zero codes under scale 0 through the same instructions (header_word's row shifts need them present) and
// neither load nor store.
//
// The stack.  The program (chiara.h chr_user_tree: push leaf j, then comb[j] combines) is the same for every lane: leaf
// count and combine counts sit in SGPRs.  The sibling tree kernels (k_mx_tree, k_mx4_tree, k_mxi8_tree) keep the whole
// stack in four named register slots picked by scalar branches.  That does not fit here: the fold alone takes 72
// VGPRs, all a streaming kernel may hold beside RCCL, and four slots of seven registers put this loop at 104.  So
// only the running top of stack (w6 codes, int scale) lives in registers; the rest is parked in LDS, private to the
// lane.  A push at depth d >= 1 writes the old top to park slot d - 1 and loads the leaf into the top's registers; a
// combine at depth d reads slot d - 2 back and runs combine<F>(top, et, x, ex).  Swap bits are not read: the rule
// commutes bit for bit.  Depth 4 needs three slots.  A slot is kSlotBytes = 2 048 bytes in two halves, each a run of 64
// 16-B units, one per lane: words 0 .. 3 of the codes in the first (ds_write_b128 / ds_read_b128), words 4 .. 5 and the
// scale in the second (ds_write_b96 / ds_read_b96, the unit's fourth word unused) -- two DS instructions a push and two
// a pop, off one address register with the half as the instruction's offset.  A lane's unit is its own four banks in
// whichever pass of the wide access serves it, so no bank is asked twice.  The park is kParkBytes = 6 144 bytes.  The
// denser forms were compiled and not kept: seven words per lane, word-major over lanes (5 376 bytes), is seven DS
// instructions each way for the same 71 VGPRs; b128 + b64 + b32 runs at three lane strides (5 376 bytes) wants three
// address registers each way, which stay live across the combine: 86 VGPRs.  Neither was timed.  No barrier: a lane
// reads only what it wrote, the workgroup is one wave, and a wave's LDS operations complete in order.
//
// One combine site.  The LDS address is computed from the run-time depth, so the loop body holds one park write, one
// leaf load, one park read and one combine<F>, where k_mxi8_tree has three combine sites, each with both of its
// paths, under a cascade of scalar branches.  Code size: a k_mx6_tree is 2.4 KB of ISA, the fold's loop plus four DS
// instructions and their address arithmetic, against k_mxi8_tree's 8.7 KB.
//
// Residency.  The park is the front of the launch's dynamic LDS, which is sized as the larger of the library's
// residency cap, chr_user::tree_lds_bytes(wg_per_cu > 0 ? wg_per_cu : 16), and kParkBytes; static LDS stays 0.  At 16
// per CU the cap is 10 240 bytes and holds the park.  The park allows 26 workgroups per CU (160 KB / 6 144), the
// registers 28: a wg_per_cu above 26 is answered with 26.
//
// Load window: none.  Leaf j is loaded when it is pushed, into the registers of the top it replaces.  With leaf j + 1
// held in registers through leaf j's combines the kernel takes 79 VGPRs, past the 72; the sixteen resident waves of a
// CU hide the latency instead.  The variant that sends leaf j + 1 straight into a spare park slot with gfx950's
// direct-to-LDS global loads was not built.
//
// Kernel set: k_mx6_tree<E2M3 | E3M2, 8-B | 4-B accesses>, 4 kernels for 2..8 leaves and every stack depth up to 4;
// 71 VGPRs, 72 allocated, against the fold's 72, no private segment, no static LDS
// (tests/test_mx6_tree_resources.py).
//
// Measured (tools/userop_bench.py --mx6 --mx6-take-all build/libchiara_mx6_tree_take_all.so, chr_reduce_tree, HBM-cold
// rotation, the fold-only op chr_mx6_sum and this kernel interleaved in each of 2 alternating rounds in one process,
// the command run twice, ms per call as the range over the 4 rounds; 31 775 tiles = 12.7 MB and 127 100 tiles = 50.8 MB
// per leaf; profiles/r19/mx6_tree/userop_bench.json and userop_bench_run2.json; the data are the fold rows', tiles
// quantized from normal samples, every block at a magnitude of its own):
//                                                     fold-only        one pass         one pass / fold-only
//   E2M3, 8 leaves, C4's program,  31 775 tiles, ms   0.0463-0.0466    0.0341-0.0347    0.73-0.74
//   E2M3, 8 leaves, C4's program,  47 662 tiles, ms   0.0663-0.0668    0.0496-0.0502    0.74-0.76
//   E2M3, 8 leaves, C4's program,  63 550 tiles, ms   0.0852-0.0858    0.0648-0.0651    0.76
//   E2M3, 8 leaves, C4's program,  95 325 tiles, ms   0.1236-0.1256    0.0950-0.0966    0.76-0.78
//   E2M3, 8 leaves, C4's program, 127 100 tiles, ms   0.1614-0.1641    0.1245-0.1260    0.76-0.78  (0.454-0.459 of 8 TB/s at 9 units)
//   E3M2, 8 leaves, C4's program,  31 775 tiles, ms   0.0461-0.0464    0.0341-0.0345    0.73-0.75
//   E3M2, 8 leaves, C4's program,  47 662 tiles, ms   0.0666-0.0669    0.0497-0.0504    0.74-0.75
//   E3M2, 8 leaves, C4's program,  63 550 tiles, ms   0.0854-0.0861    0.0649-0.0654    0.76
//   E3M2, 8 leaves, C4's program,  95 325 tiles, ms   0.1237-0.1253    0.0950-0.0962    0.76-0.77
//   E3M2, 8 leaves, C4's program, 127 100 tiles, ms   0.1610-0.1638    0.1246-0.1264    0.76-0.78  (0.453-0.459 of 8 TB/s)
//   E2M3, 4 leaves, one chain,     31 775 tiles, ms   0.0175-0.0179    0.0184-0.0189    1.05-1.06
//   E2M3, 4 leaves, one chain,    127 100 tiles, ms   0.0622-0.0627    0.0626-0.0631    1.00-1.01
//   E3M2, 4 leaves, one chain,     31 775 tiles, ms   0.0175-0.0179    0.0184-0.0188    1.04-1.06
//   E3M2, 4 leaves, one chain,    127 100 tiles, ms   0.0622-0.0631    0.0626-0.0635    1.01
//   E2M3, 2 leaves,                31 775 tiles, ms   0.0110-0.0112    0.0109-0.0111    0.98-0.99
//   E2M3, 2 leaves,               127 100 tiles, ms   0.0386-0.0391    0.0375-0.0378    0.97
//   E3M2, 2 leaves,                31 775 tiles, ms   0.0111-0.0115    0.0109-0.0112    0.97-0.98
//   E3M2, 2 leaves,               127 100 tiles, ms   0.0388-0.0393    0.0376-0.0379    0.96-0.97
//   8 virtual ranks, k = 4, b = 4, allreduce of 254 200 tiles per rank (eight 31 775-tile trees to a call), ms
//                                             E2M3    1.329-1.345      1.132-1.136      0.84-0.85
//                                             E3M2    1.327-1.346      1.130-1.136      0.84-0.85
// The expectation was the 8-leaf tree ahead of the folds with ranges clear of each other at 31 775 and at 127 100
// tiles for both formats: it holds, 0.73-0.75 and 0.76-0.78, and at every size between, so the launcher has no size
// bound.  It is the largest gain of the four tree libraries (MXINT8 0.81-0.90, MXFP8 0.86-0.92, MXFP4 0.95 at best):
// the fold was the nearest to HBM, and one pass moves 0.45-0.46 of peak at 9 units.  The 2-leaf tree and the 4-leaf
// chain ((l0 l1) l2) l3 are what one fold launch evaluates with the same traffic and the same combines and without
// the LDS round trips, so a call of nothing but such single-fold trees is declined and takes that fold (single_fold
// below) -- by that derivation, not by these rows, which agree for the chain (one pass clear behind at 31 775 tiles,
// level at 127 100) and not for the 2-leaf tree (level at 31 775, clear ahead by 0.03 at 127 100, for which these
// rows give no reason; the rule was not bent to a 3 % row).  Trees of 3..7 leaves with an inner node were not
// measured; they save traffic and launches as the 8-leaf one does and are taken.
// Residency, the take-all launcher called directly on the 8-leaf tree, ms at 31 775 / 127 100 tiles, E2M3 (E3M2 is
// within 0.0015 of it in every cell): its own 16 per CU (wg_per_cu = 0) 0.0341-0.0354 / 0.1244-0.1262, wg_per_cu = 16
// -- the same launch, timed after the 12 -- 0.0341-0.0357 / 0.1260-0.1285, which is the spread of this row; 12 (what
// the library asks for beside RCCL) 0.0450-0.0453 / 0.1754-0.1763; 26 per CU (all the park allows) 0.0340-0.0347 /
// 0.1246-0.1254.  16 stays; the cap of 12 costs a third and more, and the fold-only op, whose launcher is never told
// of it, is not a yardstick for that row.
#include <atomic>
#include <mutex>

#include <hip/hip_runtime.h>

#include "chiara_mx6_tree.h"
#include "chiara_user_op.hpp"  // tree_lds_bytes alone: the residency rule of the public header's trees
#include "mx6_tile.hpp"

namespace chr_mx6 {

constexpr int kMaxLeaves = 8, kMaxDepth = 4;
constexpr int kMaxTreesPerLaunch = 8;      // trees of one instantiation share a grid
constexpr unsigned kMaxTreeBlocks = 4096;  // one-wave workgroups a tree's trips are strided over (the fold's grid)
constexpr int kOwnWgPerCu = 16;            // resident workgroups per CU when the library asks for none

// The park: kMaxDepth - 1 slots below the top of stack; a slot holds every lane's six code words and scale as two
// 16-B units, kSlotHalf apart.
typedef unsigned int w3 __attribute__((ext_vector_type(3)));
constexpr unsigned kSlotHalf = kWave * 16, kSlotBytes = 2 * kSlotHalf;
constexpr unsigned kParkBytes = (kMaxDepth - 1) * kSlotBytes;
static_assert(kSlotBytes == 2048 && kParkBytes == 6144, "the park's layout");

struct TreeSeg {
    void* out;
    const void* leaves[kMaxLeaves];
    size_t n;       // tiles
    uint32_t nl;    // leaves
    uint32_t comb;  // 2 bits per leaf
    uint32_t nblk;  // this tree's workgroups
};
struct TreeArgs {
    uint32_t block0[kMaxTreesPerLaunch];  // each tree's first workgroup, ascending; ~0u past the last tree
    TreeSeg seg[kMaxTreesPerLaunch];
};

// A lane's block of leaf `p` at `at`.  The lanes of a missing tile hold zero codes under scale 0, as in the fold.
template <bool VEC>
__device__ __forceinline__ void ld_leaf(const void* p, const Place& at, bool live, w6& x, int& ex) {
    x = w6{0u, 0u, 0u, 0u, 0u, 0u};
    ex = 0;
    if (live) {
        x = ld24<VEC>(static_cast<const char*>(p) + at.codes());
        ex = ld_scale(static_cast<const char*>(p) + at.scale());
    }
}

// The lane's part of park slot `slot` (< kMaxDepth - 1): written by a push, read back by the combine that pops it.
__device__ __forceinline__ void park_put(char* park, uint32_t slot, const w6& v, int e) {
    char* const s = park + slot * kSlotBytes + 16u * threadIdx.x;
    *reinterpret_cast<w4*>(s) = w4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<w3*>(s + kSlotHalf) = w3{v[4], v[5], (uint32_t)e};
}
__device__ __forceinline__ void park_get(const char* park, uint32_t slot, w6& v, int& e) {
    const char* const s = park + slot * kSlotBytes + 16u * threadIdx.x;
    const w4 lo = *reinterpret_cast<const w4*>(s);
    const w3 hi = *reinterpret_cast<const w3*>(s + kSlotHalf);
    v = w6{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1]};
    e = (int)hi[2];
}

// Workgroups [block0[s], block0[s] + nblk) evaluate tree s, striding over its trips.  A tile is read and written by
// one row of a wave, every leaf's load before the root's store: `out` may alias any leaf at the same element offset.
template <int F, bool VEC>
__global__ __launch_bounds__(kWave) void k_mx6_tree(TreeArgs a) {
    extern __shared__ __attribute__((aligned(16))) char park[];  // the first kParkBytes of the launch's dynamic LDS
    const uint32_t b = blockIdx.x;
    int s = 0;
#pragma unroll
    for (int j = 1; j < kMaxTreesPerLaunch; ++j)
        if (b >= a.block0[j]) s = j;
    const TreeSeg& g = a.seg[s];
    const uint32_t nblk = g.nblk, nl = g.nl, comb = g.comb;
    const size_t trips = (g.n + kTripTiles - 1) / kTripTiles;
    char* const out = static_cast<char*>(g.out);
    for (size_t trip = b - a.block0[s]; trip < trips; trip += nblk) {
        const Place at(trip);
        const bool live = at.tile < g.n;
        w6 top, x;
        int et, ex;
        ld_leaf<VEC>(g.leaves[0], at, live, top, et);  // leaf 0 is pushed first and combines with nothing
        uint32_t d = 1;                                // values on the stack, the top included
        for (uint32_t j = 1; j < nl; ++j) {
            park_put(park, d - 1, top, et);
            ld_leaf<VEC>(g.leaves[j], at, live, top, et);
            ++d;
            for (uint32_t c = (comb >> (2 * j)) & 3u; c > 0; --c, --d) {
                park_get(park, d - 2, x, ex);
                combine<F>(top, et, x, ex);
            }
        }
        const uint32_t word = header_word(et);
        if (live) st_tile<VEC>(out, at, top, word);
    }
}

}  // namespace chr_mx6

using namespace chr_mx6;

namespace {

std::atomic<long> g_calls{0}, g_declined{0}, g_trees{0}, g_kernels{0};

// A tree the kernel takes: 2..8 leaves, n > 0 tiles, `out` and every leaf non-null and 4-B aligned, a program that
// stays within depth 4 and ends on one value.
bool tree_ok(const chr_user_tree& t) {
    if (t.nleaves < 2 || t.nleaves > kMaxLeaves || t.n == 0 || !t.out || (bits_of(t.out) & 3)) return false;
    int d = 0;
    for (int j = 0; j < t.nleaves; ++j) {
        if (!t.leaves[j] || (bits_of(t.leaves[j]) & 3) || ++d > kMaxDepth || t.comb[j] >= d) return false;
        d -= t.comb[j];
    }
    return d == 1;
}

// -DCHR_MX6_TREE_TAKE_ALL=1 (make mx6_tree_ab) takes every call the kernel can evaluate: the build that
// tools/userop_bench.py --mx6-take-all times against the folds; the default target does not build it.
#ifndef CHR_MX6_TREE_TAKE_ALL
#define CHR_MX6_TREE_TAKE_ALL 0
#endif

// A tree the fold launcher evaluates in one launch with the same traffic: every leaf folds straight into one running
// value, in one operand order (csrc/user_ops.cpp chains those folds into one call).  A call of nothing but such trees
// is declined: the same combines without the LDS round trips.
bool single_fold(const chr_user_tree& t) {
    for (int j = 1; j < t.nleaves; ++j)
        if (t.comb[j] != 1 || t.swaps[j - 1] != t.swaps[0]) return false;
    return true;
}

// 8-B accesses where `out` and every leaf allow them (a block lies at byte 16 + 24 b of its tile).
bool tree_vec(const chr_user_tree& t) {
    uintptr_t al = bits_of(t.out);
    for (int j = 0; j < t.nleaves; ++j) al |= bits_of(t.leaves[j]);
    return (al & 7) == 0;
}

template <int F>
void launch(const TreeArgs& a, unsigned grid, bool vec, unsigned lds, hipStream_t stream) {
    if (vec) hipLaunchKernelGGL((k_mx6_tree<F, true>), dim3(grid), dim3(kWave), lds, stream, a);
    else hipLaunchKernelGGL((k_mx6_tree<F, false>), dim3(grid), dim3(kWave), lds, stream, a);
}

// The chr_user_tree_fn of format F.  Every tree of the call is checked before the first launch; a call with a tree
// the kernel does not take, on any dtype but a live tile type, or of single-fold trees alone is declined whole --
// nonzero, nothing enqueued -- and the library takes the folds.  Trees of one instantiation (8-B or 4-B accesses)
// share launches, kMaxTreesPerLaunch to a grid, each tree's workgroups contiguous.  The launch's dynamic LDS is the
// library's residency cap or the park, whichever is larger.  A launch that fails is left to the caller's
// hipGetLastError.
template <int F>
int sum_tree_launch(const chr_user_tree* trees, int ntrees, chr_dtype dt, int wg_per_cu, hipStream_t stream) {
    ++g_calls;
    bool ok = ntrees > 0 && trees && is_tile_type(dt), pays = false;
    for (int t = 0; ok && t < ntrees; ++t) {
        ok = tree_ok(trees[t]);
        pays = pays || (ok && !single_fold(trees[t]));
    }
    if (!ok || (!CHR_MX6_TREE_TAKE_ALL && !pays)) {
        ++g_declined;
        return 1;
    }
    g_trees += ntrees;
    const unsigned cap = chr_user::tree_lds_bytes(wg_per_cu > 0 ? wg_per_cu : kOwnWgPerCu);
    const unsigned lds = cap > kParkBytes ? cap : kParkBytes;
    for (int vec = 1; vec >= 0; --vec) {
        TreeArgs a{};
        uint32_t grid = 0;
        int k = 0;
        auto flush = [&] {
            if (k == 0) return;
            for (int i = k; i < kMaxTreesPerLaunch; ++i) a.block0[i] = ~0u;
            launch<F>(a, grid, vec != 0, lds, stream);
            ++g_kernels;
            a = TreeArgs{};
            grid = 0;
            k = 0;
        };
        for (int t = 0; t < ntrees; ++t) {
            const chr_user_tree& tr = trees[t];
            if ((int)tree_vec(tr) != vec) continue;
            TreeSeg& g = a.seg[k];
            g.out = tr.out;
            for (int j = 0; j < tr.nleaves; ++j) {
                g.leaves[j] = tr.leaves[j];
                g.comb |= (uint32_t)(tr.comb[j] & 3u) << (2 * j);
            }
            g.n = tr.n;
            g.nl = (uint32_t)tr.nleaves;
            const size_t trips = (tr.n + kTripTiles - 1) / kTripTiles;
            g.nblk = (uint32_t)(trips < kMaxTreeBlocks ? trips : kMaxTreeBlocks);
            a.block0[k] = grid;
            grid += g.nblk;
            if (++k == kMaxTreesPerLaunch) flush();
        }
        flush();
    }
    return 0;
}

std::mutex g_mu;
int g_op[2] = {-1, -1};  // the live op of each format; -1: not registered

}  // namespace

extern "C" {

int chr_mx6_e2m3_sum_tree_launch(const chr_user_tree* trees, int ntrees, chr_dtype dt, int wg_per_cu, hipStream_t stream,
                                 void*) {
    return sum_tree_launch<CHR_MX6_E2M3>(trees, ntrees, dt, wg_per_cu, stream);
}
int chr_mx6_e3m2_sum_tree_launch(const chr_user_tree* trees, int ntrees, chr_dtype dt, int wg_per_cu, hipStream_t stream,
                                 void*) {
    return sum_tree_launch<CHR_MX6_E3M2>(trees, ntrees, dt, wg_per_cu, stream);
}

int chr_mx6_sum_tree(chr_mx6_format f, chr_op* op) {
    if (!op || (f != CHR_MX6_E2M3 && f != CHR_MX6_E3M2)) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_op[f] < 0) {
        chr_op code;
        const int rc = f == CHR_MX6_E2M3
                           ? chr_op_create_tree(chr_mx6_e2m3_sum_fold, chr_mx6_e2m3_sum_tree_launch, nullptr, 1, &code)
                           : chr_op_create_tree(chr_mx6_e3m2_sum_fold, chr_mx6_e3m2_sum_tree_launch, nullptr, 1, &code);
        if (rc) return rc;
        g_op[f] = (int)code;
    }
    *op = (chr_op)g_op[f];
    return CHR_SUCCESS;
}

int chr_mx6_tree_release(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = CHR_SUCCESS;
    for (int& op : g_op) {
        if (op < 0) continue;
        const int e = chr_op_free((chr_op)op);
        if (!rc) rc = e;
        op = -1;
    }
    return rc;
}

void chr_mx6_tree_stats(long out[4], int reset) {
    if (out) {
        out[0] = g_calls;
        out[1] = g_declined;
        out[2] = g_trees;
        out[3] = g_kernels;
    }
    if (reset) g_calls = g_declined = g_trees = g_kernels = 0;
}

}  // extern "C"
