// mx4_tree_ops.hip -- libchiara_mx4_tree.so: the MXFP4 block-scaled SUM registered with a tree launcher of its own
// (include/chiara_mx4_tree.h), so that the flat schedules' expression trees run in one HBM pass: every leaf read once,
// the root written once, every inner node requantised in registers to the bytes chr_mx4_sum_fold would have stored.
// The rule is csrc/ops/mx4_pair.hpp's combine_half, mx4_tile.hpp's combine on half a block, instruction for
// instruction.  Built with the package's HIPFLAGS and MXFLAGS: no packed f32 arithmetic in this code object either.
//
// How the work is split: not as k_mx4_fold.  There a lane owns a whole block and 32 f32 sums are live inside a
// combine; k_mx_tree's loop body over that split (mx4_tile.hpp's Place, ld16, combine, st_tile unchanged, gfx950,
// -O3, the same flags) was prototyped before this kernel was written and allocates, without scratch:
//     stack of 4 slots, a load window of one leaf   78 VGPRs (16-B accesses), 78 (4-B accesses)
//     stack of 4 slots, no load window              76
//     stack of 3 slots, a load window of one leaf   83
//     stack of 3 slots, no load window              78
//     stack of 2 slots, a load window of one leaf   64
//     stack of 2 slots, no load window              61
// and __attribute__((amdgpu_num_vgpr(72))) changed nothing.  C4's own program has depth 3, so no variant that fits
// the 72 VGPRs a wave may hold beside RCCL takes it: the fold's split cannot carry a stack.  Here a lane pair owns a
// block.  One-wave workgroups; a lane holds 8 code bytes (two words) and its own 16 f32 sums, a half-wave of 32 lanes
// is a tile, a trip covers two tiles, 544 consecutive bytes of every leaf; a tree's workgroups stride over its trips.
// The lanes of a missing second tile carry zeros through the same instructions and neither load nor store.  The
// block's amax is each lane's fmax over its 16 sums completed by one DPP exchange with the partner lane; both lanes
// then choose the same scale, which stays a per-lane register, so an inner node needs nothing more between lanes.  The
// tile's four header words are assembled once per trip, at the root, by two DPP row shifts (by 2 and by 4): no LDS and
// no ds_bpermute.
//
// The program (chiara.h chr_user_tree: push leaf j, then comb[j] combines) is the same for every lane: leaf count
// and combine counts sit in SGPRs, and each push and combine is a scalar branch over four named stack slots of
// (codes w2, scale int), 3 registers each -- an array indexed by the run-time depth would become scratch.  Swap bits
// are not read: the rule commutes bit for bit.
//
// Load window: one leaf.  Leaf j + 1 is loaded (8 B of codes and the scale byte, 3 registers) before the combines
// that follow leaf j run, so one leaf is in flight beside the stack (at most 4 x 3 registers) and the 16 f32 sums of
// the running combine; eight leaves in flight would need 8 x 3 registers before the first sum and the stack beside
// them.  The leaf count is a run-time loop, so the kernel set is k_mx4_tree<8-B | 4-B accesses>: 2 kernels for 2..8
// leaves and every stack depth up to 4.  Each of the two takes 52 VGPRs, 56 allocated, where the fold's split took 78,
// no private segment and no static LDS (tests/test_mx4_tree_resources.py); the launch's dynamic LDS is not touched, it
// caps the workgroups resident per CU.
//
// Measured (tools/userop_bench.py --mx4 --mx4-take-all, chr_reduce_tree, HBM-cold rotation, the fold-only op
// chr_mx4_sum and this kernel interleaved in each of 2 alternating rounds in one process, ms per call as the range
// over the 2 rounds; 31 775 tiles = 8.6 MB and 127 100 tiles = 34.6 MB per leaf;
// profiles/r15/mx4_tree/userop_bench.json):
//                                               fold-only        one pass         one pass / fold-only
//   8 leaves, C4's program,  31 775 tiles, ms   0.0395-0.0396    0.0376-0.0377    0.95
//   8 leaves, C4's program,  47 662 tiles, ms   0.0550-0.0552    0.0548-0.0549    0.99-1.00
//   8 leaves, C4's program,  63 550 tiles, ms   0.0701-0.0705    0.0715-0.0716    1.01-1.02
//   8 leaves, C4's program,  95 325 tiles, ms   0.0997-0.1011    0.1023-0.1024    1.01-1.03
//   8 leaves, C4's program, 127 100 tiles, ms   0.1282-0.1286    0.1363           1.06  (0.285 of 8 TB/s at 9 units)
//   4 leaves, one chain,     31 775 tiles, ms   0.0158-0.0159    0.0188-0.0189    1.18-1.20
//   4 leaves, one chain,    127 100 tiles, ms   0.0528-0.0533    0.0634-0.0637    1.19-1.21
//   2 leaves,                31 775 tiles, ms   0.0079-0.0082    0.0098-0.0099    1.20-1.25
//   2 leaves,               127 100 tiles, ms   0.0226-0.0227    0.0292-0.0298    1.29-1.32
//   8 virtual ranks, k = 4, b = 4, allreduce of 254 200 tiles per rank (eight 31 775-tile trees to a call), ms
//                                               1.112-1.114      1.001-1.005      0.90
// MXFP4 does not keep MXFP8's gain.  With twice the arithmetic per byte the kernel is held by its VALU work, not by
// HBM: the 8-leaf tree saves four units of traffic in thirteen and still loses from 63 550 tiles on, where the three
// fold launches are long enough to hide their launch cost, because a half block per lane pays the scale choice and its
// exchange twice per block where k_mx4_fold pays it once.  It is ahead, with ranges clear of the fold-only ones, at
// 31 775 tiles per tree and in the allreduce, whose calls hold eight trees of that size: one launch there stands for
// 24.  At 47 662 tiles the two ranges are 0.0001 ms apart, which two rounds do not make clear.  So the launcher takes
// a call only if no tree of it has more than kOnePassMaxTiles = 31 775 tiles, the largest size measured clear ahead;
// any other call it declines to the folds, the fold launcher's path.  The 2-leaf tree and the 4-leaf chain
// ((l0 l1) l2) l3 are what one fold launch evaluates with the same traffic and the same combines; there k_mx4_fold is
// ahead by a fifth and more in every round, so a call of nothing but such single-fold trees is declined as well
// (single_fold below).  Trees of 3..7 leaves with an inner node were not measured; they save traffic and launches as
// the 8-leaf one does and are taken.
// Residency, the take-all launcher called directly on the 8-leaf tree, ms at 31 775 / 127 100 tiles: its own 16 per CU
// 0.0376 / 0.1362-0.1363, wg_per_cu = 12 (what the library asks for beside RCCL) 0.0508-0.0509 / 0.2050-0.2059, 32 per
// CU (every wave slot) 0.0377 / 0.1369-0.1371.  16 stays; the cap of 12 costs a third and more, and the fold-only op,
// whose launcher is never told of it, is not a yardstick for that row.
#include <atomic>
#include <mutex>

#include <hip/hip_runtime.h>

#include "chiara_mx4_tree.h"
#include "chiara_user_op.hpp"  // tree_lds_bytes alone: the residency rule of the public header's trees
#include "mx4_pair.hpp"

namespace chr_mx4 {

constexpr int kMaxLeaves = 8, kMaxDepth = 4;
constexpr int kMaxTreesPerLaunch = 8;      // trees of one instantiation share a grid
constexpr unsigned kMaxTreeBlocks = 4096;  // one-wave workgroups a tree's trips are strided over (the fold's grid)
constexpr int kOwnWgPerCu = 16;            // resident workgroups per CU when the library asks for none

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

// A lane's part of leaf `p` at `at`; zeros in the lanes of a missing tile.
template <bool VEC>
__device__ __forceinline__ void ld_leaf(const void* p, const PairPlace& at, bool live, w2& x, int& ex) {
    x = w2{0u, 0u};
    ex = 0;
    if (live) {
        x = ld8<VEC>(static_cast<const char*>(p) + at.codes());
        ex = ld_scale(static_cast<const char*>(p) + at.scale());
    }
}

// Workgroups [block0[s], block0[s] + nblk) evaluate tree s, striding over its trips.  A tile is read and written by
// one half-wave, every leaf's load before the root's store: `out` may alias any leaf at the same element offset.
template <bool VEC>
__global__ __launch_bounds__(kWave) void k_mx4_tree(TreeArgs a) {
    const uint32_t b = blockIdx.x;
    int s = 0;
#pragma unroll
    for (int j = 1; j < kMaxTreesPerLaunch; ++j)
        if (b >= a.block0[j]) s = j;
    const TreeSeg& g = a.seg[s];
    const uint32_t nblk = g.nblk, nl = g.nl, comb = g.comb;
    const size_t trips = (g.n + kPairTripTiles - 1) / kPairTripTiles;
    char* const out = static_cast<char*>(g.out);
    for (size_t trip = b - a.block0[s]; trip < trips; trip += nblk) {
        const PairPlace at(trip);
        const bool live = at.tile < g.n;
        w2 s0, s1 = {0u, 0u}, s2 = s1, s3 = s1, nx;
        int e0, e1 = 0, e2 = 0, e3 = 0, ne;
        ld_leaf<VEC>(g.leaves[0], at, live, s0, e0);  // leaf 0 is pushed first and combines with nothing
        ld_leaf<VEC>(g.leaves[1], at, live, nx, ne);
        uint32_t d = 1;
        for (uint32_t j = 1; j < nl; ++j) {
            if (d == 1) s1 = nx, e1 = ne;
            else if (d == 2) s2 = nx, e2 = ne;
            else s3 = nx, e3 = ne;
            ++d;
            if (j + 1 < nl) ld_leaf<VEC>(g.leaves[j + 1], at, live, nx, ne);  // in flight while leaf j's combines run
            for (uint32_t c = (comb >> (2 * j)) & 3u; c > 0; --c, --d) {
                if (d == 2) combine_half(s0, e0, s1, e1);
                else if (d == 3) combine_half(s1, e1, s2, e2);
                else combine_half(s2, e2, s3, e3);
            }
        }
        const uint32_t word = pair_header_word(e0);
        if (live) st_pair_tile<VEC>(out, at, s0, word);
    }
}

}  // namespace chr_mx4

using namespace chr_mx4;

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

// -DCHR_MX4_TREE_TAKE_ALL=1 (make mx4_tree_ab) takes every call the kernel can evaluate: the build that
// tools/userop_bench.py --mx4-take-all times against the folds; the default target does not build it.
#ifndef CHR_MX4_TREE_TAKE_ALL
#define CHR_MX4_TREE_TAKE_ALL 0
#endif

// The most tiles a tree may have for one pass to be ahead of the folds with ranges clear of each other (the table
// above): the largest measured size at which it is.  A call with any larger tree is declined.
constexpr size_t kOnePassMaxTiles = 31775;

// A tree the fold launcher evaluates in one launch with the same traffic: every leaf folds straight into one running
// value, in one operand order (csrc/user_ops.cpp chains those folds into one call).  Measured slower in one pass (the
// table above), as for MXFP8; a call of nothing but such trees is declined.
bool single_fold(const chr_user_tree& t) {
    for (int j = 1; j < t.nleaves; ++j)
        if (t.comb[j] != 1 || t.swaps[j - 1] != t.swaps[0]) return false;
    return true;
}

// One 8-B access per lane where `out` and every leaf allow it.
bool tree_vec(const chr_user_tree& t) {
    uintptr_t al = bits_of(t.out);
    for (int j = 0; j < t.nleaves; ++j) al |= bits_of(t.leaves[j]);
    return (al & 7) == 0;
}

std::mutex g_mu;
int g_op = -1;  // the live op; -1: not registered

}  // namespace

extern "C" {

// The chr_user_tree_fn the op is registered with.  Every tree of the call is checked before the first launch; a call
// with a tree the kernel does not take, on any dtype but a live tile type, with a tree of more than kOnePassMaxTiles
// tiles, or of single-fold trees alone is declined whole -- nonzero, nothing enqueued -- and the library takes the
// folds.  Trees of one instantiation (8-B or 4-B accesses) share launches, kMaxTreesPerLaunch to a grid, each tree's
// workgroups contiguous.  A launch that fails is left to the caller's hipGetLastError.
int chr_mx4_sum_tree_launch(const chr_user_tree* trees, int ntrees, chr_dtype dt, int wg_per_cu, hipStream_t stream,
                            void*) {
    ++g_calls;
    bool ok = ntrees > 0 && trees && is_tile_type(dt), pays = false, big = false;
    for (int t = 0; ok && t < ntrees; ++t) {
        ok = tree_ok(trees[t]);
        pays = pays || (ok && !single_fold(trees[t]));
        big = big || trees[t].n > kOnePassMaxTiles;
    }
    if (!ok || (!CHR_MX4_TREE_TAKE_ALL && (!pays || big))) {
        ++g_declined;
        return 1;
    }
    g_trees += ntrees;
    const unsigned lds = chr_user::tree_lds_bytes(wg_per_cu > 0 ? wg_per_cu : kOwnWgPerCu);
    for (int vec = 1; vec >= 0; --vec) {
        TreeArgs a{};
        uint32_t grid = 0;
        int k = 0;
        auto flush = [&] {
            if (k == 0) return;
            for (int i = k; i < kMaxTreesPerLaunch; ++i) a.block0[i] = ~0u;
            if (vec) hipLaunchKernelGGL((k_mx4_tree<true>), dim3(grid), dim3(kWave), lds, stream, a);
            else hipLaunchKernelGGL((k_mx4_tree<false>), dim3(grid), dim3(kWave), lds, stream, a);
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
            const size_t trips = (tr.n + kPairTripTiles - 1) / kPairTripTiles;
            g.nblk = (uint32_t)(trips < kMaxTreeBlocks ? trips : kMaxTreeBlocks);
            a.block0[k] = grid;
            grid += g.nblk;
            if (++k == kMaxTreesPerLaunch) flush();
        }
        flush();
    }
    return 0;
}

int chr_mx4_sum_tree(chr_op* op) {
    if (!op) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_op < 0) {
        chr_op code;
        if (int rc = chr_op_create_tree(chr_mx4_sum_fold, chr_mx4_sum_tree_launch, nullptr, 1, &code)) return rc;
        g_op = (int)code;
    }
    *op = (chr_op)g_op;
    return CHR_SUCCESS;
}

int chr_mx4_tree_release(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = CHR_SUCCESS;
    if (g_op >= 0) {
        rc = chr_op_free((chr_op)g_op);
        g_op = -1;
    }
    return rc;
}

void chr_mx4_tree_stats(long out[4], int reset) {
    if (out) {
        out[0] = g_calls;
        out[1] = g_declined;
        out[2] = g_trees;
        out[3] = g_kernels;
    }
    if (reset) g_calls = g_declined = g_trees = g_kernels = 0;
}

}  // extern "C"
