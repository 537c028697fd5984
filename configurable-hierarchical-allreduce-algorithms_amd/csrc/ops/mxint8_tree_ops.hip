// mxint8_tree_ops.hip -- libchiara_mxint8_tree.so: the MXINT8 block-scaled SUM registered with a tree launcher of its
// own (include/chiara_mxint8_tree.h), so that the flat schedules' expression trees run in one HBM pass: every leaf
// read once, the root written once, every inner node requantised in registers to the bytes chr_mxi8_sum_fold would
// have stored.  The rule is csrc/ops/mxint8_tile.hpp's own text (combine_i16, combine_f32, header_word, st_tile), the
// text libchiara_mxint8.so's fold runs.  Built with the package's HIPFLAGS and MXFLAGS: no packed f32 arithmetic in
// this code object either.
//
// How the work is split: as k_mxi8_fold.  One-wave workgroups; a lane holds 16 codes in one dwordx4, a lane pair is a
// block, a half-wave a tile; a trip covers two tiles, 1 056 consecutive bytes of every leaf; a tree's workgroups
// stride over its trips, at most kMaxTreeBlocks of them, and trees of one instantiation share a grid, eight to a
// launch, each tree's workgroups contiguous.
//
// The program (chiara.h chr_user_tree: push leaf j, then comb[j] combines) is the same for every lane: leaf count
// and combine counts sit in SGPRs, and each push and combine is a scalar branch over four named stack slots of
// (codes w4, scale int) -- an array indexed by the run-time depth would become scratch.  Swap bits are not read: the
// rule commutes bit for bit.  An inner node needs no exchange of headers: both lanes of a block compute the same
// scale, which stays a per-lane register; header_word runs once per trip, at the root.  No LDS and no ds_bpermute.
//
// Path choice.  In the fold one ballot per operand picks packed 16-bit integers or f32 for the wave, and every scale
// it looks at was loaded.  Here the scales of inner nodes exist only once computed, so the choice is made per combine
// (combine_node): one ballot over the two scales the combine is about to consume and one scalar branch, nested inside
// the scalar branch that picked the stack slots, so neither combine_i16 nor combine_f32 ever runs under a partial
// mask and a wave whose blocks all stay close never executes an f32 combine, at any depth.  A node that leaves the
// integer domain -- a NaN scale, a clamp, a gap above 7 after a cancellation -- sends only the combines above it to
// f32.  Only live lanes vote: the lanes of a trip's missing second tile carry zero codes under scale 127 (ld_leaf),
// which combine_i16 and combine_f32 both map to zero codes under scale 127 again, always inside the integer domain;
// otherwise the odd tail trip of every tree, and every 1-tile tree, would be forced onto f32 whatever its data.  Those
// lanes run the same instructions (the DPP exchanges need their partners) and neither load nor store.
//
// Load window: one leaf.  Leaf j + 1 is loaded (16 B of codes and the scale byte, 5 registers) before the combines
// that follow leaf j run, so one leaf is in flight beside the stack (at most 4 x 5 registers) and the 8 packed or 16
// f32 sums of the running combine.  The leaf count is a run-time loop, so the kernel set is
// k_mxi8_tree<16-B | 4-B accesses>: 2 kernels for 2..8 leaves and every stack depth up to 4.  Each holds both paths
// at each of its three combine sites and takes 68 VGPRs, 72 allocated, against the fold's 48, no private segment and
// no static LDS (tests/test_mxint8_tree_resources.py); the launch's dynamic LDS is not touched, it caps the workgroups
// resident per CU.  Stack slots unpacked as eight h2 registers, which would spare an inner node on the integer path
// its repack and unpack, were not built or timed: four such slots are 36 registers where the packed ones are 20,
// which on top of this kernel's 68 passes the 72 a wave may hold beside RCCL.
//
// Measured (tools/userop_bench.py --mxint8 --mxint8-take-all build/libchiara_mxint8_tree_take_all.so, chr_reduce_tree,
// HBM-cold rotation, the fold-only op chr_mxi8_sum and this kernel interleaved in each of 2 alternating rounds in one
// process, the command run twice, ms per call as the range over the 4 rounds; 31 775 tiles = 16.8 MB and 127 100 tiles
// = 67.1 MB per leaf; profiles/r18/mxint8_tree/userop_bench.json and userop_bench_run2.json; `close` and `wild` are
// mxint8_ops.hip's two data sets):
//                                                      fold-only        one pass         one pass / fold-only
//   close, 8 leaves, C4's program,  31 775 tiles, ms   0.0576-0.0577    0.0466-0.0467    0.81
//   close, 8 leaves, C4's program,  47 662 tiles, ms   0.0808-0.0811    0.0676-0.0679    0.83-0.84
//   close, 8 leaves, C4's program,  63 550 tiles, ms   0.1029-0.1036    0.0885-0.0892    0.85-0.86
//   close, 8 leaves, C4's program,  95 325 tiles, ms   0.1473-0.1482    0.1274-0.1279    0.86-0.87
//   close, 8 leaves, C4's program, 127 100 tiles, ms   0.1949-0.1964    0.1689-0.1692    0.86-0.87  (0.446 of 8 TB/s at 9 units)
//   wild,  8 leaves, C4's program,  31 775 tiles, ms   0.0653-0.0655    0.0549-0.0551    0.84
//   wild,  8 leaves, C4's program,  47 662 tiles, ms   0.0926-0.0934    0.0802-0.0809    0.86-0.87
//   wild,  8 leaves, C4's program,  63 550 tiles, ms   0.1191-0.1208    0.1054-0.1060    0.88-0.89
//   wild,  8 leaves, C4's program,  95 325 tiles, ms   0.1706-0.1727    0.1521-0.1529    0.88-0.89
//   wild,  8 leaves, C4's program, 127 100 tiles, ms   0.2256-0.2280    0.2021-0.2037    0.89-0.90  (0.372 of 8 TB/s)
//   close, 4 leaves, one chain,     31 775 tiles, ms   0.0225-0.0226    0.0232-0.0233    1.03
//   close, 4 leaves, one chain,    127 100 tiles, ms   0.0759-0.0774    0.0801-0.0808    1.03-1.06
//   wild,  4 leaves, one chain,     31 775 tiles, ms   0.0263-0.0266    0.0265-0.0266    1.00-1.01
//   wild,  4 leaves, one chain,    127 100 tiles, ms   0.0910-0.0927    0.0927-0.0938    1.01-1.03
//   close, 2 leaves,                31 775 tiles, ms   0.0124-0.0125    0.0128           1.02-1.03
//   close, 2 leaves,               127 100 tiles, ms   0.0428-0.0429    0.0435-0.0437    1.01-1.02
//   wild,  2 leaves,                31 775 tiles, ms   0.0127-0.0130    0.0132-0.0138    1.03-1.07
//   wild,  2 leaves,               127 100 tiles, ms   0.0436-0.0439    0.0443-0.0448    1.01-1.02
//   8 virtual ranks, k = 4, b = 4, allreduce of 254 200 close tiles per rank (eight 31 775-tile trees to a call), ms
//                                                      1.605-1.610      1.392-1.400      0.87
// The expectation was the 8-leaf tree ahead of the folds with ranges clear of each other on close data at 31 775 and
// at 127 100 tiles: it holds, 0.81 and 0.86-0.87, and at every size between and on wild data as well, so the launcher
// has no size bound -- MXFP4's ALU ceiling is not reached: the one-pass kernel on close data moves 0.446 of peak where
// MXFP8's moved 0.338.  The 2-leaf tree and the 4-leaf chain ((l0 l1) l2) l3 are what one fold launch evaluates with
// the same traffic and the same combines; there k_mxi8_fold (48 VGPRs, no stack, one ballot per operand) is ahead or
// level in every round and one pass is never clear ahead, so a call of nothing but such single-fold trees is declined
// and takes that fold (single_fold below).  Trees of 3..7 leaves with an inner node were not measured; they save
// traffic and launches as the 8-leaf one does and are taken.
// Residency, the take-all launcher called directly on the 8-leaf tree, ms at 31 775 / 127 100 tiles, close data: its
// own 16 per CU (wg_per_cu = 0) 0.0464-0.0467 / 0.1687-0.1695, wg_per_cu = 16 -- the same launch, timed after the 12 --
// 0.0465-0.0471 / 0.1732-0.1759, which is the spread of this row; 12 (what the library asks for beside RCCL)
// 0.0617-0.0620 / 0.2496-0.2516; 28 per CU (all the registers allow) 0.0464-0.0467 / 0.1689-0.1698.  16 stays; the cap
// of 12 costs a third and more, and the fold-only op, whose launcher is never told of it, is not a yardstick for that
// row.
#include <atomic>
#include <mutex>

#include <hip/hip_runtime.h>

#include "chiara_mxint8_tree.h"
#include "chiara_user_op.hpp"  // tree_lds_bytes alone: the residency rule of the public header's trees
#include "mxint8_tile.hpp"

namespace chr_mxi8 {

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

// A lane's part of leaf `p` at `at`.  The lanes of a missing tile hold zero codes under scale 127, operands of the
// integer domain that every combine maps to themselves: they never vote a wave onto the f32 path.
template <bool VEC>
__device__ __forceinline__ void ld_leaf(const void* p, const Place& at, bool live, w4& x, int& ex) {
    x = w4{0u, 0u, 0u, 0u};
    ex = kBias;
    if (live) {
        x = ld16<VEC>(static_cast<const char*>(p) + at.codes());
        ex = ld_scale(static_cast<const char*>(p) + at.scale());
    }
}

// (r, er) = (x, ex) o (r, er) at one node of the tree: the wave's choice of path for this combine alone, by one
// ballot over the scales as they are now -- an inner node's were computed a moment ago -- and one scalar branch.
__device__ __forceinline__ void combine_node(w4& r, int& er, const w4& x, int ex) {
#if CHR_MXI8_INT
    if (__builtin_amdgcn_ballot_w64(!close_scales(er, ex)) == 0) {
        combine_i16(r, er, x, ex);
        return;
    }
#endif
    combine_f32(r, er, x, ex);
}

// Workgroups [block0[s], block0[s] + nblk) evaluate tree s, striding over its trips.  A tile is read and written by
// one half-wave, every leaf's load before the root's store: `out` may alias any leaf at the same element offset.
template <bool VEC>
__global__ __launch_bounds__(kWave) void k_mxi8_tree(TreeArgs a) {
    const uint32_t b = blockIdx.x;
    int s = 0;
#pragma unroll
    for (int j = 1; j < kMaxTreesPerLaunch; ++j)
        if (b >= a.block0[j]) s = j;
    const TreeSeg& g = a.seg[s];
    const uint32_t nblk = g.nblk, nl = g.nl, comb = g.comb;
    const size_t trips = (g.n + 1) / 2;
    char* const out = static_cast<char*>(g.out);
    for (size_t trip = b - a.block0[s]; trip < trips; trip += nblk) {
        const Place at(trip);
        const bool live = at.tile < g.n;
        w4 s0, s1 = {0u, 0u, 0u, 0u}, s2 = s1, s3 = s1, nx;
        int e0, e1 = kBias, e2 = kBias, e3 = kBias, ne;
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
                if (d == 2) combine_node(s0, e0, s1, e1);
                else if (d == 3) combine_node(s1, e1, s2, e2);
                else combine_node(s2, e2, s3, e3);
            }
        }
        const uint32_t word = header_word(e0);
        if (live) st_tile<VEC>(out, at, s0, word);
    }
}

}  // namespace chr_mxi8

using namespace chr_mxi8;

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

// -DCHR_MXI8_TREE_TAKE_ALL=1 (make mxint8_tree_ab) takes every call the kernel can evaluate: the build that
// tools/userop_bench.py --mxint8-take-all times against the folds; the default target does not build it.
#ifndef CHR_MXI8_TREE_TAKE_ALL
#define CHR_MXI8_TREE_TAKE_ALL 0
#endif

// A tree the fold launcher evaluates in one launch with the same traffic: every leaf folds straight into one running
// value, in one operand order (csrc/user_ops.cpp chains those folds into one call).  A call of nothing but such trees
// is declined.
bool single_fold(const chr_user_tree& t) {
    for (int j = 1; j < t.nleaves; ++j)
        if (t.comb[j] != 1 || t.swaps[j - 1] != t.swaps[0]) return false;
    return true;
}

// One 16-B access per lane where `out` and every leaf allow it.
bool tree_vec(const chr_user_tree& t) {
    uintptr_t al = bits_of(t.out);
    for (int j = 0; j < t.nleaves; ++j) al |= bits_of(t.leaves[j]);
    return (al & 15) == 0;
}

std::mutex g_mu;
int g_op = -1;  // the live op; -1: not registered

}  // namespace

extern "C" {

// The chr_user_tree_fn the op is registered with.  Every tree of the call is checked before the first launch; a call
// with a tree the kernel does not take, on any dtype but a live tile type, or of single-fold trees alone is declined
// whole -- nonzero, nothing enqueued -- and the library takes the folds.  Trees of one instantiation (16-B or 4-B
// accesses) share launches, kMaxTreesPerLaunch to a grid, each tree's workgroups contiguous.  A launch that fails is
// left to the caller's hipGetLastError.
int chr_mxi8_sum_tree_launch(const chr_user_tree* trees, int ntrees, chr_dtype dt, int wg_per_cu, hipStream_t stream,
                             void*) {
    ++g_calls;
    bool ok = ntrees > 0 && trees && is_tile_type(dt), pays = false;
    for (int t = 0; ok && t < ntrees; ++t) {
        ok = tree_ok(trees[t]);
        pays = pays || (ok && !single_fold(trees[t]));
    }
    if (!ok || (!CHR_MXI8_TREE_TAKE_ALL && !pays)) {
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
            if (vec) hipLaunchKernelGGL((k_mxi8_tree<true>), dim3(grid), dim3(kWave), lds, stream, a);
            else hipLaunchKernelGGL((k_mxi8_tree<false>), dim3(grid), dim3(kWave), lds, stream, a);
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
            const size_t trips = (tr.n + 1) / 2;
            g.nblk = (uint32_t)(trips < kMaxTreeBlocks ? trips : kMaxTreeBlocks);
            a.block0[k] = grid;
            grid += g.nblk;
            if (++k == kMaxTreesPerLaunch) flush();
        }
        flush();
    }
    return 0;
}

int chr_mxi8_sum_tree(chr_op* op) {
    if (!op) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_op < 0) {
        chr_op code;
        if (int rc = chr_op_create_tree(chr_mxi8_sum_fold, chr_mxi8_sum_tree_launch, nullptr, 1, &code)) return rc;
        g_op = (int)code;
    }
    *op = (chr_op)g_op;
    return CHR_SUCCESS;
}

int chr_mxi8_tree_release(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = CHR_SUCCESS;
    if (g_op >= 0) {
        rc = chr_op_free((chr_op)g_op);
        g_op = -1;
    }
    return rc;
}

void chr_mxi8_tree_stats(long out[4], int reset) {
    if (out) {
        out[0] = g_calls;
        out[1] = g_declined;
        out[2] = g_trees;
        out[3] = g_kernels;
    }
    if (reset) g_calls = g_declined = g_trees = g_kernels = 0;
}

}  // extern "C"
