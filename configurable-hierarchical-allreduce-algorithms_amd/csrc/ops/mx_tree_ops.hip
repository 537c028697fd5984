// mx_tree_ops.hip -- libchiara_mx_tree.so: the MXFP8 block-scaled SUM registered with a tree launcher of its own
// (include/chiara_mx_tree.h), so that the flat schedules' expression trees run in one HBM pass: every leaf read once,
// the root written once, every inner node requantised in registers.  The rule is csrc/ops/mx_tile.hpp's combine, the
// text libchiara_mx.so's fold runs, so the root's bytes are the fold-by-fold bytes.  Built with the package's HIPFLAGS
// and MXFLAGS: no packed f32 arithmetic in this code object either.
//
// How the work is split: as k_mx_fold.  One-wave workgroups; a lane owns 16 codes, a lane pair a block, a half-wave a
// tile; a trip covers two tiles, 1 056 consecutive bytes of every leaf; a tree's workgroups stride over its trips.
// The lanes of a missing second tile carry zeros through the same instructions and neither load nor store.
//
// The program (chiara.h chr_user_tree: push leaf j, then comb[j] combines) is the same for every lane: leaf count
// and combine counts sit in SGPRs, and each push and combine is a scalar branch over four named stack slots of
// (codes w4, scale int) -- an array indexed by the run-time depth would become scratch.  Swap bits are not read: the
// rule commutes bit for bit.  An inner node needs no ds_bpermute: both lanes of a block compute the same scale, which
// stays a per-lane register; header_word runs once per trip, at the root.
//
// Load window: one leaf.  Leaf j + 1 is loaded (16 B of codes and the scale byte, 5 registers) before the combines
// that follow leaf j run, so one leaf is in flight beside the stack (at most 4 x 5 registers) and the 16 f32 sums of
// the running combine; eight leaves in flight would need 8 x 5 registers before the first sum.  The leaf count is a
// run-time loop, so the kernel set is k_mx_tree<format, 16-B | 4-B accesses>: 4 kernels for 2..8 leaves.
// With that window each of the four kernels takes 71 VGPRs, 72 allocated, no private segment and no static LDS
// (tests/test_mx_tree_resources.py); the launch's dynamic LDS is not touched, it caps the workgroups resident per CU.
//
// Measured (tools/userop_bench.py --mx, chr_reduce_tree, HBM-cold rotation, the fold-only op chr_mx_sum and this op
// interleaved in each of 2 alternating rounds in one process, ms per call as the range over the rounds; 31 775 tiles
// = 16 MiB and 127 100 tiles = 64 MiB per leaf; profiles/r13/mx_tree/userop_bench.json).  E4M3; E5M2 is within
// 0.0005 ms of it in every row:
//                                          fold-only        one pass         one pass / fold-only
//   8 leaves, C4's program, 16 MiB, ms     0.0699-0.0700    0.0604           0.86
//   8 leaves, C4's program, 64 MiB, ms     0.2434-0.2435    0.2233-0.2237    0.92   (0.338 of 8 TB/s at 9 units)
//   4 leaves, one chain,    16 MiB, ms     0.0284           0.0288           1.01
//   4 leaves, one chain,    64 MiB, ms     0.0994           0.1020-0.1022    1.03
//   2 leaves,               16 MiB, ms     0.0132           0.0140-0.0141    1.06
//   2 leaves,               64 MiB, ms     0.0449           0.0457-0.0458    1.02
//   8 virtual ranks, k = 4, b = 4, allreduce of 128 MiB per rank, ms
//                                          1.701-1.705      1.491-1.497      0.88
// The 8-leaf tree saves three units of traffic in four and two launches in three, and its ranges lie clear of the
// fold-only ones: kept.  The 2-leaf tree and the 4-leaf chain ((l0 l1) l2) l3 are what one fold launch evaluates with
// the same traffic and the same combines; there k_mx_fold (56 VGPRs, no stack) is ahead in every round, so a call of
// nothing but such single-fold trees is declined and takes that fold (single_fold below).  Trees of 3..7 leaves with
// an inner node were not measured; they save traffic as the 8-leaf one does and are taken.
// Residency, the E4M3 launcher called directly on the 8-leaf tree, ms at 16 / 64 MiB: its own 16 per CU
// 0.0603 / 0.2232-0.2233, wg_per_cu = 12 (what the library asks for beside RCCL) 0.0805-0.0808 / 0.3216-0.3270, 28 per
// CU (all the registers allow) 0.0604-0.0605 / 0.2238.  16 stays; the cap of 12 costs a third, and the fold-only op,
// whose launcher is never told of it, is not a yardstick for that row.
#include <atomic>
#include <mutex>

#include <hip/hip_runtime.h>

#include "chiara_mx_tree.h"
#include "chiara_user_op.hpp"  // tree_lds_bytes alone: the residency rule of the public header's trees
#include "mx_tile.hpp"

namespace chr_mx {

constexpr int kMaxLeaves = 8, kMaxDepth = 4;
constexpr int kMaxTreesPerLaunch = 8;     // trees of one instantiation share a grid
constexpr unsigned kMaxTreeBlocks = 4096;  // one-wave workgroups a tree's trips are strided over (the fold's grid)
constexpr int kOwnWgPerCu = 16;           // resident workgroups per CU when the library asks for none (the fold's 16)

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
__device__ __forceinline__ void ld_leaf(const void* p, const Place& at, bool live, w4& x, int& ex) {
    x = w4{0u, 0u, 0u, 0u};
    ex = 0;
    if (live) {
        x = ld16<VEC>(static_cast<const char*>(p) + at.codes());
        ex = ld_scale(static_cast<const char*>(p) + at.scale());
    }
}

// Workgroups [block0[s], block0[s] + nblk) evaluate tree s, striding over its trips.  A tile is read and written by
// one half-wave, every leaf's load before the root's store: `out` may alias any leaf at the same element offset.
template <int FMT, bool VEC>
__global__ __launch_bounds__(kWave) void k_mx_tree(TreeArgs a) {
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
                if (d == 2) combine<FMT>(s0, e0, s1, e1);
                else if (d == 3) combine<FMT>(s1, e1, s2, e2);
                else combine<FMT>(s2, e2, s3, e3);
            }
        }
        const uint32_t word = header_word(e0);
        if (live) st_tile<VEC>(out, at, s0, word);
    }
}

}  // namespace chr_mx

using namespace chr_mx;

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

// A tree the fold launcher evaluates in one launch with the same traffic: every leaf folds straight into one running
// value, in one operand order (csrc/user_ops.cpp chains those folds into one call).  Measured slower in one pass (the
// table above), so a call of nothing but such trees is declined.
bool single_fold(const chr_user_tree& t) {
    for (int j = 1; j < t.nleaves; ++j)
        if (t.comb[j] != 1 || t.swaps[j - 1] != t.swaps[0]) return false;
    return true;
}

bool tree_vec(const chr_user_tree& t) {
    uintptr_t al = bits_of(t.out);
    for (int j = 0; j < t.nleaves; ++j) al |= bits_of(t.leaves[j]);
    return (al & 15) == 0;
}

// The chr_user_tree_fn of format FMT.  Every tree of the call is checked before the first launch; a call with a tree
// the kernel does not take, on any dtype but a live tile type, or of single-fold trees alone is declined whole --
// nonzero, nothing enqueued -- and the library takes the folds.  Trees of one instantiation (16-B or 4-B accesses)
// share launches, kMaxTreesPerLaunch to a grid, each tree's workgroups contiguous.  A launch that fails is left to the
// caller's hipGetLastError.
template <int FMT>
int tree_launcher(const chr_user_tree* trees, int ntrees, chr_dtype dt, int wg_per_cu, hipStream_t stream) {
    ++g_calls;
    bool ok = ntrees > 0 && trees && is_tile_type(dt), pays = false;
    for (int t = 0; ok && t < ntrees; ++t) {
        ok = tree_ok(trees[t]);
        pays = pays || (ok && !single_fold(trees[t]));
    }
    if (!ok || !pays) {
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
            if (vec) hipLaunchKernelGGL((k_mx_tree<FMT, true>), dim3(grid), dim3(kWave), lds, stream, a);
            else hipLaunchKernelGGL((k_mx_tree<FMT, false>), dim3(grid), dim3(kWave), lds, stream, a);
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

std::mutex g_mu;
int g_op[2] = {-1, -1};  // the live op of each format; -1: not registered

}  // namespace

extern "C" {

// The launchers the ops are registered with (chiara_mx_tree.h declares them for direct calls).
int chr_mx_e4m3_sum_tree(const chr_user_tree* trees, int ntrees, chr_dtype dt, int wg_per_cu, hipStream_t stream, void*) {
    return tree_launcher<kE4M3>(trees, ntrees, dt, wg_per_cu, stream);
}
int chr_mx_e5m2_sum_tree(const chr_user_tree* trees, int ntrees, chr_dtype dt, int wg_per_cu, hipStream_t stream, void*) {
    return tree_launcher<kE5M2>(trees, ntrees, dt, wg_per_cu, stream);
}

int chr_mx_sum_tree(chr_fp8_format f, chr_op* op) {
    if (!op) return CHR_ERR_INVALID_ARG;
    if ((int)f != kE4M3 && (int)f != kE5M2) return CHR_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(g_mu);
    int& slot = g_op[(int)f];
    if (slot < 0) {
        chr_op code;
        const int rc = f == CHR_FP8_E4M3
                           ? chr_op_create_tree(chr_mx_e4m3_sum_fold, chr_mx_e4m3_sum_tree, nullptr, 1, &code)
                           : chr_op_create_tree(chr_mx_e5m2_sum_fold, chr_mx_e5m2_sum_tree, nullptr, 1, &code);
        if (rc) return rc;
        slot = (int)code;
    }
    *op = (chr_op)slot;
    return CHR_SUCCESS;
}

int chr_mx_tree_release(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = CHR_SUCCESS;
    for (int& c : g_op) {
        if (c < 0) continue;
        const int e = chr_op_free((chr_op)c);
        if (!rc) rc = e;
        c = -1;
    }
    return rc;
}

void chr_mx_tree_stats(long out[4], int reset) {
    if (out) {
        out[0] = g_calls;
        out[1] = g_declined;
        out[2] = g_trees;
        out[3] = g_kernels;
    }
    if (reset) g_calls = g_declined = g_trees = g_kernels = 0;
}

}  // extern "C"
