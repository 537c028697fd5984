/* chiara_user_op.hpp -- a chr_user_reduce_fn (chiara.h) from a device functor: the user-defined op's
 * arithmetic in the caller's own HIP code object, the way MPI_Op_create takes a function.
 *
 *   struct MyOp { __device__ float operator()(float in, float inout) const { return ...; } };  // in o inout
 *   CHR_DEFINE_USER_OP(my_op_launcher, float, MyOp)
 *   ...
 *   chr_op op;
 *   chr_op_create(my_op_launcher, nullptr, 0, &op);
 *   chr_allreduce_radix_batch(send, recv, count, CHR_FLOAT32, op, comm, k, b);
 *
 * The functor follows MPI's user-function convention: f(in, inout) returns the new inout (x o y = f(x, y)).  Build the
 * code object with the flags your arithmetic needs to be reproducible (e.g. -ffp-contract=off).
 *
 * The flat schedules' expression trees run fold by fold through that launcher.  A second one from the same functor
 * evaluates each tree in one HBM pass (chr_user_tree_fn; k_tree below):
 *
 *   CHR_DEFINE_USER_TREE(my_op_tree, float, MyOp)
 *   chr_op_create_tree(my_op_launcher, my_op_tree, nullptr, 0, &op);
 *
 * T is trivially copyable; 16-B vector accesses for T of 1, 2, 4, 8 or 16 bytes. */
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "chiara.h"

namespace chr_user {

constexpr int kMaxIns = 16;
#ifndef CHR_USER_FOLD_U
#define CHR_USER_FOLD_U 4
#endif
constexpr int kU = CHR_USER_FOLD_U;  // 16-B vectors per lane per trip of the fold kernel (1, 2, 8: within 2 %)

struct FoldArgs {
    void* out;
    const void* acc;
    const void* ins[kMaxIns];
    int m;
    size_t n;
    int running_first;
    int vec;  // every pointer 16-B aligned: 16-B vector loads and stores
};

// 16 bytes of T (T of 1, 2, 4, 8 or 16 bytes), or one T otherwise
template <typename T>
struct FoldVec {
    static constexpr int kN = (sizeof(T) <= 16 && 16 % sizeof(T) == 0) ? int(16 / sizeof(T)) : 1;
    T e[kN];
};

// out[i] = ins[m-1][i] o ( ... (ins[0][i] o acc[i])), or with running_first (((acc[i] o ins[0][i]) o ...).  Each
// element is read and written by one thread at one index, so `out` may alias `acc`.  HBM-bound streaming: 16-B
// vectors when every pointer allows it, kU of them per lane per trip in chunks of consecutive vectors (measured:
// 5.48 TB/s for m = 1 and 5.58 for m = 3 at 64 MiB against 5.21 / 5.37 for one vector per lane, grid-stride;
// non-temporal loads and stores made no difference, tools/userop_ab.sh), then the scalar tail.
template <typename T, typename F>
__global__ void k_fold(FoldArgs a) {
    using V = FoldVec<T>;
    constexpr int kN = V::kN;
    const F f{};
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t done = 0;
    if (kN > 1 && a.vec) {
        const size_t nv = a.n / kN;
        const V* accv = static_cast<const V*>(a.acc);
        V* outv = static_cast<V*>(a.out);
        // each workgroup takes chunks of kU x blockDim consecutive vectors (a wave's loads coalesced, a chunk's
        // pages shared), every load of a chunk issued before its combines: bytes in flight
        const size_t chunk = (size_t)kU * blockDim.x;
        const size_t nfull = nv / chunk;
        for (size_t c = blockIdx.x; c < nfull; c += gridDim.x) {
            const size_t base = c * chunk + threadIdx.x;
            V r[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) r[u] = accv[base + (size_t)u * blockDim.x];
            for (int j = 0; j < a.m; ++j) {
                const V* inv = static_cast<const V*>(a.ins[j]);
                V x[kU];
#pragma unroll
                for (int u = 0; u < kU; ++u) x[u] = inv[base + (size_t)u * blockDim.x];
#pragma unroll
                for (int u = 0; u < kU; ++u)
#pragma unroll
                    for (int e = 0; e < kN; ++e)
                        r[u].e[e] = a.running_first ? f(r[u].e[e], x[u].e[e]) : f(x[u].e[e], r[u].e[e]);
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) outv[base + (size_t)u * blockDim.x] = r[u];
        }
        for (size_t v = nfull * chunk + tid; v < nv; v += stride) {
            V r = accv[v];
            for (int j = 0; j < a.m; ++j) {
                const V x = static_cast<const V*>(a.ins[j])[v];
#pragma unroll
                for (int e = 0; e < kN; ++e) r.e[e] = a.running_first ? f(r.e[e], x.e[e]) : f(x.e[e], r.e[e]);
            }
            outv[v] = r;
        }
        done = nv * kN;
    }
    for (size_t i = done + tid; i < a.n; i += stride) {
        T r = static_cast<const T*>(a.acc)[i];
        for (int j = 0; j < a.m; ++j) {
            const T x = static_cast<const T*>(a.ins[j])[i];
            r = a.running_first ? f(r, x) : f(x, r);
        }
        static_cast<T*>(a.out)[i] = r;
    }
}

// Fan-in beyond kMaxIns runs as consecutive launches, each continuing from `out`.
template <typename T, typename F>
int launch_fold(void* out, const void* acc, const void* const* ins, int m, size_t n, int running_first,
                hipStream_t stream) {
    if (m < 0) return 1;
    const unsigned block = 256;
    auto aligned = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    bool vec = aligned(out) && aligned(acc);
    for (int j = 0; j < m; ++j) vec = vec && aligned(ins[j]);
    const size_t lanes = vec ? (n / FoldVec<T>::kN + kU - 1) / kU + n % FoldVec<T>::kN : n;
    const size_t blocks = (lanes + block - 1) / block;
    const unsigned grid = (unsigned)(blocks < 4096 ? (blocks ? blocks : 1) : 4096);
    int done = 0;
    const void* cur = acc;
    do {
        FoldArgs a{};
        a.out = out;
        a.acc = cur;
        a.m = m - done < kMaxIns ? m - done : kMaxIns;
        for (int j = 0; j < a.m; ++j) a.ins[j] = ins[done + j];
        a.n = n;
        a.running_first = running_first;
        a.vec = vec ? 1 : 0;
        hipLaunchKernelGGL((k_fold<T, F>), dim3(grid), dim3(block), 0, stream, a);
        if (hipGetLastError() != hipSuccess) return 1;
        done += a.m;
        cur = out;
    } while (done < m);
    return 0;
}

// ---- whole expression trees in one pass (chr_user_tree_fn, chr_op_create_tree) -----------------------------------
//
// One launch reads each leaf once and writes the root once, (NL + 1) * n * sizeof(T) bytes; fold by fold every
// inner node goes to HBM and comes back (C4's 8-leaf tree: 13 units against 9).  The program is a stack machine in
// post-order (chiara.h chr_user_tree): push leaf j, then comb[j] combines, each run = f(top, run), or with its swap
// bit run = f(run, top).  It is the same for every lane, so each push and combine is a scalar branch over four named
// stack slots (depth <= 4): an array indexed by the run-time depth would become scratch.
constexpr int kMaxLeaves = 8;
constexpr int kMaxTreesPerLaunch = 8;  // trees of equal leaf count share a grid
constexpr int kTreeBlock = 64;         // one-wave workgroups, as the library's streaming trees
// A leaf of more bytes than this is declined (the folds take it): below it a launch of 8 trees, one trip of at least
// 1 KiB per leaf per workgroup, stays under 2^31 workgroups.
constexpr size_t kMaxLeafBytes = (size_t)1 << 37;
constexpr uint32_t kMaxElementwiseBlocks = 4096;  // workgroups an element-wise tree strides over

// 16-B vectors per lane per trip: every leaf load of a trip is issued before the first combine, NL * U <= 8 loads of
// 16 B in flight per lane (the library's streaming shapes: csrc/reduce_tree.hpp tree_u).  8 leaves at U = 1 keep
// the f32 kernel inside the 72 VGPRs a kernel may hold beside RCCL's (tests/test_user_tree_resources.py).
template <int NL>
constexpr int tree_u() {
    return NL <= 2 ? 4 : NL <= 4 ? 2 : 1;
}
// Resident workgroups per CU when the library asks for none (wg_per_cu == 0): the library's own stand-alone policy.
// The f32 8-leaf tree, HBM-cold, 16 / 64 MiB leaves, fraction of 8 TB/s at 9 units (tools/userop_bench.py,
// profiles/r07/userop_tree/userop_bench.json, 2 alternating rounds): 12 per CU 0.694-0.695 / 0.755-0.758, 16 0.725 /
// 0.774-0.776, uncapped 0.719-0.721 / 0.767-0.768.  The 2-4 leaf shapes were not measured.
#ifndef CHR_USER_TREE_WG_PER_CU
#define CHR_USER_TREE_WG_PER_CU(NL) ((NL) <= 4 ? 12 : 16)
#endif

// Two knobs kept by measurement (same file, the --ab rows; builds: tests/userop/tree_op.mk ab).  Non-temporal leaf loads
// and root stores: 16 MiB leaves 0.642-0.646 -> 0.724-0.727, 64 MiB 0.684-0.686 -> 0.769-0.771, the 8-virtual-rank
// C4-shaped allreduce 1.260-1.276 -> 1.230-1.256 ms; cache-resident 1 MiB leaves within 5 %.  XCD runs -- workgroup b
// runs on XCD b % 8, and with runs each XCD takes this many KiB of consecutive trips of a tree before the next XCD's
// run instead of every eighth trip (the library's streaming trees: csrc/reduce_tree.hpp tree_xcd_run_kib) -- 256 KiB
// against none: 16 MiB 0.670 -> 0.724-0.727, 64 MiB 0.782-0.783 -> 0.769-0.771, C4 level inside the rounds' spread
// (1.214-1.240 without); 512 KiB 0.732 / 0.756-0.759 / 1.227-1.231 ms.  The runs pay for single slice-sized trees.
#ifndef CHR_USER_TREE_NT
#define CHR_USER_TREE_NT 1
#endif
#ifndef CHR_USER_TREE_XCD_RUN_KIB
#define CHR_USER_TREE_XCD_RUN_KIB 256
#endif

typedef unsigned int tree_w4 __attribute__((ext_vector_type(4)));
typedef unsigned int tree_w2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ tree_w4 tree_ld(const tree_w4* p) {
#if CHR_USER_TREE_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
__device__ __forceinline__ void tree_st(tree_w4* p, tree_w4 v) {
#if CHR_USER_TREE_NT
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

// A tree's workgroup `lb` of `nblk` -> its first trip, a bijection on [0, nblk).  A tree's first workgroup is a
// multiple of 8, so lb % 8 is the XCD: within each whole span of 8 runs, XCD x takes run x.
template <int TRIP_BYTES>
__device__ __forceinline__ uint32_t tree_trip(uint32_t lb, uint32_t nblk) {
    constexpr uint32_t R = (uint32_t)CHR_USER_TREE_XCD_RUN_KIB * 1024u / TRIP_BYTES;  // trips per run
    if constexpr (R > 1) {
        constexpr uint32_t span = 8 * R;
        if (lb < nblk / span * span) {
            const uint32_t w = lb % span;
            return lb - w + (w % 8) * R + w / 8;
        }
    }
    return lb;
}

struct TreeSeg {
    void* out;
    const void* leaves[kMaxLeaves];
    size_t n;
    uint32_t comb;   // 2 bits per leaf
    uint32_t swaps;  // 1 bit per combine, in program order
    uint32_t vec;    // out and every leaf 16-B aligned
    uint32_t nblk;   // this tree's workgroups
};
struct TreeArgs {
    uint32_t block0[kMaxTreesPerLaunch];  // each tree's first workgroup, ascending; ~0u past the last tree
    TreeSeg seg[kMaxTreesPerLaunch];
};

// The stack slots hold the operands as words -- a 16-B vector of T on the vector path, one T on the element-wise
// one -- and become T only inside a combine: slot selects on plain words stay register moves for any T.
template <typename T, bool ARITH = std::is_arithmetic<T>::value, size_t SZ = sizeof(T)>
struct TreeSlot { using S = T; };
template <typename T> struct TreeSlot<T, false, 4> { using S = uint32_t; };
template <typename T> struct TreeSlot<T, false, 8> { using S = tree_w2; };
template <typename T> struct TreeSlot<T, false, 16> { using S = tree_w4; };

template <typename T, typename F>
struct TreeApVec {  // in o run on the 16 / sizeof(T) elements of a vector
    using S = tree_w4;
    __device__ __forceinline__ static S ap(S in, S run) {
        using V = FoldVec<T>;
        const V x = __builtin_bit_cast(V, in);
        V r = __builtin_bit_cast(V, run);
        const F f{};
#pragma unroll
        for (int e = 0; e < V::kN; ++e) r.e[e] = f(x.e[e], r.e[e]);
        return __builtin_bit_cast(S, r);
    }
};
template <typename T, typename F>
struct TreeApOne {
    using S = typename TreeSlot<T>::S;
    __device__ __forceinline__ static S ap(S in, S run) {
        return __builtin_bit_cast(S, F{}(__builtin_bit_cast(T, in), __builtin_bit_cast(T, run)));
    }
};

template <typename A, int NL, int W>
__device__ __forceinline__ void tree_eval(const typename A::S (&x)[NL][W], typename A::S (&r)[W], uint32_t comb,
                                          uint32_t swaps) {
    using S = typename A::S;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        S s0 = x[0][w], s1 = s0, s2 = s0, s3 = s0;  // leaf 0 is pushed first and combines with nothing
        int d = 1, ci = 0;
#pragma unroll
        for (int j = 1; j < NL; ++j) {
            const S v = x[j][w];
            if (d == 1) s1 = v;
            else if (d == 2) s2 = v;
            else s3 = v;
            ++d;
            for (int c = (int)((comb >> (2 * j)) & 3u); c > 0; --c, ++ci) {
                // a swapped combine is the plain one on exchanged operands: select them, combine once
                const bool sw = (swaps >> ci) & 1u;
                if (d == 2) s0 = A::ap(sw ? s0 : s1, sw ? s1 : s0);
                else if (d == 3) s1 = A::ap(sw ? s1 : s2, sw ? s2 : s1);
                else s2 = A::ap(sw ? s2 : s3, sw ? s3 : s2);
                --d;
            }
        }
        r[w] = s0;
    }
}

template <typename T, typename F, int NL>
__device__ __forceinline__ void tree_one(const TreeSeg& g, size_t i) {
    using A = TreeApOne<T, F>;
    using S = typename A::S;
    S x[NL][1], r[1];
#pragma unroll
    for (int j = 0; j < NL; ++j) x[j][0] = __builtin_bit_cast(S, static_cast<const T*>(g.leaves[j])[i]);
    tree_eval<A, NL, 1>(x, r, g.comb, g.swaps);
    static_cast<T*>(g.out)[i] = __builtin_bit_cast(T, r[0]);
}

// Workgroups [block0[s], block0[s] + nblk) evaluate tree s.  Aligned trees: trips of BL * U consecutive 16-B vectors,
// one per workgroup, the trailing partial trip vector by vector, the elements past the last whole vector one per
// lane; any other tree element-wise, striding over its workgroups.  Every element is
// read and written by one lane, all its loads before its store: `out` may alias a leaf.  No LDS is touched: the
// launch's dynamic LDS only caps the workgroups resident per CU.
template <typename T, typename F, int NL, int U, int BL>
__global__ __launch_bounds__(BL) void k_tree(TreeArgs a) {
    using V = FoldVec<T>;
    constexpr int kN = V::kN;
    const uint32_t b = blockIdx.x;
    int s = 0;
#pragma unroll
    for (int j = 1; j < kMaxTreesPerLaunch; ++j)
        if (b >= a.block0[j]) s = j;
    const TreeSeg& g = a.seg[s];
    const uint32_t nblk = g.nblk;
    if (b - a.block0[s] >= nblk) return;  // the padding that starts the next tree on XCD 0
    const uint32_t lb = tree_trip<BL * U * 16>(b - a.block0[s], nblk);
    const size_t n = g.n;
    if constexpr (sizeof(V) == 16) if (g.vec) {
        using A = TreeApVec<T, F>;
        const size_t nvec = n / kN, nfull = nvec / ((size_t)BL * U);
        const uint32_t comb = g.comb, swaps = g.swaps;
        tree_w4* const out = static_cast<tree_w4*>(g.out);
        const tree_w4* lv[NL];
#pragma unroll
        for (int j = 0; j < NL; ++j) lv[j] = static_cast<const tree_w4*>(g.leaves[j]);
        if (lb < nfull) {
            const size_t base = (size_t)lb * BL * U + threadIdx.x;
            tree_w4 x[NL][U], r[U];
#pragma unroll
            for (int j = 0; j < NL; ++j)
#pragma unroll
                for (int u = 0; u < U; ++u) x[j][u] = tree_ld(&lv[j][base + (size_t)u * BL]);
            __builtin_amdgcn_sched_barrier(0);  // every load of the trip before its first combine
            tree_eval<A, NL, U>(x, r, comb, swaps);
#pragma unroll
            for (int u = 0; u < U; ++u) tree_st(&out[base + (size_t)u * BL], r[u]);
        }
        if (lb == nfull) {  // the partial trip: the launcher gave it a workgroup of its own
            for (size_t i = nfull * BL * U + threadIdx.x; i < nvec; i += BL) {
                tree_w4 x[NL][1], r[1];
#pragma unroll
                for (int j = 0; j < NL; ++j) x[j][0] = lv[j][i];
                tree_eval<A, NL, 1>(x, r, comb, swaps);
                out[i] = r[0];
            }
        }
        if (lb == 0 && nvec * kN + threadIdx.x < n) tree_one<T, F, NL>(g, nvec * kN + threadIdx.x);
        return;
    }
    for (size_t i = (size_t)lb * BL + threadIdx.x; i < n; i += (size_t)nblk * BL) tree_one<T, F, NL>(g, i);
}

// Dynamic LDS per workgroup that leaves room for `wg_per_cu` workgroups on a CU (0: none).
inline unsigned tree_lds_bytes(int wg_per_cu) {
    static const struct Lds {
        int cu = 0, blk = 0;
        Lds() {
            int dev = 0;
            if (hipGetDevice(&dev) != hipSuccess ||
                hipDeviceGetAttribute(&cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess ||
                hipDeviceGetAttribute(&blk, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess)
                cu = blk = 0;  // unknown: no cap
        }
    } lds;
    if (wg_per_cu <= 0 || lds.cu <= 0 || lds.blk <= 0) return 0;
    const unsigned bytes = ((unsigned)lds.cu / (unsigned)wg_per_cu) & ~255u;
    return bytes > (unsigned)lds.blk ? (unsigned)lds.blk & ~255u : bytes;
}

template <typename T, typename F, int NL>
void launch_tree_nl(const chr_user_tree* const* trees, int ntrees, int wg_per_cu, hipStream_t stream) {
    constexpr int U = tree_u<NL>(), BL = kTreeBlock;
    constexpr bool kVecT = sizeof(FoldVec<T>) == 16;
    const unsigned lds = tree_lds_bytes(wg_per_cu > 0 ? wg_per_cu : CHR_USER_TREE_WG_PER_CU(NL));
    auto aligned = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    for (int t0 = 0; t0 < ntrees; t0 += kMaxTreesPerLaunch) {
        TreeArgs a{};
        uint32_t grid = 0;
        for (int k = 0; k < kMaxTreesPerLaunch; ++k) {
            if (t0 + k >= ntrees) {
                a.block0[k] = ~0u;
                continue;
            }
            const chr_user_tree& t = *trees[t0 + k];
            TreeSeg& g = a.seg[k];
            g.out = t.out;
            bool vec = kVecT && aligned(t.out);
            int ci = 0;
            for (int j = 0; j < NL; ++j) {
                g.leaves[j] = t.leaves[j];
                vec = vec && aligned(t.leaves[j]);
                g.comb |= (uint32_t)(t.comb[j] & 3u) << (2 * j);
                for (int c = 0; c < t.comb[j] && ci < 8; ++c, ++ci) g.swaps |= (uint32_t)(t.swaps[ci] & 1u) << ci;
            }
            g.n = t.n;
            g.vec = vec ? 1 : 0;
            const size_t per = vec ? (size_t)BL * U * FoldVec<T>::kN : (size_t)BL;  // elements per workgroup trip
            const size_t want = (t.n + per - 1) / per;
            g.nblk = (uint32_t)(vec || want < kMaxElementwiseBlocks ? want : kMaxElementwiseBlocks);
            a.block0[k] = grid;
            grid += (g.nblk + 7u) & ~7u;  // the next tree starts on XCD 0 (tree_trip)
        }
        hipLaunchKernelGGL((k_tree<T, F, NL, U, BL>), dim3(grid), dim3(BL), lds, stream, a);
    }
}

// Every tree of the call, grouped by leaf count.  Returns nonzero -- declining, nothing enqueued -- for a tree the
// kernel does not take (leaf count outside 2..8, n == 0 or past kMaxLeafBytes, a program deeper than 4 or that does
// not end on one value);
// a launch that fails is left to the caller's hipGetLastError.
template <typename T, typename F>
int launch_tree(const chr_user_tree* trees, int ntrees, int wg_per_cu, hipStream_t stream) {
    if (ntrees < 0 || (ntrees && !trees)) return 1;
    for (int t = 0; t < ntrees; ++t) {
        const chr_user_tree& tr = trees[t];
        if (tr.nleaves < 2 || tr.nleaves > kMaxLeaves || tr.n == 0 || tr.n > kMaxLeafBytes / sizeof(T) ||
            !tr.out)
            return 1;
        int d = 0;
        for (int j = 0; j < tr.nleaves; ++j) {
            if (!tr.leaves[j] || ++d > 4 || tr.comb[j] > 3 || tr.comb[j] >= d) return 1;
            d -= tr.comb[j];
        }
        if (d != 1) return 1;
    }
    const chr_user_tree* grp[64];
    for (int nl = 2; nl <= kMaxLeaves; ++nl) {
        int k = 0;
        auto flush = [&] {
            if (k == 0) return;
            switch (nl) {
            case 2: launch_tree_nl<T, F, 2>(grp, k, wg_per_cu, stream); break;
            case 3: launch_tree_nl<T, F, 3>(grp, k, wg_per_cu, stream); break;
            case 4: launch_tree_nl<T, F, 4>(grp, k, wg_per_cu, stream); break;
            case 5: launch_tree_nl<T, F, 5>(grp, k, wg_per_cu, stream); break;
            case 6: launch_tree_nl<T, F, 6>(grp, k, wg_per_cu, stream); break;
            case 7: launch_tree_nl<T, F, 7>(grp, k, wg_per_cu, stream); break;
            default: launch_tree_nl<T, F, 8>(grp, k, wg_per_cu, stream); break;
            }
            k = 0;
        };
        for (int t = 0; t < ntrees; ++t)
            if (trees[t].nleaves == nl) {
                grp[k++] = &trees[t];
                if (k == 64) flush();
            }
        flush();
    }
    return 0;
}

}  // namespace chr_user

/* Defines `extern "C" int name(...)`, a chr_user_tree_fn for element type T from the same functor (the dtype argument
 * is not checked); register it beside the fold launcher: chr_op_create_tree(my_op_launcher, my_op_tree, ...). */
#define CHR_DEFINE_USER_TREE(name, T, F)                                                                             \
    extern "C" int name(const chr_user_tree* trees, int ntrees, chr_dtype, int wg_per_cu, hipStream_t stream,        \
                        void*) {                                                                                     \
        return chr_user::launch_tree<T, F>(trees, ntrees, wg_per_cu, stream);                                        \
    }

/* The same for one chr_dtype: a call on any other type is declined, and the library asks the fold launcher. */
#define CHR_DEFINE_USER_TREE_FOR(name, T, F, DTYPE)                                                                   \
    extern "C" int name(const chr_user_tree* trees, int ntrees, chr_dtype dt, int wg_per_cu, hipStream_t stream,     \
                        void*) {                                                                                     \
        if (dt != (DTYPE)) return 1;                                                                                 \
        return chr_user::launch_tree<T, F>(trees, ntrees, wg_per_cu, stream);                                        \
    }

/* Defines `extern "C" int name(...)`, a chr_user_reduce_fn for element type T (the dtype argument is not checked:
 * register it for the type it was built for). */
#define CHR_DEFINE_USER_OP(name, T, F)                                                                               \
    extern "C" int name(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype,             \
                        int running_first, hipStream_t stream, void*) {                                           \
        return chr_user::launch_fold<T, F>(out, acc, ins, m, n, running_first, stream);                           \
    }

/* The same for one chr_dtype: a call on any other type is refused (the library returns CHR_ERR_UNSUPPORTED), as an
 * MPI user function may reject a datatype it does not implement. */
#define CHR_DEFINE_USER_OP_FOR(name, T, F, DTYPE)                                                                     \
    extern "C" int name(void* out, const void* acc, const void* const* ins, int m, size_t n, chr_dtype dt,          \
                        int running_first, hipStream_t stream, void*) {                                           \
        if (dt != (DTYPE)) return 1;                                                                                 \
        return chr_user::launch_fold<T, F>(out, acc, ins, m, n, running_first, stream);                           \
    }
