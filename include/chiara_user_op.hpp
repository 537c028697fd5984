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
 * T is trivially copyable; 16-B vector accesses for T of 1, 2, 4, 8 or 16 bytes.  A T of any other size S -- the struct
 * a derived type (chr_type_contiguous) describes -- runs element-wise, or, at the sizes where that measured faster, in
 * element groups of lcm(S, 16) bytes: 16-B vectors again, whole elements per lane, a head of whole elements peeled
 * element-wise until every operand is 16-B aligned (operands congruent modulo 16; any other call element-wise).  The
 * size rule, the peel rule and the measured rows: "element groups" below. */
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
    int vec;  // every pointer 16-B aligned: 16-B vector loads and stores; a T in groups: 1 + the head elements
};

// 16 bytes of T (T of 1, 2, 4, 8 or 16 bytes), or one T otherwise
template <typename T>
struct FoldVec {
    static constexpr int kN = (sizeof(T) <= 16 && 16 % sizeof(T) == 0) ? int(16 / sizeof(T)) : 1;
    T e[kN];
};

typedef unsigned int tree_w4 __attribute__((ext_vector_type(4)));
typedef unsigned int tree_w2 __attribute__((ext_vector_type(2)));

// ---- packed combines for 1-byte elements -----------------------------------------------------------------------------
//
// A functor over a 1-byte T may also offer
//     static __device__ uint32_t packed(uint32_t in, uint32_t inout);
// the combine of the four elements of a word, byte k of the result being operator()(byte k of in, byte k of inout).  The
// vector loops of k_fold and the vector path of k_tree (TreeApVec) then call it once per word instead of operator()
// once per byte; the element-wise paths and the tails keep operator().  It is for arithmetic whose conversions come
// two or four to an instruction (libchiara_fp8.so: csrc/ops/fp8_ops.hip has the measurement).  Detected at compile
// time: a functor without it compiles exactly as before.
template <typename F>
struct HasPacked {
    template <typename G> static auto test(int) -> decltype(G::packed(0u, 0u), std::true_type{});
    template <typename G> static std::false_type test(...);
    static constexpr bool value = decltype(test<F>(0))::value;
};
template <typename T, typename F>
constexpr bool packed_vec() {
    return sizeof(T) == 1 && HasPacked<F>::value;
}
struct PackedWords { uint32_t w[4]; };  // a 16-B vector of 1-byte elements as words
// r = x o r, or with running_first r o x, on the 16 elements of a vector
template <typename V, typename F>
__device__ __forceinline__ void packed_fold(V& r, const V& x, bool running_first) {
    PackedWords rw = __builtin_bit_cast(PackedWords, r);
    const PackedWords xw = __builtin_bit_cast(PackedWords, x);
#pragma unroll
    for (int k = 0; k < 4; ++k)  // a swapped combine is the plain one on exchanged operands: select them, combine once
        rw.w[k] = F::packed(running_first ? rw.w[k] : xw.w[k], running_first ? xw.w[k] : rw.w[k]);
    r = __builtin_bit_cast(V, rw);
}

// ---- element groups: 16-B vectors for a T whose size S does not divide 16 (a derived type's struct) ---------------
//
// A lane's unit of work is a group of G = lcm(S, 16) bytes: V = G / 16 vectors holding E = G / S whole elements (S = 24:
// 3 vectors, 2 elements; 12: 3, 4; 32: 2, 1; 20: 5, 4; 6: 3, 8).  Groups are lane-contiguous: lane l of a wave takes
// group g0 + l, so a wave reads 64 * G consecutive bytes in V loads of 16 B per lane at a stride of G, every cache
// line it touches consumed whole by the same wave.  No LDS, no cross-lane exchange: an element never leaves its lane.
// S dividing 16 is FoldVec<T> above and is not a group (kWide false): those kernels are as they were.
//
// Alignment.  Chunk offsets are multiples of S, so operands are often congruent modulo 16 without being aligned
// (half of all 24-byte chunks start at 8 mod 16).  group_head finds the h < 16 / gcd(S, 16) whole head elements after
// which every pointer is 16-B aligned -- the same h for every operand, which is what congruent means; they run
// element-wise, then the groups, then the elements past the last whole group element-wise.  No such h (operands not
// congruent, or an address that is no multiple of gcd(S, 16)), or n < h: the whole call runs element-wise.
//
// Which sizes take the groups is a measurement (tools/userop_bench.py --struct, profiles/r08/struct_op/, RotMix of
// tests/userop/struct_op.hip, HBM-cold, 2 alternating rounds; groups against element-wise, and the f32 op at the
// same bytes).  The element-wise path was never one scalar per lane: a struct loads as dwordx2 / x3 / x4 pieces and a
// wave's elements are consecutive, while a group's loads stride by G, three times the cache lines per instruction at
// V = 3.  Folds at 64 MiB per operand, GB/s, m = 1 / m = 3 (f32: 5449-5478 / 5484-5497):
//   S = 12  4720-4781 / 5072-5085  against  5497-5504 / 5637-5647
//   S = 24  4911-4937 / 5202-5220  against  5309-5329 / 5462-5489
//   S = 32  5152-5173 / 5347-5366  against  5311-5314 / 5418-5429
//   S = 48  4938-5007 / 5253-5280  against  4718-4724 / 5084-5088
// 2-leaf trees at 16 / 64 MiB per leaf, fraction of 8 TB/s at 3 units (f32: 0.603-0.619 / 0.773-0.778):
//   S = 12  0.441-0.444 / 0.520-0.521  against  0.463 / 0.602-0.604
//   S = 24  0.444 / 0.520-0.522        against  0.525-0.533 / 0.605-0.607
//   S = 32  0.530-0.542 / 0.666-0.669  against  0.533 / 0.643
//   S = 48  0.443-0.444 / 0.519-0.523  against  0.513-0.514 / 0.611-0.612
// and S = 32 with 4 leaves 0.615-0.619 / 0.690-0.695 against 0.579-0.583 / 0.641-0.644.  So the folds take groups at
// 48 bytes and the trees at 32; every other size, measured or not, stays element-wise.
// CHR_USER_GROUP_VEC: 1 -- those sizes; 0 -- none (the A/B baseline); 2 -- every size that has groups (the other side
// of the A/B, and the build the tests run every shape through: tests/userop/struct_op.mk).
#ifndef CHR_USER_GROUP_VEC
#define CHR_USER_GROUP_VEC 1
#endif
constexpr bool group_fold_pays(size_t s) { return s == 48; }
constexpr bool group_tree_pays(size_t s) { return s == 32; }
constexpr size_t gcd16(size_t s) {
    size_t g = 16;
    while (s % g) g >>= 1;
    return g;
}
template <typename T>
struct Grp {
    static constexpr size_t S = sizeof(T), G = S / gcd16(S) * 16;
    static constexpr int V = int(G / 16), E = int(G / S), kHeads = int(16 / gcd16(S));
    static constexpr bool kWide = 16 % S != 0;
    // In flight per lane and operand: kU * V <= 8 vectors for a fold trip, NL * U * V <= 8 for a tree trip
    // (tree_u_for); a T of V > 8 has no vector path.  The trees also need whole words: unpacking the elements of a
    // 3- or 6-byte T out of every stack slot took the 2-leaf kernels to 104 and 88 VGPRs, past the 72 a wave has
    // beside RCCL.
    static constexpr bool kCan = kWide && V <= 8;
    static constexpr bool kFold = kCan && (CHR_USER_GROUP_VEC == 2 || (CHR_USER_GROUP_VEC == 1 && group_fold_pays(S)));
    static constexpr bool kTree =
        kCan && S % 4 == 0 && (CHR_USER_GROUP_VEC == 2 || (CHR_USER_GROUP_VEC == 1 && group_tree_pays(S)));
    static constexpr int kFoldU = !kFold ? 0 : 8 / V < kU ? 8 / V : kU;
};
template <int V> struct GrpW { tree_w4 w[V]; };        // a group as loaded and stored
template <typename T> struct GrpE { T e[Grp<T>::E]; };  // the same bytes as elements
// op(a's element, b's element) on the E elements of two groups.  An S that is a multiple of 4 reinterprets the
// group; any other S (3, 6: elements straddle the words) takes each element out of the words and puts the result back
// in shifts at compile-time offsets -- reinterpreting those goes through memory, a private segment.
template <typename T> struct GrpPad { T t; unsigned char pad[(sizeof(T) + 3) / 4 * 4 - sizeof(T)]; };
template <typename T, typename OP>
__device__ __forceinline__ GrpW<Grp<T>::V> grp_map(const GrpW<Grp<T>::V>& a, const GrpW<Grp<T>::V>& b, OP op) {
    constexpr int V = Grp<T>::V, E = Grp<T>::E;
    using W = GrpW<V>;
    if constexpr (sizeof(T) % 4 == 0) {
        const GrpE<T> ae = __builtin_bit_cast(GrpE<T>, a), be = __builtin_bit_cast(GrpE<T>, b);
        GrpE<T> re;
#pragma unroll
        for (int e = 0; e < E; ++e) re.e[e] = op(ae.e[e], be.e[e]);
        return __builtin_bit_cast(W, re);
    } else {
        constexpr int S = (int)sizeof(T), NT = (S + 3) / 4, NW = 4 * V;
        struct Words { uint32_t w[NW]; };
        struct Elem { uint32_t w[NT]; };
        const Words aw = __builtin_bit_cast(Words, a), bw = __builtin_bit_cast(Words, b);
        Words rw = {};
        auto get = [](const Words& g, int o) {  // the element at byte o
            Elem t;
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                const int q = o / 4 + k, sh = o % 4 * 8;
                uint32_t lo = g.w[q];
                if (sh) lo = (lo >> sh) | (q + 1 < NW ? g.w[q + 1] << (32 - sh) : 0u);
                t.w[k] = lo;
            }
            return __builtin_bit_cast(GrpPad<T>, t).t;
        };
#pragma unroll
        for (int e = 0; e < E; ++e) {
            GrpPad<T> p = {};
            p.t = op(get(aw, e * S), get(bw, e * S));
            const Elem t = __builtin_bit_cast(Elem, p);
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                const int nb = S - 4 * k < 4 ? S - 4 * k : 4, o = e * S + 4 * k, q = o / 4, sh = o % 4 * 8;
                const uint32_t v = nb == 4 ? t.w[k] : t.w[k] & ((1u << (8 * nb)) - 1u);
                rw.w[q] |= v << sh;
                if (sh && sh + 8 * nb > 32) rw.w[q + 1] |= v >> (32 - sh);
            }
        }
        return __builtin_bit_cast(W, rw);
    }
}

inline bool congruent16(const void* p, const void* q) { return (((uintptr_t)p ^ (uintptr_t)q) & 15) == 0; }
// The head elements before the groups of n elements at p (and at every pointer congruent to it), or -1: element-wise.
template <typename T>
inline int group_head(const void* p, size_t n) {
    for (int h = 0; h < Grp<T>::kHeads; ++h)
        if ((((uintptr_t)p + (uintptr_t)h * sizeof(T)) & 15) == 0) return (size_t)h <= n ? h : -1;
    return -1;
}

// The fold over groups (FoldArgs::vec = 1 + head elements): trips of kFoldU groups per lane, every load of an
// operand's trip issued before its combines, the partial trip group by group, head and tail elements one per lane.
template <typename T, typename F>
__device__ __forceinline__ void fold_groups(const FoldArgs& a) {
    constexpr int V = Grp<T>::V, E = Grp<T>::E, U = Grp<T>::kFoldU;
    using W = GrpW<V>;
    const F f{};
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t h = (size_t)a.vec - 1, ngrp = (a.n - h) / E, off = h * sizeof(T);
    const bool rf = a.running_first != 0;
    const W* accg = reinterpret_cast<const W*>(static_cast<const char*>(a.acc) + off);
    W* outg = reinterpret_cast<W*>(static_cast<char*>(a.out) + off);
    // a swapped combine is the plain one on exchanged operands: select them, combine once
    auto one = [&](T r, T x) { return f(rf ? r : x, rf ? x : r); };
    auto comb = [&](W& r, const W& x) { r = grp_map<T>(r, x, one); };
    const size_t chunk = (size_t)U * blockDim.x;
    const size_t nfull = ngrp / chunk;
    for (size_t c = blockIdx.x; c < nfull; c += gridDim.x) {
        const size_t base = c * chunk + threadIdx.x;
        W r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = accg[base + (size_t)u * blockDim.x];
        for (int j = 0; j < a.m; ++j) {
            const W* ing = reinterpret_cast<const W*>(static_cast<const char*>(a.ins[j]) + off);
            W x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = ing[base + (size_t)u * blockDim.x];
#pragma unroll
            for (int u = 0; u < U; ++u) comb(r[u], x[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) outg[base + (size_t)u * blockDim.x] = r[u];
    }
    for (size_t g = nfull * chunk + tid; g < ngrp; g += stride) {
        W r = accg[g];
        for (int j = 0; j < a.m; ++j)
            comb(r, reinterpret_cast<const W*>(static_cast<const char*>(a.ins[j]) + off)[g]);
        outg[g] = r;
    }
    const size_t tail0 = h + ngrp * E, extra = h + (a.n - tail0);  // fewer than kHeads + E elements
    for (size_t t = tid; t < extra; t += stride) {
        const size_t i = t < h ? t : tail0 + (t - h);
        T r = static_cast<const T*>(a.acc)[i];
        for (int j = 0; j < a.m; ++j) r = one(r, static_cast<const T*>(a.ins[j])[i]);
        static_cast<T*>(a.out)[i] = r;
    }
}

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
    if constexpr (Grp<T>::kFold) {
        if (a.vec) {
            fold_groups<T, F>(a);
            return;
        }
    }
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
                if constexpr (packed_vec<T, F>()) {
#pragma unroll
                    for (int u = 0; u < kU; ++u) packed_fold<V, F>(r[u], x[u], a.running_first != 0);
                } else {
#pragma unroll
                for (int u = 0; u < kU; ++u)
#pragma unroll
                    for (int e = 0; e < kN; ++e)
                        r[u].e[e] = a.running_first ? f(r[u].e[e], x[u].e[e]) : f(x[u].e[e], r[u].e[e]);
                }
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) outv[base + (size_t)u * blockDim.x] = r[u];
        }
        for (size_t v = nfull * chunk + tid; v < nv; v += stride) {
            V r = accv[v];
            for (int j = 0; j < a.m; ++j) {
                const V x = static_cast<const V*>(a.ins[j])[v];
                if constexpr (packed_vec<T, F>()) {
                    packed_fold<V, F>(r, x, a.running_first != 0);
                } else {
#pragma unroll
                for (int e = 0; e < kN; ++e) r.e[e] = a.running_first ? f(r.e[e], x.e[e]) : f(x.e[e], r.e[e]);
                }
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
    size_t lanes = vec ? (n / FoldVec<T>::kN + kU - 1) / kU + n % FoldVec<T>::kN : n;
    int head = -1;  // a T in groups: the head elements, the same for every launch of the call
    if constexpr (Grp<T>::kFold) {
        bool same = congruent16(out, acc);
        for (int j = 0; j < m; ++j) same = same && congruent16(out, ins[j]);
        if (same) head = group_head<T>(out, n);
        if (head >= 0)
            lanes = ((n - head) / Grp<T>::E + Grp<T>::kFoldU - 1) / Grp<T>::kFoldU + Grp<T>::kHeads + Grp<T>::E;
        else
            lanes = n;
    }
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
        a.vec = Grp<T>::kFold ? head + 1 : vec ? 1 : 0;
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
// The same rule for a T in groups of V vectors: NL * U * V <= 8, so U = 8 / (NL * V), at most tree_u<NL>().  0 -- the
// rule cannot be met even at U = 1 (8 leaves of 32 bytes; any V > 4), or T's trees take no groups (Grp<T>::kTree) --
// names the instantiation without a vector path: k_tree<T, F, NL, 0, BL> is element-wise only, so every k_tree symbol
// with U > 0 keeps the rule.
template <typename T, int NL>
constexpr int tree_u_for() {
    if (!Grp<T>::kWide) return tree_u<NL>();
    if (!Grp<T>::kTree) return 0;
    return 8 / (NL * Grp<T>::V) < tree_u<NL>() ? 8 / (NL * Grp<T>::V) : tree_u<NL>();
}
// What becomes of a tree of a T whose trees take groups when its leaf count breaks the rule: 1 -- the element-wise
// one-pass tree; 0 -- the call is declined (nothing enqueued) and the folds take it.  Measured on the 8-leaf tree of
// 24-byte elements at 16 MiB per leaf, fraction of 8 TB/s at 9 units (same file): declined to the folds 0.332-0.334,
// element-wise in one pass 0.608; the 8-virtual-rank C4-shaped allreduce of 128 MiB per rank with 24-byte elements
// 2.58-2.59 ms declined against 1.26-1.27 ms (the f32 op: 1.20-1.21 ms).  Element-wise is kept.
#ifndef CHR_USER_TREE_WIDE_ELEMENTWISE
#define CHR_USER_TREE_WIDE_ELEMENTWISE 1
#endif
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
        if constexpr (packed_vec<T, F>()) {  // four elements per call (packed combines, above)
            S r;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = F::packed(in[k], run[k]);
            return r;
        }
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
struct TreeApGrp {  // in o run on the E elements of a group
    using S = GrpW<Grp<T>::V>;
    __device__ __forceinline__ static S ap(const S& in, const S& run) {
        return grp_map<T>(in, run, [](const T& x, const T& r) { return F{}(x, r); });
    }
};
template <typename T, typename F>
struct TreeApOne {
    using S = typename TreeSlot<T>::S;
    __device__ __forceinline__ static S ap(S in, S run) {
        return __builtin_bit_cast(S, F{}(__builtin_bit_cast(T, in), __builtin_bit_cast(T, run)));
    }
};

// WIDE (a T in groups, whose slot is a whole group or a whole struct): after leaf j the stack is no deeper than j + 1,
// so a slot is not live before the leaf that can reach it, and a swapped combine is a wave-uniform branch -- selecting the operands of
// slots this size would copy both.
template <typename A, int NL, int W, bool WIDE = false>
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
            if constexpr (WIDE) {
                if (d == 1) s1 = v;
                else if (j > 1 && d == 2) s2 = v;
                else if (j > 2) s3 = v;
            } else {
                if (d == 1) s1 = v;
                else if (d == 2) s2 = v;
                else s3 = v;
            }
            ++d;
            for (int c = (int)((comb >> (2 * j)) & 3u); c > 0; --c, ++ci) {
                // a swapped combine is the plain one on exchanged operands: select them, combine once
                const bool sw = (swaps >> ci) & 1u;
                if constexpr (WIDE) {
                    if (j == 1 || d == 2) {
                        if (sw) s0 = A::ap(s0, s1);
                        else s0 = A::ap(s1, s0);
                    } else if (j == 2 || d == 3) {
                        if (sw) s1 = A::ap(s1, s2);
                        else s1 = A::ap(s2, s1);
                    } else {
                        if (sw) s2 = A::ap(s2, s3);
                        else s2 = A::ap(s3, s2);
                    }
                } else {
                    if (d == 2) s0 = A::ap(sw ? s0 : s1, sw ? s1 : s0);
                    else if (d == 3) s1 = A::ap(sw ? s1 : s2, sw ? s2 : s1);
                    else s2 = A::ap(sw ? s2 : s3, sw ? s3 : s2);
                }
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
    tree_eval<A, NL, 1, Grp<T>::kWide>(x, r, g.comb, g.swaps);
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
    constexpr int kTripBytes = U == 0 ? BL * (int)sizeof(T) : BL * U * 16 * (Grp<T>::kWide ? Grp<T>::V : 1);
    const uint32_t lb = tree_trip<kTripBytes>(b - a.block0[s], nblk);
    const size_t n = g.n;
    if constexpr (Grp<T>::kTree && U > 0) if (g.vec) {  // groups: g.vec = 1 + the head elements
        using A = TreeApGrp<T, F>;
        using W = typename A::S;
        constexpr int E = Grp<T>::E;
        const size_t h = g.vec - 1, ngrp = (n - h) / E, nfull = ngrp / ((size_t)BL * U), off = h * sizeof(T);
        const uint32_t comb = g.comb, swaps = g.swaps;
        W* const out = reinterpret_cast<W*>(static_cast<char*>(g.out) + off);
        const W* lv[NL];
#pragma unroll
        for (int j = 0; j < NL; ++j) lv[j] = reinterpret_cast<const W*>(static_cast<const char*>(g.leaves[j]) + off);
        if (lb < nfull) {
            const size_t base = (size_t)lb * BL * U + threadIdx.x;
            W x[NL][U], r[U];
#pragma unroll
            for (int j = 0; j < NL; ++j)
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int v = 0; v < Grp<T>::V; ++v) x[j][u].w[v] = tree_ld(&lv[j][base + (size_t)u * BL].w[v]);
            __builtin_amdgcn_sched_barrier(0);  // every load of the trip before its first combine
            tree_eval<A, NL, U, true>(x, r, comb, swaps);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int v = 0; v < Grp<T>::V; ++v) tree_st(&out[base + (size_t)u * BL].w[v], r[u].w[v]);
        }
        if (lb == nfull) {  // the partial trip, group by group
            for (size_t i = nfull * BL * U + threadIdx.x; i < ngrp; i += BL) {
                W x[NL][1], r[1];
#pragma unroll
                for (int j = 0; j < NL; ++j) x[j][0] = lv[j][i];
                tree_eval<A, NL, 1, true>(x, r, comb, swaps);
                out[i] = r[0];
            }
        }
        if (lb == 0) {  // the head elements and those past the last whole group: fewer than kHeads + E <= BL
            const size_t tail0 = h + ngrp * E, t = threadIdx.x;
            const size_t i = t < h ? t : tail0 + (t - h);
            if (i < n) tree_one<T, F, NL>(g, i);
        }
        return;
    }
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
    constexpr int U = tree_u_for<T, NL>(), BL = kTreeBlock;
    constexpr bool kVecT = sizeof(FoldVec<T>) == 16;
    constexpr bool kGrpT = Grp<T>::kTree && U > 0;
    static_assert(!kGrpT || Grp<T>::kHeads + Grp<T>::E <= BL, "head and tail elements: one lane each");
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
            size_t want = (t.n + per - 1) / per;
            if constexpr (kGrpT) {
                bool same = true;
                for (int j = 0; j < NL; ++j) same = same && congruent16(t.out, t.leaves[j]);
                const int head = same ? group_head<T>(t.out, t.n) : -1;
                if (head >= 0) {  // a trip is BL * U groups; block 0 also takes the head and tail elements
                    vec = true;
                    g.vec = 1u + (uint32_t)head;
                    const size_t ngrp = (t.n - head) / Grp<T>::E, trip = (size_t)BL * U;
                    want = ngrp < trip ? 1 : (ngrp + trip - 1) / trip;
                }
            }
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
        // a T whose trees take groups, with a leaf count that breaks the rule (tree_u_for): the folds take the call
        if (Grp<T>::kTree && !CHR_USER_TREE_WIDE_ELEMENTWISE && tr.nleaves * Grp<T>::V > 8) return 1;
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
