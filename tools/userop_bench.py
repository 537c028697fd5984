"""User-defined op (chr_op_create) against the predefined SUM on the same shapes.  One JSON line (and --out FILE).

 * the fold (MPI_Reduce_local, 64 MiB buckets, m = 1 and 3, HBM-cold rotation);
 * an 8-virtual-rank C4-shaped allreduce (k = 4, b = 4, the flat schedule's 8-leaf trees), 128 MiB per rank, in
   three variants: SUM (k_reduce_tree), the user op registered folds-only (chr_op_create: every tree as chained
   folds, user_ops.cpp user_tree) and the same op registered with its one-pass tree launcher (chr_op_create_tree,
   include/chiara_user_op.hpp k_tree);
 * the tree API alone (chr_reduce_tree, C4's 8-leaf program) at 16 MiB and 64 MiB per leaf over an HBM-cold rotation
   of ~2.25 GiB, the same three variants, as the fraction of 8 TB/s at 9 units of traffic (8 leaves read, the root
   written: what the one-pass kernels move; the folds move 13) -- and the tree launcher called directly at the
   residency caps 12, 16 and 64 workgroups per CU (64 is above the wave-slot limit: uncapped), the A/B behind
   CHR_USER_TREE_WG_PER_CU; and the same 8-leaf tree at 1 MiB per leaf on one cache-resident set.
 * --ab NAME=LIB.so adds the one-pass rows of another build of tests/userop/halfadd_tree_op.hip (make -C tests/userop -f tree_op.mk ab:
   its flags plus e.g. -DCHR_USER_TREE_NT=0 -DCHR_USER_TREE_XCD_RUN_KIB=0): the A/B of the kernel's policy knobs.

 * --struct: derived element types (chr_type_contiguous) of 12, 24, 32 and 48 bytes with tests/userop/struct_op.hip's
   RotMix beside the f32 op at the same bytes -- folds m = 1 and 3 at 64 MiB per operand, trees of 2 and 4 leaves at
   16 and 64 MiB per leaf (fraction of 8 TB/s at leaves + 1 units), the C4-shaped allreduce with f64 x 3 HalfAdd, and
   the 8-leaf f64 x 3 tree at 16 MiB per leaf, which the register rule keeps from the vector kernel -- each row once
   per build of struct_op.hip: the shipped one (groups at the sizes the header lists, every tree in one pass), grp0
   (CHR_USER_GROUP_VEC=0: element-wise, the behaviour before the groups) and all (groups at every size that has them,
   and the trees the register rule keeps from the vector kernel declined to the folds); make -C tests/userop -f
   struct_op.mk all ab.  Only these rows run.

 * --f16: the binary16 SUM of libchiara_ops.so (chiara_amd/ops.py, include/chiara_ops.h) beside the library's own
   bf16 SUM on the same bytes -- folds m = 1 and 3 at 64 MiB per operand, C4's 8-leaf tree at 16 and 64 MiB per leaf
   (fraction of 8 TB/s at 9 units) and the C4-shaped 8-virtual-rank allreduce at 128 MiB per rank.  Only these rows
   run.

 * --numerics: the struct ops of libchiara_numerics.so (chiara_amd/numerics.py, include/chiara_numerics.h) -- sum2 on
   float and double pairs (8 and 16 bytes) and moments on double records (24 bytes) -- each beside the library's f32
   SUM on the same bytes and tests/userop/struct_op.hip's RotMix of the same element size (f32 x 2, f32 x 4, f64 x 3,
   the shipped build): folds m = 1 and 3 at 64 MiB per operand, C4's 8-leaf tree at 16 and 64 MiB per leaf (fraction
   of 8 TB/s at 9 units) and the C4-shaped 8-virtual-rank allreduce at 128 MiB per rank.  Only these rows run.

 * --fp8: the OCP FP8 SUM of libchiara_fp8.so (chiara_amd/fp8.py, include/chiara_fp8.h) -- E4M3 under each overflow
   policy and E5M2 under IEEE -- beside the binary16 SUM of libchiara_ops.so on the same bytes: folds m = 1 and 3 at
   64 MiB per operand and C4's 8-leaf tree at 16 and 64 MiB per leaf (fraction of 8 TB/s at 9 units).  Only these rows
   run.  --fp8-perbyte LIB.so adds the same SUMs of a build without the packed combines (make fp8_ab).

 * --mx: the MXFP8 block-scaled SUM of libchiara_mx.so (chiara_amd/mx.py, include/chiara_mx.h), E4M3 and E5M2, beside
   the E4M3 SATURATE SUM of libchiara_fp8.so on the same bytes: folds m = 1 and 3 at the tile count nearest 64 MiB
   per operand (127 100 tiles of 528 bytes), GB/s against the (m + 2) x bytes of traffic, and the ratio to the FP8
   SUM; then trees of 2, 4 and 8 leaves (TREE_PROGS; the 8-leaf one is C4's) through chr_reduce_tree at the tile
   counts nearest 16 and 64 MiB per leaf (ms, and the fraction of 8 TB/s at leaves + 1 units) and the C4-shaped
   8-virtual-rank allreduce at 128 MiB per rank, each with the fold-only op (mx.mx_sum: C4's tree is three fold
   launches and 13 units) and the one-pass op of libchiara_mx_tree.so (mx.mx_sum_tree) back to back; and the E4M3
   tree launcher called directly on the 8-leaf tree at its own residency cap (wg_per_cu = 0), at 12 per CU and at 28.
   Only these rows run.

 * --mx4: the MXFP4 block-scaled SUM of libchiara_mx4.so (chiara_amd/mx4.py, include/chiara_mx4.h) beside the MX E4M3
   SUM of libchiara_mx.so on the same values: folds m = 1 and 3, in place, at 127 100 tiles per operand (272-byte
   tiles against 528-byte ones: half the bytes), each variant over an HBM-cold rotation of its own, as GB/s of its
   (m + 2) x bytes of traffic and as 10^9 values per second; then trees of 2, 4 and 8 leaves (TREE_PROGS; the 8-leaf
   one is C4's) through chr_reduce_tree at 31 775 and 127 100 tiles per leaf, the 8-leaf one also at 47 662, 63 550
   and 95 325, the sizes the launcher's size bound is read from (ms, and the fraction of 8 TB/s at leaves + 1
   units) and the C4-shaped 8-virtual-rank allreduce at 254 200 tiles per rank, each with the fold-only op
   (mx4.mx4_sum) and the one-pass op of libchiara_mx4_tree.so (mx4.mx4_sum_tree) back to back; and the tree launcher
   called directly on the 8-leaf tree at its own residency cap (wg_per_cu = 0), at 12 per CU and at 32, all the
   waves a CU holds.  The shipped launcher declines single-fold chains and trees beyond its size bound to the folds, so
   the one-pass tree rows and the direct launcher rows need --mx4-take-all LIB.so, a build that takes every tree (make
   mx4_tree_ab), registered here with libchiara_mx4.so's fold launcher; without it the tree rows run the shipped op,
   whose declined trees take the folds, and a direct launcher row whose tree the shipped launcher declines is
   recorded as null.  The allreduce rows always run the shipped op.  Between the fold rows and the tree rows come the
   sr_ rows (mx4_sr_rows): libchiara_mx4_sr.so's stochastic-rounding fold (mx4.mx4_sum_sr) beside the RNE MX4 fold, m = 1
   and 3 in place on one HBM-cold rotation, and mx4.quantize_sr beside mx4.quantize from f32, each as GB/s and as the
   SR / RNE ratio.  Only these rows run.

 * --mx6: the MXFP6 block-scaled SUMs of libchiara_mx6.so (chiara_amd/mx6.py, include/chiara_mx6.h), E2M3 and E3M2,
   beside the MX E4M3 SUM of libchiara_mx.so and the MX4 SUM of libchiara_mx4.so on the same kind of values: folds
   m = 1 and 3, in place, at 127 100 tiles per operand (400-byte tiles against 528- and 272-byte ones), each variant
   over an HBM-cold rotation of its own, the four variants alternating within each round, as GB/s of its
   (m + 2) x bytes of traffic and as 10^9 values per second.  Then, per format, trees of 2, 4 and 8 leaves (TREE_PROGS;
   the 8-leaf one is C4's) through chr_reduce_tree at 31 775 and 127 100 tiles per leaf, the 8-leaf one also at
   47 662, 63 550 and 95 325 (ms, and the fraction of 8 TB/s at leaves + 1 units), and the C4-shaped 8-virtual-rank
   allreduce at 254 200 tiles per rank, each with the fold-only op (mx6.mx6_sum) and the one-pass op of
   libchiara_mx6_tree.so (mx6.mx6_sum_tree) back to back; and the tree launcher called directly on the 8-leaf tree at
   its own residency cap (wg_per_cu = 0), at 12, 16 and 26 per CU, the most its LDS stack allows.  The shipped
   launchers decline single-fold chains to the folds, so the one-pass rows of the 2-leaf tree and the 4-leaf chain need
   --mx6-take-all LIB.so, a build that takes every tree (make mx6_tree_ab), registered here with libchiara_mx6.so's
   fold launchers; the allreduce rows always run the shipped ops.  Only these rows run.

 * --mxint8: the MXINT8 block-scaled SUM of libchiara_mxint8.so (chiara_amd/mxint8.py, include/chiara_mxint8.h) beside
   the MX E4M3 SUM of libchiara_mx.so, which moves the same 528-byte tiles: folds m = 1 and 3, in place, at 127 100
   tiles per operand, each variant over an HBM-cold rotation of its own, the variants alternating within each round,
   as GB/s of the (m + 2) x bytes of traffic and as 10^9 values per second, on two sets of data: `close`, tiles
   quantized from normal samples of one variance, where the gaps between block scales are small, and `wild`, random
   codes under scales 0, 1, 253, 254, 0xFF and 118 .. 136 with 1/8 zero blocks.  --mxint8-f32 LIB.so adds the fold of a
   build whose every combine is the f32 one (make mxint8_ab), the A/B of the integer combine.  Then, on both data
   sets, trees of 2, 4 and 8 leaves (TREE_PROGS; the 8-leaf one is C4's) through chr_reduce_tree at 31 775 and 127 100
   tiles per leaf, the 8-leaf one also at 47 662, 63 550 and 95 325 (ms, and the fraction of 8 TB/s at leaves + 1
   units), and the C4-shaped 8-virtual-rank allreduce at 254 200 tiles per rank on close data, each with the fold-only
   op (mxint8.mxint8_sum) and the one-pass op of libchiara_mxint8_tree.so (mxint8.mxint8_sum_tree) back to back; and
   the tree launcher called directly on the 8-leaf tree at its own residency cap (wg_per_cu = 0), at 12, 16 and 28 per
   CU.  The shipped launcher declines single-fold chains to the folds, so the one-pass rows of the 2-leaf tree and
   the 4-leaf chain need --mxint8-take-all LIB.so, a build that takes every tree (make mxint8_tree_ab), registered here
   with libchiara_mxint8.so's fold launcher; the allreduce rows always run the shipped op.  Only these rows run.

The C4 and tree rows run in --rounds alternating rounds in one process (variants interleaved within a round), each
shape warmed before its timed window.  Measurement tool; the user op is tests/userop/halfadd_tree_op.hip (one mul
+ one add per element, like SUM's one add); the fold rows keep tests/userop/halfadd_op.hip or CHR_USEROP_SO."""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "configurable-hierarchical-allreduce-algorithms_amd"))
import chiara_amd as ca  # noqa: E402

C4_COMB, C4_SWAPS = [0, 1, 1, 1, 0, 1, 1, 2], [0] * 7
HBM_PEAK = 8e12


class UserTree(ctypes.Structure):  # chiara.h chr_user_tree
    _fields_ = [("out", ctypes.c_void_p), ("leaves", ctypes.c_void_p * 8), ("nleaves", ctypes.c_int),
                ("comb", ctypes.c_ubyte * 8), ("swaps", ctypes.c_ubyte * 8), ("n", ctypes.c_size_t)]


def timed(fn, reps):
    for _ in range(3):
        fn(0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def fold_rows(out, dev, stream):
    lib = ctypes.CDLL(os.environ.get("CHR_USEROP_SO", os.path.join(REPO, "tests", "userop", "libhalfadd_op.so")))
    out["lib"] = os.path.basename(os.environ.get("CHR_USEROP_SO", "")) or "libhalfadd_op.so"
    half = ca.op_create(ctypes.cast(lib.chr_test_halfadd, ctypes.c_void_p).value)
    n = 16 << 20  # 64 MiB fp32
    for m in (1, 3):
        sets = max(1, (2 << 30) // ((m + 1) * 4 * n))
        bufs = [[torch.rand(n, device=dev) for _ in range(m + 1)] for _ in range(sets)]
        for name, op in (("sum", ca.SUM), ("user", half)):
            def go(i, op=op):
                s = bufs[i % sets]
                ca.check(ca.reduce_multi(s[0], s[0], s[1:], n, ca.FLOAT32, op, stream))
            ms = timed(go, 60)
            out[f"fold_m{m}_{name}_GBps"] = round((m + 2) * 4 * n / (ms * 1e-3) / 1e9, 1)
        del bufs
    ca.op_free(half)


def c4_rows(rounds, variants):
    """8-virtual-rank C4-shaped allreduce, 128 MiB per rank: ms per call, per round and variant."""
    dev = torch.device("cuda:0")
    nr, cnt = 8, 8 * (4 << 20)
    g = ca.LocalGroup(nr, 0)
    sends = [torch.rand(cnt, device=dev) for _ in range(nr)]
    recvs = [torch.empty(cnt, device=dev) for _ in range(nr)]
    rows = []
    for _ in range(rounds):
        row = {}
        for name, op in variants:
            for _ in range(2):
                ca.check(g.all_reduce_radix_batch(sends, recvs, cnt, ca.FLOAT32, op, 4, 4))
            torch.cuda.synchronize()  # device-wide: the group's own stream included
            t0 = time.perf_counter()
            for _ in range(5):
                ca.check(g.all_reduce_radix_batch(sends, recvs, cnt, ca.FLOAT32, op, 4, 4))
            torch.cuda.synchronize()
            row[f"localgroup8_k4b4_128MiB_{name}_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
        rows.append(row)
    g.destroy()
    return rows


def tree_rows(rounds, variants, tree_fn, stream):
    """chr_reduce_tree on C4's 8-leaf program, HBM-cold: fraction of 8 TB/s at 9 units, per round and variant."""
    dev = torch.device("cuda:0")
    rows = [{} for _ in range(rounds)]
    for mib in (1, 16, 64):
        n = mib << 18  # fp32 elements per leaf
        # 1 MiB leaves: one set, cache-resident (what a small collective's trees see); else the HBM-cold rotation
        sets = 1 if mib == 1 else int(2.25 * (1 << 30)) // (9 * 4 * n)
        bufs = [[torch.rand(n, device=dev) for _ in range(9)] for _ in range(sets)]
        trees = []
        for s in bufs:
            t = UserTree()
            t.out = s[8].data_ptr()
            for j in range(8):
                t.leaves[j] = s[j].data_ptr()
                t.comb[j] = C4_COMB[j]
            t.nleaves, t.n = 8, n
            trees.append(t)
        reps = {1: 400, 16: 240, 64: 80}[mib]
        for r in range(rounds):
            for name, op in variants:
                def go(i, op=op):
                    s = bufs[i % sets]
                    ca.check(ca.reduce_tree(s[8], s[:8], C4_COMB, C4_SWAPS, n, ca.FLOAT32, op, stream))
                ms = timed(go, reps)
                rows[r][f"tree8_{mib}MiB_{name}_frac"] = round(9 * 4 * n / (ms * 1e-3) / HBM_PEAK, 4)
            for cap in (12, 16, 64):
                def go(i, cap=cap):
                    if tree_fn(ctypes.byref(trees[i % sets]), 1, ca.FLOAT32, cap, stream.cuda_stream, None) != 0:
                        raise RuntimeError("tree launcher declined")
                ms = timed(go, reps)
                rows[r][f"tree8_{mib}MiB_launcher_cap{cap}_frac"] = round(9 * 4 * n / (ms * 1e-3) / HBM_PEAK, 4)
        del bufs, trees
    return rows


STRUCT_SHAPES = {"f32x3": (torch.float32, 3, ca.FLOAT32), "f64x3": (torch.float64, 3, ca.FLOAT64),
                 "f64x4": (torch.float64, 4, ca.FLOAT64), "f64x6": (torch.float64, 6, ca.FLOAT64)}
STRUCT_BUILDS = {"shipped": "libstruct_op.so", "grp0": "libstruct_op_grp0.so", "all": "libstruct_op_all.so"}
TREE_PROGS = {2: ([0, 1], [0]), 4: ([0, 1, 1, 1], [0, 0, 0]), 8: (C4_COMB, C4_SWAPS)}


def struct_rows(rounds, stream):
    """Rows of --struct, per round; every variant of a row is timed back to back within the round."""
    dev = torch.device("cuda:0")
    libs = {b: ctypes.CDLL(os.path.join(REPO, "tests", "userop", so)) for b, so in STRUCT_BUILDS.items()}
    tlib = ctypes.CDLL(os.path.join(REPO, "tests", "userop", "libhalfadd_tree_op.so"))

    def addr(lib, name):
        return ctypes.cast(getattr(lib, name), ctypes.c_void_p).value

    # (row label, element bytes, torch type, words per element, chr_dtype, {variant: op})
    shapes = [("f32", 4, torch.float32, 1, ca.FLOAT32,
               {"f32": ca.op_create(addr(tlib, "chr_test_halfadd"), tree=addr(tlib, "chr_test_halfadd_tree"))})]
    for shape, (tdt, k, base) in STRUCT_SHAPES.items():
        ops = {b: ca.op_create(addr(lib, f"chr_struct_RotMixK_{shape}"), tree=addr(lib, f"chr_struct_RotMixK_{shape}_tree"))
               for b, lib in libs.items()}
        shapes.append((shape, k * torch.empty(0, dtype=tdt).element_size(), tdt, k, ca.type_contiguous(k, base), ops))
    rows = [{} for _ in range(rounds)]
    for label, es, tdt, k, dt, ops in shapes:
        for what, units, mib, reps in ([("fold", m + 1, 64, 60) for m in (1, 3)] +
                                       [("tree", nl + 1, mib, 120 if mib == 16 else 60) for nl in (2, 4) for mib in (16, 64)] +
                                       ([("tree", 9, 16, 120)] if label == "f64x3" else [])):
            n = (mib << 20) // es
            sets = max(1, (2 << 30) // (units * n * es))
            bufs = [[torch.rand(n * k, device=dev, dtype=tdt) for _ in range(units)] for _ in range(sets)]
            for r in range(rounds):
                for variant, op in ops.items():
                    if what == "fold":  # acc in place, m inputs: m + 2 units of traffic
                        def go(i, op=op):
                            s = bufs[i % sets]
                            ca.check(ca.reduce_multi(s[0], s[0], s[1:], n, dt, op, stream))
                        ms = timed(go, reps)
                        rows[r][f"fold_m{units - 1}_64MiB_{label}_{variant}_GBps"] = round((units + 1) * n * es / ms / 1e6, 1)
                    else:
                        comb, swaps = TREE_PROGS[units - 1]

                        def go(i, op=op):
                            s = bufs[i % sets]
                            ca.check(ca.reduce_tree(s[-1], s[:-1], comb, swaps, n, dt, op, stream))
                        ms = timed(go, reps)
                        rows[r][f"tree{units - 1}_{mib}MiB_{label}_{variant}_frac"] = round(units * n * es / (ms * 1e-3) / HBM_PEAK, 4)
            del bufs
    # the C4-shaped allreduce, 128 MiB per rank, f64 x 3 HalfAdd against the f32 op
    nr, nbytes = 8, 128 << 20
    g = ca.LocalGroup(nr, 0)
    sends = [torch.rand(nbytes // 8, device=dev, dtype=torch.float64) for _ in range(nr)]
    recvs = [torch.empty(nbytes // 8, device=dev, dtype=torch.float64) for _ in range(nr)]
    dt24 = ca.type_contiguous(3, ca.FLOAT64)
    c4 = [("f32", ca.FLOAT32, nbytes // 4, shapes[0][5]["f32"])]
    for b, lib in libs.items():
        c4.append((f"f64x3_{b}", dt24, nbytes // 24 // nr * nr,
                   ca.op_create(addr(lib, "chr_struct_HalfAddK_f64x3"), tree=addr(lib, "chr_struct_HalfAddK_f64x3_tree"))))
    for r in range(rounds):
        for name, dt, cnt, op in c4:
            for _ in range(2):
                ca.check(g.all_reduce_radix_batch(sends, recvs, cnt, dt, op, 4, 4))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                ca.check(g.all_reduce_radix_batch(sends, recvs, cnt, dt, op, 4, 4))
            torch.cuda.synchronize()
            rows[r][f"localgroup8_k4b4_128MiB_{name}_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
    g.destroy()
    return rows


def f16_rows(rounds, stream):
    """Rows of --f16, per round: the library's bf16 SUM and libchiara_ops.so's f16 SUM back to back on the same
    buffers (2-byte elements either way; the bits are halves in [0, 1))."""
    from chiara_amd import ops

    dev = torch.device("cuda:0")
    variants = [("bf16_sum", ca.BFLOAT16, ca.SUM), ("f16_sum", ops.F16_DTYPE, ops.float16_op(ca.SUM))]
    rows = [{} for _ in range(rounds)]

    def halves(n):
        return torch.rand(n, device=dev).to(torch.float16)

    for what, units, mib, reps in ([("fold", m + 1, 64, 60) for m in (1, 3)] + [("tree", 9, 16, 240), ("tree", 9, 64, 80)]):
        n = (mib << 20) // 2
        sets = max(1, int(2.25 * (1 << 30)) // (units * 2 * n))
        bufs = [[halves(n) for _ in range(units)] for _ in range(sets)]
        for r in range(rounds):
            for name, dt, op in variants:
                if what == "fold":  # acc in place, m inputs: m + 2 units of traffic
                    def go(i, dt=dt, op=op):
                        s = bufs[i % sets]
                        ca.check(ca.reduce_multi(s[0], s[0], s[1:], n, dt, op, stream))
                    ms = timed(go, reps)
                    rows[r][f"fold_m{units - 1}_64MiB_{name}_GBps"] = round((units + 1) * 2 * n / ms / 1e6, 1)
                else:
                    def go(i, dt=dt, op=op):
                        s = bufs[i % sets]
                        ca.check(ca.reduce_tree(s[8], s[:8], C4_COMB, C4_SWAPS, n, dt, op, stream))
                    ms = timed(go, reps)
                    rows[r][f"tree8_{mib}MiB_{name}_frac"] = round(9 * 2 * n / (ms * 1e-3) / HBM_PEAK, 4)
        del bufs
    nr, cnt = 8, (128 << 20) // 2
    g = ca.LocalGroup(nr, 0)
    sends = [halves(cnt) for _ in range(nr)]
    recvs = [torch.empty(cnt, device=dev, dtype=torch.float16) for _ in range(nr)]
    for r in range(rounds):
        for name, dt, op in variants:
            for _ in range(2):
                ca.check(g.all_reduce_radix_batch(sends, recvs, cnt, dt, op, 4, 4))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                ca.check(g.all_reduce_radix_batch(sends, recvs, cnt, dt, op, 4, 4))
            torch.cuda.synchronize()
            rows[r][f"localgroup8_k4b4_128MiB_{name}_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
    g.destroy()
    ops.release()
    return rows


def fp8_rows(rounds, stream, perbyte=None):
    """Rows of --fp8, per round: libchiara_ops.so's f16 SUM and the FP8 SUMs back to back on the same buffers (the
    same bytes either way: every byte below 0x38, so E4M3 and E5M2 codes below 1 and halves below 0.5, every sum finite)."""
    from chiara_amd import fp8, ops

    dev = torch.device("cuda:0")
    variants = [("f16_sum", ops.F16_DTYPE, ops.float16_op(ca.SUM), 2),
                ("e4m3_sum_ieee", fp8.F8_DTYPE, fp8.fp8_op(fp8.E4M3, ca.SUM, fp8.IEEE), 1),
                ("e4m3_sum_sat", fp8.F8_DTYPE, fp8.fp8_op(fp8.E4M3, ca.SUM, fp8.SATURATE), 1),
                ("e5m2_sum_ieee", fp8.F8_DTYPE, fp8.fp8_op(fp8.E5M2, ca.SUM, fp8.IEEE), 1)]
    ab = None
    if perbyte:  # the same ops of a -DCHR_FP8_PACKED=0 build (make fp8_ab): the per-byte side of the packed A/B
        ab = ctypes.CDLL(os.path.abspath(perbyte))
        for name, fmt, o in (("e4m3_sum_ieee", fp8.E4M3, fp8.IEEE), ("e4m3_sum_sat", fp8.E4M3, fp8.SATURATE),
                             ("e5m2_sum_ieee", fp8.E5M2, fp8.IEEE)):
            code = ctypes.c_int(0)
            ca.check(ab.chr_fp8_op(fmt, ca.SUM, o, ctypes.byref(code)))
            variants.append((f"{name}_perbyte", fp8.F8_DTYPE, code.value, 1))
    rows = [{} for _ in range(rounds)]

    def codes(nbytes):
        return torch.randint(0, 0x38, (nbytes,), dtype=torch.uint8, device=dev)

    for what, units, mib, reps in ([("fold", m + 1, 64, 60) for m in (1, 3)] + [("tree", 9, 16, 240), ("tree", 9, 64, 80)]):
        nbytes = mib << 20
        sets = max(1, int(2.25 * (1 << 30)) // (units * nbytes))
        bufs = [[codes(nbytes) for _ in range(units)] for _ in range(sets)]
        for r in range(rounds):
            for name, dt, op, es in variants:
                n = nbytes // es
                if what == "fold":  # acc in place, m inputs: m + 2 units of traffic
                    def go(i, dt=dt, op=op, n=n):
                        s = bufs[i % sets]
                        ca.check(ca.reduce_multi(s[0], s[0], s[1:], n, dt, op, stream))
                    ms = timed(go, reps)
                    rows[r][f"fold_m{units - 1}_64MiB_{name}_GBps"] = round((units + 1) * nbytes / ms / 1e6, 1)
                else:
                    def go(i, dt=dt, op=op, n=n):
                        s = bufs[i % sets]
                        ca.check(ca.reduce_tree(s[8], s[:8], C4_COMB, C4_SWAPS, n, dt, op, stream))
                    ms = timed(go, reps)
                    rows[r][f"tree8_{mib}MiB_{name}_frac"] = round(9 * nbytes / (ms * 1e-3) / HBM_PEAK, 4)
        del bufs
    ops.release()
    fp8.release()
    if ab is not None:
        ab.chr_fp8_release()
    return rows


def mx_rows(rounds, stream):
    """Rows of --mx, per round: libchiara_fp8.so's E4M3 SATURATE SUM and the MX SUMs back to back on the same buffers:
    tiles quantized from normal samples, every block at a magnitude of its own (as FP8 codes the same bytes are
    finite values of any size; SATURATE keeps them so)."""
    from chiara_amd import fp8, mx

    dev = torch.device("cuda:0")
    tiles = round((64 << 20) / mx.TILE_BYTES)
    nbytes, nvals = tiles * mx.TILE_BYTES, tiles * mx.TILE_VALUES
    variants = [("fp8_e4m3_sum_sat", fp8.F8_DTYPE, fp8.fp8_op(fp8.E4M3, ca.SUM, fp8.SATURATE), nbytes),
                ("mx_e4m3_sum", mx.mx_type(), mx.mx_sum(fp8.E4M3), tiles),
                ("mx_e5m2_sum", mx.mx_type(), mx.mx_sum(fp8.E5M2), tiles)]
    rows = [{"tiles": tiles, "bytes_per_operand": nbytes} for _ in range(rounds)]

    def operand(tiles=tiles):
        nvals = tiles * mx.TILE_VALUES
        x = torch.randn(nvals // 32, 32, device=dev) * torch.exp2(torch.randint(-20, 21, (nvals // 32, 1), device=dev))
        t = torch.empty(tiles * mx.TILE_BYTES, dtype=torch.uint8, device=dev)
        ca.check(mx.quantize(t, x, nvals, ca.FLOAT32, fp8.E4M3, stream))
        return t

    for m in (1, 3):
        sets = max(1, int(2.25 * (1 << 30)) // ((m + 1) * nbytes))
        bufs = [[operand() for _ in range(m + 1)] for _ in range(sets)]
        torch.cuda.synchronize()
        for r in range(rounds):
            for name, dt, op, n in variants:
                def go(i, dt=dt, op=op, n=n):  # acc in place, m inputs: m + 2 units of traffic
                    s = bufs[i % sets]
                    ca.check(ca.reduce_multi(s[0], s[0], s[1:], n, dt, op, stream))
                ms = timed(go, 60)
                rows[r][f"fold_m{m}_64MiB_{name}_GBps"] = round((m + 2) * nbytes / ms / 1e6, 1)
            for f in ("e4m3", "e5m2"):
                rows[r][f"fold_m{m}_64MiB_mx_{f}_over_fp8"] = round(
                    rows[r][f"fold_m{m}_64MiB_mx_{f}_sum_GBps"] / rows[r][f"fold_m{m}_64MiB_fp8_e4m3_sum_sat_GBps"], 3)
        del bufs
    # C4's 8-leaf tree: the fold-only op against the one-pass op, interleaved within each round
    tile_t = mx.mx_type()
    pairs = [(f, (("folds", mx.mx_sum(c)), ("tree", mx.mx_sum_tree(c)))) for f, c in (("e4m3", fp8.E4M3), ("e5m2", fp8.E5M2))]
    launcher = mx.mx_tree_lib().chr_mx_e4m3_sum_tree
    launcher.argtypes = [ctypes.POINTER(UserTree), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    launcher.restype = ctypes.c_int
    for nl, mib, reps in [(nl, mib, reps) for nl in (2, 4, 8) for mib, reps in ((16, 240), (64, 80))]:
        comb, swaps = TREE_PROGS[nl]
        tt = round((mib << 20) / mx.TILE_BYTES)
        tb = tt * mx.TILE_BYTES
        sets = max(1, int(2.25 * (1 << 30)) // ((nl + 1) * tb))
        bufs = [[operand(tt) for _ in range(nl + 1)] for _ in range(sets)]
        trees = []
        for s in bufs:
            t = UserTree()
            t.out = s[nl].data_ptr()
            for j in range(nl):
                t.leaves[j] = s[j].data_ptr()
                t.comb[j] = comb[j]
            t.nleaves, t.n = nl, tt
            trees.append(t)
        torch.cuda.synchronize()
        for r in range(rounds):
            rows[r][f"tree_{mib}MiB_tiles"] = tt
            for f, ops in pairs:
                for name, op in ops:
                    def go(i, op=op):
                        s = bufs[i % sets]
                        ca.check(ca.reduce_tree(s[nl], s[:nl], comb, swaps, tt, tile_t, op, stream))
                    ms = timed(go, reps)
                    rows[r][f"tree{nl}_{mib}MiB_mx_{f}_{name}_ms"] = round(ms, 4)
                    rows[r][f"tree{nl}_{mib}MiB_mx_{f}_{name}_frac"] = round((nl + 1) * tb / (ms * 1e-3) / HBM_PEAK, 4)
            for cap in (0, 12, 28) if nl == 8 else ():  # 0: the launcher's own 16 per CU; 28: what the registers allow
                def go(i, cap=cap):
                    if launcher(ctypes.byref(trees[i % sets]), 1, tile_t, cap, stream.cuda_stream, None) != 0:
                        raise RuntimeError("tree launcher declined")
                ms = timed(go, reps)
                rows[r][f"tree8_{mib}MiB_mx_e4m3_launcher_cap{cap}_ms"] = round(ms, 4)
        del bufs, trees
    # the C4-shaped allreduce, 8 virtual ranks, the tile count nearest 128 MiB per rank
    nr = 8
    cnt = round((128 << 20) / mx.TILE_BYTES) // nr * nr
    g = ca.LocalGroup(nr, 0)
    sends = [operand(cnt) for _ in range(nr)]
    recvs = [torch.empty(cnt * mx.TILE_BYTES, dtype=torch.uint8, device=dev) for _ in range(nr)]
    for r in range(rounds):
        for f, ops in pairs:
            for name, op in ops:
                for _ in range(2):
                    ca.check(g.all_reduce_radix_batch(sends, recvs, cnt, tile_t, op, 4, 4))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(5):
                    ca.check(g.all_reduce_radix_batch(sends, recvs, cnt, tile_t, op, 4, 4))
                torch.cuda.synchronize()
                rows[r][f"localgroup8_k4b4_128MiB_mx_{f}_{name}_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
    g.destroy()
    fp8.release()
    mx.tree_release()
    mx.release()
    return rows


def mx4_rows(rounds, stream, take_all=None):
    """Rows of --mx4, per round: the MX E4M3 fold and the MX4 fold back to back, each on tiles quantized from the same
    kind of normal samples, every block at a magnitude of its own; then the tree rows (mx4_tree_rows)."""
    from chiara_amd import fp8, mx, mx4

    dev = torch.device("cuda:0")
    tiles = round((64 << 20) / mx.TILE_BYTES)  # 127 100
    nvals = tiles * mx.TILE_VALUES
    assert mx4.TILE_VALUES == mx.TILE_VALUES
    # (name, tile type, op, bytes per operand, quantize)
    variants = [("mx_e4m3_sum", mx.mx_type(), mx.mx_sum(fp8.E4M3), tiles * mx.TILE_BYTES,
                 lambda t, x: mx.quantize(t, x, nvals, ca.FLOAT32, fp8.E4M3, stream)),
                ("mx4_sum", mx4.mx4_type(), mx4.mx4_sum(), tiles * mx4.TILE_BYTES,
                 lambda t, x: mx4.quantize(t, x, nvals, ca.FLOAT32, stream))]
    rows = [{"tiles": tiles, "values_per_operand": nvals} for _ in range(rounds)]

    def operand(nbytes, quantize):
        x = torch.randn(nvals // 32, 32, device=dev) * torch.exp2(torch.randint(-20, 21, (nvals // 32, 1), device=dev))
        t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ca.check(quantize(t, x))
        return t

    for m in (1, 3):
        bufs = {name: [[operand(nbytes, q) for _ in range(m + 1)] for _ in range(max(1, int(2.25 * (1 << 30)) // ((m + 1) * nbytes)))]
                for name, _, _, nbytes, q in variants}
        torch.cuda.synchronize()
        for r in range(rounds):
            for name, dt, op, nbytes, _ in variants:
                def go(i, dt=dt, op=op, sets=bufs[name]):  # acc in place, m inputs: m + 2 units of traffic
                    s = sets[i % len(sets)]
                    ca.check(ca.reduce_multi(s[0], s[0], s[1:], tiles, dt, op, stream))
                ms = timed(go, 60)
                rows[r][f"fold_m{m}_{name}_bytes_per_operand"] = nbytes
                rows[r][f"fold_m{m}_{name}_GBps"] = round((m + 2) * nbytes / ms / 1e6, 1)
                rows[r][f"fold_m{m}_{name}_Gvalues_per_s"] = round(nvals / ms / 1e6, 2)
            for unit in ("GBps", "Gvalues_per_s"):
                rows[r][f"fold_m{m}_mx4_over_mx_e4m3_{unit}"] = round(
                    rows[r][f"fold_m{m}_mx4_sum_{unit}"] / rows[r][f"fold_m{m}_mx_e4m3_sum_{unit}"], 3)
        del bufs
    mx.release()
    mx4_sr_rows(rows, stream)
    mx4_tree_rows(rows, stream, take_all)
    mx4.release()
    return rows


def mx4_sr_rows(rows, stream):
    """The SR rows of --mx4, into rows[r]: libchiara_mx4_sr.so's fold beside the RNE MX4 fold, m = 1 and 3 in place on
    one HBM-cold rotation, alternating within each round; then quantize_sr beside quantize from f32 (read 4 bytes and
    write 17 / 32 of a byte per value)."""
    from chiara_amd import mx4

    dev = torch.device("cuda:0")
    tiles = rows[0]["tiles"]
    nvals, nbytes = tiles * mx4.TILE_VALUES, tiles * mx4.TILE_BYTES
    tile_t = mx4.mx4_type()
    ops = (("mx4_sum", mx4.mx4_sum()), ("mx4_sum_sr", mx4.mx4_sum_sr()))

    def source():
        return torch.randn(nvals // 32, 32, device=dev) * torch.exp2(torch.randint(-20, 21, (nvals // 32, 1), device=dev))

    def operand():
        t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ca.check(mx4.quantize(t, source(), nvals, ca.FLOAT32, stream))
        return t

    for m in (1, 3):
        sets = [[operand() for _ in range(m + 1)] for _ in range(max(1, int(2.25 * (1 << 30)) // ((m + 1) * nbytes)))]
        torch.cuda.synchronize()
        for r, row in enumerate(rows):
            mx4.sr_set_seed(r + 1)
            for name, op in ops:
                def go(i, op=op):  # acc in place, m inputs: m + 2 units of traffic
                    s = sets[i % len(sets)]
                    ca.check(ca.reduce_multi(s[0], s[0], s[1:], tiles, tile_t, op, stream))
                row[f"sr_fold_m{m}_{name}_GBps"] = round((m + 2) * nbytes / timed(go, 60) / 1e6, 1)
            row[f"sr_fold_m{m}_sr_over_rne"] = round(row[f"sr_fold_m{m}_mx4_sum_sr_GBps"] / row[f"sr_fold_m{m}_mx4_sum_GBps"], 3)
        del sets
    pairs = [(source(), torch.empty(nbytes, dtype=torch.uint8, device=dev)) for _ in range(max(1, int(2.25 * (1 << 30)) // (4 * nvals + nbytes)))]
    torch.cuda.synchronize()
    for r, row in enumerate(rows):
        for name, q in (("quantize", lambda t, x: mx4.quantize(t, x, nvals, ca.FLOAT32, stream)),
                        ("quantize_sr", lambda t, x: mx4.quantize_sr(t, x, nvals, ca.FLOAT32, r + 1, stream))):
            def go(i, q=q):
                x, t = pairs[i % len(pairs)]
                ca.check(q(t, x))
            row[f"sr_{name}_f32_GBps"] = round((4 * nvals + nbytes) / timed(go, 60) / 1e6, 1)
        row["sr_quantize_f32_sr_over_rne"] = round(row["sr_quantize_sr_f32_GBps"] / row["sr_quantize_f32_GBps"], 3)
    del pairs
    mx4.sr_set_seed(0)
    mx4.sr_release()


def mx6_rows(rounds, stream, take_all=None):
    """Rows of --mx6, per round: the MX E4M3, MX4, MX6 E2M3 and MX6 E3M2 folds back to back, each on tiles quantized
    from the same kind of normal samples, every block at a magnitude of its own; then the tree rows (mx6_tree_rows)."""
    from chiara_amd import fp8, mx, mx4, mx6

    dev = torch.device("cuda:0")
    tiles = round((64 << 20) / mx.TILE_BYTES)  # 127 100
    nvals = tiles * mx.TILE_VALUES
    assert mx6.TILE_VALUES == mx4.TILE_VALUES == mx.TILE_VALUES
    # (name, tile type, op, bytes per operand, quantize)
    variants = [("mx_e4m3_sum", mx.mx_type(), mx.mx_sum(fp8.E4M3), tiles * mx.TILE_BYTES,
                 lambda t, x: mx.quantize(t, x, nvals, ca.FLOAT32, fp8.E4M3, stream)),
                ("mx4_sum", mx4.mx4_type(), mx4.mx4_sum(), tiles * mx4.TILE_BYTES,
                 lambda t, x: mx4.quantize(t, x, nvals, ca.FLOAT32, stream))]
    variants += [(f"mx6_{name}_sum", mx6.mx6_type(), mx6.mx6_sum(fmt), tiles * mx6.TILE_BYTES,
                  lambda t, x, fmt=fmt: mx6.quantize(t, x, nvals, ca.FLOAT32, fmt, stream))
                 for name, fmt in (("e2m3", mx6.E2M3), ("e3m2", mx6.E3M2))]
    rows = [{"tiles": tiles, "values_per_operand": nvals} for _ in range(rounds)]

    def operand(nbytes, quantize):
        x = torch.randn(nvals // 32, 32, device=dev) * torch.exp2(torch.randint(-20, 21, (nvals // 32, 1), device=dev))
        t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ca.check(quantize(t, x))
        return t

    for m in (1, 3):
        bufs = {name: [[operand(nbytes, q) for _ in range(m + 1)] for _ in range(max(1, int(2.25 * (1 << 30)) // ((m + 1) * nbytes)))]
                for name, _, _, nbytes, q in variants}
        torch.cuda.synchronize()
        for r in range(rounds):
            for name, dt, op, nbytes, _ in variants:
                def go(i, dt=dt, op=op, sets=bufs[name]):  # acc in place, m inputs: m + 2 units of traffic
                    s = sets[i % len(sets)]
                    ca.check(ca.reduce_multi(s[0], s[0], s[1:], tiles, dt, op, stream))
                ms = timed(go, 60)
                rows[r][f"fold_m{m}_{name}_bytes_per_operand"] = nbytes
                rows[r][f"fold_m{m}_{name}_GBps"] = round((m + 2) * nbytes / ms / 1e6, 1)
                rows[r][f"fold_m{m}_{name}_Gvalues_per_s"] = round(nvals / ms / 1e6, 2)
            for name in ("mx6_e2m3", "mx6_e3m2"):
                rows[r][f"fold_m{m}_{name}_over_mx_e4m3_Gvalues_per_s"] = round(
                    rows[r][f"fold_m{m}_{name}_sum_Gvalues_per_s"] / rows[r][f"fold_m{m}_mx_e4m3_sum_Gvalues_per_s"], 3)
        del bufs
    mx.release()
    mx4.release()
    mx6_tree_rows(rows, stream, take_all)
    mx6.release()
    return rows


def mx6_tree_rows(rows, stream, take_all=None):
    """The tree rows of --mx6, into rows[r], per format: the fold-only op and the one-pass op interleaved within each
    round, on the fold rows' kind of data."""
    from chiara_amd import mx6

    dev = torch.device("cuda:0")
    tile_t = mx6.mx6_type()
    fptr = lambda L, name: ctypes.cast(getattr(L, name), ctypes.c_void_p).value
    ab = ctypes.CDLL(os.path.abspath(take_all)) if take_all else None  # a -DCHR_MX6_TREE_TAKE_ALL=1 build (make mx6_tree_ab)

    def operand(fmt, tiles):
        nvals = tiles * mx6.TILE_VALUES
        x = torch.randn(nvals // 32, 32, device=dev) * torch.exp2(torch.randint(-20, 21, (nvals // 32, 1), device=dev))
        t = torch.empty(tiles * mx6.TILE_BYTES, dtype=torch.uint8, device=dev)
        ca.check(mx6.quantize(t, x, nvals, ca.FLOAT32, fmt, stream))
        return t

    shapes = [(nl, tt, reps) for nl in (2, 4, 8) for tt, reps in ((31775, 240), (127100, 80))]
    shapes += [(8, 47662, 160), (8, 63550, 120), (8, 95325, 100)]  # --mx4's sizes between the two
    for fname, fmt in (("e2m3", mx6.E2M3), ("e3m2", mx6.E3M2)):
        taken = mx6.mx6_sum_tree(fmt)
        launcher, tree_op = getattr(ab or mx6.mx6_tree_lib(), f"chr_mx6_{fname}_sum_tree_launch"), taken
        if ab:  # the same kernels, nothing declined for speed
            tree_op = ca.op_create(fptr(mx6.mx6_lib(), f"chr_mx6_{fname}_sum_fold"), commute=True,
                                   tree=fptr(ab, f"chr_mx6_{fname}_sum_tree_launch"))
        launcher.argtypes = [ctypes.POINTER(UserTree), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        launcher.restype = ctypes.c_int
        for nl, tt, reps in shapes:
            comb, swaps = TREE_PROGS[nl]
            tb = tt * mx6.TILE_BYTES
            sets = max(1, int(2.25 * (1 << 30)) // ((nl + 1) * tb))
            bufs = [[operand(fmt, tt) for _ in range(nl + 1)] for _ in range(sets)]
            trees = []
            for s in bufs:
                t = UserTree()
                t.out = s[nl].data_ptr()
                for j in range(nl):
                    t.leaves[j] = s[j].data_ptr()
                    t.comb[j] = comb[j]
                t.nleaves, t.n = nl, tt
                trees.append(t)
            torch.cuda.synchronize()
            for r in range(len(rows)):
                for name, op in (("folds", mx6.mx6_sum(fmt)), ("tree", tree_op)):
                    def go(i, op=op):
                        s = bufs[i % sets]
                        ca.check(ca.reduce_tree(s[nl], s[:nl], comb, swaps, tt, tile_t, op, stream))
                    ms = timed(go, reps)
                    rows[r][f"{fname}_tree{nl}_{tt}tiles_mx6_{name}_ms"] = round(ms, 4)
                    rows[r][f"{fname}_tree{nl}_{tt}tiles_mx6_{name}_frac"] = round((nl + 1) * tb / (ms * 1e-3) / HBM_PEAK, 4)
                # 0: the launcher's own 16 per CU; 12: what the library asks for beside RCCL; 26: all the LDS stack allows
                for cap in (0, 12, 16, 26) if nl == 8 and tt in (31775, 127100) else ():
                    def go(i, cap=cap):
                        return launcher(ctypes.byref(trees[i % sets]), 1, tile_t, cap, stream.cuda_stream, None)
                    took = go(0) == 0  # a launcher that declines has enqueued nothing: the row is null
                    rows[r][f"{fname}_tree8_{tt}tiles_mx6_launcher_cap{cap}_ms"] = round(timed(go, reps), 4) if took else None
            del bufs, trees
        # the C4-shaped allreduce, 8 virtual ranks, 2 x 127 100 tiles per rank (eight 31 775-tile trees to a call)
        nr, cnt = 8, 254200
        g = ca.LocalGroup(nr, 0)
        sends = [operand(fmt, cnt) for _ in range(nr)]
        recvs = [torch.empty(cnt * mx6.TILE_BYTES, dtype=torch.uint8, device=dev) for _ in range(nr)]
        for r in range(len(rows)):
            for name, op in (("folds", mx6.mx6_sum(fmt)), ("tree", taken)):
                for _ in range(2):
                    ca.check(g.all_reduce_radix_batch(sends, recvs, cnt, tile_t, op, 4, 4))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(5):
                    ca.check(g.all_reduce_radix_batch(sends, recvs, cnt, tile_t, op, 4, 4))
                torch.cuda.synchronize()
                rows[r][f"{fname}_localgroup8_k4b4_{cnt}tiles_mx6_{name}_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
        g.destroy()
        del sends, recvs
        if ab:
            ca.op_free(tree_op)
    mx6.tree_release()


def mx8_operand(data, tiles, quantize):
    """`tiles` 528-byte tiles of --mxint8's data set `data`: close, quantize(t, x) of normal samples of one variance;
    wild, random codes under scales 0, 1, 253, 254, 0xFF and 118 .. 136 with 1/8 zero blocks."""
    dev = torch.device("cuda:0")
    if data == "close":
        t = torch.empty(tiles * 528, dtype=torch.uint8, device=dev)
        ca.check(quantize(t, torch.randn(tiles * 512, device=dev)))
        return t
    pool = torch.tensor([0, 0, 1, 254, 254, 253, 0xFF] + list(range(118, 137)), dtype=torch.uint8, device=dev)
    codes = torch.randint(0, 256, (tiles, 16, 32), dtype=torch.uint8, device=dev)
    codes[torch.randint(0, 8, (tiles, 16), device=dev) == 0] = 0
    scales = pool[torch.randint(0, pool.numel(), (tiles, 16), device=dev)]
    return torch.cat([scales, codes.view(tiles, 512)], dim=1).reshape(-1)


def mxint8_rows(rounds, stream, f32_lib=None, take_all=None):
    """Rows of --mxint8, per round and data set: the MX E4M3 fold, the MXINT8 fold and (f32_lib) the f32-only build's
    fold back to back; then the tree rows (mxint8_tree_rows)."""
    from chiara_amd import fp8, mx, mxint8

    dev = torch.device("cuda:0")
    tiles = round((64 << 20) / mx.TILE_BYTES)  # 127 100
    nvals, nbytes = tiles * mx.TILE_VALUES, tiles * mx.TILE_BYTES
    assert (mxint8.TILE_VALUES, mxint8.TILE_BYTES) == (mx.TILE_VALUES, mx.TILE_BYTES)
    # (name, tile type, op, quantize)
    q8 = lambda t, x: mxint8.quantize(t, x, nvals, ca.FLOAT32, stream)
    variants = [("mx_e4m3_sum", mx.mx_type(), mx.mx_sum(fp8.E4M3), lambda t, x: mx.quantize(t, x, nvals, ca.FLOAT32, fp8.E4M3, stream)),
                ("mxint8_sum", mxint8.mxint8_type(), mxint8.mxint8_sum(), q8)]
    ab_op = None
    if f32_lib:  # a -DCHR_MXI8_INT=0 build (make mxint8_ab): the same kernels without the integer combine
        ab = ctypes.CDLL(os.path.abspath(f32_lib))
        ab_op = ca.op_create(ctypes.cast(ab.chr_mxi8_sum_fold, ctypes.c_void_p).value, commute=True)
        variants.append(("mxint8_f32_sum", mxint8.mxint8_type(), ab_op, q8))
    rows = [{"tiles": tiles, "values_per_operand": nvals, "bytes_per_operand": nbytes} for _ in range(rounds)]
    for data in ("close", "wild"):
        for m in (1, 3):
            nsets = max(1, int(2.25 * (1 << 30)) // ((m + 1) * nbytes))
            bufs = {name: [[mx8_operand(data, tiles, q) for _ in range(m + 1)] for _ in range(nsets)]
                    for name, _, _, q in variants}
            torch.cuda.synchronize()
            for r in range(rounds):
                for name, dt, op, _ in variants:
                    def go(i, dt=dt, op=op, sets=bufs[name]):  # acc in place, m inputs: m + 2 units of traffic
                        s = sets[i % len(sets)]
                        ca.check(ca.reduce_multi(s[0], s[0], s[1:], tiles, dt, op, stream))
                    ms = timed(go, 60)
                    rows[r][f"{data}_fold_m{m}_{name}_GBps"] = round((m + 2) * nbytes / ms / 1e6, 1)
                    rows[r][f"{data}_fold_m{m}_{name}_Gvalues_per_s"] = round(nvals / ms / 1e6, 2)
                for name, _, _, _ in variants[1:]:
                    rows[r][f"{data}_fold_m{m}_{name[:-4]}_over_mx_e4m3"] = round(
                        rows[r][f"{data}_fold_m{m}_{name}_GBps"] / rows[r][f"{data}_fold_m{m}_mx_e4m3_sum_GBps"], 3)
            del bufs
    if ab_op is not None:
        ca.op_free(ab_op)
    mx.release()
    mxint8_tree_rows(rows, stream, take_all)
    mxint8.release()
    return rows


def mxint8_tree_rows(rows, stream, take_all=None):
    """The tree rows of --mxint8, into rows[r]: the fold-only op and the one-pass op interleaved within each round."""
    from chiara_amd import mxint8

    dev = torch.device("cuda:0")
    tile_t = mxint8.mxint8_type()
    fptr = lambda L, name: ctypes.cast(getattr(L, name), ctypes.c_void_p).value
    taken = mxint8.mxint8_sum_tree()
    launcher, tree_op = mxint8.mxint8_tree_lib().chr_mxi8_sum_tree_launch, taken
    if take_all:  # a -DCHR_MXI8_TREE_TAKE_ALL=1 build (make mxint8_tree_ab): the same kernels, nothing declined for speed
        ab = ctypes.CDLL(os.path.abspath(take_all))
        launcher = ab.chr_mxi8_sum_tree_launch
        tree_op = ca.op_create(fptr(mxint8.mxint8_lib(), "chr_mxi8_sum_fold"), commute=True,
                               tree=fptr(ab, "chr_mxi8_sum_tree_launch"))
    launcher.argtypes = [ctypes.POINTER(UserTree), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    launcher.restype = ctypes.c_int
    operand = lambda data, tiles: mx8_operand(
        data, tiles, lambda t, x: mxint8.quantize(t, x, tiles * mxint8.TILE_VALUES, ca.FLOAT32, stream))

    shapes = [(nl, tt, reps) for nl in (2, 4, 8) for tt, reps in ((31775, 240), (127100, 80))]
    shapes += [(8, 47662, 160), (8, 63550, 120), (8, 95325, 100)]  # --mx4's sizes between the two
    for data in ("close", "wild"):
        for nl, tt, reps in shapes:
            comb, swaps = TREE_PROGS[nl]
            tb = tt * mxint8.TILE_BYTES
            sets = max(1, int(2.25 * (1 << 30)) // ((nl + 1) * tb))
            bufs = [[operand(data, tt) for _ in range(nl + 1)] for _ in range(sets)]
            trees = []
            for s in bufs:
                t = UserTree()
                t.out = s[nl].data_ptr()
                for j in range(nl):
                    t.leaves[j] = s[j].data_ptr()
                    t.comb[j] = comb[j]
                t.nleaves, t.n = nl, tt
                trees.append(t)
            torch.cuda.synchronize()
            for r in range(len(rows)):
                for name, op in (("folds", mxint8.mxint8_sum()), ("tree", tree_op)):
                    def go(i, op=op):
                        s = bufs[i % sets]
                        ca.check(ca.reduce_tree(s[nl], s[:nl], comb, swaps, tt, tile_t, op, stream))
                    ms = timed(go, reps)
                    rows[r][f"{data}_tree{nl}_{tt}tiles_mxint8_{name}_ms"] = round(ms, 4)
                    rows[r][f"{data}_tree{nl}_{tt}tiles_mxint8_{name}_frac"] = round((nl + 1) * tb / (ms * 1e-3) / HBM_PEAK, 4)
                # 0: the launcher's own 16 per CU; 12: what the library asks for beside RCCL; 28: all 68 VGPRs allow
                for cap in (0, 12, 16, 28) if nl == 8 and tt in (31775, 127100) else ():
                    def go(i, cap=cap):
                        return launcher(ctypes.byref(trees[i % sets]), 1, tile_t, cap, stream.cuda_stream, None)
                    took = go(0) == 0  # a launcher that declines has enqueued nothing: the row is null
                    rows[r][f"{data}_tree8_{tt}tiles_mxint8_launcher_cap{cap}_ms"] = round(timed(go, reps), 4) if took else None
            del bufs, trees
    # the C4-shaped allreduce, 8 virtual ranks, 2 x 127 100 tiles per rank (eight 31 775-tile trees to a call), close data
    nr, cnt = 8, 254200
    g = ca.LocalGroup(nr, 0)
    sends = [operand("close", cnt) for _ in range(nr)]
    recvs = [torch.empty(cnt * mxint8.TILE_BYTES, dtype=torch.uint8, device=dev) for _ in range(nr)]
    for r in range(len(rows)):
        for name, op in (("folds", mxint8.mxint8_sum()), ("tree", taken)):
            for _ in range(2):
                ca.check(g.all_reduce_radix_batch(sends, recvs, cnt, tile_t, op, 4, 4))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                ca.check(g.all_reduce_radix_batch(sends, recvs, cnt, tile_t, op, 4, 4))
            torch.cuda.synchronize()
            rows[r][f"localgroup8_k4b4_{cnt}tiles_mxint8_{name}_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
    g.destroy()
    if take_all:
        ca.op_free(tree_op)
    mxint8.tree_release()


def mx4_tree_rows(rows, stream, take_all=None):
    """The tree rows of --mx4, into rows[r]: the fold-only op and the one-pass op interleaved within each round."""
    from chiara_amd import mx4

    dev = torch.device("cuda:0")
    tile_t = mx4.mx4_type()
    fptr = lambda L, name: ctypes.cast(getattr(L, name), ctypes.c_void_p).value
    taken = mx4.mx4_sum_tree()
    launcher, tree_op = mx4.mx4_tree_lib().chr_mx4_sum_tree_launch, taken
    if take_all:  # a -DCHR_MX4_TREE_TAKE_ALL=1 build (make mx4_tree_ab): the same kernels, nothing declined for speed
        ab = ctypes.CDLL(os.path.abspath(take_all))
        launcher = ab.chr_mx4_sum_tree_launch
        tree_op = ca.op_create(fptr(mx4.mx4_lib(), "chr_mx4_sum_fold"), commute=True, tree=fptr(ab, "chr_mx4_sum_tree_launch"))
    launcher.argtypes = [ctypes.POINTER(UserTree), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    launcher.restype = ctypes.c_int

    def operand(tiles):
        nvals = tiles * mx4.TILE_VALUES
        x = torch.randn(nvals // 32, 32, device=dev) * torch.exp2(torch.randint(-20, 21, (nvals // 32, 1), device=dev))
        t = torch.empty(tiles * mx4.TILE_BYTES, dtype=torch.uint8, device=dev)
        ca.check(mx4.quantize(t, x, nvals, ca.FLOAT32, stream))
        return t

    shapes = [(nl, tt, reps) for nl in (2, 4, 8) for tt, reps in ((31775, 240), (127100, 80))]
    shapes += [(8, 47662, 160), (8, 63550, 120), (8, 95325, 100)]  # between the two: where one pass stops paying
    for nl, tt, reps in shapes:
        comb, swaps = TREE_PROGS[nl]
        tb = tt * mx4.TILE_BYTES
        sets = max(1, int(2.25 * (1 << 30)) // ((nl + 1) * tb))
        bufs = [[operand(tt) for _ in range(nl + 1)] for _ in range(sets)]
        trees = []
        for s in bufs:
            t = UserTree()
            t.out = s[nl].data_ptr()
            for j in range(nl):
                t.leaves[j] = s[j].data_ptr()
                t.comb[j] = comb[j]
            t.nleaves, t.n = nl, tt
            trees.append(t)
        torch.cuda.synchronize()
        ops = [("folds", mx4.mx4_sum()), ("tree", tree_op)]
        for r in range(len(rows)):
            for name, op in ops:
                def go(i, op=op):
                    s = bufs[i % sets]
                    ca.check(ca.reduce_tree(s[nl], s[:nl], comb, swaps, tt, tile_t, op, stream))
                ms = timed(go, reps)
                rows[r][f"tree{nl}_{tt}tiles_mx4_{name}_ms"] = round(ms, 4)
                rows[r][f"tree{nl}_{tt}tiles_mx4_{name}_frac"] = round((nl + 1) * tb / (ms * 1e-3) / HBM_PEAK, 4)
            # 0: the launcher's own 16 per CU; 32: all the waves a CU holds
            for cap in (0, 12, 32) if nl == 8 and tt in (31775, 127100) else ():
                def go(i, cap=cap):
                    return launcher(ctypes.byref(trees[i % sets]), 1, tile_t, cap, stream.cuda_stream, None)
                took = go(0) == 0  # a launcher that declines has enqueued nothing: the row is null
                rows[r][f"tree8_{tt}tiles_mx4_launcher_cap{cap}_ms"] = round(timed(go, reps), 4) if took else None
        del bufs, trees
    # the C4-shaped allreduce, 8 virtual ranks, 2 x 127 100 tiles per rank
    nr, cnt = 8, 254200
    g = ca.LocalGroup(nr, 0)
    sends = [operand(cnt) for _ in range(nr)]
    recvs = [torch.empty(cnt * mx4.TILE_BYTES, dtype=torch.uint8, device=dev) for _ in range(nr)]
    for r in range(len(rows)):
        for name, op in (("folds", mx4.mx4_sum()), ("tree", taken)):
            for _ in range(2):
                ca.check(g.all_reduce_radix_batch(sends, recvs, cnt, tile_t, op, 4, 4))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                ca.check(g.all_reduce_radix_batch(sends, recvs, cnt, tile_t, op, 4, 4))
            torch.cuda.synchronize()
            rows[r][f"localgroup8_k4b4_{cnt}tiles_mx4_{name}_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
    g.destroy()
    if take_all:
        ca.op_free(tree_op)
    mx4.tree_release()


def numerics_rows(rounds, stream):
    """Rows of --numerics, per round: for each element size the library's f32 SUM, the RotMix struct op and the
    numerics op back to back on the same buffers (uniform values in [0, 1): every operation finite)."""
    from chiara_amd import numerics as num

    dev = torch.device("cuda:0")
    slib = ctypes.CDLL(os.path.join(REPO, "tests", "userop", STRUCT_BUILDS["shipped"]))

    def rotmix(shape):
        return ca.op_create(ctypes.cast(getattr(slib, f"chr_struct_RotMixK_{shape}"), ctypes.c_void_p).value,
                            tree=ctypes.cast(getattr(slib, f"chr_struct_RotMixK_{shape}_tree"), ctypes.c_void_p).value)

    # (label, element bytes, torch type, the op's (dtype, op), RotMix's shape, its base and count)
    kinds = [("sum2_f32", 8, torch.float32, (num.sum2_type(ca.FLOAT32), num.sum2_op()), "f32x2", ca.FLOAT32, 2),
             ("sum2_f64", 16, torch.float64, (num.sum2_type(ca.FLOAT64), num.sum2_op()), "f32x4", ca.FLOAT32, 4),
             ("moments_f64", 24, torch.float64, (num.moments_type(ca.FLOAT64), num.moments_op()), "f64x3", ca.FLOAT64, 3)]
    rows = [{} for _ in range(rounds)]
    made = []
    for label, es, tdt, (dt, op), shape, rbase, rk in kinds:
        rdt, rop = ca.type_contiguous(rk, rbase), rotmix(shape)
        made.append((rdt, rop))
        # (variant, dtype, op, elements per `es` bytes)
        variants = [("f32_sum", ca.FLOAT32, ca.SUM, es // 4), (f"rotmix_{shape}", rdt, rop, 1), (label, dt, op, 1)]
        for what, units, mib, reps in ([("fold", m + 1, 64, 60) for m in (1, 3)] + [("tree", 9, 16, 240), ("tree", 9, 64, 80)]):
            n = (mib << 20) // es
            sets = max(1, int(2.25 * (1 << 30)) // (units * n * es))
            bufs = [[torch.rand(n * es // tdt.itemsize, device=dev, dtype=tdt) for _ in range(units)] for _ in range(sets)]
            for r in range(rounds):
                for name, vdt, vop, per in variants:
                    if what == "fold":  # acc in place, m inputs: m + 2 units of traffic
                        def go(i, vdt=vdt, vop=vop, per=per):
                            s = bufs[i % sets]
                            ca.check(ca.reduce_multi(s[0], s[0], s[1:], n * per, vdt, vop, stream))
                        ms = timed(go, reps)
                        rows[r][f"fold_m{units - 1}_64MiB_{label}_{name}_GBps"] = round((units + 1) * n * es / ms / 1e6, 1)
                    else:
                        def go(i, vdt=vdt, vop=vop, per=per):
                            s = bufs[i % sets]
                            ca.check(ca.reduce_tree(s[8], s[:8], C4_COMB, C4_SWAPS, n * per, vdt, vop, stream))
                        ms = timed(go, reps)
                        rows[r][f"tree8_{mib}MiB_{label}_{name}_frac"] = round(9 * n * es / (ms * 1e-3) / HBM_PEAK, 4)
            del bufs
        nr, cnt = 8, (128 << 20) // es // 8 * 8
        g = ca.LocalGroup(nr, 0)
        sends = [torch.rand(cnt * es // tdt.itemsize, device=dev, dtype=tdt) for _ in range(nr)]
        recvs = [torch.empty(cnt * es // tdt.itemsize, device=dev, dtype=tdt) for _ in range(nr)]
        for r in range(rounds):
            for name, vdt, vop, per in variants:
                for _ in range(2):
                    ca.check(g.all_reduce_radix_batch(sends, recvs, cnt * per, vdt, vop, 4, 4))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(5):
                    ca.check(g.all_reduce_radix_batch(sends, recvs, cnt * per, vdt, vop, 4, 4))
                torch.cuda.synchronize()
                rows[r][f"localgroup8_k4b4_128MiB_{label}_{name}_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
        g.destroy()
        del sends, recvs
    for rdt, rop in made:
        ca.op_free(rop)
        ca.type_free(rdt)
    num.release()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fp8", action="store_true", help="only the FP8 rows of libchiara_fp8.so (see above)")
    ap.add_argument("--fp8-perbyte", metavar="LIB.so",
                    help="with --fp8: a -DCHR_FP8_PACKED=0 build of fp8_ops.hip (make fp8_ab); its SUMs as *_perbyte")
    ap.add_argument("--mx", action="store_true", help="only the MXFP8 rows of libchiara_mx.so (see above)")
    ap.add_argument("--mx4", action="store_true", help="only the MXFP4 rows of libchiara_mx4.so (see above)")
    ap.add_argument("--mx4-take-all", metavar="LIB.so",
                    help="with --mx4: a -DCHR_MX4_TREE_TAKE_ALL=1 build of mx4_tree_ops.hip (make mx4_tree_ab); the "
                         "one-pass tree rows run its launcher")
    ap.add_argument("--mx6", action="store_true", help="only the MXFP6 rows of libchiara_mx6.so (see above)")
    ap.add_argument("--mx6-take-all", metavar="LIB.so",
                    help="with --mx6: a -DCHR_MX6_TREE_TAKE_ALL=1 build of mx6_tree_ops.hip (make mx6_tree_ab); the "
                         "one-pass tree rows run its launchers")
    ap.add_argument("--mxint8", action="store_true", help="only the MXINT8 rows of libchiara_mxint8.so (see above)")
    ap.add_argument("--mxint8-f32", metavar="LIB.so",
                    help="with --mxint8: a -DCHR_MXI8_INT=0 build of mxint8_ops.hip (make mxint8_ab); its fold as mxint8_f32")
    ap.add_argument("--mxint8-take-all", metavar="LIB.so",
                    help="with --mxint8: a -DCHR_MXI8_TREE_TAKE_ALL=1 build of mxint8_tree_ops.hip (make mxint8_tree_ab); "
                         "the one-pass tree rows run its launcher")
    ap.add_argument("--numerics", action="store_true", help="only the struct-op rows of libchiara_numerics.so (see above)")
    ap.add_argument("--f16", action="store_true", help="only the binary16 rows (see above)")
    ap.add_argument("--struct", action="store_true", help="only the derived-type rows (see above)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-folds", action="store_true", help="skip the fold rows")
    ap.add_argument("--ab", action="append", default=[], metavar="NAME=LIB.so",
                    help="a build of tests/userop/halfadd_tree_op.hip with other knobs (-DCHR_USER_TREE_NT=1, "
                         "-DCHR_USER_TREE_XCD_RUN_KIB=512, ...): its one-pass rows as user_tree_NAME")
    ap.add_argument("--out", help="also write the JSON here")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    out = {"tool": "tools/userop_bench.py", "tree_lib": "libhalfadd_tree_op.so"}
    if a.fp8:
        out = {"tool": "tools/userop_bench.py --fp8", "ops_lib": "libchiara_fp8.so", "f16_lib": "libchiara_ops.so",
               "perbyte_lib": a.fp8_perbyte and os.path.basename(a.fp8_perbyte), "rounds": fp8_rows(a.rounds, stream, a.fp8_perbyte)}
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if a.mx:
        out = {"tool": "tools/userop_bench.py --mx", "ops_lib": "libchiara_mx.so", "tree_lib": "libchiara_mx_tree.so",
               "fp8_lib": "libchiara_fp8.so", "rounds": mx_rows(a.rounds, stream)}
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if a.mx4:
        out = {"tool": "tools/userop_bench.py --mx4", "ops_lib": "libchiara_mx4.so", "mx_lib": "libchiara_mx.so",
               "tree_lib": "libchiara_mx4_tree.so", "take_all_lib": a.mx4_take_all and os.path.basename(a.mx4_take_all),
               "rounds": mx4_rows(a.rounds, stream, a.mx4_take_all)}
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if a.mx6:
        out = {"tool": "tools/userop_bench.py --mx6", "ops_lib": "libchiara_mx6.so", "mx_lib": "libchiara_mx.so",
               "mx4_lib": "libchiara_mx4.so", "tree_lib": "libchiara_mx6_tree.so",
               "take_all_lib": a.mx6_take_all and os.path.basename(a.mx6_take_all),
               "rounds": mx6_rows(a.rounds, stream, a.mx6_take_all)}
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if a.mxint8:
        out = {"tool": "tools/userop_bench.py --mxint8", "ops_lib": "libchiara_mxint8.so", "mx_lib": "libchiara_mx.so",
               "f32_lib": a.mxint8_f32 and os.path.basename(a.mxint8_f32), "tree_lib": "libchiara_mxint8_tree.so",
               "take_all_lib": a.mxint8_take_all and os.path.basename(a.mxint8_take_all),
               "rounds": mxint8_rows(a.rounds, stream, a.mxint8_f32, a.mxint8_take_all)}
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if a.numerics:
        out = {"tool": "tools/userop_bench.py --numerics", "ops_lib": "libchiara_numerics.so",
               "struct_lib": STRUCT_BUILDS["shipped"], "rounds": numerics_rows(a.rounds, stream)}
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if a.f16:
        out = {"tool": "tools/userop_bench.py --f16", "ops_lib": "libchiara_ops.so", "rounds": f16_rows(a.rounds, stream)}
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if a.struct:
        out["builds"] = STRUCT_BUILDS
        out["rounds"] = struct_rows(a.rounds, stream)
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if not a.no_folds:
        fold_rows(out, dev, stream)
    tlib = ctypes.CDLL(os.path.join(REPO, "tests", "userop", "libhalfadd_tree_op.so"))
    fold = ctypes.cast(tlib.chr_test_halfadd, ctypes.c_void_p).value
    tree_fn = tlib.chr_test_halfadd_tree
    tree_fn.argtypes = [ctypes.POINTER(UserTree), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                        ctypes.c_void_p]
    tree_fn.restype = ctypes.c_int
    folds_only = ca.op_create(fold)
    one_pass = ca.op_create(fold, tree=ctypes.cast(tree_fn, ctypes.c_void_p).value)
    variants = [("sum", ca.SUM), ("user_folds", folds_only), ("user_tree", one_pass)]
    ab_libs = []
    for spec in a.ab:
        name, path = spec.split("=", 1)
        ab = ctypes.CDLL(os.path.abspath(path))
        ab_libs.append(ab)
        variants.append((f"user_tree_{name}", ca.op_create(ctypes.cast(ab.chr_test_halfadd, ctypes.c_void_p).value,
                                                           tree=ctypes.cast(ab.chr_test_halfadd_tree, ctypes.c_void_p).value)))
    out["ab"] = a.ab
    c4 = c4_rows(a.rounds, variants)
    tr = tree_rows(a.rounds, variants, tree_fn, stream)
    out["rounds"] = [dict(c, **t) for c, t in zip(c4, tr)]
    for _, op in variants[1:]:
        ca.op_free(op)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
