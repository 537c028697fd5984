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
