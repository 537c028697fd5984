#!/usr/bin/env python3
"""bench.py -- CHiArA hot path on MI355X.

N=1 (default): BASELINE config C2, the device-resident fp32 bucket reduction with k=2
(one incoming 64 MiB bucket reduced into a 64 MiB accumulator = one MPI_Reduce_local
call site of the reference, all_reduce_radix_batch.cpp:364).  One step = one call.
Inputs are resident in HBM before the timed region; NSETS distinct (acc, in) pairs are
cycled so the 2 GiB working set streams from HBM and not from the 256 MiB Infinity
Cache.  value = algorithmic bytes (3 x 64 MiB per call) / wall time per step.

N>1 (one rank per GPU): the whole hierarchical allreduce over RCCL/xGMI (C4 geometry: fp32,
1 GiB per rank, k=4, b=4 at N=8; k=b=min(4,N) otherwise).  value = aggregate input bytes
reduced per second (N x 1 GiB per step / time).  `python bench.py --gpus N` starts its own N
rank processes (torch.distributed.run as a child process, before anything touches the GPU),
as the reference's run target starts its own ranks (testing/Makefile:83-87, `mpirun -np`);
under an external launcher (WORLD_SIZE set) each process is one rank.  The whole N>1 line runs
against a deadline (CHR_BENCH_DEADLINE_S, default 240 s from the launch): context entries that
would start after it are recorded as {"skipped": "deadline"}, never the metric.

A plain run sets up, warms up, times --steps steps, writes --dump-outputs if given and prints the line.
--full adds what the headline figure does not need: the CPU baseline, the result checks of the metric's
output and, at N>1, the profiled call behind `roofline` / `phase_transfer_ms` and the `compare` context lines
(--no-cpu-baseline and --no-compare leave those two out of a --full run).

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

# RCCL / cross-process device memory on this host driver need dmabuf IPC:
# set before torch or HIP is loaded, so every rank's runtime starts with it.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

REPO = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.join(REPO, "configurable-hierarchical-allreduce-algorithms_amd")
sys.path[:0] = [PKG_DIR, os.path.join(REPO, "oracle")]

METRIC = "device-resident bucket-reduction GB/s (fp32); allreduce GB/s at 2/4/8 GPUs"
HBM_PEAK_GBPS = 8000.0       # MI355X HBM3E spec (MI355X_MICROARCH.md, chip-level parameters)
XGMI_LINK_GBPS = 153.6       # per xGMI link, both directions together (AMD's spec convention); 7 links per GPU
XGMI_DIR_GBPS = XGMI_LINK_GBPS / 2  # one direction of one link: what a directed GPU pair's bytes cross
C2_ELEMS = 16 << 20          # 64 MiB fp32 per bucket
NSETS = 16                   # 16 x 128 MiB distinct = 2 GiB working set: 8x the 256 MiB Infinity Cache
SEED = 0xC41A5EED
CPU_THREADS = 16             # the GPU box's CPU share per GPU (nproc shows the whole machine)
GATE_CYCLES = 1_000_000      # torch.cuda._sleep before the timed region: ~0.4 ms at the shader clock


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--full", action="store_true",
                   help="beside the metric: the CPU baseline, the result checks of the metric's output and, at N>1, "
                        "the profiled call behind the roofline and the same-run context lines.  Without it a run "
                        "sets up, warms up, times --steps steps and prints the line")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32; "
                        "a fixed seeded sample of 8 Mi elements of a larger output; rank 0 at N>1)")
    p.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    p.add_argument("--cpu-seconds", type=float, default=10.0)
    p.add_argument("--sweep", action="store_true", help="N=1: bucket sizes 1 KiB..1 GiB, m=1/3/7 (table to stderr)")
    p.add_argument("--count", type=int, default=None, help="N>1: elements per rank (default 2^28)")
    p.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    p.add_argument("--no-compare", action="store_true",
                   help="N>1 --full: skip the same-run context lines (RCCL allreduce, MPICH ring on libchiara)")
    p.add_argument("--phases", action="store_true",
                   help="N>1: add CHiArA's stand-alone phases (phase 1, phase 2, the k-nomial scatter) to the "
                        "context lines")
    p.add_argument("--e2e", action="store_true",
                   help="N=1: host-memory (PCIe-inclusive) staging cost of the reference's host-buffer contract")
    p.add_argument("--collective-kernels", action="store_true",
                   help="N=1: the fused reductions of the C4/C5 collectives at full size (8 virtual ranks, "
                        "loopback transport), HIP-event timed against the HBM roofline")
    p.add_argument("--collective-kernels-small", action="store_true",
                   help="N=1: the same for the N=2 / N=4 lines' allreduces (1 GiB per rank) and C3's reduce-scatter "
                        "(2 ranks, 256 MiB send): the 2- and 4-leaf trees")
    p.add_argument("--rank-trees", action="store_true",
                   help="N=1: only the rank-alone rows of --collective-kernels (one GPU's own C4 / C5 grids)")
    return p.parse_args(argv)


# ---- CPU baseline (rank 0, N=1 only; runs BEFORE the GPU is touched) ------------------------

def cpu_baseline(seconds):
    ref_bin = os.path.join(REPO, "oracle", "_ref", "ref_reduce_local")
    if os.path.exists(ref_bin):
        try:
            out = subprocess.run([ref_bin, str(C2_ELEMS), str(seconds)], capture_output=True, text=True,
                                 timeout=seconds + 60)
            if out.returncode == 0:
                r = json.loads(out.stdout.strip().splitlines()[-1])
                line = {"value": round(r["gbps"], 3), "unit": "GB/s", "cores": 1, "kind": "reference",
                        "sample": f"MPICH 3.3.2 MPI_Reduce_local(MPI_FLOAT, MPI_SUM) on a 64 MiB bucket, m=1, "
                                  f"{r['calls']} calls in {r['seconds']:.1f} s, 1 thread "
                                  f"(oracle/_ref/ref_reduce_local; nproc={os.cpu_count()})"}
                # all-cores variant: the bucket cut into CPU_THREADS slices, one
                # MPI_Reduce_local stream per thread; the box's CPU share per GPU is 16 cores
                out = subprocess.run([ref_bin, str(C2_ELEMS), str(seconds / 2), str(CPU_THREADS)],
                                     capture_output=True, text=True, timeout=seconds + 60)
                if out.returncode == 0:
                    r = json.loads(out.stdout.strip().splitlines()[-1])
                    line["all_cores"] = {
                        "value": round(r["gbps"], 3), "unit": "GB/s", "cores": r["threads"], "kind": "reference",
                        "sample": f"same call, 64 MiB bucket cut into {r['threads']} slices, one thread each, "
                                  f"{r['seconds']:.1f} s"}
                return line
        except Exception:
            pass
    import numpy as np

    import pyoracle as po

    a = po.fill(C2_ELEMS, "f32", 0, SEED, 1)
    b = po.fill(C2_ELEMS, "f32", 0, SEED, 0)
    po.reduce_local(a, b, "f32", "sum")
    calls, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        po.reduce_local(a, b, "f32", "sum")
        calls += 1
    dt = time.perf_counter() - t0
    np.asarray(b).sum()
    return {"value": round(3 * 4 * C2_ELEMS * calls / dt / 1e9, 3), "unit": "GB/s", "cores": 1, "kind": "port",
            "sample": f"oracle orc_reduce_local (MPI_Reduce_local restated), 64 MiB fp32 bucket, m=1, "
                      f"{calls} calls in {dt:.1f} s, 1 thread (nproc={os.cpu_count()})"}


CPU_COLL_SAMPLE_ELEMS = 1 << 24  # the fallback sample: 64 MiB fp32 per rank


def cpu_baseline_collective(world, k, b, gpu_count, gpu_es, budget_s=None):
    """N>1: the REAL reference all_reduce_radix_batch (oracle/_ref/ref_timer: the reference file
    compiled unchanged against MPICH) on `world` host cores, one MPI rank per core, same (k, b), at the
    GPU line's own per-rank count (the reference's harness times the collective at the real count,
    Fugaku_experiments/Allreduce/main.cpp:55-69, :185-195): one warm-up call and 2 timed calls, max over
    ranks.  The reference takes ~3 s per 1 GiB call at 8 ranks, and its per-call
    malloc and first touch scale with the size, so a smaller sample overstates its rate (VERDICT r4
    missing-2).  Only when `budget_s` (the deadline's remaining seconds) cannot hold the whole workload
    is the labelled 64 MiB sample timed instead.  Same value definition as the GPU line."""
    exe = os.path.join(REPO, "oracle", "_ref", "ref_timer")
    mpiexec = "/opt/conda/bin/mpiexec"
    if not (os.path.exists(exe) and os.path.exists(mpiexec)):
        return None
    whole_elems = gpu_count - gpu_count % world
    # ~3 s per 1 GiB call at 8 ranks (scaled by size), 3 calls, plus process start-up and first touch
    est_s = 3 * 3.0 * (whole_elems * 4 / 2**30) + 10
    full = os.environ.get("CHR_BENCH_CPU_SAMPLE") != "1" and (budget_s is None or est_s < budget_s)
    elems = whole_elems if full else min(whole_elems, CPU_COLL_SAMPLE_ELEMS - CPU_COLL_SAMPLE_ELEMS % world)
    if elems <= 0:
        return None
    reps = 2 if full else 3
    try:
        out = subprocess.run([mpiexec, "-bind-to", "core", "-n", str(world), exe, "ar", str(k), str(b), str(elems),
                              str(reps)], capture_output=True, text=True, timeout=max(120, 4 * est_s))
        if out.returncode != 0:
            return None
        r = json.loads(out.stdout.strip().splitlines()[-1])
    except Exception:
        return None
    t = r["seconds_per_call"]
    whole = elems == gpu_count and gpu_es == 4
    what = ("the whole per-rank workload" if whole else
            ("the whole per-rank element count, in fp32" if elems == whole_elems else
             f"a bounded sample of the {gpu_count * gpu_es / 2**20:g} MiB per rank workload, "
             f"{elems / gpu_count * 100:.3g} % of its elements" + ("" if gpu_es == 4 else ", in fp32") +
             (", the deadline leaving too little time for the whole" if not full and budget_s is not None else "")))
    return {"value": round(world * elems * 4 / t / 1e9, 3), "unit": "GB/s", "cores": world, "kind": "reference",
            "algbw_GBps": round(elems * 4 / t / 1e9, 4),
            "sample": f"reference all_reduce_radix_batch (all_reduce_radix_batch.cpp compiled unchanged, MPICH 3.3.2), "
                      f"{world} ranks bound to {world} host cores, k={k}, b={b}, {elems * 4 / 2**20:g} MiB fp32 per rank "
                      f"({what}), 1 warm-up + {reps} timed calls, max over ranks: {t * 1e3:.1f} ms per call "
                      f"(nproc={os.cpu_count()})"}


LINE_DEFINITIONS_N1 = {
    "value": "3 x bucket bytes (acc read, incoming read, result write) / (HIP-event span of K launches / K)",
    "roofline.achieved": "the same bytes / event_span_ms_per_launch: algorithmic bytes per launch over the launch "
                         "period, gaps included",
    "roofline.traffic": "HBM bytes per launch from rocprofv3 FETCH_SIZE x 2 (gfx950) + WRITE_SIZE passes "
                        "(profiles/pmc_latest.json), reported only while the kernel symbol and source hash match",
    "cpu_baseline.value": "the same 3 x bucket bytes per MPI_Reduce_local call / its wall time"}
LINE_DEFINITIONS_NN = {
    "value": "whole job (task contract): N x S / t, S = the per-rank buffer bytes, t = the max-over-ranks time per "
             "call; the input bytes all ranks reduced per second.  = aggregate_GBps",
    "algbw_GBps": "S / t (nccl-tests; SURVEY 8(d))",
    "busbw_GBps": "algbw x 2 (N - 1) / N (nccl-tests allreduce; SURVEY 8(d))",
    "roofline": "the busiest rank's fused reductions of one call (k_reduce_tree / k_reduce_vec): algorithmic bytes "
                "(leaves + root per tree) / the summed HIP-event spans of its grids",
    "roofline.traffic": "HBM bytes per call: the algorithmic bytes x the traffic/algorithmic ratio of the PMC entry "
                        "for the same kernel symbol (profiles/pmc_latest.json), null when none matches or it is stale",
    "xgmi_roofline.frac": "the compiled plan's busiest directed GPU pair's bytes / 76.8 GB/s (one direction of one "
                          "xGMI link) / t",
    "cpu_baseline.value": "N x S / t of the reference all_reduce_radix_batch on N host cores (same definition as value)",
    "rccl.xgmi": "RCCL holds N ranks on N distinct PCI devices and every logged connection is P2P",
    "result_check": "the metric's output on every rank and element: ranks bit-identical (position-weighted int64 "
                    "checksums of the raw words) and |x - fp64 sum of the N inputs| <= (N-1) ulp sum|x_i| (DESIGN §7)"}

def line_problems(line, rccl_library=True):
    """What in a bench line disagrees with LINE_DEFINITIONS_N1 / _NN (empty list: none).  Checked by
    tests/test_bench_line.py on canned lines and on the lines GPU runs committed under profiles/.
    rccl_library: an N>1 line must name its librccl and version (round 6 on; round-5 lines predate it)."""
    probs = []
    need = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "definitions")
    probs += [f"missing {k}" for k in need if k not in line]
    if probs:
        return probs

    def close(a, b, rel=2e-3):  # the line rounds GB/s to 0.01: allow that on either side
        return abs(a - b) <= rel * max(abs(a), abs(b), 1e-12) + 0.011

    n, ms, rf = line["n_gpus"], line["ms_per_step"], line["roofline"]
    if "workload" not in line["config"]:
        probs.append("config.workload missing")
    if n == 1:
        by = rf.get("algorithmic_bytes_per_launch")
        span = rf.get("event_span_ms_per_launch")
        if "avg_kernel_ms" in rf:
            probs.append("roofline.avg_kernel_ms: the event span is not a kernel duration (event_span_ms_per_launch)")
        if by is None or span is None:
            probs.append("roofline needs algorithmic_bytes_per_launch and event_span_ms_per_launch")
        else:
            if not close(line["value"], by / (ms * 1e-3) / 1e9, 5e-3):
                probs.append("value != algorithmic bytes / ms_per_step")
            if not close(rf["achieved"], by / (span * 1e-3) / 1e9, 5e-3):
                probs.append("roofline.achieved != algorithmic bytes / event span")
        if line["definitions"] != LINE_DEFINITIONS_N1:
            probs.append("definitions differ from LINE_DEFINITIONS_N1")
    else:
        c = line["config"]
        es = 4 if line["dtype"] == "f32" else 2
        S = c.get("count", 0) * es
        for k in ("algbw_GBps", "busbw_GBps", "aggregate_GBps", "rccl"):
            if k not in line:
                probs.append(f"missing {k}")
        for k in ("k", "b", "count", "schedule", "slices", "overlap"):
            if k not in c:
                probs.append(f"config.{k} missing")
        if probs:
            return probs
        agg = n * S / (ms * 1e-3) / 1e9
        if not close(line["value"], agg, 5e-3) or not close(line["aggregate_GBps"], agg, 5e-3):
            probs.append("value / aggregate_GBps != N x S / t")
        if not close(line["algbw_GBps"], S / (ms * 1e-3) / 1e9, 5e-3):
            probs.append("algbw_GBps != S / t")
        if not close(line["busbw_GBps"], line["algbw_GBps"] * 2 * (n - 1) / n, 5e-3):
            probs.append("busbw_GBps != algbw x 2(N-1)/N")
        r = line["rccl"]
        for k in ("nranks", "user_ranks", "pci_bus_ids", "transports", "pairs", "xgmi", "not_xgmi_because"):
            if k not in r:
                probs.append(f"rccl.{k} missing")
        if rccl_library:
            probs += [f"rccl.{k} missing" for k in ("library", "version", "same_on_all_ranks") if not r.get(k)]
        if r.get("xgmi") and r.get("not_xgmi_because"):
            probs.append("rccl.xgmi true with reasons against it")
        if r.get("xgmi") is False and not r.get("not_xgmi_because"):
            probs.append("rccl.xgmi false without a reason")
        rc = line.get("result_check")
        if rc is None and line.get("full") is False:
            pass  # a run without --full makes no result check; lines from before the option are full
        elif not isinstance(rc, dict):
            probs.append("result_check missing")
        elif not (rc.get("ranks_bit_identical") and rc.get("within_tolerance")):
            probs.append(f"result_check failed: {rc}"[:300])
        elif rc.get("exact_known_answer") is False:
            probs.append(f"result_check exact known answer failed: {rc}"[:300])
        if rf is not None and rf.get("traffic") is None and not rf.get("traffic_stale"):
            probs.append("roofline.traffic null without traffic_stale")
        c5 = (line.get("compare") or {}).get("c5_allreduce_bf16_k4_b4_1GiB")
        if c5 and "skipped" not in c5 and "error" not in c5:
            probs += [f"c5.{k} missing" for k in ("schedule", "slices", "overlap") if k not in c5]
            if c5.get("slices") is not None and c5["slices"] < 2 and "overlapped_best_depth_ge2" not in c5:
                probs.append("c5 ran one slice and no overlapped depth was timed")
            c5rc = c5.get("result_check")
            if c5rc is not None and not (c5rc.get("ranks_bit_identical") and c5rc.get("within_tolerance")):
                probs.append(f"c5 result_check failed: {c5rc}"[:300])
            elif c5rc is not None and c5rc.get("exact_known_answer") is False:
                probs.append(f"c5 result_check exact known answer failed: {c5rc}"[:300])
        if line["definitions"] != LINE_DEFINITIONS_NN:
            probs.append("definitions differ from LINE_DEFINITIONS_NN")
    rc1 = line.get("result_check") if line.get("n_gpus") == 1 else None
    if rc1 is not None and not rc1.get("bit_exact_vs_torch_add"):
        probs.append(f"result_check failed: {rc1}"[:300])
    cb = line["cpu_baseline"]
    if cb is not None:
        probs += [f"cpu_baseline.{k} missing" for k in ("value", "unit", "cores", "kind", "sample") if k not in cb]
    return probs


C2_KERNEL_SYMBOL = "void chr::k_reduce_vec<0, 0, 1, 4, true, true, 64>(chr::VecArgs)"


TREE8_KERNEL_SYMBOL = "void chr::k_reduce_tree<0, 0, 8, 1, true, 64, true>(chr::TreeArgs)"
# The kernel a flat plan's reductions run on, by the plan's own ops (reduction_pmc): a tree of L leaves -> its PMC entry
# (tools/tree_pmc.py --leaves L) and the streaming instantiation a 1 GiB call launches (reduce_tree.hpp tree_u: U = 1 /
# 2 / 4; the last argument: the ACC0 slot, round 6); a single fold of m incoming pieces -- what the N = 2 and N = 4 lines' one-node geometries compile to
# (schedule.cpp tree_program) -- -> the bucket kernel out of place (tools/tree_pmc.py --vec m).  Round 5 bound the N = 2
# / N = 4 lines to the 2- / 4-leaf tree entries, kernels those lines never launch.
TREE_PMC = {8: ("tree_f32_sum_8leaves_64MiB", TREE8_KERNEL_SYMBOL),
            4: ("tree_f32_sum_4leaves_64MiB", "void chr::k_reduce_tree<0, 0, 4, 2, true, 64, true>(chr::TreeArgs)"),
            # a streaming 2-leaf tree runs as one out-of-place fold on the bucket kernel (reduce_tree.hip, round 6)
            2: ("tree_f32_sum_2leaves_64MiB", "void chr::k_reduce_vec<0, 0, 1, 4, true, true, 64>(chr::VecArgs)")}
VEC_OOP_PMC = {1: ("reduce_f32_sum_m1_oop_128MiB", "void chr::k_reduce_vec<0, 0, 1, 4, true, true, 64>(chr::VecArgs)"),
               3: ("reduce_f32_sum_m3_oop_64MiB", "void chr::k_reduce_vec<0, 0, 3, 2, true, true, 64>(chr::VecArgs)")}


def reduction_pmc(plan):
    """((pmc key, kernel symbol), None) for the reductions of a parsed plan (ca.parse_plan), or (None, why): every
    reduction of the plan must be the same kernel shape -- trees of one leaf count, or folds of one fan-in."""
    shapes = {("tree", len(op[4]) + 1) if op[0] == "tree" else ("reduce", len(op[4]))
              for st in plan["steps"] for op in st["post"] if op[0] in ("tree", "reduce")}
    if len(shapes) != 1:
        return None, f"reductions of several shapes: {sorted(shapes)}" if shapes else "no reductions"
    kind, width = shapes.pop()
    entry = (TREE_PMC if kind == "tree" else VEC_OOP_PMC).get(width)
    if entry is None:
        return None, f"no PMC entry for {kind} width {width}"
    return entry, None


def pmc_ratio(kernel_key, symbol, root=REPO):
    """(HBM traffic / algorithmic bytes, None) of a current PMC entry, or (None, why)."""
    traffic, stale = pmc_traffic(kernel_key, symbol, root)
    if traffic is None:
        return None, stale
    with open(os.path.join(root, "profiles", "pmc_latest.json")) as f:
        alg = json.load(f)["kernels"][kernel_key]["algorithmic_bytes_per_launch"]
    return traffic / alg, None


def pmc_traffic(kernel_key, symbol, root=REPO):
    """HBM bytes per launch from the committed rocprofv3 PMC summary (profiles/pmc_latest.json), or
    (None, why) when that entry was measured on another kernel symbol or before its sources last
    changed (tools/pmc_provenance.py)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import pmc_provenance

    try:
        with open(os.path.join(root, "profiles", "pmc_latest.json")) as f:
            entry = json.load(f)["kernels"].get(kernel_key)
    except Exception as e:
        return None, f"profiles/pmc_latest.json unreadable: {e}"
    return pmc_provenance.current_traffic(entry, kernel_key, symbol, root)


DUMP_MAX_ELEMS = 8 << 20     # --dump-outputs: at most 32 MiB of float32 per array


def dump_outputs(torch, out_dir, name, out):
    """--dump-outputs: the 1-D device tensor `out` (what the last timed step handed its caller) as
    out_dir/<name>.npy in float32 -- all of it up to DUMP_MAX_ELEMS elements, else the elements at DUMP_MAX_ELEMS
    positions drawn once from SEED and the length (sorted), so two runs with the same arguments write the same
    positions of the same inputs' result."""
    import numpy as np

    n = out.numel()
    if n > DUMP_MAX_ELEMS:
        idx = np.sort(np.random.default_rng(SEED).integers(0, n, size=DUMP_MAX_ELEMS, dtype=np.int64))
        out = out[torch.from_numpy(idx).to(out.device)]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, name + ".npy"), out.float().cpu().numpy())


# ---- N = 1: bucket reduction (C2) ----------------------------------------------------------------

def bench_bucket(args, cpu):
    import torch

    import chiara_amd as ca

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    n = C2_ELEMS
    # One bucket set = (acc, incoming) allocated together.  Allocating all accumulators
    # first and all inputs after measured ~2 % slower on the same kernel
    # (profiles/r01/microbench_layout.txt); page offsets made no difference.
    accs, ins = [], []
    for _ in range(NSETS):
        accs.append(torch.empty(n, dtype=torch.float32, device=dev))
        ins.append(torch.empty(n, dtype=torch.float32, device=dev))
    for i in range(NSETS):
        ca.check(ca.fill(accs[i], n, ca.FLOAT32, 0, SEED, 2 * i, stream=stream))
        ca.check(ca.fill(ins[i], n, ca.FLOAT32, 0, SEED, 2 * i + 1, stream=stream))
    torch.cuda.synchronize()

    def step(i):
        s = i % NSETS
        return ca.reduce_local(ins[s], accs[s], n, ca.FLOAT32, ca.SUM, stream)

    # Untimed warmup: at least one launch per buffer set, so every set has been streamed by the
    # kernel (and the clocks have left idle) before timing, whatever --warmup is; the working set
    # stays 2 GiB, 8x the Infinity Cache, so the timed launches still stream from HBM.
    touch = max(args.warmup, 2 * NSETS)
    for i in range(touch):
        ca.check(step(i))
    torch.cuda.synchronize()
    # Timed region: HIP events on the launch stream around K back-to-back launches of the
    # one kernel; the average launch duration is the region time / K (inter-launch gaps
    # included, so it can only under-state the kernel's own rate).  After the synchronize, an
    # untimed gate kernel (torch.cuda._sleep, ~0.4 ms of spinning) holds the stream while the host
    # enqueues the start event and the K launches: otherwise the start event fires at once on the
    # idle GPU and the first launch's host-side latency (~5-10 us from Python) is booked into the
    # region, 1-2 % of a 20-step line.  CHR_BENCH_GATE=0 leaves it out.
    gate = os.environ.get("CHR_BENCH_GATE", "1") != "0" and hasattr(torch.cuda, "_sleep")  # a private torch API
    t_start, t_end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    wall0 = time.perf_counter()
    if gate:
        torch.cuda._sleep(GATE_CYCLES)
    t_start.record(stream)
    for i in range(args.steps):
        rc = step(i)
        if rc:
            ca.check(rc)
    t_end.record(stream)
    torch.cuda.synchronize()
    wall = time.perf_counter() - wall0
    total_ms = t_start.elapsed_time(t_end)
    avg_kern_ms = total_ms / args.steps
    bytes_per_step = 3 * 4 * n
    ms_per_step = total_ms / args.steps
    if args.dump_outputs:  # the accumulator the last timed call reduced into, before anything else touches it
        dump_outputs(torch, args.dump_outputs, "acc", accs[(args.steps - 1) % NSETS])
    achieved = bytes_per_step / (avg_kern_ms * 1e-3) / 1e9
    traffic, stale = pmc_traffic("reduce_f32_sum_m1_64MiB", C2_KERNEL_SYMBOL)
    line = {
        "metric": METRIC, "value": round(bytes_per_step / (ms_per_step * 1e-3) / 1e9, 2), "unit": "GB/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 5),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "C2 bucket reduction: k=2 (m=1 incoming bucket), 64 MiB fp32 per bucket, "
                               "device-resident, MPI_Reduce_local semantics", "bucket_bytes": 4 * n, "m": 1,
                   "buffer_sets": NSETS, "untimed_launches": touch, "parallelism": "replicas",
                   "gate": "untimed spin kernel ahead of the start event" if gate else None},
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": traffic,
                     "kernel": C2_KERNEL_SYMBOL, "algorithmic_bytes_per_launch": bytes_per_step,
                     # the HIP-event span of the K back-to-back launches / K: each launch's duration plus
                     # the gap to the next (rocprof's per-kernel average is in profiles/, and is shorter)
                     "event_span_ms_per_launch": round(avg_kern_ms, 5)},
        "definitions": LINE_DEFINITIONS_N1,
        "cpu_baseline": cpu,
        "host_wall_s": round(wall, 4),
        "full": bool(args.full),  # --full: cpu_baseline and result_check beside the metric
    }
    if stale:
        line["roofline"]["traffic_stale"] = stale
    if args.full:
        line["result_check"] = bucket_result_check(torch, ca, accs[0], ins[0], n, stream)
    if cpu:
        line["gpu_vs_cpu"] = round(line["value"] / cpu["value"], 1)
        if "all_cores" in cpu:
            line["gpu_vs_cpu_all_cores"] = round(line["value"] / cpu["all_cores"]["value"], 1)
    if args.sweep:
        line["sweep"] = sweep(ca, torch, dev, stream)
    emit(line)


def bucket_result_check(torch, ca, acc, inc, n, stream):
    """The metric's own output, untimed, without the oracle: one more launch on a bucket set of the timed region,
    every element bit-compared with torch's fp32 add of the same two buckets (MPI_Reduce_local SUM on MPI_FLOAT is one
    IEEE round-to-nearest add per element, commutative for these NaN-free inputs, so an independent implementation
    must give the same bits)."""
    before = acc.clone()
    ca.check(ca.reduce_local(inc, acc, n, ca.FLOAT32, ca.SUM, stream))
    torch.cuda.synchronize()
    want = before + inc
    bad = int((acc.view(torch.int32) != want.view(torch.int32)).sum())
    del before, want
    return {"bit_exact_vs_torch_add": bad == 0, "mismatches": bad, "elements": n,
            "check": "one more launch on bucket set 0: every element == torch's fp32 (in + inout), bit for bit"}


def sweep(ca, torch, dev, stream):
    """Bucket sizes 1 KiB .. 1 GiB, m = 1, 3, 7 (fp32) and m = 3 (bf16): GB/s over HIP events."""
    rows = []
    for m, dname in ((1, "f32"), (3, "f32"), (7, "f32"), (1, "bf16"), (3, "bf16")):
        cdt, es, tdt = (ca.FLOAT32, 4, torch.float32) if dname == "f32" else (ca.BFLOAT16, 2, torch.bfloat16)
        for lg in range(10, 31, 2):
            nbytes = 1 << lg
            n = nbytes // es
            sets = max(1, min(16, (2048 << 20) // ((m + 1) * nbytes)))
            bufs = [[torch.empty(n, dtype=tdt, device=dev) for _ in range(m + 1)] for _ in range(sets)]
            for s in bufs:
                for j, t in enumerate(s):
                    ca.fill(t, n, cdt, 0, SEED, j, stream=stream)
            reps = max(20, min(200, (16 << 30) // ((m + 2) * nbytes)))

            def go(i, st=stream):
                s = bufs[i % sets]
                return ca.reduce_multi(s[0], s[0], s[1:], n, cdt, ca.SUM, st)

            for i in range(3):
                go(i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            if hasattr(torch.cuda, "_sleep"):  # the gate of bench_bucket: host latency out of the region
                torch.cuda._sleep(GATE_CYCLES)
            e0.record(stream)
            for i in range(reps):
                go(i)
            e1.record(stream)
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / reps
            # The same reps launches captured once in a HIP graph and replayed: small buckets are
            # bound by the per-call host path (~5 us from Python); the graph shows the kernel's
            # own launch-to-launch time.
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                cap = torch.cuda.current_stream(dev)
                for i in range(reps):
                    ca.check(go(i, cap), "graph capture")
            graph.replay()
            torch.cuda.synchronize()
            e0.record(stream)
            graph.replay()
            e1.record(stream)
            torch.cuda.synchronize()
            ms_g = e0.elapsed_time(e1) / reps
            del graph
            gbps = (m + 2) * nbytes / (ms * 1e-3) / 1e9
            gbps_g = (m + 2) * nbytes / (ms_g * 1e-3) / 1e9
            rows.append({"dtype": dname, "m": m, "bucket_bytes": nbytes, "us": round(ms * 1e3, 2),
                         "GBps": round(gbps, 1), "frac": round(gbps / HBM_PEAK_GBPS, 4),
                         "us_graph": round(ms_g * 1e3, 2), "GBps_graph": round(gbps_g, 1),
                         "frac_graph": round(gbps_g / HBM_PEAK_GBPS, 4)})
            print(f"sweep {dname} m={m} bucket={nbytes:>11d} B  {ms * 1e3:9.2f} us  {gbps:8.1f} GB/s   "
                  f"graph {ms_g * 1e3:9.2f} us  {gbps_g:8.1f} GB/s", file=sys.stderr, flush=True)
            del bufs
    torch.cuda.empty_cache()
    return rows


def bench_e2e(args):
    """PCIe-inclusive cost of the reference's host-memory contract on one rank: the
    collective stages send H2D and recv D2H around the device-resident schedule."""
    import numpy as np
    import torch

    import chiara_amd as ca

    torch.cuda.set_device(0)
    comm = ca.Comm(1, ca.get_unique_id(), 0, 0)
    n = 1 << 28  # 1 GiB fp32 per rank, the C4 buffer
    out = {"workload": "host-buffer staging, 1 GiB fp32, nranks=1 (H2D + schedule + D2H)"}
    # window 0: one H2D, the collective, one D2H; else chr_comm_set_host_pipeline windows of that
    # many MiB per rank, with H2D / collective / D2H of consecutive windows on three streams
    for kind in ("pageable", "pinned"):
        if kind == "pageable":
            h_send, h_recv = np.ones(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        else:
            h_send = torch.ones(n, dtype=torch.float32).pin_memory()
            h_recv = torch.zeros(n, dtype=torch.float32).pin_memory()
        for window in (0, 8, 16, 32, 128):
            comm.set_host_pipeline(window)
            h_recv[12345] = 0.0
            ca.check(ca.all_reduce_radix_batch(h_send, h_recv, n, ca.FLOAT32, ca.SUM, comm, 2, 1))
            reps = 3
            t0 = time.perf_counter()
            for _ in range(reps):
                ca.check(ca.all_reduce_radix_batch(h_send, h_recv, n, ca.FLOAT32, ca.SUM, comm, 2, 1))
            dt = (time.perf_counter() - t0) / reps
            key = kind if window == 0 else f"{kind}_pipelined_{window}MiB_windows"
            # 1 GiB goes in and 1 GiB comes out per call: bytes moved over PCIe / wall time
            out[key] = {"ms": round(dt * 1e3, 2), "GBps_both_directions": round(2 * 4 * n / dt / 1e9, 2)}
            assert float(h_recv[12345]) == 1.0
    comm.set_host_pipeline(0)
    d_send = torch.ones(n, dtype=torch.float32, device="cuda:0")
    d_recv = torch.zeros(n, dtype=torch.float32, device="cuda:0")
    ca.check(ca.all_reduce_radix_batch(d_send, d_recv, n, ca.FLOAT32, ca.SUM, comm, 2, 1))
    t0 = time.perf_counter()
    for _ in range(3):
        ca.check(ca.all_reduce_radix_batch(d_send, d_recv, n, ca.FLOAT32, ca.SUM, comm, 2, 1))
    out["device_resident_ms"] = round((time.perf_counter() - t0) / 3 * 1e3, 3)
    comm.destroy()
    emit({"e2e": out})


def bench_collective_kernels(args):
    """The kernels the 8-rank collective launches, at C4 (fp32) and C5 (bf16) full size: 8 virtual
    ranks on this GPU (chr_local_group: the real plans, the loopback transport's device copies
    instead of RCCL), every fused reduction timed with HIP events.  Unlike the one-GPU rehearsal
    of the N>1 line -- 8 processes time-sharing one GPU, whose event-timed kernels include the
    other processes' work -- nothing else runs beside these kernels; the leaves are the ones the
    loopback copies have just written, as RCCL's receives would leave them."""
    import torch

    import chiara_amd as ca

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, k, b = 8, 4, 4
    g = ca.LocalGroup(n, 0)
    rows = {}
    for dname, cdt, es in (("f32", ca.FLOAT32, 4), ("bf16", ca.BFLOAT16, 2)):
        count = (1 << 30) // es
        sends = [torch.empty(count * es, dtype=torch.uint8, device=dev) for _ in range(n)]
        recvs = [torch.empty(count * es, dtype=torch.uint8, device=dev) for _ in range(n)]
        for r, x in enumerate(sends):
            ca.check(ca.fill(x, count, cdt, 0, SEED, r, stream=g.stream))
        for slices in (0, 8):
            for batched in (True, False):  # the ranks' trees of a step in shared grids, or one grid per rank
                g.set_slices(slices)
                g.set_batching(batched)
                ca.check(g.all_reduce_radix_batch(sends, recvs, count, cdt, ca.SUM, k, b))  # warm: plans, scratch
                g.profile(True)
                g.profile_read()
                reps = 3
                for _ in range(reps):
                    ca.check(g.all_reduce_radix_batch(sends, recvs, count, cdt, ca.SUM, k, b))
                ms, by, launches = g.profile_read()
                g.profile(False)
                ach = by / (ms * 1e-3) / 1e9
                rows[f"{'c4' if dname == 'f32' else 'c5'}_{dname}_slices_{slices or 'auto'}"
                     f"{'' if batched else '_per_rank_launches'}"] = {
                    "launches_per_call_all_ranks": launches // reps, "kernel_ms_per_call_all_ranks": round(ms / reps, 4),
                    "algorithmic_bytes_per_call_all_ranks": int(by / reps), "achieved_GBps": round(ach, 1),
                    "frac": round(ach / HBM_PEAK_GBPS, 4)}
        g.set_slices(0)
        g.set_batching(True)
        del sends, recvs
        torch.cuda.empty_cache()
    g.destroy()
    for dname, cdt, es in (("f32", ca.FLOAT32, 4), ("bf16", ca.BFLOAT16, 2)):
        for slices in (4, 8):
            for recv_copies in (False, True):
                key = f"{'c4' if dname == 'f32' else 'c5'}_{dname}_rank0_alone_slices_{slices}" + \
                      ("_after_recv_copies" if recv_copies else "")
                rows[key] = replay_rank_trees(ca, torch, dev, cdt, es, (1 << 30) // es, n, k, b, slices, recv_copies)
                torch.cuda.empty_cache()
    emit({"collective_kernels": {"workload": "all_reduce_radix_batch fused reductions, 8 virtual ranks, k=4, b=4, "
                                             "1 GiB per rank, flat schedule, each reduce phase of a call timed as one "
                                             "span; the ranks' trees of a step share grids of up to 8 trees "
                                             "(*_per_rank_launches: one grid per rank and step, as each GPU of a "
                                             "node launches); *_rank0_alone rows: rank 0's own trees on its own "
                                             "send/recv/STAGE only", "rows": rows}})


def bench_rank_trees(args):
    """Only the rank-alone rows of --collective-kernels (one GPU's own grids of a C4 / C5 call at 4 and
    8 slices, with and without the receive copies in front): small enough to run under rocprofv3
    --kernel-trace, whose per-dispatch durations give the grids' own time beside the spans."""
    import torch

    import chiara_amd as ca

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rows = {}
    for dname, cdt, es in (("f32", ca.FLOAT32, 4), ("bf16", ca.BFLOAT16, 2)):
        for slices in (4, 8):
            for recv_copies in (False, True):
                key = f"{'c4' if dname == 'f32' else 'c5'}_{dname}_rank0_alone_slices_{slices}" + \
                      ("_after_recv_copies" if recv_copies else "")
                rows[key] = replay_rank_trees(ca, torch, dev, cdt, es, (1 << 30) // es, 8, 4, 4, slices, recv_copies,
                                              graph=False)
                torch.cuda.empty_cache()
    emit({"rank_trees": {"workload": "rank 0's fused reductions of one all_reduce_radix_batch call, 8 ranks, k=4, "
                                     "b=4, 1 GiB per rank, flat schedule, on its own send/recv/STAGE", "rows": rows}})


def bench_collective_kernels_small(args):
    """The fused reductions of the smaller multi-GPU configs, on virtual ranks as above: the N=2 and
    N=4 lines' allreduces (1 GiB fp32 per rank, b = N, k = min(4, N): 2- and 4-leaf trees) and C3
    (reduce-scatter, 2 ranks, 256 MiB fp32 send buffer, radix 2, b = 1 and 2: 2-leaf trees), each
    with the ranks' trees of a step in shared grids and with one grid per rank.  Also CHiArA's phases as
    stand-alone collectives at 8 ranks, 1 GiB fp32 send buffer per rank: intra_reduce_scatter_radix_batch
    (b = 2, k = 2: two stages of recexch folds, m = 1) and inter_reduce_linear (b = 2: the roots fold
    nnodes - 1 = 3 chunks, m = 3), whose reductions run on k_reduce_vec (no trees: batching does not apply)."""
    import torch

    import chiara_amd as ca

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rows = {}
    cases = [("ar_n2_k2_b2", "ar", 2, 2, 2, 1 << 28), ("ar_n4_k4_b4", "ar", 4, 4, 4, 1 << 28),
             ("c3_rs_n2_k2_b1", "rs", 2, 2, 1, 1 << 25), ("c3_rs_n2_k2_b2", "rs", 2, 2, 2, 1 << 25),
             ("phase_intra_rs_n8_k2_b2", "irs", 8, 2, 2, 1 << 25), ("phase_inter_linear_n8_b2", "ilr", 8, 2, 2, 1 << 27)]
    phase_mode = {"irs": ca.MODE_INTRA_REDUCE_SCATTER, "ilr": ca.MODE_INTER_REDUCE_LINEAR}
    for name, mode, n, k, b, cnt in cases:
        g = ca.LocalGroup(n, 0)
        nnodes = n // b
        niters = nnodes // b + (1 if nnodes % b else 0)
        # send / recv elements per rank (the phases: intra_reduce_scatter_radix.cpp:241-247, inter_linear_reduce.cpp:39-46)
        total, out = {"ar": (cnt, cnt), "rs": (cnt * n, cnt), "irs": (cnt * n, niters * cnt * b),
                      "ilr": (niters * cnt * b, cnt * b)}[mode]
        sends = [torch.empty(total * 4, dtype=torch.uint8, device=dev) for _ in range(n)]
        recvs = [torch.empty(out * 4, dtype=torch.uint8, device=dev) for _ in range(n)]
        for r, x in enumerate(sends):
            ca.check(ca.fill(x, total, ca.FLOAT32, 0, SEED, r, stream=g.stream))
        if mode in phase_mode:
            def fn(S, R, c, dt, op, k_, b_, m=phase_mode[mode], g=g):
                return g.phase_collective(m, S, R, c, dt, op, k_, b_)
        else:
            fn = g.all_reduce_radix_batch if mode == "ar" else g.reduce_scatter_radix_batch
        for batched in ((True,) if mode in phase_mode else (True, False)):
            g.set_batching(batched)
            ca.check(fn(sends, recvs, cnt, ca.FLOAT32, ca.SUM, k, b))  # warm: plans, scratch
            g.profile(True)
            g.profile_read()
            reps = 5
            for _ in range(reps):
                ca.check(fn(sends, recvs, cnt, ca.FLOAT32, ca.SUM, k, b))
            ms, by, launches = g.profile_read()
            g.profile(False)
            ach = by / (ms * 1e-3) / 1e9
            rows[name + ("" if batched else "_per_rank_launches")] = {
                "launches_per_call_all_ranks": launches // reps, "kernel_ms_per_call_all_ranks": round(ms / reps, 4),
                "algorithmic_bytes_per_call_all_ranks": int(by / reps), "achieved_GBps": round(ach, 1),
                "frac": round(ach / HBM_PEAK_GBPS, 4)}
        g.destroy()
        del sends, recvs
        torch.cuda.empty_cache()
    knobs = {k: v for k, v in os.environ.items() if k.startswith("CHR_")}
    emit({"collective_kernels_small": {"workload": "fused reductions of the N=2 / N=4 allreduce lines (1 GiB fp32 per "
                                                   "rank), C3 (reduce-scatter, 2 ranks, 256 MiB send) and the "
                                                   "stand-alone phases (8 ranks, 1 GiB send), virtual ranks on one "
                                                   "GPU, each reduce phase timed as one span",
                                       "env": knobs, "rows": rows}})


def replay_rank_trees(ca, torch, dev, cdt, es, count, n, k, b, slices, recv_copies, reps=5, graph=True):
    """Rank 0's fused reductions of one C4/C5 call, alone, on rank 0's own buffers: send, recv and
    STAGE (~3 GiB), the working set one GPU of an 8-GPU node holds.  The 8-virtual-rank rows above
    hold all eight ranks' buffers (~25 GiB, past the translation cliff of DESIGN §4.1) and so
    under-state the per-GPU case.  The plan is the flat schedule's own (describe_plan), its tree
    ops batched per step as the executor batches them (chr_reduce_tree_batch); leaf data are
    synthetic (timing only, SUM is data-independent).  With recv_copies, every step's receives are
    first written into STAGE by device copies from SEND (as RCCL's receives would leave them).

    `frac` (round 5): one call's grids back to back as ONE gated HIP-event span (the median of `reps`
    calls), every inter-grid gap included; with recv_copies, the span of copies + grids minus the span
    of the same copies alone.  `event_pairs_frac`: rounds 3-4's figure, an event pair around every
    grid, whose extra event packets add ~2-5 us per grid and +-3 % of noise (profiles/r05/ab_treebl/)."""
    plan = ca.parse_plan(ca.describe_plan(ca.MODE_ALLREDUCE, n, 0, k, b, count, slices, ca.SCHEDULE_FLAT))
    h = plan["header"]
    bufs = {name: torch.empty(max(1, h[name.lower()]) * es, dtype=torch.uint8, device=dev)
            for name in ("SEND", "RECV", "STAGE", "ACC")}
    s = torch.cuda.current_stream(dev)
    for i, (name, t) in enumerate(bufs.items()):
        ca.check(ca.fill(t, t.numel() // es, cdt, 0, SEED, i, stream=s))
    ptr = lambda ref: bufs[ref[0]].data_ptr() + ref[1] * es  # noqa: E731
    steps = []
    for st in plan["steps"]:
        trees = [op for op in st["post"] if op[0] == "tree"]
        if trees:
            assert len({len(op[4]) for op in trees}) == 1 and len({op[3] for op in trees}) == 1
        copies = [(bufs[dst[0]].narrow(0, dst[1] * es, cnt * es), bufs["SEND"].narrow(0, 0, cnt * es))
                  for (_, dst, cnt) in st["recvs"]]
        steps.append((trees, copies))
    by = sum((len(op[4]) + 2) * op[3] * es for trees, _ in steps for op in trees)
    grids = sum(1 for trees, _ in steps if trees)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in steps]

    def call(with_copies, with_trees, pairs=False):
        for (trees, copies), (e0, e1) in zip(steps, evs):
            if with_copies:
                for d, src in copies:
                    d.copy_(src)  # D2D on s
            if not trees or not with_trees:
                continue
            if pairs:
                e0.record(s)
            ca.check(ca.reduce_tree_batch([ptr(op[1]) for op in trees],
                                          [[ptr(op[2])] + [ptr(x) for x in op[4]] for op in trees],
                                          [op[5][0] for op in trees], [op[5][1] for op in trees],
                                          trees[0][3], cdt, ca.SUM, s))
            if pairs:
                e1.record(s)

    g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def span(with_copies, with_trees):
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            if hasattr(torch.cuda, "_sleep"):  # host enqueue latency out of the span (bench_bucket's gate)
                torch.cuda._sleep(GATE_CYCLES)
            g0.record(s)
            call(with_copies, with_trees)
            g1.record(s)
            torch.cuda.synchronize()
            out.append(g0.elapsed_time(g1))
        return sorted(out)[len(out) // 2]

    for _ in range(2):
        call(recv_copies, True)
    ms = span(recv_copies, True)
    row = {}
    if recv_copies:
        ms_c = span(True, False)
        row["copies_ms_per_call"] = round(ms_c, 4)
        ms -= ms_c
    ach = by / (ms * 1e-3) / 1e9
    # rounds 3-4: an event pair around every grid
    pm = 0.0
    for _ in range(reps):
        call(recv_copies, True, pairs=True)
        torch.cuda.synchronize()
        pm += sum(e0.elapsed_time(e1) for (trees, _), (e0, e1) in zip(steps, evs) if trees)
    pm /= reps
    row.update({"launches_per_call": grids, "kernel_ms_per_call": round(ms, 4),
                "algorithmic_bytes_per_call": int(by), "working_set_GiB": round(
                    (h["send"] + h["recv"] + h["stage"] + h["acc"]) * es / 2**30, 2),
                "achieved_GBps": round(ach, 1), "frac": round(ach / HBM_PEAK_GBPS, 4),
                "event_pairs_ms_per_call": round(pm, 4),
                "event_pairs_frac": round(by / (pm * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)})
    if graph and not recv_copies:
        row["graph_replay"] = trees_span_eager_vs_graph(ca, torch, s, steps, ptr, cdt, by)
    del bufs
    return row


def trees_span_eager_vs_graph(ca, torch, s, steps, ptr, cdt, bytes_per_call, reps=5):
    """One call's tree grids back to back (no receive copies between them), timed as ONE span per
    call: issued eagerly, and captured once in a HIP graph and replayed (does a
    graph remove the packet processor's turnaround between grids?).  The span includes every
    inter-grid gap, unlike the per-grid event pairs above."""
    launches = [([ptr(op[1]) for op in trees], [[ptr(op[2])] + [ptr(x) for x in op[4]] for op in trees],
                 [op[5][0] for op in trees], [op[5][1] for op in trees], trees[0][3])
                for trees, _ in steps if trees]

    def issue(st):
        for outs, leaves, comb, swaps, cnt in launches:
            ca.check(ca.reduce_tree_batch(outs, leaves, comb, swaps, cnt, cdt, ca.SUM, st))

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {}
    for mode in ("eager", "graph"):
        if mode == "graph":
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                issue(torch.cuda.current_stream())
            go = graph.replay
        else:
            def go():
                issue(s)
        go()
        torch.cuda.synchronize()
        spans = []
        for _ in range(reps):
            if hasattr(torch.cuda, "_sleep"):  # host enqueue latency out of the span (bench_bucket's gate)
                torch.cuda._sleep(GATE_CYCLES)
            e0.record(s)
            go()
            e1.record(s)
            torch.cuda.synchronize()
            spans.append(e0.elapsed_time(e1))
        ms = sorted(spans)[len(spans) // 2]
        ach = bytes_per_call / (ms * 1e-3) / 1e9
        out[mode] = {"span_ms_per_call_median": round(ms, 4), "grids_per_call": len(launches),
                     "achieved_GBps": round(ach, 1), "frac": round(ach / HBM_PEAK_GBPS, 4)}
        if mode == "graph":
            del graph
    return out


# ---- N > 1: launching the ranks ----------------------------------------------------------------

DEFAULT_DEADLINE_S = 240.0   # the whole N>1 line, from the launch (CHR_BENCH_DEADLINE_S overrides)
KILL_GRACE_S = 180.0         # the launcher kills the rank group this long after the deadline


def launch_command(argv, nproc, port):
    """The child command that starts `nproc` rank processes of this script, one per GPU."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
            "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.abspath(__file__), *argv]


def plan_launch(args, argv, env, device_count, port=0):
    """None when this process is the bench itself (one rank of an external launcher, or --gpus 1);
    otherwise the command that starts --gpus rank processes.  More ranks than visible devices is an
    error (never a silent fall-back to the one-GPU line), unless CHR_BENCH_VIRTUAL_HOSTS=1 rehearses
    the N>1 path with ranks sharing a device."""
    if "WORLD_SIZE" in env or args.gpus <= 1:
        return None
    if args.gpus > device_count and env.get("CHR_BENCH_VIRTUAL_HOSTS") != "1":
        raise ValueError(f"--gpus {args.gpus}: only {device_count} GPU(s) visible; one rank per GPU "
                         f"(CHR_BENCH_VIRTUAL_HOSTS=1 rehearses ranks sharing a GPU)")
    return launch_command(argv, args.gpus, port)


def free_port():
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def deadline_s(env=os.environ):
    return float(env.get("CHR_BENCH_DEADLINE_S", DEFAULT_DEADLINE_S))


def run_launcher(cmd):
    """Run the rank group as a child (never exec: this process may not replace itself), forward rank
    0's one JSON line to stdout, everything else to stderr, and return the group's exit status.  The
    group gets the launch time, so every rank measures the deadline from the same instant."""
    import signal

    env = dict(os.environ, CHR_BENCH_T0=repr(time.time()))
    limit = deadline_s(env) + KILL_GRACE_S
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True, start_new_session=True)
    try:
        out, _ = proc.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        out, _ = proc.communicate()
        print(f"bench.py: rank group killed {limit:.0f} s after launch", file=sys.stderr)
        return 124
    lines = []
    for ln in out.splitlines():
        try:
            obj = json.loads(ln)
        except ValueError:
            obj = None
        if isinstance(obj, dict) and "metric" in obj:
            lines.append(ln)
        elif ln.strip():
            print(ln, file=sys.stderr)
    if lines:
        emit(json.loads(lines[-1]))
    return proc.returncode if proc.returncode is not None else 1


class Deadline:
    """The N>1 line's wall-clock budget.  Rank 0 decides and broadcasts, so every rank skips the same
    context entries (a collective one rank skips and another runs would hang)."""

    def __init__(self, dist, env=os.environ):
        self.dist = dist
        self.t_end = float(env.get("CHR_BENCH_T0", time.time())) + deadline_s(env)

    def passed(self):
        import torch

        t = torch.tensor([1.0 if time.time() > self.t_end else 0.0], dtype=torch.float64)
        self.dist.broadcast(t, 0)
        return bool(t.item())


# ---- N > 1: which wire RCCL used -----------------------------------------------
# RCCL logs every connection it sets up, one line per channel and direction, under NCCL_DEBUG=INFO with
# the INIT subsystem (its P2P / SHM / NET transports log under INIT|<transport>).  The formats, from the
# strings of the librccl.so the process loads (torch's):
#   Channel %02d/%01d : %d[%lx] -> %d[%lx] via P2P/IPC%s%s comm %p nRanks %02d        (xGMI: peer GPU mapped)
#   Channel %02d/%01d : %d[%lx] -> %d[%lx] via P2P/direct pointer%s comm %p nRanks %02d
#   Channel %02d : %d[%lx] -> %d[%lx] via SHM/%s/%s comm %p nRanks %02d            (host shared memory)
#   Channel %02d/%d : %d[%d] -> %d[%d] [send] via NET/%s/%d%s%s%s comm %p nRanks %02d (network, e.g. Socket)
# Each rank writes its own file (NCCL_DEBUG_FILE), never stdout.  The flat schedule's ncclSend/ncclRecv
# connect lazily, so the file is read after the first collective call.
_RCCL_CHANNEL = re.compile(r"Channel\s+\d+(?:/\d+)?\s*:\s*(\d+)\[[0-9a-fA-Fx]+\]\s*->\s*(\d+)\[[0-9a-fA-Fx]+\]"
                           r"\s*(?:\[(send|receive)\]\s*)?via\s+(.+?)\s+comm\s+(0x[0-9a-fA-F]+|\S+)\s+nRanks\s+(\d+)")


def rccl_log_env(rank, root):
    """Environment that makes RCCL log its connection setup for this rank into its own file under root."""
    os.makedirs(root, exist_ok=True)
    return {"NCCL_DEBUG": "INFO", "NCCL_DEBUG_SUBSYS": "INIT", "NCCL_DEBUG_FILE": os.path.join(root, f"rccl.rank{rank}.%p.log")}


def parse_rccl_transports(lines, nranks=None):
    """{(src, dst): set of transports} from RCCL INFO lines ("P2P/IPC", "SHM/direct/direct", "NET/Socket/0"
    ...), keeping only communicators of `nranks` ranks when given.  A transport is named up to its
    first space; trailing read/write modes stay in it."""
    pairs = {}
    for ln in lines:
        m = _RCCL_CHANNEL.search(ln)
        if not m:
            continue
        if nranks is not None and int(m.group(6)) != nranks:
            continue
        src, dst, tr = int(m.group(1)), int(m.group(2)), m.group(4).strip()
        pairs.setdefault((src, dst), set()).add(tr)
    return pairs


def transport_family(tr):
    """"P2P" (a GPU peer mapped directly: xGMI on an MI355X node), "SHM", "NET", "COLLNET" or "?"."""
    head = tr.split("/")[0].upper()
    return head if head in ("P2P", "SHM", "NET", "COLLNET") else "?"


def rccl_library():
    """Which librccl this process runs and its version: the path from /proc/self/maps (the copy torch loaded, which
    libchiara.so resolves to) and ncclGetVersion() of that copy (RTLD_NOLOAD: never a second one).  The co-residency
    cap was tuned against two RCCL builds with different LDS footprints, so the node record names it."""
    import ctypes

    path = None
    try:
        with open("/proc/self/maps") as f:
            for ln in f:
                p = ln.split()[-1] if len(ln.split()) >= 6 else ""
                if os.path.basename(p).startswith("librccl"):
                    path = p
                    break
    except OSError:
        pass
    rec = {"library": path, "version": None, "version_code": None}
    if path:
        try:
            lib = ctypes.CDLL(path, mode=os.RTLD_NOLOAD | os.RTLD_LAZY)
            v = ctypes.c_int(0)
            if lib.ncclGetVersion(ctypes.byref(v)) == 0:
                code = v.value
                rec["version_code"] = code
                rec["version"] = (f"{code // 10000}.{code % 10000 // 100}.{code % 100}" if code >= 10000 else
                                  f"{code // 1000}.{code % 1000 // 100}.{code % 100}")
        except (OSError, AttributeError) as e:
            rec["version"] = f"error: {e}"[:80]
    return rec


def rccl_record(infos, pair_sets, world, libs=None):
    """The N>1 line's `rccl` object from every rank's chr_comm_info() and parsed pairs (rank order).
    xgmi is true only when RCCL's communicator holds `world` ranks with distinct user ranks, the ranks
    sit on `world` distinct PCI devices, at least one connection was logged, and every logged connection
    is a P2P one; false otherwise (a fall-back to SHM or NET shows as false, with the transports)."""
    merged = {}
    for ps in pair_sets:
        for k, v in ps.items():
            merged.setdefault(k, set()).update(v)
    counts = {}
    for v in merged.values():
        for tr in v:
            counts[tr] = counts.get(tr, 0) + 1
    fams = {transport_family(tr) for v in merged.values() for tr in v}
    nr = {i["nranks"] for i in infos}
    ranks = [i["rank"] for i in infos]
    buses = [i["pci_bus_id"] for i in infos]
    why = [w for bad, w in ((nr != {world}, f"RCCL communicator sizes {sorted(nr)} for {world} ranks"),
                            (sorted(ranks) != list(range(world)), f"user ranks {ranks}"),
                            (len(set(buses)) != world, f"{len(set(buses))} distinct PCI devices for {world} ranks"),
                            (not merged, "no connection lines in the RCCL logs"),
                            (bool(merged) and fams != {"P2P"},
                             f"non-P2P transports: {sorted(f for f in fams if f != 'P2P')}")) if bad]
    ok = not why
    why = why or None
    lib = {}
    if libs is not None:  # rank 0's library, and whether every rank runs the same one
        lib = dict(libs[0])
        lib["same_on_all_ranks"] = all(x == libs[0] for x in libs)
    return {**lib, "nranks": sorted(nr)[0] if len(nr) == 1 else sorted(nr), "user_ranks": ranks,
            "devices": [i["device"] for i in infos],
            "pci_bus_ids": buses, "transports": dict(sorted(counts.items())),
            "pairs": {f"{a}->{b}": "+".join(sorted(v)) for (a, b), v in sorted(merged.items())},
            "pairs_logged": len(merged), "xgmi": ok, "not_xgmi_because": why,
            "source": "ncclCommCount / ncclCommUserRank / ncclCommCuDevice / hipDeviceGetPCIBusId per rank; "
                      "transports from each rank's NCCL_DEBUG_FILE (NCCL_DEBUG=INFO, NCCL_DEBUG_SUBSYS=INIT)"}


def read_rccl_logs(root, rank, pid=None):
    """This rank's RCCL log lines under root; with `pid`, only the file that process wrote (NCCL_DEBUG_FILE's %p),
    so a file another run left behind is never parsed into the record."""
    out = []
    try:
        names = sorted(f for f in os.listdir(root) if f.startswith(f"rccl.rank{rank}.")
                       and (pid is None or f == f"rccl.rank{rank}.{pid}.log"))
    except OSError:
        return out
    for f in names:
        try:
            with open(os.path.join(root, f), errors="replace") as fh:
                out.extend(fh.read().splitlines())
        except OSError:
            pass
    return out


# ---- N > 1: hierarchical allreduce over RCCL ---------------------------------------------------

def bench_allreduce(args):
    import torch
    import torch.distributed as dist

    import chiara_amd as ca

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", rank)) % max(1, torch.cuda.device_count())
    if os.environ.get("CHR_BENCH_VIRTUAL_HOSTS") == "1":
        # rehearsal of the N>1 path on fewer GPUs than ranks: distinct host ids make RCCL
        # use its socket transport between ranks that share a device (numbers meaningless)
        os.environ["NCCL_HOSTID"] = f"chiara-bench-vhost-{rank}"
        os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    import datetime

    # a rank that dies must not leave the others in a gloo barrier for gloo's default 30 minutes
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=900))
    deadline = Deadline(dist)
    # RCCL's connection log, one file per rank (rccl_log_env), set before this process's first RCCL call, in a
    # directory named by a token rank 0 draws for this run (and read back by this process's pid only)
    log_root = None
    if os.environ.get("CHR_BENCH_RCCL_LOG", "1") != "0":
        import tempfile
        import uuid

        token = [uuid.uuid4().hex[:12] if rank == 0 else None]
        dist.broadcast_object_list(token, 0)
        log_root = os.path.join(tempfile.gettempdir(),
                                f"chiara_bench_rccl_{os.environ.get('MASTER_PORT', '0')}_{token[0]}")
        os.environ.update(rccl_log_env(rank, log_root))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    comm = ca.Comm.from_torch_distributed(device=local)
    # every blocking call (tuning included) and every comm.synchronize() gives up after this long:
    # a collective that never completes becomes ERR_TIMEOUT (communicator aborted), not a hang
    comm.set_timeout(int(os.environ.get("CHR_BENCH_TIMEOUT_MS", "300000")))
    b = 4 if world % 4 == 0 else world
    k = min(4, b) if b > 1 else 2
    dt = ca.FLOAT32 if args.dtype == "f32" else ca.BFLOAT16
    es = 4 if args.dtype == "f32" else 2
    count = args.count or ((1 << 30) // es)
    count -= count % world
    stream = comm.stream
    send = torch.empty(count * es, dtype=torch.uint8, device=dev)
    recv = torch.empty(count * es, dtype=torch.uint8, device=dev)
    ca.check(ca.fill(send, count, dt, 0, SEED, rank, stream=stream))
    torch.cuda.synchronize()
    # The metric runs CHR_SCHEDULE_AUTO (unless CHR_SCHEDULE names one): the first call for these
    # arguments times FLAT / FLAT_SEQ / FLAT_AG at several pipeline depths, the ranks agree on the
    # slowest rank's times and every later call uses the fastest.  That setup call (plan compile,
    # scratch, tuning) runs here, before warmup and outside the timed region, like communicator init.
    sched_env = os.environ.get("CHR_SCHEDULE")
    metric_sched = ca.SCHEDULE_AUTO if sched_env in (None, "auto", "6") else None
    if metric_sched is not None:
        comm.set_schedule(metric_sched)
    ca.check(ca.all_reduce_radix_batch(send, recv, count, dt, ca.SUM, comm, k, b))
    tuned = comm.tuned_schedule(ca.MODE_ALLREDUCE, count, dt, k, b)  # AUTO's choice, or the fixed schedule's depth
    sched_names = {0: "reference", 1: "balanced", 2: "flat", 3: "exact", 4: "flat_ag", 5: "flat_seq", 7: "flat_1shot"}
    # which ranks and GPUs RCCL's communicator holds, and which wire each peer pair got: the setup call
    # above has connected every pair the schedule uses (ncclSend/ncclRecv connect lazily)
    ca.check(comm.synchronize())
    try:
        info = comm.info()
    except Exception as e:
        info = {"nranks": -1, "rank": -1, "device": -1, "pci_bus_id": f"error: {e}"[:80]}
    pairs = parse_rccl_transports(read_rccl_logs(log_root, rank, os.getpid()), nranks=world) if log_root else {}
    allinfo, allpairs, alllibs = [None] * world, [None] * world, [None] * world
    dist.all_gather_object(allinfo, info)
    dist.all_gather_object(allpairs, pairs)
    dist.all_gather_object(alllibs, rccl_library())
    rccl = rccl_record(allinfo, allpairs, world, alllibs)
    if not log_root:
        rccl["not_xgmi_because"] = "CHR_BENCH_RCCL_LOG=0: transports not logged"
    for _ in range(args.warmup):
        ca.check(ca.all_reduce_radix_batch(send, recv, count, dt, ca.SUM, comm, k, b, async_op=True))
    ca.check(comm.synchronize())
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ca.check(ca.all_reduce_radix_batch(send, recv, count, dt, ca.SUM, comm, k, b, async_op=True))
    t_enq = time.perf_counter() - t0  # host time to enqueue every call (RCCL groups, launches, events)
    ca.check(comm.synchronize())  # under the timeout; the torch sync below then returns at once
    torch.cuda.synchronize()
    dist.barrier()
    el = time.perf_counter() - t0
    t = torch.tensor([el], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    el = float(t.item())
    S = count * es
    algbw = S * args.steps / el / 1e9
    busbw = algbw * 2 * (world - 1) / world
    if args.dump_outputs and rank == 0:  # what the last timed call left in rank 0's recv
        dump_outputs(torch, args.dump_outputs, "recv",
                     recv[:count * es].view(torch.float32 if es == 4 else torch.bfloat16))
    # roofline of the dominant OUR kernel inside the collective (--full): one more (untimed) call
    # with HIP events around every fused reduction launch on the comm stream
    red_ms, red_bytes, red_n, phases = 0.0, 0.0, 0, {}
    if args.full:
        comm.profile(True)
        ca.check(ca.all_reduce_radix_batch(send, recv, count, dt, ca.SUM, comm, k, b, async_op=True))
        torch.cuda.synchronize()
        red_ms, red_bytes, red_n = comm.profile_read()
        phases = comm.profile_phases()  # transfer ms per plan phase (DEBUG_MODE phase timers' analogue)
        comm.profile(False)
    # the metric's output on every rank (--full): bit-identical across ranks and within the stated tolerance of
    # the fp64 sum (recv holds the last call's result; every call computes the same bits)
    check = None
    if args.full:
        try:
            def fill_rank(r, buf):
                ca.check(ca.fill(buf, count, dt, 0, SEED, r, stream=stream))
                torch.cuda.synchronize()
            check = result_check(torch, dist, recv, count, es, world, fill_rank)
            # and bit for bit against a known answer: one more call of the same configuration on integer-valued
            # inputs
            check.update(exact_check(
                torch, dist, send, recv, count, es, rank,
                lambda: ca.check(ca.all_reduce_radix_batch(send, recv, count, dt, ca.SUM, comm, k, b)), world))
            fill_rank(rank, send)  # the metric's inputs back for the comparison lines
        except Exception as e:  # recorded, never hidden: line_problems() flags a full line without a passing check
            check = {"error": str(e)[:200]}
        torch.cuda.empty_cache()
    allph = [None] * world
    dist.all_gather_object(allph, phases)
    phases_ms = {}
    for ph in allph:  # max over ranks, per phase
        for nm, v in ph.items():
            phases_ms[nm] = round(max(phases_ms.get(nm, 0.0), v), 4)
    stats = torch.tensor([red_ms, red_bytes, float(red_n)], dtype=torch.float64)
    gathered = [torch.zeros_like(stats) for _ in range(world)]
    dist.all_gather(gathered, stats)
    busiest = max(gathered, key=lambda t: float(t[1]))  # the rank that reduces the most bytes
    roofline = None
    if float(busiest[0]) > 0:
        ach = float(busiest[1]) / (float(busiest[0]) * 1e-3) / 1e9
        traffic, stale = None, None
        pmc_key, sym = None, None
        # the kernel the metric's plan launches (its tuned schedule and depth)
        mplan = ca.parse_plan(ca.describe_plan(ca.MODE_ALLREDUCE, world, rank, k, b, count,
                                               tuned[1] if tuned else 1, tuned[0] if tuned else 2))
        entry, why = reduction_pmc(mplan)
        if entry is not None and args.dtype == "f32":
            pmc_key, sym = entry
            ratio, stale = pmc_ratio(pmc_key, sym)
            traffic = None if ratio is None else round(float(busiest[1]) * ratio)
        else:
            stale = why or f"no PMC entry for the {world}-rank {args.dtype} reductions"
        roofline = {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    "frac": round(ach / HBM_PEAK_GBPS, 4), "traffic": traffic,
                    "kernel": (sym or "chr::k_reduce_tree / k_reduce_vec") + " (fused reductions inside the collective, "
                                                                          "busiest rank)",
                    "algorithmic_bytes_per_call": float(busiest[1]), "launches_per_call": int(busiest[2]),
                    "kernel_ms_per_call": round(float(busiest[0]), 4),
                    # one GPU's own grids (one rank per GPU): the fixed per-grid cost shows directly
                    "grids_per_call": int(busiest[2]),
                    "avg_grid_us": round(float(busiest[0]) * 1e3 / max(1, int(busiest[2])), 2)}
        if stale:
            roofline["traffic_stale"] = stale
        else:
            roofline["traffic_source"] = f"profiles/pmc_latest.json {pmc_key} ratio x algorithmic bytes"
    # bytes on the busiest directed link of this schedule (max over ranks; slicing only splits messages)
    if tuned is not None:
        sched = tuned[0]
    else:
        sched = {"reference": 0, "0": 0, "balanced": 1, "1": 1, "exact": 3, "3": 3, "flat_ag": 4, "4": 4,
                 "flat_seq": 5, "5": 5}.get(sched_env or "flat", 2)
    plan = ca.parse_plan(ca.describe_plan(ca.MODE_ALLREDUCE, world, rank, k, b, count, 1, sched))
    per_peer = {}
    for st in plan["steps"]:
        for peer, _, cnt in st["sends"]:
            per_peer[peer] = per_peer.get(peer, 0) + cnt * es
    lb = torch.tensor([float(max(per_peer.values()) if per_peer else 0)], dtype=torch.float64)
    dist.all_reduce(lb, op=dist.ReduceOp.MAX)
    link_bytes = int(lb.item())
    # the reference CPU+MPI path on this box's host cores, after the metric's GPU timing and before
    # the context entries, so the deadline can only cost context (rank 0 runs it; the other ranks
    # wait at the barrier)
    cpu = None
    if rank == 0 and args.full and not args.no_cpu_baseline:
        cpu = cpu_baseline_collective(world, k, b, count, es, budget_s=deadline.t_end - time.time() - 30)
    dist.barrier()
    compare = None
    if args.full and not args.no_compare:
        compare = compare_lines(args, ca, torch, dist, comm, send, recv, count, dt, k, b, world, dev, metric_sched,
                                deadline)
    if rank == 0:
        line = {
            "metric": METRIC, "value": round(world * S * args.steps / el / 1e9, 2), "unit": "GB/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(el / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"all_reduce_radix_batch, {S >> 20} MiB per rank, k={k}, b={b}, RCCL send/recv "
                                   f"(the wire each peer pair used: rccl.pairs), device-resident", "k": k, "b": b,
                       "count": count,
                       "schedule": (f"{'auto -> ' if metric_sched is not None else ''}"
                                    f"{sched_names.get(tuned[0], tuned[0])}, {tuned[1]} slices" if tuned
                                    else sched_env or "flat"),
                       "slices": tuned[1] if tuned else None,
                       # the metric's calls run with the communicator's compute stream beside the transfers;
                       # with >= 2 slices a call reduces slice s while slice s+1 moves
                       "overlap": bool(comm.overlap and tuned is not None and tuned[1] >= 2),
                       "parallelism": f"collective x{world}",
                       # who started the ranks: bench.py itself (--gpus N) or an external launcher
                       "launcher": "bench.py" if "CHR_BENCH_T0" in os.environ else "external"},
            "algbw_GBps": round(algbw, 2), "busbw_GBps": round(busbw, 2),
            "aggregate_GBps": round(world * S * args.steps / el / 1e9, 2),
            "definitions": LINE_DEFINITIONS_NN,
            # rank 0's host enqueue time per call: close to ms_per_step would mean host-bound
            "host_enqueue_ms_per_call": round(t_enq / args.steps * 1e3, 4),
            # a directed pair's bytes cross one direction of one link: the bound is the per-direction rate
            "xgmi_roofline": {"per_link_GBps_bidirectional": XGMI_LINK_GBPS, "per_link_per_direction_GBps": XGMI_DIR_GBPS,
                              "aggregate_per_direction_GBps": 7 * XGMI_DIR_GBPS,
                              # against the task-stated 153 GB/s per link and its 7-link aggregate (SURVEY 8(d);
                              # the keys rounds 1-3 reported)
                              "busbw_frac_per_link": round(busbw / XGMI_LINK_GBPS, 4),
                              "busbw_frac_aggregate": round(busbw / (7 * XGMI_LINK_GBPS), 4),
                              # against one direction of a link (a directed pair's bytes cross one direction)
                              "busbw_frac_per_link_direction": round(busbw / XGMI_DIR_GBPS, 4),
                              "busbw_frac_aggregate_direction": round(busbw / (7 * XGMI_DIR_GBPS), 4),
                              # schedule-aware bound: the compiled plan's busiest directed link
                              "busiest_link_bytes": link_bytes,
                              "link_bound_ms": round(link_bytes / (XGMI_DIR_GBPS * 1e9) * 1e3, 4),
                              "frac": round(link_bytes / (XGMI_DIR_GBPS * 1e9) / (el / args.steps), 4)},
            "roofline": roofline, "cpu_baseline": cpu,
            # one profiled call (overlap on): transfer ms per plan phase, max over ranks
            "phase_transfer_ms": phases_ms,
            # RCCL's own view: ranks, GPUs and the transport of every connected pair (xgmi: all P2P)
            "rccl": rccl,
            # --full: roofline, phase_transfer_ms, cpu_baseline, result_check and compare beside the metric
            "full": bool(args.full),
        }
        if check is not None:
            line["result_check"] = check
        if cpu:
            line["gpu_vs_cpu"] = round(line["value"] / cpu["value"], 1)
        if compare:
            line["compare"] = compare
        emit(line)
    comm.destroy()
    dist.destroy_process_group()


RESULT_TOL_ULP = {"f32": 2.0 ** -23, "bf16": 2.0 ** -8}  # (n-1) x ulp x sum|x_i| per element


def result_check(torch, dist, recv, count, es, world, fill_rank, window=1 << 26):
    """The metric's output, checked on every rank without the oracle (which only the CPU-baseline leg may
    touch): (1) the ranks' recv buffers are bit-identical (each chunk is reduced once, at one root, then
    copied: all_reduce_radix_batch.cpp:529-756), by two position-weighted int64 checksums of the raw words;
    (2) every element is within DESIGN §7's stated tolerance of the fp64 sum of the N inputs, regenerated here
    with the same device generator: |x - sum| <= (N - 1) ulp sum|x_i| + 2^-126 (f32) / + 2^-133 (bf16),
    so a transport that delivered stale or misplaced bytes shows up in the node's own record.
    fill_rank(r, buf) writes rank r's input (count elements) into the byte buffer buf.  Windows of `window`
    elements bound the fp64 temporaries."""
    tdt = torch.float32 if es == 4 else torch.bfloat16
    words = recv[:count * es].view(torch.int32 if es == 4 else torch.int16)
    out = recv[:count * es].view(tdt)
    h1 = h2 = 0
    tmp = torch.empty(count * es, dtype=torch.uint8, device=recv.device)
    tol_ulp = RESULT_TOL_ULP["f32" if es == 4 else "bf16"]
    bad, worst, maxerr = 0, 0.0, 0.0
    for w0 in range(0, count, window):
        w1 = min(count, w0 + window)
        v = words[w0:w1].to(torch.int64)
        h1 += int(v.sum())
        idx = torch.arange(w0, w1, device=recv.device, dtype=torch.int64) % 1000003 + 1
        h2 += int((v * idx).sum())
    h1 &= (1 << 63) - 1
    h2 &= (1 << 63) - 1
    ref = torch.zeros(count, dtype=torch.float64, device=recv.device)
    mag = torch.zeros(count, dtype=torch.float64, device=recv.device)
    for r in range(world):
        fill_rank(r, tmp)
        x = tmp.view(tdt)
        for w0 in range(0, count, window):
            w1 = min(count, w0 + window)
            xd = x[w0:w1].double()
            ref[w0:w1] += xd
            mag[w0:w1] += xd.abs()
    floor = 2.0 ** -126 if es == 4 else 2.0 ** -133
    for w0 in range(0, count, window):
        w1 = min(count, w0 + window)
        err = (out[w0:w1].double() - ref[w0:w1]).abs()
        bound = (world - 1) * tol_ulp * mag[w0:w1] + floor
        bad += int((err > bound).sum())
        worst = max(worst, float((err / bound).max()))
        maxerr = max(maxerr, float(err.max()))
    del ref, mag, tmp
    mine = torch.tensor([float(h1), float(h2), float(bad), worst, maxerr], dtype=torch.float64)
    hs = [None] * world
    dist.all_gather_object(hs, (h1, h2))
    allv = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(allv, mine)
    return {"ranks_bit_identical": len(set(hs)) == 1,
            "within_tolerance": all(int(t[2]) == 0 for t in allv),
            "elements_checked_per_rank": count,
            "violations": int(sum(int(t[2]) for t in allv)),
            "max_err_over_bound": round(max(float(t[3]) for t in allv), 6),
            "max_abs_err": max(float(t[4]) for t in allv),
            "checksum_rank0": f"{hs[0][0]:016x}:{hs[0][1]:016x}",
            "tolerance": f"|x - fp64 sum| <= (N-1) x {tol_ulp:.3g} x sum|x_i| (DESIGN §7), every element, every rank"}


KNOWN_ANSWER_MUL, KNOWN_ANSWER_RANK = 2654435761, 40503


def known_answer_input(torch, idx, r):
    """Rank r's integer-valued input at positions idx (int64): in [-16, 15], so every partial sum of at most 8 ranks
    (|.| <= 128) is exact in f32 and bf16 whatever the association -- the answer is known without the oracle."""
    return ((idx * KNOWN_ANSWER_MUL + r * KNOWN_ANSWER_RANK) >> 7) % 32 - 16


def exact_check(torch, dist, send, recv, count, es, rank, run, world, window=1 << 26):
    """The reference harness's own check (Allreduce/main.cpp:55-69: known inputs, exact equality), at the metric's
    size and configuration: every rank's send buffer gets integer-valued data (known_answer_input), `run()` makes one
    call, and every element of every rank's output must EQUAL the sum of the N inputs -- bit for bit, on the wire and
    in the reductions, with no tolerance.  (Association order, which exact sums cannot show, is pinned by the
    reference's goldens and the full-size LocalGroup / RCCL-process tests.)"""
    if world > 16:  # |partial sums| <= 16 * world must stay within bf16's 8 significant bits
        return {"exact_known_answer": None, "exact": f"skipped: {world} ranks, exact only up to 16"}
    tdt = torch.float32 if es == 4 else torch.bfloat16
    src = send[:count * es].view(tdt)
    for w0 in range(0, count, window):
        w1 = min(count, w0 + window)
        idx = torch.arange(w0, w1, device=send.device, dtype=torch.int64)
        src[w0:w1] = known_answer_input(torch, idx, rank).to(tdt)
    sync = torch.cuda.synchronize if send.is_cuda else (lambda: None)
    sync()
    run()
    sync()
    out = recv[:count * es].view(tdt)
    bad = 0
    for w0 in range(0, count, window):
        w1 = min(count, w0 + window)
        idx = torch.arange(w0, w1, device=recv.device, dtype=torch.int64)
        want = sum(known_answer_input(torch, idx, r) for r in range(world))
        bad += int((out[w0:w1].to(torch.float64) != want.to(torch.float64)).sum())
    t = torch.tensor([bad], dtype=torch.int64)
    dist.all_reduce(t)
    return {"exact_known_answer": int(t.item()) == 0, "exact_violations": int(t.item()),
            "exact": "integer-valued inputs in [-16, 15]: every element of every rank == the sum of the N inputs"}


def _timed_max(torch, dist, fn, steps, warmup, comm=None):
    """Seconds for `steps` calls of fn after `warmup`, barrier + sync on both sides, max over ranks.
    With `comm`, the waits go through comm.synchronize() first (bounded by its timeout)."""
    def sync():
        if comm is not None:
            rc = comm.synchronize()
            if rc:
                raise RuntimeError(f"chr_comm_synchronize: {rc}")
        torch.cuda.synchronize()

    for _ in range(warmup):
        fn()
    sync()
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def compare_lines(args, ca, torch, dist, comm, send, recv, count, dt, k, b, world, dev, metric_sched=None,
                  deadline=None):
    """Context, not the metric: on the same buffers and ranks, (1) RCCL's own ncclAllReduce
    (torch.distributed nccl group), (2) the reference's MPICH ring baseline
    (testing/mpich_implementations/all_reduce/allreduce_ring.cpp) run on libchiara's executor and
    (3) the metric's own schedule with the reductions on the transfer stream (no overlap),
    (4) its arithmetic under the balanced, reference-route and exact (the reference's messages
    end to end) schedules, (5) the flat schedule at pipeline depths 1, 2 and 8, (6) with --phases, CHiArA's
    phases as stand-alone collectives and (7) the other multi-GPU BASELINE configs, C3 and C5
    (baseline_configs).  An entry that would start after the deadline is recorded as skipped."""
    late = (lambda: False) if deadline is None else deadline.passed
    steps, warm = max(1, min(args.steps, 20)), 2
    S = count * (4 if dt == ca.FLOAT32 else 2)
    out = {"steps": steps}

    def entry(el):
        algbw = S * steps / el / 1e9
        return {"algbw_GBps": round(algbw, 2), "busbw_GBps": round(algbw * 2 * (world - 1) / world, 2),
                "ms_per_call": round(el / steps * 1e3, 4)}

    try:
        if late():
            raise TimeoutError("deadline")
        g = dist.new_group(backend="nccl")
        x = torch.empty(count, dtype=torch.float32 if dt == ca.FLOAT32 else torch.bfloat16, device=dev)
        x.view(torch.uint8).copy_(send)
        out["rccl_allreduce"] = entry(_timed_max(torch, dist, lambda: dist.all_reduce(x, group=g), steps, warm))
        dist.destroy_process_group(g)
    except TimeoutError:
        out["rccl_allreduce"] = {"skipped": "deadline"}
    except Exception as e:  # context only: never fail the metric line for it
        out["rccl_allreduce"] = {"error": str(e)[:200]}

    def timed(name, fn):
        """One context entry on libchiara; a failure (e.g. a timeout that aborted the communicator)
        is recorded in the line instead of failing the metric, and skips the entries after it."""
        if late():  # first: a collective every rank reaches, whatever its communicator's state
            out[name] = {"skipped": "deadline"}
            return
        if out.get("aborted"):
            return
        try:
            out[name] = entry(_timed_max(torch, dist, fn, steps, warm, comm))
        except Exception as e:
            out[name] = {"error": str(e)[:200]}
            if comm.aborted:
                out["aborted"] = name

    def ring():
        ca.check(ca.MPICH_Allreduce_ring(send, recv, count, dt, ca.SUM, comm, async_op=True))
    timed("mpich_ring_on_libchiara", ring)

    # the same radix/batch arithmetic under the other schedules (same bits, other routes)
    restore = ca.SCHEDULE_FLAT if metric_sched is None else metric_sched

    def radix():
        ca.check(ca.all_reduce_radix_batch(send, recv, count, dt, ca.SUM, comm, k, b, async_op=True))
    comm.set_overlap(False)
    try:
        timed("radix_batch_no_overlap", radix)
    finally:
        comm.set_overlap(True)
    for name, sch in (("radix_batch_flat", ca.SCHEDULE_FLAT),
                      ("radix_batch_balanced", ca.SCHEDULE_BALANCED),
                      ("radix_batch_reference_route", ca.SCHEDULE_REFERENCE),
                      ("radix_batch_exact_reference_messages", ca.SCHEDULE_EXACT),
                      ("radix_batch_flat_rccl_allgather", ca.SCHEDULE_FLAT_AG),
                      ("radix_batch_flat_separate_groups", ca.SCHEDULE_FLAT_SEQ)):
        comm.set_schedule(sch)
        try:
            timed(name, radix)
        finally:
            comm.set_schedule(restore)
    # pipeline depth of the flat schedule (automatic: 4 slices at 1 GiB, 16 MiB pieces)
    comm.set_schedule(ca.SCHEDULE_FLAT)
    try:
        for P in (1, 2, 8):
            comm.set_slices(P)
            try:
                timed(f"radix_batch_flat_slices{P}", radix)
            finally:
                comm.set_slices(0)
    finally:
        comm.set_schedule(restore)
    # CHiArA's phases as stand-alone collectives (testing/custom_implementations/work_dir/reduce_scatter/), on
    # the same buffers, each reading the whole S-byte send buffer per rank: phase 1 (b = 2, k = 2), phase 2
    # (b = 2) and the reduce-scatter's k-nomial scatter (one group of all ranks, k = 2)
    if args.phases and world % 2 == 0:
        nn = world // 2
        niters = nn // 2 + (1 if nn % 2 else 0)
        rc_irs, rc_ilr, rc_isc = count // world, count // (niters * 2), count // world
        timed("phase_intra_reduce_scatter_k2_b2",
              lambda: ca.check(ca.intra_reduce_scatter_radix_batch(send, recv, rc_irs, dt, ca.SUM, comm, 2, 2)))
        timed("phase_inter_reduce_linear_b2",
              lambda: ca.check(ca.inter_reduce_linear(send, recv, rc_ilr, dt, ca.SUM, comm, 2)))
        timed(f"phase_intra_scatter_k2_b{world}",
              lambda: ca.check(ca.intra_scatter_radix_batch(send, rc_isc, dt, recv, comm, 2, world)))
    # whether any rank's communicator aborted, agreed over gloo: the entries below are collectives
    ab = torch.tensor([1.0 if out.get("aborted") else 0.0], dtype=torch.float64)
    dist.all_reduce(ab, op=dist.ReduceOp.MAX)
    if ab.item():
        out.setdefault("aborted", "on another rank")
        return out
    out["small_messages"] = ({"skipped": "deadline"} if late() else
                             small_messages(ca, torch, dist, comm, dt, k, b, world, dev, restore))
    out.update(baseline_configs(args, ca, torch, dist, comm, world, dev, steps, warm, late, restore))
    return out


def small_messages(ca, torch, dist, comm, dt, k, b, world, dev, current):
    """Latency of blocking calls (the reference harness's pattern) at small buffers: us per call, max
    over ranks, with the communicator's schedule (the metric's AUTO, whose choice is reported) issued
    eagerly and replayed from captured HIP graphs (chr_comm_set_graphs), and eagerly under FLAT
    (gather + allgather: two exchange steps) and FLAT_1SHOT (one step, every rank reduces the whole
    buffer)."""
    es = 4 if dt == ca.FLOAT32 else 2
    names = {0: "reference", 1: "balanced", 2: "flat", 3: "exact", 4: "flat_ag", 5: "flat_seq", 7: "flat_1shot"}
    res = {}
    try:
        for nbytes in (4 << 10, 256 << 10, 4 << 20):
            count = nbytes // es - (nbytes // es) % world
            s = torch.empty(count * es, dtype=torch.uint8, device=dev)
            r = torch.empty(count * es, dtype=torch.uint8, device=dev)
            ca.check(ca.fill(s, count, dt, 0, SEED, int(os.environ["RANK"]), stream=comm.stream))
            row = {}
            for name, g, sch in (("eager_us", False, current), ("graph_us", True, current),
                                 ("flat_eager_us", False, ca.SCHEDULE_FLAT),
                                 ("flat_1shot_eager_us", False, ca.SCHEDULE_FLAT_1SHOT)):
                comm.set_graphs(g)
                comm.set_schedule(sch)
                try:
                    el = _timed_max(torch, dist, lambda: ca.check(ca.all_reduce_radix_batch(s, r, count, dt, ca.SUM, comm,
                                                                                             k, b)), 50, 3)
                finally:
                    comm.set_graphs(False)
                    comm.set_schedule(current)
                row[name] = round(el / 50 * 1e6, 1)
            tuned = comm.tuned_schedule(ca.MODE_ALLREDUCE, count, dt, k, b) if current == ca.SCHEDULE_AUTO else None
            if tuned is not None:
                row["auto_choice"] = f"{names.get(tuned[0], tuned[0])}, {tuned[1]} slices"
            res[f"{nbytes >> 10}KiB"] = row
    except Exception as e:  # context only
        res["error"] = str(e)[:200]
    return res


def baseline_configs(args, ca, torch, dist, comm, world, dev, steps, warm, late=lambda: False, restore=None):
    """The other multi-GPU BASELINE configs at this world size, default schedule, same run:
    C3 (fp32 reduce-scatter, radix 2, 256 MiB send buffer; b = 1 and 2; next to it the four MPICH
    reduce-scatter baselines on the same buffers) and C5 (bf16 allreduce, b = 4 ("4x2": 4 ranks per
    group x 2 groups), k = 4, 1 GiB, compute/xGMI overlap) at 8 ranks."""
    out = {}
    try:
        rs_send = (256 << 20) // 4  # elements in the send buffer
        rc = rs_send // world
        s_rs = torch.empty(rc * world * 4, dtype=torch.uint8, device=dev)
        r_rs = torch.empty(rc * 4, dtype=torch.uint8, device=dev)
        ca.check(ca.fill(s_rs, rc * world, ca.FLOAT32, 0, SEED, int(os.environ["RANK"]), stream=comm.stream))
        for b in sorted({1, 2} & {d for d in range(1, world + 1) if world % d == 0}):
            if late():
                out[f"c3_reduce_scatter_fp32_k2_b{b}_256MiB"] = {"skipped": "deadline"}
                continue

            def rs():
                ca.check(ca.reduce_scatter_radix_batch(s_rs, r_rs, rc, ca.FLOAT32, ca.SUM, comm, 2, b, async_op=True))
            el = _timed_max(torch, dist, rs, steps, warm, comm)
            algbw = rc * world * 4 * steps / el / 1e9  # nccl-tests: send-buffer bytes / time
            out[f"c3_reduce_scatter_fp32_k2_b{b}_256MiB"] = {
                "algbw_GBps": round(algbw, 2), "busbw_GBps": round(algbw * (world - 1) / world, 2),
                "ms_per_call": round(el / steps * 1e3, 4)}
        # the MPICH reduce-scatters testing/mpich_implementations/reduce_scatter/main.cpp times
        # against, on the same buffers and executor (radix at k = 2)
        for name, fn in (("radix_k2", lambda: ca.MPICH_reduce_scatter_radix(s_rs, r_rs, rc, ca.FLOAT32, ca.SUM, comm, 2,
                                                                             async_op=True)),
                         ("rec_halving", lambda: ca.MPICH_reduce_scatter_rec_halving(s_rs, r_rs, rc, ca.FLOAT32, ca.SUM,
                                                                                     comm, async_op=True)),
                         ("rec_doubling", lambda: ca.MPICH_reduce_scatter_rec_doubling(s_rs, r_rs, rc, ca.FLOAT32,
                                                                                       ca.SUM, comm, async_op=True)),
                         ("pairwise", lambda: ca.MPICH_reduce_scatter_pairwise(s_rs, r_rs, rc, ca.FLOAT32, ca.SUM, comm,
                                                                               async_op=True))):
            if late():
                out[f"c3_mpich_reduce_scatter_{name}_256MiB"] = {"skipped": "deadline"}
                continue
            el = _timed_max(torch, dist, lambda: ca.check(fn()), steps, warm, comm)
            algbw = rc * world * 4 * steps / el / 1e9
            out[f"c3_mpich_reduce_scatter_{name}_256MiB"] = {
                "algbw_GBps": round(algbw, 2), "busbw_GBps": round(algbw * (world - 1) / world, 2),
                "ms_per_call": round(el / steps * 1e3, 4)}
        del s_rs, r_rs
        if world == 8 and late():
            out["c5_allreduce_bf16_k4_b4_1GiB"] = {"skipped": "deadline"}
        elif world == 8:
            cnt = (1 << 30) // 2
            s5 = torch.empty(cnt * 2, dtype=torch.uint8, device=dev)
            r5 = torch.empty(cnt * 2, dtype=torch.uint8, device=dev)
            ca.check(ca.fill(s5, cnt, ca.BFLOAT16, 0, SEED, int(os.environ["RANK"]), stream=comm.stream))

            def c5():
                ca.check(ca.all_reduce_radix_batch(s5, r5, cnt, ca.BFLOAT16, ca.SUM, comm, 4, 4, async_op=True))
            el = _timed_max(torch, dist, c5, steps, warm, comm)
            algbw = cnt * 2 * steps / el / 1e9
            row = out["c5_allreduce_bf16_k4_b4_1GiB"] = {
                "algbw_GBps": round(algbw, 2), "busbw_GBps": round(algbw * 2 * (world - 1) / world, 2),
                "ms_per_call": round(el / steps * 1e3, 4)}
            row.update(c5_overlap_record(ca, comm, cnt, world))
            # C5's own output, as the metric's (bf16 tolerance: DESIGN §7)
            try:
                def fill5(r, buf):
                    ca.check(ca.fill(buf, cnt, ca.BFLOAT16, 0, SEED, r, stream=comm.stream))
                    torch.cuda.synchronize()
                ca.check(comm.synchronize())
                row["result_check"] = result_check(torch, dist, r5, cnt, 2, world, fill5)
                row["result_check"].update(exact_check(
                    torch, dist, s5, r5, cnt, 2, int(os.environ["RANK"]),
                    lambda: ca.check(ca.all_reduce_radix_batch(s5, r5, cnt, ca.BFLOAT16, ca.SUM, comm, 4, 4)), world))
                fill5(int(os.environ["RANK"]), s5)
            except Exception as e:
                row["result_check"] = {"error": str(e)[:200]}
            torch.cuda.empty_cache()
            # C5 names compute/xGMI overlap: with one slice a call has nothing to overlap inside it, so
            # the best depth >= 2 is timed too and both are recorded
            if row.get("slices", 0) < 2 and not late():
                best = None
                sched_now = row.get("schedule_code", ca.SCHEDULE_FLAT)
                try:
                    for P in (2, 4, 8):
                        comm.set_schedule(ca.SCHEDULE_FLAT if sched_now in (None, ca.SCHEDULE_AUTO) else sched_now)
                        comm.set_slices(P)
                        elp = _timed_max(torch, dist, c5, steps, warm, comm)
                        if best is None or elp < best[1]:
                            best = (P, elp)
                finally:
                    comm.set_slices(0)
                    comm.set_schedule(ca.SCHEDULE_FLAT if restore is None else restore)
                ab = cnt * 2 * steps / best[1] / 1e9
                row["overlapped_best_depth_ge2"] = {
                    "slices": best[0], "overlap": True, "algbw_GBps": round(ab, 2),
                    "busbw_GBps": round(ab * 2 * (world - 1) / world, 2), "ms_per_call": round(best[1] / steps * 1e3, 4)}
            del s5, r5
    except Exception as e:  # context only: never fail the metric line for it
        out["baseline_configs_error"] = str(e)[:200]
    torch.cuda.empty_cache()
    return out


SCHED_NAMES = {0: "reference", 1: "balanced", 2: "flat", 3: "exact", 4: "flat_ag", 5: "flat_seq", 6: "auto",
               7: "flat_1shot"}


def c5_overlap_record(ca, comm, count, world):
    """What the C5 entry ran: the schedule and depth (AUTO's choice for these arguments when the
    communicator runs AUTO) and whether its reductions overlapped the transfers: overlap on (the
    communicator's compute stream) and >= 2 slices, so slice s is reduced while slice s+1 moves."""
    tuned = comm.tuned_schedule(ca.MODE_ALLREDUCE, count, ca.BFLOAT16, 4, 4)
    overlap_on = comm.overlap
    if tuned is None:
        return {"schedule": "unknown", "schedule_code": None, "slices": None, "overlap": None}
    sched, slices = tuned
    return {"schedule": SCHED_NAMES.get(sched, str(sched)), "schedule_code": sched, "slices": slices,
            "overlap": bool(overlap_on and slices >= 2)}


class _StdoutToStderr:
    """Route file descriptor 1 to stderr while libraries run (RCCL prints its init banner to
    stdout); emit() writes the one JSON line to the real stdout."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def emit(self, text):
        sys.stdout.flush()
        os.write(self.saved, (text + "\n").encode())

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)
        return False


OUT = None  # set in main(): where the JSON line goes


def emit(line):
    text = json.dumps(line)
    if OUT is not None:
        OUT.emit(text)
    else:
        print(text, flush=True)


def main():
    global OUT
    with _StdoutToStderr() as OUT:
        rc = _main()
    return rc or 0


def _main():
    argv = sys.argv[1:]
    args = parse(argv)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # start the N rank processes before any GPU work here.  torch.cuda.device_count() calls
        # hipGetDeviceCount, which loads the HIP runtime and enumerates devices in this parent; it creates no
        # context or queue, and this parent never execs (the ranks are a child process group), which is
        # what the pool forbids after GPU initialisation
        import torch

        try:
            cmd = plan_launch(args, argv, os.environ, torch.cuda.device_count(), free_port())
        except ValueError as e:
            print(f"bench.py: {e}", file=sys.stderr)
            return 2
        return run_launcher(cmd)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        bench_allreduce(args)
        return
    if args.e2e:
        bench_e2e(args)
        return
    if args.collective_kernels:
        bench_collective_kernels(args)
        return
    if args.collective_kernels_small:
        bench_collective_kernels_small(args)
        return
    if args.rank_trees:
        bench_rank_trees(args)
        return
    cpu = cpu_baseline(args.cpu_seconds) if args.full and not args.no_cpu_baseline else None
    bench_bucket(args, cpu)


if __name__ == "__main__":
    sys.exit(main())
