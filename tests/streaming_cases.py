"""The case lists and runners of tests/test_gpu_streaming_sweep.py: every streaming instantiation of the bucket and
tree kernels (csrc/reduce_vec.hpp, csrc/reduce_tree.hpp) against the oracle, bit for bit.

The tuning variables are read once per process, so the streaming sweeps run in child processes: this file is the
child's program (`python streaming_cases.py JOB`, the environment set by the parent) and the one source of the case
lists, which tests/test_tree_static_programs.py pins on the CPU (census, order visibility, the static-program table).

Operands: n = NVEC * E + 1 elements with E = 16 / element size and NVEC = 2*8*4096/16 + 3*256 + 3 = 4867 vectors.
With 4 KiB XCD runs (CHR_XCD_RUN_KIB=4) and one-wave workgroups that is, for U = 4 / 2 / 1 vectors per lane per trip,
two whole 8-XCD groups on the run map (16 / 32 / 64 trips of 4 / 2 / 1 KiB), 3 / 6 / 12 whole trips past the last
group on the identity map, one partial trip of 3 vectors and a scalar tail of one element.
  layout (a): every operand 16-byte aligned;
  layout (b): every operand and the output one element into its buffer (still 16-byte congruent), the same n: a
              scalar head of E - 1 elements, the vector body, and a scalar tail of 2 elements (none for the 8-byte
              types, whose head of one element leaves a whole number of vectors).
The odd-XCD handover stays off at these sizes (a share of 2-8 trips >> 6 is 0): tests/test_gpu_xcd_map.py sets it."""
import collections
import functools
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG_DIR = os.path.join(REPO, "configurable-hierarchical-allreduce-algorithms_amd")
for _p in (HERE, os.path.join(REPO, "oracle"), PKG_DIR):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import chiara_amd as ca  # noqa: E402
import pyoracle as po  # noqa: E402
from test_gpu_dispatch_sweep import CPLX, FLOATS, PAIRS, pattern_for, valid  # noqa: E402
from test_gpu_kernels import DT, OP, _bits, _bytes_copy  # noqa: E402
from tree_util import all_programs, random_program, tree_ref  # noqa: E402

NVEC = 2 * 8 * 4096 // 16 + 3 * 256 + 3
NOPS = 9  # acc / leaf 0 and 8 more: the widest fan-in and the widest tree
SWEEP_DTYPES = [d for d in DT if d not in PAIRS + CPLX]
SWEEP_PAIRS = [(d, o) for d in SWEEP_DTYPES for o in OP if valid(d, o)]
FAN_INS = range(1, 9)
LEAF_COUNTS = range(2, 9)
ARITH = ("sum", "prod", "max", "min")

# csrc/reduce_tree.hpp StaticProgs<NL>: the programs k_reduce_tree unrolls at compile time (tree_eval_static); every
# other program, and these with a swapped combine of an order-sensitive op, take the interpreter (tree_eval).
# tests/test_tree_static_programs.py holds this table against the header.
STATIC_PROGS = {
    2: [[0, 1]],
    4: [[0, 1, 0, 2], [0, 1, 1, 1]],
    8: [[0, 1, 1, 1, 0, 1, 1, 2], [0, 1, 0, 2, 0, 2, 0, 2], [0, 1, 0, 2, 0, 1, 0, 3], [0, 1, 1, 0, 1, 2, 0, 2],
        [0, 1, 1, 1, 0, 2, 1, 1], [0, 1, 1, 1, 1, 1, 1, 1]],
}


def order_sensitive(dtype, op):
    """reduce_tree.hpp order_sensitive<DT, OP>() for the non-pair, non-complex types."""
    return dtype in FLOATS and op in ARITH


def count(dtype):
    return NVEC * (16 // np.dtype(po.NP_DTYPES[dtype]).itemsize) + 1


# ---- the case lists ---------------------------------------------------------------------------------------

BucketCase = collections.namedtuple("BucketCase", "dtype op m layout running_first pattern")
TreeCase = collections.namedtuple("TreeCase", "dtype op nl comb swaps pattern layout alias what")


def bucket_cases():
    """Every bucket call of the sweep.  Layout (a) runs in place (out == acc, the case ACC0 exists for), layout (b)
    out of place."""
    out = []
    for dtype, op in SWEEP_PAIRS:
        for m in FAN_INS:
            for layout in "ab":
                out.append(BucketCase(dtype, op, m, layout, False, pattern_for(op)))
    for dtype in FLOATS:  # the running-first codes kSumSw, kProdSw, kMaxSw, kMinSw, on TIES so that the order shows
        for op in ARITH:
            for m in FAN_INS:
                for layout in "ab":
                    out.append(BucketCase(dtype, op, m, layout, True, po.PAT_TIES))
                    if pattern_for(op) != po.PAT_TIES:  # and the default order of SUM / PROD where NaNs meet
                        out.append(BucketCase(dtype, op, m, layout, False, po.PAT_TIES))
    for dtype in PAIRS + CPLX:  # compiled in the plain shape only: CHR_REDUCE_NT=1 must leave them correct
        for op in OP:
            if valid(dtype, op):
                out.append(BucketCase(dtype, op, 3, "a", False, pattern_for(op)))
    return out


def _nonzero_swaps(rng, nl):
    while True:
        s = [int(v) for v in rng.integers(0, 2, nl - 1)]
        if any(s):
            return s


def tree_cases(dtype, op):
    """Every tree call of the sweep for one (dtype, op); the same list runs in configurations A and B.  Swap words
    and the non-static programs are drawn from a generator seeded by (dtype, op).  The operand order of a floating
    SUM / PROD shows only where two NaNs meet (whose payload survives), so on those pairs every case runs on TIES data
    as well as on pattern_for(op): the unswapped ones too, or the unrolled body could combine in either order."""
    rng = np.random.default_rng(zlib.crc32(f"streaming-{dtype}-{op}".encode()))
    pat = pattern_for(op)
    out = []

    def add(nl, comb, swaps, layout, alias, what):
        out.append(TreeCase(dtype, op, nl, comb, swaps, pat, layout, alias, what))
        if order_sensitive(dtype, op) and pat != po.PAT_TIES:
            out.append(TreeCase(dtype, op, nl, comb, swaps, po.PAT_TIES, layout, alias, what + " ties"))

    for nl in LEAF_COUNTS:
        static = STATIC_PROGS.get(nl, [])
        for comb in static:
            add(nl, comb, [0] * (nl - 1), "a", None, "static")  # the unrolled body
            # order-sensitive ops: the interpreter; commutative ops: the unrolled body, which ignores the swaps
            add(nl, comb, _nonzero_swaps(rng, nl), "a", None, "static swapped")
        if nl > 2:  # the only 2-leaf program is the static one
            while True:
                comb, _ = random_program(rng, nl)
                if comb not in static:
                    break
            add(nl, comb, _nonzero_swaps(rng, nl), "a", None, "non-static")
        if static:
            add(nl, static[0], [0] * (nl - 1), "b", None, "static shifted")
            add(nl, static[0], [0] * (nl - 1), "a", 0, "static out = leaf 0")
            add(nl, static[0], [0] * (nl - 1), "a", nl - 1, "static out = last leaf")
        if nl == 2:  # configuration B: the bucket route, and out == in kept on the tree kernel
            for sw in (0, 1):
                for alias in (None, 0, 1):
                    add(2, [0, 1], [sw], "a", alias, "two leaves")
    return out


PROGRAM_VARIANTS = {  # name: (dtype, op, pattern, random swaps)
    "f32 max ties swapped": ("f32", "max", po.PAT_TIES, True),
    "f32 max ties": ("f32", "max", po.PAT_TIES, False),
    "bf16 sum": ("bf16", "sum", po.PAT_UNIFORM, False),
    "i32 sum swapped": ("i32", "sum", po.PAT_UNIFORM, True),
}


def program_cases(variant):
    """Every valid program of 2..8 leaves with stack depth <= 4 (377), on layout (a)."""
    dtype, op, pat, swapped = PROGRAM_VARIANTS[variant]
    rng = np.random.default_rng(zlib.crc32(f"every-program-{variant}".encode()))
    out = []
    for nl in LEAF_COUNTS:
        for comb in all_programs(nl):
            swaps = [int(v) for v in rng.integers(0, 2, nl - 1)] if swapped else [0] * (nl - 1)
            out.append(TreeCase(dtype, op, nl, comb, swaps, pat, "a", None, f"every program ({variant})"))
    return out


BATCH_DTYPE, BATCH_OP, BATCH_PATTERN = "f32", "max", po.PAT_TIES
BATCH_NVEC = (64 + 6, 2 * 64, 3 * 64 - 1)  # a streaming 8-leaf trip is 64 vectors: one to three trips, ragged


def batch_programs():
    """9 trees of 8 leaves (two launches: 8 segments and 1): static programs on the unrolled body, static programs
    with swapped combines and non-static ones on the interpreter, side by side in one grid."""
    rng = np.random.default_rng(20260)
    st = STATIC_PROGS[8]
    progs = []
    for t in range(9):
        if t % 3 == 2:
            while True:
                comb, _ = random_program(rng, 8)
                if comb not in st:
                    break
            progs.append((comb, _nonzero_swaps(rng, 8) if t == 8 else [0] * 7))
        else:
            comb = st[(t - t // 3) % 6]
            progs.append((comb, _nonzero_swaps(rng, 8) if t in (1, 4) else [0] * 7))
    return progs


# ---- references (host only) ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def host_operands(dtype, pattern):
    """The NOPS operands of (dtype, pattern), n = count(dtype) elements each: shared, never written."""
    xs = [po.fill(count(dtype), dtype, pattern, 29, r) for r in range(NOPS)]
    for x in xs:
        x.flags.writeable = False
    return xs


def operands_for(dtype, op, pattern):
    """int32 PROD on small factors: the oracle's C int product must not overflow (as test_gpu_kernels._check_multi)."""
    xs = host_operands(dtype, pattern)
    return _i32_small(pattern) if (dtype, op) == ("i32", "prod") else xs


@functools.lru_cache(maxsize=None)
def _i32_small(pattern):
    xs = [(x % 7).astype(np.int32) for x in host_operands("i32", pattern)]
    for x in xs:
        x.flags.writeable = False
    return xs


@functools.lru_cache(maxsize=None)
def bucket_ref(dtype, op, m, running_first, pattern):
    xs = operands_for(dtype, op, pattern)
    acc, ins = xs[0], xs[1:1 + m]
    if not running_first:
        return po.reduce_multi(_bytes_copy(acc), [_bytes_copy(x) for x in ins], dtype, op)
    run = _bytes_copy(acc)  # test_gpu_kernels.test_reduce_multi_running_first's chain
    for x in ins:
        nxt = _bytes_copy(x)
        po.reduce_local(run, nxt, dtype, op)
        run = nxt
    return run


_TREE_REFS = {}


def tree_case_ref(c, n=None):
    key = (c.dtype, c.op, c.pattern, tuple(c.comb), tuple(c.swaps), n)
    if key not in _TREE_REFS:
        leaves = [x[:n] for x in operands_for(c.dtype, c.op, c.pattern)[:c.nl]]
        _TREE_REFS[key] = tree_ref(leaves, c.comb, c.swaps, c.dtype, c.op)
    return _TREE_REFS[key]


def first_diff(got, ref):
    """Index of the first element whose bits differ, or None."""
    g, r = _bits(got), _bits(ref)
    if g.shape == r.shape and np.array_equal(g, r):
        return None
    if g.shape != r.shape:
        return -1
    per = g.size // max(1, got.size)  # structured elements compare as bytes
    return int(np.flatnonzero(g != r)[0]) // max(1, per)


# ---- the device side ------------------------------------------------------------------------------------------

class Device:
    """Device copies of the operand sets, each (dtype, op-set, pattern, layout) uploaded once and never written; an
    output and a work buffer per (dtype, layout).  Every buffer holds n + 1 elements: layout (b) starts one in."""

    def __init__(self, gu):
        self.gu = gu
        self._ops, self._bufs = {}, {}

    @staticmethod
    def _off(dtype, layout):
        return np.dtype(po.NP_DTYPES[dtype]).itemsize if layout == "b" else 0

    def operands(self, dtype, op, pattern, layout):
        """[(tensor, address of element 0)] per operand."""
        small = (dtype, op) == ("i32", "prod")
        key = (dtype, small, pattern, layout)
        if key not in self._ops:
            off, row = self._off(dtype, layout), []
            for x in operands_for(dtype, op, pattern):
                t = self.gu.empty_dev(x.nbytes + x.itemsize)
                t[off:off + x.nbytes] = self.gu.to_dev(x)
                row.append((t, t.data_ptr() + off))
            self._ops[key] = row
        return self._ops[key]

    def buffer(self, dtype, layout, name):
        key = (dtype, layout, name)
        if key not in self._bufs:
            es = np.dtype(po.NP_DTYPES[dtype]).itemsize
            t = self.gu.empty_dev((count(dtype) + 1) * es)
            self._bufs[key] = (t, t.data_ptr() + self._off(dtype, layout))
        return self._bufs[key]

    def read(self, t, dtype, layout, n=None):
        n = count(dtype) if n is None else n
        off = 1 if layout == "b" else 0
        return self.gu.from_dev(t, po.NP_DTYPES[dtype])[off:off + n]


def run_bucket_case(dev, c):
    """None if the device result equals the oracle's, else (first differing index | "rc N")."""
    gu, n = dev.gu, count(c.dtype)
    d = dev.operands(c.dtype, c.op, c.pattern, c.layout)
    ins = [p for _, p in d[1:1 + c.m]]
    if c.layout == "a":  # in place, on a copy of the shared accumulator
        t_out, p_out = dev.buffer(c.dtype, "a", "work")
        t_out.copy_(d[0][0])
        p_acc = p_out
    else:
        t_out, p_out = dev.buffer(c.dtype, "b", "out")
        t_out.fill_(0xA5)
        p_acc = d[0][1]
    if c.running_first:
        rc = ca.reduce_multi_ex(p_out, p_acc, ins, n, DT[c.dtype], OP[c.op], ca.REDUCE_RUNNING_FIRST, gu.stream())
    else:
        rc = ca.reduce_multi(p_out, p_acc, ins, n, DT[c.dtype], OP[c.op], gu.stream())
    if rc:
        return f"rc {rc}"
    return first_diff(dev.read(t_out, c.dtype, c.layout), bucket_ref(c.dtype, c.op, c.m, c.running_first, c.pattern))


def run_tree_case(dev, c):
    gu, n = dev.gu, count(c.dtype)
    d = dev.operands(c.dtype, c.op, c.pattern, c.layout)
    leaves = [p for _, p in d[:c.nl]]
    if c.alias is None:
        t_out, p_out = dev.buffer(c.dtype, c.layout, "out")
        t_out.fill_(0xA5)
    else:  # the root over one of its own leaves: a copy of that leaf
        t_out, p_out = dev.buffer(c.dtype, c.layout, "work")
        t_out.copy_(d[c.alias][0])
        leaves[c.alias] = p_out
    rc = ca.reduce_tree(p_out, leaves, c.comb, c.swaps, n, DT[c.dtype], OP[c.op], gu.stream())
    if rc:
        return f"rc {rc}"
    return first_diff(dev.read(t_out, c.dtype, c.layout), tree_case_ref(c))


def run_batch(dev, bad):
    """reduce_tree_batch of batch_programs() at each ragged length; tree t's leaves are the shared operands rotated
    by t.  Returns the number of trees compared."""
    gu, dtype, op = dev.gu, BATCH_DTYPE, BATCH_OP
    d = dev.operands(dtype, op, BATCH_PATTERN, "a")
    hosts = operands_for(dtype, op, BATCH_PATTERN)
    progs = batch_programs()
    outs = [dev.buffer(dtype, "a", f"batch {t}") for t in range(len(progs))]
    ran = 0
    for nvec in BATCH_NVEC:
        n = nvec * 4 + 1
        for t_out, _ in outs:
            t_out.fill_(0xA5)
        rows = [[d[(t + j) % NOPS][1] for j in range(8)] for t in range(len(progs))]
        rc = ca.reduce_tree_batch([p for _, p in outs], rows, [p[0] for p in progs], [p[1] for p in progs], n,
                                  DT[dtype], OP[op], gu.stream())
        if rc:
            bad.append([dtype, op, "batch", f"n = {n}", f"rc {rc}"])
            continue
        for t, (comb, swaps) in enumerate(progs):
            ref = tree_ref([hosts[(t + j) % NOPS][:n] for j in range(8)], comb, swaps, dtype, op)
            diff = first_diff(dev.read(outs[t][0], dtype, "a", n), ref)
            if diff is not None:
                bad.append([dtype, op, f"batch tree {t} {comb} {swaps}", f"n = {n}", diff])
            ran += 1
    return ran


def run_tree_cases(dev, cases, bad):
    for c in cases:
        diff = run_tree_case(dev, c)
        if diff is not None:
            alias = "" if c.alias is None else f" out = leaf {c.alias}"
            case = f"{c.what}: {c.comb} swaps {c.swaps} pattern {c.pattern}"
            bad.append([c.dtype, c.op, case, c.layout + alias, diff])


# ---- the child ------------------------------------------------------------------------------------------------

def job_bucket(dev, bad, ran):
    for c in bucket_cases():
        diff = run_bucket_case(dev, c)
        if diff is not None:
            bad.append([c.dtype, c.op, f"m = {c.m}" + (" running first" if c.running_first else ""), c.layout, diff])
        ran[c.dtype] = ran.get(c.dtype, 0) + 1


def job_tree(dev, bad, ran):
    for dtype, op in SWEEP_PAIRS:
        cases = tree_cases(dtype, op)
        run_tree_cases(dev, cases, bad)
        ran[dtype] = ran.get(dtype, 0) + len(cases)


def job_programs(dev, bad, ran):
    for variant in PROGRAM_VARIANTS:
        cases = program_cases(variant)
        run_tree_cases(dev, cases, bad)
        ran[variant] = len(cases)
    ran["batch"] = run_batch(dev, bad)


# A: every vector launch takes the streaming instantiation; 2-leaf trees stay on the NL = 2 streaming tree kernel.
# B: streaming by size, at every size, which also routes 2-leaf trees to the bucket kernel as one fold
#    (launch_reduce_tree_multi) unless out is the fold's input.
_UNSET = dict.fromkeys(("CHR_REDUCE_NT", "CHR_REDUCE_NT_MIN_BYTES", "CHR_XCD_RUN_KIB", "CHR_XCD_HAND_SHIFT",
                        "CHR_REDUCE_MAX_LAUNCH_VEC", "CHR_WG_PER_CU_VEC", "CHR_WG_PER_CU_TREE"))
CONFIG_A = dict(_UNSET, CHR_REDUCE_NT="1", CHR_XCD_RUN_KIB="4")
CONFIG_B = dict(_UNSET, CHR_REDUCE_NT_MIN_BYTES="1", CHR_XCD_RUN_KIB="4")
JOBS = {  # name: (runner, environment; None = unset)
    "bucket A": (job_bucket, CONFIG_A),
    "tree A": (job_tree, CONFIG_A),
    "tree B": (job_tree, CONFIG_B),
    "programs A": (job_programs, CONFIG_A),
}


def child_env(job):
    env = dict(os.environ)
    for k, v in JOBS[job][1].items():
        env.pop(k, None)
        if v is not None:
            env[k] = v
    return env


def main(job):
    import json
    import time

    import gpu_util

    t0 = time.perf_counter()
    for k, v in JOBS[job][1].items():  # the configuration is the parent's to set: refuse to run without it
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    bad, ran = [], {}
    JOBS[job][0](Device(gpu_util), bad, ran)
    gpu_util.sync()
    print(json.dumps({"job": job, "bad": bad, "ran": ran, "seconds": round(time.perf_counter() - t0, 2)}))


if __name__ == "__main__":
    main(sys.argv[1])
