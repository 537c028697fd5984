"""What a PyTorch user does with a stream-ordered library: capture its calls into a graph of their own.

After a warm-up call, torch.cuda.graph captures on one non-blocking stream a LINEAR sequence of built-in-op calls --
chr_fill, the head / body / tail fold with m = 17 (three chained groups), the 8-leaf tree, the batch of 9 trees (two
launches) -- and replays it twice with the inputs changed in between.  Each replay equals the reference, bit for bit.
A launch on the NULL stream during capture is an error code from the call, so this is a second, independent detector
of a launcher that drops its stream.  No user ops (chiara.h: never captured), no parallel branches, nothing that
configures the runtime."""
import numpy as np
import pytest

import chiara_amd as ca
import pyoracle as po
from streaming_cases import batch_programs
from tree_util import tree_ref

pytestmark = pytest.mark.gpu

N_BUCKET = 4 * (2 * 1024 + 300) + 8
N_TREE = 8 * (3 * 256 + 70) + 5
C4 = [0, 1, 1, 1, 0, 1, 1, 2]
C4_SWAPS = [1, 0, 1, 0, 1, 0, 1]
FILL_SEED, FILL_RANK = 0xC41A5EED, 3
OFF = 4  # bytes into a 16-byte aligned allocation: a scalar head, the vector body, a scalar tail


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_a_callers_graph_of_library_calls_replays():
    import torch

    import gpu_util as gu
    import stream_util as su

    S = su.nonblocking_stream()
    progs = batch_programs()

    def buf(n):
        t = gu.empty_dev(4 * n + 32)
        assert t.data_ptr() % 16 == 0
        return t[OFF:OFF + 4 * n]

    acc, out = buf(N_BUCKET), buf(N_BUCKET)
    ins = [buf(N_BUCKET) for _ in range(17)]
    leaves = [buf(N_TREE) for _ in range(9)]
    root = buf(N_TREE)
    roots = [buf(N_TREE) for _ in progs]
    rows = [[leaves[(t + j) % 9] for j in range(8)] for t in range(len(progs))]

    def sequence(stream):
        rcs = [ca.fill(acc, N_BUCKET, ca.FLOAT32, 0, FILL_SEED, FILL_RANK, stream=stream),
               ca.reduce_multi(out, acc, ins, N_BUCKET, ca.FLOAT32, ca.SUM, stream),
               ca.reduce_tree(root, leaves[:8], C4, C4_SWAPS, N_TREE, ca.FLOAT32, ca.SUM, stream),
               ca.reduce_tree_batch(roots, rows, [p[0] for p in progs], [p[1] for p in progs], N_TREE, ca.FLOAT32,
                                    ca.SUM, stream)]
        assert rcs == [0, 0, 0, 0], f"status codes of the four calls: {rcs}"

    def load(seed):
        h_ins = [po.fill(N_BUCKET, "f32", 0, seed, r) for r in range(17)]
        h_leaves = [po.fill(N_TREE, "f32", 0, seed + 1, r) for r in range(9)]
        for t, x in zip(ins + leaves, h_ins + h_leaves):
            t.copy_(gu.to_dev(x))
        for t in [acc, out, root] + roots:
            t.fill_(0xA5)
        torch.cuda.synchronize(gu.DEV)
        return h_ins, h_leaves

    def check(h_ins, h_leaves, what):
        filled = po.fill(N_BUCKET, "f32", 0, FILL_SEED, FILL_RANK)
        assert np.array_equal(_bits(gu.from_dev(acc, np.float32)), _bits(filled)), f"{what}: chr_fill"
        assert np.array_equal(_bits(gu.from_dev(out, np.float32)),
                              _bits(po.reduce_multi(filled.copy(), h_ins, "f32", "sum"))), f"{what}: the fold"
        assert np.array_equal(_bits(gu.from_dev(root, np.float32)),
                              _bits(tree_ref(h_leaves[:8], C4, C4_SWAPS, "f32", "sum"))), f"{what}: the tree"
        for t, (comb, swaps) in enumerate(progs):
            want = tree_ref([h_leaves[(t + j) % 9] for j in range(8)], comb, swaps, "f32", "sum")
            assert np.array_equal(_bits(gu.from_dev(roots[t], np.float32)), _bits(want)), f"{what}: batch tree {t}"

    host = load(101)
    sequence(0)  # the warm-up: module load and lazy initialisation outside the capture
    torch.cuda.synchronize(gu.DEV)
    check(*host, "warm-up")
    host = load(101)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=S):
        sequence(S.cuda_stream)
    for replay, seed in enumerate((211, 307)):
        host = load(seed)
        with torch.cuda.stream(S):
            graph.replay()
        S.synchronize()
        check(*host, f"replay {replay}")
