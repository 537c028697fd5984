"""Library calls in flight together: four non-blocking streams fed round-robin from one host thread, and four host
threads with a stream each.  What two calls share -- the op / type registry, reduce_tuning(), the fold-by-fold
trees' stream-ordered scratch, the lazy binary16 registry -- must not show in any result: every chain equals its host
reference chain (pyoracle, tree_util.tree_ref, struct_ref, f16_ref; bit for bit) and every input its snapshot."""
import ctypes
import os
import threading
import time

import numpy as np
import pytest

import chiara_amd as ca
import pyoracle as po
from tree_util import tree_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OPN = "user_halfadd"
C4 = [0, 1, 1, 1, 0, 1, 1, 2]
C4_SWAPS = [1, 0, 1, 0, 1, 0, 1]
ROUNDS = 8
OPERAND_BYTES = 2 << 20


@pytest.fixture(scope="module")
def su():
    import stream_util

    return stream_util


@pytest.fixture(scope="module")
def gu():
    import gpu_util

    return gpu_util


@pytest.fixture(scope="module")
def gate(su):
    return su.shared_gate()


def _lib(name, hint):
    path = os.path.join(HERE, "userop", name)
    assert os.path.exists(path), f"{path} missing: make -C tests/userop {hint} (__graft_entry__.build())"
    return ctypes.CDLL(path)


def _addr(fn):
    return ctypes.cast(fn, ctypes.c_void_p).value


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _read(gu, t, npdt, n):
    return gu.from_dev(t, npdt, n).copy()


# ---- four streams, one host thread ----------------------------------------------------------------------------------------

def test_four_streams_released_together(su, gu, gate):
    """Four non-blocking streams wait for one event recorded behind one gate; 8 rounds per stream are enqueued
    round-robin before it opens, so consecutive library calls always come from different streams and everything
    queued runs together:
      0  f32 SUM in place, m = 3 (the running value goes round to round)
      1  bf16 SUM 8-leaf tree into a fresh root each round, the root being leaf 0 of the next round
      2  halfadd registered without a tree launcher: its tree through folds, scratch allocated on every call; chained
         through leaf 0 as stream 1's
      3  binary16 PROD folds in place, m = 2, on factors near one
    2 MiB operands."""
    import torch

    import f16_ref
    from chiara_amd import ops

    halfadd = ca.op_create(_addr(_lib("libhalfadd_op.so", "").chr_test_halfadd))
    f16_prod = ops.float16_op(ca.PROD)
    try:
        streams = [su.nonblocking_stream() for _ in range(4)]
        assert len({s.cuda_stream for s in streams}) == 4
        G = su.nonblocking_stream()
        n4, n2 = OPERAND_BYTES // 4, OPERAND_BYTES // 2
        # host operands and reference chains
        a0 = [po.fill(n4, "f32", 0, 41, r) for r in range(4)]
        ref0 = a0[0].copy()
        for _ in range(ROUNDS):
            po.reduce_multi(ref0, a0[1:], "f32", "sum")
        l1 = [po.fill(n2, "bf16", 0, 43, r) for r in range(8)]
        ref1, leaf0 = [], l1[0]
        for _ in range(ROUNDS):
            leaf0 = tree_ref([leaf0] + l1[1:], C4, C4_SWAPS, "bf16", "sum")
            ref1.append(leaf0)
        l2 = [po.fill(n4, "f32", 0, 47, r) for r in range(8)]
        ref2, leaf0 = [], l2[0]
        for _ in range(ROUNDS):
            leaf0 = tree_ref([leaf0] + l2[1:], C4, C4_SWAPS, "f32", OPN)
            ref2.append(leaf0)
        rng = np.random.default_rng(53)
        a3 = [rng.uniform(0.97, 1.03, n2).astype(np.float16).view(np.uint16) for _ in range(3)]
        ref3 = a3[0].copy()
        for _ in range(ROUNDS):
            ref3 = f16_ref.fold_ref(ref3, a3[1:], "prod")
        # device buffers
        d0 = [gu.to_dev(x) for x in a0]
        d1, roots1 = [gu.to_dev(x) for x in l1], [gu.empty_dev(OPERAND_BYTES).fill_(0xA5) for _ in range(ROUNDS)]
        d2, roots2 = [gu.to_dev(x) for x in l2], [gu.empty_dev(OPERAND_BYTES).fill_(0xA5) for _ in range(ROUNDS)]
        d3 = [gu.to_dev(x) for x in a3]
        # warm-up on the NULL stream: module load and lazy initialisation (into the roots, rewritten below)
        assert ca.reduce_multi(roots1[0], d0[0], d0[1:], n4, ca.FLOAT32, ca.SUM, 0) == 0
        assert ca.reduce_tree(roots1[0], d1, C4, C4_SWAPS, n2, ca.BFLOAT16, ca.SUM, 0) == 0
        assert ca.reduce_tree(roots2[0], d2, C4, C4_SWAPS, n4, ca.FLOAT32, halfadd, 0) == 0
        assert ca.reduce_multi(roots2[1], d3[0], d3[1:], n2, ops.F16_DTYPE, f16_prod, 0) == 0
        for t in roots1 + roots2:
            t.fill_(0xA5)
        torch.cuda.synchronize(gu.DEV)
        t0 = time.perf_counter()
        with torch.cuda.stream(G):
            ev0, ev1 = gate.enqueue(G)
            opened = torch.cuda.Event()
            opened.record(G)
        for s in streams:
            s.wait_event(opened)
        h = [s.cuda_stream for s in streams]
        rcs, scratch_s = [], 0.0
        for r in range(ROUNDS):
            rcs.append(ca.reduce_multi(d0[0], d0[0], d0[1:], n4, ca.FLOAT32, ca.SUM, h[0]))
            lv = [d1[0] if r == 0 else roots1[r - 1]] + d1[1:]
            rcs.append(ca.reduce_tree(roots1[r], lv, C4, C4_SWAPS, n2, ca.BFLOAT16, ca.SUM, h[1]))
            lv = [d2[0] if r == 0 else roots2[r - 1]] + d2[1:]
            t2 = time.perf_counter()
            rcs.append(ca.reduce_tree(roots2[r], lv, C4, C4_SWAPS, n4, ca.FLOAT32, halfadd, h[2]))
            scratch_s += time.perf_counter() - t2
            rcs.append(ca.reduce_multi(d3[0], d3[0], d3[1:], n2, ops.F16_DTYPE, f16_prod, h[3]))
        still_closed, enqueue_s = not ev1.query(), time.perf_counter() - t0
        for s in streams:
            s.synchronize()
        times = (f"host time to enqueue the {4 * ROUNDS} calls {enqueue_s * 1e3:.3f} ms, of which the {ROUNDS} trees "
                 f"through scratch {scratch_s * 1e3:.3f} ms; gate {ev0.elapsed_time(ev1):.3f} ms")
        print("four streams: " + times)
        assert rcs == [0] * (4 * ROUNDS), rcs
        assert still_closed, f"inconclusive: the gate opened before the last call was enqueued ({times})"
        assert np.array_equal(_bits(_read(gu, d0[0], np.float32, n4)), _bits(ref0)), "stream 0: f32 SUM chain"
        for r in range(ROUNDS):
            assert np.array_equal(_bits(_read(gu, roots1[r], np.uint16, n2)), _bits(ref1[r])), f"stream 1: bf16 tree, round {r}"
            assert np.array_equal(_bits(_read(gu, roots2[r], np.float32, n4)), _bits(ref2[r])), f"stream 2: halfadd tree, round {r}"
        assert np.array_equal(_read(gu, d3[0], np.uint16, n2), ref3), "stream 3: binary16 PROD chain"
        for name, dev, host, npdt, n in (("f32", d0[1:], a0[1:], np.float32, n4), ("bf16", d1, l1, np.uint16, n2),
                                         ("halfadd", d2, l2, np.float32, n4), ("f16", d3[1:], a3[1:], np.uint16, n2)):
            for j, (t, x) in enumerate(zip(dev, host)):
                assert np.array_equal(_bits(_read(gu, t, npdt, n)), _bits(x)), f"{name}: input {j} changed"
    finally:
        assert ca.op_free(halfadd) == 0
        assert ops.release() == 0


# ---- four host threads ---------------------------------------------------------------------------------------------------------

NTHREADS, ITERATIONS, N = 4, 20, 4099
NS = 341  # derived elements of f32 x 3 in the rotmix fold


def test_four_host_threads(su, gu):
    """Each thread has its own non-blocking stream and buffers; behind a barrier each runs 20 iterations of: create a
    user op -> built-in fold -> user fold -> user tree through folds -> chr_type_contiguous + one rotmix fold +
    chr_type_free -> free the op.  Nothing synchronises until the thread's final stream synchronise; every iteration
    has its own outputs and is compared with its reference.  ctypes drops the GIL inside the calls."""
    import torch

    import struct_ref as sr

    half_fn = _addr(_lib("libhalfadd_op.so", "").chr_test_halfadd)
    rot_fn = _addr(_lib("libstruct_op.so", "-f struct_op.mk").chr_struct_RotMixK_f32x3)
    streams = [su.nonblocking_stream() for _ in range(NTHREADS)]
    assert len({s.cuda_stream for s in streams}) == NTHREADS
    work = []
    for t in range(NTHREADS):
        xs = [po.fill(N, "f32", 0, 61 + t, r) for r in range(9)]
        ss = [po.fill(3 * NS, "f32", 0, 71 + t, r) for r in range(3)]
        w = {"xs": xs, "ss": ss, "d_xs": [gu.to_dev(x) for x in xs], "d_ss": [gu.to_dev(x) for x in ss],
             "outs": [[gu.empty_dev(4 * N).fill_(0xA5) for _ in range(3)] + [gu.empty_dev(12 * NS).fill_(0xA5)]
                      for _ in range(ITERATIONS)], "rcs": [], "error": None}
        work.append(w)
    # warm-up on the NULL stream (module load of both code objects, lazy initialisation)
    op0, rot0, dt0 = ca.op_create(half_fn), ca.op_create(rot_fn), ca.type_contiguous(3, ca.FLOAT32)
    w = work[0]
    assert ca.reduce_multi(w["outs"][0][0], w["d_xs"][0], w["d_xs"][1:3], N, ca.FLOAT32, ca.SUM, 0) == 0
    assert ca.reduce_multi(w["outs"][0][1], w["d_xs"][0], w["d_xs"][1:3], N, ca.FLOAT32, op0, 0) == 0
    assert ca.reduce_tree(w["outs"][0][2], w["d_xs"][:8], C4, C4_SWAPS, N, ca.FLOAT32, op0, 0) == 0
    assert ca.reduce_multi(w["outs"][0][3], w["d_ss"][0], w["d_ss"][1:], NS, dt0, rot0, 0) == 0
    torch.cuda.synchronize(gu.DEV)
    for t in w["outs"][0]:
        t.fill_(0xA5)
    assert ca.op_free(op0) == 0 and ca.op_free(rot0) == 0 and ca.type_free(dt0) == 0
    torch.cuda.synchronize(gu.DEV)

    def operands_of(w, i):
        """Iteration i reads the thread's operands rotated by i, so that no two iterations agree."""
        idx = [(i + j) % 9 for j in range(8)]
        return idx

    barrier = threading.Barrier(NTHREADS)

    def body(t):
        w, h = work[t], streams[t].cuda_stream
        try:
            barrier.wait()
            for i in range(ITERATIONS):
                idx = operands_of(w, i)
                d = [w["d_xs"][j] for j in idx]
                o = w["outs"][i]
                op = ca.op_create(half_fn)
                rc = [ca.reduce_multi(o[0], d[0], d[1:3], N, ca.FLOAT32, ca.SUM, h),
                      ca.reduce_multi(o[1], d[0], d[1:3], N, ca.FLOAT32, op, h),
                      ca.reduce_tree(o[2], d, C4, C4_SWAPS, N, ca.FLOAT32, op, h)]
                dt = ca.type_contiguous(3, ca.FLOAT32)
                rot = ca.op_create(rot_fn)
                s = [w["d_ss"][(i + j) % 3] for j in range(3)]
                rc.append(ca.reduce_multi(o[3], s[0], s[1:], NS, dt, rot, h))
                rc.append(ca.type_free(dt))
                rc.append(ca.op_free(rot))
                rc.append(ca.op_free(op))
                w["rcs"].append(rc)
            streams[t].synchronize()
        except BaseException as e:  # noqa: BLE001 -- handed to the main thread
            w["error"] = e
            barrier.abort()

    threads = [threading.Thread(target=body, args=(t,)) for t in range(NTHREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120)
        assert not th.is_alive(), "a thread did not finish"
    torch.cuda.synchronize(gu.DEV)
    for t, w in enumerate(work):
        if w["error"] is not None:
            raise w["error"]
        assert w["rcs"] == [[0] * 7] * ITERATIONS, (t, w["rcs"])
        for i in range(ITERATIONS):
            x = [w["xs"][j] for j in operands_of(w, i)]
            s = [w["ss"][(i + j) % 3] for j in range(3)]
            want = [po.reduce_multi(x[0].copy(), [x[1].copy(), x[2].copy()], "f32", "sum"),
                    po.reduce_multi(x[0].copy(), [x[1].copy(), x[2].copy()], "f32", OPN),
                    tree_ref(x, C4, C4_SWAPS, "f32", OPN),
                    sr.fold_ref(s[0], s[1:], 3, sr.rotmix, False)]
            what = ("built-in fold", "user fold", "user tree through folds", "rotmix fold on f32 x 3")
            for k in range(4):
                got = _read(gu, w["outs"][i][k], np.float32, want[k].size)
                assert np.array_equal(_bits(got), _bits(want[k])), f"thread {t}, iteration {i}: {what[k]}"
        for j, x in enumerate(w["xs"]):
            assert np.array_equal(_bits(_read(gu, w["d_xs"][j], np.float32, N)), _bits(x)), f"thread {t}: input {j} changed"
