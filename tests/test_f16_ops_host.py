"""libchiara_ops.so on the host: registration (include/chiara_ops.h, chiara_amd/ops.py), the kernels' resources read
from the code object, and the self-check of the binary16 plan evaluator (tests/f16_ref.py).  No GPU."""
import ctypes
import os
import re
import sys
import threading

import numpy as np
import pytest

import chiara_amd as ca
import f16_ref
from chiara_amd import ops

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import kernel_resources as kr  # noqa: E402

KINDS = (ca.SUM, ca.PROD, ca.MAX, ca.MIN)
RCCL_ROOM_VGPRS = 72  # tests/test_kernel_resources.py: what a wave may hold beside RCCL's


@pytest.fixture(autouse=True)
def released():
    yield
    assert ops.release() == 0


# ---- registration ---------------------------------------------------------------------------------------------

def test_loading_registers_nothing_and_codes_are_stable():
    """Loading takes no code; the first call per kind registers one of 64..127, later calls return it."""
    ops.ops_lib()
    probe = [ca.op_create(_any_launcher()) for _ in range(64)]  # all 64 codes still free after the load
    for p in probe:
        assert ca.op_free(p) == 0
    codes = [ops.float16_op(k) for k in KINDS]
    assert len(set(codes)) == 4 and all(64 <= c <= 127 for c in codes), codes
    assert [ops.float16_op(k) for k in KINDS] == codes
    assert ops.F16_DTYPE == ca.UINT16 and ca.DTYPE_SIZE[ops.F16_DTYPE] == 2


def _any_launcher():
    return ctypes.cast(ops.ops_lib().chr_ops_f16_sum_fold, ctypes.c_void_p).value


def test_bad_kind_and_null_pointer_are_refused():
    L = ops.ops_lib()
    op = ctypes.c_int(-1)
    for kind in (ca.LAND, ca.BXOR, ca.MAXLOC, 64, -1):
        assert L.chr_ops_float16(kind, ctypes.byref(op)) == ca.ERR_UNSUPPORTED and op.value == -1
        with pytest.raises(ca.ChiaraError):
            ops.float16_op(kind)
    assert L.chr_ops_float16(ca.SUM, None) == ca.ERR_INVALID_ARG
    probe = [ca.op_create(_any_launcher()) for _ in range(64)]  # the refused calls registered nothing
    for p in probe:
        assert ca.op_free(p) == 0


def test_release_returns_the_codes():
    """After release the codes are dead (chr_op_free: CHR_ERR_INVALID_ARG), all 64 can be created again, and a later
    float16_op registers again."""
    codes = [ops.float16_op(k) for k in KINDS]
    assert ops.release() == 0
    for c in codes:
        assert ca.op_free(c) == ca.ERR_INVALID_ARG
    fresh = []
    try:
        for _ in range(64):
            fresh.append(ca.op_create(_any_launcher()))
        assert sorted(fresh) == list(range(64, 128))
        with pytest.raises(ca.ChiaraError) as e:  # a full registry: the registry's own error
            ops.float16_op(ca.SUM)
        assert e.value.code == ca.ERR_UNSUPPORTED
    finally:
        for c in fresh:
            assert ca.op_free(c) == 0
    again = ops.float16_op(ca.MAX)
    assert 64 <= again <= 127 and ops.float16_op(ca.MAX) == again
    assert ops.release() == 0 and ops.release() == 0  # nothing held: still success


def test_first_call_is_thread_safe():
    got, gate = [], threading.Barrier(8)

    def work():
        gate.wait()
        got.append(tuple(ops.float16_op(k) for k in KINDS))

    ts = [threading.Thread(target=work) for _ in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert len(got) == 8 and len(set(got)) == 1 and len(set(got[0])) == 4, got


def test_stats_round_trip():
    assert ops.stats(reset=True) is not None
    assert ops.stats() == (0, 0, 0)


# ---- resources --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def res():
    if not os.path.exists(kr.READELF):  # as tests/test_user_tree_resources.py
        pytest.skip("llvm-readelf not in this image")
    assert os.path.exists(ops.OPS_LIB_PATH), f"{ops.OPS_LIB_PATH} missing: __graft_entry__.build()"
    return kr.kernel_resources(ops.OPS_LIB_PATH)


def test_kernel_set_and_resources(res):
    """4 k_fold and 4 x 7 k_tree<_Float16, F, NL = 2..8, U = 4 / 2 / 1, 64>; no private segment, no static LDS, every
    kernel within the registers a wave has beside RCCL."""
    folds, trees = {}, {}
    for name, r in res.items():
        m = re.search(r"6k_foldIDF16_N7chr_ops\d+(F16[A-Za-z]+)EEE", name)
        if m:
            folds[m.group(1)] = r
        m = re.search(r"6k_treeIDF16_N7chr_ops\d+(F16[A-Za-z]+)ELi(\d+)ELi(\d+)ELi64EEE", name)
        if m:
            trees[(m.group(1), int(m.group(2)), int(m.group(3)))] = r
    names = {"F16Sum", "F16Prod", "F16Max", "F16Min"}
    assert set(folds) == names, sorted(res)
    u = {2: 4, 3: 2, 4: 2, 5: 1, 6: 1, 7: 1, 8: 1}
    assert set(trees) == {(f, nl, u[nl]) for f in names for nl in range(2, 9)}, sorted(trees)
    assert len(res) == 4 + 4 * 7, sorted(res)
    for name, r in res.items():
        assert r["scratch"] == 0, f"{name}: a private segment of {r['scratch']} bytes"
        assert r["lds"] == 0, f"{name}: {r['lds']} bytes of static LDS"
        assert kr.alloc_vgprs(r) <= RCCL_ROOM_VGPRS, f"{name}: {kr.alloc_vgprs(r)} VGPRs"


# ---- the plan evaluator ------------------------------------------------------------------------------------------

def test_reference_restates_the_functors():
    """A few hand-checked values of each op, so that the reference itself is pinned."""
    def c(op, x, y):
        return int(f16_ref.combine(op, np.array([x], np.uint16), np.array([y], np.uint16))[0])

    assert c("sum", 0x3C00, 0x3C00) == 0x4000  # 1 + 1
    assert c("sum", 0x0001, 0x0001) == 0x0002  # subnormals kept
    assert c("sum", 0x7BFF, 0x7BFF) == 0x7C00  # overflow to inf
    assert c("sum", 0x7C00, 0xFC00) == 0x7E00  # inf - inf
    assert c("sum", 0xFD01, 0x3C00) == 0x7E00  # any NaN: canonical
    assert c("prod", 0x0400, 0x3800) == 0x0200  # min normal * 0.5: a subnormal result
    assert c("prod", 0x0000, 0x7C00) == 0x7E00
    assert c("max", 0x0000, 0x8000) == 0x0000 and c("max", 0x8000, 0x0000) == 0x8000  # a tie returns `in`
    assert c("max", 0x7D01, 0x3C00) == 0x7D01 and c("max", 0x3C00, 0x7D01) == 0x3C00  # unordered returns `in`
    assert c("max", 0x3C00, 0x4000) == 0x4000 and c("min", 0x3C00, 0x4000) == 0x3C00
    assert c("min", 0xFE55, 0x3C00) == 0xFE55


def _is_one_rank_order_fold(n, k, b, count):
    """Whether the REFERENCE plans hold a single reduction over all n ranks' inputs in rank order: then the reference
    order IS the plain left fold.  Read from the plans, not from the geometry."""
    import plan_sim

    plans = plan_sim.load_plans(ca.MODE_ALLREDUCE, n, k, b, count, schedule=ca.SCHEDULE_REFERENCE)
    reds = [op for p in plans for st in [{"post": p["pre"]}] + p["steps"] for op in st["post"]
            if op[0] in ("reduce", "reduce_sw", "tree") and op[4]]
    if len(reds) != 1 or reds[0][0] != "reduce" or len(reds[0][4]) != n - 1:
        return False
    offs = [off for _, off in reds[0][4]]
    return offs == sorted(offs)  # STAGE slots in the order the peers 1..n-1 were received


@pytest.mark.parametrize("n,k,b", [(8, 4, 4), (8, 2, 2), (6, 4, 6), (4, 4, 4)])
def test_plan_evaluator_self_check(n, k, b):
    """REFERENCE, FLAT, FLAT_1SHOT and EXACT plans give identical bits under f16 SUM on U[-1, 1), and those bits
    differ from a plain rank-order left fold somewhere: the data can tell orders apart.

    At (4, 4, 4) the reference's order is itself the rank-order left fold -- one group of four, rank 0 folds s1, s2, s3
    into s0 in one reduction (the REFERENCE plan says so, _is_one_rank_order_fold) -- so no data can differ from it
    there.  That geometry is held to the stronger statement, equality with the left fold, and the data's power to tell
    orders apart is shown against the pairwise order (s0 + s1) + (s2 + s3) instead."""
    count = n * 257
    sends = [f16_ref.uniform(count, 31, r) for r in range(n)]
    want = f16_ref.expected(ca.MODE_ALLREDUCE, sends, k, b, "sum", ca.SCHEDULE_REFERENCE)
    for sch in (ca.SCHEDULE_FLAT, ca.SCHEDULE_FLAT_1SHOT, ca.SCHEDULE_EXACT):
        got = f16_ref.expected(ca.MODE_ALLREDUCE, sends, k, b, "sum", sch)
        for r in range(n):
            np.testing.assert_array_equal(got[r], want[r], err_msg=f"schedule {sch} rank {r}")
    for r in range(1, n):
        np.testing.assert_array_equal(want[r], want[0])
    assert want[0].dtype == np.uint16 and want[0].size == count
    left = f16_ref.left_fold(sends, "sum")
    if _is_one_rank_order_fold(n, k, b, count):
        np.testing.assert_array_equal(want[0], left)
        pairs = [f16_ref.combine("sum", sends[i], sends[i + 1]) for i in range(0, n, 2)]
        assert np.count_nonzero(want[0] != f16_ref.left_fold(pairs, "sum")) >= 1
    else:
        assert np.count_nonzero(want[0] != left) >= 1
