"""Derived element types (chr_type_contiguous, MPI_Type_contiguous's analogue) on the host: the registry, the sizes and
the refusals need no device.  The device side is tests/test_gpu_struct_op.py."""
import ctypes

import numpy as np
import pytest

import chiara_amd as ca
import pyoracle as po
import struct_ref as sr

L = ca.lib()
PREDEFINED = {ca.FLOAT32: 4, ca.FLOAT64: 8, ca.INT32: 4, ca.BFLOAT16: 2, ca.INT8: 1, ca.UINT8: 1, ca.INT16: 2,
              ca.UINT16: 2, ca.UINT32: 4, ca.INT64: 8, ca.UINT64: 8, ca.FLOAT_INT: 8, ca.DOUBLE_INT: 16,
              ca.LONG_INT: 16, ca.TWO_INT: 8, ca.SHORT_INT: 8, ca.C_FLOAT_COMPLEX: 8, ca.C_DOUBLE_COMPLEX: 16}


def _create(count, base):
    t = ctypes.c_int(-1)
    return L.chr_type_contiguous(count, base, ctypes.byref(t)), t.value


def _size(t):
    n = ctypes.c_size_t(0)
    return L.chr_type_size(t, ctypes.byref(n)), n.value


def _contents(t):
    base, count = ctypes.c_int(-1), ctypes.c_int(-1)
    return L.chr_type_get_contiguous(t, ctypes.byref(base), ctypes.byref(count)), base.value, count.value


def test_abi_version_stays_11():
    assert L.chr_abi_version() == 11


def test_registry_codes_limit_and_reuse():
    """Codes 64..127, 64 live at once, the 65th refused, a freed code handed out again, a double free and a predefined
    or unknown code refused."""
    made = []
    for i in range(64):
        rc, t = _create(i + 1, ca.FLOAT64)
        assert rc == 0
        made.append(t)
    try:
        assert sorted(made) == list(range(64, 128))
        assert _create(3, ca.FLOAT32)[0] == ca.ERR_UNSUPPORTED
        for i, t in enumerate(made):
            assert _size(t) == (0, 8 * (i + 1))
            assert _contents(t) == (0, ca.FLOAT64, i + 1)
        assert L.chr_type_free(made[5]) == 0 and L.chr_type_free(made[5]) == ca.ERR_INVALID_ARG
        assert _size(made[5])[0] == ca.ERR_INVALID_ARG and _contents(made[5])[0] == ca.ERR_INVALID_ARG
        rc, t = _create(7, ca.INT16)
        assert rc == 0 and t == made[5] and _size(t) == (0, 14) and _contents(t) == (0, ca.INT16, 7)
    finally:
        for t in made:
            assert L.chr_type_free(t) == 0
    for t in made:
        assert L.chr_type_free(t) == ca.ERR_INVALID_ARG
    for t in (ca.FLOAT32, ca.C_DOUBLE_COMPLEX, 18, 63, 128, 200, -1):
        assert L.chr_type_free(t) == ca.ERR_INVALID_ARG


def test_type_size_of_every_predefined_type():
    assert PREDEFINED == ca.DTYPE_SIZE and len(PREDEFINED) == 18
    for t, size in PREDEFINED.items():
        assert _size(t) == (0, size)
        assert _contents(t) == (0, t, 1)
        assert ca.type_size(t) == size and ca.type_get_contiguous(t) == (t, 1)
    for t in (18, 63, 64, 127, 128, -1):  # unknown, and derived codes that are not live
        assert _size(t)[0] == ca.ERR_INVALID_ARG and _contents(t)[0] == ca.ERR_INVALID_ARG
    assert L.chr_type_size(ca.FLOAT32, None) == ca.ERR_INVALID_ARG


def test_rejected_creations():
    assert _create(0, ca.FLOAT32)[0] == ca.ERR_INVALID_ARG
    assert _create(-3, ca.FLOAT32)[0] == ca.ERR_INVALID_ARG
    assert _create(3, 18)[0] == ca.ERR_INVALID_ARG
    assert L.chr_type_contiguous(3, ca.FLOAT32, None) == ca.ERR_INVALID_ARG
    t = ca.type_contiguous(3, ca.FLOAT64)
    try:
        assert _create(2, t)[0] == ca.ERR_INVALID_ARG  # no nesting
    finally:
        assert ca.type_free(t) == 0
    # an element is at most 65536 bytes
    rc, t = _create(8192, ca.FLOAT64)
    assert rc == 0 and _size(t) == (0, 65536) and L.chr_type_free(t) == 0
    assert _create(8193, ca.FLOAT64)[0] == ca.ERR_INVALID_ARG
    assert _create(4097, ca.C_DOUBLE_COMPLEX)[0] == ca.ERR_INVALID_ARG
    assert _create(65537, ca.UINT8)[0] == ca.ERR_INVALID_ARG
    assert _create(2 ** 31 - 1, ca.FLOAT64)[0] == ca.ERR_INVALID_ARG


def test_python_wrappers_round_trip():
    t = ca.type_contiguous(3, ca.FLOAT64)
    try:
        assert 64 <= t <= 127 and ca.type_size(t) == 24 and ca.type_get_contiguous(t) == (ca.FLOAT64, 3)
    finally:
        assert ca.type_free(t) == 0
    assert ca.type_free(t) == ca.ERR_INVALID_ARG
    with pytest.raises(ca.ChiaraError):
        ca.type_size(t)


def test_predefined_op_on_a_derived_type_is_unsupported_without_device():
    """MPI's predefined ops take no derived type (MPICH: MPI_ERR_OP): CHR_ERR_UNSUPPORTED before anything is looked at
    -- the pointers here are never read -- and CHR_ERR_INVALID_ARG once the type is dead or with a dead user op."""
    t = ca.type_contiguous(3, ca.FLOAT64)
    leaves = (ctypes.c_void_p * 2)(0x1000, 0x2000)
    ins = (ctypes.c_void_p * 1)(0x2000)
    try:
        for op in (ca.SUM, ca.MAX, ca.BXOR, ca.MINLOC):
            assert L.chr_reduce_tree(0x3000, leaves, 2, bytes([0, 1]), None, 0, t, op, None) == ca.ERR_UNSUPPORTED
            assert L.chr_reduce_multi(0x3000, 0x1000, ins, 1, 0, t, op, None) == ca.ERR_UNSUPPORTED
            assert L.chr_reduce_local(0x1000, 0x3000, 0, t, op, None) == ca.ERR_UNSUPPORTED
        assert L.chr_reduce_tree(0x3000, leaves, 2, bytes([0, 1]), None, 0, t, 12, None) == ca.ERR_INVALID_ARG
        assert L.chr_reduce_tree(0x3000, leaves, 2, bytes([0, 1]), None, 0, t, 100, None) == ca.ERR_INVALID_ARG  # no such op
        # a live user op on the derived type passes the check (n = 0: nothing to do, no launcher is called)
        fn = ctypes.cast(L.chr_abi_version, ctypes.c_void_p).value  # any address: never called here
        op = ca.op_create(fn)
        try:
            assert L.chr_reduce_tree(0x3000, leaves, 2, bytes([0, 1]), None, 0, t, op, None) == 0
            assert L.chr_reduce_multi(0x3000, 0x1000, ins, 1, 0, t, op, None) == 0
        finally:
            assert ca.op_free(op) == 0
    finally:
        assert ca.type_free(t) == 0
    assert L.chr_reduce_tree(0x3000, leaves, 2, bytes([0, 1]), None, 0, t, ca.SUM, None) == ca.ERR_INVALID_ARG


def test_fill_rejects_a_derived_type():
    t = ca.type_contiguous(3, ca.FLOAT32)
    try:
        assert L.chr_fill(0x1000, 0, t, 0, 0, 0, 0, None) == ca.ERR_INVALID_ARG
        assert L.chr_fill(0x1000, 16, t, 0, 0, 0, 0, None) == ca.ERR_INVALID_ARG
    finally:
        assert ca.type_free(t) == 0


# ---- the reference helper of the device tests checks itself against the oracle -------------------

@pytest.mark.parametrize("dt", ["f32", "f64", "i32"])
def test_struct_ref_halfadd_is_the_oracles_user_halfadd(dt):
    """K = 1 (and K = 3 on 3n base elements) HalfAdd folds and trees of struct_ref reproduce pyoracle's user_halfadd
    on the same inputs, bit for bit: the numpy arithmetic the device tests trust is the oracle's."""
    import tree_util

    n = 1000
    rng = np.random.default_rng(5)
    for k in (1, 3):
        acc = po.fill(n * k, dt, po.PAT_UNIFORM, 3, 0)
        ins = [po.fill(n * k, dt, po.PAT_UNIFORM, 3, r) for r in (1, 2, 3)]
        want = po.reduce_multi(acc.copy(), [x.copy() for x in ins], dt, "user_halfadd")
        got = sr.fold_ref(acc, ins, k, sr.halfadd, running_first=False)
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
        for nl in (2, 5, 8):
            comb, swaps = tree_util.random_program(rng, nl)
            leaves = [po.fill(n * k, dt, po.PAT_UNIFORM, 7, r) for r in range(nl)]
            want = tree_util.tree_ref(leaves, comb, swaps, dt, "user_halfadd")
            got = sr.tree_ref(leaves, comb, swaps, k, sr.halfadd)
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (dt, k, comb, swaps)


def test_struct_ref_plan_interpreter_is_plan_sim_for_halfadd():
    """struct_ref.simulate with HalfAdd on K = 3 equals plan_sim on 3x the base count (chunk boundaries coincide)."""
    import plan_sim

    n, k, b, cnt = 6, 3, 2, 6 * 7
    sends = [po.fill(cnt * 3, "f64", po.PAT_UNIFORM, 11, r) for r in range(n)]
    for schedule in (ca.SCHEDULE_FLAT, ca.SCHEDULE_EXACT):
        want = plan_sim.simulate(ca.MODE_ALLREDUCE, sends, k, b, "f64", "user_halfadd", schedule=schedule)
        got = sr.simulate(ca.MODE_ALLREDUCE, sends, k, b, 3, sr.halfadd, schedule=schedule)
        for r in range(n):
            assert np.array_equal(got[r].view(np.uint8), want[r].view(np.uint8)), (schedule, r)
