"""libchiara_numerics.so on the host: registration (include/chiara_numerics.h, chiara_amd/numerics.py), the kernels'
resources read from the code object, and the numpy restatement of the two functors (tests/numerics_ref.py) held to
what the header promises of them.  No GPU."""
import ctypes
import os
import re
import sys
import threading

import numpy as np
import pytest

import chiara_amd as ca
import numerics_ref as nr
import pyoracle as po
import struct_ref as sr
from chiara_amd import numerics as num

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import kernel_resources as kr  # noqa: E402

RCCL_ROOM_VGPRS = 72  # tests/test_kernel_resources.py: what a wave may hold beside RCCL's
BASES = (ca.FLOAT32, ca.FLOAT64)


@pytest.fixture(autouse=True)
def released():
    yield
    assert num.release() == 0


# ---- registration ---------------------------------------------------------------------------------------------

def _any_launcher():
    return ctypes.cast(num.num_lib().chr_num_sum2_fold, ctypes.c_void_p).value


def _all_op_codes_free():
    probe = [ca.op_create(_any_launcher()) for _ in range(64)]
    for p in probe:
        assert ca.op_free(p) == 0
    return sorted(probe) == list(range(64, 128))


def _all_type_codes_free():
    probe = [ca.type_contiguous(5, ca.UINT8) for _ in range(64)]
    for t in probe:
        assert ca.type_free(t) == 0
    return sorted(probe) == list(range(64, 128))


def test_loading_registers_nothing_and_codes_are_stable():
    """Loading takes no op code and no type code; the first request registers, later ones return the same code."""
    num.num_lib()
    assert _all_op_codes_free() and _all_type_codes_free()
    ops = [num.sum2_op(), num.moments_op()]
    types = [num.sum2_type(b) for b in BASES] + [num.moments_type(b) for b in BASES]
    assert len(set(ops)) == 2 and all(64 <= c <= 127 for c in ops), ops
    assert len(set(types)) == 4 and all(64 <= t <= 127 for t in types), types
    assert [num.sum2_op(), num.moments_op()] == ops
    assert [num.sum2_type(b) for b in BASES] + [num.moments_type(b) for b in BASES] == types
    assert [ca.type_get_contiguous(t) for t in types] == [(ca.FLOAT32, 2), (ca.FLOAT64, 2), (ca.FLOAT32, 3),
                                                          (ca.FLOAT64, 3)]
    assert [ca.type_size(t) for t in types] == [8, 16, 12, 24]


def test_bad_base_and_null_pointer_are_refused():
    L = num.num_lib()
    t = ctypes.c_int(-1)
    for fn, wrapper in ((L.chr_num_sum2_type, num.sum2_type), (L.chr_num_moments_type, num.moments_type)):
        for base in (ca.INT32, ca.BFLOAT16, ca.UINT16, ca.C_FLOAT_COMPLEX, 64, -1):
            assert fn(base, ctypes.byref(t)) == ca.ERR_UNSUPPORTED and t.value == -1
            with pytest.raises(ca.ChiaraError):
                wrapper(base)
        assert fn(ca.FLOAT32, None) == ca.ERR_INVALID_ARG
    assert L.chr_num_sum2(None) == ca.ERR_INVALID_ARG and L.chr_num_moments(None) == ca.ERR_INVALID_ARG
    # pack / unpack: the argument checks come before anything touches the device
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert L.chr_num_sum2_pack(None, p, 1, ca.FLOAT32, None) == ca.ERR_INVALID_ARG
    assert L.chr_num_sum2_pack(p, None, 1, ca.FLOAT32, None) == ca.ERR_INVALID_ARG
    assert L.chr_num_sum2_unpack(None, p, 1, ca.FLOAT64, None) == ca.ERR_INVALID_ARG
    assert L.chr_num_moments_pack(p, None, 1, ca.FLOAT64, None) == ca.ERR_INVALID_ARG
    assert L.chr_num_moments_unpack(p, p, p, None, 1, ca.FLOAT32, None) == ca.ERR_INVALID_ARG
    assert L.chr_num_moments_unpack(None, None, None, p, 1, ca.FLOAT32, None) == ca.ERR_INVALID_ARG
    for fn in (L.chr_num_sum2_pack, L.chr_num_sum2_unpack, L.chr_num_moments_pack):
        assert fn(p, p, 1, ca.INT32, None) == ca.ERR_UNSUPPORTED
    assert L.chr_num_moments_unpack(p, p, p, p, 1, ca.UINT32, None) == ca.ERR_UNSUPPORTED
    assert L.chr_num_sum2_pack(p, p, 0, ca.FLOAT32, None) == 0  # n == 0: nothing enqueued, success
    assert _all_op_codes_free() and _all_type_codes_free()  # the refused calls registered nothing


def test_release_returns_the_codes():
    """After release the op codes and type codes are dead, all 64 + 64 can be created again, and a later request
    registers again."""
    ops = [num.sum2_op(), num.moments_op()]
    types = [num.sum2_type(b) for b in BASES] + [num.moments_type(b) for b in BASES]
    assert num.release() == 0
    for c in ops:
        assert ca.op_free(c) == ca.ERR_INVALID_ARG
    for t in types:
        assert ca.type_free(t) == ca.ERR_INVALID_ARG
    assert _all_op_codes_free() and _all_type_codes_free()
    again = num.moments_op()
    assert 64 <= again <= 127 and num.moments_op() == again
    t = num.sum2_type(ca.FLOAT64)
    assert ca.type_get_contiguous(t) == (ca.FLOAT64, 2)
    assert num.release() == 0 and num.release() == 0  # nothing held: still success


def test_first_call_is_thread_safe():
    got, gate = [], threading.Barrier(8)

    def work():
        gate.wait()
        got.append((num.sum2_op(), num.moments_op()) + tuple(num.sum2_type(b) for b in BASES)
                   + tuple(num.moments_type(b) for b in BASES))

    ts = [threading.Thread(target=work) for _ in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert len(got) == 8 and len(set(got)) == 1, got
    assert len(set(got[0][:2])) == 2 and len(set(got[0][2:])) == 4, got


def test_stats_round_trip():
    assert num.stats(reset=True) is not None
    assert num.stats() == (0, 0, 0)


# ---- resources --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def res():
    if not os.path.exists(kr.READELF):  # as tests/test_f16_ops_host.py
        pytest.skip("llvm-readelf not in this image")
    assert os.path.exists(num.NUM_LIB_PATH), f"{num.NUM_LIB_PATH} missing: __graft_entry__.build()"
    return kr.kernel_resources(num.NUM_LIB_PATH)


def test_kernel_set_and_resources(res):
    """40 kernels: 4 k_fold (Sum2 and Moments on float and double), their 4 x 7 k_tree for NL = 2..8 -- the 8- and
    16-byte pairs at U = 4 / 2 / 1, the 12- and 24-byte records element-wise (U = 0) -- and 4 k_pack + 4 k_unpack
    (K = 2, 3 on float and double).  No private segment and no static LDS anywhere; at most 72 allocated VGPRs for
    every fold, every pack / unpack kernel and every tree with U > 0.  The element-wise trees' registers are printed
    (DESIGN section 2 records them)."""
    folds, trees, conv = {}, {}, set()
    for name in res:
        m = re.search(r"6k_foldIN7chr_num\d+(Pair|Rec)I([fd])EENS\d+_\d+(Sum2|Moments)I[fd]EEEE", name)
        if m:
            folds[(m.group(3), m.group(2))] = name
        m = re.search(r"6k_treeIN7chr_num\d+(Pair|Rec)I([fd])EENS\d+_\d+(Sum2|Moments)I[fd]EELi(\d+)ELi(\d+)ELi64EEE",
                      name)
        if m:
            trees[(m.group(3), m.group(2), int(m.group(4)), int(m.group(5)))] = name
        m = re.search(r"7chr_num\d+k_(pack|unpack)I([fd])Li(\d)EEE", name)
        if m:
            conv.add((m.group(1), m.group(2), int(m.group(3))))
    kinds = {(f, b) for f in ("Sum2", "Moments") for b in "fd"}
    assert set(folds) == kinds, sorted(res)
    u = {2: 4, 3: 2, 4: 2, 5: 1, 6: 1, 7: 1, 8: 1}
    want = {(f, b, nl, u[nl] if f == "Sum2" else 0) for f, b in kinds for nl in range(2, 9)}
    assert set(trees) == want, sorted(trees)
    assert conv == {(d, b, k) for d in ("pack", "unpack") for b in "fd" for k in (2, 3)}, sorted(conv)
    assert len(res) == 4 + 4 * 7 + 8 == 40, sorted(res)
    for name, r in res.items():
        assert r["scratch"] == 0, f"{name}: a private segment of {r['scratch']} bytes"
        assert r["lds"] == 0, f"{name}: {r['lds']} bytes of static LDS"
    elementwise = {key: name for key, name in trees.items() if key[3] == 0}
    for name, r in res.items():
        if name not in elementwise.values():
            assert kr.alloc_vgprs(r) <= RCCL_ROOM_VGPRS, f"{name}: {kr.alloc_vgprs(r)} VGPRs"
    for (f, b, nl, _), name in sorted(elementwise.items()):
        print(f"element-wise tree {f}<{'float' if b == 'f' else 'double'}> NL={nl}: "
              f"{kr.alloc_vgprs(res[name])} VGPRs")


# ---- the reference itself --------------------------------------------------------------------------------------

def _rows(T, *rows):
    return np.array(rows, dtype=T)


@pytest.mark.parametrize("T", nr.BASES)
def test_reference_restates_sum2(T):
    """A few hand-checked values, so that the reference itself is pinned."""
    fi = np.finfo(T)
    h = fi.eps / T(4)  # a quarter ulp of 1: lost by the plain sum, kept in lo

    def f(x, y):
        return nr.sum2(_rows(T, x), _rows(T, y))[0]

    def same(got, want):
        assert nr.bits(got).tolist() == nr.bits(np.array(want, dtype=T)).tolist(), (got, want)

    same(f((1, 0), (h, 0)), (1, h))
    same(f((h, 0), (1, 0)), (1, h))
    same(f((1, h), (1, h)), (2, 2 * h))
    same(f((1, h), (-1, 0)), (h, 0))                 # the cancelled head leaves the tail, renormalised
    same(f((1, h), (h, 0)), (1, 2 * h))              # two quarter ulps make half an ulp: still in lo
    same(f((1, 2 * h), (2 * h, 0)), (1 + fi.eps, 0))  # ... and a whole ulp moves into hi
    same(f((0.0, 0), (-0.0, 0)), (0.0, 0.0))
    same(f((fi.max, 0), (fi.max, 0)), (np.inf, 0))
    same(f((-fi.max, 0), (-fi.max / 2, 0)), (-np.inf, 0))
    same(f((fi.max, 0), (-fi.max, 0)), (0, 0))
    got = f((np.inf, 0), (-np.inf, 0))
    assert nr.bits(got).tolist() == [int(nr.QNAN_BITS[np.dtype(T)]), 0]
    got = f((-np.nan, 0), (1, 0))
    assert nr.bits(got).tolist() == [int(nr.QNAN_BITS[np.dtype(T)]), 0]
    same(f((np.inf, 0), (1, h)), (np.inf, 0))


@pytest.mark.parametrize("T", nr.BASES)
def test_reference_restates_moments(T):
    def f(x, y):
        return nr.moments(_rows(T, x), _rows(T, y))[0]

    def same(got, want):
        assert nr.bits(got).tolist() == nr.bits(np.array(want, dtype=T)).tolist(), (got, want)

    same(f((1, 2, 0), (1, 4, 0)), (2, 3, 2))           # samples 2, 4: mean 3, M2 = 1 + 1
    same(f((1, 4, 0), (1, 2, 0)), (2, 3, 2))
    same(f((2, 3, 2), (1, 6, 0)), (3, 4, 8))           # 2, 4, 6: mean 4, M2 = 4 + 0 + 4
    same(f((1, 6, 0), (2, 3, 2)), (3, 4, 8))
    same(f((0, 0, 0), (3, 5, 7)), (3, 5, 7))           # the identity, on either side
    same(f((3, 5, 7), (0, 0, 0)), (3, 5, 7))
    same(f((-0.0, -0.0, -0.0), (3, 5, 7)), (3, 5, 7))
    same(f((0, 0, 0), (0, 0, 0)), (0, 0, 0))           # no 0 / 0
    q = int(nr.QNAN_BITS[np.dtype(T)])
    assert nr.bits(f((np.nan, 1, 1), (1, 1, 1))).tolist() == [q, q, q]
    assert nr.bits(f((np.inf, 1, 1), (-np.inf, 1, 1))).tolist() == [q, q, q]
    same(f((1, np.inf, 0), (1, 1, 0)), (2, np.inf, np.inf))
    got = f((1, np.inf, 0), (1, -np.inf, 0))           # d = inf, mean = -inf + inf: n stays a number, the NaN is canonical
    two, inf = (int(v) for v in nr.bits(np.array([2, np.inf], dtype=T)))
    assert nr.bits(got).tolist() == [two, q, inf]


@pytest.mark.parametrize("T", nr.BASES)
def test_sum2_commutes_bitwise_and_stays_normalised(T):
    """f(x, y) and f(y, x) are bit-identical on all 2 020^2 pairs, and every finite result is normalised."""
    x, y = nr.cross(nr.sum2_partners(T))
    assert x.shape[0] == 4080400
    a, b = nr.sum2(x, y), nr.sum2(y, x)
    diff = np.flatnonzero((nr.bits(a) != nr.bits(b)).any(axis=1))
    assert diff.size == 0, f"{diff.size} pairs differ, first: x={x[diff[0]]} y={y[diff[0]]} {a[diff[0]]} {b[diff[0]]}"
    fin = np.isfinite(a[:, 0])
    with np.errstate(all="ignore"):
        assert np.array_equal(a[fin, 0] + a[fin, 1], a[fin, 0])
    assert np.array_equal(nr.bits(a[~fin, 1]), np.zeros(np.count_nonzero(~fin), dtype=nr.UINT[np.dtype(T)]))


@pytest.mark.parametrize("T", nr.BASES)
def test_moments_commutes_bitwise(T):
    """Bit-identical in both operand orders on all 1 456^2 ordered pairs."""
    x, y = nr.cross(nr.moments_partners(T))
    assert x.shape[0] == 2119936
    a, b = nr.moments(x, y), nr.moments(y, x)
    diff = np.flatnonzero((nr.bits(a) != nr.bits(b)).any(axis=1))
    assert diff.size == 0, f"{diff.size} pairs differ, first: x={x[diff[0]]} y={y[diff[0]]} {a[diff[0]]} {b[diff[0]]}"


@pytest.mark.parametrize("T,name", [(np.float32, "f32"), (np.float64, "f64")])
def test_sum2_does_not_depend_on_the_geometry(T, name):
    """Eight ranks of well-conditioned data (numerics_ref.independence_data, seed 31), packed as {x, 0}: the
    SCHEDULE_REFERENCE allreduce at (8, 4, 4), (8, 2, 2), (8, 2, 8) and (8, 8, 1) gives hi == T(math.fsum(...)) at
    every element of every rank for every geometry, while the oracle's plain SUM of the same data differs between at
    least two of those geometries somewhere: the data can tell the orders apart."""
    values = nr.independence_data(T)
    exact = nr.exact_sum(values)
    sends = [nr.sum2_pack(v) for v in values]
    plain = []
    for n, k, b in nr.GEOMETRIES:
        outs = sr.simulate(ca.MODE_ALLREDUCE, sends, k, b, 2, nr.sum2, schedule=ca.SCHEDULE_REFERENCE, commutative=True)
        for r, o in enumerate(outs):
            miss = int(np.count_nonzero(nr.bits(o.reshape(-1, 2)[:, 0]) != nr.bits(exact)))
            assert miss == 0, f"({n}, {k}, {b}) rank {r}: hi misses the exact sum at {miss} elements"
        plain.append(po.allreduce_radix_batch(values, k, b, name, "sum")[0])
    differing = max(int(np.count_nonzero(nr.bits(p) != nr.bits(plain[0]))) for p in plain[1:])
    print(f"plain {name} SUM: up to {differing} of {exact.size} elements differ between the geometries")
    assert differing >= 1


# measured on the CPU restatement: 3.7e-5 (float32) and 1.2e-13 (float64); the bound is four times that
MOMENTS_BOUND = {np.float32: 4 * 3.7e-5, np.float64: 4 * 1.2e-13}


@pytest.mark.parametrize("T", nr.BASES)
def test_moments_merge_matches_the_float64_variance(T):
    """Eight ranks of one sample each (mean 1000, sigma 3) through the (8, 4, 4) allreduce: n == 8 everywhere, the mean
    and M2 against float64's mean and variance x 8 of the same (rounded) samples."""
    values = nr.moments_data(T)
    sends = [nr.moments_pack(v) for v in values]
    outs = sr.simulate(ca.MODE_ALLREDUCE, sends, 4, 4, 3, nr.moments, schedule=ca.SCHEDULE_REFERENCE, commutative=True)
    cols = np.stack([v.astype(np.float64) for v in values])
    want_m2 = cols.var(axis=0) * 8
    for o in outs:
        rec = o.reshape(-1, 3)
        assert np.array_equal(rec[:, 0], np.full(rec.shape[0], 8, dtype=T))
        err = float(np.max(np.abs(rec[:, 2].astype(np.float64) - want_m2) / want_m2))
        print(f"{np.dtype(T).name}: M2 relative error {err:.3g}")
        assert err <= MOMENTS_BOUND[T], err
        assert float(np.max(np.abs(rec[:, 1].astype(np.float64) - cols.mean(axis=0)))) <= 1000 * 2 * np.finfo(T).eps
