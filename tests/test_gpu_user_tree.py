"""One-pass expression trees for user-defined ops (chr_op_create_tree) on the device, bit for bit.

The op is tests/userop/halfadd_tree_op.hip: the non-commutative halfadd of test_gpu_user_op.py (the oracle's
ORC_USER_HALFADD) registered with both launchers -- the fold launcher and a tree launcher built from the same
functors through include/chiara_user_op.hpp (k_tree) -- and host-side counters of what the library asked of each.
Every tree of the library must reach the tree launcher (one call per batch, no fold call), give the bits of
tree_util.tree_ref on every path of the kernel (vector trips, the partial trip, the element tail, the element-wise
path of a misaligned tree, output into a leaf), and fall back to the folds when the launcher declines.  The
collectives are checked against the reference's own outputs for this op (tests/golden/userop_outputs.npz)."""
import ctypes
import os

import numpy as np
import pytest

import chiara_amd as ca
import pyoracle as po
from test_gpu_user_op import C4_TREE, FIX, MAN, SWAP_TREE, _run_case
from tree_util import random_program, tree_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TREE_SO = os.path.join(HERE, "userop", "libhalfadd_tree_op.so")
OPN = "user_halfadd"
DT = {"f32": (ca.FLOAT32, np.float32), "f64": (ca.FLOAT64, np.float64), "i32": (ca.INT32, np.int32)}


class UserTree(ctypes.Structure):  # chiara.h chr_user_tree
    _fields_ = [("out", ctypes.c_void_p), ("leaves", ctypes.c_void_p * 8), ("nleaves", ctypes.c_int),
                ("comb", ctypes.c_ubyte * 8), ("swaps", ctypes.c_ubyte * 8), ("n", ctypes.c_size_t)]


@pytest.fixture(scope="module")
def gu():
    import gpu_util

    return gpu_util


class Op:
    def __init__(self):
        assert os.path.exists(TREE_SO), f"{TREE_SO} missing: make -C tests/userop -f tree_op.mk (__graft_entry__.build())"
        self.lib = ctypes.CDLL(TREE_SO)
        self.lib.chr_test_counters.argtypes = [ctypes.POINTER(ctypes.c_long)]
        self.lib.chr_test_counters.restype = None
        self.lib.chr_test_counters_reset.restype = None
        fold = ctypes.cast(self.lib.chr_test_halfadd, ctypes.c_void_p).value
        self.tree = ca.op_create(fold, tree=ctypes.cast(self.lib.chr_test_halfadd_tree, ctypes.c_void_p).value)
        self.decline = ca.op_create(fold, tree=ctypes.cast(self.lib.chr_test_decline_tree, ctypes.c_void_p).value)

    def reset(self):
        self.lib.chr_test_counters_reset()

    def counters(self):
        """(fold-launcher calls, tree-launcher calls, trees handed over, the last wg_per_cu)"""
        c = (ctypes.c_long * 4)()
        self.lib.chr_test_counters(c)
        return tuple(c)


@pytest.fixture(scope="module")
def op():
    o = Op()
    yield o
    assert ca.op_free(o.tree) == 0 and ca.op_free(o.decline) == 0


@pytest.fixture(scope="module")
def groups():
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = ca.LocalGroup(n, 0)
        return cache[n]

    yield get
    for g in cache.values():
        g.destroy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _programs():
    rng = np.random.default_rng(71)
    return [C4_TREE, SWAP_TREE] + [random_program(rng, nl) for nl in (2, 3, 5, 6, 7, 8)]


PROGS = _programs()


# ---- the tree API -------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "f64", "i32"])
def test_tree_api_every_path(gu, op, dt):
    """chr_reduce_tree with a tree op: n = 1 and 3 (elements only; 3 is below one f32 / i32 vector), 4099 (a partial
    trip and a tail), 65537 and 300001 (many trips, a partial one and a tail), out of place, into leaf 0 and into the
    last leaf: one tree-launcher call each, no fold call."""
    cdt, npdt = DT[dt]
    es = np.dtype(npdt).itemsize
    for comb, swaps in PROGS:
        nl = len(comb)
        for n in (1, 3, 4099, 65537, 300001):
            leaves = [po.fill(n, dt, po.PAT_UNIFORM, 13 + nl, r) for r in range(nl)]
            want = tree_ref(leaves, comb, swaps, dt, OPN)
            d = [gu.to_dev(x) for x in leaves]
            for into in (None, 0, nl - 1):
                out = gu.empty_dev(n * es) if into is None else d[into].clone()
                lv = list(d)
                if into is not None:
                    lv[into] = out
                op.reset()
                assert ca.reduce_tree(out, lv, comb, swaps, n, cdt, op.tree, gu.stream()) == 0
                gu.sync()
                assert op.counters()[:3] == (0, 1, 1), (comb, n, into, op.counters())
                np.testing.assert_array_equal(_bits(gu.from_dev(out, npdt, n)), _bits(want),
                                              err_msg=f"{dt} {comb} {swaps} n={n} into={into}")


@pytest.mark.parametrize("dt", ["f32", "f64", "i32"])
def test_tree_api_misaligned(gu, op, dt):
    """One leaf, and separately `out`, one element off 16-byte alignment: the whole tree runs element-wise -- at
    n = 257, and at 300001, where a lane takes more than one element (above 4096 workgroups of 64 lanes)."""
    cdt, npdt = DT[dt]
    es = np.dtype(npdt).itemsize
    for (comb, swaps), n in [(p, 257) for p in PROGS] + [(C4_TREE, 300001), (SWAP_TREE, 300001)]:
        nl = len(comb)
        leaves = [po.fill(n, dt, po.PAT_UNIFORM, 29 + nl, r) for r in range(nl)]
        want = tree_ref(leaves, comb, swaps, dt, OPN)
        d = [gu.to_dev(x) for x in leaves]
        for which in ("leaf", "out"):
            lv = list(d)
            out = gu.empty_dev(n * es)
            if which == "leaf":
                j = nl // 2
                shifted = gu.empty_dev((n + 1) * es)[es:]
                shifted.copy_(d[j])
                lv[j] = shifted
            else:
                out = gu.empty_dev((n + 1) * es)[es:]
            assert (lv[nl // 2].data_ptr() % 16 != 0) == (which == "leaf") and (out.data_ptr() % 16 != 0) == (which == "out")
            op.reset()
            assert ca.reduce_tree(out, lv, comb, swaps, n, cdt, op.tree, gu.stream()) == 0
            gu.sync()
            assert op.counters()[:3] == (0, 1, 1)
            np.testing.assert_array_equal(_bits(gu.from_dev(out, npdt, n)), _bits(want), err_msg=f"{dt} {comb} {which}")


def test_one_leaf_tree_calls_no_launcher(gu, op):
    n = 4099
    x = po.fill(n, "f32", po.PAT_UNIFORM, 3, 0)
    d, out = gu.to_dev(x), gu.empty_dev(n * 4)
    op.reset()
    assert ca.reduce_tree(out, [d], [0], [], n, ca.FLOAT32, op.tree, gu.stream()) == 0
    gu.sync()
    assert op.counters()[:3] == (0, 0, 0)
    np.testing.assert_array_equal(_bits(gu.from_dev(out, np.float32, n)), _bits(x))


def test_tree_batch_is_one_launcher_call(gu, op):
    rng = np.random.default_rng(9)
    n, nt, nl = 4099, 5, 6
    progs = [random_program(rng, nl) for _ in range(nt)]
    leaves = [[po.fill(n, "f32", po.PAT_UNIFORM, 40 + t, r) for r in range(nl)] for t in range(nt)]
    d_leaves = [[gu.to_dev(x) for x in lv] for lv in leaves]
    outs = [gu.empty_dev(n * 4) for _ in range(nt)]
    op.reset()
    assert ca.reduce_tree_batch(outs, d_leaves, [c for c, _ in progs], [s for _, s in progs], n, ca.FLOAT32, op.tree,
                                gu.stream()) == 0
    gu.sync()
    assert op.counters()[:3] == (0, 1, nt)
    for t, (comb, swaps) in enumerate(progs):
        np.testing.assert_array_equal(_bits(gu.from_dev(outs[t], np.float32, n)),
                                      _bits(tree_ref(leaves[t], comb, swaps, "f32", OPN)), err_msg=f"tree {t}")


# ---- the fallback -------------------------------------------------------------------------------

def test_declined_tree_falls_back_to_the_folds(gu, op):
    """A tree launcher that declines enqueues nothing: the same C4 tree fold by fold (three fold-launcher calls), the
    same bits.  A type neither launcher implements is the fold launcher's verdict, CHR_ERR_UNSUPPORTED."""
    comb, swaps = C4_TREE
    n = 65537
    leaves = [po.fill(n, "f32", po.PAT_UNIFORM, 13, r) for r in range(8)]
    want = tree_ref(leaves, comb, swaps, "f32", OPN)
    d = [gu.to_dev(x) for x in leaves]
    got = {}
    for name, code in (("tree", op.tree), ("decline", op.decline)):
        out = gu.empty_dev(n * 4)
        op.reset()
        assert ca.reduce_tree(out, d, comb, swaps, n, ca.FLOAT32, code, gu.stream()) == 0
        gu.sync()
        got[name] = (gu.from_dev(out, np.float32, n).copy(), op.counters()[:3])
    assert got["tree"][1] == (0, 1, 1) and got["decline"][1] == (3, 1, 1)
    np.testing.assert_array_equal(_bits(got["decline"][0]), _bits(want))
    np.testing.assert_array_equal(_bits(got["tree"][0]), _bits(got["decline"][0]))
    d64 = [gu.empty_dev(64 * 8) for _ in range(8)]
    op.reset()
    assert ca.reduce_tree(gu.empty_dev(64 * 8), d64, comb, swaps, 64, ca.INT64, op.tree, gu.stream()) == ca.ERR_UNSUPPORTED
    gu.sync()
    c = op.counters()
    assert c[1] == 1 and c[0] >= 1  # the tree launcher declined the type, then the fold launcher refused it


# ---- the residency cap ---------------------------------------------------------------------------

def test_cap_changes_no_bit(gu, op):
    """The tree launcher called directly with wg_per_cu = 0 and 12 (the cap beside RCCL): identical bits."""
    comb, swaps = C4_TREE
    n = 65537
    leaves = [po.fill(n, "f32", po.PAT_UNIFORM, 19, r) for r in range(8)]
    want = tree_ref(leaves, comb, swaps, "f32", OPN)
    d = [gu.to_dev(x) for x in leaves]
    fn = op.lib.chr_test_halfadd_tree
    fn.argtypes = [ctypes.POINTER(UserTree), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    for cap in (0, 12):
        out = gu.empty_dev(n * 4)
        t = UserTree()
        t.out = out.data_ptr()
        for j in range(8):
            t.leaves[j] = d[j].data_ptr()
            t.comb[j] = comb[j]
        for c in range(7):
            t.swaps[c] = swaps[c]
        t.nleaves, t.n = 8, n
        op.reset()
        assert fn(ctypes.byref(t), 1, ca.FLOAT32, cap, gu.stream().cuda_stream, None) == 0
        gu.sync()
        assert op.counters() == (0, 1, 1, cap)
        np.testing.assert_array_equal(_bits(gu.from_dev(out, np.float32, n)), _bits(want), err_msg=f"cap {cap}")


# ---- the collectives vs the reference -------------------------------------------------------------

def test_collectives_match_reference_golden_one_pass(gu, op, groups):
    """Every user-op golden case of the reference under the flat schedule, the op registered with its tree launcher:
    byte-equal to the reference's outputs.  Around one n = 8, k = 4, b = 4 allreduce, whose every reduction is an
    8-leaf tree, the counters show tree calls and no fold call."""
    bad = []
    probed = 0
    for c in MAN["cases"]:
        g = groups(c["n"])
        g.set_schedule(ca.SCHEDULE_FLAT)
        probe = (c["mode"], c["n"], c["k"], c["b"]) == ("ar", 8, 4, 4)
        op.reset()
        got = _run_case(gu, g, c, op.tree)
        if probe:
            folds, tree_calls, trees, _ = op.counters()
            assert tree_calls >= 1 and trees >= tree_calls and folds == 0, (c["id"], op.counters())
            probed += 1
        if got.dtype != FIX[c["id"]].dtype or not np.array_equal(got.view(np.uint8), FIX[c["id"]].view(np.uint8)):
            bad.append(c["id"])
    assert probed >= 1
    assert not bad, f"{len(bad)} device/reference mismatches, e.g. {bad[:5]}"


@pytest.mark.parametrize("n,k,b,slices", [(8, 4, 4, 1), (8, 2, 8, 4), (6, 3, 2, 2)])
def test_collectives_sliced_at_size_vs_oracle(gu, op, groups, n, k, b, slices):
    """MiB-sized buckets, sliced plans (a batch of trees per pipeline slice): bit-exact vs the oracle."""
    count = n * ((1 << 17) + 5)
    sends = [po.fill(count, "f32", po.PAT_UNIFORM, 17, r) for r in range(n)]
    g = groups(n)
    g.set_slices(slices)
    try:
        d_send = [gu.to_dev(s) for s in sends]
        d_recv = [gu.empty_dev(count * 4) for _ in range(n)]
        op.reset()
        assert g.all_reduce_radix_batch(d_send, d_recv, count, ca.FLOAT32, op.tree, k, b) == 0
        want = po.allreduce_radix_batch(sends, k, b, "f32", OPN)
        for r in range(n):
            np.testing.assert_array_equal(_bits(gu.from_dev(d_recv[r], np.float32, count)), _bits(want[r]))
        assert op.counters()[1] >= 1
    finally:
        g.set_slices(1)
