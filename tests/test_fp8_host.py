"""libchiara_fp8.so on the host: registration (include/chiara_fp8.h, chiara_amd/fp8.py), the kernels' resources read
from the code object, the reference (tests/fp8_ref.py) against torch's float8 casts over the whole operand domain, and
the self-check of the FP8 plan evaluator.  No GPU."""
import ctypes
import os
import re
import sys
import threading

import numpy as np
import pytest
import torch

import chiara_amd as ca
import fp8_ref
from chiara_amd import fp8

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import kernel_resources as kr  # noqa: E402

KINDS = (ca.SUM, ca.PROD, ca.MAX, ca.MIN)
FORMATS = (fp8.E4M3, fp8.E5M2)
POLICIES = (fp8.IEEE, fp8.SATURATE)
RCCL_ROOM_VGPRS = 72  # tests/test_kernel_resources.py: what a wave may hold beside RCCL's
TORCH_F8 = {fp8_ref.E4M3: torch.float8_e4m3fn, fp8_ref.E5M2: torch.float8_e5m2}


@pytest.fixture(autouse=True)
def released():
    yield
    assert fp8.release() == 0


def _all_codes():
    return [fp8.fp8_op(f, k, o) for f in FORMATS for k in KINDS for o in POLICIES]


# ---- registration ---------------------------------------------------------------------------------------------

def _any_launcher():
    return ctypes.cast(fp8.fp8_lib().chr_fp8_e4m3_sum_ieee_fold, ctypes.c_void_p).value


def test_loading_registers_nothing_and_codes_are_stable():
    """Loading takes no code; the first call per combination registers one of 64..127, later calls return it; MAX and
    MIN have one code for both policies, so 12 codes in all."""
    fp8.fp8_lib()
    probe = [ca.op_create(_any_launcher()) for _ in range(64)]  # all 64 codes still free after the load
    for p in probe:
        assert ca.op_free(p) == 0
    codes = _all_codes()
    assert len(set(codes)) == 12 and all(64 <= c <= 127 for c in codes), codes
    assert _all_codes() == codes
    for f in FORMATS:
        for k in (ca.MAX, ca.MIN):
            assert fp8.fp8_op(f, k, fp8.IEEE) == fp8.fp8_op(f, k, fp8.SATURATE)
        for k in (ca.SUM, ca.PROD):
            assert fp8.fp8_op(f, k, fp8.IEEE) != fp8.fp8_op(f, k, fp8.SATURATE)
        assert fp8.fp8_op(f, ca.SUM) == fp8.fp8_op(f, ca.SUM, fp8.IEEE)  # the default policy
    assert fp8.F8_DTYPE == ca.UINT8 and ca.DTYPE_SIZE[fp8.F8_DTYPE] == 1


def test_bad_arguments_are_refused():
    L = fp8.fp8_lib()
    op = ctypes.c_int(-1)
    for kind in (ca.LAND, ca.BXOR, ca.MAXLOC, 64, -1):
        assert L.chr_fp8_op(fp8.E4M3, kind, fp8.IEEE, ctypes.byref(op)) == ca.ERR_UNSUPPORTED and op.value == -1
        with pytest.raises(ca.ChiaraError):
            fp8.fp8_op(fp8.E4M3, kind)
    for fmt in (2, -1, 64):
        assert L.chr_fp8_op(fmt, ca.SUM, fp8.IEEE, ctypes.byref(op)) == ca.ERR_UNSUPPORTED and op.value == -1
    for o in (2, -1):
        assert L.chr_fp8_op(fp8.E5M2, ca.SUM, o, ctypes.byref(op)) == ca.ERR_UNSUPPORTED and op.value == -1
        assert L.chr_fp8_op(fp8.E5M2, ca.MAX, o, ctypes.byref(op)) == ca.ERR_UNSUPPORTED and op.value == -1
    assert L.chr_fp8_op(fp8.E4M3, ca.SUM, fp8.IEEE, None) == ca.ERR_INVALID_ARG
    probe = [ca.op_create(_any_launcher()) for _ in range(64)]  # the refused calls registered nothing
    for p in probe:
        assert ca.op_free(p) == 0


def test_release_returns_the_codes():
    """After release the codes are dead (chr_op_free: CHR_ERR_INVALID_ARG), all 64 can be created again, and a later
    fp8_op registers again."""
    codes = set(_all_codes())
    assert fp8.release() == 0
    for c in codes:
        assert ca.op_free(c) == ca.ERR_INVALID_ARG
    fresh = []
    try:
        for _ in range(64):
            fresh.append(ca.op_create(_any_launcher()))
        assert sorted(fresh) == list(range(64, 128))
        with pytest.raises(ca.ChiaraError) as e:  # a full registry: the registry's own error
            fp8.fp8_op(fp8.E4M3, ca.SUM)
        assert e.value.code == ca.ERR_UNSUPPORTED
    finally:
        for c in fresh:
            assert ca.op_free(c) == 0
    again = fp8.fp8_op(fp8.E5M2, ca.MAX)
    assert 64 <= again <= 127 and fp8.fp8_op(fp8.E5M2, ca.MAX, fp8.SATURATE) == again
    assert fp8.release() == 0 and fp8.release() == 0  # nothing held: still success


def test_first_call_is_thread_safe():
    got, gate = [], threading.Barrier(8)

    def work():
        gate.wait()
        got.append(tuple(_all_codes()))

    ts = [threading.Thread(target=work) for _ in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert len(got) == 8 and len(set(got)) == 1 and len(set(got[0])) == 12, got


def test_stats_round_trip():
    assert fp8.stats(reset=True) is not None
    assert fp8.stats() == (0, 0, 0)


# ---- resources --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def res():
    if not os.path.exists(kr.READELF):  # as tests/test_user_tree_resources.py
        pytest.skip("llvm-readelf not in this image")
    assert os.path.exists(fp8.FP8_LIB_PATH), f"{fp8.FP8_LIB_PATH} missing: __graft_entry__.build()"
    return kr.kernel_resources(fp8.FP8_LIB_PATH)


def test_kernel_set_and_resources(res):
    """12 k_fold and 12 x 7 k_tree<unsigned char, F, NL = 2..8, U = 4 / 2 / 1, 64>, 8 k_quantize<float | bf16 bits,
    format, policy> and 4 k_dequantize<float | bf16 bits, format>; no private segment, no static LDS, every kernel
    within the registers a wave has beside RCCL."""
    folds, trees, casts = {}, {}, set()
    for name, r in res.items():
        m = re.search(r"6k_foldIhN7chr_fp8\d+([A-Za-z]+)I((?:Li\d+E)+)EEEEv", name)
        if m:
            folds[(m.group(1), m.group(2))] = r
        m = re.search(r"6k_treeIhN7chr_fp8\d+([A-Za-z]+)I((?:Li\d+E)+)EELi(\d+)ELi(\d+)ELi64EEEv", name)
        if m:
            trees[(m.group(1), m.group(2), int(m.group(3)), int(m.group(4)))] = r
        m = re.search(r"N7chr_fp8\d+(k_quantize|k_dequantize)I([ft])((?:Li\d+E)+)EEv", name)
        if m:
            casts.add(m.groups())
    functors = {(f, f"Li{fmt}ELi{o}E") for f in ("Sum", "Prod") for fmt in (0, 1) for o in (0, 1)}
    functors |= {(f, f"Li{fmt}E") for f in ("Max", "Min") for fmt in (0, 1)}
    assert len(functors) == 12 and set(folds) == functors, sorted(res)
    u = {2: 4, 3: 2, 4: 2, 5: 1, 6: 1, 7: 1, 8: 1}
    assert set(trees) == {f + (nl, u[nl]) for f in functors for nl in range(2, 9)}, sorted(trees)
    want_casts = {("k_quantize", s, f"Li{fmt}ELi{o}E") for s in "ft" for fmt in (0, 1) for o in (0, 1)}
    want_casts |= {("k_dequantize", d, f"Li{fmt}E") for d in "ft" for fmt in (0, 1)}
    assert casts == want_casts, sorted(casts)
    assert len(res) == 12 + 12 * 7 + 8 + 4, sorted(res)
    for name, r in res.items():
        assert r["scratch"] == 0, f"{name}: a private segment of {r['scratch']} bytes"
        assert r["lds"] == 0, f"{name}: {r['lds']} bytes of static LDS"
        assert kr.alloc_vgprs(r) <= RCCL_ROOM_VGPRS, f"{name}: {kr.alloc_vgprs(r)} VGPRs"


# ---- the reference against torch ---------------------------------------------------------------------------------

def _torch_encode(fmt, overflow, r):
    """torch's cast of the f32 tensor r, after a clamp for SATURATE, NaNs canonicalised: codes as a uint8 array."""
    if overflow == fp8_ref.SATURATE:
        r = torch.clamp(r, -fp8_ref.MAX_VALUE[fmt], fp8_ref.MAX_VALUE[fmt])  # propagates NaN
    q = r.to(TORCH_F8[fmt])
    codes = q.view(torch.uint8).numpy().copy()
    codes[torch.isnan(q.to(torch.float32)).numpy()] = fp8_ref.CANONICAL_NAN[fmt]
    return codes


@pytest.mark.parametrize("fmt", sorted(fp8_ref.FORMATS))
def test_decode_table_is_torchs(fmt):
    f = fp8_ref.FORMATS[fmt]
    want = torch.arange(256, dtype=torch.uint8).view(TORCH_F8[f]).to(torch.float64).numpy()
    np.testing.assert_array_equal(fp8_ref.TABLE[f].view(np.uint64)[~np.isnan(want)], want.view(np.uint64)[~np.isnan(want)])
    np.testing.assert_array_equal(np.isnan(fp8_ref.TABLE[f]), np.isnan(want))


@pytest.mark.parametrize("policy", sorted(fp8_ref.POLICIES))
@pytest.mark.parametrize("op", ["sum", "prod"])
@pytest.mark.parametrize("fmt", sorted(fp8_ref.FORMATS))
def test_combine_against_torch_on_every_pair(fmt, op, policy):
    """All 65 536 (in, inout) pairs: float64 plus the nearest-even table search agrees with torch's f32 operation, a
    clamp for SATURATE and the float8 cast."""
    f, o = fp8_ref.FORMATS[fmt], fp8_ref.POLICIES[policy]
    x = np.repeat(np.arange(256, dtype=np.uint8), 256)
    y = np.tile(np.arange(256, dtype=np.uint8), 256)
    xf = torch.from_numpy(x).view(TORCH_F8[f]).to(torch.float32)
    yf = torch.from_numpy(y).view(TORCH_F8[f]).to(torch.float32)
    want = _torch_encode(f, o, yf + xf if op == "sum" else yf * xf)
    got = fp8_ref.combine(f, op, o, x, y)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(x[i]), hex(y[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]


def test_reference_hand_values():
    """A few hand-checked values of each op, so that the reference itself is pinned."""
    E4, E5, I, S = fp8_ref.E4M3, fp8_ref.E5M2, fp8_ref.IEEE, fp8_ref.SATURATE

    def c(fmt, op, o, x, y):
        return int(fp8_ref.combine(fmt, op, o, np.array([x], np.uint8), np.array([y], np.uint8))[0])

    def e(fmt, o, v):
        return int(fp8_ref.encode(fmt, o, np.array([v]))[0])

    # the four overflow cases: 448 + 16 and 448 + 32 (E4M3), 57344 + 4096 (E5M2: the tie's even side is up)
    assert fp8_ref.TABLE[E4][0x7E] == 448 and fp8_ref.TABLE[E4][0x58] == 16 and fp8_ref.TABLE[E4][0x60] == 32
    assert c(E4, "sum", I, 0x58, 0x7E) == 0x7E and c(E4, "sum", S, 0x58, 0x7E) == 0x7E
    assert c(E4, "sum", I, 0x60, 0x7E) == 0x7F and c(E4, "sum", S, 0x60, 0x7E) == 0x7E
    assert c(E4, "sum", I, 0xE0, 0xFE) == 0x7F and c(E4, "sum", S, 0xE0, 0xFE) == 0xFE  # the NaN is positive
    assert fp8_ref.TABLE[E5][0x7B] == 57344 and fp8_ref.TABLE[E5][0x6C] == 4096
    assert c(E5, "sum", I, 0x6C, 0x7B) == 0x7C and c(E5, "sum", S, 0x6C, 0x7B) == 0x7B
    assert c(E5, "sum", I, 0xEC, 0xFB) == 0xFC and c(E5, "sum", S, 0xEC, 0xFB) == 0xFB
    assert e(E4, I, 464.0) == 0x7E and e(E4, I, np.nextafter(464.0, 500.0)) == 0x7F
    assert e(E5, I, np.nextafter(61440.0, 0.0)) == 0x7B and e(E5, I, 61440.0) == 0x7C
    # saturation of infinities; NaN sources stay NaN
    assert c(E5, "sum", S, 0x7C, 0x3C) == 0x7B and c(E5, "sum", S, 0xFC, 0x3C) == 0xFB
    assert c(E5, "sum", S, 0x7C, 0xFC) == 0x7E and c(E5, "prod", S, 0x00, 0x7C) == 0x7E
    assert c(E5, "sum", I, 0xFF, 0x3C) == 0x7E and c(E4, "prod", S, 0xFF, 0x38) == 0x7F
    # subnormals kept; 1 + 1; signed zeros
    for fmt, one in ((E4, 0x38), (E5, 0x3C)):
        assert c(fmt, "sum", I, 0x01, 0x01) == 0x02
        assert c(fmt, "sum", I, one, one) == 0x40
        assert c(fmt, "sum", I, 0x80, 0x80) == 0x80 and c(fmt, "sum", I, 0x80, 0x00) == 0x00
        assert c(fmt, "sum", I, one, one | 0x80) == 0x00
        assert c(fmt, "prod", I, 0x81, 0x81) == 0x00 and c(fmt, "prod", I, 0x81, 0x01) == 0x80  # underflow keeps the sign
        # MAX / MIN: a tie returns `in`, an unordered compare returns `in`, the byte passes through
        assert c(fmt, "max", I, 0x00, 0x80) == 0x00 and c(fmt, "max", I, 0x80, 0x00) == 0x80
        assert c(fmt, "max", I, 0xFF, one) == 0xFF and c(fmt, "max", I, one, 0xFF) == one
        assert c(fmt, "min", I, 0x7F, one) == 0x7F and c(fmt, "min", I, one, 0x7F) == one
        assert c(fmt, "max", I, one, 0x40) == 0x40 and c(fmt, "min", I, one, 0x40) == one


@pytest.mark.parametrize("policy", sorted(fp8_ref.POLICIES))
@pytest.mark.parametrize("fmt", sorted(fp8_ref.FORMATS))
def test_quantize_ref_against_torch(fmt, policy):
    """quantize_ref against torch's f32 multiply and float8 cast: 64 Ki random f32 bit patterns and every bf16 value,
    at a few scales."""
    f, o = fp8_ref.FORMATS[fmt], fp8_ref.POLICIES[policy]
    rng = np.random.default_rng(88)
    src = np.concatenate([rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32).view(np.float32),
                          fp8_ref.bf16_to_f32(np.arange(1 << 16, dtype=np.uint16))])
    for scale in (1.0, 0.5, 3.0, float(np.float32(1) / np.float32(3)), 2.0 ** -120, 2.0 ** 100):
        want = _torch_encode(f, o, torch.from_numpy(src) * torch.tensor(scale, dtype=torch.float32))
        got = fp8_ref.quantize_ref(f, o, src, scale)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (scale, [(hex(src.view(np.uint32)[i]), hex(got[i]), hex(want[i])) for i in bad[:8]])


def test_dequantize_ref_values():
    E4, E5 = fp8_ref.E4M3, fp8_ref.E5M2
    codes = np.arange(256, dtype=np.uint8)
    for fmt in (E4, E5):
        f32 = fp8_ref.dequantize_ref(fmt, codes, 1.0)
        want = torch.from_numpy(codes).view(TORCH_F8[fmt]).to(torch.float32)
        keep = ~torch.isnan(want).numpy()
        np.testing.assert_array_equal(f32[keep], want.numpy().view(np.uint32)[keep])
        assert (f32[~keep] == 0x7FC00000).all()
        b = fp8_ref.dequantize_ref(fmt, codes, 1.0, bf16=True)  # every code is exact in bf16
        np.testing.assert_array_equal(b[keep], (f32[keep] >> 16).astype(np.uint16))
        assert (b[~keep] == 0x7FC0).all()
        third = fp8_ref.dequantize_ref(fmt, codes, float(np.float32(1) / np.float32(3)), bf16=True)
        t = want * (torch.tensor(1.0) / torch.tensor(3.0))
        np.testing.assert_array_equal(third[keep], t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)[keep])
    assert fp8_ref.dequantize_ref(E5, np.array([0x7C], np.uint8), 0.0)[0] == 0x7FC00000  # inf * 0


# ---- the plan evaluator ------------------------------------------------------------------------------------------

def _is_one_rank_order_fold(n, k, b, count):
    """Whether the REFERENCE plans hold a single reduction over all n ranks' inputs in rank order: then the reference
    order IS the plain left fold.  Read from the plans, not from the geometry (as tests/test_f16_ops_host.py)."""
    import plan_sim

    plans = plan_sim.load_plans(ca.MODE_ALLREDUCE, n, k, b, count, schedule=ca.SCHEDULE_REFERENCE)
    reds = [op for p in plans for st in [{"post": p["pre"]}] + p["steps"] for op in st["post"]
            if op[0] in ("reduce", "reduce_sw", "tree") and op[4]]
    if len(reds) != 1 or reds[0][0] != "reduce" or len(reds[0][4]) != n - 1:
        return False
    offs = [off for _, off in reds[0][4]]
    return offs == sorted(offs)  # STAGE slots in the order the peers 1..n-1 were received


@pytest.mark.parametrize("fmt", sorted(fp8_ref.FORMATS))
@pytest.mark.parametrize("n,k,b", [(8, 4, 4), (8, 2, 2), (6, 4, 6), (4, 4, 4)])
def test_plan_evaluator_self_check(n, k, b, fmt):
    """REFERENCE, FLAT, FLAT_1SHOT and EXACT plans give identical codes under SUM on U[-1, 1), and those codes differ
    from a plain rank-order left fold somewhere: the data can tell orders apart.

    At (4, 4, 4) the reference's order is itself the rank-order left fold (the REFERENCE plan says so,
    _is_one_rank_order_fold), so no data can differ from it there.  That geometry is held to the stronger statement,
    equality with the left fold, and the data's power to tell orders apart is shown against the pairwise order
    (s0 + s1) + (s2 + s3) instead -- as tests/test_f16_ops_host.py handles it."""
    f = fp8_ref.FORMATS[fmt]
    ref = fp8_ref.Ref(f, "sum", fp8_ref.IEEE)
    count = n * 257
    sends = [fp8_ref.uniform(f, count, 31, r) for r in range(n)]
    want = ref.expected(ca.MODE_ALLREDUCE, sends, k, b, ca.SCHEDULE_REFERENCE)
    for sch in (ca.SCHEDULE_FLAT, ca.SCHEDULE_FLAT_1SHOT, ca.SCHEDULE_EXACT):
        got = ref.expected(ca.MODE_ALLREDUCE, sends, k, b, sch)
        for r in range(n):
            np.testing.assert_array_equal(got[r], want[r], err_msg=f"schedule {sch} rank {r}")
    for r in range(1, n):
        np.testing.assert_array_equal(want[r], want[0])
    assert want[0].dtype == np.uint8 and want[0].size == count
    left = ref.left_fold(sends)
    if _is_one_rank_order_fold(n, k, b, count):
        np.testing.assert_array_equal(want[0], left)
        pairs = [ref.combine(sends[i], sends[i + 1]) for i in range(0, n, 2)]
        assert np.count_nonzero(want[0] != ref.left_fold(pairs)) >= 1
    else:
        assert np.count_nonzero(want[0] != left) >= 1
