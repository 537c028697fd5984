"""The oracle's MPI_Reduce_local over the operand-domain tables (tests/domain_util.py) against a numpy restatement
written independently of it, bit for bit: the reference tests/test_gpu_operand_domain.py holds the kernels to is
itself pinned on subnormals, overflow, underflow, invalid operations, sign boundaries and every 8-bit operand pair.

The restatement's floating SUM / PROD is the host's own IEEE arithmetic (x86: a lone NaN comes back quieted, an invalid
operation gives the default NaN with the sign set, 0xFFC00000 / 0xFFF8000000000000, 0xFFC0 after the bf16 rounding).
One class of cells is left out, and only that one: SUM / PROD of two NaNs on f32 / f64 / bf16, where the payload that
survives depends on the operand order the host's compiler picked (tests/golden/nan_reduce_local.npz pins those on
MPICH's own results).  The class is counted and capped below."""
import numpy as np
import pytest

import domain_util as du
import pyoracle as po

ALL_OPS = du.ARITH + du.LOGIC + du.BITWISE + du.LOC
EXCLUDED_CAP = 1e-4  # 0.01 % of a table


def oracle(dtype, op):
    x, y = du.table(dtype)
    return po.reduce_local(x, y.view(np.uint8).copy().view(y.dtype), dtype, op)


def test_valid_ops_is_the_oracles_table():
    assert set(du.DTYPES) == set(po.DTYPES)
    for dtype in du.DTYPES:
        assert [op for op in ALL_OPS if po.valid(dtype, op)] == list(du.valid_ops(dtype)), dtype


@pytest.mark.parametrize("dtype", du.DTYPES)
def test_table_shape(dtype):
    x, y = du.table(dtype)
    npdt = np.dtype(po.NP_DTYPES[dtype])
    assert x.dtype == npdt and y.dtype == npdt and x.shape == y.shape and x.ndim == 1
    assert not x.flags.writeable and not y.flags.writeable
    want = {"i8": 1 << 16, "u8": 1 << 16, "i16": 1 << 22, "u16": 1 << 22, "bf16": 1 << 25, "f32": 1 << 22,
            "f64": 2064 ** 2, "cf": 1 << 20, "cd": 1 << 20, "fi": 320 ** 2, "di": 320 ** 2, "li": 320 ** 2,
            "2i": 320 ** 2, "si": 320 ** 2}.get(dtype)
    if want is None:  # the 32- and 64-bit integers: an edge set squared
        want = du.int_edges(8 * npdt.itemsize).size ** 2
        assert 128 ** 2 <= want <= 1024 ** 2
    assert x.size == want
    # every (in, inout) combination once: x is na distinct elements repeated nb times each, y nb distinct ones tiled
    cx, cy = [c.reshape(c.shape[0], -1) for c in (du.cells(x), du.cells(y))]
    nb = int(np.flatnonzero((cx[1:] != cx[:-1]).any(axis=1))[0]) + 1
    na = x.size // nb
    assert na * nb == x.size
    cx, cy = cx.reshape(na, nb, -1), cy.reshape(na, nb, -1)
    assert (cx == cx[:, :1]).all() and (cy == cy[:1]).all()
    assert np.unique(cx[:, 0], axis=0).shape[0] == na and np.unique(cy[0], axis=0).shape[0] == nb


@pytest.mark.parametrize("dtype", ["i8", "u16", "bf16", "si", "cd"])
def test_inout_major_order_lists_the_same_cells(dtype):
    """The second order the device tests run (neither operand is then constant along a vector in both): the same
    cells, and du.reorder carries a per-cell result from one order to the other."""
    (x, y), (xt, yt) = du.table(dtype), du.table(dtype, du.INOUT_MAJOR)
    a, b = du.operand_sets(dtype)
    assert np.array_equal(du.cells(du.reorder(x, dtype, du.INOUT_MAJOR)), du.cells(xt))
    assert np.array_equal(du.cells(du.reorder(y, dtype, du.INOUT_MAJOR)), du.cells(yt))
    assert np.array_equal(du.cells(xt[:a.size]), du.cells(a)) and (du.cells(yt[:a.size]) == du.cells(b[:1])).all()
    op = du.valid_ops(dtype)[0]
    direct = po.reduce_local(xt, yt.view(np.uint8).copy().view(yt.dtype), dtype, op)
    assert np.array_equal(du.cells(direct), du.cells(du.reorder(oracle(dtype, op), dtype, du.INOUT_MAJOR)))


def test_integer_tables_hold_the_sign_boundaries():
    for dtype in du.INTS:
        bits = 8 * np.dtype(po.NP_DTYPES[dtype]).itemsize
        x, y = du.table(dtype)
        for side in (x, y):
            have = set(int(v) for v in np.unique(du.cells(side)))
            top = 1 << (bits - 1)
            for v in (0, 1, 2, (1 << bits) - 1, top, top - 1, top + 1, 0xFF, 0x80):
                assert v in have, (dtype, hex(v))


def test_pair_tables_hold_their_edges():
    for dtype in du.PAIRS:
        x, y = du.table(dtype)
        assert set(int(i) for i in np.unique(x["i"])) == set(du.PAIR_INDICES) == set(int(i) for i in np.unique(y["i"]))
        assert np.unique(du.pair_values(dtype)).size == 64
        es = x.dtype.itemsize
        field = np.zeros(es, dtype=bool)
        for name in ("v", "i"):
            dt, off = x.dtype.fields[name][:2]
            field[off:off + dt.itemsize] = True
        px, py = x.view(np.uint8).reshape(-1, es)[:, ~field], y.view(np.uint8).reshape(-1, es)[:, ~field]
        assert px.shape[1] == {"fi": 0, "2i": 0, "di": 4, "li": 4, "si": 2}[dtype]
        if px.shape[1]:  # non-zero, per element, and not the same on either side
            assert px.all() and py.all() and np.unique(px, axis=0).shape[0] > 64 and (px != py).any(axis=1).mean() > 0.9
        if dtype in du.PART:
            c = du.fclass(du.pair_values(dtype), du.PART[dtype])
            assert c["nan"].sum() == 1 and c["sub"].sum() >= 4 and c["inf"].sum() == 2 and c["negzero"].sum() == 1


CASES = [(d, o) for d in du.DTYPES for o in du.valid_ops(d) if d not in du.PAIRS and (d not in du.CPLX or o == "sum")]


@pytest.mark.parametrize("dtype,op", CASES, ids=[f"{d}-{o}" for d, o in CASES])
def test_oracle_equals_numpy_restatement(dtype, op):
    x, y = du.table(dtype)
    want, undefined = du.np_reduce_local(x, y, dtype, op)
    keep = None
    if undefined is not None:
        fmt = du.PART.get(dtype, dtype)
        both_nan = du.fclass(du.fbits(x, fmt), fmt)["nan"] & du.fclass(du.fbits(y, fmt), fmt)["nan"]
        assert int(undefined.sum()) == int(both_nan.sum()), "only NaN x NaN cells may be left out"
        assert undefined.sum() < EXCLUDED_CAP * x.size, (int(undefined.sum()), x.size)
        if dtype == "f32":
            assert undefined.sum() == 36
        keep = ~undefined
    else:
        assert dtype not in du.FMT or op not in ("sum", "prod")
    du.assert_cells_equal(oracle(dtype, op), want, x, y, dtype, op, "oracle vs numpy", keep=keep)


FLOATING = [(d, o) for d in ("f32", "f64", "bf16", "cf", "cd") for o in ("sum", "prod")]


@pytest.mark.parametrize("dtype,op", FLOATING, ids=[f"{d}-{o}" for d, o in FLOATING])
def test_floating_tables_reach_the_edges_they_are_for(dtype, op):
    """A subnormal result, an infinity out of finite operands, a -0 and a default NaN out of non-NaN operands: a table
    shrunk by a later edit cannot lose them silently."""
    fmt = du.PART.get(dtype, dtype)
    x, y = du.table(dtype)
    parts = 2 if dtype in du.CPLX else 1
    r = du.fclass(du.fbits(oracle(dtype, op), fmt), fmt)
    cx, cy = du.fclass(du.fbits(x, fmt), fmt), du.fclass(du.fbits(y, fmt), fmt)

    def per_cell(c, key, how):  # a cell's operands: all / any of its parts
        return np.repeat(how(c[key].reshape(-1, parts), axis=1), parts)

    finite_in = per_cell(cx, "finite", np.all) & per_cell(cy, "finite", np.all)
    no_nan_in = ~per_cell(cx, "nan", np.any) & ~per_cell(cy, "nan", np.any)
    assert r["sub"].any(), "no subnormal result"
    assert (r["inf"] & finite_in).any(), "no overflow to +-inf out of finite operands"
    assert r["negzero"].any(), "no -0 result"
    assert (r["default_nan"] & no_nan_in).any(), "no invalid operation"
    if dtype in ("bf16", "f32", "f64"):  # the counts the tables were sized by
        counts = (int(r["sub"].sum()), int((r["default_nan"] & no_nan_in).sum()))
        print(dtype, op, "subnormal results, invalid operations:", counts, "inf results:", int(r["inf"].sum()))
        if dtype == "bf16":
            assert counts == {"sum": (1750, 2), "prod": (504816, 8)}[op]
        if dtype == "f32":
            assert counts[0] == {"sum": 378, "prod": 176140}[op]
        if dtype == "f64":
            assert counts[0] == {"sum": 726, "prod": 252416}[op]


def test_bf16_table_rounds_to_inf_and_to_subnormals():
    """Results the packed RNE convert must round to +-inf (finite in f32) and to a subnormal."""
    x, y = du.table("bf16")
    fx = (x.astype(np.uint32) << np.uint32(16)).view(np.float32)
    fy = (y.astype(np.uint32) << np.uint32(16)).view(np.float32)
    with np.errstate(all="ignore"):
        wide_sum, wide_prod = fy + fx, fy * fx
    # the partners are powers of two, so a product is exact until it is subnormal and a subnormal sum is exact:
    # SUM has the roundings to inf, PROD the inexact roundings to a subnormal
    assert (np.isfinite(wide_sum) & du.fclass(oracle("bf16", "sum"), "bf16")["inf"]).any()
    inexact = (wide_prod.view(np.uint32) & np.uint32(0xFFFF)) != 0
    assert (inexact & du.fclass(oracle("bf16", "prod"), "bf16")["sub"]).any()


def test_mismatch_report_names_the_cells():
    x, y = du.table("i8")
    want = oracle("i8", "max")
    got = want.copy()
    got[[5, 70000 % got.size, 300]] ^= 1
    with pytest.raises(AssertionError) as e:
        du.assert_cells_equal(got, want, x, y, "i8", "max", "some path")
    msg = str(e.value)
    assert msg.startswith("i8 max some path: 3 of 65536 cells wrong") and "(in, inout, got, want)" in msg
    assert f"[5] (0x{int(x.view(np.uint8)[5]):02x}, 0x{int(y.view(np.uint8)[5]):02x}, " in msg
    xs, ys = du.table("di")
    w = oracle("di", "maxloc")
    g = w.view(np.uint8).copy()
    g[16 * 7 + 12] ^= 0xFF  # a padding byte
    with pytest.raises(AssertionError) as e:
        du.assert_cells_equal(g.view(w.dtype), w, xs, ys, "di", "maxloc", "p")
    assert "di maxloc p: 1 of 102400 cells wrong" in str(e.value) and "[7] (bytes:" in str(e.value)
