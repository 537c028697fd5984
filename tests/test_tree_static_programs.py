"""Host-side pins of the streaming sweep (tests/streaming_cases.py, tests/test_gpu_streaming_sweep.py; no GPU):
the sweep's table of compile-time programs is csrc/reduce_tree.hpp's, its inputs make every swapped combine of an
order-sensitive op visible, and its case list covers the whole (type, op) table at every fan-in and leaf count."""
import os
import re

import numpy as np
import pytest

import chiara_amd as ca
import pyoracle as po
import streaming_cases as sc
from test_gpu_dispatch_sweep import CPLX, FLOATS, PAIRS
from test_gpu_kernels import DT, OP, _bits
from test_tree_program import _call
from tree_util import all_programs, tree_ref

HEADER = os.path.join(sc.REPO, "configurable-hierarchical-allreduce-algorithms_amd", "csrc", "reduce_tree.hpp")


def header_programs():
    """{NL: [comb]} from the tree_prog({c0, ..., c7}, NL) initialisers of StaticProgs<NL>."""
    with open(HEADER) as f:
        text = f.read()
    out = {}
    for spec in re.finditer(r"template <> struct StaticProgs<(\d+)>\s*\{(.*?)\n\};", text, re.S):
        nl, body = int(spec.group(1)), spec.group(2)
        progs = []
        for m in re.finditer(r"tree_prog\(\{([^}]*)\},\s*(\d+)\)", body):
            comb = [int(c) for c in m.group(1).split(",")]
            assert int(m.group(2)) == nl and len(comb) == 8 and not any(comb[nl:]), (nl, comb)
            progs.append(comb[:nl])
        declared = int(re.search(r"int n = (\d+);", body).group(1))
        assert declared == len(progs), f"StaticProgs<{nl}>: n = {declared}, {len(progs)} initialisers"
        out[nl] = progs
    # every tree_prog initialiser of the header sits in one of the specialisations parsed above
    assert sum(len(p) for p in out.values()) == len(re.findall(r"tree_prog\(\{", text))
    return out


def test_sweep_table_is_the_headers():
    """Both directions: a program added to (or dropped from) the header without its row here fails, and so does a
    row the header does not unroll (the sweep would then call an interpreted program the unrolled body)."""
    hdr = header_programs()
    assert hdr, "no StaticProgs specialisation found"
    assert sorted(hdr) == sorted(sc.STATIC_PROGS)
    for nl in hdr:
        assert sorted(hdr[nl]) == sorted(sc.STATIC_PROGS[nl]), nl
        assert len(set(map(tuple, hdr[nl]))) == len(hdr[nl]), f"a program twice in StaticProgs<{nl}>"
    assert sum(len(p) for p in hdr.values()) == 9


@pytest.mark.parametrize("nl", sorted(sc.STATIC_PROGS))
def test_static_programs_are_valid(nl):
    for comb in sc.STATIC_PROGS[nl]:
        assert _call(comb, [0] * (nl - 1)) == 0, comb
        assert comb in all_programs(nl), comb


def test_every_program_count():
    assert [len(all_programs(nl)) for nl in sc.LEAF_COUNTS] == [1, 2, 5, 13, 34, 89, 233]
    for variant in sc.PROGRAM_VARIANTS:
        cases = sc.program_cases(variant)
        assert len(cases) == 377
        for c in cases[::37]:
            assert _call(c.comb, c.swaps) == 0
        assert any(any(c.swaps) for c in cases) == sc.PROGRAM_VARIANTS[variant][3]


def test_census():
    """Nothing drops out of the sweep silently: the case lists the children iterate, against the library's own
    (type, op) table (kernel_table.hpp valid_dtype_op, asked through the n = 0 call) and the oracle's."""
    table = [(d, o) for d in DT for o in OP if ca.reduce_local(0, 0, 0, DT[d], OP[o]) == 0]
    assert table == [(d, o) for d in DT for o in OP if po.valid(d, o)]
    plain = [(d, o) for d, o in table if d not in PAIRS + CPLX]
    assert len(plain) == 98 and plain == sc.SWEEP_PAIRS
    buckets = sc.bucket_cases()
    assert len(set(buckets)) == len(buckets)
    default = [c for c in buckets if not c.running_first and c.dtype in sc.SWEEP_DTYPES and
               c.pattern == sc.pattern_for(c.op)]
    assert {(c.dtype, c.op, c.m) for c in default} == {(d, o, m) for d, o in plain for m in range(1, 9)}
    for layout in "ab":
        assert sum(c.layout == layout for c in default) == 98 * 8
        assert sum(c.layout == layout and c.running_first for c in buckets) == 3 * 4 * 8
    assert all(c.pattern == po.PAT_TIES and c.dtype in FLOATS for c in buckets if c.running_first)
    on_ties = [c for c in buckets if not c.running_first and c.dtype in sc.SWEEP_DTYPES and c not in default]
    assert sorted(on_ties) == sorted(c._replace(pattern=po.PAT_TIES) for c in default
                                     if c.dtype in FLOATS and c.op in ("sum", "prod"))
    assert sorted((c.dtype, c.op) for c in buckets if c.dtype in PAIRS + CPLX) == \
        sorted((d, o) for d, o in table if d in PAIRS + CPLX)
    assert len(buckets) == 2 * 98 * 8 + 2 * 96 + 2 * 48 + 14
    trees = [c for d, o in sc.SWEEP_PAIRS for c in sc.tree_cases(d, o)]
    assert {(c.dtype, c.op, c.nl) for c in trees} == {(d, o, nl) for d, o in plain for nl in range(2, 9)}
    assert len({(c.dtype, c.op, c.nl) for c in trees}) == 98 * 7
    for d, o in plain:
        mine = [c for c in trees if (c.dtype, c.op) == (d, o)]
        on_data = [c for c in mine if c.pattern == sc.pattern_for(o)]
        for nl, progs in sc.STATIC_PROGS.items():
            for comb in progs:  # the unrolled body, and the same program swapped
                assert any(c.comb == comb and not any(c.swaps) and c.what == "static" for c in on_data)
                assert any(c.comb == comb and any(c.swaps) and c.what == "static swapped" for c in on_data)
            for what in ("static shifted", "static out = leaf 0", "static out = last leaf"):
                assert sum(c.nl == nl and c.what == what and c.comb == progs[0] for c in on_data) == 1
        for nl in range(3, 9):
            ns = [c for c in on_data if c.nl == nl and c.what == "non-static"]
            assert len(ns) == 1 and ns[0].comb not in sc.STATIC_PROGS.get(nl, [])
            assert any(ns[0].swaps) and _call(ns[0].comb, ns[0].swaps) == 0
        two = {(c.swaps[0], c.alias) for c in on_data if c.what == "two leaves"}
        assert two == {(s, a) for s in (0, 1) for a in (None, 0, 1)}
        assert sum(c.layout == "b" for c in on_data) == 3
        if sc.order_sensitive(d, o) and sc.pattern_for(o) != po.PAT_TIES:  # every case once more on TIES
            ties = [c for c in mine if c not in on_data]
            assert [c._replace(pattern=sc.pattern_for(o), what=c.what[:-5]) for c in ties] == on_data
        else:
            assert mine == on_data


ORDER_SENSITIVE = [(d, o) for d in FLOATS for o in sc.ARITH]


@pytest.mark.parametrize("dtype,op", ORDER_SENSITIVE)
def test_swapped_cases_show_the_order(dtype, op):
    """A condition on the sweep's inputs, checked with the oracle alone: for every leaf count, at least one swapped
    case on TIES data whose result differs bitwise from the same program unswapped.  Without it a kernel that
    ignored the swap bits (as the unrolled body does, by design, for commutative ops) would pass."""
    assert sc.order_sensitive(dtype, op)
    cases = [c for c in sc.tree_cases(dtype, op) if any(c.swaps)]
    assert all(c.pattern == po.PAT_TIES for c in cases if c.what.endswith("ties") or op in ("max", "min"))
    for nl in sc.LEAF_COUNTS:
        shown = 0
        for c in cases:
            if c.nl != nl or c.pattern != po.PAT_TIES:
                continue
            leaves = sc.operands_for(dtype, op, c.pattern)[:nl]
            plain = tree_ref(leaves, c.comb, [0] * (nl - 1), dtype, op)
            shown += not np.array_equal(_bits(sc.tree_case_ref(c)), _bits(plain))
        assert shown, (dtype, op, nl)


def test_running_first_buckets_show_the_order():
    for dtype, op in ORDER_SENSITIVE:
        for m in sc.FAN_INS:
            assert not np.array_equal(_bits(sc.bucket_ref(dtype, op, m, True, po.PAT_TIES)),
                                      _bits(sc.bucket_ref(dtype, op, m, False, po.PAT_TIES))), (dtype, op, m)


def test_every_program_swaps_show_the_order():
    """'f32 max ties swapped' and 'f32 max ties' are different checks: the swaps change result bits."""
    cases = sc.program_cases("f32 max ties swapped")
    for nl in sc.LEAF_COUNTS:
        leaves = sc.operands_for("f32", "max", po.PAT_TIES)[:nl]
        plain = [0] * (nl - 1)
        assert any(any(c.swaps) and not np.array_equal(_bits(tree_ref(leaves, c.comb, c.swaps, "f32", "max")),
                                                       _bits(tree_ref(leaves, c.comb, plain, "f32", "max")))
                   for c in [c for c in cases if c.nl == nl][:8]), nl


def test_layout_is_the_one_the_sweep_describes():
    """Whole 8-XCD groups of 4 KiB runs for U = 4, 2 and 1, whole trips past them, one partial trip, a scalar tail."""
    assert sc.NVEC == 4867
    for u in (4, 2, 1):
        per_trip = 64 * u
        trips = -(-sc.NVEC // per_trip)
        group = 8 * (4096 // (per_trip * 16))  # trips per 8-XCD group of 4 KiB runs
        assert trips // group >= 1 and (sc.NVEC // per_trip) % group > 0 and sc.NVEC % per_trip
    for dtype in sc.SWEEP_DTYPES:
        es = np.dtype(po.NP_DTYPES[dtype]).itemsize
        assert sc.count(dtype) * es == sc.NVEC * 16 + es
