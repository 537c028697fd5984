"""The guarded-buffer helper (tests/footprint_util.py) on CPU tensors: every check it offers can fail, and names
where.  One byte is flipped at each place a stray store could land -- either end of either guard, the middle of an
input's payload -- and must come back with its region, its offset from the payload's start and a count of one; an
untouched buffer reports nothing, at every phase and for an empty payload.  The guard size is re-derived from the
kernels' sources."""
import os
import re

import numpy as np
import pytest
import torch

from footprint_util import GUARD_BYTES, MAX_TRIP_BYTES, TRIP_SHAPES, Guarded, stream_guard

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "configurable-hierarchical-allreduce-algorithms_amd", "csrc")
CPU = torch.device("cpu")


def _mk(nbytes=1000, phase=0, lo=64, hi=96, key=7):
    g = Guarded(nbytes, phase, lo, hi, key, device=CPU)
    g.load(np.arange(nbytes, dtype=np.uint8))
    return g


@pytest.mark.parametrize("phase", [0, 1, 15])
@pytest.mark.parametrize("nbytes", [0, 1, 1000])
def test_untouched_buffer_reports_nothing(phase, nbytes):
    g = _mk(nbytes, phase)
    assert g.ptr % 16 == phase and g.payload().numel() == nbytes
    assert g.start >= 64 and g.buf.numel() - g.end >= 96  # the guards are at least what was asked for
    snap = g.snapshot()
    assert g.guards_intact() and g.guards_intact().diffs == []
    assert g.unchanged_since(snap) and g.unchanged_since(snap).diffs == []
    np.testing.assert_array_equal(g.read(np.uint8), np.arange(nbytes, dtype=np.uint8))


@pytest.mark.parametrize("phase", [0, 1, 15])
def test_a_flipped_byte_is_reported_where_it_is(phase):
    n = 1000
    places = {  # name -> (index in the allocation, region, offset from the payload's start)
        "the lower guard's last byte": lambda g: (g.start - 1, "lower", -1),
        "the lower guard's first byte": lambda g: (0, "lower", -g.start),
        "the upper guard's first byte": lambda g: (g.end, "upper", n),
        "the upper guard's last byte": lambda g: (g.buf.numel() - 1, "upper", g.buf.numel() - 1 - g.start),
    }
    for name, place in places.items():
        g = _mk(n, phase)
        snap = g.snapshot()
        i, region, off = place(g)
        g.buf[i] ^= 0x5A
        res = g.guards_intact()
        assert not res and res.diffs == [(region, off, 1)], (name, res)
        assert f"{off:+d}" in repr(res) and region in repr(res)
        since = g.unchanged_since(snap)
        assert not since and since.diffs == [(region, off, 1)], (name, since)
        np.testing.assert_array_equal(g.read(np.uint8), np.arange(n, dtype=np.uint8))  # the payload is not a guard


def test_a_clobbered_input_payload_is_reported():
    g = _mk(1000, 4)
    snap = g.snapshot()
    g.payload()[500] ^= 1
    assert g.guards_intact()  # the guards do not cover the payload ...
    res = g.unchanged_since(snap)  # ... the snapshot does
    assert not res and res.diffs == [("payload", 500, 1)]
    assert (res.diffs[0].region, res.diffs[0].offset, res.diffs[0].count) == ("payload", 500, 1)


def test_every_region_is_reported_with_its_own_count():
    g = _mk(256, 3)
    snap = g.snapshot()
    g.buf[g.start - 8:g.start - 5] ^= 0xFF
    g.payload()[10:20] ^= 0xFF
    g.buf[g.end + 32:g.end + 34] ^= 0xFF
    assert g.unchanged_since(snap).diffs == [("lower", -8, 3), ("payload", 10, 10), ("upper", 256 + 32, 2)]
    assert g.guards_intact().diffs == [("lower", -8, 3), ("upper", 256 + 32, 2)]


def test_the_stamp_depends_on_position_and_key():
    """No constant fill, no period a vector or a trip could reproduce: a guard shifted by 1, 2, 4, 8, 16 bytes, by a
    1 KiB wave-instruction or by a 16 KiB trip differs from itself almost everywhere, and two keys differ."""
    g = Guarded(0, 0, 64 << 10, 64 << 10, 1, device=CPU)
    s = g.buf.numpy()
    assert len(np.unique(s)) == 256
    for shift in (1, 2, 4, 8, 16, 1024, 16384):
        assert np.mean(s[shift:] == s[:-shift]) < 0.02
    other = Guarded(0, 0, 64 << 10, 64 << 10, 2, device=CPU).buf.numpy()
    assert np.mean(s[:other.size] == other[:s.size]) < 0.02


def test_reset_restamps_and_moves_the_payload_end():
    g = Guarded(64, 5, 32, 32, 3, device=CPU, capacity=512)
    g.load(np.full(64, 9, np.uint8))
    g.buf[g.end] ^= 1
    assert not g.guards_intact()
    g.reset(512)
    assert g.guards_intact() and g.payload().numel() == 512 and g.ptr % 16 == 5
    g.reset(0)
    assert g.guards_intact() and g.buf.numel() - g.end >= 512 + 32
    with pytest.raises(ValueError):
        g.reset(513)
    with pytest.raises(ValueError):
        g.load(np.zeros(3, np.uint8))


def _const(path, pattern):
    m = re.search(pattern, open(path).read())
    assert m, (path, pattern)
    return int(m.group(1))


def test_guard_size_follows_the_kernels_constants():
    """GUARD_BYTES is four of the largest trip any compiled shape takes: the workgroup sizes and vectors per lane in
    footprint_util.TRIP_SHAPES, read back from the sources they were taken from."""
    vec, tree = os.path.join(CSRC, "reduce_vec.hpp"), os.path.join(CSRC, "reduce_tree.hpp")
    user = os.path.join(REPO, "include", "chiara_user_op.hpp")
    kblock = _const(os.path.join(CSRC, "reduce_common.hpp"), r"constexpr int kBlock = (\d+);")
    src = {p: open(p).read() for p in (vec, tree, user)}
    # the two shapes each kernel is launched in: <.., 64, true, ..> streaming and <.., 256, false, ..> plain
    assert set(re.findall(r"launch_vec_mb_one<DT, OP, M, (\d+), (?:true|false)", src[vec])) == {"64", "256"}
    assert set(re.findall(r"launch_tree_vec<DT, OP, NL, (\d+), (?:true|false)>", src[tree])) == {"64", "256"}
    for path, text in ((vec, "return NT ? vec_u_nt<M>() : M <= 2 ? 4 : 2;"), (vec, "return M == 1 ? 4 : M <= 3 ? 2 : 1;"),
                       (tree, "if constexpr (!NT) return NL <= 4 ? 4 : 2;"), (tree, "return NL <= 2 ? 4 : NL <= 4 ? 2 : 1;")):
        assert text in src[path], (path, text)
    assert "return NL <= 2 ? 4 : NL <= 4 ? 2 : 1;" in src[user] and "const unsigned block = 256;" in src[user]
    want = {"bucket plain": (kblock, 4), "bucket streaming": (64, 4), "tree plain": (kblock, 4),
            "tree streaming": (64, 4), "user fold": (256, _const(user, r"#define CHR_USER_FOLD_U (\d+)")),
            "user tree": (_const(user, r"constexpr int kTreeBlock = (\d+);"), 4)}
    assert TRIP_SHAPES == want
    assert MAX_TRIP_BYTES == 16 << 10 and GUARD_BYTES == 4 * MAX_TRIP_BYTES == 64 << 10
    assert stream_guard(100) == GUARD_BYTES and stream_guard(8 << 20) == 8 << 20
