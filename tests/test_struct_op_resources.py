"""Registers, scratch and LDS of the derived-type kernels (include/chiara_user_op.hpp: k_fold and k_tree on elements
whose size does not divide 16), read from tests/userop/libstruct_op.so -- the header as shipped -- and
libstruct_op_all.so -- element groups at every size that has them (no GPU).  build() makes both; where one is missing
the fixture makes it the same way.

An element of S bytes in groups streams lcm(S, 16) bytes per lane, V = lcm(S, 16) / 16 vectors.  What this pins:
  * no kernel of either build has a private segment or static LDS -- the groups exchange nothing between lanes, the
    launch's dynamic LDS stays the residency cap only (0 bytes of LDS per workgroup are the kernels' own);
  * every vector tree instantiation k_tree<T, F, NL, U > 0, 64> allocates at most 72 VGPRs, the room a wave has beside
    RCCL at 12 workgroups per CU (tests/test_kernel_resources.py) -- the launcher selects exactly these
    whatever wg_per_cu is;
  * the decline rule shows in the symbols: U = 0 names an instantiation without a vector path, and none with U > 0
    has NL x U x V > 8 loads of 16 B in flight per lane, or an element size that is no multiple of 4;
  * the shipped build takes groups in its trees at 32 bytes only (the measured rows in the header)."""
import os
import re
import subprocess
import sys
from math import gcd

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(kr.READELF), reason="llvm-readelf not in this image")

USEROP = os.path.join(HERE, "userop")
RCCL_ROOM_VGPRS = 72
BASE_BYTES = {"h": 1, "s": 2, "f": 4, "i": 4, "d": 8}  # the Itanium codes of uint8_t, short, float, int, double
# base code x K of struct_op.hip's instantiations
SHAPES = {("h", 3), ("s", 3), ("f", 2), ("f", 3), ("f", 4), ("f", 5), ("d", 3), ("d", 4), ("d", 6), ("d", 8), ("d", 9),
          ("i", 3)}


@pytest.fixture(scope="module")
def both():
    paths = {b: os.path.join(USEROP, so) for b, so in (("shipped", "libstruct_op.so"), ("all", "libstruct_op_all.so"))}
    if not all(os.path.exists(p) for p in paths.values()):
        made = subprocess.run(["make", "-s", "-C", USEROP, "-f", "struct_op.mk"], capture_output=True, text=True,
                              timeout=1800)
        assert made.returncode == 0, made.stdout[-2000:] + made.stderr[-2000:]
    return {b: kr.kernel_resources(p) for b, p in paths.items()}


@pytest.fixture(scope="module", params=["shipped", "all"])
def res(both, request):
    return both[request.param]


def _trees(res):
    """(base code, K, functor, leaves, U) -> allocated VGPRs of k_tree<Blk<B, K>, F<B, K>, NL, U, 64>."""
    out = {}
    for name, r in res.items():
        m = re.search(r"6k_treeI3BlkI([a-z])Li(\d+)EE\d+([A-Za-z]+)I[a-z]Li\d+EELi(\d+)ELi(\d+)ELi64EEE", name)
        if m:
            out[(m.group(1), int(m.group(2)), m.group(3), int(m.group(4)), int(m.group(5)))] = kr.alloc_vgprs(r)
    return out


def _vectors(base, k):
    s = BASE_BYTES[base] * k
    return s // gcd(s, 16)  # lcm(S, 16) / 16


def test_no_kernel_has_a_private_segment_or_static_lds(res):
    folds = [n for n in res if "6k_foldI3Blk" in n]
    assert len(folds) == 14  # 11 RotMix shapes and 3 HalfAdd ones
    assert len(_trees(res)) == 14 * 7  # each with 2..8 leaves
    scratch = {n: r["scratch"] for n, r in res.items() if r["scratch"]}
    assert not scratch, f"kernels with a private segment: {sorted(scratch)}"
    lds = {n: r["lds"] for n, r in res.items() if r["lds"]}
    assert not lds, f"kernels with static LDS (the cap is dynamic LDS only): {sorted(lds)}"


def test_vector_trees_leave_rccl_its_registers(res):
    t = _trees(res)
    assert {(b, k) for b, k, *_ in t} == SHAPES
    vec = {key: v for key, v in t.items() if key[4] > 0}
    assert ("d", 4, "RotMixK", 4, 1) in vec and ("d", 4, "RotMixK", 2, 2) in vec  # 32-byte elements, up to 4 leaves
    over = {key: v for key, v in vec.items() if v > RCCL_ROOM_VGPRS}
    assert not over, f"vector trees above {RCCL_ROOM_VGPRS} VGPRs: {sorted(over.items())}"


def test_decline_rule_is_visible_in_the_symbols(both):
    t = _trees(both["all"])
    for (b, k, f, nl, u), _ in t.items():
        s, v = BASE_BYTES[b] * k, _vectors(b, k)
        if 16 % s == 0:  # FoldVec's sizes: the parent's shapes, 4 / 2 / 1 vectors per lane
            assert u == (4 if nl <= 2 else 2 if nl <= 4 else 1), (b, k, nl, u)
            continue
        can = nl * v <= 8 and s % 4 == 0
        assert (u > 0) == can, (b, k, f, nl, u)
        if u:
            assert nl * u * v <= 8 and u == min(8 // (nl * v), 4 if nl <= 2 else 2 if nl <= 4 else 1), (b, k, nl, u)
    # the issue's examples: 8 leaves of 24-byte elements, and any tree of V > 4 (f32 x 5: V = 5; f64 x 9: V = 9)
    assert t[("d", 3, "RotMixK", 8, 0)] and t[("f", 5, "RotMixK", 2, 0)] and t[("d", 9, "RotMixK", 2, 0)]


def test_shipped_build_groups_its_trees_at_32_bytes_only(both):
    for (b, k, f, nl, u), _ in _trees(both["shipped"]).items():
        s, v = BASE_BYTES[b] * k, _vectors(b, k)
        if 16 % s:
            assert (u > 0) == (s == 32 and nl * v <= 8), (b, k, f, nl, u)
