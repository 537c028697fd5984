"""Registers, scratch and LDS of libchiara_mx6_tree.so's kernels, read from the shipped code object (no GPU): at most the
72 VGPRs a wave may hold beside RCCL (tests/test_kernel_resources.py), no private segment, no static LDS (the stack's
park is the front of the launch's dynamic LDS)."""
import os
import re
import sys

import pytest

from chiara_amd import mx6

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_resources as kr  # noqa: E402


@pytest.mark.skipif(not os.path.exists(kr.READELF), reason="llvm-readelf not in this image")
def test_kernel_set_and_resources():
    """4 k_mx6_tree<E2M3 | E3M2, 8-B | 4-B accesses>: the leaf count, the stack depth and the program are run-time."""
    assert os.path.exists(mx6.MX6_TREE_LIB_PATH), f"{mx6.MX6_TREE_LIB_PATH} missing: __graft_entry__.build()"
    res = kr.kernel_resources(mx6.MX6_TREE_LIB_PATH)
    got = set()
    for name, r in res.items():
        m = re.fullmatch(r"_ZN7chr_mx6\d+k_mx6_treeILi([01])ELb([01])EEEv.*", name)
        assert m, name
        got.add(m.groups())
        assert r["scratch"] == 0, f"{name}: a private segment of {r['scratch']} bytes"
        assert r["lds"] == 0, f"{name}: {r['lds']} bytes of static LDS"
        assert kr.alloc_vgprs(r) <= 72, f"{name}: {kr.alloc_vgprs(r)} VGPRs"
    assert got == {(f, v) for f in "01" for v in "01"} and len(res) == 4, sorted(res)
