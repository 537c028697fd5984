"""Registers, scratch and LDS of libchiara_mxint8_tree.so's kernels, read from the shipped code object (no GPU): at most
the 72 VGPRs a wave may hold beside RCCL (tests/test_kernel_resources.py), no private segment, no static LDS."""
import os
import re
import sys

import pytest

from chiara_amd import mxint8

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_resources as kr  # noqa: E402


@pytest.mark.skipif(not os.path.exists(kr.READELF), reason="llvm-readelf not in this image")
def test_kernel_set_and_resources():
    """2 k_mxi8_tree<16-B | 4-B accesses>: the leaf count, the stack depth and each combine's path are run-time."""
    assert os.path.exists(mxint8.MXINT8_TREE_LIB_PATH), f"{mxint8.MXINT8_TREE_LIB_PATH} missing: __graft_entry__.build()"
    res = kr.kernel_resources(mxint8.MXINT8_TREE_LIB_PATH)
    got = set()
    for name, r in res.items():
        m = re.fullmatch(r"_ZN8chr_mxi8\d+k_mxi8_treeILb([01])EEEv.*", name)
        assert m, name
        got.add(m.group(1))
        assert r["scratch"] == 0, f"{name}: a private segment of {r['scratch']} bytes"
        assert r["lds"] == 0, f"{name}: {r['lds']} bytes of static LDS"
        assert kr.alloc_vgprs(r) <= 72, f"{name}: {kr.alloc_vgprs(r)} VGPRs"
    assert got == {"0", "1"} and len(res) == 2, sorted(res)
