"""Registers, scratch and LDS of libchiara_mx4_sr.so's kernels, read from the shipped code object (no GPU): at most
the 72 VGPRs a wave may hold beside RCCL (tests/test_kernel_resources.py), no private segment, no static LDS."""
import os
import re
import sys

import pytest

from chiara_amd import mx4

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_resources as kr  # noqa: E402


@pytest.mark.skipif(not os.path.exists(kr.READELF), reason="llvm-readelf not in this image")
def test_kernel_set_and_resources():
    """2 k_mx4_sr_fold<16-B | 4-B accesses> and 4 k_mx4_sr_quantize<f32 | bf16, accesses>."""
    assert os.path.exists(mx4.MX4_SR_LIB_PATH), f"{mx4.MX4_SR_LIB_PATH} missing: __graft_entry__.build()"
    res = kr.kernel_resources(mx4.MX4_SR_LIB_PATH)
    got = set()
    for name, r in res.items():
        m = re.fullmatch(r"_ZN10chr_mx4_sr\d+(k_mx4_sr_fold|k_mx4_sr_quantize)I([ft]?)Lb([01])EEEv.*", name)
        assert m, name
        got.add(m.groups())
        assert r["scratch"] == 0, f"{name}: a private segment of {r['scratch']} bytes"
        assert r["lds"] == 0, f"{name}: {r['lds']} bytes of static LDS"
        assert kr.alloc_vgprs(r) <= 72, f"{name}: {kr.alloc_vgprs(r)} VGPRs"
    want = {("k_mx4_sr_fold", "", v) for v in "01"} | {("k_mx4_sr_quantize", w, v) for w in "ft" for v in "01"}
    assert got == want and len(res) == 6, sorted(res)
