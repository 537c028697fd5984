"""Register and scratch budget of the one-pass user-op tree kernels (include/chiara_user_op.hpp k_tree), read from the
test code object tests/userop/libhalfadd_tree_op.so (no GPU).  build() makes that file; where it is missing -- a tests/
directory put in place after the build -- the fixture makes it the same way.

The kernels are compiled into the caller's code object, so the library's own resource test does not see them.  Beside
RCCL they run at 12 one-wave workgroups per CU like the library's trees, where a wave may take at
most 72 VGPRs (tests/test_kernel_resources.py); and an interpreter that indexed its stack by the run-time depth would
show as a private segment."""
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(kr.READELF), reason="llvm-readelf not in this image")

TREE_SO = os.path.join(HERE, "userop", "libhalfadd_tree_op.so")
RCCL_ROOM_VGPRS = 72
TYPES = {"f": "f32", "d": "f64", "i": "i32"}


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(TREE_SO):  # a tests/ directory put in place after build(): make it the way build() does
        made = subprocess.run(["make", "-s", "-C", os.path.dirname(TREE_SO), "-f", "tree_op.mk"], capture_output=True,
                              text=True, timeout=900)
        assert made.returncode == 0, made.stdout[-2000:] + made.stderr[-2000:]
    assert os.path.exists(TREE_SO), f"{TREE_SO} missing: make -C tests/userop -f tree_op.mk (__graft_entry__.build())"
    return kr.kernel_resources(TREE_SO)


def _trees(res):
    """(dtype, leaves, vectors per lane) -> allocated VGPRs of k_tree<T, F, NL, U, 64>."""
    out = {}
    for name, r in res.items():
        m = re.search(r"6k_treeI([fdi])\d+[A-Za-z0-9]+Li(\d+)ELi(\d+)ELi64EEE", name)
        if m:
            out[(TYPES[m.group(1)], int(m.group(2)), int(m.group(3)))] = kr.alloc_vgprs(r)
    return out


def test_no_kernel_has_a_private_segment(res):
    assert len(res) >= 24  # 3 fold kernels and 3 types x 7 leaf counts of trees
    scratch = {n: r["scratch"] for n, r in res.items() if r["scratch"]}
    assert not scratch, f"kernels with a private segment: {sorted(scratch)}"
    lds = {n: r["lds"] for n, r in res.items() if r["lds"]}
    assert not lds, f"kernels with static LDS (the cap is dynamic LDS only): {sorted(lds)}"


def test_f32_8_leaf_tree_leaves_rccl_its_registers(res):
    t = _trees(res)
    assert {(dt, nl) for dt, nl, _ in t} == {(dt, nl) for dt in TYPES.values() for nl in range(2, 9)}, sorted(t)
    c4 = [v for (dt, nl, _), v in t.items() if dt == "f32" and nl == 8]
    assert len(c4) == 1
    assert c4[0] <= RCCL_ROOM_VGPRS, f"f32 8-leaf tree: {c4[0]} VGPRs; all (dtype, leaves, U): {sorted(t.items())}"
