"""The relations of csrc/plan_util.hpp under AddressSanitizer + UBSan (host code only; no GPU): which trees of a
step share a batched launch, decided on resolved byte ranges -- so that CHR_IN_PLACE, which makes SEND and RECV one
buffer, splits a run the out-of-place call batches -- the (buffer, offset) conflict relation the compiler orders
steps by (SEND and RECV one space, L_COPY2D row by row), and the loopback matcher of the local group and the flat
schedule's symbolic execution, on hand-made steps (tests/host/plan_util_check.cpp).  The matcher over every compiled
plan is part of tools/plan_fuzz.cpp (tests/test_plan_fuzz.py)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "configurable-hierarchical-allreduce-algorithms_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plan_util_under_sanitizers(tmp_path):
    exe = str(tmp_path / "plan_util_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(REPO, "include"),
                           "-I" + os.path.join(PKG, "csrc"), os.path.join(REPO, "tests", "host", "plan_util_check.cpp"),
                           os.path.join(PKG, "csrc", "schedule.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    assert '"failures": 0' in out.stdout
