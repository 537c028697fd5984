"""Every streaming instantiation of the bucket and tree kernels against the oracle, bit for bit.

Calls of >= 40 MiB (buckets) / 64 MiB (trees) run the streaming shape of k_reduce_vec / k_reduce_tree: one-wave
workgroups, ld<NT> / st<NT> with slot 0 peeled to the default policy (ACC0), vec_u_nt<M>() / tree_u<NL, true>()
vectors per lane per trip, trips placed by xcd_trip_w, and a partial trip that falls back to plain loads and, for
trees, to the interpreter.  It is compiled separately from the plain shape, per (dtype, op) and per fan-in M = 1..8 or
leaf count NL = 2..8; the tuning variables CHR_REDUCE_NT / CHR_REDUCE_NT_MIN_BYTES select it at oracle-sized operands
(~70 KiB, tests/streaming_cases.py, which holds the case lists and runs them).  They are read once per process, so
each sweep runs in a child process with a fresh interpreter: never more than four alive, 300 s each, and after a
child that ends abnormally (time limit, signal, abort, segmentation fault, an illegal memory access) this module
starts no further child.

  bucket A    every (dtype, op) x m = 1..8 x {in place aligned, out of place shifted}; the running-first codes of the
              floating types on TIES data; one m = 3 call per pair / complex (dtype, op)
  tree A / B  every (dtype, op) x NL = 2..8: each StaticProgs<NL> program unswapped (tree_eval_static) and swapped
              (tree_eval for order-sensitive ops), a non-static program, shifted and aliased outputs, and the 2-leaf
              tree in both operand orders x out in {separate, leaf 0, leaf 1} -- in configuration B the bucket route
              and the kept-on-tree case out == in
  programs A  every valid program of 2..8 leaves (377) x 4 (dtype, op, data, swaps) variants, and one batch of 9
              trees whose segments mix the evaluators
The 377 programs also run here in process, on the plain shape."""
import collections
import concurrent.futures
import json
import os
import subprocess
import sys
import time

import pytest

import streaming_cases as sc
from test_gpu_kernels import DT

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 300
MAX_CHILDREN = 4
_ABNORMAL = []  # (job, why) of every child that ended abnormally: once set, no further child starts


def _run_child(job):
    if _ABNORMAL:
        return {"error": "earlier child ended abnormally", "not_started": True}
    t0 = time.perf_counter()
    flags = ["-s"] if sys.flags.no_user_site else []  # the child sees the packages this interpreter sees
    p = subprocess.Popen([sys.executable, *flags, os.path.join(sc.HERE, "streaming_cases.py"), job],
                         env=sc.child_env(job), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        out, err = p.communicate(timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        p.kill()
        p.communicate()
        _ABNORMAL.append((job, "time limit"))
        return {"error": f"no result within {CHILD_TIMEOUT_S} s"}
    wall = time.perf_counter() - t0
    if p.returncode < 0 or p.returncode in (134, 139) or "illegal memory access" in err:
        _ABNORMAL.append((job, f"exit status {p.returncode}"))
        return {"error": f"ended abnormally, exit status {p.returncode}: {err[-2000:]}"}
    if p.returncode != 0:
        return {"error": f"exit status {p.returncode}: {err[-2000:]}"}
    res = json.loads(out.strip().splitlines()[-1])
    res["wall"] = round(wall, 2)
    return res


@pytest.fixture(scope="module")
def children():
    """job -> the child's result line.  The children run side by side (each is a second or two of start-up in front
    of a few thousand small launches), at most MAX_CHILDREN at once."""
    with concurrent.futures.ThreadPoolExecutor(max_workers=MAX_CHILDREN) as pool:
        return dict(zip(sc.JOBS, pool.map(_run_child, sc.JOBS)))


def _result(children, job):
    res = children[job]
    assert "error" not in res, f"child '{job}': {res['error']}"
    return res


def _check(children, job, key, expected, of_dtype=None):
    """The child ran exactly the case list's cases under `key` and none differs."""
    res = _result(children, job)
    assert res["ran"].get(key, 0) == expected, (job, key, res["ran"].get(key), expected)
    bad = [b for b in res["bad"] if of_dtype is None or b[0] == of_dtype]
    per_op = dict(collections.Counter(b[1] for b in bad))
    assert not bad, (f"'{job}': {len(bad)} cases differ, per op {per_op}; (dtype, op, case, layout, first index) "
                     f"e.g. {bad[:6]}")


@pytest.mark.parametrize("job", list(sc.JOBS))
def test_child_ended_normally(children, job):
    res = _result(children, job)
    print(f"streaming sweep child '{job}': {res['seconds']} s of cases, {res['wall']} s wall, "
          f"{sum(res['ran'].values())} cases")


@pytest.mark.parametrize("dtype", list(DT))
def test_bucket_sweep_streaming(children, dtype):
    expected = sum(c.dtype == dtype for c in sc.bucket_cases())
    assert expected
    _check(children, "bucket A", dtype, expected, dtype)


@pytest.mark.parametrize("config", ["A", "B"])
@pytest.mark.parametrize("dtype", sc.SWEEP_DTYPES)
def test_tree_sweep_streaming(children, dtype, config):
    expected = sum(len(sc.tree_cases(d, o)) for d, o in sc.SWEEP_PAIRS if d == dtype)
    assert expected
    _check(children, f"tree {config}", dtype, expected, dtype)


@pytest.mark.parametrize("variant", list(sc.PROGRAM_VARIANTS))
def test_every_program_streaming(children, variant):
    res = _result(children, "programs A")
    assert res["ran"].get(variant) == 377
    bad = [b for b in res["bad"] if str(b[2]).startswith(f"every program ({variant})")]
    assert not bad, f"{len(bad)} programs differ, e.g. {bad[:6]}"


def test_batched_segments_streaming(children):
    res = _result(children, "programs A")
    assert res["ran"].get("batch") == 9 * len(sc.BATCH_NVEC)
    bad = [b for b in res["bad"] if str(b[2]).startswith("batch")]
    assert not bad, bad[:6]


@pytest.fixture(scope="module")
def dev():
    import gpu_util

    return sc.Device(gpu_util)


@pytest.mark.parametrize("variant", list(sc.PROGRAM_VARIANTS))
def test_every_program_plain(dev, variant):
    """The same 377 programs in this process: the plain shape of the vector tree kernel (256 threads, U = 4 / 2)."""
    bad = []
    cases = sc.program_cases(variant)
    assert len(cases) == 377
    sc.run_tree_cases(dev, cases, bad)
    assert not bad, f"{len(bad)} programs differ, e.g. {bad[:6]}"
