"""A derived element type over RCCL: two spawned ranks (each a fresh process, as in test_gpu_rccl_multirank.py) run an
f64 x 3 HalfAdd allreduce at k = 2, b = 1 with N = 2 * 341 elements of 24 bytes -- a size RCCL has no type for, so
the executor's byte counts (messages as bytes) carry it.  Bit-exact vs the oracle's user_halfadd on 3N doubles."""
import os

import pytest

from test_gpu_rccl_multirank import HERE, _init_worker, _setup, _spawn

pytestmark = pytest.mark.gpu


def _struct_worker(rank, world, port, q):
    _setup(rank)
    import ctypes

    import numpy as np
    import torch
    import torch.distributed as dist

    import chiara_amd as ca
    import pyoracle as po

    comm = _init_worker(rank, world, port)
    lib = ctypes.CDLL(os.path.join(HERE, "userop", "libstruct_op.so"))
    dt = ca.type_contiguous(3, ca.FLOAT64)
    half = ca.op_create(ctypes.cast(lib.chr_struct_HalfAddK_f64x3, ctypes.c_void_p).value,
                        tree=ctypes.cast(lib.chr_struct_HalfAddK_f64x3_tree, ctypes.c_void_p).value)
    bad = []
    try:
        count = 341 * world
        allx = [po.fill(3 * count, "f64", po.PAT_UNIFORM, 960, r) for r in range(world)]
        want = po.allreduce_radix_batch(allx, 2, 1, "f64", "user_halfadd")[rank]
        dx = torch.from_numpy(allx[rank]).cuda()
        dout = torch.zeros(3 * count, dtype=torch.float64, device=dx.device)
        rc = ca.all_reduce_radix_batch(dx, dout, count, dt, half, comm, 2, 1)
        out = dout.cpu().numpy()
        if rc != 0 or out.tobytes() != want.tobytes():
            bad.append((rc, int(np.count_nonzero(out.view(np.uint64) != want.view(np.uint64)))))
    finally:
        ca.op_free(half)
        ca.type_free(dt)
        comm.destroy()
        dist.destroy_process_group()
    q.put((rank, bad))


def test_rccl_struct_allreduce_world2():
    res = _spawn(_struct_worker, 2)
    bad = [r for r in res if r[1]]
    assert not bad, bad
