"""The one-pass user-op tree launcher beside RCCL: four spawned ranks (each a fresh process, as in
test_gpu_rccl_multirank.py) run an allreduce and a reduce-scatter at k = 2, b = 4 under the flat schedule -- 4-leaf
trees -- with overlap on, so the reductions share the GPU with RCCL's transfer kernels and the library asks the
launcher for its in-collective residency cap (12 workgroups per CU).  Bit-exact vs the oracle on every
rank; each rank's counters show tree-launcher calls and a last wg_per_cu of 12."""
import os

import pytest

from test_gpu_rccl_multirank import HERE, _init_worker, _setup, _spawn

pytestmark = pytest.mark.gpu


def _user_tree_worker(rank, world, port, q):
    _setup(rank)
    import ctypes

    import torch
    import torch.distributed as dist

    import chiara_amd as ca
    import pyoracle as po

    comm = _init_worker(rank, world, port)
    lib = ctypes.CDLL(os.path.join(HERE, "userop", "libhalfadd_tree_op.so"))
    lib.chr_test_counters.argtypes = [ctypes.POINTER(ctypes.c_long)]
    lib.chr_test_counters.restype = None
    half = ca.op_create(ctypes.cast(lib.chr_test_halfadd, ctypes.c_void_p).value,
                        tree=ctypes.cast(lib.chr_test_halfadd_tree, ctypes.c_void_p).value)
    bad = []
    try:
        comm.set_schedule(ca.SCHEDULE_FLAT)
        comm.set_overlap(True)
        count = 65537 * world
        for i, mode in enumerate(("ar", "rs")):
            in_n = count * world if mode == "rs" else count
            allx = [po.fill(in_n, "f32", po.PAT_UNIFORM, 950 + i, r) for r in range(world)]
            f = po.allreduce_radix_batch if mode == "ar" else po.reduce_scatter_radix_batch
            want = f(allx, 2, 4, "f32", "user_halfadd")[rank]
            fn = ca.all_reduce_radix_batch if mode == "ar" else ca.reduce_scatter_radix_batch
            dx = torch.from_numpy(allx[rank]).cuda()
            dout = torch.zeros(count, dtype=torch.float32, device=dx.device)
            lib.chr_test_counters_reset()
            rc = fn(dx, dout, count, ca.FLOAT32, half, comm, 2, 4)
            out = dout.cpu().numpy()
            c = (ctypes.c_long * 4)()
            lib.chr_test_counters(c)
            if rc != 0 or out.tobytes() != want.tobytes() or c[1] < 1 or c[3] != 12:
                bad.append((mode, rc, out.tobytes() == want.tobytes(), tuple(c)))
    finally:
        ca.op_free(half)
        comm.destroy()
        dist.destroy_process_group()
    q.put((rank, bad))


def test_rccl_user_tree_world4():
    res = _spawn(_user_tree_worker, 4)
    bad = [r for r in res if r[1]]
    assert not bad, bad
