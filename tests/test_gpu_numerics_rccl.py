"""The double-word SUM of libchiara_numerics.so beside RCCL: four spawned ranks sharing the GPU (each a fresh process,
as in tests/test_gpu_f16_ops_rccl.py) pack their values, run the sum2 f32 allreduce at (4, 2, 2) of 4 x 257 elements
under the default schedule and compare every element's bits with the same plan under struct_ref's interpreter
(tests/numerics_ref.py).  Every rank releases the op and the type before it leaves."""
import pytest

from test_gpu_rccl_multirank import _init_worker, _setup, _spawn

pytestmark = pytest.mark.gpu


def _sum2_worker(rank, world, port, q):
    _setup(rank)
    import numpy as np
    import torch
    import torch.distributed as dist

    import chiara_amd as ca
    import numerics_ref as nr
    import struct_ref as sr
    from chiara_amd import numerics as num

    comm = _init_worker(rank, world, port)
    bad = []
    try:
        op, dt = num.sum2_op(), num.sum2_type(ca.FLOAT32)
        count = 257 * world
        rng = np.random.default_rng(977)
        values = [(rng.uniform(-1, 1, count) * np.exp2(rng.integers(-8, 9, count))).astype(np.float32)
                  for _ in range(world)]
        want = sr.simulate(ca.MODE_ALLREDUCE, [nr.sum2_pack(v) for v in values], 2, 2, 2, nr.sum2,
                           commutative=True)[rank]
        dv = torch.from_numpy(values[rank].copy()).cuda()
        dx = torch.zeros(2 * count, dtype=torch.float32, device=dv.device)
        dout = torch.zeros(2 * count, dtype=torch.float32, device=dv.device)
        stream = torch.cuda.current_stream()
        rc_pack = num.sum2_pack(dx, dv, count, ca.FLOAT32, stream)
        torch.cuda.synchronize()
        rc = ca.all_reduce_radix_batch(dx, dout, count, dt, op, comm, 2, 2)
        torch.cuda.synchronize()
        out = dout.cpu().numpy()
        differ = int(np.count_nonzero(out.view(np.uint32) != want.view(np.uint32)))
        if rc_pack != 0 or rc != 0 or differ:
            bad.append((rc_pack, rc, differ))
    finally:
        num.release()
        comm.destroy()
        dist.destroy_process_group()
    q.put((rank, bad))


def test_rccl_sum2_f32_world4():
    res = _spawn(_sum2_worker, 4)
    bad = [r for r in res if r[1]]
    assert not bad, bad
