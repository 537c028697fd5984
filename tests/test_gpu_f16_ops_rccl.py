"""The binary16 ops of libchiara_ops.so beside RCCL: four spawned ranks sharing the GPU (each a fresh process, as in
tests/test_gpu_user_tree_rccl.py) run f16 SUM allreduces under the flat and the one-shot schedule, a reduce-scatter
and a host-buffer allreduce at k = 2, b = 4, overlap on.  Bit-exact on every rank against the SCHEDULE_REFERENCE plan
under the plan evaluator (tests/f16_ref.py); the device-buffer flat allreduce shows tree-launcher calls and no fold
call.  Every rank releases the ops before it leaves."""
import pytest

from test_gpu_rccl_multirank import _init_worker, _setup, _spawn

pytestmark = pytest.mark.gpu

CASES = [("ar", "flat", False), ("ar", "flat_1shot", False), ("rs", "flat", False), ("ar", "flat", True)]


def _f16_worker(rank, world, port, q):
    _setup(rank)
    import numpy as np
    import torch
    import torch.distributed as dist

    import chiara_amd as ca
    import f16_ref
    from chiara_amd import ops

    comm = _init_worker(rank, world, port)
    bad = []
    try:
        op = ops.float16_op(ca.SUM)
        comm.set_overlap(True)
        count = 4099 * world
        for i, (mode, sched, host) in enumerate(CASES):
            comm.set_schedule({"flat": ca.SCHEDULE_FLAT, "flat_1shot": ca.SCHEDULE_FLAT_1SHOT}[sched])
            in_n = count * world if mode == "rs" else count
            allx = [f16_ref.uniform(in_n, 960 + i, r) for r in range(world)]
            cmode = ca.MODE_ALLREDUCE if mode == "ar" else ca.MODE_REDUCE_SCATTER
            want = f16_ref.expected(cmode, allx, 2, 4, "sum")[rank]
            fn = ca.all_reduce_radix_batch if mode == "ar" else ca.reduce_scatter_radix_batch
            ops.stats(reset=True)
            if host:
                out = np.zeros(count, dtype=np.uint16)
                rc = fn(allx[rank].copy(), out, count, ops.F16_DTYPE, op, comm, 2, 4)
            else:
                dx = torch.from_numpy(allx[rank].view(np.int16).copy()).cuda()
                dout = torch.zeros(count, dtype=torch.int16, device=dx.device)
                rc = fn(dx, dout, count, ops.F16_DTYPE, op, comm, 2, 4)
                out = dout.cpu().numpy().view(np.uint16)
            folds, tree_calls, trees = ops.stats()
            same = out.tobytes() == want.tobytes()
            one_pass = tree_calls >= 1 and folds == 0
            if rc != 0 or not same or ((mode, sched, host) == ("ar", "flat", False) and not one_pass):
                bad.append((mode, sched, host, rc, same, int(np.count_nonzero(out != want)), (folds, tree_calls, trees)))
    finally:
        ops.release()
        comm.destroy()
        dist.destroy_process_group()
    q.put((rank, bad))


def test_rccl_f16_sum_world4():
    res = _spawn(_f16_worker, 4)
    bad = [r for r in res if r[1]]
    assert not bad, bad
