"""The FP8 ops of libchiara_fp8.so beside RCCL: four spawned ranks sharing the GPU (each a fresh process, as in
tests/test_gpu_user_tree_rccl.py) run E4M3 SATURATE SUM allreduces under the flat and the one-shot schedule, a
reduce-scatter and a host-buffer allreduce at k = 2, b = 4, overlap on.  Bit-exact on every rank against the
SCHEDULE_REFERENCE plan under the plan evaluator (tests/fp8_ref.py); the device-buffer flat allreduce shows
tree-launcher calls and no fold call.  Every rank releases the ops before it leaves."""
import pytest

from test_gpu_rccl_multirank import _init_worker, _setup, _spawn

pytestmark = pytest.mark.gpu

CASES = [("ar", "flat", False), ("ar", "flat_1shot", False), ("rs", "flat", False), ("ar", "flat", True)]


def _fp8_worker(rank, world, port, q):
    _setup(rank)
    import numpy as np
    import torch
    import torch.distributed as dist

    import chiara_amd as ca
    import fp8_ref
    from chiara_amd import fp8

    comm = _init_worker(rank, world, port)
    bad = []
    try:
        op = fp8.fp8_op(fp8.E4M3, ca.SUM, fp8.SATURATE)
        ref = fp8_ref.Ref(fp8_ref.E4M3, "sum", fp8_ref.SATURATE)
        comm.set_overlap(True)
        count = 4099 * world
        for i, (mode, sched, host) in enumerate(CASES):
            comm.set_schedule({"flat": ca.SCHEDULE_FLAT, "flat_1shot": ca.SCHEDULE_FLAT_1SHOT}[sched])
            in_n = count * world if mode == "rs" else count
            allx = [fp8_ref.uniform(fp8_ref.E4M3, in_n, 970 + i, r) for r in range(world)]
            cmode = ca.MODE_ALLREDUCE if mode == "ar" else ca.MODE_REDUCE_SCATTER
            want = ref.expected(cmode, allx, 2, 4)[rank]
            fn = ca.all_reduce_radix_batch if mode == "ar" else ca.reduce_scatter_radix_batch
            fp8.stats(reset=True)
            if host:
                out = np.zeros(count, dtype=np.uint8)
                rc = fn(allx[rank].copy(), out, count, fp8.F8_DTYPE, op, comm, 2, 4)
            else:
                dx = torch.from_numpy(allx[rank].copy()).cuda()
                dout = torch.zeros(count, dtype=torch.uint8, device=dx.device)
                rc = fn(dx, dout, count, fp8.F8_DTYPE, op, comm, 2, 4)
                out = dout.cpu().numpy()
            folds, tree_calls, trees = fp8.stats()
            same = out.tobytes() == want.tobytes()
            one_pass = tree_calls >= 1 and folds == 0
            if rc != 0 or not same or ((mode, sched, host) == ("ar", "flat", False) and not one_pass):
                bad.append((mode, sched, host, rc, same, int(np.count_nonzero(out != want)), (folds, tree_calls, trees)))
    finally:
        fp8.release()
        comm.destroy()
        dist.destroy_process_group()
    q.put((rank, bad))


def test_rccl_fp8_sum_world4():
    res = _spawn(_fp8_worker, 4)
    bad = [r for r in res if r[1]]
    assert not bad, bad
