"""The MX tile ops over RCCL: four spawned ranks (each a fresh process, as in test_gpu_rccl_multirank.py) run the MXFP8
E4M3 SUM and the MXFP4 SUM, each as the fold-only op and as its tree-registered twin, through the comm executor
(csrc/exec_comm.cpp) -- another seam than the LocalGroup's virtual ranks: a second stream, pipeline slices, and 528- and
272-byte elements that RCCL has no type for, carried as byte counts.  k = 2, b = 4 under the flat schedule (4-leaf
trees), overlap on, so the library hands the tree launchers its in-collective residency cap (user_ops.cpp user_trees;
test_gpu_user_tree_rccl.py reads that 12 from a launcher that records it); set_slices(1) and set_slices(3).
Two sizes.  An allreduce of 4 x 5 tiles and a reduce-scatter receiving 5: below the planner's 256-element slice and
64-element piece bounds (csrc/schedule.cpp build_plan_flat), so one slice whatever is set, and in the allreduce one
rank reduces the whole buffer while the others only send and receive.  And 776 tiles (allreduced, and received by the
reduce-scatter): three slices of 256, 256 and 264 tiles, the uneven cut.  Every rank's send holds a NaN block and an
all-zero block at rank-dependent positions.  Bit-exact on every rank against the plan evaluator over tests/mx_ref.py /
tests/mx4_ref.py.  Each rank also reports its launchers' counters against its own plan (chr_plan_describe): where the
plan has tree steps, the fold-only op's folds ran, never reached the tree launcher and declined nothing, and the
twin's trees reached the tree launcher, none declined; where it has none, neither launcher was called.

With set_graphs(True) a user op is not refused: exec_comm.cpp chr_comm_collective sends `c->graphs && ... &&
!chr::is_user_op(op)` to launch_graph and every user op to enqueue_rccl, since a launcher may allocate stream-ordered
scratch and is never captured.  So the two calls under set_graphs(True) -- where a native op would capture, then
replay -- run eagerly, the second on fresh input in the same buffers, and both must be exact with the tree launcher
called each time."""
import pytest

from test_gpu_rccl_multirank import HERE, _init_worker, _setup, _spawn  # noqa: F401  (HERE: the workers' import path)

pytestmark = pytest.mark.gpu


def _mx_worker(rank, world, port, q, kind):
    _setup(rank)
    import numpy as np
    import torch
    import torch.distributed as dist

    import chiara_amd as ca
    from test_gpu_mx_seams import KINDS, marked_sends, planned

    K = next(k for k in KINDS if k.name == kind)
    comm = _init_worker(rank, world, port)
    dev = torch.device("cuda:0")
    bad = []
    try:
        dt = K.lib.mx4_type() if kind == "mx4" else K.lib.mx_type()
        f = None if kind == "mx4" else {"e4m3": 0, "e5m2": 1}[kind]
        ops = {"fold": K.lib.mx4_sum() if f is None else K.lib.mx_sum(f),
               "tree": K.lib.mx4_sum_tree() if f is None else K.lib.mx_sum_tree(f)}
        comm.set_schedule(ca.SCHEDULE_FLAT)
        comm.set_overlap(True)
        cache = {}

        def reference(mode, count, seed):  # every rank builds all four sends from the seed; one reference per case
            if (mode, count, seed) not in cache:
                sends = marked_sends(K, world, count if mode == "ar" else count * world, seed)
                cmode = ca.MODE_ALLREDUCE if mode == "ar" else ca.MODE_REDUCE_SCATTER
                cache[mode, count, seed] = sends[rank], K.expected(cmode, sends, 2, 4, ca.SCHEDULE_FLAT)[rank], cmode
            return cache[mode, count, seed]

        def run(mode, count, seed, name, slices, what):
            mine, want, cmode = reference(mode, count, seed)
            send[:mine.size].copy_(torch.from_numpy(mine.copy()))
            out.fill_(0xA5)
            K.lib.stats(reset=True), K.lib.tree_stats(reset=True)
            fn = ca.all_reduce_radix_batch if mode == "ar" else ca.reduce_scatter_radix_batch
            rc = fn(send, out, count, dt, ops[name], comm, 2, 4)
            same = np.array_equal(out[:count * K.TB].cpu().numpy(), want)
            fold, tree = K.lib.stats(), K.lib.tree_stats()
            plan = planned(cmode, world, rank, 2, 4, count, slices)
            if plan[0] != (3 if slices == 3 and count >= 768 else 1):
                bad.append((what, mode, "plan", plan))
            if plan[1] == 0:
                counted = fold[0] == 0 and tree[0] == 0
            elif name == "fold":
                counted = tree[0] == 0 and fold[0] >= 1 and fold[1] == 0 and fold[2] >= 1
            else:
                counted = tree[0] >= 1 and tree[1] == 0 and tree[3] >= 1
            if rc != 0 or not same or not counted:
                bad.append((what, mode, name, rc, same, fold, tree, plan))

        big = 776
        send = torch.empty(big * world * K.TB, dtype=torch.uint8, device=dev)
        out = torch.empty(big * K.TB, dtype=torch.uint8, device=dev)
        for slices in (1, 3):
            comm.set_slices(slices)
            for i, (mode, count) in enumerate((("ar", 5 * world), ("rs", 5), ("ar", big), ("rs", big))):
                for name in ("fold", "tree"):
                    run(mode, count, 970 + i, name, slices, f"slices {slices} count {count}")
        comm.set_slices(1)
        comm.set_graphs(True)
        run("rs", 5, 980, "tree", 1, "graphs on, first call")
        run("rs", 5, 981, "tree", 1, "graphs on, second call, fresh input")
    finally:
        comm.set_graphs(False)
        K.lib.tree_release()
        K.lib.release()
        comm.destroy()
        dist.destroy_process_group()
    q.put((rank, bad))


@pytest.mark.parametrize("kind", ["e4m3", "mx4"])
def test_rccl_mx_world4(kind):
    res = _spawn(_mx_worker, 4, extra=(kind,))
    bad = [r for r in res if r[1]]
    assert not bad, bad
