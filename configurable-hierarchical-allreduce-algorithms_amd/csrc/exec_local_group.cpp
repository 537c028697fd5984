// exec_local_group.cpp -- the loopback executor: n virtual ranks on one device run the same plans and kernels, the
// messages of a step (plan_util.hpp match_step) being device-to-device copies and the ranks' trees of one step sharing
// launches.  Used to check multi-rank schedules on a single MI355X.  Also the group's lifecycle; teardown is
// ~chr_local_group.
#include "exec_internal.hpp"

namespace chr {

int local_collective(chr_local_group* g, int mode, const void* const* sends, void* const* recvs, size_t count,
                     int dtype, int op, int k, int b) {
    if (!g || !sends || !recvs) return CHR_ERR_INVALID_ARG;
    if (int rc = check_args(mode, dtype, op)) return rc;
    const int n = g->nranks;
    // the MPICH baselines branch on MPI_Op_commutative (build_plan_mpich); CHiArA's own collectives take any op
    const bool commutative = chr::op_commutative(op);
    const int depth = pick_slices(g->slices, count, mode, n, b, chr::elem_size(dtype), g->sched);
    auto key = std::make_tuple(mode, k, b, (uint64_t)count, (int)chr::elem_size(dtype), depth, g->sched, commutative);
    auto it = g->plans.find(key);
    if (it == g->plans.end()) {
        std::vector<Plan> v;
        for (int r = 0; r < n; ++r)
            v.push_back(chr::build_plan((chr::Mode)mode, n, r, k, b, count, depth, g->sched, commutative));
        it = g->plans.emplace(key, std::move(v)).first;
    }
    const std::vector<Plan>& P = it->second;
    if (P[0].error) return P[0].error;
    if (P[0].g.total == 0) return CHR_SUCCESS;
    const size_t es = chr::elem_size(dtype);
    hipError_t e = hipSetDevice(g->device);
    if (e != hipSuccess) return hip_code(e);
    std::vector<Bufs> B(n);
    for (int r = 0; r < n; ++r) {
        if (!recvs[r] && P[r].recv_elems) return CHR_ERR_INVALID_ARG;
        if ((e = g->acc[r].reserve(P[r].acc_elems * es, g->stream)) != hipSuccess) return hip_code(e);
        if ((e = g->stage[r].reserve(P[r].stage_elems * es, g->stream)) != hipSuccess) return hip_code(e);
        const void* in = nullptr;
        if (int rr = resolve_input(mode, sends[r], recvs[r], r, count, es, &in)) return rr;
        if ((P[r].send_elems && (!in || !is_device_ptr(in))) || (P[r].recv_elems && !is_device_ptr(recvs[r])))
            return CHR_ERR_INVALID_ARG;
        B[r] = Bufs{(const char*)in, (char*)recvs[r], (char*)g->acc[r].p, (char*)g->stage[r].p, es};
    }
    int rc;
    // One phase of local ops of all ranks, on the group's stream; while profiling, bracketed by events
    // on that stream.
    auto phase = [&](auto&& ops_of) -> int {
        bool any = false, reduces = false;
        for (int r = 0; r < n; ++r) {
            any = any || !ops_of(r).empty();
            for (const chr::LocalOp& op : ops_of(r)) reduces = reduces || op.kind == chr::L_REDUCE || op.kind == chr::L_TREE;
        }
        if (!any) return CHR_SUCCESS;
        // a phase of copies only (re-layouts, the stand-alone phases' copy-outs) is not a reduction span
        return g->prof.bracket(g->prof.on && reduces, g->stream, [&]() -> int {
            // The virtual ranks' local ops of one step touch only their own buffers.  When every rank's
            // ops are one batchable run of trees (the flat schedules' slice evaluations), all ranks'
            // trees go to one launch_reduce_tree_multi call: one grid per 8 trees instead of one per
            // rank, so the step pays the fixed cost of a launch -- ~4.5 us between back-to-back grids
            // on one stream plus ~3-4 us of fill and drain (tools/reduce_microbench focus22/23,
            // profiles/r03/launch_timeline/) -- once per 8 trees.  A real node has one rank per GPU
            // and so one launch per rank per slice; rows measured there are the rank-alone replays of
            // bench.py --collective-kernels.
            std::vector<TreeJob> jobs;
            std::vector<Touched> t;  // what jobs[i] touches
            double bytes = 0;
            bool merged = g->batch_ranks && n > 1;
            for (int r = 0; r < n && merged; ++r) {
                const std::vector<LocalOp>& ops = ops_of(r);
                if (!(merged = one_tree_run(ops, es, [&](const Ref& x) { return B[r].ptr(x); }))) break;
                const size_t j0 = jobs.size();
                bytes += tree_jobs(ops, 0, ops.size(), B[r], &jobs);
                for (size_t y = j0; y < jobs.size(); ++y) t.push_back(touched(jobs[y], es));
                for (size_t x = 0; x < j0 && merged; ++x)  // earlier ranks' trees vs this rank's
                    for (size_t y = j0; y < jobs.size() && merged; ++y) merged = !conflict(t[x], t[y]);
            }
            if (merged) return launch_tree_jobs(jobs, bytes, dtype, op, g->stream, g->prof);
            for (int r = 0; r < n; ++r)
                if ((rc = run_locals(ops_of(r), B[r], dtype, op, g->stream, g->prof))) return rc;
            return CHR_SUCCESS;
        });
    };
    if ((rc = phase([&](int r) -> const std::vector<chr::LocalOp>& { return P[r].pre; }))) return rc;
    const size_t nsteps = P[0].steps.size();
    for (size_t si = 0; si < nsteps; ++si) {
        // Loopback transport: a step's messages as device-to-device copies.
        Mismatch bad;
        const bool matched = match_step(P, si, [&](int r, const Xfer& rv, int q, const Xfer& sd) {
            if (e != hipSuccess) return;
            e = hipMemcpyAsync(B[r].ptr(rv.ref), B[q].ptr(sd.ref), rv.count * es, hipMemcpyDeviceToDevice, g->stream);
        }, &bad);
        if (e != hipSuccess) return hip_code(e);
        if (!matched) {
            if (bad.receiver >= 0)
                std::fprintf(stderr, "[chiara] plan mismatch: step %zu rank %d <- %d\n", si, bad.receiver, bad.sender);
            else
                std::fprintf(stderr, "[chiara] plan mismatch: unmatched send step %zu rank %d\n", si, bad.sender);
            return CHR_ERR_UNSUPPORTED;
        }
        // allgather collectives: every rank's block r to every other rank, same region
        for (size_t ci = 0; ci < P[0].steps[si].allgathers.size(); ++ci)
            for (int r = 0; r < n; ++r)
                for (int q = 0; q < n; ++q) {
                    if (q == r) continue;
                    const chr::Coll& x = P[r].steps[si].allgathers[ci];
                    const size_t off = (size_t)q * x.count * es;
                    if ((e = hipMemcpyAsync(B[r].ptr(x.ref) + off, B[q].ptr(P[q].steps[si].allgathers[ci].ref) + off,
                                            x.count * es, hipMemcpyDeviceToDevice, g->stream)) != hipSuccess)
                        return hip_code(e);
                }
        if ((rc = phase([&](int r) -> const std::vector<chr::LocalOp>& { return P[r].steps[si].post; })))
            return rc;
    }
    return hip_code(hipStreamSynchronize(g->stream));
}

}  // namespace chr

using namespace chr;

extern "C" {

int chr_local_group_create(chr_local_group** out, int nranks, int device) {
    if (!out || nranks < 1) return CHR_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return CHR_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return CHR_ERR_INVALID_ARG;
    auto g = std::make_unique<chr_local_group>();
    g->nranks = nranks;
    g->device = device;
    g->acc.resize(nranks);
    g->stage.resize(nranks);
    g->prof.span = true;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&g->stream, hipStreamDefault);
    if (e != hipSuccess) return hip_code(e);  // ~chr_local_group releases what was created
    *out = g.release();
    return CHR_SUCCESS;
}

int chr_local_group_destroy(chr_local_group* g) {
    delete g;
    return CHR_SUCCESS;
}

}  // extern "C"
