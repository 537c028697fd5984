// exec_local.cpp -- one rank's local ops on one stream: the fold / tree / copy runner, the batching of a step's trees
// into shared launches (which trees share one is plan_util.hpp's batched_runs), and the argument checks both
// executors make (check_args, resolve_input, is_device_ptr).
#include "exec_internal.hpp"
#include "reduce_tree.hpp"  // only for the limits below

namespace chr {

// The host side's limits are the tree kernel's.
static_assert(kTreeMaxLeaves == kMaxLeaves && kTreeMaxDepth == kTreeDepth, "schedule.hpp restates reduce_tree.hpp");
static_assert(sizeof(TreeJob{}.leaves) / sizeof(void*) == kTreeMaxLeaves, "TreeJob holds one tree's leaves");

namespace {

int run_local(const LocalOp& op, const Bufs& B, int dtype, int rop, hipStream_t s, ReduceProfile& prof) {
    if (op.count == 0) return CHR_SUCCESS;
    if (op.kind == L_COPY) {
        char* d = B.ptr(op.dst);
        const char* src = B.ptr(op.acc);
        if (d == src) return CHR_SUCCESS;
        return hip_code(hipMemcpyAsync(d, src, op.count * B.es, hipMemcpyDeviceToDevice, s));
    }
    if (op.kind == L_COPY2D)
        return hip_code(hipMemcpy2DAsync(B.ptr(op.dst), op.dpitch * B.es, B.ptr(op.acc), op.spitch * B.es,
                                         op.count * B.es, op.rows, hipMemcpyDeviceToDevice, s));
    const bool tree = op.kind == L_TREE;
    std::vector<const void*> ins;
    if (tree) ins.push_back(B.ptr(op.acc));  // leaf 0
    for (const Ref& r : op.ins) ins.push_back(B.ptr(r));
    auto launch = [&] {
        return tree ? reduce_tree_any(B.ptr(op.dst), ins.data(), (int)ins.size(), op.comb.data(),
                                      op.swaps.empty() ? nullptr : op.swaps.data(), op.count, dtype, rop, s)
                    : reduce_any(B.ptr(op.dst), B.ptr(op.acc), ins.data(), (int)ins.size(), op.count, dtype, rop, s,
                                 op.swap);
    };
    if (ins.empty()) return launch();  // a fold of nothing: not a reduction launch
    // algorithmic bytes: every operand read once, the result written once
    return prof.timed(s, (double)(ins.size() + (tree ? 1 : 2)) * op.count * B.es, 1, launch);
}

}  // namespace

double tree_jobs(const std::vector<LocalOp>& ops, size_t i0, size_t i1, const Bufs& B, std::vector<TreeJob>* jobs) {
    double bytes = 0;
    for (size_t i = i0; i < i1; ++i) {
        const LocalOp& op = ops[i];
        if (op.count == 0) continue;
        TreeJob jb{};
        jb.out = B.ptr(op.dst);
        jb.leaves[0] = B.ptr(op.acc);
        for (size_t j = 0; j < op.ins.size(); ++j) jb.leaves[j + 1] = B.ptr(op.ins[j]);
        jb.nl = (int)op.ins.size() + 1;
        jb.comb = op.comb.data();
        jb.swaps = op.swaps.empty() ? nullptr : op.swaps.data();
        jb.n = op.count;
        jobs->push_back(jb);
        bytes += (double)(jb.nl + 1) * op.count * B.es;
    }
    return bytes;
}

Touched touched(const TreeJob& jb, size_t es) {
    Touched t{(const char*)jb.out, {}, jb.nl, jb.n * es};
    for (int j = 0; j < jb.nl; ++j) t.in[j] = (const char*)jb.leaves[j];
    return t;
}

int launch_tree_jobs(const std::vector<TreeJob>& jobs, double bytes, int dtype, int rop, hipStream_t s,
                     ReduceProfile& prof) {
    if (jobs.empty()) return CHR_SUCCESS;
    // vector launches: launch_reduce_tree_multi packs up to kMaxTreeSegs trees of one leaf count per grid
    return prof.timed(s, bytes, (long)((jobs.size() + kMaxTreeSegs - 1) / kMaxTreeSegs),
                      [&] { return reduce_tree_multi_any(jobs.data(), (int)jobs.size(), dtype, rop, s); });
}

int run_locals(const std::vector<LocalOp>& ops, const Bufs& B, int dtype, int rop, hipStream_t s, ReduceProfile& prof) {
    const auto runs = batched_runs(ops, B.es, [&](const Ref& r) { return B.ptr(r); });
    auto run = runs.begin();
    for (size_t i = 0; i < ops.size();) {
        if (run != runs.end() && run->first == i) {
            std::vector<TreeJob> jobs;
            const double bytes = tree_jobs(ops, i, run->second, B, &jobs);
            if (int rc = launch_tree_jobs(jobs, bytes, dtype, rop, s, prof)) return rc;
            i = (run++)->second;
            continue;
        }
        if (int rc = run_local(ops[i++], B, dtype, rop, s, prof)) return rc;
    }
    return CHR_SUCCESS;
}

bool is_device_ptr(const void* p) {
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof(attr));
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// The (dtype, op) pairs a mode accepts: the data-movement collectives (allgather, the stand-alone
// intra scatter) move elements of any type, derived ones included, and ignore op.  A chr_result (check_any).
int check_args(int mode, int dtype, int op) {
    if (mode == MODE_ALLGATHER || mode == MODE_INTRA_SCATTER)
        return elem_size(dtype) != 0 ? CHR_SUCCESS : CHR_ERR_INVALID_ARG;
    return check_any(dtype, op);
}

int resolve_input(int mode, const void* send, void* recv, int rank, size_t count, size_t es, const void** input) {
    *input = send;
    if (send != CHR_IN_PLACE) return CHR_SUCCESS;
    if (mode == MODE_INTER_LINEAR || mode == MODE_INTRA_SCATTER) return CHR_ERR_INVALID_ARG;
    // allgather: the rank's own block already sits in its place of the output
    *input = mode == MODE_ALLGATHER ? (const void*)((char*)recv + (size_t)rank * count * es) : (const void*)recv;
    return CHR_SUCCESS;
}

}  // namespace chr
