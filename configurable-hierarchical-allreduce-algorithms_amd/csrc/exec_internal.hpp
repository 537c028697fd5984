// exec_internal.hpp -- what the executor's translation units (exec_*.cpp) share: the device buffers and their
// resolution, the reduction profile, the two executor objects (chr_comm: one rank per process/GPU over RCCL;
// chr_local_group: n virtual ranks on one device), the RCCL status mapping, and the prototypes of what one unit
// calls in another.  Nothing here is exported from libchiara.so.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "chr_internal.hpp"
#include "plan_util.hpp"
#include "user_ops.hpp"

#pragma GCC visibility push(hidden)

namespace chr {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    // Grows (never shrinks).  The caller has synchronised the stream before a regrow.
    hipError_t reserve(size_t want, hipStream_t s) {
        if (want <= bytes) return hipSuccess;
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        release();
        e = hipMalloc(&p, want);
        if (e == hipSuccess) bytes = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

struct Bufs {
    const char* send;
    char* recv;
    char* acc;
    char* stage;
    size_t es;
    char* ptr(const Ref& r) const {
        char* base = r.buf == BUF_SEND   ? const_cast<char*>(send)
                     : r.buf == BUF_RECV ? recv
                     : r.buf == BUF_ACC  ? acc
                                         : stage;
        return base + r.off * es;
    }
};

inline int nccl_code(ncclResult_t r) {
    if (r == ncclSuccess) return CHR_SUCCESS;
    if (std::getenv("CHR_DEBUG")) std::fprintf(stderr, "[chiara] RCCL error: %s\n", ncclGetErrorString(r));
    return CHR_ERR_RCCL;
}

// Opt-in timing of the fused reduction launches (chr_comm_profile): HIP events on the
// launch stream around each reduction, summed when read.
struct ReduceProfile {
    using Events = std::pair<hipEvent_t, hipEvent_t>;
    bool on = false;
    // span: the caller brackets whole phases with events and the launches only add their algorithmic bytes and
    // count -- the local group's mode, whose launches may run on two streams at once
    bool span = false;
    std::vector<Events> pending, spare;
    double ms = 0, bytes = 0;
    long launches = 0;
    // per-phase transfer time (the reference's DEBUG_MODE phase timers, all_reduce_radix_batch.cpp
    // :228-232, :480-489, :542-548, :572-578, :758-764): events around each step's RCCL group on
    // the transfer stream, summed per phase name (the step label without slice suffixes)
    std::vector<std::pair<std::string, Events>> steps_pending;
    std::map<std::string, double> phase_ms;
    Events take() {
        if (!spare.empty()) {
            auto e = spare.back();
            spare.pop_back();
            return e;
        }
        Events e{nullptr, nullptr};
        (void)hipEventCreate(&e.first);
        (void)hipEventCreate(&e.second);
        return e;
    }
    // Events on s around fn() when `want`, for drain() to sum.
    template <class Fn>
    int bracket(bool want, hipStream_t s, Fn&& fn) {
        if (!want) return fn();
        const Events ev = take();
        (void)hipEventRecord(ev.first, s);
        const int rc = fn();
        (void)hipEventRecord(ev.second, s);
        pending.push_back(ev);
        return rc;
    }
    // `launch()` enqueues reductions on s: nlaunches grids moving nbytes algorithmic bytes, bracketed unless the
    // caller brackets whole phases itself.
    template <class Fn>
    int timed(hipStream_t s, double nbytes, long nlaunches, Fn&& launch) {
        const int rc = bracket(on && !span, s, launch);
        if (on) bytes += nbytes, launches += nlaunches;
        return rc;
    }
    void drain() {
        auto elapsed = [&](const Events& e, double* sum) {
            float t = 0;
            if (hipEventSynchronize(e.second) == hipSuccess && hipEventElapsedTime(&t, e.first, e.second) == hipSuccess)
                *sum += t;
            spare.push_back(e);
        };
        for (auto& e : pending) elapsed(e, &ms);
        pending.clear();
        for (auto& s : steps_pending) elapsed(s.second, &phase_ms[s.first]);
        steps_pending.clear();
    }
    // chr_comm_profile_read / chr_local_group_profile_read
    void read(double* reduce_ms, double* reduce_bytes, long* nlaunches, int reset) {
        drain();
        if (reduce_ms) *reduce_ms = ms;
        if (reduce_bytes) *reduce_bytes = bytes;
        if (nlaunches) *nlaunches = launches;
        if (reset) ms = bytes = 0, launches = 0;
    }
    // chr_comm_profile_phases: "name ms\n" per phase; the length of the whole text
    long phases(char* buf, size_t len, int reset) {
        drain();
        std::string s;
        char line[160];
        for (const auto& kv : phase_ms) {
            std::snprintf(line, sizeof line, "%s %.6f\n", kv.first.c_str(), kv.second);
            s += line;
        }
        if (buf && len) {
            const size_t n = s.size() < len - 1 ? s.size() : len - 1;
            std::memcpy(buf, s.data(), n);
            buf[n] = '\0';
        }
        if (reset) phase_ms.clear();
        return (long)s.size();
    }
    void release() {
        drain();
        for (auto& e : spare) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
        spare.clear();
    }
};

// mode, rank, k, b, count, dtype size, slices, schedule, op commutative (the MPICH baselines branch on it)
using PlanKey = std::tuple<int, int, int, int, uint64_t, int, int, int, bool>;

// exec_tune.cpp: the environment's defaults and the pipeline depth
int default_schedule(), default_overlap(), default_lg_batch(), default_graphs(), default_host_window_mib(),
    default_timeout_ms();
int pick_slices(int setting, uint64_t count, int mode, int nranks, int b, size_t es, int sched);

// exec_local.cpp: local ops of one rank on one stream
bool is_device_ptr(const void* p);
int check_args(int mode, int dtype, int op);
// Where rank `rank` reads its input: `send`, or under CHR_IN_PLACE its place in `recv` (CHR_ERR_INVALID_ARG for the
// modes that have no in-place form).
int resolve_input(int mode, const void* send, void* recv, int rank, size_t count, size_t es, const void** input);
int run_locals(const std::vector<LocalOp>& ops, const Bufs& B, int dtype, int rop, hipStream_t s, ReduceProfile& prof);
// The tree ops [i0, i1) as resolved jobs for one batched launch; returns their algorithmic bytes.
double tree_jobs(const std::vector<LocalOp>& ops, size_t i0, size_t i1, const Bufs& B, std::vector<TreeJob>* jobs);
Touched touched(const TreeJob& jb, size_t es);
int launch_tree_jobs(const std::vector<TreeJob>& jobs, double bytes, int dtype, int rop, hipStream_t s,
                     ReduceProfile& prof);

}  // namespace chr

struct chr_comm {
    int rank = 0, nranks = 0, device = 0;
    int slices = 0;  // 0 = auto
    int sched = chr::default_schedule();
    int overlap = chr::default_overlap();
    ncclComm_t nccl = nullptr;
    hipStream_t stream = nullptr;   // RCCL transfers; the call completes on this stream
    hipStream_t cstream = nullptr;  // local ops (reductions, copies) when overlapping
    std::vector<hipEvent_t> events;  // pool: 2 per step
    hipEvent_t event(size_t i) {
        while (events.size() <= i) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
            events.push_back(e);
        }
        return events[i];
    }
    chr::DevBuf acc, stage, hsend, hrecv, flag;  // flag: agree_min's 4-byte exchange
    chr::ReduceProfile prof;
    std::map<chr::PlanKey, std::unique_ptr<chr::Plan>> plans;

    // Pipelined host staging (chr_comm_set_host_pipeline): copy-in and copy-out streams, two
    // device window buffers per direction, and the events that order them against the collective.
    int host_window_mib = chr::default_host_window_mib();
    hipStream_t hin = nullptr, hout = nullptr;
    chr::DevBuf wsend[2], wrecv[2];
    hipEvent_t ev_in[2] = {}, ev_coll[2] = {}, ev_out[2] = {};
    hipError_t host_pipeline_init() {
        if (hin) return hipSuccess;
        hipError_t e = hipStreamCreateWithFlags(&hin, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&hout, hipStreamNonBlocking);
        for (int i = 0; i < 2 && e == hipSuccess; ++i) {
            e = hipEventCreateWithFlags(&ev_in[i], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_coll[i], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_out[i], hipEventDisableTiming);
        }
        return e;
    }
    void host_pipeline_release() {
        if (hin) (void)hipStreamSynchronize(hin);
        if (hout) (void)hipStreamSynchronize(hout);
        for (int i = 0; i < 2; ++i) {
            wsend[i].release();
            wrecv[i].release();
            for (hipEvent_t* e : {&ev_in[i], &ev_coll[i], &ev_out[i]})
                if (*e) (void)hipEventDestroy(*e);
        }
        if (hin) (void)hipStreamDestroy(hin);
        if (hout) (void)hipStreamDestroy(hout);
        hin = hout = nullptr;
    }

    // Failure handling.  A call that fails after it has posted RCCL operations, or that times
    // out, aborts the RCCL communicator (ncclCommAbort: its kernels exit, peers see the closed
    // connections) instead of leaving peers posted; every later call then returns
    // CHR_ERR_ABORTED and the destructor skips ncclCommDestroy, which could block on a wedged
    // communicator.  The reference has no such path: under MPI_ERRORS_ARE_FATAL an error aborts
    // the job, and a lost peer is a hang.
    int timeout_ms = chr::default_timeout_ms();
    bool failed = false;
    void abort_comm() {
        if (nccl) (void)ncclCommAbort(nccl);
        nccl = nullptr;
        failed = true;
    }

    // HIP graph replay (chr_comm_set_graphs): one executable graph per (plan, send, recv, dtype, op, overlap),
    // dropped whenever the scratch buffers they point into are reallocated
    int graphs = chr::default_graphs();
    std::map<std::tuple<const chr::Plan*, const void*, void*, int, int, int>, hipGraphExec_t> gexec;
    void drop_graphs() {
        for (auto& kv : gexec) (void)hipGraphExecDestroy(kv.second);
        gexec.clear();
    }
    // The only way scratch grows: whichever path reserves it (eager, graph capture, host-staged,
    // profiled, tuning), a reallocation drops every cached graph, since they point into the old
    // buffers.  reserve() synchronises the stream first, so no replay is still running.
    hipError_t reserve_scratch(size_t acc_bytes, size_t stage_bytes) {
        const void* a0 = acc.p;
        const void* s0 = stage.p;
        hipError_t e = acc.reserve(acc_bytes, stream);
        if (e == hipSuccess) e = stage.reserve(stage_bytes, stream);
        if (acc.p != a0 || stage.p != s0) drop_graphs();
        return e;
    }
    // CHR_SCHEDULE_AUTO: (mode, count, element size, k, b, slices setting, overlap) -> (schedule, depth)
    std::map<std::tuple<int, uint64_t, int, int, int, int, int>, std::pair<int, int>> tuned;

    const chr::Plan& plan(int mode, int k, int b, uint64_t count, size_t es, int sched_, int slices_, bool commutative) {
        const int P = chr::pick_slices(slices_, count, mode, nranks, b, es, sched_);
        chr::PlanKey key{mode, rank, k, b, count, (int)es, P, sched_, commutative};
        auto it = plans.find(key);
        if (it == plans.end())
            it = plans.emplace(key, std::make_unique<chr::Plan>(chr::build_plan((chr::Mode)mode, nranks, rank, k, b,
                                                                                count, P, sched_, commutative)))
                     .first;
        return *it->second;
    }

    // What a communicator holds, whatever part of it chr_comm_init_rank got to create.
    ~chr_comm() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        drop_graphs();
        prof.release();
        if (nccl) (void)ncclCommDestroy(nccl);  // an aborted communicator was released by ncclCommAbort
        for (chr::DevBuf* d : {&acc, &stage, &hsend, &hrecv, &flag}) d->release();
        host_pipeline_release();
        if (cstream) (void)hipStreamSynchronize(cstream);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        if (cstream) (void)hipStreamDestroy(cstream);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct chr_local_group {
    int nranks = 0, device = 0;
    // chr_local_group_profile: the fused reductions of every rank, timed as whole phases (from the
    // end of a step's copies to the join of its reductions) with HIP events on the group's stream
    chr::ReduceProfile prof;
    int slices = 0;  // 0 = auto
    // chr_local_group_set_batching: the virtual ranks' tree evaluations of one step share launches
    // (CHR_LG_BATCH=0 turns it off; default on)
    int batch_ranks = chr::default_lg_batch();
    int sched = chr::default_schedule() == CHR_SCHEDULE_AUTO ? (int)chr::SCHED_FLAT : chr::default_schedule();  // no tuning
    hipStream_t stream = nullptr;
    std::vector<chr::DevBuf> acc, stage;
    std::map<std::tuple<int, int, int, uint64_t, int, int, int, bool>, std::vector<chr::Plan>> plans;

    ~chr_local_group() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        prof.release();
        for (auto& d : acc) d.release();
        for (auto& d : stage) d.release();
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace chr {

// exec_comm.cpp
int enqueue_rccl(chr_comm* c, const Plan& p, const void* send, void* recv, int dtype, int op);
int wait_call(chr_comm* c);
int wait_event(hipEvent_t ev, int timeout_ms, chr_comm* watch);
int agree_min(chr_comm* c, int mine, int* all);
int run_collective(chr_comm* c, int sched, int slices, int mode, const void* send, void* recv, size_t count, int dtype,
                   int op, int k, int b, bool sync);
int collective(chr_comm* c, int mode, const void* send, void* recv, size_t count, int dtype, int op, int k, int b,
               bool sync);
// exec_host_windows.cpp
size_t host_window_elems(const chr_comm* c, int mode, size_t count, size_t es);
int run_host_windows(chr_comm* c, int sched, int slices, int mode, const void* input, void* recv, size_t count,
                     int dtype, int op, int k, int b);
// exec_tune.cpp
int tune_schedule(chr_comm* c, int mode, const void* send, void* recv, size_t count, int dtype, int op, int k, int b,
                  int* sched_out, int* slices_out);
// exec_local_group.cpp
int local_collective(chr_local_group* g, int mode, const void* const* sends, void* const* recvs, size_t count,
                     int dtype, int op, int k, int b);

}  // namespace chr

#pragma GCC visibility pop
