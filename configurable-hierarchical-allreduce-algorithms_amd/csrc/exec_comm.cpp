// exec_comm.cpp -- the RCCL executor of one rank: a plan's steps as RCCL groups on the transfer stream with the
// local ops forked onto the compute stream, graph replay of that enqueue, the blocking waits under the communicator's
// timeout (one poll loop), the 4-byte agreement between ranks, and run_collective / collective, which every
// chr_comm entry point goes through.  Also the communicator's lifecycle; its teardown is ~chr_comm.
//
// Messages are RCCL ncclSend/ncclRecv over xGMI.  All k-1 neighbour exchanges of a recexch phase (and all nnodes-1
// lane messages of the inter-node phase) go into ONE ncclGroupStart/End, so the phase drives several xGMI links at once
// (the reference serialises them: all_reduce_radix_batch.cpp:343-367), then ONE fused reduction kernel consumes all
// incoming buckets.  Scratch (ACC, STAGE) is allocated once and reused (the reference mallocs 2x the buffer per call,
// :296-297).
#include <chrono>
#include <thread>

#include "exec_internal.hpp"

namespace chr {

// One RCCL group around post(); a failure inside still closes the group.
template <class Post>
static int rccl_group(Post&& post) {
    int rc = nccl_code(ncclGroupStart());
    if (rc) return rc;
    if ((rc = post())) {
        (void)ncclGroupEnd();
        return rc;
    }
    return nccl_code(ncclGroupEnd());
}

static int enqueue_plan(chr_comm* c, const Plan& p, const void* send, void* recv, int dtype, int op, bool* posted) {
    const size_t es = chr::elem_size(dtype);
    hipError_t e = c->reserve_scratch(p.acc_elems * es, p.stage_elems * es);
    if (e != hipSuccess) return hip_code(e);
    Bufs B{(const char*)send, (char*)recv, (char*)c->acc.p, (char*)c->stage.p, es};
    int rc;
    if ((rc = run_locals(p.pre, B, dtype, op, c->stream, c->prof))) return rc;
    // Transfers on c->stream, local ops on c->cstream.  A step's transfers wait for the local ops of
    // its comm_deps (schedule.cpp analyze_deps), a step's local ops for its own transfers.  The
    // compute stream runs in order, so one wait on the latest dependency (comm_wait) covers every
    // earlier one, and local ops never need to wait for each other.  The call ends with c->stream
    // waiting for the last local ops.
    const bool two = c->overlap && c->cstream;
    int xfer_waited = -1, last_local = -1;
    for (size_t t = 0; t < p.steps.size(); ++t) {
        const chr::Step& s = p.steps[t];
        if (two && s.comm_wait > xfer_waited) {
            hipEvent_t ew = c->event(2 * (size_t)s.comm_wait + 1);
            if (!ew || (rc = hip_code(hipStreamWaitEvent(c->stream, ew, 0)))) return ew ? rc : CHR_ERR_HIP;
            xfer_waited = s.comm_wait;
        }
        const bool xfers = !s.sends.empty() || !s.recvs.empty() || !s.allgathers.empty();
        const bool timed = c->prof.on && xfers;
        std::pair<hipEvent_t, hipEvent_t> sev{nullptr, nullptr};
        if (timed) {
            sev = c->prof.take();
            (void)hipEventRecord(sev.first, c->stream);
        }
        if (xfers) *posted = true;
        if (!s.sends.empty() || !s.recvs.empty())
            rc = rccl_group([&] {
                int r = CHR_SUCCESS;
                for (size_t i = 0; i < s.sends.size() && !r; ++i)
                    r = nccl_code(ncclSend(B.ptr(s.sends[i].ref), s.sends[i].count * es, ncclUint8, s.sends[i].peer,
                                           c->nccl, c->stream));
                for (size_t i = 0; i < s.recvs.size() && !r; ++i)
                    r = nccl_code(ncclRecv(B.ptr(s.recvs[i].ref), s.recvs[i].count * es, ncclUint8, s.recvs[i].peer,
                                           c->nccl, c->stream));
                return r;
            });
        if (!rc && !s.allgathers.empty())  // in place: my block already sits at ref + rank*count
            rc = rccl_group([&] {
                int r = CHR_SUCCESS;
                for (size_t i = 0; i < s.allgathers.size() && !r; ++i) {
                    const Coll& x = s.allgathers[i];
                    char* base = B.ptr(x.ref);
                    r = nccl_code(ncclAllGather(base + (size_t)c->rank * x.count * es, base, x.count * es, ncclUint8,
                                                c->nccl, c->stream));
                }
                return r;
            });
        if (rc) return rc;
        if (timed) {
            (void)hipEventRecord(sev.second, c->stream);
            c->prof.steps_pending.push_back({chr::phase_name(s.label), sev});
        }
        if (s.post.empty()) continue;
        if (!two) {
            if ((rc = run_locals(s.post, B, dtype, op, c->stream, c->prof))) return rc;
            continue;
        }
        hipEvent_t ec = c->event(2 * t), ed = c->event(2 * t + 1);
        if (!ec || !ed) return CHR_ERR_HIP;
        if ((rc = hip_code(hipEventRecord(ec, c->stream))) || (rc = hip_code(hipStreamWaitEvent(c->cstream, ec, 0))))
            return rc;
        {
            // RCCL's kernels run beside these launches: streaming reductions leave them room on every
            // CU (reduce_common.hpp kCoresidentWgPerCu)
            chr::CoresidentScope beside_rccl(c->nranks > 1);
            if ((rc = run_locals(s.post, B, dtype, op, c->cstream, c->prof))) return rc;
        }
        if ((rc = hip_code(hipEventRecord(ed, c->cstream)))) return rc;
        last_local = (int)t;
    }
    if (two && last_local > xfer_waited &&
        (rc = hip_code(hipStreamWaitEvent(c->stream, c->event(2 * (size_t)last_local + 1), 0))))
        return rc;
    return CHR_SUCCESS;
}

// Enqueues a whole plan.  A failure after the first RCCL operation was posted aborts the
// communicator: peers may already be waiting on this rank's messages.
int enqueue_rccl(chr_comm* c, const Plan& p, const void* send, void* recv, int dtype, int op) {
    if (c->failed) return CHR_ERR_ABORTED;
    bool posted = false;
    const int rc = enqueue_plan(c, p, send, recv, dtype, op, &posted);
    if (rc && posted) c->abort_comm();
    return rc;
}

// Graph replay of a device-resident call.  A plan's whole enqueue -- RCCL groups on the transfer
// stream, reductions and copies forked onto the compute stream and joined back by events -- is
// captured once per (plan, buffers) and replayed with one hipGraphLaunch: the host cost of a call
// drops from the RCCL group calls, launches and event records of every step to one launch, which
// is what bounds small messages.  Scratch is sized before capture (no allocation inside it); if
// that grows a buffer, every cached graph is dropped (they point into the old one).
static int launch_graph(chr_comm* c, const Plan& p, const void* send, void* recv, int dtype, int op) {
    const size_t es = chr::elem_size(dtype);
    hipError_t e = c->reserve_scratch(p.acc_elems * es, p.stage_elems * es);
    if (e != hipSuccess) return hip_code(e);
    auto key = std::make_tuple(&p, send, recv, dtype, op, c->overlap);
    auto it = c->gexec.find(key);
    if (it == c->gexec.end()) {
        if (!c->event(2 * p.steps.size() + 1)) return CHR_ERR_HIP;  // the event pool, created outside the capture
        if ((e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal)) != hipSuccess) return hip_code(e);
        const int rc = enqueue_rccl(c, p, send, recv, dtype, op);
        hipGraph_t g = nullptr;
        e = hipStreamEndCapture(c->stream, &g);
        if (rc || e != hipSuccess) {
            if (g) (void)hipGraphDestroy(g);
            return rc ? rc : hip_code(e);
        }
        hipGraphExec_t x = nullptr;
        e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) return hip_code(e);
        it = c->gexec.emplace(key, x).first;
    }
    const int rc = hip_code(hipGraphLaunch(it->second, c->stream));
    if (rc) c->abort_comm();  // the replay may have been partly submitted
    return rc;
}

// Polls `query` (hipStreamQuery / hipEventQuery) until it succeeds or timeout_ms runs out (CHR_ERR_TIMEOUT).  With a
// communicator to `watch`, RCCL's asynchronous error state (a peer that died or closed its connections) is polled
// with it, every millisecond, and an error or the timeout aborts the communicator, so a lost peer becomes an error
// code on every surviving rank instead of a hang.  whole_call (wait_call): a failed query aborts too, and the
// streams are drained after an abort (RCCL's kernels poll the abort flag and exit).
template <class Query>
static int poll_until(Query&& query, int timeout_ms, chr_comm* watch, bool whole_call) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    const auto limit = t0 + std::chrono::milliseconds(timeout_ms);
    auto next_check = t0;
    for (int spin = 0;; ++spin) {
        const hipError_t q = query();
        if (q == hipSuccess) return CHR_SUCCESS;
        if (q != hipErrorNotReady) {
            if (whole_call) watch->abort_comm();
            return hip_code(q);
        }
        const auto now = clk::now();
        ncclResult_t ae = ncclSuccess;
        if (watch && now >= next_check) {
            if (watch->nccl && ncclCommGetAsyncError(watch->nccl, &ae) == ncclSuccess && ae != ncclSuccess &&
                ae != ncclInProgress) {
                watch->abort_comm();
                if (whole_call) (void)hipStreamSynchronize(watch->stream);
                return CHR_ERR_RCCL;
            }
            next_check = now + std::chrono::milliseconds(1);
        }
        if (now >= limit) {
            if (!watch) return CHR_ERR_TIMEOUT;
            if (whole_call && std::getenv("CHR_DEBUG"))
                std::fprintf(stderr, "[chiara] rank %d: call timed out after %d ms, aborting the communicator\n",
                             watch->rank, timeout_ms);
            watch->abort_comm();
            if (whole_call) {
                (void)hipStreamSynchronize(watch->stream);
                (void)hipStreamSynchronize(watch->cstream);
            }
            return CHR_ERR_TIMEOUT;
        }
        if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

// Blocking completion of a call on the communicator stream, under the timeout when one is set.
int wait_call(chr_comm* c) {
    if (c->timeout_ms <= 0) return hip_code(hipStreamSynchronize(c->stream));
    return poll_until([&] { return hipStreamQuery(c->stream); }, c->timeout_ms, c, true);
}

// wait_call for one event.  Used before a copy to or from pageable host memory that depends on a collective: such a
// copy returns only once HIP has staged it, so issued first it would block inside HIP -- beyond the timeout -- if a
// peer is lost.  The issuing thread passes the communicator and may abort it; the copy-out thread passes none: it
// never touches the RCCL communicator (the issuing thread owns it and does any abort) and reports CHR_ERR_TIMEOUT.
int wait_event(hipEvent_t ev, int timeout_ms, chr_comm* watch) {
    if (timeout_ms <= 0) return CHR_SUCCESS;  // no timeout: let the copy itself wait
    return poll_until([&] { return hipEventQuery(ev); }, timeout_ms, watch, false);
}

// One int per rank, the minimum over the ranks, on the communicator stream (blocking, under the
// timeout).  A failure aborts the communicator: the peers are inside the same collective.
// No pageable copy is issued while the exchange may still be pending: such a copy returns only
// once HIP has staged it, i.e. it would wait for the collective inside HIP, past the timeout, if a
// peer never arrives.  The value goes in by a device memset and comes out after wait_call.
int agree_min(chr_comm* c, int mine, int* all) {
    int rc = hip_code(c->flag.reserve(sizeof(int), c->stream));
    int* d = (int*)c->flag.p;
    if (!rc) rc = hip_code(hipMemsetD32Async((hipDeviceptr_t)d, mine, 1, c->stream));
    if (!rc) rc = nccl_code(ncclAllReduce(d, d, 1, ncclInt32, ncclMin, c->nccl, c->stream));
    if (rc) {
        c->abort_comm();
        return rc;
    }
    if ((rc = wait_call(c))) return rc;  // under the timeout; aborts the communicator itself
    rc = hip_code(hipMemcpyAsync(all, d, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (!rc) rc = hip_code(hipStreamSynchronize(c->stream));
    return rc;
}

int run_collective(chr_comm* c, int sched, int slices, int mode, const void* send, void* recv, size_t count, int dtype,
                   int op, int k, int b, bool sync) {
    const Plan& p = c->plan(mode, k, b, count, chr::elem_size(dtype), sched, slices, chr::op_commutative(op));
    if (p.error) return p.error;
    if (p.g.total == 0) return CHR_SUCCESS;
    if (!recv && p.recv_elems) return CHR_ERR_INVALID_ARG;  // a rank whose plan writes no output may pass NULL
    const size_t es = chr::elem_size(dtype);
    const void* input = nullptr;
    if (int rc = resolve_input(mode, send, recv, c->rank, count, es, &input)) return rc;
    if (!input && p.send_elems) return CHR_ERR_INVALID_ARG;  // a rank whose plan reads no input may pass NULL
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_code(e);
    const bool dev_out = is_device_ptr(recv), dev_in = p.send_elems ? is_device_ptr(input) : dev_out;
    // Pipelined staging splits a call into window collectives.  Every rank must issue the same
    // collectives, so whether a call is split cannot depend on where this rank's buffers live alone:
    // a call large enough to split (host_window_elems) first agrees with one 4-byte
    // ncclAllReduce(min) whether every rank is device-resident.  If so, no rank windows (the direct,
    // graph-capable path, which the AUTO tuner also times); otherwise every rank does, a device
    // buffer then being staged device to device.  The exchange costs one small collective on calls of
    // at least one window (32 MiB per rank by default).
    if (sync && host_window_elems(c, mode, count, es)) {
        if (c->failed) return CHR_ERR_ABORTED;
        int all_dev = 0;
        int rc = agree_min(c, dev_in && dev_out, &all_dev);
        if (rc) return rc;
        if (!all_dev && (rc = run_host_windows(c, sched, slices, mode, input, recv, count, dtype, op, k, b)) >= 0)
            return rc;
    }
    if (dev_in && dev_out) {
        // a user op's launcher may allocate stream-ordered scratch: never captured (chiara.h chr_op_create)
        int rc = c->graphs && !c->prof.on && !chr::is_user_op(op) ? launch_graph(c, p, input, recv, dtype, op)
                                                                  : enqueue_rccl(c, p, input, recv, dtype, op);
        if (rc || !sync) return rc;
        return wait_call(c);
    }
    if (!sync) return CHR_ERR_UNSUPPORTED;  // async needs device-resident buffers
    // Host-memory contract of the reference: stage through HBM (PCIe H2D / D2H).  With a timeout
    // set, every copy to or from pageable memory is issued only after what it depends on has
    // completed (wait_call), since such a copy blocks inside HIP until it is staged.
    const void* dsend = input;
    void* drecv = recv;
    int rc;
    if ((rc = wait_call(c))) return rc;  // earlier _async work
    if (!dev_in && p.send_elems) {
        if ((e = c->hsend.reserve(p.send_elems * es, c->stream)) != hipSuccess) return hip_code(e);
        if ((e = hipMemcpyAsync(c->hsend.p, input, p.send_elems * es, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
            return hip_code(e);
        dsend = c->hsend.p;
    }
    if (!dev_out) {
        if ((e = c->hrecv.reserve(p.recv_elems * es, c->stream)) != hipSuccess) return hip_code(e);
        drecv = c->hrecv.p;
    }
    rc = enqueue_rccl(c, p, dsend, drecv, dtype, op);
    if (rc) return rc;
    if (!dev_out && p.recv_elems) {
        if (c->timeout_ms > 0 && (rc = wait_call(c))) return rc;  // the collective, under the timeout
        if ((e = hipMemcpyAsync(recv, drecv, p.recv_elems * es, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
            return hip_code(e);
    }
    return wait_call(c);
}

int collective(chr_comm* c, int mode, const void* send, void* recv, size_t count, int dtype, int op, int k, int b,
               bool sync) {
    // allgather moves elements of any type (its op is unused)
    if (!c) return CHR_ERR_INVALID_ARG;
    if (int rc = check_args(mode, dtype, op)) return rc;
    if (c->failed) return CHR_ERR_ABORTED;
    int sched = c->sched, slices = c->slices;
    if (sched == CHR_SCHEDULE_AUTO) {
        if (hipSetDevice(c->device) != hipSuccess) return CHR_ERR_HIP;
        int rc = tune_schedule(c, mode, send, recv, count, dtype, op, k, b, &sched, &slices);
        if (rc) return rc;
    }
    return run_collective(c, sched, slices, mode, send, recv, count, dtype, op, k, b, sync);
}

}  // namespace chr

using namespace chr;

extern "C" {

int chr_get_unique_id(chr_unique_id* id) {
    static_assert(sizeof(chr_unique_id) == sizeof(ncclUniqueId), "unique id size");
    if (!id) return CHR_ERR_INVALID_ARG;
    ncclUniqueId u;
    int rc = nccl_code(ncclGetUniqueId(&u));
    if (!rc) std::memcpy(id, &u, sizeof(u));
    return rc;
}

int chr_comm_init_rank(chr_comm** out, int nranks, const chr_unique_id* id, int rank, int device) {
    if (!out || !id || nranks < 1 || rank < 0 || rank >= nranks) return CHR_ERR_INVALID_ARG;
    {  // the entry paths set the default (api.cpp); a multi-rank communicator without it is worth a warning
        static bool warned = false;
        const char* ipc = std::getenv("HSA_ENABLE_IPC_MODE_LEGACY");
        if (!warned && nranks > 1 && (!ipc || std::strcmp(ipc, "0") != 0)) {
            std::fprintf(stderr,
                         "[chiara] HSA_ENABLE_IPC_MODE_LEGACY=%s: RCCL's IPC transport needs 0 (dmabuf) on this "
                         "driver; expect hipIpcGetMemHandle failures\n",
                         ipc ? ipc : "(unset)");
            warned = true;
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return CHR_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return CHR_ERR_INVALID_ARG;
    auto c = std::make_unique<chr_comm>();
    c->rank = rank;
    c->nranks = nranks;
    c->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamDefault);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->cstream, hipStreamDefault);
    if (e != hipSuccess) return hip_code(e);  // ~chr_comm releases what was created, here and below
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    if (int rc = nccl_code(ncclCommInitRank(&c->nccl, nranks, u, rank))) return rc;
    *out = c.release();
    return CHR_SUCCESS;
}

int chr_comm_destroy(chr_comm* c) {
    delete c;
    return CHR_SUCCESS;
}

int chr_comm_info(const chr_comm* c, int* rccl_nranks, int* rccl_rank, int* rccl_device, char* pci_bus_id,
                  int len) {
    if (!c || !rccl_nranks || !rccl_rank || !rccl_device || (!pci_bus_id && len > 0) || len < 0)
        return CHR_ERR_INVALID_ARG;
    if (c->failed || !c->nccl) return CHR_ERR_ABORTED;
    // what RCCL's communicator itself holds, not this struct's copy of the init arguments
    int rc = nccl_code(ncclCommCount(c->nccl, rccl_nranks));
    if (!rc) rc = nccl_code(ncclCommUserRank(c->nccl, rccl_rank));
    if (!rc) rc = nccl_code(ncclCommCuDevice(c->nccl, rccl_device));
    if (rc) return rc;
    if (len > 0) {
        pci_bus_id[0] = '\0';
        const hipError_t e = hipDeviceGetPCIBusId(pci_bus_id, len, *rccl_device);
        if (e != hipSuccess) return hip_code(e);
    }
    return CHR_SUCCESS;
}

int chr_comm_abort(chr_comm* c) {
    if (!c) return CHR_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    c->abort_comm();
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->cstream) (void)hipStreamSynchronize(c->cstream);
    return CHR_SUCCESS;
}

int chr_comm_synchronize(chr_comm* c) {
    if (!c) return CHR_ERR_INVALID_ARG;
    if (c->failed) return CHR_ERR_ABORTED;
    if (hipSetDevice(c->device) != hipSuccess) return CHR_ERR_HIP;
    return wait_call(c);
}

}  // extern "C"
