// exec_host_windows.cpp -- pipelined host staging of one chr_comm call: the window size, and the two-thread pipeline
// that copies window j+1 in and window j-1 out while window j is reduced.
#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "exec_internal.hpp"

namespace chr {

// Elements per block of one host window, or 0 when the call is not split (one window would cover
// it, or windows are off): a function of the communicator's setting and the arguments only.
size_t host_window_elems(const chr_comm* c, int mode, size_t count, size_t es) {
    if (c->host_window_mib <= 0 || (mode != chr::MODE_ALLREDUCE && mode != chr::MODE_REDUCE_SCATTER)) return 0;
    const size_t n = (size_t)c->nranks;
    const size_t block = mode == chr::MODE_ALLREDUCE ? count / n : count;  // recvcount
    if (mode == chr::MODE_ALLREDUCE && block * n != count) return 0;       // the plan reports the error
    size_t w = ((size_t)c->host_window_mib << 20) / (n * es);
    w -= w % 64;  // windows start 256 B-aligned within each block when the block is
    return w == 0 || w >= block ? 0 : w;
}

// Pipelined host staging (chr_comm_set_host_pipeline).  An allreduce/reduce-scatter output element
// depends only on the elements at the same offset of every recvcount block (every reduction is
// element-wise, every message block-granular; pinned by test_block_window_property), so a host
// call splits into collectives over windows [off, off + w) of every block, each with the plan for
// n*w (allreduce) or w (reduce-scatter) elements -- the bits of the whole call.  Window j's H2D
// (2-D copy, one row per block) runs on `hin`, its collective on the communicator's streams, its
// D2H on `hout`; two device buffers per direction let window j+1 come in and j-1 go out while j
// is reduced.
//
// The D2H side is issued from a second host thread.  A copy from or to pageable memory (the
// reference harness mallocs its buffers) returns only when HIP has staged it through its own
// pinned bounce buffers, so from one thread the two directions strictly alternate; from two
// threads they overlap (tools/host_stage_probe: 1 GiB each way, 38.2 ms one after the other,
// 22.5 ms from two threads, the same as pinned memory).  The threads hand windows over through
// two counters: the issuing thread publishes "window j's collective is enqueued" (the D2H may then
// wait on ev_coll), the copy-out thread "window j's D2H is enqueued" (a later collective may then
// wait on ev_out before overwriting that window's device buffer).  Returns -1 when the call is
// not split (one window would cover it).
int run_host_windows(chr_comm* c, int sched, int slices, int mode, const void* input, void* recv, size_t count,
                     int dtype, int op, int k, int b) {
    const size_t es = chr::elem_size(dtype), n = (size_t)c->nranks;
    const size_t w = host_window_elems(c, mode, count, es);
    if (w == 0) return -1;
    const size_t block = mode == chr::MODE_ALLREDUCE ? count / n : count;  // recvcount
    hipError_t e = c->host_pipeline_init();
    if (e != hipSuccess) return hip_code(e);
    int rc;
    if ((rc = wait_call(c))) return rc;  // earlier _async work, under the timeout
    const size_t out_rows = mode == chr::MODE_ALLREDUCE ? n : 1;
    for (int i = 0; i < 2; ++i) {
        if ((e = c->wsend[i].reserve(n * w * es, c->stream)) != hipSuccess) return hip_code(e);
        if ((e = c->wrecv[i].reserve(out_rows * w * es, c->stream)) != hipSuccess) return hip_code(e);
    }
    const char* hsrc = (const char*)input;
    char* hdst = (char*)recv;
    const size_t nwin = (block + w - 1) / w;
    const int timeout_ms = c->timeout_ms;

    // Window [off, off + wj) out of device buffer i: on `hout` behind the window's collective, ev_out[i] after it.
    // `waited` is the caller's own wait for that collective -- with a timeout it comes first, since a pageable copy
    // issued before would block inside HIP.
    auto copy_out_window = [&](int i, size_t off, size_t wj, int waited) -> int {
        if (waited) return waited;
        hipError_t ee = hipStreamWaitEvent(c->hout, c->ev_coll[i], 0);
        if (ee == hipSuccess)
            ee = hipMemcpy2DAsync(hdst + off * es, block * es, c->wrecv[i].p, wj * es, wj * es, out_rows,
                                  hipMemcpyDefault, c->hout);
        if (ee == hipSuccess) ee = hipEventRecord(c->ev_out[i], c->hout);
        return hip_code(ee);
    };
    std::mutex mu;
    std::condition_variable cv;
    size_t coll_enqueued = 0, out_enqueued = 0;  // windows handed over, under mu
    bool stop = false;                           // the issuing thread failed: copy-out ends
    int out_rc = CHR_SUCCESS;                    // the copy-out thread's first error
    auto copy_out_loop = [&] {
        if (hipSetDevice(c->device) != hipSuccess) {
            std::lock_guard<std::mutex> g(mu);
            out_rc = CHR_ERR_HIP;
            cv.notify_all();
            return;
        }
        for (size_t j = 0; j < nwin; ++j) {
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&] { return stop || coll_enqueued > j; });
                if (stop) return;
            }
            const int i = (int)(j & 1);
            const size_t off = j * w, wj = std::min(w, block - off);
            const int orc = copy_out_window(i, off, wj, wait_event(c->ev_coll[i], timeout_ms, nullptr));
            std::lock_guard<std::mutex> g(mu);
            if (orc) {
                out_rc = orc;
                cv.notify_all();
                return;
            }
            out_enqueued = j + 1;
            cv.notify_all();
        }
    };
    // The copy-out side runs on a second host thread; if one cannot be started, the issuing loop
    // copies each window out itself right after its collective (no overlap of the two PCIe
    // directions, same bits) -- no exception crosses the C ABI.
    std::thread copy_out;
    try {
        copy_out = std::thread(copy_out_loop);
    } catch (const std::exception&) {  // copy_out stays empty
    }
    const bool threaded = copy_out.joinable();
    auto issue = [&]() -> int {
        for (size_t j = 0; j < nwin; ++j) {
            const int i = (int)(j & 1);
            const size_t off = j * w, wj = std::min(w, block - off);
            // window j reuses window j-2's buffers: its copy-in waits for j-2's collective, and
            // the collective for j-2's copy-out, once the copy-out thread has enqueued it
            if (j >= 2) {
                int r2;
                if ((r2 = wait_event(c->ev_coll[i], timeout_ms, c))) return r2;  // before the pageable copy
                if ((e = hipStreamWaitEvent(c->hin, c->ev_coll[i], 0)) != hipSuccess) return hip_code(e);
            }
            if ((e = hipMemcpy2DAsync(c->wsend[i].p, wj * es, hsrc + off * es, block * es, wj * es, n, hipMemcpyDefault,
                                      c->hin)) != hipSuccess)
                return hip_code(e);
            if ((e = hipEventRecord(c->ev_in[i], c->hin)) != hipSuccess) return hip_code(e);
            if ((e = hipStreamWaitEvent(c->stream, c->ev_in[i], 0)) != hipSuccess) return hip_code(e);
            if (j >= 2) {
                if (threaded) {
                    std::unique_lock<std::mutex> g(mu);
                    auto ready = [&] { return out_rc != CHR_SUCCESS || out_enqueued >= j - 1; };
                    if (timeout_ms > 0) {
                        // the copy-out thread gives up after the same timeout; this is the backstop
                        if (!cv.wait_for(g, std::chrono::milliseconds(2 * (int64_t)timeout_ms + 1000), ready))
                            return CHR_ERR_TIMEOUT;
                    } else {
                        cv.wait(g, ready);
                    }
                    if (out_rc != CHR_SUCCESS) return out_rc;
                }
                if ((e = hipStreamWaitEvent(c->stream, c->ev_out[i], 0)) != hipSuccess) return hip_code(e);
            }
            const Plan& p = c->plan(mode, k, b, mode == chr::MODE_ALLREDUCE ? n * wj : wj, es, sched, slices,
                                    chr::op_commutative(op));
            if (p.error) return p.error;
            int r = enqueue_rccl(c, p, c->wsend[i].p, c->wrecv[i].p, dtype, op);
            if (r) return r;
            if ((e = hipEventRecord(c->ev_coll[i], c->stream)) != hipSuccess) return hip_code(e);
            if (!threaded) {  // this thread copies window j out itself
                if ((r = copy_out_window(i, off, wj, wait_event(c->ev_coll[i], timeout_ms, c)))) return r;
                continue;
            }
            std::lock_guard<std::mutex> g(mu);
            coll_enqueued = j + 1;
            cv.notify_all();
        }
        return CHR_SUCCESS;
    };
    rc = issue();
    if (rc) {
        if (!c->failed && (rc == CHR_ERR_TIMEOUT || rc == CHR_ERR_RCCL)) c->abort_comm();  // peers may be posted
        std::lock_guard<std::mutex> g(mu);
        stop = true;
        cv.notify_all();
    }
    if (!rc) rc = wait_call(c);  // the last collective, under the communicator's timeout
    if (threaded) copy_out.join();
    const int rc_out = hip_code(hipStreamSynchronize(c->hout));
    if (rc) return rc;
    if (out_rc && !c->failed) c->abort_comm();  // the copy-out side timed out: peers may still be posted
    return out_rc ? out_rc : rc_out;
}

}  // namespace chr
