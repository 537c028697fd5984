// exec_tune.cpp -- what a call runs with when the caller did not say: the environment's defaults, the pipeline depth
// (pick_slices) and CHR_SCHEDULE_AUTO's measured choice of schedule and depth (tune_schedule, chr_comm_tuned_schedule).
#include <algorithm>

#include "exec_internal.hpp"

namespace chr {

// The environment's defaults, each read once.
static int env_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}
// CHR_OVERLAP=0: local ops on the transfer stream (no compute/xGMI overlap); default 1
int default_overlap() { static const int v = env_int("CHR_OVERLAP", 1) != 0; return v; }
// CHR_LG_BATCH=0: a local group launches each virtual rank's trees separately; default 1
int default_lg_batch() { static const int v = env_int("CHR_LG_BATCH", 1) != 0; return v; }
// CHR_GRAPHS=1: device-resident collectives replay a captured HIP graph per (plan, buffers)
int default_graphs() { static const int v = env_int("CHR_GRAPHS", 0) != 0; return v; }
// CHR_HOST_WINDOW_MIB: host-memory calls are staged in windows of this many MiB (0 = off, the default); see
// chr_comm_set_host_pipeline
int default_host_window_mib() { static const int v = std::max(0, env_int("CHR_HOST_WINDOW_MIB", 0)); return v; }
// CHR_TIMEOUT_MS: blocking calls give up after this many milliseconds (0 = wait forever, the
// default); see chr_comm_set_timeout
int default_timeout_ms() { static const int v = env_int("CHR_TIMEOUT_MS", 0); return v; }
// CHR_SCHEDULE = reference | balanced | flat | exact | flat_ag | flat_seq | flat_1shot | auto (or 0 .. 7); default flat
int default_schedule() {
    static const int v = [] {
        const char* e = std::getenv("CHR_SCHEDULE");
        const std::pair<const char*, int> names[] = {
            {"reference", SCHED_REFERENCE}, {"balanced", SCHED_BALANCED}, {"exact", SCHED_EXACT},
            {"flat_ag", SCHED_FLAT_AG},     {"flat_seq", SCHED_FLAT_SEQ}, {"flat_1shot", SCHED_FLAT_1SHOT},
            {"auto", CHR_SCHEDULE_AUTO}};
        for (const auto& nm : names)  // by name or by number
            if (e && (std::string(e) == nm.first || std::string(e) == std::to_string(nm.second))) return nm.second;
        return (int)SCHED_FLAT;
    }();
    return v;
}

// Pipeline depth: explicit setting, else CHR_SLICES, else by chunk size (schedule.cpp auto_slices).
// The flat schedules evaluate one piece per (chunk, rank) per slice -- chunk/n elements (allreduce)
// or the rank's own block (reduce-scatter), divided by the depth -- in batched tree launches whose
// fixed fill/drain cost dominates small pieces (profiles/r02/tree_bench_batched.json, C4's two
// 8-leaf trees per slice: 8 MiB pieces 0.58-0.63 of the HBM peak, 16 MiB 0.68-0.77), so their
// default depth keeps pieces at 16 MiB or more.  CHR_SCHEDULE_AUTO still times every depth from
// the chunk-size one down.
constexpr uint64_t kMinFlatPieceBytes = (uint64_t)16 << 20;

// SCHED_FLAT_1SHOT moves (n-1) S per rank instead of 2 (n-1)/n S: a latency trade for small calls.  AUTO
// times it only up to this many bytes per rank (8 GPUs at ~350 GB/s of xGMI per direction: the
// extra 1.75 S costs one RCCL group's ~15 us of latency near S = 3 MB).
constexpr uint64_t kOneShotMaxBytes = (uint64_t)8 << 20;

int pick_slices(int setting, uint64_t count, int mode, int nranks, int b, size_t es, int sched) {
    if (chr::is_unpipelined(mode)) return 1;  // unpipelined schedules
    if (setting > 0) return setting;
    static const int env = env_int("CHR_SLICES", 0);
    if (env > 0) return env;
    const uint64_t n = (uint64_t)(nranks > 0 ? nranks : 1);
    const uint64_t recvcount = mode == chr::MODE_ALLREDUCE ? count / n : count;
    const uint64_t irc_bytes = recvcount * (uint64_t)(b > 0 ? b : 1) * es;
    int P = chr::auto_slices(irc_bytes);
    if (flat_family(sched)) {
        const uint64_t piece = mode == chr::MODE_ALLREDUCE && sched != chr::SCHED_FLAT_1SHOT ? irc_bytes / n
                               : mode == chr::MODE_ALLREDUCE                                ? irc_bytes
                                                                                            : recvcount * es;
        const int cap = (int)std::max<uint64_t>(1, piece / kMinFlatPieceBytes);
        P = std::min(P, cap);
    }
    return P;
}

// CHR_SCHEDULE_AUTO.  The single-node schedules FLAT, FLAT_SEQ and FLAT_AG move the same bits
// over the same full-mesh traffic (2S/n per link) but differ in how RCCL groups and collectives
// share the links, and the pipeline depth trades overlap against per-group latency; which is
// fastest is a property of the machine, so on the first device-resident call for a given
// (collective, count, dtype, k, b) every candidate runs TUNE_REPS timed calls, the ranks agree on
// the slowest rank's time per candidate (one ncclAllReduce(max), so every rank picks the same
// one) and the fastest is kept for every later call.  Each tuning call is a complete collective;
// an in-place call is tuned on temporary copies so the caller's data is reduced exactly once.
//
// Tuning is collective, so every decision that could differ between ranks is agreed on first:
// whether this call can be tuned (device-resident buffers, the temporaries allocated) is one
// ncclAllReduce(min) over the ranks, and a call no rank can tune runs FLAT untuned on every rank.
// The cache is then identical on every rank, and a cached choice applies to later calls of the
// same arguments whatever memory their buffers are in.  A candidate that fails after posting
// RCCL operations aborts the communicator (enqueue_rccl); peers with a timeout (chr_comm_set_timeout)
// then return an error instead of waiting.
constexpr int TUNE_REPS = 3;

int tune_schedule(chr_comm* c, int mode, const void* send, void* recv, size_t count, int dtype, int op, int k, int b,
                  int* sched_out, int* slices_out) {
    *sched_out = chr::SCHED_FLAT;
    *slices_out = c->slices;
    if (chr::is_unpipelined(mode) || c->nranks < 2) return CHR_SUCCESS;
    if (c->failed) return CHR_ERR_ABORTED;
    const size_t es = chr::elem_size(dtype);
    auto key = std::make_tuple(mode, (uint64_t)count, (int)es, k, b, c->slices, c->overlap);
    auto it = c->tuned.find(key);
    if (it != c->tuned.end()) {
        *sched_out = it->second.first;
        *slices_out = it->second.second;
        return CHR_SUCCESS;
    }
    const Plan& p0 = c->plan(mode, k, b, count, es, chr::SCHED_FLAT, c->slices, chr::op_commutative(op));
    if (p0.error) return p0.error;  // a function of the arguments only: the same on every rank
    if (p0.g.total == 0) return CHR_SUCCESS;
    const bool inplace = send == CHR_IN_PLACE;
    const void* input = nullptr;
    if (int rc = resolve_input(mode, send, recv, c->rank, count, es, &input)) return rc;
    // in place: tune on copies (the collective would otherwise reduce the caller's data again)
    void* tsend = nullptr;
    void* trecv = nullptr;
    const void* s_arg = send;
    void* r_arg = recv;
    int ok = input && recv && is_device_ptr(input) && is_device_ptr(recv);
    if (ok && inplace) {
        ok = hipMalloc(&tsend, p0.send_elems * es) == hipSuccess && hipMalloc(&trecv, p0.recv_elems * es) == hipSuccess &&
             hipMemcpyAsync(tsend, recv, p0.send_elems * es, hipMemcpyDeviceToDevice, c->stream) == hipSuccess;
        (void)hipGetLastError();
        s_arg = tsend;
        r_arg = trecv;
    }
    auto release = [&]() {
        if (tsend || trecv) (void)hipStreamSynchronize(c->stream);
        (void)hipFree(tsend);
        (void)hipFree(trecv);
    };
    int all = 0;
    int rc = agree_min(c, ok, &all);
    if (rc || !all) {  // host-staged somewhere, or an allocation failed somewhere: FLAT, untuned
        release();
        return rc;
    }
    std::vector<std::pair<int, int>> cand;
    std::vector<int> depths;
    const int pa = pick_slices(c->slices, count, mode, c->nranks, b, es, chr::SCHED_REFERENCE);  // chunk-size depth
    for (int d = pa; d >= 1; d /= 2) {
        depths.push_back(d);
        if (c->slices > 0) break;  // an explicit depth is kept
    }
    for (int sc : {(int)chr::SCHED_FLAT, (int)chr::SCHED_FLAT_SEQ, (int)chr::SCHED_FLAT_AG})
        for (int d : depths) cand.push_back({sc, d});
    if (mode == chr::MODE_ALLREDUCE && (uint64_t)count * es <= kOneShotMaxBytes)
        for (int d : depths) cand.push_back({(int)chr::SCHED_FLAT_1SHOT, d});
    std::vector<float> ms(cand.size(), 0.f);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipSuccess;
    if ((e = hipEventCreate(&e0)) != hipSuccess || (e = hipEventCreate(&e1)) != hipSuccess) {
        rc = hip_code(e);
        c->abort_comm();  // the peers are about to start the candidates
    }
    for (size_t i = 0; i < cand.size() && !rc; ++i) {
        const int sc = cand[i].first, d = cand[i].second;
        // untimed first call: plan compile, scratch growth, RCCL connection setup
        if ((rc = run_collective(c, sc, d, mode, s_arg, r_arg, count, dtype, op, k, b, true))) break;
        if ((rc = hip_code(hipEventRecord(e0, c->stream)))) break;
        for (int r = 0; r < TUNE_REPS && !rc; ++r)
            rc = run_collective(c, sc, d, mode, s_arg, r_arg, count, dtype, op, k, b, false);
        if (rc || (rc = hip_code(hipEventRecord(e1, c->stream))) || (rc = wait_call(c))) break;
        rc = hip_code(hipEventElapsedTime(&ms[i], e0, e1));
    }
    if (rc && !c->failed) c->abort_comm();  // a local failure mid-tuning: the peers are still in it
    float* dms = nullptr;
    if (!rc && (rc = hip_code(hipMalloc(&dms, ms.size() * sizeof(float)))) == CHR_SUCCESS) {
        if (!(rc = hip_code(hipMemcpyAsync(dms, ms.data(), ms.size() * sizeof(float), hipMemcpyHostToDevice,
                                           c->stream))) &&
            !(rc = nccl_code(ncclAllReduce(dms, dms, ms.size(), ncclFloat32, ncclMax, c->nccl, c->stream))) &&
            !(rc = hip_code(hipMemcpyAsync(ms.data(), dms, ms.size() * sizeof(float), hipMemcpyDeviceToHost,
                                           c->stream))))
            rc = wait_call(c);
        if (rc && !c->failed) c->abort_comm();
    } else if (rc == CHR_ERR_OUT_OF_MEMORY && !c->failed) {
        c->abort_comm();
    }
    (void)hipFree(dms);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    release();
    if (rc) return rc;
    size_t best = 0;
    for (size_t i = 1; i < cand.size(); ++i)
        if (ms[i] < ms[best]) best = i;
    if (std::getenv("CHR_TUNE_VERBOSE") && c->rank == 0)
        for (size_t i = 0; i < cand.size(); ++i)
            std::fprintf(stderr, "[chiara] tune mode %d count %zu: schedule %d slices %d  %.3f ms%s\n", mode, count,
                         cand[i].first, cand[i].second, ms[i] / TUNE_REPS, i == best ? "  <- kept" : "");
    c->tuned[key] = cand[best];
    *sched_out = cand[best].first;
    *slices_out = cand[best].second;
    return CHR_SUCCESS;
}

}  // namespace chr

extern "C" int chr_comm_tuned_schedule(const chr_comm* c, int mode, size_t count, chr_dtype dtype, int k, int b,
                                       int* schedule, int* slices) {
    if (!c || !schedule || !slices || !chr::elem_size(dtype)) return CHR_ERR_INVALID_ARG;
    if (mode != chr::MODE_ALLREDUCE && mode != chr::MODE_REDUCE_SCATTER) return CHR_ERR_INVALID_ARG;
    if (c->failed) return CHR_ERR_ABORTED;
    if (c->sched != CHR_SCHEDULE_AUTO) {  // a fixed schedule: it, at the depth such a call runs
        const int P =
            chr::pick_slices(c->slices, (uint64_t)count, mode, c->nranks, b, chr::elem_size(dtype), c->sched);
        // the arguments a call would reject (k < 2, nranks % b, count % nranks) are rejected here too
        const chr::Plan p = chr::build_plan((chr::Mode)mode, c->nranks, c->rank, k, b, (uint64_t)count, P, c->sched);
        if (p.error) return p.error;
        *schedule = c->sched;
        *slices = P;
        return CHR_SUCCESS;
    }
    auto it = c->tuned.find(std::make_tuple(mode, (uint64_t)count, (int)chr::elem_size(dtype), k, b, c->slices,
                                            c->overlap));
    if (it == c->tuned.end()) return CHR_ERR_INVALID_ARG;
    *schedule = it->second.first;
    *slices = it->second.second;
    return CHR_SUCCESS;
}
