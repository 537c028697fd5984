// exec_api.cpp -- the thin extern "C" layer over the two executors: getters and setters of chr_comm and
// chr_local_group, profile read-out, and the collective entry points, each one call of collective() (exec_comm.cpp) or
// local_collective() (exec_local_group.cpp) with its mode.
#include "exec_internal.hpp"

using namespace chr;

// A setting: the object exists and the value is one it takes.  A reading: the object and the place for it exist.
template <class T, class V>
static int set(T* obj, bool valid, V T::*field, V value) {
    if (!obj || !valid) return CHR_ERR_INVALID_ARG;
    obj->*field = value;
    return CHR_SUCCESS;
}
template <class T, class V>
static int get(const T* obj, V T::*field, V* out) {
    if (!obj || !out) return CHR_ERR_INVALID_ARG;
    *out = obj->*field;
    return CHR_SUCCESS;
}
// Profiling of either executor: on / off, and the read-out of ReduceProfile.
template <class T>
static int profile_on(T* obj, int enable) {
    if (!obj) return CHR_ERR_INVALID_ARG;
    obj->prof.on = enable != 0;
    return CHR_SUCCESS;
}
template <class T>
static int profile_read(T* obj, double* reduce_ms, double* reduce_bytes, long* launches, int reset) {
    if (!obj) return CHR_ERR_INVALID_ARG;
    (void)hipSetDevice(obj->device);
    obj->prof.read(reduce_ms, reduce_bytes, launches, reset);
    return CHR_SUCCESS;
}

extern "C" {

int chr_comm_rank(const chr_comm* c, int* rank) { return get(c, &chr_comm::rank, rank); }
int chr_comm_size(const chr_comm* c, int* n) { return get(c, &chr_comm::nranks, n); }
int chr_comm_stream(const chr_comm* c, hipStream_t* s) { return get(c, &chr_comm::stream, s); }
int chr_comm_get_overlap(const chr_comm* c, int* enable) { return get(c, &chr_comm::overlap, enable); }
int chr_comm_is_aborted(const chr_comm* c) { return c && c->failed ? 1 : 0; }

int chr_comm_set_timeout(chr_comm* c, int ms) { return set(c, ms >= 0, &chr_comm::timeout_ms, ms); }
int chr_comm_set_slices(chr_comm* c, int slices) { return set(c, slices >= 0, &chr_comm::slices, slices); }
int chr_comm_set_overlap(chr_comm* c, int enable) { return set(c, true, &chr_comm::overlap, (int)(enable != 0)); }
int chr_comm_set_host_pipeline(chr_comm* c, int mib) { return set(c, mib >= 0, &chr_comm::host_window_mib, mib); }
int chr_comm_set_schedule(chr_comm* c, int schedule) {
    return set(c, plan_schedule(schedule) || schedule == CHR_SCHEDULE_AUTO, &chr_comm::sched, schedule);
}

int chr_comm_set_graphs(chr_comm* c, int enable) {
    if (!c) return CHR_ERR_INVALID_ARG;
    if (!enable && c->stream) {
        (void)hipStreamSynchronize(c->stream);
        c->drop_graphs();
    }
    c->graphs = enable != 0;
    return CHR_SUCCESS;
}

int chr_comm_profile(chr_comm* c, int enable) { return profile_on(c, enable); }
int chr_comm_profile_read(chr_comm* c, double* reduce_ms, double* reduce_bytes, long* launches, int reset) {
    return profile_read(c, reduce_ms, reduce_bytes, launches, reset);
}
long chr_comm_profile_phases(chr_comm* c, char* buf, size_t len, int reset) {
    if (!c) return -1;
    (void)hipSetDevice(c->device);
    return c->prof.phases(buf, len, reset);
}

int chr_local_group_stream(const chr_local_group* g, hipStream_t* s) { return get(g, &chr_local_group::stream, s); }
int chr_local_group_set_slices(chr_local_group* g, int slices) {
    return set(g, slices >= 0, &chr_local_group::slices, slices);
}
int chr_local_group_set_schedule(chr_local_group* g, int schedule) {
    return set(g, plan_schedule(schedule), &chr_local_group::sched, schedule);
}
int chr_local_group_set_batching(chr_local_group* g, int enable) {
    return set(g, true, &chr_local_group::batch_ranks, (int)(enable != 0));
}

int chr_local_group_profile(chr_local_group* g, int enable) { return profile_on(g, enable); }
int chr_local_group_profile_read(chr_local_group* g, double* reduce_ms, double* reduce_bytes, long* launches,
                                 int reset) {
    return profile_read(g, reduce_ms, reduce_bytes, launches, reset);
}

int chr_allreduce_radix_batch(const void* send, void* recv, size_t count, chr_dtype dtype, chr_op op, chr_comm* comm,
                              int k, int b) {
    return collective(comm, chr::MODE_ALLREDUCE, send, recv, count, dtype, op, k, b, true);
}

int chr_reduce_scatter_radix_batch(const void* send, void* recv, size_t recvcount, chr_dtype dtype, chr_op op,
                                   chr_comm* comm, int k, int b) {
    return collective(comm, chr::MODE_REDUCE_SCATTER, send, recv, recvcount, dtype, op, k, b, true);
}

int chr_allreduce_radix_batch_async(const void* send, void* recv, size_t count, chr_dtype dtype, chr_op op,
                                    chr_comm* comm, int k, int b) {
    return collective(comm, chr::MODE_ALLREDUCE, send, recv, count, dtype, op, k, b, false);
}

int chr_reduce_scatter_radix_batch_async(const void* send, void* recv, size_t recvcount, chr_dtype dtype, chr_op op,
                                         chr_comm* comm, int k, int b) {
    return collective(comm, chr::MODE_REDUCE_SCATTER, send, recv, recvcount, dtype, op, k, b, false);
}

int chr_local_allreduce_radix_batch(chr_local_group* g, const void* const* sends, void* const* recvs, size_t count,
                                    chr_dtype dtype, chr_op op, int k, int b) {
    return local_collective(g, chr::MODE_ALLREDUCE, sends, recvs, count, dtype, op, k, b);
}

int chr_local_reduce_scatter_radix_batch(chr_local_group* g, const void* const* sends, void* const* recvs,
                                         size_t recvcount, chr_dtype dtype, chr_op op, int k, int b) {
    return local_collective(g, chr::MODE_REDUCE_SCATTER, sends, recvs, recvcount, dtype, op, k, b);
}

static bool valid_mpich_mode(chr_mode m) { return m >= CHR_MODE_MPICH_RING && m <= CHR_MODE_MPICH_RMULT; }

int chr_allreduce_mpich(const void* send, void* recv, size_t count, chr_dtype dtype, chr_op op, chr_comm* comm,
                        chr_mode algo, int k, int single_phase_recv) {
    if (!valid_mpich_mode(algo)) return CHR_ERR_INVALID_ARG;
    return collective(comm, algo, send, recv, count, dtype, op, k, single_phase_recv, true);
}

int chr_allreduce_mpich_async(const void* send, void* recv, size_t count, chr_dtype dtype, chr_op op, chr_comm* comm,
                              chr_mode algo, int k, int single_phase_recv) {
    if (!valid_mpich_mode(algo)) return CHR_ERR_INVALID_ARG;
    return collective(comm, algo, send, recv, count, dtype, op, k, single_phase_recv, false);
}

int chr_local_allreduce_mpich(chr_local_group* g, const void* const* sends, void* const* recvs, size_t count,
                              chr_dtype dtype, chr_op op, chr_mode algo, int k, int single_phase_recv) {
    if (!valid_mpich_mode(algo)) return CHR_ERR_INVALID_ARG;
    return local_collective(g, algo, sends, recvs, count, dtype, op, k, single_phase_recv);
}

int chr_reduce_scatter_mpich(const void* send, void* recv, size_t recvcount, chr_dtype dtype, chr_op op,
                             chr_comm* comm, chr_mode algo, int k) {
    if (!is_mpich_rs(algo)) return CHR_ERR_INVALID_ARG;
    return collective(comm, algo, send, recv, recvcount, dtype, op, k, 0, true);
}

int chr_reduce_scatter_mpich_async(const void* send, void* recv, size_t recvcount, chr_dtype dtype, chr_op op,
                                   chr_comm* comm, chr_mode algo, int k) {
    if (!is_mpich_rs(algo)) return CHR_ERR_INVALID_ARG;
    return collective(comm, algo, send, recv, recvcount, dtype, op, k, 0, false);
}

int chr_local_reduce_scatter_mpich(chr_local_group* g, const void* const* sends, void* const* recvs, size_t recvcount,
                                   chr_dtype dtype, chr_op op, chr_mode algo, int k) {
    if (!is_mpich_rs(algo)) return CHR_ERR_INVALID_ARG;
    return local_collective(g, algo, sends, recvs, recvcount, dtype, op, k, 0);
}

int chr_allgather_radix_batch(const void* send, size_t sendcount, chr_dtype dtype, void* recv, chr_comm* comm, int k,
                              int b) {
    return collective(comm, chr::MODE_ALLGATHER, send, recv, sendcount, dtype, CHR_SUM, k, b, true);
}

int chr_allgather_radix_batch_async(const void* send, size_t sendcount, chr_dtype dtype, void* recv, chr_comm* comm,
                                    int k, int b) {
    return collective(comm, chr::MODE_ALLGATHER, send, recv, sendcount, dtype, CHR_SUM, k, b, false);
}

int chr_local_allgather_radix_batch(chr_local_group* g, const void* const* sends, void* const* recvs, size_t sendcount,
                                    chr_dtype dtype, int k, int b) {
    return local_collective(g, chr::MODE_ALLGATHER, sends, recvs, sendcount, dtype, CHR_SUM, k, b);
}

int chr_intra_reduce_scatter_radix_batch(const void* send, void* recv, size_t recvcount, chr_dtype dtype, chr_op op,
                                         chr_comm* comm, int k, int b) {
    return collective(comm, chr::MODE_INTRA_RS, send, recv, recvcount, dtype, op, k, b, true);
}

int chr_inter_reduce_linear(const void* send, void* recv, size_t recvcount, chr_dtype dtype, chr_op op, chr_comm* comm,
                            int b) {
    return collective(comm, chr::MODE_INTER_LINEAR, send, recv, recvcount, dtype, op, 2, b, true);
}

int chr_intra_scatter_radix_batch(const void* send, size_t recvcount, chr_dtype dtype, void* recv, chr_comm* comm,
                                  int k, int b) {
    return collective(comm, chr::MODE_INTRA_SCATTER, send, recv, recvcount, dtype, CHR_SUM, k, b, true);
}

int chr_local_phase_collective(chr_local_group* g, chr_mode mode, const void* const* sends, void* const* recvs,
                               size_t recvcount, chr_dtype dtype, chr_op op, int k, int b) {
    if (!chr::is_phase(mode)) return CHR_ERR_INVALID_ARG;
    return local_collective(g, mode, sends, recvs, recvcount, dtype, mode == CHR_MODE_INTRA_SCATTER ? CHR_SUM : op,
                            mode == CHR_MODE_INTER_REDUCE_LINEAR ? 2 : k, b);
}

}  // extern "C"
