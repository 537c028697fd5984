// user_ops.cpp -- user-defined reduction ops: MPI_Op_create's analogue on MI355X.
//
// The reference is generic over MPI_Op (all_reduce_radix_batch.cpp:202-204), user-defined ops included: each of its
// MPI_Reduce_local calls (:332, :364, :446, :529) hands the op's function the host buffers.  Here a user op's
// arithmetic is the caller's own device code: chr_op_create registers a host launcher that enqueues it on the stream
// the library passes (include/chiara.h chr_user_reduce_fn; include/chiara_user_op.hpp builds one from a device
// functor).  Folds go to the launcher as they are; an expression tree (the flat schedules' one-pass evaluation,
// k_reduce_tree for the predefined ops) goes whole to the op's tree launcher where it registered one
// (chr_op_create_tree: one HBM pass, inner nodes in registers) and is otherwise, or when that launcher declines,
// evaluated fold by fold in its post-order program, intermediate values in scratch kept per stream (TreeScratch).
// Nothing runs on the host.
#include "user_ops.hpp"

#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "chiara.h"
#include "schedule.hpp"  // kTreeMaxLeaves

namespace chr {

namespace {

struct UserOp {
    chr_user_reduce_fn fn = nullptr;
    chr_user_tree_fn tree_fn = nullptr;  // optional: whole trees in one pass (chr_op_create_tree)
    void* ctx = nullptr;
    int commute = 0;
    bool live = false;
};

std::mutex g_mu;
UserOp g_ops[kMaxUserOps];

// Derived types: base and count of each live code; the same lock as the ops.
struct UserType {
    int base = 0, count = 0;
    bool live = false;
};
UserType g_types[kMaxUserTypes];

bool lookup(int op, UserOp* out) {
    if (!is_user_op(op)) return false;
    std::lock_guard<std::mutex> lk(g_mu);
    const UserOp& u = g_ops[op - kUserOpBase];
    if (!u.live) return false;
    *out = u;
    return true;
}

// The launcher's verdict: 0 = enqueued; anything else = the op refused the call (e.g. a type it does not implement).
int call(const UserOp& u, void* out, const void* acc, const void* const* ins, int m, size_t n, int dtype, bool rf,
         hipStream_t s) {
    if (u.fn(out, acc, ins, m, n, (chr_dtype)dtype, rf ? 1 : 0, s, u.ctx) != 0) return CHR_ERR_UNSUPPORTED;
    return hip_code(hipGetLastError());
}

// Scratch of the fold-by-fold trees: one slot per stack position (depth <= 4), kept per stream and reused by the next
// fold-by-fold tree enqueued on that stream.  Work on one stream runs in order, so the reuse needs no event and no
// wait.  A hipMallocAsync / hipFreeAsync pair per call kept the call from returning at once: the runtime (ROCm 7.0)
// hands a freed block back to its stream while the free is still pending, and hipFreeAsync of such a block waits on
// the host until the stream has drained -- from the second tree enqueued on a busy stream on (measured behind a 19 ms
// copy: 18.7 ms in that one hipFreeAsync, with the default pool, an own pool, and either with an unlimited release
// threshold; tests/test_gpu_stream_concurrency.py holds it).  A slot grows by a stream-ordered free and allocation
// (bytes + 16, so that any residue of `out` fits); the blocks stay with the stream's entry for the life of the
// process: at most four slots of the largest such tree per stream.  Two calls that are inside user_tree on one stream
// at once (two host threads, or a launcher that calls back into the library) and hipStreamPerThread, one handle for
// many streams, take per-call allocations instead.
struct TreeScratch {
    void* p[kTreeMaxLeaves] = {};
    size_t cap[kTreeMaxLeaves] = {};
    bool busy = false;
};
std::mutex g_scratch_mu;
// The key holds the current device: the NULL stream's handle is the same on every device.  Entries are never erased,
// so references to them stay valid.
std::map<std::pair<int, hipStream_t>, TreeScratch> g_scratch;

class ScratchLease {
  public:
    explicit ScratchLease(hipStream_t s) : s_(s) {
        int dev = 0;
        if (s == hipStreamPerThread || hipGetDevice(&dev) != hipSuccess) return;
        std::lock_guard<std::mutex> lk(g_scratch_mu);
        TreeScratch& e = g_scratch[{dev, s}];
        if (e.busy) return;
        e.busy = true;
        mine_ = &e;
    }
    ~ScratchLease() {
        if (!mine_) return;
        std::lock_guard<std::mutex> lk(g_scratch_mu);
        mine_->busy = false;
    }
    // Slot `pos` with room for `bytes`, or nullptr and the status in *err.
    void* slot(int pos, size_t bytes, int* err) {
        if (!mine_) {
            if (!own_[pos]) *err = hip_code(hipMallocAsync(&own_[pos], bytes, s_));
            return own_[pos];
        }
        if (mine_->cap[pos] < bytes) {
            if (mine_->p[pos]) {
                void* old = mine_->p[pos];
                mine_->p[pos] = nullptr;
                mine_->cap[pos] = 0;
                if ((*err = hip_code(hipFreeAsync(old, s_)))) return nullptr;  // behind the calls that used it
            }
            if ((*err = hip_code(hipMallocAsync(&mine_->p[pos], bytes, s_)))) {
                mine_->p[pos] = nullptr;
                return nullptr;
            }
            mine_->cap[pos] = bytes;
        }
        return mine_->p[pos];
    }
    // The per-call allocations go back in stream order; the stream's own slots stay.
    int release() {
        int rc = CHR_SUCCESS;
        for (void*& q : own_)
            if (q) {
                const int e = hip_code(hipFreeAsync(q, s_));
                if (!rc) rc = e;
                q = nullptr;
            }
        return rc;
    }

  private:
    hipStream_t s_;
    TreeScratch* mine_ = nullptr;
    void* own_[kTreeMaxLeaves] = {};
};

// One post-order program (launch_reduce_tree's contract): push leaf j, then comb[j] combines, each popping the top
// `in` and folding it into the value below -- MPI_Reduce_local(in, below), or with the combine's swap bit
// MPI_Reduce_local(below, in) (MPICH_do_reduce's order), the running-value-first form of the launcher.  Consecutive
// combines that fold leaves into the same running value in the same order are one chain -- one launcher call with
// m inputs, as chr_reduce_multi_ex would make it -- so C4's tree ((l0 l1 l2 l3)(l4 l5 l6 l7)) is three calls, not
// seven.  A chain's result goes to scratch slot p (its stack position; it may read slot p itself as the running
// value, never as an input), the last one straight to `out` unless `out` is one of its inputs.
int user_tree(const UserOp& u, void* out, const void* const* leaves, int nl, const uint8_t* comb,
              const uint8_t* swaps, size_t n, int dtype, hipStream_t s) {
    const size_t bytes = n * elem_size(dtype);
    // A derived type's chunks start at multiples of its size, often off 16-byte alignment; the header's kernels stream
    // operands that are congruent modulo 16, so a slot starts at the residue of `out`.
    const size_t skew = is_derived_type(dtype) ? (uintptr_t)out & 15 : 0;
    ScratchLease scratch(s);  // slots by stack position: one per leaf at most (tree_program_ok)
    struct Val {
        const void* p;
        bool leaf;
    };
    struct Chain {
        int pos = -1;  // stack position of the running value; -1: none pending
        const void* acc = nullptr;
        std::vector<const void*> ins;
        bool rf = false;
    } ch;
    std::vector<Val> st;
    int rc = CHR_SUCCESS;
    auto flush = [&](bool last) -> int {
        if (ch.pos < 0) return CHR_SUCCESS;
        void* dst = nullptr;
        if (last) {
            bool out_is_input = false;
            for (const void* q : ch.ins) out_is_input |= q == out;
            if (!out_is_input) dst = out;
        }
        if (!dst) {
            int e = CHR_SUCCESS;
            void* base = scratch.slot(ch.pos, bytes + 16, &e);
            if (!base) return e ? e : CHR_ERR_OUT_OF_MEMORY;
            dst = static_cast<char*>(base) + skew;
        }
        const int e = call(u, dst, ch.acc, ch.ins.data(), (int)ch.ins.size(), n, dtype, ch.rf, s);
        st[ch.pos] = {dst, false};
        ch.pos = -1;
        ch.ins.clear();
        return e;
    };
    int ci = 0;
    for (int j = 0; j < nl && !rc; ++j) {
        st.push_back({leaves[j], true});
        for (int c = 0; c < comb[j] && !rc; ++c, ++ci) {
            const int p = (int)st.size() - 2;  // the running value's position; the top is at p + 1
            const bool rf = swaps && swaps[ci];
            if (ch.pos == p && ch.rf == rf && st.back().leaf) {  // a leaf into the pending chain's running value
                ch.ins.push_back(st.back().p);
                st.pop_back();
                continue;
            }
            if ((rc = flush(false))) break;  // the pending chain's value lands in st[] before it is read
            ch.pos = p;
            ch.acc = st[p].p;
            ch.ins.assign(1, st.back().p);
            ch.rf = rf;
            st.pop_back();
        }
    }
    if (!rc) rc = flush(true);
    if (!rc && st.size() == 1 && st[0].p != out)
        rc = hip_code(hipMemcpyAsync(out, st[0].p, bytes, hipMemcpyDeviceToDevice, s));
    const int e = scratch.release();
    return rc ? rc : e;
}

// Every job with n > 0 and two or more leaves goes to the op's tree launcher in one call, with the residency cap a
// streaming launch of the library's own would take on this thread (stream_wg_cap: kCoresidentWgPerCu beside RCCL, else
// none).  A launcher that declines has enqueued nothing (chiara.h): those jobs, like the 1-leaf ones and every job of
// an op without a tree launcher, are evaluated fold by fold.
int user_trees(const UserOp& u, const TreeJob* jobs, int njobs, int dtype, hipStream_t s) {
    bool handed = false;
    if (u.tree_fn) {
        std::vector<chr_user_tree> ts;
        for (int t = 0; t < njobs; ++t) {
            const TreeJob& jb = jobs[t];
            if (jb.n == 0 || jb.nl < 2) continue;
            chr_user_tree ut{};
            ut.out = jb.out;
            ut.nleaves = jb.nl;
            ut.n = jb.n;
            int nc = 0;
            for (int j = 0; j < jb.nl; ++j) {
                ut.leaves[j] = jb.leaves[j];
                ut.comb[j] = jb.comb[j];
                nc += jb.comb[j];
            }
            for (int c = 0; c < nc && c < kTreeMaxLeaves; ++c) ut.swaps[c] = jb.swaps && jb.swaps[c] ? 1 : 0;
            ts.push_back(ut);
        }
        if (!ts.empty()) {
            const int cap = coresident_depth() > 0 ? kCoresidentWgPerCu : 0;
            if (u.tree_fn(ts.data(), (int)ts.size(), (chr_dtype)dtype, cap, s, u.ctx) == 0) {
                if (int rc = hip_code(hipGetLastError())) return rc;
                handed = true;
            }
        }
    }
    for (int t = 0; t < njobs; ++t) {
        const TreeJob& jb = jobs[t];
        if (jb.n == 0 || (handed && jb.nl >= 2)) continue;
        if (int rc = user_tree(u, jb.out, jb.leaves, jb.nl, jb.comb, jb.swaps, jb.n, dtype, s)) return rc;
    }
    return CHR_SUCCESS;
}

}  // namespace

bool is_user_op(int op) { return op >= kUserOpBase && op < kUserOpBase + kMaxUserOps; }

bool op_commutative(int op) {
    UserOp u;
    return !is_user_op(op) || (lookup(op, &u) && u.commute);
}

bool is_derived_type(int dtype) { return dtype >= kUserTypeBase && dtype < kUserTypeBase + kMaxUserTypes; }

size_t elem_size(int dtype) {
    if (!is_derived_type(dtype)) return dtype_size(dtype);
    std::lock_guard<std::mutex> lk(g_mu);
    const UserType& t = g_types[dtype - kUserTypeBase];
    return t.live ? (size_t)t.count * dtype_size(t.base) : 0;
}

int check_any(int dtype, int op) {
    if (!is_user_op(op)) {
        if (is_derived_type(dtype) && elem_size(dtype) != 0 && op >= 0 && op < kNumOps) return CHR_ERR_UNSUPPORTED;
        return valid_dtype_op(dtype, op) ? CHR_SUCCESS : CHR_ERR_INVALID_ARG;
    }
    UserOp u;
    return elem_size(dtype) != 0 && lookup(op, &u) ? CHR_SUCCESS : CHR_ERR_INVALID_ARG;
}

bool valid_any(int dtype, int op) { return check_any(dtype, op) == CHR_SUCCESS; }

int reduce_any(void* out, const void* acc, const void* const* ins, int m, size_t n, int dtype, int op, hipStream_t s,
               bool running_first) {
    UserOp u;
    if (!is_user_op(op)) return hip_code(launch_reduce(out, acc, ins, m, n, dtype, op, s, running_first));
    if (!lookup(op, &u)) return CHR_ERR_INVALID_ARG;
    if (n == 0) return CHR_SUCCESS;
    return call(u, out, acc, ins, m, n, dtype, running_first, s);
}

int reduce_tree_any(void* out, const void* const* leaves, int nl, const uint8_t* comb, const uint8_t* swaps, size_t n,
                    int dtype, int op, hipStream_t s) {
    UserOp u;
    if (!is_user_op(op)) return hip_code(launch_reduce_tree(out, leaves, nl, comb, swaps, n, dtype, op, s));
    if (!lookup(op, &u)) return CHR_ERR_INVALID_ARG;
    if (n == 0) return CHR_SUCCESS;
    if (nl < 1 || nl > kTreeMaxLeaves) return CHR_ERR_INVALID_ARG;
    TreeJob jb{};
    jb.out = out;
    for (int j = 0; j < nl; ++j) jb.leaves[j] = leaves[j];
    jb.nl = nl;
    jb.comb = comb;
    jb.swaps = swaps;
    jb.n = n;
    return user_trees(u, &jb, 1, dtype, s);
}

int reduce_tree_multi_any(const TreeJob* jobs, int njobs, int dtype, int op, hipStream_t s) {
    UserOp u;
    if (!is_user_op(op)) return hip_code(launch_reduce_tree_multi(jobs, njobs, dtype, op, s));
    if (!lookup(op, &u)) return CHR_ERR_INVALID_ARG;
    return user_trees(u, jobs, njobs, dtype, s);
}

}  // namespace chr

extern "C" {

int chr_op_create(chr_user_reduce_fn fn, void* ctx, int commute, chr_op* op) {
    return chr_op_create_tree(fn, nullptr, ctx, commute, op);
}

int chr_op_create_tree(chr_user_reduce_fn fn, chr_user_tree_fn tree_fn, void* ctx, int commute, chr_op* op) {
    if (!fn || !op) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(chr::g_mu);
    for (int i = 0; i < chr::kMaxUserOps; ++i) {
        chr::UserOp& u = chr::g_ops[i];
        if (u.live) continue;
        u.fn = fn;
        u.tree_fn = tree_fn;
        u.ctx = ctx;
        u.commute = commute != 0;
        u.live = true;
        *op = (chr_op)(chr::kUserOpBase + i);
        return CHR_SUCCESS;
    }
    return CHR_ERR_UNSUPPORTED;  // every slot taken
}

int chr_op_free(chr_op op) {
    if (!chr::is_user_op((int)op)) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(chr::g_mu);
    chr::UserOp& u = chr::g_ops[(int)op - chr::kUserOpBase];
    if (!u.live) return CHR_ERR_INVALID_ARG;
    u = chr::UserOp{};
    return CHR_SUCCESS;
}

int chr_type_contiguous(int count, chr_dtype base, chr_dtype* newtype) {
    const size_t bs = chr::dtype_size((int)base);  // 0 for a derived base: no nesting
    if (!newtype || count < 1 || !bs || (size_t)count > chr::kMaxElemBytes / bs) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(chr::g_mu);
    for (int i = 0; i < chr::kMaxUserTypes; ++i) {
        chr::UserType& t = chr::g_types[i];
        if (t.live) continue;
        t.base = (int)base;
        t.count = count;
        t.live = true;
        *newtype = (chr_dtype)(chr::kUserTypeBase + i);
        return CHR_SUCCESS;
    }
    return CHR_ERR_UNSUPPORTED;  // every code taken
}

int chr_type_free(chr_dtype type) {
    if (!chr::is_derived_type((int)type)) return CHR_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(chr::g_mu);
    chr::UserType& t = chr::g_types[(int)type - chr::kUserTypeBase];
    if (!t.live) return CHR_ERR_INVALID_ARG;
    t = chr::UserType{};
    return CHR_SUCCESS;
}

int chr_type_size(chr_dtype type, size_t* bytes) {
    const size_t es = chr::elem_size((int)type);
    if (!bytes || !es) return CHR_ERR_INVALID_ARG;
    *bytes = es;
    return CHR_SUCCESS;
}

int chr_type_get_contiguous(chr_dtype type, chr_dtype* base, int* count) {
    if (!base || !count) return CHR_ERR_INVALID_ARG;
    if (!chr::is_derived_type((int)type)) {
        if (!chr::dtype_size((int)type)) return CHR_ERR_INVALID_ARG;
        *base = type;
        *count = 1;
        return CHR_SUCCESS;
    }
    std::lock_guard<std::mutex> lk(chr::g_mu);
    const chr::UserType& t = chr::g_types[(int)type - chr::kUserTypeBase];
    if (!t.live) return CHR_ERR_INVALID_ARG;
    *base = (chr_dtype)t.base;
    *count = t.count;
    return CHR_SUCCESS;
}

}  // extern "C"
