// plan_util.hpp -- the relations plans are scheduled and executed by (host only, no HIP: g++ compiles it).
//
// Owns: "does A write what B touches" in its two forms -- on (buffer, offset) regions, where the compiler orders
// steps and splits folds, and on resolved byte ranges, where the executors decide which trees share a launch (under
// CHR_IN_PLACE the SEND and RECV buffers are one, which only resolved addresses show); the split of a list of local ops
// into batched runs; and the loopback message matching of one step.  tests/host/plan_util_check.cpp pins each of them.
#pragma once

#include <cstddef>
#include <utility>
#include <vector>

#include "schedule.hpp"

namespace chr {

// ---- (buffer, offset) regions.  SEND and RECV are one space (the same memory under MPI_IN_PLACE; a false conflict
// only costs overlap, never correctness).
struct Region {
    uint8_t buf;
    uint64_t lo, hi;
};
inline uint8_t space(uint8_t b) { return b == BUF_SEND ? (uint8_t)BUF_RECV : b; }
inline bool overlap(const Region& a, const Region& b) {
    return space(a.buf) == space(b.buf) && a.lo < b.hi && b.lo < a.hi;
}
// As overlap, but a SEND/RECV pair aliases whatever the offsets: in place SEND is RECV, at an offset that differs for
// allgather / reduce-scatter.
inline bool may_alias(const Ref& a, uint64_t na, const Ref& b, uint64_t nb) {
    if (a.buf != b.buf && space(a.buf) == space(b.buf)) return true;
    return overlap({a.buf, a.off, a.off + na}, {b.buf, b.off, b.off + nb});
}
inline void op_regions(const LocalOp& op, std::vector<Region>* rd, std::vector<Region>* wr) {
    if (op.kind == L_COPY2D) {
        for (uint64_t r = 0; r < op.rows; ++r) {
            rd->push_back({op.acc.buf, op.acc.off + r * op.spitch, op.acc.off + r * op.spitch + op.count});
            wr->push_back({op.dst.buf, op.dst.off + r * op.dpitch, op.dst.off + r * op.dpitch + op.count});
        }
        return;
    }
    rd->push_back({op.acc.buf, op.acc.off, op.acc.off + op.count});
    for (const Ref& x : op.ins) rd->push_back({x.buf, x.off, x.off + op.count});
    wr->push_back({op.dst.buf, op.dst.off, op.dst.off + op.count});
}
// RAW, WAW or WAR between a (writes wr_a, reads rd_a) and b.
inline bool conflict(const std::vector<Region>& wr_a, const std::vector<Region>& rd_a, const std::vector<Region>& rd_b,
                     const std::vector<Region>& wr_b) {
    auto any = [](const std::vector<Region>& x, const std::vector<Region>& y) {
        for (const Region& a : x)
            for (const Region& b : y)
                if (overlap(a, b)) return true;
        return false;
    };
    return any(wr_a, rd_b) || any(wr_a, wr_b) || any(rd_a, wr_b);
}

// ---- resolved byte ranges: what one tree evaluation touches, `bytes` at the output and at each operand.
struct Touched {
    const char* out;
    const char* in[kTreeMaxLeaves];
    int nin;
    size_t bytes;
};
// An empty range meets nothing: nothing is read or written there (the executors skip count == 0 ops).  No plan puts
// a zero-count tree beside a non-zero one -- build_plan_flat, the only emitter of trees, gives every tree of a step one
// non-zero length -- so this changes no plan's launches.
inline bool meets(const char* a, size_t an, const char* b, size_t bn) { return an && bn && a < b + bn && b < a + an; }
// Whether w's output meets r's output or any of r's operands.
inline bool writes_into(const Touched& w, const Touched& r) {
    if (meets(w.out, w.bytes, r.out, r.bytes)) return true;
    for (int j = 0; j < r.nin; ++j)
        if (meets(w.out, w.bytes, r.in[j], r.bytes)) return true;
    return false;
}
inline bool conflict(const Touched& a, const Touched& b) { return writes_into(a, b) || writes_into(b, a); }

// ---- batched runs.  Consecutive L_TREE ops of one step (the flat schedule's chunks of one pipeline slice) run as ONE
// batched launch when none writes what another reads or writes (an op's own in-place root over its own leaf is
// element-wise and fine): fewer grid fills and drains per call.  Anything else runs op by op.
inline bool batch_tree(const LocalOp& op) { return op.kind == L_TREE && op.ins.size() < (size_t)kTreeMaxLeaves; }
// `at` resolves a Ref to its address; es = element size.  op is a batch_tree.
template <class At>
Touched touched(const LocalOp& op, size_t es, At&& at) {
    Touched t{at(op.dst), {at(op.acc)}, (int)op.ins.size() + 1, (size_t)op.count * es};
    for (size_t j = 0; j < op.ins.size(); ++j) t.in[j + 1] = at(op.ins[j]);
    return t;
}
// The runs [i0, i1) of `ops` that go to one batched launch each, ascending; every op outside them runs alone.  From
// each op on, the longest stretch of batch_trees is one run if it has two or more ops and no two of them conflict;
// else that op runs alone and the next is looked at afresh.
template <class At>
std::vector<std::pair<size_t, size_t>> batched_runs(const std::vector<LocalOp>& ops, size_t es, At&& at) {
    std::vector<std::pair<size_t, size_t>> runs;
    std::vector<Touched> t;
    for (size_t i = 0, j = 0; i < ops.size();) {
        if (j <= i)  // a new stretch: [i, j)
            for (j = i, t.clear(); j < ops.size() && batch_tree(ops[j]); ++j) t.push_back(touched(ops[j], es, at));
        bool ok = j - i >= 2;
        const size_t t0 = t.size() - (j - i);
        for (size_t x = t0; x < t.size() && ok; ++x)
            for (size_t y = x + 1; y < t.size() && ok; ++y) ok = !conflict(t[x], t[y]);
        if (ok) runs.push_back({i, j});
        i = ok ? j : i + 1;
    }
    return runs;
}
// Whether `ops` is nothing but batch_trees that go to a single launch (or is a single such tree, or empty).
template <class At>
bool one_tree_run(const std::vector<LocalOp>& ops, size_t es, At&& at) {
    for (const LocalOp& op : ops)
        if (!batch_tree(op)) return false;
    return ops.size() < 2 || batched_runs(ops, es, at) == std::vector<std::pair<size_t, size_t>>{{0, ops.size()}};
}

// ---- loopback transport of step `si` over every rank's plan: each receive takes the next unmatched send of its peer
// to this rank in the same step (RCCL's per-pair ordering).  on_pair(receiver, recv xfer, sender, send xfer) per
// receive, ranks ascending.  False on a size mismatch or no send (why = {receiver, sender}) and on a send left over
// (why = {-1, sender}).
struct Mismatch {
    int receiver = -1, sender = -1;
};
template <class F>
bool match_step(const std::vector<Plan>& P, size_t si, F&& on_pair, Mismatch* why = nullptr) {
    const int n = (int)P.size();
    Mismatch m;
    std::vector<std::vector<char>> used(n);
    for (int r = 0; r < n; ++r) used[r].assign(P[r].steps[si].sends.size(), 0);
    for (int r = 0; r < n && m.sender < 0; ++r)
        for (const Xfer& rv : P[r].steps[si].recvs) {
            const int q = rv.peer;
            const auto& qs = P[q].steps[si].sends;
            size_t j = 0;
            while (j < qs.size() && (used[q][j] || qs[j].peer != r)) ++j;
            if (j == qs.size() || qs[j].count != rv.count) {
                m = {r, q};
                break;
            }
            used[q][j] = 1;
            on_pair(r, rv, q, qs[j]);
        }
    for (int r = 0; r < n && m.sender < 0; ++r)
        for (char u : used[r])
            if (!u) m = {-1, r};
    if (why) *why = m;
    return m.sender < 0;
}

}  // namespace chr
