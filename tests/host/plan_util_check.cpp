// plan_util_check.cpp -- host-only checks of csrc/plan_util.hpp: the byte-range conflict relation and the split of a
// step's local ops into batched runs (on fake base addresses: nothing is dereferenced, no device), the
// (buffer, offset) relation the compiler orders steps by, and the loopback matcher on hand-made steps.  The matcher
// over compiled plans is checked in tools/plan_fuzz.cpp, beside that tool's own pairing.  Run by
// tests/test_plan_util_host.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -I<pkg>/csrc tests/host/plan_util_check.cpp <pkg>/csrc/schedule.cpp -o plan_util_check
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "plan_util.hpp"

using namespace chr;

static int g_checks = 0, g_bad = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++g_checks;                                                          \
        if (!(cond)) {                                                       \
            ++g_bad;                                                         \
            std::fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #cond);     \
        }                                                                    \
    } while (0)

using Runs = std::vector<std::pair<size_t, size_t>>;
constexpr size_t ES = 4;

// Four buffers at fake addresses, 256 MiB apart; in place, SEND is RECV.
struct Fake {
    bool in_place;
    const char* operator()(const Ref& r) const {
        const uintptr_t base[4] = {in_place ? 0x20000000u : 0x10000000u, 0x20000000u, 0x30000000u, 0x40000000u};
        return reinterpret_cast<const char*>(base[r.buf] + r.off * ES);
    }
};

static LocalOp tree(Ref dst, std::vector<Ref> leaves, uint64_t count) {
    LocalOp op{};
    op.kind = L_TREE;
    op.dst = dst;
    op.acc = leaves[0];
    op.ins.assign(leaves.begin() + 1, leaves.end());
    op.count = count;
    return op;
}

static Runs runs(const std::vector<LocalOp>& ops, bool in_place) { return batched_runs(ops, ES, Fake{in_place}); }

static void byte_ranges_and_runs() {
    // two 4-leaf trees over 100 elements each: roots RECV [0, 100) and [100, 200); B's own leaf is SEND [50, 150)
    const LocalOp A = tree({BUF_RECV, 0}, {{BUF_SEND, 200}, {BUF_STAGE, 0}, {BUF_STAGE, 1000}, {BUF_STAGE, 2000}}, 100);
    const LocalOp B =
        tree({BUF_RECV, 100}, {{BUF_SEND, 50}, {BUF_STAGE, 100}, {BUF_STAGE, 1100}, {BUF_STAGE, 2100}}, 100);
    CHECK((runs({A, B}, false) == Runs{{0, 2}}));
    CHECK(one_tree_run({A, B}, ES, Fake{false}));
    // in place SEND resolves to RECV's base: A's root [0, 100) meets B's leaf [50, 150)
    CHECK(runs({A, B}, true).empty());
    CHECK(!one_tree_run({A, B}, ES, Fake{true}));
    CHECK(conflict(touched(A, ES, Fake{true}), touched(B, ES, Fake{true})));
    CHECK(!conflict(touched(A, ES, Fake{false}), touched(B, ES, Fake{false})));
    // a root over the tree's own leaf 0 is element-wise: it still batches with a disjoint neighbour
    const LocalOp own = tree({BUF_RECV, 300}, {{BUF_RECV, 300}, {BUF_STAGE, 3000}}, 100);
    CHECK((runs({own, A}, false) == Runs{{0, 2}}));
    CHECK((runs({A, own, B}, false) == Runs{{0, 3}}));
    // a 9-leaf tree, a fold and a copy each end a run
    std::vector<Ref> nine;
    for (uint64_t j = 0; j < 9; ++j) nine.push_back({BUF_STAGE, 10000 + 1000 * j});
    LocalOp wide = tree({BUF_ACC, 0}, nine, 100), fold = wide, copy = wide;
    fold.kind = L_REDUCE;
    fold.ins.resize(1);
    copy.kind = L_COPY;
    copy.ins.clear();
    CHECK(!batch_tree(wide) && !batch_tree(fold) && !batch_tree(copy) && batch_tree(A));
    for (const LocalOp& x : {wide, fold, copy}) {
        CHECK((runs({A, B, x, A, B}, false) == Runs{{0, 2}, {3, 5}}));
        CHECK((runs({x, A, B}, false) == Runs{{1, 3}}));
        CHECK(!one_tree_run({A, x}, ES, Fake{false}));
    }
    // a run of one is not batched
    CHECK(runs({A}, false).empty());
    CHECK(runs({A, copy, B}, false).empty());
    CHECK(one_tree_run({A}, ES, Fake{false}) && one_tree_run({}, ES, Fake{false}));
    // a conflicting head runs alone and the rest is looked at afresh: in place A conflicts with B, B and C do not
    const LocalOp C = tree({BUF_RECV, 400}, {{BUF_SEND, 500}, {BUF_STAGE, 4000}}, 100);
    CHECK((runs({A, B, C}, true) == Runs{{1, 3}}));
    // Zero count.  An empty range meets nothing, wherever its address lies: nothing is read or written there, and the
    // executors skip count == 0 ops (a batch drops them, a single op returns at once).  No compiled plan has a
    // zero-count tree beside a non-zero one (build_plan_flat gives every tree of a step one non-zero length), so the
    // choice moves no plan's launches; it makes the relation agree with what runs.
    const char* lo = (const char*)0x1000;
    CHECK(!meets(lo + 0x10, 0, lo, 0x100) && !meets(lo, 0x100, lo + 0x10, 0) && meets(lo + 0x10, 1, lo, 0x100));
    // its root lies "inside" A's leaf STAGE [0, 100)
    const LocalOp Z = tree({BUF_STAGE, 50}, {{BUF_STAGE, 5000}, {BUF_STAGE, 6000}}, 0);
    CHECK(!conflict(touched(A, ES, Fake{false}), touched(Z, ES, Fake{false})));
    CHECK((runs({A, Z}, false) == Runs{{0, 2}}));
}

static void buffer_offset_relation() {
    // SEND and RECV are one space; overlap compares offsets within it, may_alias calls any SEND/RECV pair aliased
    CHECK(space(BUF_SEND) == space(BUF_RECV) && space(BUF_ACC) != space(BUF_STAGE));
    CHECK(space(BUF_ACC) != space(BUF_RECV) && space(BUF_STAGE) != space(BUF_RECV));
    CHECK(overlap({BUF_SEND, 0, 10}, {BUF_RECV, 5, 15}));
    CHECK(!overlap({BUF_SEND, 0, 10}, {BUF_RECV, 100, 110}));
    CHECK(may_alias({BUF_SEND, 0}, 10, {BUF_RECV, 100}, 10) && may_alias({BUF_RECV, 100}, 10, {BUF_SEND, 0}, 10));
    CHECK(may_alias({BUF_RECV, 0}, 10, {BUF_RECV, 5}, 10) && !may_alias({BUF_RECV, 0}, 10, {BUF_RECV, 10}, 10));
    // ACC and STAGE are distinct
    CHECK(!overlap({BUF_ACC, 0, 10}, {BUF_STAGE, 0, 10}) && !may_alias({BUF_ACC, 0}, 10, {BUF_STAGE, 0}, 10));
    // touching ranges [a, b) and [b, c) do not conflict
    CHECK(!overlap({BUF_ACC, 0, 10}, {BUF_ACC, 10, 20}) && overlap({BUF_ACC, 0, 11}, {BUF_ACC, 10, 20}));
    // L_COPY2D: two rows of 4 elements, destination pitch 10, source pitch 20 -- only the rows conflict
    LocalOp c2{};
    c2.kind = L_COPY2D;
    c2.dst = {BUF_ACC, 0};
    c2.acc = {BUF_STAGE, 0};
    c2.count = 4;
    c2.rows = 2;
    c2.dpitch = 10;
    c2.spitch = 20;
    std::vector<Region> rd, wr;
    op_regions(c2, &rd, &wr);
    CHECK(rd.size() == 2 && wr.size() == 2);
    auto writer = [&](Region w) { return conflict(wr, rd, {}, {w}); };  // WAW against the copy's rows
    auto reader = [&](Region r) { return conflict(wr, rd, {r}, {}); };  // RAW
    CHECK(writer({BUF_ACC, 0, 4}) && writer({BUF_ACC, 12, 13}) && reader({BUF_ACC, 13, 20}));
    CHECK(!writer({BUF_ACC, 4, 10}) && !reader({BUF_ACC, 4, 10}) && !writer({BUF_ACC, 14, 100}));
    // WAR on the source rows
    CHECK(writer({BUF_STAGE, 23, 24}) && !writer({BUF_STAGE, 4, 20}) && !reader({BUF_STAGE, 0, 100}));
}

static Plan one_step(std::vector<Xfer> sends, std::vector<Xfer> recvs) {
    Plan p;
    p.steps.emplace_back();
    p.steps[0].sends = std::move(sends);
    p.steps[0].recvs = std::move(recvs);
    return p;
}

static void matcher() {
    struct Pair {
        int r;
        uint64_t roff;
        int q;
        uint64_t soff;
    };
    std::vector<Pair> got;
    auto note = [&](int r, const Xfer& rv, int q, const Xfer& sd) { got.push_back({r, rv.ref.off, q, sd.ref.off}); };
    // two sends 0 -> 1 in one step pair with rank 1's two receives from 0 in order; 1 -> 0 crosses them
    std::vector<Plan> P = {one_step({{1, {BUF_SEND, 0}, 5}, {1, {BUF_SEND, 100}, 7}}, {{1, {BUF_STAGE, 40}, 3}}),
                           one_step({{0, {BUF_SEND, 9}, 3}}, {{0, {BUF_STAGE, 10}, 5}, {0, {BUF_STAGE, 20}, 7}})};
    Mismatch why;
    CHECK(match_step(P, 0, note, &why) && why.sender < 0);
    CHECK(got.size() == 3 && got[0].r == 0 && got[0].q == 1 && got[0].soff == 9 && got[0].roff == 40);
    CHECK(got.size() == 3 && got[1].r == 1 && got[1].roff == 10 && got[1].q == 0 && got[1].soff == 0);
    CHECK(got.size() == 3 && got[2].r == 1 && got[2].roff == 20 && got[2].q == 0 && got[2].soff == 100);
    // a count mismatch fails at the receive
    P[1].steps[0].recvs[1].count = 8;
    CHECK(!match_step(P, 0, note, &why) && why.receiver == 1 && why.sender == 0);
    P[1].steps[0].recvs[1].count = 7;
    // a send left over fails
    P[0].steps[0].sends.push_back({1, {BUF_SEND, 200}, 9});
    CHECK(!match_step(P, 0, note, &why) && why.receiver == -1 && why.sender == 0);
    // a receive with no send fails
    P[0].steps[0].sends.clear();
    CHECK(!match_step(P, 0, note, &why) && why.receiver == 1 && why.sender == 0);
}

int main() {
    byte_ranges_and_runs();
    buffer_offset_relation();
    matcher();
    std::printf("{\"checks\": %d, \"failures\": %d}\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
