// Host check of align_split (csrc/reduce_common.hpp): how every bucket and tree call is cut into a scalar head, a
// body of 16-byte vectors and a scalar tail.  For es in {1, 2, 4, 8, 16}, every output address phase 0..15, one or
// two operands whose phases are the output's or differ from it (each operand at every phase, so operands on and
// off the element grid both occur), and n in [0, 4 E + 3] with E = 16 / es:
//   congruent exactly when all phases are equal and a multiple of es;
//   a non-congruent call returns all zeros (the caller runs it on the scalar kernel);
//   head + nvec E + tail == n, tail < E, head <= min(n, E - 1);
//   when nvec > 0 the vector body starts on a 16-byte boundary: (phase + head es) % 16 == 0.
// The pieces then tile [0, n) exactly, so no launch of a congruent call starts before `out` or ends past
// out + n es.  Built and run by tests/test_align_split_host.py; prints the number of violations.
#include <cstdio>
#include "reduce_common.hpp"
int main() {
    long bad = 0, cases = 0;
    alignas(16) static char arena[4][64];
    for (size_t es : {1u, 2u, 4u, 8u, 16u}) {
        const size_t E = 16 / es;
        for (unsigned po = 0; po < 16; ++po)
            for (int nops = 1; nops <= 2; ++nops)
                for (unsigned p1 = 0; p1 < 16; ++p1)
                    for (unsigned p2 = 0; p2 < (nops == 2 ? 16u : 1u); ++p2) {
                        const void* out = arena[0] + po;
                        const void* ops[2] = {arena[1] + p1, arena[2] + p2};
                        const bool want = po % es == 0 && p1 == po && (nops == 1 || p2 == po);
                        for (size_t n = 0; n <= 4 * E + 3; ++n) {
                            const chr::AlignSplit s = chr::align_split(out, ops, nops, n, es);
                            ++cases;
                            if (s.congruent != want) { ++bad; continue; }
                            if (!want) {
                                bad += s.head != 0 || s.nvec != 0 || s.tail != 0;
                                continue;
                            }
                            bad += s.head + s.nvec * E + s.tail != n;
                            bad += s.tail >= E;
                            bad += s.head > (n < E - 1 ? n : E - 1);
                            bad += s.nvec > 0 && (po + s.head * es) % 16 != 0;
                            // the head is the whole distance to the boundary unless n ends first
                            bad += s.head != (n < (16 - po) % 16 / es ? n : (16 - po) % 16 / es);
                        }
                    }
    }
    bad += cases < 100000;  // the sweep ran
    std::printf("%ld\n", bad);
    return bad != 0;
}
