// The host tables of csrc/ext_round2.cuh (the classes of the transition descriptors with their cycle constants and roots,
// the boundary constraints grouped by step with the combined constants) under both policies, the very source the driver
// calls, built stand-alone with the address and undefined-behaviour sanitizers by tests/test_ext_round2_cpu.py and run as a
// child process.  The two .hip files are taken for their policy alone (LW_EXT_POLICY_ONLY leaves their entry points out:
// nothing here needs a Context or a device).
//   argv: gl2 | bb4, log2_trace, log2_blowup, g (the primitive 2^log2_trace-th root as a word), n_transitions, then per
//   transition period, offset, end_exemptions, exemptions_period, periodic_exemptions_offset and the E::D words of its
//   coefficient, n_boundary, then per boundary constraint col, step, value and the E::D words of its coefficient (decimal).
//   Printed, one line each:
//   the class of every transition; per class "len de ne dc nc has_num" and its roots; the order of the boundary
//   constraints; per step "point first count" and the E::D words of its constant
#define LW_EXT_POLICY_ONLY
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "goldilocks_ext.hip"
#include "babybear_ext.hip"
using namespace lw;

template <class E, class B, class T> static int run(const std::vector<uint64_t> &a) {
    using word = typename E::word;
    size_t at = 0;
    auto next = [&]() -> uint64_t {
        if (at >= a.size()) exit(2);
        return a[at++];
    };
    const uint32_t log2_trace = (uint32_t)next(), log2_blowup = (uint32_t)next();
    const word g = (word)next();
    const uint64_t n = 1ull << log2_trace;
    std::vector<T> tr(next());   // exactly as long as the table: a read past it is an error
    for (T &t : tr) {
        t.period = next(), t.offset = next(), t.end_exemptions = next(), t.exemptions_period = next(), t.periodic_exemptions_offset = next();
        for (int e = 0; e < E::D; e++) t.coeff[e] = (word)next();
    }
    std::vector<B> bnd(next());
    for (B &b : bnd) {
        memset(&b, 0, sizeof(b));
        b.col = (uint32_t)next(), b.step = next(), b.value = (word)next();
        for (int e = 0; e < E::D; e++) b.coeff[e] = (word)next();
    }
    if (at != a.size()) return 2;
    std::vector<uint32_t> class_of, order;
    std::vector<ExtR2Desc> classes;
    ext_r2_classes(tr.data(), (uint32_t)tr.size(), class_of, classes);
    for (size_t c = 0; c < class_of.size(); c++) printf("%u%c", class_of[c], c + 1 < class_of.size() ? ' ' : '\n');
    if (class_of.empty()) printf("\n");
    for (const ExtR2Desc &d : classes) {
        const ExtR2Cycle<E> cy = ext_r2_cycle<E>(d, log2_trace, log2_blowup, g);
        printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", cy.len, cy.de, cy.ne, (uint64_t)cy.dc, (uint64_t)cy.nc, cy.has_num);
        std::vector<word> roots;
        ext_r2_roots<E>(d, n, g, roots);
        for (size_t r = 0; r < roots.size(); r++) printf("%" PRIu64 "%c", (uint64_t)roots[r], r + 1 < roots.size() ? ' ' : '\n');
        if (roots.empty()) printf("\n");
    }
    std::vector<ExtR2Step<E>> steps;
    ext_r2_step_groups<E>(bnd.data(), (uint32_t)bnd.size(), n, g, order, steps);
    for (size_t q = 0; q < order.size(); q++) printf("%u%c", order[q], q + 1 < order.size() ? ' ' : '\n');
    if (order.empty()) printf("\n");
    for (const ExtR2Step<E> &s : steps) {
        printf("%" PRIu64 " %u %u\n", (uint64_t)s.point, s.first, s.count);
        uint64_t packed[2];
        ext_r2_pack<E>(s.constant, packed);   // the words the kernels read back
        word w[E::D];
        memcpy(w, packed, 16);
        for (int e = 0; e < E::D; e++) printf("%" PRIu64 "%c", (uint64_t)w[e], e + 1 < E::D ? ' ' : '\n');
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    std::vector<uint64_t> args;
    for (int i = 2; i < argc; i++) args.push_back(strtoull(argv[i], nullptr, 10));
    if (!strcmp(argv[1], "gl2")) return run<Gl2Ext, lw_gl2_boundary_t, lw_gl2_transition_t>(args);
    if (!strcmp(argv[1], "bb4")) return run<Bb4Ext, lw_bb4_boundary_t, lw_bb4_transition_t>(args);
    return 2;
}
