// The host tables of csrc/circle_round2.cuh (LW_CIRCLE_R2_TABLES_ONLY: no kernels, no Context): the classes of the transition
// descriptors, their cycles and exemption points, the boundary constraints grouped by step and the parameters of the point
// table, built stand-alone with the address and undefined-behaviour sanitizers by tests/test_circle_round2_cpu.py and run as
// a child process.  The command line is log2_trace, log2_blowup, n_transitions, then period offset end_exemptions per
// transition, n_boundary, then col step value c0 c1 c2 c3 per boundary constraint.  Printed, one line each, decimal words:
//   C class_of[0 .. n_transitions)
//   K c.x c.y doublings len                 per class
//   E x y                                   per exemption point, class after class
//   O order[0 .. n_boundary)
//   S step x y first count c0 c1 c2 c3      per distinct step
//   T hbits nlo nhi g2N.x g2N.y gN.x gN.y
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#define LW_CIRCLE_R2_TABLES_ONLY
#include "circle_round2.cuh"
using namespace lw;

struct Transition {
    uint64_t period, offset, end_exemptions;
};
struct Boundary {
    uint32_t col;
    uint64_t step;
    uint32_t value;
    uint32_t coeff[4];
};

int main(int argc, char **argv) {
    int at = 1;
    auto next = [&]() -> uint64_t {
        if (at >= argc) exit(2);
        return strtoull(argv[at++], nullptr, 10);
    };
    const uint32_t log2_trace = (uint32_t)next(), log2_blowup = (uint32_t)next();
    if (log2_trace < 1 || log2_trace + log2_blowup > (uint32_t)M31Q_MAX_LOG) return 2;
    std::vector<Transition> tr(next());
    for (Transition &t : tr) {
        t.period = next();
        t.offset = next();
        t.end_exemptions = next();
    }
    std::vector<Boundary> bnd(next());
    for (Boundary &b : bnd) {
        b.col = (uint32_t)next();
        b.step = next();
        b.value = (uint32_t)next();
        for (uint32_t &w : b.coeff) w = (uint32_t)next();
    }

    std::vector<uint32_t> class_of, order;
    std::vector<CircleR2Desc> classes;
    circle_r2_classes(tr.data(), (uint32_t)tr.size(), class_of, classes);
    printf("C");
    for (uint32_t k : class_of) printf(" %u", k);
    printf("\n");
    for (const CircleR2Desc &d : classes) {
        const CircleR2Cycle cy = circle_r2_cycle(d, log2_trace, log2_blowup);
        printf("K %u %u %u %llu\n", m31_canon(cy.c.x), m31_canon(cy.c.y), cy.doublings, (unsigned long long)cy.len);
    }
    for (const CircleR2Desc &d : classes) {
        std::vector<uint64_t> pts;
        circle_r2_exemption_points(d, log2_trace, pts);
        for (uint64_t p : pts) printf("E %u %u\n", (uint32_t)p, (uint32_t)(p >> 32));
    }
    std::vector<CircleR2Step> steps;
    circle_r2_step_groups(bnd.data(), (uint32_t)bnd.size(), log2_trace, order, steps);
    printf("O");
    for (uint32_t k : order) printf(" %u", k);
    printf("\n");
    for (const CircleR2Step &s : steps) {
        const Qm31 c = m31q_canon(s.constant);
        printf("S %llu %u %u %u %u %u %u %u %u\n", (unsigned long long)s.step, m31_canon(s.point.x), m31_canon(s.point.y), s.first, s.count, c.c0, c.c1, c.c2, c.c3);
    }
    const CircleR2Table t = circle_r2_table(log2_trace + log2_blowup);
    printf("T %u %llu %llu %u %u %u %u\n", t.hbits, (unsigned long long)t.nlo, (unsigned long long)t.nhi, m31_canon(t.g2N.x), m31_canon(t.g2N.y), m31_canon(t.gN.x),
           m31_canon(t.gN.y));
    return 0;
}
