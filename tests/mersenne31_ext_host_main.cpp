// mersenne31_ext.cuh on the host: the arithmetic the kernels compile and the tables the entry points build before a launch
// (the basis at a point, a point's DEEP constants, the regrouped weights, the coset's steps), built stand-alone with the
// address and undefined-behaviour sanitizers by tests/test_mersenne31_ext_cpu.py and run as a child process.  The command
// line is nE, nE words (the set E), n_cols, m, log2n, then 8 m point words, 4 n_cols m weight words and 4 n_cols m value
// words.  Every result is printed canonical as decimal words, four to a line, and compared with Python integers there:
//   m31q_mul                      a in E^4 (c0 outermost), b = the element 7 idx + 3 places on (mod |E|^4)
//   m31q_sqr, m31q_inv, a inv(a)  a in E^4, three lines each
//   m31q_mul_base                 a in E^4, b in E
//   per point                     lo[0 .. 7], f[0 .. 29]
//   per point                     (da, db), (dc, cc), sa, sb
//   the regrouped weights         ceil(m / 4) groups of n_cols x 4
//   the coset of 2^log2n          (shift.x, shift.y, 0, 0), then (step[b].x, step[b].y, 0, 0), b < 30
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "mersenne31_ext.cuh"
using namespace lw;

static void put(Qm31 r) {
    r = m31q_canon(r);
    printf("%u %u %u %u\n", r.c0, r.c1, r.c2, r.c3);
}
static void put2(Cm31 a, Cm31 b) { put(m31q_make(a, b)); }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    int at = 1;
    auto next = [&]() -> uint32_t {
        if (at >= argc) exit(2);
        return (uint32_t)strtoul(argv[at++], nullptr, 10);
    };
    const size_t ne = next();
    std::vector<uint32_t> e(ne);
    for (size_t i = 0; i < ne; i++) e[i] = next();
    const uint32_t n_cols = next(), m = next(), log2n = next();
    if (ne == 0 || n_cols == 0 || m == 0 || log2n == 0 || log2n > (uint32_t)M31Q_MAX_LOG) return 2;
    std::vector<uint32_t> points(8 * (size_t)m), weights(4 * (size_t)n_cols * m), evals(4 * (size_t)n_cols * m);
    for (uint32_t &w : points) w = next();
    for (uint32_t &w : weights) w = next();
    for (uint32_t &w : evals) w = next();

    std::vector<Qm31> ea;
    for (size_t i = 0; i < ne; i++)
        for (size_t j = 0; j < ne; j++)
            for (size_t k = 0; k < ne; k++)
                for (size_t l = 0; l < ne; l++) {
                    const uint32_t w[4] = {e[i], e[j], e[k], e[l]};
                    ea.push_back(m31q_from_words(w));
                }
    for (size_t i = 0; i < ea.size(); i++) put(m31q_mul(ea[i], ea[(7 * i + 3) % ea.size()]));
    for (const Qm31 &a : ea) {
        const Qm31 v = m31q_inv(a);
        put(m31q_sqr(a));
        put(v);
        put(m31q_mul(a, v));
    }
    for (const Qm31 &a : ea)
        for (size_t k = 0; k < ne; k++) put(m31q_mul_base(a, m31_from_word(e[k])));

    std::vector<M31qDeepPoint> z(m);
    for (uint32_t j = 0; j < m; j++) {
        M31qBasis t;
        m31q_basis_tables(m31q_point_of(points.data() + 8 * (size_t)j), t);
        for (int k = 0; k < M31Q_E; k++) put(t.lo[k]);
        for (int k = 0; k < M31Q_MAX_LOG; k++) put(t.f[k]);
    }
    for (uint32_t j = 0; j < m; j++) {
        z[j] = m31q_deep_point(m31q_point_of(points.data() + 8 * (size_t)j), weights.data(), evals.data(), n_cols, m, j);
        put2(z[j].da, z[j].db);
        put2(z[j].dc, z[j].cc);
        put(z[j].sa);
        put(z[j].sb);
    }
    const size_t groups = (m + M31Q_PTS - 1) / M31Q_PTS;
    std::vector<Qm31> wt(groups * n_cols * M31Q_PTS);
    m31q_regroup_weights(weights.data(), z.data(), n_cols, m, wt.data());
    for (const Qm31 &w : wt) put(w);
    const M31qCoset c = m31q_coset(log2n);
    put(Qm31{c.shift.x, c.shift.y, 0, 0});
    for (int b = 0; b < M31Q_MAX_LOG; b++) put(Qm31{c.step[b].x, c.step[b].y, 0, 0});
    return 0;
}
