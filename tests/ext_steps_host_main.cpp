// The host tables of csrc/ext_steps.cuh (ext_power_tables, ext_regroup_weights, ext_deep_constant) under both policies,
// the very source the drivers call, built stand-alone with the address and undefined-behaviour sanitizers by
// tests/test_ext_steps_cpu.py and run as a child process.  The two .hip files are taken for their policy alone
// (LW_EXT_POLICY_ONLY leaves their entry points out: nothing here needs a Context or a device).
//   argv: gl2 | bb4, the number of points, the points' words, then for m = 1, 4, 5 the 3 x m weights and the 3 x m evals
//   (decimal words, E::D to a scalar).  Every element is printed as one line of E::D decimal words:
//   for every point and group in {1, 2, 257}: xp[0 .. 7], pe[0 .. 7], xt, pg[0 .. 7]
//   for every m: the regrouped weights, ceil(m / 4) x 3 x 4 elements, then c_0 .. c_(m - 1)
#define LW_EXT_POLICY_ONLY
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "goldilocks_ext.hip"
#include "babybear_ext.hip"
using namespace lw;

template <class E> static void show(typename E::elem v) {
    typename E::word w[E::D];
    E::store(ext_planes<E>(w, 1), 0, v);
    for (int e = 0; e < E::D; e++) printf("%" PRIu64 "%c", (uint64_t)w[e], e + 1 < E::D ? ' ' : '\n');
}

template <class E> static int run(const std::vector<uint64_t> &args) {
    std::vector<typename E::word> w(args.begin() + 1, args.end());   // exactly as long as the words: a read past them is an error
    const size_t n_points = args[0], n_cols = 3;
    size_t need = n_points * E::D;
    for (size_t m : {1, 4, 5}) need += 2 * n_cols * m * E::D;
    if (w.size() != need) return 2;
    const typename E::word *at = w.data();
    for (size_t p = 0; p < n_points; p++)
        for (uint32_t group : {1u, 2u, 257u}) {
            ExtPowers<E> t;
            ext_power_tables<E>(ext_elem_of<E>(at, p), group, t);
            for (int e = 0; e < EXT_E; e++) show<E>(t.xp[e]);
            for (int s = 0; s < EXT_STEPS; s++) show<E>(t.pe[s]);
            show<E>(t.xt);
            for (int s = 0; s < EXT_STEPS; s++) show<E>(t.pg[s]);
        }
    at += n_points * E::D;
    for (uint32_t m : {1u, 4u, 5u}) {
        const size_t table = n_cols * m * E::D, groups = (m + EXT_PTS - 1) / EXT_PTS;
        // copies of their exact length, so that the sanitizer sees a read past either table
        const std::vector<typename E::word> weights(at, at + table), evals(at + table, at + 2 * table);
        std::vector<typename E::elem> grouped(groups * n_cols * EXT_PTS);
        ext_regroup_weights<E>(weights.data(), n_cols, m, grouped.data());
        for (const typename E::elem &g : grouped) show<E>(g);
        for (uint32_t j = 0; j < m; j++) show<E>(ext_deep_constant<E>(weights.data(), evals.data(), n_cols, m, j));
        at += 2 * table;
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    std::vector<uint64_t> args;
    for (int i = 2; i < argc; i++) args.push_back(strtoull(argv[i], nullptr, 10));
    if (!strcmp(argv[1], "gl2")) return run<Gl2Ext>(args);
    if (!strcmp(argv[1], "bb4")) return run<Bb4Ext>(args);
    return 2;
}
