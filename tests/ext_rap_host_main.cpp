// The host code of the randomized AIR over Fp2 and Fp4 - the typing check of csrc/air_program.h (air_program_check_rap), the
// packing of the two coefficient lists of csrc/ext_aux.cuh and the step groups of csrc/ext_round2.cuh over boundary entries
// whose values are in E - under both policies, the very source the drivers call, built stand-alone with the address and
// undefined-behaviour sanitizers by tests/test_ext_rap_cpu.py and run as a child process.  The two .hip files are taken for
// their policy alone (LW_EXT_POLICY_ONLY leaves their entry points out: nothing here needs a Context or a device).
//   argv: gl2 | bb4, then one of (all numbers decimal)
//   prog  n_consts n_xconsts n_cols n_xcols log2_trace log2_lde n_transitions n_ops, then per op: op src index row
//         -> "ok n_tmps n_ext_tmps n_lds_slots" and the typed op words on one line, or "fail" and the message on the next
//   terms n_cols n_num, per term col and the E::D words of its coefficient, n_den, the same
//         (column k stands at the made-up address 4096 (k + 1)) -> per term its four table words on one line
//   steps log2_trace g n_boundary, per constraint col is_aux step, the E::D words of its value, the E::D words of its coefficient
//         -> the order of the constraints; per step "point first count" and the E::D words of its constant
#define LW_EXT_POLICY_ONLY
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "goldilocks_ext.hip"
#include "babybear_ext.hip"
using namespace lw;

struct Args {
    std::vector<uint64_t> a;
    size_t at = 0;
    uint64_t next() {
        if (at >= a.size()) exit(2);
        return a[at++];
    }
};

template <class E> static int prog(Args &in) {
    const uint32_t n_consts = (uint32_t)in.next(), n_xconsts = (uint32_t)in.next(), n_cols = (uint32_t)in.next(), n_xcols = (uint32_t)in.next();
    const uint32_t log2_trace = (uint32_t)in.next(), log2_lde = (uint32_t)in.next(), n_transitions = (uint32_t)in.next();
    std::vector<lw_stark_air_op_t> ops(in.next());   // exactly as long as the program: a read past it is an error
    for (lw_stark_air_op_t &o : ops) o.op = (uint8_t)in.next(), o.src = (uint8_t)in.next(), o.index = (uint16_t)in.next(), o.row = (uint32_t)in.next();
    std::vector<uint64_t> typed(ops.size());
    AirProgramInfo info;
    char msg[192];
    if (!air_program_check_rap(ops.data(), (uint32_t)ops.size(), n_consts, n_xconsts, nullptr, n_cols, n_xcols, E::D, log2_trace, log2_lde, n_transitions,
                               typed.empty() ? nullptr : typed.data(), &info, msg, sizeof(msg))) {
        printf("fail\n%s\n", msg);
        return 0;
    }
    printf("ok %u %u %u\n", info.n_tmps, info.n_ext_tmps, info.n_lds_slots);
    for (size_t k = 0; k < typed.size(); k++) printf("%" PRIu64 "%c", typed[k], k + 1 < typed.size() ? ' ' : '\n');
    if (typed.empty()) printf("\n");
    return 0;
}

template <class E> static int terms(Args &in) {
    using word = typename E::word;
    std::vector<const word *> cols(in.next());
    for (size_t k = 0; k < cols.size(); k++) cols[k] = (const word *)(uintptr_t)(4096 * (k + 1));
    std::vector<uint32_t> c[2];
    std::vector<word> w[2];
    for (int side = 0; side < 2; side++) {
        c[side].resize(in.next());
        w[side].resize(c[side].size() * E::D);
        for (size_t j = 0; j < c[side].size(); j++) {
            c[side][j] = (uint32_t)in.next();
            for (int e = 0; e < E::D; e++) w[side][j * E::D + e] = (word)in.next();
        }
    }
    const word unit[E::D] = {E::F_ONE};
    const ExtAuxList<E> num{unit, c[0].data(), w[0].data(), (uint32_t)c[0].size()}, den{unit, c[1].data(), w[1].data(), (uint32_t)c[1].size()};
    std::vector<uint64_t> t(4 * (c[0].size() + c[1].size()));   // exactly the table
    ext_aux_pack_terms<E>(cols.data(), num, den, t.data());
    for (size_t j = 0; j < t.size() / 4; j++) {
        word cf[E::D];
        memcpy(cf, &t[4 * j + 2], 16);
        printf("%" PRIu64 " %" PRIu64, t[4 * j], t[4 * j + 1]);
        for (int e = 0; e < E::D; e++) printf(" %" PRIu64, (uint64_t)cf[e]);
        printf("\n");
    }
    return 0;
}

template <class E, class B> static int steps(Args &in) {
    using word = typename E::word;
    const uint32_t log2_trace = (uint32_t)in.next();
    const word g = (word)in.next();
    std::vector<B> bnd(in.next());
    for (B &b : bnd) {
        memset(&b, 0, sizeof(b));
        b.col = (uint32_t)in.next(), b.is_aux = (uint32_t)in.next(), b.step = in.next();
        for (int e = 0; e < E::D; e++) b.value[e] = (word)in.next();
        for (int e = 0; e < E::D; e++) b.coeff[e] = (word)in.next();
    }
    std::vector<uint32_t> order;
    std::vector<ExtR2Step<E>> groups;
    ext_r2_step_groups<E>(bnd.data(), (uint32_t)bnd.size(), 1ull << log2_trace, g, order, groups);
    for (size_t q = 0; q < order.size(); q++) printf("%u%c", order[q], q + 1 < order.size() ? ' ' : '\n');
    if (order.empty()) printf("\n");
    for (const ExtR2Step<E> &s : groups) {
        printf("%" PRIu64 " %u %u\n", (uint64_t)s.point, s.first, s.count);
        uint64_t packed[2];
        ext_r2_pack<E>(s.constant, packed);
        word w[E::D];
        memcpy(w, packed, 16);
        for (int e = 0; e < E::D; e++) printf("%" PRIu64 "%c", (uint64_t)w[e], e + 1 < E::D ? ' ' : '\n');
    }
    return 0;
}

template <class E, class B> static int run(const char *what, Args &in) {
    int rc = 2;
    if (!strcmp(what, "prog")) rc = prog<E>(in);
    else if (!strcmp(what, "terms")) rc = terms<E>(in);
    else if (!strcmp(what, "steps")) rc = steps<E, B>(in);
    return rc ? rc : in.at == in.a.size() ? 0 : 2;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    Args in;
    for (int i = 3; i < argc; i++) in.a.push_back(strtoull(argv[i], nullptr, 10));
    if (!strcmp(argv[1], "gl2")) return run<Gl2Ext, lw_gl2_rap_boundary_t>(argv[2], in);
    if (!strcmp(argv[1], "bb4")) return run<Bb4Ext, lw_bb4_rap_boundary_t>(argv[2], in);
    return 2;
}
