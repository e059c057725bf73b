// Stand-alone host program over lambda_elliptic_curves_amd/csrc/monolith.cuh: the very source the kernels compile, built
// for the host (tests/test_monolith_cpu.py builds it with -fsanitize=address,undefined and compares what it prints with
// tests/monolith_ref.py).  Commands on standard input, answers on standard output, one line each:
//   B n  w_0 .. w_{n-1}                                       -> "B v"  per word: monolith_bar(w), w < 2^31
//   P W R n  rc (R x W)  mds (W x W)  n states of W words     -> "P v_0 .. v_{W-1}" per state: words read mod p, the
//                                                                permutation, canonical words
//   L W layer n  mds (W x W)  n states of W words             -> "L ..." per state: one layer (0 Concrete, 1 Bars, 2 Bricks)
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "monolith.cuh"

using namespace lw;

static uint32_t word() {
    unsigned long long v;
    if (scanf("%llu", &v) != 1 || v > 0xFFFFFFFFull) {
        fprintf(stderr, "bad input\n");
        exit(2);
    }
    return (uint32_t)v;
}
static std::vector<uint32_t> words(size_t n) {
    std::vector<uint32_t> v(n);
    for (size_t i = 0; i < n; i++) v[i] = word();
    return v;
}

// layer < 0: the permutation with `rounds` rounds
template <int W> static void states(char tag, int layer, uint32_t rounds, uint32_t n, const uint32_t *rc, const uint32_t *mds) {
    for (uint32_t i = 0; i < n; i++) {
        uint32_t s[W];
        for (int j = 0; j < W; j++) s[j] = m31_from_word(word());
        if (layer < 0) monolith_permute<W>(s, rounds, rc, mds);
        else if (layer == 0) monolith_concrete<W>(s, mds);
        else if (layer == 1) monolith_bars<W>(s);
        else monolith_bricks<W>(s);
        printf("%c", tag);
        for (int j = 0; j < W; j++) printf(" %u", m31_canon(s[j]));
        printf("\n");
    }
}
static void dispatch(uint32_t W, char tag, int layer, uint32_t rounds, uint32_t n, const uint32_t *rc, const uint32_t *mds) {
    switch (W) {
        case 8: return states<8>(tag, layer, rounds, n, rc, mds);
        case 12: return states<12>(tag, layer, rounds, n, rc, mds);
        case 16: return states<16>(tag, layer, rounds, n, rc, mds);
        case 20: return states<20>(tag, layer, rounds, n, rc, mds);
        case 24: return states<24>(tag, layer, rounds, n, rc, mds);
    }
    fprintf(stderr, "bad width %u\n", W);
    exit(2);
}

int main() {
    char cmd;
    while (scanf(" %c", &cmd) == 1) {
        if (cmd == 'B') {
            const uint32_t n = word();
            for (uint32_t i = 0; i < n; i++) printf("B %u\n", monolith_bar(word()));
        } else if (cmd == 'P') {
            const uint32_t W = word(), R = word(), n = word();
            const std::vector<uint32_t> rc = words((size_t)R * W), mds = words((size_t)W * W);
            dispatch(W, 'P', -1, R, n, rc.data(), mds.data());
        } else if (cmd == 'L') {
            const uint32_t W = word(), layer = word(), n = word();
            const std::vector<uint32_t> mds = words((size_t)W * W);
            dispatch(W, 'L', (int)layer, 0, n, nullptr, mds.data());
        } else {
            fprintf(stderr, "bad command %c\n", cmd);
            return 2;
        }
    }
    return 0;
}
