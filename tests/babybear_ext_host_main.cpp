// babybear_ext.cuh on the host: the very source the kernels compile, built stand-alone with the address and undefined-
// behaviour sanitizers by tests/test_babybear_ext_cpu.py and run as a child process.  The command line is nE, then nE stored
// words (the set E), then the stored words of the set B; every result is printed as decimal words, four to a line, and
// compared with Python integers there, in this order:
//   bb4_mul       a in E^4 (a0 outermost), b in B^4
//   bb4_sqr, bb4_inv, a inv(a)   a in E^4, three lines each
//   bb4_mul_base  a in E^4, b in E
//   bb4_add, bb4_sub, bb4_neg    a = (E[i], E[i+1], E[i+2], E[i+3]), b = (E[i+4], ..., E[i+7]), indices mod nE, three lines each
//   bb4_pow(x, 4), bb4_inv(0)    x^4 = -11
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "babybear_ext.cuh"
using namespace lw;

static void put(Bb4 r) { printf("%u %u %u %u\n", r.c0, r.c1, r.c2, r.c3); }

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const size_t ne = strtoul(argv[1], nullptr, 10);
    if (ne == 0 || (size_t)argc < 2 + ne + 1) return 2;
    std::vector<uint32_t> e, b;
    for (size_t i = 0; i < ne; i++) e.push_back((uint32_t)strtoul(argv[2 + i], nullptr, 10));
    for (int i = 2 + (int)ne; i < argc; i++) b.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
    const size_t nb = b.size();
    std::vector<Bb4> ea, ba;
    for (size_t i = 0; i < ne; i++)
        for (size_t j = 0; j < ne; j++)
            for (size_t k = 0; k < ne; k++)
                for (size_t l = 0; l < ne; l++) ea.push_back(Bb4{e[i], e[j], e[k], e[l]});
    for (size_t i = 0; i < nb; i++)
        for (size_t j = 0; j < nb; j++)
            for (size_t k = 0; k < nb; k++)
                for (size_t l = 0; l < nb; l++) ba.push_back(Bb4{b[i], b[j], b[k], b[l]});
    for (const Bb4 &a : ea)
        for (const Bb4 &x : ba) put(bb4_mul(a, x));
    for (const Bb4 &a : ea) {
        const Bb4 v = bb4_inv(a);
        put(bb4_sqr(a));
        put(v);
        put(bb4_mul(a, v));
    }
    for (const Bb4 &a : ea)
        for (size_t k = 0; k < ne; k++) put(bb4_mul_base(a, e[k]));
    for (size_t i = 0; i < ne; i++) {
        const Bb4 a{e[i], e[(i + 1) % ne], e[(i + 2) % ne], e[(i + 3) % ne]}, x{e[(i + 4) % ne], e[(i + 5) % ne], e[(i + 6) % ne], e[(i + 7) % ne]};
        put(bb4_add(a, x));
        put(bb4_sub(a, x));
        put(bb4_neg(a));
    }
    put(bb4_pow(Bb4{0, BabyBear::ONE, 0, 0}, 4));
    put(bb4_inv(bb4_zero()));
    return 0;
}
