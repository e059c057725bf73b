// goldilocks_ext.cuh on the host: the very source the kernels compile, built stand-alone with the address and undefined-
// behaviour sanitizers by tests/test_goldilocks_ext_cpu.py and run as a child process.  The operands are the command
// line (decimal words below p); every result is printed and compared with Python integers there.
//   m  a b      gl2_mul over operands^4
//   s  a        gl2_sqr, gl2_inv, a inv(a) over operands^2
//   b  a b      gl2_mul_base over operands^3
//   x           gl2_add / gl2_sub / gl2_neg over the pairs of neighbouring operands, gl2_inv(0), 7^((p-1)/2) via gl2_pow of t
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "goldilocks_ext.cuh"
using namespace lw;

int main(int argc, char **argv) {
    std::vector<uint64_t> e;
    for (int i = 1; i < argc; i++) e.push_back(strtoull(argv[i], nullptr, 10));
    const size_t n = e.size();
    if (n == 0) return 2;
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++) {
            const Gl2 a{e[i], e[j]};
            for (size_t k = 0; k < n; k++)
                for (size_t l = 0; l < n; l++) {
                    const Gl2 r = gl2_mul(a, Gl2{e[k], e[l]});
                    printf("m %" PRIu64 " %" PRIu64 "\n", r.c0, r.c1);
                }
            const Gl2 s = gl2_sqr(a), v = gl2_inv(a), one = gl2_mul(a, v);
            printf("s %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", s.c0, s.c1, v.c0, v.c1, one.c0, one.c1);
            for (size_t k = 0; k < n; k++) {
                const Gl2 r = gl2_mul_base(a, e[k]);
                printf("b %" PRIu64 " %" PRIu64 "\n", r.c0, r.c1);
            }
        }
    for (size_t i = 0; i + 3 < n; i++) {
        const Gl2 a{e[i], e[i + 1]}, b{e[i + 2], e[i + 3]};
        const Gl2 p = gl2_add(a, b), q = gl2_sub(a, b), m = gl2_neg(a);
        printf("x %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", p.c0, p.c1, q.c0, q.c1, m.c0, m.c1);
    }
    const Gl2 z = gl2_inv(Gl2{0, 0}), w = gl2_pow(Gl2{0, 1}, GL_P - 1), f = gl2_from_words(GL_P, ~0ull);
    printf("z %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", z.c0, z.c1, w.c0, w.c1, f.c0, f.c1);
    return 0;
}
