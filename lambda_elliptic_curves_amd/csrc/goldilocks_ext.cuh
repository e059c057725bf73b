// The quadratic extension of Goldilocks, Fp2 = F_p[t] / (t^2 - 7): Goldilocks64ExtensionField of the reference
// (u64_goldilocks_field.rs:219-227 over extensions/quadratic.rs:79-118), which is also Plonky2's quadratic extension.
// 7 is a non-residue (7^((p - 1) / 2) = p - 1), so the only element of norm zero is 0.
//
// An element is a = c0 + c1 t, two CANONICAL words of goldilocks.cuh; every function below takes canonical operands
// and returns canonical results, because gl_add / gl_sub / gl_mul do.  The same source compiles for the host (the
// power tables and argument checks of goldilocks_ext.hip, and the stand-alone program tests/goldilocks_ext_host_main.cpp).
//   gl2_mul       Karatsuba: a0 b0, a1 b1, (a0 + a1)(b0 + b1), and 7 a1 b1 - three products and the one by 7.  The two
//                 sums go through gl_add: a raw a0 + a1 can pass 2^64.
//   gl2_sqr       c0 = a0^2 + 7 a1^2, c1 = 2 a0 a1
//   gl2_mul_base  by an element of F: two products
//   gl2_inv       conj(a) / norm(a), norm = a0^2 - 7 a1^2 inverted in F (gl_inv: Fermat, 0 -> 0, so inv(0) = 0)
#pragma once
#include "goldilocks.cuh"

namespace lw {

constexpr uint64_t GL2_NON_RESIDUE = 7;

struct Gl2 {
    uint64_t c0, c1;
};

__host__ __device__ __forceinline__ Gl2 gl2_from_words(uint64_t c0, uint64_t c1) { return Gl2{gl_from_word(c0), gl_from_word(c1)}; }
__host__ __device__ __forceinline__ Gl2 gl2_add(Gl2 a, Gl2 b) { return Gl2{gl_add(a.c0, b.c0), gl_add(a.c1, b.c1)}; }
__host__ __device__ __forceinline__ Gl2 gl2_sub(Gl2 a, Gl2 b) { return Gl2{gl_sub(a.c0, b.c0), gl_sub(a.c1, b.c1)}; }
__host__ __device__ __forceinline__ Gl2 gl2_neg(Gl2 a) { return Gl2{gl_sub(0, a.c0), gl_sub(0, a.c1)}; }
__host__ __device__ __forceinline__ Gl2 gl2_mul(Gl2 a, Gl2 b) {
    const uint64_t a0b0 = gl_mul(a.c0, b.c0), a1b1 = gl_mul(a.c1, b.c1);
    const uint64_t z = gl_mul(gl_add(a.c0, a.c1), gl_add(b.c0, b.c1));
    return Gl2{gl_add(a0b0, gl_mul(a1b1, GL2_NON_RESIDUE)), gl_sub(gl_sub(z, a0b0), a1b1)};
}
__host__ __device__ __forceinline__ Gl2 gl2_sqr(Gl2 a) {
    const uint64_t v = gl_mul(a.c0, a.c1);
    return Gl2{gl_add(gl_mul(a.c0, a.c0), gl_mul(gl_mul(a.c1, a.c1), GL2_NON_RESIDUE)), gl_add(v, v)};
}
__host__ __device__ __forceinline__ Gl2 gl2_mul_base(Gl2 a, uint64_t b) { return Gl2{gl_mul(a.c0, b), gl_mul(a.c1, b)}; }
__host__ __device__ __forceinline__ uint64_t gl2_norm(Gl2 a) {
    return gl_sub(gl_mul(a.c0, a.c0), gl_mul(gl_mul(a.c1, a.c1), GL2_NON_RESIDUE));
}
__host__ __device__ __forceinline__ Gl2 gl2_inv(Gl2 a) {
    const uint64_t ninv = gl_inv(gl2_norm(a));
    return Gl2{gl_mul(a.c0, ninv), gl_sub(0, gl_mul(a.c1, ninv))};
}
__host__ __device__ __forceinline__ Gl2 gl2_pow(Gl2 a, uint64_t e) {
    Gl2 r{1, 0};
    while (e) {
        if (e & 1) r = gl2_mul(r, a);
        a = gl2_sqr(a);
        e >>= 1;
    }
    return r;
}

}  // namespace lw
