// The quartic extension of BabyBear, Fp4 = F_p[x] / (x^4 + 11): Degree4BabyBearExtensionField of the reference
// (math/src/field/fields/fft_friendly/quartic_babybear.rs), which is RISC Zero's extension.  x^4 + 11 is irreducible, so
// the only element without an inverse is 0.
//
// An element is a = a0 + a1 x + a2 x^2 + a3 x^3, four CANONICAL stored words of field.cuh's BabyBear (the Montgomery value
// with R = 2^32, below p); every function takes canonical operands and returns canonical results.  The same source
// compiles for the host (the power tables and argument checks of babybear_ext.hip, and the stand-alone program
// tests/babybear_ext_host_main.cpp).
//
// Lazy sums.  A coordinate of a product is a sum of four base products, and a base product of canonical words is at most
// (p - 1)^2 < 2^62, so the four are added in 64 bits and reduced ONCE:
//   bb_fold    x < 2 p 2^32 = p 2^33 (< 2^64)           ->  x or x - p 2^32, below p 2^32: bb_reduce's bound.  Only the high
//              word takes part: x >= p 2^32 exactly when hi(x) >= p.
//   bb_reduce4 x <= 4 (p - 1)^2 < p 2^33 (4 p < 2^33)   ->  canonical x 2^-32
//   bb_mac2    acc < p 2^32, two products <= 2 (p - 1)^2 < p 2^32: the sum is below p 2^33, folded back below p 2^32
// The factor -11 of x^4 goes onto the operand, not onto the sum (11 * 3 (p - 1)^2 does not fit 64 bits): a_i' =
// bb_mul(a_i, -11 R) is canonical again, so the products with it keep the bound above.
//   bb4_mul       16 products + 3 by -11 = 19 base products, 7 reductions (the reference's form: 19 products, 19 reductions)
//   bb4_sqr       10 products + 2 by -11 = 12 base products, 6 reductions
//   bb4_mul_base  by an element of F: 4 products
//   bb4_inv       the reference's norm to Fp2 = F_p[y] / (y^2 + 11), y = x^2: with b = a(x) a(-x) = b0 + b2 y and
//                 c = b0^2 + 11 b2^2 in F, 1 / a = a(-x) (b0 - b2 y) / c.  One bb_inv (Fermat, 0 -> 0, so inv(0) = 0).
#pragma once
#include "field.cuh"

namespace lw {

constexpr uint32_t BB4_BETA = 11;                    // x^4 = -11
constexpr uint32_t BB4_BETA_R = 0x37ffffe9u;         // 11 R mod p, R = 2^32: 11 * 0x0ffffffe - p
constexpr uint32_t BB4_NEG_BETA_R = 0x40000018u;     // -11 R mod p = p - BB4_BETA_R
static_assert(BB4_BETA_R == (uint32_t)(11ull * BabyBear::ONE % BabyBear::P) && BB4_NEG_BETA_R == BabyBear::P - BB4_BETA_R, "11 R mod p");
constexpr uint64_t BB_P_R = (uint64_t)BabyBear::P << 32;   // p 2^32: what bb_reduce takes values below
static_assert(4ull * (BabyBear::P - 1) < (1ull << 33), "four products stay below p 2^33");

struct Bb4 {
    uint32_t c0, c1, c2, c3;
};

LW_HD uint64_t bb_fold(uint64_t x) {   // x < p 2^33 -> x mod p 2^32 (same residue mod p), below p 2^32
    const uint32_t hi = (uint32_t)(x >> 32), d = hi - BabyBear::P;   // d wraps above hi exactly when hi < p
    return ((uint64_t)(d < hi ? d : hi) << 32) | (uint32_t)x;
}
LW_HD uint32_t bb_reduce4(uint64_t x) { return bb_reduce(bb_fold(x)); }   // x <= 4 (p - 1)^2
// acc + a b + c d for acc < p 2^32 and canonical a, b, c, d: below p 2^32 + 2 (p - 1)^2 < p 2^33, folded below p 2^32
LW_HD uint64_t bb_mac2(uint64_t acc, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return bb_fold(acc + (uint64_t)a * b + (uint64_t)c * d);
}
// a b + c d + e f + g h, every factor canonical: <= 4 (p - 1)^2 in 64 bits, one reduction
LW_HD uint32_t bb_dot4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e, uint32_t f, uint32_t g, uint32_t h) {
    return bb_reduce4((uint64_t)a * b + (uint64_t)c * d + (uint64_t)e * f + (uint64_t)g * h);
}

LW_HD Bb4 bb4_zero() { return Bb4{0, 0, 0, 0}; }
LW_HD bool bb4_is_zero(Bb4 a) { return (a.c0 | a.c1 | a.c2 | a.c3) == 0; }
LW_HD Bb4 bb4_add(Bb4 a, Bb4 b) { return Bb4{bb_add(a.c0, b.c0), bb_add(a.c1, b.c1), bb_add(a.c2, b.c2), bb_add(a.c3, b.c3)}; }
LW_HD Bb4 bb4_sub(Bb4 a, Bb4 b) { return Bb4{bb_sub(a.c0, b.c0), bb_sub(a.c1, b.c1), bb_sub(a.c2, b.c2), bb_sub(a.c3, b.c3)}; }
LW_HD Bb4 bb4_neg(Bb4 a) { return Bb4{bb_sub(0, a.c0), bb_sub(0, a.c1), bb_sub(0, a.c2), bb_sub(0, a.c3)}; }
LW_HD Bb4 bb4_mul(Bb4 a, Bb4 b) {
    // a_i' = -11 a_i, canonical.  Every coordinate: four products of canonical words, <= 4 (p - 1)^2 (bb_dot4).
    const uint32_t n1 = bb_mul(a.c1, BB4_NEG_BETA_R), n2 = bb_mul(a.c2, BB4_NEG_BETA_R), n3 = bb_mul(a.c3, BB4_NEG_BETA_R);
    return Bb4{bb_dot4(a.c0, b.c0, n1, b.c3, n2, b.c2, n3, b.c1),       // a0 b0 - 11 (a1 b3 + a2 b2 + a3 b1)
               bb_dot4(a.c0, b.c1, a.c1, b.c0, n2, b.c3, n3, b.c2),     // a0 b1 + a1 b0 - 11 (a2 b3 + a3 b2)
               bb_dot4(a.c0, b.c2, a.c1, b.c1, a.c2, b.c0, n3, b.c3),   // a0 b2 + a1 b1 + a2 b0 - 11 a3 b3
               bb_dot4(a.c0, b.c3, a.c1, b.c2, a.c2, b.c1, a.c3, b.c0)};
}
LW_HD Bb4 bb4_sqr(Bb4 a) {
    // the doubled products are added twice: every sum is again four products of canonical words, <= 4 (p - 1)^2
    const uint32_t n2 = bb_mul(a.c2, BB4_NEG_BETA_R), n3 = bb_mul(a.c3, BB4_NEG_BETA_R);
    const uint64_t a1n3 = (uint64_t)a.c1 * n3;                              // -11 a1 a3
    const uint64_t c1h = (uint64_t)a.c0 * a.c1 + (uint64_t)n2 * a.c3;       // a0 a1 - 11 a2 a3      <= 2 (p - 1)^2
    const uint64_t a0a2 = (uint64_t)a.c0 * a.c2;
    const uint64_t c3h = (uint64_t)a.c0 * a.c3 + (uint64_t)a.c1 * a.c2;     // a0 a3 + a1 a2         <= 2 (p - 1)^2
    return Bb4{bb_reduce4((uint64_t)a.c0 * a.c0 + a1n3 + a1n3 + (uint64_t)n2 * a.c2),     // a0^2 - 11 (2 a1 a3 + a2^2)
               bb_reduce4(c1h + c1h),
               bb_reduce4(a0a2 + a0a2 + (uint64_t)a.c1 * a.c1 + (uint64_t)n3 * a.c3),     // 2 a0 a2 + a1^2 - 11 a3^2
               bb_reduce4(c3h + c3h)};
}
LW_HD Bb4 bb4_mul_base(Bb4 a, uint32_t b) { return Bb4{bb_mul(a.c0, b), bb_mul(a.c1, b), bb_mul(a.c2, b), bb_mul(a.c3, b)}; }

// The two halves of the inverse, apart so that a kernel can share one bb_inv among many elements (Montgomery's trick on the
// norms).  bb4_norm: b0 + b2 y = a(x) a(-x) and its norm c = b0^2 + 11 b2^2 in F, zero only for a = 0.  bb4_inv_with: 1 / a
// from b0, b2 and 1 / c.  The sums of two products are <= 2 (p - 1)^2 < p 2^32: bb_reduce takes them as they are.
LW_HD uint32_t bb4_norm(Bb4 a, uint32_t &b0, uint32_t &b2) {
    const uint32_t a1a3 = bb_mul(a.c1, a.c3), a0a2 = bb_mul(a.c0, a.c2);
    // b0 = a0^2 + 11 (2 a1 a3 - a2^2),  b2 = 2 a0 a2 - a1^2 + 11 a3^2
    b0 = bb_add(bb_mul(a.c0, a.c0), bb_mul(bb_sub(bb_add(a1a3, a1a3), bb_mul(a.c2, a.c2)), BB4_BETA_R));
    b2 = bb_add(bb_sub(bb_add(a0a2, a0a2), bb_mul(a.c1, a.c1)), bb_mul(bb_mul(a.c3, a.c3), BB4_BETA_R));
    return bb_add(bb_mul(b0, b0), bb_mul(bb_mul(b2, b2), BB4_BETA_R));
}
LW_HD Bb4 bb4_inv_with(Bb4 a, uint32_t b0, uint32_t b2, uint32_t c_inv) {
    b0 = bb_mul(b0, c_inv);
    b2 = bb_mul(b2, c_inv);
    const uint32_t k2 = bb_mul(b2, BB4_BETA_R);   // 11 b2
    // (a0 - a1 x + a2 x^2 - a3 x^3)(b0 - b2 x^2), x^4 = -11
    return Bb4{bb_reduce((uint64_t)a.c0 * b0 + (uint64_t)a.c2 * k2),                        // a0 b0 + 11 a2 b2
               bb_sub(0, bb_reduce((uint64_t)a.c1 * b0 + (uint64_t)a.c3 * k2)),             // -(a1 b0 + 11 a3 b2)
               bb_sub(bb_mul(a.c2, b0), bb_mul(a.c0, b2)),                                  // a2 b0 - a0 b2
               bb_sub(bb_mul(a.c1, b2), bb_mul(a.c3, b0))};                                 // a1 b2 - a3 b0
}
LW_HD Bb4 bb4_inv(Bb4 a) {
    uint32_t b0, b2;
    const uint32_t c = bb4_norm(a, b0, b2);
    return bb4_inv_with(a, b0, b2, bb_inv(c));
}
LW_HD Bb4 bb4_pow(Bb4 a, uint64_t e) {
    Bb4 r{BabyBear::ONE, 0, 0, 0};
    while (e) {
        if (e & 1) r = bb4_mul(r, a);
        a = bb4_sqr(a);
        e >>= 1;
    }
    return r;
}

}  // namespace lw
