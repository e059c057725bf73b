// Goldilocks (p = 2^64 - 2^32 + 1) arithmetic for goldilocks.hip: U64TestField (u64_test_field.rs:98-104) and the field
// of Winterfell's Felt, Plonky2 and Miden.  The same source compiles for the host (the argument checks and root powers of
// goldilocks.hip, and the stand-alone twin of tests/test_goldilocks_cpu.py).
//
// Representation.  One u64 per element, the residue itself: no Montgomery form.  Inside the kernels every value is
// CANONICAL, in [0, p); the only words that are not come from the caller and go through gl_from_word (or straight into
// gl_mul, which takes any u64).  With EPS = 2^32 - 1 = 2^64 mod p, all in u64 arithmetic that wraps mod 2^64:
//   gl_from_word(x) any u64 -> [0, p): x >= p means x - p (from_base_type; 2^64 - 1 - p = EPS - 1 < p, one subtraction)
//   gl_canon(x)     the same function under the name the stores use
//   gl_add(a, b)    a, b < p.  s = a + b < 2p.  Wrapped (s < a): the true sum is s + 2^64 with s <= 2p - 2 - 2^64 = p - EPS - 2,
//                   and s + EPS = a + b - p < p does not wrap.  Not wrapped: s < 2^64 < 2p, one conditional subtraction
//                   of p (written as + EPS mod 2^64).  Both cases are the same "+ EPS", so one select.  -> [0, p)
//   gl_sub(a, b)    a, b < p.  d = a - b; on a borrow d = a - b + 2^64 >= 2^64 - (p - 1) = EPS + 1, so d - EPS = a - b + p
//                   in [1, p) does not wrap.  -> [0, p)
//   gl_mul(a, b)    ANY u64 a, b.  Four 32 x 32 -> 64 products make x = a b = x_lo + 2^64 x_hi < 2^128 (the partial sums
//                   lh + (ll >> 32) and hl + low32(mid) are at most (2^32 - 1)^2 + 2^32 - 1 < 2^64; x_hi < 2^64 because x < 2^128).
//                   With x_hi = 2^32 hh + hl, 2^64 = EPS and 2^96 = -1 (mod p):  x = x_lo - hh + hl EPS, which is reduce_128
//                   of u64_goldilocks_field.rs:187-203 with its three fix-ups:
//                     t0 = x_lo - hh; on a borrow t0 -= EPS (t0 wrapped >= 2^64 - 2^32 + 1 > EPS: no second wrap)
//                     t1 = hl EPS = (hl << 32) - hl = [hl - (hl != 0), -hl] in halves, <= (2^32 - 1)^2 = 2^64 - 2^33 + 1: no
//                          multiply, no wrap
//                     t2 = t0 + t1; on a carry t2 += EPS (t0 + t1 - 2^64 <= 2^64 - 2^33, + EPS < 2^64: no second wrap)
//                     t2 >= p -> t2 - p
//                   Every step keeps the value mod p, so the result is the canonical residue of a b.  -> [0, p)
//   gl_pow, gl_inv  square and multiply over gl_mul; gl_inv(a) = a^(p - 2) (Fermat), 0 -> 0
// Random operands almost never take the borrow branch or end at or above p before the last subtraction; the operand list
// EDGE of tests/goldilocks_ref.py takes every branch many times and runs through the host twin and through the device.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace lw {

constexpr uint64_t GL_P = 0xFFFFFFFF00000001ull;
constexpr uint64_t GL_EPS = 0xFFFFFFFFull;                       // 2^64 mod p
constexpr uint64_t GL_TWO_ADIC_ROOT = 1753635133440165772ull;    // 7^((p - 1) / 2^32): TWO_ADIC_PRIMITVE_ROOT_OF_UNITY
constexpr uint32_t GL_TWO_ADICITY = 32;

__host__ __device__ __forceinline__ uint64_t gl_from_word(uint64_t x) { return x >= GL_P ? x - GL_P : x; }
__host__ __device__ __forceinline__ uint64_t gl_canon(uint64_t x) { return gl_from_word(x); }
__host__ __device__ __forceinline__ uint64_t gl_add(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;
    return (s < a || s >= GL_P) ? s + GL_EPS : s;   // s - p = s + EPS mod 2^64
}
__host__ __device__ __forceinline__ uint64_t gl_sub(uint64_t a, uint64_t b) {
    const uint64_t d = a - b;
    return a < b ? d - GL_EPS : d;   // d + p = d - EPS mod 2^64
}
__host__ __device__ __forceinline__ uint64_t gl_reduce128(uint64_t x_lo, uint64_t x_hi) {
    const uint32_t hh = (uint32_t)(x_hi >> 32), hl = (uint32_t)x_hi;
    uint64_t t0 = x_lo - hh;
    if (x_lo < hh) t0 -= GL_EPS;
    // (hl << 32) - hl in halves: written as a product the compiler issues a fifth multiply for it
    const uint64_t t1 = ((uint64_t)(hl - (hl != 0 ? 1u : 0u)) << 32) | (uint32_t)(0u - hl);
    uint64_t t2 = t0 + t1;
    if (t2 < t1) t2 += GL_EPS;
    return t2 >= GL_P ? t2 - GL_P : t2;
}
__host__ __device__ __forceinline__ uint64_t gl_mul(uint64_t a, uint64_t b) {
    const uint64_t al = a & GL_EPS, ah = a >> 32, bl = b & GL_EPS, bh = b >> 32;
    const uint64_t ll = al * bl;                       // four 32 x 32 -> 64 products, the sums ride on the multiply-adds
    const uint64_t mid = al * bh + (ll >> 32);
    const uint64_t mid2 = ah * bl + (mid & GL_EPS);
    const uint64_t x_hi = ah * bh + (mid >> 32) + (mid2 >> 32);
    const uint64_t x_lo = (mid2 << 32) | (ll & GL_EPS);
    return gl_reduce128(x_lo, x_hi);
}
__host__ __device__ __forceinline__ uint64_t gl_pow(uint64_t a, uint64_t e) {
    uint64_t r = 1, b = gl_from_word(a);
    while (e) {
        if (e & 1) r = gl_mul(r, b);
        b = gl_mul(b, b);
        e >>= 1;
    }
    return r;
}
__host__ __device__ __forceinline__ uint64_t gl_inv(uint64_t a) { return gl_pow(a, GL_P - 2); }

}  // namespace lw
