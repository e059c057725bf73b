// Mersenne31 (p = 2^31 - 1) arithmetic and the circle group over it, for circle.hip.
//
// Representation.  One u32 per element, no Montgomery form.  Inside the kernels a value lives in the WEAK range [0, p]:
// p is a second spelling of zero (mersenne31/field.rs weak_reduce produces it too).  Bounds, all in u32:
//   m31_fold(s)     = (s & p) + (s >> 31): any u32 -> [0, 2^31]; s <= 2p -> [0, p]  (the top bit set leaves at most p - 1 below)
//   m31_from_word   two folds: any u32 -> [0, p]  (one fold, what from_base_type does, leaves 2^31 for the word 2^32 - 1)
//   m31_add(a, b)   a + b <= 2p = 2^32 - 2, no wrap, one fold -> [0, p]
//   m31_sub(a, b)   a + (p - b) <= 2p, one fold -> [0, p]
//   m31_mul(a, b)   a b <= p^2 < 2^62: hi = (a b) >> 31 <= 2^31 - 2, lo = (a b) & p <= p, hi + lo <= 2p - 1, one fold -> [0, p]
//   m31_canon       [0, p] -> [0, p): the only place a comparison is needed; every word the library hands back went through it
// Nothing is lazier than that: a butterfly is mul, add, sub, each closed over [0, p].
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace lw {

constexpr uint32_t M31_P = 0x7fffffffu;

__host__ __device__ __forceinline__ uint32_t m31_fold(uint32_t s) { return (s & M31_P) + (s >> 31); }
__host__ __device__ __forceinline__ uint32_t m31_from_word(uint32_t w) { return m31_fold(m31_fold(w)); }
__host__ __device__ __forceinline__ uint32_t m31_add(uint32_t a, uint32_t b) { return m31_fold(a + b); }
__host__ __device__ __forceinline__ uint32_t m31_sub(uint32_t a, uint32_t b) { return m31_fold(a + (M31_P - b)); }
__host__ __device__ __forceinline__ uint32_t m31_mul(uint32_t a, uint32_t b) {
    const uint64_t t = (uint64_t)a * b;   // one 32 x 32 -> 64 multiply
    return m31_fold(((uint32_t)t & M31_P) + (uint32_t)(t >> 31));
}
__host__ __device__ __forceinline__ uint32_t m31_canon(uint32_t a) { return a == M31_P ? 0u : a; }
__host__ __device__ __forceinline__ uint32_t m31_sqn(uint32_t a, int n) {
    for (int i = 0; i < n; i++) a = m31_mul(a, a);
    return a;
}
// a^(p - 2) = a^(2^31 - 3), exponent 1111111111111111111111111111101b, in 37 products (the chain of mersenne31/field.rs inv);
// 0 -> 0
__host__ __device__ __forceinline__ uint32_t m31_inv(uint32_t a) {
    const uint32_t e5 = m31_mul(m31_sqn(a, 2), a);                 // 101b
    const uint32_t e15 = m31_mul(m31_sqn(e5, 1), e5);              // 4 ones
    const uint32_t e255 = m31_mul(m31_sqn(e15, 4), e15);           // 8 ones
    const uint32_t e8z4 = m31_sqn(e255, 4);                        // 8 ones, 4 zeros
    const uint32_t e12 = m31_mul(e8z4, e15);                       // 12 ones
    const uint32_t e16 = m31_mul(m31_sqn(e8z4, 4), e255);          // 16 ones
    const uint32_t e28 = m31_mul(m31_sqn(e16, 12), e12);           // 28 ones
    return m31_mul(m31_sqn(e28, 3), e5);                           // 28 ones, 101b
}

// The circle group {(x, y): x^2 + y^2 = 1}: (a, b) + (c, d) = (ac - bd, ad + bc), 2 (x, y) = (2 x^2 - 1, 2 x y)
struct CirclePt {
    uint32_t x, y;
};
__host__ __device__ __forceinline__ CirclePt circle_add(CirclePt a, CirclePt b) {
    return CirclePt{m31_sub(m31_mul(a.x, b.x), m31_mul(a.y, b.y)), m31_add(m31_mul(a.x, b.y), m31_mul(a.y, b.x))};
}
__host__ __device__ __forceinline__ CirclePt circle_double(CirclePt a) {
    const uint32_t xx = m31_mul(a.x, a.x), xy = m31_mul(a.x, a.y);
    return CirclePt{m31_sub(m31_add(xx, xx), 1u), m31_add(xy, xy)};
}
// k g, k >= 1: double-and-add from the top bit
__host__ __device__ __forceinline__ CirclePt circle_mul(uint32_t k, CirclePt g) {
    CirclePt r = g;
#if defined(__HIP_DEVICE_COMPILE__)
    int top = 31 - __clz(k);
#else
    int top = 31 - __builtin_clz(k);
#endif
    for (int b = top - 1; b >= 0; b--) {
        r = circle_double(r);
        if ((k >> b) & 1u) r = circle_add(r, g);
    }
    return r;
}

}  // namespace lw
