// Rescue Prime Optimized (ePrint 2022/1577) over Goldilocks in registers: the permutation shared by the kernels of
// rpo.hip.  The same source compiles for the host (the stand-alone twin of tests/test_rpo_cpu.py), as goldilocks.cuh does.
//
// RescuePrimeOptimized (crypto/src/hash/rescue_prime/rescue_prime_optimized.rs:192-202, parameters.rs), two levels:
//   LW_RPO_128  state m = 12, capacity 4, rate 8,  digest 4 words  (the hash of Miden)
//   LW_RPO_160  state m = 16, capacity 6, rate 10, digest 5 words
// Seven rounds, each  MDS, + constants, x^7, MDS, + constants, x^(1/7):  fourteen half-rounds of one shape, so the loop
// below runs fourteen times over ONE copy of the MDS, one of x^7 and one of the inverse chain, the S-box chosen by a
// wave-uniform branch on the loop counter.  The round constants come from tools/gen_rpo_consts.py (SHAKE256 of
// "RPO(p,m,capacity,level)", rpo_consts.inc); half-round h adds row h.  The loop counter is wave-uniform, so on the device
// the row reaches the additions through scalar loads.
//
// Representation.  One u64 per word, the residue itself, as in goldilocks.cuh.  The caller's words are ANY u64 and go
// through gl_from_word; from there every value between two steps is CANONICAL, in [0, p), and so is every word stored.
//
// MDS, the circulant M[i][j] = v[(j - i) mod m], without a modular product.  A word s_j = l_j + 2^32 h_j with halves
// below 2^32; over the integers
//     out_i = sum_j v[(j - i) mod m] s_j = A_i + 2^32 B_i,   A_i = sum_j v[..] l_j,   B_i = sum_j v[..] h_j
// and the bound on A_i and B_i is (sum of v) (2^32 - 1) for ANY u64 input, canonical or not:
//   level 128: v = 7 23 8 26 13 10 9 7 6 22 21 8, sum 160 < 2^8, so A_i, B_i < 2^40: u64 sums that cannot wrap, every
//              term one 32 x 32 multiply-add with a constant of five bits
//   level 160: v = 2^8 2 2^30 2^11 2^24 2^7 2^3 2^4 2^19 2^22 1 2^28 1 2^10 2 2^13, sum 1363684766 < 2^31, so
//              A_i, B_i < 2^63: no wrap either, and every term is a shift (the constants are compile-time powers of two)
//   then x = A_i + 2^32 B_i < 2^63 + 2^95 as a 128-bit value: x_lo = A_i + (B_i << 32) mod 2^64, x_hi = (B_i >> 32) + carry
//   <= 2^31, and ONE gl_reduce128(x_lo, x_hi), which takes any 128-bit value -> [0, p).
// 2 m^2 multiply-adds (shift-adds) and m reductions per MDS against 76 m gl_mul per round for the S-boxes.
//
// S-boxes.  x^7 = ((x^2 x)^2) x: 4 products.  x^(1/7) = x^10540996611094048183 (7^-1 mod p - 1) by the chain of 72
// products, acc(b, t, n) = b^(2^n) t:
//     t1 = x^2, t2 = t1^2, t3 = acc(t2, t2, 3), t4 = acc(t3, t3, 6), t5 = acc(t4, t4, 12), t6 = acc(t5, t3, 6),
//     t7 = acc(t6, t6, 31), result = ((t7^2 t6)^2)^2 (t1 t2 x)
// The five acc steps are one loop over a table (3, 6, 12, 6, 31) around one squaring run and one product, the second
// factor of the product the value the step started from (or t3, step 3): the squaring runs stay loops and the whole
// permutation is a few kilobytes of code.  All m words go through every product together: m independent chains in one
// work-item are what covers the latency of the multiply-adds.  A squaring is gl_mul(x, x) with its four multiply-adds (the
// compiler does not merge the two equal cross products); a three-product square with bounds of its own is NOT written.
#pragma once
#include "goldilocks.cuh"

namespace lw {

constexpr int RPO_HALF_ROUNDS = 14;   // 7 rounds of (MDS, + constants, S-box) twice

template <int LEVEL> struct RpoParams;
template <> struct RpoParams<0> { static constexpr int M = 12, CAP = 4, RATE = 8, DIGEST = 4; };
template <> struct RpoParams<1> { static constexpr int M = 16, CAP = 6, RATE = 10, DIGEST = 5; };

#if defined(__HIP_DEVICE_COMPILE__)
#define LW_RPO_TABLE static __constant__ const uint64_t
#else
#define LW_RPO_TABLE static const uint64_t
#endif
// [half-round][word], canonical
LW_RPO_TABLE RPO_RC_128[RPO_HALF_ROUNDS * 12] = {
#define RPO_CONSTS_128
#include "rpo_consts.inc"
#undef RPO_CONSTS_128
};
LW_RPO_TABLE RPO_RC_160[RPO_HALF_ROUNDS * 16] = {
#define RPO_CONSTS_160
#include "rpo_consts.inc"
#undef RPO_CONSTS_160
};
#undef LW_RPO_TABLE

template <int LEVEL> __host__ __device__ __forceinline__ uint64_t rpo_round_constant(int idx) {
    if constexpr (LEVEL == 0) return RPO_RC_128[idx];
    else return RPO_RC_160[idx];
}

// first row of the circulant; k is a compile-time value wherever this is called (fully unrolled loops)
template <int LEVEL> __host__ __device__ constexpr uint64_t rpo_mds_entry(int k) {
    if constexpr (LEVEL == 0) {
        constexpr uint64_t v[12] = {7, 23, 8, 26, 13, 10, 9, 7, 6, 22, 21, 8};
        return v[k];
    } else {
        constexpr uint64_t v[16] = {1ull << 8, 2, 1ull << 30, 1ull << 11, 1ull << 24, 1ull << 7, 8, 16,
                                    1ull << 19, 1ull << 22, 1, 1ull << 28, 1, 1ull << 10, 2, 1ull << 13};
        return v[k];
    }
}

// s <- M s.  Any u64 words in, canonical out (bounds in the header comment).
template <int LEVEL> __host__ __device__ __forceinline__ void rpo_mds(uint64_t (&s)[RpoParams<LEVEL>::M]) {
    constexpr int M = RpoParams<LEVEL>::M;
    uint64_t lo[M], hi[M];
#pragma unroll
    for (int j = 0; j < M; j++) {
        lo[j] = s[j] & GL_EPS;
        hi[j] = s[j] >> 32;
    }
#pragma unroll
    for (int i = 0; i < M; i++) {
        uint64_t a = 0, b = 0;
#pragma unroll
        for (int j = 0; j < M; j++) {
            const uint64_t v = rpo_mds_entry<LEVEL>((j - i + M) % M);
            a += v * lo[j];   // < (sum v) 2^32: no wrap
            b += v * hi[j];
        }
        const uint64_t x_lo = a + (b << 32);
        const uint64_t x_hi = (b >> 32) + (x_lo < a ? 1u : 0u);
        s[i] = gl_reduce128(x_lo, x_hi);
    }
}

// x^7, canonical in and out: 4 products a word
template <int M> __host__ __device__ __forceinline__ void rpo_sbox(uint64_t (&s)[M]) {
#pragma unroll
    for (int j = 0; j < M; j++) {
        const uint64_t x2 = gl_mul(s[j], s[j]);
        const uint64_t x3 = gl_mul(x2, s[j]);
        const uint64_t x6 = gl_mul(x3, x3);
        s[j] = gl_mul(x6, s[j]);
    }
}

// x^(1/7), canonical in and out: 72 products a word, the m words side by side in every product
template <int M> __host__ __device__ __forceinline__ void rpo_sbox_inv(uint64_t (&s)[M]) {
    uint64_t a[M], u[M], t3[M], start[M];
#pragma unroll
    for (int j = 0; j < M; j++) {
        const uint64_t t1 = gl_mul(s[j], s[j]);
        a[j] = gl_mul(t1, t1);                       // t2
        u[j] = gl_mul(gl_mul(t1, a[j]), s[j]);       // t1 t2 x
        t3[j] = 0;
    }
#pragma unroll 1
    for (int step = 0; step < 5; step++) {           // t3, t4, t5, t6, t7 in a
        const int runs = step == 0 ? 3 : step == 2 ? 12 : step == 4 ? 31 : 6;
#pragma unroll
        for (int j = 0; j < M; j++) start[j] = a[j];
#pragma unroll 1
        for (int k = 0; k < runs; k++) {
#pragma unroll
            for (int j = 0; j < M; j++) a[j] = gl_mul(a[j], a[j]);
        }
#pragma unroll
        for (int j = 0; j < M; j++) {
            a[j] = gl_mul(a[j], step == 3 ? t3[j] : start[j]);
            if (step == 0) t3[j] = a[j];
        }
    }
    // a = t7, start = t6
#pragma unroll
    for (int j = 0; j < M; j++) {
        uint64_t r = gl_mul(gl_mul(a[j], a[j]), start[j]);
        r = gl_mul(r, r);
        r = gl_mul(r, r);
        s[j] = gl_mul(r, u[j]);
    }
}

// permutation(): canonical in, canonical out
template <int LEVEL> __host__ __device__ __forceinline__ void rpo_permute(uint64_t (&s)[RpoParams<LEVEL>::M]) {
    constexpr int M = RpoParams<LEVEL>::M;
#pragma unroll 1
    for (int h = 0; h < RPO_HALF_ROUNDS; h++) {
        rpo_mds<LEVEL>(s);
#pragma unroll
        for (int j = 0; j < M; j++) s[j] = gl_add(s[j], rpo_round_constant<LEVEL>(h * M + j));
        if (h & 1) rpo_sbox_inv<M>(s);
        else rpo_sbox<M>(s);
    }
}

}  // namespace lw
