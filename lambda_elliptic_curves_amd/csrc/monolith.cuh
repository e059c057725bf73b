// Monolith over Mersenne31 (crypto/src/hash/monolith/mod.rs, ported there from Plonky3): the three layers and the
// permutation, for the host and the device alike (plain C++, no inline assembly), over a state of W u32 words held in
// registers, W in {8, 12, 16, 20, 24}.
//
//   permutation (mod.rs:91-102)   concrete; R times { bars; bricks; concrete; + round constants[r] }; bars; bricks; concrete
//
// Words live in the weak range [0, p] of circle.cuh (p a second spelling of zero, as the reference's weak_reduce leaves
// it); the caller reads them with m31_from_word and hands them back through m31_canon.  Every layer maps [0, p] to [0, p]:
//   bars      bit 31 is clear going in and coming out; p -> p and 0 -> 0, so both spellings of zero agree
//   bricks    m31_add(m31_mul)
//   concrete  W = 16: the circulant of MONOLITH_CIRC16, entries < 2^16: a row sum is at most (sum m) p = 524757 p < 2^51, one
//             u64 accumulator and one reduction per output word;
//             W != 16: a dense Cauchy matrix of canonical 31-bit words read through `mds` (wave-uniform addresses): four
//             products fit a u64 (4 p^2 < 2^64), each group of four is folded once to < 2^34 and the at most six folds
//             are summed (< 2^37) before the one reduction
// Every state index is a compile-time constant after unrolling; the round loop is a loop (wave-uniform trip count).
#pragma once
#include "circle.cuh"

namespace lw {

constexpr int MONOLITH_BARS = 8;         // NUM_BARS: the words that take the S-boxes
constexpr int MONOLITH_MAX_ROUNDS = 15;  // R + 1 is one byte of the SHAKE128 seed and the reference tests R = 5
// MATRIX_CIRC_MDS_16_MERSENNE31_MONOLITH (mod.rs:16-19): row i of the matrix is this row rotated right i times
constexpr uint32_t MONOLITH_CIRC16[16] = {61402, 17845, 26798, 59689, 12021, 40901, 41351, 27521,
                                          56951, 12034, 53865, 43244, 7454,  33823, 28750, 1108};

// One word of Bars, by SWAR on the whole word (no table).  The three low bytes take the 8-bit S-box
// rotl8(y ^ (~rotl8(y, 1) & rotl8(y, 2) & rotl8(y, 3)), 1) (mod.rs:77-79), the top 7 bits take
// rotl7(y ^ (~rotl7(y, 1) & rotl7(y, 2)), 1) (:81-89).  x < 2^31.
__host__ __device__ __forceinline__ uint32_t monolith_rotl8x3(uint32_t x, int k) {   // a rotation inside each of the three low byte lanes
    const uint32_t hi = 0x010101u * ((0xFFu << k) & 0xFFu), lo = 0x010101u * (0xFFu >> (8 - k));
    return ((x << k) & hi) | ((x >> (8 - k)) & lo);
}
__host__ __device__ __forceinline__ uint32_t monolith_rotl7top(uint32_t x, int k) {  // a rotation inside bits 24 .. 30 (the others are 0 in x)
    return ((x << k) | (x >> (7 - k))) & 0x7F000000u;
}
__host__ __device__ __forceinline__ uint32_t monolith_bar(uint32_t x) {
    const uint32_t l = x & 0x00FFFFFFu, h = x & 0x7F000000u;
    const uint32_t tl = l ^ (~monolith_rotl8x3(l, 1) & monolith_rotl8x3(l, 2) & monolith_rotl8x3(l, 3));
    const uint32_t th = h ^ (~monolith_rotl7top(h, 1) & monolith_rotl7top(h, 2));
    return monolith_rotl8x3(tl, 1) | monolith_rotl7top(th, 1);
}
template <int W> __host__ __device__ __forceinline__ void monolith_bars(uint32_t (&s)[W]) {
#pragma unroll
    for (int j = 0; j < MONOLITH_BARS; j++) s[j] = monolith_bar(s[j]);
}

// s[i + 1] += s[i]^2 from the top index down: every square uses the old s[i] (mod.rs:129-133)
template <int W> __host__ __device__ __forceinline__ void monolith_bricks(uint32_t (&s)[W]) {
#pragma unroll
    for (int i = W - 1; i > 0; i--) s[i] = m31_add(s[i], m31_mul(s[i - 1], s[i - 1]));
}

// x < 2^62 -> [0, p]: the low 31 bits plus the rest is at most 2 p, one fold
__host__ __device__ __forceinline__ uint32_t monolith_reduce64(uint64_t x) {
    return m31_fold((uint32_t)(x & M31_P) + (uint32_t)(x >> 31));
}

// W = 16: out[i] = sum_j C[(j - i) mod 16] s[j].  mds is not read.
// W != 16: out[i] = sum_j mds[i * W + j] s[j], mds the W x W Cauchy matrix of the (W, R) instance (mod.rs:152-174).
template <int W> __host__ __device__ __forceinline__ void monolith_concrete(uint32_t (&s)[W], const uint32_t *mds) {
    uint32_t out[W];
    if constexpr (W == 16) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            uint64_t acc = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) acc += (uint64_t)MONOLITH_CIRC16[(j - i) & 15] * s[j];
            out[i] = monolith_reduce64(acc);   // acc < 2^51
        }
    } else {
        static_assert(W % 4 == 0, "groups of four products");
#pragma unroll
        for (int i = 0; i < W; i++) {
            uint64_t sum = 0;   // W / 4 <= 6 folded groups, each < 2^34
#pragma unroll
            for (int j = 0; j < W; j += 4) {
                const uint64_t t = (uint64_t)mds[i * W + j] * s[j] + (uint64_t)mds[i * W + j + 1] * s[j + 1] +
                                   (uint64_t)mds[i * W + j + 2] * s[j + 2] + (uint64_t)mds[i * W + j + 3] * s[j + 3];
                sum += (t & M31_P) + (t >> 31);
            }
            out[i] = monolith_reduce64(sum);
        }
    }
#pragma unroll
    for (int i = 0; i < W; i++) s[i] = out[i];
}

// The permutation with `rounds` = R full rounds.  rc: R rows of W canonical round constants; mds: as monolith_concrete.
// Written as R + 1 turns of { bars; bricks; concrete } with the constants added after all but the last, so that the
// loop body holds the only other copy of Concrete.
template <int W> __host__ __device__ __forceinline__ void monolith_permute(uint32_t (&s)[W], uint32_t rounds, const uint32_t *rc, const uint32_t *mds) {
    monolith_concrete<W>(s, mds);
#pragma unroll 1
    for (uint32_t r = 0; r <= rounds; r++) {
#if defined(__HIP_DEVICE_COMPILE__)
        // keep the loads of the Cauchy matrix inside the loop: hoisted as loop invariants, its W W words outlive the
        // SGPRs and are spilled into VGPR lanes (v_writelane / v_readlane around every product)
        if constexpr (W != 16) asm volatile("" : "+s"(mds));
#endif
        monolith_bars<W>(s);
        monolith_bricks<W>(s);
        monolith_concrete<W>(s, mds);
        if (r < rounds) {
#pragma unroll
            for (int j = 0; j < W; j++) s[j] = m31_add(s[j], rc[r * W + j]);
        }
    }
}

}  // namespace lw
