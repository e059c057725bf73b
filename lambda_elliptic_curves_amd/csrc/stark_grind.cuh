// The candidate loop of the STARK grinding search (provers/stark/src/grinding.rs:40-66), for stark_query.hip and for the
// timing tool's stand-alone build (tools/stark_grind_bench.hip), which is the only build that defines
// LW_GRIND_PLAIN_VARIANT and with it the same loop over the unmodified keccak_f1600.
//     valid(nonce)  <=>  u64_be(Keccak256(inner(32) || nonce.to_be_bytes())[0..8]) < 2^(64 - grinding_factor)
// The 40-byte message is one block of the sponge: lanes 0..3 = inner, lane 4 = bswap64(nonce) (a lane is 8 stream bytes
// little-endian), lane 5 = 0x01 (first padding byte), lane 16 = 0x80 << 56 (last byte of the rate), every other lane 0.
// Only lane 4 differs between candidates and only lane 0 of the result is read, so
//   round 0     theta, rho and pi of everything that does not depend on the nonce are done once per call on the host
//               (grind_prepare): E_i = A_i ^ D_(i mod 5) splits into a constant and v = lane 4 (columns 0 and 4) or
//               rotl(v, 1) (column 3); a rotation is linear, so B_j = KB_j ^ rotl(v, r) for 11 lanes and B_j = KB_j for 14;
//   rounds 1-22 the permutation's round as it is in keccak.cuh;
//   round 23    the five column parities, then theta / rho / pi of lanes 0, 6 and 12 only: chi and iota of lane 0.
#pragma once
#include "keccak.cuh"

namespace lw {

constexpr int GRIND_ROT[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
constexpr int GRIND_PIL[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};

struct GrindArgs {
    uint64_t kb[25];     // round 0 after theta, rho, pi with lane 4 = 0 (grind_prepare)
    uint64_t inner[4];   // lanes 0..3 of the message (the plain variant starts from these)
    uint64_t start;      // first candidate of the window
    uint32_t count;      // candidates in the window, at most 2^28
    uint32_t shift;      // 64 - grinding_factor: valid <=> bswap64(lane 0) >> shift == 0
};

// Host side of round 0.  inner: the 32 bytes of Keccak256(PREFIX || seed || grinding_factor).
inline void grind_prepare(const uint8_t *inner, GrindArgs &a) {
    auto rotl = [](uint64_t x, int n) { return n ? (x << n) | (x >> (64 - n)) : x; };
    uint64_t A[25] = {0};
    for (int i = 0; i < 4; i++) {
        uint64_t w = 0;
        for (int b = 7; b >= 0; b--) w = (w << 8) | inner[8 * i + b];
        A[i] = a.inner[i] = w;
    }
    A[5] = 0x01ull;
    A[16] = 0x8000000000000000ull;
    uint64_t C[5], E[25];
    for (int x = 0; x < 5; x++) C[x] = A[x] ^ A[x + 5] ^ A[x + 10] ^ A[x + 15] ^ A[x + 20];
    for (int i = 0; i < 25; i++) E[i] = A[i] ^ C[(i + 4) % 5] ^ rotl(C[(i + 1) % 5], 1);
    a.kb[0] = E[0];
    for (int i = 0; i < 24; i++) a.kb[GRIND_PIL[i]] = rotl(E[i ? GRIND_PIL[i - 1] : 1], GRIND_ROT[i]);
}

// chi and iota on the lanes after pi
__device__ __forceinline__ void grind_chi_iota(U64H (&a)[25], uint64_t rc) {
#pragma unroll
    for (int j = 0; j < 25; j += 5) {
        U64H bc[5];
#pragma unroll
        for (int i = 0; i < 5; i++) bc[i] = a[j + i];
#pragma unroll
        for (int i = 0; i < 5; i++) {
            a[j + i].lo = bc[i].lo ^ (~bc[(i + 1) % 5].lo & bc[(i + 2) % 5].lo);
            a[j + i].hi = bc[i].hi ^ (~bc[(i + 1) % 5].hi & bc[(i + 2) % 5].hi);
        }
    }
    a[0].lo ^= (uint32_t)rc;
    a[0].hi ^= (uint32_t)(rc >> 32);
}

__device__ __forceinline__ void grind_parities(const U64H (&a)[25], U64H (&bc)[5]) {
#pragma unroll
    for (int i = 0; i < 5; i++) {
        bc[i].lo = xor3(xor3(a[i].lo, a[i + 5].lo, a[i + 10].lo), a[i + 15].lo, a[i + 20].lo);
        bc[i].hi = xor3(xor3(a[i].hi, a[i + 5].hi, a[i + 10].hi), a[i + 15].hi, a[i + 20].hi);
    }
}

// lane 0 of Keccak-f[1600] of the candidate's block; v = lane 4 = bswap64(nonce)
__device__ __forceinline__ uint64_t grind_lane0(const GrindArgs &g, uint64_t v64) {
    const U64H v{(uint32_t)v64, (uint32_t)(v64 >> 32)};
    U64H a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = U64H{(uint32_t)g.kb[i], (uint32_t)(g.kb[i] >> 32)};
    // round 0: the nonce's share of theta, rotated to where rho and pi put it
    a[0].lo ^= v.lo;   // lane 0 is in column 0 and does not move
    a[0].hi ^= v.hi;
#pragma unroll
    for (int i = 0; i < 24; i++) {
        const int src = i ? GRIND_PIL[i - 1] : 1, dst = GRIND_PIL[i];
        if (src % 5 == 0 || src == 4 || src % 5 == 3) {
            const U64H r = rotl64h(v, GRIND_ROT[i] + (src % 5 == 3 ? 1 : 0));   // 1 .. 63 for these eleven lanes
            a[dst].lo ^= r.lo;
            a[dst].hi ^= r.hi;
        }
    }
    grind_chi_iota(a, KECCAK_RC[0]);
#pragma unroll 1
    for (int round = 1; round < 23; round++) {
        U64H bc[5];
        grind_parities(a, bc);
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const U64H u = bc[(i + 4) % 5], w = rotl64h(bc[(i + 1) % 5], 1);
#pragma unroll
            for (int j = 0; j < 25; j += 5) a[j + i] = U64H{xor3(a[j + i].lo, u.lo, w.lo), xor3(a[j + i].hi, u.hi, w.hi)};
        }
        U64H t = a[1];
#pragma unroll
        for (int i = 0; i < 24; i++) {
            const int j = GRIND_PIL[i];
            const U64H b = a[j];
            a[j] = rotl64h(t, GRIND_ROT[i]);
            t = b;
        }
        grind_chi_iota(a, KECCAK_RC[round]);
    }
    // round 23: row 0 after pi is lane 0, lane 6 rotated by 44 and lane 12 rotated by 43
    U64H bc[5];
    grind_parities(a, bc);
    const U64H r1 = rotl64h(bc[1], 1), r2 = rotl64h(bc[2], 1), r3 = rotl64h(bc[3], 1);
    const U64H b0{xor3(a[0].lo, bc[4].lo, r1.lo), xor3(a[0].hi, bc[4].hi, r1.hi)};
    const U64H b1 = rotl64h(U64H{xor3(a[6].lo, bc[0].lo, r2.lo), xor3(a[6].hi, bc[0].hi, r2.hi)}, 44);
    const U64H b2 = rotl64h(U64H{xor3(a[12].lo, bc[1].lo, r3.lo), xor3(a[12].hi, bc[1].hi, r3.hi)}, 43);
    const uint64_t rc = KECCAK_RC[23];
    const uint32_t lo = b0.lo ^ (~b1.lo & b2.lo) ^ (uint32_t)rc, hi = b0.hi ^ (~b1.hi & b2.hi) ^ (uint32_t)(rc >> 32);
    return ((uint64_t)hi << 32) | lo;
}

#ifdef LW_GRIND_PLAIN_VARIANT
__device__ __forceinline__ uint64_t grind_lane0_plain(const GrindArgs &g, uint64_t v64) {
    uint64_t st[25];
#pragma unroll
    for (int i = 0; i < 25; i++) st[i] = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) st[i] = g.inner[i];
    st[4] = v64;
    st[5] = 0x01ull;
    st[16] = 0x8000000000000000ull;
    keccak_f1600(st);
    return st[0];
}
#endif

// Candidates start .. start + count - 1 in a grid-stride loop, consecutive work-items on consecutive nonces.  *best starts
// as all-ones; a hit lowers it with atomicMin and ends the work-item (its later candidates are larger), and so does a
// candidate above the current *best.  At most ceil(count / work-items) permutations per work-item, no waiting.
template <int PLAIN>
__global__ __launch_bounds__(256) void grind_kernel(GrindArgs g, unsigned long long *best) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < g.count; k += stride) {   // count <= 2^28, stride <= 2^20: no wrap
        const uint64_t nonce = g.start + k;
        if (nonce > __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        uint64_t lane0;
#ifdef LW_GRIND_PLAIN_VARIANT
        if (PLAIN) lane0 = grind_lane0_plain(g, __builtin_bswap64(nonce));
        else
#endif
            lane0 = grind_lane0(g, __builtin_bswap64(nonce));
        if ((__builtin_bswap64(lane0) >> g.shift) == 0) {   // the digest's first 8 bytes, big-endian, below 2^shift
            atomicMin(best, (unsigned long long)nonce);
            break;
        }
    }
}

// The window of one launch: twice the expected number of candidates (a window then holds a valid nonce with probability
// 1 - e^-2 = 86 %), at least 2^20 (two candidates for each of the 2^19 work-items that fill 256 CUs) and at most 2^28.
inline uint64_t grind_window(uint32_t grinding_factor) {
    const uint32_t lg = grinding_factor + 1 < 20 ? 20 : (grinding_factor + 1 > 28 ? 28 : grinding_factor + 1);
    return 1ull << lg;
}
constexpr uint32_t GRIND_MAX_BLOCKS = 2048;   // x 256 work-items: eight waves per SIMD on 256 CUs

}  // namespace lw
