// Starknet Poseidon (Hades permutation over Stark252) in registers: device code shared by the kernels of poseidon.hip.
//
// PoseidonCairoStark252 (crypto/src/hash/poseidon/mod.rs:26-57, starknet/parameters.rs): state of 3 elements, rate 2,
// capacity 1, S-box x^3, 4 + 83 + 4 rounds,
//     mix(s) = (t + 2 s0, t - 2 s1, t - 3 s2),  t = s0 + s1 + s2.
// The round keys are the public ones, key j of round i = sha256("Hades" + str(3 i + j)) mod p, generated into
// poseidon_consts.inc by tools/gen_poseidon_consts.py.  This is the UNCOMPRESSED schedule: every round adds its three
// keys, rounds 0-3 and 87-90 cube all three words, rounds 4-86 cube word 2 only.  The reference runs the compressed
// schedule (one key per partial round, 107 keys); both give the same permutation (tests/test_poseidon_cpu.py and the
// reference's fixed vectors in tests/golden/poseidon_starknet.json).  Compressing would save two 8-limb adds and two
// reductions in each of the 83 partial rounds beside its two Montgomery products — not taken yet.
//
// One permutation is 8 * 3 * 2 + 83 * 2 = 214 Montgomery products; everything else is limb additions.  One work-item
// runs one permutation with the 3 x 8 limbs of its state in VGPRs.  The round index is a plain loop counter, hence
// wave-uniform: the keys sit in __constant__ memory and reach the carry chains as scalar loads / SGPR operands.
//
// Lazy arithmetic (Stark252 has five spare bits: 2^256 / p > 31.99, so any sum below 31p fits 8 limbs).  Written x < kp
// below: the 8-limb integer is below k * p; "canonical" is < p.
//   round entry     s_j < 10p                     (canonical on the first round)
//   + key           s_j + k_j < 11p               plain 8-limb add, key < p
//   reduce          u_j = fe_reduce_full(..) < p  one subtraction of q*p and a conditional +p: canonical, as the FIRST
//                                                 operand of fe_mul_lazy must be (hard precondition: its fused columns drop
//                                                 carry adds on a[7] <= p[7])
//   S-box           x2 = fe_mul_lazy(u, u)  < 2p  a = u < p, b = u
//                   x3 = fe_mul_lazy(u, x2) < 2p  a = u < p, b = x2 < 2p < 2^256 (b may be any 8-limb value)
//   mix             inputs a, b, c < 2p (cubed words) or < p (the untouched words of a partial round):
//                   t  = a + b + c                      < 6p
//                   o0 = t + a + a                      < 10p
//                   o1 = t + (2p - b) + (2p - b)        = a + c - b + 4p, in (0, 8p)     2p - b in (0, 2p]
//                   o2 = (a + b) + (2p - c) + (2p - c)  = a + b - 2c + 4p, in (0, 8p)
//                   every partial sum is an exact integer below 10p: nothing wraps, no conditional subtraction in a round
//   exit            fe_reduce_full(o_j) < p: every value a kernel stores is canonical
#pragma once
#include "field.cuh"

namespace lw {

typedef Fe<Stark252> PFe;
constexpr int POSEIDON_ROUNDS = 91;         // 4 full + 83 partial + 4 full
constexpr int POSEIDON_FIRST_PARTIAL = 4;
constexpr int POSEIDON_FIRST_LAST_FULL = 87;

// [3 * round + word][limb], Montgomery form, limbs least significant first
static __constant__ uint32_t POSEIDON_RC[POSEIDON_ROUNDS * 3][8] = {
#include "poseidon_consts.inc"
};

// u^3 for canonical u; result < 2p
__device__ __forceinline__ PFe poseidon_cube(const PFe &u) {
    const PFe x2 = fe_mul_lazy<Stark252>(u, u);   // u < p: < 2p
    return fe_mul_lazy<Stark252>(u, x2);          // a = u < p, b = x2 < 2p: < 2p
}

// hades_permutation (mod.rs:27-41) on s; canonical in, canonical out
__device__ __forceinline__ void poseidon_permute(PFe (&s)[3]) {
#pragma unroll 1
    for (int r = 0; r < POSEIDON_ROUNDS; r++) {   // s_j < 10p
        PFe u[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            PFe k;
#pragma unroll
            for (int i = 0; i < 8; i++) k.v[i] = POSEIDON_RC[3 * r + j][i];   // wave-uniform address: scalar loads
            u[j] = fe_reduce_full(fe_add_raw<Stark252>(s[j], k));             // < 11p -> canonical
        }
        u[2] = poseidon_cube(u[2]);                                           // < 2p
        if (r < POSEIDON_FIRST_PARTIAL || r >= POSEIDON_FIRST_LAST_FULL) {    // wave-uniform branch
            u[0] = poseidon_cube(u[0]);                                       // < 2p
            u[1] = poseidon_cube(u[1]);                                       // < 2p
        }
        // mix: u_j < 2p each
        const PFe ab = fe_add_raw<Stark252>(u[0], u[1]);                      // < 4p
        const PFe t = fe_add_raw<Stark252>(ab, u[2]);                         // < 6p
        const PFe nb = fe_neg_raw_2p<Stark252>(u[1]);                         // 2p - u1 in (0, 2p]
        const PFe nc = fe_neg_raw_2p<Stark252>(u[2]);                         // 2p - u2 in (0, 2p]
        s[0] = fe_add_raw<Stark252>(fe_add_raw<Stark252>(t, u[0]), u[0]);     // t + 2 u0 < 10p
        s[1] = fe_add_raw<Stark252>(fe_add_raw<Stark252>(t, nb), nb);         // t - 2 u1 + 4p < 8p
        s[2] = fe_add_raw<Stark252>(fe_add_raw<Stark252>(ab, nc), nc);        // t - 3 u2 + 4p < 8p
    }
#pragma unroll
    for (int j = 0; j < 3; j++) s[j] = fe_reduce_full(s[j]);                  // < 10p -> canonical
}

}  // namespace lw
