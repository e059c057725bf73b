// Starknet Pedersen hash over the Stark curve (crypto/src/hash/pedersen/mod.rs, PedersenStarkCurve::hash): the curve's
// group law over Fe<Stark252>, the lookup tables and the hash of one pair, shared by the kernels of pedersen.hip.
//
// Curve: y^2 = x^3 + a x + b over the Stark252 prime, a = 1 (math/src/elliptic_curve/short_weierstrass/curves/stark_curve.rs).
// ec.cuh is a = 0 only and lives on FpOps fields, so the law is written here.
//
// hash(x, y), x and y canonical integers below p < 2^252 (mod.rs:43-54):
//     acc = P0;  for i in 0 .. 62:  k = nibble i of x;  if k: acc += T[15 i + k - 1]
//                for i in 0 .. 62:  k = nibble i of y;  if k: acc += T[945 + 15 i + k - 1]
//     hash = affine x of acc
// T = T1 || T2 || T3 || T4 (930 + 15 + 930 + 15 = 1 890 affine points): T1[15 i + k - 1] = k 2^(4 i) P1 for the 62 nibbles of
// the low 248 bits, T2[k - 1] = k P2 for bits 248 .. 251 (k <= 8), T3, T4 the same from P3, P4.  T2 follows T1 directly, so
// nibble 62 is one more row of the same loop.  The four bases are independent points: P2 is not 2^248 P1.  The tables are
// GENERATED from StarkWare's five published points (pedersen_fill_table, on the host, once per process) and uploaded to
// PEDERSEN_TABLE on first use; nothing is copied from the reference's constants.
//
// Accumulator: Jacobian (X, Y, Z), x = X / Z^2, y = Y / Z^3, Z = 0 the point at infinity; table points are affine.  The
// addition is the incomplete mixed addition (Cohen-Miyaji-Ono 1998; "madd" of the Explicit-Formulas Database) with
// wave-divergent fallbacks:
//     ZZ = Z1^2, U2 = x2 ZZ, S2 = y2 Z1 ZZ, H = U2 - X1, r = S2 - Y1
//     HH = H^2, HHH = H HH, V = X1 HH;  X3 = r^2 - HHH - 2V,  Y3 = r (V - X3) - Y1 HHH,  Z3 = Z1 H
// 11 products (8 M + 3 S), every intermediate canonical.  A complete formula for general a (Renes-Costello-Batina 2016,
// algorithm 2 with a = 1) is 13 products per mixed addition; the fallbacks cost nothing until a lane meets them:
//     Z1 = 0            the sum is (x2, y2, 1)
//     H = 0, r = 0      acc = Q: the doubling of the affine Q with a = 1, 6 products (2 M + 4 S), Z3 = 2 y2
//     H = 0, r != 0     acc = -Q: infinity, Z3 = Z1 H = 0 falls out of the formula
// No hash input reaches the last two (it would take a discrete logarithm between the bases); they are exercised through
// pedersen_add_affine_kernel (lw_pedersen_add_affine_device), which calls the same ped_add_affine and ped_to_affine.
//
// Lookups are plain global loads: at step i every lane of a wave reads one of 15 points (960 bytes) of row i, at most 15
// cache lines a step, and the whole table is 118 KiB, resident in L2 beside any input.  A device function that stages
// nothing is what the tree policy (hash_tree.cuh) needs.  An LDS-staged flat kernel (the table fits the 160 KiB of a CU,
// at one workgroup per CU) was not built: NOT MEASURED.
//
// The affine x costs one inversion per hash (fe_inv_fast, the bounded binary GCD: ~85 products' worth of VALU work) plus
// 3 products.  Montgomery's trick across the work-items of a workgroup (3 products per hash and one inversion per
// workgroup, at the price of LDS traffic and barriers the tree policy cannot have) was not built: NOT MEASURED.
#pragma once
#include "field.cuh"

namespace lw {

typedef Fe<Stark252> SFe;
constexpr int PEDERSEN_ROW = 15;                          // non-zero values of a nibble
constexpr int PEDERSEN_CHUNKS = 63;                       // nibbles of a value below 2^252: 62 of T1 (T3), one of T2 (T4)
constexpr int PEDERSEN_HALF = PEDERSEN_CHUNKS * PEDERSEN_ROW;   // 945: T1 || T2
constexpr int PEDERSEN_POINTS = 2 * PEDERSEN_HALF;        // 1 890
constexpr size_t PEDERSEN_TABLE_BYTES = (size_t)PEDERSEN_POINTS * 64;   // 120 960

struct PedAffine { SFe x, y; };
struct PedJac { SFe x, y, z; };

// point i as (x, y), each in the boundary layout (4 u64, most significant first, Montgomery form): what
// lw_pedersen_table returns, byte for byte
#if defined(__HIPCC__)
static __device__ uint4 PEDERSEN_TABLE[PEDERSEN_POINTS * 4];
#endif

LW_HD PedAffine ped_load_affine(const void *p) {
    PedAffine q;
    q.x = fe_load<Stark252>(p);
    q.y = fe_load<Stark252>((const char *)p + 32);
    return q;
}

// 2 Q for an affine Q, a = 1 ("mdbl-2007-bl"): y = 0 gives Z3 = 0
LW_HD PedJac ped_dbl_affine(const PedAffine &q) {
    const SFe xx = fe_sqr<Stark252>(q.x), yy = fe_sqr<Stark252>(q.y), yyyy = fe_sqr<Stark252>(yy);
    SFe s = fe_sqr<Stark252>(fe_add<Stark252>(q.x, yy));
    s = fe_dbl<Stark252>(fe_sub<Stark252>(fe_sub<Stark252>(s, xx), yyyy));               // 4 x y^2
    const SFe m = fe_add<Stark252>(fe_add<Stark252>(fe_dbl<Stark252>(xx), xx), SFe::one());   // 3 x^2 + a
    PedJac r;
    r.x = fe_sub<Stark252>(fe_sqr<Stark252>(m), fe_dbl<Stark252>(s));
    const SFe y8 = fe_dbl<Stark252>(fe_dbl<Stark252>(fe_dbl<Stark252>(yyyy)));
    r.y = fe_sub<Stark252>(fe_mul<Stark252>(m, fe_sub<Stark252>(s, r.x)), y8);
    r.z = fe_dbl<Stark252>(q.y);
    return r;
}

// acc + Q for every acc and every affine Q on the curve (see the head of the file); canonical in, canonical out
LW_HD PedJac ped_add_affine(const PedJac &p, const PedAffine &q) {
    const SFe zz = fe_sqr<Stark252>(p.z);
    const SFe u2 = fe_mul<Stark252>(q.x, zz);
    const SFe s2 = fe_mul<Stark252>(q.y, fe_mul<Stark252>(p.z, zz));
    const SFe h = fe_sub<Stark252>(u2, p.x), r = fe_sub<Stark252>(s2, p.y);
    const SFe hh = fe_sqr<Stark252>(h);
    const SFe hhh = fe_mul<Stark252>(h, hh);
    const SFe v = fe_mul<Stark252>(p.x, hh);
    PedJac o;
    o.x = fe_sub<Stark252>(fe_sub<Stark252>(fe_sqr<Stark252>(r), hhh), fe_dbl<Stark252>(v));
    o.y = fe_sub<Stark252>(fe_mul<Stark252>(r, fe_sub<Stark252>(v, o.x)), fe_mul<Stark252>(p.y, hhh));
    o.z = fe_mul<Stark252>(p.z, h);                     // acc = -Q: h = 0, infinity
    if (p.z.is_zero()) {                                // infinity + Q
        o.x = q.x;
        o.y = q.y;
        o.z = SFe::one();
    } else if (h.is_zero() && r.is_zero()) {            // acc = Q
        o = ped_dbl_affine(q);
    }
    return o;
}

// affine (x, y) of acc, (0, 0) for infinity (b != 0: not a point of the curve); one inversion, 4 products
LW_HD PedAffine ped_to_affine(const PedJac &p) {
    const SFe zi = fe_inv_fast<Stark252>(p.z);          // 0 -> 0
    const SFe zi2 = fe_sqr<Stark252>(zi);
    PedAffine a;
    a.x = fe_mul<Stark252>(p.x, zi2);
    a.y = fe_mul<Stark252>(p.y, fe_mul<Stark252>(zi, zi2));
    return a;
}

// PedersenStarkCurve::hash of the canonical Montgomery elements x, y; `table`: the 1 890 points, 64 bytes each
LW_HD SFe pedersen_hash(const SFe &x, const SFe &y, const void *table) {
    PedJac acc;
    {
        // P0, the shift point, canonical limbs least significant first
        SFe px, py;
        const uint32_t p0x[8] = {0x50ca6804u, 0x551fde40u, 0x22947733u, 0x716b0b10u, 0xeb599f16u, 0x00ee1b87u, 0xa8c16007u, 0x049ee3ebu};
        const uint32_t p0y[8] = {0x6e10268au, 0xd0405d26u, 0xc0e056c1u, 0x4e621062u, 0x06ea0ed3u, 0xf346d49du, 0x4b3bc6ddu, 0x03ca0cfeu};
#pragma unroll
        for (int i = 0; i < 8; i++) {
            px.v[i] = p0x[i];
            py.v[i] = p0y[i];
        }
        acc.x = fe_to_mont<Stark252>(px);
        acc.y = fe_to_mont<Stark252>(py);
        acc.z = SFe::one();
    }
    const char *row = (const char *)table;
#pragma unroll 1
    for (int half = 0; half < 2; half++) {
        SFe e = fe_from_mont<Stark252>(half ? y : x);   // the canonical integer: its nibbles index the table
#pragma unroll 1
        for (int i = 0; i < PEDERSEN_CHUNKS; i++) {
            const uint32_t k = e.v[0] & 15u;
#pragma unroll
            for (int j = 0; j < 7; j++) e.v[j] = (e.v[j] >> 4) | (e.v[j + 1] << 28);
            e.v[7] >>= 4;
            if (k) acc = ped_add_affine(acc, ped_load_affine(row + (size_t)(k - 1) * 64));
            row += PEDERSEN_ROW * 64;
        }
    }
    return ped_to_affine(acc).x;
}

// ---- the tables, generated on the host: affine arithmetic, one inversion per point (1 890 in all, once per process)
inline PedAffine ped_host_add(const PedAffine &p, const PedAffine &q) {   // p, q finite, p != -q
    SFe lam;
    if (p.x == q.x) {
        const SFe xx = fe_sqr<Stark252>(p.x);
        lam = fe_mul<Stark252>(fe_add<Stark252>(fe_add<Stark252>(fe_dbl<Stark252>(xx), xx), SFe::one()), fe_inv_fast<Stark252>(fe_dbl<Stark252>(p.y)));
    } else {
        lam = fe_mul<Stark252>(fe_sub<Stark252>(q.y, p.y), fe_inv_fast<Stark252>(fe_sub<Stark252>(q.x, p.x)));
    }
    PedAffine r;
    r.x = fe_sub<Stark252>(fe_sub<Stark252>(fe_sqr<Stark252>(lam), p.x), q.x);
    r.y = fe_sub<Stark252>(fe_mul<Stark252>(lam, fe_sub<Stark252>(p.x, r.x)), p.y);
    return r;
}
// out: PEDERSEN_TABLE_BYTES, T1 || T2 || T3 || T4 in the boundary layout
inline void pedersen_fill_table(void *out) {
    // P1 .. P4 (x, y), canonical u64 limbs most significant first: StarkWare's published Pedersen parameters
    alignas(16) static const uint64_t BASES[4][2][4] = {
        {{0x0234287dcbaffe7full, 0x969c748655fca9e5ull, 0x8fa8120b6d56eb0cull, 0x1080d17957ebe47bull},
         {0x03b056f100f96fb2ull, 0x1e889527d41f4e39ull, 0x940135dd7a6c94ccull, 0x6ed0268ee89e5615ull}},
        {{0x04fa56f376c83db3ull, 0x3f9dab2656558f33ull, 0x99099ec1de5e3018ull, 0xb7a6932dba8aa378ull},
         {0x03fa0984c931c9e3ull, 0x8113e0c0e47e4401ull, 0x562761f92a7a23b4ull, 0x5168f4e80ff5b54dull}},
        {{0x04ba4cc166be8decull, 0x764910f75b45f74bull, 0x40c690c74709e90full, 0x3aa372f0bd2d6997ull},
         {0x0040301cf5c1751full, 0x4b971e46c4ede85full, 0xcac5c59a5ce5ae7cull, 0x48151f27b24b219cull}},
        {{0x054302dcb0e6cc1cull, 0x6e44cca8f61a63bbull, 0x2ca65048d53fb325ull, 0xd36ff12c49a58202ull},
         {0x01b77b3e37d13504ull, 0xb348046268d8ae25ull, 0xce98ad783c25561aull, 0x879dcc77e99c2426ull}},
    };
    char *dst = (char *)out;
    for (int t = 0; t < 4; t++) {
        PedAffine base;
        base.x = fe_to_mont<Stark252>(fe_load<Stark252>(BASES[t][0]));
        base.y = fe_to_mont<Stark252>(fe_load<Stark252>(BASES[t][1]));
        const int chunks = (t & 1) ? 1 : PEDERSEN_CHUNKS - 1;
        for (int i = 0; i < chunks; i++) {
            PedAffine acc = base;
            for (int k = 1; k <= PEDERSEN_ROW; k++) {
                fe_store<Stark252>(dst, acc.x);
                fe_store<Stark252>(dst + 32, acc.y);
                dst += 64;
                acc = ped_host_add(acc, base);
            }
            base = acc;   // 16 times the row's base
        }
    }
}

}  // namespace lw
