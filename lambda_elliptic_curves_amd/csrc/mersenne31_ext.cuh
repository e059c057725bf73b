// The extensions of Mersenne31 a circle STARK draws its challenges from, on the m31_* of circle.cuh:
//   CM31 = F_p[i] / (i^2 + 1)            Cm31 {a, b} = a + b i                        (Degree2ExtensionField)
//   QM31 = CM31[u] / (u^2 - (2 + i))     Qm31 {c0, c1, c2, c3} = (c0 + c1 i) + (c2 + c3 i) u   (Degree4ExtensionField)
// of math/src/field/fields/mersenne31/extensions.rs, and the host tables of mersenne31_ext.hip (plain arithmetic, no
// device: tests/mersenne31_ext_host_main.cpp runs them under sanitizers).
//
// Representation.  Every coordinate lives in the WEAK range [0, p] of circle.cuh (p is a second spelling of zero); words
// read from a caller go through m31_from_word, words handed back through m31_canon (m31q_load / m31q_store).  Bounds:
//   m31_red64(t)    any u64 -> [0, p]: s = (t & p) + (t >> 31) <= p + 2^33 - 1; r = (s & p) + (s >> 31) <= p + 7 fits a u32;
//                   one m31_fold of r <= 2^31 + 6 gives at most max(p, 7)
//   a product of two coordinates is at most p^2 < 2^62, so a u64 holds FOUR of them (4 p^2 < 2^64), or two and a few
//   words (2 p^2 + 2^34 < 2^64): a difference x y - z w is summed as x y + z (p - w), p - w in [0, p]
//   cm31_mul        two sums of two products, one m31_red64 each
//   m31q_mul        A0 B0 + (2 + i) A1 B1 and A0 B1 + A1 B0 (schoolbook, 16 products): T = A1 B1 is reduced first, then
//                   c0 = red64(a0 b0 + a1 (p - b1) + 2 T.a + (p - T.b)), c1 = red64(a0 b1 + a1 b0 + 2 T.b + T.a): two products
//                   and at most 3 p; c2, c3 are sums of four products
//   m31q_mul_base   four m31_mul
//   m31q_inv        norm = A0^2 - (2 + i) A1^2 in CM31, its inverse from ONE m31_inv of norm.a^2 + norm.b^2 (never zero for a
//                   non-zero norm: -1 is not a square mod p = 3 mod 4); 0 -> 0 because m31_inv(0) = 0 and m31_inv(p) = p
// add, sub, neg and dbl are the m31_* of each coordinate, closed over [0, p].
#pragma once
#include "circle.cuh"

#define M31Q_HD static __host__ __device__ __forceinline__

namespace lw {

M31Q_HD uint32_t m31_red64(uint64_t t) {
    const uint64_t s = (t & M31_P) + (t >> 31);
    return m31_fold((uint32_t)(s & M31_P) + (uint32_t)(s >> 31));
}
M31Q_HD uint32_t m31_neg(uint32_t a) { return M31_P - a; }   // [0, p] -> [0, p]
M31Q_HD uint64_t m31_wide(uint32_t a, uint32_t b) { return (uint64_t)a * b; }

struct Cm31 {
    uint32_t a, b;
};
struct Qm31 {
    uint32_t c0, c1, c2, c3;
};

// ---- CM31
M31Q_HD Cm31 cm31_add(Cm31 x, Cm31 y) { return Cm31{m31_add(x.a, y.a), m31_add(x.b, y.b)}; }
M31Q_HD Cm31 cm31_sub(Cm31 x, Cm31 y) { return Cm31{m31_sub(x.a, y.a), m31_sub(x.b, y.b)}; }
M31Q_HD Cm31 cm31_neg(Cm31 x) { return Cm31{m31_neg(x.a), m31_neg(x.b)}; }
M31Q_HD Cm31 cm31_dbl(Cm31 x) { return cm31_add(x, x); }
M31Q_HD Cm31 cm31_mul(Cm31 x, Cm31 y) {
    return Cm31{m31_red64(m31_wide(x.a, y.a) + m31_wide(x.b, m31_neg(y.b))), m31_red64(m31_wide(x.a, y.b) + m31_wide(x.b, y.a))};
}
M31Q_HD Cm31 cm31_mul_base(Cm31 x, uint32_t b) { return Cm31{m31_mul(x.a, b), m31_mul(x.b, b)}; }
M31Q_HD uint32_t cm31_norm(Cm31 x) { return m31_red64(m31_wide(x.a, x.a) + m31_wide(x.b, x.b)); }
// 1 / x from ninv = 1 / cm31_norm(x)
M31Q_HD Cm31 cm31_inv_with(Cm31 x, uint32_t ninv) { return Cm31{m31_mul(x.a, ninv), m31_mul(m31_neg(x.b), ninv)}; }
M31Q_HD Cm31 cm31_inv(Cm31 x) { return cm31_inv_with(x, m31_inv(cm31_norm(x))); }
// (2 + i)(a + b i) = (2a - b) + (2b + a) i: mul_fp2_by_nonresidue
M31Q_HD Cm31 cm31_nonresidue(Cm31 x) { return Cm31{m31_sub(m31_add(x.a, x.a), x.b), m31_add(m31_add(x.b, x.b), x.a)}; }

// ---- QM31
M31Q_HD Qm31 m31q_zero() { return Qm31{0, 0, 0, 0}; }
M31Q_HD Qm31 m31q_one() { return Qm31{1, 0, 0, 0}; }
M31Q_HD Qm31 m31q_make(Cm31 lo, Cm31 hi) { return Qm31{lo.a, lo.b, hi.a, hi.b}; }
M31Q_HD Cm31 m31q_lo(Qm31 x) { return Cm31{x.c0, x.c1}; }
M31Q_HD Cm31 m31q_hi(Qm31 x) { return Cm31{x.c2, x.c3}; }
M31Q_HD Qm31 m31q_from_words(const uint32_t *w) { return Qm31{m31_from_word(w[0]), m31_from_word(w[1]), m31_from_word(w[2]), m31_from_word(w[3])}; }
M31Q_HD Qm31 m31q_canon(Qm31 x) { return Qm31{m31_canon(x.c0), m31_canon(x.c1), m31_canon(x.c2), m31_canon(x.c3)}; }
M31Q_HD bool m31q_is_zero(Qm31 x) { return (m31_canon(x.c0) | m31_canon(x.c1) | m31_canon(x.c2) | m31_canon(x.c3)) == 0; }
M31Q_HD Qm31 m31q_add(Qm31 x, Qm31 y) { return Qm31{m31_add(x.c0, y.c0), m31_add(x.c1, y.c1), m31_add(x.c2, y.c2), m31_add(x.c3, y.c3)}; }
M31Q_HD Qm31 m31q_sub(Qm31 x, Qm31 y) { return Qm31{m31_sub(x.c0, y.c0), m31_sub(x.c1, y.c1), m31_sub(x.c2, y.c2), m31_sub(x.c3, y.c3)}; }
M31Q_HD Qm31 m31q_neg(Qm31 x) { return Qm31{m31_neg(x.c0), m31_neg(x.c1), m31_neg(x.c2), m31_neg(x.c3)}; }
M31Q_HD Qm31 m31q_conj(Qm31 x) { return Qm31{x.c0, x.c1, m31_neg(x.c2), m31_neg(x.c3)}; }   // sigma: u -> -u
M31Q_HD Qm31 m31q_mul(Qm31 x, Qm31 y) {
    const Cm31 t = cm31_mul(m31q_hi(x), m31q_hi(y));
    const uint32_t nb1 = m31_neg(y.c1), nb3 = m31_neg(y.c3);
    return Qm31{m31_red64(m31_wide(x.c0, y.c0) + m31_wide(x.c1, nb1) + ((uint64_t)t.a + t.a + m31_neg(t.b))),
                m31_red64(m31_wide(x.c0, y.c1) + m31_wide(x.c1, y.c0) + ((uint64_t)t.b + t.b + t.a)),
                m31_red64(m31_wide(x.c0, y.c2) + m31_wide(x.c1, nb3) + m31_wide(x.c2, y.c0) + m31_wide(x.c3, nb1)),
                m31_red64(m31_wide(x.c0, y.c3) + m31_wide(x.c1, y.c2) + m31_wide(x.c2, y.c1) + m31_wide(x.c3, y.c0))};
}
M31Q_HD Qm31 m31q_sqr(Qm31 x) { return m31q_mul(x, x); }
M31Q_HD Qm31 m31q_mul_base(Qm31 x, uint32_t b) { return Qm31{m31_mul(x.c0, b), m31_mul(x.c1, b), m31_mul(x.c2, b), m31_mul(x.c3, b)}; }
M31Q_HD Qm31 m31q_mul_cm31(Qm31 x, Cm31 y) { return m31q_make(cm31_mul(m31q_lo(x), y), cm31_mul(m31q_hi(x), y)); }
M31Q_HD Qm31 m31q_inv(Qm31 x) {
    const Cm31 lo = m31q_lo(x), hi = m31q_hi(x);
    const Cm31 n = cm31_inv(cm31_sub(cm31_mul(lo, lo), cm31_nonresidue(cm31_mul(hi, hi))));
    return m31q_make(cm31_mul(lo, n), cm31_mul(cm31_neg(hi), n));
}
M31Q_HD Qm31 m31q_times_u(Qm31 x) { return m31q_make(cm31_nonresidue(m31q_hi(x)), m31q_lo(x)); }
// pi(x) = 2 x^2 - 1, the x of the doubled point
M31Q_HD Qm31 m31q_pi(Qm31 x) {
    Qm31 s = m31q_sqr(x);
    s = m31q_add(s, s);
    s.c0 = m31_sub(s.c0, 1u);
    return s;
}

// ---------------------------------------------------------------- host tables
constexpr int M31Q_THREADS = 256;
constexpr int M31Q_E = 8;         // evaluate: consecutive coefficients per work-item, the low 3 bits of k
constexpr int M31Q_E_LOG = 3;
constexpr int M31Q_STEPS = 8;     // log2(M31Q_THREADS) steps of a block fold
constexpr int M31Q_TILE_LOG = M31Q_E_LOG + M31Q_STEPS;   // 2048 coefficients per block
constexpr int M31Q_PTS = 4;       // points per launch, evaluate and DEEP
constexpr int M31Q_ROWS = 4;      // DEEP rows per work-item: M31Q_ROWS x M31Q_PTS norms share one m31_inv
constexpr int M31Q_MAX_LOG = 30;  // the standard coset needs g_{2n} in a group of order 2^31

// a point (X, Y) of QM31^2 from its 8 words
struct M31qPoint {
    Qm31 x, y;
};
static inline M31qPoint m31q_point_of(const uint32_t *w) { return M31qPoint{m31q_canon(m31q_from_words(w)), m31q_canon(m31q_from_words(w + 4))}; }

// The basis at a point, B_k = y^(bit 0 of k) prod_{j >= 1} pi^(j-1)(x)^(bit j of k): the values of the low M31Q_E indices
// and the factor of every higher bit.  Canonical.
struct M31qBasis {
    Qm31 lo[M31Q_E];          // B_e(X, Y), e < 8
    Qm31 f[M31Q_MAX_LOG];     // f[j] = pi^(j-1)(X), the factor of bit j (f[0] = Y)
};
static inline void m31q_basis_tables(M31qPoint p, M31qBasis &t) {
    t.f[0] = p.y;
    t.f[1] = p.x;
    for (int j = 2; j < M31Q_MAX_LOG; j++) t.f[j] = m31q_canon(m31q_pi(t.f[j - 1]));
    for (int e = 0; e < M31Q_E; e++) {
        Qm31 v = m31q_one();
        for (int j = 0; j < M31Q_E_LOG; j++)
            if ((e >> j) & 1) v = m31q_mul(v, t.f[j]);
        t.lo[e] = m31q_canon(v);
    }
}

// The DEEP quotient by the line through P = (X, Y) and sigma P.  With X = X0 + X1 u, Y = Y0 + Y1 u the denominator is
// D(x, y) = u d(x, y), d = dA x + dB y + dC in CM31 with dA = 2 Y1, dB = -2 X1, dC = 2 (X1 Y0 - X0 Y1), and c = sigma Y - Y
// = -2 Y1 u, so that 1 / u cancels in c / D = -2 Y1 / d =: cc / d.  The host folds cc into the weights and 1 / u into the
// two constant sums:   out[i] += ( sum_k (cc w_k) col_k[i] - y_i sa - sb ) / d(x_i, y_i),
// sa = u^-1 sum_k w_k (sigma v_k - v_k), sb = u^-1 sum_k w_k b_k, b_k = v_k c - (sigma v_k - v_k) Y.
struct M31qDeepPoint {
    Cm31 da, db, dc, cc;
    Qm31 sa, sb;
};
static inline bool m31q_point_is_self_conjugate(M31qPoint p) { return (p.x.c2 | p.x.c3 | p.y.c2 | p.y.c3) == 0; }   // canonical words
// weights, evals: the n_cols x m tables of the call (4 words per scalar, row k, column j); j: the point's column
static inline M31qDeepPoint m31q_deep_point(M31qPoint p, const uint32_t *weights, const uint32_t *evals, uint32_t n_cols, uint32_t m, uint32_t j) {
    const Cm31 x0 = m31q_lo(p.x), x1 = m31q_hi(p.x), y0 = m31q_lo(p.y), y1 = m31q_hi(p.y);
    M31qDeepPoint d;
    d.da = cm31_dbl(y1);
    d.db = cm31_neg(cm31_dbl(x1));
    d.dc = cm31_dbl(cm31_sub(cm31_mul(x1, y0), cm31_mul(x0, y1)));
    d.cc = cm31_neg(cm31_dbl(y1));
    const Qm31 c = m31q_sub(m31q_conj(p.y), p.y);
    Qm31 sa = m31q_zero(), sb = m31q_zero();
    for (uint32_t k = 0; k < n_cols; k++) {
        const Qm31 w = m31q_from_words(weights + 4 * ((size_t)k * m + j)), v = m31q_from_words(evals + 4 * ((size_t)k * m + j));
        const Qm31 a = m31q_sub(m31q_conj(v), v), b = m31q_sub(m31q_mul(v, c), m31q_mul(a, p.y));
        sa = m31q_add(sa, m31q_mul(w, a));
        sb = m31q_add(sb, m31q_mul(w, b));
    }
    const Qm31 uinv = m31q_inv(Qm31{0, 0, 1, 0});
    d.sa = m31q_canon(m31q_mul(sa, uinv));
    d.sb = m31q_canon(m31q_mul(sb, uinv));
    return d;
}
// the n_cols x m weights, each times its point's cc, as ceil(m / M31Q_PTS) groups of [n_cols][M31Q_PTS]; zero where a
// group has no point
static inline void m31q_regroup_weights(const uint32_t *weights, const M31qDeepPoint *pts, uint32_t n_cols, uint32_t m, Qm31 *out) {
    const size_t groups = (m + M31Q_PTS - 1) / M31Q_PTS;
    for (size_t i = 0; i < groups * n_cols * M31Q_PTS; i++) out[i] = m31q_zero();
    for (uint32_t k = 0; k < n_cols; k++)
        for (uint32_t j = 0; j < m; j++)
            out[((size_t)(j / M31Q_PTS) * n_cols + k) * M31Q_PTS + j % M31Q_PTS] =
                m31q_canon(m31q_mul_cm31(m31q_from_words(weights + 4 * ((size_t)k * m + j)), pts[j].cc));
}

// the standard coset of size 2^log2n: its first point g_{2n} and the steps 2^b g_n, b < log2n
struct M31qCoset {
    CirclePt shift;
    CirclePt step[M31Q_MAX_LOG];
};
static inline M31qCoset m31q_coset(uint32_t log2n) {
    CirclePt g[32];   // g[k] = g_{2^k} = 2^(31-k) G
    CirclePt q{2u, 1268011823u};   // the generator of the circle group, order 2^31 (circle/point.rs)
    for (int k = 31; k >= 0; k--) {
        g[k] = q;
        q = circle_double(q);
    }
    M31qCoset c;
    c.shift = g[log2n + 1];
    for (uint32_t b = 0; b < (uint32_t)M31Q_MAX_LOG; b++) c.step[b] = b < log2n ? g[log2n - b] : CirclePt{1u, 0u};
    return c;
}

}  // namespace lw
