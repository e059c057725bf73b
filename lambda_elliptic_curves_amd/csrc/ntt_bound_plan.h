// Bound plan of a lazy (Stark252, F::LAZY) NTT pass: which stages may subtract without adding 2p first, and the multiple
// of p that buys it.  Plain integers only, for device and host code alike.
//
// A lazy butterfly is x' = a + t, y' = a + 2p - t with a product t < 2p (t < p on the unit-twiddle path).  The + 2p only
// keeps a - t from going negative, so a stage whose a operands are known to be at least 2p can leave it out ("free" stage).
// The pass buys that lower bound where it touches the operands anyway: the elements its first stage adds are rewritten on
// load as x - (x >> 251) p + c p (fe_reduce_offset; x + c p in a first pass, whose inputs are below p).  With
// x - (x >> 251) p in (-2^202, p] they start in (c p - 2^202, (c + 1) p], and every stage, free or not, lowers the
// guaranteed minimum by at most 2p and raises the maximum by at most 2p.
//
// In units of p, with the 2^202 rounded up to a whole p:
//   before stage s the a operands are above (c - 1 - 2s) p: stage s is free if c - 1 - 2s >= 2;
//   after the r stages of the pass every value is at most (c + 1 + 2r) p, which has to stay below 2^256: 31 p < 2^256 < 32 p.
// Free stages are a prefix 0 .. nfree - 1 of the pass and cost c = 2 nfree + 1; the plan takes the longest prefix that
// still fits: r <= 7 -> all r stages (c = 2r + 1, top (4r + 2) p <= 30 p); r = 8 -> six stages, c = 13, top 30 p (a seventh
// would need c = 15 and reach 32 p).  tests/test_ntt_bound_plan_cpu.py repeats the argument with exact integers.
#pragma once

namespace lw {

constexpr int NTT_LAZY_MAX_STAGES = 8;    // plan_passes never plans a longer pass
constexpr int NTT_LAZY_TOP_MULTIPLE = 31; // largest k with k p < 2^256 for p = 2^251 + 17 * 2^192 + 1

struct NttBoundPlan {
    int c;       // multiple of p added to the elements the first stage adds, on load (>= 1: the reduction alone can be negative)
    int nfree;   // stages 0 .. nfree - 1 of the pass subtract without the + 2p
};

// the two guarantees, in units of p: every free stage sees a >= 2p, and nothing reaches 2^256 in r stages
constexpr bool ntt_bound_plan_holds(int r, NttBoundPlan b) {
    if (b.c < 1 || b.nfree < 0 || b.nfree > r) return false;
    for (int s = 0; s < b.nfree; s++)
        if (b.c - 1 - 2 * s < 2) return false;
    return b.c + 1 + 2 * r <= NTT_LAZY_TOP_MULTIPLE;
}

constexpr NttBoundPlan ntt_bound_plan(int r) {
    for (int nfree = r; nfree > 0; nfree--) {
        const NttBoundPlan b = {2 * nfree + 1, nfree};
        if (ntt_bound_plan_holds(r, b)) return b;
    }
    return NttBoundPlan{1, 0};   // today's range: (p - 2^202, 2p] in, at most (2 + 2r) p out
}

constexpr bool ntt_bound_plans_hold() {
    for (int r = 1; r <= NTT_LAZY_MAX_STAGES; r++)
        if (!ntt_bound_plan_holds(r, ntt_bound_plan(r))) return false;
    return true;
}
static_assert(ntt_bound_plans_hold(), "lazy NTT pass: a free stage below 2p or a value at 2^256");
static_assert(ntt_bound_plan(8).c == 13 && ntt_bound_plan(8).nfree == 6, "8 stages: 13p on load, stages 0-5 free");
static_assert(ntt_bound_plan(7).c == 15 && ntt_bound_plan(7).nfree == 7, "7 stages: 15p on load, all free");
static_assert(ntt_bound_plan(6).c == 13 && ntt_bound_plan(6).nfree == 6, "6 stages: 13p on load, all free");
static_assert(!ntt_bound_plan_holds(8, NttBoundPlan{15, 7}) && !ntt_bound_plan_holds(8, NttBoundPlan{14, 7}),
              "8 stages with seven free: 14p starts too low, 15p ends at 32p");

}  // namespace lw
