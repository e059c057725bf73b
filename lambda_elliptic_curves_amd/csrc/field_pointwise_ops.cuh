// The op table of the field-arithmetic test seam (lw_hip_field_pointwise_device, include/lw_hip.h): fe_pointwise<F, OP>
// calls exactly one primitive of field.cuh on the operands of one row and returns what it returned.  There is no
// arithmetic in this file.  Two builds include it: the device kernel (field_pointwise.hip) and a stand-alone host program
// of the test suite (tests/field_pointwise_host_main.cpp), which runs the shared non-asm code (carry chains, reduce_once,
// fe_reduce_full, fe_cond_sub_kp, the raw adds, the host products, bb_*) under the sanitizers at the same operands.
//
// Operand domains, as stored integers (N = F::N 32-bit limbs, p the modulus).  The tests stay inside them; outside, the
// primitive's result is whatever its carry chains give.
//   ADD, SUB, NEG, DBL     a, b < p                                          -> canonical (< p)
//   MUL                    one operand < p, the other any N-limb value, in either order   -> canonical
//   SQR                    a < p                                             -> canonical
//   MUL_LAZY               a < p, b any N-limb value                         -> raw, in [0, 2p): (a*b + m*p) / R, not reduced
//   MUL_LAZY_UNIFORM       as MUL_LAZY; a is the same for every row and reaches the call through an address that does
//                          not depend on the work-item (the kernel's business)   -> the limbs of MUL_LAZY
//   REDUCE_FULL            Stark252: any 256-bit value; other fields: a < 2p   -> canonical
//   COND_SUB_P             any N-limb value                                  -> a - p if a >= p, else a
//   ADD_RAW                a + b < 2^(32N)                                   -> a + b
//   ADD2P_SUB_RAW          b <= a + 2p and a + 2p - b < 2^(32N)              -> a + 2p - b
//   NEG_RAW                a <= p                                            -> p - a
//   NEG_RAW_2P             a <= 2p                                           -> 2p - a
//   TO_MONT, FROM_MONT     a < p                                             -> canonical
//   DOT2, DOT4             2 / 4 elements per row in a and in b, each <= p (p itself allowed: fe_neg_raw(0) is p)
//                          -> canonical.  Only where fe_dot's static_assert holds: fpw_has_op<F, OP>()
//   INV                    a < p                                             -> canonical, 0 -> 0
// BabyBear (bb_pointwise<OP>, words in u64 registers):
//   MUL, ADD, SUB          words < p                                         -> canonical
//   REDUCE64               a u64 below p * 2^32                              -> canonical
//   FROM_R64               a u64 below p                                     -> canonical
//   TO_R64                 a word < p                                        -> a u64 below p
#pragma once
#include "../../include/lw_hip.h"
#include "field.cuh"

namespace lw {

// elements per row of d_a (and of d_b, where the op has one)
LW_HD constexpr int fpw_row_elems(int op) { return op == LW_FIELD_OP_DOT2 ? 2 : op == LW_FIELD_OP_DOT4 ? 4 : 1; }
// the op reads d_b
LW_HD constexpr bool fpw_two_operands(int op) {
    return op == LW_FIELD_OP_ADD || op == LW_FIELD_OP_SUB || op == LW_FIELD_OP_MUL || op == LW_FIELD_OP_MUL_LAZY ||
           op == LW_FIELD_OP_MUL_LAZY_UNIFORM || op == LW_FIELD_OP_ADD_RAW || op == LW_FIELD_OP_ADD2P_SUB_RAW ||
           op == LW_FIELD_OP_DOT2 || op == LW_FIELD_OP_DOT4;
}
// a multi-limb field has the op: every op up to INV, fe_dot only with the products its static_assert admits
template <class F, int OP>
LW_HD constexpr bool fpw_has_op() {
    if (OP < LW_FIELD_OP_ADD || OP > LW_FIELD_OP_INV) return false;
    if (OP == LW_FIELD_OP_DOT2 || OP == LW_FIELD_OP_DOT4)
        return (uint64_t)fpw_row_elems(OP) * ((uint64_t)F::p(F::N - 1) + 1) <= (1ull << 32);
    return true;
}

// a, b: the row's fpw_row_elems(OP) elements (b unused where the op has one operand)
template <class F, int OP>
LW_HD Fe<F> fe_pointwise(const Fe<F> *a, const Fe<F> *b) {
    static_assert(fpw_has_op<F, OP>(), "the field does not have this op");
    if constexpr (OP == LW_FIELD_OP_ADD) return fe_add<F>(a[0], b[0]);
    else if constexpr (OP == LW_FIELD_OP_SUB) return fe_sub<F>(a[0], b[0]);
    else if constexpr (OP == LW_FIELD_OP_NEG) return fe_neg<F>(a[0]);
    else if constexpr (OP == LW_FIELD_OP_DBL) return fe_dbl<F>(a[0]);
    else if constexpr (OP == LW_FIELD_OP_MUL) return fe_mul<F>(a[0], b[0]);
    else if constexpr (OP == LW_FIELD_OP_SQR) return fe_sqr<F>(a[0]);
    else if constexpr (OP == LW_FIELD_OP_MUL_LAZY) return fe_mul_lazy<F>(a[0], b[0]);
    else if constexpr (OP == LW_FIELD_OP_MUL_LAZY_UNIFORM) return fe_mul_lazy_uniform<F>(a[0], b[0]);
    else if constexpr (OP == LW_FIELD_OP_REDUCE_FULL) return fe_reduce_full(a[0]);   // overload resolution picks Stark252's
    else if constexpr (OP == LW_FIELD_OP_COND_SUB_P) return fe_cond_sub_kp<F, 0>(a[0]);
    else if constexpr (OP == LW_FIELD_OP_ADD_RAW) return fe_add_raw<F>(a[0], b[0]);
    else if constexpr (OP == LW_FIELD_OP_ADD2P_SUB_RAW) return fe_add2p_sub_raw<F>(a[0], b[0]);
    else if constexpr (OP == LW_FIELD_OP_NEG_RAW) return fe_neg_raw<F>(a[0]);
    else if constexpr (OP == LW_FIELD_OP_NEG_RAW_2P) return fe_neg_raw_2p<F>(a[0]);
    else if constexpr (OP == LW_FIELD_OP_TO_MONT) return fe_to_mont<F>(a[0]);
    else if constexpr (OP == LW_FIELD_OP_FROM_MONT) return fe_from_mont<F>(a[0]);
    else if constexpr (OP == LW_FIELD_OP_DOT2) {
        const Fe<F> *const pa[2] = {&a[0], &a[1]}, *const pb[2] = {&b[0], &b[1]};
        return fe_dot<F, 2>(pa, pb);
    } else if constexpr (OP == LW_FIELD_OP_DOT4) {
        const Fe<F> *const pa[4] = {&a[0], &a[1], &a[2], &a[3]}, *const pb[4] = {&b[0], &b[1], &b[2], &b[3]};
        return fe_dot<F, 4>(pa, pb);
    } else return fe_inv<F>(a[0]);
}

// ---- BabyBear: every word travels in a u64
LW_HD constexpr bool bb_has_op(int op) {
    return op == LW_FIELD_OP_MUL || op == LW_FIELD_OP_ADD || op == LW_FIELD_OP_SUB || op == LW_FIELD_OP_REDUCE64 ||
           op == LW_FIELD_OP_FROM_R64 || op == LW_FIELD_OP_TO_R64;
}
// bytes of one word of d_a (and d_b) / of d_out
LW_HD constexpr int bb_in_bytes(int op) { return op == LW_FIELD_OP_REDUCE64 || op == LW_FIELD_OP_FROM_R64 ? 8 : 4; }
LW_HD constexpr int bb_out_bytes(int op) { return op == LW_FIELD_OP_TO_R64 ? 8 : 4; }
template <int OP>
LW_HD uint64_t bb_pointwise(uint64_t a, uint64_t b) {
    static_assert(bb_has_op(OP), "BabyBear does not have this op");
    if constexpr (OP == LW_FIELD_OP_MUL) return bb_mul((uint32_t)a, (uint32_t)b);
    else if constexpr (OP == LW_FIELD_OP_ADD) return bb_add((uint32_t)a, (uint32_t)b);
    else if constexpr (OP == LW_FIELD_OP_SUB) return bb_sub((uint32_t)a, (uint32_t)b);
    else if constexpr (OP == LW_FIELD_OP_REDUCE64) return bb_reduce(a);
    else if constexpr (OP == LW_FIELD_OP_FROM_R64) return bb_from_r64(a);
    else return bb_to_r64((uint32_t)a);
}

}  // namespace lw
