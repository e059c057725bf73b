// The BabyBear quartic extension Fp4 = F_p[x] / (x^4 + 11) on the device (arithmetic: babybear_ext.cuh) as a policy of
// ext_steps.cuh, which holds the steps a STARK prover over BabyBear runs in it after round 1 (pointwise, evaluate,
// deep_quotients, fri_layer), the entry points of those steps, and the one call that is this extension's alone:
//   convert         LW_LAYOUT_EXT4_INTERLEAVED (4 x u64 per element, R = 2^64) to and from planes
// A vector of n Fp4 elements is four PLANES of n stored words (LW_LAYOUT_BABYBEAR_U32_R32), c0 then c1 `stride` words later
// and so on: the batch shape of lw_hip_ntt_device and the n_cols / col_stride shape of
// lw_stark_commit_columns_layout_device, so a transform of an Fp4 vector over a base-field domain is the existing transform
// with batch = 4 (the twiddles are in F) and nothing here re-implements a transform or a tree: the layer calls ntt_bb.hip
// through ntt_device_locked and merkle.hip (internal.h).  Every word read from a caller is below p: host scalars are
// checked, device words are the caller's promise.
//
// evaluate: the coefficients are in F, so a work-item does not run Horner in Fp4 (one bb4_mul, 19 base products, per
// coefficient and point).  It multiplies its EXT_E consecutive coefficients by the table 1, x, ..., x^(EXT_E - 1) of the
// point, which the host hands over as kernel arguments: four base products per coefficient and point, summed in 64 bits two
// products at a time (bb_mac2) and reduced once per coordinate.
// deep_quotients: the norm of x_i - z_j is bb4_norm, in F; bb4_inv_with turns a norm's inverse into 1 / (x_i - z_j).  The
// norm is never zero: x_i - z_j has a non-zero c1, c2 or c3 (checked).
#include "babybear_ext.cuh"
#include "ext_steps.cuh"
#include "ext_round2.cuh"
#include "ext_aux.cuh"

namespace lw {

struct Bb4Ext {
    using word = uint32_t;
    using elem = Bb4;
    static constexpr int D = 4;
    static constexpr const char *NAME = "Fp4";
    static constexpr ExtNames NAMES{"bb4_pointwise_kernel", "bb4_eval_tile_kernel", "bb4_eval_fold_kernel", "bb4_deep_kernel", "bb4_fri_fold_kernel"};
    static constexpr word F_ONE = BabyBear::ONE;
    EXT_HD word fcanon(word x) { return x; }
    EXT_HD word fadd(word a, word b) { return bb_add(a, b); }
    EXT_HD word fsub(word a, word b) { return bb_sub(a, b); }
    EXT_HD word fmul(word a, word b) { return bb_mul(a, b); }
    EXT_HD word fpow(word a, uint64_t e) { return bb_pow(a, e); }
    EXT_HD word finv(word a) { return bb_inv(a); }
    EXT_HD elem load(ExtPlanes<Bb4Ext> v, uint64_t i) { return Bb4{v.p[0][i], v.p[1][i], v.p[2][i], v.p[3][i]}; }
    EXT_HD void store(ExtPlanes<Bb4Ext> v, uint64_t i, elem a) {
        v.p[0][i] = a.c0;
        v.p[1][i] = a.c1;
        v.p[2][i] = a.c2;
        v.p[3][i] = a.c3;
    }
    EXT_HD elem canon(elem a) { return a; }
    EXT_HD elem zero() { return bb4_zero(); }
    EXT_HD elem one() { return Bb4{BabyBear::ONE, 0, 0, 0}; }
    EXT_HD bool is_zero(elem a) { return bb4_is_zero(a); }
    EXT_HD elem add(elem a, elem b) { return bb4_add(a, b); }
    EXT_HD elem sub(elem a, elem b) { return bb4_sub(a, b); }
    EXT_HD elem mul(elem a, elem b) { return bb4_mul(a, b); }
    EXT_HD elem sqr(elem a) { return bb4_sqr(a); }
    EXT_HD elem inv(elem a) { return bb4_inv(a); }
    EXT_HD elem mul_base(elem a, word b) { return bb4_mul_base(a, b); }

    struct eval_point {
        Bb4 xp[EXT_E];   // x^e, e < EXT_E
    };
    EXT_HD eval_point eval_point_of(const elem *xp) {
        eval_point pt;
        for (int e = 0; e < EXT_E; e++) pt.xp[e] = xp[e];
        return pt;
    }

    struct deep_point {
        Bb4 nz;   // -z_j: x_i - z_j = (x_i + nz.c0, nz.c1, nz.c2, nz.c3)
    };
    EXT_HD deep_point deep_point_of(elem z) { return deep_point{bb4_neg(z)}; }
    EXT_HD elem x_minus(word x, deep_point p) { return Bb4{bb_add(x, p.nz.c0), p.nz.c1, p.nz.c2, p.nz.c3}; }
    EXT_HD word norm(word x, deep_point p) {
        uint32_t b0, b2;
        return bb4_norm(x_minus(x, p), b0, b2);
    }
    // 1 / (x - z) from the norm's inverse.  b0 and b2 of the norm are computed again rather than kept from the way forward
    // (32 more live words at M = 4; not measured against keeping them).
    EXT_HD elem quotient(elem num, word x, deep_point p, word ninv) {
        const Bb4 d = x_minus(x, p);
        uint32_t b0, b2;
        bb4_norm(d, b0, b2);
        return bb4_mul(num, bb4_inv_with(d, b0, b2, ninv));
    }
    // as a loop, acc[][] indexed by a loop counter lives in scratch (272 bytes per lane at M = 4)
    static constexpr int R2_ROWS_FEW = EXT_ROWS;   // boundary rows per work-item with one or two steps (ext_round2.cuh): E::finv is short and eight 4-byte words per lane load badly: four rows throughout
    static constexpr bool DEEP_BACK_BY_RECURSION = true;

    // host: every word of a scalar below p; the domain's root is the field's own
    static int words_check(const word *words, size_t count, const char *what) {
        for (size_t i = 0; i < count; i++)
            if (words[i] >= BabyBear::P) { set_error("%s: word %zu is not below p", what, i); return LW_ERR_BAD_ARG; }
        return LW_OK;
    }
    static int size_check(uint32_t log2n) {
        if (log2n > BabyBear::TWO_ADICITY) { set_error("BabyBear has no root of unity of order 2^%u", log2n); return LW_ERR_ROOT_OF_UNITY; }
        return LW_OK;
    }
    static int root_check(uint64_t &) { return LW_OK; }
    static int offset(const word *offset_or_null, word &h) {
        h = offset_or_null ? *offset_or_null : BabyBear::ONE;
        if (h >= BabyBear::P) { set_error("coset offset is not below p"); return LW_ERR_BAD_ARG; }
        if (h == 0) { set_error("coset offset is zero"); return LW_ERR_INV_ZERO; }
        return LW_OK;
    }
    static word domain_root(uint64_t, uint32_t log2n) { return ntt_bb_root(log2n, false); }
};

}  // namespace lw

#ifndef LW_EXT_POLICY_ONLY   // tests/ext_steps_host_main.cpp takes the policy and leaves the kernels and entry points of this file
namespace lw {

// the tile sums of evaluate (ext_steps.cuh): the work-item's coefficients times the point's table
__global__ __launch_bounds__(EXT_THREADS) void bb4_eval_tile_kernel(const ExtEvalArgs<Bb4Ext> a) {
    __shared__ Bb4 lds[EXT_THREADS];
    const uint32_t k = a.k0 + blockIdx.y;
    const uint64_t t = blockIdx.x;
    const uint32_t *col = a.cols + (uint64_t)k * a.col_stride;
    const uint64_t base = t * EXT_TILE + (uint64_t)threadIdx.x * EXT_E;
    uint32_t c[EXT_E];
#pragma unroll
    for (int e = 0; e < EXT_E; e++) c[e] = base + e < a.n ? col[base + e] : 0;
#pragma unroll 1
    for (uint32_t j = 0; j < a.m; j++) {
        const Bb4 *xp = a.x[j].xp;   // uniform
        // every coordinate: EXT_E products of canonical words, two at a time onto a sum kept below p 2^32 (bb_mac2)
        uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
        for (int e = 0; e < EXT_E; e += 2) {
            s0 = bb_mac2(s0, c[e], xp[e].c0, c[e + 1], xp[e + 1].c0);
            s1 = bb_mac2(s1, c[e], xp[e].c1, c[e + 1], xp[e + 1].c1);
            s2 = bb_mac2(s2, c[e], xp[e].c2, c[e + 1], xp[e + 1].c2);
            s3 = bb_mac2(s3, c[e], xp[e].c3, c[e + 1], xp[e + 1].c3);
        }
        Bb4 h{bb_reduce(s0), bb_reduce(s1), bb_reduce(s2), bb_reduce(s3)};
        h = ext_block_fold<Bb4Ext>(h, lds, a.pe[j]);
        if (threadIdx.x == 0) a.sums[((uint64_t)k * EXT_PTS + j) * a.ntiles + t] = h;
    }
}

// ---------------------------------------------------------------- convert
// element i of the interleaved form: the four u64 words 4 i .. 4 i + 3, each a 2^64 mod p
__global__ __launch_bounds__(256) void bb4_to_planes_kernel(const uint64_t *in, uint32_t *out, uint64_t stride, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int e = 0; e < 4; e++) out[e * stride + i] = bb_from_r64(in[4 * i + e]);
}
__global__ __launch_bounds__(256) void bb4_to_interleaved_kernel(const uint32_t *in, uint64_t stride, uint64_t *out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int e = 0; e < 4; e++) out[4 * i + e] = bb_to_r64(in[e * stride + i]);
}

}  // namespace lw

using namespace lw;

extern "C" {

int lw_babybear_ext4_pointwise_device(lw_bb4_op_t op, const uint32_t *d_a, size_t a_stride, const uint32_t *d_b, size_t b_stride, uint32_t *d_out,
                                      size_t out_stride, size_t n, void *hip_stream) {
    return ext_pointwise<Bb4Ext>((int)op, d_a, a_stride, d_b, b_stride, d_out, out_stride, n, hip_stream);
}

int lw_babybear_ext4_convert_device(lw_bb4_convert_t dir, uint64_t *d_interleaved, uint32_t *d_planes, size_t plane_stride, size_t n, void *hip_stream) {
    if (dir != LW_BB4_TO_PLANES && dir != LW_BB4_TO_INTERLEAVED) { set_error("bad conversion %d", (int)dir); return LW_ERR_BAD_ARG; }
    if (n == 0) return LW_OK;
    if (n > EXT_MAX_LEN) { set_error("%zu Fp4 elements", n); return LW_ERR_ALLOC; }
    int rc = ext_device_ptrs({d_interleaved, d_planes});
    if (!rc) rc = ext_stride(plane_stride, n, "planes");
    if (rc) return rc;
    if (ext_overlap<Bb4Ext>(d_interleaved, 8 * n, d_planes, ext_span<Bb4Ext>(plane_stride, n))) { set_error("the two forms overlap"); return LW_ERR_BAD_ARG; }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    if (dir == LW_BB4_TO_PLANES)
        return launch_1d(en.c, "bb4_to_planes_kernel", bb4_to_planes_kernel, blocks_for(n), en.stream, (const uint64_t *)d_interleaved, d_planes,
                         (uint64_t)plane_stride, (uint64_t)n);
    return launch_1d(en.c, "bb4_to_interleaved_kernel", bb4_to_interleaved_kernel, blocks_for(n), en.stream, (const uint32_t *)d_planes, (uint64_t)plane_stride,
                     d_interleaved, (uint64_t)n);
}

int lw_babybear_ext4_evaluate_device(const uint32_t *d_coeffs, uint32_t n_cols, size_t col_stride, size_t n_coeffs, const uint32_t *points, uint32_t m,
                                     uint32_t *out_values, void *hip_stream) {
    return ext_evaluate<Bb4Ext>(d_coeffs, n_cols, col_stride, n_coeffs, points, m, out_values, hip_stream, bb4_eval_tile_kernel);
}

int lw_babybear_ext4_deep_quotients_device(const uint32_t *d_lde, uint32_t n_cols, size_t col_stride, uint32_t log2n, const uint32_t *offset_or_null,
                                           const uint32_t *points, uint32_t m, const uint32_t *weights, const uint32_t *evals, uint32_t *d_out,
                                           size_t out_stride, void *hip_stream) {
    return ext_deep_quotients<Bb4Ext>(d_lde, n_cols, col_stride, log2n, offset_or_null, 0, points, m, weights, evals, d_out, out_stride, hip_stream);
}

int lw_babybear_ext4_fri_layer_device(const uint32_t *d_coeffs, size_t coeff_stride, size_t n_coeffs, const uint32_t *zeta, const uint32_t *offset_or_null,
                                      size_t domain_size, uint32_t *d_out_poly, uint32_t *d_out_evaluation_or_null, uint8_t *d_nodes_or_null,
                                      uint8_t *out_root_or_null, void *hip_stream) {
    // the four planes through the existing transform, then two rows of four parts per leaf
    return ext_fri_layer<Bb4Ext>(d_coeffs, coeff_stride, n_coeffs, zeta, offset_or_null, domain_size, 0, 32, d_out_poly, d_out_evaluation_or_null,
                                 d_nodes_or_null, out_root_or_null, hip_stream, [&](Context &c, uint32_t lgb, uint32_t lgd, uint32_t, uint64_t, hipStream_t s) {
                                     const int rc = ntt_device_locked(c, LW_FIELD_BABYBEAR, LW_LAYOUT_BABYBEAR_U32_R32, LW_DIR_FORWARD, d_out_poly,
                                                                      d_out_evaluation_or_null, lgd, 4, 0, offset_or_null, s, lgb);
                                     return rc ? rc : merkle_commit_device(c, d_out_evaluation_or_null, 8, domain_size, lgd - 1, 1, d_nodes_or_null, s, 4, 2);
                                 });
}

static constexpr ExtR2Names BB4_R2_NAMES{"bb4_r2_xtable_kernel", "bb4_r2_cycle_kernel", "bb4_r2_transition_kernel", "bb4_r2_boundary_kernel", "bb4_r2_split_kernel", "bb4_r2_lengths_kernel", "bb4_r2_rap_transition_kernel"};
static constexpr ExtAuxNames BB4_AUX_NAMES{"bb4_aux_reduce_kernel", "bb4_aux_carry_kernel", "bb4_aux_rescan_kernel"};

int lw_babybear_ext4_constraint_evaluations_device(const lw_stark_air_op_t *ops, uint32_t n_ops, const uint32_t *consts, uint32_t n_consts,
                                                   const uint32_t *const *d_columns, const uint32_t *col_log2_len_or_null, uint32_t n_cols,
                                                   uint32_t log2_trace, uint32_t log2_blowup, const uint32_t *offset_or_null,
                                                   const lw_bb4_boundary_t *boundary, uint32_t n_boundary, const lw_bb4_transition_t *transitions,
                                                   uint32_t n_transitions, uint32_t *d_out, size_t out_stride, void *hip_stream) {
    return ext_r2_constraint_evaluations<Bb4Ext>(BB4_R2_NAMES, ops, n_ops, consts, n_consts, d_columns, col_log2_len_or_null, n_cols, log2_trace, log2_blowup,
                                                 offset_or_null, 0, boundary, n_boundary, transitions, n_transitions, d_out, out_stride, hip_stream);
}

int lw_babybear_ext4_composition_parts_device(const uint32_t *d_evals, size_t evals_stride, uint32_t log2_lde, const uint32_t *offset_or_null,
                                              uint32_t n_parts, uint32_t *d_parts_coeffs, uint32_t *d_parts_lde_or_null, size_t *out_part_lens_or_null,
                                              void *hip_stream) {
    // the four planes through the existing inverse transform (which keeps one stride for both sides: H takes the
    // evaluations' stride), every plane of every part through the existing LDE
    return ext_r2_composition_parts<Bb4Ext>(
        BB4_R2_NAMES, d_evals, evals_stride, log2_lde, offset_or_null, 0, n_parts, d_parts_coeffs, d_parts_lde_or_null, out_part_lens_or_null, hip_stream,
        [&](Context &c, const uint32_t *d_in, uint64_t in_stride, uint32_t *d_H, uint64_t h_stride, uint32_t lg, uint32_t, uint64_t, hipStream_t s) {
            if (in_stride == h_stride)
                return ntt_device_locked(c, LW_FIELD_BABYBEAR, LW_LAYOUT_BABYBEAR_U32_R32, LW_DIR_INVERSE, d_in, d_H, lg, 4, in_stride, offset_or_null, s);
            int rc = LW_OK;
            for (int e = 0; e < 4 && !rc; e++)
                rc = ntt_device_locked(c, LW_FIELD_BABYBEAR, LW_LAYOUT_BABYBEAR_U32_R32, LW_DIR_INVERSE, d_in + e * in_stride, d_H + e * h_stride, lg, 1, 0,
                                       offset_or_null, s);
            return rc;
        },
        [&](Context &c, const uint32_t *d_coeffs, uint32_t lgL, uint32_t *d_lde, uint32_t lg, uint32_t batch, uint32_t, uint64_t, hipStream_t s) {
            return ntt_device_locked(c, LW_FIELD_BABYBEAR, LW_LAYOUT_BABYBEAR_U32_R32, LW_DIR_FORWARD, d_coeffs, d_lde, lg, batch, 0, offset_or_null, s, lgL);
        });
}

int lw_babybear_ext4_aux_fractions_device(const uint32_t *const *d_columns, uint32_t n_cols, size_t n, const uint32_t *num_const, const uint32_t *num_cols,
        const uint32_t *num_coeffs, uint32_t n_num, const uint32_t *den_const, const uint32_t *den_cols, const uint32_t *den_coeffs, uint32_t n_den,
        uint32_t mode, uint32_t *d_out, size_t out_stride, uint32_t *d_total_or_null, uint64_t *out_zero_denominators_or_null, void *hip_stream) {
    return ext_aux_fractions<Bb4Ext>(BB4_AUX_NAMES, d_columns, n_cols, n, ExtAuxList<Bb4Ext>{num_const, num_cols, num_coeffs, n_num},
                                    ExtAuxList<Bb4Ext>{den_const, den_cols, den_coeffs, n_den}, mode, d_out, out_stride, d_total_or_null,
                                    out_zero_denominators_or_null, hip_stream);
}

int lw_babybear_ext4_rap_constraint_evaluations_device(const lw_stark_air_op_t *ops, uint32_t n_ops, const uint32_t *consts, uint32_t n_consts, const uint32_t *xconsts,
        uint32_t n_xconsts, const uint32_t *const *d_columns, const uint32_t *col_log2_len_or_null, uint32_t n_cols, const uint32_t *const *d_aux_columns,
        uint32_t n_aux, size_t aux_stride, uint32_t log2_trace, uint32_t log2_blowup, const uint32_t *offset_or_null,
        const lw_bb4_rap_boundary_t *boundary, uint32_t n_boundary, const lw_bb4_transition_t *transitions, uint32_t n_transitions, uint32_t *d_out, size_t out_stride,
        void *hip_stream) {
    ExtR2Rap<Bb4Ext> rap{d_aux_columns, n_aux, aux_stride, xconsts, n_xconsts, {}, 0};
    return ext_r2_constraint_evaluations<Bb4Ext>(BB4_R2_NAMES, ops, n_ops, consts, n_consts, d_columns, col_log2_len_or_null, n_cols, log2_trace, log2_blowup,
                                                offset_or_null, 0, boundary, n_boundary, transitions, n_transitions, d_out, out_stride, hip_stream, &rap);
}

}  // extern "C"
#endif
