// The Goldilocks quadratic extension Fp2 = F_p[t] / (t^2 - 7) on the device (arithmetic: goldilocks_ext.cuh) as a policy of
// ext_steps.cuh, which holds the steps a STARK prover over Goldilocks runs in it after round 1 (pointwise, evaluate,
// deep_quotients, fri_layer), and the entry points of those steps.
// A vector of n Fp2 elements is two PLANES of n words, c0 then c1 `stride` words later: the batch / batch_stride shape of
// lw_goldilocks_ntt_device and the n_cols / col_stride shape of lw_rpo_commit_columns_device, so a transform of an Fp2
// vector over a base-field domain is the existing transform with batch = 2 (the twiddles are in F) and nothing here
// re-implements a transform or a tree: the layer calls goldilocks.hip and rpo.hip (internal.h).  A word read from a caller
// is any u64 and is canonicalised on the way in.
//
// evaluate: a work-item runs Horner over its EXT_E coefficients (acc = acc x + c: one gl2_mul and one gl_add).
// deep_quotients: the norm of x_i - z is (x_i - z0)^2 - 7 z1^2 and 1 / (x - z) = (x - z0 + z1 t) / norm.  The norm is never
// zero: z1 != 0 is checked and 7 is a non-residue.  The way back through Montgomery's trick is a loop over (row, point).
#include "goldilocks_ext.cuh"
#include "ext_steps.cuh"
#include "ext_round2.cuh"
#include "ext_aux.cuh"

namespace lw {

struct Gl2Ext {
    using word = uint64_t;
    using elem = Gl2;
    static constexpr int D = 2;
    static constexpr const char *NAME = "Fp2";
    static constexpr ExtNames NAMES{"gl2_pointwise_kernel", "gl2_eval_tile_kernel", "gl2_eval_fold_kernel", "gl2_deep_kernel", "gl2_fri_fold_kernel"};
    static constexpr word F_ONE = 1;
    EXT_HD word fcanon(word x) { return gl_from_word(x); }
    EXT_HD word fadd(word a, word b) { return gl_add(a, b); }
    EXT_HD word fsub(word a, word b) { return gl_sub(a, b); }
    EXT_HD word fmul(word a, word b) { return gl_mul(a, b); }
    EXT_HD word fpow(word a, uint64_t e) { return gl_pow(a, e); }
    EXT_HD word finv(word a) { return gl_inv(a); }
    EXT_HD elem load(ExtPlanes<Gl2Ext> v, uint64_t i) { return Gl2{v.p[0][i], v.p[1][i]}; }
    EXT_HD void store(ExtPlanes<Gl2Ext> v, uint64_t i, elem a) {
        v.p[0][i] = a.c0;
        v.p[1][i] = a.c1;
    }
    EXT_HD elem canon(elem a) { return gl2_from_words(a.c0, a.c1); }
    EXT_HD elem zero() { return Gl2{0, 0}; }
    EXT_HD elem one() { return Gl2{1, 0}; }
    EXT_HD bool is_zero(elem a) { return (a.c0 | a.c1) == 0; }
    EXT_HD elem add(elem a, elem b) { return gl2_add(a, b); }
    EXT_HD elem sub(elem a, elem b) { return gl2_sub(a, b); }
    EXT_HD elem mul(elem a, elem b) { return gl2_mul(a, b); }
    EXT_HD elem sqr(elem a) { return gl2_sqr(a); }
    EXT_HD elem inv(elem a) { return gl2_inv(a); }
    EXT_HD elem mul_base(elem a, word b) { return gl2_mul_base(a, b); }

    using eval_point = Gl2;   // x
    EXT_HD eval_point eval_point_of(const elem *xp) { return xp[1]; }

    struct deep_point {
        Gl2 z;
        uint64_t zn;   // 7 z1^2
    };
    EXT_HD deep_point deep_point_of(elem z) { return deep_point{z, gl_mul(gl_mul(z.c1, z.c1), GL2_NON_RESIDUE)}; }
    EXT_HD word norm(word x, deep_point p) {
        const uint64_t d0 = gl_sub(x, p.z.c0);
        return gl_sub(gl_mul(d0, d0), p.zn);
    }
    // 1 / (x - z) = conj / norm, (x - z) conj = norm
    EXT_HD elem quotient(elem num, word x, deep_point p, word ninv) { return gl2_mul_base(gl2_mul(num, Gl2{gl_sub(x, p.z.c0), p.z.c1}), ninv); }
    static constexpr int R2_ROWS_FEW = 8;   // boundary rows per work-item with one or two steps (ext_round2.cuh): E::finv is 127 products: shared by eight rows where the registers allow
    static constexpr bool DEEP_BACK_BY_RECURSION = false;

    // host: any u64 is a scalar; the caller may choose the two-adic root
    static int words_check(const word *, size_t, const char *) { return LW_OK; }
    static int size_check(uint32_t log2n) { return gl_size_check(log2n); }
    static int root_check(uint64_t &root) { return gl_root_check(root); }
    static int offset(const word *offset_or_null, word &h) {
        h = offset_or_null ? gl_from_word(*offset_or_null) : 1;
        if (h == 0) { set_error("coset offset is zero"); return LW_ERR_INV_ZERO; }
        return LW_OK;
    }
    static word domain_root(uint64_t root, uint32_t log2n) { return gl_host_root(root, log2n, false); }
};

}  // namespace lw

#ifndef LW_EXT_POLICY_ONLY   // tests/ext_steps_host_main.cpp takes the policy and leaves the kernel and entry points of this file
namespace lw {

// the tile sums of evaluate (ext_steps.cuh): Horner over the work-item's coefficients
__global__ __launch_bounds__(EXT_THREADS) void gl2_eval_tile_kernel(const ExtEvalArgs<Gl2Ext> a) {
    __shared__ Gl2 lds[EXT_THREADS];
    const uint32_t k = a.k0 + blockIdx.y;
    const uint64_t t = blockIdx.x;
    const uint64_t *col = a.cols + (uint64_t)k * a.col_stride;
    const uint64_t base = t * EXT_TILE + (uint64_t)threadIdx.x * EXT_E;
    uint64_t c[EXT_E];
#pragma unroll
    for (int e = 0; e < EXT_E; e++) c[e] = base + e < a.n ? gl_from_word(col[base + e]) : 0;
#pragma unroll 1
    for (uint32_t j = 0; j < a.m; j++) {
        const Gl2 x = a.x[j];
        Gl2 h{c[EXT_E - 1], 0};
#pragma unroll
        for (int e = EXT_E - 2; e >= 0; e--) {
            h = gl2_mul(h, x);
            h.c0 = gl_add(h.c0, c[e]);
        }
        h = ext_block_fold<Gl2Ext>(h, lds, a.pe[j]);
        if (threadIdx.x == 0) a.sums[((uint64_t)k * EXT_PTS + j) * a.ntiles + t] = h;
    }
}

}  // namespace lw

using namespace lw;

extern "C" {

int lw_goldilocks_ext2_pointwise_device(lw_gl2_op_t op, const uint64_t *d_a, size_t a_stride, const uint64_t *d_b, size_t b_stride, uint64_t *d_out,
                                        size_t out_stride, size_t n, void *hip_stream) {
    return ext_pointwise<Gl2Ext>((int)op, d_a, a_stride, d_b, b_stride, d_out, out_stride, n, hip_stream);
}

int lw_goldilocks_ext2_evaluate_device(const uint64_t *d_coeffs, uint32_t n_cols, size_t col_stride, size_t n_coeffs, const uint64_t *points, uint32_t m,
                                       uint64_t *out_values, void *hip_stream) {
    return ext_evaluate<Gl2Ext>(d_coeffs, n_cols, col_stride, n_coeffs, points, m, out_values, hip_stream, gl2_eval_tile_kernel);
}

int lw_goldilocks_ext2_deep_quotients_device(const uint64_t *d_lde, uint32_t n_cols, size_t col_stride, uint32_t log2n, const uint64_t *offset_or_null,
                                             uint64_t two_adic_root, const uint64_t *points, uint32_t m, const uint64_t *weights,
                                             const uint64_t *evals, uint64_t *d_out, size_t out_stride, void *hip_stream) {
    return ext_deep_quotients<Gl2Ext>(d_lde, n_cols, col_stride, log2n, offset_or_null, two_adic_root, points, m, weights, evals, d_out, out_stride,
                                      hip_stream);
}

int lw_goldilocks_ext2_fri_layer_device(const uint64_t *d_coeffs, size_t coeff_stride, size_t n_coeffs, const uint64_t *zeta,
                                        const uint64_t *offset_or_null, size_t domain_size, uint64_t two_adic_root, lw_rpo_level_t level,
                                        uint64_t *d_out_poly, uint64_t *d_out_evaluation_or_null, uint64_t *d_nodes_or_null,
                                        uint64_t *out_root_or_null, void *hip_stream) {
    const int rc = rpo_level_check((int)level);   // before the n_coeffs == 0 return
    if (rc) return rc;
    // both planes through the existing transform, then the four "columns" of half a plane each, element after element (group 2)
    return ext_fri_layer<Gl2Ext>(d_coeffs, coeff_stride, n_coeffs, zeta, offset_or_null, domain_size, two_adic_root, level == LW_RPO_128 ? 32 : 40,
                                 d_out_poly, d_out_evaluation_or_null, d_nodes_or_null, out_root_or_null, hip_stream,
                                 [&](Context &c, uint32_t lgb, uint32_t lgd, uint64_t h, uint64_t root, hipStream_t s) {
                                     const size_t padded = (size_t)1 << lgb;
                                     const int rc = goldilocks_lde_locked(c, d_out_poly, lgb, padded, d_out_evaluation_or_null, lgd, domain_size, 2, h, root, s);
                                     return rc ? rc : rpo_commit_locked(c, (int)level, d_out_evaluation_or_null, 4, domain_size / 2, lgd - 1, 1, 2, d_nodes_or_null, s);
                                 });
}

static constexpr ExtR2Names GL2_R2_NAMES{"gl2_r2_xtable_kernel", "gl2_r2_cycle_kernel", "gl2_r2_transition_kernel", "gl2_r2_boundary_kernel", "gl2_r2_split_kernel", "gl2_r2_lengths_kernel", "gl2_r2_rap_transition_kernel"};
static constexpr ExtAuxNames GL2_AUX_NAMES{"gl2_aux_reduce_kernel", "gl2_aux_carry_kernel", "gl2_aux_rescan_kernel"};

int lw_goldilocks_ext2_constraint_evaluations_device(const lw_stark_air_op_t *ops, uint32_t n_ops, const uint64_t *consts, uint32_t n_consts,
                                                     const uint64_t *const *d_columns, const uint32_t *col_log2_len_or_null, uint32_t n_cols,
                                                     uint32_t log2_trace, uint32_t log2_blowup, const uint64_t *offset_or_null, uint64_t two_adic_root,
                                                     const lw_gl2_boundary_t *boundary, uint32_t n_boundary, const lw_gl2_transition_t *transitions,
                                                     uint32_t n_transitions, uint64_t *d_out, size_t out_stride, void *hip_stream) {
    return ext_r2_constraint_evaluations<Gl2Ext>(GL2_R2_NAMES, ops, n_ops, consts, n_consts, d_columns, col_log2_len_or_null, n_cols, log2_trace, log2_blowup,
                                                 offset_or_null, two_adic_root, boundary, n_boundary, transitions, n_transitions, d_out, out_stride, hip_stream);
}

int lw_goldilocks_ext2_composition_parts_device(const uint64_t *d_evals, size_t evals_stride, uint32_t log2_lde, const uint64_t *offset_or_null,
                                                uint64_t two_adic_root, uint32_t n_parts, uint64_t *d_parts_coeffs, uint64_t *d_parts_lde_or_null,
                                                size_t *out_part_lens_or_null, void *hip_stream) {
    // both planes through the existing inverse transform, every plane of every part through the existing LDE
    return ext_r2_composition_parts<Gl2Ext>(
        GL2_R2_NAMES, d_evals, evals_stride, log2_lde, offset_or_null, two_adic_root, n_parts, d_parts_coeffs, d_parts_lde_or_null, out_part_lens_or_null, hip_stream,
        [](Context &c, const uint64_t *d_in, uint64_t in_stride, uint64_t *d_H, uint64_t h_stride, uint32_t lg, uint64_t h, uint64_t root, hipStream_t s) {
            return goldilocks_ntt_locked(c, true, d_in, in_stride, d_H, h_stride, lg, 2, h, root, s);
        },
        [](Context &c, const uint64_t *d_coeffs, uint32_t lgL, uint64_t *d_lde, uint32_t lg, uint32_t batch, uint64_t h, uint64_t root, hipStream_t s) {
            return goldilocks_lde_locked(c, d_coeffs, lgL, (uint64_t)1 << lgL, d_lde, lg, (uint64_t)1 << lg, batch, h, root, s);
        });
}

int lw_goldilocks_ext2_aux_fractions_device(const uint64_t *const *d_columns, uint32_t n_cols, size_t n, const uint64_t *num_const, const uint32_t *num_cols,
        const uint64_t *num_coeffs, uint32_t n_num, const uint64_t *den_const, const uint32_t *den_cols, const uint64_t *den_coeffs, uint32_t n_den,
        uint32_t mode, uint64_t *d_out, size_t out_stride, uint64_t *d_total_or_null, uint64_t *out_zero_denominators_or_null, void *hip_stream) {
    return ext_aux_fractions<Gl2Ext>(GL2_AUX_NAMES, d_columns, n_cols, n, ExtAuxList<Gl2Ext>{num_const, num_cols, num_coeffs, n_num},
                                    ExtAuxList<Gl2Ext>{den_const, den_cols, den_coeffs, n_den}, mode, d_out, out_stride, d_total_or_null,
                                    out_zero_denominators_or_null, hip_stream);
}

int lw_goldilocks_ext2_rap_constraint_evaluations_device(const lw_stark_air_op_t *ops, uint32_t n_ops, const uint64_t *consts, uint32_t n_consts, const uint64_t *xconsts,
        uint32_t n_xconsts, const uint64_t *const *d_columns, const uint32_t *col_log2_len_or_null, uint32_t n_cols, const uint64_t *const *d_aux_columns,
        uint32_t n_aux, size_t aux_stride, uint32_t log2_trace, uint32_t log2_blowup, const uint64_t *offset_or_null, uint64_t two_adic_root,
        const lw_gl2_rap_boundary_t *boundary, uint32_t n_boundary, const lw_gl2_transition_t *transitions, uint32_t n_transitions, uint64_t *d_out, size_t out_stride,
        void *hip_stream) {
    ExtR2Rap<Gl2Ext> rap{d_aux_columns, n_aux, aux_stride, xconsts, n_xconsts, {}, 0};
    return ext_r2_constraint_evaluations<Gl2Ext>(GL2_R2_NAMES, ops, n_ops, consts, n_consts, d_columns, col_log2_len_or_null, n_cols, log2_trace, log2_blowup,
                                                offset_or_null, two_adic_root, boundary, n_boundary, transitions, n_transitions, d_out, out_stride, hip_stream, &rap);
}

}  // extern "C"
#endif
