// Internal functions that one translation unit defines and others call: each is declared here once, with its default
// arguments, under the file that defines it.  The exported C ABI is include/lw_hip.h.
#pragma once
#include <functional>
#include "context.h"

namespace lw {

// ---- api.hip
uint32_t field_two_adicity(lw_field_t f);
int check_field_layout(lw_field_t field, lw_layout_t layout);
// in_log2 < log2n (forward only): low-degree extension of dense blocks of 2^in_log2 coefficients, see ntt256.hip / ntt_bb.hip
int ntt_device_locked(Context &c, lw_field_t field, lw_layout_t layout, lw_dir_t dir, const void *d_in, void *d_out,
                      uint32_t log2n, uint32_t batch, size_t stride, const void *coset, hipStream_t stream,
                      uint32_t in_log2 = 0xffffffffu);
size_t srs_len(const lw_srs_t *srs);
lw_curve_t srs_curve(const lw_srs_t *srs);
int msm_srs_locked(Context &c, const lw_srs_t *srs, const uint64_t *d_scalars, size_t n, void *out_point, hipStream_t stream, int mont);

// ---- ntt256.hip
int ntt256_device(Context &c, int field, lw_dir_t dir, const void *d_in, void *d_out, uint32_t log2n, uint32_t batch,
                  uint64_t stride, const uint32_t *coset_words, hipStream_t stream, uint32_t in_log2);
int ntt256_gen_powers(int field, uint32_t order, uint64_t count, uint32_t bitrev, bool inverse, const uint32_t *scale_words, void *d_out,
                      hipStream_t stream);
// helpers for the multi-GPU cross step (ntt_cross.hip)
int ntt256_power_tables(Context &c, int field, int slot, const uint32_t *base_words, bool invert, uint32_t hbits,
                        uint32_t hi_bits, hipStream_t stream, const uint4 **lo, const uint4 **hi);
int ntt256_root_words(int field, uint32_t order, bool inverse, uint32_t *words);
int ntt256_inv_u64_words(int field, uint64_t v, uint32_t *words);
const uint4 *ntt256_twiddle_table(Context &c, int field, lw_dir_t dir, uint32_t log2n, hipStream_t stream, int *rc);

// ---- ntt_bb.hip
int ntt_bb_device(Context &c, lw_layout_t layout, lw_dir_t dir, const void *d_in, void *d_out, uint32_t log2n,
                  uint32_t batch, uint64_t stride, const void *coset_offset, hipStream_t stream, uint32_t in_log2);
int ntt_bb_gen_powers(lw_layout_t layout, uint32_t order, uint64_t count, uint32_t bitrev, bool inverse, const void *scale, void *d_out,
                      hipStream_t stream);
const uint32_t *ntt_bb_twiddle_table(Context &c, lw_dir_t dir, uint32_t log2n, hipStream_t stream, int *rc);
uint32_t ntt_bb_root(uint32_t order, bool inverse);

// ---- ntt_aux.hip
int gen_twiddles_device(Context &c, lw_field_t field, lw_layout_t layout, uint32_t order, int config, void *d_out, hipStream_t stream);
int broadcast_device(size_t elem_bytes, const void *d_in, void *d_out, uint64_t n, uint32_t batch, uint64_t out_stride, hipStream_t stream);
int bitrev_device(size_t elem_bytes, const void *d_in, void *d_out, uint32_t log2n, hipStream_t stream);

// ---- ntt_cross.hip
int ntt_cross_device(Context &c, lw_field_t field, lw_layout_t layout, lw_dir_t dir, const void *d_in, void *d_out,
                     uint32_t log2_total, uint32_t log2_g, uint64_t j2_begin, uint64_t slice_len, uint64_t chunk_stride,
                     uint32_t batch, uint64_t batch_stride, hipStream_t stream);

// ---- merkle.hip
int merkle_commit_device(Context &c, const void *d_cols, uint32_t n_cols, uint64_t col_stride, uint32_t log2n, int bit_reverse,
                         void *d_nodes, hipStream_t stream, uint32_t elem_bytes = 32, uint32_t rows_per_leaf = 1);

// ---- fri.hip
int fri_layer_device(Context &c, lw_field_t field, const void *d_coeffs, uint64_t n, const uint32_t *zeta, const void *offset_ref,
                     uint32_t log2_domain, void *d_poly, uint32_t log2_block, void *d_eval, void *d_eval_br, void *d_nodes,
                     hipStream_t stream);

// ---- goldilocks.hip
int gl_size_check(uint64_t log2n);    // 2^log2n points: LW_ERR_ROOT_OF_UNITY above 32, LW_ERR_ORDER_TOO_LARGE above 30
int gl_root_check(uint64_t &root);    // 0 becomes the reference's 2^32-th root; anything else must be a primitive one below p
uint64_t gl_host_root(uint64_t g, uint32_t order, bool inverse);   // the primitive 2^order-th root of the 2^32-th root g, or its inverse
int goldilocks_lde_locked(Context &c, const uint64_t *d_coeffs, uint32_t log2_coeffs, uint64_t in_stride, uint64_t *d_out, uint32_t log2n,
                          uint64_t out_stride, uint32_t batch, uint64_t offset, uint64_t root, hipStream_t stream);
int goldilocks_ntt_locked(Context &c, bool inverse, const uint64_t *d_in, uint64_t in_stride, uint64_t *d_out, uint64_t out_stride, uint32_t log2n,
                          uint32_t batch, uint64_t offset, uint64_t root, hipStream_t stream);

// ---- circle.hip
// the cached inverse twiddles of a transform of 2^L words (built on demand): the x-layers 0 .. L - 2, layer i at word
// 2^i - 1 (null for L = 1), and the y-layer of that size
int circle_inverse_twiddles(Context &c, uint32_t L, hipStream_t stream, const uint32_t **ix, const uint32_t **iy);
// interpolate_cfft of `batch` columns of 2^L words, and evaluate_cfft(zero_pad(coeffs, 2^Lout)) of blocks of 2^Lin
// coefficients (the padding never written): the two halves of the LDE, each side under its own stride
int circle_interpolate_locked(Context &c, const uint32_t *d_in, uint64_t in_stride, uint32_t *d_out, uint64_t out_stride, uint32_t L, uint32_t batch,
                              hipStream_t stream);
int circle_extend_locked(Context &c, const uint32_t *d_coeffs, uint32_t Lin, uint64_t in_stride, uint32_t *d_out, uint32_t Lout, uint64_t out_stride,
                         uint32_t batch, hipStream_t stream);

// ---- rpo.hip
int rpo_level_check(int level);   // LW_RPO_128 or LW_RPO_160, else LW_ERR_BAD_ARG
// the tree of lw_rpo_commit_columns_device inside another call's Entry; group: RpoHash::row's element order (0: as it is)
int rpo_commit_locked(Context &c, int level, const uint64_t *d_columns, uint32_t n_cols, uint64_t col_stride, uint32_t log2n, int bit_reverse,
                      int group, uint64_t *d_nodes, hipStream_t stream);

// ---- groth16.hip
int groth16_h_device(Context &c, const void *d_l, const void *d_r, const void *d_o, uint32_t log2_gates, void *d_out, void *d_tmp,
                     hipStream_t stream);
int stripped_length_device(const void *d_elems, uint64_t n, uint64_t *d_len, hipStream_t stream);

// ---- r1cs.hip
lw_field_t r1cs_field(const lw_r1cs_t *h);
uint32_t r1cs_rows(const lw_r1cs_t *h);
uint32_t r1cs_cols(const lw_r1cs_t *h);
// A z, B z, C z of a device-resident z into the requested d_out (n_out >= rows elements each, zero past the rows)
int r1cs_matvec_locked(Context &c, const lw_r1cs_t *h, const void *d_z, size_t n_out, void *const (&d_out)[3], hipStream_t s);

// ---- stark_query.hip
void keccak_f1600_host(uint64_t (&a)[25]);   // Keccak-f[1600] on the host: the grinding seed, the SHAKE128 of monolith.hip

// ---- poly.hip
// the lane's pinned staging c.deep_pin, at least `bytes` long and no longer read by an earlier call's upload
int deep_pin(Context &c, size_t bytes);

// ---- comm.hip
void comm_release(Context &c);

// ---- msm.hip
// What is per call in an MSM: handed from the entry points through msm_device to the curve's runner (msm_core.cuh).
struct MsmCall {
    int affine = 0;                      // d_points are affine rows made by normalize (a pre-normalised SRS)
    hipEvent_t points_ready = nullptr;   // recorded on a side stream once d_points is complete; joined before the first accumulation
    uint32_t scalar_limbs = 4;           // the scalars are n x scalar_limbs u64 (1 .. 8)
    // folded SRS (lw_hip_srs_*): the point set holds window-shifted copies, d_points[w * fold_stride + i] = 2^(fold_c w) * P_i,
    // and all windows share one bucket set (msm_core.cuh build_fold); 0: a single copy
    uint32_t fold_c = 0;
    uint64_t fold_stride = 0;
    // host-buffer calls: run right after the sort of the scalars is enqueued (upload of the points and their normalisation
    // on the side streams, so that the sort runs under the upload)
    std::function<int()> after_sort;
};
// call.points_ready and call.after_sort are msm_device's own; h_points: the points are still in host memory
int msm_device(Context &c, lw_curve_t curve, const uint64_t *d_scalars, const void *d_points, size_t n, void *out_host,
               hipStream_t stream, int scalars_montgomery, MsmCall call, const void *h_points = nullptr);
int msm_sum_points_host(lw_curve_t curve, const void *pts, size_t n, void *out);
uint32_t msm_window_bits_for(size_t n);   // the single-GPU window rule
int msm_shard_accumulate(Context &c, lw_curve_t curve, const uint64_t *d_scalars, const void *d_points, size_t n, uint32_t cbits, hipStream_t s,
                         char **buckets);
int msm_shard_reduce(Context &c, lw_curve_t curve, const char *recv, uint32_t G, uint32_t cbits, char *d_sa, hipStream_t s);
int msm_shard_combine(lw_curve_t curve, const char *sa_all, uint32_t G, uint32_t cbits, void *out);
int ensure_aux_stream(Context &c);   // the context's side stream

uint32_t msm_ch(uint64_t items);       // max points per accumulate work-item (a bucket is cut into equal pieces <= CH)
uint64_t msm_quad_max_lanes();          // LW_HIP_MSM_QUAD: levels of the bucket reduce with at most this many lanes (8 per group) spread each addition over a quad; 0 = never, ~0 = not set
uint64_t msm_accumulate_quad_max_lanes();   // LW_HIP_MSM_ACCQ: accumulate launches of projective rows with at most this many lanes (4 per piece) use the quad kernel

struct Carver {   // bump allocator over the context workspace; with base == nullptr (dry run) only the sizes are added up
    char *base;
    size_t cap, used = 0;
    void *take(size_t bytes) {
        used = (used + 255) & ~(size_t)255;
        void *p = base ? base + used : nullptr;
        used += bytes;
        return p;
    }
    // true once a real (non-dry) carve-out has run past the workspace the dry run sized: checked before every launch
    // that would touch the new pointers
    bool overrun() const { return base && used > cap; }
};
#define LW_MSM_WS_CHECK(cv)                                                                                          \
    do {                                                                                                             \
        if ((cv).overrun()) {                                                                                        \
            set_error("internal: MSM workspace of %zu bytes is too small (%zu needed so far)", (cv).cap, (cv).used); \
            return LW_ERR_ALLOC;                                                                                     \
        }                                                                                                            \
    } while (0)

// host launchers for the curve-independent kernels
uint32_t msm_max_window_bits();
uint64_t msm_sort_padded_points(uint64_t n);
int msm_launch_digits(Context &c, const uint32_t *scalars, uint64_t n, uint32_t cb, uint32_t W, uint32_t *dig, hipStream_t s,
                      uint32_t scalar_limbs);   // scalars: n x scalar_limbs u64, 1 .. 8
// The arrays of one sort over all W windows of an MSM: NW bucket sets (one per window, or one for all: folded SRS) of
// 2^(c-1) keys each, K keys and CB coarse bins in all.
struct MsmSortBufs {
    uint32_t NW = 0, K = 0, CB = 0;
    uint32_t *coarse_cnt = nullptr, *coarse_cursor = nullptr, *maxlen_d = nullptr, *key_cnt = nullptr, *key_cursor = nullptr;
    uint32_t *coarse_off = nullptr, *sub_off = nullptr, *off = nullptr, *scan_tmp = nullptr, *sorted = nullptr, *order_tmp = nullptr;
    uint64_t *items = nullptr;
};
// carve-outs of the sort of n scalars into W windows of `cbits` bits
int msm_sort_carve(MsmSortBufs &b, uint64_t n, uint32_t cbits, uint32_t W, uint64_t fold_stride, Carver &cv);
// sort of the digit matrix (W rows of msm_sort_padded_points(n) u32) on stream `s`: b.sorted holds (sign, point index)
// by key and b.off the K + 1 key offsets; the longest bucket lands in b.maxlen_d and in *maxlen_h once `s` gets there
int msm_launch_sort(Context &c, const MsmSortBufs &b, const uint32_t *dig, uint64_t n, uint32_t cbits, uint32_t W, uint64_t fold_stride,
                    volatile uint32_t *maxlen_h, hipStream_t s);
void msm_launch_scan(const uint32_t *in, uint32_t *out, uint32_t K, int mode, uint32_t *maxlen, uint32_t *scratch, hipStream_t s);
void msm_launch_piece_order(Context &c, const uint32_t *seg_off, const uint32_t *out_off, uint32_t K, uint32_t P, uint32_t *order_tmp,
                            uint32_t *perm_t, uint32_t *perm_key, hipStream_t s);

// ---- msm_<curve>.hip (msm_curve_ops<C>() in msm_core.cuh): the per-curve MSM operations
struct MsmCurveOps {
    int (*run)(Context &c, hipStream_t s, const uint64_t *d_scalars, const void *d_points, size_t n, void *out, const MsmCall &call);
    int (*normalize)(Context &c, hipStream_t s, const void *d_in, size_t n, void *d_out);
    size_t (*affine_bytes)(size_t n);   // bytes of the device-resident affine form of n points (rows may be padded, ec.cuh aff_stride)
    int (*fold_build)(Context &c, hipStream_t s, void *d_rows, size_t n, uint32_t cbits);
    int (*shard_accumulate)(Context &c, hipStream_t s, const uint64_t *d_scalars, const void *d_aff, size_t n, uint32_t cbits, char **buckets);
    int (*shard_reduce)(Context &c, hipStream_t s, const char *recv, uint32_t G, uint32_t cbits, char *d_sa);
    void (*shard_combine)(const char *sa_all, uint32_t G, uint32_t cbits, void *out);
    int (*add_outer)(Context &c, hipStream_t s, const void *d_rows, uint32_t m, const void *d_cols, uint32_t k, void *d_out);
    void (*sum_points_host)(const void *pts, size_t n, void *out);   // projective points, normalised like every MSM result
};
// (not const: HIP would emit a const table for the device too, where the host functions it points to do not exist)
extern MsmCurveOps msm_ops_bls12381_g1, msm_ops_bn254_g1, msm_ops_bn254_g2, msm_ops_bls12381_g2;
const MsmCurveOps *msm_ops(lw_curve_t curve);   // msm.hip; nullptr (error set) for a bad curve

}  // namespace lw
