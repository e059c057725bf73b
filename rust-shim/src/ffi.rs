//! `extern "C"` declarations of include/lw_hip.h, one to one.  UNVERIFIED: written without a Rust toolchain.
#![allow(non_camel_case_types)]
use core::ffi::{c_char, c_int, c_void};

/// lw_field_t
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Field {
    Stark252 = 0,
    Bls12381Fr = 1,
    BabyBear = 2,
}

/// lw_layout_t
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Layout {
    /// MontgomeryBackendPrimeField<_, 4>: 4 x u64, most significant limb first, R = 2^256
    U64LimbsMsFirst = 0,
    /// U32MontgomeryBackendPrimeField: one u32, R = 2^32
    BabyBearU32R32 = 1,
    /// MontgomeryBackendPrimeField<_, 1>: one u64, R = 2^64
    BabyBearU64R64 = 2,
    /// Degree4BabyBearExtensionField values: 4 x u64 per element, domain in the base field
    Ext4Interleaved = 3,
}

/// lw_dir_t
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Dir {
    Forward = 0,
    /// scaled by N^-1
    Inverse = 1,
}

/// lw_curve_t
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Curve {
    Bls12381G1 = 0,
    Bn254G1 = 1,
    Bn254G2 = 2,
    Bls12381G2 = 3,
}

// lw_status_t
pub const LW_OK: c_int = 0;
pub const LW_ERR_INPUT_NOT_POW2: c_int = -1;
pub const LW_ERR_ORDER_TOO_LARGE: c_int = -2;
pub const LW_ERR_ROOT_OF_UNITY: c_int = -3;
pub const LW_ERR_LENGTH_MISMATCH: c_int = -4;
pub const LW_ERR_NO_DEVICE: c_int = -5;
pub const LW_ERR_ALLOC: c_int = -6;
pub const LW_ERR_LAUNCH: c_int = -7;
pub const LW_ERR_COMM: c_int = -8;
pub const LW_ERR_BAD_ARG: c_int = -9;
pub const LW_ERR_INV_ZERO: c_int = -10;

pub const LW_HIP_COMM_ID_BYTES: usize = 128;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct lw_timings_t {
    pub last_ntt_ms: f64,
    pub last_msm_ms: f64,
    pub ntt_calls: u64,
    pub msm_calls: u64,
    pub twiddle_bytes: u64,
    pub scratch_bytes: u64,
}

/// lw_stark_tree_t: one device-resident Merkle tree and the columns it commits (lw_stark_open_trees_device)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct lw_stark_tree_t {
    pub field: Field,
    /// NULL: paths only
    pub d_columns: *const c_void,
    pub n_cols: u32,
    /// 0 = dense
    pub col_stride_elems: u64,
    pub log2_rows: u32,
    /// 1 or 2
    pub rows_per_leaf: u32,
    pub bit_reverse: c_int,
    pub d_nodes: *const c_void,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct lw_kernel_time_t {
    pub name: [c_char; 48],
    pub launches: u64,
    pub total_ms: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct lw_profile_t {
    pub n: c_int,
    pub k: [lw_kernel_time_t; 32],
}

/// opaque `lw_srs_t`
#[repr(C)]
pub struct lw_srs_t {
    _private: [u8; 0],
}
/// opaque `lw_plonk_circuit_t`
#[repr(C)]
pub struct lw_plonk_circuit_t {
    _private: [u8; 0],
}

/// opaque `lw_r1cs_t`
#[repr(C)]
pub struct lw_r1cs_t {
    _private: [u8; 0],
}

extern "C" {
    // ---- context
    pub fn lw_hip_init(device_ids: *const c_int, n_devices: c_int) -> c_int;
    pub fn lw_hip_shutdown();
    pub fn lw_hip_device_count() -> c_int;
    pub fn lw_hip_last_error() -> *const c_char;
    pub fn lw_hip_get_timings(out: *mut lw_timings_t) -> c_int;
    pub fn lw_hip_profile_begin() -> c_int;
    pub fn lw_hip_profile_end(out: *mut lw_profile_t) -> c_int;
    pub fn lw_hip_field_elem_bytes(field: Field, layout: Layout) -> usize;
    pub fn lw_hip_curve_point_bytes(curve: Curve) -> usize;

    // ---- NTT backend seam
    pub fn lw_hip_result_acquire(bytes: usize, out_ptr: *mut *mut c_void) -> c_int;
    pub fn lw_hip_result_release(ptr: *mut c_void) -> c_int;
    pub fn lw_hip_ntt(field: Field, layout: Layout, dir: Dir, input: *const c_void, output: *mut c_void, log2n: u32,
                      batch: u32, batch_stride_elems: usize, coset_offset_or_null: *const c_void) -> c_int;
    pub fn lw_hip_ntt_device(field: Field, layout: Layout, dir: Dir, d_in: *const c_void, d_out: *mut c_void, log2n: u32,
                             batch: u32, batch_stride_elems: usize, coset_offset_or_null: *const c_void,
                             hip_stream: *mut c_void) -> c_int;
    pub fn lw_hip_ntt_lde_device(field: Field, layout: Layout, d_coeffs: *const c_void, log2_coeffs: u32, d_out: *mut c_void,
                                 log2n: u32, batch: u32, coset_offset_or_null: *const c_void, hip_stream: *mut c_void) -> c_int;
    pub fn lw_hip_gen_twiddles(field: Field, layout: Layout, order: u64, config: c_int, out: *mut c_void) -> c_int;
    pub fn lw_hip_gen_powers(field: Field, layout: Layout, order: u64, count: usize, config: c_int, offset_or_null: *const c_void,
                             out: *mut c_void, out_len: *mut usize) -> c_int;
    pub fn lw_hip_bitrev_permutation(field: Field, layout: Layout, input: *const c_void, output: *mut c_void, n: usize) -> c_int;
    pub fn lw_hip_ntt_cross_device(field: Field, layout: Layout, dir: Dir, d_in: *const c_void, d_out: *mut c_void,
                                   log2n_total: u32, log2_shards: u32, j2_begin: u64, slice_len: u64, chunk_stride_elems: u64,
                                   batch: u32, batch_stride_elems: u64, hip_stream: *mut c_void) -> c_int;

    // ---- multi-GPU (library-owned RCCL communicator)
    pub fn lw_hip_comm_unique_id(out_id: *mut u8) -> c_int;
    pub fn lw_hip_comm_init(unique_id: *const u8, rank: c_int, nranks: c_int) -> c_int;
    pub fn lw_hip_comm_shutdown() -> c_int;
    pub fn lw_hip_comm_info(rank: *mut c_int, nranks: *mut c_int) -> c_int;
    pub fn lw_hip_ntt_sharded_device(field: Field, layout: Layout, dir: Dir, d_in_local: *const c_void, d_out_local: *mut c_void,
                                     log2n_total: u32, batch: u32, natural_output: c_int, hip_stream: *mut c_void) -> c_int;
    pub fn lw_hip_ntt_sharded_selftest_device(field: Field, layout: Layout, dir: Dir, d_in_full: *const c_void,
                                              d_out_full: *mut c_void, log2n_total: u32, log2_shards: u32, batch: u32,
                                              natural_output: c_int, hip_stream: *mut c_void) -> c_int;
    pub fn lw_hip_ntt_sharded_selftest_steps_device(field: Field, layout: Layout, dir: Dir, d_in_full: *const c_void,
                                                    d_out_full: *mut c_void, log2n_total: u32, log2_shards: u32, batch: u32,
                                                    natural_output: c_int, stop_after: c_int, hip_stream: *mut c_void) -> c_int;
    pub fn lw_hip_msm_sharded_device(curve: Curve, d_scalars: *const u64, d_points: *const c_void, n_local: usize,
                                     out_point_host: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn lw_hip_msm_sharded_selftest_device(curve: Curve, d_scalars: *const u64, d_points: *const c_void, n_total: usize, log2_shards: u32,
                                              out_point_host: *mut c_void, hip_stream: *mut c_void) -> c_int;

    // ---- Polynomial FFT API (host buffers, reference semantics)
    pub fn lw_polynomial_evaluate_fft(field: Field, layout: Layout, coeffs: *const c_void, n_coeffs: usize, blowup_factor: usize,
                                      domain_size: usize, offset_or_null: *const c_void, out: *mut c_void,
                                      out_capacity_elems: usize, out_len: *mut usize) -> c_int;
    pub fn lw_polynomial_interpolate_fft(field: Field, layout: Layout, evals: *const c_void, n: usize,
                                         offset_or_null: *const c_void, out_coeffs: *mut c_void, coeff_len: *mut usize) -> c_int;

    // ---- STARK commitment / FRI layer / Groth16 quotient
    pub fn lw_stark_commit_columns(field: Field, columns: *const c_void, n_cols: u32, log2n: u32, bit_reverse: c_int,
                                   out_root: *mut u8, out_nodes_or_null: *mut u8) -> c_int;
    pub fn lw_stark_commit_columns_device(field: Field, d_columns: *const c_void, n_cols: u32, col_stride_elems: u64, log2n: u32,
                                          bit_reverse: c_int, d_nodes: *mut c_void, out_root_or_null: *mut u8,
                                          hip_stream: *mut c_void) -> c_int;
    pub fn lw_stark_commit_columns_layout_device(field: Field, layout: Layout, d_columns: *const c_void, n_cols: u32, col_stride_elems: u64,
                                                 log2n: u32, bit_reverse: c_int, d_nodes: *mut c_void, out_root_or_null: *mut u8,
                                                 hip_stream: *mut c_void) -> c_int;
    pub fn lw_stark_fri_layer(field: Field, coeffs: *const c_void, n_coeffs: usize, zeta: *const c_void, coset_offset: *const c_void,
                              domain_size: usize, out_poly: *mut c_void, out_poly_len: *mut usize, out_evaluation: *mut c_void,
                              out_root: *mut u8, out_nodes_or_null: *mut u8) -> c_int;
    pub fn lw_stark_fri_layer_device(field: Field, d_coeffs: *const c_void, n_coeffs: usize, zeta: *const c_void,
                                     coset_offset: *const c_void, domain_size: usize, d_out_poly: *mut c_void,
                                     d_out_evaluation_or_null: *mut c_void, d_nodes_or_null: *mut c_void, out_root_or_null: *mut u8,
                                     hip_stream: *mut c_void) -> c_int;
    pub fn lw_groth16_h_coefficients_device(d_l: *const c_void, d_r: *const c_void, d_o: *const c_void, n_coeffs: usize,
                                            num_gates: usize, d_out_h: *mut c_void, coeff_len_or_null: *mut usize,
                                            hip_stream: *mut c_void) -> c_int;
    pub fn lw_groth16_h_coefficients(l_coeffs: *const c_void, r_coeffs: *const c_void, o_coeffs: *const c_void, n_coeffs: usize,
                                     num_gates: usize, out_h: *mut c_void, coeff_len: *mut usize) -> c_int;

    // ---- MSM
    pub fn lw_hip_msm(curve: Curve, scalars: *const u64, n_scalars: usize, points: *const c_void, n_points: usize,
                      out_point: *mut c_void) -> c_int;
    pub fn lw_hip_msm_device(curve: Curve, d_scalars: *const u64, d_points: *const c_void, n: usize, out_point_host: *mut c_void,
                             hip_stream: *mut c_void) -> c_int;
    pub fn lw_hip_msm_fr(curve: Curve, fr_elements: *const u64, n_scalars: usize, points: *const c_void, n_points: usize,
                         out_point: *mut c_void) -> c_int;
    pub fn lw_hip_msm_fr_device(curve: Curve, d_fr_elements: *const u64, d_points: *const c_void, n: usize,
                                out_point_host: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn lw_hip_msm_limbs(curve: Curve, scalars: *const u64, scalar_limbs: u32, n_scalars: usize, points: *const c_void,
                            n_points: usize, out_point: *mut c_void) -> c_int;
    pub fn lw_hip_msm_limbs_device(curve: Curve, d_scalars: *const u64, scalar_limbs: u32, d_points: *const c_void, n: usize,
                                   out_point_host: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn lw_hip_ec_add_outer_device(curve: Curve, d_rows: *const c_void, m: usize, d_cols: *const c_void, k: usize,
                                      d_out: *mut c_void, hip_stream: *mut c_void) -> c_int;
    /// The test seam of the group law: one formula of csrc/ec.cuh per row, raw (X, Y, Z) out.  op: LW_EC_OP_*.
    pub fn lw_hip_ec_pointwise_device(curve: Curve, model: c_int, op: c_int, d_a: *const c_void, d_b: *const c_void, n: usize,
                                      d_out: *mut c_void, hip_stream: *mut c_void) -> c_int;
    /// The test seam of the field arithmetic: one primitive of csrc/field.cuh per row, the returned limbs out.
    /// field: LW_PW_FIELD_*, op: LW_FIELD_OP_*.
    pub fn lw_hip_field_pointwise_device(field: c_int, op: c_int, d_a: *const c_void, d_b: *const c_void, n: usize, d_out: *mut c_void,
                                         hip_stream: *mut c_void) -> c_int;
    pub fn lw_hip_srs_create(curve: Curve, points: *const c_void, n_points: usize, out_srs: *mut *mut lw_srs_t) -> c_int;
    pub fn lw_hip_srs_create_device(curve: Curve, d_points: *const c_void, n_points: usize, hip_stream: *mut c_void,
                                    out_srs: *mut *mut lw_srs_t) -> c_int;
    pub fn lw_hip_srs_destroy(srs: *mut lw_srs_t) -> c_int;
    pub fn lw_hip_msm_srs(srs: *const lw_srs_t, scalars: *const u64, n_scalars: usize, out_point: *mut c_void) -> c_int;
    pub fn lw_hip_msm_srs_device(srs: *const lw_srs_t, d_scalars: *const u64, n_scalars: usize, out_point_host: *mut c_void,
                                 hip_stream: *mut c_void) -> c_int;
    pub fn lw_hip_msm_srs_fr(srs: *const lw_srs_t, fr_elements: *const u64, n_scalars: usize, out_point: *mut c_void) -> c_int;
    pub fn lw_hip_msm_srs_fr_device(srs: *const lw_srs_t, d_fr_elements: *const u64, n_scalars: usize, out_point_host: *mut c_void,
                                    hip_stream: *mut c_void) -> c_int;
    // ---- polynomial evaluation / Ruffini division; KZG openings (4 x u64 Montgomery elements; points, x, upsilon on the host)
    pub fn lw_poly_evaluate(field: Field, polys: *const *const c_void, lens: *const usize, k: u32, points: *const c_void, m: u32,
                            out_values: *mut c_void) -> c_int;
    pub fn lw_poly_evaluate_device(field: Field, d_polys: *const *const c_void, lens: *const usize, k: u32, points: *const c_void,
                                   m: u32, out_values_host: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn lw_poly_ruffini_division(field: Field, coeffs: *const c_void, n: usize, x: *const c_void, out_quotient: *mut c_void,
                                    out_remainder_or_null: *mut c_void) -> c_int;
    pub fn lw_poly_ruffini_division_device(field: Field, d_coeffs: *const c_void, n: usize, x: *const c_void,
                                           d_out_quotient: *mut c_void, out_remainder_host_or_null: *mut c_void,
                                           hip_stream: *mut c_void) -> c_int;
    pub fn lw_kzg_open(srs: *const lw_srs_t, coeffs: *const u64, n: usize, x: *const u64, out_proof: *mut c_void,
                       out_eval_or_null: *mut u64) -> c_int;
    pub fn lw_kzg_open_device(srs: *const lw_srs_t, d_coeffs: *const u64, n: usize, x: *const u64, out_proof_host: *mut c_void,
                              out_eval_host_or_null: *mut u64, hip_stream: *mut c_void) -> c_int;
    pub fn lw_kzg_open_batch(srs: *const lw_srs_t, polys: *const *const u64, lens: *const usize, k: u32, x: *const u64,
                             upsilon: *const u64, out_proof: *mut c_void, out_evals_or_null: *mut u64) -> c_int;
    pub fn lw_kzg_open_batch_device(srs: *const lw_srs_t, d_polys: *const *const u64, lens: *const usize, k: u32, x: *const u64,
                                    upsilon: *const u64, out_proof_host: *mut c_void, out_evals_host_or_null: *mut u64,
                                    hip_stream: *mut c_void) -> c_int;
    // ---- STARK DEEP composition polynomial (points and the k x m weight matrix on the host)
    pub fn lw_stark_deep_composition(field: Field, polys: *const *const c_void, lens: *const usize, k: u32, points: *const c_void,
                                     m: u32, weights: *const c_void, out_coeffs: *mut c_void, out_len_or_null: *mut usize,
                                     out_evals_or_null: *mut c_void) -> c_int;
    pub fn lw_stark_deep_composition_device(field: Field, d_polys: *const *const c_void, lens: *const usize, k: u32,
                                            points: *const c_void, m: u32, weights: *const c_void, d_out_coeffs: *mut c_void,
                                            out_len_or_null: *mut usize, out_evals_host_or_null: *mut c_void,
                                            hip_stream: *mut c_void) -> c_int;
    // ---- STARK round 4 tail: grinding nonce search and query openings (seed, positions and every result on the host)
    pub fn lw_stark_grinding_window(grinding_factor: u32) -> u64;
    pub fn lw_stark_grinding_nonce(seed32: *const u8, grinding_factor: u32, first: u64, last: u64, out_nonce: *mut u64,
                                   out_found: *mut c_int) -> c_int;
    pub fn lw_stark_grinding_nonce_device(seed32: *const u8, grinding_factor: u32, first: u64, last: u64, out_nonce: *mut u64,
                                          out_found: *mut c_int, hip_stream: *mut c_void) -> c_int;
    pub fn lw_stark_open_trees_device(trees: *const lw_stark_tree_t, n_trees: u32, positions: *const u64, q: u32,
                                      out_values: *mut c_void, out_paths: *mut u8, hip_stream: *mut c_void) -> c_int;
    // ---- PLONK rounds 1-3 (k1, challenges, blinders and the public input on the host)
    pub fn lw_plonk_circuit_create(field: Field, n: usize, k1: *const c_void, q_coeffs: *const c_void, s_coeffs: *const c_void,
                                   s_lagrange: *const c_void, out: *mut *mut lw_plonk_circuit_t) -> c_int;
    pub fn lw_plonk_circuit_destroy(circuit: *mut lw_plonk_circuit_t) -> c_int;
    pub fn lw_plonk_round1(circuit: *const lw_plonk_circuit_t, witness: *const c_void, blinders_or_null: *const c_void,
                           out_p_abc: *mut c_void) -> c_int;
    pub fn lw_plonk_round1_device(circuit: *const lw_plonk_circuit_t, d_witness: *const c_void, blinders_or_null: *const c_void,
                                  d_out_p_abc: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn lw_plonk_round2(circuit: *const lw_plonk_circuit_t, witness: *const c_void, beta: *const c_void, gamma: *const c_void,
                           blinders_or_null: *const c_void, out_z_values_or_null: *mut c_void, out_p_z: *mut c_void) -> c_int;
    pub fn lw_plonk_round2_device(circuit: *const lw_plonk_circuit_t, d_witness: *const c_void, beta: *const c_void,
                                  gamma: *const c_void, blinders_or_null: *const c_void, d_out_z_values_or_null: *mut c_void,
                                  d_out_p_z: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn lw_plonk_round3(circuit: *const lw_plonk_circuit_t, p_abc: *const c_void, p_z: *const c_void, public_input: *const c_void,
                           n_pub: usize, beta: *const c_void, gamma: *const c_void, alpha: *const c_void,
                           blinders_or_null: *const c_void, out_t: *mut c_void) -> c_int;
    pub fn lw_plonk_round3_device(circuit: *const lw_plonk_circuit_t, d_p_abc: *const c_void, d_p_z: *const c_void,
                                  public_input: *const c_void, n_pub: usize, beta: *const c_void, gamma: *const c_void,
                                  alpha: *const c_void, blinders_or_null: *const c_void, d_out_t: *mut c_void,
                                  hip_stream: *mut c_void) -> c_int;
    // ---- Starknet Poseidon over Stark252: batched permutations, hashes and Merkle trees
    pub fn lw_poseidon_permute(states: *const c_void, n: usize, out: *mut c_void) -> c_int;
    pub fn lw_poseidon_permute_device(d_states: *const c_void, n: usize, d_out: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn lw_poseidon_hash(x: *const c_void, y: *const c_void, n: usize, out: *mut c_void) -> c_int;
    pub fn lw_poseidon_hash_device(d_x: *const c_void, d_y: *const c_void, n: usize, d_out: *mut c_void,
                                   hip_stream: *mut c_void) -> c_int;
    pub fn lw_poseidon_hash_single(x: *const c_void, n: usize, out: *mut c_void) -> c_int;
    pub fn lw_poseidon_hash_single_device(d_x: *const c_void, n: usize, d_out: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn lw_poseidon_hash_many(rows: *const c_void, n_rows: usize, row_len: usize, out: *mut c_void) -> c_int;
    pub fn lw_poseidon_hash_many_device(d_rows: *const c_void, n_rows: usize, row_len: usize, d_out: *mut c_void,
                                        hip_stream: *mut c_void) -> c_int;
    pub fn lw_poseidon_commit_columns(columns: *const c_void, n_cols: u32, log2n: u32, bit_reverse: c_int, leaf_mode: c_int,
                                      out_root: *mut u8, out_nodes_or_null: *mut u8) -> c_int;
    pub fn lw_poseidon_commit_columns_device(d_columns: *const c_void, n_cols: u32, col_stride_elems: u64, log2n: u32,
                                             bit_reverse: c_int, leaf_mode: c_int, d_nodes: *mut c_void, out_root: *mut u8,
                                             hip_stream: *mut c_void) -> c_int;
    // ---- Starknet Pedersen hash over the Stark curve: batched hashes, the tree over leaf values, the tables, the group-law seam
    pub fn lw_pedersen_hash(x: *const c_void, y: *const c_void, n: usize, out: *mut c_void) -> c_int;
    pub fn lw_pedersen_hash_device(d_x: *const c_void, d_y: *const c_void, n: usize, d_out: *mut c_void,
                                   hip_stream: *mut c_void) -> c_int;
    pub fn lw_pedersen_commit_leaves(leaves: *const c_void, n_cols: u32, log2n: u32, bit_reverse: c_int, out_root: *mut u8,
                                     out_nodes_or_null: *mut u8) -> c_int;
    pub fn lw_pedersen_commit_leaves_device(d_leaves: *const c_void, n_cols: u32, log2n: u32, bit_reverse: c_int,
                                            d_nodes: *mut c_void, out_root: *mut u8, hip_stream: *mut c_void) -> c_int;
    pub fn lw_pedersen_table(out: *mut c_void) -> c_int;
    pub fn lw_pedersen_add_affine_device(d_p: *const c_void, d_z: *const c_void, d_q: *const c_void, n: usize,
                                         d_out: *mut c_void, hip_stream: *mut c_void) -> c_int;
    // ---- dense multilinear polynomials and the sumcheck round (4 x u64 Montgomery elements; point, r, r_prev on the host)
    pub fn lw_multilinear_evaluate(field: Field, tables: *const *const c_void, k: u32, n_vars: u32, point: *const c_void,
                                   out: *mut c_void) -> c_int;
    pub fn lw_multilinear_evaluate_device(field: Field, d_tables: *const *const c_void, k: u32, n_vars: u32, point: *const c_void,
                                          out_host: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn lw_multilinear_fix_variables(field: Field, table: *const c_void, n_vars: u32, r: *const c_void, t: u32,
                                        out: *mut c_void) -> c_int;
    pub fn lw_multilinear_fix_variables_device(field: Field, d_table: *const c_void, n_vars: u32, r: *const c_void, t: u32,
                                               d_out: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn lw_sumcheck_round(field: Field, tables: *const *mut c_void, k: u32, n_vars: u32, r_prev_or_null: *const c_void,
                             out_round: *mut c_void) -> c_int;
    pub fn lw_sumcheck_round_device(field: Field, d_tables: *const *mut c_void, k: u32, n_vars: u32, r_prev_or_null: *const c_void,
                                    out_round_host: *mut c_void, hip_stream: *mut c_void) -> c_int;
    // ---- the table of eq(point, .) and the round over an eq-weighted sum of products (masks, coefficients on the host)
    pub fn lw_multilinear_eq_table(field: Field, point: *const c_void, n_vars: u32, out: *mut c_void) -> c_int;
    pub fn lw_multilinear_eq_table_device(field: Field, point: *const c_void, n_vars: u32, d_out: *mut c_void,
                                          hip_stream: *mut c_void) -> c_int;
    pub fn lw_sumcheck_terms_round(field: Field, tables: *const *mut c_void, n_tables: u32, eq_or_null: *mut c_void,
                                   term_masks: *const u32, term_coeffs_or_null: *const c_void, n_terms: u32, n_vars: u32,
                                   r_prev_or_null: *const c_void, out_round: *mut c_void) -> c_int;
    pub fn lw_sumcheck_terms_round_device(field: Field, d_tables: *const *mut c_void, n_tables: u32, d_eq_or_null: *mut c_void,
                                          term_masks: *const u32, term_coeffs_or_null: *const c_void, n_terms: u32, n_vars: u32,
                                          r_prev_or_null: *const c_void, out_round_host: *mut c_void,
                                          hip_stream: *mut c_void) -> c_int;
    // ---- a rank-one constraint system on the device: A z, B z, C z, the row-bound matrix, Groth16's h from a witness
    pub fn lw_r1cs_create(field: Field, n_rows: u32, n_cols: u32, row_ptr: *const *const u32, col_idx: *const *const u32,
                          values: *const *const c_void, out: *mut *mut lw_r1cs_t) -> c_int;
    pub fn lw_r1cs_destroy(r1cs: *mut lw_r1cs_t) -> c_int;
    pub fn lw_r1cs_split_length() -> u32;
    pub fn lw_r1cs_lazy_terms() -> u32;
    pub fn lw_r1cs_matvec(r1cs: *const lw_r1cs_t, z: *const c_void, n_out: usize, out_az_or_null: *mut c_void,
                          out_bz_or_null: *mut c_void, out_cz_or_null: *mut c_void) -> c_int;
    pub fn lw_r1cs_matvec_device(r1cs: *const lw_r1cs_t, d_z: *const c_void, n_out: usize, d_out_az_or_null: *mut c_void,
                                 d_out_bz_or_null: *mut c_void, d_out_cz_or_null: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn lw_r1cs_bind_rows(r1cs: *const lw_r1cs_t, e: *const c_void, coeffs3: *const c_void, n_out: usize,
                             out: *mut c_void) -> c_int;
    pub fn lw_r1cs_bind_rows_device(r1cs: *const lw_r1cs_t, d_e: *const c_void, coeffs3: *const c_void, n_out: usize,
                                    d_out: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn lw_r1cs_first_unsatisfied(r1cs: *const lw_r1cs_t, z: *const c_void, out_row: *mut i64) -> c_int;
    pub fn lw_r1cs_first_unsatisfied_device(r1cs: *const lw_r1cs_t, d_z: *const c_void, out_row: *mut i64,
                                            hip_stream: *mut c_void) -> c_int;
    pub fn lw_groth16_h_from_witness(r1cs: *const lw_r1cs_t, w: *const c_void, num_gates: usize, out_h: *mut c_void,
                                     coeff_len_or_null: *mut usize) -> c_int;
    pub fn lw_groth16_h_from_witness_device(r1cs: *const lw_r1cs_t, d_w: *const c_void, num_gates: usize, d_out_h: *mut c_void,
                                            coeff_len_or_null: *mut usize, hip_stream: *mut c_void) -> c_int;
    // ---- circle FFT over Mersenne31: one u32 per element, canonical residues out
    pub fn lw_circle_evaluate_cfft(coeffs: *const u32, out: *mut u32, log2n: u32, batch: u32, batch_stride: usize) -> c_int;
    pub fn lw_circle_interpolate_cfft(evals: *const u32, out: *mut u32, log2n: u32, batch: u32, batch_stride: usize) -> c_int;
    pub fn lw_circle_evaluate_cfft_device(d_in: *const u32, d_out: *mut u32, log2n: u32, batch: u32, batch_stride: usize,
                                          hip_stream: *mut c_void) -> c_int;
    pub fn lw_circle_interpolate_cfft_device(d_in: *const u32, d_out: *mut u32, log2n: u32, batch: u32, batch_stride: usize,
                                             hip_stream: *mut c_void) -> c_int;
    pub fn lw_circle_lde_device(d_evals: *const u32, log2_in: u32, in_stride: usize, d_out: *mut u32, log2_out: u32,
                                out_stride: usize, batch: u32, hip_stream: *mut c_void) -> c_int;
    pub fn lw_circle_get_twiddles(log2n: u32, config: c_int, out: *mut u32) -> c_int;
    // ---- NTT over Goldilocks (p = 2^64 - 2^32 + 1): one u64 per element, the residue itself, canonical residues out
    pub fn lw_goldilocks_ntt(dir: c_int, input: *const u64, out: *mut u64, log2n: u32, batch: u32, batch_stride: usize,
                             offset_or_null: *const u64, two_adic_root: u64) -> c_int;
    pub fn lw_goldilocks_ntt_device(dir: c_int, d_in: *const u64, d_out: *mut u64, log2n: u32, batch: u32, batch_stride: usize,
                                    offset_or_null: *const u64, two_adic_root: u64, hip_stream: *mut c_void) -> c_int;
    pub fn lw_goldilocks_lde_device(d_coeffs: *const u64, log2_coeffs: u32, in_stride: usize, d_out: *mut u64, log2n: u32,
                                    out_stride: usize, batch: u32, offset_or_null: *const u64, two_adic_root: u64,
                                    hip_stream: *mut c_void) -> c_int;
    pub fn lw_goldilocks_gen_twiddles(order: u64, config: c_int, two_adic_root: u64, out: *mut u64) -> c_int;
    pub fn lw_goldilocks_mul_device(d_a: *const u64, d_b: *const u64, d_out: *mut u64, n: usize, hip_stream: *mut c_void) -> c_int;
    // ---- Rescue Prime Optimized over Goldilocks: batched permutations, hashes and Merkle trees; level is LW_RPO_128 / LW_RPO_160
    pub fn lw_rpo_permute(level: c_int, states: *const u64, n: usize, out: *mut u64) -> c_int;
    pub fn lw_rpo_permute_device(level: c_int, d_states: *const u64, n: usize, d_out: *mut u64, hip_stream: *mut c_void) -> c_int;
    pub fn lw_rpo_hash(level: c_int, rows: *const u64, n_rows: usize, row_len: usize, out: *mut u64) -> c_int;
    pub fn lw_rpo_hash_device(level: c_int, d_rows: *const u64, n_rows: usize, row_len: usize, row_stride: usize, d_out: *mut u64,
                              hip_stream: *mut c_void) -> c_int;
    pub fn lw_rpo_commit_columns(level: c_int, columns: *const u64, n_cols: u32, log2n: u32, bit_reverse: c_int, out_root: *mut u64,
                                 out_nodes_or_null: *mut u64) -> c_int;
    pub fn lw_rpo_commit_columns_device(level: c_int, d_columns: *const u64, n_cols: u32, col_stride: u64, log2n: u32,
                                        bit_reverse: c_int, d_nodes: *mut u64, out_root_or_null: *mut u64,
                                        hip_stream: *mut c_void) -> c_int;
    // ---- Goldilocks quadratic extension F_p[t] / (t^2 - 7): an Fp2 vector is two planes of words, a host scalar is [c0, c1];
    // op is LW_GL2_MUL / LW_GL2_SQR / LW_GL2_INV / LW_GL2_MUL_BASE
    pub fn lw_goldilocks_ext2_pointwise_device(op: c_int, d_a: *const u64, a_stride: usize, d_b: *const u64, b_stride: usize,
                                               d_out: *mut u64, out_stride: usize, n: usize, hip_stream: *mut c_void) -> c_int;
    pub fn lw_goldilocks_ext2_evaluate_device(d_coeffs: *const u64, n_cols: u32, col_stride: usize, n_coeffs: usize,
                                              points: *const u64, m: u32, out_values: *mut u64, hip_stream: *mut c_void) -> c_int;
    pub fn lw_goldilocks_ext2_deep_quotients_device(d_lde: *const u64, n_cols: u32, col_stride: usize, log2n: u32,
                                                    offset_or_null: *const u64, two_adic_root: u64, points: *const u64, m: u32,
                                                    weights: *const u64, evals: *const u64, d_out: *mut u64, out_stride: usize,
                                                    hip_stream: *mut c_void) -> c_int;
    pub fn lw_goldilocks_ext2_fri_layer_device(d_coeffs: *const u64, coeff_stride: usize, n_coeffs: usize, zeta: *const u64,
                                               offset_or_null: *const u64, domain_size: usize, two_adic_root: u64, level: c_int,
                                               d_out_poly: *mut u64, d_out_evaluation_or_null: *mut u64,
                                               d_nodes_or_null: *mut u64, out_root_or_null: *mut u64,
                                               hip_stream: *mut c_void) -> c_int;
    // ---- BabyBear quartic extension F_p[x] / (x^4 + 11): an Fp4 vector is four planes of stored u32 words (R = 2^32), a host
    // scalar is [c0, c1, c2, c3]; op is LW_BB4_MUL / LW_BB4_SQR / LW_BB4_INV / LW_BB4_MUL_BASE, dir LW_BB4_TO_PLANES / LW_BB4_TO_INTERLEAVED
    pub fn lw_babybear_ext4_pointwise_device(op: c_int, d_a: *const u32, a_stride: usize, d_b: *const u32, b_stride: usize,
                                             d_out: *mut u32, out_stride: usize, n: usize, hip_stream: *mut c_void) -> c_int;
    pub fn lw_babybear_ext4_convert_device(dir: c_int, d_interleaved: *mut u64, d_planes: *mut u32, plane_stride: usize, n: usize,
                                           hip_stream: *mut c_void) -> c_int;
    pub fn lw_babybear_ext4_evaluate_device(d_coeffs: *const u32, n_cols: u32, col_stride: usize, n_coeffs: usize,
                                            points: *const u32, m: u32, out_values: *mut u32, hip_stream: *mut c_void) -> c_int;
    pub fn lw_babybear_ext4_deep_quotients_device(d_lde: *const u32, n_cols: u32, col_stride: usize, log2n: u32,
                                                  offset_or_null: *const u32, points: *const u32, m: u32, weights: *const u32,
                                                  evals: *const u32, d_out: *mut u32, out_stride: usize,
                                                  hip_stream: *mut c_void) -> c_int;
    pub fn lw_babybear_ext4_fri_layer_device(d_coeffs: *const u32, coeff_stride: usize, n_coeffs: usize, zeta: *const u32,
                                             offset_or_null: *const u32, domain_size: usize, d_out_poly: *mut u32,
                                             d_out_evaluation_or_null: *mut u32, d_nodes_or_null: *mut u8,
                                             out_root_or_null: *mut u8, hip_stream: *mut c_void) -> c_int;
    // ---- STARK round 2 over Goldilocks with Fp2 and BabyBear with Fp4: the constraint evaluations in one pass over the LDE
    // columns (the AIR's program, the zerofiers, the random linear combination in the extension, the boundary quotients)
    // and the parts of the composition polynomial, part j plane e at plane j D + e
    pub fn lw_goldilocks_ext2_constraint_evaluations_device(ops: *const lw_stark_air_op_t, n_ops: u32, consts: *const u64, n_consts: u32,
                                                            d_columns: *const *const u64, col_log2_len_or_null: *const u32, n_cols: u32,
                                                            log2_trace: u32, log2_blowup: u32, offset_or_null: *const u64,
                                                            two_adic_root: u64, boundary: *const lw_gl2_boundary_t, n_boundary: u32,
                                                            transitions: *const lw_gl2_transition_t, n_transitions: u32,
                                                            d_out: *mut u64, out_stride: usize, hip_stream: *mut c_void) -> c_int;
    pub fn lw_goldilocks_ext2_composition_parts_device(d_evals: *const u64, evals_stride: usize, log2_lde: u32,
                                                       offset_or_null: *const u64, two_adic_root: u64, n_parts: u32,
                                                       d_parts_coeffs: *mut u64, d_parts_lde_or_null: *mut u64,
                                                       out_part_lens_or_null: *mut usize, hip_stream: *mut c_void) -> c_int;
    pub fn lw_babybear_ext4_constraint_evaluations_device(ops: *const lw_stark_air_op_t, n_ops: u32, consts: *const u32, n_consts: u32,
                                                          d_columns: *const *const u32, col_log2_len_or_null: *const u32, n_cols: u32,
                                                          log2_trace: u32, log2_blowup: u32, offset_or_null: *const u32,
                                                          boundary: *const lw_bb4_boundary_t, n_boundary: u32,
                                                          transitions: *const lw_bb4_transition_t, n_transitions: u32,
                                                          d_out: *mut u32, out_stride: usize, hip_stream: *mut c_void) -> c_int;
    pub fn lw_babybear_ext4_composition_parts_device(d_evals: *const u32, evals_stride: usize, log2_lde: u32,
                                                     offset_or_null: *const u32, n_parts: u32, d_parts_coeffs: *mut u32,
                                                     d_parts_lde_or_null: *mut u32, out_part_lens_or_null: *mut usize,
                                                     hip_stream: *mut c_void) -> c_int;
    // ---- RAP over Fp2 and Fp4: the auxiliary column (running product or sum of fractions) and the round 2 that reads it
    pub fn lw_goldilocks_ext2_aux_fractions_device(d_columns: *const *const u64, n_cols: u32, n: usize, num_const: *const u64,
                                                   num_cols: *const u32, num_coeffs: *const u64, n_num: u32, den_const: *const u64,
                                                   den_cols: *const u32, den_coeffs: *const u64, n_den: u32, mode: u32, d_out: *mut u64,
                                                   out_stride: usize, d_total_or_null: *mut u64,
                                                   out_zero_denominators_or_null: *mut u64, hip_stream: *mut c_void) -> c_int;
    pub fn lw_babybear_ext4_aux_fractions_device(d_columns: *const *const u32, n_cols: u32, n: usize, num_const: *const u32,
                                                 num_cols: *const u32, num_coeffs: *const u32, n_num: u32, den_const: *const u32,
                                                 den_cols: *const u32, den_coeffs: *const u32, n_den: u32, mode: u32, d_out: *mut u32,
                                                 out_stride: usize, d_total_or_null: *mut u32,
                                                 out_zero_denominators_or_null: *mut u64, hip_stream: *mut c_void) -> c_int;
    pub fn lw_goldilocks_ext2_rap_constraint_evaluations_device(ops: *const lw_stark_air_op_t, n_ops: u32, consts: *const u64, n_consts: u32,
                                                                xconsts: *const u64, n_xconsts: u32, d_columns: *const *const u64,
                                                                col_log2_len_or_null: *const u32, n_cols: u32,
                                                                d_aux_columns: *const *const u64, n_aux: u32, aux_stride: usize,
                                                                log2_trace: u32, log2_blowup: u32, offset_or_null: *const u64,
                                                                two_adic_root: u64, boundary: *const lw_gl2_rap_boundary_t, n_boundary: u32,
                                                                transitions: *const lw_gl2_transition_t, n_transitions: u32,
                                                                d_out: *mut u64, out_stride: usize, hip_stream: *mut c_void) -> c_int;
    pub fn lw_babybear_ext4_rap_constraint_evaluations_device(ops: *const lw_stark_air_op_t, n_ops: u32, consts: *const u32, n_consts: u32,
                                                              xconsts: *const u32, n_xconsts: u32, d_columns: *const *const u32,
                                                              col_log2_len_or_null: *const u32, n_cols: u32,
                                                              d_aux_columns: *const *const u32, n_aux: u32, aux_stride: usize,
                                                              log2_trace: u32, log2_blowup: u32, offset_or_null: *const u32,
                                                              boundary: *const lw_bb4_rap_boundary_t, n_boundary: u32,
                                                              transitions: *const lw_bb4_transition_t, n_transitions: u32,
                                                              d_out: *mut u32, out_stride: usize, hip_stream: *mut c_void) -> c_int;
    // ---- Monolith over Mersenne31: batched permutations (width 8 .. 24, rounds 1 .. 15); hash, compression and Merkle tree over width 16
    pub fn lw_monolith_permute(width: u32, rounds: u32, states: *const u32, n: usize, out: *mut u32) -> c_int;
    pub fn lw_monolith_permute_device(width: u32, rounds: u32, d_states: *const u32, n: usize, d_out: *mut u32,
                                      hip_stream: *mut c_void) -> c_int;
    pub fn lw_monolith_hash(rounds: u32, rows: *const u32, n_rows: usize, row_len: usize, out: *mut u32) -> c_int;
    pub fn lw_monolith_hash_device(rounds: u32, d_rows: *const u32, n_rows: usize, row_len: usize, row_stride: usize, d_out: *mut u32,
                                   hip_stream: *mut c_void) -> c_int;
    pub fn lw_monolith_compress(rounds: u32, left: *const u32, right: *const u32, n: usize, out: *mut u32) -> c_int;
    pub fn lw_monolith_compress_device(rounds: u32, d_left: *const u32, d_right: *const u32, n: usize, d_out: *mut u32,
                                       hip_stream: *mut c_void) -> c_int;
    pub fn lw_monolith_commit_columns(rounds: u32, columns: *const u32, n_cols: u32, log2n: u32, bit_reverse: c_int, out_root: *mut u32,
                                      out_nodes_or_null: *mut u32) -> c_int;
    pub fn lw_monolith_commit_columns_device(rounds: u32, d_columns: *const u32, n_cols: u32, col_stride: u64, log2n: u32,
                                             bit_reverse: c_int, d_nodes: *mut u32, out_root_or_null: *mut u32,
                                             hip_stream: *mut c_void) -> c_int;
    pub fn lw_monolith_constants(width: u32, rounds: u32, out_round_constants: *mut u32, out_mds: *mut u32) -> c_int;
    pub fn lw_monolith_layer_device(width: u32, rounds: u32, layer: c_int, d_states: *const u32, n: usize, d_out: *mut u32,
                                    hip_stream: *mut c_void) -> c_int;
    // ---- the quartic extension of Mersenne31 (QM31) and the circle-STARK steps in it: words as in the circle FFT, a host
    // scalar is [c0, c1, c2, c3], a point [X, Y] is 8 words; op is LW_M31EXT4_MUL / SQR / INV / MUL_BASE
    pub fn lw_mersenne31_ext4_pointwise_device(op: c_int, d_a: *const u32, a_stride: usize, d_b: *const u32, b_stride: usize,
                                               d_out: *mut u32, out_stride: usize, n: usize, hip_stream: *mut c_void) -> c_int;
    pub fn lw_mersenne31_ext4_evaluate_device(d_coeffs: *const u32, n_cols: u32, col_stride: usize, log2n: u32,
                                              points: *const u32, m: u32, out_values: *mut u32, hip_stream: *mut c_void) -> c_int;
    pub fn lw_mersenne31_ext4_deep_quotients_device(d_lde: *const u32, n_cols: u32, col_stride: usize, log2n: u32,
                                                    points: *const u32, m: u32, weights: *const u32, evals: *const u32,
                                                    d_out: *mut u32, out_stride: usize, hip_stream: *mut c_void) -> c_int;
    pub fn lw_mersenne31_ext4_fri_layer_device(d_evals: *const u32, in_stride: usize, log2m: u32, zeta: *const u32, first: c_int,
                                               d_out: *mut u32, out_stride: usize, rounds: u32, d_pairs_or_null: *mut u32,
                                               d_nodes_or_null: *mut u32, out_root_or_null: *mut u32,
                                               hip_stream: *mut c_void) -> c_int;
    // ---- circle STARK round 2 over QM31: the fused constraint pass on the LDE coset and the parts (index blocks) of its result
    pub fn lw_mersenne31_ext4_constraint_evaluations_device(ops: *const lw_stark_air_op_t, n_ops: u32, consts: *const u32, n_consts: u32,
                                                            d_columns: *const *const u32, col_log2_len_or_null: *const u32, n_cols: u32,
                                                            log2_trace: u32, log2_blowup: u32,
                                                            boundary: *const lw_m31q_boundary_t, n_boundary: u32,
                                                            transitions: *const lw_m31q_transition_t, n_transitions: u32,
                                                            d_out: *mut u32, out_stride: usize, hip_stream: *mut c_void) -> c_int;
    pub fn lw_mersenne31_ext4_composition_parts_device(d_evals: *const u32, evals_stride: usize, log2_lde: u32, log2_part: u32,
                                                       n_parts: u32, d_parts_coeffs: *mut u32, d_parts_lde_or_null: *mut u32,
                                                       out_tail_nonzero_or_null: *mut u64, hip_stream: *mut c_void) -> c_int;
    // ---- batch inversion and STARK round 2 (the coset offset, the constraint tables and every small result on the host)
    pub fn lw_field_batch_inverse(field: Field, input: *const c_void, n: usize, out: *mut c_void) -> c_int;
    pub fn lw_field_batch_inverse_device(field: Field, d_in: *const c_void, n: usize, d_out: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn lw_field_batch_inverse_block() -> u64;
    pub fn lw_stark_constraint_evaluations_device(field: Field, d_columns: *const *const c_void, n_cols: u32, log2_trace: u32,
                                                  log2_blowup: u32, coset_offset: *const c_void, boundary: *const lw_stark_boundary_t,
                                                  n_boundary: u32, transitions: *const lw_stark_transition_t, n_transitions: u32,
                                                  d_transition_evals: *const c_void, transition_stride_elems: u64, d_out: *mut c_void,
                                                  hip_stream: *mut c_void) -> c_int;
    pub fn lw_stark_composition_parts_device(field: Field, d_evals: *const c_void, log2_lde: u32, coset_offset: *const c_void,
                                             n_parts: u32, d_parts_coeffs: *mut c_void, d_parts_lde: *mut c_void,
                                             out_part_lens_or_null: *mut usize, hip_stream: *mut c_void) -> c_int;
    pub fn lw_stark_commit_composition_device(field: Field, d_parts_lde: *const c_void, n_parts: u32, col_stride_elems: u64,
                                              log2_lde: u32, d_nodes: *mut c_void, out_root_or_null: *mut u8,
                                              hip_stream: *mut c_void) -> c_int;
    pub fn lw_stark_round2(field: Field, columns: *const c_void, n_cols: u32, log2_trace: u32, log2_blowup: u32,
                           coset_offset: *const c_void, boundary: *const lw_stark_boundary_t, n_boundary: u32,
                           transitions: *const lw_stark_transition_t, n_transitions: u32, transition_evals: *const c_void,
                           n_parts: u32, out_parts_coeffs: *mut c_void, out_part_lens: *mut usize, out_root: *mut u8,
                           out_nodes_or_null: *mut u8, out_parts_lde_or_null: *mut c_void) -> c_int;
    // ---- STARK transition constraints from an AIR given as data (the program and the constants on the host)
    pub fn lw_stark_transition_evaluations_device(field: Field, ops: *const lw_stark_air_op_t, n_ops: u32, consts: *const c_void,
                                                  n_consts: u32, d_columns: *const *const c_void, col_log2_len_or_null: *const u32,
                                                  n_cols: u32, log2_trace: u32, log2_blowup: u32, n_transitions: u32,
                                                  d_out: *mut c_void, out_stride_elems: u64, hip_stream: *mut c_void) -> c_int;
    pub fn lw_stark_transition_evaluations(field: Field, ops: *const lw_stark_air_op_t, n_ops: u32, consts: *const c_void,
                                           n_consts: u32, columns: *const c_void, col_log2_len_or_null: *const u32, n_cols: u32,
                                           log2_trace: u32, log2_blowup: u32, n_transitions: u32, out: *mut c_void) -> c_int;
}

/// lw_stark_boundary_t: one boundary constraint of lw_stark_constraint_evaluations_device
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct lw_stark_boundary_t {
    /// index into the column table (main columns, then auxiliary ones)
    pub col: u32,
    pub reserved: u32,
    pub step: u64,
    pub value: [u64; 4],
    pub coeff: [u64; 4],
}

/// lw_stark_transition_t: the zerofier parameters and the coefficient of one transition constraint
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct lw_stark_transition_t {
    pub period: u64,
    pub offset: u64,
    pub end_exemptions: u64,
    /// 0: none
    pub exemptions_period: u64,
    pub periodic_exemptions_offset: u64,
    pub coeff: [u64; 4],
}

/// lw_gl2_boundary_t: one boundary constraint of lw_goldilocks_ext2_constraint_evaluations_device (value in F, coeff in Fp2)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct lw_gl2_boundary_t {
    pub col: u32,
    pub reserved: u32,
    pub step: u64,
    pub value: u64,
    pub coeff: [u64; 2],
}

/// lw_gl2_transition_t: the zerofier parameters and the Fp2 coefficient of one transition constraint
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct lw_gl2_transition_t {
    pub period: u64,
    pub offset: u64,
    pub end_exemptions: u64,
    /// 0: none
    pub exemptions_period: u64,
    pub periodic_exemptions_offset: u64,
    pub coeff: [u64; 2],
}

/// lw_bb4_boundary_t: one boundary constraint of lw_babybear_ext4_constraint_evaluations_device (stored words)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct lw_bb4_boundary_t {
    pub col: u32,
    pub reserved: u32,
    pub step: u64,
    pub value: u32,
    pub coeff: [u32; 4],
    pub reserved2: u32,
}

/// lw_gl2_rap_boundary_t: one boundary constraint of lw_goldilocks_ext2_rap_constraint_evaluations_device, its value in Fp2
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct lw_gl2_rap_boundary_t {
    pub col: u32,
    /// not 0: col indexes the auxiliary columns
    pub is_aux: u32,
    pub step: u64,
    pub value: [u64; 2],
    pub coeff: [u64; 2],
}

/// lw_bb4_rap_boundary_t: one boundary constraint of lw_babybear_ext4_rap_constraint_evaluations_device, its value in Fp4
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct lw_bb4_rap_boundary_t {
    pub col: u32,
    /// not 0: col indexes the auxiliary columns
    pub is_aux: u32,
    pub step: u64,
    pub value: [u32; 4],
    pub coeff: [u32; 4],
}

/// lw_bb4_transition_t: the zerofier parameters and the Fp4 coefficient of one transition constraint
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct lw_bb4_transition_t {
    pub period: u64,
    pub offset: u64,
    pub end_exemptions: u64,
    /// 0: none
    pub exemptions_period: u64,
    pub periodic_exemptions_offset: u64,
    pub coeff: [u32; 4],
}

/// lw_m31q_boundary_t: one boundary constraint of lw_mersenne31_ext4_constraint_evaluations_device (any u32 is a word)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct lw_m31q_boundary_t {
    pub col: u32,
    pub reserved: u32,
    /// the trace row, below n
    pub step: u64,
    pub value: u32,
    pub coeff: [u32; 4],
    pub reserved2: u32,
}

/// lw_m31q_transition_t: the zerofier parameters and the QM31 coefficient of one transition constraint on the circle
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct lw_m31q_transition_t {
    /// a power of two from 1 to n / 2
    pub period: u64,
    pub offset: u64,
    pub end_exemptions: u64,
    pub coeff: [u32; 4],
}

/// lw_stark_air_op_t: one instruction of an AIR transition program (lw_stark_transition_evaluations_device)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct lw_stark_air_op_t {
    /// LW_STARK_AIR_LOAD .. LW_STARK_AIR_EMIT
    pub op: u8,
    /// LW_STARK_AIR_CELL / CONST / TMP, for LOAD, ADD, SUB and MUL
    pub src: u8,
    /// column, constant, temporary or constraint
    pub index: u16,
    /// trace-row offset of a CELL operand
    pub row: u32,
}
/// lw_stark_air_opcode_t
pub const LW_STARK_AIR_LOAD: u8 = 0;
pub const LW_STARK_AIR_ADD: u8 = 1;
pub const LW_STARK_AIR_SUB: u8 = 2;
pub const LW_STARK_AIR_MUL: u8 = 3;
pub const LW_STARK_AIR_NEG: u8 = 4;
pub const LW_STARK_AIR_STORE: u8 = 5;
pub const LW_STARK_AIR_EMIT: u8 = 6;
/// lw_stark_air_src_t
pub const LW_STARK_AIR_CELL: u8 = 0;
pub const LW_STARK_AIR_CONST: u8 = 1;
pub const LW_STARK_AIR_TMP: u8 = 2;
/// the _rap_ entry points only: an auxiliary column, a constant of the extension
pub const LW_STARK_AIR_XCELL: u8 = 3;
pub const LW_STARK_AIR_XCONST: u8 = 4;
/// lw_ext_aux_mode_t
pub const LW_EXT_AUX_PRODUCT: u32 = 0;
pub const LW_EXT_AUX_SUM: u32 = 1;
pub const LW_EXT_AUX_EXCLUSIVE: u32 = 2;
pub const LW_EXT_AUX_MAX_TERMS: u32 = 16;
pub const LW_STARK_AIR_MAX_OPS: u32 = 4096;
pub const LW_STARK_AIR_MAX_TMPS: u32 = 8;
pub const LW_STARK_AIR_MAX_CONSTS: u32 = 256;

/// lw_poseidon_leaf_t: TreePoseidon (leaf = hash_single of one column)
pub const LW_POSEIDON_LEAF_SINGLE: c_int = 0;
/// lw_poseidon_leaf_t: BatchPoseidonTree (leaf = hash_many of the row)
pub const LW_POSEIDON_LEAF_MANY: c_int = 1;
/// lw_ec_op_t
pub const LW_EC_OP_ADD: c_int = 0;
pub const LW_EC_OP_ADD_MIXED: c_int = 1;
pub const LW_EC_OP_DBL: c_int = 2;
pub const LW_EC_OP_ADD_QUAD: c_int = 3;
pub const LW_EC_OP_TO_AFFINE: c_int = 4;
/// lw_pw_field_t
pub const LW_PW_FIELD_STARK252: c_int = 0;
pub const LW_PW_FIELD_FR381: c_int = 1;
pub const LW_PW_FIELD_FR254: c_int = 2;
pub const LW_PW_FIELD_FP381: c_int = 3;
pub const LW_PW_FIELD_FP254: c_int = 4;
pub const LW_PW_FIELD_BABYBEAR: c_int = 5;
/// lw_field_op_t
pub const LW_FIELD_OP_ADD: c_int = 0;
pub const LW_FIELD_OP_SUB: c_int = 1;
pub const LW_FIELD_OP_NEG: c_int = 2;
pub const LW_FIELD_OP_DBL: c_int = 3;
pub const LW_FIELD_OP_MUL: c_int = 4;
pub const LW_FIELD_OP_SQR: c_int = 5;
pub const LW_FIELD_OP_MUL_LAZY: c_int = 6;
pub const LW_FIELD_OP_MUL_LAZY_UNIFORM: c_int = 7;
pub const LW_FIELD_OP_REDUCE_FULL: c_int = 8;
pub const LW_FIELD_OP_COND_SUB_P: c_int = 9;
pub const LW_FIELD_OP_ADD_RAW: c_int = 10;
pub const LW_FIELD_OP_ADD2P_SUB_RAW: c_int = 11;
pub const LW_FIELD_OP_NEG_RAW: c_int = 12;
pub const LW_FIELD_OP_NEG_RAW_2P: c_int = 13;
pub const LW_FIELD_OP_TO_MONT: c_int = 14;
pub const LW_FIELD_OP_FROM_MONT: c_int = 15;
pub const LW_FIELD_OP_DOT2: c_int = 16;
pub const LW_FIELD_OP_DOT4: c_int = 17;
pub const LW_FIELD_OP_INV: c_int = 18;
pub const LW_FIELD_OP_REDUCE64: c_int = 19;
pub const LW_FIELD_OP_FROM_R64: c_int = 20;
pub const LW_FIELD_OP_TO_R64: c_int = 21;

/// lw_rpo_level_t: state 12, capacity 4, rate 8, digest 4 words
pub const LW_RPO_128: c_int = 0;
/// lw_rpo_level_t: state 16, capacity 6, rate 10, digest 5 words
pub const LW_RPO_160: c_int = 1;

/// lw_gl2_op_t: the operation of lw_goldilocks_ext2_pointwise_device
pub const LW_GL2_MUL: c_int = 0;
pub const LW_GL2_SQR: c_int = 1;
pub const LW_GL2_INV: c_int = 2;
pub const LW_GL2_MUL_BASE: c_int = 3;

/// lw_bb4_op_t: the operation of lw_babybear_ext4_pointwise_device
pub const LW_BB4_MUL: c_int = 0;
pub const LW_BB4_SQR: c_int = 1;
pub const LW_BB4_INV: c_int = 2;
pub const LW_BB4_MUL_BASE: c_int = 3;
/// lw_bb4_convert_t: the direction of lw_babybear_ext4_convert_device
pub const LW_BB4_TO_PLANES: c_int = 0;
pub const LW_BB4_TO_INTERLEAVED: c_int = 1;

/// lw_m31ext4_op_t: the operation of lw_mersenne31_ext4_pointwise_device
pub const LW_M31EXT4_MUL: c_int = 0;
pub const LW_M31EXT4_SQR: c_int = 1;
pub const LW_M31EXT4_INV: c_int = 2;
pub const LW_M31EXT4_MUL_BASE: c_int = 3;
/// lw_monolith_layer_t: the layer lw_monolith_layer_device applies
pub const LW_MONOLITH_CONCRETE: c_int = 0;
pub const LW_MONOLITH_BARS: c_int = 1;
pub const LW_MONOLITH_BRICKS: c_int = 2;

// The C structs above must keep the sizes the header gives them.
const _: () = assert!(core::mem::size_of::<lw_timings_t>() == 48);
const _: () = assert!(core::mem::size_of::<lw_kernel_time_t>() == 64);
const _: () = assert!(core::mem::size_of::<lw_profile_t>() == 8 + 32 * 64);
const _: () = assert!(core::mem::size_of::<lw_stark_tree_t>() == 56);
const _: () = assert!(core::mem::size_of::<lw_stark_boundary_t>() == 80);
const _: () = assert!(core::mem::size_of::<lw_gl2_boundary_t>() == 40 && core::mem::size_of::<lw_gl2_transition_t>() == 56);
const _: () = assert!(core::mem::size_of::<lw_bb4_boundary_t>() == 40 && core::mem::size_of::<lw_bb4_transition_t>() == 56);
const _: () = assert!(core::mem::size_of::<lw_gl2_rap_boundary_t>() == 48 && core::mem::size_of::<lw_bb4_rap_boundary_t>() == 48);
const _: () = assert!(core::mem::size_of::<lw_m31q_boundary_t>() == 40 && core::mem::size_of::<lw_m31q_transition_t>() == 40);
const _: () = assert!(core::mem::size_of::<lw_stark_transition_t>() == 72);
const _: () = assert!(core::mem::size_of::<lw_stark_air_op_t>() == 8);
