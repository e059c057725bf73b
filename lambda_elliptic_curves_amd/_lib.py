"""ctypes binding of include/lw_hip.h (liblw_hip.so, gfx950 code objects only).

There is no CPU fallback anywhere in this package: if the HIP library is missing or no MI355X is
visible, every compute entry point raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "liblw_hip.so")

# lw_field_t / lw_layout_t / lw_dir_t / lw_curve_t / lw_status_t (include/lw_hip.h)
FIELD_STARK252, FIELD_BLS12_381_FR, FIELD_BABYBEAR = 0, 1, 2
LAYOUT_U64_LIMBS_MS_FIRST, LAYOUT_BABYBEAR_U32_R32, LAYOUT_BABYBEAR_U64_R64, LAYOUT_EXT4_INTERLEAVED = 0, 1, 2, 3
DIR_FORWARD, DIR_INVERSE = 0, 1
CURVE_BLS12_381_G1, CURVE_BN254_G1, CURVE_BN254_G2, CURVE_BLS12_381_G2 = 0, 1, 2, 3
EC_OP_ADD, EC_OP_ADD_MIXED, EC_OP_DBL, EC_OP_ADD_QUAD, EC_OP_TO_AFFINE = 0, 1, 2, 3, 4   # lw_ec_op_t
PW_FIELD_STARK252, PW_FIELD_FR381, PW_FIELD_FR254, PW_FIELD_FP381, PW_FIELD_FP254, PW_FIELD_BABYBEAR = range(6)   # lw_pw_field_t
(FIELD_OP_ADD, FIELD_OP_SUB, FIELD_OP_NEG, FIELD_OP_DBL, FIELD_OP_MUL, FIELD_OP_SQR, FIELD_OP_MUL_LAZY, FIELD_OP_MUL_LAZY_UNIFORM,
 FIELD_OP_REDUCE_FULL, FIELD_OP_COND_SUB_P, FIELD_OP_ADD_RAW, FIELD_OP_ADD2P_SUB_RAW, FIELD_OP_NEG_RAW, FIELD_OP_NEG_RAW_2P,
 FIELD_OP_TO_MONT, FIELD_OP_FROM_MONT, FIELD_OP_DOT2, FIELD_OP_DOT4, FIELD_OP_INV, FIELD_OP_REDUCE64, FIELD_OP_FROM_R64,
 FIELD_OP_TO_R64) = range(22)   # lw_field_op_t
POSEIDON_LEAF_SINGLE, POSEIDON_LEAF_MANY = 0, 1   # lw_poseidon_leaf_t
RPO_128, RPO_160 = 0, 1   # lw_rpo_level_t
GL2_MUL, GL2_SQR, GL2_INV, GL2_MUL_BASE = 0, 1, 2, 3   # lw_gl2_op_t
BB4_MUL, BB4_SQR, BB4_INV, BB4_MUL_BASE = 0, 1, 2, 3   # lw_bb4_op_t
BB4_TO_PLANES, BB4_TO_INTERLEAVED = 0, 1   # lw_bb4_convert_t
MONOLITH_CONCRETE, MONOLITH_BARS, MONOLITH_BRICKS = 0, 1, 2   # lw_monolith_layer_t
M31EXT4_MUL, M31EXT4_SQR, M31EXT4_INV, M31EXT4_MUL_BASE = 0, 1, 2, 3   # lw_m31ext4_op_t
AIR_LOAD, AIR_ADD, AIR_SUB, AIR_MUL, AIR_NEG, AIR_STORE, AIR_EMIT = range(7)   # lw_stark_air_opcode_t
AIR_CELL, AIR_CONST, AIR_TMP = 0, 1, 2   # lw_stark_air_src_t
AIR_XCELL, AIR_XCONST = 3, 4             # the same, of the _rap_ entry points: an auxiliary column, a constant of E
EXT_AUX_PRODUCT, EXT_AUX_SUM, EXT_AUX_EXCLUSIVE, EXT_AUX_MAX_TERMS = 0, 1, 2, 16   # lw_ext_aux_mode_t, LW_EXT_AUX_MAX_TERMS
AIR_MAX_OPS, AIR_MAX_TMPS, AIR_MAX_CONSTS = 4096, 8, 256   # LW_STARK_AIR_MAX_*
(OK, ERR_INPUT_NOT_POW2, ERR_ORDER_TOO_LARGE, ERR_ROOT_OF_UNITY, ERR_LENGTH_MISMATCH, ERR_NO_DEVICE, ERR_ALLOC,
 ERR_LAUNCH, ERR_COMM, ERR_BAD_ARG, ERR_INV_ZERO) = (0, -1, -2, -3, -4, -5, -6, -7, -8, -9, -10)

EXPORTS = [
    "lw_hip_init", "lw_hip_shutdown", "lw_hip_device_count", "lw_hip_last_error", "lw_hip_get_timings",
    "lw_hip_profile_begin", "lw_hip_profile_end", "lw_hip_result_acquire", "lw_hip_result_release",
    "lw_hip_field_elem_bytes", "lw_hip_curve_point_bytes", "lw_hip_ntt", "lw_hip_ntt_device", "lw_hip_ntt_cross_device",
    "lw_hip_gen_twiddles", "lw_hip_gen_powers", "lw_hip_bitrev_permutation", "lw_hip_ntt_lde_device",
    "lw_polynomial_evaluate_fft", "lw_polynomial_interpolate_fft", "lw_hip_msm", "lw_hip_msm_device",
    "lw_hip_msm_fr", "lw_hip_msm_fr_device", "lw_hip_msm_limbs", "lw_hip_msm_limbs_device", "lw_groth16_h_coefficients",
    "lw_stark_commit_columns", "lw_stark_commit_columns_device", "lw_stark_commit_columns_layout_device", "lw_stark_fri_layer",
    "lw_hip_srs_create", "lw_hip_srs_create_device", "lw_hip_srs_destroy", "lw_hip_msm_srs", "lw_hip_msm_srs_device",
    "lw_hip_msm_srs_fr", "lw_hip_msm_srs_fr_device", "lw_stark_fri_layer_device", "lw_groth16_h_coefficients_device",
    "lw_hip_ec_add_outer_device", "lw_hip_ec_pointwise_device", "lw_hip_field_pointwise_device",
    "lw_hip_comm_unique_id", "lw_hip_comm_init", "lw_hip_comm_shutdown", "lw_hip_comm_info",
    "lw_hip_ntt_sharded_device", "lw_hip_ntt_sharded_selftest_device", "lw_hip_ntt_sharded_selftest_steps_device",
    "lw_hip_msm_sharded_device", "lw_hip_msm_sharded_selftest_device",
    "lw_poly_evaluate", "lw_poly_evaluate_device", "lw_poly_ruffini_division", "lw_poly_ruffini_division_device",
    "lw_kzg_open", "lw_kzg_open_device", "lw_kzg_open_batch", "lw_kzg_open_batch_device",
    "lw_stark_deep_composition", "lw_stark_deep_composition_device",
    "lw_plonk_circuit_create", "lw_plonk_circuit_destroy", "lw_plonk_round1", "lw_plonk_round1_device",
    "lw_plonk_round2", "lw_plonk_round2_device", "lw_plonk_round3", "lw_plonk_round3_device",
    "lw_stark_grinding_window", "lw_stark_grinding_nonce", "lw_stark_grinding_nonce_device", "lw_stark_open_trees_device",
    "lw_poseidon_permute", "lw_poseidon_permute_device", "lw_poseidon_hash", "lw_poseidon_hash_device",
    "lw_poseidon_hash_single", "lw_poseidon_hash_single_device", "lw_poseidon_hash_many", "lw_poseidon_hash_many_device",
    "lw_poseidon_commit_columns", "lw_poseidon_commit_columns_device",
    "lw_pedersen_hash", "lw_pedersen_hash_device", "lw_pedersen_commit_leaves", "lw_pedersen_commit_leaves_device",
    "lw_pedersen_table", "lw_pedersen_add_affine_device",
    "lw_circle_evaluate_cfft", "lw_circle_interpolate_cfft", "lw_circle_evaluate_cfft_device", "lw_circle_interpolate_cfft_device",
    "lw_circle_lde_device", "lw_circle_get_twiddles",
    "lw_goldilocks_ntt", "lw_goldilocks_ntt_device", "lw_goldilocks_lde_device", "lw_goldilocks_gen_twiddles",
    "lw_goldilocks_mul_device",
    "lw_goldilocks_ext2_pointwise_device", "lw_goldilocks_ext2_evaluate_device", "lw_goldilocks_ext2_deep_quotients_device",
    "lw_goldilocks_ext2_fri_layer_device",
    "lw_babybear_ext4_pointwise_device", "lw_babybear_ext4_convert_device", "lw_babybear_ext4_evaluate_device",
    "lw_babybear_ext4_deep_quotients_device", "lw_babybear_ext4_fri_layer_device",
    "lw_goldilocks_ext2_constraint_evaluations_device", "lw_goldilocks_ext2_composition_parts_device",
    "lw_babybear_ext4_constraint_evaluations_device", "lw_babybear_ext4_composition_parts_device",
    "lw_goldilocks_ext2_aux_fractions_device", "lw_babybear_ext4_aux_fractions_device",
    "lw_goldilocks_ext2_rap_constraint_evaluations_device", "lw_babybear_ext4_rap_constraint_evaluations_device",
    "lw_rpo_permute", "lw_rpo_permute_device", "lw_rpo_hash", "lw_rpo_hash_device",
    "lw_rpo_commit_columns", "lw_rpo_commit_columns_device",
    "lw_monolith_permute", "lw_monolith_permute_device", "lw_monolith_hash", "lw_monolith_hash_device",
    "lw_monolith_compress", "lw_monolith_compress_device", "lw_monolith_commit_columns", "lw_monolith_commit_columns_device",
    "lw_monolith_constants", "lw_monolith_layer_device",
    "lw_mersenne31_ext4_pointwise_device", "lw_mersenne31_ext4_evaluate_device", "lw_mersenne31_ext4_deep_quotients_device",
    "lw_mersenne31_ext4_fri_layer_device",
    "lw_mersenne31_ext4_constraint_evaluations_device", "lw_mersenne31_ext4_composition_parts_device",
    "lw_field_batch_inverse", "lw_field_batch_inverse_device", "lw_field_batch_inverse_block",
    "lw_stark_constraint_evaluations_device", "lw_stark_composition_parts_device", "lw_stark_commit_composition_device",
    "lw_stark_round2", "lw_stark_transition_evaluations_device", "lw_stark_transition_evaluations",
    "lw_multilinear_evaluate", "lw_multilinear_evaluate_device", "lw_multilinear_fix_variables",
    "lw_multilinear_fix_variables_device", "lw_sumcheck_round", "lw_sumcheck_round_device",
    "lw_multilinear_eq_table", "lw_multilinear_eq_table_device", "lw_sumcheck_terms_round", "lw_sumcheck_terms_round_device",
    "lw_r1cs_create", "lw_r1cs_destroy", "lw_r1cs_split_length", "lw_r1cs_lazy_terms", "lw_r1cs_matvec", "lw_r1cs_matvec_device",
    "lw_r1cs_bind_rows", "lw_r1cs_bind_rows_device", "lw_r1cs_first_unsatisfied", "lw_r1cs_first_unsatisfied_device",
    "lw_groth16_h_from_witness", "lw_groth16_h_from_witness_device",
]


class Timings(C.Structure):
    _fields_ = [("last_ntt_ms", C.c_double), ("last_msm_ms", C.c_double), ("ntt_calls", C.c_uint64),
                ("msm_calls", C.c_uint64), ("twiddle_bytes", C.c_uint64), ("scratch_bytes", C.c_uint64)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double)]


class StarkTree(C.Structure):
    """lw_stark_tree_t"""
    _fields_ = [("field", C.c_int), ("d_columns", C.c_void_p), ("n_cols", C.c_uint32), ("col_stride_elems", C.c_uint64),
                ("log2_rows", C.c_uint32), ("rows_per_leaf", C.c_uint32), ("bit_reverse", C.c_int), ("d_nodes", C.c_void_p)]


class StarkBoundary(C.Structure):
    """lw_stark_boundary_t"""
    _fields_ = [("col", C.c_uint32), ("reserved", C.c_uint32), ("step", C.c_uint64), ("value", C.c_uint64 * 4),
                ("coeff", C.c_uint64 * 4)]


class StarkTransition(C.Structure):
    """lw_stark_transition_t"""
    _fields_ = [("period", C.c_uint64), ("offset", C.c_uint64), ("end_exemptions", C.c_uint64), ("exemptions_period", C.c_uint64),
                ("periodic_exemptions_offset", C.c_uint64), ("coeff", C.c_uint64 * 4)]


class Gl2Boundary(C.Structure):
    """lw_gl2_boundary_t"""
    _fields_ = [("col", C.c_uint32), ("reserved", C.c_uint32), ("step", C.c_uint64), ("value", C.c_uint64), ("coeff", C.c_uint64 * 2)]


class Gl2Transition(C.Structure):
    """lw_gl2_transition_t"""
    _fields_ = [("period", C.c_uint64), ("offset", C.c_uint64), ("end_exemptions", C.c_uint64), ("exemptions_period", C.c_uint64),
                ("periodic_exemptions_offset", C.c_uint64), ("coeff", C.c_uint64 * 2)]


class Gl2RapBoundary(C.Structure):
    """lw_gl2_rap_boundary_t"""
    _fields_ = [("col", C.c_uint32), ("is_aux", C.c_uint32), ("step", C.c_uint64), ("value", C.c_uint64 * 2), ("coeff", C.c_uint64 * 2)]


class Bb4RapBoundary(C.Structure):
    """lw_bb4_rap_boundary_t"""
    _fields_ = [("col", C.c_uint32), ("is_aux", C.c_uint32), ("step", C.c_uint64), ("value", C.c_uint32 * 4), ("coeff", C.c_uint32 * 4)]


class Bb4Boundary(C.Structure):
    """lw_bb4_boundary_t"""
    _fields_ = [("col", C.c_uint32), ("reserved", C.c_uint32), ("step", C.c_uint64), ("value", C.c_uint32), ("coeff", C.c_uint32 * 4),
                ("reserved2", C.c_uint32)]


class Bb4Transition(C.Structure):
    """lw_bb4_transition_t"""
    _fields_ = [("period", C.c_uint64), ("offset", C.c_uint64), ("end_exemptions", C.c_uint64), ("exemptions_period", C.c_uint64),
                ("periodic_exemptions_offset", C.c_uint64), ("coeff", C.c_uint32 * 4)]


class M31qBoundary(C.Structure):
    """lw_m31q_boundary_t"""
    _fields_ = [("col", C.c_uint32), ("reserved", C.c_uint32), ("step", C.c_uint64), ("value", C.c_uint32), ("coeff", C.c_uint32 * 4),
                ("reserved2", C.c_uint32)]


class M31qTransition(C.Structure):
    """lw_m31q_transition_t"""
    _fields_ = [("period", C.c_uint64), ("offset", C.c_uint64), ("end_exemptions", C.c_uint64), ("coeff", C.c_uint32 * 4)]


class StarkAirOp(C.Structure):
    """lw_stark_air_op_t"""
    _fields_ = [("op", C.c_uint8), ("src", C.c_uint8), ("index", C.c_uint16), ("row", C.c_uint32)]


class Profile(C.Structure):
    _fields_ = [("n", C.c_int), ("k", KernelTime * 32)]


_lib = None


def lib():
    """Load liblw_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). lambda_elliptic_curves_amd has no CPU fallback.")
    # torch ships its own libamdhip64.so.7; two HIP runtimes in one process cannot both own the GPU.
    # Importing torch first makes the loader bind liblw_hip.so to the runtime torch already loaded (same
    # SONAME), so device pointers and streams are shared with torch (memory/stream plumbing only).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, sz, u32, u64p, i = C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint64), C.c_int
    L.lw_hip_init.argtypes = [C.POINTER(C.c_int), i]
    L.lw_hip_init.restype = i
    L.lw_hip_shutdown.restype = None
    L.lw_hip_device_count.restype = i
    L.lw_hip_last_error.restype = C.c_char_p
    L.lw_hip_get_timings.argtypes = [C.POINTER(Timings)]
    L.lw_hip_profile_begin.restype = i
    L.lw_hip_profile_end.argtypes = [C.POINTER(Profile)]
    L.lw_hip_profile_end.restype = i
    L.lw_hip_result_acquire.argtypes = [sz, C.POINTER(vp)]
    L.lw_hip_result_acquire.restype = i
    L.lw_hip_result_release.argtypes = [vp]
    L.lw_hip_result_release.restype = i
    L.lw_hip_field_elem_bytes.argtypes = [i, i]
    L.lw_hip_field_elem_bytes.restype = sz
    L.lw_hip_curve_point_bytes.argtypes = [i]
    L.lw_hip_curve_point_bytes.restype = sz
    L.lw_hip_ntt.argtypes = [i, i, i, vp, vp, u32, u32, sz, vp]
    L.lw_hip_ntt.restype = i
    L.lw_hip_ntt_device.argtypes = [i, i, i, vp, vp, u32, u32, sz, vp, vp]
    L.lw_hip_ntt_device.restype = i
    L.lw_hip_ntt_cross_device.argtypes = [i, i, i, vp, vp, u32, u32, C.c_uint64, C.c_uint64, C.c_uint64, u32, C.c_uint64, vp]
    L.lw_hip_ntt_cross_device.restype = i
    L.lw_hip_ntt_lde_device.argtypes = [i, i, vp, u32, vp, u32, u32, vp, vp]
    L.lw_hip_ntt_lde_device.restype = i
    L.lw_hip_gen_twiddles.argtypes = [i, i, C.c_uint64, i, vp]
    L.lw_hip_gen_twiddles.restype = i
    L.lw_hip_gen_powers.argtypes = [i, i, C.c_uint64, sz, i, vp, vp, C.POINTER(sz)]
    L.lw_hip_gen_powers.restype = i
    L.lw_hip_bitrev_permutation.argtypes = [i, i, vp, vp, sz]
    L.lw_hip_bitrev_permutation.restype = i
    L.lw_polynomial_evaluate_fft.argtypes = [i, i, vp, sz, sz, sz, vp, vp, sz, C.POINTER(sz)]
    L.lw_polynomial_evaluate_fft.restype = i
    L.lw_polynomial_interpolate_fft.argtypes = [i, i, vp, sz, vp, vp, C.POINTER(sz)]
    L.lw_polynomial_interpolate_fft.restype = i
    L.lw_hip_msm.argtypes = [i, vp, sz, vp, sz, vp]
    L.lw_hip_msm.restype = i
    L.lw_hip_msm_device.argtypes = [i, vp, vp, sz, vp, vp]
    L.lw_hip_msm_device.restype = i
    L.lw_stark_commit_columns.argtypes = [i, vp, u32, u32, i, vp, vp]
    L.lw_stark_commit_columns.restype = i
    L.lw_stark_commit_columns_device.argtypes = [i, vp, u32, C.c_uint64, u32, i, vp, vp, vp]
    L.lw_stark_commit_columns_device.restype = i
    L.lw_stark_commit_columns_layout_device.argtypes = [i, i, vp, u32, C.c_uint64, u32, i, vp, vp, vp]
    L.lw_stark_commit_columns_layout_device.restype = i
    L.lw_stark_fri_layer.argtypes = [i, vp, sz, vp, vp, sz, vp, C.POINTER(sz), vp, vp, vp]
    L.lw_stark_fri_layer.restype = i
    L.lw_groth16_h_coefficients.argtypes = [vp, vp, vp, sz, sz, vp, C.POINTER(sz)]
    L.lw_groth16_h_coefficients.restype = i
    L.lw_hip_msm_fr.argtypes = [i, vp, sz, vp, sz, vp]
    L.lw_hip_msm_fr.restype = i
    L.lw_hip_msm_fr_device.argtypes = [i, vp, vp, sz, vp, vp]
    L.lw_hip_msm_fr_device.restype = i
    L.lw_hip_msm_limbs.argtypes = [i, vp, u32, sz, vp, sz, vp]
    L.lw_hip_msm_limbs.restype = i
    L.lw_hip_msm_limbs_device.argtypes = [i, vp, u32, vp, sz, vp, vp]
    L.lw_hip_msm_limbs_device.restype = i
    L.lw_hip_srs_create.argtypes = [i, vp, sz, C.POINTER(vp)]
    L.lw_hip_srs_create.restype = i
    L.lw_hip_srs_create_device.argtypes = [i, vp, sz, vp, C.POINTER(vp)]
    L.lw_hip_srs_create_device.restype = i
    L.lw_hip_srs_destroy.argtypes = [vp]
    L.lw_hip_srs_destroy.restype = i
    L.lw_hip_msm_srs.argtypes = [vp, vp, sz, vp]
    L.lw_hip_msm_srs.restype = i
    L.lw_hip_msm_srs_fr.argtypes = [vp, vp, sz, vp]
    L.lw_hip_msm_srs_fr.restype = i
    L.lw_hip_msm_srs_device.argtypes = [vp, vp, sz, vp, vp]
    L.lw_hip_msm_srs_device.restype = i
    L.lw_hip_msm_srs_fr_device.argtypes = [vp, vp, sz, vp, vp]
    L.lw_hip_msm_srs_fr_device.restype = i
    L.lw_stark_fri_layer_device.argtypes = [i, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp]
    L.lw_stark_fri_layer_device.restype = i
    L.lw_groth16_h_coefficients_device.argtypes = [vp, vp, vp, sz, sz, vp, C.POINTER(sz), vp]
    L.lw_groth16_h_coefficients_device.restype = i
    L.lw_hip_ec_add_outer_device.argtypes = [i, vp, sz, vp, sz, vp, vp]
    L.lw_hip_ec_add_outer_device.restype = i
    L.lw_hip_ec_pointwise_device.argtypes = [i, i, i, vp, vp, sz, vp, vp]
    L.lw_hip_ec_pointwise_device.restype = i
    L.lw_hip_field_pointwise_device.argtypes = [i, i, vp, vp, sz, vp, vp]
    L.lw_hip_field_pointwise_device.restype = i
    L.lw_hip_comm_unique_id.argtypes = [vp]
    L.lw_hip_comm_unique_id.restype = i
    L.lw_hip_comm_init.argtypes = [vp, i, i]
    L.lw_hip_comm_init.restype = i
    L.lw_hip_comm_shutdown.restype = i
    L.lw_hip_comm_info.argtypes = [C.POINTER(i), C.POINTER(i)]
    L.lw_hip_comm_info.restype = i
    L.lw_hip_ntt_sharded_device.argtypes = [i, i, i, vp, vp, u32, u32, i, vp]
    L.lw_hip_ntt_sharded_device.restype = i
    L.lw_hip_ntt_sharded_selftest_device.argtypes = [i, i, i, vp, vp, u32, u32, u32, i, vp]
    L.lw_hip_ntt_sharded_selftest_device.restype = i
    L.lw_hip_ntt_sharded_selftest_steps_device.argtypes = [i, i, i, vp, vp, u32, u32, u32, i, i, vp]
    L.lw_hip_ntt_sharded_selftest_steps_device.restype = i
    L.lw_hip_msm_sharded_device.argtypes = [i, vp, vp, sz, vp, vp]
    L.lw_hip_msm_sharded_device.restype = i
    L.lw_hip_msm_sharded_selftest_device.argtypes = [i, vp, vp, sz, u32, vp, vp]
    L.lw_hip_msm_sharded_selftest_device.restype = i
    L.lw_poly_evaluate.argtypes = [i, vp, vp, u32, vp, u32, vp]
    L.lw_poly_evaluate.restype = i
    L.lw_poly_evaluate_device.argtypes = [i, vp, vp, u32, vp, u32, vp, vp]
    L.lw_poly_evaluate_device.restype = i
    L.lw_poly_ruffini_division.argtypes = [i, vp, sz, vp, vp, vp]
    L.lw_poly_ruffini_division.restype = i
    L.lw_poly_ruffini_division_device.argtypes = [i, vp, sz, vp, vp, vp, vp]
    L.lw_poly_ruffini_division_device.restype = i
    L.lw_kzg_open.argtypes = [vp, vp, sz, vp, vp, vp]
    L.lw_kzg_open.restype = i
    L.lw_kzg_open_device.argtypes = [vp, vp, sz, vp, vp, vp, vp]
    L.lw_kzg_open_device.restype = i
    L.lw_kzg_open_batch.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp]
    L.lw_kzg_open_batch.restype = i
    L.lw_kzg_open_batch_device.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp]
    L.lw_kzg_open_batch_device.restype = i
    L.lw_stark_deep_composition.argtypes = [i, vp, vp, u32, vp, u32, vp, vp, C.POINTER(sz), vp]
    L.lw_stark_deep_composition.restype = i
    L.lw_stark_deep_composition_device.argtypes = [i, vp, vp, u32, vp, u32, vp, vp, C.POINTER(sz), vp, vp]
    L.lw_stark_deep_composition_device.restype = i
    L.lw_plonk_circuit_create.argtypes = [i, sz, vp, vp, vp, vp, C.POINTER(vp)]
    L.lw_plonk_circuit_create.restype = i
    L.lw_plonk_circuit_destroy.argtypes = [vp]
    L.lw_plonk_circuit_destroy.restype = i
    L.lw_plonk_round1.argtypes = [vp, vp, vp, vp]
    L.lw_plonk_round1.restype = i
    L.lw_plonk_round1_device.argtypes = [vp, vp, vp, vp, vp]
    L.lw_plonk_round1_device.restype = i
    L.lw_plonk_round2.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.lw_plonk_round2.restype = i
    L.lw_plonk_round2_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.lw_plonk_round2_device.restype = i
    L.lw_plonk_round3.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp, vp, vp]
    L.lw_plonk_round3.restype = i
    L.lw_plonk_round3_device.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp]
    L.lw_plonk_round3_device.restype = i
    L.lw_stark_grinding_window.argtypes = [u32]
    L.lw_stark_grinding_window.restype = C.c_uint64
    L.lw_stark_grinding_nonce.argtypes = [vp, u32, C.c_uint64, C.c_uint64, u64p, C.POINTER(i)]
    L.lw_stark_grinding_nonce.restype = i
    L.lw_stark_grinding_nonce_device.argtypes = [vp, u32, C.c_uint64, C.c_uint64, u64p, C.POINTER(i), vp]
    L.lw_stark_grinding_nonce_device.restype = i
    L.lw_stark_open_trees_device.argtypes = [C.POINTER(StarkTree), u32, u64p, u32, vp, vp, vp]
    L.lw_stark_open_trees_device.restype = i
    L.lw_poseidon_permute.argtypes = [vp, sz, vp]
    L.lw_poseidon_permute.restype = i
    L.lw_poseidon_permute_device.argtypes = [vp, sz, vp, vp]
    L.lw_poseidon_permute_device.restype = i
    L.lw_poseidon_hash.argtypes = [vp, vp, sz, vp]
    L.lw_poseidon_hash.restype = i
    L.lw_poseidon_hash_device.argtypes = [vp, vp, sz, vp, vp]
    L.lw_poseidon_hash_device.restype = i
    L.lw_poseidon_hash_single.argtypes = [vp, sz, vp]
    L.lw_poseidon_hash_single.restype = i
    L.lw_poseidon_hash_single_device.argtypes = [vp, sz, vp, vp]
    L.lw_poseidon_hash_single_device.restype = i
    L.lw_poseidon_hash_many.argtypes = [vp, sz, sz, vp]
    L.lw_poseidon_hash_many.restype = i
    L.lw_poseidon_hash_many_device.argtypes = [vp, sz, sz, vp, vp]
    L.lw_poseidon_hash_many_device.restype = i
    L.lw_poseidon_commit_columns.argtypes = [vp, u32, u32, i, i, vp, vp]
    L.lw_poseidon_commit_columns.restype = i
    L.lw_poseidon_commit_columns_device.argtypes = [vp, u32, C.c_uint64, u32, i, i, vp, vp, vp]
    L.lw_poseidon_commit_columns_device.restype = i
    L.lw_pedersen_hash.argtypes = [vp, vp, sz, vp]
    L.lw_pedersen_hash.restype = i
    L.lw_pedersen_hash_device.argtypes = [vp, vp, sz, vp, vp]
    L.lw_pedersen_hash_device.restype = i
    L.lw_pedersen_commit_leaves.argtypes = [vp, u32, u32, i, vp, vp]
    L.lw_pedersen_commit_leaves.restype = i
    L.lw_pedersen_commit_leaves_device.argtypes = [vp, u32, u32, i, vp, vp, vp]
    L.lw_pedersen_commit_leaves_device.restype = i
    L.lw_pedersen_table.argtypes = [vp]
    L.lw_pedersen_table.restype = i
    L.lw_pedersen_add_affine_device.argtypes = [vp, vp, vp, sz, vp, vp]
    L.lw_pedersen_add_affine_device.restype = i
    for name in ("lw_circle_evaluate_cfft", "lw_circle_interpolate_cfft"):
        getattr(L, name).argtypes = [vp, vp, u32, u32, sz]
        getattr(L, name).restype = i
    for name in ("lw_circle_evaluate_cfft_device", "lw_circle_interpolate_cfft_device"):
        getattr(L, name).argtypes = [vp, vp, u32, u32, sz, vp]
        getattr(L, name).restype = i
    L.lw_circle_lde_device.argtypes = [vp, u32, sz, vp, u32, sz, u32, vp]
    L.lw_circle_lde_device.restype = i
    L.lw_circle_get_twiddles.argtypes = [u32, i, vp]
    L.lw_circle_get_twiddles.restype = i
    L.lw_goldilocks_ntt.argtypes = [i, vp, vp, u32, u32, sz, vp, C.c_uint64]
    L.lw_goldilocks_ntt.restype = i
    L.lw_goldilocks_ntt_device.argtypes = [i, vp, vp, u32, u32, sz, vp, C.c_uint64, vp]
    L.lw_goldilocks_ntt_device.restype = i
    L.lw_goldilocks_lde_device.argtypes = [vp, u32, sz, vp, u32, sz, u32, vp, C.c_uint64, vp]
    L.lw_goldilocks_lde_device.restype = i
    L.lw_goldilocks_gen_twiddles.argtypes = [C.c_uint64, i, C.c_uint64, vp]
    L.lw_goldilocks_gen_twiddles.restype = i
    L.lw_goldilocks_mul_device.argtypes = [vp, vp, vp, sz, vp]
    L.lw_goldilocks_mul_device.restype = i
    L.lw_goldilocks_ext2_pointwise_device.argtypes = [i, vp, sz, vp, sz, vp, sz, sz, vp]
    L.lw_goldilocks_ext2_pointwise_device.restype = i
    L.lw_goldilocks_ext2_evaluate_device.argtypes = [vp, u32, sz, sz, vp, u32, vp, vp]
    L.lw_goldilocks_ext2_evaluate_device.restype = i
    L.lw_goldilocks_ext2_deep_quotients_device.argtypes = [vp, u32, sz, u32, vp, C.c_uint64, vp, u32, vp, vp, vp, sz, vp]
    L.lw_goldilocks_ext2_deep_quotients_device.restype = i
    L.lw_goldilocks_ext2_fri_layer_device.argtypes = [vp, sz, sz, vp, vp, sz, C.c_uint64, i, vp, vp, vp, vp, vp]
    L.lw_goldilocks_ext2_fri_layer_device.restype = i
    L.lw_babybear_ext4_pointwise_device.argtypes = [i, vp, sz, vp, sz, vp, sz, sz, vp]
    L.lw_babybear_ext4_pointwise_device.restype = i
    L.lw_babybear_ext4_convert_device.argtypes = [i, vp, vp, sz, sz, vp]
    L.lw_babybear_ext4_convert_device.restype = i
    L.lw_babybear_ext4_evaluate_device.argtypes = [vp, u32, sz, sz, vp, u32, vp, vp]
    L.lw_babybear_ext4_evaluate_device.restype = i
    L.lw_babybear_ext4_deep_quotients_device.argtypes = [vp, u32, sz, u32, vp, vp, u32, vp, vp, vp, sz, vp]
    L.lw_babybear_ext4_deep_quotients_device.restype = i
    L.lw_babybear_ext4_fri_layer_device.argtypes = [vp, sz, sz, vp, vp, sz, vp, vp, vp, vp, vp]
    L.lw_babybear_ext4_fri_layer_device.restype = i
    aop, u32q, szp = C.POINTER(StarkAirOp), C.POINTER(u32), C.POINTER(sz)
    L.lw_goldilocks_ext2_constraint_evaluations_device.argtypes = [aop, u32, vp, u32, vp, u32q, u32, u32, u32, vp, C.c_uint64, C.POINTER(Gl2Boundary), u32,
                                                                   C.POINTER(Gl2Transition), u32, vp, sz, vp]
    L.lw_goldilocks_ext2_constraint_evaluations_device.restype = i
    L.lw_goldilocks_ext2_composition_parts_device.argtypes = [vp, sz, u32, vp, C.c_uint64, u32, vp, vp, szp, vp]
    L.lw_goldilocks_ext2_composition_parts_device.restype = i
    L.lw_babybear_ext4_constraint_evaluations_device.argtypes = [aop, u32, vp, u32, vp, u32q, u32, u32, u32, vp, C.POINTER(Bb4Boundary), u32,
                                                                 C.POINTER(Bb4Transition), u32, vp, sz, vp]
    L.lw_babybear_ext4_constraint_evaluations_device.restype = i
    L.lw_babybear_ext4_composition_parts_device.argtypes = [vp, sz, u32, vp, u32, vp, vp, szp, vp]
    L.lw_babybear_ext4_composition_parts_device.restype = i
    for name in ("lw_goldilocks_ext2_aux_fractions_device", "lw_babybear_ext4_aux_fractions_device"):
        getattr(L, name).argtypes = [vp, u32, sz, vp, u32q, vp, u32, vp, u32q, vp, u32, u32, vp, sz, vp, C.POINTER(C.c_uint64), vp]
        getattr(L, name).restype = i
    L.lw_goldilocks_ext2_rap_constraint_evaluations_device.argtypes = [aop, u32, vp, u32, vp, u32, vp, u32q, u32, vp, u32, sz, u32, u32, vp, C.c_uint64,
                                                                       C.POINTER(Gl2RapBoundary), u32, C.POINTER(Gl2Transition), u32, vp, sz, vp]
    L.lw_goldilocks_ext2_rap_constraint_evaluations_device.restype = i
    L.lw_babybear_ext4_rap_constraint_evaluations_device.argtypes = [aop, u32, vp, u32, vp, u32, vp, u32q, u32, vp, u32, sz, u32, u32, vp,
                                                                     C.POINTER(Bb4RapBoundary), u32, C.POINTER(Bb4Transition), u32, vp, sz, vp]
    L.lw_babybear_ext4_rap_constraint_evaluations_device.restype = i
    L.lw_rpo_permute.argtypes = [i, vp, sz, vp]
    L.lw_rpo_permute.restype = i
    L.lw_rpo_permute_device.argtypes = [i, vp, sz, vp, vp]
    L.lw_rpo_permute_device.restype = i
    L.lw_rpo_hash.argtypes = [i, vp, sz, sz, vp]
    L.lw_rpo_hash.restype = i
    L.lw_rpo_hash_device.argtypes = [i, vp, sz, sz, sz, vp, vp]
    L.lw_rpo_hash_device.restype = i
    L.lw_rpo_commit_columns.argtypes = [i, vp, u32, u32, i, vp, vp]
    L.lw_rpo_commit_columns.restype = i
    L.lw_rpo_commit_columns_device.argtypes = [i, vp, u32, C.c_uint64, u32, i, vp, vp, vp]
    L.lw_rpo_commit_columns_device.restype = i
    L.lw_monolith_permute.argtypes = [u32, u32, vp, sz, vp]
    L.lw_monolith_permute.restype = i
    L.lw_monolith_permute_device.argtypes = [u32, u32, vp, sz, vp, vp]
    L.lw_monolith_permute_device.restype = i
    L.lw_monolith_hash.argtypes = [u32, vp, sz, sz, vp]
    L.lw_monolith_hash.restype = i
    L.lw_monolith_hash_device.argtypes = [u32, vp, sz, sz, sz, vp, vp]
    L.lw_monolith_hash_device.restype = i
    L.lw_monolith_compress.argtypes = [u32, vp, vp, sz, vp]
    L.lw_monolith_compress.restype = i
    L.lw_monolith_compress_device.argtypes = [u32, vp, vp, sz, vp, vp]
    L.lw_monolith_compress_device.restype = i
    L.lw_monolith_commit_columns.argtypes = [u32, vp, u32, u32, i, vp, vp]
    L.lw_monolith_commit_columns.restype = i
    L.lw_monolith_commit_columns_device.argtypes = [u32, vp, u32, C.c_uint64, u32, i, vp, vp, vp]
    L.lw_monolith_commit_columns_device.restype = i
    L.lw_monolith_constants.argtypes = [u32, u32, vp, vp]
    L.lw_monolith_constants.restype = i
    L.lw_monolith_layer_device.argtypes = [u32, u32, i, vp, sz, vp, vp]
    L.lw_monolith_layer_device.restype = i
    L.lw_mersenne31_ext4_pointwise_device.argtypes = [i, vp, sz, vp, sz, vp, sz, sz, vp]
    L.lw_mersenne31_ext4_pointwise_device.restype = i
    L.lw_mersenne31_ext4_evaluate_device.argtypes = [vp, u32, sz, u32, vp, u32, vp, vp]
    L.lw_mersenne31_ext4_evaluate_device.restype = i
    L.lw_mersenne31_ext4_deep_quotients_device.argtypes = [vp, u32, sz, u32, vp, u32, vp, vp, vp, sz, vp]
    L.lw_mersenne31_ext4_deep_quotients_device.restype = i
    L.lw_mersenne31_ext4_fri_layer_device.argtypes = [vp, sz, u32, vp, i, vp, sz, u32, vp, vp, vp, vp]
    L.lw_mersenne31_ext4_fri_layer_device.restype = i
    L.lw_mersenne31_ext4_constraint_evaluations_device.argtypes = [aop, u32, vp, u32, vp, u32q, u32, u32, u32, C.POINTER(M31qBoundary), u32,
                                                                   C.POINTER(M31qTransition), u32, vp, sz, vp]
    L.lw_mersenne31_ext4_constraint_evaluations_device.restype = i
    L.lw_mersenne31_ext4_composition_parts_device.argtypes = [vp, sz, u32, u32, u32, vp, vp, C.POINTER(C.c_uint64), vp]
    L.lw_mersenne31_ext4_composition_parts_device.restype = i
    L.lw_field_batch_inverse.argtypes = [i, vp, sz, vp]
    L.lw_field_batch_inverse.restype = i
    L.lw_field_batch_inverse_device.argtypes = [i, vp, sz, vp, vp]
    L.lw_field_batch_inverse_device.restype = i
    L.lw_field_batch_inverse_block.argtypes = []
    L.lw_field_batch_inverse_block.restype = C.c_uint64
    bp, tp = C.POINTER(StarkBoundary), C.POINTER(StarkTransition)
    L.lw_stark_constraint_evaluations_device.argtypes = [i, vp, u32, u32, u32, vp, bp, u32, tp, u32, vp, C.c_uint64, vp, vp]
    L.lw_stark_constraint_evaluations_device.restype = i
    L.lw_stark_composition_parts_device.argtypes = [i, vp, u32, vp, u32, vp, vp, C.POINTER(sz), vp]
    L.lw_stark_composition_parts_device.restype = i
    L.lw_stark_commit_composition_device.argtypes = [i, vp, u32, C.c_uint64, u32, vp, vp, vp]
    L.lw_stark_commit_composition_device.restype = i
    L.lw_stark_round2.argtypes = [i, vp, u32, u32, u32, vp, bp, u32, tp, u32, vp, u32, vp, C.POINTER(sz), vp, vp, vp]
    L.lw_stark_round2.restype = i
    ap, u32p = C.POINTER(StarkAirOp), C.POINTER(u32)
    L.lw_stark_transition_evaluations_device.argtypes = [i, ap, u32, vp, u32, vp, u32p, u32, u32, u32, u32, vp, C.c_uint64, vp]
    L.lw_stark_transition_evaluations_device.restype = i
    L.lw_stark_transition_evaluations.argtypes = [i, ap, u32, vp, u32, vp, u32p, u32, u32, u32, u32, vp]
    L.lw_stark_transition_evaluations.restype = i
    L.lw_multilinear_evaluate.argtypes = [i, vp, u32, u32, vp, vp]
    L.lw_multilinear_evaluate.restype = i
    L.lw_multilinear_evaluate_device.argtypes = [i, vp, u32, u32, vp, vp, vp]
    L.lw_multilinear_evaluate_device.restype = i
    L.lw_multilinear_fix_variables.argtypes = [i, vp, u32, vp, u32, vp]
    L.lw_multilinear_fix_variables.restype = i
    L.lw_multilinear_fix_variables_device.argtypes = [i, vp, u32, vp, u32, vp, vp]
    L.lw_multilinear_fix_variables_device.restype = i
    L.lw_sumcheck_round.argtypes = [i, vp, u32, u32, vp, vp]
    L.lw_sumcheck_round.restype = i
    L.lw_sumcheck_round_device.argtypes = [i, vp, u32, u32, vp, vp, vp]
    L.lw_sumcheck_round_device.restype = i
    L.lw_multilinear_eq_table.argtypes = [i, vp, u32, vp]
    L.lw_multilinear_eq_table.restype = i
    L.lw_multilinear_eq_table_device.argtypes = [i, vp, u32, vp, vp]
    L.lw_multilinear_eq_table_device.restype = i
    L.lw_sumcheck_terms_round.argtypes = [i, vp, u32, vp, vp, vp, u32, u32, vp, vp]
    L.lw_sumcheck_terms_round.restype = i
    L.lw_sumcheck_terms_round_device.argtypes = [i, vp, u32, vp, vp, vp, u32, u32, vp, vp, vp]
    L.lw_sumcheck_terms_round_device.restype = i
    L.lw_r1cs_create.argtypes = [i, u32, u32, vp, vp, vp, C.POINTER(vp)]
    L.lw_r1cs_create.restype = i
    L.lw_r1cs_destroy.argtypes = [vp]
    L.lw_r1cs_destroy.restype = i
    L.lw_r1cs_split_length.argtypes = []
    L.lw_r1cs_split_length.restype = u32
    L.lw_r1cs_lazy_terms.argtypes = []
    L.lw_r1cs_lazy_terms.restype = u32
    L.lw_r1cs_matvec.argtypes = [vp, vp, sz, vp, vp, vp]
    L.lw_r1cs_matvec.restype = i
    L.lw_r1cs_matvec_device.argtypes = [vp, vp, sz, vp, vp, vp, vp]
    L.lw_r1cs_matvec_device.restype = i
    L.lw_r1cs_bind_rows.argtypes = [vp, vp, vp, sz, vp]
    L.lw_r1cs_bind_rows.restype = i
    L.lw_r1cs_bind_rows_device.argtypes = [vp, vp, vp, sz, vp, vp]
    L.lw_r1cs_bind_rows_device.restype = i
    L.lw_r1cs_first_unsatisfied.argtypes = [vp, vp, C.POINTER(C.c_int64)]
    L.lw_r1cs_first_unsatisfied.restype = i
    L.lw_r1cs_first_unsatisfied_device.argtypes = [vp, vp, C.POINTER(C.c_int64), vp]
    L.lw_r1cs_first_unsatisfied_device.restype = i
    L.lw_groth16_h_from_witness.argtypes = [vp, vp, sz, vp, C.POINTER(sz)]
    L.lw_groth16_h_from_witness.restype = i
    L.lw_groth16_h_from_witness_device.argtypes = [vp, vp, sz, vp, C.POINTER(sz), vp]
    L.lw_groth16_h_from_witness_device.restype = i
    _lib = L
    return L


def profile_begin():
    rc = lib().lw_hip_profile_begin()
    if rc:
        raise RuntimeError(f"lw_hip_profile_begin: [{rc}] {last_error()}")


def profile_end():
    """-> {kernel name: (launches, total_ms)} measured with HIP events on the launch stream."""
    p = Profile()
    rc = lib().lw_hip_profile_end(C.byref(p))
    if rc:
        raise RuntimeError(f"lw_hip_profile_end: [{rc}] {last_error()}")
    return {p.k[j].name.decode(): (int(p.k[j].launches), float(p.k[j].total_ms)) for j in range(p.n)}


def last_error():
    return lib().lw_hip_last_error().decode("utf-8", "replace")


# ---- argument helpers of the bindings that take both numpy arrays and torch tensors (poseidon.py, rpo.py)
def host_ptr(a):
    """numpy array -> void *; None or an empty array -> NULL"""
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def device_ptr(t):
    return C.c_void_p(t.data_ptr())


def stream_ptr(stream):
    """a hipStream_t as an integer, or None for torch's current stream"""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    return C.c_void_p(stream)
