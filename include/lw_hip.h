/*
 * lw_hip.h — C ABI of the MI355X (gfx950) NTT + MSM backend for lambdaworks.
 *
 * This is the drop-in boundary for the reference's data-parallel prover hot path.  Each entry point cites
 * the reference interface it replaces (paths relative to the lambdaworks tree, v0.11.0):
 *
 *   - lw_hip_ntt / lw_hip_ntt_device        <->  evaluate_fft_cuda / interpolate_fft_cuda
 *                                                (math/src/fft/gpu/cuda/polynomial.rs:16-49), i.e. the backend arm
 *                                                of Polynomial::evaluate_fft / interpolate_fft
 *                                                (math/src/fft/polynomial.rs:54-62,103-110)
 *   - lw_polynomial_evaluate_fft            <->  Polynomial::evaluate_fft / evaluate_offset_fft
 *                                                (math/src/fft/polynomial.rs:25-68,74-82)
 *   - lw_polynomial_interpolate_fft         <->  Polynomial::interpolate_fft / interpolate_offset_fft
 *                                                (math/src/fft/polynomial.rs:87-127)
 *   - lw_hip_gen_twiddles                   <->  gen_twiddles (math/src/fft/gpu/cuda/ops.rs:45-66), get_twiddles
 *                                                (math/src/fft/cpu/roots_of_unity.rs:66-75)
 *   - lw_hip_bitrev_permutation             <->  bitrev_permutation (math/src/fft/gpu/cuda/ops.rs:68-77),
 *                                                in_place_bit_reverse_permute (math/src/fft/cpu/bit_reversing.rs:2-9)
 *   - lw_hip_msm / lw_hip_msm_device        <->  msm::pippenger::msm (math/src/msm/pippenger.rs:18-32)
 *   - lw_hip_msm_limbs[_device]             <->  the same for UnsignedInteger<NUM_LIMBS>, NUM_LIMBS = 1 .. 8
 *   - lw_circle_evaluate_cfft / interpolate <->  evaluate_cfft / interpolate_cfft (math/src/circle/polynomial.rs:18-72),
 *     lw_circle_get_twiddles                     get_twiddles (math/src/circle/twiddles.rs:13-58), over Mersenne31
 *   - lw_goldilocks_ntt[_device]            <->  the same backend arm of Polynomial::evaluate_fft / interpolate_fft and their
 *     lw_goldilocks_lde_device                   offset forms (math/src/fft/polynomial.rs:25-127) over p = 2^64 - 2^32 + 1:
 *     lw_goldilocks_gen_twiddles                 U64TestField (math/src/field/test_fields/u64_test_field.rs:98-104) and
 *                                                Winterfell's Felt (math/src/field/fields/winterfell.rs:21-24)
 *   - lw_hip_init / lw_hip_shutdown         <->  CudaState::new (math/src/fft/gpu/cuda/state.rs:29-38); the
 *                                                reference builds and drops device state on every call, this
 *                                                library keeps one context (twiddle caches, scratch, streams)
 *   - error codes                           <->  FFTError (math/src/fft/errors.rs:12-20), MSMError
 *                                                (math/src/msm/naive.rs:7-9), CudaError
 *                                                (gpu/src/cuda/abstractions/errors.rs:3-21)
 *
 * Data crosses the boundary bit-for-bit as the reference keeps it in memory (no conversion, as
 * math/src/gpu/cuda/field/element.rs:30-42): a field element is UnsignedInteger{limbs:[u64;N]} with
 * limbs[0] MOST significant, in Montgomery form; a projective point is X,Y,Z consecutive; an Fp2
 * coordinate is [c0,c1]; MSM scalars are canonical (non-Montgomery) UnsignedInteger<4> (UnsignedInteger<1..8>
 * through lw_hip_msm_limbs).
 *
 * All functions return 0 on success or a negative lw_status_t; lw_hip_last_error() gives a thread-local
 * message.  No exceptions or panics cross the ABI.  The caller owns every buffer; nothing is retained.
 * There is NO CPU fallback: without a usable gfx950 device every compute entry point fails with
 * LW_ERR_NO_DEVICE.
 */
#ifndef LW_HIP_H
#define LW_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    LW_FIELD_STARK252 = 0,      /* field_name() == "stark256" (stark_252_prime_field.rs:26-28) */
    LW_FIELD_BLS12_381_FR = 1,  /* bls12_381/default_types.rs:25-30 */
    LW_FIELD_BABYBEAR = 2       /* field_name() == "babybear31" (babybear.rs:33-35, babybear_u32.rs:21-23) */
} lw_field_t;

typedef enum {
    LW_LAYOUT_U64_LIMBS_MS_FIRST = 0, /* MontgomeryBackendPrimeField<_,4>: 4 x u64, R = 2^256 */
    LW_LAYOUT_BABYBEAR_U32_R32 = 1,   /* U32MontgomeryBackendPrimeField: one u32, R = 2^32 (babybear_u32.rs:6) */
    LW_LAYOUT_BABYBEAR_U64_R64 = 2,   /* MontgomeryBackendPrimeField<_,1>: one u64, R = 2^64 (babybear.rs:19-20) */
    LW_LAYOUT_EXT4_INTERLEAVED = 3    /* Degree4BabyBearExtensionField values: 4 x u64 (R = 2^64) per element,
                                         domain in the base field (quartic_babybear.rs:16-19,155-166) */
} lw_layout_t;

typedef enum { LW_DIR_FORWARD = 0, LW_DIR_INVERSE = 1 /* scaled by N^-1 */ } lw_dir_t;

typedef enum {
    LW_CURVE_BLS12_381_G1 = 0, /* 3 x 6 u64 per point */
    LW_CURVE_BN254_G1 = 1,     /* 3 x 4 u64 */
    LW_CURVE_BN254_G2 = 2,     /* 3 x 2 x 4 u64 */
    LW_CURVE_BLS12_381_G2 = 3  /* 3 x 2 x 6 u64 */
} lw_curve_t;

typedef enum {
    LW_OK = 0,
    LW_ERR_INPUT_NOT_POW2 = -1,  /* FFTError::InputError */
    LW_ERR_ORDER_TOO_LARGE = -2, /* FFTError::OrderError */
    LW_ERR_ROOT_OF_UNITY = -3,   /* FFTError::RootOfUnityError / FieldError::RootOfUnityError */
    LW_ERR_LENGTH_MISMATCH = -4, /* MSMError::LengthMismatch */
    LW_ERR_NO_DEVICE = -5,       /* CudaError::DeviceNotFound */
    LW_ERR_ALLOC = -6,           /* CudaError::AllocateMemory */
    LW_ERR_LAUNCH = -7,          /* CudaError::Launch / FunctionError */
    LW_ERR_COMM = -8,            /* RCCL unavailable / no communicator / collective failed (multi-GPU entry points) */
    LW_ERR_BAD_ARG = -9,
    LW_ERR_INV_ZERO = -10        /* FieldError::InvZeroError (zero coset offset) */
} lw_status_t;

typedef struct {
    double last_ntt_ms;      /* host wall time of the last lw_hip_ntt* call */
    double last_msm_ms;
    uint64_t ntt_calls, msm_calls;
    uint64_t twiddle_bytes;  /* device bytes held by twiddle caches */
    uint64_t scratch_bytes;
} lw_timings_t;

/* Per-kernel device timing (HIP events recorded on the launch stream around every kernel this library
 * launches between begin and end).  Instrumentation only; the reference's analogue is the `instruments`
 * feature's per-round timers (provers/stark/src/prover.rs:884-1049). */
typedef struct {
    char name[48];
    uint64_t launches;
    double total_ms;
} lw_kernel_time_t;
typedef struct {
    int n;
    lw_kernel_time_t k[32];
} lw_profile_t;

/* ---- context ---- */
/* One context per process, bound to ONE device: NULL,0 -> the calling thread's current device; n_devices > 1 ->
 * LW_ERR_BAD_ARG (multi-GPU jobs run one process per GPU and shard through lw_hip_comm_init below).  Calling it again
 * with another device id releases every cached table / workspace of the old device first; destroy lw_srs_t handles
 * before doing that.  Every entry point binds the context's device for the calling thread for the duration of the call
 * (the HIP current device is per thread) and restores the caller's afterwards.
 *
 * Stream contract of the *_device entry points: work is enqueued on `hip_stream` and the call returns without waiting
 * for it, except where a result is handed back through a host pointer (the MSM's out_point_host, out_root): those
 * synchronise the stream before returning.
 *
 * Threads: the library keeps LW_LANES (4) independent sets of scratch, staging buffers, workspaces and side streams
 * ("lanes", csrc/context.h).  A call takes the first lane that is free, so calls from different host threads — the
 * reference's rayon loop over columns (provers/stark/src/trace.rs:186-190), an NTT caller beside an MSM caller — run
 * concurrently: one caller's download overlaps another's upload and kernels (host-buffer entry points run on their lane's
 * own stream).  More concurrent callers than lanes wait for a lane.  A single-threaded caller always gets lane 0 and sees
 * a one-context library; lanes allocate lazily, so memory grows only with the concurrency actually used.  Within a lane,
 * a call on a different stream than the lane's previous one first waits (hipStreamWaitEvent) for that call's work, so
 * calls may be issued from any stream or thread in any order.  The twiddle tables are shared by all lanes and rebuilt,
 * when a larger transform arrives, with every other call out of the library.  The multi-GPU entry points (one
 * communicator per process) always run on lane 0.  Callers that want column parallelism inside ONE call still pass
 * `batch`. */
int lw_hip_init(const int *device_ids, int n_devices);
void lw_hip_shutdown(void);
int lw_hip_device_count(void);
const char *lw_hip_last_error(void);
int lw_hip_get_timings(lw_timings_t *out);
int lw_hip_profile_begin(void);             /* start recording kernel events */
int lw_hip_profile_end(lw_profile_t *out);  /* synchronise, stop, report */
size_t lw_hip_field_elem_bytes(lw_field_t field, lw_layout_t layout);
size_t lw_hip_curve_point_bytes(lw_curve_t curve);

/* Result buffers for the host-buffer entry points.  Polynomial::evaluate_fft returns a NEW Vec on every call
 * (math/src/fft/polynomial.rs:37-38, fft/gpu/cuda/state.rs:61-68,197-202): a 512 MiB result that has never been touched costs
 * 131072 first-touch page faults when the device-to-host copy lands in it — several times the copy itself.  A caller that
 * can hold its result in a library buffer asks for one here: pinned, resident memory from a small pool (reused across
 * calls, released with lw_hip_result_release or at lw_hip_shutdown), into which lw_hip_ntt / lw_polynomial_evaluate_fft
 * copy at the PCIe rate.  Any other `out` pointer keeps working: large fresh buffers are populated (huge pages where the
 * host grants them) by helper threads while the upload and the kernels run, and downloaded chunk by chunk behind that. */
int lw_hip_result_acquire(size_t bytes, void **out_ptr);
int lw_hip_result_release(void *ptr);

/* ---- NTT backend seam ----
 * `in` holds `batch` transforms of 2^log2n elements, `batch_stride_elems` apart (0 -> dense).  Forward:
 * natural-order coefficients -> natural-order evaluations at w^i.  Inverse: evaluations -> coefficients,
 * already multiplied by N^-1.  coset_offset (one domain-field element in the same layout's base word, or
 * NULL): forward evaluates on offset*w^i, inverse divides the result by offset^i.  `in` may alias `out`.
 * log2n > TWO_ADICITY -> LW_ERR_ROOT_OF_UNITY; log2n > 63 -> LW_ERR_ORDER_TOO_LARGE. */
int lw_hip_ntt(lw_field_t field, lw_layout_t layout, lw_dir_t dir, const void *in, void *out, uint32_t log2n,
               uint32_t batch, size_t batch_stride_elems, const void *coset_offset_or_null);

/* Same, on device-resident buffers; `hip_stream` is a hipStream_t (NULL = default stream); asynchronous. */
int lw_hip_ntt_device(lw_field_t field, lw_layout_t layout, lw_dir_t dir, const void *d_in, void *d_out,
                      uint32_t log2n, uint32_t batch, size_t batch_stride_elems, const void *coset_offset_or_null,
                      void *hip_stream);

/* Low-degree extension on device buffers: the forward transform of 2^log2_coeffs coefficients (batch blocks, dense)
 * zero-padded to 2^log2n, i.e. Polynomial::evaluate_fft / evaluate_offset_fft with blowup_factor / domain_size
 * (math/src/fft/polynomial.rs:30-38) as the STARK prover calls it (provers/stark/src/prover.rs:150-167), without
 * materialising the padding: the log2n - log2_coeffs stages that would only replicate the block are skipped.
 * All fields and layouts (BASELINE config 4, the BabyBear STARK LDE, is this call with batch = 4); d_out must not alias
 * d_coeffs. */
int lw_hip_ntt_lde_device(lw_field_t field, lw_layout_t layout, const void *d_coeffs, uint32_t log2_coeffs, void *d_out,
                          uint32_t log2n, uint32_t batch, const void *coset_offset_or_null, void *hip_stream);

/* RootsConfig (math/src/field/traits.rs): 0 Natural, 1 NaturalInversed, 2 BitReverse, 3 BitReverseInversed.
 * Writes 2^order / 2 domain-field elements (host buffer, the layout's base word type).  order > 63 ->
 * LW_ERR_ORDER_TOO_LARGE; order > TWO_ADICITY -> LW_ERR_ROOT_OF_UNITY; order 0 -> nothing written. */
int lw_hip_gen_twiddles(lw_field_t field, lw_layout_t layout, uint64_t order, int config, void *out);
/* get_powers_of_primitive_root(order, count, config) and, with offset != NULL (config 0 only),
 * get_powers_of_primitive_root_coset(order, count, offset) (math/src/fft/cpu/roots_of_unity.rs:13-61): out[i] =
 * [offset *] w^(+-i), w the primitive 2^order-th root, as domain-field elements in the layout's base word (host
 * buffer).  The bit-reversed configurations return next_power_of_two(count) entries, bit-reverse permuted, as the
 * reference does; *out_len receives the number of entries (call with out == NULL to query it).  count 0 -> nothing.
 * order > TWO_ADICITY -> LW_ERR_ROOT_OF_UNITY. */
int lw_hip_gen_powers(lw_field_t field, lw_layout_t layout, uint64_t order, size_t count, int config, const void *offset_or_null,
                      void *out, size_t *out_len);
/* out[i] = in[bitrev(i)] over n = 2^k elements of the layout (host buffers, may alias). */
int lw_hip_bitrev_permutation(lw_field_t field, lw_layout_t layout, const void *in, void *out, size_t n);

/* Cross-shard step of the multi-GPU NTT (no reference counterpart: the reference has no multi-device path).
 * A 2^log2n_total vector is block-distributed over G = 2^log2_shards GPUs (M = N/G elements each).  After the
 * first all-to-all this rank holds x[j1][j2] for j1 = 0..G-1 and its slice j2 in [j2_begin, j2_begin+slice_len),
 * chunk j1 starting chunk_stride_elems*j1 elements into d_in.  Writes, with the same chunking over k1,
 *     y[k1][j2] = w_N^(j2*k1) * sum_j1 w_G^(j1*k1) * x[j1][j2]        (inverse: inverse roots, times G^-1).
 * The second all-to-all then gives rank k1 the row y[k1][0..M), whose local M-point NTT (lw_hip_ntt_device) is
 * X[k1 + G*k2].  See lambda_elliptic_curves_amd/distributed.py for the full exchange schedule. */
int lw_hip_ntt_cross_device(lw_field_t field, lw_layout_t layout, lw_dir_t dir, const void *d_in, void *d_out,
                            uint32_t log2n_total, uint32_t log2_shards, uint64_t j2_begin, uint64_t slice_len,
                            uint64_t chunk_stride_elems, uint32_t batch, uint64_t batch_stride_elems, void *hip_stream);

/* ---- Multi-GPU: one process per GPU, library-owned RCCL communicator over xGMI (no reference counterpart: the
 * reference has no multi-device path).  Rank 0 calls lw_hip_comm_unique_id and hands the 128 bytes to the other
 * processes out of band (exactly ncclGetUniqueId's contract); every process then calls lw_hip_comm_init (collective)
 * after lw_hip_init(&device, 1).  The communicator lives in the library context and is released by
 * lw_hip_comm_shutdown / lw_hip_shutdown.  nranks in {1, 2, 4, 8}.  Every failure of this path (RCCL not loadable,
 * no communicator, a failing collective) is LW_ERR_COMM. */
#define LW_HIP_COMM_ID_BYTES 128
int lw_hip_comm_unique_id(uint8_t *out_id /* LW_HIP_COMM_ID_BYTES */);
int lw_hip_comm_init(const uint8_t *unique_id, int rank, int nranks);
int lw_hip_comm_shutdown(void);
int lw_hip_comm_info(int *rank, int *nranks);

/* One transform of 2^log2n_total elements (or `batch` of them) block-distributed over the communicator's G ranks: this
 * rank holds elements [rank*M, (rank+1)*M) of the natural-order vector, M = 2^log2n_total / G; batch entries are M
 * elements apart (dense).  Collective: every rank calls it with the same arguments.  natural_output != 0: d_out_local
 * receives this rank's block of the natural-order result, i.e. the concatenation over ranks is byte-identical to
 * lw_hip_ntt_device on the concatenated input (Polynomial::evaluate_fft / interpolate_fft semantics);
 * natural_output == 0: the cyclic shard X[rank + G*k], k = 0..M-1 (one all-to-all fewer).  d_out_local may alias
 * d_in_local.  Schedule: all-to-all, cross-shard step (lw_hip_ntt_cross_device), all-to-all, local M-point NTT
 * [, all-to-all, interleave] — see csrc/comm.hip. */
int lw_hip_ntt_sharded_device(lw_field_t field, lw_layout_t layout, lw_dir_t dir, const void *d_in_local, void *d_out_local,
                              uint32_t log2n_total, uint32_t batch, int natural_output, void *hip_stream);
/* The same schedule with G = 2^log2_shards virtual ranks walked on ONE device (exchanges are device-to-device
 * copies): d_in_full / d_out_full hold the whole vectors (batch entries 2^log2n_total apart), virtual rank g owning
 * block g.  With natural_output == 0 block g of d_out_full receives X[g + G*k].  Used to parity-test the exchange
 * schedule on a one-GPU box; needs no communicator. */
int lw_hip_ntt_sharded_selftest_device(lw_field_t field, lw_layout_t layout, lw_dir_t dir, const void *d_in_full, void *d_out_full,
                                       uint32_t log2n_total, uint32_t log2_shards, uint32_t batch, int natural_output,
                                       void *hip_stream);
/* Self-test hook: the same run cut after step `stop_after` of the schedule (1 exchange A, 2 cross step, 3 exchange C,
 * 4 local NTT, 5 exchange E, 6 interleave): block g of d_out_full receives the batch x M elements virtual rank g holds at
 * that point.  tests/test_gpu_distributed.py checks the Python transliteration of the schedule
 * (lambda_elliptic_curves_amd/distributed.py, the one the world-size-2 gloo test drives) against it step by step. */
int lw_hip_ntt_sharded_selftest_steps_device(lw_field_t field, lw_layout_t layout, lw_dir_t dir, const void *d_in_full, void *d_out_full,
                                             uint32_t log2n_total, uint32_t log2_shards, uint32_t batch, int natural_output,
                                             int stop_after, void *hip_stream);
/* msm over pairs sharded across the ranks: every rank passes its n_local (scalar, point) pairs (n_local may differ per
 * rank, 0 allowed).  Schedule (csrc/comm.hip msm_sharded_run; the north star's "bucket all-reduce"): all ranks agree on the
 * window width from the largest shard; each accumulates its pairs into the full bucket array [W][2^(c-1)]; an all-to-all
 * hands rank g the bucket range g of every window from everyone (W x 2^(c-1) x point bytes per rank and MSM: 654 MB for
 * BN254 G1 at c = 20); rank g adds the G contributions and runs the running sums over its slice only, so the bucket reduce —
 * ~4.7 ms per MSM at c = 20 on one GPU, whatever N — costs 1/G per rank; an all-gather of 2 W points per rank carries the
 * per-slice sums and every rank folds the result.  Every rank receives the sum over all ranks' pairs, normalised like
 * lw_hip_msm. */
int lw_hip_msm_sharded_device(lw_curve_t curve, const uint64_t *d_scalars, const void *d_points, size_t n_local,
                              void *out_point_host, void *hip_stream);

/* The same run with G = 2^log2_shards virtual ranks walked on ONE device (virtual rank g owns the pairs [g n / G, (g+1) n / G));
 * parity-tests the exchange and the per-slice running sums on a one-GPU box, needs no communicator. */
int lw_hip_msm_sharded_selftest_device(lw_curve_t curve, const uint64_t *d_scalars, const void *d_points, size_t n_total,
                                       uint32_t log2_shards, void *out_point_host, void *hip_stream);

/* ---- Polynomial FFT API (host buffers, reference semantics) ----
 * evaluate: len = max(coeff_len, domain_size).next_power_of_two() * blowup_factor where coeff_len is
 * taken after stripping trailing zero coefficients (Polynomial::new); writes *out_len elements.  Call with
 * out == NULL to query *out_len.  Zero polynomial -> *out_len zeros.  Non-power-of-two len ->
 * LW_ERR_INPUT_NOT_POW2. */
int lw_polynomial_evaluate_fft(lw_field_t field, lw_layout_t layout, const void *coeffs, size_t n_coeffs,
                               size_t blowup_factor, size_t domain_size, const void *offset_or_null, void *out,
                               size_t out_capacity_elems, size_t *out_len);
/* interpolate: n must be a power of two; writes all n coefficients and reports in *coeff_len the length
 * after Polynomial::new would strip trailing zeros. */
int lw_polynomial_interpolate_fft(lw_field_t field, lw_layout_t layout, const void *evals, size_t n,
                                  const void *offset_or_null, void *out_coeffs, size_t *coeff_len);

/* ---- STARK commitment (SURVEY 8f "next" #1) ----
 * The commitment interpolate_and_commit_main makes right after the LDE (provers/stark/src/prover.rs:229-244): each of
 * the n_cols columns (2^log2n FieldElements, natural order, column-major) is bit-reverse permuted (bit_reverse != 0,
 * :232-234), rows are formed (columns2rows) and BatchedMerkleTree<BatchKeccak256Backend> is built
 * (crypto/src/merkle_tree/merkle.rs:31-56; field_element_vector.rs:41-58; utils.rs:44-72).  The permutation and the
 * transposition are folded into the leaf hash, nothing is copied.  nodes: (2*2^log2n - 1) x 32 bytes, root first,
 * leaves last — the reference's `nodes` vector.  n_cols = 1 is the FRI layer tree (Keccak256Backend).  col_stride_elems (both
 * _device forms): elements between column starts, 0 = dense, at least 2^log2n otherwise. */
int lw_stark_commit_columns(lw_field_t field, const void *columns, uint32_t n_cols, uint32_t log2n, int bit_reverse,
                            uint8_t *out_root /* 32 bytes */, uint8_t *out_nodes_or_null);
int lw_stark_commit_columns_device(lw_field_t field, const void *d_columns, uint32_t n_cols, uint64_t col_stride_elems,
                                   uint32_t log2n, int bit_reverse, void *d_nodes, uint8_t *out_root_or_null, void *hip_stream);

/* The same commitment for any layout whose elements have an AsBytes in the reference — in particular the BabyBear columns
 * of BASELINE config 4 (the STARK LDE): U32MontgomeryBackendPrimeField hashes value().to_be_bytes(), 4 bytes per element
 * (u32_montgomery_backend_prime_field.rs:258-262), the u64-limb BabyBear its one limb big-endian
 * (montgomery_backed_prime_fields.rs:367-373).  LW_LAYOUT_EXT4_INTERLEAVED is rejected (no AsBytes in the reference). */
int lw_stark_commit_columns_layout_device(lw_field_t field, lw_layout_t layout, const void *d_columns, uint32_t n_cols,
                                          uint64_t col_stride_elems, uint32_t log2n, int bit_reverse, void *d_nodes,
                                          uint8_t *out_root_or_null, void *hip_stream);

/* One layer of the FRI commit phase (SURVEY 8f "next" #4), the loop body of commit_phase
 * (provers/stark/src/fri/mod.rs:44-58): p' = 2 * fold_polynomial(p, zeta) (fri/fri_functions.rs:7-30), then
 * new_fri_layer(p', coset_offset, domain_size) (fri/mod.rs:115-141): evaluation on the coset, bit-reverse permuted,
 * Merkle tree over pairs of consecutive evaluations.  The caller (transcript owner) passes the already squared offset
 * and halved domain.  out_poly: ceil(n/2) coefficients (+ stripped length); out_evaluation: domain_size elements
 * (bit-reversed order, as FriLayer stores it); out_nodes: (domain_size - 1) x 32 bytes, root first. */
int lw_stark_fri_layer(lw_field_t field, const void *coeffs, size_t n_coeffs, const void *zeta, const void *coset_offset,
                       size_t domain_size, void *out_poly, size_t *out_poly_len, void *out_evaluation, uint8_t *out_root,
                       uint8_t *out_nodes_or_null);

/* The same layer with every large object resident in HBM (commit_phase's loop, provers/stark/src/fri/mod.rs:44-58, keeps
 * current_poly and the layers; only the challenge and the 32-byte root go through the transcript): d_coeffs holds
 * n_coeffs coefficients; d_out_poly receives p' as a zero-padded block of max(2, next_power_of_two(ceil(n_coeffs/2)))
 * coefficients — the next layer's d_coeffs (pass ceil(n_coeffs/2) or the block length, trailing zeros change nothing);
 * d_out_evaluation_or_null: domain_size elements, bit-reversed order; d_nodes_or_null: (domain_size - 1) x 32 bytes, root
 * first; out_root_or_null: host, 32 bytes (synchronises the stream when given).  zeta and coset_offset are host
 * pointers.  d_nodes_or_null == NULL: fold only — the last step of commit_phase (mod.rs:61-63), whose constant
 * coefficient is the value sent to the verifier; domain_size and coset_offset are then ignored. */
int lw_stark_fri_layer_device(lw_field_t field, const void *d_coeffs, size_t n_coeffs, const void *zeta, const void *coset_offset,
                              size_t domain_size, void *d_out_poly, void *d_out_evaluation_or_null, void *d_nodes_or_null,
                              uint8_t *out_root_or_null, void *hip_stream);

/* ---- Groth16 quotient (SURVEY 8f "next" #3) ----
 * QuadraticArithmeticProgram::calculate_h_coefficients (provers/groth16/src/qap.rs:15-39) once the variable
 * polynomials L, R, O have been accumulated: n_coeffs <= num_gates BLS12-381 FrElements each, num_gates a power of two.
 * Writes 2*num_gates coefficients of h (and the stripped length, as Polynomial::new would leave it). */
int lw_groth16_h_coefficients(const void *l_coeffs, const void *r_coeffs, const void *o_coeffs, size_t n_coeffs, size_t num_gates,
                              void *out_h, size_t *coeff_len);

/* Device-resident form: d_l / d_r / d_o hold n_coeffs FrElements each, d_out_h receives 2*num_gates coefficients (trailing
 * zeros included) and stays in HBM for the MSM that consumes it — Prover::prove feeds h straight into
 * msm(h.representative(), z_powers_of_tau_g1[..h.len()]) (provers/groth16/src/prover.rs:68-72,97-101), which is
 * lw_hip_msm_srs_fr_device on d_out_h.  coeff_len_or_null (host): the stripped length; asking for it synchronises. */
int lw_groth16_h_coefficients_device(const void *d_l, const void *d_r, const void *d_o, size_t n_coeffs, size_t num_gates, void *d_out_h,
                                     size_t *coeff_len_or_null, void *hip_stream);

/* ---- MSM ----
 * scalars: n x 4 u64, canonical integers, MS limb first (callers pass .representative()).
 * points: n projective points, not necessarily normalised (Z != 1 allowed), identity = (0:1:0).
 * out_point: one projective point (same layout); only its affine image is canonical. */
int lw_hip_msm(lw_curve_t curve, const uint64_t *scalars, size_t n_scalars, const void *points, size_t n_points,
               void *out_point);
int lw_hip_msm_device(lw_curve_t curve, const uint64_t *d_scalars, const void *d_points, size_t n,
                      void *out_point_host, void *hip_stream);
/* Same, but the scalars are FrElements of the curve's scalar field as they sit in memory (Montgomery form): the
 * `.representative()` map every reference caller runs on the CPU first (provers/groth16/src/prover.rs:69-78,
 * crypto/src/commitments/kzg.rs:159-163) is done on the device (SURVEY 8f "next" #2). */
int lw_hip_msm_fr(lw_curve_t curve, const uint64_t *fr_elements, size_t n_scalars, const void *points, size_t n_points,
                  void *out_point);
int lw_hip_msm_fr_device(lw_curve_t curve, const uint64_t *d_fr_elements, const void *d_points, size_t n,
                         void *out_point_host, void *hip_stream);
/* Same as lw_hip_msm / lw_hip_msm_device for scalars of any width from 1 to 8 u64 limbs, as the reference's Pippenger is
 * generic over it: msm<const NUM_LIMBS, G>(cs: &[UnsignedInteger<NUM_LIMBS>], ...) (math/src/msm/pippenger.rs:18-32).
 * scalars: n x scalar_limbs u64, each a canonical unsigned integer of 64 * scalar_limbs bits, MS limb first (as
 * UnsignedInteger<scalar_limbs> sits in memory).  The result is sum k_i * P_i over the FULL integers k_i: the scalars are
 * NOT reduced mod r (that would give the same element only inside the prime-order subgroup, and any curve point is
 * accepted).  Different lengths -> LW_ERR_LENGTH_MISMATCH (checked first); scalar_limbs outside 1 .. 8 -> LW_ERR_BAD_ARG;
 * both before any device work.  d_scalars rows are 8 * scalar_limbs bytes: the buffer must be 16-byte aligned for even
 * scalar_limbs and 8-byte aligned for odd (LW_ERR_BAD_ARG otherwise).  Output as lw_hip_msm; scalar_limbs == 4 is
 * exactly lw_hip_msm / lw_hip_msm_device. */
int lw_hip_msm_limbs(lw_curve_t curve, const uint64_t *scalars, uint32_t scalar_limbs, size_t n_scalars, const void *points,
                     size_t n_points, void *out_point);
int lw_hip_msm_limbs_device(lw_curve_t curve, const uint64_t *d_scalars, uint32_t scalar_limbs, const void *d_points, size_t n,
                            void *out_point_host, void *hip_stream);

/* Batched group law, IsGroup::operate_with (math/src/elliptic_curve/short_weierstrass/point.rs:171-207) on device
 * buffers: d_out[j*m + i] = d_rows[i] + d_cols[j] (projective points, reference layout; the sums are generally not
 * normalised, Z != 1).  bench.py builds its 2^24 distinct input points with it from two short runs. */
int lw_hip_ec_add_outer_device(lw_curve_t curve, const void *d_rows, size_t m, const void *d_cols, size_t k, void *d_out,
                               void *hip_stream);

/* The test seam of the group law: one formula of csrc/ec.cuh per row, exactly as the MSM kernels call it, so that a test
 * chooses every operand of every field product.  The complete formulas (RCB16 Alg. 7, 8, 9) are polynomials in the
 * coordinates: the rows need not be on the curve, and d_out receives the (X, Y, Z) the function returned, bit for bit —
 * nothing is normalised and nothing is mapped back.
 *   model   0: the caller's curve; 1: the isomorphic model the MSM runs normalised point sets on (BLS12-381 G1:
 *           y^2 = x^3 + 2/3, BN254 G2: y^2 = x^3 + 9 + u); LW_ERR_BAD_ARG for the curves that have none.
 *   d_a     n projective rows, reference layout (coordinates are canonical Montgomery residues, < p).
 *   d_b     LW_EC_OP_ADD, LW_EC_OP_ADD_QUAD: n projective rows.  LW_EC_OP_ADD_MIXED: n dense affine rows (x, y), two
 *           coordinates apart; a row (0, 0) is the identity and returns row a.  LW_EC_OP_DBL, LW_EC_OP_TO_AFFINE: NULL.
 *   op      ADD_QUAD is ADD spread over the four lanes of a quad (pt_add_quad): same group element, same bytes.
 *           TO_AFFINE is (X/Z : Y/Z : 1), Z = 0 -> (0 : 1 : 0).
 * A bad curve, op or model, a NULL or misaligned buffer (16 bytes), a missing or a superfluous d_b: LW_ERR_BAD_ARG, before
 * any device work.  n = 0 (checked after curve, op and model): LW_OK, nothing is touched.  d_out must not overlap d_a or
 * d_b. */
typedef enum { LW_EC_OP_ADD = 0, LW_EC_OP_ADD_MIXED = 1, LW_EC_OP_DBL = 2, LW_EC_OP_ADD_QUAD = 3, LW_EC_OP_TO_AFFINE = 4 } lw_ec_op_t;
int lw_hip_ec_pointwise_device(lw_curve_t curve, int model, lw_ec_op_t op, const void *d_a, const void *d_b,
                               size_t n, void *d_out, void *hip_stream);

/* The test seam of the field arithmetic: one primitive of csrc/field.cuh per row (csrc/field_pointwise_ops.cuh holds the
 * table, csrc/field_pointwise.hip the kernel), on operands the caller chooses, the returned limbs written back bit for
 * bit.  Fields and ops have enums of their own: the seam reaches fields (the base fields, Fr254) and operand ranges that
 * no transform takes, so lw_field_t and lw_layout_t are not involved.
 *   rows    Multi-limb fields: an element is N/2 u64 limbs, most significant first (the reference layout), read and
 *           written as stored: nothing is converted.  "a < p" below is about that stored integer.  BabyBear: u32 words,
 *           except the u64 words REDUCE64 and FROM_R64 read and TO_R64 writes.
 *   op      (out "canonical": < p; "raw": the limbs the primitive returned, see its comment in field.cuh)
 *           ADD, SUB, NEG, DBL    fe_add, fe_sub, fe_neg, fe_dbl; a, b < p; canonical
 *           MUL                   fe_mul; one operand < p, the other any N-limb value, in either order; canonical
 *           SQR                   fe_sqr; a < p; canonical
 *           MUL_LAZY              fe_mul_lazy; a < p, b any N-limb value; raw, in [0, 2p)
 *           MUL_LAZY_UNIFORM      fe_mul_lazy_uniform; d_a holds ONE row, read by every work-item through the same address,
 *                                 a < p; b any N-limb value; the bytes of MUL_LAZY
 *           REDUCE_FULL           fe_reduce_full; Stark252: any 256-bit value, other fields: a < 2p; canonical
 *           COND_SUB_P            fe_cond_sub_kp<F, 0>; any N-limb value; a - p if a >= p, else a
 *           ADD_RAW               fe_add_raw; a + b < 2^(32N); a + b
 *           ADD2P_SUB_RAW         fe_add2p_sub_raw; b <= a + 2p and a + 2p - b < 2^(32N); a + 2p - b
 *           NEG_RAW, NEG_RAW_2P   fe_neg_raw, a <= p: p - a; fe_neg_raw_2p, a <= 2p: 2p - a
 *           TO_MONT, FROM_MONT    fe_to_mont, fe_from_mont; a < p; canonical
 *           DOT2, DOT4            fe_dot<F, 2>, fe_dot<F, 4>; rows of 2 / 4 elements in d_a and in d_b, each <= p (p itself
 *                                 allowed); one element out, canonical.  LW_ERR_BAD_ARG for a field whose modulus leaves
 *                                 fe_dot no room for that many products (DOT4 on Fr381)
 *           INV                   fe_inv (Fermat); a < p, 0 -> 0; canonical
 *           BabyBear only: MUL, ADD, SUB (bb_mul, bb_add, bb_sub; words < p); REDUCE64 (bb_reduce; a u64 below p * 2^32);
 *           FROM_R64 (bb_from_r64; a u64 below p); TO_R64 (bb_to_r64; a word < p, a u64 out).  Every other pairing of
 *           BabyBear, or of a multi-limb field, with an op: LW_ERR_BAD_ARG.
 * Operands outside the stated domain are not detected: the result is whatever the primitive gives.
 * One work-item per row; rows past n are never written.  A bad field or op, an op the field does not have, a NULL or
 * misaligned buffer (16 bytes), a missing or a superfluous d_b: LW_ERR_BAD_ARG, before any device work.  n = 0 (checked
 * after field and op): LW_OK, nothing is touched.  d_out may be exactly d_a or exactly d_b where the rows of that operand
 * are as long as the output's (not DOT2 / DOT4, not the single row of MUL_LAZY_UNIFORM, not across word sizes); any other
 * overlap of d_out with an operand is LW_ERR_BAD_ARG. */
typedef enum {
    LW_PW_FIELD_STARK252 = 0, LW_PW_FIELD_FR381 = 1, LW_PW_FIELD_FR254 = 2, LW_PW_FIELD_FP381 = 3, LW_PW_FIELD_FP254 = 4,
    LW_PW_FIELD_BABYBEAR = 5
} lw_pw_field_t;
typedef enum {
    LW_FIELD_OP_ADD = 0, LW_FIELD_OP_SUB = 1, LW_FIELD_OP_NEG = 2, LW_FIELD_OP_DBL = 3, LW_FIELD_OP_MUL = 4, LW_FIELD_OP_SQR = 5,
    LW_FIELD_OP_MUL_LAZY = 6, LW_FIELD_OP_MUL_LAZY_UNIFORM = 7, LW_FIELD_OP_REDUCE_FULL = 8, LW_FIELD_OP_COND_SUB_P = 9,
    LW_FIELD_OP_ADD_RAW = 10, LW_FIELD_OP_ADD2P_SUB_RAW = 11, LW_FIELD_OP_NEG_RAW = 12, LW_FIELD_OP_NEG_RAW_2P = 13,
    LW_FIELD_OP_TO_MONT = 14, LW_FIELD_OP_FROM_MONT = 15, LW_FIELD_OP_DOT2 = 16, LW_FIELD_OP_DOT4 = 17, LW_FIELD_OP_INV = 18,
    LW_FIELD_OP_REDUCE64 = 19, LW_FIELD_OP_FROM_R64 = 20, LW_FIELD_OP_TO_R64 = 21
} lw_field_op_t;
int lw_hip_field_pointwise_device(lw_pw_field_t field, lw_field_op_t op, const void *d_a, const void *d_b, size_t n, void *d_out,
                                  void *hip_stream);

/* Fixed point set cached on the device in affine form (SURVEY 8f "next" #2, second half).  Every reference caller
 * multiplies against a structured reference string it built once: KZG commits with
 * msm(&coefficients, &srs.powers_main_group[..coefficients.len()]) (crypto/src/commitments/kzg.rs:159-163), Groth16 with
 * the proving key's l_tau_g1 / r_tau_g1 / ... vectors (provers/groth16/src/prover.rs:69-85).  lw_hip_srs_create uploads
 * the projective points once, normalises them on the device (the to_affine of short_weierstrass/point.rs:91-129; the
 * identity is kept as a marked row) and keeps the affine rows resident; lw_hip_msm_srs then runs the same Pippenger
 * with mixed additions over the first n_scalars points.  Results are identical to lw_hip_msm on the same inputs.
 * n_scalars may be any length <= the SRS length (the KZG call shape); longer is LW_ERR_LENGTH_MISMATCH.
 * Memory: sets of 2^19 points and more keep 13 window-shifted affine copies (2^(20 w) P_i, w = 0..12) so that all windows
 * of an MSM share one bucket set — 13 x n x {128, 64, 128, 192} bytes for BLS12-381 G1 / BN254 G1 / BN254 G2 /
 * BLS12-381 G2 (27 GiB at 2^24 BLS12-381 G1 points), built once in lw_hip_srs_create (0.6 s at 2^24) and only while it
 * fits a quarter of the free device memory; LW_HIP_SRS_FOLD=0 keeps a single copy.  Results do not depend on it. */
typedef struct lw_srs lw_srs_t;
int lw_hip_srs_create(lw_curve_t curve, const void *points, size_t n_points, lw_srs_t **out_srs);
int lw_hip_srs_create_device(lw_curve_t curve, const void *d_points, size_t n_points, void *hip_stream, lw_srs_t **out_srs);
int lw_hip_srs_destroy(lw_srs_t *srs);
int lw_hip_msm_srs(const lw_srs_t *srs, const uint64_t *scalars, size_t n_scalars, void *out_point);
int lw_hip_msm_srs_device(const lw_srs_t *srs, const uint64_t *d_scalars, size_t n_scalars, void *out_point_host,
                          void *hip_stream);
/* scalars as stored FrElements (Montgomery form), see lw_hip_msm_fr */
int lw_hip_msm_srs_fr(const lw_srs_t *srs, const uint64_t *fr_elements, size_t n_scalars, void *out_point);
int lw_hip_msm_srs_fr_device(const lw_srs_t *srs, const uint64_t *d_fr_elements, size_t n_scalars, void *out_point_host,
                             void *hip_stream);

/* ---- polynomial evaluation and Ruffini division; KZG openings ----
 * Elements are 4 x u64, MS limb first, in Montgomery form, exactly as FieldElement sits in memory: the coefficients, the
 * points, x, upsilon and every returned value.  Inputs are canonical residues (< p).  field: LW_FIELD_STARK252 or
 * LW_FIELD_BLS12_381_FR (4-limb layout); anything else is LW_ERR_BAD_ARG.  Device buffers are 16-byte aligned.  Every
 * argument is checked before any device work.  Points, x and upsilon are host memory in the _device forms too.
 *
 * Polynomial::evaluate (math/src/polynomial/mod.rs:98-109) of K polynomials at M points:
 * out_values[k * m + j] = polys[k](points[j]).  Polynomial k has lens[k] coefficients (0 gives the value 0). */
int lw_poly_evaluate(lw_field_t field, const void *const *polys, const size_t *lens, uint32_t k, const void *points, uint32_t m,
                     void *out_values);
int lw_poly_evaluate_device(lw_field_t field, const void *const *d_polys, const size_t *lens, uint32_t k, const void *points,
                            uint32_t m, void *out_values_host, void *hip_stream);
/* Polynomial::ruffini_division_inplace (mod.rs:157-164) by (X - x): a quotient of n - 1 elements (none for n <= 1) and the
 * remainder p(x) that the reference pops (n = 0: 0; n = 1: a_0).  The _device form writes d_out_quotient (which must not
 * overlap d_coeffs: LW_ERR_BAD_ARG) and synchronises only when the remainder is asked for. */
int lw_poly_ruffini_division(lw_field_t field, const void *coeffs, size_t n, const void *x, void *out_quotient,
                             void *out_remainder_or_null);
int lw_poly_ruffini_division_device(lw_field_t field, const void *d_coeffs, size_t n, const void *x, void *d_out_quotient,
                                    void *out_remainder_host_or_null, void *hip_stream);
/* KateZaveruchaGoldberg::open / open_batch (crypto/src/commitments/kzg.rs:171-180, 206-226) against an SRS handle.  The
 * scalar field is the SRS curve's: BLS12-381 -> Fr381, BN254 -> Fr254.  out_proof is one projective point of the curve
 * (lw_hip_msm's output form).
 * There is no y argument: open(x, y, p) commits the quotient of (p - y) by (X - x), and y changes only coefficient 0,
 * which no quotient coefficient reads (the remainder is popped).  When p - y strips to the zero polynomial the quotient
 * is empty and the proof is the neutral element either way.
 * n <= 1 coefficients give the neutral element.  out_eval: p(x).  open_batch folds sum_k upsilon^k p_k while the division
 * loads the coefficients (the combined polynomial is never stored) and opens it; the polynomials may differ in length
 * and k has no fixed cap; out_evals[k] are the K individual values p_k(x), not the folded remainder.  upsilon may be
 * null when k <= 1.  A quotient (longest n - 1) longer than the SRS is LW_ERR_LENGTH_MISMATCH (the reference panics
 * slicing srs[..len]).  Host results synchronise before returning. */
int lw_kzg_open(const lw_srs_t *srs, const uint64_t *coeffs, size_t n, const uint64_t *x, void *out_proof, uint64_t *out_eval_or_null);
int lw_kzg_open_device(const lw_srs_t *srs, const uint64_t *d_coeffs, size_t n, const uint64_t *x, void *out_proof_host,
                       uint64_t *out_eval_host_or_null, void *hip_stream);
int lw_kzg_open_batch(const lw_srs_t *srs, const uint64_t *const *polys, const size_t *lens, uint32_t k, const uint64_t *x,
                      const uint64_t *upsilon, void *out_proof, uint64_t *out_evals_or_null);
int lw_kzg_open_batch_device(const lw_srs_t *srs, const uint64_t *const *d_polys, const size_t *lens, uint32_t k, const uint64_t *x,
                             const uint64_t *upsilon, void *out_proof_host, uint64_t *out_evals_host_or_null, void *hip_stream);

/* ---- STARK DEEP composition polynomial ----
 * compute_deep_composition_poly / compute_trace_term (provers/stark/src/prover.rs:643-714, 720-747), the step of
 * round_4_compute_and_run_fri_on_the_deep_composition_polynomial (:536-594) that produces fri::commit_phase's input:
 *   deep = sum_i gamma'_i (H_i - H_i(z^P)) / (X - z^P)  +  sum_j sum_r gamma_{j,r} (t_j - y_{j,r}) / (X - g^r z).
 * Stated over K polynomials, M points and a K x M weight matrix (row-major, weights[k * m + j]):
 *   out = sum_j quot(sum_k weights[k][j] * polys[k], points[j]),    quot(p, x) = ruffini_division_inplace of p by (X - x).
 * The subtracted evaluations are no input: they change only coefficient 0, which no quotient coefficient reads (the
 * remainder is popped, as in lw_kzg_open), and division is linear, so the per-term quotients of the reference add up to
 * one quotient per distinct point.  The prover's call has K = trace columns + composition parts and
 * M = frame rows + 1; trace rows carry weight 0 at z^P and the parts weight 0 at the frame points.
 * Elements are as in lw_poly_*: 4 x u64, MS limb first, Montgomery form, canonical; field LW_FIELD_STARK252 or
 * LW_FIELD_BLS12_381_FR.  points (m elements) and weights (k * m elements) are host memory in both forms.  The
 * polynomials may differ in length, k and m have no fixed cap, duplicate points and zero weights are legal; the
 * coefficients of a polynomial are not read for the points where its weight is 0.
 * out_coeffs receives n - 1 elements, n = the longest length: the Polynomial addition result before Polynomial::new
 * strips it; *out_len_or_null is the stripped length.  n <= 1 or k = 0: nothing is written, length 0, LW_OK.
 * out_evals[k * m + j] = polys[k](points[j]) where weights[k][j] != 0 and 0 elsewhere (round 3's trace_ood_evaluations
 * and composition_poly_parts_ood_evaluation in one table; they are the totals the division computes anyway).
 * m = 0, a null pointer, a field other than the two: LW_ERR_BAD_ARG; a length above 2^36: LW_ERR_ALLOC.  The _device
 * form also rejects (LW_ERR_BAD_ARG) a buffer that is not 16-byte aligned and a d_out_coeffs that overlaps an input
 * polynomial.  d_out_coeffs can go to lw_stark_fri_layer_device as d_coeffs unchanged.  The _device form synchronises
 * only when out_len or out_evals is asked for; with neither it enqueues and returns (stream contract above). */
int lw_stark_deep_composition(lw_field_t field, const void *const *polys, const size_t *lens, uint32_t k, const void *points,
                              uint32_t m, const void *weights, void *out_coeffs, size_t *out_len_or_null, void *out_evals_or_null);
int lw_stark_deep_composition_device(lw_field_t field, const void *const *d_polys, const size_t *lens, uint32_t k,
                                     const void *points, uint32_t m, const void *weights, void *d_out_coeffs,
                                     size_t *out_len_or_null, void *out_evals_host_or_null, void *hip_stream);

/* ---- STARK round 4 tail: grinding and query openings ----
 * What round_4_compute_and_run_fri_on_the_deep_composition_polynomial does after fri::commit_phase
 * (provers/stark/src/prover.rs:596-617), on the data the calls above left in HBM.
 *
 * Grinding, grinding::generate_nonce (provers/stark/src/grinding.rs:40-54, is_valid_nonce_for_inner_hash :58-68,
 * get_inner_hash :72-80):
 *   inner = Keccak256(01 23 45 67 89 ab cd ed || seed (32 bytes) || grinding_factor (1 byte))
 *   valid(nonce) <=> u64_be(Keccak256(inner || nonce.to_be_bytes())[0..8]) < 2^(64 - grinding_factor)
 * The result is the SMALLEST valid nonce in [first, last], which is what the reference's build without `parallel` returns
 * for [0, u64::MAX) (its rayon build returns any valid nonce).  *out_found = 1 and *out_nonce set, or *out_found = 0 and
 * *out_nonce untouched when the range holds none.  seed32 and the outputs are host memory in both forms.
 * 2^64 - 1 is never a candidate, as in the reference, whose loop is 0..u64::MAX: last = 2^64 - 1 is accepted and means
 * 2^64 - 2, and the range [2^64 - 1, 2^64 - 1] holds none.
 * grinding_factor outside 1 .. 63 (the reference's 1 << (64 - g) is undefined there; 0 means "no grinding", which is the
 * caller's decision), a null pointer, first > last: LW_ERR_BAD_ARG, before any device work.
 * The range is searched in ascending windows of lw_stark_grinding_window(grinding_factor) candidates, one bounded kernel
 * launch and one 8-byte read-back per window; both forms return after the window that holds the result. */
uint64_t lw_stark_grinding_window(uint32_t grinding_factor);
int lw_stark_grinding_nonce(const uint8_t *seed32, uint32_t grinding_factor, uint64_t first, uint64_t last, uint64_t *out_nonce,
                            int *out_found);
int lw_stark_grinding_nonce_device(const uint8_t *seed32, uint32_t grinding_factor, uint64_t first, uint64_t last,
                                   uint64_t *out_nonce, int *out_found, void *hip_stream);

/* Query openings: MerkleTree::get_proof_by_pos (crypto/src/merkle_tree/merkle.rs:58-91, sibling_index / parent_index
 * utils.rs:7-21) and the committed rows under the opened leaves, for any number of device-resident trees in one call.
 * The path of leaf position pos in a tree of L leaves: i = pos + L - 1; push nodes[sibling(i)], i = parent(i) until i = 0:
 * log2 L nodes, bottom first, none for L = 1.  The three openers of round 4 are this primitive:
 *   fri::query_phase (fri/mod.rs:77-113)            tree k = layer k: n_cols 1, rows_per_leaf 2, bit_reverse 0 (the layer's
 *                                                   evaluation is stored permuted), position iota >> (k + 1); the leaf holds
 *                                                   evaluation[index & ~1], evaluation[index | 1], index = iota >> k
 *   open_trace_polys (prover.rs:794-820)            rows_per_leaf 1, bit_reverse 1, positions 2 iota and 2 iota + 1
 *   open_composition_poly (prover.rs:752-789)       rows_per_leaf 2, bit_reverse 1, position iota
 * The primitive reads `nodes` and the columns however they were made (lw_stark_commit_columns* hashes one row per leaf). */
typedef struct {
    lw_field_t field;          /* LW_FIELD_STARK252 or LW_FIELD_BLS12_381_FR (elements of 4 x u64) */
    const void *d_columns;     /* n_cols columns, column c at element c * col_stride_elems; NULL: paths only */
    uint32_t n_cols;
    uint64_t col_stride_elems; /* 0 = dense (2^log2_rows) */
    uint32_t log2_rows;        /* rows committed */
    uint32_t rows_per_leaf;    /* 1 or 2: leaf p covers committed rows p * r .. p * r + r - 1 */
    int bit_reverse;           /* committed row j is natural row bitrev(j, log2_rows), as in lw_stark_commit_columns */
    const void *d_nodes;       /* (2 * leaves - 1) x 32 bytes, root first; leaves = 2^log2_rows / rows_per_leaf */
} lw_stark_tree_t;
/* Opens every tree at its own q leaf positions: positions[t * q + s] (host).  Outputs are host buffers, tree-major, then
 * query:  out_values  per (t, s) rows_per_leaf * n_cols elements, row-major (row, then column); trees with
 *                     d_columns == NULL contribute nothing;
 *         out_paths   per (t, s) log2(leaves_t) x 32 bytes, bottom first.
 * One gather kernel for all trees and queries, one upload (tree table and positions), one download; synchronises.
 * Duplicate positions are legal.  q = 0 or n_trees = 0: LW_OK, nothing written, no device needed.  LW_ERR_BAD_ARG before
 * any device work: a position >= leaves, rows_per_leaf not 1 or 2, log2_rows = 0 with rows_per_leaf = 2, log2_rows > 31,
 * a field other than the two, null d_nodes, a device buffer that is not 16-byte aligned, a stride below the column
 * length, n_cols = 0 with columns, a null output that would be written. */
int lw_stark_open_trees_device(const lw_stark_tree_t *trees, uint32_t n_trees, const uint64_t *positions, uint32_t q,
                               void *out_values, uint8_t *out_paths, void *hip_stream);

/* ---- Batch inversion ----
 * FieldElement::inplace_batch_inverse (math/src/field/element.rs:47-65): out[i] = in[i]^-1, canonical, over
 * LW_FIELD_STARK252 or LW_FIELD_BLS12_381_FR (anything else: LW_ERR_BAD_ARG).  in == out is legal.  n = 0: LW_OK, no
 * device needed.  A zero element: LW_ERR_INV_ZERO (FieldError::InvZeroError), the output is then unspecified.  Both forms
 * synchronise once, to learn whether there was a zero.  Device buffers are 16-byte aligned.
 * lw_field_batch_inverse_block(): the elements one workgroup owns (a chunk per work-item, one inversion per chunk). */
int lw_field_batch_inverse(lw_field_t field, const void *in, size_t n, void *out);
int lw_field_batch_inverse_device(lw_field_t field, const void *d_in, size_t n, void *d_out, void *hip_stream);
uint64_t lw_field_batch_inverse_block(void);

/* ---- STARK round 2: the composition polynomial and its commitment ----
 * round_2_compute_composition_polynomial (provers/stark/src/prover.rs:428-484) without the AIR's compute_transition
 * (for an AIR given as data, lw_stark_transition_evaluations_device below writes the table this section reads):
 * ConstraintEvaluator::evaluate (constraints/evaluator.rs:33-225), interpolate_offset_fft, break_in_parts, the LDE of the
 * parts and commit_composition_polynomial (prover.rs:398-425).  Fields as above; elements as stored (Montgomery form,
 * 4 x u64, most significant limb first); scalars are host values, vectors device pointers in the _device forms.
 *
 * n = 2^log2_trace, N = n * 2^log2_blowup, g and w the primitive n-th and N-th roots, h = coset_offset, x_i = h w^i.
 * d_columns[c]: LDE column c, N elements, natural order (main columns first, then auxiliary ones; a boundary
 * constraint's col indexes this table).  Row c of d_transition_evals, at c * transition_stride_elems (0 = N), holds T_c(i),
 * compute_transition's value for constraint c at LDE row i.  For i in [0, N):
 *     out[i] = sum_c coeff_c Zc[i] T_c(i)  +  sum_k coeff_k (col_k[i] - value_k) / (x_i - g^step_k)
 *     Zc[i]  = cycle_c[i mod len_c] * prod_{k = 1 .. end_exemptions} (x_i - g^(n - k period))
 * with zerofier_evaluations_on_extended_domain's cycle (constraints/transition.rs:108-205, integer divisions truncate):
 *     exemptions_period == 0:  len = 2^log2_blowup * period,  cycle[e] = 1 / ((h w^e)^(n / period) - g^(offset n / period))
 *     otherwise (ep):          len = 2^log2_blowup * ep,      cycle[e] = ((h w^e)^(n / ep) - g^(n peo / ep)) / (that denominator)
 * n_boundary = 0 or n_transitions = 0 is legal (both: zeros).  LW_ERR_BAD_ARG: period = 0, col >= n_cols, log2_trace +
 * log2_blowup beyond the NTT (34, or the field's two-adicity), end_exemptions * period > n (the reference's unsigned
 * n - k period underflows), a null or misaligned buffer.  LW_ERR_INV_ZERO: a zero denominator — in the boundary part exactly
 * when h^N = 1 (checked on the host), in a cycle table as the device finds it.  Synchronises once when n_transitions > 0. */
typedef struct {
    uint32_t col, reserved;
    uint64_t step;
    uint64_t value[4];
    uint64_t coeff[4];
} lw_stark_boundary_t;
typedef struct {
    uint64_t period, offset, end_exemptions;
    uint64_t exemptions_period; /* 0: none */
    uint64_t periodic_exemptions_offset;
    uint64_t coeff[4];
} lw_stark_transition_t;
int lw_stark_constraint_evaluations_device(lw_field_t field, const void *const *d_columns, uint32_t n_cols, uint32_t log2_trace,
                                           uint32_t log2_blowup, const void *coset_offset, const lw_stark_boundary_t *boundary,
                                           uint32_t n_boundary, const lw_stark_transition_t *transitions, uint32_t n_transitions,
                                           const void *d_transition_evals, uint64_t transition_stride_elems, void *d_out,
                                           void *hip_stream);
/* H = interpolate_offset_fft(d_evals, h) (N = 2^log2_lde coefficients); break_in_parts(n_parts)
 * (math/src/polynomial/mod.rs:289-302): part j takes coefficients j, j + P, j + 2 P, ... into a zero-padded block of
 * L = next_power_of_two(ceil(N / P)) elements, d_parts_coeffs is P x L; evaluate_polynomial_on_lde_domain of every part
 * (prover.rs:150-166: its values at x_0 .. x_{N-1}, whatever the part's degree) into d_parts_lde, P x N, natural order
 * (NULL: not wanted).  out_part_lens_or_null: the P stripped lengths, as lw_stark_deep_composition_device takes them;
 * asking for them synchronises.  1 <= n_parts <= N, else LW_ERR_BAD_ARG.  d_evals is not modified. */
int lw_stark_composition_parts_device(lw_field_t field, const void *d_evals, uint32_t log2_lde, const void *coset_offset,
                                      uint32_t n_parts, void *d_parts_coeffs, void *d_parts_lde, size_t *out_part_lens_or_null,
                                      void *hip_stream);
/* commit_composition_polynomial: rows of n_parts elements, bit-reverse permuted, consecutive rows merged in pairs, then
 * BatchedMerkleTree<Keccak256>: leaf i of N / 2 hashes [H_0 .. H_{P-1}](rho) || [H_0 .. H_{P-1}](rho + N / 2),
 * rho = bitrev(i, log2_lde - 1).  Part j starts at element j * col_stride_elems (0 = N).  d_nodes: (N - 1) x 32 bytes, root
 * first — the layout lw_stark_open_trees_device reads with rows_per_leaf = 2.  log2_lde = 0: LW_ERR_BAD_ARG.
 * out_root_or_null: host, 32 bytes (synchronises when given). */
int lw_stark_commit_composition_device(lw_field_t field, const void *d_parts_lde, uint32_t n_parts, uint64_t col_stride_elems,
                                       uint32_t log2_lde, void *d_nodes, uint8_t *out_root_or_null, void *hip_stream);
/* The three calls above on host arrays, through the library's staging: columns is n_cols x N, transition_evals
 * n_transitions x N, both dense.  out_parts_coeffs: P x L; out_part_lens: P; out_root: 32 bytes; out_nodes_or_null:
 * (N - 1) x 32 bytes; out_parts_lde_or_null: P x N. */
int lw_stark_round2(lw_field_t field, const void *columns, uint32_t n_cols, uint32_t log2_trace, uint32_t log2_blowup,
                    const void *coset_offset, const lw_stark_boundary_t *boundary, uint32_t n_boundary,
                    const lw_stark_transition_t *transitions, uint32_t n_transitions, const void *transition_evals, uint32_t n_parts,
                    void *out_parts_coeffs, size_t *out_part_lens, uint8_t *out_root, uint8_t *out_nodes_or_null,
                    void *out_parts_lde_or_null);

/* ---- STARK transition constraints from an AIR given as data ----
 * The AIR's compute_transition (provers/stark/src/traits.rs) as a straight-line program that the device runs at every LDE
 * row: it writes the T_c rows lw_stark_constraint_evaluations_device reads.  Fields and elements as above.
 *
 * An accumulator machine with one field element acc and LW_STARK_AIR_MAX_TMPS temporaries; one instruction is 8 bytes:
 *     LOAD  acc = s        ADD  acc += s        SUB  acc -= s        MUL  acc *= s        NEG  acc = -acc
 *     STORE tmp[index] = acc                    EMIT T_index[i] = acc
 * s, for LOAD / ADD / SUB / MUL, by src:
 *     CELL   column `index` at trace-row offset `row`: at LDE row i, col[(i + row * 2^log2_blowup) mod len_col]
 *            (Frame::read_from_lde with the rows of a step flattened: row = offset * STEP_SIZE + row_in_step)
 *     CONST  consts[index]          TMP  tmp[index]
 * len_col = 2^col_log2_len[c] <= N; a NULL table: every column has N elements.  A periodic column is a short one: its LDE
 * has period * 2^log2_blowup elements and is stored once.  consts: n_consts host elements (the RAP challenges and the AIR's
 * literals), per call.  A field an instruction does not use (src and row of STORE and EMIT, row of a CONST or TMP operand,
 * all three of NEG) must be 0.
 *
 * Every check runs on the host before any device work; a failure is LW_ERR_BAD_ARG and lw_hip_last_error names the op:
 * an unknown op or src; a column, constant, temporary or constraint index out of range; row >= n; a non-zero unused field;
 * acc read (by anything but LOAD) before the first LOAD; a TMP read before its STORE; a constraint emitted twice or never;
 * more than LW_STARK_AIR_MAX_OPS ops or LW_STARK_AIR_MAX_CONSTS constants; col_log2_len[c] > log2_trace + log2_blowup;
 * a field other than the two; an LDE domain beyond the NTT; a null or misaligned buffer; 0 < out_stride_elems < N with
 * more than one constraint.  n_transitions = 0 with n_ops = 0 is legal and writes nothing. */
#define LW_STARK_AIR_MAX_OPS 4096
#define LW_STARK_AIR_MAX_TMPS 8
#define LW_STARK_AIR_MAX_CONSTS 256
typedef enum {
    LW_STARK_AIR_LOAD = 0,
    LW_STARK_AIR_ADD = 1,
    LW_STARK_AIR_SUB = 2,
    LW_STARK_AIR_MUL = 3,
    LW_STARK_AIR_NEG = 4,
    LW_STARK_AIR_STORE = 5,
    LW_STARK_AIR_EMIT = 6
} lw_stark_air_opcode_t;
typedef enum {
    LW_STARK_AIR_CELL = 0,
    LW_STARK_AIR_CONST = 1,
    LW_STARK_AIR_TMP = 2,
    LW_STARK_AIR_XCELL = 3, /* the _rap_ entry points of the extension sections only: auxiliary column `index`, an element of E */
    LW_STARK_AIR_XCONST = 4 /* the same: xconsts[index], an element of E */
} lw_stark_air_src_t;
typedef struct {
    uint8_t op, src;
    uint16_t index;
    uint32_t row;
} lw_stark_air_op_t;
/* d_columns: host array of n_cols device pointers, 16-byte aligned.  Row c of d_out starts at element c * out_stride_elems
 * (0 = N) and takes N elements; the rest of a stride is not written.  ops and consts are copied into the library's
 * staging before the call returns.  Enqueues on hip_stream and returns: no synchronisation. */
int lw_stark_transition_evaluations_device(lw_field_t field, const lw_stark_air_op_t *ops, uint32_t n_ops, const void *consts,
                                           uint32_t n_consts, const void *const *d_columns, const uint32_t *col_log2_len_or_null,
                                           uint32_t n_cols, uint32_t log2_trace, uint32_t log2_blowup, uint32_t n_transitions,
                                           void *d_out, uint64_t out_stride_elems, void *hip_stream);
/* The same on host arrays through the library's staging: columns holds the n_cols columns back to back, each with its
 * own 2^col_log2_len[c] (or N) elements; out is n_transitions x N, dense. */
int lw_stark_transition_evaluations(lw_field_t field, const lw_stark_air_op_t *ops, uint32_t n_ops, const void *consts,
                                    uint32_t n_consts, const void *columns, const uint32_t *col_log2_len_or_null, uint32_t n_cols,
                                    uint32_t log2_trace, uint32_t log2_blowup, uint32_t n_transitions, void *out);

/* ---- PLONK prover rounds 1-3 ----
 * Prover::round_1 / round_2 / round_3 (provers/plonk/src/prover.rs:311-341, 343-381, 383-535) without the commitments:
 * the blinded wire polynomials, the permutation grand product z and the quotient parts t_lo, t_mid, t_hi.  With
 * lw_hip_msm_srs_fr_device for the commitments and lw_kzg_open_batch_device for rounds 4-5 the reference prover runs
 * device-resident: only challenges, blinders and commitments cross the bus.
 * Elements are as in lw_poly_*: 4 x u64, MS limb first, Montgomery form, canonical; field LW_FIELD_STARK252 or
 * LW_FIELD_BLS12_381_FR, anything else LW_ERR_BAD_ARG.  Device buffers are 16-byte aligned (LW_ERR_BAD_ARG otherwise).
 * Every argument is checked before any device work.  beta, gamma, alpha, k1, the blinders and the public input are host
 * memory in the _device forms too.  Outputs overlap no input.  Stream contract as at the top of this header.
 *
 * The circuit handle is the device-side CommonPreprocessedInput (provers/plonk/src/setup.rs), built once per circuit like
 * lw_srs_t, from host buffers: q_coeffs = ql | qr | qo | qm | qc and s_coeffs = s1 | s2 | s3 in coefficient form, n
 * coefficients each (zero padded); s_lagrange = s1_lagrange | s2_lagrange | s3_lagrange, n values each.  n not a power
 * of two: LW_ERR_INPUT_NOT_POW2; log2(4n) above the field's two-adicity: LW_ERR_ROOT_OF_UNITY.  On the coset
 * k1 * <w_4n> the vanishing polynomial X^n - 1 takes the four values k1^n * i4^j - 1 (i4 = w_4n^n, j = 0 .. 3); if one of
 * them is zero — or k1 is — the result is LW_ERR_INV_ZERO (round 3 divides by them).
 * The handle keeps on the device: the three s_lagrange columns (3n elements), the evaluations of the eight polynomials
 * and of l1 on the coset (9 x 4n), and the table x_i = k1 * w_4n^i (4n): 43 n elements = 1376 n bytes, 1.34 GiB at
 * n = 2^20.  The inverse vanishing values, k1^n * i4^j, 1 / k1 and w_n are kept on the host side of the handle.
 * A handle is read-only once created: any number of calls, threads and streams may share it.  Destroy it before
 * lw_hip_init rebinds the device. */
typedef struct lw_plonk_circuit lw_plonk_circuit_t;
int lw_plonk_circuit_create(lw_field_t field, size_t n, const void *k1, const void *q_coeffs, const void *s_coeffs,
                            const void *s_lagrange, lw_plonk_circuit_t **out);
int lw_plonk_circuit_destroy(lw_plonk_circuit_t *circuit);

/* Round 1: p_w = interpolate_fft(w) + (b0 + b1 X)(X^n - 1) for w = a, b, c.  witness: a | b | c, n values each.
 * blinders_or_null: six host elements, b0 b1 of a, then of b, then of c (NULL: no blinding, the reference's test
 * generator).  out_p_abc: three blocks of n + 2 coefficients (trailing zeros are not stripped).  The blinding is added as
 * out[i] -= b_i, out[n + i] += b_i, which is the product for every n >= 1. */
int lw_plonk_round1(const lw_plonk_circuit_t *circuit, const void *witness, const void *blinders_or_null, void *out_p_abc);
int lw_plonk_round1_device(const lw_plonk_circuit_t *circuit, const void *d_witness, const void *blinders_or_null,
                           void *d_out_p_abc, void *hip_stream);

/* Round 2: z_0 = 1, z_{i+1} = z_i * num_i / den_i for i = 0 .. n-2 with num, den as prover.rs:360-363, then
 * p_z = interpolate_fft(z) + (b0 + b1 X + b2 X^2)(X^n - 1).  blinders_or_null: three host elements.
 * out_z_values_or_null: the n values z_i; out_p_z: n + 3 coefficients.  Row n-1 of the witness and of s_lagrange is never
 * read.  A zero den_i with i <= n-2 is LW_ERR_INV_ZERO (the reference's division fails there); a zero num_i is legal and
 * zeroes the rest of z.  The rows are not divided one by one: z_i = (prod_{j<i} num_j) (prod_{i<=j<=n-2} den_j) / (prod
 * of all den_j), with one inversion per call, on the host, of the 32 bytes that also decide LW_ERR_INV_ZERO — so BOTH
 * forms synchronise the stream once in mid-call; the _device form returns with the rest of its work enqueued. */
int lw_plonk_round2(const lw_plonk_circuit_t *circuit, const void *witness, const void *beta, const void *gamma,
                    const void *blinders_or_null, void *out_z_values_or_null, void *out_p_z);
int lw_plonk_round2_device(const lw_plonk_circuit_t *circuit, const void *d_witness, const void *beta, const void *gamma,
                           const void *blinders_or_null, void *d_out_z_values_or_null, void *d_out_p_z, void *hip_stream);

/* Round 3: t = interpolate_offset_fft(p_eval / Z_H, k1) on the 4n-point coset with offset k1, p_eval as
 * prover.rs:440-498, from round 1's p_abc (3 x (n + 2)) and round 2's p_z (n + 3).  public_input: n_pub host elements,
 * zero padded to n (n_pub > n: LW_ERR_LENGTH_MISMATCH).  t is cut as the reference cuts it: zero padded to 3 (n + 2)
 * where 4n is shorter (n <= 4), coefficients from 3 (n + 2) on dropped.  out_t: three blocks of n + 3 coefficients,
 *   block 0 = t[0 .. n+2) then b_0,
 *   block 1 = t[n+2 .. 2n+4) with b_0 subtracted from coefficient 0, then b_1,
 *   block 2 = t[2n+4 .. 3n+6) with b_1 subtracted from coefficient 0, then 0,
 * with blinders_or_null = b_0 b_1 (two host elements; NULL: zero).  Each block can go to lw_hip_msm_srs_fr_device and to
 * lw_kzg_open_batch_device as it is.  Per call: one n-point inverse transform for the public input (none when
 * n_pub = 0), one batch of low-degree extensions n -> 4n (a, b, c, z and the public input), one kernel over the 4n points,
 * one 4n-point inverse transform.  The _device form enqueues and returns. */
int lw_plonk_round3(const lw_plonk_circuit_t *circuit, const void *p_abc, const void *p_z, const void *public_input, size_t n_pub,
                    const void *beta, const void *gamma, const void *alpha, const void *blinders_or_null, void *out_t);
int lw_plonk_round3_device(const lw_plonk_circuit_t *circuit, const void *d_p_abc, const void *d_p_z, const void *public_input,
                           size_t n_pub, const void *beta, const void *gamma, const void *alpha, const void *blinders_or_null,
                           void *d_out_t, void *hip_stream);

/* ---- Starknet Poseidon (PoseidonCairoStark252, crypto/src/hash/poseidon/mod.rs) ----
 * The Hades permutation over Stark252 with the public Starknet parameters (state 3, rate 2, x^3, 4 + 83 + 4 rounds; round
 * keys derived from sha256("Hades" + index), tools/gen_poseidon_consts.py), the three hashes built on it and the two
 * Poseidon Merkle trees of the reference, batched: one work-item per permutation chain.  Stark252 only, so no lw_field_t.
 * Elements are as everywhere else: 4 x u64, most significant limb first, Montgomery form, canonical (< p); every output
 * is canonical.  Each function has a host form (buffers in host memory, complete on return) and a _device form (16-byte
 * aligned device pointers, work enqueued on hip_stream; misaligned: LW_ERR_BAD_ARG).  n = 0 / n_rows = 0: LW_OK, nothing is
 * touched.  More than 2^36 inputs: LW_ERR_ALLOC.
 *
 *   permute      n states of 3 elements -> n states (hades_permutation, mod.rs:27-41); out may be states (in place)
 *   hash         out[i] = hash(x[i], y[i]): word 0 of the permuted (x, y, 2)                                (mod.rs:59-64)
 *   hash_single  out[i] = hash_single(x[i]): word 0 of the permuted (x, 0, 1)                              (mod.rs:66-71)
 *   hash_many    n_rows row-major rows of row_len >= 0 elements -> one digest each: the row, a 1, zeros up to a multiple
 *                of 2, absorbed two elements per permutation into words 0 and 1; row_len = 0 hashes the padding block
 *                alone (rows may then be NULL)                                                               (mod.rs:73-96) */
int lw_poseidon_permute(const void *states, size_t n, void *out);
int lw_poseidon_permute_device(const void *d_states, size_t n, void *d_out, void *hip_stream);
int lw_poseidon_hash(const void *x, const void *y, size_t n, void *out);
int lw_poseidon_hash_device(const void *d_x, const void *d_y, size_t n, void *d_out, void *hip_stream);
int lw_poseidon_hash_single(const void *x, size_t n, void *out);
int lw_poseidon_hash_single_device(const void *d_x, size_t n, void *d_out, void *hip_stream);
int lw_poseidon_hash_many(const void *rows, size_t n_rows, size_t row_len, void *out);
int lw_poseidon_hash_many_device(const void *d_rows, size_t n_rows, size_t row_len, void *d_out, void *hip_stream);

/* The Poseidon twin of lw_stark_commit_columns[_device]: the tree over the 2^log2n rows of n_cols columns, with
 *   leaf_mode = LW_POSEIDON_LEAF_SINGLE  TreePoseidon (merkle_tree/backends/field_element.rs:53-76): leaf = hash_single(v);
 *                                        n_cols must be 1 (else LW_ERR_BAD_ARG)
 *   leaf_mode = LW_POSEIDON_LEAF_MANY    BatchPoseidonTree (backends/field_element_vector.rs:61-85): leaf = hash_many(row),
 *                                        which for n_cols = 1 is NOT hash_single
 * and parent = hash(left, right).  nodes: (2 * 2^log2n - 1) elements of 32 bytes in the layout above, root first and leaves
 * last (merkle_tree/utils.rs:43-71), so lw_stark_open_trees_device reads such a tree as it is; out_root: the root element,
 * 32 bytes.  bit_reverse and col_stride_elems (0: dense) as in the Keccak form: leaf i commits natural row bitrev(i), the
 * gather and the transposition happen in the leaf kernel and nothing is copied.  Exactly 2^log2n leaves: completing a
 * shorter list by repeating its last leaf (utils.rs:24-29) stays with the caller, as for the Keccak trees.  log2n > 31:
 * LW_ERR_ALLOC.  The _device form synchronises the stream only when out_root is not NULL. */
typedef enum { LW_POSEIDON_LEAF_SINGLE = 0, LW_POSEIDON_LEAF_MANY = 1 } lw_poseidon_leaf_t;
int lw_poseidon_commit_columns(const void *columns, uint32_t n_cols, uint32_t log2n, int bit_reverse, int leaf_mode,
                               uint8_t *out_root, uint8_t *out_nodes_or_null);
int lw_poseidon_commit_columns_device(const void *d_columns, uint32_t n_cols, uint64_t col_stride_elems, uint32_t log2n,
                                      int bit_reverse, int leaf_mode, void *d_nodes, uint8_t *out_root, void *hip_stream);

/* ---- Starknet Pedersen hash over the Stark curve (PedersenStarkCurve::hash, crypto/src/hash/pedersen/mod.rs) ----
 * The Stark curve is y^2 = x^3 + x + b over the Stark252 prime; it is not an lw_curve_t (nothing else here runs on it).
 * Elements, host and _device forms, alignment, n = 0 and the 2^36 limit as for Poseidon above.
 *   hash           out[i] = hash(x[i], y[i]): the affine x of P0 + sum of table points chosen by the nibbles of the
 *                  canonical integers x[i], y[i] (mod.rs:43-54); one work-item per hash, about 117 curve additions and one
 *                  inversion each
 *   commit_leaves  the 2-to-1 tree over 2^log2n leaf VALUES (Starknet's Pedersen trees): the reference's MerkleTree with
 *                  hash_new_parent = hash and identity leaves.  nodes, out_root, bit_reverse, log2n > 31 and the
 *                  synchronisation of the _device form as lw_poseidon_commit_columns[_device]; n_cols is the number of
 *                  columns offered and must be 1 (else LW_ERR_BAD_ARG: a leaf is one element)
 *   table          host only, no device needed: the 1 890 affine points of the lookup tables T1 || T2 || T3 || T4
 *                  (930 + 15 + 930 + 15; T1[15 i + k - 1] = k 2^(4 i) P1, T2[k - 1] = k P2, T3, T4 from P3, P4), as they are
 *                  generated from StarkWare's five published points: (x, y), 8 u64 each, 120 960 bytes
 *   add_affine     test seam of the group law, device form only: out[i] = p[i] + q[i] for affine points (x, y) of 8 u64,
 *                  (0, 0) standing for the point at infinity in p and out.  p[i] is lifted to the hash kernel's Jacobian
 *                  accumulator and rescaled by z[i] != 0 ((X, Y, Z) -> (X z^2, Y z^3, Z z)), q[i] is added with the
 *                  device function the hash calls and the sum is normalised by the hash's own code path, so doubling
 *                  (p = q), p = -q and p = infinity are reachable with chosen operands */
int lw_pedersen_hash(const void *x, const void *y, size_t n, void *out);
int lw_pedersen_hash_device(const void *d_x, const void *d_y, size_t n, void *d_out, void *hip_stream);
int lw_pedersen_commit_leaves(const void *leaves, uint32_t n_cols, uint32_t log2n, int bit_reverse, uint8_t *out_root,
                              uint8_t *out_nodes_or_null);
int lw_pedersen_commit_leaves_device(const void *d_leaves, uint32_t n_cols, uint32_t log2n, int bit_reverse, void *d_nodes,
                                     uint8_t *out_root, void *hip_stream);
int lw_pedersen_table(void *out);
int lw_pedersen_add_affine_device(const void *d_p, const void *d_z, const void *d_q, size_t n, void *d_out, void *hip_stream);

/* ---- dense multilinear polynomials and the sumcheck prover's round ----
 * DenseMultilinearPolynomial::evaluate / fix_variables (math/src/polynomial/dense_multilinear_poly.rs) and the round
 * polynomial of a sumcheck over a product of K tables.  Elements are as in lw_poly_*: 4 x u64, MS limb first, Montgomery
 * form, canonical in and out; field LW_FIELD_STARK252 or LW_FIELD_BLS12_381_FR.  point, r and r_prev are host memory in
 * both forms.
 * A table T of 2^n_vars elements is a polynomial in x_0 .. x_{n-1}, x_0 on the MOST significant bit of the index (the
 * order of the reference's chis table).  eq(r, 1) = r, eq(r, 0) = 1 - r.
 *   evaluate       out[kk] = sum_i tables[kk][i] * prod_j eq(point[j], bit_{n-1-j}(i)) for k >= 1 tables at one point;
 *                  n_vars = 0 returns tables[kk][0] (the host form then needs no device).  Synchronises once.
 *   fix_variables  out[j] = sum_{b < 2^t} eq(r[0..t), b) * table[b * 2^(n-t) + j], 2^(n-t) elements: t = n is evaluate,
 *                  t = 0 a copy.  The _device form enqueues and returns; for t > 0 d_out must not overlap d_table.
 *   sumcheck_round out_round[u] = g(u) = sum_{j<h} prod_k (T_k[j] + u * (T_k[j+h] - T_k[j])), u = 0 .. k, h = 2^(n-1):
 *                  k + 1 elements, g(0) + g(1) = the sum of the product over the cube.  k is 1, 2 or 3.  With r_prev
 *                  (fused form, n_vars >= 2) every table is first replaced IN PLACE by fix_variables(T_k, [r_prev]) - its
 *                  first 2^(n-1) elements hold the bound table, the rest is unspecified afterwards - and g is taken over
 *                  the n - 1 remaining variables; a round then reads every table once.  Synchronises once.
 * LW_ERR_BAD_ARG, decided before any device work: a field other than the two, a null pointer where data is needed,
 * n_vars > 30, k = 0, k > 3 for a round, t > n_vars, a round with n_vars = 0, a fused round with n_vars < 2, a device
 * pointer that is not 16-byte aligned, two tables of a round that overlap, a d_out that overlaps d_table when t > 0. */
int lw_multilinear_evaluate(lw_field_t field, const void *const *tables, uint32_t k, uint32_t n_vars, const void *point, void *out);
int lw_multilinear_evaluate_device(lw_field_t field, const void *const *d_tables, uint32_t k, uint32_t n_vars, const void *point,
                                   void *out_host, void *hip_stream);
int lw_multilinear_fix_variables(lw_field_t field, const void *table, uint32_t n_vars, const void *r, uint32_t t, void *out);
int lw_multilinear_fix_variables_device(lw_field_t field, const void *d_table, uint32_t n_vars, const void *r, uint32_t t,
                                        void *d_out, void *hip_stream);
int lw_sumcheck_round(lw_field_t field, void *const *tables, uint32_t k, uint32_t n_vars, const void *r_prev_or_null,
                      void *out_round);
int lw_sumcheck_round_device(lw_field_t field, void *const *d_tables, uint32_t k, uint32_t n_vars, const void *r_prev_or_null,
                             void *out_round_host, void *hip_stream);

/* ---- the table of eq(point, .) and the sumcheck round over an eq-weighted sum of products ----
 * The shape of Spartan's two sumchecks, of a GKR layer and of HyperPlonk's zero check:
 * sum_x E(x) * sum_t c_t * prod_{m in S_t} T_m(x), E the table of eq(tau, .).  Fields, element form, variable order and
 * n_vars <= 30 are those of lw_multilinear_* above; point, masks, coefficients and r_prev are host memory in both forms.
 *   eq_table     out[i] = prod_j eq(point[j], bit_{n-1-j}(i)), i < 2^n_vars, canonical residues: the reference's chis table,
 *                bit for bit.  n_vars = 0 writes the element one (the host form then needs no device).  The _device form
 *                enqueues and returns; nothing in flight reads caller memory.
 *   terms_round  out_round[u] = g(u) = sum_{j<h} E_j(u) * sum_t c_t * prod_{m in mask_t} T_m,j(u), u = 0 .. D, with
 *                X_j(u) = X[j] + u * (X[j+h] - X[j]) and h = 2^(n-1).  Bit m of term_masks[t] puts tables[m] into term t;
 *                D = max_t popcount(term_masks[t]) + (eq ? 1 : 0), and D + 1 elements are written.  Without eq the factor E
 *                is absent.  term_coeffs_or_null holds n_terms elements; NULL means every coefficient is one.  The
 *                coefficients one and minus one cost no product.  With r_prev (fused form, n_vars >= 2) every table and
 *                the eq table is first replaced IN PLACE by its binding to r_prev, exactly as in sumcheck_round: the first
 *                2^(n-1) elements hold the bound table, the rest is unspecified, g is taken over the n - 1 remaining
 *                variables, and a round reads every table once.  Synchronises once.
 * Limits: 1 <= n_tables <= 4 not counting eq, 1 <= n_terms <= 8, every mask non-zero, within n_tables bits and of at most
 * three bits, so D <= 4.  A power of one table (A^2) and more than four tables are out of scope: the pair of every table
 * and the D + 1 running sums of a thread live in registers, and a fifth table would not fit beside them.
 * LW_ERR_BAD_ARG, decided before any device work: a field other than the two, a null pointer where data is needed,
 * n_tables or n_terms out of range, a mask that is zero, has a bit at or above n_tables or more than three bits,
 * n_vars > 30, a round with n_vars = 0, a fused round with n_vars < 2, a device pointer that is not 16-byte aligned, any
 * two of the tables and eq that overlap. */
int lw_multilinear_eq_table(lw_field_t field, const void *point, uint32_t n_vars, void *out);
int lw_multilinear_eq_table_device(lw_field_t field, const void *point, uint32_t n_vars, void *d_out, void *hip_stream);
int lw_sumcheck_terms_round(lw_field_t field, void *const *tables, uint32_t n_tables, void *eq_or_null,
                            const uint32_t *term_masks, const void *term_coeffs_or_null, uint32_t n_terms, uint32_t n_vars,
                            const void *r_prev_or_null, void *out_round);
int lw_sumcheck_terms_round_device(lw_field_t field, void *const *d_tables, uint32_t n_tables, void *d_eq_or_null,
                                   const uint32_t *term_masks, const void *term_coeffs_or_null, uint32_t n_terms,
                                   uint32_t n_vars, const void *r_prev_or_null, void *out_round_host, void *hip_stream);

/* ---- a rank-one constraint system on the device: A z, B z, C z, the row-bound matrix, Groth16's h from a witness ----
 * The handle keeps the three sparse matrices A, B, C of an R1CS (n_rows constraints over n_cols variables) resident, built
 * once per circuit like lw_plonk_circuit_t.  Fields and element form are those of lw_multilinear_*: LW_FIELD_STARK252 or
 * LW_FIELD_BLS12_381_FR, 4 x u64, MS limb first, Montgomery form, canonical.
 *   create       three CSR matrices in host memory: row_ptr[m] has n_rows + 1 entries, col_idx[m] and values[m] have
 *                nnz_m = row_ptr[m][n_rows] (< 2^32).  1 <= n_rows, n_cols <= 2^30.  A matrix may be empty (its col_idx and
 *                values may then be NULL), rows may be empty, the columns of a row need no order, a repeated (row, column)
 *                is summed, explicit zeros are allowed.  LW_ERR_BAD_ARG, decided on the host before any device work: a field
 *                other than the two, NULL where data is needed, n_rows or n_cols out of range, row_ptr[m][0] != 0 or a
 *                decreasing row_ptr, a column index >= n_cols, a value >= p.  The handle holds the CSR arrays, the
 *                transposed index, a class per entry (one, minus one, general: the first two cost no product) and the plan
 *                of the lists longer than lw_r1cs_split_length() entries, which are cut into pieces of that length.
 *   matvec       every requested output receives n_out >= n_rows elements: (M z)[i] for i < n_rows, zero above, whatever
 *                the buffer held.  z holds n_cols elements.  n_out is the padded table or gate-domain length (<= 2^34).
 *   bind_rows    out[j] = sum_i e[i] * (c_A A[i,j] + c_B B[i,j] + c_C C[i,j]) for j < n_cols, zero for n_cols <= j < n_out.
 *                e holds n_rows elements; coeffs3 = (c_A, c_B, c_C) is host memory in both forms.  With e the table of
 *                eq(r_x, .) this is the table of Spartan's second sumcheck.
 *   first_unsatisfied  *out_row = the smallest i with (A z)_i (B z)_i != (C z)_i, or -1.  Synchronises.
 *   The _device forms take 16-byte aligned device pointers and enqueue on hip_stream; matvec and bind_rows wait for nothing.
 *   LW_ERR_BAD_ARG before any device work: a NULL handle or vector, n_out below the rows (columns) or above 2^34, a
 *   misaligned device pointer, an output that overlaps the input vector or another output.
 *   lw_r1cs_lazy_terms(): the terms a Stark252 sum carries between two full reductions (the bound is in csrc/r1cs.hip).
 *   h_from_witness  QuadraticArithmeticProgram::calculate_h_coefficients from the witness w (n_cols elements) of a system
 *                over LW_FIELD_BLS12_381_FR (else LW_ERR_BAD_ARG): A w, B w, C w padded to num_gates, their interpolations
 *                over the gate domain (what scale_and_accumulate_variable_polynomials sums on the host,
 *                provers/groth16/src/qap.rs:44-66), then lw_groth16_h_coefficients, bit for bit.  num_gates: a power of two
 *                (else LW_ERR_INPUT_NOT_POW2) >= n_rows (else LW_ERR_BAD_ARG).  out_h and coeff_len_or_null as there. */
typedef struct lw_r1cs lw_r1cs_t;
int lw_r1cs_create(lw_field_t field, uint32_t n_rows, uint32_t n_cols, const uint32_t *const row_ptr[3],
                   const uint32_t *const col_idx[3], const void *const values[3], lw_r1cs_t **out);
int lw_r1cs_destroy(lw_r1cs_t *r1cs);
uint32_t lw_r1cs_split_length(void);
uint32_t lw_r1cs_lazy_terms(void);
int lw_r1cs_matvec(const lw_r1cs_t *r1cs, const void *z, size_t n_out, void *out_az_or_null, void *out_bz_or_null,
                   void *out_cz_or_null);
int lw_r1cs_matvec_device(const lw_r1cs_t *r1cs, const void *d_z, size_t n_out, void *d_out_az_or_null, void *d_out_bz_or_null,
                          void *d_out_cz_or_null, void *hip_stream);
int lw_r1cs_bind_rows(const lw_r1cs_t *r1cs, const void *e, const void *coeffs3, size_t n_out, void *out);
int lw_r1cs_bind_rows_device(const lw_r1cs_t *r1cs, const void *d_e, const void *coeffs3, size_t n_out, void *d_out,
                             void *hip_stream);
int lw_r1cs_first_unsatisfied(const lw_r1cs_t *r1cs, const void *z, int64_t *out_row);
int lw_r1cs_first_unsatisfied_device(const lw_r1cs_t *r1cs, const void *d_z, int64_t *out_row, void *hip_stream);
int lw_groth16_h_from_witness(const lw_r1cs_t *r1cs, const void *w, size_t num_gates, void *out_h, size_t *coeff_len_or_null);
int lw_groth16_h_from_witness_device(const lw_r1cs_t *r1cs, const void *d_w, size_t num_gates, void *d_out_h,
                                     size_t *coeff_len_or_null, void *hip_stream);

/* ---- Circle FFT over Mersenne31 (math/src/circle/: evaluate_cfft, interpolate_cfft, get_twiddles) ----
 * The transform between the 2^log2n coefficients of a polynomial in the basis {1, y, x, xy, 2x^2 - 1, ...} (coefficient k
 * multiplies y^(k & 1) * prod_t pi^t(x)^(bit t+1 of k), pi(x) = 2x^2 - 1) and its values on the standard coset
 * g_{2n} + i g_n, i = 0 .. n-1 in that order, of the circle group over p = 2^31 - 1 (polynomial.rs:18-72).  Mersenne31 only,
 * one u32 per element and no Montgomery form, so no lw_field_t / lw_layout_t.  Every input word is read as from_base_type
 * reads it, (w & p) + (w >> 31): any u32 is accepted and p means 0.  Every output word is the canonical residue (< p), which
 * is what the reference's PartialEq compares.
 *   log2n      1 .. 30 (g_{2n} must exist in a group of order 2^31); 0: LW_ERR_BAD_ARG; above 30: LW_ERR_ORDER_TOO_LARGE
 *   batch      columns of n words, batch_stride words apart (0: n); the words between two columns are not touched
 *   in place   out == in is allowed; any other overlap of the two is LW_ERR_BAD_ARG, like a NULL pointer, batch = 0 and a
 *              stride below n.  All of this is decided before any device work.
 * interpolate_cfft includes the factor n^-1.  The twiddle tables are generated on the device and cached (the x-layers once
 * for every size, the y-layer per size); both permutations of each direction are folded into the first and last pass.
 * The reference's own evaluate_cfft stops at 2^8 points (Coset::get_coset_points keeps the size in a u8). */
int lw_circle_evaluate_cfft(const uint32_t *coeffs, uint32_t *out, uint32_t log2n, uint32_t batch, size_t batch_stride);
int lw_circle_interpolate_cfft(const uint32_t *evals, uint32_t *out, uint32_t log2n, uint32_t batch, size_t batch_stride);
int lw_circle_evaluate_cfft_device(const uint32_t *d_in, uint32_t *d_out, uint32_t log2n, uint32_t batch, size_t batch_stride,
                                   void *hip_stream);
int lw_circle_interpolate_cfft_device(const uint32_t *d_in, uint32_t *d_out, uint32_t log2n, uint32_t batch, size_t batch_stride,
                                      void *hip_stream);
/* out = evaluate_cfft(zero_pad(interpolate_cfft(evals), 2^log2_out)) per column: the basis does not depend on n, so zero
 * padding is the embedding into the larger domain.  The coefficients stay on the device, the padding is never written and
 * the evaluation layers that would only meet it are skipped.  log2_out < log2_in: LW_ERR_BAD_ARG; log2_out = log2_in
 * returns the input reduced mod p.  Strides in words, 0: dense. */
int lw_circle_lde_device(const uint32_t *d_evals, uint32_t log2_in, size_t in_stride, uint32_t *d_out, uint32_t log2_out,
                         size_t out_stride, uint32_t batch, void *hip_stream);
/* get_twiddles(Coset::new_standard(log2n), config) (twiddles.rs:13-58), the layers concatenated: n - 1 words to host memory.
 * config 0 (Evaluation): lengths 1, 2, .., n/2; config 1 (Interpolation): the inverses, lengths n/2, .., 1. */
int lw_circle_get_twiddles(uint32_t log2n, int config, uint32_t *out);

/* ---- NTT over Goldilocks, p = 2^64 - 2^32 + 1 (U64TestField, u64_test_field.rs:98-104; Felt, winterfell.rs:21-24) ----
 * One u64 per element in host byte order, the residue itself: no Montgomery form, no lw_field_t / lw_layout_t.  Every input
 * word is read as from_base_type reads it (any u64, x >= p means x - p); every output word is the canonical residue (< p).
 *   forward   out[i] = sum_j in[j] (h w^i)^j         evaluate_fft / evaluate_offset_fft (fft/polynomial.rs:25-82) on a slice
 *                                                     that is already a power of two; w the primitive 2^log2n-th root, h the
 *                                                     offset or 1
 *   inverse   out[j] = h^-j n^-1 sum_i in[i] w^-ij   interpolate_fft / interpolate_offset_fft (fft/polynomial.rs:87-127)
 * Input and output are in natural order.  The transform is linear: elements kept in Montgomery form with R = 2^64
 * (U64GoldilocksPrimeField, Winterfell's BaseElement) come out in Montgomery form, provided the offset is passed as the
 * plain residue.
 *   two_adic_root   the primitive 2^32-th root g; the primitive 2^k-th root is g^(2^(32-k)) (traits.rs:82-94).  0 selects
 *                   the reference's TWO_ADIC_PRIMITVE_ROOT_OF_UNITY = 1753635133440165772 = 7^((p-1)/2^32); any other value
 *                   must be below p with g^(2^31) = p - 1, else LW_ERR_ROOT_OF_UNITY (a Winterfell-style Felt passes its own
 *                   constant).  The twiddle tables are generated on the device and cached for one root at a time.
 *   offset_or_null  one u64 in host memory, or NULL; a value = 0 mod p is LW_ERR_INV_ZERO in both directions
 *   log2n           0 .. 30 (0: the reduced copy); 31 and 32: LW_ERR_ORDER_TOO_LARGE (32-bit word indices, a table of 2^(n-1)
 *                   entries); above 32: LW_ERR_ROOT_OF_UNITY, the reference's error above TWO_ADICITY
 *   batch           columns of n words, batch_stride words apart (0: n); the words between two columns are not touched
 *   in place        out == in is allowed; any other overlap is LW_ERR_BAD_ARG, like a NULL pointer, batch = 0, a stride below
 *                   the column length and an unknown dir.  All of this is decided before any device work.
 * Stream and lane contract of the _device forms as for the other *_device entry points. */
int lw_goldilocks_ntt(lw_dir_t dir, const uint64_t *in, uint64_t *out, uint32_t log2n, uint32_t batch, size_t batch_stride,
                      const uint64_t *offset_or_null, uint64_t two_adic_root);
int lw_goldilocks_ntt_device(lw_dir_t dir, const uint64_t *d_in, uint64_t *d_out, uint32_t log2n, uint32_t batch,
                             size_t batch_stride, const uint64_t *offset_or_null, uint64_t two_adic_root, void *hip_stream);
/* evaluate_offset_fft(poly, blowup, Some(domain), offset): the forward transform of the 2^log2_coeffs coefficients zero
 * padded to 2^log2n, per column.  The padding is never written or read and the stages that would only meet it are skipped.
 * log2_coeffs > log2n and any overlap of the two buffers: LW_ERR_BAD_ARG.  Strides in words, 0: dense. */
int lw_goldilocks_lde_device(const uint64_t *d_coeffs, uint32_t log2_coeffs, size_t in_stride, uint64_t *d_out, uint32_t log2n,
                             size_t out_stride, uint32_t batch, const uint64_t *offset_or_null, uint64_t two_adic_root,
                             void *hip_stream);
/* get_twiddles(order, config) (fft/cpu/roots_of_unity.rs:66-75): 2^order / 2 words to host memory.  config is RootsConfig
 * as in lw_hip_gen_twiddles: 0 Natural, 1 NaturalInversed, 2 BitReverse, 3 BitReverseInversed.  order as log2n above. */
int lw_goldilocks_gen_twiddles(uint64_t order, int config, uint64_t two_adic_root, uint64_t *out);
/* out[i] = a[i] b[i] mod p, the step between evaluate_fft and interpolate_fft of a polynomial product.  Words as above.
 * d_out == d_a and d_out == d_b are allowed, any other overlap of d_out with an operand is LW_ERR_BAD_ARG. */
int lw_goldilocks_mul_device(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t n, void *hip_stream);

/* ---- Rescue Prime Optimized over Goldilocks (RescuePrimeOptimized, crypto/src/hash/rescue_prime/; ePrint 2022/1577) ----
 * The permutation, the sponge `hash` of the reference and a Merkle tree built from it, batched: one work-item per
 * permutation.  Words are Goldilocks elements as above: one u64, the residue itself; every input word is read as
 * from_base_type reads it (any u64), every output word is the canonical residue.
 *   level   LW_RPO_128: state 12, capacity 4, rate 8, digest 4 words (the hash of Miden);
 *           LW_RPO_160: state 16, capacity 6, rate 10, digest 5 words.  Anything else: LW_ERR_BAD_ARG.
 *   permute n states of 12 (16) words -> n states (permutation(), rescue_prime_optimized.rs:192-202); out may be states
 *   hash    n_rows rows of row_len >= 0 words -> one digest of rate / 2 words each (hash(), :205-230): word 0 of the state is
 *           1 iff row_len is no multiple of the rate, every block overwrites the rate part, a partial last block is
 *           padded with a 1 and zeros; row_len = 0 runs no permutation and gives zeros (rows may then be NULL).  The host
 *           form reads dense row-major rows; the _device form rows row_stride words apart (0: row_len; below row_len:
 *           LW_ERR_BAD_ARG).  hash_bytes of the reference is bytes_to_field_elements on the host, then this.
 * Each function has a host form (buffers in host memory, complete on return, no CPU fallback) and a _device form (16-byte
 * aligned device pointers, work enqueued on hip_stream; misaligned: LW_ERR_BAD_ARG).  n = 0 / n_rows = 0: LW_OK, nothing is
 * touched and no device is needed.  More than 2^36 inputs: LW_ERR_ALLOC.  Every check happens before any device work.
 *
 * commit_columns: the tree over the 2^log2n rows of n_cols columns of words.  Leaf j = hash(committed row j over all
 * columns), a node = hash(left || right) (2 digests = one block: one permutation; for LW_RPO_128 this is Miden's 2-to-1
 * merge).  The reference has no RPO Merkle backend: this tree is built from its hash in the layout of its other trees.
 * nodes: (2 * 2^log2n - 1) digests, root first and leaves last (merkle_tree/utils.rs:43-71); for LW_RPO_128 a digest is 32
 * bytes and lw_stark_open_trees_device reads the authentication paths of such a tree as it is (d_columns = NULL).  out_root:
 * one digest.  bit_reverse and col_stride (in words, 0: dense, below 2^log2n: LW_ERR_BAD_ARG) as in the other commit calls:
 * leaf j commits natural row bitrev(j), gathered in the leaf kernel.  log2n 0 .. 30, above: LW_ERR_ALLOC.  The _device form
 * synchronises the stream only when out_root is not NULL. */
typedef enum { LW_RPO_128 = 0, LW_RPO_160 = 1 } lw_rpo_level_t;
int lw_rpo_permute(lw_rpo_level_t level, const uint64_t *states, size_t n, uint64_t *out);
int lw_rpo_permute_device(lw_rpo_level_t level, const uint64_t *d_states, size_t n, uint64_t *d_out, void *hip_stream);
int lw_rpo_hash(lw_rpo_level_t level, const uint64_t *rows, size_t n_rows, size_t row_len, uint64_t *out);
int lw_rpo_hash_device(lw_rpo_level_t level, const uint64_t *d_rows, size_t n_rows, size_t row_len, size_t row_stride,
                       uint64_t *d_out, void *hip_stream);
int lw_rpo_commit_columns(lw_rpo_level_t level, const uint64_t *columns, uint32_t n_cols, uint32_t log2n, int bit_reverse,
                          uint64_t *out_root, uint64_t *out_nodes_or_null);
int lw_rpo_commit_columns_device(lw_rpo_level_t level, const uint64_t *d_columns, uint32_t n_cols, uint64_t col_stride,
                                 uint32_t log2n, int bit_reverse, uint64_t *d_nodes, uint64_t *out_root_or_null, void *hip_stream);

/* ---- The quadratic extension of Goldilocks, Fp2 = F_p[t] / (t^2 - 7), and the prover steps that run in it ----
 * Goldilocks64ExtensionField (math/src/field/fields/u64_goldilocks_field.rs:219-227 over extensions/quadratic.rs:79-118;
 * also Plonky2's quadratic extension): what a STARK over Goldilocks needs after round 1 - out-of-domain evaluation, the
 * DEEP composition and the FRI commit phase (fri::commit_phase<F, E>, provers/stark/src/fri/mod.rs:22-75, with F
 * Goldilocks and E = Fp2).  Together with lw_goldilocks_lde_device and lw_rpo_commit_columns_device the Goldilocks path
 * runs LDE -> RPO commit -> OOD -> DEEP -> FRI commit phase on data that stays in device memory.
 *   word            as in the Goldilocks section: one u64, the residue itself; any u64 is accepted on input, every
 *                   output word is canonical (< p)
 *   Fp2 element     a = a0 + a1 t, t^2 = 7
 *   host scalar     uint64_t[2] = {c0, c1}: the challenge, the points, the weights and the returned values
 *   device vector   n elements are two PLANES of n words: plane c0, then plane c1 `stride` words later.  A stride of 0
 *                   means n; a stride below n is LW_ERR_BAD_ARG.  This is the batch / batch_stride shape of
 *                   lw_goldilocks_ntt_device and the n_cols / col_stride shape of lw_rpo_commit_columns_device: an Fp2
 *                   vector goes through them with batch = 2 / n_cols = 2 as it is (the twiddles are in F, so an Fp2
 *                   transform over a base-field domain is two base transforms).  There is no interleaved form.
 * All entry points are _device forms under the stream and lane contract of the other *_device calls.  Device pointers
 * must be 16-byte aligned (else LW_ERR_BAD_ARG).  Every argument check runs before any device work; n = 0 returns LW_OK
 * without a device.  A call that hands a small result to the host (values, a root) waits for the stream; the others only
 * enqueue.
 *
 * pointwise: out[i] = a[i] b[i] (LW_GL2_MUL), a[i]^2 (LW_GL2_SQR), a[i]^-1 (LW_GL2_INV), a[i] b[i] with b in F
 * (LW_GL2_MUL_BASE: d_b is a single plane, b_stride is not read).  d_b is not read for SQR and INV and may be NULL.
 * d_out == d_a or d_out == d_b (the whole vector, under the same stride) is allowed; any other overlap of d_out with an
 * operand, like an unknown op, is LW_ERR_BAD_ARG.  The inverse of 0 is written as 0: the reference returns InvZeroError
 * there, and 0 is the only element without an inverse (its norm a0^2 - 7 a1^2 vanishes only at 0, 7 being a non-residue).
 *
 * evaluate (STARK round 3): out_values[k m + j] = sum_i col_k[i] points[j]^i for n_cols base-field coefficient columns
 * of n_coeffs words each, col_stride words apart, at m points of Fp2; out_values is host memory, n_cols m scalars.  A
 * polynomial with Fp2 coefficients is its two planes passed as two columns, its value v0 + t v1.  No cap on n_cols or m.
 * n_coeffs = 0 gives zeros.
 *
 * deep_quotients: the DEEP composition polynomial (compute_deep_composition_poly, provers/stark/src/prover.rs:643-714,
 * over a weight matrix as lw_stark_deep_composition states it) in evaluation form.  For every row i of the LDE domain,
 * x_i = h w^i in natural order, w the primitive 2^log2n-th root:
 *     out[i] = sum_j ( sum_k weights[k][j] (col_k[i] - evals[k][j]) ) / (x_i - points[j])
 * d_lde: n_cols base-field columns of 2^log2n words, col_stride apart.  points: m scalars; weights, evals: n_cols x m
 * scalars, row k, column j (host).  A zero weight skips its pair.  A part with Fp2 values is its two planes as two columns,
 * the weight of the c1 plane multiplied by t by the caller.  A point with c1 = 0 is LW_ERR_BAD_ARG: a base-field point can
 * lie on the domain.  offset_or_null (h, NULL: 1; 0 mod p: LW_ERR_INV_ZERO), two_adic_root and the range of log2n as
 * in lw_goldilocks_ntt_device.  d_out: an Fp2 vector of 2^log2n elements that overlaps no column.  n_cols = 0 or m = 0:
 * LW_ERR_BAD_ARG.  lw_goldilocks_ntt_device (inverse, same offset, batch = 2) of the result gives the coefficients of
 * the DEEP polynomial.
 *
 * fri_layer: the Fp2 counterpart of lw_stark_fri_layer_device (fri/mod.rs:44-58, 115-141).
 *   fold        d_out_poly[i] = 2 (c[2i] + zeta c[2i+1]), the odd term absent past n_coeffs, as a zero-padded block of
 *               max(2, next_pow2(ceil(n_coeffs / 2))) elements in two DENSE planes: the next layer's d_coeffs
 *   fold only   d_nodes_or_null == NULL (the last step, whose coefficient 0 is the value sent); an evaluation or a root
 *               asked for without nodes is LW_ERR_BAD_ARG
 *   evaluation  d_out_evaluation receives evaluate_offset_fft(p', 1, Some(domain_size), offset) in natural order, two dense
 *               planes of domain_size words.  offset_or_null is the layer's offset in F (already squared by the caller),
 *               domain_size the layer's domain (already halved).  NULL with nodes: LW_ERR_BAD_ARG
 *   tree        domain_size / 2 leaves; leaf j is the RPO hash (level as in lw_rpo_hash) of the four words (a.c0, a.c1,
 *               b.c0, b.c1) of a = e[i], b = e[i + domain_size / 2], i = bitrev(j) over log2(domain_size) - 1 bits - the
 *               reference's chunks of two of the bit-reversed vector; a node is the 2-to-1 hash of lw_rpo_commit_columns.
 *               d_nodes: (domain_size - 1) digests, root first; lw_stark_open_trees_device reads an LW_RPO_128 tree as it
 *               is.  out_root_or_null: one digest to host memory.
 *   errors      domain_size not a power of two: LW_ERR_INPUT_NOT_POW2; below the block length, d_out_poly overlapping
 *               d_coeffs (or any two buffers of the layer overlapping), an unknown level: LW_ERR_BAD_ARG */
typedef enum { LW_GL2_MUL = 0, LW_GL2_SQR = 1, LW_GL2_INV = 2, LW_GL2_MUL_BASE = 3 } lw_gl2_op_t;
int lw_goldilocks_ext2_pointwise_device(lw_gl2_op_t op, const uint64_t *d_a, size_t a_stride, const uint64_t *d_b, size_t b_stride,
                                        uint64_t *d_out, size_t out_stride, size_t n, void *hip_stream);
int lw_goldilocks_ext2_evaluate_device(const uint64_t *d_coeffs, uint32_t n_cols, size_t col_stride, size_t n_coeffs,
                                       const uint64_t *points, uint32_t m, uint64_t *out_values, void *hip_stream);
int lw_goldilocks_ext2_deep_quotients_device(const uint64_t *d_lde, uint32_t n_cols, size_t col_stride, uint32_t log2n,
                                             const uint64_t *offset_or_null, uint64_t two_adic_root, const uint64_t *points,
                                             uint32_t m, const uint64_t *weights, const uint64_t *evals, uint64_t *d_out,
                                             size_t out_stride, void *hip_stream);
int lw_goldilocks_ext2_fri_layer_device(const uint64_t *d_coeffs, size_t coeff_stride, size_t n_coeffs, const uint64_t *zeta,
                                        const uint64_t *offset_or_null, size_t domain_size, uint64_t two_adic_root,
                                        lw_rpo_level_t level, uint64_t *d_out_poly, uint64_t *d_out_evaluation_or_null,
                                        uint64_t *d_nodes_or_null, uint64_t *out_root_or_null, void *hip_stream);

/* ---- The quartic extension of BabyBear, Fp4 = F_p[x] / (x^4 + 11), and the prover steps that run in it ----
 * Degree4BabyBearExtensionField (math/src/field/fields/fft_friendly/quartic_babybear.rs; RISC Zero's extension): what a
 * STARK over BabyBear needs after round 1 - out-of-domain evaluation, the DEEP composition and the FRI commit phase
 * (fri::commit_phase<F, E>, provers/stark/src/fri/mod.rs:22-75, with F BabyBear and E = Fp4).  Together with
 * lw_hip_ntt_lde_device and lw_stark_commit_columns_layout_device the BabyBear path runs LDE -> Keccak commit -> OOD ->
 * DEEP -> FRI commit phase on data that stays in device memory.
 *   word            one uint32_t, the stored Montgomery value with R = 2^32, canonical (< p = 2013265921): exactly
 *                   LW_LAYOUT_BABYBEAR_U32_R32.  Inputs must be canonical; every output word is canonical.
 *   Fp4 element     a = a0 + a1 x + a2 x^2 + a3 x^3, x^4 = -11
 *   host scalar     uint32_t[4] = {c0, c1, c2, c3}, stored words: the challenge, the points, the weights and the returned
 *                   values.  A host scalar word >= p is LW_ERR_BAD_ARG.
 *   device vector   n elements are four PLANES of n words: c0, then c1 `stride` words later, and so on.  A stride of 0
 *                   means n; a stride below n is LW_ERR_BAD_ARG.  This is the batch shape of lw_hip_ntt_device /
 *                   lw_hip_ntt_lde_device and the n_cols / col_stride shape of lw_stark_commit_columns_layout_device: an
 *                   Fp4 vector goes through them with batch = 4 / n_cols = 4 as it is (the twiddles are in F, so an Fp4
 *                   transform over a base-field domain is four base transforms).  LW_LAYOUT_EXT4_INTERLEAVED stays the
 *                   NTT-only layout it is; convert (below) is the bridge to it.
 * All entry points are _device forms under the stream and lane contract of the other *_device calls.  Device pointers
 * must be 16-byte aligned (else LW_ERR_BAD_ARG).  Every argument check runs before any device work; n = 0 returns LW_OK
 * without a device.  A call that hands a small result to the host (values, a root) waits for the stream; the others only
 * enqueue.
 *
 * pointwise: out[i] = a[i] b[i] (LW_BB4_MUL), a[i]^2 (LW_BB4_SQR), a[i]^-1 (LW_BB4_INV), a[i] b[i] with b in F
 * (LW_BB4_MUL_BASE: d_b is a single plane, b_stride is not read).  d_b is not read for SQR and INV and may be NULL.
 * d_out == d_a or d_out == d_b (the whole vector, under the same stride) is allowed; any other overlap of d_out with an
 * operand, like an unknown op, is LW_ERR_BAD_ARG.  The inverse of 0 is written as 0: the reference returns an error
 * there, and 0 is the only element without an inverse (x^4 + 11 is irreducible).
 *
 * convert: LW_BB4_TO_PLANES reads n elements of LW_LAYOUT_EXT4_INTERLEAVED from d_interleaved (four u64 words per
 * element, each a 2^64 mod p, below p) and writes four planes of stored u32 words to d_planes, plane_stride apart;
 * LW_BB4_TO_INTERLEAVED is the way back.  The two buffers must not overlap; an unknown direction is LW_ERR_BAD_ARG.
 *
 * evaluate (STARK round 3): out_values[k m + j] = sum_i col_k[i] points[j]^i for n_cols base-field coefficient columns
 * of n_coeffs words each, col_stride words apart, at m points of Fp4; out_values is host memory, n_cols m scalars.  A
 * polynomial with Fp4 coefficients is its four planes passed as four columns, its value sum_e x^e v_e.  No cap on n_cols
 * or m.  n_coeffs = 0 gives zeros.
 *
 * deep_quotients: the DEEP composition polynomial (compute_deep_composition_poly, provers/stark/src/prover.rs:643-714,
 * over a weight matrix as lw_stark_deep_composition states it) in evaluation form.  For every row i of the LDE domain,
 * x_i = h w^i in natural order, w the library's primitive 2^log2n-th root of BabyBear (log2n > 24: LW_ERR_ROOT_OF_UNITY):
 *     out[i] = sum_j ( sum_k weights[k][j] (col_k[i] - evals[k][j]) ) / (x_i - points[j])
 * d_lde: n_cols base-field columns of 2^log2n words, col_stride apart.  points: m scalars; weights, evals: n_cols x m
 * scalars, row k, column j (host).  A zero weight skips its pair.  A part with Fp4 values is its four planes as four
 * columns, the weight of plane e multiplied by x^e by the caller.  A point whose c1, c2 and c3 are all zero is
 * LW_ERR_BAD_ARG: a base-field point can lie on the domain.  offset_or_null: h as one stored word (NULL: 1; 0:
 * LW_ERR_INV_ZERO).  d_out: an Fp4 vector of 2^log2n elements that overlaps no column.  n_cols = 0 or m = 0:
 * LW_ERR_BAD_ARG.  lw_hip_ntt_device (inverse, same offset, batch = 4) of the result gives the coefficients of the DEEP
 * polynomial.
 *
 * fri_layer: the Fp4 counterpart of lw_stark_fri_layer_device (fri/mod.rs:44-58, 115-141).
 *   fold        d_out_poly[i] = 2 (c[2i] + zeta c[2i+1]), the odd term absent past n_coeffs, as a zero-padded block of
 *               max(2, next_pow2(ceil(n_coeffs / 2))) elements in four DENSE planes: the next layer's d_coeffs
 *   fold only   d_nodes_or_null == NULL (the last step, whose coefficient 0 is the value sent); an evaluation or a root
 *               asked for without nodes is LW_ERR_BAD_ARG
 *   evaluation  d_out_evaluation receives evaluate_offset_fft(p', 1, Some(domain_size), offset) in natural order, four
 *               dense planes of domain_size words.  offset_or_null is the layer's offset in F (already squared by the
 *               caller), domain_size the layer's domain (already halved).  NULL with nodes: LW_ERR_BAD_ARG
 *   tree        Keccak-256, domain_size / 2 leaves; leaf j hashes the 32 bytes a.c0 a.c1 a.c2 a.c3 b.c0 b.c1 b.c2 b.c3, every
 *               word big-endian (U32MontgomeryBackendPrimeField::as_bytes), of a = e[i], b = e[i + domain_size / 2],
 *               i = bitrev(j) over log2(domain_size) - 1 bits - the reference's chunks of two of the bit-reversed vector
 *               in a BatchedMerkleTree; a node is the 2-to-1 hash of lw_stark_commit_columns.  d_nodes:
 *               (domain_size - 1) x 32 bytes, root first; lw_stark_open_trees_device reads the tree as it is.
 *               out_root_or_null: 32 bytes to host memory.
 *   errors      domain_size not a power of two: LW_ERR_INPUT_NOT_POW2; above 2^24: LW_ERR_ROOT_OF_UNITY; below the block
 *               length, d_out_poly overlapping d_coeffs (or any two buffers of the layer overlapping): LW_ERR_BAD_ARG */
typedef enum { LW_BB4_MUL = 0, LW_BB4_SQR = 1, LW_BB4_INV = 2, LW_BB4_MUL_BASE = 3 } lw_bb4_op_t;
typedef enum { LW_BB4_TO_PLANES = 0, LW_BB4_TO_INTERLEAVED = 1 } lw_bb4_convert_t;
int lw_babybear_ext4_pointwise_device(lw_bb4_op_t op, const uint32_t *d_a, size_t a_stride, const uint32_t *d_b, size_t b_stride,
                                      uint32_t *d_out, size_t out_stride, size_t n, void *hip_stream);
int lw_babybear_ext4_convert_device(lw_bb4_convert_t dir, uint64_t *d_interleaved, uint32_t *d_planes, size_t plane_stride, size_t n,
                                    void *hip_stream);
int lw_babybear_ext4_evaluate_device(const uint32_t *d_coeffs, uint32_t n_cols, size_t col_stride, size_t n_coeffs,
                                     const uint32_t *points, uint32_t m, uint32_t *out_values, void *hip_stream);
int lw_babybear_ext4_deep_quotients_device(const uint32_t *d_lde, uint32_t n_cols, size_t col_stride, uint32_t log2n,
                                           const uint32_t *offset_or_null, const uint32_t *points, uint32_t m,
                                           const uint32_t *weights, const uint32_t *evals, uint32_t *d_out, size_t out_stride,
                                           void *hip_stream);
int lw_babybear_ext4_fri_layer_device(const uint32_t *d_coeffs, size_t coeff_stride, size_t n_coeffs, const uint32_t *zeta,
                                      const uint32_t *offset_or_null, size_t domain_size, uint32_t *d_out_poly,
                                      uint32_t *d_out_evaluation_or_null, uint8_t *d_nodes_or_null, uint8_t *out_root_or_null,
                                      void *hip_stream);

/* ---- STARK round 2 over Goldilocks with Fp2 and over BabyBear with Fp4: the composition polynomial ----
 * round_2_compute_composition_polynomial (provers/stark/src/prover.rs:428-484) for a trace in a small field F whose random
 * coefficients are in the extension E: ConstraintEvaluator::evaluate with the AIR's compute_transition given as a program,
 * then interpolate_offset_fft, break_in_parts and the LDE of the parts.  Words, host scalars, planes and strides (0: dense),
 * the 16-byte alignment of device pointers, offset_or_null and (Goldilocks only) two_adic_root are those of the two
 * extension sections above.  Every argument check runs before any device work.  _device forms only.
 *
 * constraint_evaluations: ONE pass over the LDE columns, no row T_c is ever stored.  n = 2^log2_trace, N = n 2^log2_blowup,
 * g and w the library's primitive n-th and N-th roots of F, h the offset, x_i = h w^i.  For every LDE row i in [0, N):
 *     out[i] = sum_c coeff_c ( Z_c[i] T_c(i) )  +  sum_k coeff_k (col_k[i] - value_k) / (x_i - g^step_k)        (in E)
 *   T_c(i)   what the program emits for constraint c at row i: ops, the accumulator machine with its 8 temporaries, the
 *            CELL addressing col[(i + row 2^log2_blowup) mod len_col], the short (periodic) columns of
 *            col_log2_len_or_null and the host check are exactly those of lw_stark_transition_evaluations_device.  Cells
 *            and constants are words of F: Goldilocks words are any u64, canonicalised on load; BabyBear words and
 *            constants must be below p (a constant that is not: LW_ERR_BAD_ARG; device words are the caller's promise).
 *            Extension-valued (auxiliary) columns and constants: the _rap_ entry points below.
 *   Z_c[i]   the zerofier of lw_stark_constraint_evaluations_device, in F: cycle_c[i mod len_c] times the product of
 *            (x_i - g^(n - k period)) over k = 1 .. end_exemptions, both cycle branches and the truncating divisions.
 *            The cycle tables are built on the device.  Transitions whose five integers are all equal share one table and
 *            one value per row; a call takes at most 8 distinct descriptors (more: LW_ERR_BAD_ARG).
 *   coeff    one scalar of E per transition and per boundary constraint; value is one word of F.
 *   d_columns  host array of n_cols device pointers; column c has N words (2^col_log2_len[c] for a short one; a boundary
 *            constraint on a short column is LW_ERR_BAD_ARG).  d_out: an E vector of N elements, out_stride apart, that
 *            overlaps no column; the words between two planes are not written.
 * No denominator is zero unless h^N = 1 (a zero x^(n / period) - g^(...) or x - g^step forces x^n = 1), so nothing is
 * looked for on the device: h^N = 1 with any constraint present, a NULL offset included, is LW_ERR_INV_ZERO from the
 * host (a period that does not divide n is refused the same way where its truncated exponent allows a zero).  h = 0 mod p
 * is LW_ERR_INV_ZERO as in the LDE calls.  The call only enqueues.  LW_ERR_BAD_ARG: period = 0, end_exemptions * period > n,
 * col >= n_cols, a domain beyond the field's transform (2^30 for Goldilocks, 2^24 for BabyBear), a null or misaligned buffer,
 * a malformed program (lw_hip_last_error names the op).  n_boundary = 0 or n_transitions = 0 is legal; both: zeros.
 *
 * composition_parts: the counterpart of lw_stark_composition_parts_device.  H = interpolate_offset_fft(d_evals, h) plane
 * by plane; part j takes coefficients j, j + P, ... into a zero-padded block of L = next_power_of_two(ceil(N / P))
 * elements; every part is evaluated at x_0 .. x_{N-1}.  Part j, plane e lies at plane index j D + e (D = 2 or 4) in both
 * outputs: d_parts_coeffs is P D dense planes of L words, d_parts_lde_or_null P D dense planes of N words - the
 * n_cols = P D shape of lw_rpo_commit_columns_device / lw_stark_commit_columns_layout_device, whose column commitment over
 * these planes is the commitment of round 2, and the "part as D columns" shape of evaluate and deep_quotients.
 * out_part_lens_or_null: per part the last index where any plane is not zero, plus one; asking for it synchronises.
 * 1 <= n_parts <= N, else LW_ERR_BAD_ARG, like buffers that overlap.  d_evals is not modified. */
typedef struct {
    uint32_t col, reserved;
    uint64_t step;
    uint64_t value;
    uint64_t coeff[2];
} lw_gl2_boundary_t;
typedef struct {
    uint64_t period, offset, end_exemptions;
    uint64_t exemptions_period; /* 0: none */
    uint64_t periodic_exemptions_offset;
    uint64_t coeff[2];
} lw_gl2_transition_t;
typedef struct {
    uint32_t col, reserved;
    uint64_t step;
    uint32_t value;
    uint32_t coeff[4];
    uint32_t reserved2;
} lw_bb4_boundary_t;
typedef struct {
    uint64_t period, offset, end_exemptions;
    uint64_t exemptions_period; /* 0: none */
    uint64_t periodic_exemptions_offset;
    uint32_t coeff[4];
} lw_bb4_transition_t;
int lw_goldilocks_ext2_constraint_evaluations_device(const lw_stark_air_op_t *ops, uint32_t n_ops, const uint64_t *consts,
                                                     uint32_t n_consts, const uint64_t *const *d_columns,
                                                     const uint32_t *col_log2_len_or_null, uint32_t n_cols, uint32_t log2_trace,
                                                     uint32_t log2_blowup, const uint64_t *offset_or_null, uint64_t two_adic_root,
                                                     const lw_gl2_boundary_t *boundary, uint32_t n_boundary,
                                                     const lw_gl2_transition_t *transitions, uint32_t n_transitions,
                                                     uint64_t *d_out, size_t out_stride, void *hip_stream);
int lw_goldilocks_ext2_composition_parts_device(const uint64_t *d_evals, size_t evals_stride, uint32_t log2_lde,
                                                const uint64_t *offset_or_null, uint64_t two_adic_root, uint32_t n_parts,
                                                uint64_t *d_parts_coeffs, uint64_t *d_parts_lde_or_null,
                                                size_t *out_part_lens_or_null, void *hip_stream);
int lw_babybear_ext4_constraint_evaluations_device(const lw_stark_air_op_t *ops, uint32_t n_ops, const uint32_t *consts,
                                                   uint32_t n_consts, const uint32_t *const *d_columns,
                                                   const uint32_t *col_log2_len_or_null, uint32_t n_cols, uint32_t log2_trace,
                                                   uint32_t log2_blowup, const uint32_t *offset_or_null,
                                                   const lw_bb4_boundary_t *boundary, uint32_t n_boundary,
                                                   const lw_bb4_transition_t *transitions, uint32_t n_transitions,
                                                   uint32_t *d_out, size_t out_stride, void *hip_stream);
int lw_babybear_ext4_composition_parts_device(const uint32_t *d_evals, size_t evals_stride, uint32_t log2_lde,
                                              const uint32_t *offset_or_null, uint32_t n_parts, uint32_t *d_parts_coeffs,
                                              uint32_t *d_parts_lde_or_null, size_t *out_part_lens_or_null, void *hip_stream);

/* ---- RAP over Fp2 and Fp4: the auxiliary column of round 1 and a round 2 that reads it ----
 * The randomized AIR with preprocessing (AIR::build_rap_challenges, AIR::build_auxiliary_trace, BoundaryConstraint::new_aux,
 * get_aux_evaluation_element) for a trace in F whose challenges are in E: the auxiliary column is in E, D planes of words
 * like every E vector here, so the LDE (batch = D), the column commitment (n_cols = D), evaluate and deep_quotients take it
 * as D base columns.  Words, host scalars (D words each), planes, strides and alignment as in the sections above.
 *
 * aux_fractions: one column from the n rows of base columns,
 *     f_i = (num_const + sum_j num_coeffs[j] col_{num_cols[j]}[i]) / (den_const + sum_j den_coeffs[j] col_{den_cols[j]}[i])
 *     LW_EXT_AUX_PRODUCT   out[i] = f_0 ... f_i      with LW_EXT_AUX_EXCLUSIVE  out[0] = 1, out[i] = f_0 ... f_{i-1}
 *     LW_EXT_AUX_SUM       out[i] = f_0 + ... + f_i  with LW_EXT_AUX_EXCLUSIVE  out[0] = 0, out[i] = f_0 + ... + f_{i-1}
 *   (the grand product of a permutation or memory argument, inclusive as in read_only_memory.rs or exclusive as in
 *   fibonacci_rap.rs, and a LogUp running sum).  d_columns: host array of n_cols device pointers to n words each; n >= 1 is
 *   any length.  A list has at most LW_EXT_AUX_MAX_TERMS terms and may be empty (its arrays may then be NULL); a numerator
 *   with no terms and the constant 1 costs no product.  d_out: D planes of n words, out_stride apart (0: n), the words
 *   between the planes are not written; it overlaps no column.  d_total_or_null: D consecutive words on the device, the
 *   product or the sum over all n rows (the last inclusive value).  out_zero_denominators_or_null: the number of rows
 *   whose denominator is zero; asking for it synchronises and a count that is not zero is LW_ERR_INV_ZERO.  With a zero
 *   denominator the contents of d_out and d_total are unspecified, asked for or not.  Without the pointer the call only
 *   enqueues.  Reduce-then-scan in three launches whatever n; no workgroup waits for another.
 *   Before any device work: n = 0, an unknown mode, more than 16 terms, a NULL table, col >= n_cols, a BabyBear scalar
 *   word not below p, a null or misaligned buffer, a stride below n, d_out overlapping a column: LW_ERR_BAD_ARG; n above
 *   2^36: LW_ERR_ALLOC.
 *
 * rap_constraint_evaluations: lw_*_constraint_evaluations_device with the same definition of out[i], where T_c and col_k
 * are in E where the program or the constraint says so.  The arguments of that call, and
 *   xconsts, n_xconsts     host scalars of E (D words each), at most LW_STARK_AIR_MAX_CONSTS: the operand XCONST
 *   d_aux_columns, n_aux   host array of device pointers, each to D planes of N words aux_stride apart (0: N): the operand
 *                          XCELL (column `index` at row offset `row`, addressed like CELL) and the boundary constraints
 *                          with is_aux set
 *   boundary               value is a scalar of E (BoundaryConstraints<FieldExtension>); non-zero high coordinates on a
 *                          main-column constraint are legal.  col indexes d_aux_columns where is_aux is not 0.
 * The host types every value of the (straight-line) program as F or E: an op on F operands runs the base-field
 * arithmetic of the call above, F with E is a product by a base word, E with E a product in E.  The typed interpreter's
 * loop is longer per op: a program with no E value at all was measured at 1.10 (Fp2) and 1.19 (Fp4) times the call above,
 * which remains the one to take for such a program.  A program without the two sources and
 * boundary values in F give the output of the call above bit for bit.  Further LW_ERR_BAD_ARG: an auxiliary column or
 * extension constant index out of range (lw_hip_last_error names the op or the constraint), a null or misaligned
 * auxiliary buffer, aux_stride below N, d_out overlapping an auxiliary column. */
#define LW_EXT_AUX_MAX_TERMS 16
typedef enum { LW_EXT_AUX_PRODUCT = 0, LW_EXT_AUX_SUM = 1, LW_EXT_AUX_EXCLUSIVE = 2 /* or-ed onto either */ } lw_ext_aux_mode_t;
typedef struct {
    uint32_t col, is_aux;
    uint64_t step;
    uint64_t value[2];
    uint64_t coeff[2];
} lw_gl2_rap_boundary_t;
typedef struct {
    uint32_t col, is_aux;
    uint64_t step;
    uint32_t value[4];
    uint32_t coeff[4];
} lw_bb4_rap_boundary_t;
int lw_goldilocks_ext2_aux_fractions_device(const uint64_t *const *d_columns, uint32_t n_cols, size_t n, const uint64_t *num_const,
                                            const uint32_t *num_cols, const uint64_t *num_coeffs, uint32_t n_num,
                                            const uint64_t *den_const, const uint32_t *den_cols, const uint64_t *den_coeffs,
                                            uint32_t n_den, uint32_t mode, uint64_t *d_out, size_t out_stride,
                                            uint64_t *d_total_or_null, uint64_t *out_zero_denominators_or_null, void *hip_stream);
int lw_babybear_ext4_aux_fractions_device(const uint32_t *const *d_columns, uint32_t n_cols, size_t n, const uint32_t *num_const,
                                          const uint32_t *num_cols, const uint32_t *num_coeffs, uint32_t n_num,
                                          const uint32_t *den_const, const uint32_t *den_cols, const uint32_t *den_coeffs,
                                          uint32_t n_den, uint32_t mode, uint32_t *d_out, size_t out_stride,
                                          uint32_t *d_total_or_null, uint64_t *out_zero_denominators_or_null, void *hip_stream);
int lw_goldilocks_ext2_rap_constraint_evaluations_device(const lw_stark_air_op_t *ops, uint32_t n_ops, const uint64_t *consts,
                                                         uint32_t n_consts, const uint64_t *xconsts, uint32_t n_xconsts,
                                                         const uint64_t *const *d_columns, const uint32_t *col_log2_len_or_null,
                                                         uint32_t n_cols, const uint64_t *const *d_aux_columns, uint32_t n_aux,
                                                         size_t aux_stride, uint32_t log2_trace, uint32_t log2_blowup,
                                                         const uint64_t *offset_or_null, uint64_t two_adic_root,
                                                         const lw_gl2_rap_boundary_t *boundary, uint32_t n_boundary,
                                                         const lw_gl2_transition_t *transitions, uint32_t n_transitions,
                                                         uint64_t *d_out, size_t out_stride, void *hip_stream);
int lw_babybear_ext4_rap_constraint_evaluations_device(const lw_stark_air_op_t *ops, uint32_t n_ops, const uint32_t *consts,
                                                       uint32_t n_consts, const uint32_t *xconsts, uint32_t n_xconsts,
                                                       const uint32_t *const *d_columns, const uint32_t *col_log2_len_or_null,
                                                       uint32_t n_cols, const uint32_t *const *d_aux_columns, uint32_t n_aux,
                                                       size_t aux_stride, uint32_t log2_trace, uint32_t log2_blowup,
                                                       const uint32_t *offset_or_null, const lw_bb4_rap_boundary_t *boundary,
                                                       uint32_t n_boundary, const lw_bb4_transition_t *transitions,
                                                       uint32_t n_transitions, uint32_t *d_out, size_t out_stride, void *hip_stream);

/* ---- Monolith over Mersenne31 (crypto/src/hash/monolith/: MonolithMersenne31<WIDTH, NUM_FULL_ROUNDS>, from Plonky3) ----
 * The permutation, batched (one work-item per state), and for width 16 a hash, a 2-to-1 compression and a Merkle tree
 * built from it.  Words are Mersenne31 elements as in the circle FFT: one u32; every input word is read mod p = 2^31 - 1
 * (any u32), every output word is the canonical residue.
 *   width    8, 12, 16, 20 or 24; rounds (NUM_FULL_ROUNDS) 1 .. 15, the reference tests 5.  Anything else: LW_ERR_BAD_ARG.
 *   permute  n states of `width` words -> n states (permutation(), mod.rs:91-102); out may be states
 *   hash     n_rows rows of row_len >= 0 words -> 8 words each.  Plonky3's PaddingFreeSponge<16, 8, 8> over the width-16
 *            permutation: the state starts as 16 zeros; every chunk of up to 8 words overwrites state[0 .. chunk length),
 *            the rest stays, then the state is permuted; the digest is state[0 .. 8).  row_len = 0 gives zeros and runs no
 *            permutation.  There is NO padding: rows of different lengths can collide ([a] and [a, 0] have the same
 *            digest), so the hash is only meant for rows of one fixed length, as a tree's leaves are.
 *            row_stride in words, 0: dense, below row_len: LW_ERR_BAD_ARG.
 *   compress n pairs of 8-word digests -> permute(left || right)[0 .. 8), Plonky3's TruncatedPermutation<2, 8, 16>
 * The reference ships the permutation only; the two modes are specified by the lines above.
 * NULL buffers and _device buffers that are not 16-byte aligned are LW_ERR_BAD_ARG once there is work; n = 0 (n_rows = 0)
 * touches nothing and needs no device.  More than 2^36 inputs: LW_ERR_ALLOC.  Every check happens before any device work.
 *
 * commit_columns: the tree over the 2^log2n rows of n_cols columns of words.  Leaf j = hash(committed row j over all
 * columns), a node = compress(left, right).  nodes: (2 * 2^log2n - 1) digests of 32 bytes, root first and leaves last
 * (merkle_tree/utils.rs:43-71): lw_stark_open_trees_device reads the authentication paths of such a tree as it is
 * (d_columns = NULL).  bit_reverse, col_stride (in words), log2n 0 .. 30 and the synchronisation as lw_rpo_commit_columns.
 *
 * constants: the round constants (rounds x width words) and the matrix of Concrete (width x width words, row-major; for
 * width 16 the circulant written out) of one instance, generated from their SHAKE128 rule (mod.rs:47-55, 109-116).  No device.
 * layer_device: a test seam.  One layer per state, through the function the permutation inlines: words are read mod p,
 * the layer is applied, canonical words are written.  Bars changes the first 8 words of a state. */
typedef enum { LW_MONOLITH_CONCRETE = 0, LW_MONOLITH_BARS = 1, LW_MONOLITH_BRICKS = 2 } lw_monolith_layer_t;
int lw_monolith_permute(uint32_t width, uint32_t rounds, const uint32_t *states, size_t n, uint32_t *out);
int lw_monolith_permute_device(uint32_t width, uint32_t rounds, const uint32_t *d_states, size_t n, uint32_t *d_out, void *hip_stream);
int lw_monolith_hash(uint32_t rounds, const uint32_t *rows, size_t n_rows, size_t row_len, uint32_t *out);
int lw_monolith_hash_device(uint32_t rounds, const uint32_t *d_rows, size_t n_rows, size_t row_len, size_t row_stride, uint32_t *d_out,
                            void *hip_stream);
int lw_monolith_compress(uint32_t rounds, const uint32_t *left, const uint32_t *right, size_t n, uint32_t *out);
int lw_monolith_compress_device(uint32_t rounds, const uint32_t *d_left, const uint32_t *d_right, size_t n, uint32_t *d_out,
                                void *hip_stream);
int lw_monolith_commit_columns(uint32_t rounds, const uint32_t *columns, uint32_t n_cols, uint32_t log2n, int bit_reverse,
                               uint32_t *out_root, uint32_t *out_nodes_or_null);
int lw_monolith_commit_columns_device(uint32_t rounds, const uint32_t *d_columns, uint32_t n_cols, uint64_t col_stride, uint32_t log2n,
                                      int bit_reverse, uint32_t *d_nodes, uint32_t *out_root_or_null, void *hip_stream);
int lw_monolith_constants(uint32_t width, uint32_t rounds, uint32_t *out_round_constants, uint32_t *out_mds);
int lw_monolith_layer_device(uint32_t width, uint32_t rounds, lw_monolith_layer_t layer, const uint32_t *d_states, size_t n,
                             uint32_t *d_out, void *hip_stream);

/* ---- The quartic extension of Mersenne31 and the circle-STARK prover steps that run in it ----
 * CM31 = F_p[i] / (i^2 + 1) and QM31 = CM31[u] / (u^2 - (2 + i)), Degree2ExtensionField / Degree4ExtensionField of
 * math/src/field/fields/mersenne31/extensions.rs (mul, square, inv as there), with out-of-domain evaluation, the DEEP
 * quotients and the circle FRI fold with its layer commitment.  Together with lw_circle_lde_device and
 * lw_monolith_commit_columns_device the Mersenne31 path runs LDE -> commit -> OOD -> DEEP -> FRI commit phase on data that
 * stays in device memory.
 *   word            one uint32_t as in the circle FFT: any word is accepted and read as (w & p) + (w >> 31), every word
 *                   handed back is the canonical residue
 *   QM31 element    (c0 + c1 i) + (c2 + c3 i) u, the order of to_subfield_vec.  sigma(c0, c1, c2, c3) = (c0, c1, -c2, -c3).
 *   host scalar     uint32_t[4] = {c0, c1, c2, c3}; a point (X, Y) of QM31^2 is uint32_t[8], X first
 *   device vector   n elements are four PLANES of n words, c0, then c1 `stride` words later, and so on (0: n; below n:
 *                   LW_ERR_BAD_ARG): the batch = 4 shape of lw_circle_*_device and the n_cols = 4 shape of
 *                   lw_monolith_commit_columns_device
 *   domain          the standard coset of 2^log2n points in natural order, point i = g_{2N} + i g_N = (x_i, y_i); log2n 1 .. 30
 *                   (0: LW_ERR_BAD_ARG, above: LW_ERR_ORDER_TOO_LARGE)
 * All entry points are _device forms under the stream and lane contract of the other *_device calls.  Device pointers
 * must be 16-byte aligned (else LW_ERR_BAD_ARG).  Every argument check runs before any device work.  A call that hands a
 * small result to the host (values, a root) waits for the stream; the others only enqueue.
 *
 * pointwise: as lw_babybear_ext4_pointwise_device, over QM31: MUL, SQR, INV (0 -> 0), MUL_BASE (d_b a single plane).
 *
 * evaluate: out_values[k m + j] = sum_i col_k[i] B_i(X_j, Y_j) for n_cols columns of 2^log2n base-field coefficients in the
 * basis of lw_circle_evaluate_cfft, B_i(x, y) = y^(bit 0 of i) prod_{t >= 1} pi^(t-1)(x)^(bit t of i), pi(x) = 2x^2 - 1, at m
 * points (host, 8 words each, not required to lie on the circle); out_values: host, n_cols m scalars.  A polynomial with
 * QM31 coefficients is its four planes as four columns, its value v0 + i v1 + u v2 + i u v3.  n_cols = 0 or m = 0: LW_OK.
 *
 * deep_quotients: for every row i of the domain
 *     out[i] = sum_j ( sum_k weights[k][j] (c_j col_k[i] - a_kj y_i - b_kj) ) / D_j(x_i, y_i)
 * with c_j = sigma Y_j - Y_j, a_kj = sigma v_kj - v_kj, b_kj = v_kj c_j - a_kj Y_j for v_kj = evals[k][j], and the line
 * through P_j and sigma P_j, D_j(x, y) = (Y_j - sigma Y_j) x + (sigma X_j - X_j) y + (X_j sigma Y_j - Y_j sigma X_j).  On
 * the circle D_j vanishes at P_j and sigma P_j only.  points: m points; weights, evals: n_cols x m scalars, row k, column
 * j (host).  A point with sigma P_j = P_j (the u-parts of X_j and Y_j zero) is LW_ERR_BAD_ARG, as are n_cols = 0, m = 0
 * and d_out overlapping a column.  A column of QM31 values is its four planes as four columns, the weight of plane e
 * multiplied by 1, i, u, iu by the caller.
 *
 * fri_layer: one fold of the circle FRI commit phase in evaluation form.  d_evals: 2^log2m = M values in natural order.
 *     d_out[i] = ( v[i] + v[M-1-i] + zeta (v[i] - v[M-1-i]) / t_i ) / 2,  i < M / 2
 * first != 0: the fold from the circle to the line, t_i = y_i of the coset of size M; first == 0: t_i = x_i of the coset
 * of size 2M (log2m <= 29).  In coefficients this is c'_m = c_2m + zeta c_2m+1.  d_out may not overlap d_evals.
 *   fold only   d_nodes_or_null == NULL; pair rows or a root asked for without nodes: LW_ERR_BAD_ARG
 *   tree        the M / 2 folded values (at least 4) committed as lw_monolith_commit_columns_device(rounds, d_pairs, 8, 0,
 *               log2m - 2, bit_reverse = 0): leaf i hashes out[i].c0..c3, out[M/2-1-i].c0..c3.  d_pairs: 2 M words, written
 *               by the fold (eight columns of M / 4 words); d_nodes: (M / 2 - 1) x 8 words, root first, readable by
 *               lw_stark_open_trees_device as it is; out_root_or_null: 8 words to host memory.  rounds 1 .. 15. */
typedef enum { LW_M31EXT4_MUL = 0, LW_M31EXT4_SQR = 1, LW_M31EXT4_INV = 2, LW_M31EXT4_MUL_BASE = 3 } lw_m31ext4_op_t;
int lw_mersenne31_ext4_pointwise_device(lw_m31ext4_op_t op, const uint32_t *d_a, size_t a_stride, const uint32_t *d_b, size_t b_stride,
                                        uint32_t *d_out, size_t out_stride, size_t n, void *hip_stream);
int lw_mersenne31_ext4_evaluate_device(const uint32_t *d_coeffs, uint32_t n_cols, size_t col_stride, uint32_t log2n,
                                       const uint32_t *points, uint32_t m, uint32_t *out_values, void *hip_stream);
int lw_mersenne31_ext4_deep_quotients_device(const uint32_t *d_lde, uint32_t n_cols, size_t col_stride, uint32_t log2n,
                                             const uint32_t *points, uint32_t m, const uint32_t *weights, const uint32_t *evals,
                                             uint32_t *d_out, size_t out_stride, void *hip_stream);
int lw_mersenne31_ext4_fri_layer_device(const uint32_t *d_evals, size_t in_stride, uint32_t log2m, const uint32_t *zeta, int first,
                                        uint32_t *d_out, size_t out_stride, uint32_t rounds, uint32_t *d_pairs_or_null,
                                        uint32_t *d_nodes_or_null, uint32_t *out_root_or_null, void *hip_stream);

/* ---- Circle STARK round 2 over Mersenne31 with QM31: the composition polynomial on the LDE coset in one pass, its parts ----
 * Words, planes, strides (0: dense), the 16-byte alignment of device pointers and host scalars {c0, c1, c2, c3} are those
 * of the lw_mersenne31_ext4_* section above.  n = 2^log2_trace, B = 2^log2_blowup, N = n B.  Trace points p_j = g_{2n} + j g_n,
 * LDE points q_i = g_{2N} + i g_N, both in natural order; q_i + g_n = q_(i + B mod N).  A - C for circle points is
 * (Ax Cx + Ay Cy, Ay Cx - Ax Cy).  The reference has no circle STARK prover: these lines are the definition.
 *
 * constraint_evaluations: ONE pass over the LDE columns, no row of transition evaluations is ever stored.  For every LDE
 * row i in [0, N), in QM31:
 *     out[i] = sum_c coeff_c T_c(i) E_c(q_i) / Z_c(q_i)  +  sum_k coeff_k (col_k[i] - value_k) (1 + x'_k) / y'_k
 *   T_c(i)   what the program emits for constraint c at row i: ops, the accumulator machine with its 8 temporaries, the
 *            CELL addressing col[(i + row B) mod len_col], the short (periodic) columns of col_log2_len_or_null and the host
 *            check are exactly those of lw_stark_transition_evaluations_device.  Cells and constants are any u32, read as
 *            (w & p) + (w >> 31).  A periodic column of period m_c is a column of m_c B words.
 *   transition {period, offset, end_exemptions, coeff}: the constraint holds at the trace rows j = offset mod period, except
 *            the last end_exemptions of those rows.  With m = n / period = 2^mu and c = p_offset:
 *            Z(Q) = the y-coordinate of 2^(mu-1) (Q - c), that is mu - 1 doublings: simple zeros exactly at the constrained
 *                   rows; on the LDE coset of period 2 B period in i and never zero when B >= 2;
 *            E(Q) = prod_{k = 1 .. end_exemptions} (1 - (P_k.x Q.x + P_k.y Q.y)), P_k = p_(offset + (m - k) period): the line
 *                   with a double zero at P_k.  There is no exemptions_period.
 *            Transitions whose three integers are equal share one table of 1 / Z and one value per row; a call takes at
 *            most 8 distinct descriptors.
 *   boundary {col, step, value, coeff}: (x'_k, y'_k) = q_i - p_step.  (t - v)(1 + x') / y' is a polynomial exactly when
 *            t(p_step) = v; y' vanishes at p_step and its antipode only, both trace points.
 *   d_columns  host array of n_cols device pointers; column c has N words (2^col_log2_len[c] for a short one).  d_out: four
 *            planes of N words, out_stride apart, that overlap no column; the words between two planes are not written.
 * Every check runs before any device work and the call only enqueues.  LW_ERR_BAD_ARG: log2_trace < 1 or log2_trace +
 * log2_blowup > 30; a period that is 0, not a power of two or above n / 2; offset >= period; end_exemptions > n / period;
 * col >= n_cols or step >= n; a boundary constraint on a short column; more than 8 distinct descriptors; a malformed program
 * (lw_hip_last_error names the op); a null or misaligned buffer; an out that overlaps a column.  LW_ERR_INV_ZERO:
 * log2_blowup = 0 with any constraint present.  n_boundary = 0 or n_transitions = 0 is legal; both: zeros.
 *
 * composition_parts: the four planes of d_evals are interpolated (lw_circle_interpolate_cfft_device, batch = 4).  In the
 * basis of lw_circle_evaluate_cfft bit t of a coefficient's index contributes the factor pi^(t-1)(x), so with
 * L = 2^log2_part and P = n_parts part j is the CONTIGUOUS block of coefficients [j L, (j + 1) L) and
 *     H(z) = sum_j M_j(z.x) H_j(z),   M_j = prod_{t: bit t of j set} pi^(log2_part + t - 1)(z.x).
 * Part j, plane e lies at plane index 4 j + e in both outputs: d_parts_coeffs is 4 P dense planes of L words,
 * d_parts_lde_or_null 4 P dense planes of N words, each the part on the LDE coset (its zero-padded coefficients through
 * the forward transform of lw_circle_lde_device, the padding never written) - the n_cols = 4 P shape of
 * lw_monolith_commit_columns_device and the "column as four planes" shape of evaluate and deep_quotients.
 * out_tail_nonzero_or_null receives the number of non-zero words at the coefficient indices >= P L over the four planes
 * (0 when the degree fits); asking for it synchronises.  d_evals is not modified.  LW_ERR_BAD_ARG: n_parts that is 0 or not
 * a power of two, log2_part < 1, P L > N, overlapping buffers, a null or misaligned buffer; log2_lde as in the section above.
 * The degree to budget: a transition of degree d in the cells with e end exemptions gives a quotient of total degree at
 * most d n / 2 + 2 e - m / 2, a boundary constraint one of at most n / 2; a polynomial of total degree D has no coefficient
 * at or above the smallest power of two greater than 2 D.  P L must reach that power of two for the tail to be 0. */
typedef struct {
    uint32_t col, reserved;
    uint64_t step;
    uint32_t value;
    uint32_t coeff[4];
    uint32_t reserved2;
} lw_m31q_boundary_t;
typedef struct {
    uint64_t period, offset, end_exemptions;
    uint32_t coeff[4];
} lw_m31q_transition_t;
int lw_mersenne31_ext4_constraint_evaluations_device(const lw_stark_air_op_t *ops, uint32_t n_ops, const uint32_t *consts,
                                                     uint32_t n_consts, const uint32_t *const *d_columns,
                                                     const uint32_t *col_log2_len_or_null, uint32_t n_cols, uint32_t log2_trace,
                                                     uint32_t log2_blowup, const lw_m31q_boundary_t *boundary, uint32_t n_boundary,
                                                     const lw_m31q_transition_t *transitions, uint32_t n_transitions,
                                                     uint32_t *d_out, size_t out_stride, void *hip_stream);
int lw_mersenne31_ext4_composition_parts_device(const uint32_t *d_evals, size_t evals_stride, uint32_t log2_lde, uint32_t log2_part,
                                                uint32_t n_parts, uint32_t *d_parts_coeffs, uint32_t *d_parts_lde_or_null,
                                                uint64_t *out_tail_nonzero_or_null, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
