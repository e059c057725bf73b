// STARK transition constraints on the device from an AIR given as data: the AIR's compute_transition
// (provers/stark/src/traits.rs, the examples of provers/stark/src/examples/*.rs) as a straight-line program of
// lw_stark_air_op_t (include/lw_hip.h) that one kernel runs at every LDE row, writing the T_c rows
// lw_stark_constraint_evaluations_device (stark_round2.hip) reads.  air_program.h checks the program on the host; the
// kernel relies on every index being in range and checks nothing.
//
// air_transition_kernel   one work-item per LDE row runs the program with air_run (air_interp.cuh) over the value policy
//                         AirFe<F> and stores the accumulator at EMIT c as element i of row T_c.  The temporaries live in LDS
//                         as limb planes [slot][limb][lane], so that consecutive lanes hit consecutive banks.  The launch
//                         asks for the slots the program stores (AirProgramInfo::n_tmps), 4 KiB each for AIR_THREADS lanes:
//                         a program without temporaries uses no LDS, one with all eight 32 KiB.
// Arithmetic is the canonical fe_add / fe_sub / fe_mul / fe_neg of field.cuh: every value held or stored is in [0, p).
#include <string.h>
#include <vector>
#include "field.cuh"
#include "air_interp.cuh"

namespace lw {

constexpr int AIR_THREADS = 128;   // 8 slots x 8 limbs x 4 bytes x 128 lanes = 32 KiB of LDS at most

struct AirArgs {
    const uint64_t *ops, *cells, *consts;   // the sections of air_interp.cuh; a constant is 32 bytes as fe_load reads them
    char *out;
    uint64_t out_stride;           // elements between the rows of two constraints
    uint64_t N;
    uint32_t n_ops, log2_blowup;
};

// a 256-bit element of F in [0, p), limb planes [slot][limb][lane] in LDS
template <class F> struct AirFe {
    using value = Fe<F>;
    using lds_word = uint32_t;
    static __device__ __forceinline__ value zero() { return Fe<F>::zero(); }
    static __device__ __forceinline__ value cell(uint64_t col, uint64_t pos) { return fe_load<F>((const char *)col + pos * 32); }
    static __device__ __forceinline__ value constant(const uint64_t *consts, uint32_t index) {
        constexpr int N = F::N;
        uint32_t m[N];
#pragma unroll
        for (int j = 0; j < N / 2; j++) {
            const uint64_t x = air_uniform(consts, (size_t)index * (N / 2) + j);
            m[2 * j] = (uint32_t)x;
            m[2 * j + 1] = (uint32_t)(x >> 32);
        }
        value r;
#pragma unroll
        for (int k = 0; k < N; k++) r.v[k] = m[mem_index<F>(k)];
        return r;
    }
    static __device__ __forceinline__ value tmp(const lds_word *lds, uint32_t slot) {
        value s;
#pragma unroll
        for (int k = 0; k < F::N; k++) s.v[k] = lds[(slot * F::N + k) * AIR_THREADS + threadIdx.x];
        return s;
    }
    static __device__ __forceinline__ void put(lds_word *lds, uint32_t slot, const value &v) {
#pragma unroll
        for (int k = 0; k < F::N; k++) lds[(slot * F::N + k) * AIR_THREADS + threadIdx.x] = v.v[k];
    }
    static __device__ __forceinline__ value add(const value &a, const value &b) { return fe_add<F>(a, b); }
    static __device__ __forceinline__ value sub(const value &a, const value &b) { return fe_sub<F>(a, b); }
    static __device__ __forceinline__ value mul(const value &a, const value &b) { return fe_mul<F>(a, b); }
    static __device__ __forceinline__ value neg(const value &a) { return fe_neg<F>(a); }
};

template <class F>
__global__ __launch_bounds__(AIR_THREADS) void air_transition_kernel(const AirArgs a) {
    extern __shared__ uint32_t air_tmp[];
    const uint64_t i = (uint64_t)blockIdx.x * AIR_THREADS + threadIdx.x;
    if (i >= a.N) return;
    char *const out = a.out + i * 32;
    const uint64_t row_bytes = a.out_stride * 32;
    air_run<AirFe<F>>(a.ops, a.n_ops, a.cells, a.consts, air_tmp, i, a.log2_blowup,
                      [=](uint32_t c, const Fe<F> &acc) { fe_store<F>(out + c * row_bytes, acc); });
}

// ---- host side ----
static bool air_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// The checks of both forms that need no device; *info out
static int air_check(lw_field_t field, const lw_stark_air_op_t *ops, uint32_t n_ops, const void *consts, uint32_t n_consts,
                     const uint32_t *col_log2_len, uint32_t n_cols, uint32_t log2_trace, uint32_t log2_blowup, uint32_t n_transitions,
                     AirProgramInfo *info) {
    if (field != LW_FIELD_STARK252 && field != LW_FIELD_BLS12_381_FR) {
        set_error("field %d: the STARK transition evaluation takes STARK252 or BLS12_381_FR (4 x u64 limbs)", (int)field);
        return LW_ERR_BAD_ARG;
    }
    const uint64_t lg = (uint64_t)log2_trace + log2_blowup;
    if (lg > 34 || lg > field_two_adicity(field)) { set_error("an LDE domain of 2^%llu points is beyond the NTT", (unsigned long long)lg); return LW_ERR_BAD_ARG; }
    if (n_consts <= LW_STARK_AIR_MAX_CONSTS && n_consts && !consts) { set_error("null constants"); return LW_ERR_BAD_ARG; }
    return air_program_checked(ops, n_ops, n_consts, col_log2_len, n_cols, log2_trace, (uint32_t)lg, n_transitions, info);
}

// cols: n_cols device pointers (host array).  Enqueue only.
template <class F>
static int air_locked(Context &c, const lw_stark_air_op_t *ops, uint32_t n_ops, const void *consts, uint32_t n_consts,
                      const void *const *cols, const uint32_t *col_log2_len, uint32_t n_cols, uint32_t log2_lde, uint32_t log2_blowup,
                      uint32_t n_transitions, const AirProgramInfo &info, void *d_out, uint64_t out_stride, hipStream_t s) {
    if (n_ops == 0 || n_transitions == 0) return LW_OK;   // nothing is emitted
    const uint64_t N = 1ull << log2_lde;
    R2Arena t;   // one upload through the lane's pinned staging
    const size_t s_ops = t.add((size_t)n_ops * sizeof(lw_stark_air_op_t)), s_cells = t.add((size_t)n_cols * 16), s_consts = t.add((size_t)n_consts * 32);
    int rc = air_tables_stage(c, t, t.total);
    if (rc) return rc;
    r2_fill_ops(t.h(s_ops), ops, n_ops);
    r2_fill_cells(t.h(s_cells), cols, col_log2_len, n_cols, N);
    if (n_consts) memcpy(t.h(s_consts), consts, (size_t)n_consts * 32);
    if ((rc = air_tables_upload(c, t, t.total, s))) return rc;
    AirArgs a;
    memset(&a, 0, sizeof(a));
    a.ops = t.d(s_ops);
    a.cells = t.d(s_cells);
    a.consts = t.d(s_consts);
    a.out = (char *)d_out;
    a.out_stride = out_stride;
    a.N = N;
    a.n_ops = n_ops;
    a.log2_blowup = log2_blowup;
    const size_t lds = (size_t)info.n_tmps * F::N * AIR_THREADS * sizeof(uint32_t);
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL((air_transition_kernel<F>), dim3((uint32_t)((N + AIR_THREADS - 1) / AIR_THREADS)), dim3(AIR_THREADS), lds, s, a);
    c.prof_end("air_transition_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}

}  // namespace lw

using namespace lw;

static_assert(sizeof(lw_stark_air_op_t) == 8, "an AIR op is one 64-bit word");

extern "C" {

int lw_stark_transition_evaluations_device(lw_field_t field, const lw_stark_air_op_t *ops, uint32_t n_ops, const void *consts,
                                           uint32_t n_consts, const void *const *d_columns, const uint32_t *col_log2_len_or_null,
                                           uint32_t n_cols, uint32_t log2_trace, uint32_t log2_blowup, uint32_t n_transitions,
                                           void *d_out, uint64_t out_stride_elems, void *hip_stream) {
    AirProgramInfo info;
    int rc = air_check(field, ops, n_ops, consts, n_consts, col_log2_len_or_null, n_cols, log2_trace, log2_blowup, n_transitions, &info);
    if (rc) return rc;
    const uint32_t log2_lde = log2_trace + log2_blowup;
    const uint64_t N = 1ull << log2_lde;
    if ((n_cols && !d_columns) || (n_transitions && !d_out)) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    if (!air_aligned16(d_out)) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    for (uint32_t k = 0; k < n_cols; k++)
        if (!d_columns[k] || !air_aligned16(d_columns[k])) { set_error("column %u: null or misaligned buffer", k); return LW_ERR_BAD_ARG; }
    if (out_stride_elems == 0) out_stride_elems = N;
    if (n_transitions > 1 && out_stride_elems < N) { set_error("output stride %llu < 2^%u rows", (unsigned long long)out_stride_elems, log2_lde); return LW_ERR_BAD_ARG; }
    if (n_ops == 0 || n_transitions == 0) return LW_OK;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return field == LW_FIELD_STARK252
               ? air_locked<Stark252>(en.c, ops, n_ops, consts, n_consts, d_columns, col_log2_len_or_null, n_cols, log2_lde, log2_blowup,
                                      n_transitions, info, d_out, out_stride_elems, en.stream)
               : air_locked<Fr381>(en.c, ops, n_ops, consts, n_consts, d_columns, col_log2_len_or_null, n_cols, log2_lde, log2_blowup,
                                   n_transitions, info, d_out, out_stride_elems, en.stream);
}

// a: the columns, back to back   b: the T rows
int lw_stark_transition_evaluations(lw_field_t field, const lw_stark_air_op_t *ops, uint32_t n_ops, const void *consts, uint32_t n_consts,
                                    const void *columns, const uint32_t *col_log2_len_or_null, uint32_t n_cols, uint32_t log2_trace,
                                    uint32_t log2_blowup, uint32_t n_transitions, void *out) {
    AirProgramInfo info;
    int rc = air_check(field, ops, n_ops, consts, n_consts, col_log2_len_or_null, n_cols, log2_trace, log2_blowup, n_transitions, &info);
    if (rc) return rc;
    if ((n_cols && !columns) || (n_transitions && !out)) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    if (n_ops == 0 || n_transitions == 0) return LW_OK;
    const uint32_t log2_lde = log2_trace + log2_blowup;
    const size_t N = (size_t)1 << log2_lde;
    Entry en(nullptr);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    std::vector<const void *> cols(n_cols);
    size_t a_cols = 0;
    for (uint32_t k = 0; k < n_cols; k++) a_cols += (col_log2_len_or_null ? (size_t)1 << col_log2_len_or_null[k] : N) * 32;
    const size_t b_out = (size_t)n_transitions * N * 32;
    if (c.host_io_a.ensure(a_cols + 256) || c.host_io_b.ensure(b_out)) return LW_ERR_ALLOC;
    if (a_cols) LW_HIP_CHECK(hipMemcpyAsync(c.host_io_a.p, columns, a_cols, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    size_t at = 0;
    for (uint32_t k = 0; k < n_cols; k++) {
        cols[k] = (const char *)c.host_io_a.p + at;
        at += (col_log2_len_or_null ? (size_t)1 << col_log2_len_or_null[k] : N) * 32;
    }
    rc = field == LW_FIELD_STARK252
             ? air_locked<Stark252>(c, ops, n_ops, consts, n_consts, cols.data(), col_log2_len_or_null, n_cols, log2_lde, log2_blowup,
                                    n_transitions, info, c.host_io_b.p, N, s)
             : air_locked<Fr381>(c, ops, n_ops, consts, n_consts, cols.data(), col_log2_len_or_null, n_cols, log2_lde, log2_blowup,
                                 n_transitions, info, c.host_io_b.p, N, s);
    if (rc) return rc;
    LW_HIP_CHECK(hipMemcpyAsync(out, c.host_io_b.p, b_out, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    return LW_OK;
}

}  // extern "C"
