// STARK transition constraints on the device from an AIR given as data: the AIR's compute_transition
// (provers/stark/src/traits.rs, the examples of provers/stark/src/examples/*.rs) as a straight-line program of
// lw_stark_air_op_t (include/lw_hip.h) that one kernel runs at every LDE row, writing the T_c rows
// lw_stark_constraint_evaluations_device (stark_round2.hip) reads.  air_program.h checks the program on the host; the
// kernel relies on every index being in range and checks nothing.
//
// air_transition_kernel   one work-item per LDE row.  The program counter, the op and its fields are the same for every
//                         lane: the ops, the column table and the constants are read from wave-uniform addresses through
//                         the scalar cache and the dispatch is a scalar branch, so no lane diverges.  acc and the operand
//                         are the only field elements in registers.  The temporaries live in LDS as limb planes
//                         [slot][limb][lane]: a slot index known only at run time would turn a register array into
//                         scratch memory, while in LDS it is an address; a lane reads and writes its own words only,
//                         so there is no barrier and consecutive lanes hit consecutive banks.  The launch asks for the
//                         slots the program stores (AirProgramInfo::n_tmps), 4 KiB each for AIR_THREADS lanes:
//                         a program without temporaries uses no LDS, one with all eight 32 KiB.
// Arithmetic is the canonical fe_add / fe_sub / fe_mul / fe_neg of field.cuh: every value held or stored is in [0, p).
#include <string.h>
#include <vector>
#include "internal.h"
#include "field.cuh"
#include "air_program.h"

namespace lw {

constexpr int AIR_THREADS = 128;   // 8 slots x 8 limbs x 4 bytes x 128 lanes = 32 KiB of LDS at most

struct alignas(16) AirCell {
    const char *col;
    uint64_t mask;                 // len_col - 1 (a power of two)
};
struct AirArgs {
    const uint64_t *ops;           // lw_stark_air_op_t as one word: op | src << 8 | index << 16 | row << 32
    const AirCell *cells;
    const char *consts;
    char *out;
    uint64_t out_stride;           // elements between the rows of two constraints
    uint64_t N;
    uint32_t n_ops, log2_blowup;
};

// word `k` of the u64 array at a wave-uniform address of memory nothing writes while the kernel runs: through the scalar cache
__device__ __forceinline__ uint64_t air_uniform(const void *p, size_t k) {
    return ((const __attribute__((address_space(4))) uint64_t *)(uintptr_t)p)[k];
}
template <class F>
__device__ __forceinline__ Fe<F> air_uniform_fe(const char *p) {
    constexpr int N = F::N;
    uint32_t m[N];
#pragma unroll
    for (int j = 0; j < N / 2; j++) {
        const uint64_t x = air_uniform(p, j);
        m[2 * j] = (uint32_t)x;
        m[2 * j + 1] = (uint32_t)(x >> 32);
    }
    Fe<F> r;
#pragma unroll
    for (int k = 0; k < N; k++) r.v[k] = m[mem_index<F>(k)];
    return r;
}

template <class F>
__global__ __launch_bounds__(AIR_THREADS) void air_transition_kernel(const AirArgs a) {
    extern __shared__ uint32_t air_tmp[];   // [slot][limb][lane]
    constexpr int N = F::N;
    const uint64_t i = (uint64_t)blockIdx.x * AIR_THREADS + threadIdx.x;
    if (i >= a.N) return;
    Fe<F> acc = Fe<F>::zero();
#pragma unroll 1
    for (uint32_t pc = 0; pc < a.n_ops; pc++) {
        const uint64_t w = air_uniform(a.ops, pc);
        const uint32_t op = (uint32_t)w & 0xffu, src = (uint32_t)(w >> 8) & 0xffu, index = (uint32_t)(w >> 16) & 0xffffu, row = (uint32_t)(w >> 32);
        if (op <= LW_STARK_AIR_MUL) {
            Fe<F> s;
            if (src == LW_STARK_AIR_CELL) {
                const char *col = (const char *)air_uniform(a.cells, 2 * index);
                const uint64_t mask = air_uniform(a.cells, 2 * index + 1);
                s = fe_load<F>(col + ((i + ((uint64_t)row << a.log2_blowup)) & mask) * 32);
            } else if (src == LW_STARK_AIR_CONST) {
                s = air_uniform_fe<F>(a.consts + (size_t)index * 32);
            } else {
#pragma unroll
                for (int k = 0; k < N; k++) s.v[k] = air_tmp[(index * N + k) * AIR_THREADS + threadIdx.x];
            }
            if (op == LW_STARK_AIR_LOAD) acc = s;
            else if (op == LW_STARK_AIR_ADD) acc = fe_add<F>(acc, s);
            else if (op == LW_STARK_AIR_SUB) acc = fe_sub<F>(acc, s);
            else acc = fe_mul<F>(acc, s);
        } else if (op == LW_STARK_AIR_NEG) {
            acc = fe_neg<F>(acc);
        } else if (op == LW_STARK_AIR_STORE) {
#pragma unroll
            for (int k = 0; k < N; k++) air_tmp[(index * N + k) * AIR_THREADS + threadIdx.x] = acc.v[k];
        } else {   // EMIT
            fe_store<F>(a.out + ((uint64_t)index * a.out_stride + i) * 32, acc);
        }
    }
}

// ---- host side ----
static size_t air_round256(size_t b) { return (b + 255) & ~(size_t)255; }
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
    char msg[192];
    if (!air_program_check(ops, n_ops, n_consts, col_log2_len, n_cols, log2_trace, (uint32_t)lg, n_transitions, info, msg, sizeof(msg))) {
        set_error("AIR program: %s", msg);
        return LW_ERR_BAD_ARG;
    }
    return LW_OK;
}

// cols: n_cols device pointers (host array).  Enqueue only.
template <class F>
static int air_locked(Context &c, const lw_stark_air_op_t *ops, uint32_t n_ops, const void *consts, uint32_t n_consts,
                      const void *const *cols, const uint32_t *col_log2_len, uint32_t n_cols, uint32_t log2_lde, uint32_t log2_blowup,
                      uint32_t n_transitions, const AirProgramInfo &info, void *d_out, uint64_t out_stride, hipStream_t s) {
    if (n_ops == 0 || n_transitions == 0) return LW_OK;   // nothing is emitted
    const uint64_t N = 1ull << log2_lde;
    const size_t b_ops = air_round256((size_t)n_ops * sizeof(lw_stark_air_op_t)), b_cells = air_round256((size_t)n_cols * sizeof(AirCell)),
                 b_consts = air_round256((size_t)n_consts * 32), tables = b_ops + b_cells + b_consts;
    if (c.poly_ws.ensure(tables)) return LW_ERR_ALLOC;
    int rc = deep_pin(c, tables);   // one upload through the lane's pinned staging: the caller's arrays are free on return
    if (rc) return rc;
    char *hp = (char *)c.deep_pin, *d_tab = (char *)c.poly_ws.p;
    memset(hp, 0, tables);
    memcpy(hp, ops, (size_t)n_ops * sizeof(lw_stark_air_op_t));
    AirCell *cells = (AirCell *)(hp + b_ops);
    for (uint32_t k = 0; k < n_cols; k++) {
        cells[k].col = (const char *)cols[k];
        cells[k].mask = (col_log2_len ? 1ull << col_log2_len[k] : N) - 1;
    }
    if (n_consts) memcpy(hp + b_ops + b_cells, consts, (size_t)n_consts * 32);
    LW_HIP_CHECK(hipMemcpyAsync(d_tab, hp, tables, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipEventRecord(c.deep_pin_read, s), LW_ERR_LAUNCH);
    AirArgs a;
    memset(&a, 0, sizeof(a));
    a.ops = (const uint64_t *)d_tab;
    a.cells = (const AirCell *)(d_tab + b_ops);
    a.consts = d_tab + b_ops + b_cells;
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
