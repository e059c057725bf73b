// The interpreter of an AIR transition program (lw_stark_air_op_t, include/lw_hip.h, checked by air_program.h): the one op
// loop that air_transition_kernel (stark_air.hip), ext_r2_transition_kernel (ext_round2.cuh) and m31q_r2_transition_kernel
// (circle_round2.cuh) run at every LDE row, its two halves (operand fetch, apply op) for the F arms of
// ext_r2_rap_transition_kernel, and the staging of the tables it reads.  The kernels rely on every index being in range and
// check nothing: the host's air_program_check has.
//
// One work-item per LDE row.  The program counter, the op and its fields are the same for every lane: the tables are read at
// wave-uniform addresses through the scalar cache and the dispatch is a scalar branch, so no lane diverges.  The accumulator
// and the operand are the only values in registers.  The temporaries live in LDS, a lane's own words only: a slot known only
// at run time would turn a register array into scratch memory, while in LDS it is an address, and there is no barrier.
//
// The tables are 64-bit words in sections of one upload (R2Arena, r2_tables.h), every one read at a wave-uniform index:
//   ops      lw_stark_air_op_t as one word: op | src << 8 | index << 16 | row << 32
//   cells    per column: its address, its length - 1 (a power of two)
//   consts   per constant: the value as the value policy reads it (a word, or the 32 bytes of a 256-bit element)
//   trans    per constraint: beta_c (two words), its class, 0                                     (the round 2 kernels)
//   classes  per class: the address of its cycle table and three words of the kernel's own        (the round 2 kernels)
//   bnd      per boundary constraint, in the order of the steps: the address of its column, the stride of an auxiliary
//            column's planes in words (0 on a main column), gamma_k (two words)                   (the boundary kernels)
//
// A value policy V says what a value is:
//   V::value, V::lds_word           the type computed with, the type of an LDS word
//   V::zero()                       the accumulator before the first op
//   V::cell(address, pos)           element pos of the column at address, as the kernel computes with it
//   V::constant(consts, index)      constant index of the consts section
//   V::tmp(lds, slot), V::put(lds, slot, v)   the lane's temporary
//   V::add, V::sub, V::mul, V::neg
#pragma once
#include "internal.h"
#include "air_program.h"
#include "r2_tables.h"

namespace lw {

// word `k` of the u64 array at a wave-uniform address of memory nothing writes while the kernel runs: through the scalar cache
__device__ __forceinline__ uint64_t air_uniform(const void *p, size_t k) {
    return ((const __attribute__((address_space(4))) uint64_t *)(uintptr_t)p)[k];
}
// the 16-byte element at words k, k + 1
template <class Elem> __device__ __forceinline__ Elem air_uniform_elem(const uint64_t *p, size_t k) {
    static_assert(sizeof(Elem) == 16, "an element is two 64-bit words of a table");
    const uint64_t w[2] = {air_uniform(p, k), air_uniform(p, k + 1)};
    Elem v;
    __builtin_memcpy(&v, w, 16);
    return v;
}

struct AirOp {
    uint64_t word;   // as uploaded: the RAP kernel's type bits are in the op byte
    uint32_t op, src, index, row;
};
__device__ __forceinline__ AirOp air_decode(uint64_t w) {
    return AirOp{w, (uint32_t)w & 0xffu, (uint32_t)(w >> 8) & 0xffu, (uint32_t)(w >> 16) & 0xffffu, (uint32_t)(w >> 32)};
}

// the operand of a LOAD / ADD / SUB / MUL whose source is CELL, CONST or TMP, at LDE row i
template <class V>
__device__ __forceinline__ typename V::value air_operand(const AirOp o, const uint64_t *cells, const uint64_t *consts, typename V::lds_word *lds, uint64_t i,
                                                         uint32_t log2_blowup) {
    if (o.src == LW_STARK_AIR_CELL) {
        const uint64_t col = air_uniform(cells, 2 * o.index), mask = air_uniform(cells, 2 * o.index + 1);
        return V::cell(col, (i + ((uint64_t)o.row << log2_blowup)) & mask);
    }
    if (o.src == LW_STARK_AIR_CONST) return V::constant(consts, o.index);
    return V::tmp(lds, o.index);
}
// op: LOAD, ADD, SUB or MUL
template <class V> __device__ __forceinline__ typename V::value air_apply(uint32_t op, typename V::value acc, typename V::value s) {
    if (op == LW_STARK_AIR_LOAD) return s;
    if (op == LW_STARK_AIR_ADD) return V::add(acc, s);
    if (op == LW_STARK_AIR_SUB) return V::sub(acc, s);
    return V::mul(acc, s);
}

// runs the program at LDE row i; emit(c, acc) at EMIT c
template <class V, class Emit>
__device__ __forceinline__ void air_run(const uint64_t *ops, uint32_t n_ops, const uint64_t *cells, const uint64_t *consts, typename V::lds_word *lds, uint64_t i,
                                        uint32_t log2_blowup, Emit emit) {
    typename V::value acc = V::zero();
#pragma unroll 1
    for (uint32_t pc = 0; pc < n_ops; pc++) {
        const AirOp o = air_decode(air_uniform(ops, pc));
        if (o.op <= LW_STARK_AIR_MUL) acc = air_apply<V>(o.op, acc, air_operand<V>(o, cells, consts, lds, i, log2_blowup));
        else if (o.op == LW_STARK_AIR_NEG) acc = V::neg(acc);
        else if (o.op == LW_STARK_AIR_STORE) V::put(lds, o.index, acc);
        else emit(o.index, acc);
    }
}

// a word of the extension policy E (ext_steps.cuh), [slot][lane] in the LDS of a block of THREADS lanes
template <class E, int THREADS> struct AirWord {
    using value = typename E::word;
    using lds_word = typename E::word;
    static __device__ __forceinline__ value zero() { return 0; }
    static __device__ __forceinline__ value cell(uint64_t col, uint64_t pos) { return E::fcanon(((const value *)col)[pos]); }
    static __device__ __forceinline__ value constant(const uint64_t *consts, uint32_t index) { return (value)air_uniform(consts, index); }
    static __device__ __forceinline__ value tmp(const lds_word *lds, uint32_t slot) { return lds[slot * THREADS + threadIdx.x]; }
    static __device__ __forceinline__ void put(lds_word *lds, uint32_t slot, value v) { lds[slot * THREADS + threadIdx.x] = v; }
    static __device__ __forceinline__ value add(value a, value b) { return E::fadd(a, b); }
    static __device__ __forceinline__ value sub(value a, value b) { return E::fsub(a, b); }
    static __device__ __forceinline__ value mul(value a, value b) { return E::fmul(a, b); }
    static __device__ __forceinline__ value neg(value a) { return E::fsub(0, a); }
};

// ---------------------------------------------------------------- host
// the program check of the entry points that take a program without the RAP sources
static int air_program_checked(const lw_stark_air_op_t *ops, uint32_t n_ops, uint32_t n_consts, const uint32_t *col_log2_len, uint32_t n_cols, uint32_t log2_trace,
                               uint32_t log2_lde, uint32_t n_transitions, AirProgramInfo *info) {
    char msg[192];
    if (air_program_check(ops, n_ops, n_consts, col_log2_len, n_cols, log2_trace, log2_lde, n_transitions, info, msg, sizeof(msg))) return LW_OK;
    set_error("AIR program: %s", msg);
    return LW_ERR_BAD_ARG;
}

// The arena at c.poly_ws on the device, its first `bytes` (the sections that are uploaded) zeroed in the lane's pinned
// staging, so that the caller's arrays are free on return: fill the sections, then air_tables_upload.
static int air_tables_stage(Context &c, R2Arena &t, size_t bytes) {
    if (c.poly_ws.ensure(t.total)) return LW_ERR_ALLOC;
    t.dev = (char *)c.poly_ws.p;
    if (bytes == 0) return LW_OK;
    int rc = deep_pin(c, bytes);
    if (rc) return rc;
    t.host = (char *)c.deep_pin;
    memset(t.host, 0, bytes);
    return LW_OK;
}
static int air_tables_upload(Context &c, const R2Arena &t, size_t bytes, hipStream_t s) {
    LW_HIP_CHECK(hipMemcpyAsync(t.dev, t.host, bytes, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipEventRecord(c.deep_pin_read, s), LW_ERR_LAUNCH);
    return LW_OK;
}

}  // namespace lw
