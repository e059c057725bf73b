// The host-side check of an AIR transition program (lw_stark_air_op_t, include/lw_hip.h) for stark_air.hip: everything the
// kernel relies on is established here, before any device work, so that the kernel itself checks nothing.
// Host only, plain C++ (no HIP header): tests/air_program_host_main.cpp compiles it alone, with sanitizers.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/lw_hip.h"

namespace lw {

struct AirProgramInfo {
    uint32_t n_tmps;       // temporaries the program stores: slots 0 .. n_tmps - 1 (the highest STORE index + 1)
    uint32_t n_mul;        // MUL count
    uint32_t n_cell_reads; // CELL operands: the column elements one LDE row reads
};

// -> true when the program is well formed; otherwise msg names the offending op.  n = 2^log2_trace trace rows;
// col_log2_len_or_null[c] <= log2_lde is checked here too (a short column's length is a property of the program's input).
inline bool air_program_check(const lw_stark_air_op_t *ops, uint32_t n_ops, uint32_t n_consts, const uint32_t *col_log2_len_or_null,
                              uint32_t n_cols, uint32_t log2_trace, uint32_t log2_lde, uint32_t n_transitions, AirProgramInfo *info,
                              char *msg, size_t msg_len) {
    auto fail = [&](const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        if (msg && msg_len) vsnprintf(msg, msg_len, fmt, ap);
        va_end(ap);
        return false;
    };
    if (info) info->n_tmps = info->n_mul = info->n_cell_reads = 0;
    if (n_ops > LW_STARK_AIR_MAX_OPS) return fail("%u ops: a program has at most %d", n_ops, LW_STARK_AIR_MAX_OPS);
    if (n_consts > LW_STARK_AIR_MAX_CONSTS) return fail("%u constants: a program has at most %d", n_consts, LW_STARK_AIR_MAX_CONSTS);
    if (n_ops && !ops) return fail("null program of %u ops", n_ops);
    if (log2_trace > 63 || log2_lde > 63 || log2_lde < log2_trace) return fail("trace 2^%u, LDE 2^%u", log2_trace, log2_lde);
    if (col_log2_len_or_null)
        for (uint32_t c = 0; c < n_cols; c++)
            if (col_log2_len_or_null[c] > log2_lde)
                return fail("column %u: 2^%u elements exceed the LDE domain of 2^%u", c, col_log2_len_or_null[c], log2_lde);
    // constraint c is emitted exactly once: 64 constraints per word
    constexpr uint32_t WORDS = (65536 + 63) / 64;
    uint64_t emitted[WORDS] = {0};
    const uint64_t n = 1ull << log2_trace;
    bool acc_live = false;
    uint32_t stored = 0;   // bit t: tmp[t] has been stored
    uint32_t n_emitted = 0, n_tmps = 0, n_mul = 0, n_cell = 0;
    for (uint32_t k = 0; k < n_ops; k++) {
        const lw_stark_air_op_t &o = ops[k];
        switch (o.op) {
            case LW_STARK_AIR_LOAD:
            case LW_STARK_AIR_ADD:
            case LW_STARK_AIR_SUB:
            case LW_STARK_AIR_MUL:
                if (o.op != LW_STARK_AIR_LOAD && !acc_live) return fail("op %u: the accumulator is read before the first LOAD", k);
                switch (o.src) {
                    case LW_STARK_AIR_CELL:
                        if (o.index >= n_cols) return fail("op %u: column %u of %u", k, o.index, n_cols);
                        if (o.row >= n) return fail("op %u: row offset %u of a trace of 2^%u rows", k, o.row, log2_trace);
                        n_cell++;
                        break;
                    case LW_STARK_AIR_CONST:
                        if (o.index >= n_consts) return fail("op %u: constant %u of %u", k, o.index, n_consts);
                        if (o.row) return fail("op %u: row %u on a constant operand", k, o.row);
                        break;
                    case LW_STARK_AIR_TMP:
                        if (o.index >= LW_STARK_AIR_MAX_TMPS) return fail("op %u: temporary %u of %d", k, o.index, LW_STARK_AIR_MAX_TMPS);
                        if (o.row) return fail("op %u: row %u on a temporary operand", k, o.row);
                        if (!(stored >> o.index & 1)) return fail("op %u: temporary %u is read before it is stored", k, o.index);
                        break;
                    default:
                        return fail("op %u: unknown src %u", k, o.src);
                }
                if (o.op == LW_STARK_AIR_MUL) n_mul++;
                acc_live = true;
                break;
            case LW_STARK_AIR_NEG:
                if (o.src || o.index || o.row) return fail("op %u: NEG takes no operand (src %u, index %u, row %u)", k, o.src, o.index, o.row);
                if (!acc_live) return fail("op %u: the accumulator is read before the first LOAD", k);
                break;
            case LW_STARK_AIR_STORE:
                if (o.src || o.row) return fail("op %u: STORE takes an index only (src %u, row %u)", k, o.src, o.row);
                if (o.index >= LW_STARK_AIR_MAX_TMPS) return fail("op %u: temporary %u of %d", k, o.index, LW_STARK_AIR_MAX_TMPS);
                if (!acc_live) return fail("op %u: the accumulator is read before the first LOAD", k);
                stored |= 1u << o.index;
                if (o.index + 1u > n_tmps) n_tmps = o.index + 1u;
                break;
            case LW_STARK_AIR_EMIT:
                if (o.src || o.row) return fail("op %u: EMIT takes an index only (src %u, row %u)", k, o.src, o.row);
                if (o.index >= n_transitions) return fail("op %u: constraint %u of %u", k, o.index, n_transitions);
                if (!acc_live) return fail("op %u: the accumulator is read before the first LOAD", k);
                if (emitted[o.index / 64] >> (o.index % 64) & 1) return fail("op %u: constraint %u is emitted twice", k, o.index);
                emitted[o.index / 64] |= 1ull << (o.index % 64);
                n_emitted++;
                break;
            default:
                return fail("op %u: unknown op %u", k, o.op);
        }
    }
    if (n_emitted != n_transitions) {
        uint32_t c = 0;
        while (c < n_transitions && c < 65536 && (emitted[c / 64] >> (c % 64) & 1)) c++;
        return fail("op %u (the end of the program): constraint %u of %u is never emitted", n_ops, c, n_transitions);
    }
    if (info) {
        info->n_tmps = n_tmps;
        info->n_mul = n_mul;
        info->n_cell_reads = n_cell;
    }
    return true;
}

}  // namespace lw
