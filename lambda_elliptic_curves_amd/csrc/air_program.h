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
    uint32_t n_ext_tmps;   // air_program_check_rap: the temporaries that hold an element of E at some point of the program
    uint32_t n_lds_slots;  // air_program_check_rap: words per lane for the temporaries, (n_tmps - n_ext_tmps) + D n_ext_tmps
};

// What air_program_check_rap adds to the op byte of the word the kernel reads (op | src << 8 | index << 16 | row << 32):
// the types are the host's, so the kernel's dispatch on them is a scalar branch.
constexpr uint64_t AIR_TYPED_ACC_EXT = 1u << 4;   // the accumulator holds an element of E before the op
constexpr uint64_t AIR_TYPED_SRC_EXT = 1u << 5;   // the operand is an element of E (XCELL, XCONST, a temporary that holds one)

struct AirRapLimits {   // what only the RAP entry points have; nullptr: XCELL and XCONST are unknown sources
    uint32_t n_xcols, n_xconsts, ext_degree;
    uint64_t *typed;    // n_ops words or nullptr: the op words with the type bits, TMP and STORE indices as LDS slots
};

// -> true when the program is well formed; otherwise msg names the offending op.  n = 2^log2_trace trace rows;
// col_log2_len_or_null[c] <= log2_lde is checked here too (a short column's length is a property of the program's input).
inline bool air_program_check_body(const lw_stark_air_op_t *ops, uint32_t n_ops, uint32_t n_consts, const uint32_t *col_log2_len_or_null,
                                   uint32_t n_cols, uint32_t log2_trace, uint32_t log2_lde, uint32_t n_transitions, const AirRapLimits *rap,
                                   AirProgramInfo *info, char *msg, size_t msg_len) {
    auto fail = [&](const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        if (msg && msg_len) vsnprintf(msg, msg_len, fmt, ap);
        va_end(ap);
        return false;
    };
    if (info) info->n_tmps = info->n_mul = info->n_cell_reads = info->n_ext_tmps = info->n_lds_slots = 0;
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
    // the program is straight-line, so every value has one type at every point: the accumulator's, and per temporary the
    // type of what it holds now (tmp_ext) and whether it ever holds an element of E (ever_ext: it takes D LDS slots then)
    bool acc_ext = false;
    uint32_t tmp_ext = 0, ever_ext = 0;
    auto typed = [&](uint32_t k, uint64_t bits) {
        if (rap && rap->typed)
            rap->typed[k] = ((uint64_t)ops[k].op | bits) | (uint64_t)ops[k].src << 8 | (uint64_t)ops[k].index << 16 | (uint64_t)ops[k].row << 32;
    };
    for (uint32_t k = 0; k < n_ops; k++) {
        const lw_stark_air_op_t &o = ops[k];
        bool src_ext = false;   // the operand of a LOAD / ADD / SUB / MUL is an element of E
        switch (o.op) {
            case LW_STARK_AIR_LOAD:
            case LW_STARK_AIR_ADD:
            case LW_STARK_AIR_SUB:
            case LW_STARK_AIR_MUL:
                if (o.op != LW_STARK_AIR_LOAD && !acc_live) return fail("op %u: the accumulator is read before the first LOAD", k);
                src_ext = false;
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
                        src_ext = tmp_ext >> o.index & 1;
                        break;
                    case LW_STARK_AIR_XCELL:
                        if (!rap) return fail("op %u: unknown src %u", k, o.src);
                        if (o.index >= rap->n_xcols) return fail("op %u: auxiliary column %u of %u", k, o.index, rap->n_xcols);
                        if (o.row >= n) return fail("op %u: row offset %u of a trace of 2^%u rows", k, o.row, log2_trace);
                        n_cell++;
                        src_ext = true;
                        break;
                    case LW_STARK_AIR_XCONST:
                        if (!rap) return fail("op %u: unknown src %u", k, o.src);
                        if (o.index >= rap->n_xconsts) return fail("op %u: extension constant %u of %u", k, o.index, rap->n_xconsts);
                        if (o.row) return fail("op %u: row %u on an extension constant operand", k, o.row);
                        src_ext = true;
                        break;
                    default:
                        return fail("op %u: unknown src %u", k, o.src);
                }
                if (o.op == LW_STARK_AIR_MUL) n_mul++;
                typed(k, (o.op != LW_STARK_AIR_LOAD && acc_ext ? AIR_TYPED_ACC_EXT : 0) | (src_ext ? AIR_TYPED_SRC_EXT : 0));
                acc_ext = o.op == LW_STARK_AIR_LOAD ? src_ext : acc_ext || src_ext;
                acc_live = true;
                break;
            case LW_STARK_AIR_NEG:
                if (o.src || o.index || o.row) return fail("op %u: NEG takes no operand (src %u, index %u, row %u)", k, o.src, o.index, o.row);
                if (!acc_live) return fail("op %u: the accumulator is read before the first LOAD", k);
                typed(k, acc_ext ? AIR_TYPED_ACC_EXT : 0);
                break;
            case LW_STARK_AIR_STORE:
                if (o.src || o.row) return fail("op %u: STORE takes an index only (src %u, row %u)", k, o.src, o.row);
                if (o.index >= LW_STARK_AIR_MAX_TMPS) return fail("op %u: temporary %u of %d", k, o.index, LW_STARK_AIR_MAX_TMPS);
                if (!acc_live) return fail("op %u: the accumulator is read before the first LOAD", k);
                stored |= 1u << o.index;
                if (o.index + 1u > n_tmps) n_tmps = o.index + 1u;
                tmp_ext = (tmp_ext & ~(1u << o.index)) | (acc_ext ? 1u << o.index : 0);
                if (acc_ext) ever_ext |= 1u << o.index;
                typed(k, acc_ext ? AIR_TYPED_ACC_EXT : 0);
                break;
            case LW_STARK_AIR_EMIT:
                if (o.src || o.row) return fail("op %u: EMIT takes an index only (src %u, row %u)", k, o.src, o.row);
                if (o.index >= n_transitions) return fail("op %u: constraint %u of %u", k, o.index, n_transitions);
                if (!acc_live) return fail("op %u: the accumulator is read before the first LOAD", k);
                if (emitted[o.index / 64] >> (o.index % 64) & 1) return fail("op %u: constraint %u is emitted twice", k, o.index);
                emitted[o.index / 64] |= 1ull << (o.index % 64);
                n_emitted++;
                typed(k, acc_ext ? AIR_TYPED_ACC_EXT : 0);
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
    // temporary t lies at LDS slot base[t]: one slot, or ext_degree slots where it ever holds an element of E
    uint32_t base[LW_STARK_AIR_MAX_TMPS], slots = 0, n_ext = 0;
    for (uint32_t t = 0; t < n_tmps; t++) {
        base[t] = slots;
        slots += (ever_ext >> t & 1) ? (rap ? rap->ext_degree : 1) : 1;
        n_ext += ever_ext >> t & 1;
    }
    if (rap && rap->typed)
        for (uint32_t k = 0; k < n_ops; k++)
            if (ops[k].op == LW_STARK_AIR_STORE || (ops[k].op <= LW_STARK_AIR_MUL && ops[k].src == LW_STARK_AIR_TMP))
                rap->typed[k] = (rap->typed[k] & ~(0xffffull << 16)) | (uint64_t)base[ops[k].index] << 16;
    if (info) {
        info->n_tmps = n_tmps;
        info->n_mul = n_mul;
        info->n_cell_reads = n_cell;
        info->n_ext_tmps = n_ext;
        info->n_lds_slots = slots;
    }
    return true;
}

inline bool air_program_check(const lw_stark_air_op_t *ops, uint32_t n_ops, uint32_t n_consts, const uint32_t *col_log2_len_or_null,
                              uint32_t n_cols, uint32_t log2_trace, uint32_t log2_lde, uint32_t n_transitions, AirProgramInfo *info,
                              char *msg, size_t msg_len) {
    return air_program_check_body(ops, n_ops, n_consts, col_log2_len_or_null, n_cols, log2_trace, log2_lde, n_transitions, nullptr, info, msg, msg_len);
}

// The same with the two sources of a randomized AIR: XCELL reads one of n_xcols auxiliary columns, XCONST one of n_xconsts
// constants, both elements of the extension E of degree ext_degree.  typed_or_null[k] is op k as the kernel reads it: the
// op word with AIR_TYPED_ACC_EXT / AIR_TYPED_SRC_EXT set where the accumulator (before the op) or the operand holds an
// element of E, and the index of a TMP operand or a STORE replaced by the temporary's first LDS slot.
inline bool air_program_check_rap(const lw_stark_air_op_t *ops, uint32_t n_ops, uint32_t n_consts, uint32_t n_xconsts,
                                  const uint32_t *col_log2_len_or_null, uint32_t n_cols, uint32_t n_xcols, uint32_t ext_degree, uint32_t log2_trace,
                                  uint32_t log2_lde, uint32_t n_transitions, uint64_t *typed_or_null, AirProgramInfo *info, char *msg, size_t msg_len) {
    if (n_xconsts > LW_STARK_AIR_MAX_CONSTS) {
        if (msg && msg_len) snprintf(msg, msg_len, "%u extension constants: a program has at most %d", n_xconsts, LW_STARK_AIR_MAX_CONSTS);
        if (info) info->n_tmps = info->n_mul = info->n_cell_reads = info->n_ext_tmps = info->n_lds_slots = 0;
        return false;
    }
    const AirRapLimits rap{n_xcols, n_xconsts, ext_degree, typed_or_null};
    return air_program_check_body(ops, n_ops, n_consts, col_log2_len_or_null, n_cols, log2_trace, log2_lde, n_transitions, &rap, info, msg, msg_len);
}

}  // namespace lw
