// The validator of AIR transition programs (csrc/air_program.h) alone, for a build with -fsanitize=address,undefined:
// every malformed program of tests/test_air_program_cpu.py is refused with the op it names, and a maximal valid program
// (4096 ops, 8 temporaries, 256 constants, row = n - 1, constraints emitted out of order) is accepted.
#include "../lambda_elliptic_curves_amd/csrc/air_program.h"

#include <string.h>
#include <string>
#include <vector>

using lw::AirProgramInfo;
using lw::air_program_check;
typedef lw_stark_air_op_t Op;

static int failures = 0;
static const uint32_t LOG2_TRACE = 3, LOG2_LDE = 5, N_COLS = 2, N_CONSTS = 3;

static Op op(int o, int src = 0, int index = 0, uint32_t row = 0) {
    Op r;
    r.op = (uint8_t)o;
    r.src = (uint8_t)src;
    r.index = (uint16_t)index;
    r.row = row;
    return r;
}

// the program must be refused and the message must contain `needle`
static void refuse(const char *what, const std::vector<Op> &ops, uint32_t n_transitions, const char *needle, uint32_t n_consts = N_CONSTS,
                   const uint32_t *lens = nullptr) {
    // an exact-size heap copy: a read past the program is an AddressSanitizer report
    Op *heap = new Op[ops.size() ? ops.size() : 1];
    if (!ops.empty()) memcpy(heap, ops.data(), ops.size() * sizeof(Op));
    char msg[160] = "";
    AirProgramInfo info;
    const bool ok = air_program_check(heap, (uint32_t)ops.size(), n_consts, lens, N_COLS, LOG2_TRACE, LOG2_LDE, n_transitions, &info, msg, sizeof(msg));
    if (ok || !strstr(msg, needle)) {
        printf("FAIL %s: %s \"%s\" (expected \"%s\")\n", what, ok ? "accepted" : "refused with", msg, needle);
        failures++;
    }
    delete[] heap;
}

int main() {
    const int LOAD = LW_STARK_AIR_LOAD, ADD = LW_STARK_AIR_ADD, SUB = LW_STARK_AIR_SUB, MUL = LW_STARK_AIR_MUL, NEG = LW_STARK_AIR_NEG,
              STORE = LW_STARK_AIR_STORE, EMIT = LW_STARK_AIR_EMIT, CELL = LW_STARK_AIR_CELL, CONST = LW_STARK_AIR_CONST, TMP = LW_STARK_AIR_TMP;
    const std::vector<Op> good = {op(LOAD, CELL, 0, 1), op(SUB, CELL, 1, 0), op(STORE, 0, 2), op(MUL, CONST, 2), op(ADD, TMP, 2), op(NEG), op(EMIT, 0, 0)};
    {
        char msg[160] = "";
        AirProgramInfo info;
        if (!air_program_check(good.data(), (uint32_t)good.size(), N_CONSTS, nullptr, N_COLS, LOG2_TRACE, LOG2_LDE, 1, &info, msg, sizeof(msg)) ||
            info.n_tmps != 3 || info.n_mul != 1 || info.n_cell_reads != 2) {
            printf("FAIL good: %s\n", msg);
            failures++;
        }
        if (!air_program_check(nullptr, 0, 0, nullptr, 0, LOG2_TRACE, LOG2_LDE, 0, &info, msg, sizeof(msg))) {
            printf("FAIL empty: %s\n", msg);
            failures++;
        }
    }
    auto with = [&](size_t k, Op o) {
        std::vector<Op> v = good;
        v[k] = o;
        return v;
    };
    refuse("unknown op", with(5, op(7)), 1, "op 5: unknown op 7");
    refuse("unknown op 255", with(5, op(255)), 1, "op 5: unknown op 255");
    refuse("unknown src", with(1, op(SUB, 3, 1)), 1, "op 1: unknown src 3");
    refuse("column out of range", with(1, op(SUB, CELL, 2)), 1, "op 1: column 2 of 2");
    refuse("constant out of range", with(3, op(MUL, CONST, 3)), 1, "op 3: constant 3 of 3");
    refuse("temporary out of range (read)", with(4, op(ADD, TMP, 8)), 1, "op 4: temporary 8 of 8");
    refuse("temporary out of range (store)", with(2, op(STORE, 0, 8)), 1, "op 2: temporary 8 of 8");
    refuse("row = n", with(0, op(LOAD, CELL, 0, 8)), 1, "op 0: row offset 8");
    refuse("row on a constant", with(3, op(MUL, CONST, 2, 1)), 1, "op 3: row 1");
    refuse("row on a temporary", with(4, op(ADD, TMP, 2, 1)), 1, "op 4: row 1");
    refuse("NEG with src", with(5, op(NEG, 1)), 1, "op 5: NEG");
    refuse("NEG with index", with(5, op(NEG, 0, 1)), 1, "op 5: NEG");
    refuse("NEG with row", with(5, op(NEG, 0, 0, 1)), 1, "op 5: NEG");
    refuse("STORE with src", with(2, op(STORE, 1, 2)), 1, "op 2: STORE");
    refuse("EMIT with row", with(6, op(EMIT, 0, 0, 1)), 1, "op 6: EMIT");
    refuse("first reader is ADD", with(0, op(ADD, CELL, 0, 1)), 1, "op 0: the accumulator is read before the first LOAD");
    refuse("first reader is NEG", {op(NEG), op(LOAD, CELL, 0), op(EMIT, 0, 0)}, 1, "op 0: the accumulator");
    refuse("first reader is STORE", {op(STORE, 0, 0), op(LOAD, CELL, 0), op(EMIT, 0, 0)}, 1, "op 0: the accumulator");
    refuse("first reader is EMIT", {op(EMIT, 0, 0)}, 1, "op 0: the accumulator");
    refuse("TMP before its STORE", with(4, op(ADD, TMP, 1)), 1, "op 4: temporary 1 is read before it is stored");
    refuse("EMIT index = n_transitions", with(6, op(EMIT, 0, 1)), 1, "op 6: constraint 1 of 1");
    {
        std::vector<Op> twice = good;
        twice.push_back(op(EMIT, 0, 0));
        refuse("emitted twice", twice, 1, "op 7: constraint 0 is emitted twice");
        refuse("never emitted", good, 2, "op 7 (the end of the program): constraint 1 of 2 is never emitted");
        refuse("nothing emitted", {}, 1, "op 0 (the end of the program): constraint 0 of 1 is never emitted");
    }
    refuse("too many constants", good, 1, "257 constants", 257);
    {
        const uint32_t lens[2] = {5, 6};
        refuse("a column longer than the LDE", good, 1, "column 1: 2^6", N_CONSTS, lens);
    }
    {   // one op too many: a valid straight line of 4097 ops
        std::vector<Op> v(LW_STARK_AIR_MAX_OPS + 1, op(ADD, CELL, 0));
        v[0] = op(LOAD, CELL, 0);
        v.back() = op(EMIT, 0, 0);
        refuse("too many ops", v, 1, "4097 ops");
    }
    {   // maximal valid program: 4096 ops, all 8 temporaries and all 256 constants, row = n - 1, 16 constraints backwards
        std::vector<Op> v;
        v.push_back(op(LOAD, CELL, 1, (1u << LOG2_TRACE) - 1));
        for (int t = 0; t < LW_STARK_AIR_MAX_TMPS; t++) v.push_back(op(STORE, 0, t));
        for (int c = 15; c >= 0; c--) {
            v.push_back(op(MUL, TMP, c % LW_STARK_AIR_MAX_TMPS));
            v.push_back(op(EMIT, 0, c));
        }
        for (int k = 0; v.size() < LW_STARK_AIR_MAX_OPS; k++) v.push_back(op(k & 1 ? MUL : ADD, CONST, k % LW_STARK_AIR_MAX_CONSTS));
        Op *heap = new Op[v.size()];
        memcpy(heap, v.data(), v.size() * sizeof(Op));
        char msg[160] = "";
        AirProgramInfo info;
        const uint32_t lens[2] = {5, 0};
        if (!air_program_check(heap, (uint32_t)v.size(), LW_STARK_AIR_MAX_CONSTS, lens, N_COLS, LOG2_TRACE, LOG2_LDE, 16, &info, msg, sizeof(msg)) ||
            info.n_tmps != LW_STARK_AIR_MAX_TMPS || v.size() != LW_STARK_AIR_MAX_OPS) {
            printf("FAIL maximal: %s\n", msg);
            failures++;
        }
        // a message buffer of one byte, and none
        char tiny[1];
        (void)air_program_check(heap, (uint32_t)v.size(), 3, lens, N_COLS, LOG2_TRACE, LOG2_LDE, 16, &info, tiny, sizeof(tiny));
        (void)air_program_check(heap, (uint32_t)v.size(), 3, lens, N_COLS, LOG2_TRACE, LOG2_LDE, 16, nullptr, nullptr, 0);
        delete[] heap;
    }
    printf(failures ? "%d failures\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
