// The host tables that the AIR interpreters and the round 2 kernels read (air_interp.cuh has their layouts): the arena of
// their sections, the fill of the sections that are the same for every field, and the classes of the transition descriptors.
// Host only, plain C++ (no HIP header, no Context): tests/circle_round2_host_main.cpp and tests/ext_round2_host_main.cpp
// compile it stand-alone, with sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>

namespace lw {

static inline size_t r2_round256(size_t b) { return (b + 255) & ~(size_t)255; }

// Sections of one buffer, 256 bytes apart at least: add() them in order, point host and dev at the buffer's two copies.
struct R2Arena {
    size_t total = 0;
    char *host = nullptr, *dev = nullptr;
    size_t add(size_t bytes) {   // -> the offset of a new section
        const size_t at = total;
        total += r2_round256(bytes);
        return at;
    }
    uint64_t *h(size_t section) const { return (uint64_t *)(host + section); }
    const uint64_t *d(size_t section) const { return (const uint64_t *)(dev + section); }
};

// an element of an extension as the two 64-bit words the kernels read it back from
template <class Elem> static void r2_pack(Elem v, uint64_t *dst) {
    static_assert(sizeof(Elem) == 16, "an element is two 64-bit words of a table");
    memcpy(dst, &v, 16);
}

// ops: n_ops words of 8 bytes (lw_stark_air_op_t, or the typed words of air_program_check_rap)
static inline void r2_fill_ops(uint64_t *t, const void *ops, uint32_t n_ops) {
    if (n_ops) memcpy(t, ops, (size_t)n_ops * 8);
}
// cells: per column its address and its length - 1; N: the length of a column without a length of its own
template <class P> static void r2_fill_cells(uint64_t *t, const P *const *cols, const uint32_t *col_log2_len, uint32_t n_cols, uint64_t N) {
    for (uint32_t k = 0; k < n_cols; k++) {
        t[2 * k] = (uint64_t)(uintptr_t)cols[k];
        t[2 * k + 1] = (col_log2_len ? 1ull << col_log2_len[k] : N) - 1;
    }
}
// trans, entry k: beta_k, the constraint's class, 0
template <class Elem> static void r2_fill_trans(uint64_t *t, size_t k, Elem beta, uint32_t cls) {
    r2_pack(beta, t + 4 * k);
    t[4 * k + 2] = cls;
}
// bnd, entry q: the column's address, the stride of an auxiliary column's planes (0 on a main column), gamma
template <class Elem> static void r2_fill_bnd(uint64_t *t, size_t q, const void *col, uint64_t aux_stride, Elem gamma) {
    t[4 * q] = (uint64_t)(uintptr_t)col;
    t[4 * q + 1] = aux_stride;
    r2_pack(gamma, t + 4 * q + 2);
}

// steps [s0, s0 + S) of the boundary constraints' step groups into the argument struct of a boundary kernel's launch
template <class Args, class Step> static void r2_fill_steps(Args &b, const std::vector<Step> &steps, size_t s0, size_t S) {
    for (size_t j = 0; j < S; j++) {
        b.point[j] = steps[s0 + j].point;
        b.first[j] = steps[s0 + j].first;
        b.count[j] = steps[s0 + j].count;
        b.constant[j] = steps[s0 + j].constant;
    }
}

// the distinct descriptors Desc::of(tr[c]) in the order of their first appearance; class_of[c] indexes them
template <class T, class Desc> static void r2_classes(const T *tr, uint32_t n_tr, std::vector<uint32_t> &class_of, std::vector<Desc> &classes) {
    class_of.assign(n_tr, 0);
    classes.clear();
    for (uint32_t c = 0; c < n_tr; c++) {
        const Desc d = Desc::of(tr[c]);
        uint32_t k = 0;
        while (k < classes.size() && !(classes[k] == d)) k++;
        if (k == classes.size()) classes.push_back(d);
        class_of[c] = k;
    }
}

}  // namespace lw
