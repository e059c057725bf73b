// STARK round 2 over a small field with its extension, written once for goldilocks_ext.hip (F Goldilocks, E = Fp2) and
// babybear_ext.hip (F BabyBear, E = Fp4) over the policy E of ext_steps.cuh: the evaluations of the composition polynomial
// on the LDE coset in ONE pass over the LDE columns, and its parts.
//
//   out[i] = sum_c beta_c Z_c[i] T_c(i)  +  sum_k gamma_k (col_k[i] - v_k) / (x_i - g^step_k)        x_i = h w^i, out[i] in E
//
// T_c(i) is what the AIR's program (lw_stark_air_op_t, checked by air_program.h) leaves in the accumulator at EMIT c, Z_c
// the zerofier of lw_stark_constraint_evaluations_device, both in F; beta_c and gamma_k are in E.  The 256-bit path
// (stark_air.hip, stark_round2.hip) writes a row T_c per constraint and reads it back; with words of 4 and 8 bytes those
// rows would be most of the traffic, so here they never exist.
//
// ext_r2_xtable_kernel     the two-level table of the LDE coset: lo[a] = w^a, hi[b] = h w^(b 2^hbits), so that x_i is one product
//                          and two loads (a block reads consecutive lo entries and one hi entry) where E::fpow takes some
//                          thirty products
// ext_r2_cycle_kernel      the cycle tables of the distinct transition descriptors (EXT_R2_CLASSES at most), back to back:
//                          numerator / denominator per entry, EXT_ROWS entries of a work-item share one E::finv
// ext_r2_transition_kernel one work-item per LDE row.  It first forms the zerofier value of every class at its row (cycle
//                          entry times the end-exemption roots) and keeps it in LDS, then runs the program with air_run
//                          (air_interp.cuh) over words of F and at EMIT c folds beta_c (Z_class(c) acc) into its E
//                          accumulator with E::mul_base.  Temporaries and class values live in LDS as [slot][lane] words.
//                          Writes out.
// ext_r2_boundary_kernel   up to EXT_R2_STEPS distinct steps per launch, EXT_ROWS consecutive rows per work-item
//                          (E::R2_ROWS_FEW with one or two steps): the rows x steps denominators inverted with ONE E::finv
//                          (Montgomery's trick), the numerators sum_k gamma_k col_k[i] - c_s (c_s = sum_k gamma_k v_k is the
//                          host's) formed on the way back, the sum added into out.  More steps are more launches.
// The boundary part is a launch of its own: the interpreter wants one row per lane, so that the temporaries are one LDS word
// per slot and lane, while a base-field inversion (127 products in Goldilocks) wants to be shared by several rows; one kernel
// for both would pay an inversion per row or several times the LDS.  The price is one more read and write of out.
// ext_r2_split_kernel      break_in_parts over words: part j, plane e at plane j D + e
// ext_r2_lengths_kernel    the stripped length of every part
//
//
// The randomized AIR (the _rap_ entry points): auxiliary columns and constants in E.  An auxiliary column is D planes of N
// words; the program reads it with XCELL and a constant of E with XCONST, and a boundary constraint may sit on it.
// air_program_check_rap types every value of the straight-line program as F or E and writes the types into the op words, so
// ext_r2_rap_transition_kernel, an interpreter with two accumulators (a word and an element), branches on them with a
// scalar branch: an op on F operands is air_interp.cuh's as above, F with E is E::mul_base, E with E is E::mul,
// and an emitted element folds as beta_c (Z acc) with one E::mul.  A temporary that ever holds an element takes D LDS slots
// [slot][coordinate][lane], any other one: (F temporaries + D E temporaries + classes) words per lane, 48 KiB (Fp2) or 40 KiB
// (Fp4) at most.  The boundary kernel takes a template flag: a constraint on an auxiliary column adds E::mul(gamma_k,
// aux_k[i]) where one on a main column adds E::mul_base, and v_k in E only changes the host's constant c_s.
#pragma once
#include <algorithm>
#include "air_interp.cuh"
#include "ext_steps.cuh"

namespace lw {

constexpr int EXT_R2_CLASSES = 8;   // distinct transition descriptors per call (their per-row values are LDS slots)
constexpr int EXT_R2_STEPS = 4;     // distinct boundary steps per launch: EXT_ROWS x EXT_R2_STEPS denominators per inversion

// ---------------------------------------------------------------- host tables: plain arithmetic, no Context
struct ExtR2Desc {   // a transition's zerofier: the classes of r2_classes
    uint64_t period, offset, end_exemptions, exemptions_period, periodic_exemptions_offset;
    template <class T> static ExtR2Desc of(const T &t) { return ExtR2Desc{t.period, t.offset, t.end_exemptions, t.exemptions_period, t.periodic_exemptions_offset}; }
    bool operator==(const ExtR2Desc &o) const {
        return period == o.period && offset == o.offset && end_exemptions == o.end_exemptions && exemptions_period == o.exemptions_period &&
               periodic_exemptions_offset == o.periodic_exemptions_offset;
    }
};
// the names under which the stand-alone host programs of tests/ call r2_classes and r2_pack
template <class T> static void ext_r2_classes(const T *tr, uint32_t n_tr, std::vector<uint32_t> &class_of, std::vector<ExtR2Desc> &classes) { r2_classes(tr, n_tr, class_of, classes); }
template <class E> static void ext_r2_pack(typename E::elem v, uint64_t *dst) { r2_pack(v, dst); }
// cycle[e] = ((h w^e)^ne - nc) / ((h w^e)^de - dc) for e < len (the numerator 1 without an exemptions period), then the
// roots g^(n - k period), k = 1 .. end_exemptions (zerofier_evaluations_on_extended_domain with its truncating divisions)
template <class E> struct ExtR2Cycle {
    uint64_t off, len, de, ne;
    typename E::word dc, nc;
    uint32_t has_num;
};
template <class E> static ExtR2Cycle<E> ext_r2_cycle(const ExtR2Desc &d, uint32_t log2_trace, uint32_t log2_blowup, typename E::word g) {
    typedef unsigned __int128 u128;
    const uint64_t n = 1ull << log2_trace, N = n << log2_blowup, ep = d.exemptions_period;
    ExtR2Cycle<E> cy{};
    cy.de = n / d.period;
    cy.dc = E::fpow(g, (uint64_t)((u128)d.offset * n / d.period % n));
    cy.nc = E::F_ONE;
    if (ep) {
        cy.has_num = 1;
        cy.ne = n / ep;
        cy.nc = E::fpow(g, (uint64_t)((u128)n * d.periodic_exemptions_offset / ep % n));
    }
    const u128 len = ((u128)1 << log2_blowup) * (ep ? ep : d.period);
    cy.len = len > N ? N : (uint64_t)len;   // a longer table is read below N only
    return cy;
}
template <class E> static void ext_r2_roots(const ExtR2Desc &d, uint64_t n, typename E::word g, std::vector<typename E::word> &roots) {
    for (uint64_t k = 1; k <= d.end_exemptions; k++) roots.push_back(E::fpow(g, (n - k * d.period) % n));
}
// boundary constraints by distinct step (mod n: g has order n), stable: order[q] is the constraint at place q,
// steps[s] covers the places [first, first + count)
template <class E> struct ExtR2Step {
    typename E::word point;      // g^step
    uint32_t first, count;
    typename E::elem constant;   // sum_k gamma_k v_k over the step's constraints
};
// gamma_k v_k with v_k a word of F (the boundary entries of the plain entry points) or a scalar of E (the _rap_ ones)
template <class E> static typename E::elem ext_r2_times_value(typename E::elem gamma, const typename E::word &v) { return E::mul_base(gamma, E::fcanon(v)); }
template <class E> static typename E::elem ext_r2_times_value(typename E::elem gamma, const typename E::word (&v)[E::D]) {
    return E::mul(gamma, ext_elem_of<E>(v, 0));
}
template <class E> static int ext_r2_value_check(const typename E::word &v) { return E::words_check(&v, 1, "boundary value"); }
template <class E> static int ext_r2_value_check(const typename E::word (&v)[E::D]) { return E::words_check(v, E::D, "boundary value"); }
// whether a boundary entry sits on an auxiliary column: only the _rap_ entries have the member
template <class B> static auto ext_r2_is_aux(const B &b, int) -> decltype(b.is_aux != 0) { return b.is_aux != 0; }
template <class B> static bool ext_r2_is_aux(const B &, long) { return false; }
template <class E, class B>
static void ext_r2_step_groups(const B *bnd, uint32_t n_bnd, uint64_t n, typename E::word g, std::vector<uint32_t> &order, std::vector<ExtR2Step<E>> &steps) {
    order.resize(n_bnd);
    for (uint32_t k = 0; k < n_bnd; k++) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return bnd[x].step % n < bnd[y].step % n; });
    steps.clear();
    for (uint32_t q = 0; q < n_bnd; q++) {
        const B &b = bnd[order[q]];
        if (q == 0 || b.step % n != bnd[order[q - 1]].step % n) steps.push_back(ExtR2Step<E>{E::fpow(g, b.step % n), q, 0, E::zero()});
        steps.back().count++;
        steps.back().constant = E::add(steps.back().constant, ext_r2_times_value<E>(ext_elem_of<E>(b.coeff, 0), b.value));
    }
}

// ---------------------------------------------------------------- kernels
// x_i = lo[i & (2^hbits - 1)] hi[i >> hbits]
template <class E> struct ExtR2Domain {
    const typename E::word *lo, *hi;
    uint32_t hbits;
};
template <class E> __device__ __forceinline__ typename E::word ext_r2_x(const ExtR2Domain<E> d, uint64_t i) {
    return E::fmul(d.lo[i & ((1ull << d.hbits) - 1)], d.hi[i >> d.hbits]);
}
template <class E>
__global__ __launch_bounds__(EXT_THREADS) void ext_r2_xtable_kernel(typename E::word *lo, typename E::word *hi, uint64_t nlo, uint64_t nhi, typename E::word w,
                                                                    typename E::word wh, typename E::word h) {
    const uint64_t i = (uint64_t)blockIdx.x * EXT_THREADS + threadIdx.x;
    if (i < nlo) lo[i] = E::fpow(w, i);
    else if (i - nlo < nhi) hi[i - nlo] = E::fmul(h, E::fpow(wh, i - nlo));
}

template <class E> struct ExtR2CycleArgs {
    ExtR2Cycle<E> cy[EXT_R2_CLASSES];
    uint32_t n_classes;
    uint64_t total;
    typename E::word h, w;
    typename E::word *table;
};
template <class E> __global__ __launch_bounds__(EXT_THREADS) void ext_r2_cycle_kernel(const ExtR2CycleArgs<E> a) {
    using word = typename E::word;
    const uint64_t i0 = ((uint64_t)blockIdx.x * EXT_THREADS + threadIdx.x) * EXT_ROWS;
    if (i0 >= a.total) return;
    word num[EXT_ROWS], den[EXT_ROWS], pre[EXT_ROWS];
    word run = E::F_ONE;
#pragma unroll
    for (int r = 0; r < EXT_ROWS; r++) {
        num[r] = den[r] = E::F_ONE;
        if (i0 + r < a.total) {
            // the entry's table, by selects over constant indices: an index that differs from lane to lane would copy
            // the argument struct to private memory
            ExtR2Cycle<E> cy = a.cy[0];
#pragma unroll
            for (int t = 1; t < EXT_R2_CLASSES; t++)
                if ((uint32_t)t < a.n_classes && i0 + r >= a.cy[t].off) cy = a.cy[t];
            const word x = E::fmul(a.h, E::fpow(a.w, i0 + r - cy.off));
            den[r] = E::fsub(E::fpow(x, cy.de), cy.dc);   // not zero: the host refuses the offsets that allow it
            if (cy.has_num) num[r] = E::fsub(E::fpow(x, cy.ne), cy.nc);
        }
        pre[r] = run;
        run = E::fmul(run, den[r]);
    }
    word inv = E::finv(run);
#pragma unroll
    for (int r = EXT_ROWS - 1; r >= 0; r--) {
        if (i0 + r < a.total) a.table[i0 + r] = E::fmul(num[r], E::fmul(inv, pre[r]));
        inv = E::fmul(inv, den[r]);
    }
}

// The sections of air_interp.cuh, and
//   classes  per class: the address of its cycle table, the table's length, pow2 | n_roots << 32, its first root
//   roots    per root: the word
// and for the RAP kernel
//   ops      the words of air_program_check_rap: AIR_TYPED_ACC_EXT and AIR_TYPED_SRC_EXT in the op byte, LDS slots as the
//            indices of temporaries
//   xcells   per auxiliary column: the address of its plane 0, the stride of its planes in words
//   xconsts  per constant of E: two words
template <class E> struct ExtR2Args {
    const uint64_t *ops, *cells, *consts, *trans, *classes, *roots, *xcells, *xconsts;   // the last two null in the plain kernel
    uint64_t N;
    uint32_t n_ops, log2_blowup, n_classes, n_slots, any_roots;   // n_slots: LDS slots of the temporaries (the plain kernel's n_tmps)
    ExtR2Domain<E> dom;
    ExtPlanes<E> out;
};

extern __shared__ uint64_t ext_r2_lds[];   // [slot][lane] words: the program's temporaries, then the classes' values

// the zerofier value of every class at row i, cycle entry times the end-exemption roots, into the LDS slots from `first` on
template <class E>
__device__ __forceinline__ void ext_r2_class_values(const uint64_t *classes, const uint64_t *roots, uint32_t n_classes, uint32_t any_roots, const ExtR2Domain<E> dom,
                                                    typename E::word *lds, uint32_t first, uint64_t i) {
    using word = typename E::word;
    const word x = any_roots ? ext_r2_x<E>(dom, i) : E::F_ONE;
#pragma unroll 1
    for (uint32_t k = 0; k < n_classes; k++) {
        const word *cycle = (const word *)air_uniform(classes, 4 * k);
        const uint64_t len = air_uniform(classes, 4 * k + 1), meta = air_uniform(classes, 4 * k + 2), root0 = air_uniform(classes, 4 * k + 3);
        word v = cycle[(meta & 1) ? (i & (len - 1)) : i % len];
        const uint32_t n_roots = (uint32_t)(meta >> 32);
#pragma unroll 1
        for (uint32_t r = 0; r < n_roots; r++) v = E::fmul(v, E::fsub(x, (word)air_uniform(roots, root0 + r)));
        lds[(first + k) * EXT_THREADS + threadIdx.x] = v;
    }
}

template <class E> __global__ __launch_bounds__(EXT_THREADS) void ext_r2_transition_kernel(const ExtR2Args<E> a) {
    using word = typename E::word;
    using elem = typename E::elem;
    word *lds = (word *)ext_r2_lds;
    const uint64_t i = (uint64_t)blockIdx.x * EXT_THREADS + threadIdx.x;
    if (i >= a.N) return;
    ext_r2_class_values<E>(a.classes, a.roots, a.n_classes, a.any_roots, a.dom, lds, a.n_slots, i);
    elem sum = E::zero();
    const uint64_t *trans = a.trans;
    const uint32_t n_slots = a.n_slots;
    air_run<AirWord<E, EXT_THREADS>>(a.ops, a.n_ops, a.cells, a.consts, lds, i, a.log2_blowup, [&sum, trans, lds, n_slots](uint32_t c, word acc) {
        // no row T_c, the term goes onto the sum
        const uint32_t cls = (uint32_t)air_uniform(trans, 4 * c + 2);
        sum = E::add(sum, E::mul_base(air_uniform_elem<elem>(trans, 4 * c), E::fmul(lds[(n_slots + cls) * EXT_THREADS + threadIdx.x], acc)));
    });
    E::store(a.out, i, sum);
}

// the D LDS slots of a temporary that holds an element, as planes: element threadIdx.x is the lane's
template <class E> __device__ __forceinline__ ExtPlanes<E> ext_r2_lds_planes(typename E::word *lds, uint32_t slot) {
    ExtPlanes<E> v;
#pragma unroll
    for (int e = 0; e < E::D; e++) v.p[e] = lds + (size_t)(slot + e) * EXT_THREADS;
    return v;
}

template <class E> __global__ __launch_bounds__(EXT_THREADS) void ext_r2_rap_transition_kernel(const ExtR2Args<E> a) {
    using word = typename E::word;
    using elem = typename E::elem;
    using W = AirWord<E, EXT_THREADS>;
    word *lds = (word *)ext_r2_lds;
    const uint64_t i = (uint64_t)blockIdx.x * EXT_THREADS + threadIdx.x;
    if (i >= a.N) return;
    ext_r2_class_values<E>(a.classes, a.roots, a.n_classes, a.any_roots, a.dom, lds, a.n_slots, i);
    elem sum = E::zero(), ea = E::zero();   // ea: the accumulator while it holds an element, acc: while it holds a word
    word acc = 0;
#pragma unroll 1
    for (uint32_t pc = 0; pc < a.n_ops; pc++) {
        const AirOp o = air_decode(air_uniform(a.ops, pc));
        const uint32_t op = o.op & 0xfu, index = o.index;
        const bool acc_ext = o.word & AIR_TYPED_ACC_EXT, src_ext = o.word & AIR_TYPED_SRC_EXT;   // the host's: uniform
        if (op <= LW_STARK_AIR_MUL && !src_ext) {
            const word s = air_operand<W>(o, a.cells, a.consts, lds, i, a.log2_blowup);
            if (!acc_ext) {   // F with F: as ext_r2_transition_kernel
                acc = air_apply<W>(op, acc, s);
            } else if (op == LW_STARK_AIR_ADD) {
                ea.c0 = E::fadd(ea.c0, s);
            } else if (op == LW_STARK_AIR_SUB) {
                ea.c0 = E::fsub(ea.c0, s);
            } else {
                ea = E::mul_base(ea, s);
            }
        } else if (op <= LW_STARK_AIR_MUL) {
            elem se;
            if (o.src == LW_STARK_AIR_XCELL) {
                const word *col = (const word *)air_uniform(a.xcells, 2 * index);
                se = E::canon(E::load(ext_planes<E>(col, air_uniform(a.xcells, 2 * index + 1)), (i + ((uint64_t)o.row << a.log2_blowup)) & (a.N - 1)));
            } else if (o.src == LW_STARK_AIR_XCONST) {
                se = air_uniform_elem<elem>(a.xconsts, 2 * index);
            } else {
                se = E::load(ext_r2_lds_planes<E>(lds, index), threadIdx.x);
            }
            if (op == LW_STARK_AIR_LOAD) {
                ea = se;
            } else if (acc_ext) {
                if (op == LW_STARK_AIR_ADD) ea = E::add(ea, se);
                else if (op == LW_STARK_AIR_SUB) ea = E::sub(ea, se);
                else ea = E::mul(ea, se);
            } else if (op == LW_STARK_AIR_ADD) {   // F with E: the word is the element (acc, 0, ...)
                ea = se;
                ea.c0 = E::fadd(acc, se.c0);
            } else if (op == LW_STARK_AIR_SUB) {
                ea = E::sub(E::zero(), se);
                ea.c0 = E::fadd(ea.c0, acc);
            } else {
                ea = E::mul_base(se, acc);
            }
        } else if (op == LW_STARK_AIR_NEG) {
            if (acc_ext) ea = E::sub(E::zero(), ea);
            else acc = W::neg(acc);
        } else if (op == LW_STARK_AIR_STORE) {
            if (acc_ext) E::store(ext_r2_lds_planes<E>(lds, index), threadIdx.x, ea);
            else W::put(lds, index, acc);
        } else {   // EMIT
            const uint32_t cls = (uint32_t)air_uniform(a.trans, 4 * index + 2);
            const word zc = lds[(a.n_slots + cls) * EXT_THREADS + threadIdx.x];
            const elem beta = air_uniform_elem<elem>(a.trans, 4 * index);
            if (acc_ext) sum = E::add(sum, E::mul(beta, E::mul_base(ea, zc)));
            else sum = E::add(sum, E::mul_base(beta, E::fmul(zc, acc)));
        }
    }
    E::store(a.out, i, sum);
}

// bnd: the section of air_interp.cuh
template <class E> struct ExtR2BoundaryArgs {
    const uint64_t *bnd;
    uint64_t N;
    uint32_t accumulate;
    ExtR2Domain<E> dom;
    typename E::word w;
    typename E::word point[EXT_R2_STEPS];
    uint32_t first[EXT_R2_STEPS], count[EXT_R2_STEPS];
    typename E::elem constant[EXT_R2_STEPS];
    ExtPlanes<E> out;
};

// R rows per work-item: E::R2_ROWS_FEW with up to two steps, EXT_ROWS with more, so that R x S stays at 16 denominators or
// fewer.  Eight rows with few steps took Fp2's launch from 0.148 to 0.107 ms at 2^22 rows (E::finv is 127 products there) and
// Fp4's from 0.052 to 0.082 ms (31 squarings, and a lane's eight 4-byte words are a quarter of a line): the extension says.  The way forward forms the denominators alone; the numerators of a step are formed on the way back, when the step's
// inverses are due, so that only the denominators and their running products stay live across the inversion.
template <class E, int R, int S, bool AUX = false> __global__ __launch_bounds__(EXT_THREADS) void ext_r2_boundary_kernel(const ExtR2BoundaryArgs<E> a) {
    using word = typename E::word;
    using elem = typename E::elem;
    const uint64_t row0 = ((uint64_t)blockIdx.x * EXT_THREADS + threadIdx.x) * R;
    if (row0 >= a.N) return;
    // the denominators x_i - g^step and their running products, step after step
    word x[R], d[S][R], pre[S][R];
    x[0] = ext_r2_x<E>(a.dom, row0);
#pragma unroll
    for (int r = 1; r < R; r++) x[r] = E::fmul(x[r - 1], a.w);
    word run = E::F_ONE;
#pragma unroll
    for (int s = 0; s < S; s++)
#pragma unroll
        for (int r = 0; r < R; r++) {
            d[s][r] = E::fsub(x[r], a.point[s]);   // not zero: h^N != 1 (the host's check)
            pre[s][r] = run;
            run = E::fmul(run, d[s][r]);
        }
    word inv = E::finv(run);
    elem sum[R];
#pragma unroll
    for (int r = 0; r < R; r++) sum[r] = E::zero();
#pragma unroll
    for (int s = S - 1; s >= 0; s--) {
        elem t[R];
#pragma unroll
        for (int r = 0; r < R; r++) t[r] = E::zero();
#pragma unroll 1
        for (uint32_t k = a.first[s]; k < a.first[s] + a.count[s]; k++) {
            const word *col = (const word *)air_uniform(a.bnd, 4 * k) + row0;
            const elem gamma = air_uniform_elem<elem>(a.bnd, 4 * k + 2);
            const uint64_t aux_stride = AUX ? air_uniform(a.bnd, 4 * k + 1) : 0;
            if (AUX && aux_stride) {
                const ExtPlanes<E> aux = ext_planes<E>(col, aux_stride);
#pragma unroll
                for (int r = 0; r < R; r++)
                    if (row0 + r < a.N) t[r] = E::add(t[r], E::mul(gamma, E::canon(E::load(aux, r))));
            } else {
#pragma unroll
                for (int r = 0; r < R; r++)
                    if (row0 + r < a.N) t[r] = E::add(t[r], E::mul_base(gamma, E::fcanon(col[r])));   // N < R: the rows past the domain
            }
        }
#pragma unroll
        for (int r = R - 1; r >= 0; r--) {
            sum[r] = E::add(sum[r], E::mul_base(E::sub(t[r], a.constant[s]), E::fmul(inv, pre[s][r])));
            inv = E::fmul(inv, d[s][r]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (row0 + r >= a.N) break;
        elem o = sum[r];
        if (a.accumulate) o = E::add(o, E::load(a.out, row0 + r));   // canonical: an earlier launch wrote them
        E::store(a.out, row0 + r, o);
    }
}

// part j, plane e, slot m <- plane e of H[j + m P] (zero past N): P D planes of 2^log2_L words, plane j D + e
template <class E>
__global__ __launch_bounds__(EXT_THREADS) void ext_r2_split_kernel(const ExtPlanes<E> H, uint64_t N, uint64_t P, uint32_t log2_L, typename E::word *parts) {
    const uint64_t idx = (uint64_t)blockIdx.x * EXT_THREADS + threadIdx.x;
    if (idx >= (P << log2_L)) return;
    const uint64_t j = idx >> log2_L, m = idx & ((1ull << log2_L) - 1), src = j + m * P;
#pragma unroll
    for (int e = 0; e < E::D; e++) parts[((j * E::D + e) << log2_L) + m] = src < N ? H.p[e][src] : 0;
}
// lens[j] = the last slot of part j where any plane is not zero, plus one (lens zeroed before the launch)
template <class E>
__global__ __launch_bounds__(EXT_THREADS) void ext_r2_lengths_kernel(const typename E::word *parts, uint64_t P, uint32_t log2_L, unsigned long long *lens) {
    const uint64_t idx = (uint64_t)blockIdx.x * EXT_THREADS + threadIdx.x;
    if (idx >= (P << log2_L)) return;
    const uint64_t j = idx >> log2_L, m = idx & ((1ull << log2_L) - 1);
    typename E::word any = 0;
#pragma unroll
    for (int e = 0; e < E::D; e++) any |= parts[((j * E::D + e) << log2_L) + m];
    if (any) atomicMax(lens + j, (unsigned long long)(m + 1));
}

struct ExtR2Names { const char *xtable, *cycle, *transition, *boundary, *split, *lengths, *rap_transition; };

// what the _rap_ entry points add to a call: the auxiliary columns, the constants of E and the typed program
template <class E> struct ExtR2Rap {
    const typename E::word *const *aux;
    uint32_t n_aux;
    size_t aux_stride;
    const typename E::word *xconsts;
    uint32_t n_xconsts;
    std::vector<uint64_t> typed;   // the op words of air_program_check_rap
    uint32_t n_slots;
};

// ---------------------------------------------------------------- host: the constraint evaluations
// B, T: the extension's boundary and transition entries (lw_gl2_boundary_t, lw_bb4_boundary_t, ...).  cols: n_cols device
// pointers (host array).  Everything is checked; enqueue only.
template <class E, class B, class T>
static int ext_r2_constraints_locked(Context &c, const ExtR2Names &names, const lw_stark_air_op_t *ops, uint32_t n_ops, const typename E::word *consts,
                                     uint32_t n_consts, const typename E::word *const *cols, const uint32_t *col_log2_len, uint32_t n_cols,
                                     uint32_t log2_trace, uint32_t log2_blowup, typename E::word h, uint64_t root, const B *bnd, uint32_t n_bnd, const T *tr,
                                     uint32_t n_tr, uint32_t n_tmps, typename E::word *d_out, uint64_t out_stride, hipStream_t s,
                                     const ExtR2Rap<E> *rap = nullptr) {
    using word = typename E::word;
    const uint32_t log2_lde = log2_trace + log2_blowup;
    const uint64_t n = 1ull << log2_trace, N = 1ull << log2_lde;
    const word g = E::domain_root(root, log2_trace), w = E::domain_root(root, log2_lde);
    std::vector<uint32_t> class_of, order;
    std::vector<ExtR2Desc> classes;
    std::vector<ExtR2Step<E>> steps;
    r2_classes(tr, n_tr, class_of, classes);
    ext_r2_step_groups<E>(bnd, n_bnd, n, g, order, steps);
    ExtR2CycleArgs<E> ca;
    memset(&ca, 0, sizeof(ca));
    std::vector<word> roots;
    std::vector<uint64_t> root0;
    for (size_t k = 0; k < classes.size(); k++) {
        ca.cy[k] = ext_r2_cycle<E>(classes[k], log2_trace, log2_blowup, g);
        ca.cy[k].off = ca.total;
        ca.total += ca.cy[k].len;
        root0.push_back(roots.size());
        ext_r2_roots<E>(classes[k], n, g, roots);
    }
    // workspace: the tables uploaded at once, then the cycle tables and the table of the coset
    R2Arena t;
    const size_t s_ops = t.add((size_t)n_ops * 8), s_cells = t.add((size_t)n_cols * 16), s_consts = t.add((size_t)n_consts * 8), s_trans = t.add((size_t)n_tr * 32),
                 s_classes = t.add(classes.size() * 32), s_roots = t.add(roots.size() * 8), s_bnd = t.add((size_t)n_bnd * 32),
                 s_xcells = t.add(rap ? (size_t)rap->n_aux * 16 : 0), s_xconsts = t.add(rap ? (size_t)rap->n_xconsts * 16 : 0);
    const size_t tables = t.total;
    const uint32_t hbits = (log2_lde + 1) / 2;
    const uint64_t nlo = 1ull << hbits, nhi = 1ull << (log2_lde - hbits);
    const size_t s_cycle = t.add((size_t)ca.total * sizeof(word)), s_x = t.add((size_t)(nlo + nhi) * sizeof(word));
    int rc = air_tables_stage(c, t, tables);
    if (rc) return rc;
    ca.table = (word *)(t.dev + s_cycle);
    word *d_x = (word *)(t.dev + s_x);
    const ExtR2Domain<E> dom{d_x, d_x + nlo, hbits};
    bool any_aux = false;   // a boundary constraint on an auxiliary column: the boundary kernel's AUX form
    if (tables) {
        r2_fill_ops(t.h(s_ops), rap ? (const void *)rap->typed.data() : (const void *)ops, n_ops);
        r2_fill_cells(t.h(s_cells), cols, col_log2_len, n_cols, N);
        for (uint32_t k = 0; k < n_consts; k++) t.h(s_consts)[k] = E::fcanon(consts[k]);
        for (uint32_t k = 0; k < n_tr; k++) r2_fill_trans(t.h(s_trans), k, ext_elem_of<E>(tr[k].coeff, 0), class_of[k]);
        uint64_t *cl = t.h(s_classes);
        for (size_t k = 0; k < classes.size(); k++) {
            const uint64_t len = ca.cy[k].len;
            cl[4 * k] = (uint64_t)(uintptr_t)(ca.table + ca.cy[k].off);
            cl[4 * k + 1] = len;
            cl[4 * k + 2] = ((len & (len - 1)) == 0 ? 1u : 0u) | classes[k].end_exemptions << 32;
            cl[4 * k + 3] = root0[k];
        }
        for (size_t k = 0; k < roots.size(); k++) t.h(s_roots)[k] = roots[k];
        for (uint32_t q = 0; q < n_bnd; q++) {
            const B &b = bnd[order[q]];
            const bool on_aux = ext_r2_is_aux(b, 0);
            any_aux = any_aux || on_aux;
            r2_fill_bnd(t.h(s_bnd), q, on_aux ? rap->aux[b.col] : cols[b.col], on_aux ? rap->aux_stride : 0, ext_elem_of<E>(b.coeff, 0));
        }
        if (rap) {
            for (uint32_t k = 0; k < rap->n_aux; k++) {
                t.h(s_xcells)[2 * k] = (uint64_t)(uintptr_t)rap->aux[k];
                t.h(s_xcells)[2 * k + 1] = rap->aux_stride;
            }
            for (uint32_t k = 0; k < rap->n_xconsts; k++) r2_pack(ext_elem_of<E>(rap->xconsts, k), t.h(s_xconsts) + 2 * k);
        }
        if ((rc = air_tables_upload(c, t, tables, s))) return rc;
    }
    if (n_tr || n_bnd) {
        rc = launch_1d(c, names.xtable, ext_r2_xtable_kernel<E>, blocks_for(nlo + nhi), s, d_x, d_x + nlo, nlo, nhi, w, E::fpow(w, nlo), h);
        if (rc) return rc;
    }
    if (n_tr) {
        ca.n_classes = (uint32_t)classes.size();
        ca.h = h;
        ca.w = w;
        rc = launch_1d(c, names.cycle, ext_r2_cycle_kernel<E>, blocks_for((ca.total + EXT_ROWS - 1) / EXT_ROWS), s, ca);
        if (rc) return rc;
        ExtR2Args<E> a;
        memset(&a, 0, sizeof(a));
        a.ops = t.d(s_ops);
        a.cells = t.d(s_cells);
        a.consts = t.d(s_consts);
        a.trans = t.d(s_trans);
        a.classes = t.d(s_classes);
        a.roots = t.d(s_roots);
        if (rap) {
            a.xcells = t.d(s_xcells);
            a.xconsts = t.d(s_xconsts);
        }
        a.N = N;
        a.n_ops = n_ops;
        a.log2_blowup = log2_blowup;
        a.n_classes = ca.n_classes;
        a.n_slots = rap ? rap->n_slots : n_tmps;
        a.any_roots = !roots.empty();
        a.dom = dom;
        a.out = ext_planes<E>(d_out, out_stride);
        // plain: 16 slots, 32 KiB, at most; RAP: 8 D + 8 slots, 48 KiB (Fp2), 40 KiB (Fp4)
        const size_t lds = (size_t)(a.n_slots + a.n_classes) * sizeof(word) * EXT_THREADS;
        void (*kernel)(ExtR2Args<E>) = rap ? ext_r2_rap_transition_kernel<E> : ext_r2_transition_kernel<E>;
        hipEvent_t pe = c.prof_begin(s);
        hipLaunchKernelGGL(kernel, dim3(blocks_for(N)), dim3(EXT_THREADS), lds, s, a);
        c.prof_end(rap ? names.rap_transition : names.transition, pe, s);
        LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    } else if (n_bnd == 0) {
        for (int e = 0; e < E::D; e++) LW_HIP_CHECK(hipMemsetAsync(d_out + e * out_stride, 0, N * sizeof(word), s), LW_ERR_LAUNCH);
    }
    ExtR2BoundaryArgs<E> b;
    memset(&b, 0, sizeof(b));
    b.bnd = t.d(s_bnd);
    b.N = N;
    b.dom = dom;
    b.w = w;
    b.out = ext_planes<E>(d_out, out_stride);
    for (size_t s0 = 0; s0 < steps.size(); s0 += EXT_R2_STEPS) {
        const size_t S = steps.size() - s0 < (size_t)EXT_R2_STEPS ? steps.size() - s0 : (size_t)EXT_R2_STEPS;
        r2_fill_steps(b, steps, s0, S);
        b.accumulate = n_tr > 0 || s0 > 0;
        void (*kernel)(ExtR2BoundaryArgs<E>) = S == 1   ? ext_r2_boundary_kernel<E, E::R2_ROWS_FEW, 1>
                                               : S == 2 ? ext_r2_boundary_kernel<E, E::R2_ROWS_FEW, 2>
                                               : S == 3 ? ext_r2_boundary_kernel<E, EXT_ROWS, 3>
                                                        : ext_r2_boundary_kernel<E, EXT_ROWS, 4>;
        if (any_aux)
            kernel = S == 1   ? ext_r2_boundary_kernel<E, E::R2_ROWS_FEW, 1, true>
                     : S == 2 ? ext_r2_boundary_kernel<E, E::R2_ROWS_FEW, 2, true>
                     : S == 3 ? ext_r2_boundary_kernel<E, EXT_ROWS, 3, true>
                              : ext_r2_boundary_kernel<E, EXT_ROWS, 4, true>;
        const uint64_t rows = S <= 2 ? E::R2_ROWS_FEW : EXT_ROWS;
        rc = launch_1d(c, names.boundary, kernel, blocks_for((N + rows - 1) / rows), s, b);
        if (rc) return rc;
    }
    return LW_OK;
}

// The checks that the bodies of the entry points here and in circle_round2.cuh share, texts included.
static bool r2_null_tables(const void *consts, uint32_t n_consts, const void *boundary, uint32_t n_boundary, const void *transitions, uint32_t n_transitions,
                           const void *d_columns, uint32_t n_cols) {
    return (n_consts && n_consts <= LW_STARK_AIR_MAX_CONSTS && !consts) || (n_boundary && !boundary) || (n_transitions && !transitions) || (n_cols && !d_columns);
}
// boundary constraint k sits on main column col: in range and not a short column
static int r2_boundary_col_check(uint32_t k, uint32_t col, uint32_t n_cols, const uint32_t *col_log2_len_or_null, uint64_t lg) {
    if (col >= n_cols) { set_error("boundary constraint %u: column %u of %u", k, col, n_cols); return LW_ERR_BAD_ARG; }
    if (col_log2_len_or_null && col_log2_len_or_null[col] != lg) { set_error("boundary constraint %u: column %u is a short one", k, col); return LW_ERR_BAD_ARG; }
    return LW_OK;
}
static int r2_class_cap_check(size_t n_classes, int cap) {
    if (n_classes > (size_t)cap) { set_error("%zu distinct transition zerofiers: a call takes at most %d", n_classes, cap); return LW_ERR_BAD_ARG; }
    return LW_OK;
}
// out and its stride (0 becomes N), then every column: not null, aligned, not under out
template <class E>
static int r2_buffers_check(const typename E::word *d_out, size_t &out_stride, uint64_t N, const typename E::word *const *d_columns, const uint32_t *col_log2_len_or_null,
                            uint32_t n_cols) {
    int rc = ext_device_ptrs({d_out});
    if (!rc) rc = ext_stride(out_stride, N, "out");
    if (rc) return rc;
    for (uint32_t k = 0; k < n_cols; k++) {
        if (!d_columns[k] || !aligned16(d_columns[k])) { set_error("column %u: null or misaligned buffer", k); return LW_ERR_BAD_ARG; }
        if (ext_overlap<E>(d_columns[k], col_log2_len_or_null ? (size_t)1 << col_log2_len_or_null[k] : N, d_out, ext_span<E>(out_stride, N))) {
            set_error("out overlaps column %u", k);
            return LW_ERR_BAD_ARG;
        }
    }
    return LW_OK;
}

// The body of the entry points.  The order of the checks: the domain, null tables, the program, the words of the constants
// (then of the constants of E), the boundary entries, the transition entries and their classes, the device buffers (out, the
// columns, then the auxiliary stride and columns), the root and the offset, h^N = 1.  rap: the _rap_ entry points' additions
// (aux, n_aux, aux_stride, xconsts, n_xconsts; typed and n_slots are filled here), nullptr for the plain ones.
template <class E, class B, class T>
static int ext_r2_constraint_evaluations(const ExtR2Names &names, const lw_stark_air_op_t *ops, uint32_t n_ops, const typename E::word *consts, uint32_t n_consts,
                                         const typename E::word *const *d_columns, const uint32_t *col_log2_len_or_null, uint32_t n_cols, uint32_t log2_trace,
                                         uint32_t log2_blowup, const typename E::word *offset_or_null, uint64_t two_adic_root, const B *boundary,
                                         uint32_t n_boundary, const T *transitions, uint32_t n_transitions, typename E::word *d_out, size_t out_stride,
                                         void *hip_stream, ExtR2Rap<E> *rap = nullptr) {
    typedef unsigned __int128 u128;
    const uint64_t lg = (uint64_t)log2_trace + log2_blowup;
    if (lg > 63 || E::size_check((uint32_t)lg)) { set_error("an LDE domain of 2^%llu points is beyond the transform", (unsigned long long)lg); return LW_ERR_BAD_ARG; }
    const uint64_t n = 1ull << log2_trace, N = 1ull << lg;
    if (r2_null_tables(consts, n_consts, boundary, n_boundary, transitions, n_transitions, d_columns, n_cols) ||
        (rap && ((rap->n_xconsts && rap->n_xconsts <= LW_STARK_AIR_MAX_CONSTS && !rap->xconsts) || (rap->n_aux && !rap->aux)))) {
        set_error("null table");
        return LW_ERR_BAD_ARG;
    }
    AirProgramInfo info;
    int rc;
    if (rap) {
        char msg[192];
        rap->typed.assign(n_ops <= LW_STARK_AIR_MAX_OPS && ops ? n_ops : 0, 0);
        if (!air_program_check_rap(ops, n_ops, n_consts, rap->n_xconsts, col_log2_len_or_null, n_cols, rap->n_aux, E::D, log2_trace, (uint32_t)lg, n_transitions,
                                   rap->typed.empty() ? nullptr : rap->typed.data(), &info, msg, sizeof(msg))) {
            set_error("AIR program: %s", msg);
            return LW_ERR_BAD_ARG;
        }
        rap->n_slots = info.n_lds_slots;
    } else if ((rc = air_program_checked(ops, n_ops, n_consts, col_log2_len_or_null, n_cols, log2_trace, (uint32_t)lg, n_transitions, &info))) {
        return rc;
    }
    rc = E::words_check(consts, n_consts, "constants");
    if (!rc && rap) rc = E::words_check(rap->xconsts, (size_t)rap->n_xconsts * E::D, "extension constants");
    if (rc) return rc;
    for (uint32_t k = 0; k < n_boundary; k++) {
        const B &b = boundary[k];
        if (ext_r2_is_aux(b, 0)) {
            if (b.col >= rap->n_aux) { set_error("boundary constraint %u: auxiliary column %u of %u", k, b.col, rap->n_aux); return LW_ERR_BAD_ARG; }
        } else if ((rc = r2_boundary_col_check(k, b.col, n_cols, col_log2_len_or_null, lg))) {
            return rc;
        }
        if ((rc = ext_r2_value_check<E>(b.value)) || (rc = E::words_check(b.coeff, E::D, "boundary coefficient"))) return rc;
    }
    for (uint32_t k = 0; k < n_transitions; k++) {
        const T &t = transitions[k];
        if (t.period == 0) { set_error("transition %u: period 0", k); return LW_ERR_BAD_ARG; }
        if (t.end_exemptions && (t.end_exemptions > n || t.period > n / t.end_exemptions)) {
            set_error("transition %u: %llu end exemptions of period %llu exceed the trace", k, (unsigned long long)t.end_exemptions, (unsigned long long)t.period);
            return LW_ERR_BAD_ARG;
        }
        if ((rc = E::words_check(t.coeff, E::D, "transition coefficient"))) return rc;
    }
    std::vector<uint32_t> class_of;
    std::vector<ExtR2Desc> classes;
    r2_classes(transitions, n_transitions, class_of, classes);
    if ((rc = r2_class_cap_check(classes.size(), EXT_R2_CLASSES)) || (rc = r2_buffers_check<E>(d_out, out_stride, N, d_columns, col_log2_len_or_null, n_cols))) return rc;
    if (rap) {
        if ((rc = ext_stride(rap->aux_stride, N, "auxiliary columns"))) return rc;
        for (uint32_t k = 0; k < rap->n_aux; k++) {
            if (!rap->aux[k] || !aligned16(rap->aux[k])) { set_error("auxiliary column %u: null or misaligned buffer", k); return LW_ERR_BAD_ARG; }
            if (ext_overlap<E>(rap->aux[k], ext_span<E>(rap->aux_stride, N), d_out, ext_span<E>(out_stride, N))) {
                set_error("out overlaps auxiliary column %u", k);
                return LW_ERR_BAD_ARG;
            }
        }
    }
    typename E::word h;
    rc = E::root_check(two_adic_root);
    if (!rc) rc = E::offset(offset_or_null, h);
    if (rc) return rc;
    if (n_boundary || n_transitions) {
        // x_i = g^step, or x_i^(n / period) = g^(...) with period | n, for some i exactly when x_i^n = 1: when h^N = 1.  A
        // period that does not divide n (the division truncates to m) can vanish only where x_i^(m n) = 1.
        const typename E::word hN = E::fpow(h, N);
        bool zero = hN == E::F_ONE;
        const typename E::word g = E::domain_root(two_adic_root, log2_trace);
        for (const ExtR2Desc &d : classes)
            if (n % d.period) {
                const uint64_t m = n / d.period;
                zero = zero || (m ? E::fpow(hN, m) == E::F_ONE : E::fpow(g, (uint64_t)((u128)d.offset * n / d.period % n)) == E::F_ONE);
            }
        if (zero) { set_error("the coset offset lies in the LDE domain (h^N = 1): a zerofier vanishes on it"); return LW_ERR_INV_ZERO; }
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return ext_r2_constraints_locked<E>(en.c, names, ops, n_ops, consts, n_consts, d_columns, col_log2_len_or_null, n_cols, log2_trace, log2_blowup, h, two_adic_root,
                                        boundary, n_boundary, transitions, n_transitions, info.n_tmps, d_out, out_stride, en.stream, rap);
}

// ---------------------------------------------------------------- host: the parts
static uint32_t ext_r2_parts_log2_block(uint32_t log2_lde, uint32_t n_parts) {   // next_power_of_two(ceil(N / P))
    const uint64_t per = ((1ull << log2_lde) + n_parts - 1) / n_parts;
    uint32_t x = 0;
    while ((1ull << x) < per) x++;
    return x;
}

// interpolate_offset_fft plane by plane -> break_in_parts -> the LDE of every plane of every part.
// inverse(c, d_in, in_stride, d_out, out_stride, log2n, s): the extension's inverse transform of D planes on the coset;
// lde(c, d_coeffs, log2_coeffs, d_out, log2n, batch, s): its LDE of dense blocks onto dense planes of the same coset.
template <class E, class Inverse, class Lde>
static int ext_r2_composition_parts(const ExtR2Names &names, const typename E::word *d_evals, size_t evals_stride, uint32_t log2_lde,
                                    const typename E::word *offset_or_null, uint64_t two_adic_root, uint32_t n_parts, typename E::word *d_parts_coeffs,
                                    typename E::word *d_parts_lde_or_null, size_t *out_part_lens_or_null, void *hip_stream, Inverse inverse, Lde lde) {
    using word = typename E::word;
    if (log2_lde > 63 || E::size_check(log2_lde)) { set_error("an LDE domain of 2^%u points is beyond the transform", log2_lde); return LW_ERR_BAD_ARG; }
    const uint64_t N = 1ull << log2_lde;
    if (n_parts == 0 || n_parts > N) { set_error("%u parts of a polynomial of 2^%u coefficients", n_parts, log2_lde); return LW_ERR_BAD_ARG; }
    int rc = d_parts_lde_or_null ? ext_device_ptrs({d_evals, d_parts_coeffs, d_parts_lde_or_null}) : ext_device_ptrs({d_evals, d_parts_coeffs});
    if (!rc) rc = ext_stride(evals_stride, N, "evaluations");
    if (rc) return rc;
    const uint32_t log2_L = ext_r2_parts_log2_block(log2_lde, n_parts);
    const size_t planes = (size_t)n_parts * E::D, coeff_words = planes << log2_L, lde_words = planes << log2_lde;
    if (ext_overlap<E>(d_parts_coeffs, coeff_words, d_evals, ext_span<E>(evals_stride, N)) ||
        (d_parts_lde_or_null && (ext_overlap<E>(d_parts_lde_or_null, lde_words, d_evals, ext_span<E>(evals_stride, N)) ||
                                 ext_overlap<E>(d_parts_lde_or_null, lde_words, d_parts_coeffs, coeff_words)))) {
        set_error("the buffers of the parts overlap");
        return LW_ERR_BAD_ARG;
    }
    word h;
    rc = E::root_check(two_adic_root);
    if (!rc) rc = E::offset(offset_or_null, h);
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.stream;
    const size_t b_H = r2_round256((size_t)E::D * N * sizeof(word));
    if (c.pipe_tmp.ensure(b_H + (size_t)n_parts * 8)) return LW_ERR_ALLOC;
    word *d_H = (word *)c.pipe_tmp.p;
    unsigned long long *d_lens = (unsigned long long *)((char *)c.pipe_tmp.p + b_H);
    rc = inverse(c, d_evals, evals_stride, d_H, N, log2_lde, h, two_adic_root, s);
    if (rc) return rc;
    const uint64_t items = (uint64_t)n_parts << log2_L;
    rc = launch_1d(c, names.split, ext_r2_split_kernel<E>, blocks_for(items), s, ext_planes<E>(d_H, N), N, (uint64_t)n_parts, log2_L, d_parts_coeffs);
    if (rc) return rc;
    if (d_parts_lde_or_null) {
        rc = lde(c, d_parts_coeffs, log2_L, d_parts_lde_or_null, log2_lde, (uint32_t)planes, h, two_adic_root, s);
        if (rc) return rc;
    }
    if (!out_part_lens_or_null) return LW_OK;
    LW_HIP_CHECK(hipMemsetAsync(d_lens, 0, (size_t)n_parts * 8, s), LW_ERR_LAUNCH);
    rc = launch_1d(c, names.lengths, ext_r2_lengths_kernel<E>, blocks_for(items), s, (const word *)d_parts_coeffs, (uint64_t)n_parts, log2_L, d_lens);
    if (rc) return rc;
    std::vector<unsigned long long> lens(n_parts);
    rc = download(lens.data(), d_lens, (size_t)n_parts * 8, s);
    if (rc) return rc;
    for (uint32_t j = 0; j < n_parts; j++) out_part_lens_or_null[j] = (size_t)lens[j];
    return LW_OK;
}

}  // namespace lw
