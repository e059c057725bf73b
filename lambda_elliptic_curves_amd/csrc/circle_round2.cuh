// Circle STARK round 2 over Mersenne31 with QM31, for mersenne31_ext.hip: the evaluations of the composition polynomial on the
// LDE coset in ONE pass over the LDE columns, and its parts.  The counterpart of ext_round2.cuh on the circle: the domain is
// the standard coset q_i = g_{2N} + i g_N, the zerofiers are coordinates of doubled points, a single point has no linear
// factor and the parts are index blocks.
//
//   out[i] = sum_c beta_c T_c(i) E_c(q_i) / Z_c(q_i)  +  sum_k gamma_k (col_k[i] - v_k) (1 + x'_k) / y'_k          out[i] in QM31
//
// T_c(i) is what the AIR's program (lw_stark_air_op_t, checked by air_program.h) leaves in the accumulator at EMIT c.  For a
// transition {period, offset, end_exemptions} with m = n / period = 2^mu and c = p_offset (p_j = g_{2n} + j g_n):
//   Z(Q) = y(2^(mu-1) (Q - c))                  simple zeros at the trace rows j = offset mod period; on the LDE coset of period
//                                               2 B period in i and never zero for B >= 2
//   E(Q) = prod_k (1 - (P_k.x Q.x + P_k.y Q.y)) P_k = p_(offset + (m - k) period), k = 1 .. end_exemptions: 1 - x(Q - P_k), the
//                                               line with a double zero at P_k
// and for a boundary constraint {col, step, value}: (x', y') = q_i - p_step, whose y' vanishes at p_step and its antipode only.
//
// m31q_r2_table_kernel      the two-level table of the LDE coset: lo[a] = a g_N, hi[b] = g_{2N} + b 2^hbits g_N, so that q_i is
//                           one circle addition (4 products) and two 8-byte loads
// m31q_r2_cycle_kernel      1 / Z of the distinct transition descriptors (M31Q_R2_CLASSES at most), back to back, 2 B period
//                           entries each; M31Q_R2_CYCLE_ROWS entries of a work-item share one m31_inv
// m31q_r2_transition_kernel one work-item per LDE row.  It first forms E(q_i) cycle[i & mask] of every class and keeps it in
//                           LDS, then runs the program with air_run (air_interp.cuh) over words of M31qExt and at EMIT c
//                           folds beta_c (class value x acc) into its QM31 accumulator with m31q_mul_base.  Temporaries and
//                           class values live in dynamic LDS as [slot][lane] words.  No T_c is stored.
// m31q_r2_boundary_kernel   up to M31Q_R2_STEPS distinct steps per launch, R consecutive rows per work-item: the R x S
//                           denominators y' share ONE m31_inv (Montgomery's trick), the numerators sum_k gamma_k col_k[i] - c_s
//                           (c_s = sum_k gamma_k v_k is the host's) are formed on the way back and multiplied by
//                           (1 + x') / y' with m31q_mul_base.  Adds into out.
// m31q_r2_tail_kernel       the number of non-zero words of the interpolated planes at or above an index
//
// The host tables (classes, exemption points, step groups, point-table parameters) are plain arithmetic without a Context:
// tests/circle_round2_host_main.cpp takes them alone (LW_CIRCLE_R2_TABLES_ONLY) and runs them under sanitizers.
#pragma once
#include <algorithm>
#include <vector>
#include "mersenne31_ext.cuh"
#include "r2_tables.h"

namespace lw {

constexpr int M31Q_R2_CLASSES = 8;      // distinct transition descriptors per call (their per-row values are LDS slots)
constexpr int M31Q_R2_STEPS = 4;        // distinct boundary steps per launch
constexpr int M31Q_R2_ROWS = 4;         // boundary rows per work-item: M31Q_R2_ROWS x M31Q_R2_STEPS denominators per inversion
constexpr int M31Q_R2_CYCLE_ROWS = 4;   // cycle entries per work-item; every table is a multiple of it long (B >= 2)

// ---------------------------------------------------------------- host tables: plain arithmetic, no Context
// a - c in the circle group
M31Q_HD CirclePt circle_sub(CirclePt a, CirclePt c) {
    return CirclePt{m31_add(m31_mul(a.x, c.x), m31_mul(a.y, c.y)), m31_sub(m31_mul(a.y, c.x), m31_mul(a.x, c.y))};
}
// g_{2^k} = 2^(31-k) G, k <= 31
static inline CirclePt circle_r2_gen(uint32_t k) {
    CirclePt q{2u, 1268011823u};   // the generator of the circle group, order 2^31 (circle/point.rs)
    for (uint32_t d = k; d < 31; d++) q = circle_double(q);
    return q;
}
// trace point p_j = g_{2n} + j g_n = (2j + 1) g_{2n}, j < n = 2^log2_trace <= 2^30
static inline CirclePt circle_r2_trace_point(uint32_t log2_trace, uint64_t j) { return circle_mul((uint32_t)(2 * j + 1), circle_r2_gen(log2_trace + 1)); }

struct CircleR2Desc {   // a transition's zerofier: the classes of r2_classes
    uint64_t period, offset, end_exemptions;
    template <class T> static CircleR2Desc of(const T &t) { return CircleR2Desc{t.period, t.offset, t.end_exemptions}; }
    bool operator==(const CircleR2Desc &o) const { return period == o.period && offset == o.offset && end_exemptions == o.end_exemptions; }
};
// the name under which tests/circle_round2_host_main.cpp calls r2_classes
template <class T> static void circle_r2_classes(const T *tr, uint32_t n_tr, std::vector<uint32_t> &class_of, std::vector<CircleR2Desc> &classes) { r2_classes(tr, n_tr, class_of, classes); }
// a class's cycle: cycle[e] = 1 / y(2^doublings (q_e - c)), e < len = 2 B period (a power of two, at most N)
struct CircleR2Cycle {
    CirclePt c;
    uint32_t doublings;
    uint64_t off, len;
};
static inline CircleR2Cycle circle_r2_cycle(const CircleR2Desc &d, uint32_t log2_trace, uint32_t log2_blowup) {
    uint32_t mu = 0;
    while ((d.period << mu) < (1ull << log2_trace)) mu++;   // m = n / period = 2^mu, mu >= 1
    CircleR2Cycle cy{};
    cy.c = circle_r2_trace_point(log2_trace, d.offset);
    cy.doublings = mu - 1;
    cy.len = (d.period << log2_blowup) * 2;
    return cy;
}
// the class's exemption points P_k = p_(offset + (m - k) period), k = 1 .. end_exemptions, as the words x | y << 32 (canonical)
static inline void circle_r2_exemption_points(const CircleR2Desc &d, uint32_t log2_trace, std::vector<uint64_t> &pts) {
    const uint64_t m = (1ull << log2_trace) / d.period;
    for (uint64_t k = 1; k <= d.end_exemptions; k++) {
        const CirclePt p = circle_r2_trace_point(log2_trace, d.offset + (m - k) * d.period);
        pts.push_back((uint64_t)m31_canon(p.x) | (uint64_t)m31_canon(p.y) << 32);
    }
}
// boundary constraints by distinct step (below n), stable: order[q] is the constraint at place q, steps[s] covers the places
// [first, first + count)
struct CircleR2Step {
    uint64_t step;
    CirclePt point;   // p_step
    uint32_t first, count;
    Qm31 constant;    // sum_k gamma_k v_k over the step's constraints
};
template <class B> static void circle_r2_step_groups(const B *bnd, uint32_t n_bnd, uint32_t log2_trace, std::vector<uint32_t> &order, std::vector<CircleR2Step> &steps) {
    order.resize(n_bnd);
    for (uint32_t k = 0; k < n_bnd; k++) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return bnd[x].step < bnd[y].step; });
    steps.clear();
    for (uint32_t q = 0; q < n_bnd; q++) {
        const B &b = bnd[order[q]];
        if (q == 0 || b.step != bnd[order[q - 1]].step) steps.push_back(CircleR2Step{b.step, circle_r2_trace_point(log2_trace, b.step), q, 0, m31q_zero()});
        steps.back().count++;
        steps.back().constant = m31q_add(steps.back().constant, m31q_mul_base(m31q_from_words(b.coeff), m31_from_word(b.value)));
    }
}
// the two-level point table of the LDE coset: q_i = lo[i & (2^hbits - 1)] + hi[i >> hbits]
struct CircleR2Table {
    uint32_t hbits;
    uint64_t nlo, nhi;
    CirclePt g2N, gN;
};
static inline CircleR2Table circle_r2_table(uint32_t log2_lde) {
    CircleR2Table t;
    t.hbits = (log2_lde + 1) / 2;
    t.nlo = 1ull << t.hbits;
    t.nhi = 1ull << (log2_lde - t.hbits);
    t.g2N = circle_r2_gen(log2_lde + 1);
    t.gN = circle_r2_gen(log2_lde);
    return t;
}

}  // namespace lw

#ifndef LW_CIRCLE_R2_TABLES_ONLY
#include "ext_round2.cuh"   // air_interp.cuh, and the checks the entry bodies share

namespace lw {

// ---------------------------------------------------------------- kernels
struct M31qR2Domain {
    const uint2 *lo, *hi;
    uint32_t hbits;
};
__device__ __forceinline__ CirclePt m31q_r2_point(const M31qR2Domain d, uint64_t i) {
    const uint2 l = d.lo[i & ((1ull << d.hbits) - 1)], h = d.hi[i >> d.hbits];
    return circle_add(CirclePt{h.x, h.y}, CirclePt{l.x, l.y});
}
// lo[a] = a g_N = 2a g_{2N}; hi[b] = g_{2N} + b 2^hbits g_N = (1 + b 2^(hbits+1)) g_{2N}, the multiplier below 2^31
__global__ __launch_bounds__(M31Q_THREADS) void m31q_r2_table_kernel(uint2 *lo, uint2 *hi, uint64_t nlo, uint64_t nhi, uint32_t hbits, CirclePt g2N) {
    const uint64_t i = (uint64_t)blockIdx.x * M31Q_THREADS + threadIdx.x;
    if (i < nlo) {
        const CirclePt p = i ? circle_mul((uint32_t)(2 * i), g2N) : CirclePt{1u, 0u};
        lo[i] = make_uint2(p.x, p.y);
    } else if (i - nlo < nhi) {
        const CirclePt p = circle_mul((uint32_t)(1 + ((i - nlo) << (hbits + 1))), g2N);
        hi[i - nlo] = make_uint2(p.x, p.y);
    }
}

struct M31qR2CycleArgs {
    CircleR2Cycle cy[M31Q_R2_CLASSES];
    uint32_t n_classes;
    uint64_t total;
    CirclePt g2N, gN;
    uint32_t *table;
};
__global__ __launch_bounds__(M31Q_THREADS) void m31q_r2_cycle_kernel(const M31qR2CycleArgs a) {
    const uint64_t i0 = ((uint64_t)blockIdx.x * M31Q_THREADS + threadIdx.x) * M31Q_R2_CYCLE_ROWS;
    if (i0 >= a.total) return;
    // the work-item's table, by selects over constant indices (a lane's own index would copy the struct to private memory);
    // every table is a multiple of M31Q_R2_CYCLE_ROWS long, so the rows of a work-item are one table's
    CircleR2Cycle cy = a.cy[0];
#pragma unroll
    for (int t = 1; t < M31Q_R2_CLASSES; t++)
        if ((uint32_t)t < a.n_classes && i0 >= a.cy[t].off) cy = a.cy[t];
    CirclePt q = circle_mul((uint32_t)(2 * (i0 - cy.off) + 1), a.g2N);   // q_e = (2e + 1) g_{2N}
    uint32_t den[M31Q_R2_CYCLE_ROWS], pre[M31Q_R2_CYCLE_ROWS];
    uint32_t run = 1u;
#pragma unroll
    for (int r = 0; r < M31Q_R2_CYCLE_ROWS; r++) {
        CirclePt d = circle_sub(q, cy.c);
#pragma unroll 1
        for (uint32_t k = 0; k < cy.doublings; k++) d = circle_double(d);
        den[r] = d.y;   // not zero: the host refuses a blow-up of 1
        pre[r] = run;
        run = m31_mul(run, den[r]);
        q = circle_add(q, a.gN);
    }
    uint32_t inv = m31_inv(run);
#pragma unroll
    for (int r = M31Q_R2_CYCLE_ROWS - 1; r >= 0; r--) {
        if (i0 + r < a.total) a.table[i0 + r] = m31_mul(inv, pre[r]);
        inv = m31_mul(inv, den[r]);
    }
}

// The sections of air_interp.cuh (a constant is a word in [0, p]), and
//   classes  per class: the address of its cycle table, the table's length - 1, its number of exemption points, the first of them
//   expts    per exemption point: x | y << 32
struct M31qR2Args {
    const uint64_t *ops, *cells, *consts, *trans, *classes, *expts;
    uint64_t N;
    uint32_t n_ops, log2_blowup, n_classes, n_tmps, any_expts;
    M31qR2Domain dom;
    M31qPlanes out;
};

extern __shared__ uint32_t m31q_r2_lds[];   // [slot][lane] words: the program's temporaries, then the classes' values

__global__ __launch_bounds__(M31Q_THREADS) void m31q_r2_transition_kernel(const M31qR2Args a) {
    uint32_t *lds = m31q_r2_lds;
    const uint64_t i = (uint64_t)blockIdx.x * M31Q_THREADS + threadIdx.x;
    if (i >= a.N) return;
    const CirclePt q = a.any_expts ? m31q_r2_point(a.dom, i) : CirclePt{1u, 0u};
#pragma unroll 1
    for (uint32_t k = 0; k < a.n_classes; k++) {
        const uint32_t *cycle = (const uint32_t *)air_uniform(a.classes, 4 * k);
        const uint64_t mask = air_uniform(a.classes, 4 * k + 1), n_ex = air_uniform(a.classes, 4 * k + 2), ex0 = air_uniform(a.classes, 4 * k + 3);
        uint32_t v = cycle[i & mask];
#pragma unroll 1
        for (uint64_t r = 0; r < n_ex; r++) {
            const uint64_t pt = air_uniform(a.expts, ex0 + r);
            v = m31_mul(v, m31_sub(1u, m31_add(m31_mul((uint32_t)pt, q.x), m31_mul((uint32_t)(pt >> 32), q.y))));
        }
        lds[(a.n_tmps + k) * M31Q_THREADS + threadIdx.x] = v;
    }
    Qm31 sum = m31q_zero();
    const uint64_t *trans = a.trans;
    const uint32_t n_tmps = a.n_tmps;
    air_run<AirWord<M31qExt, M31Q_THREADS>>(a.ops, a.n_ops, a.cells, a.consts, lds, i, a.log2_blowup, [&sum, trans, lds, n_tmps](uint32_t c, uint32_t acc) {
        // no row T_c, the term goes onto the sum
        const uint32_t cls = (uint32_t)air_uniform(trans, 4 * c + 2);
        sum = m31q_add(sum, m31q_mul_base(air_uniform_elem<Qm31>(trans, 4 * c), m31_mul(lds[(n_tmps + cls) * M31Q_THREADS + threadIdx.x], acc)));
    });
    M31qExt::store(a.out, i, sum);
}

// bnd: the section of air_interp.cuh
struct M31qR2BoundaryArgs {
    const uint64_t *bnd;
    uint64_t N;
    uint32_t accumulate;
    M31qR2Domain dom;
    CirclePt gN;
    CirclePt point[M31Q_R2_STEPS];
    uint32_t first[M31Q_R2_STEPS], count[M31Q_R2_STEPS];
    Qm31 constant[M31Q_R2_STEPS];
    M31qPlanes out;
};

// The way forward forms the denominators y' alone; a step's numerators and its 1 + x' are formed on the way back, when the
// step's inverses are due, so that only the denominators and their running products stay live across the inversion.
template <int R, int S> __global__ __launch_bounds__(M31Q_THREADS) void m31q_r2_boundary_kernel(const M31qR2BoundaryArgs a) {
    const uint64_t row0 = ((uint64_t)blockIdx.x * M31Q_THREADS + threadIdx.x) * R;
    if (row0 >= a.N) return;
    CirclePt q[R];
    q[0] = m31q_r2_point(a.dom, row0);
#pragma unroll
    for (int r = 1; r < R; r++) q[r] = circle_add(q[r - 1], a.gN);
    uint32_t d[S][R], pre[S][R];
    uint32_t run = 1u;
#pragma unroll
    for (int s = 0; s < S; s++)
#pragma unroll
        for (int r = 0; r < R; r++) {
            d[s][r] = m31_sub(m31_mul(q[r].y, a.point[s].x), m31_mul(q[r].x, a.point[s].y));   // y(q - p_step): not zero off the trace domain
            pre[s][r] = run;
            run = m31_mul(run, d[s][r]);
        }
    uint32_t inv = m31_inv(run);
    Qm31 sum[R];
#pragma unroll
    for (int r = 0; r < R; r++) sum[r] = m31q_zero();
#pragma unroll
    for (int s = S - 1; s >= 0; s--) {
        Qm31 t[R];
#pragma unroll
        for (int r = 0; r < R; r++) t[r] = m31q_zero();
#pragma unroll 1
        for (uint32_t k = a.first[s]; k < a.first[s] + a.count[s]; k++) {
            const uint32_t *col = (const uint32_t *)air_uniform(a.bnd, 4 * k) + row0;
            const Qm31 gamma = air_uniform_elem<Qm31>(a.bnd, 4 * k + 2);
#pragma unroll
            for (int r = 0; r < R; r++)
                if (row0 + r < a.N) t[r] = m31q_add(t[r], m31q_mul_base(gamma, m31_from_word(col[r])));   // N < R: the rows past the domain
        }
#pragma unroll
        for (int r = R - 1; r >= 0; r--) {
            const uint32_t x1 = m31_add(1u, m31_add(m31_mul(q[r].x, a.point[s].x), m31_mul(q[r].y, a.point[s].y)));   // 1 + x(q - p_step)
            sum[r] = m31q_add(sum[r], m31q_mul_base(m31q_sub(t[r], a.constant[s]), m31_mul(x1, m31_mul(inv, pre[s][r]))));
            inv = m31_mul(inv, d[s][r]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (row0 + r >= a.N) break;
        Qm31 o = sum[r];
        if (a.accumulate) o = m31q_add(o, M31qExt::load(a.out, row0 + r));
        M31qExt::store(a.out, row0 + r, o);
    }
}

// *count += the non-zero words of the four dense planes of N words at the indices from `first` on (canonical words)
__global__ __launch_bounds__(M31Q_THREADS) void m31q_r2_tail_kernel(const uint32_t *H, uint64_t N, uint64_t first, unsigned long long *count) {
    const uint64_t tail = N - first, total = 4 * tail, step = (uint64_t)gridDim.x * M31Q_THREADS;
    unsigned long long mine = 0;
    for (uint64_t idx = (uint64_t)blockIdx.x * M31Q_THREADS + threadIdx.x; idx < total; idx += step) mine += H[(idx / tail) * N + first + idx % tail] != 0;
    if (mine) atomicAdd(count, mine);   // a polynomial whose degree fits adds nothing
}

// ---------------------------------------------------------------- host: the constraint evaluations
// cols: n_cols device pointers (host array).  Everything is checked; enqueue only.
static int m31q_r2_constraints_locked(Context &c, const lw_stark_air_op_t *ops, uint32_t n_ops, const uint32_t *consts, uint32_t n_consts, const uint32_t *const *cols,
                                      const uint32_t *col_log2_len, uint32_t n_cols, uint32_t log2_trace, uint32_t log2_blowup, const lw_m31q_boundary_t *bnd,
                                      uint32_t n_bnd, const lw_m31q_transition_t *tr, uint32_t n_tr, uint32_t n_tmps, uint32_t *d_out, uint64_t out_stride,
                                      hipStream_t s) {
    const uint32_t log2_lde = log2_trace + log2_blowup;
    const uint64_t N = 1ull << log2_lde;
    std::vector<uint32_t> class_of, order;
    std::vector<CircleR2Desc> classes;
    std::vector<CircleR2Step> steps;
    r2_classes(tr, n_tr, class_of, classes);
    circle_r2_step_groups(bnd, n_bnd, log2_trace, order, steps);
    M31qR2CycleArgs ca;
    memset(&ca, 0, sizeof(ca));
    std::vector<uint64_t> expts, ex0;
    for (size_t k = 0; k < classes.size(); k++) {
        ca.cy[k] = circle_r2_cycle(classes[k], log2_trace, log2_blowup);
        ca.cy[k].off = ca.total;
        ca.total += ca.cy[k].len;
        ex0.push_back(expts.size());
        circle_r2_exemption_points(classes[k], log2_trace, expts);
    }
    // workspace: the tables uploaded at once, then the cycle tables and the point table
    R2Arena t;
    const size_t s_ops = t.add((size_t)n_ops * 8), s_cells = t.add((size_t)n_cols * 16), s_consts = t.add((size_t)n_consts * 8), s_trans = t.add((size_t)n_tr * 32),
                 s_classes = t.add(classes.size() * 32), s_expts = t.add(expts.size() * 8), s_bnd = t.add((size_t)n_bnd * 32);
    const size_t tables = t.total;
    const CircleR2Table pt = circle_r2_table(log2_lde);
    const size_t s_cycle = t.add((size_t)ca.total * sizeof(uint32_t)), s_pts = t.add((size_t)(pt.nlo + pt.nhi) * sizeof(uint2));
    int rc = air_tables_stage(c, t, tables);
    if (rc) return rc;
    ca.table = (uint32_t *)(t.dev + s_cycle);
    uint2 *d_pts = (uint2 *)(t.dev + s_pts);
    const M31qR2Domain dom{d_pts, d_pts + pt.nlo, pt.hbits};
    if (tables) {
        r2_fill_ops(t.h(s_ops), ops, n_ops);
        r2_fill_cells(t.h(s_cells), cols, col_log2_len, n_cols, N);
        for (uint32_t k = 0; k < n_consts; k++) t.h(s_consts)[k] = m31_from_word(consts[k]);
        for (uint32_t k = 0; k < n_tr; k++) r2_fill_trans(t.h(s_trans), k, m31q_from_words(tr[k].coeff), class_of[k]);
        uint64_t *cl = t.h(s_classes);
        for (size_t k = 0; k < classes.size(); k++) {
            cl[4 * k] = (uint64_t)(uintptr_t)(ca.table + ca.cy[k].off);
            cl[4 * k + 1] = ca.cy[k].len - 1;
            cl[4 * k + 2] = classes[k].end_exemptions;
            cl[4 * k + 3] = ex0[k];
        }
        for (size_t k = 0; k < expts.size(); k++) t.h(s_expts)[k] = expts[k];
        for (uint32_t q = 0; q < n_bnd; q++) r2_fill_bnd(t.h(s_bnd), q, cols[bnd[order[q]].col], 0, m31q_from_words(bnd[order[q]].coeff));
        if ((rc = air_tables_upload(c, t, tables, s))) return rc;
    }
    if (n_bnd || !expts.empty()) {   // the boundary kernel's points, and the transition kernel's when a class has exemptions
        rc = launch_1d(c, "m31q_r2_table_kernel", m31q_r2_table_kernel, blocks_for(pt.nlo + pt.nhi), s, d_pts, d_pts + pt.nlo, pt.nlo, pt.nhi, pt.hbits, pt.g2N);
        if (rc) return rc;
    }
    if (n_tr) {
        ca.n_classes = (uint32_t)classes.size();
        ca.g2N = pt.g2N;
        ca.gN = pt.gN;
        rc = launch_1d(c, "m31q_r2_cycle_kernel", m31q_r2_cycle_kernel, blocks_for((ca.total + M31Q_R2_CYCLE_ROWS - 1) / M31Q_R2_CYCLE_ROWS), s, ca);
        if (rc) return rc;
        M31qR2Args a;
        memset(&a, 0, sizeof(a));
        a.ops = t.d(s_ops);
        a.cells = t.d(s_cells);
        a.consts = t.d(s_consts);
        a.trans = t.d(s_trans);
        a.classes = t.d(s_classes);
        a.expts = t.d(s_expts);
        a.N = N;
        a.n_ops = n_ops;
        a.log2_blowup = log2_blowup;
        a.n_classes = ca.n_classes;
        a.n_tmps = n_tmps;
        a.any_expts = !expts.empty();
        a.dom = dom;
        a.out = ext_planes<M31qExt>(d_out, out_stride);
        const size_t lds = (size_t)(n_tmps + a.n_classes) * sizeof(uint32_t) * M31Q_THREADS;   // 16 slots, 16 KiB, at most
        hipEvent_t pe = c.prof_begin(s);
        hipLaunchKernelGGL(m31q_r2_transition_kernel, dim3(blocks_for(N)), dim3(M31Q_THREADS), lds, s, a);
        c.prof_end("m31q_r2_transition_kernel", pe, s);
        LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    } else if (n_bnd == 0) {
        for (int e = 0; e < 4; e++) LW_HIP_CHECK(hipMemsetAsync(d_out + e * out_stride, 0, N * sizeof(uint32_t), s), LW_ERR_LAUNCH);
    }
    M31qR2BoundaryArgs b;
    memset(&b, 0, sizeof(b));
    b.bnd = t.d(s_bnd);
    b.N = N;
    b.dom = dom;
    b.gN = pt.gN;
    b.out = ext_planes<M31qExt>(d_out, out_stride);
    for (size_t s0 = 0; s0 < steps.size(); s0 += M31Q_R2_STEPS) {
        const size_t S = steps.size() - s0 < (size_t)M31Q_R2_STEPS ? steps.size() - s0 : (size_t)M31Q_R2_STEPS;
        r2_fill_steps(b, steps, s0, S);
        b.accumulate = n_tr > 0 || s0 > 0;
        void (*kernel)(M31qR2BoundaryArgs) = S == 1   ? m31q_r2_boundary_kernel<M31Q_R2_ROWS, 1>
                                             : S == 2 ? m31q_r2_boundary_kernel<M31Q_R2_ROWS, 2>
                                             : S == 3 ? m31q_r2_boundary_kernel<M31Q_R2_ROWS, 3>
                                                      : m31q_r2_boundary_kernel<M31Q_R2_ROWS, 4>;
        rc = launch_1d(c, "m31q_r2_boundary_kernel", kernel, blocks_for((N + M31Q_R2_ROWS - 1) / M31Q_R2_ROWS), s, b);
        if (rc) return rc;
    }
    return LW_OK;
}

// The body of the entry point.  The order of the checks: the domain, null tables, the program, the boundary entries, the
// transition entries and their classes, the device buffers, a blow-up of 1 with a constraint present.
static int m31q_r2_constraint_evaluations(const lw_stark_air_op_t *ops, uint32_t n_ops, const uint32_t *consts, uint32_t n_consts, const uint32_t *const *d_columns,
                                          const uint32_t *col_log2_len_or_null, uint32_t n_cols, uint32_t log2_trace, uint32_t log2_blowup,
                                          const lw_m31q_boundary_t *boundary, uint32_t n_boundary, const lw_m31q_transition_t *transitions, uint32_t n_transitions,
                                          uint32_t *d_out, size_t out_stride, void *hip_stream) {
    const uint64_t lg = (uint64_t)log2_trace + log2_blowup;
    if (log2_trace < 1 || lg > (uint64_t)M31Q_MAX_LOG) {
        set_error("a trace of 2^%u rows under a blow-up of 2^%u: the trace has at least 2 rows, the LDE coset at most 2^%d points", log2_trace, log2_blowup, M31Q_MAX_LOG);
        return LW_ERR_BAD_ARG;
    }
    const uint64_t n = 1ull << log2_trace, N = 1ull << lg;
    if (r2_null_tables(consts, n_consts, boundary, n_boundary, transitions, n_transitions, d_columns, n_cols)) {
        set_error("null table");
        return LW_ERR_BAD_ARG;
    }
    AirProgramInfo info;
    int rc = air_program_checked(ops, n_ops, n_consts, col_log2_len_or_null, n_cols, log2_trace, (uint32_t)lg, n_transitions, &info);
    if (rc) return rc;
    for (uint32_t k = 0; k < n_boundary; k++) {
        const lw_m31q_boundary_t &b = boundary[k];
        if ((rc = r2_boundary_col_check(k, b.col, n_cols, col_log2_len_or_null, lg))) return rc;
        if (b.step >= n) { set_error("boundary constraint %u: step %llu of a trace of %llu rows", k, (unsigned long long)b.step, (unsigned long long)n); return LW_ERR_BAD_ARG; }
    }
    for (uint32_t k = 0; k < n_transitions; k++) {
        const lw_m31q_transition_t &t = transitions[k];
        if (t.period == 0 || (t.period & (t.period - 1)) || t.period > n / 2) {
            set_error("transition %u: period %llu is not a power of two from 1 to n / 2", k, (unsigned long long)t.period);
            return LW_ERR_BAD_ARG;
        }
        if (t.offset >= t.period) { set_error("transition %u: offset %llu of period %llu", k, (unsigned long long)t.offset, (unsigned long long)t.period); return LW_ERR_BAD_ARG; }
        if (t.end_exemptions > n / t.period) {
            set_error("transition %u: %llu end exemptions of period %llu exceed the trace", k, (unsigned long long)t.end_exemptions, (unsigned long long)t.period);
            return LW_ERR_BAD_ARG;
        }
    }
    std::vector<uint32_t> class_of;
    std::vector<CircleR2Desc> classes;
    r2_classes(transitions, n_transitions, class_of, classes);
    if ((rc = r2_class_cap_check(classes.size(), M31Q_R2_CLASSES)) || (rc = r2_buffers_check<M31qExt>(d_out, out_stride, N, d_columns, col_log2_len_or_null, n_cols))) return rc;
    if (log2_blowup == 0 && (n_boundary || n_transitions)) {
        set_error("a blow-up of 1: the LDE coset is the trace domain, where the zerofiers vanish");
        return LW_ERR_INV_ZERO;
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return m31q_r2_constraints_locked(en.c, ops, n_ops, consts, n_consts, d_columns, col_log2_len_or_null, n_cols, log2_trace, log2_blowup, boundary, n_boundary,
                                      transitions, n_transitions, info.n_tmps, d_out, out_stride, en.stream);
}

// ---------------------------------------------------------------- host: the parts
// interpolate the four planes -> the blocks of L coefficients -> the forward transform of every block onto the LDE coset
static int m31q_r2_composition_parts(const uint32_t *d_evals, size_t evals_stride, uint32_t log2_lde, uint32_t log2_part, uint32_t n_parts, uint32_t *d_parts_coeffs,
                                     uint32_t *d_parts_lde_or_null, uint64_t *out_tail_nonzero_or_null, void *hip_stream) {
    int rc = m31q_size_check(log2_lde);
    if (rc) return rc;
    uint32_t log2_P = 0;
    while (log2_P < 31 && (1u << log2_P) < n_parts) log2_P++;
    if (n_parts == 0 || (n_parts & (n_parts - 1)) || log2_part < 1 || (uint64_t)log2_part + log2_P > log2_lde) {
        set_error("%u parts of 2^%u coefficients of a polynomial of 2^%u: a power of two of parts of at least 2 coefficients, in all at most N", n_parts, log2_part,
                  log2_lde);
        return LW_ERR_BAD_ARG;
    }
    const uint64_t N = 1ull << log2_lde, L = 1ull << log2_part, used = (uint64_t)n_parts << log2_part;
    rc = d_parts_lde_or_null ? ext_device_ptrs({d_evals, d_parts_coeffs, d_parts_lde_or_null}) : ext_device_ptrs({d_evals, d_parts_coeffs});
    if (!rc) rc = ext_stride(evals_stride, N, "evaluations");
    if (rc) return rc;
    const size_t planes = (size_t)n_parts * 4, coeff_words = planes << log2_part, lde_words = planes << log2_lde;
    if (ext_overlap<M31qExt>(d_parts_coeffs, coeff_words, d_evals, ext_span<M31qExt>(evals_stride, N)) ||
        (d_parts_lde_or_null && (ext_overlap<M31qExt>(d_parts_lde_or_null, lde_words, d_evals, ext_span<M31qExt>(evals_stride, N)) ||
                                 ext_overlap<M31qExt>(d_parts_lde_or_null, lde_words, d_parts_coeffs, coeff_words)))) {
        set_error("the buffers of the parts overlap");
        return LW_ERR_BAD_ARG;
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.stream;
    const size_t b_H = r2_round256((size_t)4 * N * sizeof(uint32_t));
    if (c.pipe_tmp.ensure(b_H + 8)) return LW_ERR_ALLOC;
    uint32_t *d_H = (uint32_t *)c.pipe_tmp.p;
    unsigned long long *d_count = (unsigned long long *)((char *)c.pipe_tmp.p + b_H);
    rc = circle_interpolate_locked(c, d_evals, evals_stride, d_H, N, log2_lde, 4, s);
    if (rc) return rc;
    // part j, plane e <- plane e of H at [j L, (j + 1) L): P rows of L words, 4 L words apart
    for (int e = 0; e < 4; e++)
        LW_HIP_CHECK(hipMemcpy2DAsync(d_parts_coeffs + e * L, 4 * L * sizeof(uint32_t), d_H + e * N, L * sizeof(uint32_t), L * sizeof(uint32_t), n_parts,
                                      hipMemcpyDeviceToDevice, s),
                     LW_ERR_LAUNCH);
    if (d_parts_lde_or_null) {
        rc = circle_extend_locked(c, d_parts_coeffs, log2_part, L, d_parts_lde_or_null, log2_lde, N, (uint32_t)planes, s);
        if (rc) return rc;
    }
    if (!out_tail_nonzero_or_null) return LW_OK;
    unsigned long long count = 0;
    if (used < N) {
        LW_HIP_CHECK(hipMemsetAsync(d_count, 0, 8, s), LW_ERR_LAUNCH);
        const uint64_t blocks = (4 * (N - used) + M31Q_THREADS - 1) / M31Q_THREADS;
        rc = launch_1d(c, "m31q_r2_tail_kernel", m31q_r2_tail_kernel, (uint32_t)(blocks < 4096 ? blocks : 4096), s, (const uint32_t *)d_H, (uint64_t)N, used, d_count);
        if (!rc) rc = download(&count, d_count, 8, s);
        if (rc) return rc;
    } else {
        LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);   // no tail: the count is 0, the parts are complete on return all the same
    }
    *out_tail_nonzero_or_null = count;
    return LW_OK;
}

}  // namespace lw
#endif
