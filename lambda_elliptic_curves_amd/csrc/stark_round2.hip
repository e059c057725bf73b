// STARK round 2 on the device (round_2_compute_composition_polynomial, provers/stark/src/prover.rs:428-484): the
// constraint evaluations of ConstraintEvaluator::evaluate (constraints/evaluator.rs:33-225) over caller-written transition
// evaluations, interpolation and break_in_parts (math/src/polynomial/mod.rs:289-302), the LDE of the parts and the
// paired-row commitment (prover.rs:398-425; the leaf kernel is merkle.hip's).  Under all of it: batch inversion
// (FieldElement::inplace_batch_inverse, math/src/field/element.rs:47-65) as a public call.
//
//   out[i] = sum_c coeff_c Zc[i] T_c(i)  +  sum_k coeff_k (col_k[i] - value_k) / (x_i - g^step_k),     x_i = h w^i
//   Zc[i]  = cycle_c[i mod len_c] E_c(x_i),   E_c(x) = prod_{k = 1 .. end_exemptions} (x - g^(n - k period))
//   cycle_c[e] = 1 / ((h w^e)^(n / period) - g^(offset n / period))                     len = blowup period
//              = ((h w^e)^(n / ep) - g^(n peo / ep)) / (the same denominator)           len = blowup ep (exemptions period ep)
// (zerofier_evaluations_on_extended_domain, constraints/transition.rs:108-205, with its truncating integer divisions).
//
// Kernels:
//   field_batch_inverse_kernel  Montgomery's trick per work-item over BINV_CHUNK elements BINV_THREADS apart (every step of
//                               a wave touches 64 consecutive elements), one fe_inv_fast per chunk.  Only the running
//                               products stay in registers; the elements are read again on the way back (the second read
//                               of a workgroup's 64 KiB comes from L2), which also makes in == out legal.
//   r2_xtable_kernel            two-level table of the LDE coset: lo[a] = w^a, hi[b] = h w^(b 2^hbits); x_i is one product
//   r2_cycle_kernel             numerators and denominators of every distinct cycle table, square-and-multiply per entry;
//                               the batch inversion then turns them into the tables
//   r2_constraint_kernel        R2_PTS LDE points per work-item: boundary constraints grouped by distinct step, the
//                               (step x own points) denominators of up to R2_STEPS steps inverted with one fe_inv_fast;
//                               transitions grouped by (end_exemptions, period) so that E_c is formed once per group.
//                               Reads each referenced column element and each T_c element once, writes out once.
//   r2_split_kernel             break_in_parts as a strided gather into zero-padded blocks
//   r2_part_lengths_kernel      stripped length of every part
// Every stored value is canonical: fe_add / fe_sub / fe_mul return canonical residues for canonical operands.
#include <string.h>
#include <algorithm>
#include <vector>
#include "internal.h"
#include "field.cuh"

namespace lw {

constexpr int BINV_THREADS = 256;
constexpr int BINV_CHUNK = 8;                                              // elements per work-item
constexpr uint64_t BINV_BLOCK = (uint64_t)BINV_THREADS * BINV_CHUNK;     // elements one workgroup owns

// out[i] = in[i]^-1 [* mul[i]].  A zero element raises *zero_flag and is replaced by one, so that the other elements of
// its chunk still come out right (the caller reports LW_ERR_INV_ZERO and the output is unspecified anyway).
template <class F, bool MUL>
__global__ __launch_bounds__(BINV_THREADS) void field_batch_inverse_kernel(const char *in, const char *mul, char *out, uint64_t n,
                                                                          uint32_t *zero_flag) {
    const uint64_t base = (uint64_t)blockIdx.x * BINV_BLOCK + threadIdx.x;
    auto elem = [&](int j, bool &zero) -> Fe<F> {
        const uint64_t i = base + (uint64_t)j * BINV_THREADS;
        if (i >= n) return Fe<F>::one();
        const Fe<F> v = fe_load<F>(in + i * 32);
        if (!v.is_zero()) return v;
        zero = true;
        return Fe<F>::one();
    };
    if (base >= n) return;
    bool zero = false;
    Fe<F> pre[BINV_CHUNK];   // pre[j] = a_0 ... a_j
    pre[0] = elem(0, zero);
#pragma unroll
    for (int j = 1; j < BINV_CHUNK; j++) pre[j] = fe_mul<F>(pre[j - 1], elem(j, zero));
    if (zero) atomicOr(zero_flag, 1u);
    Fe<F> inv = fe_inv_fast<F>(pre[BINV_CHUNK - 1]);
#pragma unroll
    for (int j = BINV_CHUNK - 1; j >= 0; j--) {
        const uint64_t i = base + (uint64_t)j * BINV_THREADS;
        if (i >= n) continue;   // a_j = 1: inv stays
        Fe<F> r = j ? fe_mul<F>(inv, pre[j ? j - 1 : 0]) : inv;
        if (j) inv = fe_mul<F>(inv, elem(j, zero));
        if (MUL) r = fe_mul<F>(r, fe_load<F>(mul + i * 32));
        fe_store<F>(out + i * 32, r);
    }
}

// ---- constraint evaluations ----
constexpr int R2_THREADS = 256;
constexpr int R2_PTS = 2;      // LDE points per work-item, R2_THREADS apart
constexpr int R2_STEPS = 2;    // distinct boundary steps per inversion

// device tables of one call; elements in the reference's memory form
struct alignas(16) R2Step {       // the boundary constraints bnd[first, first + count) divide by x - point
    uint64_t point[4];            // g^step
    uint32_t first, count;
    uint64_t pad;
};
struct alignas(16) R2Boundary {
    uint64_t value[4], coeff[4];
    const char *col;
    uint64_t pad;
};
struct alignas(16) R2Group {      // transitions trans[first, first + count) share E(x) = prod (x - roots[root0 + r])
    uint32_t first, count, root0, n_roots;
};
struct alignas(16) R2Trans {
    uint64_t coeff[4];
    const char *cycle;            // len entries
    const char *evals;            // T_c, N elements
    uint64_t len, pow2;           // pow2: len is a power of two
};
struct alignas(16) R2Cycle {      // entries [off, off + len) of the concatenated tables
    uint64_t dc[4], nc[4];        // g^(offset n / period), g^(n peo / ep)
    uint64_t de, ne;              // n / period, n / ep
    uint64_t off, len;
    uint64_t has_num, pad;
};

struct R2Domain {                 // x_i = lo[i & (2^hbits - 1)] * hi[i >> hbits]
    const char *lo, *hi;
    uint32_t hbits;
};
template <class F>
__device__ __forceinline__ Fe<F> r2_x(const R2Domain &d, uint64_t i) {
    return fe_mul<F>(fe_load<F>(d.lo + (i & ((1ull << d.hbits) - 1)) * 32), fe_load<F>(d.hi + (i >> d.hbits) * 32));
}

template <class F>
__global__ __launch_bounds__(256) void r2_xtable_kernel(char *lo, char *hi, uint64_t nlo, uint64_t nhi, const Fe<F> w, const Fe<F> wh,
                                                        const Fe<F> h) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nlo) fe_store<F>(lo + i * 32, fe_pow_u64<F>(w, i));
    else if (i - nlo < nhi) fe_store<F>(hi + (i - nlo) * 32, fe_mul<F>(h, fe_pow_u64<F>(wh, i - nlo)));
}

template <class F>
__global__ __launch_bounds__(256) void r2_cycle_kernel(const R2Cycle *cyc, uint32_t n_cyc, uint64_t total, const R2Domain dom, char *den,
                                                       char *num) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    uint32_t t = 0;
    while (t + 1 < n_cyc && idx >= cyc[t + 1].off) t++;
    const R2Cycle &cy = cyc[t];
    const Fe<F> x = r2_x<F>(dom, idx - cy.off);
    fe_store<F>(den + idx * 32, fe_sub<F>(fe_pow_u64<F>(x, cy.de), fe_load<F>(cy.dc)));
    if (num) fe_store<F>(num + idx * 32, cy.has_num ? fe_sub<F>(fe_pow_u64<F>(x, cy.ne), fe_load<F>(cy.nc)) : Fe<F>::one());
}

struct R2Args {
    const R2Step *steps;
    const R2Boundary *bnd;
    const R2Group *groups;
    const R2Trans *trans;
    const char *roots;
    uint32_t n_steps, n_groups;
    uint64_t N;
    R2Domain dom;
    char *out;
};

template <class F>
__global__ __launch_bounds__(R2_THREADS) void r2_constraint_kernel(const R2Args a) {
    constexpr int Q = R2_STEPS * R2_PTS;
    const uint64_t i0 = (uint64_t)blockIdx.x * (R2_THREADS * R2_PTS) + threadIdx.x;
    if (i0 >= a.N) return;
    uint64_t idx[R2_PTS];
    bool live[R2_PTS];
    Fe<F> x[R2_PTS], acc[R2_PTS];
#pragma unroll
    for (int j = 0; j < R2_PTS; j++) {
        idx[j] = i0 + (uint64_t)j * R2_THREADS;
        live[j] = idx[j] < a.N;
        x[j] = live[j] ? r2_x<F>(a.dom, idx[j]) : Fe<F>::one();
        acc[j] = Fe<F>::zero();
    }
    // boundary part: sum_s (x - g^step_s)^-1 sum_{k in s} coeff_k (col_k - value_k), R2_STEPS steps per inversion.
    // Slot q = s * R2_PTS + j; a slot past the last step or of a point past N holds the denominator one.
#pragma unroll 1
    for (uint32_t s0 = 0; s0 < a.n_steps; s0 += R2_STEPS) {
        Fe<F> pre[Q];   // running products of the denominators
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int s = q / R2_PTS, j = q % R2_PTS;
            if (s0 + s < a.n_steps && live[j]) {
                const Fe<F> d = fe_sub<F>(x[j], fe_load<F>(a.steps[s0 + s].point));
                pre[q] = q ? fe_mul<F>(pre[q ? q - 1 : 0], d) : d;
            } else {
                pre[q] = q ? pre[q ? q - 1 : 0] : Fe<F>::one();
            }
        }
        Fe<F> inv = fe_inv_fast<F>(pre[Q - 1]);
#pragma unroll
        for (int q = Q - 1; q >= 0; q--) {
            const int s = q / R2_PTS, j = q % R2_PTS;
            if (!(s0 + s < a.n_steps && live[j])) continue;
            const R2Step &st = a.steps[s0 + s];
            const Fe<F> dinv = q ? fe_mul<F>(inv, pre[q ? q - 1 : 0]) : inv;
            if (q) inv = fe_mul<F>(inv, fe_sub<F>(x[j], fe_load<F>(st.point)));
            Fe<F> num = Fe<F>::zero();
#pragma unroll 1
            for (uint32_t k = st.first; k < st.first + st.count; k++) {
                const R2Boundary &b = a.bnd[k];
                num = fe_add<F>(num, fe_mul<F>(fe_load<F>(b.coeff), fe_sub<F>(fe_load<F>(b.col + idx[j] * 32), fe_load<F>(b.value))));
            }
            acc[j] = fe_add<F>(acc[j], fe_mul<F>(dinv, num));
        }
    }
    // transition part: sum_groups E(x) sum_{c in group} coeff_c cycle_c[i mod len_c] T_c(i)
#pragma unroll 1
    for (uint32_t g = 0; g < a.n_groups; g++) {
        const R2Group gr = a.groups[g];
#pragma unroll
        for (int j = 0; j < R2_PTS; j++) {
            if (!live[j]) continue;
            Fe<F> sum = Fe<F>::zero();
#pragma unroll 1
            for (uint32_t c = gr.first; c < gr.first + gr.count; c++) {
                const R2Trans &t = a.trans[c];
                const uint64_t e = t.pow2 ? (idx[j] & (t.len - 1)) : idx[j] % t.len;
                const Fe<F> zt = fe_mul<F>(fe_load<F>(t.cycle + e * 32), fe_load<F>(t.evals + idx[j] * 32));
                sum = fe_add<F>(sum, fe_mul<F>(fe_load<F>(t.coeff), zt));
            }
            if (gr.n_roots) {
                Fe<F> E = fe_sub<F>(x[j], fe_load<F>(a.roots + (uint64_t)gr.root0 * 32));
#pragma unroll 1
                for (uint32_t r = 1; r < gr.n_roots; r++) E = fe_mul<F>(E, fe_sub<F>(x[j], fe_load<F>(a.roots + (uint64_t)(gr.root0 + r) * 32)));
                sum = fe_mul<F>(sum, E);
            }
            acc[j] = fe_add<F>(acc[j], sum);
        }
    }
#pragma unroll
    for (int j = 0; j < R2_PTS; j++)
        if (live[j]) fe_store<F>(a.out + idx[j] * 32, acc[j]);
}

// ---- parts ----
// part j, slot m <- H[j + m P] (zero past N): parts is P blocks of L elements
__global__ __launch_bounds__(256) void r2_split_kernel(const uint4 *H, uint64_t N, uint64_t P, uint32_t log2_L, uint4 *parts) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (P << log2_L)) return;
    const uint64_t j = idx >> log2_L, m = idx & ((1ull << log2_L) - 1), src = j + m * P;
    uint4 a = make_uint4(0, 0, 0, 0), b = a;
    if (src < N) {
        a = H[2 * src];
        b = H[2 * src + 1];
    }
    parts[2 * idx] = a;
    parts[2 * idx + 1] = b;
}
// lens[j] = stripped length of part j (lens zeroed before the launch)
__global__ __launch_bounds__(256) void r2_part_lengths_kernel(const uint4 *parts, uint64_t P, uint32_t log2_L, unsigned long long *lens) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (P << log2_L)) return;
    const uint4 a = parts[2 * idx], b = parts[2 * idx + 1];
    if (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) atomicMax(lens + (idx >> log2_L), (unsigned long long)((idx & ((1ull << log2_L) - 1)) + 1));
}

// ---- host side ----
static size_t r2_round256(size_t b) { return (b + 255) & ~(size_t)255; }
static bool r2_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
template <class F>
static Fe<F> r2_load(const void *ref) {
    alignas(16) uint64_t w[4];
    memcpy(w, ref, 32);
    return fe_load<F>(w);
}
template <class F>
static void r2_store(uint64_t (&dst)[4], const Fe<F> &v) {
    alignas(16) uint64_t w[4];
    fe_store<F>(w, v);
    memcpy(dst, w, 32);
}
template <class F>
static Fe<F> r2_root(lw_field_t field, uint32_t order) {
    Fe<F> r;
    (void)ntt256_root_words((int)field, order, false, r.v);
    return r;
}
static bool r2_field_ok(lw_field_t f, const char *what) {
    if (f == LW_FIELD_STARK252 || f == LW_FIELD_BLS12_381_FR) return true;
    set_error("field %d: %s takes STARK252 or BLS12_381_FR (4 x u64 limbs)", (int)f, what);
    return false;
}
static uint32_t r2_blocks(uint64_t items, uint64_t per_block) { return (uint32_t)((items + per_block - 1) / per_block); }

// d_flag: one zeroed u32 in device memory; enqueue only
template <class F>
static void batch_inverse_launch(Context &c, const void *d_in, const void *d_mul, void *d_out, uint64_t n, uint32_t *d_flag, hipStream_t s) {
    hipEvent_t pe = c.prof_begin(s);
    if (d_mul)
        hipLaunchKernelGGL((field_batch_inverse_kernel<F, true>), dim3(r2_blocks(n, BINV_BLOCK)), dim3(BINV_THREADS), 0, s, (const char *)d_in,
                           (const char *)d_mul, (char *)d_out, n, d_flag);
    else
        hipLaunchKernelGGL((field_batch_inverse_kernel<F, false>), dim3(r2_blocks(n, BINV_BLOCK)), dim3(BINV_THREADS), 0, s, (const char *)d_in,
                           (const char *)nullptr, (char *)d_out, n, d_flag);
    c.prof_end("field_batch_inverse_kernel", pe, s);
}
// the flag of a batch inversion, once the stream gets there
static int read_zero_flag(const uint32_t *d_flag, const char *what, hipStream_t s) {
    uint32_t flag = 0;
    LW_HIP_CHECK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    if (!flag) return LW_OK;
    set_error("%s: inverse of zero", what);
    return LW_ERR_INV_ZERO;
}

template <class F>
static int batch_inverse_locked(Context &c, const void *d_in, uint64_t n, void *d_out, hipStream_t s) {
    if (c.poly_ws.ensure(256)) return LW_ERR_ALLOC;
    uint32_t *d_flag = (uint32_t *)c.poly_ws.p;
    LW_HIP_CHECK(hipMemsetAsync(d_flag, 0, 4, s), LW_ERR_LAUNCH);
    batch_inverse_launch<F>(c, d_in, nullptr, d_out, n, d_flag, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return read_zero_flag(d_flag, "batch inverse", s);
}

// The argument checks of the constraint evaluations that need no device (both forms); *log2_lde out
static int constraints_check(lw_field_t field, uint32_t n_cols, uint32_t log2_trace, uint32_t log2_blowup, const void *coset,
                             const lw_stark_boundary_t *boundary, uint32_t n_boundary, const lw_stark_transition_t *transitions,
                             uint32_t n_transitions) {
    if (!r2_field_ok(field, "the STARK constraint evaluation")) return LW_ERR_BAD_ARG;
    if (!coset || (n_boundary && !boundary) || (n_transitions && !transitions)) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    const uint64_t lg = (uint64_t)log2_trace + log2_blowup;
    if (lg > 34 || lg > field_two_adicity(field)) { set_error("an LDE domain of 2^%llu points is beyond the NTT", (unsigned long long)lg); return LW_ERR_BAD_ARG; }
    const uint64_t n = 1ull << log2_trace;
    for (uint32_t k = 0; k < n_boundary; k++)
        if (boundary[k].col >= n_cols) { set_error("boundary constraint %u: column %u of %u", k, boundary[k].col, n_cols); return LW_ERR_BAD_ARG; }
    for (uint32_t k = 0; k < n_transitions; k++) {
        const lw_stark_transition_t &t = transitions[k];
        if (t.period == 0) { set_error("transition %u: period 0", k); return LW_ERR_BAD_ARG; }
        // end_exemptions_poly takes g^(n - k period) with an unsigned subtraction (transition.rs:99-100)
        if (t.end_exemptions && (t.end_exemptions > n || t.period > n / t.end_exemptions)) {
            set_error("transition %u: %llu end exemptions of period %llu exceed the trace", k, (unsigned long long)t.end_exemptions,
                      (unsigned long long)t.period);
            return LW_ERR_BAD_ARG;
        }
    }
    return LW_OK;
}

// cols: n_cols device pointers (host array).  Synchronises once when there are transitions (the zero flag of the tables).
template <class F>
static int constraints_locked(Context &c, lw_field_t field, const void *const *cols, uint32_t log2_trace, uint32_t log2_blowup,
                              const void *coset, const lw_stark_boundary_t *boundary, uint32_t n_boundary,
                              const lw_stark_transition_t *transitions, uint32_t n_transitions, const void *d_tevals, uint64_t t_stride,
                              void *d_out, hipStream_t s) {
    typedef unsigned __int128 u128;
    const uint32_t log2_lde = log2_trace + log2_blowup;
    const uint64_t n = 1ull << log2_trace, N = 1ull << log2_lde, blowup = 1ull << log2_blowup;
    const Fe<F> h = r2_load<F>(coset), g = r2_root<F>(field, log2_trace), w = r2_root<F>(field, log2_lde);
    if (n_boundary) {   // x_i = g^step for some i exactly when h lies in the LDE group
        Fe<F> hn = h;
        for (uint32_t i = 0; i < log2_lde; i++) hn = fe_sqr<F>(hn);
        if (hn == Fe<F>::one()) { set_error("the coset offset lies in the LDE domain: a boundary zerofier vanishes on it"); return LW_ERR_INV_ZERO; }
    }
    // boundary constraints by distinct step (mod n: g has order n)
    std::vector<uint32_t> order(n_boundary);
    for (uint32_t k = 0; k < n_boundary; k++) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return boundary[x].step % n < boundary[y].step % n; });
    std::vector<R2Step> steps;
    std::vector<R2Boundary> bnd(n_boundary);
    for (uint32_t q = 0; q < n_boundary; q++) {
        const lw_stark_boundary_t &b = boundary[order[q]];
        if (q == 0 || b.step % n != boundary[order[q - 1]].step % n) {
            R2Step st;
            memset(&st, 0, sizeof(st));
            r2_store<F>(st.point, fe_pow_u64<F>(g, b.step % n));
            st.first = q;
            steps.push_back(st);
        }
        steps.back().count++;
        memset(&bnd[q], 0, sizeof(R2Boundary));
        memcpy(bnd[q].value, b.value, 32);
        memcpy(bnd[q].coeff, b.coeff, 32);
        bnd[q].col = (const char *)cols[b.col];
    }
    // distinct cycle tables; a table longer than N is read below N only
    std::vector<R2Cycle> cycles;
    std::vector<uint32_t> cycle_of(n_transitions);
    uint64_t total = 0;
    bool any_num = false;
    for (uint32_t k = 0; k < n_transitions; k++) {
        const lw_stark_transition_t &t = transitions[k];
        uint32_t found = (uint32_t)cycles.size();
        for (uint32_t j = 0; j < k && found == cycles.size(); j++) {
            const lw_stark_transition_t &u = transitions[j];
            if (u.period == t.period && u.offset == t.offset && u.exemptions_period == t.exemptions_period &&
                (t.exemptions_period == 0 || u.periodic_exemptions_offset == t.periodic_exemptions_offset))
                found = cycle_of[j];
        }
        cycle_of[k] = found;
        if (found < cycles.size()) continue;
        R2Cycle cy;
        memset(&cy, 0, sizeof(cy));
        const uint64_t ep = t.exemptions_period;
        cy.de = n / t.period;
        r2_store<F>(cy.dc, fe_pow_u64<F>(g, (uint64_t)((u128)t.offset * n / t.period % n)));
        if (ep) {
            cy.has_num = 1;
            any_num = true;
            cy.ne = n / ep;
            r2_store<F>(cy.nc, fe_pow_u64<F>(g, (uint64_t)((u128)n * t.periodic_exemptions_offset / ep % n)));
        }
        const u128 len = (u128)blowup * (ep ? ep : t.period);
        cy.len = len > N ? N : (uint64_t)len;
        cy.off = total;
        total += cy.len;
        cycles.push_back(cy);
    }
    // transitions by (end_exemptions, period)
    std::vector<uint32_t> torder(n_transitions);
    for (uint32_t k = 0; k < n_transitions; k++) torder[k] = k;
    auto same_group = [&](uint32_t x, uint32_t y) {
        const lw_stark_transition_t &a = transitions[x], &b = transitions[y];
        return a.end_exemptions == b.end_exemptions && (a.end_exemptions == 0 || a.period == b.period);
    };
    std::stable_sort(torder.begin(), torder.end(), [&](uint32_t x, uint32_t y) {
        const lw_stark_transition_t &a = transitions[x], &b = transitions[y];
        if (a.end_exemptions != b.end_exemptions) return a.end_exemptions < b.end_exemptions;
        return a.end_exemptions != 0 && a.period < b.period;
    });
    std::vector<R2Group> groups;
    std::vector<uint64_t> roots;   // 4 words per root
    // workspace: [tables | flag | x lo | x hi | cycle denominators -> tables | cycle numerators]
    const uint32_t hbits = (log2_lde + 1) / 2;
    const uint64_t nlo = 1ull << hbits, nhi = 1ull << (log2_lde - hbits);
    std::vector<R2Trans> trans(n_transitions);
    for (uint32_t q = 0; q < n_transitions; q++) {
        const lw_stark_transition_t &t = transitions[torder[q]];
        if (q == 0 || !same_group(torder[q], torder[q - 1])) {
            R2Group gr = {q, 0, (uint32_t)(roots.size() / 4), (uint32_t)t.end_exemptions};
            for (uint64_t k = 1; k <= t.end_exemptions; k++) {
                uint64_t r[4];
                r2_store<F>(r, fe_pow_u64<F>(g, (n - k * t.period) % n));
                roots.insert(roots.end(), r, r + 4);
            }
            groups.push_back(gr);
        }
        groups.back().count++;
        memset(&trans[q], 0, sizeof(R2Trans));
        memcpy(trans[q].coeff, t.coeff, 32);
        const R2Cycle &cy = cycles[cycle_of[torder[q]]];
        trans[q].cycle = (const char *)(uintptr_t)(cy.off * 32);   // relative until the workspace is known
        trans[q].evals = (const char *)d_tevals + (uint64_t)torder[q] * t_stride * 32;
        trans[q].len = cy.len;
        trans[q].pow2 = (cy.len & (cy.len - 1)) == 0;
    }
    const size_t b_steps = r2_round256(steps.size() * sizeof(R2Step)), b_bnd = r2_round256(bnd.size() * sizeof(R2Boundary)),
                 b_groups = r2_round256(groups.size() * sizeof(R2Group)), b_trans = r2_round256(trans.size() * sizeof(R2Trans)),
                 b_roots = r2_round256(roots.size() * 8), b_cyc = r2_round256(cycles.size() * sizeof(R2Cycle));
    const size_t tables = b_steps + b_bnd + b_groups + b_trans + b_roots + b_cyc;
    const size_t b_x = r2_round256((size_t)(nlo + nhi) * 32), b_den = r2_round256((size_t)total * 32), b_num = any_num ? b_den : 0;
    if (c.poly_ws.ensure(tables + 256 + b_x + b_den + b_num)) return LW_ERR_ALLOC;
    char *d_tab = (char *)c.poly_ws.p, *d_flag = d_tab + tables, *d_x = d_flag + 256, *d_den = d_x + b_x, *d_num = any_num ? d_den + b_den : nullptr;
    for (auto &t : trans) t.cycle = d_den + (uintptr_t)t.cycle;
    LW_HIP_CHECK(hipMemsetAsync(d_flag, 0, 4, s), LW_ERR_LAUNCH);
    char *d_steps = d_tab, *d_bnd = d_steps + b_steps, *d_groups = d_bnd + b_bnd, *d_trans = d_groups + b_groups, *d_roots = d_trans + b_trans,
         *d_cyc = d_roots + b_roots;
    if (tables) {   // one upload through the lane's pinned staging
        int rc = deep_pin(c, tables);
        if (rc) return rc;
        char *hp = (char *)c.deep_pin;
        memset(hp, 0, tables);
        if (!steps.empty()) memcpy(hp + (d_steps - d_tab), steps.data(), steps.size() * sizeof(R2Step));
        if (!bnd.empty()) memcpy(hp + (d_bnd - d_tab), bnd.data(), bnd.size() * sizeof(R2Boundary));
        if (!groups.empty()) memcpy(hp + (d_groups - d_tab), groups.data(), groups.size() * sizeof(R2Group));
        if (!trans.empty()) memcpy(hp + (d_trans - d_tab), trans.data(), trans.size() * sizeof(R2Trans));
        if (!roots.empty()) memcpy(hp + (d_roots - d_tab), roots.data(), roots.size() * 8);
        if (!cycles.empty()) memcpy(hp + (d_cyc - d_tab), cycles.data(), cycles.size() * sizeof(R2Cycle));
        LW_HIP_CHECK(hipMemcpyAsync(d_tab, hp, tables, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
        LW_HIP_CHECK(hipEventRecord(c.deep_pin_read, s), LW_ERR_LAUNCH);
    }
    R2Domain dom;
    dom.lo = d_x;
    dom.hi = d_x + nlo * 32;
    dom.hbits = hbits;
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL((r2_xtable_kernel<F>), dim3(r2_blocks(nlo + nhi, 256)), dim3(256), 0, s, d_x, d_x + nlo * 32, nlo, nhi, w,
                       fe_pow_u64<F>(w, nlo), h);
    c.prof_end("r2_xtable_kernel", pe, s);
    if (total) {
        pe = c.prof_begin(s);
        hipLaunchKernelGGL((r2_cycle_kernel<F>), dim3(r2_blocks(total, 256)), dim3(256), 0, s, (const R2Cycle *)d_cyc, (uint32_t)cycles.size(), total,
                           dom, d_den, d_num);
        c.prof_end("r2_cycle_kernel", pe, s);
        batch_inverse_launch<F>(c, d_den, d_num, d_den, total, (uint32_t *)d_flag, s);
    }
    R2Args a;
    memset(&a, 0, sizeof(a));
    a.steps = (const R2Step *)d_steps;
    a.bnd = (const R2Boundary *)d_bnd;
    a.groups = (const R2Group *)d_groups;
    a.trans = (const R2Trans *)d_trans;
    a.roots = d_roots;
    a.n_steps = (uint32_t)steps.size();
    a.n_groups = (uint32_t)groups.size();
    a.N = N;
    a.dom = dom;
    a.out = (char *)d_out;
    pe = c.prof_begin(s);
    hipLaunchKernelGGL((r2_constraint_kernel<F>), dim3(r2_blocks(N, R2_THREADS * R2_PTS)), dim3(R2_THREADS), 0, s, a);
    c.prof_end("r2_constraint_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return total ? read_zero_flag((const uint32_t *)d_flag, "transition zerofier", s) : (int)LW_OK;
}

static uint32_t r2_ceil_log2(uint64_t v) {
    uint32_t x = 0;
    while ((1ull << x) < v) x++;
    return x;
}
// log2 of the block a part is padded to: next_power_of_two(ceil(N / P))
static uint32_t parts_log2_block(uint32_t log2_lde, uint32_t n_parts) {
    const uint64_t N = 1ull << log2_lde;
    return r2_ceil_log2((N + n_parts - 1) / n_parts);
}
static int parts_check(lw_field_t field, uint32_t log2_lde, uint32_t n_parts) {
    if (!r2_field_ok(field, "the composition polynomial")) return LW_ERR_BAD_ARG;
    if (log2_lde > 34 || log2_lde > field_two_adicity(field)) { set_error("an LDE domain of 2^%u points is beyond the NTT", log2_lde); return LW_ERR_BAD_ARG; }
    if (n_parts == 0 || n_parts > (1ull << log2_lde)) { set_error("%u parts of a polynomial of 2^%u coefficients", n_parts, log2_lde); return LW_ERR_BAD_ARG; }
    return LW_OK;
}

// interpolate_offset_fft -> break_in_parts -> evaluate_polynomial_on_lde_domain of every part.  lens_host: synchronises.
static int parts_locked(Context &c, lw_field_t field, const void *d_evals, uint32_t log2_lde, const void *coset, uint32_t P,
                        void *d_parts_coeffs, void *d_parts_lde, size_t *lens_host, hipStream_t s) {
    const uint64_t N = 1ull << log2_lde;
    const uint32_t log2_L = parts_log2_block(log2_lde, P);
    const size_t b_H = r2_round256((size_t)N * 32);
    if (c.pipe_tmp.ensure(b_H + (size_t)P * 8)) return LW_ERR_ALLOC;
    char *d_H = (char *)c.pipe_tmp.p;
    unsigned long long *d_lens = (unsigned long long *)(d_H + b_H);
    int rc = ntt_device_locked(c, field, LW_LAYOUT_U64_LIMBS_MS_FIRST, LW_DIR_INVERSE, d_evals, d_H, log2_lde, 1, 0, coset, s);
    if (rc) return rc;
    const uint64_t items = (uint64_t)P << log2_L;
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL(r2_split_kernel, dim3(r2_blocks(items, 256)), dim3(256), 0, s, (const uint4 *)d_H, N, (uint64_t)P, log2_L, (uint4 *)d_parts_coeffs);
    c.prof_end("r2_split_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    if (d_parts_lde) {
        rc = ntt_device_locked(c, field, LW_LAYOUT_U64_LIMBS_MS_FIRST, LW_DIR_FORWARD, d_parts_coeffs, d_parts_lde, log2_lde, P, 0, coset, s, log2_L);
        if (rc) return rc;
    }
    if (!lens_host) return LW_OK;
    LW_HIP_CHECK(hipMemsetAsync(d_lens, 0, (size_t)P * 8, s), LW_ERR_LAUNCH);
    pe = c.prof_begin(s);
    hipLaunchKernelGGL(r2_part_lengths_kernel, dim3(r2_blocks(items, 256)), dim3(256), 0, s, (const uint4 *)d_parts_coeffs, (uint64_t)P, log2_L, d_lens);
    c.prof_end("r2_part_lengths_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    std::vector<unsigned long long> lens(P);
    LW_HIP_CHECK(hipMemcpyAsync(lens.data(), d_lens, (size_t)P * 8, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    for (uint32_t j = 0; j < P; j++) lens_host[j] = (size_t)lens[j];
    return LW_OK;
}

static int commit_check(lw_field_t field, uint32_t n_parts, uint32_t log2_lde) {
    if (!r2_field_ok(field, "the composition commitment")) return LW_ERR_BAD_ARG;
    if (n_parts == 0 || n_parts >= (1u << 24)) { set_error("%u parts per row", n_parts); return LW_ERR_BAD_ARG; }
    if (log2_lde == 0 || log2_lde > 32) { set_error("rows are committed in pairs: 2^%u rows", log2_lde); return LW_ERR_BAD_ARG; }
    return LW_OK;
}
static int root_download(const void *d_nodes, uint8_t *out_root, hipStream_t s) {
    LW_HIP_CHECK(hipMemcpyAsync(out_root, d_nodes, 32, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    return LW_OK;
}

}  // namespace lw

using namespace lw;

extern "C" {

uint64_t lw_field_batch_inverse_block(void) { return BINV_BLOCK; }

static int batch_inverse_check(lw_field_t field, const void *in, size_t n, const void *out, bool device) {
    if (!r2_field_ok(field, "batch inversion")) return LW_ERR_BAD_ARG;
    if (n && (!in || !out)) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    if (n > ((size_t)1 << 36)) { set_error("%zu elements", n); return LW_ERR_ALLOC; }
    if (device && n && (!r2_aligned16(in) || !r2_aligned16(out))) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    return LW_OK;
}
int lw_field_batch_inverse_device(lw_field_t field, const void *d_in, size_t n, void *d_out, void *hip_stream) {
    int rc = batch_inverse_check(field, d_in, n, d_out, true);
    if (rc || n == 0) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return field == LW_FIELD_STARK252 ? batch_inverse_locked<Stark252>(en.c, d_in, n, d_out, en.stream)
                                      : batch_inverse_locked<Fr381>(en.c, d_in, n, d_out, en.stream);
}
int lw_field_batch_inverse(lw_field_t field, const void *in, size_t n, void *out) {
    int rc = batch_inverse_check(field, in, n, out, false);
    if (rc || n == 0) return rc;
    Entry en(nullptr);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    if (c.host_io_a.ensure(n * 32)) return LW_ERR_ALLOC;
    LW_HIP_CHECK(hipMemcpyAsync(c.host_io_a.p, in, n * 32, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    rc = field == LW_FIELD_STARK252 ? batch_inverse_locked<Stark252>(c, c.host_io_a.p, n, c.host_io_a.p, s)
                                    : batch_inverse_locked<Fr381>(c, c.host_io_a.p, n, c.host_io_a.p, s);
    if (rc) return rc;
    LW_HIP_CHECK(hipMemcpyAsync(out, c.host_io_a.p, n * 32, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    return LW_OK;
}

int lw_stark_constraint_evaluations_device(lw_field_t field, const void *const *d_columns, uint32_t n_cols, uint32_t log2_trace,
                                           uint32_t log2_blowup, const void *coset_offset, const lw_stark_boundary_t *boundary,
                                           uint32_t n_boundary, const lw_stark_transition_t *transitions, uint32_t n_transitions,
                                           const void *d_transition_evals, uint64_t transition_stride_elems, void *d_out, void *hip_stream) {
    int rc = constraints_check(field, n_cols, log2_trace, log2_blowup, coset_offset, boundary, n_boundary, transitions, n_transitions);
    if (rc) return rc;
    const uint64_t N = 1ull << (log2_trace + log2_blowup);
    if (!d_out || (n_cols && !d_columns) || (n_transitions && !d_transition_evals)) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    if (!r2_aligned16(d_out) || !r2_aligned16(d_transition_evals)) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    for (uint32_t k = 0; k < n_cols; k++)
        if (!d_columns[k] || !r2_aligned16(d_columns[k])) { set_error("column %u: null or misaligned buffer", k); return LW_ERR_BAD_ARG; }
    if (transition_stride_elems == 0) transition_stride_elems = N;
    if (n_transitions > 1 && transition_stride_elems < N) { set_error("transition stride %llu < 2^%u rows", (unsigned long long)transition_stride_elems, log2_trace + log2_blowup); return LW_ERR_BAD_ARG; }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return field == LW_FIELD_STARK252
               ? constraints_locked<Stark252>(en.c, field, d_columns, log2_trace, log2_blowup, coset_offset, boundary, n_boundary, transitions,
                                              n_transitions, d_transition_evals, transition_stride_elems, d_out, en.stream)
               : constraints_locked<Fr381>(en.c, field, d_columns, log2_trace, log2_blowup, coset_offset, boundary, n_boundary, transitions,
                                           n_transitions, d_transition_evals, transition_stride_elems, d_out, en.stream);
}

int lw_stark_composition_parts_device(lw_field_t field, const void *d_evals, uint32_t log2_lde, const void *coset_offset, uint32_t n_parts,
                                      void *d_parts_coeffs, void *d_parts_lde, size_t *out_part_lens_or_null, void *hip_stream) {
    int rc = parts_check(field, log2_lde, n_parts);
    if (rc) return rc;
    if (!d_evals || !coset_offset || !d_parts_coeffs) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    if (!r2_aligned16(d_evals) || !r2_aligned16(d_parts_coeffs) || !r2_aligned16(d_parts_lde)) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    if (d_parts_lde == d_parts_coeffs) { set_error("the parts' LDE aliases their coefficients"); return LW_ERR_BAD_ARG; }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return parts_locked(en.c, field, d_evals, log2_lde, coset_offset, n_parts, d_parts_coeffs, d_parts_lde, out_part_lens_or_null, en.stream);
}

int lw_stark_commit_composition_device(lw_field_t field, const void *d_parts_lde, uint32_t n_parts, uint64_t col_stride_elems, uint32_t log2_lde,
                                       void *d_nodes, uint8_t *out_root_or_null, void *hip_stream) {
    int rc = commit_check(field, n_parts, log2_lde);
    if (rc) return rc;
    if (!d_parts_lde || !d_nodes) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    if (!r2_aligned16(d_parts_lde) || !r2_aligned16(d_nodes)) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    if (col_stride_elems == 0) col_stride_elems = 1ull << log2_lde;
    if (n_parts > 1 && col_stride_elems < (1ull << log2_lde)) { set_error("part stride %llu < 2^%u rows", (unsigned long long)col_stride_elems, log2_lde); return LW_ERR_BAD_ARG; }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    rc = merkle_commit_device(en.c, d_parts_lde, 2 * n_parts, col_stride_elems, log2_lde - 1, 1, d_nodes, en.stream, 32, 2);
    if (rc) return rc;
    return out_root_or_null ? root_download(d_nodes, out_root_or_null, en.stream) : (int)LW_OK;
}

// Round 2 on host arrays: parts 2 to 4 over the lane's staging buffers
int lw_stark_round2(lw_field_t field, const void *columns, uint32_t n_cols, uint32_t log2_trace, uint32_t log2_blowup, const void *coset_offset,
                    const lw_stark_boundary_t *boundary, uint32_t n_boundary, const lw_stark_transition_t *transitions,
                    uint32_t n_transitions, const void *transition_evals, uint32_t n_parts, void *out_parts_coeffs, size_t *out_part_lens,
                    uint8_t *out_root, uint8_t *out_nodes_or_null, void *out_parts_lde_or_null) {
    int rc = constraints_check(field, n_cols, log2_trace, log2_blowup, coset_offset, boundary, n_boundary, transitions, n_transitions);
    if (rc) return rc;
    const uint32_t log2_lde = log2_trace + log2_blowup;
    if ((rc = parts_check(field, log2_lde, n_parts)) || (rc = commit_check(field, n_parts, log2_lde))) return rc;
    if ((n_cols && !columns) || (n_transitions && !transition_evals) || !out_parts_coeffs || !out_part_lens || !out_root) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    const size_t N = (size_t)1 << log2_lde, L = (size_t)1 << parts_log2_block(log2_lde, n_parts);
    Entry en(nullptr);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    // a: [columns | transition evaluations]   b: [H evaluations | parts | parts' LDE | nodes]
    const size_t a_cols = (size_t)n_cols * N * 32, a_t = (size_t)n_transitions * N * 32;
    const size_t b_ev = N * 32, b_parts = (size_t)n_parts * L * 32, b_lde = (size_t)n_parts * N * 32, b_nodes = (N - 1) * 32;
    if (c.host_io_a.ensure(a_cols + a_t + 256) || c.host_io_b.ensure(b_ev + b_parts + b_lde + b_nodes)) return LW_ERR_ALLOC;
    char *da = (char *)c.host_io_a.p, *db = (char *)c.host_io_b.p;
    char *d_ev = db, *d_parts = d_ev + b_ev, *d_lde = d_parts + b_parts, *d_nodes = d_lde + b_lde;
    if (a_cols) LW_HIP_CHECK(hipMemcpyAsync(da, columns, a_cols, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    if (a_t) LW_HIP_CHECK(hipMemcpyAsync(da + a_cols, transition_evals, a_t, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    std::vector<const void *> cols(n_cols);
    for (uint32_t k = 0; k < n_cols; k++) cols[k] = da + (size_t)k * N * 32;
    rc = field == LW_FIELD_STARK252
             ? constraints_locked<Stark252>(c, field, cols.data(), log2_trace, log2_blowup, coset_offset, boundary, n_boundary, transitions,
                                            n_transitions, da + a_cols, N, d_ev, s)
             : constraints_locked<Fr381>(c, field, cols.data(), log2_trace, log2_blowup, coset_offset, boundary, n_boundary, transitions,
                                         n_transitions, da + a_cols, N, d_ev, s);
    if (rc) return rc;
    rc = parts_locked(c, field, d_ev, log2_lde, coset_offset, n_parts, d_parts, d_lde, out_part_lens, s);
    if (rc) return rc;
    rc = merkle_commit_device(c, d_lde, 2 * n_parts, N, log2_lde - 1, 1, d_nodes, s, 32, 2);
    if (rc) return rc;
    LW_HIP_CHECK(hipMemcpyAsync(out_parts_coeffs, d_parts, b_parts, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    if (out_parts_lde_or_null) LW_HIP_CHECK(hipMemcpyAsync(out_parts_lde_or_null, d_lde, b_lde, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    if (out_nodes_or_null) LW_HIP_CHECK(hipMemcpyAsync(out_nodes_or_null, d_nodes, b_nodes, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    return root_download(d_nodes, out_root, s);
}

}  // extern "C"
