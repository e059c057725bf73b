// Dense multilinear polynomials on the device (DenseMultilinearPolynomial::evaluate / fix_variables,
// math/src/polynomial/dense_multilinear_poly.rs) and the prover's round of a sumcheck over a product of K of them.
//
// A table T of 2^n elements is a multilinear polynomial in x_0 .. x_{n-1} with x_0 on the MOST significant bit of the index
// (the order of the reference's chis table).  eq(r, 1) = r, eq(r, 0) = 1 - r.
//
//   evaluate        sum_i T[i] prod_j eq(r_j, bit_{n-1-j}(i)).  One kernel, ml_eval_pass_kernel, folds the LAST (least
//                   significant) up to ML_LO = 11 variables of a table: a block takes one run of 2^11 = 2048 consecutive
//                   elements, thread r the elements r + 256 e (e < 8, coalesced).  The eq table of the 11 variables is
//                   never stored: it factors into eq8[e] (index bits 8..10, wave-uniform) and eq16hi[r >> 4] * eq16lo[r & 15]
//                   (bits 4..7 and 0..3), 40 elements that travel as the kernel's argument.  The block's sum is one element of
//                   a table in the remaining n - 11 variables, so the same kernel runs again on the partials: two launches
//                   up to 2^22, three up to 2^30, the last one a single block per table.  The table index is blockIdx.y.
//   fix_variables   T'[j] = sum_{b < 2^t} eq(r, b) T[b 2^(n-t) + j], t <= ML_FIX_T = 3 variables per pass (ml_fix_kernel<t>):
//                   thread j reads 2^t elements 2^(n-t) apart (every load and the store coalesced) against 2^t wave-uniform
//                   weights in the kernel's argument.  More variables are more passes through two workspace buffers.
//   sumcheck round  g(t) = sum_{j<h} prod_k (T_k[j] + t (T_k[j+h] - T_k[j])), t = 0 .. K, h = 2^(n-1)
//                   (ml_round_kernel<K, FUSED>).  FUSED first binds the leading variable to the previous challenge in place:
//                   with h = 2^(n-1) and q = h / 2 a thread owns the indices j, j + q, j + h, j + h + q of every table,
//                   stores the bound values at j and j + q and feeds them to the products, so that a round reads every
//                   table once and no thread reads what another one writes (ml_load_pair).  The values at t >= 2 come from
//                   adding b - a; only the products multiply.  Blocks reduce in LDS, ml_sum_finish_kernel adds up their
//                   partials.
// Every stored value is a canonical residue (fe_add / fe_sub / fe_mul / fe_dot of canonical operands), and field addition
// is exact, so the order of the reductions does not show in the result.  Small operands (eq tables, weights, challenges,
// table pointers) travel as kernel arguments: a call without a host result leaves nothing in flight that reads caller
// memory; a call with one synchronises once (ml_result).
// What the composed round of sumcheck_terms.hip uses as well is in multilinear.cuh: the pair loader, the epilogue and the
// finish kernel of a round, its driver (ml_round_plan, ml_round_finish) and the helpers of the entry points (MlTables).
#include "multilinear.cuh"

namespace lw {

constexpr int ML_LO = 11;                          // variables one evaluation pass folds
constexpr uint64_t ML_TILE = (uint64_t)1 << ML_LO;   // elements per block: 256 threads x 8
constexpr int ML_TABS = 8;                         // tables per evaluation launch (blockIdx.y)
constexpr int ML_FIX_T = 3;                        // variables one fix_variables pass folds

// w0 x0 + w1 x1 with one reduction (fe_dot admits two products of canonical operands in both fields)
template <class F>
__device__ __forceinline__ Fe<F> ml_dot2(const Fe<F> &w0, const Fe<F> &x0, const Fe<F> &w1, const Fe<F> &x1) {
    const Fe<F> *const pa[2] = {&w0, &w1}, *const pb[2] = {&x0, &x1};
    return fe_dot<F, 2>(pa, pb);
}

// ---- evaluate ----
template <class F>
struct MlEvalArgs {
    const char *tab[ML_TABS];   // tables of this launch
    char *dst;                  // [table][block] block sums
    uint64_t len;               // elements per table: a power of two
    uint64_t nblocks;
    Fe<F> eq8[8];               // index bits 8..10 of the run
    Fe<F> eq16hi[16];           // bits 4..7
    Fe<F> eq16lo[16];           // bits 0..3
};

template <class F>
__global__ __launch_bounds__(ML_THREADS) void ml_eval_pass_kernel(const MlEvalArgs<F> a) {
    __shared__ Fe<F> lds[ML_THREADS];
    const int r = threadIdx.x;
    const char *t = a.tab[blockIdx.y];
    const uint64_t base = (uint64_t)blockIdx.x * ML_TILE + (uint64_t)r;
    // A table shorter than the run (one block, len < 2048) wraps around: every index stays inside it, and the weight of an
    // index past the end is zero in one of the three tables.  So the eight loads are unconditional and issue together.
    Fe<F> v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = fe_load<F>(t + ((base + (uint64_t)e * ML_THREADS) & (a.len - 1)) * 32);
    Fe<F> acc = ml_dot2<F>(a.eq8[0], v[0], a.eq8[1], v[1]);
#pragma unroll
    for (int e = 2; e < 8; e += 2) acc = fe_add<F>(acc, ml_dot2<F>(a.eq8[e], v[e], a.eq8[e + 1], v[e + 1]));
    acc = fe_mul<F>(fe_mul<F>(a.eq16hi[r >> 4], a.eq16lo[r & 15]), acc);
    acc = ml_block_sum<F>(acc, lds);
    if (r == 0) fe_store<F>(a.dst + ((uint64_t)blockIdx.y * a.nblocks + blockIdx.x) * 32, acc);
}

// ---- fix_variables ----
template <class F>
struct MlFixArgs {
    const char *src;
    char *dst;
    uint64_t m;                 // elements of the result
    Fe<F> w[1 << ML_FIX_T];     // eq(r, b), the first variable on the top bit of b
};

template <class F, int T>
__global__ __launch_bounds__(ML_THREADS) void ml_fix_kernel(const MlFixArgs<F> a) {
    const uint64_t j = (uint64_t)blockIdx.x * ML_THREADS + threadIdx.x;
    if (j >= a.m) return;
    Fe<F> v[1 << T];
#pragma unroll
    for (int b = 0; b < (1 << T); b++) v[b] = fe_load<F>(a.src + ((uint64_t)b * a.m + j) * 32);
    Fe<F> acc = ml_dot2<F>(a.w[0], v[0], a.w[1], v[1]);
#pragma unroll
    for (int b = 2; b < (1 << T); b += 2) acc = fe_add<F>(acc, ml_dot2<F>(a.w[b], v[b], a.w[b + 1], v[b + 1]));
    fe_store<F>(a.dst + j * 32, acc);
}

// ---- sumcheck round ----
template <class F>
struct MlRoundArgs {
    char *tab[3];
    char *partials;             // [K + 1][gridDim.x]
    uint64_t q;                 // pairs (a, b) = (T[j], T[j + q]) of the table the products run over
    Fe<F> r;                    // FUSED: the previous round's challenge
};

template <class F, int K, bool FUSED>
__global__ __launch_bounds__(ML_THREADS) void ml_round_kernel(const MlRoundArgs<F> a) {
    __shared__ Fe<F> lds[ML_THREADS];
    Fe<F> acc[K + 1];
#pragma unroll
    for (int t = 0; t <= K; t++) acc[t] = Fe<F>::zero();
    const uint64_t q = a.q, step = (uint64_t)gridDim.x * ML_THREADS;
#pragma unroll 1
    for (uint64_t j = (uint64_t)blockIdx.x * ML_THREADS + threadIdx.x; j < q; j += step) {
        Fe<F> v[K], d[K];
#pragma unroll
        for (int k = 0; k < K; k++) ml_load_pair<F, FUSED>(a.tab[k] + j * 32, q, FUSED ? &a.r : nullptr, v[k], d[k]);
#pragma unroll
        for (int t = 0; t <= K; t++) {
            Fe<F> prod = v[0];
#pragma unroll
            for (int k = 1; k < K; k++) prod = fe_mul<F>(prod, v[k]);
            acc[t] = fe_add<F>(acc[t], prod);
            if (t < K) {
#pragma unroll
                for (int k = 0; k < K; k++) v[k] = fe_add<F>(v[k], d[k]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t <= K; t++) ml_store_partial<F>(acc[t], lds, a.partials, t);
}

// ---- host side ----
// out[b] = prod_{i < nb} eq(r[i], bit_{nb-1-i}(b)) for b < 2^nb; the entries from 2^nb up to `size` are zero, which is what
// a variable that is not there amounts to (r = 0 keeps bit 0 and drops bit 1)
template <class F>
static void ml_eq_table(const char *r, uint32_t nb, Fe<F> *out, uint32_t size) {
    out[0] = Fe<F>::one();
    for (uint32_t b = 1; b < size; b++) out[b] = Fe<F>::zero();
    for (uint32_t i = 0; i < nb; i++) {
        const Fe<F> ri = ml_load<F>(r + (size_t)i * 32);
        for (uint32_t b = 1u << i; b-- > 0;) {   // the reference's chis loop: the new variable becomes the lowest bit
            const Fe<F> hi = fe_mul<F>(out[b], ri);
            out[2 * b + 1] = hi;
            out[2 * b] = fe_sub<F>(out[b], hi);
        }
    }
}

// values[kk] = table kk at `point` -> out_host (k elements); synchronises.  n >= 1.
template <class F>
static int ml_evaluate_locked(Context &c, const void *const *tabs, uint32_t k, uint32_t n, const void *point, void *out_host,
                              hipStream_t s) {
    const uint64_t nb1 = n > (uint32_t)ML_LO ? (uint64_t)1 << (n - ML_LO) : 1;
    const uint64_t nb2 = n > 2u * ML_LO ? (uint64_t)1 << (n - 2 * ML_LO) : 1;
    // workspace: [values | partials of the first pass | partials of the second]
    const size_t vals_b = ml_round256((size_t)k * 32), p1_b = ml_round256((size_t)ML_TABS * nb1 * 32), p2_b = ml_round256((size_t)ML_TABS * nb2 * 32);
    if (c.poly_ws.ensure(vals_b + p1_b + p2_b)) return LW_ERR_ALLOC;
    char *vals = (char *)c.poly_ws.p, *part[2] = {vals + vals_b, vals + vals_b + p1_b};
    const char *r = (const char *)point;
    for (uint32_t k0 = 0; k0 < k; k0 += ML_TABS) {
        const uint32_t kc = k - k0 < (uint32_t)ML_TABS ? k - k0 : (uint32_t)ML_TABS;
        MlEvalArgs<F> a;
        memset(&a, 0, sizeof(a));
        for (uint32_t i = 0; i < kc; i++) a.tab[i] = (const char *)tabs[k0 + i];
        uint32_t nv = n;   // variables r[0 .. nv) are still free
        for (int pass = 0; nv > 0; pass++) {
            const uint32_t lo = nv < (uint32_t)ML_LO ? nv : (uint32_t)ML_LO;   // this pass folds r[nv - lo .. nv)
            a.len = (uint64_t)1 << nv;
            a.nblocks = (uint64_t)1 << (nv - lo);
            a.dst = nv == lo ? vals + (size_t)k0 * 32 : part[pass & 1];
            // index bit q of the run belongs to r[nv - 1 - q]: bits 0..3, 4..7, 8..10
            const uint32_t b0 = lo < 4 ? lo : 4, b1 = lo < 4 ? 0 : (lo < 8 ? lo - 4 : 4), b2 = lo < 8 ? 0 : lo - 8;
            ml_eq_table<F>(r + (size_t)(nv - b0) * 32, b0, a.eq16lo, 16);
            ml_eq_table<F>(r + (size_t)(nv - b0 - b1) * 32, b1, a.eq16hi, 16);
            ml_eq_table<F>(r + (size_t)(nv - lo) * 32, b2, a.eq8, 8);
            hipEvent_t pe = c.prof_begin(s);
            hipLaunchKernelGGL((ml_eval_pass_kernel<F>), dim3((uint32_t)a.nblocks, kc), dim3(ML_THREADS), 0, s, a);
            c.prof_end("ml_eval_pass_kernel", pe, s);
            LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
            nv -= lo;
            for (uint32_t i = 0; i < kc; i++) a.tab[i] = a.dst + (size_t)i * a.nblocks * 32;
        }
    }
    return ml_result(c, vals, (size_t)k * 32, out_host, s);
}

template <class F, int T>
static void ml_fix_launch(Context &c, const MlFixArgs<F> &a, hipStream_t s) {
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL((ml_fix_kernel<F, T>), dim3((uint32_t)((a.m + ML_THREADS - 1) / ML_THREADS)), dim3(ML_THREADS), 0, s, a);
    c.prof_end("ml_fix_kernel", pe, s);
}

// d_out = d_table with its first t variables bound to r; 1 <= t <= n.  Enqueues only.
template <class F>
static int ml_fix_locked(Context &c, const void *d_table, uint32_t n, const void *r, uint32_t t, void *d_out, hipStream_t s) {
    // intermediate tables of 2^(n-3), 2^(n-6), ... elements alternate between two workspace buffers
    const size_t wa = t > (uint32_t)ML_FIX_T ? ml_round256(((size_t)32 << n) >> ML_FIX_T) : 0;
    const size_t wb = t > 2u * ML_FIX_T ? ml_round256(((size_t)32 << n) >> (2 * ML_FIX_T)) : 0;
    if (wa && c.poly_ws.ensure(wa + wb)) return LW_ERR_ALLOC;
    char *ws[2] = {(char *)c.poly_ws.p, (char *)c.poly_ws.p + wa};
    MlFixArgs<F> a;
    memset(&a, 0, sizeof(a));
    a.src = (const char *)d_table;
    uint32_t nv = n;
    for (uint32_t done = 0, pass = 0; done < t; pass++) {
        const uint32_t tt = t - done < (uint32_t)ML_FIX_T ? t - done : (uint32_t)ML_FIX_T;
        a.m = (uint64_t)1 << (nv - tt);
        a.dst = done + tt == t ? (char *)d_out : ws[pass & 1];
        ml_eq_table<F>((const char *)r + (size_t)done * 32, tt, a.w, 1u << ML_FIX_T);
        if (tt == 1) ml_fix_launch<F, 1>(c, a, s);
        else if (tt == 2) ml_fix_launch<F, 2>(c, a, s);
        else ml_fix_launch<F, 3>(c, a, s);
        LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
        a.src = a.dst;
        nv -= tt;
        done += tt;
    }
    return LW_OK;
}

template <class F, int K>
static void ml_round_launch(Context &c, const MlRoundArgs<F> &a, bool fused, uint32_t blocks, hipStream_t s) {
    hipEvent_t pe = c.prof_begin(s);
    if (fused) hipLaunchKernelGGL((ml_round_kernel<F, K, true>), dim3(blocks), dim3(ML_THREADS), 0, s, a);
    else hipLaunchKernelGGL((ml_round_kernel<F, K, false>), dim3(blocks), dim3(ML_THREADS), 0, s, a);
    c.prof_end(fused ? "ml_round_kernel(fused)" : "ml_round_kernel", pe, s);
}

// the round polynomial's K + 1 values -> out_host; with r_prev the tables are first bound in place.  Synchronises.
template <class F>
static int ml_round_locked(Context &c, void *const *tabs, uint32_t k, uint32_t n, const void *r_prev, void *out_host, hipStream_t s) {
    MlRoundPlan plan;
    int rc = ml_round_plan(c, n, r_prev, k + 1, plan);
    if (rc) return rc;
    MlRoundArgs<F> a;
    memset(&a, 0, sizeof(a));
    for (uint32_t i = 0; i < k; i++) a.tab[i] = (char *)tabs[i];
    a.partials = plan.partials;
    a.q = plan.q;
    if (r_prev) a.r = ml_load<F>(r_prev);
    if (k == 1) ml_round_launch<F, 1>(c, a, r_prev != nullptr, plan.blocks, s);
    else if (k == 2) ml_round_launch<F, 2>(c, a, r_prev != nullptr, plan.blocks, s);
    else ml_round_launch<F, 3>(c, a, r_prev != nullptr, plan.blocks, s);
    return ml_round_finish<F>(c, plan, k + 1, out_host, s);
}

}  // namespace lw

using namespace lw;

extern "C" {

static int ml_evaluate_entry(lw_field_t field, const void *const *tabs, uint32_t k, uint32_t n, const void *point, void *out,
                             void *hip_stream, bool device) {
    if (!ml_field_ok(field)) return LW_ERR_BAD_ARG;
    if (k == 0) { set_error("no table"); return LW_ERR_BAD_ARG; }
    if (!ml_vars_ok(n)) return LW_ERR_BAD_ARG;
    if (!tabs || !out || (n && !point)) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    MlTables t = {(void *const *)tabs, k, n, device};   // only read here, so two may be the same table
    if (!t.ok(false)) return LW_ERR_BAD_ARG;
    if (n == 0 && !device) {   // a constant: no device needed
        for (uint32_t i = 0; i < k; i++) memcpy((char *)out + (size_t)i * 32, tabs[i], 32);
        return LW_OK;
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.stream;
    if (n == 0) {
        for (uint32_t i = 0; i < k; i++) LW_HIP_CHECK(hipMemcpyAsync((char *)out + (size_t)i * 32, tabs[i], 32, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
        LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
        return LW_OK;
    }
    int rc = t.stage(en, s);
    if (rc) return rc;
    return ml_with_field(field, [&](auto F) { return ml_evaluate_locked<decltype(F)>(c, t.on_device(), k, n, point, out, s); });
}
int lw_multilinear_evaluate(lw_field_t field, const void *const *tables, uint32_t k, uint32_t n_vars, const void *point, void *out) {
    return ml_evaluate_entry(field, tables, k, n_vars, point, out, nullptr, false);
}
int lw_multilinear_evaluate_device(lw_field_t field, const void *const *d_tables, uint32_t k, uint32_t n_vars, const void *point,
                                   void *out_host, void *hip_stream) {
    return ml_evaluate_entry(field, d_tables, k, n_vars, point, out_host, hip_stream, true);
}

static int ml_fix_entry(lw_field_t field, const void *table, uint32_t n, const void *r, uint32_t t, void *out, void *hip_stream,
                        bool device) {
    if (!ml_field_ok(field)) return LW_ERR_BAD_ARG;
    if (!ml_vars_ok(n)) return LW_ERR_BAD_ARG;
    if (t > n) { set_error("%u variables to bind of %u", t, n); return LW_ERR_BAD_ARG; }
    if (!table || !out || (t && !r)) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    const size_t in_b = (size_t)32 << n, out_b = (size_t)32 << (n - t);
    if (device) {
        if (!ml_aligned16(table) || !ml_aligned16(out)) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
        if (t && ml_overlap(table, in_b, out, out_b)) { set_error("the output overlaps the table"); return LW_ERR_BAD_ARG; }
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.stream;
    const void *d_table = table;
    void *d_out = out;
    if (!device) {
        s = en.use_lane_stream();
        if (!s) return en.rc;
        int rc = ml_upload(c.host_io_a, table, in_b, s);
        if (rc) return rc;
        d_table = c.host_io_a.p;
        if (c.host_io_b.ensure(out_b)) return LW_ERR_ALLOC;
        d_out = c.host_io_b.p;
    }
    if (t == 0) {
        if (d_out != d_table) LW_HIP_CHECK(hipMemcpyAsync(d_out, d_table, in_b, hipMemcpyDeviceToDevice, s), LW_ERR_LAUNCH);
    } else {
        int rc = ml_with_field(field, [&](auto F) { return ml_fix_locked<decltype(F)>(c, d_table, n, r, t, d_out, s); });
        if (rc) return rc;
    }
    return device ? LW_OK : ml_download(out, d_out, out_b, s);
}
int lw_multilinear_fix_variables(lw_field_t field, const void *table, uint32_t n_vars, const void *r, uint32_t t, void *out) {
    return ml_fix_entry(field, table, n_vars, r, t, out, nullptr, false);
}
int lw_multilinear_fix_variables_device(lw_field_t field, const void *d_table, uint32_t n_vars, const void *r, uint32_t t, void *d_out,
                                        void *hip_stream) {
    return ml_fix_entry(field, d_table, n_vars, r, t, d_out, hip_stream, true);
}

static int ml_round_entry(lw_field_t field, void *const *tabs, uint32_t k, uint32_t n, const void *r_prev, void *out, void *hip_stream,
                          bool device) {
    if (!ml_field_ok(field)) return LW_ERR_BAD_ARG;
    if (k == 0 || k > 3) { set_error("%u tables: a round takes 1, 2 or 3", k); return LW_ERR_BAD_ARG; }
    if (!ml_vars_ok(n) || !ml_round_vars_ok(n, r_prev)) return LW_ERR_BAD_ARG;
    if (!tabs || !out) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    MlTables t = {tabs, k, n, device};
    if (!t.ok(true)) return LW_ERR_BAD_ARG;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    hipStream_t s = en.stream;
    int rc = t.stage(en, s);
    if (rc) return rc;
    rc = ml_with_field(field, [&](auto F) { return ml_round_locked<decltype(F)>(en.c, t.on_device(), k, n, r_prev, out, s); });
    return rc || device || !r_prev ? rc : t.return_bound(s);
}
int lw_sumcheck_round(lw_field_t field, void *const *tables, uint32_t k, uint32_t n_vars, const void *r_prev_or_null, void *out_round) {
    return ml_round_entry(field, tables, k, n_vars, r_prev_or_null, out_round, nullptr, false);
}
int lw_sumcheck_round_device(lw_field_t field, void *const *d_tables, uint32_t k, uint32_t n_vars, const void *r_prev_or_null,
                             void *out_round_host, void *hip_stream) {
    return ml_round_entry(field, d_tables, k, n_vars, r_prev_or_null, out_round_host, hip_stream, true);
}

}  // extern "C"
