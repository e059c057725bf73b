// The prover's round of a sumcheck over an eq-weighted sum of products of dense multilinear tables, and the table of
// eq(point, .) that weights it.  Tables, element form and variable order are those of multilinear.hip.
//
//   eq table   out[i] = prod_j eq(point[j], bit_{n-1-j}(i)), i < 2^n.  With s = n / 2 the product splits into a factor over
//              the leading n - s variables (index bits s .. n-1) and one over the trailing s (bits 0 .. s-1):
//              ml_eq_half_kernel builds the two half tables, at most 2^15 elements each, every thread its own product of at
//              most 15 factors, with the point in the kernel's argument; ml_eq_outer_kernel writes
//              out[i] = hi[i >> s] * lo[i & (2^s - 1)], one product and one 32-byte store per element.  A half table over no
//              variable is the single element one, so n = 0 and n = 1 take the same path.
//   round      g(u) = sum_{j<h} E_j(u) * sum_t c_t * prod_{m in mask_t} T_m,j(u), u = 0 .. D, X_j(u) = X[j] + u (X[j+h] - X[j]),
//              h = 2^(n-1), D = max_t popcount(mask_t) + (eq ? 1 : 0)  (ml_terms_round_kernel<F, M, HAS_EQ, FUSED>).
//              The M tables and the eq table of a pair are loaded once into v[m], d[m] = hi - lo by ml_load_pair
//              (multilinear.cuh), the loader of ml_round_kernel, which also does the fused bind of four indices per table; u
//              walks by adding d[m].  The terms are a runtime loop over wave-uniform masks in the kernel's argument, the tables
//              of a term an unrolled loop behind a uniform test of the mask's bit, so that no register array is indexed by a
//              runtime value.  Per u the bracket sum_t c_t prod is formed first and E multiplies it once.  A coefficient one
//              costs no product and minus one is a subtraction: the host compares the coefficients with both and passes a
//              kind per term.  The accumulators are per u.  Blocks reduce and store with ml_store_partial, and the round is
//              planned and finished by the driver of the product round (ml_round_plan, ml_round_finish).
// Every stored value is a canonical residue, so neither the order of the products nor that of the sums shows in a result.
#include "multilinear.cuh"

namespace lw {

constexpr uint32_t MLT_MAX_TABLES = 4;
constexpr uint32_t MLT_MAX_TERMS = 8;
constexpr uint32_t MLT_MAX_FACTORS = 3;            // tables in one term
constexpr uint32_t MLT_EQ_HALF_VARS = 15;          // ceil(30 / 2)

// ---- eq table ----
template <class F>
struct MlEqArgs {
    char *half[2];              // [0]: over point[0 .. nv[0]), [1]: over point[nv[0] .. nv[0] + nv[1])
    uint32_t nv[2];
    Fe<F> point[ML_MAX_VARS];
};

// blockIdx.y picks the half table; thread i forms prod_j eq(r[j], bit_{nv-1-j}(i))
template <class F>
__global__ __launch_bounds__(ML_THREADS) void ml_eq_half_kernel(const MlEqArgs<F> a) {
    const uint32_t y = blockIdx.y, nv = a.nv[y], first = y ? a.nv[0] : 0;
    const uint32_t i = blockIdx.x * ML_THREADS + threadIdx.x;
    if (i >= (1u << nv)) return;
    Fe<F> acc = Fe<F>::one();
#pragma unroll 1
    for (uint32_t j = 0; j < nv; j++) {
        const Fe<F> r = a.point[first + j], nr = fe_sub<F>(Fe<F>::one(), r);
        const bool bit = (i >> (nv - 1 - j)) & 1;
        Fe<F> f;
#pragma unroll
        for (int w = 0; w < F::N; w++) f.v[w] = bit ? r.v[w] : nr.v[w];
        acc = fe_mul<F>(acc, f);
    }
    fe_store<F>(a.half[y] + (uint64_t)i * 32, acc);
}

template <class F>
__global__ __launch_bounds__(ML_THREADS) void ml_eq_outer_kernel(const char *hi, const char *lo, uint32_t s, uint64_t len, char *out) {
    const uint64_t i = (uint64_t)blockIdx.x * ML_THREADS + threadIdx.x;
    if (i >= len) return;
    const Fe<F> h = fe_load<F>(hi + (i >> s) * 32), l = fe_load<F>(lo + (i & (((uint64_t)1 << s) - 1)) * 32);
    fe_store<F>(out + i * 32, fe_mul<F>(h, l));
}

// ---- composed round ----
enum : uint32_t { MLT_COEFF_GENERAL = 0, MLT_COEFF_ONE = 1, MLT_COEFF_MINUS_ONE = 2 };

template <class F>
struct MlTermsArgs {
    char *tab[MLT_MAX_TABLES + 1];   // the M tables, then the eq table
    char *partials;                  // [deg + 1][gridDim.x]
    uint64_t q;                      // pairs (a, b) = (T[j], T[j + q]) of the table the products run over
    Fe<F> r;                         // FUSED: the previous round's challenge
    Fe<F> coeff[MLT_MAX_TERMS];
    uint32_t mask[MLT_MAX_TERMS];
    uint32_t kind[MLT_MAX_TERMS];
    uint32_t n_terms;
    uint32_t deg;                    // D: g(0) .. g(D) are summed
};

// One u: acc += E(u) * sum_t c_t prod_{m in mask_t} T_m(u), then (unless LAST) every table walks on to u + 1.
template <class F, int M, bool HAS_EQ, bool LAST>
__device__ __forceinline__ void mlt_point(const MlTermsArgs<F> &a, uint32_t n_terms, Fe<F> (&v)[M + (HAS_EQ ? 1 : 0)],
                                          const Fe<F> (&d)[M + (HAS_EQ ? 1 : 0)], Fe<F> &acc) {
    Fe<F> bracket = Fe<F>::zero();
#pragma unroll 1
    for (uint32_t t = 0; t < n_terms; t++) {
        const uint32_t mask = a.mask[t], kind = a.kind[t];
        Fe<F> prod = Fe<F>::zero();
        bool have = false;
#pragma unroll
        for (int m = 0; m < M; m++) {
            if ((mask >> m) & 1) {   // uniform
                prod = have ? fe_mul<F>(prod, v[m]) : v[m];
                have = true;
            }
        }
        if (kind == MLT_COEFF_ONE) bracket = fe_add<F>(bracket, prod);
        else if (kind == MLT_COEFF_MINUS_ONE) bracket = fe_sub<F>(bracket, prod);
        else bracket = fe_add<F>(bracket, fe_mul<F>(a.coeff[t], prod));
    }
    if (HAS_EQ) bracket = fe_mul<F>(v[M], bracket);
    acc = fe_add<F>(acc, bracket);
    if (!LAST) {
#pragma unroll
        for (int k = 0; k < M + (HAS_EQ ? 1 : 0); k++) v[k] = fe_add<F>(v[k], d[k]);
    }
}

template <class F, int M, bool HAS_EQ, bool FUSED>
__global__ __launch_bounds__(ML_THREADS) void ml_terms_round_kernel(const MlTermsArgs<F> a) {
    constexpr int MT = M + (HAS_EQ ? 1 : 0);                                             // tables a pair loads
    constexpr int DMAX = (M < (int)MLT_MAX_FACTORS ? M : (int)MLT_MAX_FACTORS) + (HAS_EQ ? 1 : 0);   // the most D can be
    __shared__ Fe<F> lds[ML_THREADS];
    Fe<F> acc[DMAX + 1];
#pragma unroll
    for (int u = 0; u <= DMAX; u++) acc[u] = Fe<F>::zero();
    const uint64_t q = a.q, step = (uint64_t)gridDim.x * ML_THREADS;
    const uint32_t n_terms = a.n_terms, deg = a.deg;
#pragma unroll 1
    for (uint64_t j = (uint64_t)blockIdx.x * ML_THREADS + threadIdx.x; j < q; j += step) {
        Fe<F> v[MT], d[MT];
#pragma unroll
        for (int k = 0; k < MT; k++) ml_load_pair<F, FUSED>(a.tab[k < M ? k : (int)MLT_MAX_TABLES] + j * 32, q, FUSED ? &a.r : nullptr, v[k], d[k]);
        // u = 0 .. DMAX written out: the loop's own unrolling is not left to the optimiser, since acc[] indexed by a loop
        // counter would go to scratch.  D >= 1 always.
        mlt_point<F, M, HAS_EQ, false>(a, n_terms, v, d, acc[0]);
        mlt_point<F, M, HAS_EQ, DMAX == 1>(a, n_terms, v, d, acc[1]);
        if constexpr (DMAX >= 2) {
            if (deg >= 2) mlt_point<F, M, HAS_EQ, DMAX == 2>(a, n_terms, v, d, acc[2]);
        }
        if constexpr (DMAX >= 3) {
            if (deg >= 3) mlt_point<F, M, HAS_EQ, DMAX == 3>(a, n_terms, v, d, acc[3]);
        }
        if constexpr (DMAX >= 4) {
            if (deg >= 4) mlt_point<F, M, HAS_EQ, true>(a, n_terms, v, d, acc[4]);
        }
    }
#pragma unroll
    for (int u = 0; u <= DMAX; u++) {
        if ((uint32_t)u <= deg) ml_store_partial<F>(acc[u], lds, a.partials, u);   // uniform: every thread reaches the barriers or none does
    }
}

// ---- host side ----
template <class F>
static int mlt_eq_locked(Context &c, const void *point, uint32_t n, void *d_out, hipStream_t s) {
    const uint32_t lo_v = n / 2, hi_v = n - lo_v;
    const size_t hi_b = ml_round256((size_t)32 << hi_v), lo_b = ml_round256((size_t)32 << lo_v);
    if (c.poly_ws.ensure(hi_b + lo_b)) return LW_ERR_ALLOC;
    MlEqArgs<F> a;
    memset(&a, 0, sizeof(a));
    a.half[0] = (char *)c.poly_ws.p;
    a.half[1] = a.half[0] + hi_b;
    a.nv[0] = hi_v;
    a.nv[1] = lo_v;
    for (uint32_t j = 0; j < n; j++) a.point[j] = ml_load<F>((const char *)point + (size_t)j * 32);
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL((ml_eq_half_kernel<F>), dim3(((1u << hi_v) + ML_THREADS - 1) / ML_THREADS, 2), dim3(ML_THREADS), 0, s, a);
    c.prof_end("ml_eq_half_kernel", pe, s);
    const uint64_t len = (uint64_t)1 << n;
    pe = c.prof_begin(s);
    hipLaunchKernelGGL((ml_eq_outer_kernel<F>), dim3((uint32_t)((len + ML_THREADS - 1) / ML_THREADS)), dim3(ML_THREADS), 0, s,
                       (const char *)a.half[0], (const char *)a.half[1], lo_v, len, (char *)d_out);
    c.prof_end("ml_eq_outer_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}

struct MltCall {   // a checked call
    uint32_t n_tables, n_terms, n, deg;
    const uint32_t *masks;
    const void *coeffs, *r_prev;
};

template <class F, int M, bool HAS_EQ>
static void mlt_launch(Context &c, const MlTermsArgs<F> &a, bool fused, uint32_t blocks, hipStream_t s) {
    hipEvent_t pe = c.prof_begin(s);
    if (fused) hipLaunchKernelGGL((ml_terms_round_kernel<F, M, HAS_EQ, true>), dim3(blocks), dim3(ML_THREADS), 0, s, a);
    else hipLaunchKernelGGL((ml_terms_round_kernel<F, M, HAS_EQ, false>), dim3(blocks), dim3(ML_THREADS), 0, s, a);
    c.prof_end(fused ? "ml_terms_round_kernel(fused)" : "ml_terms_round_kernel", pe, s);
}

template <class F, bool HAS_EQ>
static void mlt_launch_m(Context &c, const MlTermsArgs<F> &a, uint32_t m, bool fused, uint32_t blocks, hipStream_t s) {
    if (m == 1) mlt_launch<F, 1, HAS_EQ>(c, a, fused, blocks, s);
    else if (m == 2) mlt_launch<F, 2, HAS_EQ>(c, a, fused, blocks, s);
    else if (m == 3) mlt_launch<F, 3, HAS_EQ>(c, a, fused, blocks, s);
    else mlt_launch<F, 4, HAS_EQ>(c, a, fused, blocks, s);
}

// the round polynomial's deg + 1 values -> out_host; with r_prev the tables are first bound in place.  Synchronises.
template <class F>
static int mlt_round_locked(Context &c, void *const *tabs, void *eq, const MltCall &call, void *out_host, hipStream_t s) {
    MlRoundPlan plan;
    int rc = ml_round_plan(c, call.n, call.r_prev, call.deg + 1, plan);
    if (rc) return rc;
    MlTermsArgs<F> a;
    memset(&a, 0, sizeof(a));
    for (uint32_t i = 0; i < call.n_tables; i++) a.tab[i] = (char *)tabs[i];
    a.tab[MLT_MAX_TABLES] = (char *)eq;
    a.partials = plan.partials;
    a.q = plan.q;
    if (call.r_prev) a.r = ml_load<F>(call.r_prev);
    a.n_terms = call.n_terms;
    a.deg = call.deg;
    const Fe<F> one = Fe<F>::one(), minus_one = fe_neg<F>(one);
    for (uint32_t t = 0; t < call.n_terms; t++) {
        a.mask[t] = call.masks[t];
        a.coeff[t] = call.coeffs ? ml_load<F>((const char *)call.coeffs + (size_t)t * 32) : one;
        a.kind[t] = a.coeff[t] == one ? MLT_COEFF_ONE : a.coeff[t] == minus_one ? MLT_COEFF_MINUS_ONE : MLT_COEFF_GENERAL;
    }
    if (eq) mlt_launch_m<F, true>(c, a, call.n_tables, call.r_prev != nullptr, plan.blocks, s);
    else mlt_launch_m<F, false>(c, a, call.n_tables, call.r_prev != nullptr, plan.blocks, s);
    return ml_round_finish<F>(c, plan, call.deg + 1, out_host, s);
}

}  // namespace lw

using namespace lw;

extern "C" {

static int mlt_eq_entry(lw_field_t field, const void *point, uint32_t n, void *out, void *hip_stream, bool device) {
    if (!ml_field_ok(field)) return LW_ERR_BAD_ARG;
    if (!ml_vars_ok(n)) return LW_ERR_BAD_ARG;
    if (!out || (n && !point)) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    if (device && !ml_aligned16(out)) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    if (n == 0 && !device) {   // the element one: no device needed
        alignas(16) uint64_t w[4];
        ml_with_field(field, [&](auto F) { fe_store<decltype(F)>(w, Fe<decltype(F)>::one()); });
        memcpy(out, w, 32);
        return LW_OK;
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.stream;
    void *d_out = out;
    const size_t bytes = (size_t)32 << n;
    if (!device) {
        s = en.use_lane_stream();
        if (!s) return en.rc;
        if (c.host_io_a.ensure(bytes)) return LW_ERR_ALLOC;
        d_out = c.host_io_a.p;
    }
    int rc = ml_with_field(field, [&](auto F) { return mlt_eq_locked<decltype(F)>(c, point, n, d_out, s); });
    return rc || device ? rc : ml_download(out, d_out, bytes, s);
}
int lw_multilinear_eq_table(lw_field_t field, const void *point, uint32_t n_vars, void *out) {
    return mlt_eq_entry(field, point, n_vars, out, nullptr, false);
}
int lw_multilinear_eq_table_device(lw_field_t field, const void *point, uint32_t n_vars, void *d_out, void *hip_stream) {
    return mlt_eq_entry(field, point, n_vars, d_out, hip_stream, true);
}

static int mlt_round_entry(lw_field_t field, void *const *tabs, uint32_t n_tables, void *eq, const uint32_t *masks, const void *coeffs,
                           uint32_t n_terms, uint32_t n, const void *r_prev, void *out, void *hip_stream, bool device) {
    if (!ml_field_ok(field)) return LW_ERR_BAD_ARG;
    if (n_tables == 0 || n_tables > MLT_MAX_TABLES) { set_error("%u tables: a composed round takes 1 to %u", n_tables, MLT_MAX_TABLES); return LW_ERR_BAD_ARG; }
    if (n_terms == 0 || n_terms > MLT_MAX_TERMS) { set_error("%u terms: a composed round takes 1 to %u", n_terms, MLT_MAX_TERMS); return LW_ERR_BAD_ARG; }
    if (!ml_vars_ok(n) || !ml_round_vars_ok(n, r_prev)) return LW_ERR_BAD_ARG;
    if (!tabs || !masks || !out) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    uint32_t deg = 0;
    for (uint32_t t = 0; t < n_terms; t++) {
        const uint32_t m = masks[t], bits = (uint32_t)__builtin_popcount(m);
        if (m == 0 || (m >> n_tables) || bits > MLT_MAX_FACTORS) {
            set_error("term %u: mask 0x%x must name 1 to %u of the %u tables", t, m, MLT_MAX_FACTORS, n_tables);
            return LW_ERR_BAD_ARG;
        }
        if (bits > deg) deg = bits;
    }
    if (eq) deg++;
    void *all[MLT_MAX_TABLES + 1];   // the tables, then the eq table: the indices that the messages name
    uint32_t n_all = 0;
    for (uint32_t i = 0; i < n_tables; i++) all[n_all++] = tabs[i];
    if (eq) all[n_all++] = eq;
    MlTables t = {all, n_all, n, device};
    if (!t.ok(true)) return LW_ERR_BAD_ARG;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    hipStream_t s = en.stream;
    int rc = t.stage(en, s);
    if (rc) return rc;
    const MltCall call = {n_tables, n_terms, n, deg, masks, coeffs, r_prev};
    void *const *d_all = t.on_device();
    void *d_eq = eq ? d_all[n_tables] : nullptr;
    rc = ml_with_field(field, [&](auto F) { return mlt_round_locked<decltype(F)>(en.c, d_all, d_eq, call, out, s); });
    return rc || device || !r_prev ? rc : t.return_bound(s);
}
int lw_sumcheck_terms_round(lw_field_t field, void *const *tables, uint32_t n_tables, void *eq_or_null, const uint32_t *term_masks,
                            const void *term_coeffs_or_null, uint32_t n_terms, uint32_t n_vars, const void *r_prev_or_null, void *out_round) {
    return mlt_round_entry(field, tables, n_tables, eq_or_null, term_masks, term_coeffs_or_null, n_terms, n_vars, r_prev_or_null, out_round,
                           nullptr, false);
}
int lw_sumcheck_terms_round_device(lw_field_t field, void *const *d_tables, uint32_t n_tables, void *d_eq_or_null, const uint32_t *term_masks,
                                   const void *term_coeffs_or_null, uint32_t n_terms, uint32_t n_vars, const void *r_prev_or_null,
                                   void *out_round_host, void *hip_stream) {
    return mlt_round_entry(field, d_tables, n_tables, d_eq_or_null, term_masks, term_coeffs_or_null, n_terms, n_vars, r_prev_or_null,
                           out_round_host, hip_stream, true);
}

}  // extern "C"
