// The auxiliary column of a randomized AIR (the second half of round 1: AIR::build_auxiliary_trace) over a small field F with
// challenges in its extension E, written once over the policy E of ext_steps.cuh for goldilocks_ext.hip and babybear_ext.hip:
// the running product or the running sum of the fractions
//
//   f_i = (a_0 + sum_j a_j col_{s_j}[i]) / (b_0 + sum_j b_j col_{t_j}[i])          a, b in E, the columns in F, i < n
//
// inclusive (out[i] = f_0 .. f_i) or exclusive (out[0] = the neutral element, out[i] = f_0 .. f_{i-1}): the grand product of a
// permutation or memory argument and a LogUp sum.  Reduce-then-scan in three launches whatever n, as plonk.hip does for its
// grand product; no workgroup ever waits for another one.
//
// ext_aux_reduce_kernel   every tile of EXT_AUX_TILE rows: the product of its numerators and of its denominators (product
//                         mode) or the sum of its fractions (sum mode); counts the denominators that are zero
// ext_aux_carry_kernel    ONE workgroup of EXT_AUX_TOP work-items scans the tile values, work-item r owning ceil(tiles /
//                         EXT_AUX_TOP) consecutive tiles: per tile what comes before it (and, of the denominators, after it),
//                         the total, and in product mode the ONE inversion of the call, 1 / (the product of all
//                         denominators), by work-item 0
// ext_aux_rescan_kernel   every tile forms its rows again, scans them with its carries and stores the column
// Product mode is PLONK's form: with N_i the prefix product of the numerators through row i, S_i the product of the
// denominators after row i and T the inverse of all of them, f_0 .. f_i = N_i S_i T, so no row is inverted.  Sum mode needs
// every 1 / den_i: the EXT_AUX_E rows of a work-item share one E::inv (Montgomery's trick in registers).  The two lists are
// one uploaded table read at wave-uniform indices (air_uniform).  Rows from n on count as the neutral fraction.
// The carry launch is one workgroup whatever n: a work-item walks ceil(tiles / EXT_AUX_TOP) tile values serially (twice in
// product mode), so its time grows linearly with n - 16 tiles a work-item at 2^20 rows, a third of the product call there,
// and about 2^20 at the 2^36 rows the entry allows.  A 256-wide carry workgroup, or a second level of reduce-then-scan over
// the tile values, is the way out once traces of that length matter; neither is built.
#pragma once
#include "ext_round2.cuh"

namespace lw {

constexpr int EXT_AUX_E = 4;                                            // consecutive rows per work-item
constexpr uint64_t EXT_AUX_TILE = (uint64_t)EXT_THREADS * EXT_AUX_E;   // 1024 rows per workgroup
constexpr int EXT_AUX_TOP = 64;                                         // work-items of the carry kernel
constexpr uint32_t EXT_AUX_TERMS = LW_EXT_AUX_MAX_TERMS;

struct ExtAuxNames { const char *reduce, *carry, *rescan; };

// terms: per term the address of its column, 0, its coefficient (two words); the numerator's terms, then the denominator's
template <class E> struct ExtAuxArgs {
    const uint64_t *terms;
    uint64_t n, ntiles;
    uint32_t n_num, n_den, sum, exclusive, num_one;   // num_one: no numerator term and a_0 = 1
    typename E::elem num0, den0;
    typename E::elem *tile_a, *tile_b, *carry_a, *carry_b;   // a: numerators or fractions, b: denominators (product mode)
    typename E::elem *scale;                                 // product mode: 1 / (the product of all denominators)
    unsigned long long *zeros;
    typename E::word *total;                                 // or null
    ExtPlanes<E> out;
};

// the numerators and denominators of the rows base .. base + EXT_AUX_E - 1; a row from n on is the neutral fraction
template <class E>
__device__ __forceinline__ void ext_aux_rows(const ExtAuxArgs<E> &a, uint64_t base, typename E::elem (&num)[EXT_AUX_E], typename E::elem (&den)[EXT_AUX_E]) {
    using word = typename E::word;
    using elem = typename E::elem;
#pragma unroll
    for (int e = 0; e < EXT_AUX_E; e++) {
        const bool in = base + e < a.n;
        num[e] = in ? a.num0 : (a.sum ? E::zero() : E::one());
        den[e] = in ? a.den0 : E::one();
    }
#pragma unroll 1
    for (uint32_t j = 0; j < a.n_num; j++) {
        const word *col = (const word *)air_uniform(a.terms, 4 * (size_t)j) + base;
        const elem cf = air_uniform_elem<elem>(a.terms, 4 * (size_t)j + 2);
#pragma unroll
        for (int e = 0; e < EXT_AUX_E; e++)
            if (base + e < a.n) num[e] = E::add(num[e], E::mul_base(cf, E::fcanon(col[e])));
    }
#pragma unroll 1
    for (uint32_t j = a.n_num; j < a.n_num + a.n_den; j++) {
        const word *col = (const word *)air_uniform(a.terms, 4 * (size_t)j) + base;
        const elem cf = air_uniform_elem<elem>(a.terms, 4 * (size_t)j + 2);
#pragma unroll
        for (int e = 0; e < EXT_AUX_E; e++)
            if (base + e < a.n) den[e] = E::add(den[e], E::mul_base(cf, E::fcanon(col[e])));
    }
}

// f[e] = num[e] / den[e] with one inversion for the work-item's rows; `rows` of them lie below n, the others count as zero
// (with num_one their numerator is not looked at)
template <class E>
__device__ __forceinline__ void ext_aux_fractions_of(uint32_t num_one, uint64_t rows, const typename E::elem (&num)[EXT_AUX_E],
                                                     const typename E::elem (&den)[EXT_AUX_E], typename E::elem (&f)[EXT_AUX_E]) {
    using elem = typename E::elem;
    elem pre[EXT_AUX_E], run = E::one();
#pragma unroll
    for (int e = 0; e < EXT_AUX_E; e++) {
        pre[e] = run;
        run = E::mul(run, den[e]);
    }
    elem inv = E::inv(run);
#pragma unroll
    for (int e = EXT_AUX_E - 1; e >= 0; e--) {
        f[e] = E::mul(inv, pre[e]);
        if (!num_one) f[e] = E::mul(f[e], num[e]);
        if ((uint64_t)e >= rows) f[e] = E::zero();
        inv = E::mul(inv, den[e]);
    }
}

template <class E, bool MUL> __device__ __forceinline__ typename E::elem ext_aux_op(typename E::elem a, typename E::elem b) {
    if constexpr (MUL) return E::mul(a, b);
    else return E::add(a, b);
}
template <class E, bool MUL> __device__ __forceinline__ typename E::elem ext_aux_neutral() {
    if constexpr (MUL) return E::one();
    else return E::zero();
}
// Hillis-Steele scan over the workgroup's T work-items: on return v (and lds[r]) is the product or sum over r' <= r
// (SUFFIX: r' >= r).  The caller synchronises before it uses lds again.
template <class E, bool MUL, bool SUFFIX, int T> __device__ __forceinline__ typename E::elem ext_aux_block_scan(typename E::elem v, typename E::elem *lds) {
    const int r = threadIdx.x;
#pragma unroll 1
    for (int d = 1; d < T; d <<= 1) {
        lds[r] = v;
        __syncthreads();
        const int o = SUFFIX ? r + d : r - d;
        if (o >= 0 && o < T) v = ext_aux_op<E, MUL>(v, lds[o]);
        __syncthreads();
    }
    lds[r] = v;
    __syncthreads();
    return v;
}
// the neighbour's inclusive value is this work-item's exclusive one
template <class E, bool MUL, bool SUFFIX, int T> __device__ __forceinline__ typename E::elem ext_aux_scan_exclusive(const typename E::elem *lds) {
    const int o = SUFFIX ? (int)threadIdx.x + 1 : (int)threadIdx.x - 1;
    return (o >= 0 && o < T) ? lds[o] : ext_aux_neutral<E, MUL>();
}

template <class E> __global__ __launch_bounds__(EXT_THREADS) void ext_aux_reduce_kernel(const ExtAuxArgs<E> a) {
    using elem = typename E::elem;
    __shared__ elem lds[2][EXT_THREADS];
    const int r = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * EXT_AUX_TILE + (uint64_t)r * EXT_AUX_E;
    elem num[EXT_AUX_E], den[EXT_AUX_E];
    ext_aux_rows<E>(a, base, num, den);
    uint32_t zeros = 0;
#pragma unroll
    for (int e = 0; e < EXT_AUX_E; e++) zeros += E::is_zero(den[e]) ? 1u : 0u;   // a row from n on has the denominator 1
    if (zeros) atomicAdd(a.zeros, (unsigned long long)zeros);
    elem pa, pb = E::one();
    if (a.sum) {
        elem f[EXT_AUX_E];
        ext_aux_fractions_of<E>(a.num_one, base < a.n ? a.n - base : 0, num, den, f);
        pa = f[0];
#pragma unroll
        for (int e = 1; e < EXT_AUX_E; e++) pa = E::add(pa, f[e]);
    } else {
        pa = num[0];
        pb = den[0];
#pragma unroll
        for (int e = 1; e < EXT_AUX_E; e++) {
            if (!a.num_one) pa = E::mul(pa, num[e]);
            pb = E::mul(pb, den[e]);
        }
    }
#pragma unroll 1
    for (int s = EXT_THREADS / 2; s >= 1; s >>= 1) {
        lds[0][r] = pa;
        lds[1][r] = pb;
        __syncthreads();
        if (r < s) {
            if (a.sum) {
                pa = E::add(pa, lds[0][r + s]);
            } else {
                if (!a.num_one) pa = E::mul(pa, lds[0][r + s]);
                pb = E::mul(pb, lds[1][r + s]);
            }
        }
        __syncthreads();
    }
    if (r == 0) {
        a.tile_a[blockIdx.x] = pa;
        if (!a.sum) a.tile_b[blockIdx.x] = pb;
    }
}

template <class E> __global__ __launch_bounds__(EXT_AUX_TOP) void ext_aux_carry_kernel(const ExtAuxArgs<E> a) {
    using elem = typename E::elem;
    __shared__ elem lds[EXT_AUX_TOP];
    const uint64_t g = (a.ntiles + EXT_AUX_TOP - 1) / EXT_AUX_TOP;
    const uint64_t t0 = (uint64_t)threadIdx.x * g;
    const uint64_t t1 = t0 + g < a.ntiles ? t0 + g : a.ntiles;   // t0 >= t1: this work-item owns no tile
    elem total;
    if (a.sum) {
        elem ps = E::zero();
        for (uint64_t t = t0; t < t1; t++) ps = E::add(ps, a.tile_a[t]);
        ext_aux_block_scan<E, false, false, EXT_AUX_TOP>(ps, lds);
        elem carry = ext_aux_scan_exclusive<E, false, false, EXT_AUX_TOP>(lds);
        total = lds[EXT_AUX_TOP - 1];
        for (uint64_t t = t0; t < t1; t++) {
            a.carry_a[t] = carry;
            carry = E::add(carry, a.tile_a[t]);
        }
    } else {
        elem pn = E::one(), pd = E::one();
        for (uint64_t t = t0; t < t1; t++) {
            if (!a.num_one) pn = E::mul(pn, a.tile_a[t]);
            pd = E::mul(pd, a.tile_b[t]);
        }
        ext_aux_block_scan<E, true, false, EXT_AUX_TOP>(pn, lds);
        elem carry = ext_aux_scan_exclusive<E, true, false, EXT_AUX_TOP>(lds);
        const elem all_num = lds[EXT_AUX_TOP - 1];
        __syncthreads();
        if (!a.num_one)
            for (uint64_t t = t0; t < t1; t++) {
                a.carry_a[t] = carry;
                carry = E::mul(carry, a.tile_a[t]);
            }
        const elem all_den = ext_aux_block_scan<E, true, true, EXT_AUX_TOP>(pd, lds);   // work-item 0's is the product of all
        carry = ext_aux_scan_exclusive<E, true, true, EXT_AUX_TOP>(lds);
        for (uint64_t t = t1; t > t0; t--) {
            a.carry_b[t - 1] = carry;
            carry = E::mul(carry, a.tile_b[t - 1]);
        }
        total = all_num;
        if (threadIdx.x == 0) {   // the one inversion of the call
            const elem scale = E::inv(all_den);
            a.scale[0] = scale;
            total = E::mul(all_num, scale);
        }
    }
    if (threadIdx.x == 0 && a.total) {
        ExtPlanes<E> tp;
#pragma unroll
        for (int e = 0; e < E::D; e++) tp.p[e] = a.total + e;
        E::store(tp, 0, total);
    }
}

template <class E> __global__ __launch_bounds__(EXT_THREADS) void ext_aux_rescan_kernel(const ExtAuxArgs<E> a) {
    using elem = typename E::elem;
    __shared__ elem lds[EXT_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * EXT_AUX_TILE + (uint64_t)threadIdx.x * EXT_AUX_E;
    elem num[EXT_AUX_E], den[EXT_AUX_E], o[EXT_AUX_E];
    ext_aux_rows<E>(a, base, num, den);
    if (a.sum) {
        elem f[EXT_AUX_E];
        ext_aux_fractions_of<E>(a.num_one, base < a.n ? a.n - base : 0, num, den, f);
        elem ps = f[0];
#pragma unroll
        for (int e = 1; e < EXT_AUX_E; e++) ps = E::add(ps, f[e]);
        ext_aux_block_scan<E, false, false, EXT_THREADS>(ps, lds);
        elem run = E::add(ext_aux_scan_exclusive<E, false, false, EXT_THREADS>(lds), a.carry_a[blockIdx.x]);
#pragma unroll
        for (int e = 0; e < EXT_AUX_E; e++) {
            if (a.exclusive) o[e] = run;
            run = E::add(run, f[e]);
            if (!a.exclusive) o[e] = run;
        }
    } else {
        elem pn = num[0], pd = den[0];
#pragma unroll
        for (int e = 1; e < EXT_AUX_E; e++) {
            if (!a.num_one) pn = E::mul(pn, num[e]);
            pd = E::mul(pd, den[e]);
        }
        elem before = E::one();
        if (!a.num_one) {
            ext_aux_block_scan<E, true, false, EXT_THREADS>(pn, lds);
            before = E::mul(ext_aux_scan_exclusive<E, true, false, EXT_THREADS>(lds), a.carry_a[blockIdx.x]);
            __syncthreads();
        }
        ext_aux_block_scan<E, true, true, EXT_THREADS>(pd, lds);
        elem after = E::mul(E::mul(ext_aux_scan_exclusive<E, true, true, EXT_THREADS>(lds), a.carry_b[blockIdx.x]), a.scale[0]);
        // f_0 .. f_i = N_i S_i: S_i takes in the denominators after row i (and T), N_i the numerators through row i
        elem S[EXT_AUX_E];
#pragma unroll
        for (int e = EXT_AUX_E - 1; e >= 0; e--) {
            S[e] = after;
            after = E::mul(after, den[e]);
        }
#pragma unroll
        for (int e = 0; e < EXT_AUX_E; e++) {
            if (a.exclusive) o[e] = E::mul(before, E::mul(den[e], S[e]));   // N_{i-1} S_{i-1}
            if (!a.num_one) before = E::mul(before, num[e]);
            if (!a.exclusive) o[e] = E::mul(before, S[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < EXT_AUX_E; e++)
        if (base + e < a.n) E::store(a.out, base + e, o[e]);
}

// ---------------------------------------------------------------- host
// one list as the entry point takes it: the constant, the columns and the coefficients of its terms
template <class E> struct ExtAuxList {
    const typename E::word *constant;
    const uint32_t *cols;
    const typename E::word *coeffs;
    uint32_t n;
};

// the uploaded table of the two lists: per term the column's address, 0 and the coefficient as air_uniform_elem reads it
template <class E>
static void ext_aux_pack_terms(const typename E::word *const *cols, const ExtAuxList<E> &num, const ExtAuxList<E> &den, uint64_t *t) {
    uint32_t at = 0;
    for (const ExtAuxList<E> *l : {&num, &den})
        for (uint32_t j = 0; j < l->n; j++, at++) {
            t[4 * at] = (uint64_t)(uintptr_t)cols[l->cols[j]];
            t[4 * at + 1] = 0;
            r2_pack(ext_elem_of<E>(l->coeffs, j), t + 4 * at + 2);
        }
}

template <class E>
static int ext_aux_list_check(const ExtAuxList<E> &l, uint32_t n_cols, const char *what) {
    if (l.n > EXT_AUX_TERMS) { set_error("%s: %u terms, a list has at most %u", what, l.n, EXT_AUX_TERMS); return LW_ERR_BAD_ARG; }
    if (!l.constant || (l.n && (!l.cols || !l.coeffs))) { set_error("%s: null table", what); return LW_ERR_BAD_ARG; }
    for (uint32_t j = 0; j < l.n; j++)
        if (l.cols[j] >= n_cols) { set_error("%s: term %u: column %u of %u", what, j, l.cols[j], n_cols); return LW_ERR_BAD_ARG; }
    int rc = E::words_check(l.constant, E::D, what);
    if (!rc) rc = E::words_check(l.coeffs, (size_t)l.n * E::D, what);
    return rc;
}

// The body of the entry point.  The order of the checks: the length, the mode, the two lists (terms, null tables, columns,
// words), the output and its stride, the total, the columns (null, misaligned, overlapped by the output).
template <class E>
static int ext_aux_fractions(const ExtAuxNames &names, const typename E::word *const *d_columns, uint32_t n_cols, size_t n, const ExtAuxList<E> &num,
                             const ExtAuxList<E> &den, uint32_t mode, typename E::word *d_out, size_t out_stride, typename E::word *d_total_or_null,
                             uint64_t *out_zero_denominators_or_null, void *hip_stream) {
    using elem = typename E::elem;
    if (n == 0) { set_error("an auxiliary column of no rows"); return LW_ERR_BAD_ARG; }
    if (n > EXT_MAX_LEN) { set_error("%zu rows", n); return LW_ERR_ALLOC; }
    if (mode > (LW_EXT_AUX_SUM | LW_EXT_AUX_EXCLUSIVE)) { set_error("bad auxiliary column mode %u", mode); return LW_ERR_BAD_ARG; }
    int rc = ext_aux_list_check<E>(num, n_cols, "numerator");
    if (!rc) rc = ext_aux_list_check<E>(den, n_cols, "denominator");
    if (rc) return rc;
    if (n_cols && !d_columns) { set_error("null table"); return LW_ERR_BAD_ARG; }
    rc = d_total_or_null ? ext_device_ptrs({d_out, d_total_or_null}) : ext_device_ptrs({d_out});
    if (!rc) rc = ext_stride(out_stride, n, "out");
    if (rc) return rc;
    if (d_total_or_null && ext_overlap<E>(d_total_or_null, E::D, d_out, ext_span<E>(out_stride, n))) { set_error("the total overlaps out"); return LW_ERR_BAD_ARG; }
    for (uint32_t k = 0; k < n_cols; k++) {
        if (!d_columns[k] || !aligned16(d_columns[k])) { set_error("column %u: null or misaligned buffer", k); return LW_ERR_BAD_ARG; }
        if (ext_overlap<E>(d_columns[k], n, d_out, ext_span<E>(out_stride, n)) || (d_total_or_null && ext_overlap<E>(d_columns[k], n, d_total_or_null, E::D))) {
            set_error("out overlaps column %u", k);
            return LW_ERR_BAD_ARG;
        }
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.stream;
    const uint64_t nt = (n + EXT_AUX_TILE - 1) / EXT_AUX_TILE;
    const size_t b_terms = r2_round256((size_t)2 * EXT_AUX_TERMS * 32), b_tiles = r2_round256((size_t)nt * sizeof(elem));
    if (c.poly_ws.ensure(b_terms + 4 * b_tiles + 256)) return LW_ERR_ALLOC;
    char *ws = (char *)c.poly_ws.p;
    ExtAuxArgs<E> a;
    memset(&a, 0, sizeof(a));
    a.terms = (const uint64_t *)ws;
    a.n = n;
    a.ntiles = nt;
    a.n_num = num.n;
    a.n_den = den.n;
    a.sum = mode & LW_EXT_AUX_SUM;
    a.exclusive = (mode & LW_EXT_AUX_EXCLUSIVE) ? 1 : 0;
    a.num0 = ext_elem_of<E>(num.constant, 0);
    a.den0 = ext_elem_of<E>(den.constant, 0);
    const elem one = E::one();
    a.num_one = num.n == 0 && memcmp(&a.num0, &one, sizeof(elem)) == 0;
    a.tile_a = (elem *)(ws + b_terms);
    a.tile_b = (elem *)(ws + b_terms + b_tiles);
    a.carry_a = (elem *)(ws + b_terms + 2 * b_tiles);
    a.carry_b = (elem *)(ws + b_terms + 3 * b_tiles);
    a.scale = (elem *)(ws + b_terms + 4 * b_tiles);
    a.zeros = (unsigned long long *)(ws + b_terms + 4 * b_tiles + 64);
    a.total = d_total_or_null;
    a.out = ext_planes<E>(d_out, out_stride);
    if (num.n + den.n) {
        rc = deep_pin(c, b_terms);   // the caller's arrays are free on return
        if (rc) return rc;
        memset(c.deep_pin, 0, b_terms);
        ext_aux_pack_terms<E>(d_columns, num, den, (uint64_t *)c.deep_pin);
        LW_HIP_CHECK(hipMemcpyAsync(ws, c.deep_pin, b_terms, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
        LW_HIP_CHECK(hipEventRecord(c.deep_pin_read, s), LW_ERR_LAUNCH);
    }
    LW_HIP_CHECK(hipMemsetAsync(a.zeros, 0, 8, s), LW_ERR_LAUNCH);
    rc = launch_1d(c, names.reduce, ext_aux_reduce_kernel<E>, (uint32_t)nt, s, a);
    if (rc) return rc;
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL(ext_aux_carry_kernel<E>, dim3(1), dim3(EXT_AUX_TOP), 0, s, a);
    c.prof_end(names.carry, pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    rc = launch_1d(c, names.rescan, ext_aux_rescan_kernel<E>, (uint32_t)nt, s, a);
    if (rc || !out_zero_denominators_or_null) return rc;
    unsigned long long zeros = 0;
    rc = download(&zeros, a.zeros, 8, s);
    if (rc) return rc;
    *out_zero_denominators_or_null = zeros;
    if (zeros) { set_error("%llu rows have a zero denominator", zeros); return LW_ERR_INV_ZERO; }
    return LW_OK;
}

}  // namespace lw
