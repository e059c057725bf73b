// The steps a STARK prover runs in an extension field after round 1, written once for goldilocks_ext.hip (Fp2 over
// Goldilocks, u64 words) and babybear_ext.hip (Fp4 over BabyBear, stored u32 words): the kernels, the drivers that launch
// them, the argument helpers and the bodies of the four entry points (pointwise, evaluate, deep_quotients, fri_layer).
// A vector of n elements is E::D PLANES of n words, `stride` words apart.  An extension is a compile-time policy E, a
// struct of types, constants and static __device__ __forceinline__ functions, so every kernel holds a single inlined copy
// of E's arithmetic.
//
// evaluate: a work-item takes the partial sum of EXT_E consecutive coefficients (the extension's tile kernel), the 256 partial sums of
// a block fold in LDS under x^EXT_E, x^2EXT_E, ..., and a second launch of one block per (column, point) folds the tile
// sums the same way under x^EXT_TILE.  The coefficients are loaded once for all points of a launch (EXT_PTS at most; more
// points are more launches).  The power tables come from the host as kernel arguments (ext_power_tables).
//
// deep_quotients is one pass over the columns, no scan.  A work-item owns EXT_ROWS consecutive rows of the domain and the
// EXT_PTS points of the launch: it accumulates N_j(i) = sum_k w[k][j] col_k[i] (E::mul_base: the columns are in F; the
// constant sum_k w[k][j] e[k][j] is the host's, ext_deep_constant), takes x of its first row from one E::fpow and steps by
// w, and inverts the EXT_ROWS x EXT_PTS norms of x_i - z_j with ONE E::finv (Montgomery's trick over registers); E::quotient
// turns a norm's inverse into (N_j(i) - c_j) / (x_i - z_j).  The way back through the trick is a loop in the kernel or a
// recursion over a template argument, as E says (E::DEEP_BACK_BY_RECURSION): one form does not suit both, DESIGN 4.25.
// A hook that takes a member of the kernel's argument struct takes it BY VALUE: a reference makes the compiler copy the
// whole struct to private memory at entry, which cost gl2_deep_kernel 8 to 12 VGPRs and a wave of occupancy.
//
// What E supplies:
//   E::word, E::elem, E::D                    a word of F, an element, its number of coordinates (elem has a member c0)
//   E::NAME, E::NAMES                         "Fp2" in error texts; the kernels' lines in lw_hip_profile_end (ExtNames)
//   E::F_ONE, E::fcanon, E::fmul, E::fpow, E::finv   the base field: one, a word as the kernels compute with it (Goldilocks
//                                             takes any u64), product, power, inverse
//   E::load(planes, i), E::store(planes, i, v)   element i of a vector (ExtPlanes) as it lies there, and back
//   E::canon(v)                               the element of words read from a caller (E::fcanon of every coordinate)
//   E::zero, E::one, E::is_zero, E::add, E::sub, E::mul, E::sqr, E::inv, E::mul_base
//   E::eval_point, E::eval_point_of(xp)       what the extension's tile kernel needs of a point, from the table 1, x, ..., x^(EXT_E - 1)
//   E::deep_point, E::deep_point_of(z)        a point's constants in the DEEP kernel
//   E::norm(x, pt)                            the norm of x - z in F, x in F: never zero for z outside F
//   E::quotient(num, x, pt, ninv)             num / (x - z) from ninv = 1 / norm
//   E::DEEP_BACK_BY_RECURSION                 the form of the way back through Montgomery's trick
//   E::fadd, E::fsub, E::R2_ROWS_FEW          round 2 (ext_round2.cuh): sum and difference in F, the boundary kernel's rows per work-item
// and on the host:
//   E::words_check(words, count, what)        host scalars: LW_ERR_BAD_ARG unless every word is one the kernels may take
//   E::size_check(log2n), E::root_check(root), E::offset(offset_or_null, h), E::domain_root(root, log2n)
//                                             the domain x_i = h w^i of 2^log2n points; root is the caller's two-adic root
//                                             where the field lets the caller choose one
#pragma once
#include <string.h>
#include <vector>
#include "hash_tree.cuh"

#define EXT_HD static __host__ __device__ __forceinline__   // a policy function that the host tables call too

namespace lw {

constexpr int EXT_THREADS = 256;
constexpr int EXT_E = 8;                                          // evaluate: consecutive coefficients per work-item
constexpr uint64_t EXT_TILE = (uint64_t)EXT_THREADS * EXT_E;      // 2048 coefficients per block
constexpr int EXT_STEPS = 8;                                      // log2(EXT_THREADS) steps of the block fold
constexpr int EXT_PTS = 4;                                        // points per launch, evaluate and DEEP
constexpr int EXT_ROWS = 4;   // DEEP rows per work-item: EXT_ROWS x EXT_PTS norms share one inversion.  Not measured against 2 or 8.
constexpr uint64_t EXT_MAX_LEN = (uint64_t)1 << 36;               // the grids' block indices stay below 2^31
static_assert((int)LW_GL2_MUL == (int)LW_BB4_MUL && (int)LW_GL2_SQR == (int)LW_BB4_SQR && (int)LW_GL2_INV == (int)LW_BB4_INV &&
                  (int)LW_GL2_MUL_BASE == (int)LW_BB4_MUL_BASE, "one pointwise kernel reads the ops of both extensions");
enum { EXT_MUL = LW_GL2_MUL, EXT_SQR = LW_GL2_SQR, EXT_INV = LW_GL2_INV, EXT_MUL_BASE = LW_GL2_MUL_BASE };

// a vector on its way into a kernel: one pointer per plane, formed on the host
template <class E> struct ExtPlanes { typename E::word *p[E::D]; };
template <class E> static __host__ __device__ ExtPlanes<E> ext_planes(const typename E::word *p, size_t stride) {
    ExtPlanes<E> v;
    for (int e = 0; e < E::D; e++) v.p[e] = const_cast<typename E::word *>(p) + e * stride;
    return v;
}

struct ExtNames { const char *pointwise, *eval_tile, *eval_fold, *deep, *fri_fold; };

// ---------------------------------------------------------------- host tables: plain arithmetic, no Context
// host scalar i of a table of E::D words per scalar
template <class E> static typename E::elem ext_elem_of(const typename E::word *tab, size_t i) { return E::canon(E::load(ext_planes<E>(tab + E::D * i, 1), 0)); }

// the power tables of the point x for a fold kernel whose work-items take `group` tile sums each
template <class E> struct ExtPowers {
    typename E::elem xp[EXT_E];       // x^e, e < EXT_E
    typename E::elem pe[EXT_STEPS];   // x^(EXT_E 2^s)
    typename E::elem xt;              // x^EXT_TILE
    typename E::elem pg[EXT_STEPS];   // x^(EXT_TILE group 2^s)
};
template <class E> static void ext_power_tables(typename E::elem x, uint32_t group, ExtPowers<E> &t) {
    t.xp[0] = E::one();
    for (int e = 1; e < EXT_E; e++) t.xp[e] = E::mul(t.xp[e - 1], x);
    t.pe[0] = E::mul(t.xp[EXT_E - 1], x);
    for (int st = 1; st < EXT_STEPS; st++) t.pe[st] = E::sqr(t.pe[st - 1]);
    t.xt = E::sqr(t.pe[EXT_STEPS - 1]);   // x^(EXT_E 2^EXT_STEPS) = x^EXT_TILE
    t.pg[0] = E::one();
    typename E::elem b = t.xt;
    for (uint32_t e = group; e; e >>= 1, b = E::sqr(b))
        if (e & 1) t.pg[0] = E::mul(t.pg[0], b);
    for (int st = 1; st < EXT_STEPS; st++) t.pg[st] = E::sqr(t.pg[st - 1]);
}
// the n_cols x m weights as ceil(m / EXT_PTS) groups of [n_cols][EXT_PTS], zero where a group has no point
template <class E> static void ext_regroup_weights(const typename E::word *weights, uint32_t n_cols, uint32_t m, typename E::elem *out) {
    memset(out, 0, (size_t)((m + EXT_PTS - 1) / EXT_PTS) * n_cols * EXT_PTS * sizeof(typename E::elem));
    for (uint32_t k = 0; k < n_cols; k++)
        for (uint32_t j = 0; j < m; j++) out[((size_t)(j / EXT_PTS) * n_cols + k) * EXT_PTS + j % EXT_PTS] = ext_elem_of<E>(weights, (size_t)k * m + j);
}
// c_j = sum_k w[k][j] e[k][j]
template <class E>
static typename E::elem ext_deep_constant(const typename E::word *weights, const typename E::word *evals, uint32_t n_cols, uint32_t m, uint32_t j) {
    typename E::elem cj = E::zero();
    for (uint32_t k = 0; k < n_cols; k++) cj = E::add(cj, E::mul(ext_elem_of<E>(weights, (size_t)k * m + j), ext_elem_of<E>(evals, (size_t)k * m + j)));
    return cj;
}

// ---------------------------------------------------------------- pointwise
template <class E>
__global__ __launch_bounds__(EXT_THREADS) void ext_pointwise_kernel(int op, const ExtPlanes<E> a, const ExtPlanes<E> b, const ExtPlanes<E> out, uint64_t n) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const typename E::elem x = E::canon(E::load(a, i));
        typename E::elem r;
        switch (op) {   // uniform
        case EXT_MUL: r = E::mul(x, E::canon(E::load(b, i))); break;
        case EXT_SQR: r = E::sqr(x); break;
        case EXT_INV: r = E::inv(x); break;
        default: r = E::mul_base(x, E::fcanon(b.p[0][i])); break;   // EXT_MUL_BASE
        }
        E::store(out, i, r);
    }
}

// ---------------------------------------------------------------- evaluate
template <class E> struct ExtEvalArgs {
    const typename E::word *cols;
    uint64_t col_stride, n, ntiles;
    uint32_t k0;               // first column of this launch
    uint32_t m, m_total, j0;   // points of this launch, of the call, and the first of this launch
    uint32_t group;            // fold: tiles per work-item
    typename E::elem *sums;    // [n_cols][EXT_PTS][ntiles]
    typename E::elem *vals;    // [n_cols][m_total]
    typename E::eval_point x[EXT_PTS];
    typename E::elem pe[EXT_PTS][EXT_STEPS];   // x^(EXT_E 2^s)
    typename E::elem xt[EXT_PTS];              // x^EXT_TILE
    typename E::elem pg[EXT_PTS][EXT_STEPS];   // x^(EXT_TILE group 2^s)
};

// sum_r w^r v_r over the block's 256 work-items, pw[s] = w^(2^s): the result is work-item 0's.  At step s the work-items
// whose index is a multiple of 2^(s+1) take in the one 2^s above, which was active in the step before.
template <class E> __device__ __forceinline__ typename E::elem ext_block_fold(typename E::elem v, typename E::elem *lds, const typename E::elem *pw) {
    const int r = threadIdx.x;
#pragma unroll 1
    for (int s = 0; s < EXT_STEPS; s++) {
        lds[r] = v;
        __syncthreads();
        const int d = 1 << s;
        if ((r & (2 * d - 1)) == 0) v = E::add(v, E::mul(pw[s], lds[r + d]));   // r + d <= 255
        __syncthreads();
    }
    return v;
}

// The tile kernel is the extension's own (gl2_eval_tile_kernel, bb4_eval_tile_kernel): tile sums S[k][j][t] = sum_{i in tile t}
// col_k[i] x_j^(i - t EXT_TILE) into a.sums[(k EXT_PTS + j) ntiles + t], the partial sum of a work-item its own way, then
// ext_block_fold under a.pe[j].  As a shared kernel over a partial-sum hook, Fp4's came out 8 instructions longer per point
// and 2 to 3 % slower; the hook's function boundary alone did that.
// one block per (column, point): the value sum_t S[t] x^(t EXT_TILE).  A work-item folds `group` consecutive tile sums.
template <class E> __global__ __launch_bounds__(EXT_THREADS) void ext_eval_fold_kernel(const ExtEvalArgs<E> a) {
    __shared__ typename E::elem lds[EXT_THREADS];
    const uint32_t k = a.k0 + blockIdx.x / a.m, j = blockIdx.x % a.m;
    const typename E::elem *s = a.sums + ((uint64_t)k * EXT_PTS + j) * a.ntiles;
    const uint64_t first = (uint64_t)threadIdx.x * a.group;
    const typename E::elem xt = a.xt[j];
    typename E::elem v = E::zero();
    for (uint32_t g = a.group; g-- > 0;)
        if (first + g < a.ntiles) v = E::add(E::mul(v, xt), s[first + g]);
    v = ext_block_fold<E>(v, lds, a.pg[j]);
    if (threadIdx.x == 0) a.vals[(uint64_t)k * a.m_total + a.j0 + j] = v;
}

// ---------------------------------------------------------------- DEEP quotients
template <class E> struct ExtDeepArgs {
    const typename E::word *cols;
    uint64_t col_stride;
    uint32_t n_cols, log2n, accumulate;
    typename E::word h, w;                  // x_i = h w^i
    const typename E::elem *wt;             // [n_cols][EXT_PTS]: the weights of this launch's points
    typename E::deep_point z[EXT_PTS];      // the points
    typename E::elem c[EXT_PTS];            // sum_k w[k][j] e[k][j]
    ExtPlanes<E> out;
};

// The way back as a recursion over the template argument, steps Q, Q - 1, ..., 0 with (row, point) = (Q / M, Q % M), for an
// extension whose step is long enough that the 16-step loop is left partly rolled (E::DEEP_BACK_BY_RECURSION).
template <class E, int Q, int M>
__device__ __forceinline__ void ext_deep_back(const ExtDeepArgs<E> &a, const typename E::word (&x)[EXT_ROWS], const typename E::word (&nr)[EXT_ROWS][M],
                                              const typename E::word (&pre)[EXT_ROWS][M], const typename E::elem (&acc)[EXT_ROWS][M], typename E::word inv,
                                              typename E::elem (&sum)[EXT_ROWS]) {
    constexpr int r = Q / M, j = Q % M;
    const typename E::elem q = E::quotient(E::sub(acc[r][j], a.c[j]), x[r], a.z[j], E::fmul(inv, pre[r][j]));
    sum[r] = j == M - 1 ? q : E::add(sum[r], q);
    if constexpr (Q > 0) ext_deep_back<E, Q - 1, M>(a, x, nr, pre, acc, E::fmul(inv, nr[r][j]), sum);
}

template <class E, int M> __global__ __launch_bounds__(EXT_THREADS) void ext_deep_kernel(const ExtDeepArgs<E> a) {
    using word = typename E::word;
    using elem = typename E::elem;
    const uint64_t n = 1ull << a.log2n;
    const uint64_t row0 = ((uint64_t)blockIdx.x * EXT_THREADS + threadIdx.x) * EXT_ROWS;
    if (row0 >= n) return;
    elem acc[EXT_ROWS][M];
#pragma unroll
    for (int r = 0; r < EXT_ROWS; r++)
#pragma unroll
        for (int j = 0; j < M; j++) acc[r][j] = E::zero();
#pragma unroll 1
    for (uint32_t k = 0; k < a.n_cols; k++) {
        const word *col = a.cols + (uint64_t)k * a.col_stride + row0;
        word v[EXT_ROWS];
#pragma unroll
        for (int r = 0; r < EXT_ROWS; r++) v[r] = row0 + r < n ? E::fcanon(col[r]) : 0;   // n < EXT_ROWS: the rows past the domain
#pragma unroll
        for (int j = 0; j < M; j++) {
            const elem w = a.wt[(uint64_t)k * EXT_PTS + j];   // uniform
            if (E::is_zero(w)) continue;                      // a zero weight skips the pair
#pragma unroll
            for (int r = 0; r < EXT_ROWS; r++) acc[r][j] = E::add(acc[r][j], E::mul_base(w, v[r]));
        }
    }
    // the norms of x_i - z_j and their running products
    word x[EXT_ROWS], nr[EXT_ROWS][M], pre[EXT_ROWS][M];
    x[0] = E::fmul(a.h, E::fpow(a.w, row0));
#pragma unroll
    for (int r = 1; r < EXT_ROWS; r++) x[r] = E::fmul(x[r - 1], a.w);
    word run = E::F_ONE;
#pragma unroll
    for (int r = 0; r < EXT_ROWS; r++)
#pragma unroll
        for (int j = 0; j < M; j++) {
            nr[r][j] = E::norm(x[r], a.z[j]);
            pre[r][j] = run;
            run = E::fmul(run, nr[r][j]);
        }
    // the way back: 1 / norm from the running inverse, the quotient from it (E::quotient) onto the row's sum
    word inv = E::finv(run);   // run != 0: every norm is non-zero
    elem sum[EXT_ROWS];
    if constexpr (E::DEEP_BACK_BY_RECURSION) {
        ext_deep_back<E, EXT_ROWS * M - 1, M>(a, x, nr, pre, acc, inv, sum);
    } else {
#pragma unroll
        for (int r = EXT_ROWS - 1; r >= 0; r--) {
            sum[r] = E::zero();
#pragma unroll
            for (int j = M - 1; j >= 0; j--) {
                const word ninv = E::fmul(inv, pre[r][j]);
                inv = E::fmul(inv, nr[r][j]);
                sum[r] = E::add(sum[r], E::quotient(E::sub(acc[r][j], a.c[j]), x[r], a.z[j], ninv));
            }
        }
    }
#pragma unroll
    for (int r = 0; r < EXT_ROWS; r++) {
        if (row0 + r >= n) break;
        elem o = sum[r];
        if (a.accumulate) o = E::add(o, E::load(a.out, row0 + r));   // canonical: an earlier launch wrote them
        E::store(a.out, row0 + r, o);
    }
}

// ---------------------------------------------------------------- FRI fold
// out[i] = 2 (c[2i] + zeta c[2i+1]) for i < n_out, the odd term absent past n; zeros up to `padded`
template <class E>
__global__ __launch_bounds__(EXT_THREADS) void ext_fri_fold_kernel(const ExtPlanes<E> c, uint64_t n, typename E::elem zeta, const ExtPlanes<E> out,
                                                                   uint64_t n_out, uint64_t padded) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= padded) return;
    typename E::elem r = E::zero();
    if (i < n_out) {
        r = E::canon(E::load(c, 2 * i));
        if (2 * i + 1 < n) r = E::add(r, E::mul(zeta, E::canon(E::load(c, 2 * i + 1))));
        r = E::add(r, r);
    }
    E::store(out, i, r);
}

// ---------------------------------------------------------------- host: argument helpers
template <class E> static bool ext_overlap(const void *a, size_t a_words, const void *b, size_t b_words) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + sizeof(typename E::word) * b_words && b0 < a0 + sizeof(typename E::word) * a_words;
}
// the words from the first of a vector of n elements to its last, the planes `stride` apart
template <class E> static size_t ext_span(size_t stride, size_t n) { return (E::D - 1) * stride + n; }
// a vector of n elements in planes `stride` words apart (0: n; below n: an error)
static int ext_stride(size_t &stride, size_t n, const char *what) {
    if (stride == 0) stride = n;
    if (stride < n) { set_error("%s: plane stride %zu below the length %zu", what, stride, n); return LW_ERR_BAD_ARG; }
    return LW_OK;
}
static int ext_device_ptrs(std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs) {
        if (!p) { set_error("null buffer"); return LW_ERR_BAD_ARG; }
        if (!aligned16(p)) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    }
    return LW_OK;
}

// ---------------------------------------------------------------- host: drivers
template <class E>
static int ext_evaluate_locked(Context &c, void (*tile_kernel)(ExtEvalArgs<E>), const typename E::word *d_coeffs, uint32_t n_cols, uint64_t col_stride, uint64_t n,
                               const typename E::word *points, uint32_t m, typename E::word *out_values, hipStream_t s) {
    using elem = typename E::elem;
    const uint64_t nt = (n + EXT_TILE - 1) / EXT_TILE;
    const size_t sums_b = ((size_t)n_cols * EXT_PTS * nt * sizeof(elem) + 255) & ~(size_t)255;
    if (c.poly_ws.ensure(sums_b + (size_t)n_cols * m * sizeof(elem))) return LW_ERR_ALLOC;
    ExtEvalArgs<E> a;
    memset(&a, 0, sizeof(a));
    a.cols = d_coeffs;
    a.col_stride = col_stride;
    a.n = n;
    a.ntiles = nt;
    a.m_total = m;
    a.group = (uint32_t)((nt + EXT_THREADS - 1) / EXT_THREADS);
    a.sums = (elem *)c.poly_ws.p;
    a.vals = (elem *)((char *)c.poly_ws.p + sums_b);
    for (uint32_t j0 = 0; j0 < m; j0 += EXT_PTS) {
        a.j0 = j0;
        a.m = m - j0 < (uint32_t)EXT_PTS ? m - j0 : (uint32_t)EXT_PTS;
        for (uint32_t j = 0; j < a.m; j++) {
            ExtPowers<E> t;
            ext_power_tables<E>(ext_elem_of<E>(points, j0 + j), a.group, t);
            a.x[j] = E::eval_point_of(t.xp);
            memcpy(a.pe[j], t.pe, sizeof(t.pe));
            a.xt[j] = t.xt;
            memcpy(a.pg[j], t.pg, sizeof(t.pg));
        }
        for (uint32_t k0 = 0; k0 < n_cols; k0 += 65535) {   // the grid's y extent
            const uint32_t kc = n_cols - k0 < 65535 ? n_cols - k0 : 65535;
            a.k0 = k0;
            hipEvent_t pe = c.prof_begin(s);
            hipLaunchKernelGGL(tile_kernel, dim3((uint32_t)nt, kc), dim3(EXT_THREADS), 0, s, a);
            c.prof_end(E::NAMES.eval_tile, pe, s);
            pe = c.prof_begin(s);
            hipLaunchKernelGGL(ext_eval_fold_kernel<E>, dim3(kc * a.m), dim3(EXT_THREADS), 0, s, a);
            c.prof_end(E::NAMES.eval_fold, pe, s);
            LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
        }
    }
    return download(out_values, a.vals, (size_t)n_cols * m * sizeof(elem), s);
}

template <class E>
static int ext_deep_locked(Context &c, const typename E::word *d_lde, uint32_t n_cols, uint64_t col_stride, uint32_t log2n, typename E::word h,
                           typename E::word w, const typename E::word *points, uint32_t m, const typename E::word *weights,
                           const typename E::word *evals, typename E::word *d_out, uint64_t out_stride, hipStream_t s) {
    using elem = typename E::elem;
    const uint32_t groups = (m + EXT_PTS - 1) / EXT_PTS;
    const size_t group_b = (size_t)n_cols * EXT_PTS * sizeof(elem), tables = group_b * groups;
    if (c.poly_ws.ensure(tables)) return LW_ERR_ALLOC;
    int rc = deep_pin(c, tables);
    if (rc) return rc;
    ext_regroup_weights<E>(weights, n_cols, m, (elem *)c.deep_pin);
    LW_HIP_CHECK(hipMemcpyAsync(c.poly_ws.p, c.deep_pin, tables, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipEventRecord(c.deep_pin_read, s), LW_ERR_LAUNCH);
    ExtDeepArgs<E> a;
    memset(&a, 0, sizeof(a));
    a.cols = d_lde;
    a.col_stride = col_stride;
    a.n_cols = n_cols;
    a.log2n = log2n;
    a.h = h;
    a.w = w;
    a.out = ext_planes<E>(d_out, out_stride);
    const uint64_t rows = 1ull << log2n, items = (rows + EXT_ROWS - 1) / EXT_ROWS;
    for (uint32_t g = 0; g < groups; g++) {
        const uint32_t j0 = g * EXT_PTS, mp = m - j0 < (uint32_t)EXT_PTS ? m - j0 : (uint32_t)EXT_PTS;
        a.wt = (const elem *)((const char *)c.poly_ws.p + group_b * g);
        a.accumulate = g > 0;
        for (uint32_t j = 0; j < mp; j++) {
            a.z[j] = E::deep_point_of(ext_elem_of<E>(points, j0 + j));
            a.c[j] = ext_deep_constant<E>(weights, evals, n_cols, m, j0 + j);
        }
        void (*kernel)(ExtDeepArgs<E>) = mp == 1 ? ext_deep_kernel<E, 1> : mp == 2 ? ext_deep_kernel<E, 2> : mp == 3 ? ext_deep_kernel<E, 3> : ext_deep_kernel<E, 4>;
        rc = launch_1d(c, E::NAMES.deep, kernel, blocks_for(items), s, a);
        if (rc) return rc;
    }
    return LW_OK;
}

// ---------------------------------------------------------------- host: the bodies of the entry points
template <class E>
static int ext_pointwise(int op, const typename E::word *d_a, size_t a_stride, const typename E::word *d_b, size_t b_stride, typename E::word *d_out,
                         size_t out_stride, size_t n, void *hip_stream) {
    if (op != EXT_MUL && op != EXT_SQR && op != EXT_INV && op != EXT_MUL_BASE) { set_error("bad %s op %d", E::NAME, op); return LW_ERR_BAD_ARG; }
    if (n == 0) return LW_OK;
    if (n > EXT_MAX_LEN) { set_error("%zu %s elements", n, E::NAME); return LW_ERR_ALLOC; }
    const bool has_b = op == EXT_MUL || op == EXT_MUL_BASE;
    int rc = has_b ? ext_device_ptrs({d_a, d_b, d_out}) : ext_device_ptrs({d_a, d_out});
    if (!rc) rc = ext_stride(a_stride, n, "a");
    if (!rc) rc = ext_stride(out_stride, n, "out");
    if (!rc && op == EXT_MUL) rc = ext_stride(b_stride, n, "b");
    if (rc) return rc;
    // The output may BE an operand, the whole vector under the same stride (work-item i reads element i of everything
    // before it writes element i); any other overlap of a plane of the output with a plane of an operand is refused.
    const bool out_is_a = d_out == d_a && out_stride == a_stride, out_is_b = op == EXT_MUL && d_out == d_b && out_stride == b_stride;
    const int b_planes = op == EXT_MUL ? E::D : has_b ? 1 : 0;
    for (int o = 0; o < E::D; o++)
        for (int e = 0; e < E::D; e++)
            if ((!out_is_a && ext_overlap<E>(d_out + o * out_stride, n, d_a + e * a_stride, n)) ||
                (!out_is_b && e < b_planes && ext_overlap<E>(d_out + o * out_stride, n, d_b + e * b_stride, n))) {
                set_error("out overlaps an operand without being the same vector under the same stride");
                return LW_ERR_BAD_ARG;
            }
    ExtPlanes<E> b{};   // MUL_BASE reads plane 0 alone
    if (has_b) b = ext_planes<E>(d_b, op == EXT_MUL ? b_stride : 0);
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    const uint64_t blocks = (n + 255) / 256;
    return launch_1d(en.c, E::NAMES.pointwise, ext_pointwise_kernel<E>, (uint32_t)(blocks < 65536 ? blocks : 65536), en.stream, op,
                     ext_planes<E>(d_a, a_stride), b, ext_planes<E>(d_out, out_stride), (uint64_t)n);
}

template <class E>
static int ext_evaluate(const typename E::word *d_coeffs, uint32_t n_cols, size_t col_stride, size_t n_coeffs, const typename E::word *points, uint32_t m,
                        typename E::word *out_values, void *hip_stream, void (*tile_kernel)(ExtEvalArgs<E>)) {
    if (n_cols == 0 || m == 0) return LW_OK;
    if (!points || !out_values) { set_error("null points or values"); return LW_ERR_BAD_ARG; }
    int rc = E::words_check(points, (size_t)m * E::D, "points");
    if (rc) return rc;
    if (n_coeffs == 0) {   // the zero polynomial
        memset(out_values, 0, (size_t)n_cols * m * sizeof(typename E::elem));
        return LW_OK;
    }
    if (n_coeffs > EXT_MAX_LEN) { set_error("%zu coefficients", n_coeffs); return LW_ERR_ALLOC; }
    rc = ext_device_ptrs({d_coeffs});
    if (!rc) rc = ext_stride(col_stride, n_coeffs, "coefficient columns");
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return ext_evaluate_locked<E>(en.c, tile_kernel, d_coeffs, n_cols, col_stride, n_coeffs, points, m, out_values, en.stream);
}

template <class E>
static int ext_deep_quotients(const typename E::word *d_lde, uint32_t n_cols, size_t col_stride, uint32_t log2n, const typename E::word *offset_or_null,
                              uint64_t two_adic_root, const typename E::word *points, uint32_t m, const typename E::word *weights,
                              const typename E::word *evals, typename E::word *d_out, size_t out_stride, void *hip_stream) {
    int rc = E::size_check(log2n);
    if (rc) return rc;
    const size_t n = (size_t)1 << log2n;
    if (n_cols == 0 || m == 0 || !points || !weights || !evals) { set_error("null table, no columns or no points"); return LW_ERR_BAD_ARG; }
    rc = ext_device_ptrs({d_lde, d_out});
    if (!rc) rc = ext_stride(col_stride, n, "LDE columns");
    if (!rc) rc = ext_stride(out_stride, n, "out");
    if (!rc) rc = E::words_check(points, (size_t)m * E::D, "points");
    if (!rc) rc = E::words_check(weights, (size_t)n_cols * m * E::D, "weights");
    if (!rc) rc = E::words_check(evals, (size_t)n_cols * m * E::D, "evals");
    if (rc) return rc;
    if (ext_overlap<E>(d_lde, (size_t)(n_cols - 1) * col_stride + n, d_out, ext_span<E>(out_stride, n))) { set_error("out overlaps the columns"); return LW_ERR_BAD_ARG; }
    for (uint32_t j = 0; j < m; j++) {
        typename E::elem z = ext_elem_of<E>(points, j);
        z.c0 = 0;
        if (E::is_zero(z)) { set_error("point %u lies in the base field: it may be on the domain", j); return LW_ERR_BAD_ARG; }
    }
    typename E::word h;
    rc = E::root_check(two_adic_root);
    if (!rc) rc = E::offset(offset_or_null, h);
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return ext_deep_locked<E>(en.c, d_lde, n_cols, col_stride, log2n, h, E::domain_root(two_adic_root, log2n), points, m, weights, evals, d_out, out_stride,
                              en.stream);
}

// One layer of the FRI commit phase (fri/mod.rs:44-58, 115-141): fold, then, with d_nodes, commit(c, lgb, lgd, h, root,
// stream): evaluate_offset_fft(p', 1, Some(domain_size), offset) of the planes of the block of 2^lgb coefficients on the
// domain of 2^lgd points and the tree over the pairs (e[i], e[i + N/2]), leaf j at i = bitrev(j), digests of digest_bytes.
template <class E, class Commit>
static int ext_fri_layer(const typename E::word *d_coeffs, size_t coeff_stride, size_t n_coeffs, const typename E::word *zeta,
                         const typename E::word *offset_or_null, size_t domain_size, uint64_t two_adic_root, size_t digest_bytes, typename E::word *d_out_poly,
                         typename E::word *d_out_evaluation_or_null, void *d_nodes_or_null, void *out_root_or_null, void *hip_stream, Commit commit) {
    if (n_coeffs == 0) return LW_OK;
    if (n_coeffs > EXT_MAX_LEN) { set_error("%zu coefficients", n_coeffs); return LW_ERR_ALLOC; }
    if (!zeta) { set_error("null zeta"); return LW_ERR_BAD_ARG; }
    int rc = E::words_check(zeta, E::D, "zeta");
    if (!rc) rc = ext_device_ptrs({d_coeffs, d_out_poly});
    if (!rc) rc = ext_stride(coeff_stride, n_coeffs, "coefficients");
    if (rc) return rc;
    const size_t n_out = (n_coeffs + 1) / 2;
    uint32_t lgb = 1;
    while (((size_t)1 << lgb) < n_out) lgb++;
    const size_t padded = (size_t)1 << lgb, in_words = ext_span<E>(coeff_stride, n_coeffs), poly_words = E::D * padded;
    if (ext_overlap<E>(d_out_poly, poly_words, d_coeffs, in_words)) { set_error("d_out_poly overlaps d_coeffs"); return LW_ERR_BAD_ARG; }
    const bool layer = d_nodes_or_null != nullptr;
    if (layer && !d_out_evaluation_or_null) { set_error("a tree needs d_out_evaluation"); return LW_ERR_BAD_ARG; }
    if (!layer && (d_out_evaluation_or_null || out_root_or_null)) { set_error("an evaluation or a root needs d_nodes"); return LW_ERR_BAD_ARG; }
    uint32_t lgd = 0;
    typename E::word h = E::F_ONE;
    if (layer) {
        if (domain_size == 0 || (domain_size & (domain_size - 1))) { set_error("domain size %zu is not a power of two", domain_size); return LW_ERR_INPUT_NOT_POW2; }
        if (padded > domain_size) { set_error("folded block of %zu coefficients exceeds the domain %zu", padded, domain_size); return LW_ERR_BAD_ARG; }
        while (((size_t)1 << lgd) < domain_size) lgd++;
        rc = E::size_check(lgd);
        if (!rc) rc = E::root_check(two_adic_root);
        if (!rc) rc = E::offset(offset_or_null, h);
        if (!rc) rc = ext_device_ptrs({d_out_evaluation_or_null, d_nodes_or_null});
        if (rc) return rc;
        const size_t node_words = (domain_size - 1) * (digest_bytes / sizeof(typename E::word)), eval_words = E::D * domain_size;
        if (ext_overlap<E>(d_out_evaluation_or_null, eval_words, d_coeffs, in_words) || ext_overlap<E>(d_out_evaluation_or_null, eval_words, d_out_poly, poly_words) ||
            ext_overlap<E>(d_nodes_or_null, node_words, d_coeffs, in_words) || ext_overlap<E>(d_nodes_or_null, node_words, d_out_poly, poly_words) ||
            ext_overlap<E>(d_nodes_or_null, node_words, d_out_evaluation_or_null, eval_words)) {
            set_error("the buffers of a layer overlap");
            return LW_ERR_BAD_ARG;
        }
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    rc = launch_1d(en.c, E::NAMES.fri_fold, ext_fri_fold_kernel<E>, blocks_for(padded), en.stream, ext_planes<E>(d_coeffs, coeff_stride),
                   (uint64_t)n_coeffs, ext_elem_of<E>(zeta, 0), ext_planes<E>(d_out_poly, padded), (uint64_t)n_out, (uint64_t)padded);
    if (rc || !layer) return rc;
    rc = commit(en.c, lgb, lgd, h, two_adic_root, en.stream);
    if (rc || !out_root_or_null) return rc;
    return download(out_root_or_null, d_nodes_or_null, digest_bytes, en.stream);
}

}  // namespace lw
