// The BabyBear quartic extension Fp4 = F_p[x] / (x^4 + 11) on the device (arithmetic: babybear_ext.cuh) and the steps a
// STARK prover over BabyBear runs in it after round 1, all on device-resident data:
//   pointwise       mul / sqr / inv / mul_base over vectors: the test seam of the arithmetic and the step between two
//                   transforms of an Fp4 polynomial product
//   convert         LW_LAYOUT_EXT4_INTERLEAVED (4 x u64 per element, R = 2^64) to and from planes
//   evaluate        out-of-domain evaluation of base-field coefficient columns at Fp4 points (round 3)
//   deep_quotients  the DEEP composition polynomial in evaluation form over the LDE domain
//   fri_layer       one layer of the FRI commit phase (fri/mod.rs:44-58, 115-141 with F = BabyBear, E = Fp4): fold,
//                   evaluate on the halved domain, commit pairs of evaluations in a Keccak-256 tree
// A vector of n Fp4 elements is four PLANES of n stored words (LW_LAYOUT_BABYBEAR_U32_R32), c0 then c1 `stride` words later
// and so on: the batch shape of lw_hip_ntt_device and the n_cols / col_stride shape of
// lw_stark_commit_columns_layout_device, so a transform of an Fp4 vector over a base-field domain is the existing transform
// with batch = 4 (the twiddles are in F) and nothing here re-implements a transform or a tree: the layer calls ntt_bb.hip
// through ntt_device_locked and merkle.hip (internal.h).
//
// evaluate: the coefficients are in F, so a work-item does not run Horner in Fp4 (one bb4_mul, 19 base products, per
// coefficient and point).  It multiplies its BE_E consecutive coefficients by the table 1, x, ..., x^(BE_E - 1) of the point,
// which the host hands over as kernel arguments: four base products per coefficient and point, summed in 64 bits two
// products at a time (bb_mac2) and reduced once per coordinate.  The 256 partial sums of a block then fold in LDS under
// x^BE_E, x^2BE_E, ... (bb4_mul), and a second launch of one block per (column, point) folds the tile sums the same way
// under x^BE_TILE.  The coefficients are loaded once for all points of a launch (BE_PTS at most; more points are more
// launches).
//
// deep_quotients is one pass over the columns, no scan.  A work-item owns BD_ROWS consecutive rows of the domain and the
// BD_PTS points of the launch: it accumulates N_j(i) = sum_k w[k][j] col_k[i] (bb4_mul_base: the columns are in F; the
// constant sum_k w[k][j] e[k][j] is the host's), takes x of its first row from one bb_pow and steps by w, and inverts the
// BD_ROWS x BD_PTS norms of x_i - z_j (bb4_norm, in F) with ONE bb_inv (Montgomery's trick over registers); bb4_inv_with
// turns a norm's inverse into 1 / (x_i - z_j).  The norm is never zero: x_i - z_j has a non-zero c1, c2 or c3 (checked).
#include <string.h>
#include <vector>
#include "babybear_ext.cuh"
#include "hash_tree.cuh"

namespace lw {

// ---------------------------------------------------------------- pointwise
struct Bb4Planes {
    const uint32_t *p[4];
};
__device__ __forceinline__ Bb4 bb4_load(const Bb4Planes &v, uint64_t i) { return Bb4{v.p[0][i], v.p[1][i], v.p[2][i], v.p[3][i]}; }

__global__ __launch_bounds__(256) void bb4_pointwise_kernel(int op, const Bb4Planes a, const Bb4Planes b, uint32_t *o0, uint32_t *o1, uint32_t *o2,
                                                            uint32_t *o3, uint64_t n) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const Bb4 x = bb4_load(a, i);
        Bb4 r;
        switch (op) {   // uniform
        case LW_BB4_MUL: r = bb4_mul(x, bb4_load(b, i)); break;
        case LW_BB4_SQR: r = bb4_sqr(x); break;
        case LW_BB4_INV: r = bb4_inv(x); break;
        default: r = bb4_mul_base(x, b.p[0][i]); break;   // LW_BB4_MUL_BASE
        }
        o0[i] = r.c0;
        o1[i] = r.c1;
        o2[i] = r.c2;
        o3[i] = r.c3;
    }
}

// ---------------------------------------------------------------- convert
// element i of the interleaved form: the four u64 words 4 i .. 4 i + 3, each a 2^64 mod p
__global__ __launch_bounds__(256) void bb4_to_planes_kernel(const uint64_t *in, uint32_t *out, uint64_t stride, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int e = 0; e < 4; e++) out[e * stride + i] = bb_from_r64(in[4 * i + e]);
}
__global__ __launch_bounds__(256) void bb4_to_interleaved_kernel(const uint32_t *in, uint64_t stride, uint64_t *out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int e = 0; e < 4; e++) out[4 * i + e] = bb_to_r64(in[e * stride + i]);
}

// ---------------------------------------------------------------- evaluate
constexpr int BE_THREADS = 256;
constexpr int BE_E = 8;                                          // consecutive coefficients per work-item
constexpr uint64_t BE_TILE = (uint64_t)BE_THREADS * BE_E;        // 2048 coefficients per block
constexpr int BE_PTS = 4;                                        // points per launch
constexpr int BE_STEPS = 8;                                      // log2(BE_THREADS) steps of the block fold

struct Bb4EvalArgs {
    const uint32_t *cols;
    uint64_t col_stride, n, ntiles;
    uint32_t k0;               // first column of this launch
    uint32_t m, m_total, j0;   // points of this launch, of the call, and the first of this launch
    uint32_t group;            // fold: tiles per work-item
    Bb4 *sums;                 // [n_cols][BE_PTS][ntiles]
    Bb4 *vals;                 // [n_cols][m_total]
    Bb4 xp[BE_PTS][BE_E];      // x^e, e < BE_E
    Bb4 pe[BE_PTS][BE_STEPS];  // x^(BE_E 2^s)
    Bb4 xt[BE_PTS];            // x^BE_TILE
    Bb4 pg[BE_PTS][BE_STEPS];  // x^(BE_TILE group 2^s)
};

// sum_r w^r v_r over the block's 256 work-items, pw[s] = w^(2^s): the result is work-item 0's.  At step s the work-items
// whose index is a multiple of 2^(s+1) take in the one 2^s above, which was active in the step before.
__device__ __forceinline__ Bb4 bb4_block_fold(Bb4 v, Bb4 *lds, const Bb4 *pw) {
    const int r = threadIdx.x;
#pragma unroll 1
    for (int s = 0; s < BE_STEPS; s++) {
        lds[r] = v;
        __syncthreads();
        const int d = 1 << s;
        if ((r & (2 * d - 1)) == 0) v = bb4_add(v, bb4_mul(pw[s], lds[r + d]));   // r + d <= 255
        __syncthreads();
    }
    return v;
}

// tile sums: S[k][j][t] = sum_{i in tile t} col_k[i] x_j^(i - t BE_TILE)
__global__ __launch_bounds__(BE_THREADS) void bb4_eval_tile_kernel(const Bb4EvalArgs a) {
    __shared__ Bb4 lds[BE_THREADS];
    const uint32_t k = a.k0 + blockIdx.y;
    const uint64_t t = blockIdx.x;
    const uint32_t *col = a.cols + (uint64_t)k * a.col_stride;
    const uint64_t base = t * BE_TILE + (uint64_t)threadIdx.x * BE_E;
    uint32_t c[BE_E];
#pragma unroll
    for (int e = 0; e < BE_E; e++) c[e] = base + e < a.n ? col[base + e] : 0;
#pragma unroll 1
    for (uint32_t j = 0; j < a.m; j++) {
        const Bb4 *xp = a.xp[j];   // uniform
        // every coordinate: BE_E products of canonical words, two at a time onto a sum kept below p 2^32 (bb_mac2)
        uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
        for (int e = 0; e < BE_E; e += 2) {
            s0 = bb_mac2(s0, c[e], xp[e].c0, c[e + 1], xp[e + 1].c0);
            s1 = bb_mac2(s1, c[e], xp[e].c1, c[e + 1], xp[e + 1].c1);
            s2 = bb_mac2(s2, c[e], xp[e].c2, c[e + 1], xp[e + 1].c2);
            s3 = bb_mac2(s3, c[e], xp[e].c3, c[e + 1], xp[e + 1].c3);
        }
        Bb4 h{bb_reduce(s0), bb_reduce(s1), bb_reduce(s2), bb_reduce(s3)};
        h = bb4_block_fold(h, lds, a.pe[j]);
        if (threadIdx.x == 0) a.sums[((uint64_t)k * BE_PTS + j) * a.ntiles + t] = h;
    }
}

// one block per (column, point): the value sum_t S[t] x^(t BE_TILE).  A work-item folds `group` consecutive tile sums.
__global__ __launch_bounds__(BE_THREADS) void bb4_eval_fold_kernel(const Bb4EvalArgs a) {
    __shared__ Bb4 lds[BE_THREADS];
    const uint32_t k = a.k0 + blockIdx.x / a.m, j = blockIdx.x % a.m;
    const Bb4 *s = a.sums + ((uint64_t)k * BE_PTS + j) * a.ntiles;
    const uint64_t first = (uint64_t)threadIdx.x * a.group;
    const Bb4 xt = a.xt[j];
    Bb4 v = bb4_zero();
    for (uint32_t g = a.group; g-- > 0;)
        if (first + g < a.ntiles) v = bb4_add(bb4_mul(v, xt), s[first + g]);
    v = bb4_block_fold(v, lds, a.pg[j]);
    if (threadIdx.x == 0) a.vals[(uint64_t)k * a.m_total + a.j0 + j] = v;
}

// ---------------------------------------------------------------- DEEP quotients
constexpr int BD_THREADS = 256;
constexpr int BD_ROWS = 4;   // rows per work-item: BD_ROWS x BD_PTS norms share one inversion.  Not measured against 2 or 8.
constexpr int BD_PTS = 4;    // points per launch

struct Bb4DeepArgs {
    const uint32_t *cols;
    uint64_t col_stride;
    uint32_t n_cols, log2n, accumulate;
    uint32_t h, w;          // x_i = h w^i
    const Bb4 *wt;          // [n_cols][BD_PTS]: the weights of this launch's points
    Bb4 nz[BD_PTS];         // -z_j: x_i - z_j = (x_i + nz.c0, nz.c1, nz.c2, nz.c3)
    Bb4 c[BD_PTS];          // sum_k w[k][j] e[k][j]
    uint32_t *out;
    uint64_t out_stride;
};

// Steps Q, Q - 1, ..., 0 of the way back through Montgomery's trick, (row, point) = (Q / M, Q % M): 1 / norm from the
// running inverse, 1 / (x - z) from it, the quotient onto the row's sum.  A recursion over the template argument and not a
// loop: the body is long enough that a 16-step loop is left partly rolled, and acc[][] indexed by a loop counter lives in
// scratch (272 bytes per lane at M = 4).  b0 and b2 of the norm are computed again rather than kept from the way forward
// (32 more live words at M = 4; not measured against keeping them).
template <int Q, int M>
__device__ __forceinline__ void bb4_deep_back(const Bb4DeepArgs &a, const uint32_t (&x)[BD_ROWS], const uint32_t (&nr)[BD_ROWS][M],
                                              const uint32_t (&pre)[BD_ROWS][M], const Bb4 (&acc)[BD_ROWS][M], uint32_t inv, Bb4 (&sum)[BD_ROWS]) {
    constexpr int r = Q / M, j = Q % M;
    const uint32_t ninv = bb_mul(inv, pre[r][j]);
    const Bb4 d{bb_add(x[r], a.nz[j].c0), a.nz[j].c1, a.nz[j].c2, a.nz[j].c3};
    uint32_t b0, b2;
    bb4_norm(d, b0, b2);
    const Bb4 q = bb4_mul(bb4_sub(acc[r][j], a.c[j]), bb4_inv_with(d, b0, b2, ninv));
    sum[r] = j == M - 1 ? q : bb4_add(sum[r], q);
    if constexpr (Q > 0) bb4_deep_back<Q - 1, M>(a, x, nr, pre, acc, bb_mul(inv, nr[r][j]), sum);
}

template <int M> __global__ __launch_bounds__(BD_THREADS) void bb4_deep_kernel(const Bb4DeepArgs a) {
    const uint64_t n = 1ull << a.log2n;
    const uint64_t row0 = ((uint64_t)blockIdx.x * BD_THREADS + threadIdx.x) * BD_ROWS;
    if (row0 >= n) return;
    Bb4 acc[BD_ROWS][M];
#pragma unroll
    for (int r = 0; r < BD_ROWS; r++)
#pragma unroll
        for (int j = 0; j < M; j++) acc[r][j] = bb4_zero();
#pragma unroll 1
    for (uint32_t k = 0; k < a.n_cols; k++) {
        const uint32_t *col = a.cols + (uint64_t)k * a.col_stride + row0;
        uint32_t v[BD_ROWS];
#pragma unroll
        for (int r = 0; r < BD_ROWS; r++) v[r] = row0 + r < n ? col[r] : 0;   // n < BD_ROWS: the rows past the domain
#pragma unroll
        for (int j = 0; j < M; j++) {
            const Bb4 w = a.wt[(uint64_t)k * BD_PTS + j];   // uniform
            if (bb4_is_zero(w)) continue;                   // a zero weight skips the pair
#pragma unroll
            for (int r = 0; r < BD_ROWS; r++) acc[r][j] = bb4_add(acc[r][j], bb4_mul_base(w, v[r]));
        }
    }
    // the norms of x_i - z_j and their running products
    uint32_t x[BD_ROWS], nr[BD_ROWS][M], pre[BD_ROWS][M];
    x[0] = bb_mul(a.h, bb_pow(a.w, row0));
#pragma unroll
    for (int r = 1; r < BD_ROWS; r++) x[r] = bb_mul(x[r - 1], a.w);
    uint32_t run = BabyBear::ONE;
#pragma unroll
    for (int r = 0; r < BD_ROWS; r++)
#pragma unroll
        for (int j = 0; j < M; j++) {
            const Bb4 d{bb_add(x[r], a.nz[j].c0), a.nz[j].c1, a.nz[j].c2, a.nz[j].c3};
            uint32_t b0, b2;
            nr[r][j] = bb4_norm(d, b0, b2);
            pre[r][j] = run;
            run = bb_mul(run, nr[r][j]);
        }
    uint32_t inv = bb_inv(run);   // run != 0: every norm is non-zero
    Bb4 sum[BD_ROWS];
    bb4_deep_back<BD_ROWS * M - 1, M>(a, x, nr, pre, acc, inv, sum);
#pragma unroll
    for (int r = 0; r < BD_ROWS; r++) {
        if (row0 + r >= n) break;
        uint32_t *o = a.out + row0 + r;
        Bb4 v = sum[r];
        if (a.accumulate) v = bb4_add(v, Bb4{o[0], o[a.out_stride], o[2 * a.out_stride], o[3 * a.out_stride]});   // canonical: an earlier launch wrote them
        o[0] = v.c0;
        o[a.out_stride] = v.c1;
        o[2 * a.out_stride] = v.c2;
        o[3 * a.out_stride] = v.c3;
    }
}

// ---------------------------------------------------------------- FRI fold
// out[i] = 2 (c[2i] + zeta c[2i+1]) for i < n_out, the odd term absent past n; zeros up to `padded`, the planes' stride
__global__ __launch_bounds__(256) void bb4_fri_fold_kernel(const Bb4Planes c, uint64_t n, Bb4 zeta, uint32_t *out, uint64_t n_out, uint64_t padded) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= padded) return;
    Bb4 r = bb4_zero();
    if (i < n_out) {
        r = bb4_load(c, 2 * i);
        if (2 * i + 1 < n) r = bb4_add(r, bb4_mul(zeta, bb4_load(c, 2 * i + 1)));
        r = bb4_add(r, r);
    }
    out[i] = r.c0;
    out[padded + i] = r.c1;
    out[2 * padded + i] = r.c2;
    out[3 * padded + i] = r.c3;
}

// ---------------------------------------------------------------- host
static constexpr uint64_t BB4_MAX_LEN = (uint64_t)1 << 36;   // the grids' block indices stay below 2^31

static bool bb4_overlap(const void *a, size_t a_words, const void *b, size_t b_words) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + 4 * b_words && b0 < a0 + 4 * a_words;
}
// a vector of n elements in planes `stride` words apart (0: n; below n: an error)
static int bb4_stride(size_t &stride, size_t n, const char *what) {
    if (stride == 0) stride = n;
    if (stride < n) { set_error("%s: plane stride %zu below the length %zu", what, stride, n); return LW_ERR_BAD_ARG; }
    return LW_OK;
}
static int bb4_device_ptrs(std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs) {
        if (!p) { set_error("null buffer"); return LW_ERR_BAD_ARG; }
        if (!aligned16(p)) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    }
    return LW_OK;
}
// `count` host scalars of four stored words each, every word below p
static int bb4_scalars(const uint32_t *words, size_t count, const char *what) {
    for (size_t i = 0; i < 4 * count; i++)
        if (words[i] >= BabyBear::P) { set_error("%s: word %zu is not below p", what, i); return LW_ERR_BAD_ARG; }
    return LW_OK;
}
static int bb4_offset(const uint32_t *offset_or_null, uint32_t &h) {
    h = offset_or_null ? *offset_or_null : BabyBear::ONE;
    if (h >= BabyBear::P) { set_error("coset offset is not below p"); return LW_ERR_BAD_ARG; }
    if (h == 0) { set_error("coset offset is zero"); return LW_ERR_INV_ZERO; }
    return LW_OK;
}
static int bb4_size_check(uint32_t log2n) {
    if (log2n > BabyBear::TWO_ADICITY) { set_error("BabyBear has no root of unity of order 2^%u", log2n); return LW_ERR_ROOT_OF_UNITY; }
    return LW_OK;
}
static Bb4 bb4_elem(const uint32_t *tab, size_t i) { return Bb4{tab[4 * i], tab[4 * i + 1], tab[4 * i + 2], tab[4 * i + 3]}; }

static int bb4_evaluate_locked(Context &c, const uint32_t *d_coeffs, uint32_t n_cols, uint64_t col_stride, uint64_t n, const uint32_t *points,
                               uint32_t m, uint32_t *out_values, hipStream_t s) {
    const uint64_t nt = (n + BE_TILE - 1) / BE_TILE;
    const size_t sums_b = ((size_t)n_cols * BE_PTS * nt * sizeof(Bb4) + 255) & ~(size_t)255;
    if (c.poly_ws.ensure(sums_b + (size_t)n_cols * m * sizeof(Bb4))) return LW_ERR_ALLOC;
    Bb4EvalArgs a;
    memset(&a, 0, sizeof(a));
    a.cols = d_coeffs;
    a.col_stride = col_stride;
    a.n = n;
    a.ntiles = nt;
    a.m_total = m;
    a.group = (uint32_t)((nt + BE_THREADS - 1) / BE_THREADS);
    a.sums = (Bb4 *)c.poly_ws.p;
    a.vals = (Bb4 *)((char *)c.poly_ws.p + sums_b);
    for (uint32_t j0 = 0; j0 < m; j0 += BE_PTS) {
        a.j0 = j0;
        a.m = m - j0 < (uint32_t)BE_PTS ? m - j0 : (uint32_t)BE_PTS;
        for (uint32_t j = 0; j < a.m; j++) {
            const Bb4 x = bb4_elem(points, j0 + j);
            a.xp[j][0] = Bb4{BabyBear::ONE, 0, 0, 0};
            for (int e = 1; e < BE_E; e++) a.xp[j][e] = bb4_mul(a.xp[j][e - 1], x);
            a.pe[j][0] = bb4_mul(a.xp[j][BE_E - 1], x);
            for (int st = 1; st < BE_STEPS; st++) a.pe[j][st] = bb4_sqr(a.pe[j][st - 1]);
            a.xt[j] = bb4_sqr(a.pe[j][BE_STEPS - 1]);   // x^(BE_E 2^BE_STEPS) = x^BE_TILE
            a.pg[j][0] = bb4_pow(a.xt[j], a.group);
            for (int st = 1; st < BE_STEPS; st++) a.pg[j][st] = bb4_sqr(a.pg[j][st - 1]);
        }
        for (uint32_t k0 = 0; k0 < n_cols; k0 += 65535) {   // the grid's y extent
            const uint32_t kc = n_cols - k0 < 65535 ? n_cols - k0 : 65535;
            a.k0 = k0;
            hipEvent_t pe = c.prof_begin(s);
            hipLaunchKernelGGL(bb4_eval_tile_kernel, dim3((uint32_t)nt, kc), dim3(BE_THREADS), 0, s, a);
            c.prof_end("bb4_eval_tile_kernel", pe, s);
            pe = c.prof_begin(s);
            hipLaunchKernelGGL(bb4_eval_fold_kernel, dim3(kc * a.m), dim3(BE_THREADS), 0, s, a);
            c.prof_end("bb4_eval_fold_kernel", pe, s);
            LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
        }
    }
    return download(out_values, a.vals, (size_t)n_cols * m * sizeof(Bb4), s);
}

static int bb4_deep_locked(Context &c, const uint32_t *d_lde, uint32_t n_cols, uint64_t col_stride, uint32_t log2n, uint32_t h, const uint32_t *points,
                           uint32_t m, const uint32_t *weights, const uint32_t *evals, uint32_t *d_out, uint64_t out_stride, hipStream_t s) {
    const uint32_t groups = (m + BD_PTS - 1) / BD_PTS;
    const size_t group_b = (size_t)n_cols * BD_PTS * sizeof(Bb4), tables = group_b * groups;
    if (c.poly_ws.ensure(tables)) return LW_ERR_ALLOC;
    int rc = deep_pin(c, tables);
    if (rc) return rc;
    Bb4 *hw = (Bb4 *)c.deep_pin;
    memset(hw, 0, tables);
    for (uint32_t k = 0; k < n_cols; k++)
        for (uint32_t j = 0; j < m; j++) hw[((size_t)(j / BD_PTS) * n_cols + k) * BD_PTS + j % BD_PTS] = bb4_elem(weights, (size_t)k * m + j);
    LW_HIP_CHECK(hipMemcpyAsync(c.poly_ws.p, hw, tables, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipEventRecord(c.deep_pin_read, s), LW_ERR_LAUNCH);
    Bb4DeepArgs a;
    memset(&a, 0, sizeof(a));
    a.cols = d_lde;
    a.col_stride = col_stride;
    a.n_cols = n_cols;
    a.log2n = log2n;
    a.h = h;
    a.w = ntt_bb_root(log2n, false);
    a.out = d_out;
    a.out_stride = out_stride;
    const uint64_t rows = 1ull << log2n, items = (rows + BD_ROWS - 1) / BD_ROWS;
    for (uint32_t g = 0; g < groups; g++) {
        const uint32_t j0 = g * BD_PTS, mp = m - j0 < (uint32_t)BD_PTS ? m - j0 : (uint32_t)BD_PTS;
        a.wt = (const Bb4 *)((const char *)c.poly_ws.p + group_b * g);
        a.accumulate = g > 0;
        for (uint32_t j = 0; j < mp; j++) {
            a.nz[j] = bb4_neg(bb4_elem(points, j0 + j));
            Bb4 cj = bb4_zero();
            for (uint32_t k = 0; k < n_cols; k++) cj = bb4_add(cj, bb4_mul(bb4_elem(weights, (size_t)k * m + j0 + j), bb4_elem(evals, (size_t)k * m + j0 + j)));
            a.c[j] = cj;
        }
        void (*kernel)(Bb4DeepArgs) = mp == 1 ? bb4_deep_kernel<1> : mp == 2 ? bb4_deep_kernel<2> : mp == 3 ? bb4_deep_kernel<3> : bb4_deep_kernel<4>;
        rc = launch_1d(c, "bb4_deep_kernel", kernel, blocks_for(items), s, a);
        if (rc) return rc;
    }
    return LW_OK;
}

}  // namespace lw

using namespace lw;

extern "C" {

int lw_babybear_ext4_pointwise_device(lw_bb4_op_t op, const uint32_t *d_a, size_t a_stride, const uint32_t *d_b, size_t b_stride, uint32_t *d_out,
                                      size_t out_stride, size_t n, void *hip_stream) {
    if (op != LW_BB4_MUL && op != LW_BB4_SQR && op != LW_BB4_INV && op != LW_BB4_MUL_BASE) { set_error("bad Fp4 op %d", (int)op); return LW_ERR_BAD_ARG; }
    if (n == 0) return LW_OK;
    if (n > BB4_MAX_LEN) { set_error("%zu Fp4 elements", n); return LW_ERR_ALLOC; }
    const bool has_b = op == LW_BB4_MUL || op == LW_BB4_MUL_BASE;
    int rc = has_b ? bb4_device_ptrs({d_a, d_b, d_out}) : bb4_device_ptrs({d_a, d_out});
    if (!rc) rc = bb4_stride(a_stride, n, "a");
    if (!rc) rc = bb4_stride(out_stride, n, "out");
    if (!rc && op == LW_BB4_MUL) rc = bb4_stride(b_stride, n, "b");
    if (rc) return rc;
    // The output may BE an operand, the whole vector under the same stride (work-item i reads element i of everything
    // before it writes element i); any other overlap of a plane of the output with a plane of an operand is refused.
    Bb4Planes a, b;
    memset(&b, 0, sizeof(b));
    for (int e = 0; e < 4; e++) a.p[e] = d_a + e * a_stride;
    if (has_b) b.p[0] = d_b;
    if (op == LW_BB4_MUL)
        for (int e = 1; e < 4; e++) b.p[e] = d_b + e * b_stride;
    const bool out_is_a = d_out == d_a && out_stride == a_stride, out_is_b = op == LW_BB4_MUL && d_out == d_b && out_stride == b_stride;
    for (int o = 0; o < 4; o++)
        for (int e = 0; e < 4; e++)
            if ((!out_is_a && bb4_overlap(d_out + o * out_stride, n, a.p[e], n)) || (!out_is_b && b.p[e] && bb4_overlap(d_out + o * out_stride, n, b.p[e], n))) {
                set_error("out overlaps an operand without being the same vector under the same stride");
                return LW_ERR_BAD_ARG;
            }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    const uint64_t blocks = (n + 255) / 256;
    return launch_1d(en.c, "bb4_pointwise_kernel", bb4_pointwise_kernel, (uint32_t)(blocks < 65536 ? blocks : 65536), en.stream, (int)op, a, b, d_out,
                     d_out + out_stride, d_out + 2 * out_stride, d_out + 3 * out_stride, (uint64_t)n);
}

int lw_babybear_ext4_convert_device(lw_bb4_convert_t dir, uint64_t *d_interleaved, uint32_t *d_planes, size_t plane_stride, size_t n, void *hip_stream) {
    if (dir != LW_BB4_TO_PLANES && dir != LW_BB4_TO_INTERLEAVED) { set_error("bad conversion %d", (int)dir); return LW_ERR_BAD_ARG; }
    if (n == 0) return LW_OK;
    if (n > BB4_MAX_LEN) { set_error("%zu Fp4 elements", n); return LW_ERR_ALLOC; }
    int rc = bb4_device_ptrs({d_interleaved, d_planes});
    if (!rc) rc = bb4_stride(plane_stride, n, "planes");
    if (rc) return rc;
    if (bb4_overlap(d_interleaved, 8 * n, d_planes, 3 * plane_stride + n)) { set_error("the two forms overlap"); return LW_ERR_BAD_ARG; }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    if (dir == LW_BB4_TO_PLANES)
        return launch_1d(en.c, "bb4_to_planes_kernel", bb4_to_planes_kernel, blocks_for(n), en.stream, (const uint64_t *)d_interleaved, d_planes,
                         (uint64_t)plane_stride, (uint64_t)n);
    return launch_1d(en.c, "bb4_to_interleaved_kernel", bb4_to_interleaved_kernel, blocks_for(n), en.stream, (const uint32_t *)d_planes, (uint64_t)plane_stride,
                     d_interleaved, (uint64_t)n);
}

int lw_babybear_ext4_evaluate_device(const uint32_t *d_coeffs, uint32_t n_cols, size_t col_stride, size_t n_coeffs, const uint32_t *points, uint32_t m,
                                     uint32_t *out_values, void *hip_stream) {
    if (n_cols == 0 || m == 0) return LW_OK;
    if (!points || !out_values) { set_error("null points or values"); return LW_ERR_BAD_ARG; }
    int rc = bb4_scalars(points, m, "points");
    if (rc) return rc;
    if (n_coeffs == 0) {   // the zero polynomial
        memset(out_values, 0, (size_t)n_cols * m * 16);
        return LW_OK;
    }
    if (n_coeffs > BB4_MAX_LEN) { set_error("%zu coefficients", n_coeffs); return LW_ERR_ALLOC; }
    rc = bb4_device_ptrs({d_coeffs});
    if (!rc) rc = bb4_stride(col_stride, n_coeffs, "coefficient columns");
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return bb4_evaluate_locked(en.c, d_coeffs, n_cols, col_stride, n_coeffs, points, m, out_values, en.stream);
}

int lw_babybear_ext4_deep_quotients_device(const uint32_t *d_lde, uint32_t n_cols, size_t col_stride, uint32_t log2n, const uint32_t *offset_or_null,
                                           const uint32_t *points, uint32_t m, const uint32_t *weights, const uint32_t *evals, uint32_t *d_out,
                                           size_t out_stride, void *hip_stream) {
    int rc = bb4_size_check(log2n);
    if (rc) return rc;
    const size_t n = (size_t)1 << log2n;
    if (n_cols == 0 || m == 0 || !points || !weights || !evals) { set_error("null table, no columns or no points"); return LW_ERR_BAD_ARG; }
    rc = bb4_device_ptrs({d_lde, d_out});
    if (!rc) rc = bb4_stride(col_stride, n, "LDE columns");
    if (!rc) rc = bb4_stride(out_stride, n, "out");
    if (!rc) rc = bb4_scalars(points, m, "points");
    if (!rc) rc = bb4_scalars(weights, (size_t)n_cols * m, "weights");
    if (!rc) rc = bb4_scalars(evals, (size_t)n_cols * m, "evals");
    if (rc) return rc;
    if (bb4_overlap(d_lde, (size_t)(n_cols - 1) * col_stride + n, d_out, 3 * out_stride + n)) { set_error("out overlaps the columns"); return LW_ERR_BAD_ARG; }
    for (uint32_t j = 0; j < m; j++)
        if ((points[4 * (size_t)j + 1] | points[4 * (size_t)j + 2] | points[4 * (size_t)j + 3]) == 0) {
            set_error("point %u lies in the base field (c1 = c2 = c3 = 0): it may be on the domain", j);
            return LW_ERR_BAD_ARG;
        }
    uint32_t h;
    rc = bb4_offset(offset_or_null, h);
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return bb4_deep_locked(en.c, d_lde, n_cols, col_stride, log2n, h, points, m, weights, evals, d_out, out_stride, en.stream);
}

int lw_babybear_ext4_fri_layer_device(const uint32_t *d_coeffs, size_t coeff_stride, size_t n_coeffs, const uint32_t *zeta, const uint32_t *offset_or_null,
                                      size_t domain_size, uint32_t *d_out_poly, uint32_t *d_out_evaluation_or_null, uint8_t *d_nodes_or_null,
                                      uint8_t *out_root_or_null, void *hip_stream) {
    if (n_coeffs == 0) return LW_OK;
    if (n_coeffs > BB4_MAX_LEN) { set_error("%zu coefficients", n_coeffs); return LW_ERR_ALLOC; }
    if (!zeta) { set_error("null zeta"); return LW_ERR_BAD_ARG; }
    int rc = bb4_scalars(zeta, 1, "zeta");
    if (!rc) rc = bb4_device_ptrs({d_coeffs, d_out_poly});
    if (!rc) rc = bb4_stride(coeff_stride, n_coeffs, "coefficients");
    if (rc) return rc;
    const size_t n_out = (n_coeffs + 1) / 2;
    uint32_t lgb = 1;
    while (((size_t)1 << lgb) < n_out) lgb++;
    const size_t padded = (size_t)1 << lgb, in_words = 3 * coeff_stride + n_coeffs;
    if (bb4_overlap(d_out_poly, 4 * padded, d_coeffs, in_words)) { set_error("d_out_poly overlaps d_coeffs"); return LW_ERR_BAD_ARG; }
    const bool layer = d_nodes_or_null != nullptr;
    if (layer && !d_out_evaluation_or_null) { set_error("a tree needs d_out_evaluation"); return LW_ERR_BAD_ARG; }
    if (!layer && (d_out_evaluation_or_null || out_root_or_null)) { set_error("an evaluation or a root needs d_nodes"); return LW_ERR_BAD_ARG; }
    uint32_t lgd = 0, h = BabyBear::ONE;
    if (layer) {
        if (domain_size == 0 || (domain_size & (domain_size - 1))) { set_error("domain size %zu is not a power of two", domain_size); return LW_ERR_INPUT_NOT_POW2; }
        if (padded > domain_size) { set_error("folded block of %zu coefficients exceeds the domain %zu", padded, domain_size); return LW_ERR_BAD_ARG; }
        while (((size_t)1 << lgd) < domain_size) lgd++;
        rc = bb4_size_check(lgd);
        if (!rc) rc = bb4_offset(offset_or_null, h);
        if (!rc) rc = bb4_device_ptrs({d_out_evaluation_or_null, d_nodes_or_null});
        if (rc) return rc;
        const size_t node_words = (domain_size - 1) * 8;
        if (bb4_overlap(d_out_evaluation_or_null, 4 * domain_size, d_coeffs, in_words) || bb4_overlap(d_out_evaluation_or_null, 4 * domain_size, d_out_poly, 4 * padded) ||
            bb4_overlap(d_nodes_or_null, node_words, d_coeffs, in_words) || bb4_overlap(d_nodes_or_null, node_words, d_out_poly, 4 * padded) ||
            bb4_overlap(d_nodes_or_null, node_words, d_out_evaluation_or_null, 4 * domain_size)) {
            set_error("the buffers of a layer overlap");
            return LW_ERR_BAD_ARG;
        }
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    Bb4Planes in;
    for (int e = 0; e < 4; e++) in.p[e] = d_coeffs + e * coeff_stride;
    rc = launch_1d(c, "bb4_fri_fold_kernel", bb4_fri_fold_kernel, blocks_for(padded), en.stream, in, (uint64_t)n_coeffs, bb4_elem(zeta, 0), d_out_poly,
                   (uint64_t)n_out, (uint64_t)padded);
    if (rc || !layer) return rc;
    // evaluate_offset_fft(p', 1, Some(domain_size), offset) of the four planes, then the tree over the pairs (e[i], e[i + N/2]):
    // two rows of four parts per leaf, leaf j at i = bitrev(j)
    rc = ntt_device_locked(c, LW_FIELD_BABYBEAR, LW_LAYOUT_BABYBEAR_U32_R32, LW_DIR_FORWARD, d_out_poly, d_out_evaluation_or_null, lgd, 4, 0, offset_or_null,
                           en.stream, lgb);
    if (!rc) rc = merkle_commit_device(c, d_out_evaluation_or_null, 8, domain_size, lgd - 1, 1, d_nodes_or_null, en.stream, 4, 2);
    if (rc || !out_root_or_null) return rc;
    return download(out_root_or_null, d_nodes_or_null, 32, en.stream);
}

}  // extern "C"
