// The Goldilocks quadratic extension Fp2 = F_p[t] / (t^2 - 7) on the device (arithmetic: goldilocks_ext.cuh) and the three
// steps a STARK prover over Goldilocks runs in it after round 1, all on device-resident data:
//   pointwise       mul / sqr / inv / mul_base over vectors: the test seam of the arithmetic and the step between two
//                   transforms of an Fp2 polynomial product
//   evaluate        out-of-domain evaluation of base-field coefficient columns at Fp2 points (round 3)
//   deep_quotients  the DEEP composition polynomial in evaluation form over the LDE domain
//   fri_layer       one layer of the FRI commit phase (fri/mod.rs:44-58, 115-141 with F = Goldilocks, E = Fp2): fold,
//                   evaluate on the halved domain, commit pairs of evaluations in an RPO tree
// A vector of n Fp2 elements is two PLANES of n words, c0 then c1 `stride` words later: the batch / batch_stride shape of
// lw_goldilocks_ntt_device and the n_cols / col_stride shape of lw_rpo_commit_columns_device, so a transform of an Fp2
// vector over a base-field domain is the existing transform with batch = 2 (the twiddles are in F) and nothing here
// re-implements a transform or a tree: the layer calls goldilocks.hip and rpo.hip (internal.h).
//
// evaluate is shaped as poly.hip's: every work-item runs Horner over GE_E consecutive coefficients (acc = acc x + c: one
// gl2_mul and one gl_add), the 256 partial sums of a block fold in LDS under x^GE_E, x^2GE_E, ..., and a second launch of
// one block per (column, point) folds the tile sums the same way under x^GE_TILE.  The coefficients are loaded once for
// all points of a launch (GE_PTS at most; more points are more launches).  The power tables come from the host as kernel
// arguments.
//
// deep_quotients is one pass over the columns, no scan.  A work-item owns GD_ROWS consecutive rows of the domain and the
// GD_PTS points of the launch: it accumulates N_j(i) = sum_k w[k][j] col_k[i] (gl2_mul_base: the columns are in F; the
// constant sum_k w[k][j] e[k][j] is the host's), takes x of its first row from one gl_pow and steps by w, and inverts all
// its GD_ROWS x GD_PTS norms (x_i - z0)^2 - 7 z1^2 with ONE gl_inv (Montgomery's trick over registers): 1 / (x - z) =
// (x - z0 + z1 t) / norm.  The norm is never zero: z1 != 0 is checked and 7 is a non-residue.
#include <string.h>
#include <vector>
#include "goldilocks_ext.cuh"
#include "hash_tree.cuh"

namespace lw {

// ---------------------------------------------------------------- pointwise
__global__ __launch_bounds__(256) void gl2_pointwise_kernel(int op, const uint64_t *a0, const uint64_t *a1, const uint64_t *b0, const uint64_t *b1,
                                                            uint64_t *o0, uint64_t *o1, uint64_t n) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const Gl2 a = gl2_from_words(a0[i], a1[i]);
        Gl2 r;
        switch (op) {   // uniform
        case LW_GL2_MUL: r = gl2_mul(a, gl2_from_words(b0[i], b1[i])); break;
        case LW_GL2_SQR: r = gl2_sqr(a); break;
        case LW_GL2_INV: r = gl2_inv(a); break;
        default: r = gl2_mul_base(a, gl_from_word(b0[i])); break;   // LW_GL2_MUL_BASE
        }
        o0[i] = r.c0;
        o1[i] = r.c1;
    }
}

// ---------------------------------------------------------------- evaluate
constexpr int GE_THREADS = 256;
constexpr int GE_E = 8;                                          // consecutive coefficients per work-item
constexpr uint64_t GE_TILE = (uint64_t)GE_THREADS * GE_E;        // 2048 coefficients per block
constexpr int GE_PTS = 4;                                        // points per launch
constexpr int GE_STEPS = 8;                                      // log2(GE_THREADS) steps of the block fold

struct Gl2EvalArgs {
    const uint64_t *cols;
    uint64_t col_stride, n, ntiles;
    uint32_t k0;               // first column of this launch
    uint32_t m, m_total, j0;   // points of this launch, of the call, and the first of this launch
    uint32_t group;            // fold: tiles per work-item
    Gl2 *sums;                 // [n_cols][GE_PTS][ntiles]
    Gl2 *vals;                 // [n_cols][m_total]
    Gl2 x[GE_PTS];             // the points
    Gl2 pe[GE_PTS][GE_STEPS];  // x^(GE_E 2^s)
    Gl2 xt[GE_PTS];            // x^GE_TILE
    Gl2 pg[GE_PTS][GE_STEPS];  // x^(GE_TILE group 2^s)
};

// sum_r w^r v_r over the block's 256 work-items, pw[s] = w^(2^s): the result is work-item 0's.  At step s the work-items
// whose index is a multiple of 2^(s+1) take in the one 2^s above, which was active in the step before.
__device__ __forceinline__ Gl2 gl2_block_fold(Gl2 v, Gl2 *lds, const Gl2 *pw) {
    const int r = threadIdx.x;
#pragma unroll 1
    for (int s = 0; s < GE_STEPS; s++) {
        lds[r] = v;
        __syncthreads();
        const int d = 1 << s;
        if ((r & (2 * d - 1)) == 0) v = gl2_add(v, gl2_mul(pw[s], lds[r + d]));   // r + d <= 255
        __syncthreads();
    }
    return v;
}

// tile sums: S[k][j][t] = sum_{i in tile t} col_k[i] x_j^(i - t GE_TILE)
__global__ __launch_bounds__(GE_THREADS) void gl2_eval_tile_kernel(const Gl2EvalArgs a) {
    __shared__ Gl2 lds[GE_THREADS];
    const uint32_t k = a.k0 + blockIdx.y;
    const uint64_t t = blockIdx.x;
    const uint64_t *col = a.cols + (uint64_t)k * a.col_stride;
    const uint64_t base = t * GE_TILE + (uint64_t)threadIdx.x * GE_E;
    uint64_t c[GE_E];
#pragma unroll
    for (int e = 0; e < GE_E; e++) c[e] = base + e < a.n ? gl_from_word(col[base + e]) : 0;
#pragma unroll 1
    for (uint32_t j = 0; j < a.m; j++) {
        const Gl2 x = a.x[j];
        Gl2 h{c[GE_E - 1], 0};
#pragma unroll
        for (int e = GE_E - 2; e >= 0; e--) {
            h = gl2_mul(h, x);
            h.c0 = gl_add(h.c0, c[e]);
        }
        h = gl2_block_fold(h, lds, a.pe[j]);
        if (threadIdx.x == 0) a.sums[((uint64_t)k * GE_PTS + j) * a.ntiles + t] = h;
    }
}

// one block per (column, point): the value sum_t S[t] x^(t GE_TILE).  A work-item folds `group` consecutive tile sums.
__global__ __launch_bounds__(GE_THREADS) void gl2_eval_fold_kernel(const Gl2EvalArgs a) {
    __shared__ Gl2 lds[GE_THREADS];
    const uint32_t k = a.k0 + blockIdx.x / a.m, j = blockIdx.x % a.m;
    const Gl2 *s = a.sums + ((uint64_t)k * GE_PTS + j) * a.ntiles;
    const uint64_t first = (uint64_t)threadIdx.x * a.group;
    const Gl2 xt = a.xt[j];
    Gl2 v{0, 0};
    for (uint32_t g = a.group; g-- > 0;)
        if (first + g < a.ntiles) v = gl2_add(gl2_mul(v, xt), s[first + g]);
    v = gl2_block_fold(v, lds, a.pg[j]);
    if (threadIdx.x == 0) a.vals[(uint64_t)k * a.m_total + a.j0 + j] = v;
}

// ---------------------------------------------------------------- DEEP quotients
constexpr int GD_THREADS = 256;
constexpr int GD_ROWS = 4;   // rows per work-item: GD_ROWS x GD_PTS norms share one inversion.  Not measured against 2 or 8.
constexpr int GD_PTS = 4;    // points per launch

struct Gl2DeepArgs {
    const uint64_t *cols;
    uint64_t col_stride;
    uint32_t n_cols, log2n, accumulate;
    uint64_t h, w;          // x_i = h w^i
    const Gl2 *wt;          // [n_cols][GD_PTS]: the weights of this launch's points
    Gl2 z[GD_PTS];          // the points
    Gl2 c[GD_PTS];          // sum_k w[k][j] e[k][j]
    uint64_t zn[GD_PTS];    // 7 z1^2
    uint64_t *out0, *out1;
};

template <int M> __global__ __launch_bounds__(GD_THREADS) void gl2_deep_kernel(const Gl2DeepArgs a) {
    const uint64_t n = 1ull << a.log2n;
    const uint64_t row0 = ((uint64_t)blockIdx.x * GD_THREADS + threadIdx.x) * GD_ROWS;
    if (row0 >= n) return;
    Gl2 acc[GD_ROWS][M];
#pragma unroll
    for (int r = 0; r < GD_ROWS; r++)
#pragma unroll
        for (int j = 0; j < M; j++) acc[r][j] = Gl2{0, 0};
#pragma unroll 1
    for (uint32_t k = 0; k < a.n_cols; k++) {
        const uint64_t *col = a.cols + (uint64_t)k * a.col_stride + row0;
        uint64_t v[GD_ROWS];
#pragma unroll
        for (int r = 0; r < GD_ROWS; r++) v[r] = row0 + r < n ? gl_from_word(col[r]) : 0;   // n < GD_ROWS: the rows past the domain
#pragma unroll
        for (int j = 0; j < M; j++) {
            const Gl2 w = a.wt[(uint64_t)k * GD_PTS + j];   // uniform
            if ((w.c0 | w.c1) == 0) continue;               // a zero weight skips the pair
#pragma unroll
            for (int r = 0; r < GD_ROWS; r++) acc[r][j] = gl2_add(acc[r][j], gl2_mul_base(w, v[r]));
        }
    }
    // the norms of x_i - z_j and their running products
    uint64_t x[GD_ROWS], nr[GD_ROWS][M], pre[GD_ROWS][M];
    x[0] = gl_mul(a.h, gl_pow(a.w, row0));
#pragma unroll
    for (int r = 1; r < GD_ROWS; r++) x[r] = gl_mul(x[r - 1], a.w);
    uint64_t run = 1;
#pragma unroll
    for (int r = 0; r < GD_ROWS; r++)
#pragma unroll
        for (int j = 0; j < M; j++) {
            const uint64_t d0 = gl_sub(x[r], a.z[j].c0);
            nr[r][j] = gl_sub(gl_mul(d0, d0), a.zn[j]);
            pre[r][j] = run;
            run = gl_mul(run, nr[r][j]);
        }
    uint64_t inv = gl_inv(run);   // run != 0: every norm is non-zero
    Gl2 sum[GD_ROWS];
#pragma unroll
    for (int r = GD_ROWS - 1; r >= 0; r--) {
        sum[r] = Gl2{0, 0};
#pragma unroll
        for (int j = M - 1; j >= 0; j--) {
            const uint64_t ninv = gl_mul(inv, pre[r][j]);
            inv = gl_mul(inv, nr[r][j]);
            const Gl2 conj{gl_sub(x[r], a.z[j].c0), a.z[j].c1};   // (x - z) conj = norm
            sum[r] = gl2_add(sum[r], gl2_mul_base(gl2_mul(gl2_sub(acc[r][j], a.c[j]), conj), ninv));
        }
    }
#pragma unroll
    for (int r = 0; r < GD_ROWS; r++) {
        if (row0 + r >= n) break;
        Gl2 o = sum[r];
        if (a.accumulate) o = gl2_add(o, Gl2{a.out0[row0 + r], a.out1[row0 + r]});   // canonical: an earlier launch wrote them
        a.out0[row0 + r] = o.c0;
        a.out1[row0 + r] = o.c1;
    }
}

// ---------------------------------------------------------------- FRI fold
// out[i] = 2 (c[2i] + zeta c[2i+1]) for i < n_out, the odd term absent past n; zeros up to `padded`
__global__ __launch_bounds__(256) void gl2_fri_fold_kernel(const uint64_t *c0, const uint64_t *c1, uint64_t n, Gl2 zeta, uint64_t *o0, uint64_t *o1,
                                                           uint64_t n_out, uint64_t padded) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= padded) return;
    Gl2 r{0, 0};
    if (i < n_out) {
        r = gl2_from_words(c0[2 * i], c1[2 * i]);
        if (2 * i + 1 < n) r = gl2_add(r, gl2_mul(zeta, gl2_from_words(c0[2 * i + 1], c1[2 * i + 1])));
        r = gl2_add(r, r);
    }
    o0[i] = r.c0;
    o1[i] = r.c1;
}

// ---------------------------------------------------------------- host
static constexpr uint64_t GL2_MAX_LEN = (uint64_t)1 << 36;   // the grids' block indices stay below 2^31

static bool gl2_overlap(const void *a, size_t a_words, const void *b, size_t b_words) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + 8 * b_words && b0 < a0 + 8 * a_words;
}
// a vector of n elements in planes `stride` words apart (0: n; below n: an error)
static int gl2_stride(size_t &stride, size_t n, const char *what) {
    if (stride == 0) stride = n;
    if (stride < n) { set_error("%s: plane stride %zu below the length %zu", what, stride, n); return LW_ERR_BAD_ARG; }
    return LW_OK;
}
static int gl2_device_ptrs(std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs) {
        if (!p) { set_error("null buffer"); return LW_ERR_BAD_ARG; }
        if (!aligned16(p)) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    }
    return LW_OK;
}
static int gl2_offset(const uint64_t *offset_or_null, uint64_t &h) {
    h = offset_or_null ? gl_from_word(*offset_or_null) : 1;
    if (h == 0) { set_error("coset offset is zero"); return LW_ERR_INV_ZERO; }
    return LW_OK;
}

static int gl2_evaluate_locked(Context &c, const uint64_t *d_coeffs, uint32_t n_cols, uint64_t col_stride, uint64_t n, const uint64_t *points,
                               uint32_t m, uint64_t *out_values, hipStream_t s) {
    const uint64_t nt = (n + GE_TILE - 1) / GE_TILE;
    const size_t sums_b = ((size_t)n_cols * GE_PTS * nt * sizeof(Gl2) + 255) & ~(size_t)255;
    if (c.poly_ws.ensure(sums_b + (size_t)n_cols * m * sizeof(Gl2))) return LW_ERR_ALLOC;
    Gl2EvalArgs a;
    memset(&a, 0, sizeof(a));
    a.cols = d_coeffs;
    a.col_stride = col_stride;
    a.n = n;
    a.ntiles = nt;
    a.m_total = m;
    a.group = (uint32_t)((nt + GE_THREADS - 1) / GE_THREADS);
    a.sums = (Gl2 *)c.poly_ws.p;
    a.vals = (Gl2 *)((char *)c.poly_ws.p + sums_b);
    for (uint32_t j0 = 0; j0 < m; j0 += GE_PTS) {
        a.j0 = j0;
        a.m = m - j0 < (uint32_t)GE_PTS ? m - j0 : (uint32_t)GE_PTS;
        for (uint32_t j = 0; j < a.m; j++) {
            const Gl2 x = gl2_from_words(points[2 * (size_t)(j0 + j)], points[2 * (size_t)(j0 + j) + 1]);
            a.x[j] = x;
            a.pe[j][0] = gl2_pow(x, GE_E);
            for (int st = 1; st < GE_STEPS; st++) a.pe[j][st] = gl2_sqr(a.pe[j][st - 1]);
            a.xt[j] = gl2_sqr(a.pe[j][GE_STEPS - 1]);   // x^(GE_E 2^GE_STEPS) = x^GE_TILE
            a.pg[j][0] = gl2_pow(a.xt[j], a.group);
            for (int st = 1; st < GE_STEPS; st++) a.pg[j][st] = gl2_sqr(a.pg[j][st - 1]);
        }
        for (uint32_t k0 = 0; k0 < n_cols; k0 += 65535) {   // the grid's y extent
            const uint32_t kc = n_cols - k0 < 65535 ? n_cols - k0 : 65535;
            a.k0 = k0;
            hipEvent_t pe = c.prof_begin(s);
            hipLaunchKernelGGL(gl2_eval_tile_kernel, dim3((uint32_t)nt, kc), dim3(GE_THREADS), 0, s, a);
            c.prof_end("gl2_eval_tile_kernel", pe, s);
            pe = c.prof_begin(s);
            hipLaunchKernelGGL(gl2_eval_fold_kernel, dim3(kc * a.m), dim3(GE_THREADS), 0, s, a);
            c.prof_end("gl2_eval_fold_kernel", pe, s);
            LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
        }
    }
    return download(out_values, a.vals, (size_t)n_cols * m * sizeof(Gl2), s);
}

static int gl2_deep_locked(Context &c, const uint64_t *d_lde, uint32_t n_cols, uint64_t col_stride, uint32_t log2n, uint64_t h, uint64_t root,
                           const uint64_t *points, uint32_t m, const uint64_t *weights, const uint64_t *evals, uint64_t *d_out, uint64_t out_stride,
                           hipStream_t s) {
    const uint32_t groups = (m + GD_PTS - 1) / GD_PTS;
    const size_t group_b = (size_t)n_cols * GD_PTS * sizeof(Gl2), tables = group_b * groups;
    if (c.poly_ws.ensure(tables)) return LW_ERR_ALLOC;
    int rc = deep_pin(c, tables);
    if (rc) return rc;
    Gl2 *hw = (Gl2 *)c.deep_pin;
    memset(hw, 0, tables);
    const auto elem = [](const uint64_t *tab, size_t i) { return gl2_from_words(tab[2 * i], tab[2 * i + 1]); };
    for (uint32_t k = 0; k < n_cols; k++)
        for (uint32_t j = 0; j < m; j++) hw[((size_t)(j / GD_PTS) * n_cols + k) * GD_PTS + j % GD_PTS] = elem(weights, (size_t)k * m + j);
    LW_HIP_CHECK(hipMemcpyAsync(c.poly_ws.p, hw, tables, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipEventRecord(c.deep_pin_read, s), LW_ERR_LAUNCH);
    Gl2DeepArgs a;
    memset(&a, 0, sizeof(a));
    a.cols = d_lde;
    a.col_stride = col_stride;
    a.n_cols = n_cols;
    a.log2n = log2n;
    a.h = h;
    a.w = gl_host_root(root, log2n, false);
    a.out0 = d_out;
    a.out1 = d_out + out_stride;
    const uint64_t rows = 1ull << log2n, items = (rows + GD_ROWS - 1) / GD_ROWS;
    for (uint32_t g = 0; g < groups; g++) {
        const uint32_t j0 = g * GD_PTS, mp = m - j0 < (uint32_t)GD_PTS ? m - j0 : (uint32_t)GD_PTS;
        a.wt = (const Gl2 *)((const char *)c.poly_ws.p + group_b * g);
        a.accumulate = g > 0;
        for (uint32_t j = 0; j < mp; j++) {
            a.z[j] = elem(points, j0 + j);
            a.zn[j] = gl_mul(gl_mul(a.z[j].c1, a.z[j].c1), GL2_NON_RESIDUE);
            Gl2 cj{0, 0};
            for (uint32_t k = 0; k < n_cols; k++) cj = gl2_add(cj, gl2_mul(elem(weights, (size_t)k * m + j0 + j), elem(evals, (size_t)k * m + j0 + j)));
            a.c[j] = cj;
        }
        void (*kernel)(Gl2DeepArgs) = mp == 1 ? gl2_deep_kernel<1> : mp == 2 ? gl2_deep_kernel<2> : mp == 3 ? gl2_deep_kernel<3> : gl2_deep_kernel<4>;
        rc = launch_1d(c, "gl2_deep_kernel", kernel, blocks_for(items), s, a);
        if (rc) return rc;
    }
    return LW_OK;
}

}  // namespace lw

using namespace lw;

extern "C" {

int lw_goldilocks_ext2_pointwise_device(lw_gl2_op_t op, const uint64_t *d_a, size_t a_stride, const uint64_t *d_b, size_t b_stride, uint64_t *d_out,
                                        size_t out_stride, size_t n, void *hip_stream) {
    if (op != LW_GL2_MUL && op != LW_GL2_SQR && op != LW_GL2_INV && op != LW_GL2_MUL_BASE) { set_error("bad Fp2 op %d", (int)op); return LW_ERR_BAD_ARG; }
    if (n == 0) return LW_OK;
    if (n > GL2_MAX_LEN) { set_error("%zu Fp2 elements", n); return LW_ERR_ALLOC; }
    const bool has_b = op == LW_GL2_MUL || op == LW_GL2_MUL_BASE;
    int rc = has_b ? gl2_device_ptrs({d_a, d_b, d_out}) : gl2_device_ptrs({d_a, d_out});
    if (!rc) rc = gl2_stride(a_stride, n, "a");
    if (!rc) rc = gl2_stride(out_stride, n, "out");
    if (!rc && op == LW_GL2_MUL) rc = gl2_stride(b_stride, n, "b");
    if (rc) return rc;
    // A plane of the output may BE a plane of an operand (work-item i reads element i of everything before it writes
    // element i), which is what d_out == d_a and d_out == d_b come to; any other overlap is refused.
    const uint64_t *in[4] = {d_a, d_a + a_stride, has_b ? d_b : nullptr, op == LW_GL2_MUL ? d_b + b_stride : nullptr};
    uint64_t *const out[2] = {d_out, d_out + out_stride};
    for (const uint64_t *o : out)
        for (const uint64_t *p : in)
            if (p && p != o && gl2_overlap(o, n, p, n)) { set_error("out overlaps an operand without being the same vector"); return LW_ERR_BAD_ARG; }
    if ((d_out == d_a && out_stride != a_stride) || (op == LW_GL2_MUL && d_out == d_b && out_stride != b_stride)) {
        set_error("out is an operand under another plane stride");
        return LW_ERR_BAD_ARG;
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    const uint64_t blocks = (n + 255) / 256;
    return launch_1d(en.c, "gl2_pointwise_kernel", gl2_pointwise_kernel, (uint32_t)(blocks < 65536 ? blocks : 65536), en.stream, (int)op, in[0], in[1],
                     in[2], in[3], out[0], out[1], (uint64_t)n);
}

int lw_goldilocks_ext2_evaluate_device(const uint64_t *d_coeffs, uint32_t n_cols, size_t col_stride, size_t n_coeffs, const uint64_t *points, uint32_t m,
                                       uint64_t *out_values, void *hip_stream) {
    if (n_cols == 0 || m == 0) return LW_OK;
    if (!points || !out_values) { set_error("null points or values"); return LW_ERR_BAD_ARG; }
    if (n_coeffs == 0) {   // the zero polynomial
        memset(out_values, 0, (size_t)n_cols * m * 16);
        return LW_OK;
    }
    if (n_coeffs > GL2_MAX_LEN) { set_error("%zu coefficients", n_coeffs); return LW_ERR_ALLOC; }
    int rc = gl2_device_ptrs({d_coeffs});
    if (!rc) rc = gl2_stride(col_stride, n_coeffs, "coefficient columns");
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return gl2_evaluate_locked(en.c, d_coeffs, n_cols, col_stride, n_coeffs, points, m, out_values, en.stream);
}

int lw_goldilocks_ext2_deep_quotients_device(const uint64_t *d_lde, uint32_t n_cols, size_t col_stride, uint32_t log2n, const uint64_t *offset_or_null,
                                             uint64_t two_adic_root, const uint64_t *points, uint32_t m, const uint64_t *weights,
                                             const uint64_t *evals, uint64_t *d_out, size_t out_stride, void *hip_stream) {
    int rc = gl_size_check(log2n);
    if (rc) return rc;
    const size_t n = (size_t)1 << log2n;
    if (n_cols == 0 || m == 0 || !points || !weights || !evals) { set_error("null table, no columns or no points"); return LW_ERR_BAD_ARG; }
    rc = gl2_device_ptrs({d_lde, d_out});
    if (!rc) rc = gl2_stride(col_stride, n, "LDE columns");
    if (!rc) rc = gl2_stride(out_stride, n, "out");
    if (rc) return rc;
    if (gl2_overlap(d_lde, (size_t)(n_cols - 1) * col_stride + n, d_out, out_stride + n)) { set_error("out overlaps the columns"); return LW_ERR_BAD_ARG; }
    for (uint32_t j = 0; j < m; j++)
        if (gl_from_word(points[2 * (size_t)j + 1]) == 0) {
            set_error("point %u lies in the base field (c1 = 0): it may be on the domain", j);
            return LW_ERR_BAD_ARG;
        }
    uint64_t h;
    rc = gl_root_check(two_adic_root);
    if (!rc) rc = gl2_offset(offset_or_null, h);
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return gl2_deep_locked(en.c, d_lde, n_cols, col_stride, log2n, h, two_adic_root, points, m, weights, evals, d_out, out_stride, en.stream);
}

int lw_goldilocks_ext2_fri_layer_device(const uint64_t *d_coeffs, size_t coeff_stride, size_t n_coeffs, const uint64_t *zeta,
                                        const uint64_t *offset_or_null, size_t domain_size, uint64_t two_adic_root, lw_rpo_level_t level,
                                        uint64_t *d_out_poly, uint64_t *d_out_evaluation_or_null, uint64_t *d_nodes_or_null,
                                        uint64_t *out_root_or_null, void *hip_stream) {
    int rc = rpo_level_check((int)level);
    if (rc || n_coeffs == 0) return rc;
    const size_t digest_words = level == LW_RPO_128 ? 4 : 5;
    if (n_coeffs > GL2_MAX_LEN) { set_error("%zu coefficients", n_coeffs); return LW_ERR_ALLOC; }
    if (!zeta) { set_error("null zeta"); return LW_ERR_BAD_ARG; }
    rc = gl2_device_ptrs({d_coeffs, d_out_poly});
    if (!rc) rc = gl2_stride(coeff_stride, n_coeffs, "coefficients");
    if (rc) return rc;
    const size_t n_out = (n_coeffs + 1) / 2;
    uint32_t lgb = 1;
    while (((size_t)1 << lgb) < n_out) lgb++;
    const size_t padded = (size_t)1 << lgb, in_words = coeff_stride + n_coeffs;
    if (gl2_overlap(d_out_poly, 2 * padded, d_coeffs, in_words)) { set_error("d_out_poly overlaps d_coeffs"); return LW_ERR_BAD_ARG; }
    const bool layer = d_nodes_or_null != nullptr;
    if (layer && !d_out_evaluation_or_null) { set_error("a tree needs d_out_evaluation"); return LW_ERR_BAD_ARG; }
    if (!layer && (d_out_evaluation_or_null || out_root_or_null)) { set_error("an evaluation or a root needs d_nodes"); return LW_ERR_BAD_ARG; }
    uint32_t lgd = 0;
    uint64_t h = 1;
    if (layer) {
        if (domain_size == 0 || (domain_size & (domain_size - 1))) { set_error("domain size %zu is not a power of two", domain_size); return LW_ERR_INPUT_NOT_POW2; }
        if (padded > domain_size) { set_error("folded block of %zu coefficients exceeds the domain %zu", padded, domain_size); return LW_ERR_BAD_ARG; }
        while (((size_t)1 << lgd) < domain_size) lgd++;
        rc = gl_size_check(lgd);
        if (!rc) rc = gl_root_check(two_adic_root);
        if (!rc) rc = gl2_offset(offset_or_null, h);
        if (!rc) rc = gl2_device_ptrs({d_out_evaluation_or_null, d_nodes_or_null});
        if (rc) return rc;
        const size_t node_words = (domain_size - 1) * digest_words;
        if (gl2_overlap(d_out_evaluation_or_null, 2 * domain_size, d_coeffs, in_words) || gl2_overlap(d_out_evaluation_or_null, 2 * domain_size, d_out_poly, 2 * padded) ||
            gl2_overlap(d_nodes_or_null, node_words, d_coeffs, in_words) || gl2_overlap(d_nodes_or_null, node_words, d_out_poly, 2 * padded) ||
            gl2_overlap(d_nodes_or_null, node_words, d_out_evaluation_or_null, 2 * domain_size)) {
            set_error("the buffers of a layer overlap");
            return LW_ERR_BAD_ARG;
        }
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    rc = launch_1d(c, "gl2_fri_fold_kernel", gl2_fri_fold_kernel, blocks_for(padded), en.stream, d_coeffs, d_coeffs + coeff_stride, (uint64_t)n_coeffs,
                   gl2_from_words(zeta[0], zeta[1]), d_out_poly, d_out_poly + padded, (uint64_t)n_out, (uint64_t)padded);
    if (rc || !layer) return rc;
    // evaluate_offset_fft(p', 1, Some(domain_size), offset) of both planes, then the tree over the pairs (e[i], e[i + N/2]):
    // the four "columns" of half a plane each, element after element (group 2), leaf j at i = bitrev(j)
    rc = goldilocks_lde_locked(c, d_out_poly, lgb, padded, d_out_evaluation_or_null, lgd, domain_size, 2, h, two_adic_root, en.stream);
    if (!rc) rc = rpo_commit_locked(c, (int)level, d_out_evaluation_or_null, 4, domain_size / 2, lgd - 1, 1, 2, d_nodes_or_null, en.stream);
    if (rc || !out_root_or_null) return rc;
    return download(out_root_or_null, d_nodes_or_null, digest_words * 8, en.stream);
}

}  // extern "C"
