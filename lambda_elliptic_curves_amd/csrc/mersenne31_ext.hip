// The quartic extension QM31 of Mersenne31 on the device (arithmetic and host tables: mersenne31_ext.cuh) and the steps a
// circle STARK prover runs in it after round 1, on the resident LDE of circle.hip and next to the Monolith commitment:
//   pointwise        mul / sqr / inv / mul_base of vectors in planes (the shared pointwise kernel and entry body of
//                    ext_steps.cuh under a policy of its own: nothing there depends on the domain)
//   evaluate         columns of base-field coefficients in the basis of evaluate_cfft at points of QM31^2
//   deep_quotients   the quotients by the lines through P_j and sigma P_j over the standard coset, in evaluation form
//   fri_layer        one circle FRI fold in evaluation form and, optionally, the Monolith tree over the folded pairs
//   round 2          the fused constraint pass and the parts of the composition polynomial (circle_round2.cuh)
// A vector of n elements is four PLANES of n words, `stride` words apart: circle.hip's batch = 4, monolith.hip's n_cols = 4.
// The univariate steps of ext_steps.cuh do not apply: the domain is the standard coset g_{2N} + i g_N, the basis is a
// product over the bits of the index, the quotients are by lines and the fold reads the inverse twiddles of circle.hip.
//
// evaluate: B_k = B_lo(P) prod_{bit j of k, j >= 3} f_j, f_j = pi^(j-1)(X).  A work-item multiplies its M31Q_E consecutive
// coefficients by the table B_0 .. B_7 of the point (kernel arguments): four base products per coefficient and point, four
// of them summed in 64 bits before one reduction.  The 256 partial sums of a block fold in LDS under f_3 .. f_10, and
// further launches of the same fold take 256 block sums each under the next eight factors until one is left (one launch
// up to 2^19 coefficients).  The coefficients are loaded once for all points of a launch.
// deep_quotients: one pass over the columns.  A work-item owns M31Q_ROWS consecutive rows and the points of the launch; the
// point of its first row is the coset's first plus the steps 2^b g_N of the set bits of the row (kernel arguments: a
// circle_mul whose doublings are the host's), the others follow by g_N.  The denominators are u times a CM31 value, so the
// M31Q_ROWS x M31Q_PTS CM31 norms share ONE m31_inv (Montgomery's trick over registers).
// fri_layer: work-item i reads v[i] and v[M-1-i], so a wave reads two runs of 256 bytes per plane, the mirrored one
// backwards.  The twiddle 1 / t_i comes from the cached inverse tables, which hold the points (1 + 4j) g: even i is entry
// i / 2, odd i the entry of the point mirrored at the axis ((M/2 - 1 - i) / 2 for y; (M - 1 - i) / 2, negated, for x).
#include "mersenne31_ext.cuh"
#include "ext_steps.cuh"

namespace lw {

// ---------------------------------------------------------------- pointwise: the policy of ext_pointwise
struct M31qExt {
    using word = uint32_t;
    using elem = Qm31;
    static constexpr int D = 4;
    static constexpr const char *NAME = "QM31";
    static constexpr ExtNames NAMES{"m31q_pointwise_kernel", "m31q_eval_tile_kernel", "m31q_eval_fold_kernel", "m31q_deep_kernel", "m31q_fri_fold_kernel"};
    EXT_HD word fcanon(word x) { return m31_from_word(x); }
    EXT_HD word fadd(word a, word b) { return m31_add(a, b); }   // fadd, fsub, fmul: the interpreter of circle_round2.cuh (AirWord)
    EXT_HD word fsub(word a, word b) { return m31_sub(a, b); }
    EXT_HD word fmul(word a, word b) { return m31_mul(a, b); }
    EXT_HD elem load(ExtPlanes<M31qExt> v, uint64_t i) { return Qm31{m31_from_word(v.p[0][i]), m31_from_word(v.p[1][i]), m31_from_word(v.p[2][i]), m31_from_word(v.p[3][i])}; }
    EXT_HD void store(ExtPlanes<M31qExt> v, uint64_t i, elem a) {
        v.p[0][i] = m31_canon(a.c0);
        v.p[1][i] = m31_canon(a.c1);
        v.p[2][i] = m31_canon(a.c2);
        v.p[3][i] = m31_canon(a.c3);
    }
    EXT_HD elem canon(elem a) { return a; }   // load has read the words
    EXT_HD elem mul(elem a, elem b) { return m31q_mul(a, b); }
    EXT_HD elem sqr(elem a) { return m31q_sqr(a); }
    EXT_HD elem inv(elem a) { return m31q_inv(a); }
    EXT_HD elem mul_base(elem a, word b) { return m31q_mul_base(a, b); }
};
using M31qPlanes = ExtPlanes<M31qExt>;
static_assert((int)LW_M31EXT4_MUL == EXT_MUL && (int)LW_M31EXT4_SQR == EXT_SQR && (int)LW_M31EXT4_INV == EXT_INV && (int)LW_M31EXT4_MUL_BASE == EXT_MUL_BASE,
              "the shared pointwise kernel reads this extension's ops");

// ---------------------------------------------------------------- evaluate
struct M31qEvalArgs {
    const uint32_t *cols;
    uint64_t col_stride, n;
    uint32_t k0, m, m_total, j0;   // first column of this launch; points of this launch, of the call, the first of this launch
    uint64_t count, count_out;     // fold: sums per (column, point) coming in and going out
    const Qm31 *in;                // fold: [n_cols][M31Q_PTS][count]
    Qm31 *out;                     // tile: [n_cols][M31Q_PTS][ntiles]; fold: [n_cols][M31Q_PTS][count_out]
    Qm31 *vals;                    // [n_cols][m_total], written by the fold that leaves one sum
    Qm31 lo[M31Q_PTS][M31Q_E];     // tile: B_e(P_j)
    Qm31 f[M31Q_PTS][M31Q_STEPS];  // the factors of the eight index bits this launch folds
};

// sum_r v_r prod_{bit s of r} f[s] over the block's 256 work-items: the result is work-item 0's.  At step s the work-items
// whose index is a multiple of 2^(s+1) take in the one 2^s above, which was active in the step before.
__device__ __forceinline__ Qm31 m31q_block_fold(Qm31 v, Qm31 *lds, const Qm31 *f) {
    const int r = threadIdx.x;
#pragma unroll 1
    for (int s = 0; s < M31Q_STEPS; s++) {
        lds[r] = v;
        __syncthreads();
        const int d = 1 << s;
        if ((r & (2 * d - 1)) == 0) v = m31q_add(v, m31q_mul(f[s], lds[r + d]));   // r + d <= 255
        __syncthreads();
    }
    return v;
}

__global__ __launch_bounds__(M31Q_THREADS) void m31q_eval_tile_kernel(const M31qEvalArgs a) {
    __shared__ Qm31 lds[M31Q_THREADS];
    const uint32_t k = a.k0 + blockIdx.y;
    const uint64_t t = blockIdx.x;
    const uint32_t *col = a.cols + (uint64_t)k * a.col_stride;
    const uint64_t base = (t << M31Q_TILE_LOG) + (uint64_t)threadIdx.x * M31Q_E;
    uint32_t c[M31Q_E];
#pragma unroll
    for (int e = 0; e < M31Q_E; e++) c[e] = base + e < a.n ? m31_from_word(col[base + e]) : 0;
#pragma unroll 1
    for (uint32_t j = 0; j < a.m; j++) {
        const Qm31 *lo = a.lo[j];   // uniform
        Qm31 h;
        h.c0 = m31_add(m31_red64(m31_wide(c[0], lo[0].c0) + m31_wide(c[1], lo[1].c0) + m31_wide(c[2], lo[2].c0) + m31_wide(c[3], lo[3].c0)),
                       m31_red64(m31_wide(c[4], lo[4].c0) + m31_wide(c[5], lo[5].c0) + m31_wide(c[6], lo[6].c0) + m31_wide(c[7], lo[7].c0)));
        h.c1 = m31_add(m31_red64(m31_wide(c[0], lo[0].c1) + m31_wide(c[1], lo[1].c1) + m31_wide(c[2], lo[2].c1) + m31_wide(c[3], lo[3].c1)),
                       m31_red64(m31_wide(c[4], lo[4].c1) + m31_wide(c[5], lo[5].c1) + m31_wide(c[6], lo[6].c1) + m31_wide(c[7], lo[7].c1)));
        h.c2 = m31_add(m31_red64(m31_wide(c[0], lo[0].c2) + m31_wide(c[1], lo[1].c2) + m31_wide(c[2], lo[2].c2) + m31_wide(c[3], lo[3].c2)),
                       m31_red64(m31_wide(c[4], lo[4].c2) + m31_wide(c[5], lo[5].c2) + m31_wide(c[6], lo[6].c2) + m31_wide(c[7], lo[7].c2)));
        h.c3 = m31_add(m31_red64(m31_wide(c[0], lo[0].c3) + m31_wide(c[1], lo[1].c3) + m31_wide(c[2], lo[2].c3) + m31_wide(c[3], lo[3].c3)),
                       m31_red64(m31_wide(c[4], lo[4].c3) + m31_wide(c[5], lo[5].c3) + m31_wide(c[6], lo[6].c3) + m31_wide(c[7], lo[7].c3)));
        h = m31q_block_fold(h, lds, a.f[j]);
        if (threadIdx.x == 0) a.out[((uint64_t)k * M31Q_PTS + j) * gridDim.x + t] = h;
    }
}

// block (b, column x point): the sums 256 b .. 256 b + 255 of the (column, point) under the next eight factors
__global__ __launch_bounds__(M31Q_THREADS) void m31q_eval_fold_kernel(const M31qEvalArgs a) {
    __shared__ Qm31 lds[M31Q_THREADS];
    const uint32_t k = a.k0 + blockIdx.y / a.m, j = blockIdx.y % a.m;
    const uint64_t i = (uint64_t)blockIdx.x * M31Q_THREADS + threadIdx.x;
    Qm31 v = i < a.count ? a.in[((uint64_t)k * M31Q_PTS + j) * a.count + i] : m31q_zero();
    v = m31q_block_fold(v, lds, a.f[j]);
    if (threadIdx.x != 0) return;
    if (a.count_out == 1)
        a.vals[(uint64_t)k * a.m_total + a.j0 + j] = m31q_canon(v);
    else
        a.out[((uint64_t)k * M31Q_PTS + j) * a.count_out + blockIdx.x] = v;
}

// ---------------------------------------------------------------- DEEP quotients
struct M31qDeepArgs {
    const uint32_t *cols;
    uint64_t col_stride;
    uint32_t n_cols, log2n, accumulate;
    const Qm31 *wt;                 // [n_cols][M31Q_PTS]: cc_j w[k][j] of this launch's points
    M31qDeepPoint z[M31Q_PTS];
    M31qCoset coset;
    M31qPlanes out;
};

template <int M> __global__ __launch_bounds__(M31Q_THREADS) void m31q_deep_kernel(const M31qDeepArgs a) {
    const uint64_t n = 1ull << a.log2n;
    const uint64_t row0 = ((uint64_t)blockIdx.x * M31Q_THREADS + threadIdx.x) * M31Q_ROWS;
    if (row0 >= n) return;
    Qm31 acc[M31Q_ROWS][M];
#pragma unroll
    for (int r = 0; r < M31Q_ROWS; r++)
#pragma unroll
        for (int j = 0; j < M; j++) acc[r][j] = m31q_zero();
    // acc[r][j] += w[k][j] col_k[row0 + r], two columns to a reduction: acc + two products <= p + 2 p^2 < 2^64
#pragma unroll 1
    for (uint32_t k = 0; k < a.n_cols; k += 2) {
        const bool two = k + 1 < a.n_cols;   // uniform
        const uint32_t *col = a.cols + (uint64_t)k * a.col_stride + row0;
        uint32_t v0[M31Q_ROWS], v1[M31Q_ROWS];
#pragma unroll
        for (int r = 0; r < M31Q_ROWS; r++) {   // n < M31Q_ROWS: the rows past the domain read nothing
            v0[r] = row0 + r < n ? m31_from_word(col[r]) : 0;
            v1[r] = two && row0 + r < n ? m31_from_word(col[a.col_stride + r]) : 0;
        }
#pragma unroll
        for (int j = 0; j < M; j++) {
            const Qm31 w0 = a.wt[(uint64_t)k * M31Q_PTS + j];                          // uniform
            const Qm31 w1 = two ? a.wt[(uint64_t)(k + 1) * M31Q_PTS + j] : m31q_zero();
#pragma unroll
            for (int r = 0; r < M31Q_ROWS; r++) {
                acc[r][j].c0 = m31_red64(acc[r][j].c0 + m31_wide(w0.c0, v0[r]) + m31_wide(w1.c0, v1[r]));
                acc[r][j].c1 = m31_red64(acc[r][j].c1 + m31_wide(w0.c1, v0[r]) + m31_wide(w1.c1, v1[r]));
                acc[r][j].c2 = m31_red64(acc[r][j].c2 + m31_wide(w0.c2, v0[r]) + m31_wide(w1.c2, v1[r]));
                acc[r][j].c3 = m31_red64(acc[r][j].c3 + m31_wide(w0.c3, v0[r]) + m31_wide(w1.c3, v1[r]));
            }
        }
    }
    // the points of the rows: g_{2N} + row0 g_N from the steps of the set bits of row0 (a multiple of M31Q_ROWS), then by g_N
    CirclePt pt[M31Q_ROWS];
    pt[0] = a.coset.shift;
#pragma unroll 1
    for (uint32_t b = 2; b < a.log2n; b++)
        if ((row0 >> b) & 1u) pt[0] = circle_add(pt[0], a.coset.step[b]);
#pragma unroll
    for (int r = 1; r < M31Q_ROWS; r++) pt[r] = circle_add(pt[r - 1], a.coset.step[0]);
    // the norms of d_j(x_i, y_i) and their running products
    uint32_t nr[M31Q_ROWS][M], pre[M31Q_ROWS][M];
    uint32_t run = 1u;
#pragma unroll
    for (int r = 0; r < M31Q_ROWS; r++)
#pragma unroll
        for (int j = 0; j < M; j++) {
            const Cm31 d = cm31_add(cm31_add(cm31_mul_base(a.z[j].da, pt[r].x), cm31_mul_base(a.z[j].db, pt[r].y)), a.z[j].dc);
            nr[r][j] = cm31_norm(d);
            pre[r][j] = run;
            run = m31_mul(run, nr[r][j]);
        }
    // the way back: 1 / norm from the running inverse, 1 / d from it, the quotient onto the row's sum
    uint32_t inv = m31_inv(run);   // run != 0: no line meets the domain
    Qm31 sum[M31Q_ROWS];
#pragma unroll
    for (int r = M31Q_ROWS - 1; r >= 0; r--) {
        sum[r] = m31q_zero();
#pragma unroll
        for (int j = M - 1; j >= 0; j--) {
            const uint32_t ninv = m31_mul(inv, pre[r][j]);
            inv = m31_mul(inv, nr[r][j]);
            const Cm31 d = cm31_add(cm31_add(cm31_mul_base(a.z[j].da, pt[r].x), cm31_mul_base(a.z[j].db, pt[r].y)), a.z[j].dc);
            const Qm31 num = m31q_sub(m31q_sub(acc[r][j], m31q_mul_base(a.z[j].sa, pt[r].y)), a.z[j].sb);
            sum[r] = m31q_add(sum[r], m31q_mul_cm31(num, cm31_inv_with(d, ninv)));
        }
    }
#pragma unroll
    for (int r = 0; r < M31Q_ROWS; r++) {
        if (row0 + r >= n) break;
        Qm31 o = sum[r];
        if (a.accumulate) o = m31q_add(o, M31qExt::load(a.out, row0 + r));
        M31qExt::store(a.out, row0 + r, o);
    }
}

// ---------------------------------------------------------------- FRI fold
// out[i] = (v[i] + v[M-1-i] + zeta / t_i (v[i] - v[M-1-i])) / 2, i < M / 2.  tw: the inverse y-layer of size M (first fold)
// or the inverse x-layer with M / 2 entries.  pairs (or null): the eight columns of M / 4 words the folded layer is
// committed as, column e = out[i].ce, column 4 + e = out[M/2 - 1 - i].ce, i < M / 4.
__global__ __launch_bounds__(M31Q_THREADS) void m31q_fri_fold_kernel(const M31qPlanes v, uint64_t m, Qm31 zeta, const uint32_t *tw, int first,
                                                                     const M31qPlanes out, uint32_t *pairs) {
    const uint64_t half = m >> 1, i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= half) return;
    const Qm31 x = M31qExt::load(v, i), y = M31qExt::load(v, m - 1 - i);
    uint32_t tinv;
    if ((i & 1) == 0)
        tinv = tw[i >> 1];
    else
        tinv = first ? tw[(half - 1 - i) >> 1] : m31_neg(tw[(m - 1 - i) >> 1]);
    Qm31 r = m31q_add(m31q_add(x, y), m31q_mul(m31q_mul_base(zeta, tinv), m31q_sub(x, y)));
    r = m31q_canon(m31q_mul_base(r, 1u << 30));   // 2^30 = 1 / 2
    out.p[0][i] = r.c0;
    out.p[1][i] = r.c1;
    out.p[2][i] = r.c2;
    out.p[3][i] = r.c3;
    if (pairs) {
        const uint64_t q = half >> 1;
        uint32_t *p = i < q ? pairs + i : pairs + 4 * q + (half - 1 - i);
        p[0] = r.c0;
        p[q] = r.c1;
        p[2 * q] = r.c2;
        p[3 * q] = r.c3;
    }
}

// ---------------------------------------------------------------- host: drivers
static int m31q_evaluate_locked(Context &c, const uint32_t *d_coeffs, uint32_t n_cols, uint64_t col_stride, uint32_t log2n, const uint32_t *points, uint32_t m,
                                uint32_t *out_values, hipStream_t s) {
    const uint64_t n = 1ull << log2n, nt = (n + (1ull << M31Q_TILE_LOG) - 1) >> M31Q_TILE_LOG;
    const uint64_t nt2 = (nt + M31Q_THREADS - 1) / M31Q_THREADS;
    const size_t a_b = ((size_t)n_cols * M31Q_PTS * nt * sizeof(Qm31) + 255) & ~(size_t)255, b_b = ((size_t)n_cols * M31Q_PTS * nt2 * sizeof(Qm31) + 255) & ~(size_t)255;
    if (c.poly_ws.ensure(a_b + b_b + (size_t)n_cols * m * sizeof(Qm31))) return LW_ERR_ALLOC;
    Qm31 *buf[2] = {(Qm31 *)c.poly_ws.p, (Qm31 *)((char *)c.poly_ws.p + a_b)};
    M31qEvalArgs a;
    memset(&a, 0, sizeof(a));
    a.cols = d_coeffs;
    a.col_stride = col_stride;
    a.n = n;
    a.m_total = m;
    a.vals = (Qm31 *)((char *)c.poly_ws.p + a_b + b_b);
    for (uint32_t j0 = 0; j0 < m; j0 += M31Q_PTS) {
        a.j0 = j0;
        a.m = m - j0 < (uint32_t)M31Q_PTS ? m - j0 : (uint32_t)M31Q_PTS;
        M31qBasis basis[M31Q_PTS];
        for (uint32_t j = 0; j < a.m; j++) {
            m31q_basis_tables(m31q_point_of(points + 8 * (size_t)(j0 + j)), basis[j]);
            memcpy(a.lo[j], basis[j].lo, sizeof(basis[j].lo));
        }
        // the factors of bits bit0 .. bit0 + 7; past the last bit of a coefficient index nothing multiplies them
        auto factors = [&](int bit0) {
            for (uint32_t j = 0; j < a.m; j++)
                for (int st = 0; st < M31Q_STEPS; st++) a.f[j][st] = bit0 + st < M31Q_MAX_LOG ? basis[j].f[bit0 + st] : m31q_zero();
        };
        for (uint32_t k0 = 0; k0 < n_cols; k0 += 65535 / M31Q_PTS) {   // the grid's y extent, in the fold too
            const uint32_t kc = n_cols - k0 < 65535 / M31Q_PTS ? n_cols - k0 : 65535 / M31Q_PTS;
            a.k0 = k0;
            a.out = buf[0];
            factors(M31Q_E_LOG);
            hipEvent_t pe = c.prof_begin(s);
            hipLaunchKernelGGL(m31q_eval_tile_kernel, dim3((uint32_t)nt, kc), dim3(M31Q_THREADS), 0, s, a);
            c.prof_end(M31qExt::NAMES.eval_tile, pe, s);
            uint64_t count = nt;
            int bit0 = M31Q_TILE_LOG, from = 0;
            do {
                a.count = count;
                a.count_out = (count + M31Q_THREADS - 1) / M31Q_THREADS;
                a.in = buf[from];
                a.out = buf[from ^ 1];
                factors(bit0);
                pe = c.prof_begin(s);
                hipLaunchKernelGGL(m31q_eval_fold_kernel, dim3((uint32_t)a.count_out, kc * a.m), dim3(M31Q_THREADS), 0, s, a);
                c.prof_end(M31qExt::NAMES.eval_fold, pe, s);
                count = a.count_out;
                bit0 += M31Q_STEPS;
                from ^= 1;
            } while (count > 1);
            LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
        }
    }
    return download(out_values, a.vals, (size_t)n_cols * m * sizeof(Qm31), s);
}

static int m31q_deep_locked(Context &c, const uint32_t *d_lde, uint32_t n_cols, uint64_t col_stride, uint32_t log2n, const uint32_t *points, uint32_t m,
                            const uint32_t *weights, const uint32_t *evals, uint32_t *d_out, uint64_t out_stride, hipStream_t s) {
    const uint32_t groups = (m + M31Q_PTS - 1) / M31Q_PTS;
    const size_t group_b = (size_t)n_cols * M31Q_PTS * sizeof(Qm31), tables = group_b * groups;
    if (c.poly_ws.ensure(tables)) return LW_ERR_ALLOC;
    int rc = deep_pin(c, tables);
    if (rc) return rc;
    std::vector<M31qDeepPoint> z(m);
    for (uint32_t j = 0; j < m; j++) z[j] = m31q_deep_point(m31q_point_of(points + 8 * (size_t)j), weights, evals, n_cols, m, j);
    m31q_regroup_weights(weights, z.data(), n_cols, m, (Qm31 *)c.deep_pin);
    LW_HIP_CHECK(hipMemcpyAsync(c.poly_ws.p, c.deep_pin, tables, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipEventRecord(c.deep_pin_read, s), LW_ERR_LAUNCH);
    M31qDeepArgs a;
    memset(&a, 0, sizeof(a));
    a.cols = d_lde;
    a.col_stride = col_stride;
    a.n_cols = n_cols;
    a.log2n = log2n;
    a.coset = m31q_coset(log2n);
    a.out = ext_planes<M31qExt>(d_out, out_stride);
    const uint64_t rows = 1ull << log2n, items = (rows + M31Q_ROWS - 1) / M31Q_ROWS;
    for (uint32_t g = 0; g < groups; g++) {
        const uint32_t j0 = g * M31Q_PTS, mp = m - j0 < (uint32_t)M31Q_PTS ? m - j0 : (uint32_t)M31Q_PTS;
        a.wt = (const Qm31 *)((const char *)c.poly_ws.p + group_b * g);
        a.accumulate = g > 0;
        for (uint32_t j = 0; j < mp; j++) a.z[j] = z[j0 + j];
        void (*kernel)(M31qDeepArgs) = mp == 1 ? m31q_deep_kernel<1> : mp == 2 ? m31q_deep_kernel<2> : mp == 3 ? m31q_deep_kernel<3> : m31q_deep_kernel<4>;
        rc = launch_1d(c, M31qExt::NAMES.deep, kernel, blocks_for(items), s, a);
        if (rc) return rc;
    }
    return LW_OK;
}

static int m31q_size_check(uint32_t log2n) {
    if (log2n > (uint32_t)M31Q_MAX_LOG) {
        set_error("2^%u points: the standard coset needs g_{2n} in a group of order 2^31", log2n);
        return LW_ERR_ORDER_TOO_LARGE;
    }
    if (log2n == 0) { set_error("a circle domain has at least 2 points"); return LW_ERR_BAD_ARG; }
    return LW_OK;
}

}  // namespace lw

#include "circle_round2.cuh"   // round 2: the fused constraint pass and the parts, on M31qExt and m31q_size_check above

using namespace lw;

extern "C" {

int lw_mersenne31_ext4_pointwise_device(lw_m31ext4_op_t op, const uint32_t *d_a, size_t a_stride, const uint32_t *d_b, size_t b_stride, uint32_t *d_out,
                                        size_t out_stride, size_t n, void *hip_stream) {
    return ext_pointwise<M31qExt>((int)op, d_a, a_stride, d_b, b_stride, d_out, out_stride, n, hip_stream);
}

int lw_mersenne31_ext4_evaluate_device(const uint32_t *d_coeffs, uint32_t n_cols, size_t col_stride, uint32_t log2n, const uint32_t *points, uint32_t m,
                                       uint32_t *out_values, void *hip_stream) {
    int rc = m31q_size_check(log2n);
    if (rc) return rc;
    if (n_cols == 0 || m == 0) return LW_OK;
    if (!points || !out_values) { set_error("null points or values"); return LW_ERR_BAD_ARG; }
    rc = ext_device_ptrs({d_coeffs});
    if (!rc) rc = ext_stride(col_stride, (size_t)1 << log2n, "coefficient columns");
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return m31q_evaluate_locked(en.c, d_coeffs, n_cols, col_stride, log2n, points, m, out_values, en.stream);
}

int lw_mersenne31_ext4_deep_quotients_device(const uint32_t *d_lde, uint32_t n_cols, size_t col_stride, uint32_t log2n, const uint32_t *points, uint32_t m,
                                             const uint32_t *weights, const uint32_t *evals, uint32_t *d_out, size_t out_stride, void *hip_stream) {
    int rc = m31q_size_check(log2n);
    if (rc) return rc;
    const size_t n = (size_t)1 << log2n;
    if (n_cols == 0 || m == 0 || !points || !weights || !evals) { set_error("null table, no columns or no points"); return LW_ERR_BAD_ARG; }
    rc = ext_device_ptrs({d_lde, d_out});
    if (!rc) rc = ext_stride(col_stride, n, "LDE columns");
    if (!rc) rc = ext_stride(out_stride, n, "out");
    if (rc) return rc;
    if (ext_overlap<M31qExt>(d_lde, (size_t)(n_cols - 1) * col_stride + n, d_out, ext_span<M31qExt>(out_stride, n))) {
        set_error("out overlaps the columns");
        return LW_ERR_BAD_ARG;
    }
    for (uint32_t j = 0; j < m; j++)
        if (m31q_point_is_self_conjugate(m31q_point_of(points + 8 * (size_t)j))) {
            set_error("point %u is its own conjugate: the line through it and its conjugate does not exist", j);
            return LW_ERR_BAD_ARG;
        }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return m31q_deep_locked(en.c, d_lde, n_cols, col_stride, log2n, points, m, weights, evals, d_out, out_stride, en.stream);
}

int lw_mersenne31_ext4_fri_layer_device(const uint32_t *d_evals, size_t in_stride, uint32_t log2m, const uint32_t *zeta, int first, uint32_t *d_out,
                                        size_t out_stride, uint32_t rounds, uint32_t *d_pairs_or_null, uint32_t *d_nodes_or_null,
                                        uint32_t *out_root_or_null, void *hip_stream) {
    int rc = m31q_size_check(log2m);
    if (rc) return rc;
    if (!first && log2m >= (uint32_t)M31Q_MAX_LOG) { set_error("a later fold of 2^%u values: its twiddles are those of a coset of twice the size", log2m); return LW_ERR_ORDER_TOO_LARGE; }
    if (!zeta) { set_error("null zeta"); return LW_ERR_BAD_ARG; }
    const size_t m = (size_t)1 << log2m, half = m >> 1;
    rc = ext_device_ptrs({d_evals, d_out});
    if (!rc) rc = ext_stride(in_stride, m, "evaluations");
    if (!rc) rc = ext_stride(out_stride, half, "out");
    if (rc) return rc;
    const size_t in_words = ext_span<M31qExt>(in_stride, m), out_words = ext_span<M31qExt>(out_stride, half);
    if (ext_overlap<M31qExt>(d_out, out_words, d_evals, in_words)) { set_error("d_out overlaps d_evals"); return LW_ERR_BAD_ARG; }
    const bool layer = d_nodes_or_null != nullptr;
    if (!layer && (d_pairs_or_null || out_root_or_null)) { set_error("pair rows or a root need d_nodes"); return LW_ERR_BAD_ARG; }
    if (layer) {
        if (half < 4) { set_error("a committed layer has at least 4 values, not %zu", half); return LW_ERR_BAD_ARG; }
        if (rounds < 1 || rounds > 15) { set_error("Monolith rounds %u: 1 .. 15", rounds); return LW_ERR_BAD_ARG; }
        rc = ext_device_ptrs({d_pairs_or_null, d_nodes_or_null});
        if (rc) return rc;
        const size_t pair_words = 4 * half, node_words = (half - 1) * 8;   // 8 columns of half / 2 words; 2 (half / 2) - 1 digests
        if (ext_overlap<M31qExt>(d_pairs_or_null, pair_words, d_evals, in_words) || ext_overlap<M31qExt>(d_pairs_or_null, pair_words, d_out, out_words) ||
            ext_overlap<M31qExt>(d_nodes_or_null, node_words, d_evals, in_words) || ext_overlap<M31qExt>(d_nodes_or_null, node_words, d_out, out_words) ||
            ext_overlap<M31qExt>(d_nodes_or_null, node_words, d_pairs_or_null, pair_words)) {
            set_error("the buffers of a layer overlap");
            return LW_ERR_BAD_ARG;
        }
    }
    {
        Entry en(hip_stream);
        if (en.rc) return en.rc;
        // a later fold of M values reads x-layer log2m - 1, which a transform of 2M words keeps
        const uint32_t *ix = nullptr, *iy = nullptr;
        rc = circle_inverse_twiddles(en.c, first ? log2m : log2m + 1, en.stream, &ix, &iy);
        if (rc) return rc;
        const uint32_t *tw = first ? iy : ix + (half - 1);   // layer s at word 2^s - 1, 2^s = M / 2
        rc = launch_1d(en.c, M31qExt::NAMES.fri_fold, m31q_fri_fold_kernel, blocks_for(half), en.stream, ext_planes<M31qExt>(d_evals, in_stride), (uint64_t)m,
                       m31q_canon(m31q_from_words(zeta)), tw, first ? 1 : 0, ext_planes<M31qExt>(d_out, out_stride), layer ? d_pairs_or_null : (uint32_t *)nullptr);
        if (rc || !layer) return rc;
    }
    // the tree of the existing commitment over the eight pair columns, on the same stream behind the fold
    return lw_monolith_commit_columns_device(rounds, d_pairs_or_null, 8, 0, log2m - 2, 0, d_nodes_or_null, out_root_or_null, hip_stream);
}

int lw_mersenne31_ext4_constraint_evaluations_device(const lw_stark_air_op_t *ops, uint32_t n_ops, const uint32_t *consts, uint32_t n_consts,
                                                     const uint32_t *const *d_columns, const uint32_t *col_log2_len_or_null, uint32_t n_cols,
                                                     uint32_t log2_trace, uint32_t log2_blowup, const lw_m31q_boundary_t *boundary, uint32_t n_boundary,
                                                     const lw_m31q_transition_t *transitions, uint32_t n_transitions, uint32_t *d_out, size_t out_stride,
                                                     void *hip_stream) {
    return m31q_r2_constraint_evaluations(ops, n_ops, consts, n_consts, d_columns, col_log2_len_or_null, n_cols, log2_trace, log2_blowup, boundary, n_boundary,
                                          transitions, n_transitions, d_out, out_stride, hip_stream);
}

int lw_mersenne31_ext4_composition_parts_device(const uint32_t *d_evals, size_t evals_stride, uint32_t log2_lde, uint32_t log2_part, uint32_t n_parts,
                                                uint32_t *d_parts_coeffs, uint32_t *d_parts_lde_or_null, uint64_t *out_tail_nonzero_or_null,
                                                void *hip_stream) {
    return m31q_r2_composition_parts(d_evals, evals_stride, log2_lde, log2_part, n_parts, d_parts_coeffs, d_parts_lde_or_null, out_tail_nonzero_or_null,
                                     hip_stream);
}

}  // extern "C"
