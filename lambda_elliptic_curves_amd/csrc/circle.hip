// Circle FFT over Mersenne31 on gfx950: evaluate_cfft / interpolate_cfft / get_twiddles of math/src/circle/ and the
// low-degree extension built from them.  One u32 per element (circle.cuh), LDS-tiled multi-layer passes as in ntt_bb.hip.
//
// Frame.  The reference bit-reverses the coefficients, runs L layers with half chunks h = 2^i and twiddle tw[i][j] at
// position j of the half chunk, and reorders the result (out[2i] = a[i], out[2i+1] = a[n-1-i]).  Here the vector is kept
// in the index q = bitrev(position): the coefficients are read as they lie, layer s pairs the words whose q differ in bit
// L-1-s, and its twiddle is tw[s][bitrev_s(q >> (L - s))].  That is the NR-DIT dataflow of ntt_bb.hip with one table per
// layer, kept in the reference's order (which is also what lw_circle_get_twiddles returns).  Interpolation is the same
// passes backwards with (hi, lo) <- (hi + lo, (hi - lo) / tw).
//
// Passes.  A transform of 2^L words takes ceil(L / 8) passes (plan_passes), each a tile of 2^r rows x 2^logC columns in LDS:
//   HI pass  (every evaluation pass but the last, every interpolation pass but the first): rows are the q bits
//            [L-s0-r, L-s0), columns lower bits, so a tile reads and writes 2^logC consecutive words per row and all of it
//            shares the 2^r - 1 twiddles of its stages (they depend on the bits above the rows only): staged in LDS.
//   LO pass  (last of an evaluation, first of an interpolation): rows are the q bits [0, r), i.e. the high bits of the
//            position.  On the coefficient side a column is 2^r consecutive words.  On the evaluation side both
//            permutations are in the addresses: position P = (bitrev(row) << cb) | column goes to word 2P (P < n/2) or
//            2(n-1-P)+1.  A tile takes 2^(logC-1) neighbouring columns AND their complements, so that it holds word
//            2P+1 next to word 2P and moves runs of 2^logC consecutive words, through LDS (XOR-swizzled by row, so that
//            neither the row-wise nor the column-wise side of the tile runs into one bank).
//            The stages' twiddles are tw[s][(bitrev(x) << s0) | column]: consecutive over the columns a wave covers.
// N^-1 rides on the last store of an interpolation; every word of a result is canonical (< p), intermediates are in [0, p].
#include <stdlib.h>
#include <string.h>
#include "internal.h"
#include "circle.cuh"
#include "ntt_plan.h"

namespace lw {

constexpr int CIRCLE_TILE_LOG = 13;   // 8192 u32 = 32 KiB of LDS
constexpr int CIRCLE_TILE = 1 << CIRCLE_TILE_LOG;
constexpr int CIRCLE_THREADS = 256;
constexpr int CIRCLE_KMAX = 4;        // radix-16 register steps
constexpr uint32_t CIRCLE_MAX_LOG = 30;   // g_{2n} must exist in a group of order 2^31

struct CirclePassParams {
    const uint32_t *in;
    uint32_t *out;
    const uint32_t *twx;   // x-layers (or their inverses), layer i at word 2^i - 1
    const uint32_t *twy;   // layer L - 1 of this size (or its inverses)
    uint64_t in_stride, out_stride;   // words between the columns of a batch
    uint32_t L, s0, r, logC;
    uint32_t nsteps, k[4], t0[4];     // register steps in the order they run: stages t0 .. t0 + k - 1 of the pass
    // low-degree extension (first evaluation pass): word q of the zero-padded coefficients is in[q & in_mask] — the stages
    // that only pair data with padding leave the block replicated and are skipped (s0 starts behind them)
    uint32_t in_mask;
    uint32_t sc;           // != 0: the store multiplies by it (N^-1)
    uint32_t canonical;    // the store writes canonical residues (the caller's buffer)
};

__device__ __forceinline__ uint32_t circle_bitrev(uint32_t x, uint32_t bits) { return bits ? (__brev(x) >> (32 - bits)) : 0u; }
__device__ __forceinline__ uint32_t circle_slot(uint32_t m, uint32_t c, uint32_t logC) {
    return (m << logC) | (c ^ ((m ^ (m >> 4)) & ((1u << logC) - 1)));
}
// LO pass: the low cb = L - r position bits of tile column c of block b.  Columns below 2^(logC-1) are the block's own,
// the others their complements (the partners under P -> n-1-P).
__device__ __forceinline__ uint32_t circle_column(uint32_t b, uint32_t c, uint32_t logC, uint32_t cb) {
    if (cb == 0) return 0u;
    const uint32_t half = logC - 1;
    const uint32_t v = (b << half) | (c & ((1u << half) - 1));
    return (c >> half) ? (~v & ((1u << cb) - 1)) : v;
}
// LO pass, evaluation side: item e of the tile -> (row, column) such that consecutive e are consecutive words
__device__ __forceinline__ void circle_fold_item(uint32_t e, uint32_t r, uint32_t logC, uint32_t &m, uint32_t &c) {
    const uint32_t rmask = (1u << r) - 1, odd = e & 1u;
    if (logC == 0) {   // the whole transform in one tile
        const uint32_t m0 = e & ~1u;
        m = odd ? (~m0 & rmask) : m0;
        c = 0;
        return;
    }
    const uint32_t hmask = (1u << (logC - 1)) - 1;
    const uint32_t cl = (e >> 1) & hmask, u = e >> logC;
    const uint32_t m0 = u & ~1u, f0 = u & 1u;   // even row: P < n/2, word 2P; its partner row ~m0 holds word 2P+1
    m = odd ? (~m0 & rmask) : m0;
    c = ((f0 ^ odd) << (logC - 1)) | (f0 ? (~cl & hmask) : cl);
}
__device__ __forceinline__ uint32_t circle_fold_word(uint32_t m, uint32_t col, uint32_t r, uint32_t cb) {
    const uint32_t P = (circle_bitrev(m, r) << cb) | col, n = 1u << (r + cb);
    return P < n / 2 ? 2 * P : 2 * (n - 1 - P) + 1;
}

template <int K, bool LO, bool INV>
__device__ __forceinline__ void circle_item(const CirclePassParams &p, uint32_t *lds, const uint32_t *ltw, uint32_t w, uint32_t t0, uint32_t b) {
    constexpr int E = 1 << K;
    const uint32_t r = p.r, logC = p.logC, L = p.L, s0 = p.s0;
    const uint32_t c = w & ((1u << logC) - 1), mr = w >> logC;   // columns fastest: LDS rows and LO twiddles are consecutive
    const uint32_t sh = r - t0 - K;
    const uint32_t m_high = mr >> sh;
    const uint32_t mbase = (m_high << (sh + K)) | (mr & ((1u << sh) - 1));
    const uint32_t col = LO ? circle_column(b, c, logC, L - r) : 0u;
    uint32_t x[E];
#pragma unroll
    for (int j = 0; j < E; j++) x[j] = lds[circle_slot(mbase | ((uint32_t)j << sh), c, logC)];
    auto twiddle = [&](uint32_t t, uint32_t xg) -> uint32_t {   // stage t of the pass, group xg of its 2^t
        if (!LO) return ltw[(1u << t) - 1 + xg];
        const uint32_t s = s0 + t, j = (circle_bitrev(xg, t) << s0) | col;
        return s == L - 1 ? p.twy[j] : p.twx[(1u << s) - 1 + j];
    };
    if (!INV) {
#pragma unroll
        for (int u = 0; u < K; u++) {
            const int half = 1 << (K - 1 - u);
#pragma unroll
            for (int jt = 0; jt < (1 << u); jt++) {
                const uint32_t tw = twiddle(t0 + u, (m_high << u) | (uint32_t)jt);
#pragma unroll
                for (int jl = 0; jl < half; jl++) {
                    const int j = (jt << (K - u)) | jl;
                    const uint32_t t = m31_mul(x[j + half], tw), a = x[j];
                    x[j] = m31_add(a, t);
                    x[j + half] = m31_sub(a, t);
                }
            }
        }
    } else {
#pragma unroll
        for (int u = K - 1; u >= 0; u--) {
            const int half = 1 << (K - 1 - u);
#pragma unroll
            for (int jt = 0; jt < (1 << u); jt++) {
                const uint32_t tw = twiddle(t0 + u, (m_high << u) | (uint32_t)jt);
#pragma unroll
                for (int jl = 0; jl < half; jl++) {
                    const int j = (jt << (K - u)) | jl;
                    const uint32_t a = x[j], d = x[j + half];
                    x[j] = m31_add(a, d);
                    x[j + half] = m31_mul(m31_sub(a, d), tw);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < E; j++) lds[circle_slot(mbase | ((uint32_t)j << sh), c, logC)] = x[j];
}

template <bool LO, bool INV>
__global__ __launch_bounds__(CIRCLE_THREADS) void circle_pass_kernel(CirclePassParams p) {
    __shared__ uint32_t lds[CIRCLE_TILE];
    __shared__ uint32_t ltw[LO ? 1 : 256];   // HI pass: stage t group x at slot 2^t - 1 + x (r <= 8)
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const uint32_t r = p.r, logC = p.logC, L = p.L, s0 = p.s0;
    const uint32_t total = 1u << (r + logC), rmask = (1u << r) - 1, cmask = (1u << logC) - 1, cb = L - r;
    const uint32_t *gin = p.in + (uint64_t)blockIdx.y * p.in_stride;
    uint32_t *gout = p.out + (uint64_t)blockIdx.y * p.out_stride;

    uint32_t lgS = 0, base = 0;
    if (!LO) {
        lgS = L - s0 - r;   // row stride in words
        const uint32_t lo_bits = lgS - logC;
        const uint32_t hi = b >> lo_bits;
        base = (hi << (L - s0)) + ((b & ((1u << lo_bits) - 1)) << logC);
        const uint32_t hrev = circle_bitrev(hi, s0);
        for (uint32_t i = tid; i + 1 < (1u << r); i += CIRCLE_THREADS) {
            const uint32_t t = 31 - __clz(i + 1), xg = i + 1 - (1u << t), s = s0 + t;
            ltw[i] = p.twx[(1u << s) - 1 + ((circle_bitrev(xg, t) << s0) | hrev)];   // s <= L - 2: an x-layer
        }
    }
    // (row, column, word) of tile item e on the side of the pass that faces memory `fold`-wise or plainly
    auto place = [&](uint32_t e, bool folded, uint32_t &m, uint32_t &c) -> uint32_t {
        if (!LO) {
            c = e & cmask;
            m = e >> logC;
            return base + (m << lgS) + c;
        }
        if (folded) {
            circle_fold_item(e, r, logC, m, c);
            return circle_fold_word(m, circle_column(b, c, logC, cb), r, cb);
        }
        m = e & rmask;
        c = e >> r;
        return (circle_bitrev(circle_column(b, c, logC, cb), cb) << r) | m;
    };
    for (uint32_t e = tid; e < total; e += CIRCLE_THREADS) {
        uint32_t m, c;
        const uint32_t g = place(e, LO && INV, m, c);
        lds[circle_slot(m, c, logC)] = m31_from_word(gin[g & p.in_mask]);
    }
    for (uint32_t step = 0; step < p.nsteps; step++) {
        const uint32_t k = p.k[step], t0 = p.t0[step];
        const uint32_t nitems = total >> k;
        __syncthreads();
        for (uint32_t w = tid; w < nitems; w += CIRCLE_THREADS) {
            if (k == 4) circle_item<4, LO, INV>(p, lds, ltw, w, t0, b);
            else if (k == 3) circle_item<3, LO, INV>(p, lds, ltw, w, t0, b);
            else if (k == 2) circle_item<2, LO, INV>(p, lds, ltw, w, t0, b);
            else circle_item<1, LO, INV>(p, lds, ltw, w, t0, b);
        }
    }
    __syncthreads();
    for (uint32_t e = tid; e < total; e += CIRCLE_THREADS) {
        uint32_t m, c;
        const uint32_t g = place(e, LO && !INV, m, c);
        uint32_t v = lds[circle_slot(m, c, logC)];
        if (p.sc) v = m31_mul(v, p.sc);
        if (p.canonical) v = m31_canon(v);
        gout[g] = v;
    }
}

// ---- twiddle tables, generated on the device (twiddles.rs: tw[i][j] = x((1 + 4j) g_{2^(i+3)}) below the last layer,
// y((1 + 4j) g_{2^(L+1)}) in it; none is zero)
struct CircleGens {
    uint32_t x[32], y[32];   // g_{2^k} = 2^(31-k) G
};
static CircleGens circle_gens() {
    CircleGens g;
    CirclePt q{2u, 1268011823u};   // the generator of the circle group, order 2^31 (circle/point.rs)
    for (int k = 31; k >= 0; k--) {
        g.x[k] = q.x;
        g.y[k] = q.y;
        q = circle_double(q);
    }
    return g;
}
__global__ void circle_fill_x_kernel(uint32_t *tw, uint32_t *itw, CircleGens g, uint32_t count) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    const uint32_t i = 31 - __clz(e + 1), j = e + 1 - (1u << i);
    const uint32_t v = circle_mul(1 + 4 * j, CirclePt{g.x[i + 3], g.y[i + 3]}).x;
    tw[e] = m31_canon(v);
    itw[e] = m31_canon(m31_inv(v));
}
__global__ void circle_fill_y_kernel(uint32_t *tw, uint32_t *itw, CirclePt g, uint32_t count) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const uint32_t v = circle_mul(1 + 4 * j, g).y;
    tw[j] = m31_canon(v);
    itw[j] = m31_canon(m31_inv(v));
}

// both tables a transform of 2^L words needs; the x-layers are shared by every size, the y-layer is the size's own
static int circle_ensure_twiddles(Context &c, uint32_t L, hipStream_t stream) {
    SharedState &sh = shared_state();
    int rc = LW_OK;
    if (L >= 2) {   // layers 0 .. L-2; a table for 2^Lt words holds 2^(Lt-1) - 1 of them in each half of 2^(Lt-1)
        TwiddleTable &t = sh.circle_x;
        rc = ensure_twiddle_table(c, t, L, CIRCLE_MAX_LOG, 8, stream, [&](uint32_t Lt) {
            const uint32_t half = 1u << (Lt - 1), count = half - 1;
            uint32_t *T = (uint32_t *)t.buf.p;
            hipLaunchKernelGGL(circle_fill_x_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, T, T + half, circle_gens(), count);
            return (int)LW_OK;
        });
        if (rc) return rc;
    }
    TwiddleTable &y = sh.circle_y[L];
    return ensure_twiddle_table(c, y, L, L, 8, stream, [&](uint32_t Lt) {   // two-adicity L: built for exactly this size
        const uint32_t half = 1u << (Lt - 1);
        const CircleGens g = circle_gens();
        uint32_t *T = (uint32_t *)y.buf.p;
        hipLaunchKernelGGL(circle_fill_y_kernel, dim3((half + 255) / 256), dim3(256), 0, stream, T, T + half, CirclePt{g.x[Lt + 1], g.y[Lt + 1]}, half);
        return (int)LW_OK;
    });
}

static uint32_t circle_max_r() {   // LW_HIP_CIRCLE_MAX_R (LW_HIP_TUNING only): fewer stages per pass, for the pass counts of 2^25 and up at test sizes
    const char *e = tuning_env("LW_HIP_CIRCLE_MAX_R");
    const int v = e ? atoi(e) : 0;
    return v >= 4 && v <= (int)NTT_MAX_R ? (uint32_t)v : NTT_MAX_R;
}
static int circle_passes(uint32_t L, uint32_t in_log2) {
    return plan_passes(L, L, L - in_log2, CIRCLE_TILE_LOG, CIRCLE_KMAX, false, circle_max_r()).npass;
}

// One transform of `batch` columns of 2^L words.  Evaluation reads 2^in_log2 coefficients per column (in_log2 < L: zero
// padded).  `work` holds batch x 2^L words for what lies between two passes and for the copy of an in-place single pass;
// it is only touched when there is more than one pass or d_in == d_out.  The tables must be there (circle_ensure_twiddles).
static int circle_run(Context &c, bool inv, const uint32_t *d_in, uint64_t in_stride, uint32_t in_log2, uint32_t *d_out, uint64_t out_stride,
                      uint32_t L, uint32_t batch, uint32_t *work, hipStream_t stream) {
    const SharedState &sh = shared_state();
    const uint64_t n = 1ull << L;
    const NttPlan pl = plan_passes(L, L, L - in_log2, CIRCLE_TILE_LOG, CIRCLE_KMAX, false, circle_max_r());
    const uint32_t *xt = (const uint32_t *)sh.circle_x.buf.p, *yt = (const uint32_t *)sh.circle_y[L].buf.p;
    if (inv) {
        if (xt) xt += 1ull << (sh.circle_x.log_n - 1);
        yt += n / 2;
    }
    const uint32_t *src = d_in;
    uint64_t src_stride = in_stride;
    if (pl.npass == 1 && d_in == d_out) {
        LW_HIP_CHECK(hipMemcpy2DAsync(work, n * 4, d_in, in_stride * 4, n * 4, batch, hipMemcpyDeviceToDevice, stream), LW_ERR_LAUNCH);
        src = work;
        src_stride = n;
    }
    for (int q = 0; q < pl.npass; q++) {
        const int i = inv ? pl.npass - 1 - q : q;   // interpolation: the evaluation's passes backwards
        const bool lo = i == pl.npass - 1, last = q == pl.npass - 1;
        CirclePassParams p{};
        p.in = src;
        p.in_stride = src_stride;
        p.out = last ? d_out : work;
        p.out_stride = last ? out_stride : n;
        p.twx = xt;
        p.twy = yt;
        p.L = L;
        p.s0 = pl.s0[i];
        p.r = pl.r[i];
        p.logC = pl.logC[i];
        p.nsteps = pl.nsteps[i];
        uint32_t t0 = 0;
        for (uint32_t j = 0; j < p.nsteps; j++) {   // the steps of an interpolation pass backwards too
            const uint32_t at = inv ? p.nsteps - 1 - j : j;
            p.k[at] = pl.k[i][j];
            p.t0[at] = t0;
            t0 += pl.k[i][j];
        }
        p.in_mask = (!inv && q == 0) ? (uint32_t)((1ull << in_log2) - 1) : 0xffffffffu;
        p.sc = (inv && last) ? 1u << (31 - L) : 0u;   // N^-1 = 2^-L = 2^(31-L): 2^31 = 1
        p.canonical = last ? 1u : 0u;
        const dim3 grid(1u << (L - p.r - p.logC), batch);
        hipEvent_t pe = c.prof_begin(stream);
        if (lo && inv) hipLaunchKernelGGL((circle_pass_kernel<true, true>), grid, dim3(CIRCLE_THREADS), 0, stream, p);
        else if (lo) hipLaunchKernelGGL((circle_pass_kernel<true, false>), grid, dim3(CIRCLE_THREADS), 0, stream, p);
        else if (inv) hipLaunchKernelGGL((circle_pass_kernel<false, true>), grid, dim3(CIRCLE_THREADS), 0, stream, p);
        else hipLaunchKernelGGL((circle_pass_kernel<false, false>), grid, dim3(CIRCLE_THREADS), 0, stream, p);
        c.prof_end(lo ? (inv ? "circle_pass_kernel<lo,inv>" : "circle_pass_kernel<lo>") : (inv ? "circle_pass_kernel<hi,inv>" : "circle_pass_kernel<hi>"),
                   pe, stream);
        LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
        src = p.out;
        src_stride = p.out_stride;
    }
    return LW_OK;
}

constexpr uint32_t CIRCLE_MAX_BATCH = 32768;   // grid.y carries the batch: wider ones are split

static int circle_transform_device(Context &c, bool inv, const uint32_t *d_in, uint32_t *d_out, uint32_t L, uint32_t batch, uint64_t stride,
                                   hipStream_t stream) {
    const uint64_t n = 1ull << L;
    if (!stride) stride = n;
    int rc = circle_ensure_twiddles(c, L, stream);
    if (rc) return rc;
    const uint32_t chunk = batch < CIRCLE_MAX_BATCH ? batch : CIRCLE_MAX_BATCH;
    if ((circle_passes(L, L) > 1 || d_in == d_out) && c.scratch.ensure((size_t)n * chunk * 4)) return LW_ERR_ALLOC;
    for (uint32_t b0 = 0; b0 < batch; b0 += chunk) {
        const uint32_t nb = batch - b0 < chunk ? batch - b0 : chunk;
        rc = circle_run(c, inv, d_in + b0 * stride, stride, L, d_out + b0 * stride, stride, L, nb, (uint32_t *)c.scratch.p, stream);
        if (rc) return rc;
    }
    return LW_OK;
}

// evaluate_cfft(zero_pad(interpolate_cfft(evals), 2^L_out)); the coefficients stay in the lane's scratch
static int circle_lde_device(Context &c, const uint32_t *d_evals, uint32_t Lin, uint64_t in_stride, uint32_t *d_out, uint32_t Lout,
                             uint64_t out_stride, uint32_t batch, hipStream_t stream) {
    const uint64_t nin = 1ull << Lin, nout = 1ull << Lout;
    if (!in_stride) in_stride = nin;
    if (!out_stride) out_stride = nout;
    int rc = circle_ensure_twiddles(c, Lin, stream);
    if (!rc) rc = circle_ensure_twiddles(c, Lout, stream);
    if (rc) return rc;
    const uint32_t chunk = batch < CIRCLE_MAX_BATCH ? batch : CIRCLE_MAX_BATCH;
    if (c.scratch.ensure((size_t)(nin + nout) * chunk * 4)) return LW_ERR_ALLOC;   // coefficients | what lies between two passes
    uint32_t *coeffs = (uint32_t *)c.scratch.p, *work = coeffs + nin * chunk;
    for (uint32_t b0 = 0; b0 < batch; b0 += chunk) {
        const uint32_t nb = batch - b0 < chunk ? batch - b0 : chunk;
        rc = circle_run(c, true, d_evals + b0 * in_stride, in_stride, Lin, coeffs, nin, Lin, nb, work, stream);
        if (!rc) rc = circle_run(c, false, coeffs, nin, Lin, d_out + b0 * out_stride, out_stride, Lout, nb, work, stream);
        if (rc) return rc;
    }
    return LW_OK;
}

// ---- argument checks, before any device work
static int circle_size_check(uint32_t log2n) {
    if (log2n > CIRCLE_MAX_LOG) {
        set_error("2^%u points: the standard coset needs g_{2n} in a group of order 2^31", log2n);
        return LW_ERR_ORDER_TOO_LARGE;
    }
    if (log2n == 0) { set_error("a circle transform has at least 2 points"); return LW_ERR_BAD_ARG; }
    return LW_OK;
}
static bool circle_overlap(const void *a, size_t a_words, const void *b, size_t b_words) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_words * 4 && b0 < a0 + a_words * 4;
}
static int circle_check(const void *in, const void *out, uint32_t log2n, uint32_t batch, size_t stride) {
    const int rc = circle_size_check(log2n);
    if (rc) return rc;
    const size_t n = (size_t)1 << log2n;
    if (!in || !out || batch == 0) { set_error("null buffer or empty batch"); return LW_ERR_BAD_ARG; }
    if (stride != 0 && stride < n) { set_error("batch stride %zu < transform length", stride); return LW_ERR_BAD_ARG; }
    const size_t span = (size_t)(batch - 1) * (stride ? stride : n) + n;
    if (in != out && circle_overlap(in, span, out, span)) { set_error("in and out overlap without being the same buffer"); return LW_ERR_BAD_ARG; }
    return LW_OK;
}

}  // namespace lw

using namespace lw;

extern "C" {

static int circle_device_entry(bool inv, const uint32_t *d_in, uint32_t *d_out, uint32_t log2n, uint32_t batch, size_t stride, void *hip_stream) {
    const int rc = circle_check(d_in, d_out, log2n, batch, stride);
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return circle_transform_device(en.c, inv, d_in, d_out, log2n, batch, stride, en.stream);
}
int lw_circle_evaluate_cfft_device(const uint32_t *d_in, uint32_t *d_out, uint32_t log2n, uint32_t batch, size_t batch_stride, void *hip_stream) {
    return circle_device_entry(false, d_in, d_out, log2n, batch, batch_stride, hip_stream);
}
int lw_circle_interpolate_cfft_device(const uint32_t *d_in, uint32_t *d_out, uint32_t log2n, uint32_t batch, size_t batch_stride,
                                      void *hip_stream) {
    return circle_device_entry(true, d_in, d_out, log2n, batch, batch_stride, hip_stream);
}

static int circle_host_entry(bool inv, const uint32_t *in, uint32_t *out, uint32_t log2n, uint32_t batch, size_t stride) {
    int rc = circle_check(in, out, log2n, batch, stride);
    if (rc) return rc;
    Entry en(nullptr);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t io = en.use_lane_stream();
    if (!io) return en.rc;
    const size_t n = (size_t)1 << log2n;
    if (!stride) stride = n;
    const size_t span = ((size_t)(batch - 1) * stride + n) * 4;
    if (c.host_io_a.ensure(span) || c.host_io_b.ensure(span)) return LW_ERR_ALLOC;
    LW_HIP_CHECK(hipMemcpyAsync(c.host_io_a.p, in, span, hipMemcpyHostToDevice, io), LW_ERR_LAUNCH);
    rc = circle_transform_device(c, inv, (const uint32_t *)c.host_io_a.p, (uint32_t *)c.host_io_b.p, log2n, batch, stride, io);
    if (rc) return rc;
    // column by column: the words between strided columns stay as they are
    LW_HIP_CHECK(hipMemcpy2DAsync(out, stride * 4, c.host_io_b.p, stride * 4, n * 4, batch, hipMemcpyDeviceToHost, io), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(io), LW_ERR_LAUNCH);
    return LW_OK;
}
int lw_circle_evaluate_cfft(const uint32_t *coeffs, uint32_t *out, uint32_t log2n, uint32_t batch, size_t batch_stride) {
    return circle_host_entry(false, coeffs, out, log2n, batch, batch_stride);
}
int lw_circle_interpolate_cfft(const uint32_t *evals, uint32_t *out, uint32_t log2n, uint32_t batch, size_t batch_stride) {
    return circle_host_entry(true, evals, out, log2n, batch, batch_stride);
}

int lw_circle_lde_device(const uint32_t *d_evals, uint32_t log2_in, size_t in_stride, uint32_t *d_out, uint32_t log2_out, size_t out_stride,
                         uint32_t batch, void *hip_stream) {
    int rc = circle_size_check(log2_out);
    if (!rc) rc = circle_size_check(log2_in);
    if (rc) return rc;
    if (log2_out < log2_in) { set_error("2^%u evaluations do not fit a 2^%u domain", log2_in, log2_out); return LW_ERR_BAD_ARG; }
    const size_t nin = (size_t)1 << log2_in, nout = (size_t)1 << log2_out;
    if (!d_evals || !d_out || batch == 0) { set_error("null buffer or empty batch"); return LW_ERR_BAD_ARG; }
    if ((in_stride != 0 && in_stride < nin) || (out_stride != 0 && out_stride < nout)) { set_error("batch stride < transform length"); return LW_ERR_BAD_ARG; }
    if (d_evals != d_out && circle_overlap(d_evals, (size_t)(batch - 1) * (in_stride ? in_stride : nin) + nin, d_out,
                                           (size_t)(batch - 1) * (out_stride ? out_stride : nout) + nout)) {
        set_error("evals and out overlap without being the same buffer");
        return LW_ERR_BAD_ARG;
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return circle_lde_device(en.c, d_evals, log2_in, in_stride, d_out, log2_out, out_stride, batch, en.stream);
}

// get_twiddles(Coset::new_standard(log2n), config): the layers concatenated, n - 1 words.  Evaluation: lengths 1, 2, .., n/2;
// interpolation: the inverses, lengths n/2, .., 1.
int lw_circle_get_twiddles(uint32_t log2n, int config, uint32_t *out) {
    const int rc0 = circle_size_check(log2n);
    if (rc0) return rc0;
    if (!out) { set_error("null buffer"); return LW_ERR_BAD_ARG; }
    if (config != 0 && config != 1) { set_error("bad twiddle config %d", config); return LW_ERR_BAD_ARG; }
    Entry en(nullptr);
    if (en.rc) return en.rc;
    hipStream_t io = en.use_lane_stream();
    if (!io) return en.rc;
    const int rc = circle_ensure_twiddles(en.c, log2n, io);
    if (rc) return rc;
    const SharedState &sh = shared_state();
    const size_t half = (size_t)1 << (log2n - 1);
    const uint32_t *yt = (const uint32_t *)sh.circle_y[log2n].buf.p, *xt = (const uint32_t *)sh.circle_x.buf.p;
    if (config == 0) {
        if (half > 1) LW_HIP_CHECK(hipMemcpyAsync(out, xt, (half - 1) * 4, hipMemcpyDeviceToHost, io), LW_ERR_LAUNCH);
        LW_HIP_CHECK(hipMemcpyAsync(out + half - 1, yt, half * 4, hipMemcpyDeviceToHost, io), LW_ERR_LAUNCH);
    } else {
        LW_HIP_CHECK(hipMemcpyAsync(out, yt + half, half * 4, hipMemcpyDeviceToHost, io), LW_ERR_LAUNCH);
        uint32_t *dst = out + half;
        for (int i = (int)log2n - 2; i >= 0; i--) {
            const size_t len = (size_t)1 << i;
            const uint32_t *ixt = xt + ((size_t)1 << (sh.circle_x.log_n - 1));
            LW_HIP_CHECK(hipMemcpyAsync(dst, ixt + len - 1, len * 4, hipMemcpyDeviceToHost, io), LW_ERR_LAUNCH);
            dst += len;
        }
    }
    LW_HIP_CHECK(hipStreamSynchronize(io), LW_ERR_LAUNCH);
    return LW_OK;
}

}  // extern "C"
