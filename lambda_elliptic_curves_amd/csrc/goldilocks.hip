// NTT over Goldilocks (p = 2^64 - 2^32 + 1) on gfx950: evaluate_fft / interpolate_fft and their coset forms
// (math/src/fft/polynomial.rs:25-127) for U64TestField (u64_test_field.rs:98-104) and Winterfell's Felt (winterfell.rs:21-24),
// the low-degree extension and the pointwise product.  One u64 per element, the residue itself (goldilocks.cuh).
//
// Dataflow.  NR-DIT with bit-reversed twiddles as in ntt_bb.hip (math/src/fft/cpu/fft.rs:20-55 + bit_reversing.rs:2-18): the
// input is read in natural order, stage s pairs the words whose index differs in bit L-1-s with the twiddle T[index >> (L-s)],
// T[g] = w^bitrev(g), and the bit reversal of the result is folded into the last pass's stores.  The inverse transform is the
// same passes over the table of w^-1; N^-1 (and h^-i of a coset) rides on the last store.
//
// Passes.  2^L words take ceil(L / 8) passes (plan_passes), each a tile of 2^r rows x 2^logC columns of u64 in LDS
// (2^12 words = 32 KiB: four workgroups per CU; 2^13 would leave two):
//   non-last pass: rows are the index bits [L-s0-r, L-s0), columns lower bits.  A tile reads and writes runs of 2^logC
//                  consecutive words and shares the 2^r - 1 twiddles of its stages, staged in LDS.
//   last pass:     rows are the index bits [0, r): a column is 2^r consecutive words of the source, and with the columns
//                  chosen as bitrev(c) the stores of one row are 2^logC consecutive words of the natural-order result.
//                  LDS slots are XOR-swizzled by row; work-items walk rows fastest so that a wave's twiddles are neighbours.
// Register steps are radix 16 at most (32 VGPRs of data).  Every value in LDS, in registers and between two passes is canonical.
#include <stdlib.h>
#include "internal.h"
#include "goldilocks.cuh"
#include "ntt_plan.h"

namespace lw {

constexpr int GL_TILE_LOG = 12;   // 4096 u64 = 32 KiB of LDS
constexpr int GL_TILE = 1 << GL_TILE_LOG;
constexpr int GL_THREADS = 256;
constexpr int GL_KMAX = 4;        // radix-16 register steps
constexpr uint32_t GL_MAX_LOG = 30;   // 32-bit word indices and a table of 2^(L-1) entries

struct GlPassParams {
    const uint64_t *in;
    uint64_t *out;
    const uint64_t *tw;               // T[g] = w^bitrev(g)
    uint64_t in_stride, out_stride;   // words between the columns of a batch
    uint32_t L, s0, r, logC;
    uint32_t nsteps, k[4], t0[4];     // register steps: stages t0 .. t0 + k - 1 of the pass
    // low-degree extension (first pass): word g of the zero-padded coefficients is in[g & in_mask] — the stages that only
    // pair data with padding leave the block replicated and are skipped (s0 starts behind them)
    uint32_t in_mask;
    // coset: element i is multiplied by lo[i & mask] * hi[i >> hbits] = h^i while the first pass loads it (cos_in), or by
    // h^-i * N^-1 while the last pass stores it (cos_out, N^-1 folded into hi)
    const uint64_t *cos_lo, *cos_hi;
    uint32_t cos_hbits, cos_in, cos_out;
    uint64_t sc;                      // != 0: the store multiplies by it (N^-1 of an inverse without offset)
};

__device__ __forceinline__ uint32_t gl_bitrev(uint32_t x, uint32_t bits) { return bits ? (__brev(x) >> (32 - bits)) : 0u; }
__device__ __forceinline__ uint32_t gl_slot(uint32_t m, uint32_t c, uint32_t logC) {
    return (m << logC) | (c ^ ((m ^ (m >> 4)) & ((1u << logC) - 1)));
}
__device__ __forceinline__ uint64_t gl_coset_factor(const GlPassParams &p, uint32_t i) {
    return gl_mul(p.cos_lo[i & ((1u << p.cos_hbits) - 1)], p.cos_hi[i >> p.cos_hbits]);
}
// last pass: the index bits above the rows of tile column c of block b
__device__ __forceinline__ uint32_t gl_column_high(uint32_t b, uint32_t c, uint32_t logC, uint32_t hb) {
    return (gl_bitrev(c, logC) << (hb - logC)) | gl_bitrev(b, hb - logC);
}

template <int K, bool LAST>
__device__ __forceinline__ void gl_item(const GlPassParams &p, uint64_t *lds, const uint64_t *ltw, uint32_t w, uint32_t t0, uint32_t b) {
    constexpr int E = 1 << K;
    const uint32_t r = p.r, logC = p.logC, L = p.L;
    uint32_t c, mr;
    if (LAST) {   // rows fastest
        mr = w & ((1u << (r - K)) - 1);
        c = w >> (r - K);
    } else {
        c = w & ((1u << logC) - 1);
        mr = w >> logC;
    }
    const uint32_t sh = r - t0 - K;
    const uint32_t m_high = mr >> sh;
    const uint32_t mbase = (m_high << (sh + K)) | (mr & ((1u << sh) - 1));
    const uint32_t hi_c = LAST ? gl_column_high(b, c, logC, L - r) : 0u;
    uint64_t x[E];
#pragma unroll
    for (int j = 0; j < E; j++) x[j] = lds[gl_slot(mbase | ((uint32_t)j << sh), c, logC)];
#pragma unroll
    for (int u = 0; u < K; u++) {
        const int half = 1 << (K - 1 - u);
        const uint32_t t = t0 + u;
#pragma unroll
        for (int jt = 0; jt < (1 << u); jt++) {
            const uint32_t xg = (m_high << u) | (uint32_t)jt;   // group of stage t inside the tile
            const uint64_t tw = LAST ? p.tw[(hi_c << t) | xg] : ltw[(1u << t) - 1 + xg];
#pragma unroll
            for (int jl = 0; jl < half; jl++) {
                const int j = (jt << (K - u)) | jl;
                const uint64_t v = gl_mul(x[j + half], tw), a = x[j];
                x[j] = gl_add(a, v);
                x[j + half] = gl_sub(a, v);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < E; j++) lds[gl_slot(mbase | ((uint32_t)j << sh), c, logC)] = x[j];
}

template <bool LAST>
__global__ __launch_bounds__(GL_THREADS) void gl_pass_kernel(GlPassParams p) {
    __shared__ uint64_t lds[GL_TILE];
    __shared__ uint64_t ltw[LAST ? 1 : 256];   // non-last pass: stage t group x at slot 2^t - 1 + x (r <= 8)
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const uint32_t r = p.r, logC = p.logC, L = p.L, s0 = p.s0;
    const uint32_t total = 1u << (r + logC), rmask = (1u << r) - 1, cmask = (1u << logC) - 1;
    const uint64_t *gin = p.in + (uint64_t)blockIdx.y * p.in_stride;
    uint64_t *gout = p.out + (uint64_t)blockIdx.y * p.out_stride;

    uint32_t lgS = 0, base = 0;
    if (!LAST) {
        lgS = L - s0 - r;   // row stride in words
        const uint32_t lo_bits = lgS - logC;
        const uint32_t hi = b >> lo_bits;
        base = (hi << (L - s0)) + ((b & ((1u << lo_bits) - 1)) << logC);
        for (uint32_t i = tid; i + 1 < (1u << r); i += GL_THREADS) {
            const uint32_t t = 31 - __clz(i + 1), xg = i + 1 - (1u << t);
            ltw[i] = p.tw[(hi << t) | xg];
        }
    }
    for (uint32_t e = tid; e < total; e += GL_THREADS) {
        uint32_t m, c, g;
        if (LAST) {   // a column is 2^r consecutive words
            m = e & rmask;
            c = e >> r;
            g = (gl_column_high(b, c, logC, L - r) << r) | m;
        } else {
            c = e & cmask;
            m = e >> logC;
            g = base + (m << lgS) + c;
        }
        g &= p.in_mask;
        uint64_t v = gl_from_word(gin[g]);
        if (p.cos_in) v = gl_mul(v, gl_coset_factor(p, g));   // c_i h^i
        lds[gl_slot(m, c, logC)] = v;
    }
    for (uint32_t step = 0; step < p.nsteps; step++) {
        const uint32_t k = p.k[step], t0 = p.t0[step];
        const uint32_t nitems = total >> k;
        __syncthreads();
        for (uint32_t w = tid; w < nitems; w += GL_THREADS) {
            if (k == 4) gl_item<4, LAST>(p, lds, ltw, w, t0, b);
            else if (k == 3) gl_item<3, LAST>(p, lds, ltw, w, t0, b);
            else if (k == 2) gl_item<2, LAST>(p, lds, ltw, w, t0, b);
            else gl_item<1, LAST>(p, lds, ltw, w, t0, b);
        }
    }
    __syncthreads();
    for (uint32_t e = tid; e < total; e += GL_THREADS) {
        const uint32_t c = e & cmask, m = e >> logC;
        uint32_t g;
        if (LAST) g = (gl_bitrev(m, r) << (L - r)) + (b << logC) + c;   // the natural-order index of word (column, row)
        else g = base + (m << lgS) + c;
        uint64_t v = lds[gl_slot(m, c, logC)];
        if (p.cos_out) v = gl_mul(v, gl_coset_factor(p, g));   // h^-i N^-1
        else if (p.sc) v = gl_mul(v, p.sc);
        gout[g] = v;
    }
}

__global__ void gl_twiddle_fill_kernel(uint64_t *tw, uint64_t root, uint32_t bits, uint32_t count) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    tw[g] = gl_pow(root, gl_bitrev(g, bits));
}
// two-level power tables of a coset offset: lo[j] = h^j (j < 2^hbits), hi[j] = scale * h^(j << hbits) (j < n_hi)
__global__ void gl_power_tables_kernel(uint64_t *lo, uint64_t *hi, uint64_t h, uint32_t hbits, uint32_t n_hi, uint64_t scale) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < (1u << hbits)) lo[t] = gl_pow(h, t);
    if (t < n_hi) hi[t] = gl_mul(scale, gl_pow(h, (uint64_t)t << hbits));
}
// get_twiddles: out[i] = root^i or root^bitrev(i)
__global__ void gl_powers_kernel(uint64_t *out, uint64_t root, uint32_t bitrev_bits, uint32_t natural, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    out[i] = gl_pow(root, natural ? i : gl_bitrev(i, bitrev_bits));
}
__global__ void gl_mul_kernel(const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t n) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) out[i] = gl_mul(a[i], b[i]);
}

// ---------------------------------------------------------------- host
// the primitive 2^order-th root g^(2^(32 - order)) (traits.rs:82-94) of the 2^32-th root g, or its inverse
static uint64_t gl_host_root(uint64_t g, uint32_t order, bool inverse) {
    for (uint32_t i = order; i < GL_TWO_ADICITY; i++) g = gl_mul(g, g);
    return inverse ? gl_inv(g) : g;
}

// The table of direction `inv` for transforms of up to 2^L words under the 2^32-th root g.  The cache holds one root: with
// another one both directions are dropped first, under the exclusive hold that every rebuild of a shared table takes.
static int gl_ensure_twiddles(Context &c, bool inv, uint32_t L, uint64_t g, hipStream_t stream) {
    if (L < 1) return LW_OK;
    SharedState &sh = shared_state();
    TwiddleTable &t = sh.goldilocks[inv ? 1 : 0];
    constexpr int RETRY = 1;   // another lane changed the root while this one waited for the exclusive hold
    for (;;) {
        if (sh.goldilocks_root == g && t.valid && t.log_n >= L) return LW_OK;
        if (sh.goldilocks_root != g) {
            ExclusiveScope excl(c);
            if (sh.goldilocks_root != g) {
                (void)hipDeviceSynchronize();   // the tables are refilled in place: transforms still in flight read them
                sh.goldilocks[0].valid = sh.goldilocks[1].valid = false;
                sh.goldilocks_root = g;
            }
        }
        const int rc = ensure_twiddle_table(c, t, L, GL_MAX_LOG, 8, stream, [&](uint32_t Lt) {
            if (sh.goldilocks_root != g) return RETRY;
            const uint32_t count = 1u << (Lt - 1);
            hipLaunchKernelGGL(gl_twiddle_fill_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, (uint64_t *)t.buf.p,
                               gl_host_root(g, Lt, inv), Lt - 1, count);
            return (int)LW_OK;
        });
        if (rc != LW_OK && rc != RETRY) return rc;
    }
}

static uint32_t gl_max_r() {   // LW_HIP_GOLDILOCKS_MAX_R (LW_HIP_TUNING only): fewer stages per pass, for the pass counts of 2^17 and up at test sizes
    const char *e = tuning_env("LW_HIP_GOLDILOCKS_MAX_R");
    const int v = e ? atoi(e) : 0;
    return v >= 4 && v <= (int)NTT_MAX_R ? (uint32_t)v : NTT_MAX_R;
}

struct GlCall {
    bool inv;
    uint64_t root;      // the 2^32-th root, validated
    bool coset;
    uint64_t h;         // the offset mod p, not zero
};

// One transform of `batch` columns of 2^L words; the forward one reads 2^in_log2 coefficients per column (in_log2 < L:
// zero padded).  `work` holds batch x 2^L words for what lies between two passes and for the copy of an in-place single
// pass; it is only touched when there is more than one pass or d_in == d_out.  cos_lo / cos_hi: the call's power tables.
static int gl_run(Context &c, const GlCall &call, const uint64_t *d_in, uint64_t in_stride, uint32_t in_log2, uint64_t *d_out,
                  uint64_t out_stride, uint32_t L, uint32_t batch, uint64_t *work, const uint64_t *cos_lo, const uint64_t *cos_hi,
                  uint32_t cos_hbits, hipStream_t stream) {
    const SharedState &sh = shared_state();
    const uint64_t n = 1ull << L;
    const NttPlan pl = plan_passes(L, L, L - in_log2, GL_TILE_LOG, GL_KMAX, false, gl_max_r());
    const uint64_t *src = d_in;
    uint64_t src_stride = in_stride;
    if (pl.npass == 1 && d_in == d_out) {
        LW_HIP_CHECK(hipMemcpy2DAsync(work, n * 8, d_in, in_stride * 8, n * 8, batch, hipMemcpyDeviceToDevice, stream), LW_ERR_LAUNCH);
        src = work;
        src_stride = n;
    }
    for (int i = 0; i < pl.npass; i++) {
        const bool last = i == pl.npass - 1;
        GlPassParams p{};
        p.in = src;
        p.in_stride = src_stride;
        p.out = last ? d_out : work;
        p.out_stride = last ? out_stride : n;
        p.tw = (const uint64_t *)sh.goldilocks[call.inv ? 1 : 0].buf.p;
        p.L = L;
        p.s0 = pl.s0[i];
        p.r = pl.r[i];
        p.logC = pl.logC[i];
        p.nsteps = pl.nsteps[i];
        uint32_t t0 = 0;
        for (uint32_t j = 0; j < p.nsteps; j++) {
            p.k[j] = pl.k[i][j];
            p.t0[j] = t0;
            t0 += pl.k[i][j];
        }
        p.in_mask = i == 0 ? (uint32_t)((1ull << in_log2) - 1) : 0xffffffffu;
        p.cos_lo = cos_lo;
        p.cos_hi = cos_hi;
        p.cos_hbits = cos_hbits;
        p.cos_in = (call.coset && !call.inv && i == 0) ? 1u : 0u;
        p.cos_out = (call.coset && call.inv && last) ? 1u : 0u;
        p.sc = (call.inv && last && !call.coset && L > 0) ? gl_inv(n) : 0u;   // with an offset N^-1 rides in the hi table
        const dim3 grid(1u << (L - p.r - p.logC), batch);
        hipEvent_t pe = c.prof_begin(stream);
        if (last) hipLaunchKernelGGL((gl_pass_kernel<true>), grid, dim3(GL_THREADS), 0, stream, p);
        else hipLaunchKernelGGL((gl_pass_kernel<false>), grid, dim3(GL_THREADS), 0, stream, p);
        c.prof_end(last ? "gl_pass_kernel<last>" : "gl_pass_kernel", pe, stream);
        LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
        src = p.out;
        src_stride = p.out_stride;
    }
    return LW_OK;
}

constexpr uint32_t GL_MAX_BATCH = 32768;   // grid.y carries the batch: wider ones are split

// forward / inverse / low-degree extension (forward, in_log2 < L) of `batch` columns
static int gl_transform_device(Context &c, const GlCall &call, const uint64_t *d_in, uint64_t in_stride, uint32_t in_log2, uint64_t *d_out,
                               uint64_t out_stride, uint32_t L, uint32_t batch, hipStream_t stream) {
    const uint64_t n = 1ull << L, nin = 1ull << in_log2;
    if (!in_stride) in_stride = nin;
    if (!out_stride) out_stride = n;
    int rc = gl_ensure_twiddles(c, call.inv, L, call.root, stream);
    if (rc) return rc;
    // coset factors: h^i over the 2^in_log2 coefficients (the padding comes after Polynomial::scale), h^-i N^-1 over the result
    const uint32_t cos_hbits = in_log2 < 12 ? in_log2 : 12, cos_nhi = 1u << (in_log2 - cos_hbits);
    uint64_t *cos_lo = nullptr, *cos_hi = nullptr;
    if (call.coset) {
        if (c.gl_coset.ensure(8 * ((size_t)(1u << cos_hbits) + cos_nhi))) return LW_ERR_ALLOC;
        cos_lo = (uint64_t *)c.gl_coset.p;
        cos_hi = cos_lo + (1u << cos_hbits);
        const uint32_t cnt = (1u << cos_hbits) > cos_nhi ? (1u << cos_hbits) : cos_nhi;
        hipLaunchKernelGGL(gl_power_tables_kernel, dim3((cnt + 255) / 256), dim3(256), 0, stream, cos_lo, cos_hi,
                           call.inv ? gl_inv(call.h) : call.h, cos_hbits, cos_nhi, call.inv ? gl_inv(n) : 1ull);
        LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    }
    const uint32_t chunk = batch < GL_MAX_BATCH ? batch : GL_MAX_BATCH;
    const int npass = plan_passes(L, L, L - in_log2, GL_TILE_LOG, GL_KMAX, false, gl_max_r()).npass;
    uint64_t *work = nullptr;
    if (npass > 1 || d_in == d_out) {
        if (c.scratch.ensure((size_t)n * chunk * 8)) return LW_ERR_ALLOC;
        work = (uint64_t *)c.scratch.p;
    }
    for (uint32_t b0 = 0; b0 < batch; b0 += chunk) {
        const uint32_t nb = batch - b0 < chunk ? batch - b0 : chunk;
        rc = gl_run(c, call, d_in + b0 * in_stride, in_stride, in_log2, d_out + b0 * out_stride, out_stride, L, nb, work, cos_lo, cos_hi,
                    cos_hbits, stream);
        if (rc) return rc;
    }
    return LW_OK;
}

// ---- argument checks, before any device work
static int gl_size_check(uint64_t log2n) {
    if (log2n > GL_TWO_ADICITY) {
        set_error("order %llu exceeds the field's two-adicity 32", (unsigned long long)log2n);
        return LW_ERR_ROOT_OF_UNITY;
    }
    if (log2n > GL_MAX_LOG) {
        set_error("2^%llu points: this library indexes words with 32 bits and tables 2^(n-1) twiddles, 2^30 is its limit", (unsigned long long)log2n);
        return LW_ERR_ORDER_TOO_LARGE;
    }
    return LW_OK;
}
static int gl_root_check(uint64_t &root) {
    if (root == 0) { root = GL_TWO_ADIC_ROOT; return LW_OK; }
    uint64_t v = root;
    for (int i = 0; i < 31; i++) v = gl_mul(v, v);
    if (root >= GL_P || v != GL_P - 1) {
        set_error("two_adic_root %llu is not a primitive 2^32-th root of unity below p", (unsigned long long)root);
        return LW_ERR_ROOT_OF_UNITY;
    }
    return LW_OK;
}
static int gl_offset_check(const uint64_t *offset_or_null, GlCall &call) {
    call.coset = offset_or_null != nullptr;
    call.h = call.coset ? gl_from_word(*offset_or_null) : 1;
    if (call.coset && call.h == 0) { set_error("coset offset is zero"); return LW_ERR_INV_ZERO; }
    return LW_OK;
}
static bool gl_overlap(const void *a, size_t a_words, const void *b, size_t b_words) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_words * 8 && b0 < a0 + a_words * 8;
}
static int gl_check(int dir, const void *in, const void *out, uint32_t log2n, uint32_t batch, size_t stride, const uint64_t *offset_or_null,
                    uint64_t root, GlCall &call) {
    int rc = gl_size_check(log2n);
    if (rc) return rc;
    if (dir != LW_DIR_FORWARD && dir != LW_DIR_INVERSE) { set_error("bad direction %d", dir); return LW_ERR_BAD_ARG; }
    const size_t n = (size_t)1 << log2n;
    if (!in || !out || batch == 0) { set_error("null buffer or empty batch"); return LW_ERR_BAD_ARG; }
    if (stride != 0 && stride < n) { set_error("batch stride %zu < transform length", stride); return LW_ERR_BAD_ARG; }
    const size_t span = (size_t)(batch - 1) * (stride ? stride : n) + n;
    if (in != out && gl_overlap(in, span, out, span)) { set_error("in and out overlap without being the same buffer"); return LW_ERR_BAD_ARG; }
    call.inv = dir == LW_DIR_INVERSE;
    call.root = root;
    rc = gl_root_check(call.root);
    if (rc) return rc;
    return gl_offset_check(offset_or_null, call);
}

}  // namespace lw

using namespace lw;

extern "C" {

int lw_goldilocks_ntt_device(lw_dir_t dir, const uint64_t *d_in, uint64_t *d_out, uint32_t log2n, uint32_t batch, size_t batch_stride,
                             const uint64_t *offset_or_null, uint64_t two_adic_root, void *hip_stream) {
    GlCall call{};
    const int rc = gl_check((int)dir, d_in, d_out, log2n, batch, batch_stride, offset_or_null, two_adic_root, call);
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return gl_transform_device(en.c, call, d_in, batch_stride, log2n, d_out, batch_stride, log2n, batch, en.stream);
}

int lw_goldilocks_ntt(lw_dir_t dir, const uint64_t *in, uint64_t *out, uint32_t log2n, uint32_t batch, size_t batch_stride,
                      const uint64_t *offset_or_null, uint64_t two_adic_root) {
    GlCall call{};
    int rc = gl_check((int)dir, in, out, log2n, batch, batch_stride, offset_or_null, two_adic_root, call);
    if (rc) return rc;
    Entry en(nullptr);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t io = en.use_lane_stream();
    if (!io) return en.rc;
    const size_t n = (size_t)1 << log2n;
    const size_t stride = batch_stride ? batch_stride : n;
    const size_t span = ((size_t)(batch - 1) * stride + n) * 8;
    if (c.host_io_a.ensure(span) || c.host_io_b.ensure(span)) return LW_ERR_ALLOC;
    LW_HIP_CHECK(hipMemcpyAsync(c.host_io_a.p, in, span, hipMemcpyHostToDevice, io), LW_ERR_LAUNCH);
    rc = gl_transform_device(c, call, (const uint64_t *)c.host_io_a.p, stride, log2n, (uint64_t *)c.host_io_b.p, stride, log2n, batch, io);
    if (rc) return rc;
    // column by column: the words between strided columns stay as they are
    LW_HIP_CHECK(hipMemcpy2DAsync(out, stride * 8, c.host_io_b.p, stride * 8, n * 8, batch, hipMemcpyDeviceToHost, io), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(io), LW_ERR_LAUNCH);
    return LW_OK;
}

int lw_goldilocks_lde_device(const uint64_t *d_coeffs, uint32_t log2_coeffs, size_t in_stride, uint64_t *d_out, uint32_t log2n,
                             size_t out_stride, uint32_t batch, const uint64_t *offset_or_null, uint64_t two_adic_root, void *hip_stream) {
    int rc = gl_size_check(log2n);
    if (rc) return rc;
    if (log2_coeffs > log2n) { set_error("2^%u coefficients do not fit a 2^%u domain", log2_coeffs, log2n); return LW_ERR_BAD_ARG; }
    const size_t nin = (size_t)1 << log2_coeffs, nout = (size_t)1 << log2n;
    if (!d_coeffs || !d_out || batch == 0) { set_error("null buffer or empty batch"); return LW_ERR_BAD_ARG; }
    if ((in_stride != 0 && in_stride < nin) || (out_stride != 0 && out_stride < nout)) { set_error("batch stride < column length"); return LW_ERR_BAD_ARG; }
    if (gl_overlap(d_coeffs, (size_t)(batch - 1) * (in_stride ? in_stride : nin) + nin, d_out,
                   (size_t)(batch - 1) * (out_stride ? out_stride : nout) + nout)) {
        set_error("coefficients and out overlap");
        return LW_ERR_BAD_ARG;
    }
    GlCall call{};
    call.inv = false;
    call.root = two_adic_root;
    rc = gl_root_check(call.root);
    if (!rc) rc = gl_offset_check(offset_or_null, call);
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return gl_transform_device(en.c, call, d_coeffs, in_stride, log2_coeffs, d_out, out_stride, log2n, batch, en.stream);
}

int lw_goldilocks_gen_twiddles(uint64_t order, int config, uint64_t two_adic_root, uint64_t *out) {
    int rc = gl_size_check(order);
    if (rc) return rc;
    if (config < 0 || config > 3) { set_error("bad twiddle config %d", config); return LW_ERR_BAD_ARG; }
    if (!out && order > 0) { set_error("null buffer"); return LW_ERR_BAD_ARG; }
    rc = gl_root_check(two_adic_root);
    if (rc) return rc;
    Entry en(nullptr);
    if (en.rc) return en.rc;
    if (order == 0) return LW_OK;   // 2^0 / 2 = no words
    hipStream_t io = en.use_lane_stream();
    if (!io) return en.rc;
    const uint32_t count = 1u << (order - 1);
    if (en.c.scratch.ensure((size_t)count * 8)) return LW_ERR_ALLOC;
    // RootsConfig: 0 Natural, 1 NaturalInversed, 2 BitReverse, 3 BitReverseInversed
    hipLaunchKernelGGL(gl_powers_kernel, dim3((count + 255) / 256), dim3(256), 0, io, (uint64_t *)en.c.scratch.p,
                       gl_host_root(two_adic_root, (uint32_t)order, (config & 1) != 0), (uint32_t)order - 1, config < 2 ? 1u : 0u, count);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipMemcpyAsync(out, en.c.scratch.p, (size_t)count * 8, hipMemcpyDeviceToHost, io), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(io), LW_ERR_LAUNCH);
    return LW_OK;
}

int lw_goldilocks_mul_device(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t n, void *hip_stream) {
    if (!d_a || !d_b || !d_out) { set_error("null buffer"); return LW_ERR_BAD_ARG; }
    if ((d_out != d_a && gl_overlap(d_out, n, d_a, n)) || (d_out != d_b && gl_overlap(d_out, n, d_b, n))) {
        set_error("out overlaps an operand without being the same buffer");
        return LW_ERR_BAD_ARG;
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    if (n == 0) return LW_OK;
    const uint64_t blocks = (n + 255) / 256;
    hipEvent_t pe = en.c.prof_begin(en.stream);
    hipLaunchKernelGGL(gl_mul_kernel, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, en.stream, d_a, d_b, d_out, (uint64_t)n);
    en.c.prof_end("gl_mul_kernel", pe, en.stream);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}

}  // extern "C"
