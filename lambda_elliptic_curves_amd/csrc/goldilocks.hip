// NTT over Goldilocks (p = 2^64 - 2^32 + 1) on gfx950: evaluate_fft / interpolate_fft and their coset forms
// (math/src/fft/polynomial.rs:25-127) for U64TestField (u64_test_field.rs:98-104) and Winterfell's Felt (winterfell.rs:21-24),
// the low-degree extension and the pointwise product.  One u64 per element, the residue itself (goldilocks.cuh).
//
// Dataflow.  NR-DIT with bit-reversed twiddles as in ntt_bb.hip (math/src/fft/cpu/fft.rs:20-55 + bit_reversing.rs:2-18): the
// input is read in natural order, stage s pairs the words whose index differs in bit L-1-s with the twiddle T[index >> (L-s)],
// T[g] = w^bitrev(g), and the bit reversal of the result is folded into the last pass's stores.  The inverse transform is the
// same passes over the table of w^-1; N^-1 (and h^-i of a coset) rides on the last store.
//
// The passes themselves are tile_pass.cuh; GoldilocksPolicy below is this field's side of them.  In the last pass the
// columns of a tile are chosen as bitrev(c), so that the stores of one row are 2^logC consecutive words of the natural-order
// result; its work-items walk rows fastest so that a wave's twiddles are neighbours.
// Register steps are radix 16 at most (32 VGPRs of data).  Every value in LDS, in registers and between two passes is canonical.
#include "goldilocks.cuh"
#include "tile_pass.cuh"

namespace lw {

constexpr uint32_t GL_MAX_LOG = 30;   // 32-bit word indices and a table of 2^(L-1) entries

struct GoldilocksPolicy {
    typedef uint64_t word;
    static constexpr int TILE_LOG = 12;   // 4096 u64 = 32 KiB of LDS
    static constexpr bool LAST_ROWS_FASTEST = true;
    static constexpr const char *MAX_R_ENV = "LW_HIP_GOLDILOCKS_MAX_R";
    struct Fields {
        const uint64_t *tw;   // T[g] = w^bitrev(g)
        // coset: element i is multiplied by lo[i & mask] * hi[i >> hbits] = h^i while the first pass loads it (cos_in), or by
        // h^-i * N^-1 while the last pass stores it (cos_out, N^-1 folded into hi)
        const uint64_t *cos_lo, *cos_hi;
        uint32_t cos_hbits, cos_in, cos_out;
        uint64_t sc;          // != 0: the store multiplies by it (N^-1 of an inverse without offset)
    };
    typedef TilePassParams<GoldilocksPolicy> Params;

    static __device__ __forceinline__ uint64_t add(uint64_t a, uint64_t b) { return gl_add(a, b); }
    static __device__ __forceinline__ uint64_t sub(uint64_t a, uint64_t b) { return gl_sub(a, b); }
    static __device__ __forceinline__ uint64_t mul(uint64_t a, uint64_t b) { return gl_mul(a, b); }

    // last pass: the index bits above the rows of tile column c of block b
    static __device__ __forceinline__ uint32_t column_high(uint32_t b, uint32_t c, uint32_t logC, uint32_t hb) {
        return (tile_bitrev(c, logC) << (hb - logC)) | tile_bitrev(b, hb - logC);
    }
    template <bool STORE, bool INV>
    static __device__ __forceinline__ uint32_t place_last(const Params &p, uint32_t b, uint32_t e, uint32_t &m, uint32_t &c) {
        const uint32_t r = p.r, logC = p.logC, L = p.L;
        if (STORE) {   // the natural-order index of word (column, row)
            c = e & ((1u << logC) - 1);
            m = e >> logC;
            return (tile_bitrev(m, r) << (L - r)) + (b << logC) + c;
        }
        m = e & ((1u << r) - 1);   // a column is 2^r consecutive words
        c = e >> r;
        return (column_high(b, c, logC, L - r) << r) | m;
    }

    static __device__ __forceinline__ uint32_t tile_ctx(const Params &, uint32_t hi) { return hi; }
    static __device__ __forceinline__ uint32_t column_ctx(const Params &p, uint32_t b, uint32_t c) { return column_high(b, c, p.logC, p.L - p.r); }
    template <bool LO> static __device__ __forceinline__ uint64_t twiddle(const Params &p, uint32_t ctx, uint32_t t, uint32_t xg) {
        return p.f.tw[(ctx << t) | xg];
    }

    static __device__ __forceinline__ uint64_t coset_factor(const Params &p, uint32_t i) {
        return gl_mul(p.f.cos_lo[i & ((1u << p.f.cos_hbits) - 1)], p.f.cos_hi[i >> p.f.cos_hbits]);
    }
    static __device__ __forceinline__ uint64_t load(const Params &p, uint64_t w, uint32_t g) {
        uint64_t v = gl_from_word(w);
        if (p.f.cos_in) v = gl_mul(v, coset_factor(p, g));   // c_i h^i
        return v;
    }
    static __device__ __forceinline__ uint64_t store(const Params &p, uint64_t v, uint32_t g) {
        if (p.f.cos_out) return gl_mul(v, coset_factor(p, g));   // h^-i N^-1
        return p.f.sc ? gl_mul(v, p.f.sc) : v;
    }
};

__global__ void gl_twiddle_fill_kernel(uint64_t *tw, uint64_t root, uint32_t bits, uint32_t count) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    tw[g] = gl_pow(root, tile_bitrev(g, bits));
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
    out[i] = gl_pow(root, natural ? i : tile_bitrev(i, bitrev_bits));
}
__global__ void gl_mul_kernel(const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t n) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) out[i] = gl_mul(a[i], b[i]);
}

// ---------------------------------------------------------------- host
// the primitive 2^order-th root g^(2^(32 - order)) (traits.rs:82-94) of the 2^32-th root g, or its inverse
uint64_t gl_host_root(uint64_t g, uint32_t order, bool inverse) {
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

// a validated call, and the host side of its passes (tile_run)
struct GlCall {
    bool inv;
    uint64_t root;      // the 2^32-th root, validated
    bool coset;
    uint64_t h;         // the offset mod p, not zero
    const uint64_t *cos_lo, *cos_hi;   // the call's power tables (gl_transform_device)
    uint32_t cos_hbits;

    bool backward() const { return false; }   // the inverse is the same forward passes over the table of w^-1
    void fill(GoldilocksPolicy::Fields &f, uint32_t L, bool first, bool last) const {
        f.tw = (const uint64_t *)shared_state().goldilocks[inv ? 1 : 0].buf.p;
        f.cos_lo = cos_lo;
        f.cos_hi = cos_hi;
        f.cos_hbits = cos_hbits;
        f.cos_in = (coset && !inv && first) ? 1u : 0u;
        f.cos_out = (coset && inv && last) ? 1u : 0u;
        f.sc = (inv && last && !coset && L > 0) ? gl_inv(1ull << L) : 0u;   // with an offset N^-1 rides in the hi table
    }
    void (*kernel(bool last, const char *&name) const)(GoldilocksPolicy::Params) {
        name = last ? "gl_pass_kernel<last>" : "gl_pass_kernel";
        return last ? tile_pass_kernel<GoldilocksPolicy, true, false> : tile_pass_kernel<GoldilocksPolicy, false, false>;
    }
};

// forward / inverse / low-degree extension (forward, in_log2 < L) of `batch` columns
static int gl_transform_device(Context &c, GlCall call, const uint64_t *d_in, uint64_t in_stride, uint32_t in_log2, uint64_t *d_out,
                               uint64_t out_stride, uint32_t L, uint32_t batch, hipStream_t stream) {
    const uint64_t n = 1ull << L, nin = 1ull << in_log2;
    if (!in_stride) in_stride = nin;
    if (!out_stride) out_stride = n;
    const int rc = gl_ensure_twiddles(c, call.inv, L, call.root, stream);
    if (rc) return rc;
    // coset factors: h^i over the 2^in_log2 coefficients (the padding comes after Polynomial::scale), h^-i N^-1 over the result
    call.cos_hbits = in_log2 < 12 ? in_log2 : 12;
    if (call.coset) {
        const uint32_t n_lo = 1u << call.cos_hbits, n_hi = 1u << (in_log2 - call.cos_hbits);
        if (c.gl_coset.ensure(8 * ((size_t)n_lo + n_hi))) return LW_ERR_ALLOC;
        uint64_t *lo = (uint64_t *)c.gl_coset.p, *hi = lo + n_lo;
        call.cos_lo = lo;
        call.cos_hi = hi;
        hipLaunchKernelGGL(gl_power_tables_kernel, dim3(((n_lo > n_hi ? n_lo : n_hi) + 255) / 256), dim3(256), 0, stream, lo, hi,
                           call.inv ? gl_inv(call.h) : call.h, call.cos_hbits, n_hi, call.inv ? gl_inv(n) : 1ull);
        LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    }
    return tile_transform_device<GoldilocksPolicy>(c, call, d_in, in_stride, in_log2, d_out, out_stride, L, batch, stream);
}

// the low-degree extension inside another call's Entry (the Fp2 FRI layer of goldilocks_ext.hip: batch = 2 planes); root and
// offset are validated, offset = 1 is no coset
int goldilocks_lde_locked(Context &c, const uint64_t *d_coeffs, uint32_t log2_coeffs, uint64_t in_stride, uint64_t *d_out, uint32_t log2n,
                          uint64_t out_stride, uint32_t batch, uint64_t offset, uint64_t root, hipStream_t stream) {
    GlCall call{};
    call.inv = false;
    call.root = root;
    call.coset = offset != 1;
    call.h = offset;
    return gl_transform_device(c, call, d_coeffs, in_stride, log2_coeffs, d_out, out_stride, log2n, batch, stream);
}

// a whole transform inside another call's Entry (the Fp2 composition parts of goldilocks_ext.hip: the inverse of two planes);
// root and offset are validated, offset = 1 is no coset
int goldilocks_ntt_locked(Context &c, bool inverse, const uint64_t *d_in, uint64_t in_stride, uint64_t *d_out, uint64_t out_stride, uint32_t log2n,
                          uint32_t batch, uint64_t offset, uint64_t root, hipStream_t stream) {
    GlCall call{};
    call.inv = inverse;
    call.root = root;
    call.coset = offset != 1;
    call.h = offset;
    return gl_transform_device(c, call, d_in, in_stride, log2n, d_out, out_stride, log2n, batch, stream);
}

// ---- argument checks, before any device work (the first two are goldilocks_ext.hip's too: internal.h)
int gl_size_check(uint64_t log2n) {
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
int gl_root_check(uint64_t &root) {
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
static int gl_check(int dir, const void *in, const void *out, uint32_t log2n, uint32_t batch, size_t stride, const uint64_t *offset_or_null,
                    uint64_t root, GlCall &call) {
    int rc = gl_size_check(log2n);
    if (rc) return rc;
    if (dir != LW_DIR_FORWARD && dir != LW_DIR_INVERSE) { set_error("bad direction %d", dir); return LW_ERR_BAD_ARG; }
    const size_t n = (size_t)1 << log2n;
    if (!in || !out || batch == 0) { set_error("null buffer or empty batch"); return LW_ERR_BAD_ARG; }
    if (stride != 0 && stride < n) { set_error("batch stride %zu < transform length", stride); return LW_ERR_BAD_ARG; }
    const size_t span = (size_t)(batch - 1) * (stride ? stride : n) + n;
    if (in != out && spans_overlap(in, span * 8, out, span * 8)) { set_error("in and out overlap without being the same buffer"); return LW_ERR_BAD_ARG; }
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
    const int rc = gl_check((int)dir, in, out, log2n, batch, batch_stride, offset_or_null, two_adic_root, call);
    if (rc) return rc;
    const size_t stride = batch_stride ? batch_stride : (size_t)1 << log2n;
    return tile_host_entry(in, out, log2n, batch, stride, [&](Context &c, const uint64_t *d_in, uint64_t *d_out, hipStream_t io) {
        return gl_transform_device(c, call, d_in, stride, log2n, d_out, stride, log2n, batch, io);
    });
}

int lw_goldilocks_lde_device(const uint64_t *d_coeffs, uint32_t log2_coeffs, size_t in_stride, uint64_t *d_out, uint32_t log2n,
                             size_t out_stride, uint32_t batch, const uint64_t *offset_or_null, uint64_t two_adic_root, void *hip_stream) {
    int rc = gl_size_check(log2n);
    if (rc) return rc;
    if (log2_coeffs > log2n) { set_error("2^%u coefficients do not fit a 2^%u domain", log2_coeffs, log2n); return LW_ERR_BAD_ARG; }
    const size_t nin = (size_t)1 << log2_coeffs, nout = (size_t)1 << log2n;
    if (!d_coeffs || !d_out || batch == 0) { set_error("null buffer or empty batch"); return LW_ERR_BAD_ARG; }
    if ((in_stride != 0 && in_stride < nin) || (out_stride != 0 && out_stride < nout)) { set_error("batch stride < column length"); return LW_ERR_BAD_ARG; }
    if (spans_overlap(d_coeffs, ((size_t)(batch - 1) * (in_stride ? in_stride : nin) + nin) * 8, d_out,
                      ((size_t)(batch - 1) * (out_stride ? out_stride : nout) + nout) * 8)) {
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
    if ((d_out != d_a && spans_overlap(d_out, n * 8, d_a, n * 8)) || (d_out != d_b && spans_overlap(d_out, n * 8, d_b, n * 8))) {
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
