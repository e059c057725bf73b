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
// The passes themselves are tile_pass.cuh; CirclePolicy below is this field's side of them.  On the evaluation side of
// an LO pass both permutations are in the addresses: position P = (bitrev(row) << cb) | column goes to word 2P (P < n/2)
// or 2(n-1-P)+1.  A tile takes 2^(logC-1) neighbouring columns AND their complements, so that it holds word 2P+1 next to
// word 2P and moves runs of 2^logC consecutive words.  The twiddles of an LO pass are tw[s][(bitrev(x) << s0) | column]:
// consecutive over the columns a wave covers, so its work-items walk columns fastest.
// N^-1 rides on the last store of an interpolation; every word of a result is canonical (< p), intermediates are in [0, p].
#include <string.h>
#include "circle.cuh"
#include "tile_pass.cuh"

namespace lw {

constexpr uint32_t CIRCLE_MAX_LOG = 30;   // g_{2n} must exist in a group of order 2^31

struct CirclePolicy {
    typedef uint32_t word;
    static constexpr int TILE_LOG = 13;   // 8192 u32 = 32 KiB of LDS
    static constexpr bool LAST_ROWS_FASTEST = false;
    static constexpr const char *MAX_R_ENV = "LW_HIP_CIRCLE_MAX_R";
    struct Fields {
        const uint32_t *twx;   // x-layers (or their inverses), layer i at word 2^i - 1
        const uint32_t *twy;   // layer L - 1 of this size (or its inverses)
        uint32_t sc;           // != 0: the store multiplies by it (N^-1)
        uint32_t canonical;    // the store writes canonical residues (the caller's buffer)
    };
    typedef TilePassParams<CirclePolicy> Params;

    static __device__ __forceinline__ uint32_t add(uint32_t a, uint32_t b) { return m31_add(a, b); }
    static __device__ __forceinline__ uint32_t sub(uint32_t a, uint32_t b) { return m31_sub(a, b); }
    static __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) { return m31_mul(a, b); }

    // LO pass: the low cb = L - r position bits of tile column c of block b.  Columns below 2^(logC-1) are the block's own,
    // the others their complements (the partners under P -> n-1-P).
    static __device__ __forceinline__ uint32_t column(uint32_t b, uint32_t c, uint32_t logC, uint32_t cb) {
        if (cb == 0) return 0u;
        const uint32_t half = logC - 1;
        const uint32_t v = (b << half) | (c & ((1u << half) - 1));
        return (c >> half) ? (~v & ((1u << cb) - 1)) : v;
    }
    // LO pass, evaluation side: item e of the tile -> (row, column) such that consecutive e are consecutive words
    static __device__ __forceinline__ void fold_item(uint32_t e, uint32_t r, uint32_t logC, uint32_t &m, uint32_t &c) {
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
    static __device__ __forceinline__ uint32_t fold_word(uint32_t m, uint32_t col, uint32_t r, uint32_t cb) {
        const uint32_t P = (tile_bitrev(m, r) << cb) | col, n = 1u << (r + cb);
        return P < n / 2 ? 2 * P : 2 * (n - 1 - P) + 1;
    }
    // the evaluation side (folded) is what an evaluation stores to and an interpolation loads from
    template <bool STORE, bool INV>
    static __device__ __forceinline__ uint32_t place_last(const Params &p, uint32_t b, uint32_t e, uint32_t &m, uint32_t &c) {
        const uint32_t r = p.r, logC = p.logC, cb = p.L - r;
        if (STORE != INV) {
            fold_item(e, r, logC, m, c);
            return fold_word(m, column(b, c, logC, cb), r, cb);
        }
        m = e & ((1u << r) - 1);
        c = e >> r;
        return (tile_bitrev(column(b, c, logC, cb), cb) << r) | m;
    }

    static __device__ __forceinline__ uint32_t tile_ctx(const Params &p, uint32_t hi) { return tile_bitrev(hi, p.s0); }
    static __device__ __forceinline__ uint32_t column_ctx(const Params &p, uint32_t b, uint32_t c) { return column(b, c, p.logC, p.L - p.r); }
    template <bool LO> static __device__ __forceinline__ uint32_t twiddle(const Params &p, uint32_t ctx, uint32_t t, uint32_t xg) {
        const uint32_t s = p.s0 + t, j = (tile_bitrev(xg, t) << p.s0) | ctx;
        return LO && s == p.L - 1 ? p.f.twy[j] : p.f.twx[(1u << s) - 1 + j];   // an HI pass ends at s <= L - 2: x-layers only
    }

    static __device__ __forceinline__ uint32_t load(const Params &, uint32_t w, uint32_t) { return m31_from_word(w); }
    static __device__ __forceinline__ uint32_t store(const Params &p, uint32_t v, uint32_t) {
        if (p.f.sc) v = m31_mul(v, p.f.sc);
        if (p.f.canonical) v = m31_canon(v);
        return v;
    }
};

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

// The cached inverse tables of a transform of 2^L words, for mersenne31_ext.hip (internal.h): *ix the inverse x-layers
// 0 .. L - 2 (layer i at word 2^i - 1; null for L = 1), *iy the 2^(L-1) inverses of the y-layer of that size, both in the
// order of the transform: entry j belongs to the point (1 + 4j) g.
int circle_inverse_twiddles(Context &c, uint32_t L, hipStream_t stream, const uint32_t **ix, const uint32_t **iy) {
    const int rc = circle_ensure_twiddles(c, L, stream);
    if (rc) return rc;
    const SharedState &sh = shared_state();
    const uint32_t *xt = (const uint32_t *)sh.circle_x.buf.p;
    *ix = L >= 2 && xt ? xt + (1ull << (sh.circle_x.log_n - 1)) : nullptr;
    *iy = (const uint32_t *)sh.circle_y[L].buf.p + (1ull << (L - 1));
    return LW_OK;
}

// the host side of a transform's passes (tile_run); the tables must be there (circle_ensure_twiddles)
struct CircleCall {
    bool inv;
    bool backward() const { return inv; }   // interpolation: the evaluation's passes backwards, and their steps
    void fill(CirclePolicy::Fields &f, uint32_t L, bool first, bool last) const {
        const SharedState &sh = shared_state();
        f.twx = (const uint32_t *)sh.circle_x.buf.p;
        f.twy = (const uint32_t *)sh.circle_y[L].buf.p;
        if (inv) {
            if (f.twx) f.twx += 1ull << (sh.circle_x.log_n - 1);
            f.twy += 1ull << (L - 1);
        }
        f.sc = (inv && last) ? 1u << (31 - L) : 0u;   // N^-1 = 2^-L = 2^(31-L): 2^31 = 1
        f.canonical = last ? 1u : 0u;
    }
    void (*kernel(bool lo, const char *&name) const)(CirclePolicy::Params) {
        name = lo ? (inv ? "circle_pass_kernel<lo,inv>" : "circle_pass_kernel<lo>") : (inv ? "circle_pass_kernel<hi,inv>" : "circle_pass_kernel<hi>");
        if (lo) return inv ? tile_pass_kernel<CirclePolicy, true, true> : tile_pass_kernel<CirclePolicy, true, false>;
        return inv ? tile_pass_kernel<CirclePolicy, false, true> : tile_pass_kernel<CirclePolicy, false, false>;
    }
};

static int circle_transform_device(Context &c, bool inv, const uint32_t *d_in, uint32_t *d_out, uint32_t L, uint32_t batch, uint64_t stride,
                                   hipStream_t stream) {
    if (!stride) stride = 1ull << L;
    const int rc = circle_ensure_twiddles(c, L, stream);
    if (rc) return rc;
    return tile_transform_device<CirclePolicy>(c, CircleCall{inv}, d_in, stride, L, d_out, stride, L, batch, stream);
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
    const uint32_t chunk = batch < MAX_BATCH ? batch : MAX_BATCH;
    if (c.scratch.ensure((size_t)(nin + nout) * chunk * 4)) return LW_ERR_ALLOC;   // coefficients | what lies between two passes
    uint32_t *coeffs = (uint32_t *)c.scratch.p, *work = coeffs + nin * chunk;
    const NttPlan back = tile_plan<CirclePolicy>(Lin, Lin), out = tile_plan<CirclePolicy>(Lout, Lin);
    return split_batch(batch, [&](uint32_t b0, uint32_t nb) {
        const int rc = tile_run<CirclePolicy>(c, CircleCall{true}, back, d_evals + b0 * in_stride, in_stride, Lin, coeffs, nin, Lin, nb, work, stream);
        return rc ? rc : tile_run<CirclePolicy>(c, CircleCall{false}, out, coeffs, nin, Lin, d_out + b0 * out_stride, out_stride, Lout, nb, work, stream);
    });
}

// The two halves of the LDE for mersenne31_ext.hip (internal.h), each side under a stride of its own: interpolate_cfft of
// `batch` columns of 2^L words, and evaluate_cfft(zero_pad(coeffs, 2^Lout)) of blocks of 2^Lin coefficients, the padding
// never written.  The arguments are the caller's to check.
int circle_interpolate_locked(Context &c, const uint32_t *d_in, uint64_t in_stride, uint32_t *d_out, uint64_t out_stride, uint32_t L, uint32_t batch,
                              hipStream_t stream) {
    const int rc = circle_ensure_twiddles(c, L, stream);
    if (rc) return rc;
    return tile_transform_device<CirclePolicy>(c, CircleCall{true}, d_in, in_stride, L, d_out, out_stride, L, batch, stream);
}
int circle_extend_locked(Context &c, const uint32_t *d_coeffs, uint32_t Lin, uint64_t in_stride, uint32_t *d_out, uint32_t Lout, uint64_t out_stride,
                         uint32_t batch, hipStream_t stream) {
    const int rc = circle_ensure_twiddles(c, Lout, stream);
    if (rc) return rc;
    return tile_transform_device<CirclePolicy>(c, CircleCall{false}, d_coeffs, in_stride, Lin, d_out, out_stride, Lout, batch, stream);
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
static int circle_check(const void *in, const void *out, uint32_t log2n, uint32_t batch, size_t stride) {
    const int rc = circle_size_check(log2n);
    if (rc) return rc;
    const size_t n = (size_t)1 << log2n;
    if (!in || !out || batch == 0) { set_error("null buffer or empty batch"); return LW_ERR_BAD_ARG; }
    if (stride != 0 && stride < n) { set_error("batch stride %zu < transform length", stride); return LW_ERR_BAD_ARG; }
    const size_t span = (size_t)(batch - 1) * (stride ? stride : n) + n;
    if (in != out && spans_overlap(in, span * 4, out, span * 4)) { set_error("in and out overlap without being the same buffer"); return LW_ERR_BAD_ARG; }
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
    const int rc = circle_check(in, out, log2n, batch, stride);
    if (rc) return rc;
    if (!stride) stride = (size_t)1 << log2n;
    return tile_host_entry(in, out, log2n, batch, stride, [&](Context &c, const uint32_t *d_in, uint32_t *d_out, hipStream_t io) {
        return circle_transform_device(c, inv, d_in, d_out, log2n, batch, stride, io);
    });
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
    if (d_evals != d_out && spans_overlap(d_evals, ((size_t)(batch - 1) * (in_stride ? in_stride : nin) + nin) * 4, d_out,
                                          ((size_t)(batch - 1) * (out_stride ? out_stride : nout) + nout) * 4)) {
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
