// The LDS-tiled multi-stage pass of a radix-2 transform over one-word elements, written once for circle.hip (Mersenne31,
// u32) and goldilocks.hip (u64): the pass kernel, this family's side of the loop that launches the passes of a transform
// (pass_run.h) and the host-buffer entry body.  A field is a compile-time policy T, a struct of constants, types and static
// __device__ __forceinline__ functions, so every kernel holds a single inlined copy of T's arithmetic and addressing.
//
// Passes.  A transform of 2^L words takes ceil(L / 8) passes (plan_passes), each a tile of 2^r rows x 2^logC columns in
// LDS, 2^T::TILE_LOG words = 32 KiB (Goldilocks 2^12 u64: four workgroups per CU, 2^13 would leave two; circle 2^13 u32).
// The vector is indexed so that stage s pairs the words whose index differs in bit L-1-s (the NR-DIT dataflow of ntt_bb.hip):
//   HI pass  (every pass but the one that faces the reordered side: the last of a forward transform, the first of a
//            backward one): rows are the index bits [L-s0-r, L-s0), columns lower bits, so a tile reads and writes runs of
//            2^logC consecutive words per row and all of it shares the 2^r - 1 twiddles of its stages (they depend on the
//            bits above the rows only): staged in LDS, stage t group x at slot 2^t - 1 + x.
//   LO pass  rows are the index bits [0, r), so on the plain side a column is 2^r consecutive words.  Which columns a tile
//            takes and where its words go on the other side is the field's reordering (T::place_last: the bit reversal, or
//            the circle transform's fold), chosen so that both sides move runs of 2^logC consecutive words through LDS.
//            LDS slots are XOR-swizzled by row, so that neither the row-wise nor the column-wise side of the tile runs into
//            one bank.  The stages' twiddles differ per column and are fetched per work-item (T::twiddle<true>).
// A pass runs its r stages as register steps of at most 2^4 words (radix 16, TILE_KMAX), a barrier between two steps.
// The butterfly direction is a property of the instantiation: forward (a + b tw, a - b tw), stages ascending, or backward
// (a + d, (a - d) tw), stages descending, over tables of inverses (the circle interpolation; Goldilocks runs its inverse
// as forward passes over the table of w^-1 and never instantiates it).
//
// What T supplies:
//   T::word, T::TILE_LOG, T::LAST_ROWS_FASTEST    element, log2 words of a tile, the walk of the work-items of an LO pass
//                                                 (rows fastest or columns fastest: whichever makes a wave's twiddles neighbours)
//   T::Fields                                     the field's own kernel parameters (tables, factors on load and store)
//   T::add, T::sub, T::mul                        on values as they lie in LDS
//   T::tile_ctx(p, hi), T::column_ctx(p, b, c)    what the twiddle index of an HI tile / of column c of LO block b depends on
//   T::twiddle<LO>(p, ctx, t, xg)                 the twiddle of stage t of the pass, group xg of its 2^t
//   T::place_last<STORE, INV>(p, b, e, m, c)      LO pass: item e of block b -> (row m, column c), returns its word index
//                                                 on the side the pass loads from or (STORE) stores to
//   T::load(p, w, g), T::store(p, v, g)           word g on its way into LDS (the first pass) and out of it (the last)
//   T::MAX_R_ENV                                  the name of the field's stages-per-pass tuning switch
// and on the host a call object: backward(), fill(fields, L, first, last) and kernel(lo, name), see tile_run.
#pragma once
#include <stdlib.h>
#include "pass_run.h"

namespace lw {

constexpr int TILE_THREADS = 256;
constexpr int TILE_KMAX = 4;                 // radix-16 register steps

template <class T> struct TilePassParams {
    const typename T::word *in;
    typename T::word *out;
    // the field's own, behind the pointers where its tables lay before the kernel was shared: with it at the end the two
    // pointers and the strides are one 32-byte scalar load, and the circle LO kernels, already at the SGPR limit, keep a
    // dead 36-byte stack slot that turns their scratch on (profiles/tile_pass_isa.txt)
    typename T::Fields f;
    uint64_t in_stride, out_stride;   // words between the columns of a batch
    uint32_t L, s0, r, logC;
    uint32_t nsteps, k[4], t0[4];     // register steps in the order they run: stages t0 .. t0 + k - 1 of the pass
    // low-degree extension (first forward pass): word g of the zero-padded coefficients is in[g & in_mask] — the stages
    // that only pair data with padding leave the block replicated and are skipped (s0 starts behind them)
    uint32_t in_mask;
};

__device__ __forceinline__ uint32_t tile_bitrev(uint32_t x, uint32_t bits) { return bits ? (__brev(x) >> (32 - bits)) : 0u; }
__device__ __forceinline__ uint32_t tile_slot(uint32_t m, uint32_t c, uint32_t logC) {
    return (m << logC) | (c ^ ((m ^ (m >> 4)) & ((1u << logC) - 1)));
}

// one register step of one work-item: 2^K words of one column, K stages
template <class T, int K, bool LO, bool INV>
__device__ __forceinline__ void tile_item(const TilePassParams<T> &p, typename T::word *lds, const typename T::word *ltw, uint32_t w, uint32_t t0,
                                          uint32_t b) {
    using word = typename T::word;
    constexpr int E = 1 << K;
    const uint32_t r = p.r, logC = p.logC;
    uint32_t c, mr;
    if (LO && T::LAST_ROWS_FASTEST) {
        mr = w & ((1u << (r - K)) - 1);
        c = w >> (r - K);
    } else {   // columns fastest: LDS rows are consecutive
        c = w & ((1u << logC) - 1);
        mr = w >> logC;
    }
    const uint32_t sh = r - t0 - K;
    const uint32_t m_high = mr >> sh;
    const uint32_t mbase = (m_high << (sh + K)) | (mr & ((1u << sh) - 1));
    const uint32_t ctx = LO ? T::column_ctx(p, b, c) : 0u;
    word x[E];
#pragma unroll
    for (int j = 0; j < E; j++) x[j] = lds[tile_slot(mbase | ((uint32_t)j << sh), c, logC)];
    auto twiddle = [&](uint32_t t, uint32_t xg) -> word {   // stage t of the pass, group xg of its 2^t
        return LO ? T::template twiddle<true>(p, ctx, t, xg) : ltw[(1u << t) - 1 + xg];
    };
    if (!INV) {
#pragma unroll
        for (int u = 0; u < K; u++) {
            const int half = 1 << (K - 1 - u);
#pragma unroll
            for (int jt = 0; jt < (1 << u); jt++) {
                const word tw = twiddle(t0 + u, (m_high << u) | (uint32_t)jt);
#pragma unroll
                for (int jl = 0; jl < half; jl++) {
                    const int j = (jt << (K - u)) | jl;
                    const word v = T::mul(x[j + half], tw), a = x[j];
                    x[j] = T::add(a, v);
                    x[j + half] = T::sub(a, v);
                }
            }
        }
    } else {
#pragma unroll
        for (int u = K - 1; u >= 0; u--) {
            const int half = 1 << (K - 1 - u);
#pragma unroll
            for (int jt = 0; jt < (1 << u); jt++) {
                const word tw = twiddle(t0 + u, (m_high << u) | (uint32_t)jt);
#pragma unroll
                for (int jl = 0; jl < half; jl++) {
                    const int j = (jt << (K - u)) | jl;
                    const word a = x[j], d = x[j + half];
                    x[j] = T::add(a, d);
                    x[j + half] = T::mul(T::sub(a, d), tw);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < E; j++) lds[tile_slot(mbase | ((uint32_t)j << sh), c, logC)] = x[j];
}

template <class T, bool LO, bool INV>
__global__ __launch_bounds__(TILE_THREADS) void tile_pass_kernel(TilePassParams<T> p) {
    using word = typename T::word;
    __shared__ word lds[1 << T::TILE_LOG];
    __shared__ word ltw[LO ? 1 : 256];   // HI pass: stage t group x at slot 2^t - 1 + x (r <= 8)
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const uint32_t r = p.r, logC = p.logC, L = p.L, s0 = p.s0;
    const uint32_t total = 1u << (r + logC), cmask = (1u << logC) - 1;
    const word *gin = p.in + (uint64_t)blockIdx.y * p.in_stride;
    word *gout = p.out + (uint64_t)blockIdx.y * p.out_stride;

    uint32_t lgS = 0, base = 0;
    if (!LO) {
        lgS = L - s0 - r;   // row stride in words
        const uint32_t lo_bits = lgS - logC;
        const uint32_t hi = b >> lo_bits;
        base = (hi << (L - s0)) + ((b & ((1u << lo_bits) - 1)) << logC);
        const uint32_t ctx = T::tile_ctx(p, hi);
        for (uint32_t i = tid; i + 1 < (1u << r); i += TILE_THREADS) {
            const uint32_t t = 31 - __clz(i + 1), xg = i + 1 - (1u << t);
            ltw[i] = T::template twiddle<false>(p, ctx, t, xg);
        }
    }
    for (uint32_t e = tid; e < total; e += TILE_THREADS) {
        uint32_t m, c, g;
        if (LO) {
            g = T::template place_last<false, INV>(p, b, e, m, c);
        } else {
            c = e & cmask;
            m = e >> logC;
            g = base + (m << lgS) + c;
        }
        g &= p.in_mask;
        lds[tile_slot(m, c, logC)] = T::load(p, gin[g], g);
    }
    for (uint32_t step = 0; step < p.nsteps; step++) {
        const uint32_t k = p.k[step], t0 = p.t0[step];
        const uint32_t nitems = total >> k;
        __syncthreads();
        for (uint32_t w = tid; w < nitems; w += TILE_THREADS) {
            if (k == 4) tile_item<T, 4, LO, INV>(p, lds, ltw, w, t0, b);
            else if (k == 3) tile_item<T, 3, LO, INV>(p, lds, ltw, w, t0, b);
            else if (k == 2) tile_item<T, 2, LO, INV>(p, lds, ltw, w, t0, b);
            else tile_item<T, 1, LO, INV>(p, lds, ltw, w, t0, b);
        }
    }
    __syncthreads();
    for (uint32_t e = tid; e < total; e += TILE_THREADS) {
        uint32_t m, c, g;
        if (LO) {
            g = T::template place_last<true, INV>(p, b, e, m, c);
        } else {
            c = e & cmask;
            m = e >> logC;
            g = base + (m << lgS) + c;
        }
        gout[g] = T::store(p, lds[tile_slot(m, c, logC)], g);
    }
}

// ---------------------------------------------------------------- host
// a *_MAX_R switch (LW_HIP_TUNING only): fewer stages per pass, for the pass counts of the largest sizes at test sizes
static uint32_t tile_max_r(const char *name) {
    const char *e = tuning_env(name);
    const int v = e ? atoi(e) : 0;
    return v >= 4 && v <= (int)NTT_MAX_R ? (uint32_t)v : NTT_MAX_R;
}
template <class T> static NttPlan tile_plan(uint32_t L, uint32_t in_log2) {
    return plan_passes(L, L, L - in_log2, T::TILE_LOG, TILE_KMAX, false, tile_max_r(T::MAX_R_ENV));
}
static bool spans_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// One transform of `batch` columns of 2^L words by the passes of `pl` (tile_plan(L, in_log2)); a forward one reads
// 2^in_log2 words per column (in_log2 < L: zero padded).  `work` holds batch x 2^L words for what lies between two
// passes and for the copy of an in-place single pass; it is only touched when there is more than one pass or
// d_in == d_out (run_passes).  The field's tables must be there.  `call` is the field's side of the loop:
//   call.backward()                  the passes, and the steps of each, run in reverse order (the backward butterfly)
//   call.fill(f, L, first, last)     the field's parameters of the first / last pass that runs, or one between
//   call.kernel(lo, name)            the instantiation for an LO or HI pass and its line in lw_hip_profile_end
template <class T, class Call>
static int tile_run(Context &c, const Call &call, const NttPlan &pl, const typename T::word *d_in, uint64_t in_stride, uint32_t in_log2,
                    typename T::word *d_out, uint64_t out_stride, uint32_t L, uint32_t batch, typename T::word *work, hipStream_t stream) {
    using word = typename T::word;
    return run_passes(c, schedule_passes(pl, call.backward(), d_in == d_out), L, d_in, in_stride, d_out, out_stride, batch, work, sizeof(word), stream,
                      [&](const PassStep &st, const void *in, void *out, uint64_t src_stride, uint64_t dst_stride, dim3 grid) {
        TilePassParams<T> p{};
        p.in = (const word *)in;
        p.in_stride = src_stride;
        p.out = (word *)out;
        p.out_stride = dst_stride;
        p.L = L;
        p.s0 = st.s0;
        p.r = st.r;
        p.logC = st.logC;
        p.nsteps = st.nsteps;
        for (uint32_t j = 0; j < p.nsteps; j++) {
            p.k[j] = st.k[j];
            p.t0[j] = st.t0[j];
        }
        p.in_mask = st.first ? (uint32_t)((1ull << in_log2) - 1) : 0xffffffffu;
        call.fill(p.f, L, st.first, st.last);
        const char *name = nullptr;
        void (*kernel)(TilePassParams<T>) = call.kernel(st.lo, name);
        hipLaunchKernelGGL(kernel, grid, dim3(TILE_THREADS), 0, stream, p);
        return name;
    });
}

// tile_run over a batch of any width, with the lane's scratch as `work`
template <class T, class Call>
static int tile_transform_device(Context &c, const Call &call, const typename T::word *d_in, uint64_t in_stride, uint32_t in_log2,
                                 typename T::word *d_out, uint64_t out_stride, uint32_t L, uint32_t batch, hipStream_t stream) {
    using word = typename T::word;
    const NttPlan pl = tile_plan<T>(L, in_log2);
    if ((pl.npass > 1 || d_in == d_out) && c.scratch.ensure(((size_t)(batch < MAX_BATCH ? batch : MAX_BATCH) << L) * sizeof(word))) return LW_ERR_ALLOC;
    word *work = (word *)c.scratch.p;
    return split_batch(batch, [&](uint32_t b0, uint32_t nb) {
        return tile_run<T>(c, call, pl, d_in + b0 * in_stride, in_stride, in_log2, d_out + b0 * out_stride, out_stride, L, nb, work, stream);
    });
}

// The body of a host-buffer entry after its argument checks: `batch` columns of 2^log2n words, `stride` words apart, go
// up, transform(context, d_in, d_out, stream) runs on the lane's stream and the columns come back one by one, so that the
// words of `out` between strided columns stay as they are.  Complete on return.
template <class W, class F> static int tile_host_entry(const W *in, W *out, uint32_t log2n, uint32_t batch, size_t stride, F transform) {
    Entry en(nullptr);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t io = en.use_lane_stream();
    if (!io) return en.rc;
    const size_t n = (size_t)1 << log2n;
    const size_t span = ((size_t)(batch - 1) * stride + n) * sizeof(W);
    if (c.host_io_a.ensure(span) || c.host_io_b.ensure(span)) return LW_ERR_ALLOC;
    LW_HIP_CHECK(hipMemcpyAsync(c.host_io_a.p, in, span, hipMemcpyHostToDevice, io), LW_ERR_LAUNCH);
    const int rc = transform(c, (const W *)c.host_io_a.p, (W *)c.host_io_b.p, io);
    if (rc) return rc;
    LW_HIP_CHECK(hipMemcpy2DAsync(out, stride * sizeof(W), c.host_io_b.p, stride * sizeof(W), n * sizeof(W), batch, hipMemcpyDeviceToHost, io),
                 LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(io), LW_ERR_LAUNCH);
    return LW_OK;
}

}  // namespace lw
