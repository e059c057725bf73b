// Radix-2 NTT passes for 256-bit Montgomery fields (Stark252, BLS12-381 Fr) on gfx950.
//
// Dataflow = the reference's NR decimation-in-time transform (math/src/fft/cpu/fft.rs:20-55) followed by
// the bit-reverse permutation (math/src/fft/cpu/bit_reversing.rs:2-18): stage s pairs elements N/2^(s+1)
// apart and group g uses twiddle T[g] = w^bitrev(g) (math/src/fft/cpu/roots_of_unity.rs:26-45).  Because
// every field op returns the canonical residue, results are byte-identical to the reference however
// the stages are scheduled; here they are scheduled for the GPU:
//
//   * log2(N) stages are cut into passes of r <= 8 stages (the staged twiddles ltw[2][256] and the lazy bounds, 17p and
//     the 30p of ntt_bound_plan.h, all need r <= 8; plan_passes, ntt_plan.h, never plans more).  One workgroup owns a tile of 2^r "rows"
//     (the index bits the pass's stages touch) x C adjacent "columns" (contiguous elements), stages it in
//     LDS once and runs all r stages there: a pass costs one HBM read + one HBM write of the vector,
//     versus one round trip per stage in the reference's CUDA path (math/src/fft/gpu/cuda/ops.rs:28-38).
//   * inside a pass a work-item keeps 2^k (k <= 3) elements in VGPRs and runs k stages register-only
//     (radix-8 = 12 Montgomery products per 8 elements), exchanging through LDS between groups of k stages.
//   * the passes before the last over full-size tiles exchange one 16-byte plane of the elements at a time (ntt_exchange):
//     half the LDS, and for Stark252 three workgroups per CU instead of two (ntt_waves_per_simd); the twiddles of their
//     first two register steps are wave-uniform and reach the products through scalar loads and SGPR operands.
//   * the last pass folds the bit-reverse permutation into its store addresses: a workgroup takes the C
//     tiles whose bit-reversed tile ids are consecutive, so natural-order output leaves as C*32-byte runs.
//   * the INTT's N^-1 scaling (math/src/fft/polynomial.rs:172-173) is fused into the last pass.
//   * the passes before the last store their result straight from the registers of the last register step: their
//     work-items walk columns fastest, so the lanes of a row already hold one contiguous run of the output (256 B for an
//     8-stage tile).  Only the last pass goes back through LDS, for the transpose that turns its bit-reversed rows into
//     coalesced runs.
//   * lazy values (< 17p, at most 30p behind a full-size tile) handed from pass to pass are reduced on load only where the
//     first stage adds them (half of the elements of a work-item); the other half enters a Montgomery product, which takes
//     any 256-bit operand (ntt_item).
//   * over full-size tiles that reduction leaves c*p in place (c = 13 or 15, ntt_bound_plan.h), which lets the butterflies
//     of the first six or seven stages of the pass subtract without adding 2p first (ntt_butterflies).
#pragma once
#include "field.cuh"
#include "ntt_bound_plan.h"

namespace lw {

// Kernel geometry: a tile of 2^NTT_TILE_LOG elements (32 B each) per workgroup, NTT_THREADS threads, and at most NTT_KMAX
// stages per register step (2^NTT_KMAX elements per work-item).  What a workgroup keeps in LDS, and with it how many
// fit on a CU, is decided per kernel: see ntt_one_plane / ntt_waves_per_simd.
// (measured and dropped: 32 KiB tile / 256 threads -> 128-byte runs, 5.4 G elem/s; 64 KiB / 256 threads / radix-8 steps
//  -> 2 waves/SIMD, 7.4 G elem/s, against 9.6 for 2048 elements / 512 threads / radix-4 at the time)
constexpr int NTT_TILE_LOG = 11;
constexpr int NTT_TILE = 1 << NTT_TILE_LOG;
constexpr int NTT_THREADS = 512;
constexpr int NTT_KMAX = 2;
constexpr int NTT_LTW = 256;   // slots of the staged twiddle table: a pass of r <= 8 stages has 2^r - 1 <= 255 twiddles

struct NttPassParams {
    const uint4 *in;       // element e = in[2e], in[2e+1] (reference memory layout)
    uint4 *out;
    const uint4 *tw;       // bit-reversed twiddle table, internal layout (8 x u32, LS limb first)
    uint64_t in_batch_stride;   // elements between consecutive transforms of a batch
    uint64_t out_batch_stride;
    uint32_t L;            // log2 N
    uint32_t s0;           // first stage of this pass
    uint32_t r;            // stages in this pass
    uint32_t logC;         // log2 columns per tile
    uint32_t nsteps;
    uint32_t k[8];         // stages per register step, sum = r
    const uint4 *cos_lo, *cos_hi;   // coset powers h^e = cos_lo[e & mask] * cos_hi[e >> cos_hbits] (internal layout), or null
    uint32_t cos_hbits;
    uint32_t cos_in;       // first pass: multiply element e by h^e on load (Polynomial::scale, polynomial/mod.rs:259-271)
    uint32_t cos_out;      // last pass of an inverse transform: multiply natural output i by h^-i * N^-1 (folded into cos_hi)
    uint64_t in_mask;      // first pass of a low-degree extension: element g is read from in[g & in_mask] (see ntt256.hip)
    uint32_t lazy_in;      // input of this pass may be non-canonical (any 256-bit value; <= 30p in fact): a previous lazy pass wrote it
    uint32_t wave_sync;    // WL kernels: bit s set = the exchange before register step s stays inside a wavefront (no workgroup barrier)
    uint32_t scale;        // multiply outputs by sc (last pass of an inverse transform)
    uint32_t sc[8];
};

__device__ __forceinline__ uint32_t bitrev_bits(uint32_t x, uint32_t bits) {
    return bits ? (__brev(x) >> (32 - bits)) : 0u;
}

template <class F>
__device__ __forceinline__ Fe<F> tw_load(const uint4 *tw, uint64_t g) {
    uint4 a = tw[2 * g], b = tw[2 * g + 1];
    Fe<F> r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
}
// the same entry through a wave-uniform address: scalar loads into SGPRs.  The table is written before the pass kernels
// start and never while they run, which is what the constant address space asserts.
template <class F>
__device__ __forceinline__ Fe<F> tw_load_uniform(const uint4 *tw, uint64_t g) {
    typedef const __attribute__((address_space(4))) uint32_t *const_words;
    const_words w = (const_words)(uintptr_t)(tw + 2 * g);
    Fe<F> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = w[i];
    return r;
}
template <class F>
__device__ __forceinline__ void tw_store(uint4 *tw, uint64_t g, const Fe<F> &x) {
    tw[2 * g] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
    tw[2 * g + 1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}

// element in reference memory layout (two 16-byte halves) <-> limbs; pure register renaming
template <class F>
__device__ __forceinline__ Fe<F> unpack_mem(uint4 q0, uint4 q1) {
    Fe<F> r;
    r.v[6] = q0.x; r.v[7] = q0.y; r.v[4] = q0.z; r.v[5] = q0.w;
    r.v[2] = q1.x; r.v[3] = q1.y; r.v[0] = q1.z; r.v[1] = q1.w;
    return r;
}
template <class F>
__device__ __forceinline__ void pack_mem(const Fe<F> &a, uint4 &q0, uint4 &q1) {
    q0 = make_uint4(a.v[6], a.v[7], a.v[4], a.v[5]);
    q1 = make_uint4(a.v[2], a.v[3], a.v[0], a.v[1]);
}

// LDS slot (16-byte units within a plane) of tile element (row m, column c).
//   plain layout  (WL = false): rows of C columns, (m << logC) | c — work-items walk columns fastest.
//   column layout (WL = true):  every column's 2^r rows are contiguous and work-items walk ROWS fastest, so that a
//       column's butterflies of all stages belong to one wavefront (64 work-items x 4 elements = 256 rows) and the
//       exchanges between register steps need no workgroup barrier.  The low four row bits are XOR-ed with row bits 4-5
//       (into both bit pairs) and with the column, which makes every access pattern of the pass conflict-free over the
//       64 banks, 16 lanes at a time: the steps' row sets {0-3}, {0,1,4,5}, {2-5} and the (column, row&1) sets of the
//       coalesced global phases all map bijectively onto the four low slot bits.
template <bool WL>
__device__ __forceinline__ uint32_t lds_slot(uint32_t m, uint32_t c, uint32_t r, uint32_t logC) {
    if (!WL) return (m << logC) | c;
    const uint32_t sw = r >= 4 ? ((5u * ((m >> 4) & 3u)) ^ ((c & 7u) << 1)) : 0u;
    return (c << r) | (m ^ sw);
}
// exchange through LDS between two register steps when producer and consumer lanes share a wavefront: LDS operations
// of one wave execute in order, so only the compiler has to be kept from reordering them
__device__ __forceinline__ void lds_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Where the 2^K elements of one work-item sit in the tile during one register step: element j is row mbase | (j << sh)
// of column c.
struct NttItemGeo {
    uint32_t c, mbase, m_high, sh;
    uint32_t hi_c;     // index bits above the tile's rows (selects the twiddle groups)
    uint64_t gbase;    // global element index of the tile's row 0 (LAST) / of its row 0, column 0 (other passes)
};
// FX = r: a full-size tile of NTT_TILE = 2048 elements (r = 8 stages x 8 columns, 7 x 16 or 6 x 32) with its shape as
// compile-time constants, so that the shifts, masks, bit reversals and swizzles of the index arithmetic fold (every pass
// of a 2^24 transform, the last pass from 2^16 on).
template <int K, bool LAST, bool WL, int FX>
__device__ __forceinline__ NttItemGeo ntt_item_geo(const NttPassParams &p, uint32_t w, uint32_t step, uint32_t t0, uint64_t base,
                                                   uint32_t hi_uniform, uint32_t hi_low) {
    const uint32_t r = FX ? (uint32_t)FX : p.r, logC = FX ? (uint32_t)(NTT_TILE_LOG - FX) : p.logC, L = p.L;
    NttItemGeo g;
    g.sh = r - t0 - K;
    uint32_t mr;
    if ((LAST && step == 0) || (WL && (LAST || step > 0))) {   // rows fastest: contiguous global rows / one column per wave
        mr = w & ((1u << (r - K)) - 1);
        g.c = w >> (r - K);
    } else {                           // columns fastest
        g.c = w & ((1u << logC) - 1);
        mr = w >> logC;
    }
    const uint32_t m_low = mr & ((1u << g.sh) - 1);
    g.m_high = mr >> g.sh;
    g.mbase = (g.m_high << (g.sh + K)) | m_low;
    g.hi_c = hi_uniform;
    g.gbase = base;
    if (LAST) {
        g.hi_c = (bitrev_bits(g.c, logC) << (L - r - logC)) | hi_low;
        g.gbase = (uint64_t)g.hi_c << r;
    }
    return g;
}

// Non-last passes stage the tile's 2^r - 1 twiddles in LDS (stage t, group x -> slot 2^t - 1 + x holds
// T[(hi << t) | x], shared by every column).  Their loads are issued first and the data loads right behind
// them, so the workgroup pays one memory latency, not two, before its first butterfly.
__device__ __forceinline__ void ntt_tw_stage_load(const NttPassParams &p, uint32_t r, uint32_t hi_uniform, uint4 &tq0, uint4 &tq1) {
    const uint32_t ti = threadIdx.x;
    if (ti + 1 < (1u << r)) {
        const uint32_t t = 31 - __clz(ti + 1), xg = ti + 1 - (1u << t);
        const uint64_t g = ((uint64_t)hi_uniform << t) | xg;
        tq0 = p.tw[2 * g];
        tq1 = p.tw[2 * g + 1];
    }
}
__device__ __forceinline__ void ntt_tw_stage_store(uint4 (*ltw)[NTT_LTW], uint32_t r, const uint4 &tq0, const uint4 &tq1) {
    const uint32_t ti = threadIdx.x;
    if (ti + 1 < (1u << r)) {
        ltw[0][ti] = tq0;
        ltw[1][ti] = tq1;
    }
}

// the tile's elements of a work-item from global memory (register step 0)
// EXTRA: the pass carries a coset scaling or the N^-1 factor (kept out of the plain transform's code: the last-pass
// kernel is ~60 KiB of straight-line MAC chains and shares a 64 KiB instruction cache with its neighbour CU)
template <class F, int K, bool LAST, bool EXTRA>
__device__ __forceinline__ void ntt_load_global(const NttPassParams &p, const NttItemGeo &g, const uint4 *gin, uint32_t lgS, Fe<F> *x) {
    constexpr int E = 1 << K;
#pragma unroll
    for (int j = 0; j < E; j++) {   // the 2E global loads are issued back to back
        const uint32_t m = g.mbase | ((uint32_t)j << g.sh);
        const uint64_t e = (LAST ? (g.gbase + m) : (g.gbase + ((uint64_t)m << lgS) + g.c)) & p.in_mask;
        x[j] = unpack_mem<F>(gin[2 * e], gin[2 * e + 1]);
    }
    if (EXTRA && p.cos_in) {   // evaluate_offset_fft: c_e * h^e, fused into the first pass's load
#pragma unroll
        for (int j = 0; j < E; j++) {
            const uint32_t m = g.mbase | ((uint32_t)j << g.sh);
            const uint64_t e = (LAST ? (g.gbase + m) : (g.gbase + ((uint64_t)m << lgS) + g.c)) & p.in_mask;
            Fe<F> pw = fe_mul<F>(tw_load<F>(p.cos_lo, e & ((1ull << p.cos_hbits) - 1)), tw_load<F>(p.cos_hi, e >> p.cos_hbits));
            x[j] = fe_mul<F>(x[j], pw);
        }
    }
}

// Twiddle group q = 2^u - 1 + jt of a register step that starts at stage t0 of the pass (stage u of the step, group jt)
template <class F, bool LAST, bool WL>
__device__ __forceinline__ Fe<F> ntt_fetch_tw(const NttPassParams &p, const NttItemGeo &g, uint4 (*ltw)[NTT_LTW], uint32_t t0, int q) {
    const int u = 31 - __builtin_clz(q + 1), jt = q + 1 - (1 << u);
    Fe<F> tw;
    if (LAST || WL) {   // from the table (L1/L2): per-lane twiddles would cost LDS bandwidth the exchanges need
        const uint64_t gt = ((uint64_t)g.hi_c << (t0 + u)) | ((uint64_t)g.m_high << u);
        tw = tw_load<F>(p.tw, gt | (uint32_t)jt);
    } else {   // slot 2^t - 1 + x of the staged table
        const uint32_t li = (1u << (t0 + u)) - 1 + ((g.m_high << u) | (uint32_t)jt);
        uint4 a = ltw[0][li], b = ltw[1][li];
        tw.v[0] = a.x; tw.v[1] = a.y; tw.v[2] = a.z; tw.v[3] = a.w;
        tw.v[4] = b.x; tw.v[5] = b.y; tw.v[6] = b.z; tw.v[7] = b.w;
    }
    return tw;
}

// K stages on the 2^K elements of a work-item, register-only.  first: register step 0 (values straight from memory).
// PF: fetch the next twiddle under the current group's butterflies (eight more live VGPRs; see ntt_waves_per_simd).
// UNI: the step's twiddles are the same for the whole wavefront (g.m_high is wave-uniform and the pass is not the last):
// they come from the table through scalar loads, all E - 1 up front, and feed the products from SGPRs.
template <class F, int K, bool LAST, bool WL, bool PF, bool UNI = false, int FX = 0>
__device__ __forceinline__ void ntt_butterflies(const NttPassParams &p, const NttItemGeo &g, uint4 (*ltw)[NTT_LTW], uint32_t t0, bool first,
                                                Fe<F> *x) {
    constexpr int E = 1 << K;
    static_assert(!UNI || (!LAST && !WL), "wave-uniform twiddles: plain non-last passes only");
    const uint32_t m_high = UNI ? (uint32_t)__builtin_amdgcn_readfirstlane((int)g.m_high) : g.m_high;
    // Lazy reduction (fields with 4+ spare bits, F::LAZY): values ride in [0, 17p) — a butterfly is
    //   t = w*y in [0,2p) (no final subtraction), x' = x + t, y' = x + 2p - t, so the bound grows by 2p per stage;
    // a pass has <= 8 stages and starts them from values below p (so < 17p at its end); the last pass canonicalises on exit.
    // On load only the elements the first stage ADDS are reduced, j < E/2: the others, j >= E/2, go straight into that
    // stage's Montgomery product as the b operand, which takes any 256-bit value (a lazy input is < 17p < 2^256) and
    // returns t < 2p (the unit branch reduces its operand itself).  After the stage x'[j] = x + t < 3p and
    // x'[j + E/2] = x + 2p - t < 3p with x < p, the same p + 2p per stage as if all E had been reduced.
    // Every result is still the unique canonical residue when it leaves the transform, so parity is unaffected.
    //
    // Full-size tiles (FX stages, known here) go one step further, by the bound plan of ntt_bound_plan.h: the elements
    // the first stage adds get BP.c * p on load, with the reduction where the input is lazy (the masked + p becomes a
    // constant) and as a plain add in a first pass, whose inputs are below p (so are the canonical products of a coset
    // load).  In exchange the stages below BP.nfree subtract without adding 2p, 8 instructions less per butterfly; values
    // then ride in (0, 30p] and a pass hands on anything below 2^256, which the next pass's reduction and products take.
    // The run-time-shape kernels (FX = 0) keep [0, 17p) and the + 2p in every butterfly.
    constexpr bool OFFSET = F::LAZY && FX != 0;
    constexpr NttBoundPlan BP = ntt_bound_plan(FX ? FX : 1);
    if constexpr (OFFSET) {
        if (first) {
            if (p.lazy_in) {   // launch-uniform; with the add below this is fe_reduce_offset
#pragma unroll
                for (int j = 0; j < E / 2; j++) x[j] = fe_sub_qp(x[j]);
            }
#pragma unroll
            for (int j = 0; j < E / 2; j++) x[j] = fe_add_cp<BP.c>(x[j]);
        }
    } else if (F::LAZY && first && p.lazy_in) {
#pragma unroll
        for (int j = 0; j < E / 2; j++) x[j] = fe_reduce_full(x[j]);
    }

    // stage u of this step == stage s0 + t0 + u of the transform.  The E-1 twiddle groups of the step are walked in
    // order q = 2^u - 1 + jt; with PF group q+1's twiddle is fetched (LDS, or the table in the last pass) before group q's
    // butterflies run, so its latency hides behind a Montgomery product (the sched_barrier below pins it there).
    // Fetching all of a step's twiddles up front measured slower (more live registers, no fewer stalls).
    auto fetch_tw = [&](int q) -> Fe<F> { return ntt_fetch_tw<F, LAST, WL>(p, g, ltw, t0, q); };
    Fe<F> tw_next, tw_uni[E - 1];
    if (UNI) {
#pragma unroll
        for (int q = 0; q < E - 1; q++) {
            const int u = 31 - __builtin_clz(q + 1), jt = q + 1 - (1 << u);
            tw_uni[q] = tw_load_uniform<F>(p.tw, ((uint64_t)g.hi_c << (t0 + u)) | ((uint64_t)m_high << u) | (uint32_t)jt);
        }
    } else if (PF) {
        tw_next = fetch_tw(0);
    }
#pragma unroll
    for (int q = 0; q < E - 1; q++) {
        const int u = 31 - __builtin_clz(q + 1), jt = q + 1 - (1 << u);
        const int half = 1 << (K - 1 - u);
        const Fe<F> tw = UNI ? tw_uni[q] : PF ? tw_next : fetch_tw(q);
        if (!UNI && PF && q + 1 < E - 1) tw_next = fetch_tw(q + 1);
        // T[0] = 1: the first group of every stage multiplies by one (2^-t of stage t's butterflies, i.e. a
        // quarter of the first pass's products).  The reference multiplies anyway (fft.rs:40-43); the product
        // by the Montgomery one is the identity on canonical residues, so skipping it changes no byte.
        const bool unit = (jt == 0) && (g.hi_c == 0) && (m_high == 0);
        const bool free_stage = OFFSET && t0 + (uint32_t)u < (uint32_t)BP.nfree;   // t0 is a literal at every FX call site
#pragma unroll
        for (int jl = 0; jl < half; jl++) {
            const int j = (jt << (K - u)) | jl;
            if (F::LAZY) {
                Fe<F> wb = unit ? fe_reduce_full(x[j + half]) : UNI ? fe_mul_lazy_uniform<F>(tw, x[j + half]) : fe_mul_lazy<F>(tw, x[j + half]);
                if (free_stage) fe_butterfly_raw<F, true>(x[j], wb);
                else fe_butterfly_raw<F, false>(x[j], wb);
                x[j + half] = wb;
            } else {
                Fe<F> wb = unit ? x[j + half] : fe_mul<F>(tw, x[j + half]);
                Fe<F> a = x[j];
                x[j] = fe_add<F>(a, wb);
                x[j + half] = fe_sub<F>(a, wb);
            }
            __builtin_amdgcn_sched_barrier(0);   // keep butterflies serial: interleaved products cost too many VGPRs
        }
    }
}

// what the last register step of a pass does to its results before they leave: the inverse transform's scaling in its
// last pass, and the canonical form at the end of the last pass
template <class F, int K, bool LAST, bool EXTRA, int FX>
__device__ __forceinline__ void ntt_finish(const NttPassParams &p, const NttItemGeo &g, Fe<F> *x) {
    constexpr int E = 1 << K;
    const uint32_t r = FX ? (uint32_t)FX : p.r, logC = FX ? (uint32_t)(NTT_TILE_LOG - FX) : p.logC, L = p.L;
    if (EXTRA && LAST && p.cos_out) {   // interpolate_offset_fft: N^-1 and h^-i in one product
#pragma unroll
        for (int j = 0; j < E; j++) {
            const uint32_t m = g.mbase | ((uint32_t)j << g.sh);
            const uint64_t i_nat = ((uint64_t)bitrev_bits(m, r) << (L - r)) + ((uint64_t)blockIdx.x << logC) + g.c;
            Fe<F> pw = fe_mul<F>(tw_load<F>(p.cos_lo, i_nat & ((1ull << p.cos_hbits) - 1)), tw_load<F>(p.cos_hi, i_nat >> p.cos_hbits));
            if (F::LAZY) x[j] = fe_cond_sub_kp<F, 0>(fe_mul_lazy<F>(pw, x[j]));
            else x[j] = fe_mul<F>(x[j], pw);
        }
    } else if (EXTRA && p.scale) {
        Fe<F> sc;
#pragma unroll
        for (int i = 0; i < 8; i++) sc.v[i] = p.sc[i];
#pragma unroll
        for (int j = 0; j < E; j++) {
            if (F::LAZY) x[j] = fe_cond_sub_kp<F, 0>(fe_mul_lazy<F>(sc, x[j]));   // N^-1 < p: product in [0,2p)
            else x[j] = fe_mul<F>(x[j], sc);
        }
    } else if (F::LAZY && LAST) {
#pragma unroll
        for (int j = 0; j < E; j++) x[j] = fe_reduce_full(x[j]);
    }
}

// Non-last passes store their result straight from registers: work-items walk columns fastest, so the 2^logC
// lanes of a row hold one contiguous run of the output (8 x 32 B = 256 B for an 8-stage tile) and no transpose
// through LDS is needed.  Same tile elements as the load of step 0, so an in-place pass stays safe: every load
// of the tile is behind the barriers between the steps.
template <class F, int K>
__device__ __forceinline__ void ntt_store_global(const NttItemGeo &g, uint4 *gout, uint32_t lgS, const Fe<F> *x) {
#pragma unroll
    for (int j = 0; j < (1 << K); j++) {
        const uint32_t m = g.mbase | ((uint32_t)j << g.sh);
        const uint64_t e = g.gbase + ((uint64_t)m << lgS) + g.c;
        uint4 q0, q1;
        pack_mem<F>(x[j], q0, q1);
        gout[2 * e] = q0;
        gout[2 * e + 1] = q1;
    }
}

// One work-item of a tile that keeps both 16-byte planes in LDS between the register steps (the last pass, and every
// tile whose shape is a run-time value): 2^K elements, K stages in registers.
template <class F, int K, bool LAST, bool EXTRA, bool WL, int FX = 0>
__device__ __forceinline__ void ntt_item(const NttPassParams &p, uint4 (*lds)[NTT_TILE], uint4 (*ltw)[NTT_LTW], const uint4 *gin,
                                         uint4 *gout, uint32_t w, uint32_t step, uint32_t t0, uint64_t base, uint32_t lgS,
                                         uint32_t hi_uniform, uint32_t hi_low, bool last_step, bool stage_tw) {
    constexpr int E = 1 << K;
    const uint32_t r = FX ? (uint32_t)FX : p.r, logC = FX ? (uint32_t)(NTT_TILE_LOG - FX) : p.logC;
    const NttItemGeo g = ntt_item_geo<K, LAST, WL, FX>(p, w, step, t0, base, hi_uniform, hi_low);
    uint4 tq0, tq1;
    if (!LAST && !WL && stage_tw) ntt_tw_stage_load(p, r, hi_uniform, tq0, tq1);
    Fe<F> x[E];
    if (step == 0) {   // branch hoisted out of the element loop: the 2E global loads are issued back to back
        ntt_load_global<F, K, LAST, EXTRA>(p, g, gin, lgS, x);
    } else {
#pragma unroll
        for (int j = 0; j < E; j++) {
            const uint32_t idx = lds_slot<WL>(g.mbase | ((uint32_t)j << g.sh), g.c, r, logC);
            x[j] = unpack_mem<F>(lds[0][idx], lds[1][idx ^ (WL ? 1u : 0u)]);
        }
    }
    if (!LAST && !WL && stage_tw) {   // uniform across the workgroup (see the kernel)
        ntt_tw_stage_store(ltw, r, tq0, tq1);
        __syncthreads();
    }
    ntt_butterflies<F, K, LAST, WL, true, false, FX>(p, g, ltw, t0, step == 0, x);
    if (last_step) ntt_finish<F, K, LAST, EXTRA, FX>(p, g, x);
    if (!LAST && last_step) {
        ntt_store_global<F, K>(g, gout, lgS, x);
        return;
    }
#pragma unroll
    for (int j = 0; j < E; j++) {
        const uint32_t idx = lds_slot<WL>(g.mbase | ((uint32_t)j << g.sh), g.c, r, logC);
        pack_mem<F>(x[j], lds[0][idx], lds[1][idx ^ (WL ? 1u : 0u)]);   // the planes are offset by one slot so that plane-interleaved reads spread too
    }
}

// The non-last passes over full-size tiles (FX) hand the tile from one register step to the next through ONE 16-byte
// plane of LDS (ntt_exchange): 32 KiB plus 8 KiB of staged twiddles per workgroup, so LDS allows four workgroups per CU
// and registers decide.  The lazy Stark252 butterflies fit 80 VGPRs without scratch once the twiddle prefetch is gone
// (78, 0 B; with it 80 and 28 to 32 B of scratch): six waves per SIMD = three workgroups of eight waves per CU, so that
// one workgroup's wait for its tile or at a barrier is covered by two others, not one.  The canonical butterflies of
// the other fields and the kernels with a coset product (EXTRA) do not fit and keep a bound of four with the prefetch.
// Every other kernel holds both planes (64 KiB + twiddles): two workgroups, four waves per SIMD, as the bound says.
// The last pass stays there on its measurement (profiles/ntt_three_wg_ab.txt): through one plane it lost 3.5 % at two
// workgroups per CU (three more synchronisations per hand-over and write-out) and still 2 % at three, where its
// twiddles, one per lane from the table, can no longer be prefetched.
template <bool LAST, int FX>
constexpr bool ntt_one_plane() { return FX && !LAST; }
template <class F, bool LAST, bool EXTRA, int FX>
constexpr int ntt_waves_per_simd() { return ntt_one_plane<LAST, FX>() && F::LAZY && !EXTRA ? 6 : 4; }

// Hand-over of a full-size tile between two register steps through one plane: the work-item writes plane 0 of its four
// results to their slots so[], reads plane 0 of its four next inputs from si[], then the same for plane 1, with a
// workgroup barrier after each but the last of the four phases.  At the worst point a work-item holds 16 dwords of old
// results and 16 of new inputs, the 32 a whole element set takes.  The si[] of one hand-over are the so[] of the next
// and no other work-item touches them in between, so consecutive hand-overs need no barrier between them.
template <class F>
__device__ __forceinline__ void ntt_exchange(uint4 *lds, const uint32_t (&so)[4], const uint32_t (&si)[4], Fe<F> *x) {
    uint4 o0[4], o1[4], n0[4];
#pragma unroll
    for (int j = 0; j < 4; j++) pack_mem<F>(x[j], o0[j], o1[j]);
#pragma unroll
    for (int j = 0; j < 4; j++) lds[so[j]] = o0[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) n0[j] = lds[si[j]];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) lds[so[j]] = o1[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) x[j] = unpack_mem<F>(n0[j], lds[si[j]]);
}

// LDS slots of a work-item's elements (K = 2: four of one item; K = 1: two, of one of the two items of a radix-2 step)
template <int K, int FX>
__device__ __forceinline__ void ntt_item_slots(const NttItemGeo &g, uint32_t *s) {
#pragma unroll
    for (int j = 0; j < (1 << K); j++) s[j] = lds_slot<false>(g.mbase | ((uint32_t)j << g.sh), g.c, FX, NTT_TILE_LOG - FX);
}

// A non-last pass over a full-size tile (FX = r stages, see ntt_item_geo): every register step has one radix-4 item per
// work-item (the odd stage of FX = 7: two radix-2 items), so the four elements stay in registers from the load to the
// store and only cross LDS in ntt_exchange.  Work-items walk columns fastest, which makes g.m_high 0 in register step 0
// and tid >> 7 in step 1 for every FX: the twiddles of those two steps are wave-uniform (ntt_butterflies, UNI) and the
// staged table is first read in step 2.
template <class F, bool EXTRA, int FX>
__device__ __forceinline__ void ntt_tile_fx(const NttPassParams &p, uint4 *lds, uint4 (*ltw)[NTT_LTW], const uint4 *gin, uint4 *gout,
                                            uint64_t base, uint32_t lgS, uint32_t hi_uniform) {
    constexpr bool PF = ntt_waves_per_simd<F, false, EXTRA, FX>() < 6;   // no room for the prefetched twiddle in 80 VGPRs
    // m_high = tid >> (9 - 2) in step 1 (log2 threads - the step's two stages): whole wavefronts of 64 share it
    static_assert(NTT_TILE_LOG - NTT_KMAX == 9 && NTT_THREADS == 512, "wave-uniform twiddles of steps 0 and 1 assume 512 radix-4 items");
    const uint32_t tid = threadIdx.x;
    Fe<F> x[4];
    uint32_t so[4], si[4];

    NttItemGeo g = ntt_item_geo<2, false, false, FX>(p, tid, 0u, 0u, base, hi_uniform, 0u);
    uint4 tq0, tq1;
    ntt_tw_stage_load(p, FX, hi_uniform, tq0, tq1);   // issued ahead of the data loads: one memory latency, not two
    ntt_load_global<F, 2, false, EXTRA>(p, g, gin, lgS, x);
    // no barrier of its own: the barriers of the first hand-over order these stores before step 2 reads the table
    ntt_tw_stage_store(ltw, FX, tq0, tq1);
    ntt_butterflies<F, 2, false, false, PF, true, FX>(p, g, ltw, 0u, true, x);
    ntt_item_slots<2, FX>(g, so);
#pragma unroll
    for (uint32_t s = 1; s < FX / 2; s++) {
        g = ntt_item_geo<2, false, false, FX>(p, tid, s, 2 * s, base, hi_uniform, 0u);
        ntt_item_slots<2, FX>(g, si);
        ntt_exchange<F>(lds, so, si, x);
        if (s == 1) ntt_butterflies<F, 2, false, false, PF, true, FX>(p, g, ltw, 2 * s, false, x);
        else ntt_butterflies<F, 2, false, false, PF, false, FX>(p, g, ltw, 2 * s, false, x);
#pragma unroll
        for (int j = 0; j < 4; j++) so[j] = si[j];
    }
    if constexpr (FX % 2) {   // the odd stage: a radix-2 step, two items per work-item
        const NttItemGeo ga = ntt_item_geo<1, false, false, FX>(p, tid, FX / 2, FX - 1, base, hi_uniform, 0u);
        const NttItemGeo gb = ntt_item_geo<1, false, false, FX>(p, tid + NTT_THREADS, FX / 2, FX - 1, base, hi_uniform, 0u);
        ntt_item_slots<1, FX>(ga, si);
        ntt_item_slots<1, FX>(gb, si + 2);
        ntt_exchange<F>(lds, so, si, x);
        ntt_butterflies<F, 1, false, false, PF, false, FX>(p, ga, ltw, FX - 1, false, x);
        ntt_butterflies<F, 1, false, false, PF, false, FX>(p, gb, ltw, FX - 1, false, x + 2);
        ntt_finish<F, 1, false, EXTRA, FX>(p, ga, x);
        ntt_finish<F, 1, false, EXTRA, FX>(p, gb, x + 2);
        ntt_store_global<F, 1>(ga, gout, lgS, x);
        ntt_store_global<F, 1>(gb, gout, lgS, x + 2);
    } else {
        ntt_finish<F, 2, false, EXTRA, FX>(p, g, x);
        ntt_store_global<F, 2>(g, gout, lgS, x);
    }
}

template <class F, bool LAST, bool EXTRA, bool WL, int FX = 0>
__global__ __launch_bounds__(NTT_THREADS, (ntt_waves_per_simd<F, LAST, EXTRA, FX>())) void ntt_pass_kernel(NttPassParams p) {
    __shared__ uint4 lds[ntt_one_plane<LAST, FX>() ? 1 : 2][NTT_TILE];
    __shared__ uint4 ltw[LAST ? 1 : 2][LAST ? 1 : NTT_LTW];   // non-last passes: the tile's twiddles (<= 255 x 32 B)
    const uint32_t tid = threadIdx.x;
    static_assert(!FX || (NTT_TILE == 2048 && NTT_THREADS == 512 && (FX == 8 || FX == 7 || FX == 6)), "FX: 2^8 x 8, 2^7 x 16 or 2^6 x 32 rows x columns");
    static_assert(!WL || LAST, "the column layout is the last pass's");
    const uint32_t r = FX ? (uint32_t)FX : p.r, logC = FX ? (uint32_t)(NTT_TILE_LOG - FX) : p.logC, L = p.L;
    const uint32_t tile_log = r + logC;
    const uint4 *gin = p.in + 2 * (uint64_t)blockIdx.y * p.in_batch_stride;
    uint4 *gout = p.out + 2 * (uint64_t)blockIdx.y * p.out_batch_stride;
    const uint32_t b = blockIdx.x;

    uint64_t base = 0;
    uint32_t lgS = 0, hi_uniform = 0, hi_low = 0;
    if (!LAST) {
        lgS = L - p.s0 - r;                       // log2 of the row stride
        const uint32_t lo_bits = lgS - logC;      // column blocks per `hi`
        const uint32_t lo_blk = b & ((1u << lo_bits) - 1);
        hi_uniform = b >> lo_bits;
        base = ((uint64_t)hi_uniform << (L - p.s0)) + ((uint64_t)lo_blk << logC);
    } else {
        hi_low = bitrev_bits(b, L - r - logC);
    }

    if constexpr (ntt_one_plane<LAST, FX>()) {
        ntt_tile_fx<F, EXTRA, FX>(p, lds[0], (uint4 (*)[NTT_LTW])ltw, gin, gout, base, lgS, hi_uniform);
    } else {
    if constexpr (FX) {
#define LW_FX_STEP(S)                                                                                                                  \
    do {                                                                                                                                \
        if (S) {                                                                                                                        \
            if (WL && ((p.wave_sync >> (S)) & 1u)) lds_wave_sync();                                                                     \
            else __syncthreads();                                                                                                       \
        }                                                                                                                               \
        ntt_item<F, 2, LAST, EXTRA, WL, FX>(p, lds, (uint4 (*)[NTT_LTW])ltw, gin, gout, tid, (S), 2u * (S), base, lgS, hi_uniform, hi_low,    \
                                            2 * ((S) + 1) == FX, false);                                                                \
    } while (0)
        LW_FX_STEP(0u);
        LW_FX_STEP(1u);
        LW_FX_STEP(2u);
        if constexpr (FX == 8) LW_FX_STEP(3u);
        if constexpr (FX == 7) {   // the odd stage: a radix-2 step, two items per work-item
            __syncthreads();
            ntt_item<F, 1, LAST, EXTRA, WL, FX>(p, lds, (uint4 (*)[NTT_LTW])ltw, gin, gout, tid, 3u, 6u, base, lgS, hi_uniform, hi_low, true, false);
            ntt_item<F, 1, LAST, EXTRA, WL, FX>(p, lds, (uint4 (*)[NTT_LTW])ltw, gin, gout, tid + NTT_THREADS, 3u, 6u, base, lgS, hi_uniform, hi_low, true, false);
        }
#undef LW_FX_STEP
    } else {
    // twiddle staging happens inside the first register step when every thread runs it (the usual case);
    // tiles with fewer items than threads (small transforms) stage up front
    const bool stage_inside = !LAST && !WL && (1u << (tile_log - p.k[0])) >= (uint32_t)NTT_THREADS && (1u << r) <= (uint32_t)NTT_THREADS;
    if (!LAST && !WL && !stage_inside) {
        // stage t of the pass uses T[(hi << t) | x], x < 2^t, shared by every column of the tile
        for (uint32_t i = tid; i + 1 < (1u << r); i += NTT_THREADS) {
            const uint32_t t = 31 - __clz(i + 1), x = i + 1 - (1u << t);
            const uint64_t g = ((uint64_t)hi_uniform << t) | x;
            ltw[0][i] = p.tw[2 * g];
            ltw[1][i] = p.tw[2 * g + 1];
        }
        __syncthreads();
    }
    uint32_t t0 = 0;
    for (uint32_t step = 0; step < p.nsteps; step++) {
        const uint32_t k = p.k[step];
        const uint32_t nitems = 1u << (tile_log - k);
        const bool last_step = (step + 1 == p.nsteps);
        if (step) {
            if (WL && ((p.wave_sync >> step) & 1u)) lds_wave_sync();
            else __syncthreads();
        }
        for (uint32_t w = tid; w < nitems; w += NTT_THREADS) {
            if (NTT_KMAX >= 3 && k == 3) ntt_item<F, (NTT_KMAX >= 3 ? 3 : 1), LAST, EXTRA, WL>(p, lds, (uint4 (*)[NTT_LTW])ltw, gin, gout, w, step, t0, base, lgS, hi_uniform, hi_low, last_step, stage_inside && step == 0 && w == tid);
            else if (k == 2) ntt_item<F, 2, LAST, EXTRA, WL>(p, lds, (uint4 (*)[NTT_LTW])ltw, gin, gout, w, step, t0, base, lgS, hi_uniform, hi_low, last_step, stage_inside && step == 0 && w == tid);
            else ntt_item<F, 1, LAST, EXTRA, WL>(p, lds, (uint4 (*)[NTT_LTW])ltw, gin, gout, w, step, t0, base, lgS, hi_uniform, hi_low, last_step, stage_inside && step == 0 && w == tid);
        }
        t0 += k;
    }
    }
    if constexpr (!LAST) return;   // stored from registers by the last register step (ntt_item)
    __syncthreads();

    // last pass: coalesced write-out of the bit-reversed tile, two lanes per element, 16 B each
    auto write_one = [&](uint32_t f) {
        const uint32_t e = f >> 1, plane = f & 1;
        const uint32_t c = e & ((1u << logC) - 1);
        const uint32_t m = e >> logC;
        const uint64_t g = ((uint64_t)bitrev_bits(m, r) << (L - r)) + ((uint64_t)b << logC) + c;
        gout[2 * g + plane] = lds[plane][lds_slot<WL>(m, c, r, logC) ^ (WL ? plane : 0u)];
    };
    if constexpr (FX) {
#pragma unroll
        for (int q = 0; q < 2 * NTT_TILE / NTT_THREADS; q++) write_one(tid + (uint32_t)q * NTT_THREADS);
    } else {
        const uint32_t total = 2u << tile_log;
        for (uint32_t f = tid; f < total; f += NTT_THREADS) write_one(f);
    }
    }
}

// T[g] = w^bitrev_{bits}(g), from two small power tables: w^e = lo[e & mask] * hi[e >> hbits]
template <class F>
__global__ void twiddle_fill_kernel(uint4 *tw, const uint4 *lo, const uint4 *hi, uint32_t bits, uint32_t hbits,
                                    uint64_t count) {
    uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    uint32_t e = bitrev_bits((uint32_t)g, bits);
    Fe<F> a = tw_load<F>(lo, e & ((1u << hbits) - 1));
    Fe<F> b = tw_load<F>(hi, e >> hbits);
    tw_store<F>(tw, g, fe_mul<F>(a, b));
}

// The two power tables of a coset offset on the device: lo[i] = base^i (i < 2^hbits), hi[j] = scale * base^(j * 2^hbits)
// (j < hi_count), one square-and-multiply per entry — a few thousand work-items, nothing uploaded, nothing to wait for.
// (Built on the host and uploaded, a new offset cost a stream synchronisation, ~3000 serial products and two copies:
// ~110 us per call, every layer of a FRI commit phase.)
struct FeWords8 {
    uint32_t w[8];
};
template <class F>
__global__ void power_tables_kernel(uint4 *lo, uint4 *hi, FeWords8 base, uint32_t hbits, uint64_t hi_count, FeWords8 scale, int has_scale) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t lo_count = 1ull << hbits;
    if (t >= lo_count + hi_count) return;
    const bool is_lo = t < lo_count;
    const uint64_t e = is_lo ? t : ((t - lo_count) << hbits);
    Fe<F> b, r = Fe<F>::one();
#pragma unroll
    for (int k = 0; k < 8; k++) b.v[k] = base.w[k];
    for (int bit = 63 - (e ? __clzll((long long)e) : 63); bit >= 0; bit--) {
        r = fe_sqr<F>(r);
        if ((e >> bit) & 1) r = fe_mul<F>(r, b);
    }
    if (!is_lo && has_scale) {
        Fe<F> sc;
#pragma unroll
        for (int k = 0; k < 8; k++) sc.v[k] = scale.w[k];
        r = fe_mul<F>(r, sc);
    }
    if (is_lo) tw_store<F>(lo, t, r);
    else tw_store<F>(hi, t - lo_count, r);
}

}  // namespace lw
