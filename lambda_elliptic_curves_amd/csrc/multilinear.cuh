// What multilinear.hip, sumcheck_terms.hip and r1cs.hip share.  Device side: the block reduction, and of a sumcheck round
// the pair loader (ml_load_pair), the epilogue (ml_store_partial) and the finish kernel.  Host side: the round driver
// (ml_round_plan, ml_round_finish), the tables of an entry point (MlTables), the field dispatch (ml_with_field), the
// argument predicates and the copies of the host-buffer forms (ml_upload, ml_download, ml_download_each, ml_result).
#pragma once
#include <string.h>
#include <vector>
#include "internal.h"
#include "field.cuh"

namespace lw {

constexpr int ML_THREADS = 256;
constexpr uint32_t ML_ROUND_BLOCKS = 1024;         // most blocks of a round: 4 per CU, each thread strides over its share
constexpr uint32_t ML_MAX_VARS = 30;

// sum of v over the block's 256 threads, valid in thread 0.  A step writes lds[d, 2d) and reads it back, the next one
// writes [d/2, d): one barrier per step; the leading barrier separates two calls.
template <class F>
__device__ __forceinline__ Fe<F> ml_block_sum(Fe<F> v, Fe<F> *lds) {
    const int r = threadIdx.x;
    __syncthreads();
#pragma unroll 1
    for (int d = ML_THREADS / 2; d >= 1; d >>= 1) {
        if (r >= d && r < 2 * d) lds[r] = v;
        __syncthreads();
        if (r < d) v = fe_add<F>(v, lds[r + d]);
    }
    return v;
}

// One table's pair of a round: v = T[j], d = T[j + q] - T[j], with p the address of T[j].  FUSED first binds the leading
// variable to r in place, x + r (y - x) with the halves h = 2 q apart: the thread owns T[j], T[j + q], T[j + h] and
// T[j + h + q], stores the bound values at j and j + q and returns the pair of those.  Only FUSED reads r; a plain round
// passes null, so that its kernel never takes the address of a part of its argument (that alone changes how the compiler
// lays out the argument loads and the scalar code of the j loop, profiles/sumcheck_shared_isa.txt).
template <class F, bool FUSED>
__device__ __forceinline__ void ml_load_pair(char *p, uint64_t q, const Fe<F> *r, Fe<F> &v, Fe<F> &d) {
    Fe<F> lo = fe_load<F>(p), hi = fe_load<F>(p + q * 32);
    if (FUSED) {
        const uint64_t h = 2 * q;
        const Fe<F> lo1 = fe_load<F>(p + h * 32), hi1 = fe_load<F>(p + (h + q) * 32);
        lo = fe_add<F>(lo, fe_mul<F>(*r, fe_sub<F>(lo1, lo)));
        hi = fe_add<F>(hi, fe_mul<F>(*r, fe_sub<F>(hi1, hi)));
        fe_store<F>(p, lo);
        fe_store<F>(p + q * 32, hi);
    }
    v = lo;
    d = fe_sub<F>(hi, lo);
}

// partials[row][blockIdx.x] = sum of acc over the block.  Every thread of the block calls it or none does (barriers).
template <class F>
__device__ __forceinline__ void ml_store_partial(const Fe<F> &acc, Fe<F> *lds, char *partials, uint32_t row) {
    const Fe<F> s = ml_block_sum<F>(acc, lds);
    if (threadIdx.x == 0) fe_store<F>(partials + ((uint64_t)row * gridDim.x + blockIdx.x) * 32, s);
}

// block t: out[t] = sum of partials[t][0 .. nblocks)
template <class F>
__global__ __launch_bounds__(ML_THREADS) void ml_sum_finish_kernel(const char *partials, uint32_t nblocks, char *out) {
    __shared__ Fe<F> lds[ML_THREADS];
    Fe<F> acc = Fe<F>::zero();
#pragma unroll 1
    for (uint32_t b = threadIdx.x; b < nblocks; b += ML_THREADS)
        acc = fe_add<F>(acc, fe_load<F>(partials + ((uint64_t)blockIdx.x * nblocks + b) * 32));
    acc = ml_block_sum<F>(acc, lds);
    if (threadIdx.x == 0) fe_store<F>(out + (uint64_t)blockIdx.x * 32, acc);
}

// ---- host side ----
template <class F>
static Fe<F> ml_load(const void *ref) {
    alignas(16) uint64_t w[4];
    memcpy(w, ref, 32);
    return fe_load<F>(w);
}
static size_t ml_round256(size_t b) { return (b + 255) & ~(size_t)255; }

static bool ml_field_ok(lw_field_t f) {
    if (f == LW_FIELD_STARK252 || f == LW_FIELD_BLS12_381_FR) return true;
    set_error("field %d: multilinear tables take STARK252 or BLS12_381_FR (4 x u64 limbs)", (int)f);
    return false;
}
// f(F{}) with F = Stark252 or Fr381, for a field that ml_field_ok admits
template <class Fn>
static auto ml_with_field(lw_field_t field, Fn f) {
    return field == LW_FIELD_STARK252 ? f(Stark252{}) : f(Fr381{});
}
static bool ml_vars_ok(uint32_t n) {
    if (n <= ML_MAX_VARS) return true;
    set_error("%u variables: at most %u", n, ML_MAX_VARS);
    return false;
}
static bool ml_round_vars_ok(uint32_t n, const void *r_prev) {
    if (n >= (r_prev ? 2u : 1u)) return true;
    set_error("%u variables: a round needs 1, a fused round 2", n);
    return false;
}
static bool ml_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
static bool ml_overlap(const void *x, size_t xb, const void *y, size_t yb) {
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
    return a < b + yb && b < a + xb;
}

// host -> the staging buffer `buf`, grown to hold it.  Enqueues only.
static int ml_upload(DeviceBuf &buf, const void *host, size_t bytes, hipStream_t s) {
    if (buf.ensure(bytes)) return LW_ERR_ALLOC;
    LW_HIP_CHECK(hipMemcpyAsync(buf.p, host, bytes, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    return LW_OK;
}
// staging -> host: `bytes` from d_src to host, then the call's one synchronise
static int ml_download(void *host, const void *d_src, size_t bytes, hipStream_t s) {
    LW_HIP_CHECK(hipMemcpyAsync(host, d_src, bytes, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    return LW_OK;
}
// the same for k buffers of `bytes` each, host[i] from d_src[i] where host[i] is not null: one synchronise behind them all
static int ml_download_each(void *const *host, const void *const *d_src, uint32_t k, size_t bytes, hipStream_t s) {
    for (uint32_t i = 0; i < k; i++)
        if (host[i]) LW_HIP_CHECK(hipMemcpyAsync(host[i], d_src[i], bytes, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    return LW_OK;
}

// The one small host result of a call: `bytes` from d_src to out_host, then the call's one synchronise.  Up to 256 bytes
// go through the lane's pinned words (a copy into pageable memory is staged and waited for inside the runtime).
static int ml_result(Context &c, const void *d_src, size_t bytes, void *out_host, hipStream_t s) {
    if (bytes > 256) return ml_download(out_host, d_src, bytes, s);
    if (!c.pinned_words) LW_HIP_CHECK(hipHostMalloc((void **)&c.pinned_words, 256, hipHostMallocDefault), LW_ERR_ALLOC);
    LW_HIP_CHECK(hipMemcpyAsync(c.pinned_words, d_src, bytes, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    memcpy(out_host, c.pinned_words, bytes);
    return LW_OK;
}

// The k tables of 2^n elements of a call, in the caller's order (a round: the tables, then the eq table).
struct MlTables {
    void *const *tabs;
    uint32_t k, n;
    bool device;
    std::vector<void *> staged;   // host form: the copies in the lane's staging block

    size_t bytes() const { return (size_t)32 << n; }
    // none null, device tables aligned and, with `disjoint` (tables that a fused round writes), no two overlapping
    bool ok(bool disjoint) const {
        for (uint32_t i = 0; i < k; i++) {
            if (!tabs[i] || (device && !ml_aligned16(tabs[i]))) { set_error("table %u: null or misaligned buffer", i); return false; }
            for (uint32_t j = 0; disjoint && j < i; j++)
                if (ml_overlap(tabs[i], bytes(), tabs[j], bytes())) { set_error("tables %u and %u overlap", j, i); return false; }
        }
        return true;
    }
    // host form: the call moves to the lane's stream (s) and the tables into one staging block
    int stage(Entry &en, hipStream_t &s) {
        if (device) return LW_OK;
        s = en.use_lane_stream();
        if (!s) return en.rc;
        if (en.c.host_io_a.ensure((size_t)k * bytes())) return LW_ERR_ALLOC;
        staged.resize(k);
        for (uint32_t i = 0; i < k; i++) {
            staged[i] = (char *)en.c.host_io_a.p + (size_t)i * bytes();
            LW_HIP_CHECK(hipMemcpyAsync(staged[i], tabs[i], bytes(), hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
        }
        return LW_OK;
    }
    void *const *on_device() const { return device ? tabs : staged.data(); }
    // after a fused round of the host form: the bound first halves go back to the caller; synchronises
    int return_bound(hipStream_t s) const { return ml_download_each(tabs, on_device(), k, bytes() / 2, s); }
};

// ---- the driver of a round: n_values sums over q pairs, block by block into the partials, then ml_sum_finish_kernel ----
struct MlRoundPlan {
    uint64_t q;                 // pairs (T[j], T[j + q]): 2^(n-1), after a fused bind 2^(n-2)
    uint32_t blocks;
    char *vals, *partials;      // poly_ws: [values | partials[n_values][blocks]]
};
static int ml_round_plan(Context &c, uint32_t n, const void *r_prev, uint32_t n_values, MlRoundPlan &p) {
    p.q = (uint64_t)1 << (n - (r_prev ? 2 : 1));
    const uint64_t want = (p.q + ML_THREADS - 1) / ML_THREADS;
    p.blocks = want < ML_ROUND_BLOCKS ? (uint32_t)want : ML_ROUND_BLOCKS;
    if (c.poly_ws.ensure(256 + (size_t)n_values * p.blocks * 32)) return LW_ERR_ALLOC;
    p.vals = (char *)c.poly_ws.p;
    p.partials = p.vals + 256;
    return LW_OK;
}
// after the round kernel's launch: the finish kernel, then the n_values values -> out_host.  Synchronises.
template <class F>
static int ml_round_finish(Context &c, const MlRoundPlan &p, uint32_t n_values, void *out_host, hipStream_t s) {
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL((ml_sum_finish_kernel<F>), dim3(n_values), dim3(ML_THREADS), 0, s, (const char *)p.partials, p.blocks, p.vals);
    c.prof_end("ml_sum_finish_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return ml_result(c, p.vals, (size_t)n_values * 32, out_host, s);
}

}  // namespace lw
