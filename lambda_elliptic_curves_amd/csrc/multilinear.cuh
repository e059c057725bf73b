// What multilinear.hip and sumcheck_terms.hip share: the block reduction and the finish kernel of a round, the round's
// block cap, and the host helpers of the entry points (argument predicates, staging of host tables, the one host result).
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

// The one host result of a call: `bytes` from d_src to out_host, then the call's one synchronise.  Up to 256 bytes go
// through the lane's pinned words (a copy into pageable memory is staged and waited for inside the runtime).
static int ml_result(Context &c, const void *d_src, size_t bytes, void *out_host, hipStream_t s) {
    if (bytes > 256) {
        LW_HIP_CHECK(hipMemcpyAsync(out_host, d_src, bytes, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
        LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
        return LW_OK;
    }
    if (!c.pinned_words) LW_HIP_CHECK(hipHostMalloc((void **)&c.pinned_words, 256, hipHostMallocDefault), LW_ERR_ALLOC);
    LW_HIP_CHECK(hipMemcpyAsync(c.pinned_words, d_src, bytes, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    memcpy(out_host, c.pinned_words, bytes);
    return LW_OK;
}

static bool ml_field_ok(lw_field_t f) {
    if (f == LW_FIELD_STARK252 || f == LW_FIELD_BLS12_381_FR) return true;
    set_error("field %d: multilinear tables take STARK252 or BLS12_381_FR (4 x u64 limbs)", (int)f);
    return false;
}
static bool ml_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
static bool ml_overlap(const void *x, size_t xb, const void *y, size_t yb) {
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
    return a < b + yb && b < a + xb;
}

// k host tables of 2^n elements -> one device staging block
static int ml_stage(Context &c, const void *const *tabs, uint32_t k, uint32_t n, std::vector<void *> &d_tabs, hipStream_t s) {
    const size_t bytes = (size_t)32 << n;
    if (c.host_io_a.ensure((size_t)k * bytes)) return LW_ERR_ALLOC;
    d_tabs.resize(k);
    for (uint32_t i = 0; i < k; i++) {
        d_tabs[i] = (char *)c.host_io_a.p + (size_t)i * bytes;
        LW_HIP_CHECK(hipMemcpyAsync(d_tabs[i], tabs[i], bytes, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    }
    return LW_OK;
}

}  // namespace lw
