// Rescue Prime Optimized over Goldilocks on the device: batched permutations and hashes, and the Merkle tree built from
// the reference's `hash` (crypto/src/hash/rescue_prime/rescue_prime_optimized.rs:192-230).  The permutation itself and
// its bounds are in rpo.cuh.
//
// Four kernels per level, one work-item per permutation chain, each with a single inlined copy of the permutation:
//   rpo_permute_kernel   n states of m words                                              permutation
//   rpo_sponge_kernel    one digest per row, words gathered by two strides                hash; the leaves of a tree
//   rpo_pair_kernel      out[i] = hash(children[2 i] || children[2 i + 1])                a wide tree level
//   rpo_top_kernel       the last <= 256 parents down to the root, one workgroup          the top of a tree
// A permutation is 6384 (8512) Goldilocks products against at most a few hundred bytes of traffic, so the accesses are
// left as they fall (rows of a row-major matrix, a bit-reversed gather of the columns): nothing is transposed or copied.
#include <string.h>
#include <initializer_list>
#include "internal.h"
#include "rpo.cuh"

namespace lw {

template <int LEVEL> __global__ __launch_bounds__(256) void rpo_permute_kernel(const uint64_t *in, uint64_t *out, uint64_t n) {
    constexpr int M = RpoParams<LEVEL>::M;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t s[M];
#pragma unroll
    for (int j = 0; j < M; j++) s[j] = gl_from_word(in[i * M + j]);
    rpo_permute<LEVEL>(s);
#pragma unroll
    for (int j = 0; j < M; j++) out[i * M + j] = s[j];
}

// Digest i of n: hash (rescue_prime_optimized.rs:205-230) of the `len` words base[src * row_stride + c * elem_stride],
// c = 0 .. len - 1, with src = i, or the bit reversal of i over `bitrev_bits` bits (bitrev_bits >= 0).  Word 0 of the
// state is 1 iff len is no multiple of the rate; every block OVERWRITES the rate part; a partial last block is the words,
// a 1, zeros; len = 0 runs no permutation and the digest is zeros.  len and the block count are wave-uniform.
template <int LEVEL>
__global__ __launch_bounds__(256) void rpo_sponge_kernel(const uint64_t *base, uint64_t n, uint32_t len, uint64_t row_stride,
                                                         uint64_t elem_stride, int bitrev_bits, uint64_t *out) {
    typedef RpoParams<LEVEL> R;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t src = bitrev_bits < 0 ? i : (bitrev_bits ? (uint64_t)(__brevll(i) >> (64 - bitrev_bits)) : 0);
    const uint64_t *row = base + src * row_stride;
    uint64_t s[R::M];
#pragma unroll
    for (int j = 0; j < R::M; j++) s[j] = 0;
    if (len % R::RATE) s[0] = 1;
    const uint32_t blocks = (len + R::RATE - 1) / R::RATE;
    for (uint32_t b = 0; b < blocks; b++) {
#pragma unroll
        for (int h = 0; h < R::RATE; h++) {
            const uint32_t c = b * R::RATE + h;   // wave-uniform
            s[R::CAP + h] = c < len ? gl_from_word(row[(uint64_t)c * elem_stride]) : (c == len ? 1 : 0);
        }
        rpo_permute<LEVEL>(s);
    }
#pragma unroll
    for (int j = 0; j < R::DIGEST; j++) out[i * R::DIGEST + j] = s[R::CAP + j];
}

// parent of two digests: hash(left || right), 2 * DIGEST = RATE words, so one full block, word 0 of the state 0, one
// permutation at both levels.  The digests are canonical (the kernels wrote them).
template <int LEVEL> __device__ __forceinline__ void rpo_parent(const uint64_t *children, uint64_t *parent) {
    typedef RpoParams<LEVEL> R;
    static_assert(2 * R::DIGEST == R::RATE, "a pair of digests is one block");
    uint64_t s[R::M];
#pragma unroll
    for (int j = 0; j < R::CAP; j++) s[j] = 0;
#pragma unroll
    for (int j = 0; j < R::RATE; j++) s[R::CAP + j] = gl_from_word(children[j]);
    rpo_permute<LEVEL>(s);
#pragma unroll
    for (int j = 0; j < R::DIGEST; j++) parent[j] = s[R::CAP + j];
}

// out[i] = parent of children[2 i], children[2 i + 1] (digests, adjacent)
template <int LEVEL> __global__ __launch_bounds__(256) void rpo_pair_kernel(const uint64_t *children, uint64_t n, uint64_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rpo_parent<LEVEL>(children + i * RpoParams<LEVEL>::RATE, out + i * RpoParams<LEVEL>::DIGEST);
}

// The top of a tree in one launch, as poseidon_top_kernel: every level from the one starting at node level_begin (at most
// 512 nodes, level_end its last) down to the root, one parent per work-item, a barrier between levels.
template <int LEVEL> __global__ __launch_bounds__(256) void rpo_top_kernel(uint64_t *nodes, uint64_t level_begin, uint64_t level_end) {
    constexpr int D = RpoParams<LEVEL>::DIGEST;
    while (level_begin != level_end) {
        const uint64_t new_begin = level_begin / 2, count = level_begin - new_begin;
        const uint64_t k = threadIdx.x;
        if (k < count) rpo_parent<LEVEL>(nodes + (level_begin + 2 * k) * D, nodes + (new_begin + k) * D);
        __threadfence_block();   // workgroup scope is enough: the children of the next level were written by this workgroup
        __syncthreads();
        level_end = level_begin - 1;
        level_begin = new_begin;
    }
}

static dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }
static uint32_t rpo_width(int level) { return level == LW_RPO_128 ? RpoParams<0>::M : RpoParams<1>::M; }
static uint32_t rpo_digest(int level) { return level == LW_RPO_128 ? RpoParams<0>::DIGEST : RpoParams<1>::DIGEST; }

static int rpo_permute_device(Context &c, int level, const void *d_in, void *d_out, uint64_t n, hipStream_t s) {
    hipEvent_t pe = c.prof_begin(s);
    if (level == LW_RPO_128) hipLaunchKernelGGL(rpo_permute_kernel<0>, grid_for(n), dim3(256), 0, s, (const uint64_t *)d_in, (uint64_t *)d_out, n);
    else hipLaunchKernelGGL(rpo_permute_kernel<1>, grid_for(n), dim3(256), 0, s, (const uint64_t *)d_in, (uint64_t *)d_out, n);
    c.prof_end("rpo_permute_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}
static int rpo_sponge_device(Context &c, int level, const void *d_base, uint64_t n, uint32_t len, uint64_t row_stride,
                             uint64_t elem_stride, int bitrev_bits, void *d_out, hipStream_t s) {
    hipEvent_t pe = c.prof_begin(s);
    if (level == LW_RPO_128)
        hipLaunchKernelGGL(rpo_sponge_kernel<0>, grid_for(n), dim3(256), 0, s, (const uint64_t *)d_base, n, len, row_stride, elem_stride,
                           bitrev_bits, (uint64_t *)d_out);
    else
        hipLaunchKernelGGL(rpo_sponge_kernel<1>, grid_for(n), dim3(256), 0, s, (const uint64_t *)d_base, n, len, row_stride, elem_stride,
                           bitrev_bits, (uint64_t *)d_out);
    c.prof_end("rpo_sponge_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}
static int rpo_pair_device(Context &c, int level, const uint64_t *d_children, uint64_t n, uint64_t *d_out, hipStream_t s) {
    hipEvent_t pe = c.prof_begin(s);
    if (level == LW_RPO_128) hipLaunchKernelGGL(rpo_pair_kernel<0>, grid_for(n), dim3(256), 0, s, d_children, n, d_out);
    else hipLaunchKernelGGL(rpo_pair_kernel<1>, grid_for(n), dim3(256), 0, s, d_children, n, d_out);
    c.prof_end("rpo_pair_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}

// d_nodes: (2 * 2^log2n - 1) digests, root first (crypto/src/merkle_tree/utils.rs:43-71: the level of 2^m nodes starts at
// node 2^m - 1).
// Schedule, from the arithmetic as for the Poseidon tree (thresholds NOT MEASURED against
// alternatives).  A work-item's permutation is 6384 (8512) gl_mul, and a wave issues them one after the other: with m
// chains side by side the wave is bound by issue, not by latency, so a lone wave takes
// 6384 x 64 lanes / (the per-SIMD product rate) whatever else runs — hundreds of microseconds (profiles/rpo.txt has the
// rate), against ~10 us for a dependent launch.  Hence:
//   * no levels fused into the leaf kernel or into one another: in a fused launch level k + 1 runs on half the work-items
//     of level k while the others hold their slots, a whole permutation time spent to save a launch that costs a few
//     hundredths of it; every wide level is one launch of the pair kernel;
//   * the top kernel takes over at 256 parents (TOP_LOG2 = 9: a level of 2^9 nodes), one parent per work-item of one
//     workgroup, its four waves on the four SIMDs of one CU: from there every level costs one wave's permutation time on
//     one CU or on many, and the barrier replaces 9 launches.  A larger top (1024 parents, 16 waves on one CU) would put
//     4 issue-bound waves on each SIMD: four permutation times for that level where a launch spreads them out.
static int rpo_commit_device(Context &c, int level, const void *d_cols, uint32_t n_cols, uint64_t col_stride, uint32_t log2n,
                             int bit_reverse, void *d_nodes, hipStream_t s) {
    constexpr uint32_t TOP_LOG2 = 9;
    const uint64_t n = 1ull << log2n, d = rpo_digest(level);
    uint64_t *nodes = (uint64_t *)d_nodes;
    int rc = rpo_sponge_device(c, level, d_cols, n, n_cols, 1, col_stride, bit_reverse ? (int)log2n : -1, nodes + (n - 1) * d, s);
    if (rc) return rc;
    uint32_t m = log2n;   // the level whose parents are built next holds 2^m nodes
    for (; m > TOP_LOG2; m--) {
        rc = rpo_pair_device(c, level, nodes + ((1ull << m) - 1) * d, 1ull << (m - 1), nodes + ((1ull << (m - 1)) - 1) * d, s);
        if (rc) return rc;
    }
    if (m > 0) {
        const uint64_t level_begin = (1ull << m) - 1;
        hipEvent_t pe = c.prof_begin(s);
        if (level == LW_RPO_128) hipLaunchKernelGGL(rpo_top_kernel<0>, dim3(1), dim3(256), 0, s, nodes, level_begin, 2 * level_begin);
        else hipLaunchKernelGGL(rpo_top_kernel<1>, dim3(1), dim3(256), 0, s, nodes, level_begin, 2 * level_begin);
        c.prof_end("rpo_top_kernel", pe, s);
        LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    }
    return LW_OK;
}

// ---- argument checks: one per entry-point family, run before any device work
static constexpr uint64_t RPO_MAX_N = (uint64_t)1 << 36;   // the grid's block index stays below 2^31
static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
static int upload(void *dst, const void *src, size_t bytes, hipStream_t s) {
    LW_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    return LW_OK;
}
static int download(void *dst, const void *src, size_t bytes, hipStream_t s) {   // complete on return
    LW_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    return LW_OK;
}
static int level_check(int level) {
    if (level != LW_RPO_128 && level != LW_RPO_160) { set_error("bad RPO level %d", level); return LW_ERR_BAD_ARG; }
    return LW_OK;
}
// `count` items; every pointer in bufs must be there (and 16-byte aligned for the _device forms) once there is work
static int flat_check(uint64_t count, std::initializer_list<const void *> bufs, bool device) {
    if (count > RPO_MAX_N) { set_error("%llu RPO inputs", (unsigned long long)count); return LW_ERR_ALLOC; }
    if (count == 0) return LW_OK;
    for (const void *p : bufs) {
        if (!p) { set_error("null buffer"); return LW_ERR_BAD_ARG; }
        if (device && !aligned16(p)) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    }
    return LW_OK;
}

}  // namespace lw

using namespace lw;

extern "C" {

static int permute_entry(int level, const void *states, size_t n, void *out, void *hip_stream, bool device) {
    int rc = level_check(level);
    if (!rc) rc = flat_check(n, {states, out}, device);
    if (rc || n == 0) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    if (device) return rpo_permute_device(en.c, level, states, out, n, en.stream);
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    Context &c = en.c;
    const size_t bytes = n * rpo_width(level) * 8;
    if (c.host_io_a.ensure(bytes)) return LW_ERR_ALLOC;
    int r = upload(c.host_io_a.p, states, bytes, s);
    if (!r) r = rpo_permute_device(c, level, c.host_io_a.p, c.host_io_a.p, n, s);
    return r ? r : download(out, c.host_io_a.p, bytes, s);
}
int lw_rpo_permute(lw_rpo_level_t level, const uint64_t *states, size_t n, uint64_t *out) { return permute_entry(level, states, n, out, nullptr, false); }
int lw_rpo_permute_device(lw_rpo_level_t level, const uint64_t *d_states, size_t n, uint64_t *d_out, void *hip_stream) {
    return permute_entry(level, d_states, n, d_out, hip_stream, true);
}

static int hash_entry(int level, const void *rows, size_t n_rows, size_t row_len, size_t row_stride, void *out, void *hip_stream,
                      bool device) {
    int rc = level_check(level);
    if (rc) return rc;
    if (row_stride == 0) row_stride = row_len;
    if (row_stride < row_len) { set_error("row stride %zu below the row length %zu", row_stride, row_len); return LW_ERR_BAD_ARG; }
    if (row_len > ((size_t)1 << 31) || (row_stride && n_rows > (RPO_MAX_N << 4) / row_stride)) {
        set_error("%zu rows of %zu words", n_rows, row_stride);
        return LW_ERR_ALLOC;
    }
    rc = row_len ? flat_check(n_rows, {rows, out}, device) : flat_check(n_rows, {out}, device);   // no row data: rows is not read
    if (rc || n_rows == 0) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    if (device) return rpo_sponge_device(en.c, level, rows, n_rows, (uint32_t)row_len, row_stride, 1, -1, out, en.stream);
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    Context &c = en.c;
    const size_t in_bytes = n_rows * row_len * 8, out_bytes = n_rows * rpo_digest(level) * 8;
    if (c.host_io_a.ensure(in_bytes ? in_bytes : 16) || c.host_io_b.ensure(out_bytes)) return LW_ERR_ALLOC;
    int r = in_bytes ? upload(c.host_io_a.p, rows, in_bytes, s) : LW_OK;
    if (!r) r = rpo_sponge_device(c, level, c.host_io_a.p, n_rows, (uint32_t)row_len, row_len, 1, -1, c.host_io_b.p, s);
    return r ? r : download(out, c.host_io_b.p, out_bytes, s);
}
int lw_rpo_hash(lw_rpo_level_t level, const uint64_t *rows, size_t n_rows, size_t row_len, uint64_t *out) {
    return hash_entry(level, rows, n_rows, row_len, 0, out, nullptr, false);
}
int lw_rpo_hash_device(lw_rpo_level_t level, const uint64_t *d_rows, size_t n_rows, size_t row_len, size_t row_stride, uint64_t *d_out,
                       void *hip_stream) {
    return hash_entry(level, d_rows, n_rows, row_len, row_stride, d_out, hip_stream, true);
}

// checks of both commitment forms; nodes_or_root: d_nodes (device form) or out_root (host form)
static int commit_check(int level, const void *columns, const void *nodes_or_root, uint32_t n_cols, uint64_t col_stride, uint32_t log2n,
                        bool device) {
    const int rc = level_check(level);
    if (rc) return rc;
    if (!columns || !nodes_or_root || n_cols == 0) { set_error("null buffer or no columns"); return LW_ERR_BAD_ARG; }
    if (device && (!aligned16(columns) || !aligned16(nodes_or_root))) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    if (log2n > 30) { set_error("2^%u leaves", log2n); return LW_ERR_ALLOC; }
    if (col_stride && col_stride < (1ull << log2n)) {
        set_error("column stride %llu below the column length", (unsigned long long)col_stride);
        return LW_ERR_BAD_ARG;
    }
    return LW_OK;
}
int lw_rpo_commit_columns_device(lw_rpo_level_t level, const uint64_t *d_columns, uint32_t n_cols, uint64_t col_stride, uint32_t log2n,
                                 int bit_reverse, uint64_t *d_nodes, uint64_t *out_root, void *hip_stream) {
    int rc = commit_check(level, d_columns, d_nodes, n_cols, col_stride, log2n, true);
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    if (col_stride == 0) col_stride = 1ull << log2n;
    rc = rpo_commit_device(en.c, level, d_columns, n_cols, col_stride, log2n, bit_reverse, d_nodes, en.stream);
    if (rc) return rc;
    return out_root ? download(out_root, d_nodes, rpo_digest(level) * 8, en.stream) : LW_OK;
}
int lw_rpo_commit_columns(lw_rpo_level_t level, const uint64_t *columns, uint32_t n_cols, uint32_t log2n, int bit_reverse, uint64_t *out_root,
                          uint64_t *out_nodes_or_null) {
    int rc = commit_check(level, columns, out_root, n_cols, 0, log2n, false);
    if (rc) return rc;
    const size_t n = (size_t)1 << log2n, db = rpo_digest(level) * 8;
    Entry en(nullptr);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    if (c.host_io_a.ensure((size_t)n_cols * n * 8) || c.host_io_b.ensure((2 * n - 1) * db)) return LW_ERR_ALLOC;
    rc = upload(c.host_io_a.p, columns, (size_t)n_cols * n * 8, s);
    if (!rc) rc = rpo_commit_device(c, level, c.host_io_a.p, n_cols, n, log2n, bit_reverse, c.host_io_b.p, s);
    if (rc) return rc;
    if (out_nodes_or_null) {
        rc = download(out_nodes_or_null, c.host_io_b.p, (2 * n - 1) * db, s);
        if (rc) return rc;
        memcpy(out_root, out_nodes_or_null, db);
        return LW_OK;
    }
    return download(out_root, c.host_io_b.p, db, s);
}

}  // extern "C"
